// The MATS_NESTED kernels of libmiwave.so in a split build (device/nested_instances.h): the kernel headers of miwave.hip without
// its host side, and the explicit instantiations of part MIW_NESTED_PART. mitsuba2_amd/build.py compiles this file once per part,
// beside miwave.hip (-DMIW_SPLIT_NESTED=1), and links the objects into the one library.
#ifndef MIW_NESTED_PART
#error "compile with -DMIW_NESTED_PART=1 .. MIW_NESTED_PARTS (mitsuba2_amd/build.py)"
#endif
#include "miwave.hip"
