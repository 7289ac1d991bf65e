// The MATS_LIGHTS kernels of libmiwave.so in a split build (device/lights_instances.h): the kernel headers of miwave.hip without
// its host side, and the explicit instantiations of part MIW_LIGHTS_PART. mitsuba2_amd/build.py compiles this file once per part,
// beside miwave.hip (-DMIW_SPLIT_LIGHTS=1), and links the objects into the one library.
#ifndef MIW_LIGHTS_PART
#error "compile with -DMIW_LIGHTS_PART=1 .. MIW_LIGHTS_PARTS (mitsuba2_amd/build.py)"
#endif
#include "miwave.hip"
