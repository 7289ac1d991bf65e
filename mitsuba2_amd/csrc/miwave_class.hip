// The MATS_NESTED and MATS_LIGHTS kernels of libmiwave.so in a split build (device/class_instances.h): the kernel headers of miwave.hip
// without its host side, and the explicit instantiations of part MIW_CLASS_PART of class MIW_CLASS. mitsuba2_amd/build.py compiles this
// file once per class and part, beside miwave.hip (-DMIW_SPLIT_CLASSES=1), and links the objects into the one library.
#if !defined(MIW_CLASS) || !defined(MIW_CLASS_PART)
#error "compile with -DMIW_CLASS=MATS_NESTED | MATS_LIGHTS -DMIW_CLASS_PART=1 .. MIW_CLASS_PARTS (mitsuba2_amd/build.py)"
#endif
#include "miwave.hip"
