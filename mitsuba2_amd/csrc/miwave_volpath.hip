// The volpath integrator's kernels of libmiwave.so in a split build (device/volpath_kernel.h): the kernel headers of miwave.hip
// without its host side, then k_sample_volpath and its launch function (device/volpath_launch.h).
// mitsuba2_amd/build.py compiles this file beside miwave.hip (-DMIW_SPLIT_VOLPATH=1) and links the object into the one library.
#define MIW_VOLPATH_UNIT 1
#include "miwave.hip"
