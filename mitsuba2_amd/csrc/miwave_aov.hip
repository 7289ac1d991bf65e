// The aov integrator's kernels of libmiwave.so in a split build (device/aov_kernel.h): the kernel headers of miwave.hip without its
// host side, then k_aov_samples, k_aov_finish, k_aov_film, k_aov_film_merge and their launch functions (device/aov_launch.h).
// mitsuba2_amd/build.py compiles this file beside miwave.hip (-DMIW_SPLIT_AOV=1) and links the object into the one library.
#define MIW_AOV_UNIT 1
#include "miwave.hip"
