// The general sensor route's kernels of libmiwave.so in a split build (device/sensor_kernel.h): the kernel headers of miwave.hip
// without its host side, then k_sensor_step, k_sensor_rays and their launch functions (device/sensor_launch.h).
// mitsuba2_amd/build.py compiles this file beside miwave.hip (-DMIW_SPLIT_SENSOR=1) and links the object into the one library.
#define MIW_SENSOR_UNIT 1
#include "miwave.hip"
