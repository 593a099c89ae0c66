// The prefix instantiation of the Zstd decoder (zstd_decode.hip with ZPFX =
// true: jfs_launch_zstd_decode_prefix, jfs_zstd_plan_host_prefix) in a
// translation unit of its own, so that the full decoder's module holds the
// kernels it always held and compiles to the same code.
#define JFS_ZSTD_DECODE_PREFIX_TU
#undef JFS_PROF  // the phase counters belong to the full decoder's unit
#include "zstd_decode.hip"
