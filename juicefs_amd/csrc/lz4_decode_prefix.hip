// The prefix instantiation of the one-workgroup LZ4 decoder (lz4_decode.hip:
// lz4_decode_kernel<true>, jfs_launch_lz4_decode_prefix) in a translation unit
// of its own, so that the full decoder's module holds the one kernel it always
// held and compiles to the same code.
#define JFS_LZ4_DECODE_PREFIX_TU
#undef JFS_PROF  // the phase counters belong to the full decoder's unit
#include "lz4_decode.hip"
