// libjfsgpu.so host side: the device-resident entry points of the C ABI
// (include/jfs_gpucodec.h).  Buffers, descriptors and results live on the
// caller's current device and every launch goes to the caller's stream; no
// kernel lives here (the jfs_launch_* of jfs_internal.h have them).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "batch_plan.h"
#include "capi_host.h"
#include "jfs_internal.h"
#include "zstd_seek.h"

using namespace jfs_host;

namespace {

// the shared scratch blocks (SplitScratch), per device: the small-batch LZ4 decoders and the chase, the
// segment-parallel and the fast LZ4 encoder, the flat gather's tile prefix, the splice's frame places
SplitScratch g_split[64], g_eseg_scr[64], g_fast_scr[64], g_read_scr[64], g_splice_scr[64];
constexpr int64_t SCRATCH_FLOOR = 64ll << 20, SMALL_SCRATCH_FLOOR = 1ll << 20;

// the current device's block of `tab`, or null
SplitScratch *current_scratch(SplitScratch *tab) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    return &tab[dev];
}

// One LZ4 small-batch launch (nblk > 0) on the caller's stream with `need`
// bytes of the current device's scratch in `tab`: launch(scratch, cap, stream)
template <class Launch>
int64_t scratch_launch(SplitScratch *tab, int dir, int nblk, int64_t need, void *stream, Launch launch) {
    SplitScratch *z = current_scratch(tab);
    if (!z) return JFS_ERR_HIP;
    stat_launch(JFS_ALGO_LZ4, dir, nblk);
    std::lock_guard<std::mutex> lk(z->mu);
    hipStream_t st = (hipStream_t)stream;
    const int64_t rc = z->acquire(need, SCRATCH_FLOOR, st);
    if (rc != JFS_OK) return rc;
    if (launch(z->p, z->cap, st) != 0) return JFS_ERR_HIP;
    return z->release(st);
}

}  // namespace

extern "C" {

// The device-resident entry points launch on the caller's current device; it
// must be one the library selected (gfx950, in JFS_GPU_DEVICES).
static bool current_device_ok() {
    std::vector<DevCtx *> &ds = devices();
    int cur = -1;
    if (ds.empty() || hipGetDevice(&cur) != hipSuccess) return false;
    for (DevCtx *d : ds)
        if (d->id == cur) return true;
    return false;
}

int64_t jfs_lz4_decompress_device(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    stat_launch(JFS_ALGO_LZ4, DECOMPRESS, nblk);
    return launch_rc(jfs_launch_lz4_decode(d_blocks, nblk, d_ret, (hipStream_t)stream));
}

int64_t jfs_lz4_decompress_device_small(const jfs_dev_block *d_blocks, const int32_t *src_len, const int32_t *dst_cap,
                                        int nblk, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk < 0 || (nblk > 0 && (!src_len || !dst_cap))) return JFS_ERR_INVALID;
    if (nblk == 0) return JFS_OK;
    const jfs_plan::Lz4SplitGeom g = jfs_plan::lz4_split_geom(nblk, src_len, dst_cap);
    return scratch_launch(g_split, DECOMPRESS, nblk, jfs_lz4_split_scratch_bytes(nblk, src_len, dst_cap), stream,
                          [&](uint8_t *p, int64_t, hipStream_t st) {
                              return jfs_launch_lz4_split(d_blocks, nblk, d_ret, p, g.nseg, g.max_cap, g.norg, st);
                          });
}

int64_t jfs_lz4_decompress_prefix_device(const jfs_dev_block *d_blocks, const int32_t *d_want, int nblk,
                                         int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk > 0 && !d_want) return JFS_ERR_INVALID;
    stat_launch(JFS_ALGO_LZ4, DECOMPRESS, nblk);
    return launch_rc(jfs_launch_lz4_decode_prefix(d_blocks, nblk, d_ret, d_want, nullptr, (hipStream_t)stream));
}

int64_t jfs_lz4_decompress_prefix_device_small(const jfs_dev_block *d_blocks, const int32_t *src_len,
                                               const int32_t *dst_cap, const int32_t *d_want, int nblk,
                                               int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk < 0 || (nblk > 0 && (!src_len || !dst_cap || !d_want))) return JFS_ERR_INVALID;
    if (nblk == 0) return JFS_OK;
    const jfs_plan::Lz4SplitGeom g = jfs_plan::lz4_split_geom(nblk, src_len, dst_cap);
    // (want lives on the device only: the grids stay sized by the largest dst_cap)
    return scratch_launch(g_split, DECOMPRESS, nblk, jfs_lz4_split_scratch_bytes(nblk, src_len, dst_cap), stream,
                          [&](uint8_t *p, int64_t, hipStream_t st) {
                              return jfs_launch_lz4_split_prefix(d_blocks, nblk, d_ret, d_want, p, g.nseg, g.max_cap,
                                                                 g.norg, g.max_cap, st);
                          });
}

int64_t jfs_lz4_decompress_window_device_small(const jfs_dev_block *d_blocks, const int32_t *src_len,
                                               const int32_t *dst_cap, const int32_t *d_lo, const int32_t *d_hi, int nblk,
                                               int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk < 0 || (nblk > 0 && (!d_blocks || !src_len || !dst_cap || !d_lo || !d_hi || !d_ret))) return JFS_ERR_INVALID;
    if (nblk == 0) return JFS_OK;
    const jfs_plan::Lz4SplitGeom g = jfs_plan::lz4_split_geom(nblk, src_len, dst_cap);
    // (the windows live on the device only: the grids stay sized by the largest dst_cap)
    return scratch_launch(g_split, DECOMPRESS, nblk, jfs_lz4_split_scratch_bytes(nblk, src_len, dst_cap), stream,
                          [&](uint8_t *p, int64_t, hipStream_t st) {
                              return jfs_launch_lz4_split_window(d_blocks, nblk, d_ret, d_lo, d_hi, p, g.nseg, g.max_cap,
                                                                 g.norg, g.max_cap, st);
                          });
}

int64_t jfs_lz4_decompress_ranges_device(const jfs_dev_block *d_blocks, const int32_t *src_len, const int32_t *dst_cap,
                                         const int32_t *d_rng_first, const jfs_range *d_rng, int nblk, int32_t *d_ret,
                                         void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    // (d_rng: every list may be empty)
    if (nblk < 0 || (nblk > 0 && (!d_blocks || !src_len || !dst_cap || !d_rng_first || !d_ret))) return JFS_ERR_INVALID;
    if (nblk == 0) return JFS_OK;
    // (the lists live on the device only: the capacities bound the chase's grid)
    return scratch_launch(g_split, DECOMPRESS, nblk, jfs_lz4_chase_scratch_bytes(nblk, src_len), stream,
                          [&](uint8_t *p, int64_t, hipStream_t st) {
                              return jfs_launch_lz4_chase(d_blocks, src_len, dst_cap, d_rng_first, d_rng, nblk, d_ret, p,
                                                          -1, st);
                          });
}

int64_t jfs_lz4_compress_device_small(const jfs_dev_block *d_blocks, const int32_t *src_len, int nblk, int32_t *d_ret,
                                      void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk < 0 || (nblk > 0 && !src_len)) return JFS_ERR_INVALID;
    if (nblk == 0) return JFS_OK;
    return scratch_launch(g_eseg_scr, COMPRESS, nblk, jfs_lz4_eseg_scratch_bytes(nblk, src_len), stream,
                          [&](uint8_t *p, int64_t cap, hipStream_t st) {
                              return jfs_launch_lz4_encode_seg(d_blocks, nblk, src_len, d_ret, p, cap, st);
                          });
}

int64_t jfs_lz4_compress_fast_device(const jfs_dev_block *d_blocks, const int32_t *src_len, int nblk, int32_t *d_ret,
                                     void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk < 0 || (nblk > 0 && !src_len)) return JFS_ERR_INVALID;
    if (nblk == 0) return JFS_OK;
    return scratch_launch(g_fast_scr, COMPRESS, nblk, jfs_lz4_fast_scratch_bytes(nblk, src_len), stream,
                          [&](uint8_t *p, int64_t cap, hipStream_t st) {
                              return jfs_launch_lz4_fast(d_blocks, nblk, src_len, d_ret, p, cap, st);
                          });
}

int64_t jfs_lz4_compress_fast_lift_device(const jfs_dev_block *d_blocks, const int32_t *src_len, int nblk,
                                          const jfs_lz4_lift *d_lift, const jfs_dev_block *d_src,
                                          const int32_t *d_src_n, const int32_t *src_src_len, const int32_t *src_cap,
                                          int nsrc, int32_t *d_ret, int32_t *d_lifted, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk < 0 || nsrc < 0 || (nblk > 0 && (!d_blocks || !src_len || !d_lift || !d_ret)) ||
        (nsrc > 0 && (!d_src || !d_src_n || !src_src_len || !src_cap)))
        return JFS_ERR_INVALID;
    if (nblk == 0) return JFS_OK;
    // (no source: every chunk is a parse chunk, and there is nothing to index)
    if (nsrc == 0) {
        if (d_lifted && hipMemsetAsync(d_lifted, 0, (size_t)nblk * 4, (hipStream_t)stream) != hipSuccess) return JFS_ERR_HIP;
        return jfs_lz4_compress_fast_device(d_blocks, src_len, nblk, d_ret, stream);
    }
    // (the candidates live on the device only: every source is indexed)
    const jfs_lz4_lift_srcs S{d_src, d_src_n, nsrc, nullptr, nsrc, src_src_len, src_cap};
    return scratch_launch(g_fast_scr, COMPRESS, nblk, jfs_lz4_fast_lift_scratch_bytes(nblk, src_len, nsrc, nsrc, src_src_len),
                          stream, [&](uint8_t *p, int64_t cap, hipStream_t st) {
                              return jfs_launch_lz4_fast_lift(d_blocks, nblk, src_len, d_lift, &S, d_ret, d_lifted, p, cap, st);
                          });
}

int64_t jfs_lz4_compress_device(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    stat_launch(JFS_ALGO_LZ4, COMPRESS, nblk);
    return launch_rc(jfs_launch_lz4_encode(d_blocks, nblk, d_ret, (hipStream_t)stream));
}

int64_t jfs_zstd_compress_device(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    stat_launch(JFS_ALGO_ZSTD, COMPRESS, nblk);
    return launch_rc(jfs_launch_zstd_encode(d_blocks, nblk, d_ret, (hipStream_t)stream, JFS_ZSTD_PARSE_EXACT));
}

int64_t jfs_zstd_compress_fast_device(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    stat_launch(JFS_ALGO_ZSTD, COMPRESS, nblk);
    return launch_rc(jfs_launch_zstd_encode(d_blocks, nblk, d_ret, (hipStream_t)stream, JFS_ZSTD_PARSE_FAST));
}

int64_t jfs_zstd_splice_device(const jfs_splice_out *d_out, int nout, const jfs_splice_frame *d_frames, int nframes,
                               const int32_t *d_unit_len, const uint64_t *d_unit_hash, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nout < 0 || nframes < 0 || (nout > 0 && (!d_out || !d_ret)) || (nframes > 0 && !d_frames)) return JFS_ERR_INVALID;
    if (nout == 0) return JFS_OK;
    // the frames' places: the current device's shared scratch, ordered across streams by its event
    SplitScratch *z = current_scratch(g_splice_scr);
    if (!z) return JFS_ERR_HIP;
    std::lock_guard<std::mutex> lk(z->mu);
    hipStream_t st = (hipStream_t)stream;
    const int64_t rc = z->acquire(((int64_t)nframes + 1) * 4, SMALL_SCRATCH_FLOOR, st);
    if (rc != JFS_OK) return rc;
    if (jfs_launch_zstd_splice(d_out, nout, d_frames, nframes, d_unit_len, d_unit_hash, (uint32_t *)z->p, d_ret, st) != 0)
        return JFS_ERR_HIP;
    return z->release(st);
}

int64_t jfs_zstd_seek_tables_device(const jfs_dev_block *d_blocks, const int32_t *d_len, int nblk,
                                    const int32_t *d_slot_first, uint8_t *d_tables, int32_t *d_table_len, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk < 0 || (nblk > 0 && (!d_blocks || !d_len || !d_slot_first || !d_tables || !d_table_len))) return JFS_ERR_INVALID;
    return launch_rc(
        jfs_launch_zstd_seek_tables(d_blocks, d_len, nblk, d_slot_first, d_tables, d_table_len, (hipStream_t)stream));
}

int64_t jfs_zstd_compress_seekable_device(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    stat_launch(JFS_ALGO_ZSTD, COMPRESS, nblk);
    return launch_rc(jfs_launch_zstd_encode(d_blocks, nblk, d_ret, (hipStream_t)stream, JFS_ZSTD_PARSE_SEEKABLE));
}

int64_t jfs_zstd_decompress_range_device(const jfs_dev_block *d_blocks, const int32_t *d_lo, const int32_t *d_hi,
                                         int nblk, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk > 0 && (!d_lo || !d_hi)) return JFS_ERR_INVALID;
    stat_launch(JFS_ALGO_ZSTD, DECOMPRESS, nblk);
    return launch_rc(jfs_launch_zstd_decode_range(d_blocks, d_lo, d_hi, nblk, d_ret, (hipStream_t)stream));
}

int64_t jfs_zstd_decompress_ranges_device(const jfs_dev_block *d_blocks, const int32_t *d_rng_first,
                                          const jfs_range *d_rng, int nblk, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk > 0 && (!d_blocks || !d_rng_first || !d_ret)) return JFS_ERR_INVALID;  // (d_rng: every list may be empty)
    stat_launch(JFS_ALGO_ZSTD, DECOMPRESS, nblk);
    return launch_rc(jfs_launch_zstd_decode_ranges(d_blocks, d_rng_first, d_rng, nblk, d_ret, (hipStream_t)stream));
}

int64_t jfs_xxh64_device(const jfs_dev_block *d_blocks, int nblk, uint64_t *d_hash, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk < 0 || (nblk > 0 && (!d_blocks || !d_hash))) return JFS_ERR_INVALID;
    return launch_rc(jfs_launch_xxh64(d_blocks, nblk, d_hash, d_ret, (hipStream_t)stream));
}

int64_t jfs_zstd_compress_seekable_csum_device(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    // (the descriptors are copied back to the host from the pointer given)
    if (nblk < 0 || (nblk > 0 && (!d_blocks || !d_ret))) return JFS_ERR_INVALID;
    stat_launch(JFS_ALGO_ZSTD, COMPRESS, nblk);
    return launch_rc(jfs_launch_zstd_encode_seek_csum(d_blocks, nblk, d_ret, (hipStream_t)stream));
}

int64_t jfs_zstd_decompress_frames_device(const jfs_seek_frag *d_frags, const int32_t *d_lo, const int32_t *d_hi,
                                          int nblk, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk > 0 && (!d_frags || !d_lo || !d_hi || !d_ret)) return JFS_ERR_INVALID;
    stat_launch(JFS_ALGO_ZSTD, DECOMPRESS, nblk);
    return launch_rc(jfs_launch_zstd_decode_frames(d_frags, d_lo, d_hi, nblk, d_ret, (hipStream_t)stream));
}

int64_t jfs_zstd_seek_plan(const uint8_t *tail, int64_t tail_len, int64_t object_len, int64_t lo, int64_t hi,
                           jfs_seek_plan *out) {
    namespace zs = jfs::zseek;
    if (!out || tail_len < 0 || object_len < 0 || tail_len > object_len || object_len > 0x7FFFFFFFll ||
        (!tail && tail_len > 0))
        return JFS_ERR_INVALID;
    memset(out, 0, sizeof(*out));
    out->status = JFS_SEEK_PLAN_NONE;
    if (tail_len < zs::FOOTER) return JFS_OK;
    // the footer: the frame count and the entry size place the table
    const uint8_t *f = tail + tail_len - zs::FOOTER;
    int32_t n = 0, entry = 0;
    if (!zs::footer_peek([f](int32_t p) { return (uint32_t)f[p]; }, zs::FOOTER, true, &n, &entry)) return JFS_OK;
    const int64_t table_len = (int64_t)entry * n + zs::TABLE_FIXED;
    if (table_len > object_len) return JFS_OK;
    if (tail_len < table_len) {
        out->status = JFS_SEEK_PLAN_MORE;
        out->checksums = entry == zs::ENTRY_CSUM;
        out->nf = n;
        out->table_off = object_len - table_len;
        out->table_len = table_len;
        return JFS_OK;
    }
    const uint8_t *t = tail + tail_len - table_len;
    const zs::TableSel s = zs::table_select([t](int32_t p) { return (uint32_t)t[p]; }, table_len, object_len, -1, lo, hi);
    if (!s.table) return JFS_OK;
    out->status = JFS_SEEK_PLAN_OK;
    out->checksums = s.checksums;
    out->nf = s.nf;
    out->first = s.first;
    out->count = s.count;
    out->table_off = object_len - table_len;
    out->table_len = table_len;
    out->get_off = (int64_t)s.coff;
    out->get_len = (int64_t)(s.cend - s.coff);
    out->content = (int64_t)s.total;
    out->first_off = (int64_t)s.doff;
    return JFS_OK;
}

int64_t jfs_zstd_decompress_prefix_device(const jfs_dev_block *d_blocks, const int32_t *d_want, int nblk,
                                          int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk > 0 && !d_want) return JFS_ERR_INVALID;
    stat_launch(JFS_ALGO_ZSTD, DECOMPRESS, nblk);
    return launch_rc(jfs_launch_zstd_decode_prefix(d_blocks, nblk, d_ret, d_want, (hipStream_t)stream));
}

int64_t jfs_zstd_decompress_device(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    stat_launch(JFS_ALGO_ZSTD, DECOMPRESS, nblk);
    return launch_rc(jfs_launch_zstd_decode(d_blocks, nblk, d_ret, nullptr, (hipStream_t)stream));
}

int64_t jfs_crc32c_device(const jfs_dev_block *d_blocks, int nblk, int32_t seg_bytes, uint32_t *d_crc,
                          int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk < 0 || seg_bytes < 0 || (seg_bytes > 0 && seg_bytes % 4096 != 0)) return JFS_ERR_INVALID;
    return launch_rc(jfs_launch_crc32c(d_blocks, nblk, seg_bytes, d_crc, d_ret, (hipStream_t)stream));
}

int64_t jfs_aes256gcm_seal_device(const jfs_aead_block *d_blocks, int nblk, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk < 0) return JFS_ERR_INVALID;
    return launch_rc(jfs_launch_aes256gcm(d_blocks, nblk, 0, d_ret, nullptr, (hipStream_t)stream));
}

int64_t jfs_aes256gcm_open_device(const jfs_aead_block *d_blocks, int nblk, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk < 0) return JFS_ERR_INVALID;
    return launch_rc(jfs_launch_aes256gcm(d_blocks, nblk, 1, d_ret, nullptr, (hipStream_t)stream));
}

int64_t jfs_aead_seal_device(int cipher, const jfs_aead_block *d_blocks, int nblk, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk < 0 || jfs_cipher_key_size(cipher) < 0) return JFS_ERR_INVALID;
    return launch_rc(jfs_launch_aead(cipher, d_blocks, nblk, 0, d_ret, nullptr, (hipStream_t)stream));
}

int64_t jfs_aead_open_device(int cipher, const jfs_aead_block *d_blocks, int nblk, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk < 0 || jfs_cipher_key_size(cipher) < 0) return JFS_ERR_INVALID;
    return launch_rc(jfs_launch_aead(cipher, d_blocks, nblk, 1, d_ret, nullptr, (hipStream_t)stream));
}

int64_t jfs_lz4_compress_seal_device(const jfs_dev_block *d_comp, const jfs_aead_block *d_aead, int nblk,
                                     int32_t *d_ret_comp, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk < 0) return JFS_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (jfs_launch_lz4_encode(d_comp, nblk, d_ret_comp, st) != 0) return JFS_ERR_HIP;
    return launch_rc(jfs_launch_aes256gcm(d_aead, nblk, 0, d_ret, d_ret_comp, st));
}

int64_t jfs_open_lz4_decompress_device(const jfs_aead_block *d_aead, const jfs_dev_block *d_dec, int nblk,
                                       int32_t *d_ret_open, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk < 0) return JFS_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (jfs_launch_aes256gcm(d_aead, nblk, 1, d_ret_open, nullptr, st) != 0) return JFS_ERR_HIP;
    return launch_rc(jfs_launch_lz4_decode_lens(d_dec, nblk, d_ret, d_ret_open, st));
}

int64_t jfs_gather_device(const jfs_dev_block *d_src, const int32_t *d_src_n, int nsrc, const jfs_compact_out *d_out,
                          int nout, const jfs_compact_seg *d_seg, int32_t max_dst_cap, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nsrc < 0 || nout < 0 || (nout > 0 && (!d_out || !d_ret))) return JFS_ERR_INVALID;
    return launch_rc(
        jfs_launch_gather(d_src, d_src_n, nsrc, d_out, nout, d_seg, max_dst_cap, d_ret, 0, (hipStream_t)stream));
}

int64_t jfs_lz4_compact_device(const jfs_dev_block *d_src, int nsrc, int32_t *d_src_ret,
                               const jfs_compact_out *d_gather, const jfs_compact_seg *d_seg,
                               const jfs_dev_block *d_enc, int nout, int32_t max_dst_cap, int32_t *d_ret,
                               void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nsrc < 0 || nout < 0 || (nsrc > 0 && (!d_src || !d_src_ret)) || (nout > 0 && (!d_gather || !d_enc || !d_ret)))
        return JFS_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    stat_launch(JFS_ALGO_LZ4, DECOMPRESS, nsrc);
    stat_launch(JFS_ALGO_LZ4, COMPRESS, nout);
    if (nsrc > 0 && jfs_launch_lz4_decode(d_src, nsrc, d_src_ret, st) != 0) return JFS_ERR_HIP;
    if (jfs_launch_gather(d_src, d_src_ret, nsrc, d_gather, nout, d_seg, max_dst_cap, d_ret, 0, st) != 0)
        return JFS_ERR_HIP;
    if (nout > 0 && jfs_launch_lz4_encode(d_enc, nout, d_ret, st) != 0) return JFS_ERR_HIP;
    // the encoder ran on every block: a failed gather's verdict replaces its result
    return launch_rc(jfs_launch_gather(d_src, d_src_ret, nsrc, d_gather, nout, d_seg, max_dst_cap, d_ret, 1, st));
}

int64_t jfs_read_gather_device(const jfs_dev_block *d_src, const int32_t *d_src_n, int nsrc, const jfs_compact_out *d_out,
                               const int32_t *dst_cap, int nout, const jfs_compact_seg *d_seg, int32_t *d_ret,
                               void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nsrc < 0 || nout < 0 || (nout > 0 && (!d_out || !d_ret || !dst_cap))) return JFS_ERR_INVALID;
    if (nout == 0) return JFS_OK;
    int64_t ntiles = 0;
    for (int j = 0; j < nout; j++) ntiles += jfs_gather_tiles(dst_cap[j]);
    if (ntiles > INT32_MAX) return JFS_ERR_INVALID;
    // the tile prefix is built on the device from d_out, in the current device's shared scratch
    SplitScratch *z = current_scratch(g_read_scr);
    if (!z) return JFS_ERR_HIP;
    std::lock_guard<std::mutex> lk(z->mu);
    hipStream_t st = (hipStream_t)stream;
    const int64_t rc = z->acquire(((int64_t)nout + 1) * 4, SMALL_SCRATCH_FLOOR, st);
    if (rc != JFS_OK) return rc;
    int32_t *d_tf = (int32_t *)z->p;
    if (jfs_launch_gather_prefix(d_out, nout, d_tf, st) != 0 ||
        jfs_launch_gather_flat(d_src, d_src_n, nsrc, d_out, nout, d_seg, d_ret, d_tf, ntiles, st) != 0)
        return JFS_ERR_HIP;
    return z->release(st);
}

int64_t jfs_read_csum_device(const jfs_compact_out *d_out, const int32_t *d_ret, int nout, const int32_t *d_piece_first,
                             int64_t npiece, uint8_t *d_csum, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nout < 0 || npiece < 0 || npiece > INT32_MAX || (nout > 0 && (!d_out || !d_ret || !d_piece_first)) ||
        (npiece > 0 && (!d_csum || ((uintptr_t)d_csum & 3u) != 0)))
        return JFS_ERR_INVALID;
    if (nout == 0 || npiece == 0) return JFS_OK;
    return launch_rc(
        jfs_launch_read_csum_flat(d_out, nout, d_ret, d_piece_first, npiece, (uint32_t *)d_csum, (hipStream_t)stream));
}

}  // extern "C"
