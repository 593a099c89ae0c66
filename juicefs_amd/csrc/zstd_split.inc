// ===========================================================================
// Small batches: one workgroup per BLOCK.  The kernels above run one wave per
// INPUT, so a lone 4 MiB frame -- pkg/chunk decodes exactly one per cache
// miss (cached_store.go:755-823 -> compress.go:94-103) -- walks its 32 blocks
// through one wave (~45 ms).  Here the same items, literal buffer and error
// order are produced block-parallel, and the replay is an origin map with
// pointer jumping over all output bytes at once:
//   zsplan    per-input scratch offsets;
//   zswalk    one wave per input walks the headers (zseqa's walk without the
//             table builds): FSTART / FEND / BSTART / ERR items, the items of
//             raw and RLE blocks, and one SBlk per block (where it is, its
//             literal offset, the blocks whose Huffman table and FSE tables
//             its repeat modes use -- never a block of an earlier frame --
//             and SB_FEND on the last block of a frame, whose IT_FEND item
//             follows the block's items);
//   zsblk     one workgroup per block: wave 0 decodes the literals (zlit's
//             lit_block; a treeless block rebuilds the table of its source
//             block), wave 1 builds the FSE tables in LDS and decodes the
//             sequences wave-uniformly (zseqb's items, symbolic repeat
//             offsets);
//   zsfix     one wave per input resolves the blocks' repeat-offset entry
//             states in order (IT_BREP items), the first literal error, and
//             the blocks' output offsets and the output offset their frame
//             starts at (fbase; libzstd's prefix restarts at every frame); an
//             input outside the proven cases (no frame or more than the
//             jfs_set_zstd_split_frames limit, a checksum, any error item, a
//             frame's content size or a literal-count check) is marked for the
//             exact replay;
//   zsemit    one workgroup per block writes the ORIGIN of each output byte
//             (origin_map.h: the entries, the jump and gather rules and the
//             round count); a literal's index is its place in the input's
//             literal area;
//   zsjump    pointer jumping over the map;
//   zsgather  the output bytes; an entry that is not a literal marks its
//             input;
//   zsverd    the marked inputs go to the exact replay;
//   zexec     the exact replay, for the marked inputs only: it reads the same
//             items and literals, so results and error codes are the exact
//             path's on every input.
// ===========================================================================
constexpr int ST = om::THREADS;  // threads per workgroup (emit / jump / gather)
constexpr int SCHUNK = 2048;     // sequence bitstream chunk staged per refill
constexpr int SRING = 4 * SCHUNK;
enum { SB_STORE = 1, SB_FIRST = 2, SB_SEQ = 4, SB_LIT = 8, SB_FEND = 16 };

struct SBlk {              // one block of an input, in stream order
    int32_t bpos, bsize;   // block content within the input
    uint32_t slot;         // its BSTART item (relative to the input)
    uint32_t lpos;         // first literal byte (relative to the input's literal area)
    int32_t regen, nseq;   // literal count (raw / RLE: the block size), sequences
    int32_t sip;           // the Symbol_Compression_Modes byte (nseq > 0)
    int32_t hsrc;          // block whose Huffman table a treeless literal section uses (-1 none)
    int32_t tsrc[3];       // block whose LL / OF / ML description a repeat mode uses (-1 none)
    uint8_t btype, flags;  // SB_*
    // zsblk
    int32_t lerr, serr;    // literal error code; the block's items hold an ERR
    uint32_t r0, r1, r2;   // repeat offsets at the block end (symbolic in the entry state)
    uint32_t brep;         // an IT_BREP item belongs at slot + 1
    uint64_t sll, sml;     // sums of literal and match lengths
    // zsfix
    uint32_t e0, e1, e2;  // repeat offsets at the block start
    uint32_t fbase;       // output offset at which the block's frame starts (<= out)
    int64_t out;          // output offset of the block
};

struct SIn {                 // one input
    int64_t blk_off, org_off;
    int32_t nb, ok, frames, todo;  // frames: the frames the walk entered
    int32_t unsettled, pad;        // the gather met an entry that is not a literal yet
    int64_t total;
    int32_t jmp[om::MAX_ROUNDS];
};

struct SScr {
    SIn *in;
    SBlk *blk;
    int32_t *todo;
    int32_t *org;
};

__global__ void zsplan_kernel(const ZInfo *__restrict__ info, int nblk, SScr sc) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;  // a few inputs
    int64_t bo = 0, oo = 0;
    for (int i = 0; i < nblk; i++) {
        SIn &x = sc.in[i];
        x.blk_off = bo;
        x.org_off = oo;
        x.nb = 0; x.ok = 0; x.frames = 0; x.todo = 1; x.unsettled = 0;
        x.total = 0;
        for (int r = 0; r < om::MAX_ROUNDS; r++) x.jmp[r] = 0;
        sc.todo[i] = 1;
        bo += info[i].n_blk;
        oo += ((int64_t)(info[i].cap > 0 ? info[i].cap : 0) + 3) & ~3ll;
    }
}

// the input owning global block record g: the last i with blk_off <= g
__device__ __forceinline__ int input_of(const SIn *in, int n, int64_t g) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (in[mid].blk_off <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(64) void zswalk_kernel(const jfs_dev_block *__restrict__ blocks, int nblk,
                                                    ZInfo *__restrict__ info, uint4 *__restrict__ items_all, SScr sc,
                                                    int strict_reserved, int max_frames) {
    const int bi = blockIdx.x;
    if (bi >= nblk) return;
    const int l = lane_id();
    const jfs_dev_block b = blocks[bi];
    ZInfo &zi = info[bi];
    SIn &si = sc.in[bi];
    if (zi.ovf) return;  // stays marked: zexec reports E_SCRATCH
    const gc_u8 *s = (const gc_u8 *)b.src;
    g_u4 *items = (g_u4 *)items_all + zi.item_off;
    SBlk *bk = sc.blk + si.blk_off;
    const uint32_t cap_items = zi.n_items, cap_blk = zi.n_blk;
    const int64_t lend = zi.lit_bytes;
    Walk w;
    walk_init(w, s, b.src_len, b.dst_cap, zwant(zi));
    uint32_t cur = 0, nb = 0;
    int bug = 0, clean = 0, frames = 0, in_frame = 0, check = 0, first = 0;
    uint32_t last_flags = 0;  // of record nb - 1
    int32_t last_h = -1, ts0 = -1, ts1 = -1, ts2 = -1;
    int64_t lpos = 0;
    auto put = [&](uint32_t x, uint32_t y, uint32_t z, uint32_t kind) {
        if (cur >= cap_items) { bug = 1; return; }
        if (l == 0) items[cur] = make_uint4(x, y, z, kind);
        cur++;
    };
    auto rec = [&](const SBlk &d) {
        if (l == 0) bk[nb] = d;
        last_flags = d.flags;
        nb++;
    };
    for (;;) {
        int32_t err = 0;
        uint32_t fl = 0, chk = 0;
        const int ev = walk_next<ZPFX>(w, &err, &fl, &chk);
        // (prefix decode) a walk stopped inside a frame is a proven case too: that frame has no end, so no checks
        if (ev == EV_DONE) { clean = !in_frame || (ZPFX && w.stopped); break; }
        if (ev == EV_ERROR) { put(0, 0, (uint32_t)err, IT_ERR); break; }
        if (ev == EV_FSTART) {
            frames++;
            in_frame = 1;
            first = 1;
            last_h = ts0 = ts1 = ts2 = -1;
            put(0, 0, 0, IT_FSTART);
            continue;
        }
        if (ev == EV_FEND) {
            put((uint32_t)w.fcs, (uint32_t)(w.fcs >> 32), chk, IT_FEND | (fl << 8));
            in_frame = 0;
            // every frame ends behind a block of its own (a last block, if only an empty raw
            // one): zsfix finds this item, and the frame's content size in it, behind that
            // block's items
            if (l == 0 && nb > 0) bk[nb - 1].flags = (uint8_t)(last_flags | SB_FEND);
            check |= (fl & FE_CHECK) != 0;
            if (fl & FE_MISSING) break;
            continue;
        }
        if (nb >= cap_blk) { bug = 1; break; }
        SBlk d;
        d.bpos = w.bpos; d.bsize = w.bsize; d.slot = cur; d.lpos = (uint32_t)lpos;
        d.regen = 0; d.nseq = 0; d.sip = 0; d.hsrc = -1;
        d.tsrc[0] = d.tsrc[1] = d.tsrc[2] = -1;
        d.btype = (uint8_t)w.btype; d.flags = 0;
        d.lerr = 0; d.serr = 0; d.r0 = d.r1 = d.r2 = 0; d.brep = 0; d.sll = d.sml = 0;
        d.e0 = d.e1 = d.e2 = d.fbase = 0; d.out = 0;
        const uint32_t ord = w.ordinal - 1;
        if (w.btype != 2) {  // zlit copies the bytes only while they fit the output
            const int64_t room = (int64_t)w.cap - w.lb;
            int stop = 0;
            d.regen = w.bsize;
            if ((int64_t)w.bsize <= room) {
                if (lpos + w.bsize > lend) { d.lerr = -104; stop = 1; }
                else { d.flags = SB_STORE; lpos += w.bsize; }
            }
            put(ord, (uint32_t)w.bsize, 0, IT_BSTART);
            put((uint32_t)w.bsize, 0, 0, IT_SEQ);
            put(0, 0, 0, IT_BEND);
            w.lb += w.bsize;
            rec(d);
            if (stop) break;
            continue;
        }
        LitHdr h;
        int32_t e = lit_header(s, w.bpos, w.bsize, h);
        put(ord, e ? 0u : (uint32_t)h.regen, 0, IT_BSTART);
        if (e) { put(0, 0, (uint32_t)e, IT_ERR); d.lerr = e; rec(d); break; }
        if (lpos + h.regen + 4 > lend) { d.lerr = -104; rec(d); break; }
        d.regen = h.regen;
        d.flags = SB_LIT;
        if (h.type == 2) last_h = (int32_t)nb;
        d.hsrc = last_h;
        lpos += h.regen;
        const int32_t end = w.bpos + w.bsize;
        int32_t ip = w.bpos + h.sec, nseq = 0, used = 0;
        e = nbseq_header(s, ip, end, &nseq, &used);
        if (e) { put(0, 0, (uint32_t)e, IT_ERR); rec(d); break; }
        ip += used;
        w.lb += (int64_t)h.regen + 3 * (int64_t)nseq;
        if (d.slot + 3 + (uint32_t)nseq > cap_items) { bug = 1; break; }
        if (nseq > 0) {
            if (ip + 1 > end) { put(0, 0, (uint32_t)E_SRCSIZE, IT_ERR); rec(d); break; }
            const uint32_t modes = rd8(s, ip);
            if ((modes & 3) && strict_reserved) { put(0, 0, (uint32_t)E_CORRUPT, IT_ERR); rec(d); break; }
            if (((modes >> 6) & 3) != 3) ts0 = (int32_t)nb;
            if (((modes >> 4) & 3) != 3) ts1 = (int32_t)nb;
            if (((modes >> 2) & 3) != 3) ts2 = (int32_t)nb;
            d.tsrc[0] = ts0; d.tsrc[1] = ts1; d.tsrc[2] = ts2;
            d.sip = ip;
        }
        d.nseq = nseq;
        d.flags |= SB_SEQ | (first ? SB_FIRST : 0);
        first = 0;
        cur = d.slot + 3 + (uint32_t)nseq;
        rec(d);
    }
    if (l == 0) {
        zi.n_items = bug ? 0xFFFFFFFFu : cur;
        si.nb = (int32_t)nb;
        si.ok = !bug && clean && frames >= 1 && frames <= max_frames && !check;
        si.frames = frames;
    }
}

struct SBSmem {
    alignas(16) uint8_t ring[SRING + 16];  // first: its reads need no base add
    LitSmem lit;  // wave 0
    ASmem a;      // wave 1: table-build scratch
    alignas(16) uint16_t cells[TAB_CELLS];
    alignas(16) uint32_t vx[TAB_CELLS];  // value pass: value base | extra bits << 24
    alignas(16) uint32_t sy[TAB_CELLS];  // state pass: see zsblk_kernel
};

// the description of field f (0 LL, 1 OF, 2 ML) in block d's sequence
// section: its mode, and its first byte (-1 if an earlier one does not parse)
__device__ __forceinline__ int32_t seq_desc(ASmem &sm, const gc_u8 *s, const SBlk &d, int f, int32_t *mode) {
    const int32_t end = d.bpos + d.bsize;
    const uint32_t modes = rd8(s, d.sip);
    int32_t ip = d.sip + 1;
    for (int g = 0; g < f; g++) {
        const int32_t mg = (modes >> (6 - 2 * g)) & 3;
        if (mg == 1) {
            ip += 1;
        } else if (mg == 2) {
            const int32_t n = end - ip, k = n < 256 ? n : 256;
            stage_bytes(sm.stage, s, ip, k);
            int32_t ms = g == 0 ? 35 : g == 1 ? 31 : 52, a = 0;
            const int32_t c = read_ncount(sm.stage, k, sm.norm, &ms, &a, g == 1 ? 8 : 9);
            if (c < 0 || c > n) return -1;
            ip += c;
        }
    }
    *mode = (modes >> (6 - 2 * f)) & 3;
    return ip;
}

// 16 bytes of the ring at byte q (multiple of 4): bits [left - 96, left)
__device__ __forceinline__ void sfill(const uint8_t *ring, int32_t left, uint64_t &hi, uint32_t &lo) {
    const int32_t cb = ((left - 96) >> 5) << 2;
    const uint32_t *w = (const uint32_t *)(ring + (cb & (SRING - 1)));
    const uint32_t d0 = uniform(w[0]), d1 = uniform(w[1]), d2 = uniform(w[2]), d3 = uniform(w[3]);
    const uint64_t A = ((uint64_t)d1 << 32) | d0, B = ((uint64_t)d3 << 32) | d2;
    const int32_t t = left - 8 * cb - 64;
    hi = (A >> t) | (B << (64 - t));
    lo = (uint32_t)(A >> (t - 32));
}

// chunk c of the stream's 16-byte blocks (relative to b16): this lane's 32 B.
// The loads are unconditional (clamped into the stream) so a prefetch stays
// in flight until its chunk is stored; schunk_put zeroes what lies outside.
__device__ __forceinline__ void schunk_ld(const gc_u4 *b16, int32_t c, int32_t kt, uint4 &v0, uint4 &v1) {
    const int32_t k0 = c * (SCHUNK / 16) + 2 * lane_id();
    const int32_t a0 = k0 < 0 ? 0 : k0 > kt ? kt : k0, a1 = k0 + 1 < 0 ? 0 : k0 + 1 > kt ? kt : k0 + 1;
    v0 = b16[a0];
    v1 = b16[a1];
}
__device__ __forceinline__ void schunk_put(uint8_t *ring, int32_t c, int32_t kt, int32_t m, uint4 v0, uint4 v1) {
    const int32_t k0 = c * (SCHUNK / 16) + 2 * lane_id(), k1 = k0 + 1;
    if (k0 < 0 || k0 > kt) v0 = make_uint4(0, 0, 0, 0);
    if (k1 < 0 || k1 > kt) v1 = make_uint4(0, 0, 0, 0);
    v0 = zclip(v0, k0, m);
    v1 = zclip(v1, k1, m);
    const int32_t q = (c * SCHUNK + 32 * lane_id()) & (SRING - 1);
    *(uint4 *)(ring + q) = v0;
    *(uint4 *)(ring + q + 16) = v1;
    if (q == 0) *(uint4 *)(ring + SRING) = v0;  // mirror: a 16-byte read never wraps
}
// next n (<= 32) bits below the c already consumed from the top of w (scalar code)
__device__ __forceinline__ uint32_t sget(uint64_t w, int32_t &c, uint32_t n) {
    const uint32_t v = n ? (uint32_t)((w << c) >> (64 - n)) : 0u;
    c += (int32_t)n;
    return v;
}

// s_bfe_u32: bits [op[4:0], op[4:0] + op[22:16]) of v (the packed operand
// lets a state-pass cell serve as its own bit-field descriptor)
__device__ __forceinline__ uint32_t sbfe(uint32_t v, uint32_t op) {
    uint32_t r;
    asm("s_bfe_u32 %0, %1, %2" : "=s"(r) : "s"(v), "s"(op));
    return r;
}

// lane j of (r0, r1, r2, r3) := (v0, v1, v2, v3): one lane select in M0 (a
// second scalar operand would break the constant-bus limit), s_nop for the
// M0 write before its first use as a lane select
__device__ __forceinline__ void record4(uint32_t &r0, uint32_t &r1, uint32_t &r2, uint32_t &r3, uint32_t v0,
                                        uint32_t v1, uint32_t v2, uint32_t v3, int32_t j) {
    asm volatile(
        "s_nop 0\n\t"
        "v_writelane_b32 %0, %4, m0\n\tv_writelane_b32 %1, %5, m0\n\t"
        "v_writelane_b32 %2, %6, m0\n\tv_writelane_b32 %3, %7, m0"
        : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3)
        : "s"(v0), "s"(v1), "s"(v2), "s"(v3), "{m0}"(j));
}

// t[k] for a wave-uniform k: the index scaled by a VALU shift straight from
// the scalar register (no scalar shift + move)
__device__ __forceinline__ uint32_t lds_u32(const uint32_t *t, uint32_t k) {
    uint32_t a;
    asm("v_lshlrev_b32 %0, 2, %1" : "=v"(a) : "s"(k));
    return *(const uint32_t *)((const uint8_t *)t + a);
}

__global__ __launch_bounds__(128) void zsblk_kernel(const jfs_dev_block *__restrict__ blocks, int nblk,
                                                    const ZInfo *__restrict__ info, uint8_t *__restrict__ litbuf,
                                                    uint4 *__restrict__ items_all, SScr sc) {
    __shared__ SBSmem sm;
    const int64_t g = blockIdx.x;
    const int bi = input_of(sc.in, nblk, g);
    const SIn &si = sc.in[bi];
    const int64_t k = g - si.blk_off;
    if (k >= si.nb) return;
    SBlk *bk = sc.blk + si.blk_off;
    const SBlk d = bk[k];
    const jfs_dev_block b = blocks[bi];
    const ZInfo zi = info[bi];
    const gc_u8 *s = (const gc_u8 *)b.src;
    const int l = lane_id();
    if (threadIdx.x < 64) {  // wave 0: literals (zlit semantics)
        g_u8 *lb = (g_u8 *)litbuf + zi.lit_off;
        if (d.btype != 2) {
            if (d.flags & SB_STORE) {
                if (d.btype == 0) {
                    for (int32_t q = l; q < d.bsize; q += 64) lb[d.lpos + q] = s[d.bpos + q];
                } else {
                    const uint8_t v = (uint8_t)rd8(s, d.bpos);
                    for (int32_t q = l; q < d.bsize; q += 64) lb[d.lpos + q] = v;
                }
            }
            return;
        }
        if (!(d.flags & SB_LIT)) return;
        LitHdr h;
        (void)lit_header(s, d.bpos, d.bsize, h);  // parsed by the walk
        if (l == 0) sm.lit.cur = -1;
        __builtin_amdgcn_wave_barrier();
        int32_t e = 0;
        if (h.type == 3) {
            if (d.hsrc < 0) {
                e = E_CORRUPT;
            } else {
                const SBlk hs = bk[d.hsrc];
                LitHdr hh;
                (void)lit_header(s, hs.bpos, hs.bsize, hh);
                int32_t m = 0;
                const int32_t u = read_huf(sm.lit, s, s, hs.bpos + hh.hsz, hh.csize, 0, false, &m);
                if (u < 0 || u >= hh.csize) e = E_CORRUPT;
                else lit_set_cur(sm.lit, m == 12 ? 2 : 0, m);
                __builtin_amdgcn_wave_barrier();
            }
        }
        if (!e) e = lit_block(sm.lit, s, s, h, d.bpos, lb, (int64_t)d.lpos);
        if (l == 0) bk[k].lerr = e;
        return;
    }
    // wave 1: FSE tables and sequences
    if (d.btype != 2 || !(d.flags & SB_SEQ)) return;
    g_u4 *it = (g_u4 *)items_all + zi.item_off + d.slot;
    uint32_t r0 = SYMB | (0u << 29), r1 = SYMB | (1u << 29), r2 = SYMB | (2u << 29);
    auto finish = [&](uint32_t brep, int32_t serr, uint64_t sll, uint64_t sml) {
        if (l == 0) {
            SBlk &o = bk[k];
            o.r0 = r0; o.r1 = r1; o.r2 = r2;
            o.brep = brep; o.serr = serr; o.sll = sll; o.sml = sml;
        }
    };
    if (d.nseq == 0) {
        if (l == 0) {
            it[1] = make_uint4(0, 0, 0, IT_BREP);
            it[2] = make_uint4(0, 0, 0, IT_BEND);
        }
        finish(1, 0, 0, 0);
        return;
    }
    const int32_t end = d.bpos + d.bsize;
    const uint32_t modes = rd8(s, d.sip);
    int32_t ip = d.sip + 1, al[3] = {0, 0, 0};
    bool bad = false;
#pragma unroll
    for (int f = 0; f < 3; f++) {
        if (bad) break;
        const int32_t mo = (modes >> (6 - 2 * f)) & 3;
        const uint32_t area = f == 0 ? 0u : f == 1 ? 512u : 768u;
        uint32_t curc = 0;
        int32_t have = 0;
        if (mo != 3) {
            const int32_t c = seq_table_g(sm.a, sm.cells, area, &curc, &al[f], &have, mo, s, ip, end - ip, f);
            if (c < 0) bad = true;
            else ip += c;
        } else if (d.tsrc[f] < 0) {
            bad = true;  // repeat mode without a previous table
        } else {
            const SBlk sb = bk[d.tsrc[f]];
            int32_t smo = 0;
            const int32_t sp = seq_desc(sm.a, s, sb, f, &smo);
            if (sp < 0 || seq_table_g(sm.a, sm.cells, area, &curc, &al[f], &have, smo, s, sp,
                                      sb.bpos + sb.bsize - sp, f) < 0)
                bad = true;
        }
    }
    if (bad) {
        if (l == 0) it[1] = make_uint4(0, 0, (uint32_t)E_CORRUPT, IT_ERR);
        finish(0, 1, 0, 0);
        return;
    }
    // cells: vx = the symbol's value base | extra bits << 24 (OF: extra bits
    // only, base 1 << bits) for the value pass; sy for the state pass =
    // (extra bits + state bits) << 5 | state bits << 16 | next-state base << 23.
    // The three cells of a sequence summed hold its total bit count in bits
    // [11:5] (<= 89), and each cell is an s_bfe operand (offset [4:0] = 0,
    // width [22:16]) for its own state bits.
#pragma unroll
    for (int f = 0; f < 3; f++) {
        const uint32_t area = f == 0 ? 0u : f == 1 ? 512u : 768u;
        const int32_t size = 1 << al[f];
        for (int u = l; u < size; u += 64) {
            const uint32_t c = sm.cells[area + u], sym = c & 63, ns = c >> 6;
            const uint32_t nbt = (uint32_t)al[f] - (31u - (uint32_t)__builtin_clz(ns));
            const uint32_t nsb = (ns << nbt) - (uint32_t)size;
            uint32_t x;
            if (f == 0) x = LL_BASE[sym < 36 ? sym : 0] | ((uint32_t)LL_BITS[sym < 36 ? sym : 0] << 24);
            else if (f == 1) x = sym << 24;
            else x = ML_BASE[sym < 53 ? sym : 0] | ((uint32_t)ML_BITS[sym < 53 ? sym : 0] << 24);
            sm.vx[area + u] = x;
            sm.sy[area + u] = (((x >> 24) + nbt) << 5) | (nbt << 16) | (nsb << 23);
        }
    }
    // the bitstream [ip, end), staged in SCHUNK pieces below its top
    const uintptr_t a = (uintptr_t)(s + ip);
    const gc_u4 *b16 = (const gc_u4 *)(a & ~(uintptr_t)15);
    const int32_t m = (int32_t)(a & 15), bsz = end - ip, top = m + bsz, m8 = 8 * m;
    const uint32_t last = bsz > 0 ? rd8(s, end - 1) : 0u;
    if (last == 0) {
        if (l == 0) it[1] = make_uint4(0, 0, (uint32_t)E_CORRUPT, IT_ERR);
        finish(0, 1, 0, 0);
        return;
    }
    const int32_t kt = (top - 1) >> 4, ct = (top - 1) / SCHUNK;
    int32_t lo_c = ct - 2 > -1 ? ct - 2 : -1;  // lowest resident chunk
    {
        uint4 v[3][2];
#pragma unroll
        for (int c = 0; c < 3; c++) schunk_ld(b16, ct - c, kt, v[c][0], v[c][1]);
#pragma unroll
        for (int c = 0; c < 3; c++)
            if (ct - c >= lo_c) schunk_put(sm.ring, ct - c, kt, m, v[c][0], v[c][1]);
    }
    uint4 pf0, pf1;  // chunk lo_c - 1, loaded ahead
    schunk_ld(b16, lo_c - 1, kt, pf0, pf1);
    __builtin_amdgcn_wave_barrier();
    // Two passes per 64 sequences.  The STATE pass is the only serial part:
    // wave-uniform (scalar registers), per sequence three cells and one
    // 128-bit bitstream window (a dword per lane) from LDS read together,
    // then the bit count (one sum of the cells), the 32 state bits below it
    // (two v_readlane and one shift) and the three next states (one s_bfe each: the cells are
    // their own bfe operands) -- it records (position, states) in lane j of
    // four VGPRs.  The VALUE pass is lane-parallel over the
    // recorded sequences: extra bits -> literal length, match length, offset
    // value; the repeat-offset updates as a prefix composition of
    // per-sequence transforms of (rep0, rep1, rep2) (SYMB terms, see rep_res)
    // over the lanes; the items stored together.
    int32_t left = (int32_t)uniform((uint32_t)(8 * (top - 1) + (31 - __builtin_clz(last))));
    const int32_t m8u = (int32_t)uniform((uint32_t)m8);
    const uint32_t *tl = sm.sy, *to = sm.sy + 512, *tm = sm.sy + 768;
    uint32_t sll, sof, sml;
    {
        uint64_t hi;
        uint32_t lo;
        sfill(sm.ring, left, hi, lo);
        int32_t c = 0;
        sll = sget(hi, c, uniform((uint32_t)al[0]));
        sof = sget(hi, c, uniform((uint32_t)al[1]));
        sml = sget(hi, c, uniform((uint32_t)al[2]));
        left -= c;
    }
    uint64_t Sll = 0, Sml = 0;
    int32_t serr = 0;
    g_u4 *itp = it + 2;
    const int32_t nseq = (int32_t)uniform((uint32_t)d.nseq);
    uint32_t rl = 0, rsl = 0, rso = 0, rsm = 0;  // lane j: bit position and states of pending sequence j
    // the value pass over the pending sequences (lanes [0, pn)); r0..r2 carry
    // the block's repeat offsets (symbolic in its entry state)
    auto values = [&](int32_t pn) {
        const bool on = l < pn;
        uint32_t ll = 0, ml = 0, ofv = 4;
        if (on) {
            const uint32_t bl = sm.vx[rsl], bo = sm.vx[512 + rso], bm = sm.vx[768 + rsm];
            const int32_t cb = (((int32_t)rl - 96) >> 5) << 2;
            const uint32_t *w = (const uint32_t *)(sm.ring + (cb & (SRING - 1)));
            const uint64_t A = ((uint64_t)w[1] << 32) | w[0], B = ((uint64_t)w[3] << 32) | w[2];
            const int32_t t = (int32_t)rl - 8 * cb - 64;
            const uint64_t hi = (A >> t) | (B << (64 - t));
            int32_t c = 0;
            const uint32_t ofc = bo >> 24;
            ofv = (1u << ofc) + sget(hi, c, ofc);
            if (ofc == 31) ofv = OFF_BEYOND + 3u;  // as zvalues: the item offset is ofv - 3
            ml = (bm & 0xFFFFFFu) + sget(hi, c, bm >> 24);
            ll = (bl & 0xFFFFFFu) + sget(hi, c, bl >> 24);
        }
        // this sequence's transform of (rep0, rep1, rep2): terms are constants
        // or SYMB | j << 29 | d = max(1, rep_j - d) of the batch's entry state
        const uint32_t I0 = SYMB, I1 = SYMB | (1u << 29), I2 = SYMB | (2u << 29);
        uint32_t t0 = I0, t1 = I1, t2 = I2;
        if (on) {
            if (ofv > 3) {
                t0 = ofv - 3; t1 = I0; t2 = I1;
            } else {
                const uint32_t kk = ofv - 1 + (ll == 0 ? 1u : 0u);
                if (kk == 1) { t0 = I1; t1 = I0; }
                else if (kk == 2) { t0 = I2; t1 = I0; t2 = I1; }
                else if (kk == 3) { t0 = I0 + 1u; t1 = I0; t2 = I1; }
            }
        }
        auto dec = [](uint32_t y, uint32_t dd) -> uint32_t {
            if (y & SYMB) return y + dd;
            return y > dd ? y - dd : 1u;
        };
        auto sub = [&](uint32_t x, uint32_t a0, uint32_t a1, uint32_t a2) -> uint32_t {
            if (!(x & SYMB)) return x;
            const uint32_t j = (x >> 29) & 3u, dd = x & 0x1FFFFFFFu;
            return dec(j == 0 ? a0 : j == 1 ? a1 : a2, dd);
        };
#pragma unroll
        for (int sft = 1; sft < 64; sft <<= 1) {  // inclusive prefix composition over the lanes
            const uint32_t a0 = (uint32_t)__shfl_up((int)t0, sft, 64), a1 = (uint32_t)__shfl_up((int)t1, sft, 64),
                           a2 = (uint32_t)__shfl_up((int)t2, sft, 64);
            if (l >= sft) {
                const uint32_t n0 = sub(t0, a0, a1, a2), n1 = sub(t1, a0, a1, a2), n2 = sub(t2, a0, a1, a2);
                t0 = n0; t1 = n1; t2 = n2;
            }
        }
        const uint32_t off = sub(t0, r0, r1, r2);  // the offset = rep0 after the sequence
        if (on) itp[l] = make_uint4(ll, ml, off, IT_SEQ);
        const uint32_t e0 = readlane(t0, pn - 1), e1 = readlane(t1, pn - 1), e2 = readlane(t2, pn - 1);
        const uint32_t n0 = sub(e0, r0, r1, r2), n1 = sub(e1, r0, r1, r2), n2 = sub(e2, r0, r1, r2);
        r0 = n0; r1 = n1; r2 = n2;
        Sll += dwave_sum(ll);
        Sml += dwave_sum(ml);
        itp += pn;
    };
    // The reader enters chunk lo_c - 1 soon when ((left - 96) >> 3) - 8 <
    // lo_c * SCHUNK; one compare against max(that, overflow) per sequence.
    // The rotation overwrites chunk lo_c + 3's slot: the pending sequences
    // (<= 64 x 89 bits above the reader) never reach it, so no flush first.
    auto threshold = [&]() -> int32_t {
        const int32_t r = lo_c > -1 ? 8 * lo_c * SCHUNK + 160 : INT32_MIN;
        return (int32_t)uniform((uint32_t)(r > m8u ? r : m8u));
    };
    int32_t thr = threshold();
    const uint32_t lane4 = 4u * (uint32_t)l;
    uint32_t T = 0;  // the last sequence's summed cells
    for (int32_t i0 = 0; i0 < nseq; i0 += 64) {
        const int32_t n = (int32_t)uniform((uint32_t)(nseq - i0 < 64 ? nseq - i0 : 64));
        // an overflow does not leave the loop (one exit keeps it scalar): the
        // rest of the batch decodes garbage inside the ring and tables, and
        // only the sequences before it are kept
        int32_t ovf = n;
        for (int32_t j = 0; j < n; j++) {
            if (left < thr) {
                if (left < m8u) {
                    ovf = ovf < j ? ovf : j;
                } else {
                    schunk_put(sm.ring, lo_c - 1, kt, m, pf0, pf1);
                    lo_c--;
                    schunk_ld(b16, lo_c - 1, kt, pf0, pf1);
                    __builtin_amdgcn_wave_barrier();
                    thr = threshold();
                }
            }
            // lane i: dword i of the window from bit bb (the mirror covers
            // lanes 0..4 at the ring's top; other lanes read unused bytes)
            const int32_t bb = (left - 96) & ~31;
            const uint32_t wv = *(const uint32_t *)(sm.ring + (((uint32_t)bb >> 3) & (SRING - 4)) + lane4);
            const uint32_t cl = lds_u32(tl, sll), co = lds_u32(to, sof), cm = lds_u32(tm, sml);
            __builtin_amdgcn_sched_barrier(0);  // all four reads in flight together
            const uint32_t yl = uniform(cl), yo = uniform(co), ym = uniform(cm);
            record4(rl, rsl, rso, rsm, (uint32_t)left, sll, sof, sml, j);
            T = yl + yo + ym;
            left -= (int32_t)((T >> 5) & 127u);  // extra bits + state bits
            // the next states' bits start at `left`, e = left - bb in [7, 127]
            const int32_t e = left - bb, dw = e >> 5;
            const uint32_t F = (uint32_t)((((uint64_t)readlane(wv, dw + 1) << 32) | readlane(wv, dw)) >> (e & 31));
            const uint32_t no = (yo >> 16) & 31u, nm = (ym >> 16) & 31u;
            sof = (yo >> 23) + sbfe(F, yo);
            sml = (ym >> 23) + sbfe(F, ym + no);
            sll = (yl >> 23) + sbfe(F, yl + no + nm);
        }
        if (ovf) values(ovf);
        if (ovf < n) {
            if (l == 0) itp[0] = make_uint4(0, 0, (uint32_t)E_CORRUPT, IT_ERR);
            serr = 1;
            break;
        }
    }
    if (!serr) {
        left += (int32_t)((T >> 16) & 31u);  // the last sequence reads no states
        if (l == 0)
            itp[0] = left == m8u ? make_uint4(0, 0, 0, IT_BEND) : make_uint4(0, 0, (uint32_t)E_CORRUPT, IT_ERR);
        serr = left != m8u;
    }
    finish(1, serr, Sll, Sml);
}

// Repeat-offset entry states (IT_BREP items, as zseqb's phase C), the first
// literal error (zlit's lit_err_blk / lit_err_code), and the output plan.
// Per frame: the repeat offsets restart at its first sequence block
// (SB_FIRST), fbase is the output offset it starts at, and at its end
// (SB_FEND) a declared content size must equal run - fbase.  A frame that
// declares more than the capacity left either produces that much (run > cap)
// or does not (the size check): the input is marked either way, and zexec
// gives libzstd's code.
__global__ __launch_bounds__(64) void zsfix_kernel(const jfs_dev_block *__restrict__ blocks, int nblk,
                                                   ZInfo *__restrict__ info, uint4 *__restrict__ items_all, SScr sc) {
    const int bi = blockIdx.x;
    if (bi >= nblk) return;
    const int l = lane_id();
    ZInfo &zi = info[bi];
    if (zi.ovf) return;
    SIn &si = sc.in[bi];
    const int32_t nb = si.nb;
    SBlk *bk = sc.blk + si.blk_off;
    g_u4 *items = (g_u4 *)items_all + zi.item_off;
    const int64_t cap = blocks[bi].dst_cap;
    uint32_t e0 = 1, e1 = 4, e2 = 8;
    int64_t run = 0, fbase = 0;
    int ok = si.ok && zi.n_items != 0xFFFFFFFFu;
    uint32_t lerr_blk = 0xFFFFFFFFu;
    int32_t lerr_code = 0;
    for (int32_t k0 = 0; k0 < nb; k0 += 64) {
        const int32_t kk = k0 + l, cnt = nb - k0 < 64 ? nb - k0 : 64;
        SBlk d;
        if (kk < nb) d = bk[kk];
        else d = bk[k0];
        const uint32_t bt = d.btype, fl = d.flags;
        // the IT_FEND item behind a frame's last block: {fcs lo, fcs hi, checksum, kind | FE_* << 8}
        uint4 fe = make_uint4(0, 0, 0, 0);
        if (ok && kk < nb && (fl & SB_FEND)) fe = items[d.slot + 3 + (bt == 2 ? (uint32_t)d.nseq : 0u)];
        uint32_t me0 = 0, me1 = 0, me2 = 0;
        int64_t mout = 0, mbase = 0;
        for (int32_t j = 0; j < cnt; j++) {
            const uint32_t jbt = readlane(bt, j), jfl = readlane(fl, j), jslot = readlane(d.slot, j);
            const int32_t jregen = (int32_t)readlane((uint32_t)d.regen, j), jbsize = (int32_t)readlane((uint32_t)d.bsize, j);
            const int32_t jlerr = (int32_t)readlane((uint32_t)d.lerr, j), jserr = (int32_t)readlane((uint32_t)d.serr, j);
            const uint64_t jsll = ((uint64_t)readlane((uint32_t)(d.sll >> 32), j) << 32) | readlane((uint32_t)d.sll, j);
            const uint64_t jsml = ((uint64_t)readlane((uint32_t)(d.sml >> 32), j) << 32) | readlane((uint32_t)d.sml, j);
            if (lerr_blk == 0xFFFFFFFFu && jlerr != 0) { lerr_blk = (uint32_t)(k0 + j); lerr_code = jlerr; }
            if (jbt == 2 && (jfl & SB_SEQ)) {
                if (jfl & SB_FIRST) { e0 = 1; e1 = 4; e2 = 8; }
                if (readlane(d.brep, j) && l == 0) items[jslot + 1] = make_uint4(e0, e1, e2, IT_BREP);
                if (l == j) { me0 = e0; me1 = e1; me2 = e2; }
                const uint32_t x0 = readlane(d.r0, j), x1 = readlane(d.r1, j), x2 = readlane(d.r2, j);
                const uint32_t n0 = rep_res(x0, e0, e1, e2), n1 = rep_res(x1, e0, e1, e2), n2 = rep_res(x2, e0, e1, e2);
                e0 = n0; e1 = n1; e2 = n2;
                ok = ok && !jserr && jsll <= (uint64_t)jregen;
            } else if (jbt != 2) {
                ok = ok && (jfl & SB_STORE);
            } else {
                ok = 0;
            }
            ok = ok && !jlerr;
            if (l == j) { mout = run; mbase = fbase; }
            run += jbt == 2 ? (int64_t)jregen + (int64_t)(jsml < (1ull << 40) ? jsml : (1ull << 40)) : (int64_t)jbsize;
            if (run > cap) ok = 0;
            if (jfl & SB_FEND) {
                const uint64_t jfcs = ((uint64_t)readlane(fe.y, j) << 32) | readlane(fe.x, j);
                if (((readlane(fe.w, j) >> 8) & FE_FCS) && (uint64_t)(run - fbase) != jfcs) ok = 0;
                fbase = run;
            }
        }
        if (kk < nb) {
            bk[kk].e0 = me0; bk[kk].e1 = me1; bk[kk].e2 = me2;
            bk[kk].fbase = (uint32_t)mbase;  // (an input whose run passes 2^31 is marked below)
            bk[kk].out = mout;
        }
    }
    if (run > 0x7FFFFFFF) ok = 0;
    // prefix decode: the origin map is settled and gathered over [0, want) only
    // (origins point backwards), and that is the result
    if (ZPFX && run > (int64_t)zwant(zi)) run = zwant(zi);
    if (l == 0) {
        zi.lit_err_blk = lerr_blk;
        zi.lit_err_code = lerr_code;
        si.todo = !ok;
        si.total = run;
        sc.todo[bi] = !ok;
    }
}

// grid (x: block record, y: ZSE_PARTS ranges of the block's sequences): a
// range's workgroup first sums the items before it (a coalesced pass: its
// start in the output and in the literals), then scans its own and writes
// the entries
constexpr int ZSE_PARTS = 16;
__global__ __launch_bounds__(ST) void zsemit_kernel(int nblk, const ZInfo *__restrict__ info,
                                                    const uint4 *__restrict__ items_all, SScr sc) {
    __shared__ uint32_t scan_n[ST], scan_l[ST];
    const int64_t g = blockIdx.x;
    const int part = blockIdx.y;
    const int bi = input_of(sc.in, nblk, g);
    SIn &si = sc.in[bi];
    const int64_t k = g - si.blk_off;
    if (si.todo || k >= si.nb) return;
    const SBlk d = sc.blk[g];
    g_u32 *org = (g_u32 *)(sc.org + si.org_off);
    const int t = threadIdx.x;
    const int64_t o0 = d.out;
    if (ZPFX && o0 >= si.total) return;  // prefix decode: a block behind `want` (si.total <= want) is never read
    if (d.btype != 2) {
        for (int64_t i = part * ST + t; i < d.bsize; i += ST * ZSE_PARTS)
            org[o0 + i] = om::lit_entry((int64_t)(d.lpos + i));
        return;
    }
    const gc_u4 *it = (const gc_u4 *)items_all + info[bi].item_off + d.slot + 2;
    const int32_t nsb = d.nseq;
    const int32_t r0 = (int32_t)((int64_t)nsb * part / ZSE_PARTS), r1 = (int32_t)((int64_t)nsb * (part + 1) / ZSE_PARTS);
    // the items before this range
    uint32_t bn = 0, bl = 0;
    for (int32_t q = t; q < r0; q += ST) {
        const uint4 v = it[q];
        bl += v.x;
        bn += v.x + v.y;
    }
    scan_n[t] = bn;
    scan_l[t] = bl;
    __syncthreads();
    for (int o = ST / 2; o > 0; o >>= 1) {
        if (t < o) {
            scan_n[t] += scan_n[t + o];
            scan_l[t] += scan_l[t + o];
        }
        __syncthreads();
    }
    const uint32_t pre_n = scan_n[0], pre_l = scan_l[0];
    __syncthreads();
    const int32_t ns = r1 - r0, per = (ns + ST - 1) / ST;
    const int32_t q0 = r0 + (t * per < ns ? t * per : ns), q1 = q0 + per < r1 ? q0 + per : r1;
    uint32_t sn = 0, sl = 0;
    for (int32_t q = q0; q < q1; q++) {
        const uint4 v = it[q];
        sl += v.x;
        sn += v.x + v.y;
    }
    scan_n[t] = sn;
    scan_l[t] = sl;
    __syncthreads();
    for (int o = 1; o < ST; o <<= 1) {  // inclusive scan
        const uint32_t a = t >= o ? scan_n[t - o] : 0u, c = t >= o ? scan_l[t - o] : 0u;
        __syncthreads();
        scan_n[t] += a;
        scan_l[t] += c;
        __syncthreads();
    }
    int64_t pos = o0 + pre_n + (scan_n[t] - sn);
    uint32_t lp = d.lpos + pre_l + (scan_l[t] - sl);
    const uint32_t e0 = d.e0, e1 = d.e1, e2 = d.e2;
    // a match of this frame never takes a byte of the frame before: libzstd's
    // ZSTD_decompress restarts its prefix at every frame
    const int64_t fbase = (int64_t)d.fbase;
    bool bad = false;
    for (int32_t q = q0; q < q1 && !bad; q++) {
        const uint4 v = it[q];
        const uint32_t ll = v.x, ml = v.y, off = rep_res(v.z, e0, e1, e2);
        om::put_lits<int64_t>(org, pos, ll, om::lit_entry((int64_t)lp));
        pos += ll;
        lp += ll;
        if (ml) {
            if ((int64_t)off > pos - fbase) { bad = true; break; }  // before the frame start
            om::put_match<int64_t>(org, pos, ml, off);
            pos += ml;
        }
    }
    // the literals after the last sequence
    const int64_t rest = (int64_t)d.regen - (int64_t)d.sll;
    const int64_t tail = o0 + (int64_t)d.regen + (int64_t)d.sml - rest;
    if (part == ZSE_PARTS - 1)
        for (int64_t i = t; i < rest; i += ST) org[tail + i] = om::lit_entry((int64_t)(d.lpos + d.sll + i));
    if (bad) {
        si.todo = 1;
        sc.todo[bi] = 1;
    }
}

// grid (x: workgroups per input, y: input)
__global__ __launch_bounds__(ST) void zsjump_kernel(SScr sc, int round) {
    const int bi = blockIdx.y;
    SIn &si = sc.in[bi];
    if (si.todo) return;
    if (round > 0 && !si.jmp[round - 1]) return;
    g_u32 *org = (g_u32 *)(sc.org + si.org_off);
    if (om::jump_walk(org, si.total, ((int64_t)blockIdx.x * ST + threadIdx.x) * 4, (int64_t)gridDim.x * ST * 4,
                      [org](int32_t o) -> uint32_t { return org[o]; }))
        si.jmp[round] = 1;
}

// inputs (small-batch path) decoded by the origin map / handed to zexec
__device__ unsigned long long g_zsplit_counts[2];
// of the former, the inputs of two frames or more, and the frames they held
__device__ unsigned long long g_zsplit_frame_counts[2];

__global__ void zsverd_kernel(int nblk, SScr sc, int32_t *__restrict__ ret) {
    const int bi = blockIdx.x * blockDim.x + threadIdx.x;
    if (bi >= nblk) return;
    SIn &si = sc.in[bi];
    const int todo = si.todo || si.unsettled;
    si.todo = todo;
    sc.todo[bi] = todo;
    if (!todo) ret[bi] = (int32_t)si.total;
    atomicAdd(&g_zsplit_counts[todo ? 1 : 0], 1ull);
    if (!todo && si.frames >= 2) {
        atomicAdd(&g_zsplit_frame_counts[0], 1ull);
        atomicAdd(&g_zsplit_frame_counts[1], (unsigned long long)si.frames);
    }
}

__global__ __launch_bounds__(ST) void zsgather_kernel(const jfs_dev_block *__restrict__ blocks,
                                                      const ZInfo *__restrict__ info,
                                                      const uint8_t *__restrict__ litbuf, SScr sc) {
    const int bi = blockIdx.y;
    const SIn &si = sc.in[bi];
    if (si.todo) return;
    const int64_t p = ((int64_t)blockIdx.x * ST + threadIdx.x) * 4;
    const int64_t total = si.total;
    if (p >= total) return;
    const gc_u32 *org = (const gc_u32 *)(sc.org + si.org_off);
    const gc_u8 *lit = (const gc_u8 *)litbuf + info[bi].lit_off;
    // (runs before the verdict: the exact replay rewrites a marked input)
    if (!om::gather_quad(org, lit, (g_u8 *)blocks[bi].dst, p, total)) sc.in[bi].unsettled = 1;
}
