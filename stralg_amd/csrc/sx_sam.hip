// sx_sam.hip -- SAM text of k-edit search hits on the device, and the read mapper's loop around it
// (tools/readmappers/bwt_readmapper/bwt_readmapper.c map_read + bioinf/sam.c print_sam_line).
//
// One hit (sx_approx_hit) is an interval of a suffix array; it prints R - L lines
//     <qname>\t0\t<rname>\t<sa[i]+1>\t0\t<cigar>\t*\t0\t0\t<seq>\t<qual>\n          i = L .. R-1
// that differ in the position's digits only.  The second field is 0, or, where the batch brings a FLAG per read (the
// kernels' kFlags form: the reads of both strands), that FLAG in decimal.  Two steps (DESIGN.md
// section 11, "SAM text"):
//  * layout: a size pass gives every hit its byte count, (R - L) x (the fixed part for this read, record name and
//    CIGAR) plus the digits of every sa[i] + 1 (hits of more than 32 matches are summed by their whole workgroup),
//    and a 64-bit exclusive scan turns the counts into each hit's first output byte and the total.
//  * emit: writes the bytes of a window [byte_lo, byte_hi) of the output.  A workgroup owns a slice of the window,
//    finds the hit at its first byte by a search in the scanned offsets and the match inside the hit by a walk over
//    the interval (1024 matches a step), lays lines out in LDS, one lane a line, 256 lines a step (the CIGAR of a hit
//    is rendered once into LDS, not once per match), and stores the slice in 16-byte vector stores.  The last < 16
//    bytes of a window whose length is not a multiple of 16 are the only bytes stored singly.  Where a byte goes is
//    fixed by the scan alone (no atomics), so the text does not depend on scheduling.
// The output does not fit the device in general: the caller fills a fixed buffer window after window; lines may start
// in one window (or slice) and end in the next, the concatenation of the windows is the file.
#include "sx_common.hpp"
#include "sx_device.hpp"
#include "sx_scan.hpp"
#include "sx_hostio.hpp"
#include "sx_index.hpp"
#include "sx_locate.hpp"

#include <stdlib.h>

#include <vector>

namespace sx {

#ifndef SX_SAM_SLICE_BYTES
#define SX_SAM_SLICE_BYTES 16384u // output bytes a workgroup lays out in LDS (a multiple of 16)
#endif
#ifndef SX_SAM_WINDOW_BYTES
#define SX_SAM_WINDOW_BYTES (32u << 20) // window of the streamed form: one pinned staging buffer
#endif
static_assert(SX_SAM_SLICE_BYTES % 16 == 0 && SX_SAM_SLICE_BYTES >= 16 && SX_SAM_SLICE_BYTES <= 32768, "slice");

constexpr uint32_t kSlice = SX_SAM_SLICE_BYTES;
constexpr uint32_t kCigarMax = 80;  // 9 runs of M (5 digits) and 8 of I / D (1 digit) take 70 bytes; longer ones are cut
constexpr uint32_t kInlineMatches = 32;
constexpr uint32_t kWalk = 4; // matches per lane in one step of the walk inside a long hit

struct SamArgs {
    const uint4 *hits; // sx_approx_hit as two 16-byte words
    uint64_t n_hits;
    const uint32_t *sa;
    uint64_t sa_len;
    const uint32_t *const *sa_list; // one suffix array per record rank (then sa is not used)
    const uint64_t *sa_len_list;
    const uint8_t *names, *seqs, *quals;
    const uint32_t *name_off, *seq_off, *qual_off;
    uint32_t n_reads;
    const uint8_t *rnames;
    const uint32_t *rname_off;
    uint32_t n_records;
    // an index with a sampled suffix array (the kernels' kLocated form): the positions of a run of hits, located before
    // the layout; hit h's stand at positions[pos_off[h] - pos_base ..)
    const uint32_t *positions;
    const uint64_t *pos_off;
    uint64_t pos_base;
    const uint16_t *flags; // a FLAG per read (the kernels' kFlags form), or null: every line has FLAG 0
};

struct HitInfo {
    const uint32_t *pos; // the hit's positions: pos[0 .. cnt)
    uint32_t cnt, fixed, cig_len, m, flag;
    uint32_t name_b, name_l, seq_b, seq_l, qual_b, qual_l, rn_b, rn_l;
    uint4 gaps;
    uint32_t n_gaps;
};

__device__ __forceinline__ uint32_t dec_digits(uint32_t v)
{
    return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u
           : v < 10000000u ? 7u : v < 100000000u ? 8u : v < 1000000000u ? 9u : 10u;
}

// decimal digits of v into out[at ..) as far as cap allows (out == nullptr: count only); returns the new length
__device__ __forceinline__ uint32_t put_dec(uint8_t *out, uint32_t at, uint32_t cap, uint32_t v)
{
    const uint32_t nd = dec_digits(v);
    for (uint32_t d = 0; d < nd; ++d) {
        const uint32_t where = at + nd - 1u - d;
        if (out && where < cap) out[where] = (uint8_t)('0' + v % 10u);
        v /= 10u;
    }
    return at + nd < cap ? at + nd : cap;
}

// cigar.c edits_to_cigar of the hit's edit string in pattern order (stralg_host.c approx_cigar): runs of equal
// operations, "%d%c" each; at most cap bytes
__device__ __forceinline__ uint32_t cigar_render(uint8_t *out, uint32_t cap, uint32_t m, uint4 gaps, uint32_t ng)
{
    const uint32_t gw[4] = {gaps.x, gaps.y, gaps.z, gaps.w};
    uint32_t n_d = 0;
    for (uint32_t g = 0; g < ng; ++g) n_d += ((gw[g >> 1] >> (16u * (g & 1u))) & SX_APPROX_GAP_D) ? 1u : 0u;
    const uint32_t len = m + n_d;
    uint32_t w = 0, pos = 0, g = 0;
    while (pos < len) {
        const uint32_t e = g < ng ? (gw[g >> 1] >> (16u * (g & 1u))) & 0xFFFFu : 0u;
        uint32_t run = 0;
        uint8_t op = 'M';
        if (g < ng && (e & 0x7FFFu) == pos) {
            op = (e & SX_APPROX_GAP_D) ? 'D' : 'I';
            while (g < ng && pos < len) {
                const uint32_t e2 = (gw[g >> 1] >> (16u * (g & 1u))) & 0xFFFFu;
                if ((e2 & 0x7FFFu) != pos || (e2 & SX_APPROX_GAP_D) != (e & SX_APPROX_GAP_D)) break;
                ++g;
                ++pos;
                ++run;
            }
        } else {
            const uint32_t next = (g < ng && (e & 0x7FFFu) > pos && (e & 0x7FFFu) < len) ? (e & 0x7FFFu) : len;
            run = next - pos;
            pos = next;
        }
        w = put_dec(out, w, cap, run);
        if (w < cap) {
            if (out) out[w] = op;
            ++w;
        }
    }
    return w;
}

// what the lines of hit h are made of; false: the hit does not fit the batch (its query, interval or offsets)
template <bool kLocated, bool kFlags> __device__ __forceinline__ bool hit_info(const SamArgs &A, uint64_t h, HitInfo &I)
{
    const uint4 h0 = A.hits[2 * h];
    I.gaps = A.hits[2 * h + 1];
    I.cnt = 0;
    I.fixed = 0;
    I.cig_len = 0;
    I.flag = 0;
    I.pos = nullptr;
    const uint32_t vq = h0.x, L = h0.y, R = h0.z;
    if ((uint64_t)vq >= (uint64_t)A.n_reads * A.n_records || L > R) return false;
    const uint32_t read = vq / A.n_records, rec = vq - read * A.n_records;
    const uint32_t *sa = kLocated ? nullptr : A.sa_list ? A.sa_list[rec] : A.sa;
    const uint64_t sa_len = A.sa_list ? A.sa_len_list[rec] : A.sa_len;
    if ((uint64_t)R > sa_len) return false;
    I.name_b = A.name_off[read];
    I.seq_b = A.seq_off[read];
    I.qual_b = A.qual_off[read];
    I.rn_b = A.rname_off[rec];
    const uint32_t name_e = A.name_off[read + 1], seq_e = A.seq_off[read + 1], qual_e = A.qual_off[read + 1],
                   rn_e = A.rname_off[rec + 1];
    if (name_e < I.name_b || seq_e < I.seq_b || qual_e < I.qual_b || rn_e < I.rn_b) return false;
    I.name_l = name_e - I.name_b;
    I.seq_l = seq_e - I.seq_b;
    I.qual_l = qual_e - I.qual_b;
    I.rn_l = rn_e - I.rn_b;
    I.m = I.seq_l;
    I.n_gaps = h0.w >> 16;
    if (I.n_gaps > SX_APPROX_MAX_EDITS) I.n_gaps = SX_APPROX_MAX_EDITS;
    I.pos = kLocated ? A.positions + (A.pos_off[h] - A.pos_base) : sa + L;
    I.cnt = R - L;
    if (kFlags) I.flag = A.flags[read];
    return true;
}

// "\t0\t" + "\t" + "\t0\t" + "\t*\t0\t0\t" + "\t" + "\n": the 16 bytes of a line beside its fields and digits; a FLAG
// takes its digits in place of the first "0" (without kFlags I.flag is the constant 0: one digit, 16 bytes)
__device__ __forceinline__ uint32_t fixed_bytes(const HitInfo &I)
{
    return I.name_l + I.rn_l + I.cig_len + I.seq_l + I.qual_l + 15u + dec_digits(I.flag);
}

// ---- layout: bytes per hit ---------------------------------------------------------------------
template <bool kLocated, bool kFlags> __global__ __launch_bounds__(kBlock) void sam_size_kernel(SamArgs A, uint64_t *len_out, uint32_t *err)
{
    __shared__ uint64_t red[kWavesPerBlock];
    __shared__ uint32_t long_cnt[kBlock];
    __shared__ const uint32_t *long_pos[kBlock];
    const uint32_t t = threadIdx.x;
    const uint64_t h = (uint64_t)blockIdx.x * kBlock + t;
    uint64_t bytes = 0;
    long_cnt[t] = 0;
    if (h < A.n_hits) {
        HitInfo I = {};
        if (!hit_info<kLocated, kFlags>(A, h, I)) {
            atomicOr(err, 1u);
        } else {
            I.cig_len = cigar_render(nullptr, kCigarMax, I.m, I.gaps, I.n_gaps);
            bytes = (uint64_t)I.cnt * fixed_bytes(I);
            if (I.cnt <= kInlineMatches) {
                for (uint32_t i = 0; i < I.cnt; ++i) bytes += dec_digits(I.pos[i] + 1u);
            } else {
                long_cnt[t] = I.cnt;
                long_pos[t] = I.pos;
            }
        }
    }
    __syncthreads();
    // long intervals (up to 10^5 matches and more): the whole workgroup sums one's digits
    for (uint32_t u = 0; u < (uint32_t)kBlock; ++u) {
        const uint32_t cnt = long_cnt[u]; // (the same for every lane)
        if (cnt == 0) continue;
        const uint32_t *pos = long_pos[u];
        uint64_t d = 0;
        for (uint32_t i = t; i < cnt; i += kBlock) d += dec_digits(pos[i] + 1u);
        uint64_t tot;
        (void)block_exclusive_sum_u64(d, red, tot);
        if (u == t) bytes += tot;
    }
    if (h < A.n_hits) len_out[h] = bytes;
}

// ---- emit ---------------------------------------------------------------------------------------
struct HitLds {
    const uint32_t *pos;
    uint32_t cnt, fixed, cig_len;
    uint32_t name_b, name_l, seq_b, seq_l, qual_b, qual_l, rn_b, rn_l;
};

// n bytes of a line that begins at slice offset `off` (may be negative), clipped to the slice
__device__ __forceinline__ void put_bytes(uint8_t *obuf, int64_t &off, int64_t slice_len, const uint8_t *src, uint32_t n)
{
    int64_t k0 = off < 0 ? -off : 0, k1 = (int64_t)n < slice_len - off ? (int64_t)n : slice_len - off;
    for (int64_t k = k0; k < k1; ++k) obuf[off + k] = src[k];
    off += n;
}

template <bool kLocated, bool kFlags> __global__ __launch_bounds__(kBlock) void sam_emit_kernel(SamArgs A, const uint64_t *byte_off, uint64_t lo, uint64_t hi,
                                                          uint8_t *out)
{
    __shared__ uint4 obuf4[kSlice / 16];
    __shared__ uint8_t cig[kBlock * kCigarMax];
    __shared__ HitLds hl[kBlock];
    __shared__ uint32_t mo[kBlock + 1];
    __shared__ uint64_t red[kWavesPerBlock];
    __shared__ uint32_t red32[kWavesPerBlock];
    __shared__ uint64_t nxt[2];
    __shared__ uint16_t hflag[kFlags ? kBlock : 1]; // (kFlags) the FLAG of the step's hits
    uint8_t *obuf = (uint8_t *)obuf4;
    const uint32_t t = threadIdx.x;
    const uint64_t s_lo = lo + (uint64_t)blockIdx.x * kSlice;
    if (s_lo >= hi) return; // (the whole workgroup)
    const uint64_t s_hi = hi - s_lo < kSlice ? hi : s_lo + kSlice;
    const int64_t slice_len = (int64_t)(s_hi - s_lo);

    // the hit at the slice's first byte: the last h with byte_off[h] <= s_lo (byte_off[n_hits] = total > s_lo)
    uint64_t h = 0;
    {
        uint64_t b = A.n_hits;
        while (b - h > 1) {
            const uint64_t mid = h + (b - h) / 2;
            if (byte_off[mid] <= s_lo) h = mid;
            else b = mid;
        }
    }
    uint64_t pos = byte_off[h]; // first byte of line (h, i)
    uint32_t i = 0;
    {   // the walk inside the hit: whole steps of 1024 lines that end at or before the slice's first byte are skipped
        HitInfo I = {};
        if (hit_info<kLocated, kFlags>(A, h, I)) {
            I.cig_len = cigar_render(nullptr, kCigarMax, I.m, I.gaps, I.n_gaps);
            const uint32_t fixed = fixed_bytes(I);
            while (I.cnt - i > kWalk * kBlock) {
                uint64_t b = 0;
#pragma unroll
                for (uint32_t k = 0; k < kWalk; ++k) b += fixed + dec_digits(I.pos[i + k * kBlock + t] + 1u);
                uint64_t tot;
                (void)block_exclusive_sum_u64(b, red, tot);
                if (pos + tot > s_lo) break;
                pos += tot;
                i += kWalk * kBlock;
            }
        }
    }

    while (pos < s_hi && h < A.n_hits) {
        // hits h .. h + 255: how many lines each has left, the first 256 lines' hits, their CIGARs
        HitInfo I = {};
        uint32_t c = 0;
        if (h + t < A.n_hits && hit_info<kLocated, kFlags>(A, h + t, I)) c = I.cnt - (t == 0 ? (i < I.cnt ? i : I.cnt) : 0u);
        const uint32_t cc = c < (uint32_t)kBlock ? c : (uint32_t)kBlock;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan<OpAdd>(cc, red32, total);
        mo[t] = ex;
        if (t == 0) mo[kBlock] = total;
        if (cc && ex < (uint32_t)kBlock) {
            I.cig_len = cigar_render(cig + t * kCigarMax, kCigarMax, I.m, I.gaps, I.n_gaps);
            HitLds &H = hl[t];
            H.pos = I.pos;
            H.cnt = I.cnt;
            H.cig_len = I.cig_len;
            H.fixed = fixed_bytes(I);
            H.name_b = I.name_b, H.name_l = I.name_l, H.seq_b = I.seq_b, H.seq_l = I.seq_l;
            H.qual_b = I.qual_b, H.qual_l = I.qual_l, H.rn_b = I.rn_b, H.rn_l = I.rn_l;
            if (kFlags) hflag[t] = (uint16_t)I.flag;
        }
        __syncthreads();
        const uint32_t nlines = total < (uint32_t)kBlock ? total : (uint32_t)kBlock;
        if (nlines == 0) { // 256 hits without a line (malformed ones): on to the next
            h += kBlock;
            i = 0;
            __syncthreads();
            continue;
        }
        // line t of this step
        uint32_t u = 0, mi = 0, p1 = 0, len = 0;
        if (t < nlines) {
            uint32_t a = 0, b = kBlock; // mo[a] <= t < mo[b]
            while (b - a > 1) {
                const uint32_t mid = (a + b) / 2;
                if (mo[mid] <= t) a = mid;
                else b = mid;
            }
            u = a;
            mi = t - mo[u] + (u == 0 ? i : 0u);
            p1 = hl[u].pos[mi] + 1u;
            len = hl[u].fixed + dec_digits(p1);
        }
        uint32_t step_bytes;
        const uint32_t lstart = block_exclusive_scan<OpAdd>(len, red32, step_bytes);
        const uint64_t line_abs = pos + lstart;
        if (t < nlines && line_abs < s_hi && line_abs + len > s_lo) {
            const HitLds &H = hl[u];
            int64_t off = (int64_t)line_abs - (int64_t)s_lo;
            uint8_t dig[10];
            const uint32_t nd = put_dec(dig, 0, 10, p1);
            put_bytes(obuf, off, slice_len, A.names + H.name_b, H.name_l);
            if (kFlags) {
                uint8_t fdig[5];
                const uint32_t nf = put_dec(fdig, 0, 5, hflag[u]);
                put_bytes(obuf, off, slice_len, (const uint8_t *)"\t", 1);
                put_bytes(obuf, off, slice_len, fdig, nf);
                put_bytes(obuf, off, slice_len, (const uint8_t *)"\t", 1);
            } else {
                put_bytes(obuf, off, slice_len, (const uint8_t *)"\t0\t", 3);
            }
            put_bytes(obuf, off, slice_len, A.rnames + H.rn_b, H.rn_l);
            put_bytes(obuf, off, slice_len, (const uint8_t *)"\t", 1);
            put_bytes(obuf, off, slice_len, dig, nd);
            put_bytes(obuf, off, slice_len, (const uint8_t *)"\t0\t", 3);
            put_bytes(obuf, off, slice_len, cig + u * kCigarMax, H.cig_len);
            put_bytes(obuf, off, slice_len, (const uint8_t *)"\t*\t0\t0\t", 7);
            put_bytes(obuf, off, slice_len, A.seqs + H.seq_b, H.seq_l);
            put_bytes(obuf, off, slice_len, (const uint8_t *)"\t", 1);
            put_bytes(obuf, off, slice_len, A.quals + H.qual_b, H.qual_l);
            put_bytes(obuf, off, slice_len, (const uint8_t *)"\n", 1);
        }
        if (t == nlines - 1u) { // the line behind this step's last one
            const bool more = mi + 1u < hl[u].cnt;
            nxt[0] = h + u + (more ? 0u : 1u);
            nxt[1] = more ? mi + 1u : 0u;
        }
        __syncthreads();
        h = nxt[0];
        i = (uint32_t)nxt[1];
        pos += step_bytes;
        __syncthreads();
    }
    __syncthreads();
    // the slice leaves in 16-byte stores; a window that does not end on a 16-byte boundary has up to 15 single bytes
    uint8_t *dst = out + (s_lo - lo);
    const uint32_t full = (uint32_t)(slice_len / 16);
    for (uint32_t k = t; k < full; k += kBlock) stream_store16((uint4 *)dst + k, obuf4[k]);
    const uint32_t tail = (uint32_t)slice_len - full * 16u;
    if (t < tail) dst[full * 16u + t] = obuf[full * 16u + t];
}

// ---- the mapper's loop: remap per record, hits of all records in (read, record rank, hit) order ----------------------
__global__ __launch_bounds__(kBlock) void sam_remap_kernel(const uint8_t *seqs, const uint8_t *table, uint8_t *out, uint64_t lo,
                                                           uint64_t hi)
{
    const uint64_t i = lo + (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < hi) out[i] = table[seqs[i]];
}

// cnt[q * n_rec + r] = hits of read q in record r (ho: n_rec arrays of stride entries, the searches' hit offsets)
__global__ __launch_bounds__(kBlock) void sam_vq_count_kernel(const uint64_t *ho, uint64_t stride, uint32_t batch, uint32_t n_rec,
                                                              uint64_t *cnt)
{
    const uint64_t idx = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= (uint64_t)batch * n_rec) return;
    const uint32_t q = (uint32_t)(idx / n_rec), r = (uint32_t)(idx - (uint64_t)q * n_rec);
    cnt[idx] = ho[r * stride + q + 1] - ho[r * stride + q];
}

// hit j of the searches' hit arrays (record r's at seg[r] .. seg[r + 1]) goes behind the hits of its read in the
// records before r: query <- read * n_rec + r
__global__ __launch_bounds__(kBlock) void sam_merge_kernel(const uint4 *src, uint64_t n_hits, const uint64_t *seg, uint32_t n_rec,
                                                           const uint64_t *ho, uint64_t stride, uint32_t batch, const uint64_t *vbase,
                                                           uint4 *dst, uint32_t *err)
{
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n_hits) return;
    uint32_t r = 0;
    {
        uint32_t b = n_rec; // seg[r] <= j < seg[b]
        while (b - r > 1) {
            const uint32_t mid = (r + b) / 2;
            if (seg[mid] <= j) r = mid;
            else b = mid;
        }
    }
    uint4 h0 = src[2 * j];
    const uint32_t q = h0.x;
    if (q >= batch) {
        atomicOr(err, 2u);
        return;
    }
    const uint64_t at = vbase[(uint64_t)q * n_rec + r] + (j - seg[r] - ho[r * stride + q]);
    if (at >= n_hits) {
        atomicOr(err, 2u);
        return;
    }
    h0.x = q * n_rec + r;
    dst[2 * at] = h0;
    dst[2 * at + 1] = src[2 * j + 1];
}

// what the kernels get of a batch (SamArgs has sx_sam_batch's fields in its order)
static SamArgs sam_args_of(const sx_sam_batch &b)
{
    return SamArgs{(const uint4 *)b.d_hits, b.n_hits,     b.d_sa,       b.sa_len,     b.d_sa_list, b.d_sa_len_list, b.d_names,   b.d_seqs,
                   b.d_quals,               b.d_name_off, b.d_seq_off,  b.d_qual_off, b.n_reads,   b.d_rnames,      b.d_rname_off, b.n_records,
                   nullptr,                 nullptr,      0,            nullptr};
}

static int sam_args(sx_ctx *ctx, const sx_sam_batch *b, SamArgs &A)
{
    if (!ctx || !b) return SX_E_ARG;
    if (b->n_hits && (!b->d_hits || ((uintptr_t)b->d_hits & 15) || !(b->d_sa || (b->d_sa_list && b->d_sa_len_list))))
        return sx_fail_msg(ctx, SX_E_ARG, "SAM text: hits (16-byte aligned) and a suffix array are needed");
    if (!b->d_name_off || !b->d_seq_off || !b->d_qual_off || !b->d_rname_off || b->n_records == 0 ||
        (uint64_t)b->n_reads * b->n_records > 0xFFFFFFFFull)
        return sx_fail_msg(ctx, SX_E_ARG, "SAM text: offsets of the reads and record names; reads x records below 2^32");
    A = sam_args_of(*b);
    return 0;
}

// the same of a batch that may bring a FLAG per read
static int sam_args_ex(sx_ctx *ctx, const sx_sam_batch_ex *b, SamArgs &A)
{
    if (!b) return SX_E_ARG;
    SX_TRY(sam_args(ctx, &b->batch, A));
    if ((uintptr_t)b->d_read_flags & 1) return sx_fail_msg(ctx, SX_E_ARG, "SAM text: the reads' flags are 16-bit entries");
    A.flags = b->d_read_flags;
    return 0;
}

// the four forms of the two kernels: positions located beforehand or read from a suffix array, a FLAG per read or none
#define SX_SAM_KERNEL(kernel, A) \
    ((A).positions ? ((A).flags ? kernel<true, true> : kernel<true, false>) : ((A).flags ? kernel<false, true> : kernel<false, false>))

static int sam_layout(sx_ctx *ctx, const SamArgs &A, uint64_t *d_byte_off, uint64_t *total_out)
{
    *total_out = 0;
    SX_TRY(sx_slab_ensure(ctx, SX_SLAB_SORT, 4096));
    uint32_t *d_err = (uint32_t *)ctx->slab[SX_SLAB_SORT].p;
    SX_CHECK(hipMemsetAsync(d_err, 0, 16, ctx->stream));
    if (A.n_hits)
        sx_launch(ctx, SX_KC_SAM, A.n_hits * 40, SX_SAM_KERNEL(sam_size_kernel, A), dim3(sx_div_up(A.n_hits, kBlock)),
                  dim3(kBlock), A, d_byte_off, d_err);
    SX_TRY(device_scan64_inplace(ctx, d_byte_off, A.n_hits, SX_KC_SAM));
    uint32_t h[2] = {0, 0}, e = 0;
    SX_TRY(sx_readback(ctx, (const uint32_t *)(d_byte_off + A.n_hits), 2, h));
    SX_TRY(sx_readback(ctx, d_err, 1, &e));
    if (e) return sx_fail_msg(ctx, SX_E_ARG, "SAM text: a hit's query, interval or offsets lie outside the batch");
    *total_out = (uint64_t)h[0] | ((uint64_t)h[1] << 32);
    return 0;
}

// (asynchronous: the caller syncs)
static int sam_emit(sx_ctx *ctx, const SamArgs &A, const uint64_t *d_byte_off, uint64_t lo, uint64_t hi, uint8_t *d_out)
{
    if (hi <= lo) return 0;
    const uint64_t slices = (hi - lo + kSlice - 1) / kSlice;
    if (slices > 0x7FFFFFFFull) return sx_fail_msg(ctx, SX_E_ARG, "SAM text: window too long");
    // per line: its bytes out, 4 bytes of position in; the read's fields once a slice
    sx_launch(ctx, SX_KC_SAM, hi - lo, SX_SAM_KERNEL(sam_emit_kernel, A), dim3((uint32_t)slices), dim3(kBlock), A,
              d_byte_off, lo, hi, d_out);
    return 0;
}

template <class T, class H> static int upload(sx_ctx *ctx, sx_dev_scope &B, const T **d, const H *h, size_t count)
{
    T *p;
    SX_TRY(B.take(ctx, &p, count));
    if (count) SX_CHECK(hipMemcpyAsync(p, h, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    *d = p;
    return 0;
}

// ---- the pieces of the mapper's loop (sx_map_reads_core) -----------------------------------------------------------
// what a mapping call asks of its reads and records; records_ok: sx_map_dims_ok / sx_map_record_check with sigma >= 2
static int map_check(sx_ctx *ctx, uint64_t n_reads, uint64_t n_records, uint32_t flags, bool records_ok)
{
    if (flags & ~sx_map_known_flags) return sx_fail_msg(ctx, SX_E_ARG, "read mapping: unknown flags");
    if (sx_map_reads_limit(n_reads, n_records, flags) != 0)
        return sx_fail_msg(ctx, SX_E_ARG, "read mapping: reads x records (twice that for both strands) must stay below 2^32");
    if (!records_ok) return sx_fail_msg(ctx, SX_E_ARG, "read mapping: a record lacks its name, suffix array, tables or remap table");
    return 0;
}

// Room for the hits of a batch's searches: a guess to start with; a batch that needs more makes it
// grow, up to 2^27 hits or what a quarter of the free memory holds (72 bytes a hit: the searches' array, the merged one,
// the byte offsets), before the batch is halved -- a search over few reads leaves most of its lanes idle
struct HitRoom {
    uint64_t cap = 0, cap_max = 1ull << 26;
    sx_approx_hit *d_raw = nullptr;
    sx_dev_scope own;
    int init(sx_ctx *ctx, uint64_t guess)
    {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b) cap_max = free_b / 4 / 72 < (1ull << 27) ? free_b / 4 / 72 : 1ull << 27;
        else (void)hipGetLastError();
        if (cap_max < (1u << 16)) cap_max = 1u << 16;
        cap = guess < (1u << 16) ? 1u << 16 : guess > cap_max ? cap_max : guess;
        return own.take(ctx, &d_raw, (size_t)cap);
    }
    // the searches of `batch` reads need room for `need` hits: it grows where that is allowed (one read alone gets whatever
    // it needs); otherwise *halve, and the caller goes on with half the reads
    int grow_or_halve(sx_ctx *ctx, uint64_t need, uint32_t batch, bool *halve)
    {
        *halve = need > cap_max && batch > 1;
        if (*halve) return 0;
        cap = need + need / 4 > 2 * cap ? need + need / 4 : 2 * cap;
        if (cap > cap_max && need <= cap_max) cap = cap_max;
        own.drop(d_raw);
        return own.take(ctx, &d_raw, (size_t)cap);
    }
};

struct MapBufs { // what a mapping call holds on the device beside the hits' room
    uint8_t *d_pat, *d_win[2];
    uint64_t *d_ho, *d_vbase, *d_seg, *d_byte_off = nullptr;
    uint32_t *d_err;
    sx_approx_hit *d_merged = nullptr;
    // an index with a sampled suffix array: the lines in front of every hit of the batch, the positions of a run of hits
    uint64_t *d_pos_off = nullptr;
    uint32_t *d_positions = nullptr;
    uint64_t pos_cap = 0;
    uint64_t merged_cap = 0, stride = 0; // stride: entries of a record's hit offsets in d_ho
    size_t window = 0;
    sx_dev_scope own;
};

// The searches of reads q0 .. q0 + batch, record after record, into the room: seg[r] <- where record r's hits start,
// seg[records] <- how many there are.  SX_E_CAPACITY: the room is too small for the *need_out hits known of so far.
// [*p_lo, *p_hi): the sequence bytes of reads q0 .. q0 + batch
static int batch_bytes(sx_ctx *ctx, const sx_reads_dev &reads, uint32_t q0, uint32_t batch, uint64_t *p_lo, uint64_t *p_hi)
{
    if (reads.h_seq_off) {
        *p_lo = reads.h_seq_off[q0], *p_hi = reads.h_seq_off[q0 + batch];
    } else { // (the offsets were made on the device: the two this batch needs come back)
        const uint32_t *src[2] = {reads.d_seq_off + q0, reads.d_seq_off + q0 + batch};
        const uint32_t one[2] = {1, 1};
        uint32_t got[2];
        SX_TRY(sx_readback_ranges(ctx, src, one, 2, got));
        *p_lo = got[0], *p_hi = got[1];
    }
    return 0;
}

static int search_batch(sx_ctx *ctx, const sx_index *idx, const sx_reads_dev &reads, const MapBufs &M, const HitRoom &room, uint32_t q0,
                        uint32_t batch, int edits, std::vector<uint64_t> &seg, uint64_t *need_out)
{
    uint64_t p_lo, p_hi;
    SX_TRY(batch_bytes(ctx, reads, q0, batch, &p_lo, &p_hi));
    const uint32_t n_records = (uint32_t)idx->recs.size();
    uint64_t used = 0;
    for (uint32_t r = 0; r < n_records; ++r) {
        const sx_index_rec &R = idx->recs[r];
        if (p_hi > p_lo)
            sx_launch(ctx, SX_KC_REMAP, 2 * (p_hi - p_lo), sam_remap_kernel, dim3(sx_div_up(p_hi - p_lo, kBlock)), dim3(kBlock), reads.d_seqs,
                      (const uint8_t *)(idx->d_tabs + (size_t)r * 256), M.d_pat, p_lo, p_hi);
        uint64_t tot = 0;
        // (whichever form the record has: the hits and their order are the same)
        const int rc = sx_approx_search_record(ctx, R, M.d_pat, reads.d_seq_off + q0, batch, edits, M.d_ho + r * M.stride, room.d_raw + used,
                                               room.cap - used, &tot);
        if (rc == SX_E_CAPACITY) *need_out = used + tot;
        if (rc != 0) return rc;
        seg[r] = used;
        used += tot;
    }
    seg[n_records] = used;
    return 0;
}

// The hits of the batch's searches in (read, record rank, hit) order: M.d_merged, query <- read x records + rank
// room for `used` hits in (read, record, hit) order and for their byte offsets
static int merged_room(sx_ctx *ctx, MapBufs &M, const HitRoom &room, uint64_t used)
{
    if (used > M.merged_cap) {
        if (M.d_merged) M.own.drop(M.d_merged), M.own.drop(M.d_byte_off), M.own.drop(M.d_pos_off);
        M.d_pos_off = nullptr;
        M.merged_cap = used > room.cap ? used : room.cap;
        SX_TRY(M.own.take(ctx, &M.d_merged, (size_t)M.merged_cap));
        SX_TRY(M.own.take(ctx, &M.d_byte_off, (size_t)M.merged_cap + 1));
    }
    return 0;
}

static int merge_batch(sx_ctx *ctx, MapBufs &M, const HitRoom &room, const std::vector<uint64_t> &seg, uint32_t batch)
{
    const uint32_t n_records = (uint32_t)seg.size() - 1;
    const uint64_t used = seg[n_records];
    SX_TRY(merged_room(ctx, M, room, used));
    SX_CHECK(hipMemcpyAsync(M.d_seg, seg.data(), seg.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    SX_CHECK(hipStreamSynchronize(ctx->stream)); // (seg is reused by the next batch)
    const uint64_t nvq = (uint64_t)batch * n_records;
    sx_launch(ctx, SX_KC_SAM, nvq * 24, sam_vq_count_kernel, dim3(sx_div_up(nvq, kBlock)), dim3(kBlock), (const uint64_t *)M.d_ho, M.stride,
              batch, n_records, M.d_vbase);
    SX_TRY(device_scan64_inplace(ctx, M.d_vbase, nvq, SX_KC_SAM));
    sx_launch(ctx, SX_KC_SAM, used * 64, sam_merge_kernel, dim3(sx_div_up(used, kBlock)), dim3(kBlock), (const uint4 *)room.d_raw, used,
              (const uint64_t *)M.d_seg, n_records, (const uint64_t *)M.d_ho, M.stride, batch, (const uint64_t *)M.d_vbase,
              (uint4 *)M.d_merged, M.d_err);
    uint32_t e = 0;
    SX_TRY(sx_readback(ctx, M.d_err, 1, &e));
    if (e) return sx_fail_msg(ctx, SX_E_INTERNAL, "read mapping: the hits of a batch do not add up");
    return 0;
}

// The batch's text: its layout, then window after window through the two device windows and the context's staging
// buffers: emit and copy of window w are queued, then the sink works on window w - 1
static int emit_windows(sx_ctx *ctx, const SamArgs &A, const MapBufs &M, const sx_stage_events &E, sx_sink_fn sink, void *user)
{
    uint64_t total = 0;
    SX_TRY(sam_layout(ctx, A, M.d_byte_off, &total));
    const uint64_t window = M.window, n_win = (total + window - 1) / window;
    for (uint64_t w = 0; w <= n_win; ++w) {
        if (w < n_win) {
            const uint64_t lo = w * window, hi = total - lo < window ? total : lo + window;
            SX_TRY(sam_emit(ctx, A, M.d_byte_off, lo, hi, M.d_win[w & 1]));
            SX_CHECK(hipMemcpyAsync(ctx->h_stage[w & 1], M.d_win[w & 1], (size_t)(hi - lo), hipMemcpyDeviceToHost, ctx->stream));
            SX_CHECK(hipEventRecord(E.ev[w & 1], ctx->stream));
        }
        if (w > 0) {
            const uint64_t lo = (w - 1) * window, hi = total - lo < window ? total : lo + window;
            SX_CHECK(hipEventSynchronize(E.ev[(w - 1) & 1]));
            if (sink(user, SX_SECTION_SAM, ctx->h_stage[(w - 1) & 1], (size_t)(hi - lo)) != 0) {
                (void)hipStreamSynchronize(ctx->stream);
                return sx_fail_msg(ctx, SX_E_ARG, "the sink refused a chunk");
            }
        }
    }
    return sx_sync(ctx);
}

// The text of a batch against an index with a sampled suffix array: its hits are taken in runs of consecutive hits whose
// lines fit the cap (SX_FLAG_LOCATE_CHUNK_ROWS; a hit is never split: one with more lines gets a buffer of its own length);
// a run is located, laid out and emitted through its windows before the next one starts
static int emit_located(sx_ctx *ctx, const sx_index *idx, sx_sam_batch text, const uint16_t *d_read_flags, MapBufs &M, const sx_stage_events &E,
                        sx_sink_fn sink, void *user)
{
    const LocRec *d_recs = (const LocRec *)idx->d_loc_list;
    const uint64_t n_hits = text.n_hits, cap = ctx->locate_chunk_rows > 0 ? (uint64_t)ctx->locate_chunk_rows : 1ull << 28;
    const uint4 *d_hits = (const uint4 *)text.d_hits;
    if (!M.d_pos_off) SX_TRY(M.own.take(ctx, &M.d_pos_off, (size_t)M.merged_cap + 1));
    uint64_t total = 0;
    SX_TRY(sx_sa_hits_offsets(ctx, d_recs, text.n_records, (uint64_t)text.n_reads * text.n_records, d_hits, n_hits, M.d_pos_off, &total));
    uint32_t *d_loc_err = M.d_err + 4, *d_run = M.d_err + 8;
    for (uint64_t h_lo = 0, base = 0; h_lo < n_hits;) {
        uint64_t h_hi = n_hits, rows = total - base;
        if (rows > cap) SX_TRY(sx_sa_hits_run(ctx, M.d_pos_off, n_hits, h_lo, base, cap, d_run, &h_hi, &rows));
        if (rows > M.pos_cap) {
            if (M.d_positions) M.own.drop(M.d_positions);
            M.d_positions = nullptr, M.pos_cap = 0;
            SX_TRY(M.own.take(ctx, &M.d_positions, (size_t)rows));
            M.pos_cap = rows;
        }
        if (!M.d_positions) SX_TRY(M.own.take(ctx, &M.d_positions, 1)); // (hits without a line: the kernels still want an address)
        SX_TRY(sx_sa_locate_hits(ctx, d_recs, text.n_records, idx->packed, d_hits, M.d_pos_off, h_lo, h_hi, base, rows, M.d_positions, d_loc_err));
        uint32_t e = 0;
        SX_TRY(sx_readback(ctx, d_loc_err, 1, &e));
        if (e) return sx_fail_msg(ctx, SX_E_INTERNAL, "read mapping: a walk over a sampled suffix array met its bound");
        sx_sam_batch run = text;
        run.d_hits = text.d_hits + h_lo, run.n_hits = h_hi - h_lo;
        SamArgs A = sam_args_of(run);
        A.positions = M.d_positions, A.pos_off = M.d_pos_off + h_lo, A.pos_base = base;
        A.flags = d_read_flags;
        SX_TRY(emit_windows(ctx, A, M, E, sink, user));
        base += rows;
        h_lo = h_hi;
    }
    return 0;
}

} // namespace sx

using namespace sx;

extern "C" {

int sx_sam_layout_dev_ex(sx_ctx *ctx, const sx_sam_batch_ex *batch, uint64_t *d_byte_offsets, uint64_t *total_bytes_out)
{
    SamArgs A;
    SX_TRY(sam_args_ex(ctx, batch, A));
    if (!d_byte_offsets || !total_bytes_out) return SX_E_ARG;
    SX_CHECK(hipSetDevice(ctx->device));
    return sam_layout(ctx, A, d_byte_offsets, total_bytes_out);
}

int sx_sam_emit_dev_ex(sx_ctx *ctx, const sx_sam_batch_ex *batch, const uint64_t *d_byte_offsets, uint64_t total_bytes, uint64_t byte_lo,
                       uint64_t byte_hi, uint8_t *d_out)
{
    SamArgs A;
    SX_TRY(sam_args_ex(ctx, batch, A));
    if (!d_byte_offsets || byte_lo > byte_hi || byte_hi > total_bytes || (A.n_hits == 0 && byte_hi > byte_lo) || (byte_hi > byte_lo && (!d_out || ((uintptr_t)d_out & 15))))
        return sx_fail_msg(ctx, SX_E_ARG, "SAM text: a window inside [0, total) and a 16-byte aligned buffer are needed");
    SX_CHECK(hipSetDevice(ctx->device));
    SX_TRY(sam_emit(ctx, A, d_byte_offsets, byte_lo, byte_hi, d_out));
    return sx_sync(ctx);
}

int sx_sam_layout_dev(sx_ctx *ctx, const sx_sam_batch *batch, uint64_t *d_byte_offsets, uint64_t *total_bytes_out)
{
    if (!batch) return SX_E_ARG;
    const sx_sam_batch_ex ex = {*batch, nullptr};
    return sx_sam_layout_dev_ex(ctx, &ex, d_byte_offsets, total_bytes_out);
}

int sx_sam_emit_dev(sx_ctx *ctx, const sx_sam_batch *batch, const uint64_t *d_byte_offsets, uint64_t total_bytes, uint64_t byte_lo,
                    uint64_t byte_hi, uint8_t *d_out)
{
    if (!batch) return SX_E_ARG;
    const sx_sam_batch_ex ex = {*batch, nullptr};
    return sx_sam_emit_dev_ex(ctx, &ex, d_byte_offsets, total_bytes, byte_lo, byte_hi, d_out);
}

int sx_map_reads_limit(uint64_t n_reads, uint64_t n_records, uint32_t flags)
{
    if (flags & ~sx_map_known_flags) return SX_E_ARG;
    const uint64_t strands = (flags & SX_MAP_BOTH_STRANDS) ? 2 : 1;
    // (no product is formed before it is known to fit)
    if (n_reads > 0xFFFFFFFFull / strands) return SX_E_ARG;
    if (n_records && n_reads * strands > 0xFFFFFFFFull / n_records) return SX_E_ARG;
    return 0;
}

int sx_map_reads_stream(sx_ctx *ctx, const sx_map_record *records, uint32_t n_records, const uint8_t *fastq, size_t fastq_len,
                        int edits, sx_sink_fn sink, void *user)
{
    return sx_map_reads_stream_ex(ctx, records, n_records, fastq, fastq_len, edits, 0, sink, user);
}

int sx_map_reads_stream_ex(sx_ctx *ctx, const sx_map_record *records, uint32_t n_records, const uint8_t *fastq, size_t fastq_len,
                           int edits, uint32_t flags, sx_sink_fn sink, void *user)
{
    if (!ctx || !sink || (n_records && !records) || (fastq_len && !fastq)) return SX_E_ARG;
    if (edits < 0 || edits > SX_APPROX_MAX_EDITS)
        return sx_fail_msg(ctx, SX_E_ARG, "read mapping: edits must be in [0, 8]");
    if (flags & ~sx_map_known_flags) return sx_fail_msg(ctx, SX_E_ARG, "read mapping: unknown flags");
    sx_fastq fq;
    const int frc = sx_fastq_index(fastq, fastq_len, &fq);
    if (frc != 0) return sx_fail_msg(ctx, frc, "read mapping: malformed FASTQ image (see sx_fastq_index)");
    struct FqFree {
        sx_fastq *f;
        ~FqFree() { sx_fastq_free(f); }
    } fq_free{&fq};
    if (fq.count == 0 || n_records == 0) return 0;
    bool records_ok = true;
    for (uint32_t r = 0; r < n_records; ++r) records_ok = records_ok && sx_map_record_check(records[r], 2);
    SX_TRY(map_check(ctx, fq.count, n_records, flags, records_ok));
    SX_CHECK(hipSetDevice(ctx->device));
    // the reads of this call, then a temporary index of the host tables (every record's suffix array and tables:
    // N x (4 + 8 sigma) bytes a record with its RO table), the loop, and the index goes again
    const uint32_t n_reads = fq.count;
    sx_dev_scope B;
    sx_reads_dev reads;
    reads.count = n_reads;
    SX_TRY(upload(ctx, B, &reads.d_names, fq.names, fq.name_off[n_reads]));
    SX_TRY(upload(ctx, B, &reads.d_seqs, fq.seqs, fq.seq_off[n_reads]));
    SX_TRY(upload(ctx, B, &reads.d_quals, fq.quals, fq.qual_off[n_reads]));
    SX_TRY(upload(ctx, B, &reads.d_name_off, fq.name_off, (size_t)n_reads + 1));
    SX_TRY(upload(ctx, B, &reads.d_seq_off, fq.seq_off, (size_t)n_reads + 1));
    SX_TRY(upload(ctx, B, &reads.d_qual_off, fq.qual_off, (size_t)n_reads + 1));
    reads.h_seq_off = fq.seq_off;
    reads.name_bytes = fq.name_off[n_reads], reads.seq_bytes = fq.seq_off[n_reads], reads.qual_bytes = fq.qual_off[n_reads];
    sx_index *idx = nullptr;
    SX_TRY(sx_index_from_tables(ctx, records, n_records, &idx));
    const int rc = sx_map_reads_core(ctx, idx, reads, edits, flags, sink, user);
    sx_index_destroy(idx);
    return rc;
}

} // extern "C"

// The mapper's loop (bwt_readmapper.c:130-160, 257-266) over reads and tables that lie on the device: what
// sx_map_reads_stream and sx_index_map_reads share.  A batch: search (on capacity: grow_or_halve, again), merge, emit.
// d_read_flags: a FLAG per read, or null.
// group: 0, or (SX_MAP_BEST_STRATUM) the reads that share a stratum: 1, or 2 for the strands of a read;
// the searches of a batch are then the rounds of sx_best.hip and its hits are put in order by their place step.
static int map_reads_loop(sx_ctx *ctx, const sx_index *idx, const sx_reads_dev &reads, const uint16_t *d_read_flags, int edits, uint32_t group,
                          sx_sink_fn sink, void *user);

// Both strands: the read set of 2 x count reads, read 2q + strand, is made once and searched like any
// read set, so its hits come in (read, strand, record, hit) order, which is the text's; the FLAGs go with the batches.
int sx_map_reads_core(sx_ctx *ctx, const sx_index *idx, const sx_reads_dev &reads, int edits, uint32_t flags, sx_sink_fn sink, void *user)
{
    const uint32_t n_records = (uint32_t)idx->recs.size();
    if (reads.count == 0 || n_records == 0) return 0;
    bool records_ok = true;
    for (const sx_index_rec &R : idx->recs) records_ok = records_ok && sx_map_dims_ok(R.N, R.sigma, 2);
    SX_TRY(map_check(ctx, reads.count, n_records, flags, records_ok));
    const bool best = (flags & SX_MAP_BEST_STRATUM) != 0;
    if (!(flags & SX_MAP_BOTH_STRANDS)) return map_reads_loop(ctx, idx, reads, nullptr, edits, best ? 1u : 0u, sink, user);
    SX_CHECK(hipSetDevice(ctx->device));
    sx_fastq_dev in = {}, both = {};
    in.count = reads.count;
    in.d_names = (uint8_t *)reads.d_names, in.d_seqs = (uint8_t *)reads.d_seqs, in.d_quals = (uint8_t *)reads.d_quals;
    in.d_name_off = (uint32_t *)reads.d_name_off, in.d_seq_off = (uint32_t *)reads.d_seq_off, in.d_qual_off = (uint32_t *)reads.d_qual_off;
    in.name_bytes = reads.name_bytes, in.seq_bytes = reads.seq_bytes, in.qual_bytes = reads.qual_bytes;
    sx_dev_scope F;
    uint16_t *d_flags;
    SX_TRY(F.take(ctx, &d_flags, 2 * (size_t)reads.count));
    SX_TRY(sx_fastq_strands_dev(ctx, &in, &both, d_flags)); // (syncs: the callers' uploads from pageable memory are done)
    sx_reads_dev stranded;
    stranded.count = both.count;
    stranded.d_names = both.d_names, stranded.d_seqs = both.d_seqs, stranded.d_quals = both.d_quals;
    stranded.d_name_off = both.d_name_off, stranded.d_seq_off = both.d_seq_off, stranded.d_qual_off = both.d_qual_off;
    stranded.name_bytes = both.name_bytes, stranded.seq_bytes = both.seq_bytes, stranded.qual_bytes = both.qual_bytes;
    const int rc = map_reads_loop(ctx, idx, stranded, d_flags, edits, best ? 2u : 0u, sink, user);
    sx_fastq_dev_free(&both);
    return rc;
}

void sx_sam_remap(sx_ctx *ctx, const uint8_t *d_seqs, const uint8_t *d_table, uint8_t *d_out, uint64_t lo, uint64_t hi)
{
    if (hi > lo) sx_launch(ctx, SX_KC_REMAP, 2 * (hi - lo), sam_remap_kernel, dim3(sx_div_up(hi - lo, kBlock)), dim3(kBlock), d_seqs, d_table, d_out, lo, hi);
}

// The best-stratum searches of reads q0 .. q0 + batch (whole groups): the rounds into the room, then the hits in (read, record,
// hit) order in M.d_merged.  SX_E_CAPACITY: as search_batch
static int best_batch(sx_ctx *ctx, const sx_index *idx, const sx_reads_dev &reads, MapBufs &M, const HitRoom &room, sx_best_state &S, uint32_t q0,
                      uint32_t batch, int edits, uint32_t group, uint64_t *used_out)
{
    sx_best_batch B = {};
    B.recs = idx->recs.data(), B.n_rec = (uint32_t)idx->recs.size(), B.d_tabs = idx->d_tabs, B.d_pat = M.d_pat;
    B.d_bytes = reads.d_seqs, B.bytes_total = reads.seq_bytes, B.d_off = reads.d_seq_off + q0;
    SX_TRY(batch_bytes(ctx, reads, q0, batch, &B.p_lo, &B.p_hi));
    B.count = batch, B.gsize = group, B.k = edits;
    B.d_ho = M.d_ho, B.ho_stride = M.stride, B.d_stratum = S.d_stratum;
    B.d_raw = room.d_raw, B.raw_cap = room.cap, B.go_on_counting = false;
    SX_TRY(sx_best_rounds(ctx, S, B, used_out));
    if (*used_out == 0) return 0;
    SX_TRY(merged_room(ctx, M, room, *used_out));
    return sx_best_place(ctx, S, B, *used_out, M.d_vbase, M.d_merged);
}

static int map_reads_loop(sx_ctx *ctx, const sx_index *idx, const sx_reads_dev &reads, const uint16_t *d_read_flags, int edits, uint32_t group,
                          sx_sink_fn sink, void *user)
{
    const uint32_t n_reads = reads.count, n_records = (uint32_t)idx->recs.size();
    SX_CHECK(hipSetDevice(ctx->device));
    MapBufs M;
    SX_TRY(M.own.take(ctx, &M.d_pat, (size_t)reads.seq_bytes));
    SX_TRY(sx_sync(ctx)); // (the callers' uploads from pageable memory are done)

    uint32_t batch_max = ctx->sam_batch_reads > 0 ? (uint32_t)ctx->sam_batch_reads : (1u << 20);
    if (group == 2) batch_max += batch_max & 1u; // (a batch holds whole groups: both strands of a read; n_reads is even)
    if (batch_max > n_reads) batch_max = n_reads;
    M.window = ctx->sam_window_bytes > 0 ? ((size_t)ctx->sam_window_bytes + 15) & ~(size_t)15 : (size_t)SX_SAM_WINDOW_BYTES;
    if (M.window > sx_stage_bytes) M.window = sx_stage_bytes;
    SX_TRY(sx_stage_ensure(ctx));
    sx_stage_events E;
    for (uint8_t *&w : M.d_win) SX_TRY(M.own.take(ctx, &w, M.window));
    SX_TRY(E.create(ctx));
    M.stride = (uint64_t)batch_max + 1;
    SX_TRY(M.own.take(ctx, &M.d_ho, (size_t)M.stride * n_records));
    SX_TRY(M.own.take(ctx, &M.d_vbase, (size_t)batch_max * n_records + 1));
    SX_TRY(M.own.take(ctx, &M.d_seg, (size_t)n_records + 1));
    SX_TRY(M.own.take(ctx, &M.d_err, 64));
    SX_CHECK(hipMemsetAsync(M.d_err, 0, 256, ctx->stream));
    HitRoom room;
    SX_TRY(room.init(ctx, (uint64_t)batch_max * n_records * 4));
    std::vector<uint64_t> seg(n_records + 1);
    sx_best_state S;
    if (group) SX_TRY(S.init(ctx, batch_max, reads.seq_bytes, n_records, edits, true));
    sx_sam_batch text = {}; // the batch whose text is emitted: what is the same for every batch here
    text.d_sa_list = idx->d_sa_list, text.d_sa_len_list = idx->d_sa_lens;
    text.d_names = reads.d_names, text.d_seqs = reads.d_seqs, text.d_quals = reads.d_quals;
    text.d_rnames = idx->d_rnames, text.d_rname_off = idx->d_rname_off, text.n_records = n_records;

    uint32_t q0 = 0, batch = batch_max;
    while (q0 < n_reads) {
        if (batch > n_reads - q0) batch = n_reads - q0;
        uint64_t need = 0, used = 0;
        const int rc = group ? best_batch(ctx, idx, reads, M, room, S, q0, batch, edits, group, &used)
                             : search_batch(ctx, idx, reads, M, room, q0, batch, edits, seg, &need);
        if (rc == SX_E_CAPACITY) {
            bool halve;
            if (group) { // (a group alone gets whatever it needs; a batch of groups is halved to whole groups)
                SX_TRY(room.grow_or_halve(ctx, used, batch / group, &halve));
                if (halve) batch_max = batch = (batch / group + 1) / 2 * group;
                continue;
            }
            SX_TRY(room.grow_or_halve(ctx, need, batch, &halve));
            if (halve) batch_max = batch = (batch + 1) / 2; // (it is not tried longer again)
            continue;
        }
        if (rc != 0) return rc;
        if (!group) used = seg[n_records];
        if (used) {
            if (!group) SX_TRY(merge_batch(ctx, M, room, seg, batch));
            text.d_hits = M.d_merged, text.n_hits = used;
            text.d_name_off = reads.d_name_off + q0, text.d_seq_off = reads.d_seq_off + q0, text.d_qual_off = reads.d_qual_off + q0;
            text.n_reads = batch;
            // (the offsets are this batch's: so are the flags)
            const uint16_t *d_batch_flags = d_read_flags ? d_read_flags + q0 : nullptr;
            if (idx->sa_log2) {
                SX_TRY(emit_located(ctx, idx, text, d_batch_flags, M, E, sink, user));
            } else {
                SamArgs A = sam_args_of(text);
                A.flags = d_batch_flags;
                SX_TRY(emit_windows(ctx, A, M, E, sink, user));
            }
        }
        q0 += batch;
    }
    return sx_sync(ctx);
}
