// sx_sam.hip -- SAM text of k-edit search hits on the device, and the read mapper's loop around it
// (tools/readmappers/bwt_readmapper/bwt_readmapper.c map_read + bioinf/sam.c print_sam_line).
//
// One hit (sx_approx_hit) is an interval of a suffix array; it prints R - L lines
//     <qname>\t0\t<rname>\t<sa[i]+1>\t0\t<cigar>\t*\t0\t0\t<seq>\t<qual>\n          i = L .. R-1
// that differ in the position's digits only.  Two steps ("SAM text"):
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
#include "sx_index.hpp"

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
constexpr size_t kStageBytes = (size_t)32 << 20; // the context's pinned staging buffers (sx_build.hip: stream_out)

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
};

struct HitInfo {
    const uint32_t *pos; // the hit's positions: pos[0 .. cnt)
    uint32_t cnt, fixed, cig_len, m;
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
__device__ __forceinline__ bool hit_info(const SamArgs &A, uint64_t h, HitInfo &I)
{
    const uint4 h0 = A.hits[2 * h];
    I.gaps = A.hits[2 * h + 1];
    I.cnt = 0;
    I.fixed = 0;
    I.cig_len = 0;
    I.pos = nullptr;
    const uint32_t vq = h0.x, L = h0.y, R = h0.z;
    if ((uint64_t)vq >= (uint64_t)A.n_reads * A.n_records || L > R) return false;
    const uint32_t read = vq / A.n_records, rec = vq - read * A.n_records;
    const uint32_t *sa = A.sa_list ? A.sa_list[rec] : A.sa;
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
    I.pos = sa + L;
    I.cnt = R - L;
    return true;
}

// "\t0\t" + "\t" + "\t0\t" + "\t*\t0\t0\t" + "\t" + "\n": the 16 bytes of a line beside its fields and digits
__device__ __forceinline__ uint32_t fixed_bytes(const HitInfo &I)
{
    return I.name_l + I.rn_l + I.cig_len + I.seq_l + I.qual_l + 16u;
}

// exclusive sum over the workgroup's 256 lanes, 64-bit with carries; ends with a barrier (lds: kWavesPerBlock words)
__device__ __forceinline__ uint64_t block_exclusive_sum_u64(uint64_t v, uint64_t *lds, uint64_t &total)
{
    const int lane = lane_id(), w = wave_id();
    unsigned long long inc = v;
    for (unsigned d = 1; d < (unsigned)kWave; d <<= 1) {
        const unsigned long long up = __shfl_up(inc, d, kWave);
        if (lane >= (int)d) inc += up;
    }
    if (lane == kWave - 1) lds[w] = inc;
    __syncthreads();
    uint64_t base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < kWavesPerBlock; ++i) {
        const uint64_t x = lds[i];
        if (i < w) base += x;
        tot += x;
    }
    __syncthreads();
    total = tot;
    return base + inc - v;
}

// ---- layout: bytes per hit ---------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void sam_size_kernel(SamArgs A, uint64_t *len_out, uint32_t *err)
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
        if (!hit_info(A, h, I)) {
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

// ---- 64-bit exclusive scan in place: d[0 .. n) -> prefixes, d[n] <- total -------------------------
constexpr int kScan64Items = 8;
constexpr int kScan64Tile = kBlock * kScan64Items;

__global__ __launch_bounds__(kBlock) void scan64_reduce_kernel(const uint64_t *d, uint64_t n, uint64_t *tile_tot)
{
    __shared__ uint64_t red[kWavesPerBlock];
    const uint64_t base = (uint64_t)blockIdx.x * kScan64Tile + (uint64_t)threadIdx.x * kScan64Items;
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < kScan64Items; ++k)
        if (base + k < n) acc += d[base + k];
    uint64_t tot;
    (void)block_exclusive_sum_u64(acc, red, tot);
    if (threadIdx.x == 0) tile_tot[blockIdx.x] = tot;
}

__global__ __launch_bounds__(kBlock) void scan64_spine_kernel(uint64_t *tile_tot, uint32_t ntiles, uint64_t *total_out)
{
    __shared__ uint64_t red[kWavesPerBlock];
    uint64_t carry = 0;
    for (uint64_t start = 0; start < ntiles; start += kBlock) { // uniform trip count
        const uint64_t i = start + threadIdx.x;
        const uint64_t v = i < ntiles ? tile_tot[i] : 0;
        uint64_t tot;
        const uint64_t ex = block_exclusive_sum_u64(v, red, tot);
        if (i < ntiles) tile_tot[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) *total_out = carry;
}

__global__ __launch_bounds__(kBlock) void scan64_apply_kernel(uint64_t *d, uint64_t n, const uint64_t *tile_pre)
{
    __shared__ uint64_t red[kWavesPerBlock];
    const uint64_t base = (uint64_t)blockIdx.x * kScan64Tile + (uint64_t)threadIdx.x * kScan64Items;
    uint64_t v[kScan64Items];
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < kScan64Items; ++k) {
        v[k] = base + k < n ? d[base + k] : 0;
        acc += v[k];
    }
    uint64_t tot;
    uint64_t run = tile_pre[blockIdx.x] + block_exclusive_sum_u64(acc, red, tot);
#pragma unroll
    for (int k = 0; k < kScan64Items; ++k) {
        if (base + k < n) d[base + k] = run;
        run += v[k];
    }
}

static int scan64_inplace(sx_ctx *ctx, uint64_t *d, uint64_t n)
{
    if (n == 0) {
        SX_CHECK(hipMemsetAsync(d, 0, sizeof(uint64_t), ctx->stream));
        return 0;
    }
    const uint32_t ntiles = sx_div_up(n, kScan64Tile);
    uint64_t *tile_tot = (uint64_t *)sx_scan_scratch(ctx, 2 * ntiles + 2);
    if (!tile_tot) return sx_fail_msg(ctx, SX_E_NOMEM, "scan scratch");
    sx_launch(ctx, SX_KC_SAM, n * 8, scan64_reduce_kernel, dim3(ntiles), dim3(kBlock), (const uint64_t *)d, n, tile_tot);
    sx_launch(ctx, SX_KC_SAM, 0, scan64_spine_kernel, dim3(1), dim3(kBlock), tile_tot, ntiles, d + n);
    sx_launch(ctx, SX_KC_SAM, n * 16, scan64_apply_kernel, dim3(ntiles), dim3(kBlock), d, n, (const uint64_t *)tile_tot);
    return 0;
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

__global__ __launch_bounds__(kBlock) void sam_emit_kernel(SamArgs A, const uint64_t *byte_off, uint64_t lo, uint64_t hi,
                                                          uint8_t *out)
{
    __shared__ uint4 obuf4[kSlice / 16];
    __shared__ uint8_t cig[kBlock * kCigarMax];
    __shared__ HitLds hl[kBlock];
    __shared__ uint32_t mo[kBlock + 1];
    __shared__ uint64_t red[kWavesPerBlock];
    __shared__ uint32_t red32[kWavesPerBlock];
    __shared__ uint64_t nxt[2];
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
        if (hit_info(A, h, I)) {
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
        if (h + t < A.n_hits && hit_info(A, h + t, I)) c = I.cnt - (t == 0 ? (i < I.cnt ? i : I.cnt) : 0u);
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
            put_bytes(obuf, off, slice_len, (const uint8_t *)"\t0\t", 3);
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

static int sam_args(sx_ctx *ctx, const sx_sam_batch *b, SamArgs &A)
{
    if (!ctx || !b) return SX_E_ARG;
    if (b->n_hits && (!b->d_hits || ((uintptr_t)b->d_hits & 15) || !(b->d_sa || (b->d_sa_list && b->d_sa_len_list))))
        return sx_fail_msg(ctx, SX_E_ARG, "SAM text: hits (16-byte aligned) and a suffix array are needed");
    if (!b->d_name_off || !b->d_seq_off || !b->d_qual_off || !b->d_rname_off || b->n_records == 0 ||
        (uint64_t)b->n_reads * b->n_records > 0xFFFFFFFFull)
        return sx_fail_msg(ctx, SX_E_ARG, "SAM text: offsets of the reads and record names; reads x records below 2^32");
    A.hits = (const uint4 *)b->d_hits;
    A.n_hits = b->n_hits;
    A.sa = b->d_sa;
    A.sa_len = b->sa_len;
    A.sa_list = b->d_sa_list;
    A.sa_len_list = b->d_sa_len_list;
    A.names = b->d_names;
    A.seqs = b->d_seqs;
    A.quals = b->d_quals;
    A.name_off = b->d_name_off;
    A.seq_off = b->d_seq_off;
    A.qual_off = b->d_qual_off;
    A.n_reads = b->n_reads;
    A.rnames = b->d_rnames;
    A.rname_off = b->d_rname_off;
    A.n_records = b->n_records;
    return 0;
}

static int sam_layout(sx_ctx *ctx, const SamArgs &A, uint64_t *d_byte_off, uint64_t *total_out)
{
    *total_out = 0;
    SX_TRY(sx_slab_ensure(ctx, SX_SLAB_SORT, 4096));
    uint32_t *d_err = (uint32_t *)ctx->slab[SX_SLAB_SORT].p;
    SX_CHECK(hipMemsetAsync(d_err, 0, 16, ctx->stream));
    if (A.n_hits)
        sx_launch(ctx, SX_KC_SAM, A.n_hits * 40, sam_size_kernel, dim3(sx_div_up(A.n_hits, kBlock)), dim3(kBlock), A, d_byte_off,
                  d_err);
    SX_TRY(scan64_inplace(ctx, d_byte_off, A.n_hits));
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
    sx_launch(ctx, SX_KC_SAM, hi - lo, sam_emit_kernel, dim3((uint32_t)slices), dim3(kBlock), A, d_byte_off, lo, hi, d_out);
    return 0;
}

struct DevBufs { // device and pinned allocations of one sx_map_reads_stream call
    std::vector<void *> dev;
    hipEvent_t ev[2] = {nullptr, nullptr};
    ~DevBufs()
    {
        for (void *p : dev) (void)hipFree(p);
        for (int k = 0; k < 2; ++k)
            if (ev[k]) (void)hipEventDestroy(ev[k]);
    }
    template <class T> int take(sx_ctx *ctx, T **out, size_t count)
    {
        void *p = nullptr;
        const size_t bytes = (count * sizeof(T) + 255) & ~(size_t)255;
        if (hipMalloc(&p, bytes ? bytes : 256) != hipSuccess) return sx_fail_msg(ctx, SX_E_NOMEM, "read mapping: device memory");
        dev.push_back(p);
        *out = (T *)p;
        return 0;
    }
    void drop(void *p)
    {
        for (size_t k = 0; k < dev.size(); ++k)
            if (dev[k] == p) {
                (void)hipFree(p);
                dev.erase(dev.begin() + (long)k);
                return;
            }
    }
};

template <class T> static int upload(sx_ctx *ctx, DevBufs &B, T **d, const T *h, size_t count)
{
    SX_TRY(B.take(ctx, d, count + 16));
    if (count) SX_CHECK(hipMemcpyAsync(*d, h, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return 0;
}

} // namespace sx

using namespace sx;

extern "C" {

int sx_sam_layout_dev(sx_ctx *ctx, const sx_sam_batch *batch, uint64_t *d_byte_offsets, uint64_t *total_bytes_out)
{
    SamArgs A;
    SX_TRY(sam_args(ctx, batch, A));
    if (!d_byte_offsets || !total_bytes_out) return SX_E_ARG;
    SX_CHECK(hipSetDevice(ctx->device));
    return sam_layout(ctx, A, d_byte_offsets, total_bytes_out);
}

int sx_sam_emit_dev(sx_ctx *ctx, const sx_sam_batch *batch, const uint64_t *d_byte_offsets, uint64_t total_bytes, uint64_t byte_lo,
                    uint64_t byte_hi, uint8_t *d_out)
{
    SamArgs A;
    SX_TRY(sam_args(ctx, batch, A));
    if (!d_byte_offsets || byte_lo > byte_hi || byte_hi > total_bytes || (batch->n_hits == 0 && byte_hi > byte_lo) || (byte_hi > byte_lo && (!d_out || ((uintptr_t)d_out & 15))))
        return sx_fail_msg(ctx, SX_E_ARG, "SAM text: a window inside [0, total) and a 16-byte aligned buffer are needed");
    SX_CHECK(hipSetDevice(ctx->device));
    SX_TRY(sam_emit(ctx, A, d_byte_offsets, byte_lo, byte_hi, d_out));
    return sx_sync(ctx);
}

int sx_map_reads_stream(sx_ctx *ctx, const sx_map_record *records, uint32_t n_records, const uint8_t *fastq, size_t fastq_len,
                        int edits, sx_sink_fn sink, void *user)
{
    if (!ctx || !sink || (n_records && !records) || (fastq_len && !fastq)) return SX_E_ARG;
    if (edits < 0 || edits > SX_APPROX_MAX_EDITS)
        return sx_fail_msg(ctx, SX_E_ARG, "read mapping: edits must be in [0, 8]");
    sx_fastq fq;
    const int frc = sx_fastq_index(fastq, fastq_len, &fq);
    if (frc != 0) return sx_fail_msg(ctx, frc, "read mapping: malformed FASTQ image (see sx_fastq_index)");
    struct FqFree {
        sx_fastq *f;
        ~FqFree() { sx_fastq_free(f); }
    } fq_free{&fq};
    if (fq.count == 0 || n_records == 0) return 0;
    if ((uint64_t)fq.count * n_records > 0xFFFFFFFFull)
        return sx_fail_msg(ctx, SX_E_ARG, "read mapping: reads x records must stay below 2^32");
    for (uint32_t r = 0; r < n_records; ++r) {
        const sx_map_record &R = records[r];
        if (!R.name || !R.sa || !R.c_table || !R.o_table || !R.remap || R.N == 0 || R.N > 0xFFFFFFFFull || R.sigma < 2 || R.sigma > 128)
            return sx_fail_msg(ctx, SX_E_ARG, "read mapping: a record lacks its name, suffix array, tables or remap table");
    }
    SX_CHECK(hipSetDevice(ctx->device));
    const uint32_t n_reads = fq.count;
    DevBufs B;
    // the reads of this call, then a temporary index of the host tables (every record's suffix array and tables:
    // N x (4 + 8 sigma) bytes a record with its RO table), the loop, and the index goes again
    uint8_t *d_names, *d_seqs, *d_quals;
    uint32_t *d_name_off, *d_seq_off, *d_qual_off;
    SX_TRY(upload(ctx, B, &d_names, (const uint8_t *)fq.names, fq.name_off[n_reads]));
    SX_TRY(upload(ctx, B, &d_seqs, (const uint8_t *)fq.seqs, fq.seq_off[n_reads]));
    SX_TRY(upload(ctx, B, &d_quals, (const uint8_t *)fq.quals, fq.qual_off[n_reads]));
    SX_TRY(upload(ctx, B, &d_name_off, (const uint32_t *)fq.name_off, (size_t)n_reads + 1));
    SX_TRY(upload(ctx, B, &d_seq_off, (const uint32_t *)fq.seq_off, (size_t)n_reads + 1));
    SX_TRY(upload(ctx, B, &d_qual_off, (const uint32_t *)fq.qual_off, (size_t)n_reads + 1));
    sx_index *idx = nullptr;
    SX_TRY(sx_index_from_records_impl(ctx, records, n_records, &idx));
    struct IdxFree {
        sx_index *i;
        ~IdxFree() { sx_index_destroy(i); }
    } idx_free{idx};
    sx_reads_dev reads;
    reads.count = n_reads;
    reads.d_names = d_names, reads.d_seqs = d_seqs, reads.d_quals = d_quals;
    reads.d_name_off = d_name_off, reads.d_seq_off = d_seq_off, reads.d_qual_off = d_qual_off;
    reads.h_seq_off = fq.seq_off;
    reads.seq_bytes = fq.seq_off[n_reads];
    return sx_map_reads_core(ctx, idx, reads, edits, sink, user);
}

} // extern "C"

// The mapper's loop (bwt_readmapper.c:130-160, 257-266) over reads and tables that lie on the device: what
// sx_map_reads_stream and sx_index_map_reads share.
int sx_map_reads_core(sx_ctx *ctx, const sx_index *idx, const sx_reads_dev &reads, int edits, sx_sink_fn sink, void *user)
{
    const uint32_t n_reads = reads.count, n_records = (uint32_t)idx->recs.size();
    if (n_reads == 0 || n_records == 0) return 0;
    if ((uint64_t)n_reads * n_records > 0xFFFFFFFFull)
        return sx_fail_msg(ctx, SX_E_ARG, "read mapping: reads x records must stay below 2^32");
    for (const sx_index_rec &R : idx->recs)
        if (R.N == 0 || R.N > 0xFFFFFFFFull || R.sigma < 2 || R.sigma > 128)
            return sx_fail_msg(ctx, SX_E_ARG, "read mapping: a record lacks its name, suffix array, tables or remap table");
    SX_CHECK(hipSetDevice(ctx->device));
    DevBufs B;
    const uint8_t *d_names = reads.d_names, *d_seqs = reads.d_seqs, *d_quals = reads.d_quals, *d_rnames = idx->d_rnames,
                  *d_tabs = idx->d_tabs;
    const uint32_t *d_name_off = reads.d_name_off, *d_seq_off = reads.d_seq_off, *d_qual_off = reads.d_qual_off,
                   *d_rname_off = idx->d_rname_off;
    const uint32_t *const *d_sa_list = idx->d_sa_list;
    const uint64_t *d_sa_lens = idx->d_sa_lens;
    uint8_t *d_pat;
    SX_TRY(B.take(ctx, &d_pat, (size_t)reads.seq_bytes + 16));
    SX_TRY(sx_sync(ctx)); // (the callers' uploads from pageable memory are done)

    uint32_t batch_max = ctx->sam_batch_reads > 0 ? (uint32_t)ctx->sam_batch_reads : (1u << 20);
    if (batch_max > n_reads) batch_max = n_reads;
    size_t window = ctx->sam_window_bytes > 0 ? ((size_t)ctx->sam_window_bytes + 15) & ~(size_t)15 : (size_t)SX_SAM_WINDOW_BYTES;
    if (window > kStageBytes) window = kStageBytes;
    for (int b = 0; b < 2; ++b)
        if (!ctx->h_stage[b] && hipHostMalloc((void **)&ctx->h_stage[b], kStageBytes, hipHostMallocDefault) != hipSuccess) {
            ctx->h_stage[b] = nullptr;
            return sx_fail_msg(ctx, SX_E_NOMEM, "pinned staging buffers");
        }
    uint8_t *d_win[2];
    for (int b = 0; b < 2; ++b) {
        SX_TRY(B.take(ctx, &d_win[b], window));
        SX_CHECK(hipEventCreate(&B.ev[b]));
    }
    const uint64_t stride = (uint64_t)batch_max + 1;
    uint64_t *d_ho, *d_vbase, *d_seg, *d_byte_off = nullptr;
    uint32_t *d_err;
    SX_TRY(B.take(ctx, &d_ho, (size_t)stride * n_records));
    SX_TRY(B.take(ctx, &d_vbase, (size_t)batch_max * n_records + 1));
    SX_TRY(B.take(ctx, &d_seg, (size_t)n_records + 1));
    SX_TRY(B.take(ctx, &d_err, 64));
    SX_CHECK(hipMemsetAsync(d_err, 0, 256, ctx->stream));
    // room for hits: a guess to start with; a batch that needs more makes it grow, up to 2^27 hits or what a quarter of the
    // free memory holds (72 bytes a hit: the searches' array, the merged one, the byte offsets), before the batch is halved
    // -- a search over few reads leaves most of its lanes idle, so batches stay as long as memory allows
    uint64_t cap = (uint64_t)batch_max * n_records * 4, cap_max = 1ull << 26;
    {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b) {
            cap_max = free_b / 4 / 72;
            if (cap_max > (1ull << 27)) cap_max = 1ull << 27;
        } else {
            (void)hipGetLastError();
        }
        if (cap_max < (1u << 16)) cap_max = 1u << 16;
    }
    if (cap < (1u << 16)) cap = 1u << 16;
    if (cap > cap_max) cap = cap_max;
    sx_approx_hit *d_raw = nullptr, *d_merged = nullptr;
    uint64_t merged_cap = 0;
    SX_TRY(B.take(ctx, &d_raw, (size_t)cap));
    std::vector<uint64_t> seg(n_records + 1);

    uint32_t q0 = 0, batch = batch_max;
    while (q0 < n_reads) {
        if (batch > n_reads - q0) batch = n_reads - q0;
        // the searches, record after record, into one hit array; too many hits: half the reads, or (one read) more room
        uint64_t used = 0;
        bool again = false;
        uint64_t p_lo, p_hi;
        if (reads.h_seq_off) {
            p_lo = reads.h_seq_off[q0], p_hi = reads.h_seq_off[q0 + batch];
        } else { // (the offsets were made on the device: the two this batch needs come back)
            const uint32_t *src[2] = {d_seq_off + q0, d_seq_off + q0 + batch};
            const uint32_t one[2] = {1, 1};
            uint32_t got[2];
            SX_TRY(sx_readback_ranges(ctx, src, one, 2, got));
            p_lo = got[0], p_hi = got[1];
        }
        for (uint32_t r = 0; r < n_records && !again; ++r) {
            const sx_index_rec &R = idx->recs[r];
            if (p_hi > p_lo)
                sx_launch(ctx, SX_KC_REMAP, 2 * (p_hi - p_lo), sam_remap_kernel, dim3(sx_div_up(p_hi - p_lo, kBlock)), dim3(kBlock),
                          (const uint8_t *)d_seqs, (const uint8_t *)(d_tabs + (size_t)r * 256), d_pat, p_lo, p_hi);
            uint64_t tot = 0;
            const int rc = sx_bwt_approx_search_dev(ctx, R.d_c, R.d_o, R.d_ro, R.N, R.sigma, d_pat, d_seq_off + q0, batch, edits,
                                                    d_ho + r * stride, d_raw + used, cap - used, &tot);
            if (rc == SX_E_CAPACITY) {
                const uint64_t need = used + tot;
                if (need <= cap_max || batch == 1) { // more room (one read alone gets whatever it needs)
                    cap = need + need / 4 > 2 * cap ? need + need / 4 : 2 * cap;
                    if (cap > cap_max && need <= cap_max) cap = cap_max;
                    B.drop(d_raw);
                    SX_TRY(B.take(ctx, &d_raw, (size_t)cap));
                } else {
                    batch = (batch + 1) / 2;
                    batch_max = batch; // (it is not tried longer again)
                }
                again = true;
                break;
            }
            if (rc != 0) return rc;
            seg[r] = used;
            used += tot;
        }
        if (again) continue;
        seg[n_records] = used;
        if (used) {
            if (used > merged_cap) {
                if (d_merged) B.drop(d_merged), B.drop(d_byte_off);
                merged_cap = used > cap ? used : cap;
                SX_TRY(B.take(ctx, &d_merged, (size_t)merged_cap));
                SX_TRY(B.take(ctx, &d_byte_off, (size_t)merged_cap + 1));
            }
            SX_CHECK(hipMemcpyAsync(d_seg, seg.data(), seg.size() * 8, hipMemcpyHostToDevice, ctx->stream));
            SX_CHECK(hipStreamSynchronize(ctx->stream)); // (seg is reused by the next batch)
            const uint64_t nvq = (uint64_t)batch * n_records;
            sx_launch(ctx, SX_KC_SAM, nvq * 24, sam_vq_count_kernel, dim3(sx_div_up(nvq, kBlock)), dim3(kBlock), (const uint64_t *)d_ho,
                      stride, batch, n_records, d_vbase);
            SX_TRY(scan64_inplace(ctx, d_vbase, nvq));
            sx_launch(ctx, SX_KC_SAM, used * 64, sam_merge_kernel, dim3(sx_div_up(used, kBlock)), dim3(kBlock), (const uint4 *)d_raw, used,
                      (const uint64_t *)d_seg, n_records, (const uint64_t *)d_ho, stride, batch, (const uint64_t *)d_vbase,
                      (uint4 *)d_merged, d_err);
            uint32_t e = 0;
            SX_TRY(sx_readback(ctx, d_err, 1, &e));
            if (e) return sx_fail_msg(ctx, SX_E_INTERNAL, "read mapping: the hits of a batch do not add up");
            SamArgs A{};
            A.hits = (const uint4 *)d_merged;
            A.n_hits = used;
            A.sa_list = d_sa_list;
            A.sa_len_list = d_sa_lens;
            A.names = d_names, A.seqs = d_seqs, A.quals = d_quals;
            A.name_off = d_name_off + q0, A.seq_off = d_seq_off + q0, A.qual_off = d_qual_off + q0;
            A.n_reads = batch;
            A.rnames = d_rnames;
            A.rname_off = d_rname_off;
            A.n_records = n_records;
            uint64_t total = 0;
            SX_TRY(sam_layout(ctx, A, d_byte_off, &total));
            // windows: emit and copy of window w are queued, then the sink works on window w - 1
            const uint64_t n_win = (total + window - 1) / window;
            for (uint64_t w = 0; w <= n_win; ++w) {
                if (w < n_win) {
                    const uint64_t lo = w * window, hi = total - lo < window ? total : lo + window;
                    SX_TRY(sam_emit(ctx, A, d_byte_off, lo, hi, d_win[w & 1]));
                    SX_CHECK(hipMemcpyAsync(ctx->h_stage[w & 1], d_win[w & 1], (size_t)(hi - lo), hipMemcpyDeviceToHost, ctx->stream));
                    SX_CHECK(hipEventRecord(B.ev[w & 1], ctx->stream));
                }
                if (w > 0) {
                    const uint64_t lo = (w - 1) * window, hi = total - lo < window ? total : lo + window;
                    SX_CHECK(hipEventSynchronize(B.ev[(w - 1) & 1]));
                    if (sink(user, SX_SECTION_SAM, ctx->h_stage[(w - 1) & 1], (size_t)(hi - lo)) != 0) {
                        (void)hipStreamSynchronize(ctx->stream);
                        return sx_fail_msg(ctx, SX_E_ARG, "the sink refused a chunk");
                    }
                }
            }
            SX_TRY(sx_sync(ctx));
        }
        q0 += batch;
    }
    return sx_sync(ctx);
}
