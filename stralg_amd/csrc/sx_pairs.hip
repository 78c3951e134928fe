// sx_pairs.hip -- the join of paired reads: from a batch's merged hits to two line descriptors
// (sx_pair_line) a proper combination, in the text's order.
//
// The hits of a batch of whole pairs stand in (read, record, hit) order, read 4p + 2m + s being strand s of mate m + 1 of
// pair p; a hit prints R - L lines.  A line a of (mate 1, strand s, record r) can only be proper with the lines b of (mate 2,
// strand 1 - s, record r): one run of consecutive lines of the batch.  Four steps:
//  * lines: R - L of every hit, scanned: the lines in front of every hit, and per line its position, its span and its hit
//    (a line's hit by a search in the scanned counts);
//  * count: one lane a line a, grid over all lines of the batch, so every lane of a wave works whatever the pairs' sizes (a
//    7 600 x 7 600 pair fills thirty workgroups, a million pairs of one line each fill the same lanes); the lane walks its run
//    of b -- the lanes of a wave that share a run read the same 8 bytes, one fetch for all of them -- and counts the proper
//    ones in a register; a line of a second mate counts 0;
//  * a 64-bit scan of the counts: the combinations in front of every line's;
//  * fill: the same walk; combination (a, b) goes to the scanned count of a plus the proper b in front of b, a number the lane
//    counts as it walks.  Nothing is placed by an atomic: a descriptor's slot is a function of (pair, a, b) alone.
// All per-lane state is a handful of registers; no LDS, no scratch.
#include "sx_common.hpp"
#include "sx_device.hpp"
#include "sx_scan.hpp"
#include "sx_pairs.hpp"

namespace sx {

// ---- the lines of a batch ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void pair_hit_lines_kernel(PairJoin J, uint64_t *cnt, uint32_t *err)
{
    const uint64_t h = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (h >= J.n_hits) return;
    const uint4 h0 = J.hits[2 * h];
    const uint32_t vq = h0.x, L = h0.y, R = h0.z;
    uint64_t c = 0;
    if ((uint64_t)vq >= (uint64_t)J.n_reads * J.n_records || L > R || (uint64_t)R > J.sa_len_list[vq % J.n_records]) atomicOr(err, 1u);
    else c = R - L;
    cnt[h] = c;
}

__global__ __launch_bounds__(kBlock) void pair_line_expand_kernel(PairJoin J, PairLines P)
{
    const uint64_t l = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (l >= P.n_lines) return;
    uint64_t h = 0;
    { // the last h with line_off[h] <= l (line_off[n_hits] = n_lines > l)
        uint64_t b = J.n_hits;
        while (b - h > 1) {
            const uint64_t mid = h + (b - h) / 2;
            if (P.line_off[mid] <= l) h = mid;
            else b = mid;
        }
    }
    const uint4 h0 = J.hits[2 * h];
    const uint32_t pos = J.positions ? J.positions[l] : J.sa_list[h0.x % J.n_records][h0.y + (l - P.line_off[h])];
    const uint2 v = {pos, h0.w & 0xFFFFu};
    P.ps[l] = v;
    P.hit[l] = (uint32_t)h;
}

// ---- count and fill ------------------------------------------------------------------------------------------------------
// (a, b) with a on strand s of mate 1 and b on strand 1 - s of mate 2 of the same pair and record: is it proper, and its t
__device__ __forceinline__ bool pair_proper(uint32_t s, uint2 a, uint2 b, uint32_t lo, uint32_t hi, uint64_t &t)
{
    const uint2 f = s ? b : a, r = s ? a : b; // the FLAG 0 line and the FLAG 16 line
    const uint64_t f_end = (uint64_t)f.x + f.y, r_end = (uint64_t)r.x + r.y;
    t = r_end - f.x;
    return f.x <= r.x && f_end <= r_end && t >= lo && t <= hi;
}

template <bool kFill> __global__ __launch_bounds__(kBlock) void pair_join_kernel(PairJoin J, PairLines P, uint64_t *cnt, const uint64_t *base, sx_pair_line *out)
{
    const uint64_t l = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (l >= P.n_lines) return;
    const uint32_t ha = P.hit[l], vq = J.hits[2 * (uint64_t)ha].x;
    const uint32_t read = vq / J.n_records, rec = vq - read * J.n_records;
    uint64_t b_lo = 0, b_hi = 0;
    const uint32_t s = read & 1u;
    if (!(read & 2u)) { // a line of mate 1: its partners are the lines of (mate 2, the other strand, this record)
        const uint64_t pvq = (uint64_t)((read & ~3u) + 2u + (1u - s)) * J.n_records + rec;
        const uint64_t h_lo = J.vbase[pvq], h_hi = J.vbase[pvq + 1];
        if (h_lo <= h_hi && h_hi <= J.n_hits) b_lo = P.line_off[h_lo], b_hi = P.line_off[h_hi];
    }
    const uint2 a = P.ps[l];
    uint64_t n = 0, at = kFill ? base[l] : 0;
    for (uint64_t b = b_lo; b < b_hi; ++b) {
        const uint2 pb = P.ps[b];
        uint64_t t;
        if (!pair_proper(s, a, pb, J.min_insert, J.max_insert, t)) continue;
        if (kFill) {
            const int32_t tl = (int32_t)(uint32_t)t; // (max_insert < 2^31)
            out[2 * (at + n)] = sx_pair_line{ha, a.x + 1u, pb.x + 1u, s ? -tl : tl, 1u + 2u + 64u + (s ? 16u : 32u)};
            out[2 * (at + n) + 1] = sx_pair_line{P.hit[b], pb.x + 1u, a.x + 1u, s ? tl : -tl, 1u + 2u + 128u + (s ? 32u : 16u)};
        }
        ++n;
    }
    if (!kFill) cnt[l] = n;
}

int pair_lines_count(sx_ctx *ctx, const PairJoin &J, PairLines &L)
{
    L.n_lines = 0;
    SX_TRY(sx_slab_ensure(ctx, SX_SLAB_SORT, 4096));
    uint32_t *d_err = (uint32_t *)ctx->slab[SX_SLAB_SORT].p;
    SX_CHECK(hipMemsetAsync(d_err, 0, 16, ctx->stream));
    if (J.n_hits)
        sx_launch(ctx, SX_KC_PAIR_COUNT, J.n_hits * 24, pair_hit_lines_kernel, dim3(sx_div_up(J.n_hits, kBlock)), dim3(kBlock), J, L.line_off, d_err);
    SX_TRY(device_scan64_inplace(ctx, L.line_off, J.n_hits, SX_KC_PAIR_SCAN));
    uint32_t h[2] = {0, 0}, e = 0;
    SX_TRY(sx_readback(ctx, (const uint32_t *)(L.line_off + J.n_hits), 2, h));
    SX_TRY(sx_readback(ctx, d_err, 1, &e));
    if (e) return sx_fail_msg(ctx, SX_E_INTERNAL, "paired reads: a hit's query or interval lies outside its batch or record");
    L.n_lines = (uint64_t)h[0] | ((uint64_t)h[1] << 32);
    return 0;
}

int pair_lines_expand(sx_ctx *ctx, const PairJoin &J, const PairLines &L)
{
    if (L.n_lines) // (a position in, 12 bytes out, the search in the scanned counts)
        sx_launch(ctx, SX_KC_PAIR_COUNT, L.n_lines * 24, pair_line_expand_kernel, dim3(sx_div_up(L.n_lines, kBlock)), dim3(kBlock), J, L);
    return 0;
}

int pair_count(sx_ctx *ctx, const PairJoin &J, const PairLines &L, uint64_t *d_cnt, uint64_t *combos_out)
{
    *combos_out = 0;
    if (L.n_lines)
        sx_launch(ctx, SX_KC_PAIR_COUNT, L.n_lines * 24, pair_join_kernel<false>, dim3(sx_div_up(L.n_lines, kBlock)), dim3(kBlock), J, L, d_cnt,
                  (const uint64_t *)nullptr, (sx_pair_line *)nullptr);
    SX_TRY(device_scan64_inplace(ctx, d_cnt, L.n_lines, SX_KC_PAIR_SCAN));
    uint32_t h[2] = {0, 0};
    SX_TRY(sx_readback(ctx, (const uint32_t *)(d_cnt + L.n_lines), 2, h));
    *combos_out = (uint64_t)h[0] | ((uint64_t)h[1] << 32);
    return 0;
}

int pair_fill(sx_ctx *ctx, const PairJoin &J, const PairLines &L, const uint64_t *d_cnt, sx_pair_line *d_out)
{
    if (L.n_lines)
        sx_launch(ctx, SX_KC_PAIR_FILL, L.n_lines * 24, pair_join_kernel<true>, dim3(sx_div_up(L.n_lines, kBlock)), dim3(kBlock), J, L,
                  (uint64_t *)nullptr, d_cnt, d_out);
    return 0;
}

} // namespace sx
