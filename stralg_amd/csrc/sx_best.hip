// sx_best.hip -- best-stratum search: for every pattern the hits of the k-edit search at the smallest
// edit count that has any, by iterative deepening around the search's two passes (sx_approx.hip).
//
// A batch runs rounds d = 0 .. k over a shrinking set of groups (a group: one pattern, or the two strands of a read):
//  * count: per record, the round's patterns are remapped and the count pass runs at max_edits = d;
//  * verdict: a lane a group sums the round's counts over the group's patterns and all records; a group with hits has its
//    stratum, d, and leaves the set (two keep-masks: found this round, still open);
//  * select: the found patterns and the open ones are compacted, each into a flat set of its own.  The open set is the
//    next round's input; the emit pass runs over the found set only, once a record, at hit offsets that are a scan of the
//    found patterns' counts -- it walks a pattern's whole search tree again, and the patterns that found nothing at d are
//    the ones whose trees are largest;
//  * place, after the last round: the hits lie in the room as segments (round, record) with the pattern's number inside its
//    round's found set as their query; a count per (pattern, record) from the pattern's own round, a 64-bit scan, and a
//    lane a hit moves the hit to its place in (pattern, record, hit) order -- sam_merge_kernel with one more level.
// Where a byte or a hit goes is fixed by scans alone (no atomics beside the error word), so the output is the same from
// run to run.
#include "sx_common.hpp"
#include "sx_device.hpp"
#include "sx_scan.hpp"
#include "sx_hostio.hpp"
#include "sx_index.hpp"

namespace sx {

constexpr uint32_t kSelPer = 16, kSelTile = kBlock * kSelPer; // bytes a lane, bytes a workgroup
constexpr uint32_t kMaxRounds = SX_APPROX_MAX_EDITS + 1;

// ---- select ---------------------------------------------------------------------------------------------------------------
struct InKeep {
    const uint8_t *keep;
    __device__ __forceinline__ uint32_t operator()(uint64_t q) const { return keep[q] != 0 ? 1u : 0u; }
};
// rel[rank] <- q for the kept q
struct OutKeptIds {
    uint32_t *rel;
    __device__ __forceinline__ void operator()(uint64_t q, uint32_t excl, uint32_t v) const
    {
        if (v) rel[excl] = (uint32_t)q;
    }
};
// the length of kept pattern j (offsets that descend: 0)
struct InKeptLen {
    const uint32_t *off, *rel;
    __device__ __forceinline__ uint32_t operator()(uint64_t j) const
    {
        const uint32_t q = rel[j], b = off[q], e = off[q + 1];
        return e > b ? e - b : 0u;
    }
};
// off_out[j] <- the bytes in front of kept pattern j; ids_out[j] <- its number in the set that ids_in numbers (null: rel)
struct OutKeptOff {
    uint32_t *off_out, *ids_out;
    const uint32_t *rel, *ids_in;
    __device__ __forceinline__ void operator()(uint64_t j, uint32_t excl, uint32_t) const
    {
        off_out[j] = excl;
        if (ids_out) ids_out[j] = ids_in ? ids_in[rel[j]] : rel[j];
    }
};

struct SelectArgs {
    const uint8_t *src;
    const uint32_t *src_off, *rel, *out_off; // src_off: the input set's; rel: kept j -> its number there; out_off: kept + 1 entries
    uint8_t *out;
    uint32_t src_bytes; // src is read below this
    uint32_t kept, total; // total = out_off[kept], read back by the host: the grid and every store rest on it
};

// the last j in [lo, hi] with off[j] <= at (off[lo] <= at)
__device__ __forceinline__ uint32_t select_pattern_of(const uint32_t *__restrict__ off, uint32_t lo, uint32_t hi, uint32_t at)
{
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1u) / 2u;
        if (off[mid] <= at) lo = mid;
        else hi = mid - 1u;
    }
    return lo;
}

// The bytes of the kept patterns, moved as fq_strand_bytes_kernel moves a read set's: the work is cut
// by output bytes, a workgroup makes a tile of 4096 of them, a lane 16 in one store; the workgroup finds the patterns at its
// tile's ends by a search in the output offsets, a lane the pattern of its first byte by a search between them.  The last
// store of the array may run up to 15 bytes beyond it, into its 16 spare bytes, and writes zeros there.
__global__ __launch_bounds__(kBlock) void best_select_bytes_kernel(SelectArgs A)
{
    const uint32_t t = threadIdx.x;
    const uint64_t tile0 = (uint64_t)blockIdx.x * kSelTile;
    if (tile0 >= A.total) return; // (the whole workgroup)
    const uint32_t tile_last = A.total - tile0 < kSelTile ? A.total - 1u : (uint32_t)tile0 + kSelTile - 1u;
    const uint32_t p0 = select_pattern_of(A.out_off, 0u, A.kept - 1u, (uint32_t)tile0), p1 = select_pattern_of(A.out_off, p0, A.kept - 1u, tile_last);
    const uint64_t j0 = tile0 + (uint64_t)t * kSelPer;
    if (j0 >= A.total) return;
    uint32_t q = select_pattern_of(A.out_off, p0, p1, (uint32_t)j0);
    uint32_t b = A.out_off[q], e = A.out_off[q + 1], s = A.src_off[A.rel[q]];
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t k = 0; k < kSelPer; ++k) {
        const uint64_t j = j0 + k;
        if (j >= A.total) break; // (the bytes behind the array's end are zeros: they lie in its 16 spare bytes)
        while (j >= e && q + 1u < A.kept) { // (the next pattern; more than one step only over patterns without a byte)
            ++q;
            b = e;
            e = A.out_off[q + 1];
            s = A.src_off[A.rel[q]];
        }
        const uint64_t at = (uint64_t)s + (j - b); // (offsets that do not ascend: some byte of the source, or 0)
        uint32_t c = 0;
        if (j >= b && j < e && at < A.src_bytes) c = A.src[at];
        w[k >> 2] |= c << (8u * (k & 3u));
    }
    const uint4 v = {w[0], w[1], w[2], w[3]};
    *reinterpret_cast<uint4 *>(A.out + j0) = v;
}

// ---- verdict ---------------------------------------------------------------------------------------------------------------
// One lane a group of the round's set: its hits at d over its patterns and all records (ho: n_rec arrays of stride entries,
// the count passes' hit offsets).  ids: the set's patterns' numbers in the batch (null: the set is the batch)
__global__ __launch_bounds__(kBlock) void best_verdict_kernel(const uint64_t *ho, uint64_t stride, uint32_t n_rec, uint32_t groups, uint32_t gsize,
                                                              const uint32_t *ids, uint32_t d, uint8_t *stratum, uint8_t *keep_found,
                                                              uint8_t *keep_open)
{
    const uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= groups) return;
    const uint64_t p = g * gsize;
    uint64_t sum = 0;
    for (uint32_t r = 0; r < n_rec; ++r) sum += ho[r * stride + p + gsize] - ho[r * stride + p];
    const bool found = sum != 0;
    for (uint32_t s = 0; s < gsize; ++s) {
        keep_found[p + s] = found ? 1 : 0;
        keep_open[p + s] = found ? 0 : 1;
    }
    if (found) stratum[(ids ? ids[p] : (uint32_t)p) / gsize] = (uint8_t)d;
}

// ---- the found set's hit offsets: a scan of its patterns' counts, gathered from the count pass ---------------------------------
struct InFoundCount {
    const uint64_t *ho;
    const uint32_t *rel;
    __device__ __forceinline__ uint32_t operator()(uint64_t j) const
    {
        const uint32_t q = rel[j];
        return (uint32_t)(ho[q + 1] - ho[q]); // (a call has fewer than 2^32 hits)
    }
};
struct OutFoundOff {
    uint64_t *p;
    uint64_t n;
    __device__ __forceinline__ void operator()(uint64_t j, uint32_t excl, uint32_t v) const
    {
        p[j] = excl;
        if (j + 1 == n) p[n] = (uint64_t)excl + v;
    }
};

// ---- place ----------------------------------------------------------------------------------------------------------------
struct PlaceArgs {
    uint32_t fbase[kMaxRounds + 1]; // round d's found patterns: entries [fbase[d], fbase[d + 1]) of ids
    uint32_t rounds, n_rec, count;
    const uint32_t *ids;  // found pattern -> its number in the batch
    const uint64_t *fho;  // found-set hit offsets: (record r, round d, j) at fho[r * fstride + fbase[d] + d + j]
    uint64_t fstride;
};

// the round of found entry jj
__device__ __forceinline__ uint32_t place_round_of(const PlaceArgs &A, uint32_t jj)
{
    uint32_t d = 0;
    for (uint32_t s = 1; s < A.rounds; ++s)
        if (A.fbase[s] <= jj) d = s;
    return d;
}

// cnt[pattern * n_rec + r] <- the hits of a found pattern in record r, from its own round (the others keep their 0)
__global__ __launch_bounds__(kBlock) void best_vq_count_kernel(PlaceArgs A, uint64_t *cnt, uint32_t *err)
{
    const uint64_t idx = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint32_t found = A.fbase[A.rounds];
    if (idx >= (uint64_t)found * A.n_rec) return;
    const uint32_t jj = (uint32_t)(idx / A.n_rec), r = (uint32_t)(idx - (uint64_t)jj * A.n_rec);
    const uint32_t d = place_round_of(A, jj), j = jj - A.fbase[d], q = A.ids[jj];
    if (q >= A.count) {
        atomicOr(err, 2u);
        return;
    }
    const uint64_t *f = A.fho + r * A.fstride + A.fbase[d] + d;
    cnt[(uint64_t)q * A.n_rec + r] = f[j + 1] - f[j];
}

// Hit h of the room (segment (d, r) at seg[d * n_rec + r] .. seg[d * n_rec + r + 1]) goes behind the hits of its pattern in
// the records before r: query <- pattern * n_rec + r (sam_merge_kernel, with the rounds as one more level of segments;
// n_dst: dst's entries, the hits and SX_MAP_UNMAPPED's placeholders)
__global__ __launch_bounds__(kBlock) void best_place_kernel(PlaceArgs A, const uint4 *src, uint64_t n_hits, const uint64_t *seg, const uint64_t *vbase,
                                                            uint4 *dst, uint64_t n_dst, uint32_t *err)
{
    const uint64_t h = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (h >= n_hits) return;
    uint32_t s = 0;
    {
        uint32_t b = A.rounds * A.n_rec; // seg[s] <= h < seg[b]
        while (b - s > 1) {
            const uint32_t mid = (s + b) / 2;
            if (seg[mid] <= h) s = mid;
            else b = mid;
        }
    }
    const uint32_t d = s / A.n_rec, r = s - d * A.n_rec;
    uint4 h0 = src[2 * h];
    const uint32_t j = h0.x;
    if (j >= A.fbase[d + 1] - A.fbase[d]) {
        atomicOr(err, 2u);
        return;
    }
    const uint32_t q = A.ids[A.fbase[d] + j];
    if (q >= A.count) {
        atomicOr(err, 2u);
        return;
    }
    const uint64_t *f = A.fho + r * A.fstride + A.fbase[d] + d;
    const uint64_t at = vbase[(uint64_t)q * A.n_rec + r] + (h - seg[s] - f[j]);
    if (at >= n_dst) {
        atomicOr(err, 2u);
        return;
    }
    h0.x = q * A.n_rec + r;
    dst[2 * at] = h0;
    dst[2 * at + 1] = src[2 * h + 1];
}

// The kept patterns of a set: ids and offsets by two scans, then the bytes.  d_rel (count entries): the kept patterns' numbers
// in the input set; d_ids_out (optional): their numbers in the set that d_ids_in numbers (null: d_rel's).  d_scal: two words.
// src_bytes: d_bytes is read below it; out_max: the bytes d_bytes_out holds before its 16 spare ones
static int patterns_select(sx_ctx *ctx, const uint8_t *d_bytes, uint64_t src_bytes, const uint32_t *d_off, uint32_t count, const uint8_t *d_keep,
                           const uint32_t *d_ids_in, uint32_t *d_rel, uint8_t *d_bytes_out, uint64_t out_max, uint32_t *d_off_out,
                           uint32_t *d_ids_out, uint32_t *d_scal, uint32_t *count_out, uint64_t *bytes_out)
{
    uint32_t kept = 0, total = 0;
    SX_TRY((device_scan<OpAdd>(ctx, count, InKeep{d_keep}, OutKeptIds{d_rel}, d_scal, SX_KC_REMAP, (uint64_t)count * 6)));
    SX_TRY(sx_readback(ctx, d_scal, 1, &kept));
    if (kept > count) return sx_fail_msg(ctx, SX_E_INTERNAL, "pattern select: more patterns kept than there are");
    // (off_out[kept] <- the total: with no pattern kept the scan writes the 0 there itself)
    SX_TRY((device_scan<OpAdd>(ctx, kept, InKeptLen{d_off, d_rel}, OutKeptOff{d_off_out, d_ids_out, d_rel, d_ids_in}, d_off_out + kept, SX_KC_REMAP,
                               (uint64_t)kept * 20)));
    SX_TRY(sx_readback(ctx, d_off_out + kept, 1, &total));
    *count_out = kept, *bytes_out = total;
    if (total > out_max) return sx_fail_msg(ctx, SX_E_ARG, "pattern select: the offsets do not ascend");
    SX_CHECK(hipMemsetAsync(d_bytes_out + total, 0, 16, ctx->stream));
    if (total) {
        const SelectArgs A = {d_bytes, d_off, d_rel, d_off_out, d_bytes_out, (uint32_t)(src_bytes > 0xFFFFFFFFull ? 0xFFFFFFFFull : src_bytes), kept, total};
        sx_launch(ctx, SX_KC_REMAP, 2ull * total, best_select_bytes_kernel, dim3(sx_div_up(total, kSelTile)), dim3(kBlock), A);
    }
    return 0;
}

} // namespace sx

using namespace sx;

int sx_best_state::init(sx_ctx *ctx, uint32_t count_max, uint64_t bytes_max, uint32_t n_records, int max_edits, bool own_stratum)
{
    cap_count = count_max, cap_bytes = bytes_max, n_rec = n_records, rounds = (uint32_t)max_edits + 1u;
    fstride = (uint64_t)count_max + rounds + 1;
    const size_t c = count_max;
    if (own_stratum) SX_TRY(own.take(ctx, &d_stratum, c));
    SX_TRY(own.take(ctx, &d_keep_found, c));
    SX_TRY(own.take(ctx, &d_keep_open, c));
    for (int s = 0; s < 2; ++s) {
        SX_TRY(own.take(ctx, &d_open[s], (size_t)bytes_max + 16));
        SX_TRY(own.take(ctx, &d_open_off[s], c + 1));
        SX_TRY(own.take(ctx, &d_open_ids[s], c));
    }
    // the found sets of the rounds lie one behind the other: each has its 16 spare bytes and offsets of its own
    SX_TRY(own.take(ctx, &d_found, (size_t)bytes_max + 32 * (size_t)rounds));
    SX_TRY(own.take(ctx, &d_found_off, c + rounds));
    SX_TRY(own.take(ctx, &d_found_ids, c));
    SX_TRY(own.take(ctx, &d_rel_found, c));
    SX_TRY(own.take(ctx, &d_rel_open, c));
    SX_TRY(own.take(ctx, &d_fho, (size_t)fstride * n_records));
    SX_TRY(own.take(ctx, &d_seg, (size_t)rounds * n_records + 1));
    SX_TRY(own.take(ctx, &d_err, 64));
    seg.assign((size_t)rounds * n_records + 1, 0);
    return 0;
}

int sx_best_rounds(sx_ctx *ctx, sx_best_state &S, const sx_best_batch &B, uint64_t *total_out)
{
    *total_out = 0;
    const uint32_t n_rec = B.n_rec, gsize = B.gsize, rounds = (uint32_t)B.k + 1u;
    if (B.count > S.cap_count || B.p_hi - B.p_lo > S.cap_bytes || n_rec != S.n_rec || rounds > S.rounds || gsize == 0 || B.count % gsize ||
        B.ho_stride < (uint64_t)B.count + 1)
        return sx_fail_msg(ctx, SX_E_INTERNAL, "best stratum: a batch beyond what its state was sized for");
    uint32_t *d_scal = S.d_err + 16;
    SX_CHECK(hipMemsetAsync(S.d_err, 0, 256, ctx->stream));
    SX_CHECK(hipMemsetAsync(B.d_stratum, 0xFF, B.count / gsize, ctx->stream));
    for (uint32_t d = 0; d <= kMaxRounds; ++d) S.fbase[d] = 0;
    std::fill(S.seg.begin(), S.seg.end(), 0);

    // the round's set: at first the batch itself, where it lies
    const uint8_t *cur = B.d_bytes;
    const uint32_t *cur_off = B.d_off, *cur_ids = nullptr;
    uint64_t cur_lo = B.p_lo, cur_hi = B.p_hi, cur_src_bytes = B.bytes_total;
    uint32_t cur_count = B.count;
    uint64_t used = 0, found_bytes_at = 0;
    bool emitting = B.d_raw != nullptr, over = false;
    for (uint32_t d = 0; d < rounds; ++d) {
        S.fbase[d + 1] = S.fbase[d];
        if (cur_count == 0) { // (the rounds that are left have nothing to search: their segments are empty)
            for (uint32_t r = 0; r < n_rec; ++r) S.seg[(size_t)d * n_rec + r] = used;
            continue;
        }
        // count
        uint64_t round_total = 0;
        std::vector<uint64_t> rec_total(n_rec, 0);
        for (uint32_t r = 0; r < n_rec; ++r) {
            const uint8_t *pat = cur;
            if (B.d_tabs) {
                sx_sam_remap(ctx, cur, B.d_tabs + (size_t)r * 256, B.d_pat, cur_lo, cur_hi);
                pat = B.d_pat;
            }
            SX_TRY(sx_approx_count_record(ctx, B.recs[r], pat, cur_off, cur_count, (int)d, B.d_ho + r * B.ho_stride, &rec_total[r], B.search_flags));
            round_total += rec_total[r];
        }
        if (used + round_total >= (1ull << 32)) return sx_fail_msg(ctx, SX_E_ARG, "approximate search: 2^32 hits or more in one call");
        if (emitting && used + round_total > B.raw_cap) {
            over = true;
            emitting = false;
            if (!B.go_on_counting) {
                *total_out = used + round_total;
                sx_fail_msg(ctx, SX_E_CAPACITY, "best stratum: more hits than the room holds");
                return SX_E_CAPACITY;
            }
        }
        // verdict
        sx_launch(ctx, SX_KC_SEARCH, (uint64_t)cur_count * (8 * n_rec + 2), best_verdict_kernel, dim3(sx_div_up(cur_count / gsize, kBlock)), dim3(kBlock),
                  (const uint64_t *)B.d_ho, B.ho_stride, n_rec, cur_count / gsize, gsize, cur_ids, d, B.d_stratum, S.d_keep_found, S.d_keep_open);
        // select: the found set (for the emit pass and the place step), the open one (the next round's)
        uint32_t n_found = 0;
        uint64_t found_bytes = 0;
        uint8_t *f_bytes = S.d_found + found_bytes_at;
        uint32_t *f_off = S.d_found_off + S.fbase[d] + d, *f_ids = S.d_found_ids + S.fbase[d];
        if (round_total) {
            SX_TRY(patterns_select(ctx, cur, cur_src_bytes, cur_off, cur_count, S.d_keep_found, cur_ids, S.d_rel_found, f_bytes, cur_hi - cur_lo, f_off,
                                   f_ids, d_scal, &n_found, &found_bytes));
            S.fbase[d + 1] = S.fbase[d] + n_found;
            found_bytes_at += (found_bytes + 31) & ~(uint64_t)15;
        }
        for (uint32_t r = 0; r < n_rec; ++r) {
            S.seg[(size_t)d * n_rec + r] = used;
            if (n_found == 0) continue;
            uint64_t *fho = S.d_fho + r * S.fstride + S.fbase[d] + d;
            SX_TRY((device_scan<OpAdd>(ctx, n_found, InFoundCount{B.d_ho + r * B.ho_stride, S.d_rel_found}, OutFoundOff{fho, n_found}, nullptr,
                                       SX_KC_SEARCH, (uint64_t)n_found * 28)));
            if (emitting && rec_total[r]) {
                const uint8_t *pat = f_bytes;
                if (B.d_tabs) {
                    sx_sam_remap(ctx, f_bytes, B.d_tabs + (size_t)r * 256, B.d_pat, 0, found_bytes);
                    pat = B.d_pat;
                }
                SX_TRY(sx_approx_emit_record(ctx, B.recs[r], pat, f_off, n_found, (int)d, fho, B.d_raw + used, rec_total[r], B.search_flags));
            }
            used += rec_total[r];
        }
        if (d + 1 < rounds) {
            const uint32_t s = d & 1u;
            uint32_t n_open = 0;
            uint64_t open_bytes = 0;
            SX_TRY(patterns_select(ctx, cur, cur_src_bytes, cur_off, cur_count, S.d_keep_open, cur_ids, S.d_rel_open, S.d_open[s], cur_hi - cur_lo,
                                   S.d_open_off[s], S.d_open_ids[s], d_scal, &n_open, &open_bytes));
            cur = S.d_open[s], cur_off = S.d_open_off[s], cur_ids = S.d_open_ids[s];
            cur_lo = 0, cur_hi = open_bytes, cur_src_bytes = open_bytes, cur_count = n_open;
        }
    }
    S.seg[(size_t)rounds * n_rec] = used;
    *total_out = used;
    SX_TRY(sx_sync(ctx));
    if (over) {
        sx_fail_msg(ctx, SX_E_CAPACITY, "best stratum: more hits than the room holds");
        return SX_E_CAPACITY;
    }
    return 0;
}

int sx_best_place(sx_ctx *ctx, sx_best_state &S, const sx_best_batch &B, uint64_t total, uint64_t *d_vbase, sx_approx_hit *d_placed, bool unmapped,
                  uint64_t *placed_out)
{
    const uint32_t n_rec = B.n_rec, rounds = (uint32_t)B.k + 1u;
    PlaceArgs A = {};
    for (uint32_t d = 0; d <= kMaxRounds; ++d) A.fbase[d] = S.fbase[d < rounds ? d : rounds];
    A.rounds = rounds, A.n_rec = n_rec, A.count = B.count;
    A.ids = S.d_found_ids, A.fho = S.d_fho, A.fstride = S.fstride;
    const uint64_t nvq = (uint64_t)B.count * n_rec, nf = (uint64_t)S.fbase[rounds] * n_rec;
    const uint32_t groups = unmapped && d_placed ? B.count / B.gsize : 0; // (SX_MAP_UNMAPPED: a placeholder a group without a hit)
    SX_CHECK(hipMemsetAsync(d_vbase, 0, (size_t)(nvq + 1) * 8, ctx->stream));
    if (nf) sx_launch(ctx, SX_KC_SAM, nf * 28, best_vq_count_kernel, dim3(sx_div_up(nf, kBlock)), dim3(kBlock), A, d_vbase, S.d_err);
    if (groups) sx_map_unmapped_count(ctx, d_vbase, groups, B.gsize, n_rec);
    SX_TRY(device_scan64_inplace(ctx, d_vbase, nvq, SX_KC_SAM));
    uint64_t placed = total;
    if (groups) {
        uint32_t w[2] = {0, 0};
        SX_TRY(sx_readback(ctx, (const uint32_t *)(d_vbase + nvq), 2, w));
        placed = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
        if (placed < total || placed > total + groups) return sx_fail_msg(ctx, SX_E_INTERNAL, "best stratum: the hits of a batch do not add up");
        sx_map_unmapped_place(ctx, d_vbase, groups, B.gsize, n_rec, d_placed, placed, S.d_err);
    }
    if (d_placed && total) {
        SX_CHECK(hipMemcpyAsync(S.d_seg, S.seg.data(), ((size_t)rounds * n_rec + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        sx_launch(ctx, SX_KC_SAM, total * 64, best_place_kernel, dim3(sx_div_up(total, kBlock)), dim3(kBlock), A, (const uint4 *)B.d_raw, total,
                  (const uint64_t *)S.d_seg, (const uint64_t *)d_vbase, (uint4 *)d_placed, placed, S.d_err);
    }
    uint32_t e = 0;
    SX_TRY(sx_readback(ctx, S.d_err, 1, &e)); // (syncs: seg is the next batch's again)
    if (e) return sx_fail_msg(ctx, SX_E_INTERNAL, "best stratum: the hits of a batch do not add up");
    if (placed_out) *placed_out = placed;
    return 0;
}

extern "C" {

int sx_patterns_select_dev(sx_ctx *ctx, const uint8_t *d_bytes, const uint32_t *d_off, uint32_t count, const uint8_t *d_keep, uint8_t *d_bytes_out,
                           uint32_t *d_off_out, uint32_t *d_ids_out, uint32_t *count_out, uint64_t *bytes_out)
{
    if (!ctx || !d_off || !d_bytes_out || ((uintptr_t)d_bytes_out & 15) || !d_off_out || !count_out || !bytes_out || (count && (!d_keep || !d_ids_out)))
        return SX_E_ARG;
    SX_CHECK(hipSetDevice(ctx->device));
    *count_out = 0, *bytes_out = 0;
    // the bounds of every access rest on the offsets' ends
    const uint32_t *ends[2] = {d_off, d_off + count};
    const uint32_t one[2] = {1, 1};
    uint32_t h[2] = {0, 0};
    SX_TRY(sx_readback_ranges(ctx, ends, one, 2, h));
    if (h[1] < h[0] || (h[1] && !d_bytes)) return sx_fail_msg(ctx, SX_E_ARG, "pattern select: the offsets do not ascend");
    SX_TRY(sx_slab_ensure(ctx, SX_SLAB_SORT, 4096));
    uint32_t *d_scal = (uint32_t *)ctx->slab[SX_SLAB_SORT].p;
    // (the kept patterns' numbers in the input are the ids asked for)
    SX_TRY(patterns_select(ctx, d_bytes, h[1], d_off, count, d_keep, nullptr, d_ids_out, d_bytes_out, h[1] - h[0], d_off_out, nullptr, d_scal, count_out,
                           bytes_out));
    return sx_sync(ctx);
}

int sx_bwt_best_search_dev(sx_ctx *ctx, const uint32_t *d_c_table, const uint32_t *d_o_table, const uint32_t *d_ro_table, uint64_t N, uint32_t sigma,
                           const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t count, int max_edits, uint8_t *d_stratum,
                           uint64_t *d_hit_offsets, sx_approx_hit *d_hits, uint64_t hit_capacity, uint64_t *total_hits_out)
{
    return sx_bwt_best_search_dev_ex(ctx, d_c_table, d_o_table, d_ro_table, N, sigma, d_patterns, d_offsets, count, max_edits, d_stratum, d_hit_offsets,
                                     d_hits, hit_capacity, total_hits_out, 0);
}

int sx_bwt_best_search_dev_ex(sx_ctx *ctx, const uint32_t *d_c_table, const uint32_t *d_o_table, const uint32_t *d_ro_table, uint64_t N, uint32_t sigma,
                              const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t count, int max_edits, uint8_t *d_stratum,
                              uint64_t *d_hit_offsets, sx_approx_hit *d_hits, uint64_t hit_capacity, uint64_t *total_hits_out,
                              uint32_t search_flags)
{
    if (search_flags & ~(uint32_t)SX_SEARCH_NO_INDELS) return SX_E_ARG;
    if (!ctx || !d_hit_offsets || !total_hits_out || ((uintptr_t)d_hits & 15) || (count && !d_stratum)) return SX_E_ARG;
    if (!d_c_table || !d_o_table || !d_offsets || N == 0 || N > 0xFFFFFFFFull || sigma < 2 || sigma > 256 || max_edits > SX_APPROX_MAX_EDITS)
        return SX_E_ARG;
    SX_CHECK(hipSetDevice(ctx->device));
    *total_hits_out = 0;
    if (max_edits < 0 || count == 0) { // no search: every offset 0, every stratum 0xFF
        SX_CHECK(hipMemsetAsync(d_hit_offsets, 0, ((size_t)count + 1) * sizeof(uint64_t), ctx->stream));
        if (count) SX_CHECK(hipMemsetAsync(d_stratum, 0xFF, count, ctx->stream));
        return sx_sync(ctx);
    }
    const uint32_t *ends[2] = {d_offsets, d_offsets + count};
    const uint32_t one[2] = {1, 1};
    uint32_t h[2] = {0, 0};
    SX_TRY(sx_readback_ranges(ctx, ends, one, 2, h));
    if (h[1] < h[0]) return sx_fail_msg(ctx, SX_E_ARG, "best stratum: the patterns' offsets do not ascend");
    sx_index_rec R; // the mapper's round loop with one record, no symbol table and groups of one
    R.N = N, R.sigma = sigma;
    R.d_c = (uint32_t *)d_c_table, R.d_o = (uint32_t *)d_o_table, R.d_ro = (uint32_t *)d_ro_table;
    sx_best_state S;
    SX_TRY(sx_nomem_of(S.init(ctx, count, h[1] - h[0], 1, max_edits, false)));
    sx_dev_scope T;
    sx_best_batch B = {};
    B.recs = &R, B.n_rec = 1, B.d_bytes = d_patterns, B.bytes_total = h[1], B.d_off = d_offsets, B.p_lo = h[0], B.p_hi = h[1];
    B.count = count, B.gsize = 1, B.k = max_edits, B.search_flags = search_flags;
    SX_TRY(T.take(ctx, &B.d_ho, (size_t)count + 1));
    B.ho_stride = (uint64_t)count + 1, B.d_stratum = d_stratum;
    // the rounds leave their hits in the caller's array; the place step orders them through the M slab
    B.d_raw = d_hits, B.raw_cap = hit_capacity, B.go_on_counting = true;
    uint64_t total = 0;
    const int rc = sx_best_rounds(ctx, S, B, &total);
    if (rc != 0 && rc != SX_E_CAPACITY) return rc;
    *total_hits_out = total;
    sx_approx_hit *d_placed = nullptr;
    if (rc == 0 && d_hits && total) {
        SX_TRY(sx_slab_ensure(ctx, SX_SLAB_M, total * sizeof(sx_approx_hit)));
        d_placed = (sx_approx_hit *)ctx->slab[SX_SLAB_M].p;
    }
    SX_TRY(sx_best_place(ctx, S, B, total, d_hit_offsets, d_placed));
    if (d_placed) SX_CHECK(hipMemcpyAsync(d_hits, d_placed, total * sizeof(sx_approx_hit), hipMemcpyDeviceToDevice, ctx->stream));
    SX_TRY(sx_sync(ctx));
    if (rc == SX_E_CAPACITY) sx_fail_msg(ctx, SX_E_CAPACITY, "best stratum: more hits than hit_capacity");
    return rc;
}

} // extern "C"
