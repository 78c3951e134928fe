// sx_locate.hip -- the sampled suffix array of a compact index (sx_locate.hpp): its marks and
// values from a suffix array, and suffix array entries from them by walks over the BWT blocks.
//
// Sample, over blocks of 64 rows (a wave a block, a lane a row):
//   1. the ballot of "SA[row] is a multiple of s" is the block's bits word,
//   2. a scan of the words' popcounts (sx_scan.hpp) gives every block its `before`,
//   3. a marked row stores its SA value at before + its rank in the ballot.
// A suffix array on the host comes up in windows of whole blocks; the same passes run a window, the samples in front of
// the window carried over.  Where a value goes is a function of the scan alone (no atomics): the same array gives the
// same bytes.
// Locate: a lane takes an output slot and walks from its row to a marked one; output is placed by slot only.
#include "sx_common.hpp"
#include "sx_device.hpp"
#include "sx_hostio.hpp"
#include "sx_index.hpp"
#include "sx_locate.hpp"
#include "sx_scan.hpp"

namespace sx {

// ---- sample ----------------------------------------------------------------------------------------------------------
// pass 1: the bits of blocks [b0, b0 + nb); win holds SA[64 b0 .. min(64 (b0 + nb), N))
__global__ __launch_bounds__(kBlock) void sa_mark_kernel(const uint32_t *__restrict__ win, uint64_t N, uint32_t smask, uint64_t b0, uint32_t nb,
                                                         uint4 *__restrict__ marks)
{
    const uint32_t k = blockIdx.x * kWavesPerBlock + (uint32_t)wave_id(), lane = (uint32_t)lane_id();
    if (k >= nb) return; // (the whole wave)
    const uint64_t rel = (uint64_t)k * kOccRows + lane, i = (b0 + k) * kOccRows + lane;
    const bool marked = i < N && (win[rel] & smask) == 0u;
    const uint64_t bits = __ballot(marked ? 1 : 0);
    if (lane == 0) marks[b0 + k] = uint4{(uint32_t)bits, (uint32_t)(bits >> 32), 0u, 0u};
}

struct InMarkCount {
    const uint4 *marks; // (from the window's first block on)
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const
    {
        const uint4 m = marks[i];
        return (uint32_t)__popc(m.x) + (uint32_t)__popc(m.y);
    }
};
struct OutMarkBefore {
    uint4 *marks;
    uint32_t base; // the samples in front of the window
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t excl, uint32_t) const { marks[i].z = base + excl; }
};

// pass 3: the values of the marked rows of the same blocks
__global__ __launch_bounds__(kBlock) void sa_values_kernel(const uint32_t *__restrict__ win, uint64_t b0, uint32_t nb, const uint4 *__restrict__ marks,
                                                           uint32_t *__restrict__ values, uint32_t n_samples)
{
    const uint32_t k = blockIdx.x * kWavesPerBlock + (uint32_t)wave_id(), lane = (uint32_t)lane_id();
    if (k >= nb) return;
    const uint4 m = marks[b0 + k];
    const uint64_t bits = (uint64_t)m.x | ((uint64_t)m.y << 32);
    if ((bits >> lane) & 1ull) {
        const uint32_t at = m.z + (uint32_t)__popcll(bits & lanemask_lt());
        if (at < n_samples) values[at] = win[(uint64_t)k * kOccRows + lane]; // (more multiples of s than a suffix array has: the caller refuses)
    }
}

// ---- locate ----------------------------------------------------------------------------------------------------------
enum { LOC_ERR_BOUND = 1 };

// the accessor of a record's blocks in the form of the launch
template <class Occ> __device__ __forceinline__ Occ loc_occ(const LocRec &T);
template <> __device__ __forceinline__ OccCompact loc_occ<OccCompact>(const LocRec &T) { return OccCompact{T.occ, T.stride}; }
template <> __device__ __forceinline__ OccPacked loc_occ<OccPacked>(const LocRec &T) { return OccPacked{T.occ}; }

template <class Occ> __device__ __forceinline__ uint32_t locate_row(const LocRec &T, uint32_t row, uint32_t *err)
{
    const Occ occ = loc_occ<Occ>(T);
    uint32_t steps = 0;
    bool bad = row >= T.N;
    while (!bad) {
        const uint32_t b = row / kOccRows, j = row % kOccRows;
        const uint4 m = T.marks[b]; // the block's mark entry: one load
        const uint64_t bits = (uint64_t)m.x | ((uint64_t)m.y << 32);
        if ((bits >> j) & 1ull) {
            const uint32_t at = m.z + (uint32_t)__popcll(bits & ((1ull << j) - 1ull));
            if (at < T.n_samples) return T.values[at] + steps;
            break;
        }
        const uint32_t a = occ.symbol(row); // the row's BWT symbol: one load
        if (steps == T.s || a >= T.sigma) break; // tables that do not belong together: the walk ends at its bound
        row = T.c[a] + occ.rank(a, row, T.sigma);
        ++steps;
        bad = row >= T.N;
    }
    atomicOr(err, (uint32_t)LOC_ERR_BOUND);
    return 0u;
}

// rows [lo, lo + count) into out[0 .. count): the expansion
template <class Occ>
__global__ __launch_bounds__(kBlock) void locate_rows_kernel(LocRec T, uint64_t lo, uint64_t count, uint32_t *__restrict__ out, uint32_t *err)
{
    for (uint64_t idx = (uint64_t)blockIdx.x * kBlock + threadIdx.x; idx < count; idx += (uint64_t)gridDim.x * kBlock)
        out[idx] = locate_row<Occ>(T, (uint32_t)(lo + idx), err);
}

// the rows of a run of hits: slot pos_off[h] - base + i gets row L_h + i (pos_off: from the run's first hit on, n entries + 1)
template <class Occ>
__global__ __launch_bounds__(kBlock) void locate_hits_kernel(const LocRec *__restrict__ recs, uint32_t n_records, const uint4 *__restrict__ hits,
                                                             const uint64_t *__restrict__ pos_off, uint64_t n, uint64_t base, uint64_t count,
                                                             uint32_t *__restrict__ out, uint32_t *err)
{
    for (uint64_t idx = (uint64_t)blockIdx.x * kBlock + threadIdx.x; idx < count; idx += (uint64_t)gridDim.x * kBlock) {
        const uint64_t slot = base + idx;
        uint64_t h = 0, e = n; // the last h with pos_off[h] <= slot (pos_off[n] = base + count > slot)
        while (e - h > 1) {
            const uint64_t mid = h + (e - h) / 2;
            if (pos_off[mid] <= slot) h = mid;
            else e = mid;
        }
        const uint4 h0 = hits[2 * h];
        const LocRec T = recs[h0.x % n_records];
        out[idx] = locate_row<Occ>(T, h0.y + (uint32_t)(slot - pos_off[h]), err);
    }
}

// cnt[h] <- the lines of hit h, 0 for a hit whose query or interval does not fit (the SAM size pass reports those)
__global__ __launch_bounds__(kBlock) void locate_count_kernel(const LocRec *__restrict__ recs, uint32_t n_records, uint64_t n_queries,
                                                              const uint4 *__restrict__ hits, uint64_t n_hits, uint64_t *__restrict__ cnt)
{
    const uint64_t h = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (h >= n_hits) return;
    const uint4 h0 = hits[2 * h];
    const bool ok = (uint64_t)h0.x < n_queries && h0.y <= h0.z && h0.z <= recs[h0.x % n_records].N;
    cnt[h] = ok ? (uint64_t)(h0.z - h0.y) : 0ull;
}

// out[0 .. 1] <- the last h in (h_lo, n_hits] with pos_off[h] - base <= cap, h_lo + 1 where there is none; out[2 .. 3] <-
// pos_off of it (one lane)
__global__ void locate_run_kernel(const uint64_t *__restrict__ pos_off, uint64_t n_hits, uint64_t h_lo, uint64_t base, uint64_t cap,
                                  uint32_t *__restrict__ out)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint64_t h = h_lo + 1, e = n_hits + 1; // pos_off[h] - base <= cap holds for h (or h is the one hit a run has at least)
    while (e - h > 1) {
        const uint64_t mid = h + (e - h) / 2;
        if (pos_off[mid] - base <= cap) h = mid;
        else e = mid;
    }
    const uint64_t at = pos_off[h];
    out[0] = (uint32_t)h, out[1] = (uint32_t)(h >> 32), out[2] = (uint32_t)at, out[3] = (uint32_t)(at >> 32);
}

static uint32_t locate_grid(uint64_t count)
{
    const uint64_t grid = (count + kBlock - 1) / kBlock;
    return (uint32_t)(grid < (1u << 20) ? grid : (1u << 20));
}

// a few words of device scratch for totals and error bits (behind the words sx_sam.hip's layout uses)
static int locate_scratch(sx_ctx *ctx, uint32_t **out)
{
    SX_TRY(sx_slab_ensure(ctx, SX_SLAB_SORT, 4096));
    *out = (uint32_t *)ctx->slab[SX_SLAB_SORT].p + 64;
    return 0;
}

// the passes over one window: blocks [b0, b0 + nb), `base` samples in front of them; *total_out: the window's samples
static int sample_window(sx_ctx *ctx, const uint32_t *d_win, uint64_t N, uint32_t q, uint64_t b0, uint32_t nb, uint32_t base, uint4 *marks,
                         uint32_t *values, uint32_t *d_scal, uint32_t *total_out)
{
    const uint32_t grid = sx_div_up(nb, kWavesPerBlock), n_samples = (uint32_t)sa_sample_count(N, q);
    const uint64_t rows = (uint64_t)nb * kOccRows;
    sx_launch(ctx, SX_KC_OTABLE, rows * 4 + (uint64_t)nb * 16, sa_mark_kernel, dim3(grid), dim3(kBlock), d_win, N, (1u << q) - 1u, b0, nb, marks);
    SX_TRY((device_scan<OpAdd>(ctx, nb, InMarkCount{marks + b0}, OutMarkBefore{marks + b0, base}, d_scal, SX_KC_OTABLE, (uint64_t)nb * 36)));
    sx_launch(ctx, SX_KC_OTABLE, (uint64_t)nb * 16 + (rows >> q) * 8, sa_values_kernel, dim3(grid), dim3(kBlock), d_win, b0, nb, (const uint4 *)marks,
              values, n_samples);
    return sx_readback(ctx, d_scal, 1, total_out);
}

static int sample_total_check(sx_ctx *ctx, uint64_t have, uint64_t N, uint32_t q)
{
    if (have == sa_sample_count(N, q)) return 0;
    return sx_fail_msg(ctx, SX_E_ARG, "sampled suffix array: the array does not hold every multiple of the sampling distance once");
}

} // namespace sx

using namespace sx;

int sx_sa_sample_dev_impl(sx_ctx *ctx, const uint32_t *d_sa, uint64_t N, uint32_t q, void *d_marks, uint32_t *d_values)
{
    uint32_t *d_scal, total = 0;
    SX_TRY(locate_scratch(ctx, &d_scal));
    SX_TRY(sample_window(ctx, d_sa, N, q, 0, (uint32_t)occ_blocks(N), 0, (uint4 *)d_marks, d_values, d_scal, &total));
    return sample_total_check(ctx, total, N, q);
}

int sx_sa_sample_host_impl(sx_ctx *ctx, const uint32_t *h_sa, uint64_t N, uint32_t q, void *d_marks, uint32_t *d_values)
{
    uint32_t *d_scal;
    SX_TRY(locate_scratch(ctx, &d_scal));
    uint64_t have = 0;
    // a window: whole blocks' rows.  More samples than the array may have end the loop at once: the check fails then, and
    // its failure is what the body returns (no more windows come up); otherwise the check is made behind the last window
    SX_TRY(sx_upload_windows(ctx, h_sa, N, 4, kOccRows, 0, [&](const uint32_t *d_win, uint64_t b0, uint32_t nb, uint64_t) {
        uint32_t total = 0;
        SX_TRY(sample_window(ctx, d_win, N, q, b0, nb, (uint32_t)have, (uint4 *)d_marks, d_values, d_scal, &total)); // (ends with a sync)
        have += total;
        return have > sa_sample_count(N, q) ? sample_total_check(ctx, have, N, q) : 0;
    }));
    return sample_total_check(ctx, have, N, q);
}

int sx_sa_locate_rows_impl(sx_ctx *ctx, const LocRec &rec, uint64_t row_lo, uint64_t row_hi, uint32_t *d_out)
{
    const uint64_t count = row_hi - row_lo;
    if (!count) return 0;
    uint32_t *d_err, e = 0;
    SX_TRY(locate_scratch(ctx, &d_err));
    SX_CHECK(hipMemsetAsync(d_err, 0, 4, ctx->stream));
    // a row: half a sampling distance of steps, a step one block line and one mark entry
    const uint64_t alg_bytes = count * (4 + (uint64_t)rec.s / 2 * (rec.stride + 16));
    if (rec.packed)
        sx_launch(ctx, SX_KC_SEARCH, alg_bytes, locate_rows_kernel<OccPacked>, dim3(locate_grid(count)), dim3(kBlock), rec, row_lo, count, d_out,
                  d_err);
    else
        sx_launch(ctx, SX_KC_SEARCH, alg_bytes, locate_rows_kernel<OccCompact>, dim3(locate_grid(count)), dim3(kBlock), rec, row_lo, count, d_out,
                  d_err);
    SX_TRY(sx_readback(ctx, d_err, 1, &e));
    if (e) return sx_fail_msg(ctx, SX_E_INTERNAL, "sampled suffix array: a walk met its bound (the samples do not belong to the blocks)");
    return 0;
}

int sx_sa_hits_offsets(sx_ctx *ctx, const LocRec *d_recs, uint32_t n_records, uint64_t n_queries, const uint4 *d_hits, uint64_t n_hits,
                       uint64_t *d_pos_off, uint64_t *total_out)
{
    *total_out = 0;
    if (n_hits)
        sx_launch(ctx, SX_KC_SEARCH, n_hits * 24, locate_count_kernel, dim3(sx_div_up(n_hits, kBlock)), dim3(kBlock), d_recs, n_records, n_queries,
                  d_hits, n_hits, d_pos_off);
    SX_TRY(device_scan64_inplace(ctx, d_pos_off, n_hits, SX_KC_SEARCH));
    uint32_t h[2] = {0, 0};
    SX_TRY(sx_readback(ctx, (const uint32_t *)(d_pos_off + n_hits), 2, h));
    *total_out = (uint64_t)h[0] | ((uint64_t)h[1] << 32);
    return 0;
}

int sx_sa_hits_run(sx_ctx *ctx, const uint64_t *d_pos_off, uint64_t n_hits, uint64_t h_lo, uint64_t base, uint64_t cap, uint32_t *d_scratch4,
                   uint64_t *h_hi_out, uint64_t *rows_out)
{
    sx_launch(ctx, SX_KC_SEARCH, 0, locate_run_kernel, dim3(1), dim3(kWave), d_pos_off, n_hits, h_lo, base, cap, d_scratch4);
    uint32_t h[4] = {0, 0, 0, 0};
    SX_TRY(sx_readback(ctx, d_scratch4, 4, h));
    *h_hi_out = (uint64_t)h[0] | ((uint64_t)h[1] << 32);
    *rows_out = ((uint64_t)h[2] | ((uint64_t)h[3] << 32)) - base;
    if (*h_hi_out <= h_lo || *h_hi_out > n_hits) return sx_fail_msg(ctx, SX_E_INTERNAL, "read mapping: the runs of a batch's hits do not add up");
    return 0;
}

int sx_sa_locate_hits(sx_ctx *ctx, const LocRec *d_recs, uint32_t n_records, bool packed, const uint4 *d_hits, const uint64_t *d_pos_off,
                      uint64_t h_lo, uint64_t h_hi, uint64_t base, uint64_t rows, uint32_t *d_out, uint32_t *d_err)
{
    if (!rows) return 0;
    if (packed)
        sx_launch(ctx, SX_KC_SEARCH, rows * 4, locate_hits_kernel<OccPacked>, dim3(locate_grid(rows)), dim3(kBlock), d_recs, n_records, d_hits + 2 * h_lo,
                  d_pos_off + h_lo, h_hi - h_lo, base, rows, d_out, d_err);
    else
        sx_launch(ctx, SX_KC_SEARCH, rows * 4, locate_hits_kernel<OccCompact>, dim3(locate_grid(rows)), dim3(kBlock), d_recs, n_records, d_hits + 2 * h_lo,
                  d_pos_off + h_lo, h_hi - h_lo, base, rows, d_out, d_err);
    return 0;
}

extern "C" {

int sx_sa_sample_bytes(uint64_t N, uint32_t q, uint64_t *marks_bytes_out, uint64_t *values_bytes_out)
{
    if (N == 0 || N > 0xFFFFFFFFull || !sa_sample_log2_ok(q)) return SX_E_ARG;
    if (marks_bytes_out) *marks_bytes_out = sa_mark_bytes(N);
    if (values_bytes_out) *values_bytes_out = sa_sample_count(N, q) * 4;
    return 0;
}

int sx_sa_sample_build_dev(sx_ctx *ctx, const uint32_t *d_sa, uint64_t N, uint32_t q, void *d_marks_out, uint32_t *d_values_out)
{
    if (!ctx || !d_sa || !d_values_out) return SX_E_ARG;
    if (N == 0 || N > 0xFFFFFFFFull || !sa_sample_log2_ok(q))
        return sx_fail_msg(ctx, SX_E_ARG, "sampled suffix array: N must be in [1, 2^32 - 1] and the sampling distance 2^1 .. 2^10");
    if (!d_marks_out || ((uintptr_t)d_marks_out & 15u)) return sx_fail_msg(ctx, SX_E_ARG, "sampled suffix array: the marks start on a 16-byte boundary");
    SX_CHECK(hipSetDevice(ctx->device));
    return sx_nomem_of(sx_sa_sample_dev_impl(ctx, d_sa, N, q, d_marks_out, d_values_out));
}

int sx_sa_locate_rows_dev(sx_ctx *ctx, const uint32_t *d_c_table, const uint8_t *d_occ, uint64_t N, uint32_t sigma, const void *d_marks,
                          const uint32_t *d_values, uint32_t q, uint64_t row_lo, uint64_t row_hi, uint32_t *d_out)
{
    if (!ctx || !d_c_table || !d_values) return SX_E_ARG;
    if (!sx_map_dims_ok(N, sigma, 1) || !sa_sample_log2_ok(q))
        return sx_fail_msg(ctx, SX_E_ARG, "sampled suffix array: N must be in [1, 2^32 - 1], sigma in [1, 128] and the sampling distance 2^1 .. 2^10");
    if (!d_occ || ((uintptr_t)d_occ & 15u) || !d_marks || ((uintptr_t)d_marks & 15u))
        return sx_fail_msg(ctx, SX_E_ARG, "sampled suffix array: the blocks and the marks start on 16-byte boundaries");
    if (row_lo > row_hi || row_hi > N || (row_hi > row_lo && !d_out)) return sx_fail_msg(ctx, SX_E_ARG, "sampled suffix array: the rows to locate lie in [0, N)");
    SX_CHECK(hipSetDevice(ctx->device));
    return sx_sa_locate_rows_impl(ctx, loc_rec_of(d_c_table, d_occ, N, sigma, d_marks, d_values, q), row_lo, row_hi, d_out);
}

} // extern "C"
