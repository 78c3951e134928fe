// sx_occ.hip -- the compact occurrence table (sx_occ.hpp): its blocks from a BWT, its blocks from
// full O rows, and full O rows from its blocks.
//
// From a BWT, over tiles of 64 blocks (4096 rows):
//   1. every tile counts its symbols: a wave takes a block at a time, a lane one byte, the count of symbol a in the block
//      is the popcount of a ballot; the 64 x sigma block counts stand in LDS and a thread a symbol adds them up,
//   2. a scan of the tile counts, symbol after symbol (sx_scan.hpp), gives every tile its starting counts,
//   3. the writers count their tile's blocks again, a thread a symbol walks down the blocks with the running count and
//      writes the counters; the bytes are copied a word a lane, 0xFF from N on.
// Where a value goes is a function of the scans alone (no atomics anywhere): the same BWT gives the same bytes.
#include "sx_common.hpp"
#include "sx_device.hpp"
#include "sx_hostio.hpp"
#include "sx_index.hpp"
#include "sx_occ.hpp"
#include "sx_scan.hpp"

namespace sx {

constexpr uint32_t kOccTileBlocks = 64, kOccMaxSigma = 128;
constexpr uint32_t kOccPadByte = 0xFFu;

// cnt[k][a] <- how often symbol a stands in block block0 + k (at most 64: a byte holds it); ends without a barrier
__device__ __forceinline__ void occ_tile_counts(const uint8_t *__restrict__ bwt, uint64_t N, uint32_t sigma, uint64_t block0,
                                                uint8_t (*cnt)[kOccMaxSigma])
{
    const uint32_t lane = (uint32_t)lane_id();
    for (uint32_t k = (uint32_t)wave_id(); k < kOccTileBlocks; k += kWavesPerBlock) {
        const uint64_t i = (block0 + k) * kOccRows + lane;
        const uint32_t sym = i < N ? (uint32_t)bwt[i] : kOccPadByte;
        uint32_t mine[2] = {0, 0}; // the counts of symbols lane and lane + 64
        for (uint32_t a = 0; a < sigma; ++a) {
            const uint32_t c = (uint32_t)__popcll(__ballot(sym == a ? 1 : 0));
            if ((a & 63u) == lane) mine[a >> 6] = c;
        }
        cnt[k][lane] = (uint8_t)mine[0];
        cnt[k][lane + 64u] = (uint8_t)mine[1];
    }
}

// pass 1: tilehist[a][tile] <- symbol a's count in the tile
__global__ __launch_bounds__(kBlock) void occ_count_kernel(const uint8_t *__restrict__ bwt, uint64_t N, uint32_t sigma,
                                                           uint32_t *__restrict__ tilehist, uint32_t ntiles)
{
    __shared__ uint8_t cnt[kOccTileBlocks][kOccMaxSigma];
    const uint32_t tile = blockIdx.x, a = threadIdx.x;
    occ_tile_counts(bwt, N, sigma, (uint64_t)tile * kOccTileBlocks, cnt);
    __syncthreads();
    if (a < sigma) {
        uint32_t tot = 0;
        for (uint32_t k = 0; k < kOccTileBlocks; ++k) tot += cnt[k][a];
        tilehist[(uint64_t)a * ntiles + tile] = tot;
    }
}

// pass 3: the tile's blocks; tilepre: the scanned counts, flat over [sigma][ntiles] (the prefix inside symbol a's row is
// the difference to the row's first entry, as in sx_bwt.hip)
__global__ __launch_bounds__(kBlock) void occ_write_kernel(const uint8_t *__restrict__ bwt, uint64_t N, uint32_t sigma,
                                                           const uint32_t *__restrict__ tilepre, uint32_t ntiles,
                                                           uint8_t *__restrict__ blocks, uint32_t stride, uint64_t nblocks)
{
    __shared__ uint8_t cnt[kOccTileBlocks][kOccMaxSigma];
    const uint32_t tile = blockIdx.x, t = threadIdx.x, cnt_bytes = stride - kOccRows;
    const uint64_t block0 = (uint64_t)tile * kOccTileBlocks;
    occ_tile_counts(bwt, N, sigma, block0, cnt);
    __syncthreads();
    if (t < cnt_bytes / 4u) { // sigma_pad counters a block; those from sigma on are 0
        const bool real = t < sigma;
        uint32_t run = real ? tilepre[(uint64_t)t * ntiles + tile] - tilepre[(uint64_t)t * ntiles] : 0u;
        for (uint32_t k = 0; k < kOccTileBlocks && block0 + k < nblocks; ++k) {
            reinterpret_cast<uint32_t *>(blocks + (block0 + k) * stride)[t] = run;
            if (real) run += cnt[k][t];
        }
    }
    const bool words = ((uintptr_t)bwt & 3u) == 0;
    for (uint32_t wd = t; wd < kOccTileBlocks * (kOccRows / 4u); wd += kBlock) {
        const uint64_t b = block0 + wd / (kOccRows / 4u);
        if (b >= nblocks) break;
        const uint32_t at = 4u * (wd % (kOccRows / 4u));
        const uint64_t i = b * kOccRows + at;
        uint32_t w;
        if (words && i + 4 <= N) {
            w = *reinterpret_cast<const uint32_t *>(bwt + i);
        } else {
            w = 0;
            for (uint32_t e = 0; e < 4; ++e) w |= (i + e < N ? (uint32_t)bwt[i + e] : kOccPadByte) << (8u * e);
        }
        *reinterpret_cast<uint32_t *>(blocks + b * stride + cnt_bytes + at) = w;
    }
}

// Blocks [b0, b0 + nb) from full rows: win holds rows 64 b0 .. min(64 (b0 + nb), N).  A wave a block, a lane a row: the
// row's symbol is the one a whose count differs in the next row; the counters are row 64 b itself.
__global__ __launch_bounds__(kBlock) void occ_from_rows_kernel(const uint32_t *__restrict__ win, uint64_t N, uint32_t sigma, uint64_t b0,
                                                               uint32_t nb, uint8_t *__restrict__ blocks, uint32_t stride)
{
    const uint32_t k = blockIdx.x * kWavesPerBlock + (uint32_t)wave_id(), lane = (uint32_t)lane_id();
    if (k >= nb) return;
    const uint32_t cnt_bytes = stride - kOccRows;
    const uint64_t rel = (uint64_t)k * kOccRows + lane, i = (b0 + k) * kOccRows + lane; // the lane's row in the window, in the table
    uint32_t sym = kOccPadByte;
    if (i < N) {
        const uint32_t *__restrict__ here = win + rel * sigma, *__restrict__ next = here + sigma;
        for (uint32_t a = 0; a < sigma; ++a)
            if (next[a] != here[a]) sym = a;
    }
    uint8_t *blk = blocks + (b0 + k) * stride;
    for (uint32_t a = lane; a < cnt_bytes / 4u; a += kWave)
        reinterpret_cast<uint32_t *>(blk)[a] = a < sigma ? win[(uint64_t)k * kOccRows * sigma + a] : 0u;
    blk[cnt_bytes + lane] = (uint8_t)sym;
}

// rows[(row - lo) * sigma + a] <- O(a, row) for the rows [lo, hi): one rank an entry, through the searches' accessor
__global__ __launch_bounds__(kBlock) void occ_expand_kernel(OccCompact occ, uint32_t sigma, uint64_t lo, uint64_t count,
                                                            uint32_t *__restrict__ rows)
{
    for (uint64_t idx = (uint64_t)blockIdx.x * kBlock + threadIdx.x; idx < count; idx += (uint64_t)gridDim.x * kBlock)
        rows[idx] = occ.rank((uint32_t)(idx % sigma), (uint32_t)(lo + idx / sigma), sigma);
}

static int occ_dims_check(sx_ctx *ctx, uint64_t N, uint32_t sigma, const void *d_blocks)
{
    if (!sx_map_dims_ok(N, sigma, 1)) return sx_fail_msg(ctx, SX_E_ARG, "compact table: N must be in [1, 2^32 - 1] and sigma in [1, 128]");
    if (!d_blocks || ((uintptr_t)d_blocks & 15u)) return sx_fail_msg(ctx, SX_E_ARG, "compact table: the blocks start on a 16-byte boundary");
    return 0;
}

} // namespace sx

using namespace sx;

int sx_occ_build_impl(sx_ctx *ctx, const uint8_t *d_bwt, uint64_t N, uint32_t sigma, uint8_t *d_blocks)
{
    const uint64_t nblocks = occ_blocks(N);
    const uint32_t ntiles = sx_div_up(nblocks, kOccTileBlocks), stride = occ_stride(sigma);
    const uint64_t flat_n = (uint64_t)sigma * ntiles;
    SX_TRY(sx_slab_ensure(ctx, SX_SLAB_BWT, (size_t)flat_n * 4 + 256));
    uint32_t *tilehist = (uint32_t *)ctx->slab[SX_SLAB_BWT].p;
    sx_launch(ctx, SX_KC_OTABLE, N, occ_count_kernel, dim3(ntiles), dim3(kBlock), d_bwt, N, sigma, tilehist, ntiles);
    SX_TRY((device_scan<OpAdd>(ctx, flat_n, InU32{tilehist}, OutExclusive{tilehist}, nullptr, SX_KC_SCAN, flat_n * 12)));
    sx_launch(ctx, SX_KC_OTABLE, N + nblocks * stride, occ_write_kernel, dim3(ntiles), dim3(kBlock), d_bwt, N, sigma, (const uint32_t *)tilehist,
              ntiles, d_blocks, stride, nblocks);
    return 0;
}

int sx_occ_from_rows_impl(sx_ctx *ctx, const uint32_t *h_o_table, uint64_t N, uint32_t sigma, uint8_t *d_blocks)
{
    const uint64_t row_bytes = 4ull * sigma; // a window: whole blocks' rows and the row behind them
    const uint32_t stride = occ_stride(sigma);
    return sx_upload_windows(ctx, h_o_table, N, row_bytes, kOccRows, 1, [&](const uint32_t *d_win, uint64_t b0, uint32_t nb, uint64_t rows) {
        sx_launch(ctx, SX_KC_OTABLE, rows * row_bytes, occ_from_rows_kernel, dim3(sx_div_up(nb, kWavesPerBlock)), dim3(kBlock), d_win, N, sigma, b0, nb,
                  d_blocks, stride);
        return 0;
    }); // (ends with a sync, before the window goes)
}

int sx_occ_expand_impl(sx_ctx *ctx, const uint8_t *d_blocks, uint64_t N, uint32_t sigma, uint64_t row_lo, uint64_t row_hi, uint32_t *d_rows)
{
    (void)N;
    const uint64_t count = (row_hi - row_lo) * sigma;
    if (!count) return 0;
    const uint64_t grid = (count + kBlock - 1) / kBlock;
    sx_launch(ctx, SX_KC_OTABLE, count * 4, occ_expand_kernel, dim3((uint32_t)(grid < (1u << 20) ? grid : (1u << 20))), dim3(kBlock),
              OccCompact{d_blocks, occ_stride(sigma)}, sigma, row_lo, count, d_rows);
    return 0;
}

extern "C" {

uint64_t sx_occ_compact_bytes(uint64_t N, uint32_t sigma) { return sx_map_dims_ok(N, sigma, 1) ? occ_bytes(N, sigma) : 0; }

int sx_occ_compact_build_dev(sx_ctx *ctx, const uint8_t *d_bwt, uint64_t N, uint32_t sigma, uint8_t *d_blocks_out)
{
    if (!ctx || !d_bwt) return SX_E_ARG;
    SX_TRY(occ_dims_check(ctx, N, sigma, d_blocks_out));
    SX_CHECK(hipSetDevice(ctx->device));
    SX_TRY(sx_occ_build_impl(ctx, d_bwt, N, sigma, d_blocks_out));
    return sx_sync(ctx);
}

int sx_occ_compact_expand_dev(sx_ctx *ctx, const uint8_t *d_blocks, uint64_t N, uint32_t sigma, uint64_t row_lo, uint64_t row_hi,
                              uint32_t *d_rows_out)
{
    if (!ctx) return SX_E_ARG;
    SX_TRY(occ_dims_check(ctx, N, sigma, d_blocks));
    if (row_lo > row_hi || row_hi > N + 1 || (row_hi > row_lo && !d_rows_out))
        return sx_fail_msg(ctx, SX_E_ARG, "compact table: the rows to expand lie in [0, N]");
    SX_CHECK(hipSetDevice(ctx->device));
    SX_TRY(sx_occ_expand_impl(ctx, d_blocks, N, sigma, row_lo, row_hi, d_rows_out));
    return sx_sync(ctx);
}

} // extern "C"
