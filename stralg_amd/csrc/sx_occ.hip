// sx_occ.hip -- the compact occurrence table (sx_occ.hpp) and its packed form (section 15): their
// blocks from a BWT, their blocks from full O rows, and full O rows from their blocks.  The kernels are the same for both
// forms but for how a block's symbols are stored (BlockBytes, BlockNibbles) and read (OccCompact, OccPacked).
//
// From a BWT, over tiles of 64 blocks (4096 rows):
//   1. every tile counts its symbols: a wave takes a block at a time, a lane one byte, the count of symbol a in the block
//      is the popcount of a ballot; the 64 x sigma block counts stand in LDS and a thread a symbol adds them up,
//   2. a scan of the tile counts, symbol after symbol (sx_scan.hpp), gives every tile its starting counts,
//   3. the writers count their tile's blocks again, a thread a symbol walks down the blocks with the running count and
//      writes the counters; the symbols are copied a word a lane (4 bytes, or 8 nibbles), 0xFF / 0xF from N on.
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

// How a block's symbols are stored.  word(lo, hi): the word of kRowsPerWord rows given as bytes, the first row lowest
// (hi: rows 4 .. 7); put_row: a wave a block, a lane a row, every lane of the wave calls it.
struct BlockBytes { // the compact block: a byte a row behind 4 sigma_pad bytes of counters
    uint32_t stride;
    static constexpr uint32_t kRowsPerWord = 4;
    __device__ __forceinline__ uint32_t cnt_bytes() const { return stride - kOccRows; }
    static __device__ __forceinline__ uint32_t word(uint32_t lo, uint32_t) { return lo; }
    __device__ __forceinline__ void put_row(uint8_t *blk, uint32_t lane, uint32_t sym) const { blk[cnt_bytes() + lane] = (uint8_t)sym; }
};
struct BlockNibbles { // the packed block: a nibble a row behind 8 counters
    static constexpr uint32_t stride = kOccPackedStride, kRowsPerWord = 8;
    static __device__ __forceinline__ uint32_t cnt_bytes() { return kOccPackedCntBytes; }
    static __device__ __forceinline__ uint32_t half(uint32_t w) // the low nibbles of w's four bytes
    {
        return (w & 0xFu) | ((w >> 4) & 0xF0u) | ((w >> 8) & 0xF00u) | ((w >> 12) & 0xF000u);
    }
    static __device__ __forceinline__ uint32_t word(uint32_t lo, uint32_t hi) { return half(lo) | (half(hi) << 16); }
    __device__ __forceinline__ void put_row(uint8_t *blk, uint32_t lane, uint32_t sym) const
    {
        const uint32_t odd = __shfl_xor(sym, 1); // (to the even lane: the row behind its own)
        if (!(lane & 1u)) blk[cnt_bytes() + lane / 2u] = (uint8_t)((sym & 0xFu) | ((odd & 0xFu) << 4));
    }
};

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
template <class Store>
__global__ __launch_bounds__(kBlock) void occ_write_kernel(const uint8_t *__restrict__ bwt, uint64_t N, uint32_t sigma,
                                                           const uint32_t *__restrict__ tilepre, uint32_t ntiles,
                                                           uint8_t *__restrict__ blocks, Store store, uint64_t nblocks)
{
    __shared__ uint8_t cnt[kOccTileBlocks][kOccMaxSigma];
    const uint32_t tile = blockIdx.x, t = threadIdx.x, cnt_bytes = store.cnt_bytes(), stride = store.stride;
    constexpr uint32_t kWords = kOccRows / Store::kRowsPerWord; // words of symbols a block
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
    for (uint32_t wd = t; wd < kOccTileBlocks * kWords; wd += kBlock) {
        const uint64_t b = block0 + wd / kWords;
        if (b >= nblocks) break;
        const uint32_t at = wd % kWords;
        uint32_t w[2] = {0u, 0u}; // the rows' bytes, four a word
#pragma unroll
        for (uint32_t h = 0; h < Store::kRowsPerWord / 4u; ++h) {
            const uint64_t i = b * kOccRows + at * Store::kRowsPerWord + 4u * h;
            if (words && i + 4 <= N) {
                w[h] = *reinterpret_cast<const uint32_t *>(bwt + i);
            } else {
                for (uint32_t e = 0; e < 4; ++e) w[h] |= (i + e < N ? (uint32_t)bwt[i + e] : kOccPadByte) << (8u * e);
            }
        }
        *reinterpret_cast<uint32_t *>(blocks + b * stride + cnt_bytes + 4u * at) = Store::word(w[0], w[1]);
    }
}

// Blocks [b0, b0 + nb) from full rows: win holds rows 64 b0 .. min(64 (b0 + nb), N).  A wave a block, a lane a row: the
// row's symbol is the one a whose count differs in the next row; the counters are row 64 b itself.
template <class Store>
__global__ __launch_bounds__(kBlock) void occ_from_rows_kernel(const uint32_t *__restrict__ win, uint64_t N, uint32_t sigma, uint64_t b0,
                                                               uint32_t nb, uint8_t *__restrict__ blocks, Store store)
{
    const uint32_t k = blockIdx.x * kWavesPerBlock + (uint32_t)wave_id(), lane = (uint32_t)lane_id();
    if (k >= nb) return; // (the whole wave)
    const uint32_t cnt_bytes = store.cnt_bytes(), stride = store.stride;
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
    store.put_row(blk, lane, sym);
}

// rows[(row - lo) * sigma + a] <- O(a, row) for the rows [lo, hi): one rank an entry, through the searches' accessor
template <class Occ>
__global__ __launch_bounds__(kBlock) void occ_expand_kernel(Occ occ, uint32_t sigma, uint64_t lo, uint64_t count,
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
static int occ_packed_dims_check(sx_ctx *ctx, uint64_t N, uint32_t sigma, const void *d_blocks)
{
    if (!sx_map_dims_ok(N, sigma, 1) || sigma > kOccPackedMaxSigma)
        return sx_fail_msg(ctx, SX_E_ARG, "packed table: N must be in [1, 2^32 - 1] and sigma in [1, 8]");
    if (!d_blocks || ((uintptr_t)d_blocks & 15u)) return sx_fail_msg(ctx, SX_E_ARG, "packed table: the blocks start on a 16-byte boundary");
    return 0;
}

template <class Store>
static void occ_write_launch(sx_ctx *ctx, const uint8_t *d_bwt, uint64_t N, uint32_t sigma, const uint32_t *tilepre, uint32_t ntiles,
                             uint8_t *d_blocks, Store store, uint64_t nblocks)
{
    sx_launch(ctx, SX_KC_OTABLE, N + nblocks * store.stride, occ_write_kernel<Store>, dim3(ntiles), dim3(kBlock), d_bwt, N, sigma, tilepre, ntiles,
              d_blocks, store, nblocks);
}

template <class Store>
static int occ_from_rows(sx_ctx *ctx, const uint32_t *h_o_table, uint64_t N, uint32_t sigma, uint8_t *d_blocks, Store store)
{
    const uint64_t row_bytes = 4ull * sigma; // a window: whole blocks' rows and the row behind them
    return sx_upload_windows(ctx, h_o_table, N, row_bytes, kOccRows, 1, [&](const uint32_t *d_win, uint64_t b0, uint32_t nb, uint64_t rows) {
        sx_launch(ctx, SX_KC_OTABLE, rows * row_bytes, occ_from_rows_kernel<Store>, dim3(sx_div_up(nb, kWavesPerBlock)), dim3(kBlock), d_win, N, sigma,
                  b0, nb, d_blocks, store);
        return 0;
    }); // (ends with a sync, before the window goes)
}

template <class Occ> static void occ_expand_launch(sx_ctx *ctx, Occ occ, uint32_t sigma, uint64_t row_lo, uint64_t count, uint32_t *d_rows)
{
    const uint64_t grid = (count + kBlock - 1) / kBlock;
    sx_launch(ctx, SX_KC_OTABLE, count * 4, occ_expand_kernel<Occ>, dim3((uint32_t)(grid < (1u << 20) ? grid : (1u << 20))), dim3(kBlock), occ, sigma,
              row_lo, count, d_rows);
}

} // namespace sx

using namespace sx;

int sx_occ_build_impl(sx_ctx *ctx, const uint8_t *d_bwt, uint64_t N, uint32_t sigma, uint8_t *d_blocks, bool packed)
{
    const uint64_t nblocks = occ_blocks(N);
    const uint32_t ntiles = sx_div_up(nblocks, kOccTileBlocks);
    const uint64_t flat_n = (uint64_t)sigma * ntiles;
    SX_TRY(sx_slab_ensure(ctx, SX_SLAB_BWT, (size_t)flat_n * 4 + 256));
    uint32_t *tilehist = (uint32_t *)ctx->slab[SX_SLAB_BWT].p;
    sx_launch(ctx, SX_KC_OTABLE, N, occ_count_kernel, dim3(ntiles), dim3(kBlock), d_bwt, N, sigma, tilehist, ntiles);
    SX_TRY((device_scan<OpAdd>(ctx, flat_n, InU32{tilehist}, OutExclusive{tilehist}, nullptr, SX_KC_SCAN, flat_n * 12)));
    if (packed) occ_write_launch(ctx, d_bwt, N, sigma, tilehist, ntiles, d_blocks, BlockNibbles{}, nblocks);
    else occ_write_launch(ctx, d_bwt, N, sigma, tilehist, ntiles, d_blocks, BlockBytes{occ_stride(sigma)}, nblocks);
    return 0;
}

int sx_occ_from_rows_impl(sx_ctx *ctx, const uint32_t *h_o_table, uint64_t N, uint32_t sigma, uint8_t *d_blocks, bool packed)
{
    return packed ? occ_from_rows(ctx, h_o_table, N, sigma, d_blocks, BlockNibbles{})
                  : occ_from_rows(ctx, h_o_table, N, sigma, d_blocks, BlockBytes{occ_stride(sigma)});
}

int sx_occ_expand_impl(sx_ctx *ctx, const uint8_t *d_blocks, uint64_t N, uint32_t sigma, uint64_t row_lo, uint64_t row_hi, uint32_t *d_rows,
                       bool packed)
{
    (void)N;
    const uint64_t count = (row_hi - row_lo) * sigma;
    if (!count) return 0;
    if (packed) occ_expand_launch(ctx, OccPacked{d_blocks}, sigma, row_lo, count, d_rows);
    else occ_expand_launch(ctx, OccCompact{d_blocks, occ_stride(sigma)}, sigma, row_lo, count, d_rows);
    return 0;
}

extern "C" {

uint64_t sx_occ_compact_bytes(uint64_t N, uint32_t sigma) { return sx_map_dims_ok(N, sigma, 1) ? occ_bytes(N, sigma) : 0; }

int sx_occ_compact_build_dev(sx_ctx *ctx, const uint8_t *d_bwt, uint64_t N, uint32_t sigma, uint8_t *d_blocks_out)
{
    if (!ctx || !d_bwt) return SX_E_ARG;
    SX_TRY(occ_dims_check(ctx, N, sigma, d_blocks_out));
    SX_CHECK(hipSetDevice(ctx->device));
    SX_TRY(sx_occ_build_impl(ctx, d_bwt, N, sigma, d_blocks_out, false));
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
    SX_TRY(sx_occ_expand_impl(ctx, d_blocks, N, sigma, row_lo, row_hi, d_rows_out, false));
    return sx_sync(ctx);
}

uint64_t sx_occ_packed_bytes(uint64_t N, uint32_t sigma)
{
    return sx_map_dims_ok(N, sigma, 1) && sigma <= kOccPackedMaxSigma ? occ_packed_bytes(N) : 0;
}

int sx_occ_packed_build_dev(sx_ctx *ctx, const uint8_t *d_bwt, uint64_t N, uint32_t sigma, uint8_t *d_blocks_out)
{
    if (!ctx || !d_bwt) return SX_E_ARG;
    SX_TRY(occ_packed_dims_check(ctx, N, sigma, d_blocks_out));
    SX_CHECK(hipSetDevice(ctx->device));
    SX_TRY(sx_occ_build_impl(ctx, d_bwt, N, sigma, d_blocks_out, true));
    return sx_sync(ctx);
}

int sx_occ_packed_expand_dev(sx_ctx *ctx, const uint8_t *d_blocks, uint64_t N, uint32_t sigma, uint64_t row_lo, uint64_t row_hi,
                             uint32_t *d_rows_out)
{
    if (!ctx) return SX_E_ARG;
    SX_TRY(occ_packed_dims_check(ctx, N, sigma, d_blocks));
    if (row_lo > row_hi || row_hi > N + 1 || (row_hi > row_lo && !d_rows_out))
        return sx_fail_msg(ctx, SX_E_ARG, "packed table: the rows to expand lie in [0, N]");
    SX_CHECK(hipSetDevice(ctx->device));
    SX_TRY(sx_occ_expand_impl(ctx, d_blocks, N, sigma, row_lo, row_hi, d_rows_out, true));
    return sx_sync(ctx);
}

} // extern "C"
