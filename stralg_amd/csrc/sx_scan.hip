// sx_scan.hip -- what of the device-wide scans (sx_scan.hpp) is no template: the scratch of the tile totals, and the
// 64-bit exclusive sum in place (three launches, as device_scan: tile reduce, one-workgroup spine, tile apply).
#include "sx_scan.hpp"

namespace sx {

uint32_t *sx_scan_scratch(sx_ctx *ctx, uint32_t ntiles)
{
    // tile totals of the scan in flight; a slab of its own so that growing it never moves a caller's data
    if (sx_slab_ensure(ctx, SX_SLAB_SCAN, (size_t)ntiles * sizeof(uint32_t)) != 0) return nullptr;
    return (uint32_t *)ctx->slab[SX_SLAB_SCAN].p;
}

constexpr int kScan64Items = 8, kScan64Tile = kBlock * kScan64Items;

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

int device_scan64_inplace(sx_ctx *ctx, uint64_t *d, uint64_t n, int kclass)
{
    if (n == 0) {
        SX_CHECK(hipMemsetAsync(d, 0, sizeof(uint64_t), ctx->stream));
        return 0;
    }
    const uint32_t ntiles = sx_div_up(n, kScan64Tile);
    uint64_t *tile_tot = (uint64_t *)sx_scan_scratch(ctx, 2 * ntiles + 2);
    if (!tile_tot) return sx_fail_msg(ctx, SX_E_NOMEM, "scan scratch");
    sx_launch(ctx, kclass, n * 8, scan64_reduce_kernel, dim3(ntiles), dim3(kBlock), (const uint64_t *)d, n, tile_tot);
    sx_launch(ctx, kclass, 0, scan64_spine_kernel, dim3(1), dim3(kBlock), tile_tot, ntiles, d + n);
    sx_launch(ctx, kclass, n * 16, scan64_apply_kernel, dim3(ntiles), dim3(kBlock), d, n, (const uint64_t *)tile_tot);
    return 0;
}

} // namespace sx
