// sx_occ.hpp -- the occurrence counts O(a, row) = #{k < row : bwt[k] == a} behind one accessor in two forms (DESIGN.md
// section 13): the full table of sx_bwt.hip, one word a symbol a row, and the compact form, BWT blocks with counters
// sampled every 64 rows.  The searches (sx_approx.hip, sx_extras.hip) are templated on the accessor.
//
// Compact layout, the same for every sigma in [1, 128]: rows 0 .. N in blocks of 64; block b is sigma_pad u32 counters
// (sigma rounded up to a multiple of 16; counter a = O(a, 64 b), counters from sigma on are 0) followed by the 64 bytes
// bwt[64 b .. 64 b + 64), bytes from N on 0xFF (they equal no symbol).  N / 64 + 1 blocks, so row N has one; the base
// is 16-byte aligned at least and the stride a multiple of 64: the bytes of a block are four aligned 16-byte words.  An
// index's blocks start on the 256-byte boundary of a device allocation: for sigma <= 16 a block is one 128-byte line.
#pragma once
#include "sx_common.hpp"
#include "sx_bytes16.hpp"

namespace sx {

constexpr uint32_t kOccRows = 64; // rows (and BWT bytes) a block

static inline uint32_t occ_sigma_pad(uint32_t sigma) { return (sigma + 15u) & ~15u; }
static inline uint32_t occ_stride(uint32_t sigma) { return 4u * occ_sigma_pad(sigma) + kOccRows; }
static inline uint64_t occ_blocks(uint64_t N) { return N / kOccRows + 1; }
static inline uint64_t occ_bytes(uint64_t N, uint32_t sigma) { return occ_blocks(N) * occ_stride(sigma); }


// rank(a, row, sigma) = O(a, row): the full table's word ...
struct OccFull {
    const uint32_t *p;
    __device__ __forceinline__ bool present() const { return p != nullptr; }
    __device__ __forceinline__ uint32_t rank(uint32_t a, uint32_t row, uint32_t sigma) const { return p[(uint64_t)row * sigma + a]; }
};

// ... or the block's counter plus the bytes equal to a among the block's first row % 64: 16 bytes a load, a mask of the
// equal bytes (eq16) cut to the prefix, a popcount; the 16-byte words behind the prefix are not read
struct OccCompact {
    const uint8_t *p;
    uint32_t stride; // 4 sigma_pad + 64
    __device__ __forceinline__ bool present() const { return p != nullptr; }
    __device__ __forceinline__ uint32_t rank(uint32_t a, uint32_t row, uint32_t) const
    {
        const uint8_t *__restrict__ blk = p + (uint64_t)(row / kOccRows) * stride;
        const uint32_t r = row % kOccRows, k4 = a * 0x01010101u;
        uint32_t n = reinterpret_cast<const uint32_t *>(blk)[a];
        const uint4 *__restrict__ bytes = reinterpret_cast<const uint4 *>(blk + (stride - kOccRows));
#pragma unroll
        for (uint32_t q = 0; q < kOccRows / kBytes16; ++q) {
            if (r > q * kBytes16) {
                const uint32_t left = r - q * kBytes16;
                const uint32_t prefix = left < (uint32_t)kBytes16 ? (1u << left) - 1u : 0xFFFFu;
                n += (uint32_t)__popc(eq16(bytes[q], k4) & prefix);
            }
        }
        return n;
    }
};

} // namespace sx

// sx_occ.hip (checks of the arguments are the callers'): blocks from a BWT on the device, blocks from full rows that
// come up from the host in windows, full rows [lo, hi) from blocks
int sx_occ_build_impl(sx_ctx *ctx, const uint8_t *d_bwt, uint64_t N, uint32_t sigma, uint8_t *d_blocks);
int sx_occ_from_rows_impl(sx_ctx *ctx, const uint32_t *h_o_table, uint64_t N, uint32_t sigma, uint8_t *d_blocks);
int sx_occ_expand_impl(sx_ctx *ctx, const uint8_t *d_blocks, uint64_t N, uint32_t sigma, uint64_t row_lo, uint64_t row_hi, uint32_t *d_rows);
