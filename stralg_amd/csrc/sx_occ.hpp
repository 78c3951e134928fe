// sx_occ.hpp -- the occurrence counts O(a, row) = #{k < row : bwt[k] == a} behind one accessor in three forms (DESIGN.md
// sections 13 and 15): the full table of sx_bwt.hip, one word a symbol a row, the compact form, BWT blocks with counters
// sampled every 64 rows, and the packed form, the same blocks with a nibble a row for alphabets of up to 8 symbols.  The
// searches (sx_approx.hip, sx_extras.hip) and the walks (sx_locate.hip) are templated on the accessor.
//
// Compact layout, the same for every sigma in [1, 128]: rows 0 .. N in blocks of 64; block b is sigma_pad u32 counters
// (sigma rounded up to a multiple of 16; counter a = O(a, 64 b), counters from sigma on are 0) followed by the 64 bytes
// bwt[64 b .. 64 b + 64), bytes from N on 0xFF (they equal no symbol).  N / 64 + 1 blocks, so row N has one; the base
// is 16-byte aligned at least and the stride a multiple of 64: the bytes of a block are four aligned 16-byte words.  An
// index's blocks start on the 256-byte boundary of a device allocation: for sigma <= 16 a block is one 128-byte line.
//
// Packed layout, the same for every sigma in [1, 8]: the same 64-row blocks, N / 64 + 1 of them; block b is 64 bytes,
// 8 u32 counters (counter a = O(a, 64 b), counters from sigma on are 0) followed by 32 bytes of 64 nibbles: row 64 b + j in
// byte j / 2, the low nibble for even j, the high one for odd j, nibbles from row N on 0xF (they equal no symbol).  The
// base is 16-byte aligned at least: the nibbles of a block are two aligned 16-byte words, and two blocks of an index
// share a 128-byte line.
#pragma once
#include "sx_common.hpp"
#include "sx_bytes16.hpp"

namespace sx {

constexpr uint32_t kOccRows = 64; // rows (and BWT bytes) a block

static inline uint32_t occ_sigma_pad(uint32_t sigma) { return (sigma + 15u) & ~15u; }
static inline uint32_t occ_stride(uint32_t sigma) { return 4u * occ_sigma_pad(sigma) + kOccRows; }
static inline uint64_t occ_blocks(uint64_t N) { return N / kOccRows + 1; }
static inline uint64_t occ_bytes(uint64_t N, uint32_t sigma) { return occ_blocks(N) * occ_stride(sigma); }

constexpr uint32_t kOccPackedMaxSigma = 8, kOccPackedStride = 64, kOccPackedCntBytes = 4u * kOccPackedMaxSigma;
static inline uint64_t occ_packed_bytes(uint64_t N) { return occ_blocks(N) * kOccPackedStride; }
// the blocks of a table in either block form
static inline uint32_t occ_form_stride(uint32_t sigma, bool packed) { return packed ? kOccPackedStride : occ_stride(sigma); }
static inline uint64_t occ_form_bytes(uint64_t N, uint32_t sigma, bool packed) { return occ_blocks(N) * occ_form_stride(sigma, packed); }

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
    // the BWT symbol of a row (0xFF from row N on)
    __device__ __forceinline__ uint32_t symbol(uint32_t row) const
    {
        return p[(uint64_t)(row / kOccRows) * stride + (stride - kOccRows) + row % kOccRows];
    }
};

// the nibbles of w that equal k8's (k8 = a * 0x11111111) among its first `take` (<= 0: none, >= 8: all): a nibble of
// w ^ k8 is zero iff its four bits, folded onto its lowest, leave that one clear
__device__ __forceinline__ uint32_t eq_nibbles(uint32_t w, uint32_t k8, int32_t take)
{
    const uint32_t x = w ^ k8;
    const uint32_t zero = ~(x | (x >> 1) | (x >> 2) | (x >> 3)) & 0x11111111u;
    const uint32_t prefix = take <= 0 ? 0u : take >= 8 ? 0xFFFFFFFFu : (1u << (4 * take)) - 1u;
    return (uint32_t)__popc(zero & prefix);
}

// ... or the packed block's counter plus the nibbles equal to a among the block's first row % 64: one 64-byte half line,
// 32 nibbles a 16-byte load, and the second load only for row % 64 > 32
struct OccPacked {
    const uint8_t *p;
    __device__ __forceinline__ bool present() const { return p != nullptr; }
    __device__ __forceinline__ uint32_t rank(uint32_t a, uint32_t row, uint32_t) const
    {
        const uint8_t *__restrict__ blk = p + (uint64_t)(row / kOccRows) * kOccPackedStride;
        const uint32_t r = row % kOccRows, k8 = a * 0x11111111u;
        uint32_t n = reinterpret_cast<const uint32_t *>(blk)[a];
        const uint4 *__restrict__ nibbles = reinterpret_cast<const uint4 *>(blk + kOccPackedCntBytes);
#pragma unroll
        for (uint32_t q = 0; q < 2; ++q) {
            if (r > q * 32u) {
                const int32_t left = (int32_t)(r - q * 32u);
                const uint4 v = nibbles[q];
                n += eq_nibbles(v.x, k8, left) + eq_nibbles(v.y, k8, left - 8) + eq_nibbles(v.z, k8, left - 16) + eq_nibbles(v.w, k8, left - 24);
            }
        }
        return n;
    }
    // the BWT symbol of a row (0xF from row N on)
    __device__ __forceinline__ uint32_t symbol(uint32_t row) const
    {
        const uint32_t j = row % kOccRows;
        return ((uint32_t)p[(uint64_t)(row / kOccRows) * kOccPackedStride + kOccPackedCntBytes + j / 2u] >> (4u * (j & 1u))) & 0xFu;
    }
};

} // namespace sx

// sx_occ.hip (checks of the arguments are the callers'): blocks from a BWT on the device, blocks from full rows that
// come up from the host in windows, full rows [lo, hi) from blocks; packed: the nibble blocks (sigma <= 8) in place of the
// byte blocks
int sx_occ_build_impl(sx_ctx *ctx, const uint8_t *d_bwt, uint64_t N, uint32_t sigma, uint8_t *d_blocks, bool packed);
int sx_occ_from_rows_impl(sx_ctx *ctx, const uint32_t *h_o_table, uint64_t N, uint32_t sigma, uint8_t *d_blocks, bool packed);
int sx_occ_expand_impl(sx_ctx *ctx, const uint8_t *d_blocks, uint64_t N, uint32_t sigma, uint64_t row_lo, uint64_t row_hi, uint32_t *d_rows,
                       bool packed);
