// sx_locate.hpp -- a sampled suffix array for the compact index: SA values kept at a sampling
// distance, the others recovered by walking LF over the BWT blocks of sx_occ.hpp.
//
// Layout.  The sampling distance is s = 2^q, q in 1 .. 10, and sampling is by text position: row r is marked iff
// SA[r] % s == 0.  Position 0 is always sampled, and the row whose BWT byte is the sentinel has SA = 0, so a walk never
// steps through the sentinel.  A record of N rows has ceil(N / s) samples.  Rows are cut into the 64-row blocks of
// sx_occ.hpp, N / 64 + 1 of them:
//   marks   one 16-byte entry a block (sx_sa_mark): u64 bits, bit j set iff row 64 b + j is marked (rows from N on are
//           clear); u32 before, the number of marked rows in all earlier blocks; u32 zero
//   values  u32 values[ceil(N / s)]: SA[r] of the marked rows in row order; the value of a marked row r = 64 b + j is
//           values[before + popcount(bits & ((1 << j) - 1))]
// Both start on a 16-byte boundary at least (an index allocates them on 256-byte boundaries with a 256-byte tail).
//
// Locate.  SA[row]: while the row is not marked, a = the row's BWT symbol (from the forward blocks), row = C[a] + O(a, row),
// one more step; the value of the marked row plus the steps.  At most s - 1 steps for tables that belong together; a walk
// that reaches s steps, meets a byte that is no symbol or leaves [0, N) sets a bit in an error word and ends.
#pragma once
#include "sx_common.hpp"
#include "sx_occ.hpp"

namespace sx {

constexpr uint32_t kSaSampleMaxLog2 = 10;

struct sx_sa_mark {
    uint64_t bits;
    uint32_t before, zero;
};
static_assert(sizeof(sx_sa_mark) == 16, "a mark entry is one 16-byte word");

static inline bool sa_sample_log2_ok(uint32_t q) { return q >= 1 && q <= kSaSampleMaxLog2; }
static inline uint64_t sa_sample_count(uint64_t N, uint32_t q) { return (N + (1ull << q) - 1) >> q; }
static inline uint64_t sa_mark_bytes(uint64_t N) { return occ_blocks(N) * sizeof(sx_sa_mark); }

// what a walk reads of one record: every pointer is device memory (also the entry of an index's table of its records)
struct LocRec {
    const uint8_t *occ; // the forward blocks
    const uint32_t *c;
    const uint4 *marks;
    const uint32_t *values;
    uint32_t N, sigma, stride, n_samples;
    uint32_t s, packed; // packed: the blocks are the nibble blocks of sx_occ.hpp (the walks read them through OccPacked)
};

static inline LocRec loc_rec_of(const uint32_t *d_c, const uint8_t *d_occ, uint64_t N, uint32_t sigma, const void *d_marks,
                                const uint32_t *d_values, uint32_t q, bool packed = false)
{
    return LocRec{d_occ, d_c, (const uint4 *)d_marks, d_values, (uint32_t)N, sigma, occ_form_stride(sigma, packed),
                  (uint32_t)sa_sample_count(N, q), 1u << q, packed ? 1u : 0u};
}

} // namespace sx

// sx_locate.hip (checks of the arguments are the callers')
// marks and values from a suffix array on the device / on the host (windows of whole blocks through the staging buffers:
// the full array is never resident); SX_E_ARG when the array does not have ceil(N / s) multiples of s
int sx_sa_sample_dev_impl(sx_ctx *ctx, const uint32_t *d_sa, uint64_t N, uint32_t q, void *d_marks, uint32_t *d_values);
int sx_sa_sample_host_impl(sx_ctx *ctx, const uint32_t *h_sa, uint64_t N, uint32_t q, void *d_marks, uint32_t *d_values);
// SA[row_lo .. row_hi) -> d_out[0 .. row_hi - row_lo); synchronous; SX_E_INTERNAL when a walk met its bound
int sx_sa_locate_rows_impl(sx_ctx *ctx, const sx::LocRec &rec, uint64_t row_lo, uint64_t row_hi, uint32_t *d_out);
// The hits form, for the mapper (hits: sx_approx_hit as two 16-byte words, query = read x n_records + record rank):
// d_pos_off[h] <- R - L of hit h (0 for a hit that does not fit its record), scanned in place: d_pos_off[n_hits] <- the sum
int sx_sa_hits_offsets(sx_ctx *ctx, const sx::LocRec *d_recs, uint32_t n_records, uint64_t n_queries, const uint4 *d_hits, uint64_t n_hits,
                       uint64_t *d_pos_off, uint64_t *total_out);
// the run of hits that starts at h_lo and whose rows fit `cap` (one hit at least): *h_hi_out, *rows_out
int sx_sa_hits_run(sx_ctx *ctx, const uint64_t *d_pos_off, uint64_t n_hits, uint64_t h_lo, uint64_t base, uint64_t cap, uint32_t *d_scratch4,
                   uint64_t *h_hi_out, uint64_t *rows_out);
// slot d_pos_off[h] - base + i of d_out <- SA[L_h + i] for the hits [h_lo, h_hi) (asynchronous; d_err |= 1 at a bound);
// packed: the form of every record of d_recs (an index has one form as a whole)
int sx_sa_locate_hits(sx_ctx *ctx, const sx::LocRec *d_recs, uint32_t n_records, bool packed, const uint4 *d_hits, const uint64_t *d_pos_off,
                      uint64_t h_lo, uint64_t h_hi, uint64_t base, uint64_t rows, uint32_t *d_out, uint32_t *d_err);
