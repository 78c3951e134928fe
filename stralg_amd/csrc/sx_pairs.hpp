// sx_pairs.hpp -- the join of paired reads (sx_pairs.hip): what the mapper's loop (sx_map.hip) asks of it
// between a batch's merged hits and the text of its line descriptors (sx_sam.hpp).
#pragma once
#include "sx_common.hpp"

namespace sx {

// A batch of whole pairs as the join reads it: its hits in (read, record, hit) order with query = read x records + record,
// read 4p + 2m + s being strand s of mate m + 1 of pair p, and where the hits of every (read, record) start
struct PairJoin {
    const uint4 *hits; // sx_approx_hit as two 16-byte words
    uint64_t n_hits;
    const uint64_t *vbase; // n_reads x n_records + 1 entries
    uint32_t n_reads, n_records;
    const uint32_t *const *sa_list; // one suffix array per record rank, or (a sampled index) not read
    const uint64_t *sa_len_list;
    const uint32_t *positions; // (a sampled index) the position of every line of the batch, in line order; else null
    uint32_t min_insert, max_insert;
};

// what the join keeps of every line of the batch: its 0-based position and its span, and its hit
struct PairLines {
    uint64_t *line_off; // n_hits + 1: the lines in front of every hit
    uint2 *ps;          // per line: position, span
    uint32_t *hit;      // per line: its hit
    uint64_t n_lines;
};

// L.line_off <- R - L of every hit, scanned; L.n_lines <- their sum.  SX_E_INTERNAL: a hit does not fit its batch or record
int pair_lines_count(sx_ctx *ctx, const PairJoin &J, PairLines &L);
// L.ps and L.hit of every line (the positions from the suffix arrays, or from J.positions)
int pair_lines_expand(sx_ctx *ctx, const PairJoin &J, const PairLines &L);
// d_cnt[l] (n_lines + 1 entries) <- the proper combinations (a, b) of line l as a, for a line of a first mate, else 0;
// scanned in place: d_cnt[l] <- the combinations in front of line l's, *combos_out <- all of them
int pair_count(sx_ctx *ctx, const PairJoin &J, const PairLines &L, uint64_t *d_cnt, uint64_t *combos_out);
// d_out[2 c], d_out[2 c + 1] <- a's and b's line of combination c: c = d_cnt[a] + the proper b in front of b
int pair_fill(sx_ctx *ctx, const PairJoin &J, const PairLines &L, const uint64_t *d_cnt, sx_pair_line *d_out);

} // namespace sx
