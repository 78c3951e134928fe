// sx_index.hpp -- the device-resident index (sx_index.hip) and what the mapper's loop (sx_map.hip) reads of it.
#pragma once
#include "sx_common.hpp"
#include "sx_hostio.hpp"
#include "sx_locate.hpp"

#include <string>
#include <vector>

struct sx_index_rec {
    std::string name;
    uint64_t N = 0;
    uint32_t sigma = 0;
    signed char remap[256];
    uint8_t *d_string = nullptr; // N bytes (the sentinel last), or null
    uint32_t *d_sa = nullptr, *d_c = nullptr, *d_o = nullptr, *d_ro = nullptr;
    // a record of a compact index has the blocks of sx_occ.hpp in place of d_o / d_ro (d_rocc null: no reverse); packed:
    // they are the nibble blocks (sigma <= 8)
    uint8_t *d_occ = nullptr, *d_rocc = nullptr;
    bool packed = false;
    // a record of a sampled index has the marks and values of sx_locate.hpp in place of d_sa (which is null then)
    uint8_t *d_sa_marks = nullptr;
    uint32_t *d_sa_values = nullptr;
    uint32_t sa_log2 = 0;
    // the record's form: full (d_sa, d_o, d_ro), compact (byte or nibble blocks for d_o / d_ro) or compact
    // and sampled
    bool compact() const { return d_occ != nullptr; }
    bool sampled() const { return sa_log2 != 0; }
    bool has_ro() const { return d_ro || d_rocc; }
    sx::LocRec loc() const { return sx::loc_rec_of(d_c, d_occ, N, sigma, d_sa_marks, d_sa_values, sa_log2, packed); } // what a walk reads of it
};

struct sx_index {
    int device = 0;
    bool compact = false; // SX_INDEX_COMPACT: every record it has or gets is in the compact form
    bool packed = false;  // SX_INDEX_PACKED (with compact): every record's blocks are nibble blocks, and a record has sigma <= 8
    uint32_t sa_log2 = 0; // SX_INDEX_SA_SAMPLE_LOG2: 0, or every record keeps a suffix array sampled at this distance's log2
    std::vector<sx_index_rec> recs; // FASTA file order
    size_t device_bytes = 0;
    // the mapper's view of the records (rebuilt whenever a record is added): names and their offsets, one 256-byte
    // symbol table a record, the suffix arrays' addresses and lengths and, in a sampled index, what a walk reads of every
    // record (an array of sx::LocRec, sx_locate.hpp); for NM and MD (SX_MAP_TAGS) the remapped strings' addresses (null
    // where a record has none) and a 256-byte table a record, the letter behind every code: the inverse of its remap table
    uint8_t *d_rnames = nullptr, *d_tabs = nullptr, *d_letters = nullptr;
    const uint8_t **d_text_list = nullptr;
    void *d_loc_list = nullptr;
    uint32_t *d_rname_off = nullptr;
    const uint32_t **d_sa_list = nullptr;
    uint64_t *d_sa_lens = nullptr;
    size_t view_bytes = 0;
};

// the letter behind every code of a record: the inverse of its remap table (code 0, the sentinel, and the codes the table
// does not give stay 0)
static inline void sx_map_letters_of(const signed char *remap, uint32_t sigma, uint8_t *letters)
{
    for (int c = 0; c < 256; ++c) letters[c] = 0;
    for (int b = 0; b < 256; ++b)
        if (remap[b] > 0 && (uint32_t)remap[b] < sigma) letters[(int)remap[b]] = (uint8_t)b;
}

// A record's host tables as an index takes them (min_sigma 1: the record without symbols has N = 1, sigma = 1) or as the
// mapper searches them (min_sigma 2): N and sigma in range, and every array there
static inline bool sx_map_dims_ok(uint64_t N, uint32_t sigma, uint32_t min_sigma)
{
    return N != 0 && N <= 0xFFFFFFFFull && sigma >= min_sigma && sigma <= 128;
}
static inline bool sx_map_record_check(const sx_map_record &R, uint32_t min_sigma)
{
    return R.name && R.sa && R.c_table && R.o_table && R.remap && sx_map_dims_ok(R.N, R.sigma, min_sigma);
}

// the bits of a mapping call's flags word that mean something (sx_map_reads_stream_ex, sx_index_map_reads_ex, sx_map_reads_limit)
constexpr uint32_t sx_map_known_flags = SX_MAP_BOTH_STRANDS | SX_MAP_BEST_STRATUM | SX_MAP_NO_INDELS | SX_MAP_TAGS | SX_MAP_UNMAPPED | SX_MAP_HEADER | SX_MAP_MAPQ;
// the search flags (SX_SEARCH_*) that a mapping call's flags word asks of its searches
static inline uint32_t sx_map_search_flags(uint32_t flags) { return (flags & SX_MAP_NO_INDELS) ? (uint32_t)SX_SEARCH_NO_INDELS : 0u; }

// sx_map.hip: the mapper's loop over reads and an index that both lie on ctx's device (flags: those of
// sx_map_reads_stream_ex); h_seq_off: the host's copy of reads.d_seq_off, or null (the loop then reads the two entries a
// batch needs back)
int sx_map_reads_core(sx_ctx *ctx, const sx_index *idx, const sx_fastq_dev &reads, const uint32_t *h_seq_off, int edits, uint32_t flags,
                      sx_sink_fn sink, void *user);
// sx_map.hip: the paired call over the two mates' read sets on ctx's device; flags: SX_MAP_BEST_STRATUM,
// SX_MAP_NO_INDELS (the callers have refused the others)
int sx_map_pairs_core(sx_ctx *ctx, const sx_index *idx, const sx_fastq_dev &reads1, const sx_fastq_dev &reads2, int edits, const sx_pair_opts &opts,
                      uint32_t flags, sx_sink_fn sink, void *user);
// sx_fastq.hip: the mates of two read sets of the same count as one set of twice as many reads, read 2p + m
int sx_fastq_mates_dev(sx_ctx *ctx, const sx_fastq_dev *in1, const sx_fastq_dev *in2, sx_fastq_dev *out);
// sx_map.hip: SX_MAP_TAGS reads every record's string; SX_E_ARG with a message where the flag is set and a record has none
int sx_map_tags_check(sx_ctx *ctx, const sx_index *idx, uint32_t flags);
// sx_map.hip: SX_MAP_MAPQ needs SX_MAP_BEST_STRATUM; SX_E_ARG with a message where it stands alone
int sx_map_mapq_check(sx_ctx *ctx, uint32_t flags);
// sx_approx.hip: sx_bwt_approx_search_dev_ex over the tables of a record, full, compact or packed (search_flags: SX_SEARCH_*)
int sx_approx_search_record(sx_ctx *ctx, const sx_index_rec &R, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t count, int max_edits,
                            uint64_t *d_hit_offsets, sx_approx_hit *d_hits, uint64_t hit_capacity, uint64_t *total_hits_out, uint32_t search_flags);
// the two passes of that search on their own (sx_best.hip runs them over different pattern sets).  Count: the hit offsets
// (count + 1 entries) and the total of `count` >= 1 patterns.  Emit: the hits of patterns whose offsets are known (total of
// them, total >= 1) to d_hits; hit.query is the pattern's number in this set
int sx_approx_count_record(sx_ctx *ctx, const sx_index_rec &R, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t count, int max_edits,
                           uint64_t *d_hit_offsets, uint64_t *total_hits_out, uint32_t search_flags);
int sx_approx_emit_record(sx_ctx *ctx, const sx_index_rec &R, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t count, int max_edits,
                          const uint64_t *d_hit_offsets, sx_approx_hit *d_hits, uint64_t total_hits, uint32_t search_flags);
// sx_map.hip: out[i] = table[seqs[i]] for i in [lo, hi) (a record's 256-byte symbol table; sam_remap_kernel)
void sx_sam_remap(sx_ctx *ctx, const uint8_t *d_seqs, const uint8_t *d_table, uint8_t *d_out, uint64_t lo, uint64_t hi);
// sx_map.hip, SX_MAP_UNMAPPED.  Count: d_cnt (groups x gsize x n_rec counts of (read, record), not yet
// scanned) gives every group of gsize reads whose counts are all 0 one slot, its first read's with record 0.  Place: over
// those counts scanned (d_vbase), the placeholder (query: that slot, L = R = 0, no gaps) of every group with exactly one
// slot into d_dst (n_dst entries; error bit 2 in *d_err beyond them) -- before the hits are merged, which overwrite it
// where that one slot is a hit's
void sx_map_unmapped_count(sx_ctx *ctx, uint64_t *d_cnt, uint32_t groups, uint32_t gsize, uint32_t n_rec);
void sx_map_unmapped_place(sx_ctx *ctx, const uint64_t *d_vbase, uint32_t groups, uint32_t gsize, uint32_t n_rec, sx_approx_hit *d_dst, uint64_t n_dst,
                           uint32_t *d_err);

// ---- sx_best.hip: best-stratum search -----------------------------------------------------------
// What a batch of the round loop holds on the device; sized once (init) for the largest batch, nothing is allocated in a round
struct sx_best_state {
    sx_dev_scope own;
    uint32_t cap_count = 0, n_rec = 0, rounds = 0; // patterns a batch may have, records, rounds (max_edits + 1)
    uint64_t cap_bytes = 0, fstride = 0;           // bytes a batch may have; entries of a record's found-set hit offsets
    uint8_t *d_stratum = nullptr;                  // (unless the caller brings its own) a byte a group
    uint8_t *d_keep_found = nullptr, *d_keep_open = nullptr;
    uint8_t *d_open[2] = {nullptr, nullptr}, *d_found = nullptr; // compacted pattern sets: the open one of the next round, the found ones
    uint32_t *d_open_off[2] = {nullptr, nullptr}, *d_open_ids[2] = {nullptr, nullptr}, *d_found_off = nullptr, *d_found_ids = nullptr;
    uint32_t *d_rel_found = nullptr, *d_rel_open = nullptr; // a select's ids inside its input set
    uint64_t *d_fho = nullptr, *d_seg = nullptr;   // hit offsets of the found sets (round, record); the segments' starts
    uint32_t *d_err = nullptr;
    // the batch in flight (host): round d's found set is entries [fbase[d], fbase[d + 1]) of d_found_ids
    uint32_t fbase[SX_APPROX_MAX_EDITS + 2] = {0};
    std::vector<uint64_t> seg; // rounds x records + 1: where (round, record)'s hits start in the room
    int init(sx_ctx *ctx, uint32_t count_max, uint64_t bytes_max, uint32_t n_records, int max_edits, bool own_stratum);
};
// one batch of patterns against the records
struct sx_best_batch {
    const sx_index_rec *recs;
    uint32_t n_rec;
    const uint8_t *d_tabs; // a 256-byte symbol table a record, or null: the patterns hold symbols already
    uint8_t *d_pat;        // (with d_tabs) room for the remapped bytes of any set of the batch, indexed like d_bytes
    const uint8_t *d_bytes;
    uint64_t bytes_total;  // d_bytes is readable in [0, bytes_total)
    const uint32_t *d_off; // count + 1 offsets into d_bytes; [p_lo, p_hi): the batch's bytes
    uint64_t p_lo, p_hi;
    uint32_t count, gsize; // patterns; patterns a group (1, or 2: both strands of a read)
    int k;
    uint32_t search_flags; // SX_SEARCH_*: the strata and the hits are those of the search with these flags
    uint64_t *d_ho;        // n_rec x ho_stride entries of scratch (the count passes' hit offsets), ho_stride >= count + 1
    uint64_t ho_stride;
    uint8_t *d_stratum;    // a byte a group
    sx_approx_hit *d_raw;  // the room: hits as segments (round, record); null: nothing is emitted
    uint64_t raw_cap;
    bool go_on_counting;   // more hits than raw_cap: the rounds go on without emitting (else they end there)
};
// The rounds d = 0 .. k.  *total_out <- the hits (with SX_E_CAPACITY and !go_on_counting: those known of so far).
// SX_E_CAPACITY: the room is too small; the strata and (go_on_counting) the found sets' offsets are complete all the same
int sx_best_rounds(sx_ctx *ctx, sx_best_state &S, const sx_best_batch &B, uint64_t *total_out);
// d_vbase (count x n_rec + 1 entries) <- where the hits of (pattern, record) start in (pattern, record, hit) order and,
// last, the total; with d_placed the room's hits go there in that order, query <- pattern x n_rec + record.
// unmapped (SX_MAP_UNMAPPED, with d_placed): every group without a hit gets its placeholder in that order too (d_placed
// has room for total + count / gsize entries) and *placed_out <- the entries placed
int sx_best_place(sx_ctx *ctx, sx_best_state &S, const sx_best_batch &B, uint64_t total, uint64_t *d_vbase, sx_approx_hit *d_placed, bool unmapped = false,
                  uint64_t *placed_out = nullptr);
