// sx_index.hpp -- the device-resident index (sx_index.hip) and what the mapper's loop (sx_sam.hip) reads of it.
#pragma once
#include "sx_common.hpp"
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
    // record (an array of sx::LocRec, sx_locate.hpp)
    uint8_t *d_rnames = nullptr, *d_tabs = nullptr;
    void *d_loc_list = nullptr;
    uint32_t *d_rname_off = nullptr;
    const uint32_t **d_sa_list = nullptr;
    uint64_t *d_sa_lens = nullptr;
    size_t view_bytes = 0;
};

// the reads of one call on the device; h_seq_off: the host's copy of d_seq_off, or null (the loop then reads the two
// entries a batch needs back)
struct sx_reads_dev {
    uint32_t count = 0;
    const uint8_t *d_names = nullptr, *d_seqs = nullptr, *d_quals = nullptr;
    const uint32_t *d_name_off = nullptr, *d_seq_off = nullptr, *d_qual_off = nullptr;
    const uint32_t *h_seq_off = nullptr;
    uint64_t name_bytes = 0, seq_bytes = 0, qual_bytes = 0; // the offsets' last entries
};

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

// sx_sam.hip: the mapper's loop over reads and an index that both lie on ctx's device
// (flags: those of sx_map_reads_stream_ex)
int sx_map_reads_core(sx_ctx *ctx, const sx_index *idx, const sx_reads_dev &reads, int edits, uint32_t flags, sx_sink_fn sink, void *user);
// sx_approx.hip: sx_bwt_approx_search_dev over the tables of a record, full, compact or packed
int sx_approx_search_record(sx_ctx *ctx, const sx_index_rec &R, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t count, int max_edits,
                            uint64_t *d_hit_offsets, sx_approx_hit *d_hits, uint64_t hit_capacity, uint64_t *total_hits_out);
