// sx_sam.hpp -- what the read mapper's loop (sx_map.hip) uses of the SAM text (sx_sam.hip): the kernels' view of a batch of
// hits, its layout and the emit of a window.
#pragma once
#include "sx_common.hpp"

namespace sx {

struct SamArgs {
    const uint4 *hits; // sx_approx_hit as two 16-byte words
    uint64_t n_hits;
    const uint32_t *sa;
    uint64_t sa_len;
    const uint32_t *const *sa_list; // one suffix array per record rank (then sa is not used)
    const uint64_t *sa_len_list;
    const uint8_t *names, *seqs, *quals;
    const uint32_t *name_off, *seq_off, *qual_off;
    uint32_t n_reads;
    const uint8_t *rnames;
    const uint32_t *rname_off;
    uint32_t n_records;
    // an index with a sampled suffix array (the kernels' kLocated form): the positions of a run of hits, located before
    // the layout; hit h's stand at positions[pos_off[h] - pos_base ..)
    const uint32_t *positions;
    const uint64_t *pos_off;
    uint64_t pos_base;
    const uint16_t *flags; // a FLAG per read (the kernels' kFlags form), or null: every line has FLAG 0
};

// The same with what NM:i and MD:Z behind QUAL are made of (the kernels' kTags form), or both null:
// per record rank the address of its remapped text (as many bytes as its suffix array has entries, the sentinel last) and
// a 256-byte table, the letter behind every code.  The kernels without tags take the SamArgs part alone, as they did
// before there were tags.
struct SamTagArgs : SamArgs {
    const uint8_t *const *text_list = nullptr;
    const uint8_t *letters = nullptr;
};

// The same with a 16-bit quality word a hit (the kernels' kMapq form): its low 8 bits are the MAPQ of
// every line of the hit, its bit 8 puts 256 on top of their FLAG.  The other kernels take the parts above alone.
struct SamMapqArgs : SamTagArgs {
    const uint16_t *quality = nullptr;
};

// d_byte_off[h] (n_hits + 1 entries) <- the first output byte of hit h's lines, the last entry and *total_out <- the
// text's length.  unmapped (SX_MAP_UNMAPPED): a hit with R == L is a read group's placeholder and
// prints the FLAG 4 line of its read (kernels of their own; without it a hit with R == L prints nothing)
// quality (SX_MAP_MAPQ): a quality word a hit, or null; with it the kernels are the kMapq forms, which
// print placeholders whatever `unmapped` says
int sam_layout(sx_ctx *ctx, const SamTagArgs &A, uint64_t *d_byte_off, uint64_t *total_out, bool unmapped = false, const uint16_t *quality = nullptr);
// bytes [lo, hi) of the text to d_out (asynchronous: the caller syncs)
int sam_emit(sx_ctx *ctx, const SamTagArgs &A, const uint64_t *d_byte_off, uint64_t lo, uint64_t hi, uint8_t *d_out, bool unmapped = false,
             const uint16_t *quality = nullptr);

// Lines with a mate: the text of n_lines line descriptors over A's hits, reads and records (A's suffix
// arrays, positions and flags are not read: a descriptor has its POS and its FLAG).  d_byte_off[j] (n_lines + 1 entries) <-
// the first output byte of line j, the last entry and *total_out <- the text's length
int sam_layout_pairs(sx_ctx *ctx, const SamArgs &A, const sx_pair_line *d_lines, uint64_t n_lines, uint64_t *d_byte_off, uint64_t *total_out);
// bytes [lo, hi) of that text to d_out (asynchronous: the caller syncs)
int sam_emit_pairs(sx_ctx *ctx, const SamArgs &A, const sx_pair_line *d_lines, uint64_t n_lines, const uint64_t *d_byte_off, uint64_t lo,
                   uint64_t hi, uint8_t *d_out);

} // namespace sx
