/*
 * stralg_amd.h -- C-ABI of the MI355X suffix-array / BWT-table construction
 * path (libstralg_amd.so).  Plain pointers and sizes only.
 *
 * These are the device-side entry points that stralg's own constructors bind
 * (include/stralg_compat.h declares the reference-named wrappers on top):
 *
 *   sx_sa_build      replaces the body of  sa_is_construction      stralg/sa_is.c:466-509
 *                                          sa_is_mem_construction  stralg/sa_is_mem.c:471-494
 *                                          skew_sa_construction    stralg/skew.c:388-395
 *   sx_bwt_tables    replaces the C/O/RO loops of init_bwt_table   stralg/bwt.c:35-88
 *
 * Every function returns 0 on success or a non-zero code (HIP error number,
 * or one of SX_E_*); sx_last_error() gives the text.  There is no CPU
 * fallback: without a usable GPU the calls fail.
 */
#ifndef STRALG_AMD_H
#define STRALG_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sx_ctx sx_ctx;

enum {
    SX_OK = 0,
    SX_E_ARG = -1,     /* malformed argument (symbol >= alphabet_size, interior 0, n too large) */
    SX_E_NOMEM = -2,   /* host allocation failed */
    SX_E_INTERNAL = -3, /* a device-side invariant did not hold */
    SX_E_MALFORMED = -4, /* a FASTA image that ends inside a header line (bioinf/fasta.c:121-124 MALFORMED_FILE) */
    SX_E_CAPACITY = -5   /* more results than the caller's buffer holds (the count is reported all the same) */
};

/* Kernel classes for the in-library HIP-event profiler (bench.py roofline). */
enum {
    SX_KC_CLASSIFY = 0,   /* S/L types, LMS flags, bucket histograms      sa_is.c:134-174 */
    SX_KC_SAMPLES,        /* sample (LMS + cut) flags and compaction                       */
    SX_KC_KEYS,           /* LMS-substring pieces / prefixes -> 64-bit keys sa_is.c:265-292; a sort's first pass when it
                             computes its keys from the text itself (no key kernel) */
    SX_KC_RADIX_HIST,     /* radix sort: per-tile digit histogram                          */
    SX_KC_RADIX_SCATTER,  /* radix sort: stable scatter                                    */
    SX_KC_SCAN,           /* device-wide scans / compactions                               */
    SX_KC_NAMES,          /* names + reduced string                       sa_is.c:295-336 */
    SX_KC_DOUBLING,       /* reduced-string suffix sort (elementwise steps)                */
    SX_KC_INDUCE_GATHER,  /* induce: gather text[SA[i]-1] + per-tile bucket histogram      */
    SX_KC_INDUCE_SCAN,    /* induce: per-bucket offsets                                    */
    SX_KC_INDUCE_SCATTER, /* induce: stable scatter to bucket cursors     sa_is.c:220-263 */
    SX_KC_INDUCE_CHAIN,   /* induce: small rounds, one chained launch (count + look-back + scatter) */
    SX_KC_BWT_GATHER,     /* bwt[i] = text[SA[i]-1] + per-tile symbol counts bwt.c:13-20  */
    SX_KC_OTABLE,         /* O-table rows                                 bwt.c:47-65     */
    SX_KC_MISC,
    SX_KC_FASTA,          /* FASTA image -> packed records                bioinf/fasta.c:92-135 */
    SX_KC_REMAP,          /* presence bits + table lookup                 remap.c:8-31,102-114  */
    SX_KC_LCP,            /* inverse + LCP                                suffix_array.c:53-85  */
    SX_KC_SEARCH,         /* batched exact and k-edit BWT search          bwt.c:164-199, 226-422 */
    SX_KC_LOCAL_SORT,     /* hybrid LMS sort: sub-buckets ordered in LDS, ties listed          */
    SX_KC_SAM,            /* SAM text of search hits: size pass, 64-bit scan, emit  bioinf/sam.c:4-10 */
    SX_KC_PAIR_COUNT,     /* paired reads: the lines of a batch and the proper combinations of every line */
    SX_KC_PAIR_SCAN,      /* paired reads: the 64-bit scans of the lines and of the combinations */
    SX_KC_PAIR_FILL,      /* paired reads: two line descriptors a proper combination               */
    SX_KC_PAIR_LAYOUT,    /* paired reads: bytes of every described line and their scan            */
    SX_KC_PAIR_EMIT,      /* paired reads: the text of a window of described lines                 */
    SX_KC_MAPQ,           /* SX_MAP_MAPQ: the quality pass over a batch's merged hits */
    SX_KC_COUNT
};

typedef struct sx_kernel_stat {
    uint64_t launches;
    double ms;          /* sum of HIP-event durations */
    uint64_t alg_bytes; /* sum of algorithmic bytes (per kernel) */
} sx_kernel_stat;

typedef struct sx_build_stats {
    uint64_t n;              /* symbols without the sentinel */
    uint64_t n_lms;          /* LMS positions incl. the sentinel */
    uint64_t n_samples;      /* LMS positions + cut points = reduced string length */
    uint64_t n_names;        /* distinct piece names */
    uint32_t key_bits;       /* bits per symbol in a piece key */
    uint32_t key_slots;      /* symbols per piece key */
    uint32_t doubling_rounds;
    uint32_t induce_rounds;  /* multisplit rounds over both passes */
    uint32_t sort_passes;    /* radix passes, all sorts */
    uint32_t lms_path;       /* 1: prefix-key LMS sort resolved everything, 2: general path, 3: direct sort of all suffixes */
    uint32_t sort_local;     /* bit 0: the prefix-key sort finished in LDS (hybrid: HBM passes on the top 24 key bits only);
                                bit 1: some workgroup of it met crowded bins and took stable passes; bit 2: HBM passes on the top 32 bits (four);
                                bit 3: its first HBM pass computed the keys from the text (no key kernel) */
    uint32_t refine_tiers;   /* tie refinement of the prefix-key sort: bit 0: some round ordered groups of 9 .. 2048 members in
                                LDS; bit 1: some round sent the members of longer groups through radix sorts; prefix doubling of the
                                general path: bit 2: some round ordered small groups by one wave each, bit 3: some round sent
                                members through radix sorts */
    double ms_total;         /* wall time of the last build on the device stream */
    uint32_t induce_redo;    /* buckets of the induced-sort passes whose rounds the queued launches did not finish (runs longer than
                                the tail kernel's steps reach, more entries alive than it holds): the host carried them on */
    uint32_t long_runs;      /* the classification saw a run that fills a 4096-symbol tile: the passes are attended from the start */
    uint32_t recursion_levels; /* reduced strings over a byte alphabet that were sorted by the pipeline itself, one below the other */
    uint32_t sample_tied_permille; /* 0: no sample was looked at; else 1 + the tied share (per mille) of the sampled suffixes under
                                      the longest prefix key: from 300 on the prefix-key sort is not attempted */
    uint32_t long_subbuckets; /* hybrid prefix-key sort: sub-buckets too long for a workgroup's LDS (repeat families, AT-rich
                                 prefixes) that were ordered by HBM passes of their own */
    uint32_t induce_early_s; /* induced-sort passes over at most 8 buckets: S-type entries that the L pass placed itself, as
                                the predecessors of the L-type entries it was scanning (the S pass did not scan those again) */
} sx_build_stats;

/* ---- context ------------------------------------------------------------ */
int sx_device_count(void);
/* NUMA node of the device's PCI function (/sys/bus/pci/devices/<bus id>/numa_node), or -1 when unknown */
int sx_device_numa_node(int device);
int sx_ctx_create(int device, sx_ctx **out);
void sx_ctx_destroy(sx_ctx *ctx);
/* contexts alive in this process (created minus destroyed) */
int sx_ctx_live_count(void);
const char *sx_last_error(const sx_ctx *ctx);
/* drop cached workspace (it is otherwise kept between calls) */
void sx_ctx_trim(sx_ctx *ctx);
/* behaviour switches (testing / measurement) */
enum {
    SX_FLAG_FORCE_GENERAL_PATH = 1, /* skip the prefix-key LMS sort: always pieces + names + prefix doubling */
    SX_FLAG_CHAIN_MAX_ENTRIES = 2,  /* induce rounds up to this many entries use the single chained launch */
    SX_FLAG_NO_DIRECT_SORT = 3,     /* wide alphabets: never sort all suffixes by prefix directly, always LMS sort + induction */
    SX_FLAG_PREFIX_SYMBOLS = 4,     /* first attempt of the prefix-key sort takes this many symbols (0: by the text's size) */
    SX_FLAG_RADIX_DIGIT_BITS = 5,   /* digit width of the LSD radix passes: 8 (default), 9 or 10 */
    SX_FLAG_SORT_MODE = 6,          /* prefix-key sort: 0 choose, 1 LSD passes only (tie refinement too: no group is ordered in
                                       LDS), 2 hybrid (HBM passes on the top 24 key bits + sub-buckets ordered in LDS) whenever the
                                       key shape allows it, whatever the size, 3 the same with the top 32 bits */
    SX_FLAG_INDUCE_BATCH_OFF = 7,   /* induced-sort passes over at most 8 buckets: 1 = every self round of a bucket is a launch of
                                       its own (no eight-rounds-at-a-time form) */
    SX_FLAG_INDUCE_BATCH_MIN = 8,   /* ranges longer than this many entries take the eight-rounds-at-a-time form (negative: the
                                       default, what the one-workgroup tail kernel holds; tests set 0) */
    SX_FLAG_INDUCE_ATTENDED = 9     /* 0 (default) = the buckets of an induced-sort pass are queued one behind the other; a bucket
                                       whose rounds the tail kernel could not finish leaves word, the launches behind it do nothing,
                                       and the host carries that bucket on before it queues the rest; 1 = attended: the host reads
                                       every bucket's last range back before it queues the next bucket (rounds 1 and 2) */
    ,SX_FLAG_COPY_TEXT_FIRST = 10   /* 1 = the build's padded copy of the text is made by a device copy before the classification
                                       (rounds 1 and 2); 0 = the classification writes it while it reads the caller's text */
    ,SX_FLAG_RECURSE_MIN = 11      /* a reduced string of at most 255 names and at least this many symbols is sorted by the whole
                                       pipeline again (in a child context) instead of by prefix doubling; negative: the default
                                       (2^20); tests set small values */
    ,SX_FLAG_SAMPLE_MIN = 12       /* texts of more than 8 symbols and at least this many suffixes get a look at a sample before a
                                       prefix-key sort (negative: the default, 2^20; tests set small values) */
    ,SX_FLAG_INDUCE_NO_HOIST = 13  /* texts of more than 8 symbols: 1 = every bucket's LMS seeds (L pass) and L-type entries (S pass)
                                       are scanned by launches of the bucket's own, as in rounds 1 - 3; 0 (default) = all buckets'
                                       at once, up front, placed by the text's bigram counts */
    ,SX_FLAG_TEXT_KEYS_OFF = 14    /* the direct sort of all suffixes and the LMS sort of four-letter texts: 1 = a key kernel writes
                                       the keys before the first radix pass (rounds 1 - 3); 0 (default) = the first pass computes them
                                       from the text */
    ,SX_FLAG_LONG_SUBBUCKETS_OFF = 15 /* hybrid prefix-key sort: 1 = a sub-bucket too long for a workgroup makes the whole sort fall
                                       back to plain passes, and texts with skewed symbol counts do not try it (rounds 1 - 3); 0
                                       (default) = such sub-buckets are listed and ordered by HBM passes of their own */
    ,SX_FLAG_SMALL_DIRECT_MAX = 16 /* texts of at most 16 symbols and at most this many suffixes are sorted directly (all suffixes by
                                       prefix key, as wide alphabets are: a third of the launches of classification + LMS sort +
                                       induced passes, which is what a short record's build consists of); 0 = never; negative: the
                                       default (2^24, 2^25, 2^27 suffixes for at most 4, 7, 15 letters) */
    ,SX_FLAG_LOCAL_SORT_LEAN_OFF = 17 /* hybrid prefix-key sort, the step that orders the sub-buckets in LDS: 1 = every workgroup
                                       takes the kernel of rounds 3 and 4 (pairs through LDS, stable passes where equal keys
                                       crowd a bin); 0 (default) = the lean kernel of round 5, which leaves only the workgroups it
                                       cannot finish to that one */
    ,SX_FLAG_SAM_BATCH_READS = 18  /* sx_map_reads_stream: at most this many reads in one search batch (0: the default, 2^20;
                                       tests set small values so that one run takes several batches) */
    ,SX_FLAG_SAM_WINDOW_BYTES = 19 /* sx_map_reads_stream: bytes of SAM text per window, rounded up to 16 (0: the default and the
                                       most, 32 MiB, one pinned staging buffer) */
    ,SX_FLAG_LOCATE_CHUNK_ROWS = 20 /* mapping against an index with a sampled suffix array: the hits of a batch are located and
                                       printed in runs of consecutive hits whose lines fit this many positions (0: the default,
                                       2^28, a buffer of 1 GiB; a single hit with more lines gets a buffer of its own length;
                                       tests set small values) */
    ,SX_FLAG_INDUCE_EARLY_S_OFF = 21 /* induced-sort passes over at most 8 buckets: 1 = the S pass scans every bucket's whole L
                                       region for the S-type predecessors (as before); 0 (default) = the L pass's large rounds
                                       place them while they hold the entries, the S pass scans what those rounds left */
    ,SX_FLAG_SAM_ROOM_HITS = 22    /* read mapping, a test switch: > 0 = the largest room for the hits of a batch's searches, in
                                       hits, in place of what the free memory gives, and the room a call starts with may be as
                                       small as 1 hit (it is 2^16 at least otherwise); 0 (default) = by the free memory.  Tests
                                       set small values so that the room grows and batches are halved (sx_map_last_stats) */
    ,SX_FLAG_CHAIN_EPOCH = 23      /* a test switch: the look-back epoch of the context, and of its child context if it has one,
                                       becomes this value (0 .. 2^24 - 1; the next chained launch takes the one after it, and the
                                       status words are retired where the 24 bits wrap) */
    ,SX_FLAG_READBACK_SEQ = 24     /* a test switch: the value, taken as a 32-bit pattern, becomes the sequence number of the last
                                       read-back, in the context and (after a wait for the stream) in the word of the pinned page
                                       that holds it, so that the page still holds the last sequence number */
    ,SX_FLAG_PAIRS_ROOM_LINES = 25 /* paired reads, a test switch: > 0 = the lines, and the line descriptors, that a batch of
                                       several pairs may have before it is halved, in place of what the free memory gives (and
                                       of SX_FLAG_SAM_ROOM_HITS, which sets it as well where this one is 0); the hits' room
                                       is left as it is.  0 (default) = by the free memory */
};
int sx_ctx_set_flag(sx_ctx *ctx, int flag, int value);

/* Test hooks: what a context carries from one call to the next ("What a context carries from call to call").
 *
 * sx_ctx_scribble waits for the stream and then overwrites everything a later call must not rely on: the whole capacity
 * of the workspace slabs 0 .. 5 and the pinned staging buffers (where they exist) with `byte`, words 0 .. 1023 of the
 * read-back page likewise (the sequence word behind them is left alone).  The slab of look-back status words is filled
 * within its invariant, which is stronger than arbitrary bytes: every header word becomes non-zero, every status word a
 * ready inclusive prefix of the last launch's epoch with the value 0xEEEEEEEE -- the worst a past launch can have left, and
 * never an epoch above the context's.  The child context, if there is one, gets the same.  `byte`: 0 .. 255.
 *
 * sx_ctx_counters reads the counters back; chain_slab_max_epoch is the largest epoch field among the status words, by a
 * copy of the slab to the host (slow). */
typedef struct sx_ctx_counts {
    uint32_t chain_epoch;          /* the epoch of the last chained launch (24 bits) */
    uint32_t readback_seq;         /* the sequence number of the last read-back */
    uint32_t chain_slab_max_epoch; /* the largest epoch field in the status words (0: no slab, or nothing but zeros) */
    uint32_t has_child;            /* whether a child context exists; its counters follow, zeros where there is none */
    uint64_t slab_bytes[7];        /* the capacity of every workspace slab */
    uint32_t child_chain_epoch, child_readback_seq, child_chain_slab_max_epoch, child_reserved;
    uint64_t child_slab_bytes[7];
} sx_ctx_counts;
int sx_ctx_scribble(sx_ctx *ctx, int byte);
int sx_ctx_counters(const sx_ctx *ctx, sx_ctx_counts *out);

/* ---- suffix array -------------------------------------------------------- */
/* Host buffers.  text[0..n) holds symbols in [1, alphabet_size), alphabet_size
 * <= 256; sa_out receives n+1 entries (sa_out[0] == n, the sentinel suffix).
 * Unlike sort_SA's shortcut (sa_is.c:423-428) the result is the true suffix
 * array for any alphabet_size that bounds the symbols. */
int sx_sa_build(sx_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t alphabet_size,
                uint32_t *sa_out);
/* Device buffers (inputs resident in HBM); d_text has n bytes, d_sa_out n+1 entries. */
int sx_sa_build_dev(sx_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t alphabet_size,
                    uint32_t *d_sa_out);

/* Suffix array and BWT in one build: the induced-sort passes carry text[SA[i]-1]
 * with every entry, so the BWT costs no extra gather.  d_bwt_out has n+1 bytes. */
int sx_sa_bwt_build_dev(sx_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t alphabet_size,
                        uint32_t *d_sa_out, uint8_t *d_bwt_out);

/* ---- BWT tables ------------------------------------------------------------ */
/* text[0..N-1) symbols in [1, sigma) (N = n+1 counts the sentinel), sa[N].
 * c_out[sigma]; o_out[(N+1)*sigma] position-major: o_out[i*sigma + a] = O(a,i).
 * o_out may be NULL (C table only).  sigma <= 128 as in stralg/remap.h:14-18. */
int sx_bwt_tables(sx_ctx *ctx, const uint8_t *text, const uint32_t *sa, uint64_t N,
                  uint32_t sigma, uint32_t *c_out, uint32_t *o_out);
/* Device buffers; d_bwt_out (N bytes) is optional. */
int sx_bwt_tables_dev(sx_ctx *ctx, const uint8_t *d_text, const uint32_t *d_sa, uint64_t N,
                      uint32_t sigma, uint32_t *d_c_out, uint32_t *d_o_out, uint8_t *d_bwt_out);

/* C/O tables from a BWT already on the device (pairs with sx_sa_bwt_build_dev). */
int sx_bwt_tables_from_bwt_dev(sx_ctx *ctx, const uint8_t *d_bwt, uint64_t N, uint32_t sigma,
                               uint32_t *d_c_out, uint32_t *d_o_out);
/* build_complete_table's device work in one call (stralg/bwt.c:134-161): host text ->
 * suffix array (sa_out, n+1 entries, may be NULL), C table, O table (may be NULL). */
int sx_build_tables(sx_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t sigma, uint32_t *sa_out,
                    uint32_t *c_out, uint32_t *o_out);

/* ---- consumers of a resident suffix array / table (SURVEY.md section 8f "next") ------------ */
/* stralg/suffix_array.c:53-60 compute_inverse: inv[sa[i]] = i. */
int sx_sa_inverse_dev(sx_ctx *ctx, const uint32_t *d_sa, uint64_t N, uint32_t *d_inv_out);
/* stralg/suffix_array.c:62-85 compute_lcp: lcp[0] = 0, lcp[j] = lcp(suffix sa[j-1], suffix sa[j]).
 * d_text has N-1 bytes; d_inv_out (N entries) is optional and receives the inverse. */
int sx_sa_lcp_dev(sx_ctx *ctx, const uint8_t *d_text, const uint32_t *d_sa, uint64_t N, uint32_t *d_inv_out,
                  uint32_t *d_lcp_out);
/* host buffers; inv_out or lcp_out may be NULL (not both) */
int sx_sa_inverse_lcp(sx_ctx *ctx, const uint8_t *text, const uint32_t *sa, uint64_t N, uint32_t *inv_out,
                      uint32_t *lcp_out);
/* stralg/bwt.c:164-199 init_bwt_exact_match_iter for `count` patterns at once: pattern q is
 * d_patterns[d_offsets[q] .. d_offsets[q+1]) (remapped symbols); the matches of q are
 * sa[l_out[q] .. r_out[q]) (empty when l_out[q] >= r_out[q]).  Tables as sx_bwt_tables_dev writes them. */
int sx_bwt_exact_search_dev(sx_ctx *ctx, const uint32_t *d_c_table, const uint32_t *d_o_table, uint64_t N,
                            uint32_t sigma, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t count,
                            uint32_t *d_l_out, uint32_t *d_r_out);

/* stralg/bwt.c:226-422 init_bwt_approx_iter / next_bwt_approx_match for `count` patterns at once, at most max_edits
 * edits (mismatch, insertion I, deletion D).  One hit is one interval of the reference iterator's list: the matches
 * sa[L], sa[L+1], ..., sa[R-1], each with match_length and the CIGAR of the hit.  Matches and mismatches are both 'M'
 * in the reference's CIGARs, so a hit's CIGAR is fixed by its I/D operations: gap[j] (j < n_gaps, ascending) is the
 * index of the j-th I/D in the edit string in pattern order (low 15 bits; the edit string has pattern length + the
 * number of D symbols) and SX_APPROX_GAP_D set for a D.  Render it as runs of equal operations, "%d%c" each
 * (cigar.c edits_to_cigar). */
#define SX_APPROX_MAX_EDITS 8
#define SX_APPROX_GAP_D 0x8000u
typedef struct sx_approx_hit {
    uint32_t query;        /* pattern number */
    uint32_t L, R;         /* interval of the suffix array, L < R */
    uint16_t match_length; /* symbols of the text the pattern is aligned to */
    uint16_t n_gaps;       /* I/D operations (<= max_edits) */
    uint16_t gap[SX_APPROX_MAX_EDITS];
} sx_approx_hit; /* 32 bytes */
/* Patterns as in sx_bwt_exact_search_dev; tables as sx_bwt_tables_dev writes them; d_ro_table (the reversed text's
 * O table, build_complete_table(.., true)) feeds the reference's D table, NULL: a D table of zeros (bwt.c:319-338).
 * The hits of pattern q are d_hits[d_hit_offsets[q] .. d_hit_offsets[q+1]) in the reference's order (a depth-first
 * search from the pattern's last symbol; children M over a = 1 .. sigma-1, I, D over a = 1 .. sigma-1; no D at the
 * root); identical from run to run.  d_hit_offsets (count + 1 entries) and *total_hits_out are always written; more
 * than hit_capacity hits: no hit is written and the call returns SX_E_CAPACITY; d_hits == NULL: count only.
 * d_hits 16-byte aligned.  Limits: max_edits <= SX_APPROX_MAX_EDITS, every pattern length + max_edits < 2^15, fewer
 * than 2^32 hits in one call (else SX_E_ARG); max_edits < 0: no hits.  A pattern that is empty or holds a symbol 0 or
 * >= sigma has no hits (the reference asserts or reads out of bounds there). */
int sx_bwt_approx_search_dev(sx_ctx *ctx, const uint32_t *d_c_table, const uint32_t *d_o_table,
                             const uint32_t *d_ro_table, uint64_t N, uint32_t sigma, const uint8_t *d_patterns,
                             const uint32_t *d_offsets, uint32_t count, int max_edits, uint64_t *d_hit_offsets,
                             sx_approx_hit *d_hits, uint64_t hit_capacity, uint64_t *total_hits_out);
/* Search flags.  SX_SEARCH_NO_INDELS: mismatches only.  The hits of pattern q are those of the call
 * without the flag at the same max_edits whose n_gaps is 0, in the same order: the intervals of the strings at Hamming
 * distance <= max_edits from the pattern that occur in the text, each once, depth first from the last symbol with the
 * children M over a = 1 .. sigma-1.  Every hit has match_length = the pattern's length, n_gaps = 0 and gap[] all zero.  The
 * D table is the same one (NULL RO: zeros) and the result does not depend on it.  Limits, the count-only form,
 * SX_E_CAPACITY, the patterns without hits and the identity from run to run are those of the plain call.  search_flags
 * == 0: the plain call, launch for launch; unknown bits: SX_E_ARG.  The _ex forms below and of the compact, packed,
 * best-stratum and host-buffer calls take the flags as their last argument; the calls without it pass 0. */
enum { SX_SEARCH_NO_INDELS = 1 };
int sx_bwt_approx_search_dev_ex(sx_ctx *ctx, const uint32_t *d_c_table, const uint32_t *d_o_table, const uint32_t *d_ro_table,
                                uint64_t N, uint32_t sigma, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t count,
                                int max_edits, uint64_t *d_hit_offsets, sx_approx_hit *d_hits, uint64_t hit_capacity,
                                uint64_t *total_hits_out, uint32_t search_flags);
/* The same over host buffers: the tables and patterns are uploaded (the whole O / RO tables, (N+1) x sigma words each,
 * once per call), hit_offsets (host, count + 1) is filled, *hits_out receives a malloc'd array of *total_hits_out hits
 * (NULL when there are none) that the caller releases with free(). */
int sx_bwt_approx_search(sx_ctx *ctx, const uint32_t *c_table, const uint32_t *o_table, const uint32_t *ro_table,
                         uint64_t N, uint32_t sigma, const uint8_t *patterns, const uint32_t *offsets, uint32_t count,
                         int max_edits, uint64_t *hit_offsets, sx_approx_hit **hits_out, uint64_t *total_hits_out);
int sx_bwt_approx_search_ex(sx_ctx *ctx, const uint32_t *c_table, const uint32_t *o_table, const uint32_t *ro_table, uint64_t N,
                            uint32_t sigma, const uint8_t *patterns, const uint32_t *offsets, uint32_t count, int max_edits,
                            uint64_t *hit_offsets, sx_approx_hit **hits_out, uint64_t *total_hits_out, uint32_t search_flags);
/* Best stratum: sx_bwt_approx_search_dev by iterative deepening.  d_stratum[q] (count bytes) <-
 * e*(q), the smallest d in 0 .. max_edits at which pattern q has a hit, or 0xFF where it has none; the hits of pattern q
 * are exactly, and in the order of, those of sx_bwt_approx_search_dev at max_edits = d_stratum[q] (query = q), so every
 * one of them uses exactly e*(q) edits.  Arguments, limits, the count-only form (d_hits == NULL) and the order of the
 * output are those of sx_bwt_approx_search_dev; on SX_E_CAPACITY the offsets, the strata and the total are written all
 * the same; max_edits < 0: no hits, every stratum 0xFF.  The same from run to run. */
int sx_bwt_best_search_dev(sx_ctx *ctx, const uint32_t *d_c_table, const uint32_t *d_o_table, const uint32_t *d_ro_table,
                           uint64_t N, uint32_t sigma, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t count,
                           int max_edits, uint8_t *d_stratum, uint64_t *d_hit_offsets, sx_approx_hit *d_hits,
                           uint64_t hit_capacity, uint64_t *total_hits_out);
/* the same over the search with search_flags: with SX_SEARCH_NO_INDELS e*(q) is the smallest Hamming distance in 0 ..
 * max_edits at which pattern q occurs, and its hits are those of sx_bwt_approx_search_dev_ex with the flag at e*(q) */
int sx_bwt_best_search_dev_ex(sx_ctx *ctx, const uint32_t *d_c_table, const uint32_t *d_o_table, const uint32_t *d_ro_table,
                              uint64_t N, uint32_t sigma, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t count,
                              int max_edits, uint8_t *d_stratum, uint64_t *d_hit_offsets, sx_approx_hit *d_hits,
                              uint64_t hit_capacity, uint64_t *total_hits_out, uint32_t search_flags);
/* The patterns q with d_keep[q] != 0 (count bytes), in order and flat: kept pattern j has its bytes at
 * d_bytes_out[d_off_out[j] .. d_off_out[j+1]) with d_off_out[0] = 0, and d_ids_out[j] is its number in the input.
 * d_off (count + 1 entries) need not start at 0; d_bytes is readable up to d_off[count].  d_bytes_out holds
 * d_off[count] - d_off[0] + 16 bytes and is 16-byte aligned: the 16 bytes behind the kept ones are zeros.  d_off_out
 * has count + 1, d_ids_out count entries.  *count_out, *bytes_out <- the kept patterns and their bytes.  Offsets that
 * do not ascend give wrong bytes or SX_E_ARG, never an access outside the arrays.  No atomics: the same bytes from run
 * to run. */
int sx_patterns_select_dev(sx_ctx *ctx, const uint8_t *d_bytes, const uint32_t *d_off, uint32_t count, const uint8_t *d_keep,
                           uint8_t *d_bytes_out, uint32_t *d_off_out, uint32_t *d_ids_out, uint32_t *count_out,
                           uint64_t *bytes_out);

/* ---- streaming download (serialisation without a host copy of the tables) ---- */
/* sink(user, section, data, bytes): consecutive chunks of one section after the other; data is only valid
 * during the call; a non-zero return aborts the build. */
typedef int (*sx_sink_fn)(void *user, int section, const void *data, size_t bytes);
enum { SX_SECTION_SA = 0, SX_SECTION_C = 1, SX_SECTION_O = 2, SX_SECTION_SAM = 3 /* sx_map_reads_stream */,
       SX_SECTION_INDEX = 4 /* sx_index_write */ };
/* sx_build_tables, but the suffix array (when want_sa), the C table and the O table leave the device through
 * `sink` in 32 MiB chunks from pinned staging memory, in this order (the order of stralg/serialise.c:7-18 around
 * the remap table); the copy of a chunk overlaps the sink's work on the previous one. */
int sx_build_tables_stream(sx_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t sigma, int want_sa, sx_sink_fn sink,
                           void *user);

/* ---- the read mapper's output on the device (tools/readmappers/bwt_readmapper/bwt_readmapper.c) ---------------- */
/* One batch of hits and what their SAM lines are made of; every pointer is device memory.  Hit h prints, for
 * i = L .. R-1 ascending, the line of bioinf/sam.c print_sam_line
 *     <qname>\t0\t<rname>\t<sa[i]+1>\t0\t<cigar>\t*\t0\t0\t<seq>\t<qual>\n
 * with read = query / n_records and record rank = query % n_records (n_records == 1: query is the read, as
 * sx_bwt_approx_search_dev leaves it).  Read q has its name at d_names[d_name_off[q] .. d_name_off[q+1]), sequence and
 * quality alike (raw bytes, n_reads + 1 offsets each; the pattern length of the CIGAR is the sequence's length); record
 * rank r has its name at d_rnames[d_rname_off[r] .. d_rname_off[r+1]).  The suffix array is d_sa (sa_len entries) for
 * every record, or, when d_sa_list is given, d_sa_list[r] with d_sa_len_list[r] entries for rank r.  The CIGAR is
 * rendered from gap[] as approx_cigar / cigar.c edits_to_cigar do (at most 80 bytes; 8 gaps need 70). */
typedef struct sx_sam_batch {
    const sx_approx_hit *d_hits; /* 16-byte aligned */
    uint64_t n_hits;
    const uint32_t *d_sa;
    uint64_t sa_len;
    const uint32_t *const *d_sa_list;
    const uint64_t *d_sa_len_list;
    const uint8_t *d_names, *d_seqs, *d_quals;
    const uint32_t *d_name_off, *d_seq_off, *d_qual_off;
    uint32_t n_reads;
    const uint8_t *d_rnames;
    const uint32_t *d_rname_off;
    uint32_t n_records;
} sx_sam_batch;
/* Size pass and 64-bit scan: d_byte_offsets[h] (n_hits + 1 entries) <- the first output byte of hit h's lines,
 * d_byte_offsets[n_hits] and *total_bytes_out <- the length of the text.  SX_E_ARG when a hit's query or interval lies
 * outside the batch. */
int sx_sam_layout_dev(sx_ctx *ctx, const sx_sam_batch *batch, uint64_t *d_byte_offsets, uint64_t *total_bytes_out);
/* Bytes [byte_lo, byte_hi) of the text (byte_hi <= total_bytes) to d_out[0 .. byte_hi - byte_lo), d_out 16-byte
 * aligned.  Windows may cut lines anywhere; the concatenation of consecutive windows is the text, and it is the same
 * from run to run. */
int sx_sam_emit_dev(sx_ctx *ctx, const sx_sam_batch *batch, const uint64_t *d_byte_offsets, uint64_t total_bytes, uint64_t byte_lo,
                    uint64_t byte_hi, uint8_t *d_out);
/* The same with a FLAG per read: d_read_flags[q] (device memory, n_reads entries, indexed like d_name_off) is printed in
 * decimal as the second field of every line of read q; NULL: every line has FLAG 0, the calls are sx_sam_layout_dev and
 * sx_sam_emit_dev and give their bytes. */
typedef struct sx_sam_batch_ex {
    sx_sam_batch batch;
    const uint16_t *d_read_flags;
} sx_sam_batch_ex;
int sx_sam_layout_dev_ex(sx_ctx *ctx, const sx_sam_batch_ex *batch, uint64_t *d_byte_offsets, uint64_t *total_bytes_out);
int sx_sam_emit_dev_ex(sx_ctx *ctx, const sx_sam_batch_ex *batch, const uint64_t *d_byte_offsets, uint64_t total_bytes, uint64_t byte_lo,
                       uint64_t byte_hi, uint8_t *d_out);
/* The same with two optional fields between QUAL and the newline of every line:
 *     ...<seq>\t<qual>\tNM:i:<nm>\tMD:Z:<md>\n
 * d_text_list[r] (device memory, n_records addresses) is the remapped text of record rank r, as many bytes as its suffix
 * array has entries with the sentinel last; d_letters (n_records x 256 bytes) has at [r * 256 + c] the letter behind code c
 * of rank r.  NM and MD are those of the line's POS, CIGAR and SEQ over the record's letters: the CIGAR is walked from POS - 1;
 * an M step with equal bytes extends the match run, one with unequal bytes prints "<run><letter of the text>", sets the run
 * to 0 and adds 1 to NM; an I run adds its length to NM; a D run prints "<run>^<the deleted letters>", sets the run to 0 and
 * adds its length to NM; the last run is printed at the end, so MD begins and ends with a number.  Bytes are compared as they
 * are.  The fields are rendered once per hit, from the window at its first position (every row of a hit of the search is a
 * suffix with the same first match_length symbols); a search of at most 8 operations gives one digit of NM and at most 61
 * bytes of MD.  SX_E_ARG from the layout, as for a hit outside the batch: a hit with a line whose window does not lie in
 * front of the record's sentinel, or whose walk finds more than SX_APPROX_MAX_EDITS differences.
 * d_positions / d_pos_off (both or neither): the hits' positions located beforehand, as the mapper has them of a sampled
 * suffix array -- hit h prints d_positions[d_pos_off[h] - pos_base + i] + 1, i = 0 .. R - L - 1, and no suffix array is
 * read (the lengths of d_sa_len_list, or sa_len, still bound R and give the texts' lengths). */
typedef struct sx_sam_batch_tags {
    sx_sam_batch_ex ex;
    const uint8_t *const *d_text_list;
    const uint8_t *d_letters;
    const uint32_t *d_positions;
    const uint64_t *d_pos_off;
    uint64_t pos_base;
} sx_sam_batch_tags;
int sx_sam_layout_dev_tags(sx_ctx *ctx, const sx_sam_batch_tags *batch, uint64_t *d_byte_offsets, uint64_t *total_bytes_out);
int sx_sam_emit_dev_tags(sx_ctx *ctx, const sx_sam_batch_tags *batch, const uint64_t *d_byte_offsets, uint64_t total_bytes, uint64_t byte_lo,
                         uint64_t byte_hi, uint8_t *d_out);
/* The emitter of SX_MAP_UNMAPPED: the batch of sx_sam_batch_tags, d_text_list and d_letters both or
 * neither (neither: no tags), and a hit with R == L is the placeholder of a read that has no line: it prints
 *     <qname>\t4\t*\t0\t0\t*\t*\t0\t0\t<seq>\t<qual>\n
 * of the read of its query (no position, CIGAR, NM or MD; FLAG 4 whatever d_read_flags says).  Every other hit prints its
 * lines as the calls above do. */
int sx_sam_layout_dev_unmapped(sx_ctx *ctx, const sx_sam_batch_tags *batch, uint64_t *d_byte_offsets, uint64_t *total_bytes_out);
int sx_sam_emit_dev_unmapped(sx_ctx *ctx, const sx_sam_batch_tags *batch, const uint64_t *d_byte_offsets, uint64_t total_bytes, uint64_t byte_lo,
                             uint64_t byte_hi, uint8_t *d_out);
/* The emitter of SX_MAP_MAPQ: the batch of sx_sam_layout_dev_unmapped (d_text_list and d_letters both
 * or neither; a hit with R == L is a placeholder and prints its FLAG 4 line) and a 16-bit quality word a hit, d_hit_quality[h]
 * (device memory, n_hits entries, indexed like d_hits): its low 8 bits are the MAPQ, printed in decimal where the "0" behind
 * POS stands on every line of hit h; its bit 8 set means every line of the hit has 256 added to its FLAG (d_read_flags, or 0
 * where that is NULL).  A placeholder's quality word is ignored: its line is the one above, with MAPQ 0.  A NULL
 * d_hit_quality answers SX_E_ARG. */
typedef struct sx_sam_batch_mapq {
    sx_sam_batch_tags tags;
    const uint16_t *d_hit_quality;
} sx_sam_batch_mapq;
int sx_sam_layout_dev_mapq(sx_ctx *ctx, const sx_sam_batch_mapq *batch, uint64_t *d_byte_offsets, uint64_t *total_bytes_out);
int sx_sam_emit_dev_mapq(sx_ctx *ctx, const sx_sam_batch_mapq *batch, const uint64_t *d_byte_offsets, uint64_t total_bytes, uint64_t byte_lo,
                         uint64_t byte_hi, uint8_t *d_out);

/* Lines with a mate.  A line descriptor names a hit of the batch (its read, record, CIGAR, SEQ and QUAL
 * are the hit's) and carries what the hit does not say: line j prints
 *     <qname>\t<flag>\t<rname>\t<pos>\t0\t<cigar>\t=\t<pnext>\t<tlen>\t<seq>\t<qual>\n
 * with pos, pnext and flag in decimal as they stand in the descriptor (pos is the 1-based POS itself: no suffix array is
 * read) and tlen as a signed decimal.  d_lines is device memory, 4-byte aligned, n_lines entries; batch.d_sa / d_sa_list
 * may be NULL.  Layout: d_byte_offsets[j] (n_lines + 1 entries) <- the first output byte of line j, the last entry and
 * *total_bytes_out <- the text's length; SX_E_ARG when a descriptor's hit lies outside the batch.  Emit: a window of the
 * text, as sx_sam_emit_dev; the same bytes from run to run. */
typedef struct sx_pair_line {
    uint32_t hit;   /* index into batch.d_hits */
    uint32_t pos;   /* POS */
    uint32_t pnext; /* PNEXT */
    int32_t tlen;   /* TLEN */
    uint32_t flag;  /* FLAG (< 65536) */
} sx_pair_line; /* 20 bytes */
int sx_sam_layout_dev_pairs(sx_ctx *ctx, const sx_sam_batch *batch, const sx_pair_line *d_lines, uint64_t n_lines, uint64_t *d_byte_offsets,
                            uint64_t *total_bytes_out);
int sx_sam_emit_dev_pairs(sx_ctx *ctx, const sx_sam_batch *batch, const sx_pair_line *d_lines, uint64_t n_lines, const uint64_t *d_byte_offsets,
                          uint64_t total_bytes, uint64_t byte_lo, uint64_t byte_hi, uint8_t *d_out);

/* A FASTQ image indexed on the host (one pass of memchr over the file): read q's name is names[name_off[q] ..
 * name_off[q+1]), its sequence seqs[seq_off[q] ..), its quality quals[qual_off[q] ..): the raw bytes of the record's
 * first line behind '@' (blanks stay), of its second and of its fourth line; the third line is dropped
 * (bioinf/fastq.c:17-35).  A file without a final newline is fine.  Out of contract, where the reference reads a line in
 * pieces or crashes, and answered with SX_E_MALFORMED: a line of 2047 bytes or more, an empty name, sequence or quality
 * line (so also blank lines between or behind the records; the first byte of a record's first line is dropped whatever
 * it is, as the reference does), a record cut off before
 * its fourth line, a NUL byte inside a record; SX_E_ARG: an image of 2^32 - 1 bytes or more.  Release with sx_fastq_free. */
typedef struct sx_fastq {
    uint32_t count;
    uint8_t *names, *seqs, *quals;
    uint32_t *name_off, *seq_off, *qual_off; /* count + 1 entries each */
} sx_fastq;
int sx_fastq_index(const uint8_t *file, size_t len, sx_fastq *out);
void sx_fastq_free(sx_fastq *fq);

/* One genome record of the mapper's list (host pointers): tables as build_complete_table leaves them. */
typedef struct sx_map_record {
    const char *name;          /* NUL-terminated */
    const uint32_t *sa;        /* N entries */
    const uint32_t *c_table;   /* sigma */
    const uint32_t *o_table;   /* (N + 1) x sigma, position-major */
    const uint32_t *ro_table;  /* the same of the reversed text, or NULL (then the D table is zeros) */
    uint64_t N;
    uint32_t sigma;
    const signed char *remap;  /* 256 entries: the code of every byte, < 0 where the record lacks it (remap_table.table) */
} sx_map_record;
/* The mapper's loop (bwt_readmapper.c:130-160, 257-266) over a FASTQ image: for every read in file order, for every record in
 * the order given, for every interval of the k-edit search in the iterator's order, for i = L .. R-1: one SAM line;
 * byte-identical to the reference mapper's stdout.  A read with a byte that a record's remap table lacks has no lines
 * for that record.  The text leaves through sink(user, SX_SECTION_SAM, data, bytes) in windows (SX_FLAG_SAM_WINDOW_BYTES)
 * from two pinned staging buffers; the copy of a window overlaps the sink's work on the one before.  Reads are searched
 * in batches (SX_FLAG_SAM_BATCH_READS) that are halved when their hits do not fit.  Memory: the reads, and every
 * record's suffix array and tables (N x (4 + 8 sigma) bytes with RO) stay on the device for the whole call; 32 bytes a
 * hit twice and 8 bytes a hit of offsets for one batch.  Limits: 0 <= edits <= 8, reads x records < 2^32, the FASTQ
 * contract of sx_fastq_index (SX_E_MALFORMED); its lines of at most 2046 bytes keep every read below the search's limit
 * (pattern length + edits < 2^15), so that limit cannot be met here. */
int sx_map_reads_stream(sx_ctx *ctx, const sx_map_record *records, uint32_t n_records, const uint8_t *fastq, size_t fastq_len,
                        int edits, sx_sink_fn sink, void *user);
/* Both strands.  rc(read) has the read's name, its sequence reversed and complemented and its quality
 * string reversed; the complement acts on the raw bytes, before any record's remap table, keeps the case and maps
 * A<->T, C<->G, U->A, R<->Y, K<->M, B<->V, D<->H; N, S, W and every other byte (also '*', '-', 0x80 .. 0xFF) stay.  With
 * SX_MAP_BOTH_STRANDS the text is, per read in file order, the lines of the read (FLAG 0) and then the lines that rc(read)
 * would print as a read of its own, with FLAG 16 in place of 0: POS is the leftmost forward coordinate, CIGAR, SEQ and QUAL
 * are in forward orientation, as SAM prescribes for a reverse-strand hit -- the reference mapper's stdout on the FASTQ file
 * "read0, rc(read0), read1, rc(read1), ..." with the second field of the odd entries' lines rewritten.  The limit becomes
 * 2 x reads x records < 2^32; the reads take twice the device memory.  flags == 0: sx_map_reads_stream, byte for byte and
 * launch for launch; unknown bits: SX_E_ARG.
 * Best stratum.  With SX_MAP_BEST_STRATUM and edits = k, e*(q) is the smallest d in 0 .. k for which
 * the same call with edits = d and without this flag prints at least one line for read q, over all records (with
 * SX_MAP_BOTH_STRANDS: over both strands of the read together); the text is, per read in file order, exactly the lines
 * that call prints for q with edits = e*(q): the reference mapper's stdout for that read at -d e*(q).  A read without
 * such a d prints nothing; k = 0 gives the text without the flag.  Every printed line uses exactly e*(q) edits.  The
 * reads are searched at 0 edits, the rest at 1, ... (sx_bwt_best_search_dev over all records); batches hold whole
 * reads (both strands of a read stay together).
 * No indels.  With SX_MAP_NO_INDELS every search of the call is the one of SX_SEARCH_NO_INDELS: the
 * text is that of the same call without the flag with every line removed whose CIGAR is not "<length of SEQ>M", i.e. the
 * placements of every read within `edits` substitutions, each once.  With SX_MAP_BEST_STRATUM the strata are taken under
 * the flag (the smallest number of substitutions).  It composes with the other two flags in any combination and does not
 * change the limit on reads x records; edits = 0 gives the text without the flag.  Bits 2 and 4 stay unknown.
 * Tags.  With SX_MAP_TAGS every line has "\tNM:i:<nm>\tMD:Z:<md>" between QUAL and its newline: the
 * edit distance and the mismatch string of the line's own POS, CIGAR and SEQ over the record's letters as the FASTA gives
 * them (the walk of sx_sam_batch_tags; FLAG 16 lines are in forward orientation already), rendered on the device once per
 * hit.  The lines and their order are those of the same call without the flag.  It composes with the other three flags in
 * any combination and with every form of the index, and does not change the limit on reads x records.  The records'
 * remapped strings must be on the device: an index with a record that was given without its string (sx_index_from_tables),
 * and sx_map_reads_stream_ex, whose records have none, answer SX_E_ARG before anything is launched or sunk.  Bit 32 stays
 * unknown.
 * Unmapped reads.  With SX_MAP_UNMAPPED the lines of the same call without the flag stay as they
 * are, and every read group for which that call prints no line (a group: a read, or with SX_MAP_BOTH_STRANDS the read and
 * its reverse complement; no line in any record, on either strand, in any stratum) gets one, where its lines would stand:
 *     <qname>\t4\t*\t0\t0\t*\t*\t0\t0\t<seq>\t<qual>\n
 * with QNAME, SEQ and QUAL of the read as the FASTQ has them (forward orientation, FLAG 4 also with both strands) and no
 * NM / MD under SX_MAP_TAGS.  It composes with the other flags and every index form and does not change the limit;
 * sx_index_map_pairs answers it with SX_E_ARG.
 * Header.  With SX_MAP_HEADER one sink call in front of the text writes "@HD\tVN:1.6\tSO:unsorted\n"
 * and, per record in the mapper's list order, "@SQ\tSN:<name>\tLN:<N - 1>\n", <name> byte for byte the RNAME of the lines.
 * Every argument check comes first (a refused call sinks nothing); an empty FASTQ gives the header alone.  It composes with
 * everything, sx_index_map_pairs included.  Neither bit changes a byte or a launch of a call without it.
 * MAPQ and secondary lines.  SX_MAP_MAPQ needs SX_MAP_BEST_STRATUM (without it a hit does not say how
 * many edits it uses, and a read's first line need not be one of its best): the bit alone answers SX_E_ARG with a message,
 * with every other argument check, before anything is sunk.  A group is a best-stratum group: a read, or with
 * SX_MAP_BOTH_STRANDS the read and its reverse complement.  Let n be the number of lines the same call without the bit prints
 * for the group, over all records and strands.  The text has the same lines in the same order with the same bytes but for
 * two fields.  FLAG: the group's first line in output order keeps its FLAG (0 or 16), every other line of the group has 256
 * added (256 or 272).  MAPQ, the same on every line of the group: 50 for n = 1, 3 for n = 2, 1 for n = 3 or 4, 0 for n >= 5
 * (-10 log10(1 - 1/n), rounded and floored as TopHat and STAR do; neither e* nor `edits` enters, and the lines of the next
 * stratum, e* + 1, are not counted).  n counts lines, not distinct positions: the search with indels reports some placements
 * twice ("1I99M" beside "100M"), so SX_MAP_NO_INDELS is what a caller combines the bit with.  FLAG 4 lines, NM and MD, the
 * header and the limit are unchanged; the bit composes with the other flags and every index form; sx_index_map_pairs answers
 * it with SX_E_ARG.  Bit 512 stays unknown.  A call without the bit launches what it launched and prints what it printed. */
enum {
    SX_MAP_BOTH_STRANDS = 1,
    SX_MAP_BEST_STRATUM = 8,
    SX_MAP_NO_INDELS = 16,
    SX_MAP_TAGS = 64,
    SX_MAP_UNMAPPED = 128,
    SX_MAP_HEADER = 256,
    SX_MAP_MAPQ = 1024
};
int sx_map_reads_stream_ex(sx_ctx *ctx, const sx_map_record *records, uint32_t n_records, const uint8_t *fastq, size_t fastq_len,
                           int edits, uint32_t flags, sx_sink_fn sink, void *user);
/* the limit of a mapping call on its reads and records: 0, or SX_E_ARG when reads x records (twice that with
 * SX_MAP_BOTH_STRANDS) does not stay below 2^32 or flags has unknown bits */
int sx_map_reads_limit(uint64_t n_reads, uint64_t n_records, uint32_t flags);
/* What the loop of the last mapping call on ctx did with its batches (zeroed when a call's loop starts; host counts only).
 * A batch's searches answer SX_E_CAPACITY when their hits do not fit the room: the room grows, or the batch is halved,
 * and the batch runs again (SX_FLAG_SAM_ROOM_HITS makes that happen on small inputs). */
typedef struct sx_map_stats {
    uint64_t batches;     /* batches whose text was emitted or that had no hits */
    uint64_t retries;     /* capacity returns: room_grown + lone_grown + halved */
    uint64_t room_grown;  /* the room grew for a batch of several groups (a group: a read, or both strands of a read) */
    uint64_t lone_grown;  /* the room grew for one group alone, which gets whatever it needs */
    uint64_t halved;      /* a batch was halved */
    uint64_t room_first, room_final;   /* the room, in hits, at the start and at the end of the call */
    uint64_t batch_first, batch_final; /* the reads of a batch at the start and at the end of the call */
} sx_map_stats;
int sx_map_last_stats(const sx_ctx *ctx, sx_map_stats *out);

/* ---- a device-resident index: build from FASTA once, map many read sets ---------------- */
/* sx_fastq_index on the device: the FASTQ image lies in device memory (len bytes), the six arrays of sx_fastq are
 * written to device memory that the call allocates (release with sx_fastq_dev_free; names, seqs and quals are 16-byte
 * aligned and followed by 16 readable bytes).  Contract, limits and error codes are exactly those of sx_fastq_index;
 * after an error *out holds no memory.  The same image gives the same bytes from run to run. */
typedef struct sx_fastq_dev {
    uint32_t count;
    uint8_t *d_names, *d_seqs, *d_quals;
    uint32_t *d_name_off, *d_seq_off, *d_qual_off; /* count + 1 entries each */
    uint64_t name_bytes, seq_bytes, qual_bytes;     /* = the offsets' last entries */
} sx_fastq_dev;
int sx_fastq_index_dev(sx_ctx *ctx, const uint8_t *d_image, uint64_t len, sx_fastq_dev *out);
/* The read set of both strands: from the device arrays of sx_fastq_index_dev (`in`, left as it is) a set of 2 x count reads
 * in device memory of its own (release with sx_fastq_dev_free; the contract of sx_fastq_dev holds: 16-byte aligned byte
 * arrays followed by 16 readable bytes): read 2q is read q, read 2q + 1 is rc(read q) (sx_map_reads_stream_ex).
 * d_flags_out (device memory of the caller, 2 x count entries): 0 for the even reads, 16 for the odd ones.  The same
 * input gives the same bytes from run to run.  SX_E_ARG: 2 x count or a doubled offset does not fit 32 bits (answered
 * before anything is launched), or the offsets' last entries are not in->name_bytes, seq_bytes, qual_bytes; after an
 * error *out holds no memory. */
int sx_fastq_strands_dev(sx_ctx *ctx, const sx_fastq_dev *in, sx_fastq_dev *out, uint16_t *d_flags_out);
void sx_fastq_dev_free(sx_fastq_dev *fq);

/* The index: for every record, in FASTA file order, its name, N (symbols + sentinel), sigma, remap table, the remapped
 * string (N bytes, the sentinel last) and SA, C, O and, when built with the reverse, RO as sx_bwt_tables_dev writes
 * them, in device allocations of its own: sx_ctx_trim and other builds on the same context leave it intact.
 * N x (5 + 8 sigma) bytes a record with RO.  It belongs to the device of the context that made it; a call with a
 * context on another device returns SX_E_ARG.  One index must not be used from two threads at once. */
typedef struct sx_index sx_index;
/* From a host FASTA image: upload through the pinned staging buffers, sx_fasta_pack_dev, then per record remap, suffix
 * array + BWT, C and O from the BWT and, with include_reverse, the same for the reversed string, whose suffix array is
 * dropped.  No table crosses to the host.  Errors are those of the calls it is made of: SX_E_MALFORMED (FASTA), SX_E_ARG
 * (an image of 2^31 - 1 bytes or more, more than 127 letters in a record), SX_E_NOMEM (host or device memory); nothing is
 * left allocated then.  A record with an empty sequence becomes what build_complete_table makes of an empty string: N = 1,
 * sigma = 1, SA = {0}; the index builds, saves and loads, and mapping against it answers SX_E_ARG as sx_map_reads_stream
 * does for such a table (sigma < 2). */
int sx_index_build_fasta(sx_ctx *ctx, const uint8_t *fasta, uint64_t len, int include_reverse, sx_index **out);
/* From host tables: the upload that sx_map_reads_stream performs, once.  `string` (optional): the N - 1 remapped symbols;
 * an index with a record that lacks it cannot be written (SX_E_ARG). */
typedef struct sx_index_source {
    sx_map_record record;
    const uint8_t *string;
} sx_index_source;
int sx_index_from_tables(sx_ctx *ctx, const sx_map_record *records, uint32_t n_records, sx_index **out);
int sx_index_from_sources(sx_ctx *ctx, const sx_index_source *sources, uint32_t n_records, sx_index **out);
/* one more record, behind the others or (at_front) in front of them: a loader goes record by record with one host copy */
int sx_index_add_record(sx_ctx *ctx, sx_index *idx, const sx_index_source *source, int at_front);
/* sx_map_reads_stream against the resident tables: the FASTQ image is uploaded and indexed on the device
 * (sx_fastq_index_dev).  Output, order, batch and window flags, limits and error codes are those of
 * sx_map_reads_stream. */
int sx_index_map_reads(sx_ctx *ctx, const sx_index *idx, const uint8_t *fastq, size_t fastq_len, int edits, sx_sink_fn sink,
                       void *user);
/* the same with the flags of sx_map_reads_stream_ex (SX_MAP_BOTH_STRANDS, SX_MAP_BEST_STRATUM, SX_MAP_NO_INDELS) and with
 * SX_MAP_TAGS, which needs every record's string in the index */
int sx_index_map_reads_ex(sx_ctx *ctx, const sx_index *idx, const uint8_t *fastq, size_t fastq_len, int edits, uint32_t flags,
                          sx_sink_fn sink, void *user);
/* Paired-end reads.  Read p of image 1 and read p of image 2 are the mates of pair p (different read
 * counts: SX_E_ARG before anything runs; the names need not be equal).  Let lines(x) be what sx_index_map_reads_ex prints
 * for read x with SX_MAP_BOTH_STRANDS and the same edits and flags.  (a, b), a in lines(mate 1), b in lines(mate 2), is a
 * proper combination when both have the same record, one has FLAG 0 (f) and the other FLAG 16 (r), POS(f) <= POS(r),
 * POS(f) + span(f) <= POS(r) + span(r) -- span: the hit's match_length, the M and D lengths of the CIGAR -- and
 * min_insert <= t <= max_insert for t = POS(r) + span(r) - POS(f).  The text is, per pair in file order, for a over
 * lines(mate 1) in order and b over lines(mate 2) in order, a's line and then b's line of every proper (a, b): the
 * both-strands line with FLAG = 1 + 2 + (64 on mate 1's line, 128 on mate 2's) + (16 on the reverse line, else 32), RNEXT
 * "=", PNEXT the other line's POS and TLEN t on f's line, -t on r's.  A pair without a proper combination prints nothing;
 * there are no discordant, single-mate or unmapped lines.  Placements that the search reports twice (1I99M beside 100M)
 * multiply: SX_MAP_BEST_STRATUM and SX_MAP_NO_INDELS are what a caller combines this with.  TLEN is a signed 32-bit
 * field, [-2^31 + 1, 2^31 - 1] in SAM: a combination with t >= 2^31 (only on a record of more than 2^31 symbols) has no
 * TLEN that can be written and is not printed, so a max_insert above 2^31 - 1 acts as 2^31 - 1.
 * flags: SX_MAP_BOTH_STRANDS (implied: set or not, the same text), SX_MAP_BEST_STRATUM (each mate has its own stratum over
 * its two strands) and SX_MAP_NO_INDELS; SX_MAP_TAGS and every other bit: SX_E_ARG, as min_insert > max_insert and a
 * NULL opts.  The limit is 4 x pairs x records < 2^32 (sx_map_pairs_limit).  Batches hold whole pairs: here
 * SX_FLAG_SAM_BATCH_READS counts pairs.  A batch whose lines or combinations do not fit the device is halved like one
 * whose hits do not fit; a pair alone gets what it needs.  Windows, sink and the other error codes are those of
 * sx_index_map_reads. */
typedef struct sx_pair_opts {
    uint32_t min_insert, max_insert;
} sx_pair_opts;
int sx_index_map_pairs(sx_ctx *ctx, const sx_index *idx, const uint8_t *fastq1, size_t len1, const uint8_t *fastq2, size_t len2, int edits,
                       const sx_pair_opts *opts, uint32_t flags, sx_sink_fn sink, void *user);
/* 0, or SX_E_ARG when 4 x pairs x records does not stay below 2^32 */
int sx_map_pairs_limit(uint64_t n_pairs, uint64_t n_records);
typedef struct sx_index_record {
    const char *name; /* valid until the index changes or is destroyed */
    uint64_t N;
    uint32_t sigma;
    int has_ro, has_string;
    const signed char *remap; /* host, 256 entries */
    /* device memory, exposed for tests */
    const uint8_t *d_string;
    const uint32_t *d_sa, *d_c, *d_o, *d_ro;
} sx_index_record;
int sx_index_info(const sx_index *idx, uint32_t *n_records_out, int *device_out, int *has_ro_out, uint64_t *device_bytes_out);
int sx_index_record_info(const sx_index *idx, uint32_t record, sx_index_record *out);
void sx_index_destroy(sx_index *idx);
/* indexes alive in this process (created minus destroyed) */
int sx_index_live_count(void);
/* The read mapper's index file from the resident buffers, through sink(user, SX_SECTION_INDEX, ..) in chunks of at most
 * 32 MiB from pinned staging: a u32 record count, then, last record first, a u32 name length, the name with its NUL and
 * the image of stralg/serialise.c (string, suffix array, remap table, C, O, a flag byte, RO). */
int sx_index_write(sx_ctx *ctx, const sx_index *idx, sx_sink_fn sink, void *user);
/* bytes of device memory to the host on the context's stream, then a sync (the tests read the index's buffers back) */
int sx_download(sx_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);

/* ---- the compact form of the O / RO tables ---------------- */
/* BWT blocks with occurrence counts sampled every 64 rows, one layout for every sigma in [1, 128]: rows 0 .. N in blocks
 * of 64; block b is sigma_pad u32 counters (sigma rounded up to a multiple of 16; counter a = O(a, 64 b), the counters
 * from sigma on are 0) followed by the 64 bytes bwt[64 b .. 64 b + 64), bytes from N on 0xFF.  N / 64 + 1 blocks of
 * 4 sigma_pad + 64 bytes; the first starts on a 16-byte boundary at least (the calls below answer SX_E_ARG otherwise; an
 * index allocates its blocks on 256-byte boundaries, so that a block of sigma <= 16 is one 128-byte line).  O(a, row) is counter a of block row / 64 plus the
 * number of bytes equal to a among the block's first row % 64: 4 N bytes for O and RO of DNA where the full tables take
 * 40 N.  The same BWT gives the same bytes from run to run. */
/* bytes of the blocks of a table of N rows + 1 (0 for N or sigma out of range) */
uint64_t sx_occ_compact_bytes(uint64_t N, uint32_t sigma);
/* blocks from a BWT on the device (N bytes, as sx_sa_bwt_build_dev leaves it); d_blocks_out: sx_occ_compact_bytes bytes */
int sx_occ_compact_build_dev(sx_ctx *ctx, const uint8_t *d_bwt, uint64_t N, uint32_t sigma, uint8_t *d_blocks_out);
/* rows [row_lo, row_hi) of the full table (row_hi <= N + 1) from the blocks: d_rows_out[(row - row_lo) * sigma + a] */
int sx_occ_compact_expand_dev(sx_ctx *ctx, const uint8_t *d_blocks, uint64_t N, uint32_t sigma, uint64_t row_lo, uint64_t row_hi,
                              uint32_t *d_rows_out);
/* sx_bwt_exact_search_dev and sx_bwt_approx_search_dev over blocks in place of the full tables (d_rocc may be NULL as
 * d_ro_table may): the same intervals, hits, offsets and order; sigma <= 128 */
int sx_bwt_exact_search_compact_dev(sx_ctx *ctx, const uint32_t *d_c_table, const uint8_t *d_occ, uint64_t N, uint32_t sigma,
                                    const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t count, uint32_t *d_l_out,
                                    uint32_t *d_r_out);
int sx_bwt_approx_search_compact_dev(sx_ctx *ctx, const uint32_t *d_c_table, const uint8_t *d_occ, const uint8_t *d_rocc, uint64_t N,
                                     uint32_t sigma, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t count, int max_edits,
                                     uint64_t *d_hit_offsets, sx_approx_hit *d_hits, uint64_t hit_capacity, uint64_t *total_hits_out);
int sx_bwt_approx_search_compact_dev_ex(sx_ctx *ctx, const uint32_t *d_c_table, const uint8_t *d_occ, const uint8_t *d_rocc, uint64_t N,
                                        uint32_t sigma, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t count, int max_edits,
                                        uint64_t *d_hit_offsets, sx_approx_hit *d_hits, uint64_t hit_capacity, uint64_t *total_hits_out,
                                        uint32_t search_flags); /* SX_SEARCH_* */
/* An index in the compact form (flags: SX_INDEX_COMPACT): every record keeps blocks in place of O and RO, about
 * N x (5 + 2 (1 + sigma_pad / 16)) bytes with RO (9 N for DNA in place of 45 N); no buffer of (N + 1) x sigma words exists
 * during the build (the BWT goes into the block builder; tables that arrive as full tables come up in windows through
 * the staging buffers).  Mapping gives the same text, sx_index_write the same file (the tables are expanded window by
 * window), sx_index_add_record follows the index's form; sx_index_record_info reports d_o = d_ro = NULL for such a
 * record and sx_index_record_occ its blocks.  Errors as sx_index_build_fasta / sx_index_from_sources; flags with unknown
 * bits: SX_E_ARG. */
enum { SX_INDEX_COMPACT = 1 };
int sx_index_build_fasta_ex(sx_ctx *ctx, const uint8_t *fasta, uint64_t len, int include_reverse, uint32_t flags, sx_index **out);
int sx_index_from_sources_ex(sx_ctx *ctx, const sx_index_source *sources, uint32_t n_records, uint32_t flags, sx_index **out);
typedef struct sx_index_occ {
    int compact;                  /* 0: the record has full tables and the rest is 0; 1: byte blocks; 2: packed blocks */
    const uint8_t *d_occ, *d_rocc; /* device memory; d_rocc NULL without the reverse */
    uint32_t stride, sigma_pad;   /* bytes a block, counters a block */
    uint64_t n_blocks;
} sx_index_occ;
int sx_index_record_occ(const sx_index *idx, uint32_t record, sx_index_occ *out);
/* 1 for an index in the compact form */
int sx_index_is_compact(const sx_index *idx);
/* rows [row_lo, row_hi) of a compact record's O table (reverse: of RO) to host memory, (row_hi - row_lo) x sigma words:
 * expanded on the device window by window (sx_occ_compact_expand_dev).  SX_E_ARG: a record with full tables, or without
 * the reverse, rows outside [0, N + 1]. */
int sx_index_expand_o(sx_ctx *ctx, const sx_index *idx, uint32_t record, int reverse, uint64_t row_lo, uint64_t row_hi,
                      uint32_t *rows_out);

/* ---- the packed form of the compact tables, for alphabets of up to 8 symbols ---------------- */
/* The same 64-row blocks with a nibble a row, one layout for every sigma in [1, 8]: block b is 64 bytes, 8 u32 counters
 * (counter a = O(a, 64 b), the counters from sigma on are 0) followed by 32 bytes of 64 nibbles: row 64 b + j in byte j / 2,
 * the low nibble for even j, the high one for odd j, nibbles from row N on 0xF.  N / 64 + 1 blocks; the first starts on a
 * 16-byte boundary at least (SX_E_ARG otherwise; an index allocates on 256-byte boundaries, so that two blocks share a
 * 128-byte line).  O(a, row) is counter a of block row / 64 plus the nibbles equal to a among the block's first row % 64:
 * 2 N bytes for O and RO of DNA where the byte blocks take 4 N.  The same BWT gives the same bytes from run to run.  The
 * calls are those of the compact form; each answers SX_E_ARG for sigma > 8 (sx_occ_packed_bytes answers 0). */
uint64_t sx_occ_packed_bytes(uint64_t N, uint32_t sigma);
int sx_occ_packed_build_dev(sx_ctx *ctx, const uint8_t *d_bwt, uint64_t N, uint32_t sigma, uint8_t *d_blocks_out);
int sx_occ_packed_expand_dev(sx_ctx *ctx, const uint8_t *d_blocks, uint64_t N, uint32_t sigma, uint64_t row_lo, uint64_t row_hi,
                             uint32_t *d_rows_out);
int sx_bwt_exact_search_packed_dev(sx_ctx *ctx, const uint32_t *d_c_table, const uint8_t *d_occ, uint64_t N, uint32_t sigma,
                                   const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t count, uint32_t *d_l_out,
                                   uint32_t *d_r_out);
int sx_bwt_approx_search_packed_dev(sx_ctx *ctx, const uint32_t *d_c_table, const uint8_t *d_occ, const uint8_t *d_rocc, uint64_t N,
                                    uint32_t sigma, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t count, int max_edits,
                                    uint64_t *d_hit_offsets, sx_approx_hit *d_hits, uint64_t hit_capacity, uint64_t *total_hits_out);
int sx_bwt_approx_search_packed_dev_ex(sx_ctx *ctx, const uint32_t *d_c_table, const uint8_t *d_occ, const uint8_t *d_rocc, uint64_t N,
                                       uint32_t sigma, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t count, int max_edits,
                                       uint64_t *d_hit_offsets, sx_approx_hit *d_hits, uint64_t hit_capacity, uint64_t *total_hits_out,
                                       uint32_t search_flags); /* SX_SEARCH_* */
/* An index in the packed form (flags: SX_INDEX_COMPACT | SX_INDEX_PACKED, with or without SX_INDEX_SA_SAMPLE_LOG2(q);
 * SX_INDEX_PACKED alone is SX_E_ARG): every record keeps packed blocks, about 7 N bytes with RO for DNA where the compact
 * index takes 9 N, 3.4 N with a suffix array sampled at 32 where it takes 5.4 N.  Mapping gives the same text and
 * sx_index_write the same file; sx_index_expand_o, sx_index_expand_sa and sx_index_add_record follow the index's form;
 * sx_index_record_occ reports compact = 2, stride = 64 and sigma_pad = 8.  A record of more than 8 symbols (7 letters and
 * the sentinel) has no place in such an index: a build or a load that meets one fails as a whole with SX_E_ARG and leaves
 * nothing behind, sx_index_add_record answers SX_E_ARG and leaves the index as it was. */
enum { SX_INDEX_PACKED = 4 };
/* 1 for an index in the packed form */
int sx_index_is_packed(const sx_index *idx);

/* ---- a sampled suffix array for the compact index ---------------- */
/* SA values kept at a sampling distance s = 2^q, q in 1 .. 10, the others recovered by walking LF over the forward blocks.
 * Sampling is by text position: row r is marked iff SA[r] % s == 0, so a record of N rows has (N + s - 1) / s samples.
 * Rows are cut into the blocks of the compact table (N / 64 + 1 of them).  Marks: one 16-byte entry a block, a u64 whose
 * bit j is set iff row 64 b + j is marked (rows from N on are clear), a u32 `before`, the number of marked rows in all
 * earlier blocks, and a u32 zero.  Values: SA[r] of the marked rows in row order, so the value of the marked row 64 b + j
 * is values[before + popcount(bits & ((1 << j) - 1))].  SA[row]: while the row is not marked, a = the row's BWT byte,
 * row = C[a] + O(a, row), one more step; the marked row's value plus the steps.  The same suffix array gives the same
 * bytes from run to run. */
/* bytes of the marks and of the values of a record of N rows; SX_E_ARG for N or q out of range */
int sx_sa_sample_bytes(uint64_t N, uint32_t q, uint64_t *marks_bytes_out, uint64_t *values_bytes_out);
/* marks and values from a suffix array on the device (N entries); d_marks_out 16-byte aligned.  SX_E_ARG when the array
 * does not hold (N + s - 1) / s multiples of s (it is no suffix array); nothing behind the buffers' ends is written */
int sx_sa_sample_build_dev(sx_ctx *ctx, const uint32_t *d_sa, uint64_t N, uint32_t q, void *d_marks_out, uint32_t *d_values_out);
/* SA[row_lo .. row_hi) (row_hi <= N) into d_out[0 .. row_hi - row_lo) from the C table, the forward blocks
 * (sx_occ_compact_build_dev), marks and values.  A walk is bounded at s steps: samples that do not belong to the blocks
 * end with SX_E_INTERNAL, not with a hang.  SX_E_ARG: misaligned blocks or marks, rows outside [0, N]. */
int sx_sa_locate_rows_dev(sx_ctx *ctx, const uint32_t *d_c_table, const uint8_t *d_occ, uint64_t N, uint32_t sigma, const void *d_marks,
                          const uint32_t *d_values, uint32_t q, uint64_t row_lo, uint64_t row_hi, uint32_t *d_out);
/* An index with a sampled suffix array: bits 8 .. 15 of the flags of sx_index_build_fasta_ex / sx_index_from_sources_ex
 * carry q (0: the whole suffix array, as before); q in 1 .. 10 needs SX_INDEX_COMPACT, anything else is SX_E_ARG.  Every
 * record keeps marks and values in place of its suffix array: about N x (5 + 1/4 + 4/s) + 4 N bytes of blocks for DNA with
 * RO, 5.4 N at s = 32 where the compact index takes 9 N.  A build from FASTA samples the suffix array and releases it before
 * the record is finished; tables that arrive from the host come up in windows.  Mapping locates the hits of a batch in
 * runs (SX_FLAG_LOCATE_CHUNK_ROWS) before their text is laid out and gives the same text; sx_index_write the same file
 * (the suffix array is located window by window); sx_index_add_record follows the index's form; sx_index_record_info
 * reports d_sa = NULL for such a record and sx_index_record_samples its marks and values. */
#define SX_INDEX_SA_SAMPLE_LOG2(q) ((uint32_t)(q) << 8)
typedef struct sx_index_samples {
    const void *d_marks;      /* device memory; NULL (and the rest 0) for a record with its whole suffix array */
    const uint32_t *d_values;
    uint32_t sa_log2;         /* q */
    uint64_t n_samples, n_blocks;
} sx_index_samples;
int sx_index_record_samples(const sx_index *idx, uint32_t record, sx_index_samples *out);
/* rows [row_lo, row_hi) of a sampled record's suffix array to host memory, located on the device window by window.
 * SX_E_ARG: a record with its whole suffix array, row_hi > N, row_lo > row_hi; row_lo == row_hi writes nothing. */
int sx_index_expand_sa(sx_ctx *ctx, const sx_index *idx, uint32_t record, uint64_t row_lo, uint64_t row_hi, uint32_t *rows_out);

/* ---- FASTA ingest and remap on the device ---------------- */
/* bioinf/fasta.c:92-135 load_fasta_records' packing of a file image in device memory into
 * "name\0sequence\0name\0sequence\0..." (file order; the reference's record list is the reverse).
 * d_packed_out: file_len + 1 bytes.  d_term_out (optional, term_cap entries): positions of the
 * terminators in the packed image, so record r has its name at (r ? term[2r-1] + 1 : 0), its
 * sequence at term[2r] + 1 and seq_len = term[2r+1] - term[2r] - 1.  file_len < 2^31 - 1.
 * Returns SX_E_MALFORMED where the reference reports MALFORMED_FILE. */
int sx_fasta_pack_dev(sx_ctx *ctx, const uint8_t *d_file, uint64_t file_len, uint8_t *d_packed_out,
                      uint64_t *packed_len_out, uint32_t *d_term_out, uint64_t term_cap, uint32_t *n_records_out);
/* the same with host buffers (staged through the context) */
int sx_fasta_pack(sx_ctx *ctx, const uint8_t *file, uint64_t file_len, uint8_t *packed_out, uint64_t *packed_len_out,
                  uint32_t *term_out, uint64_t term_cap, uint32_t *n_records_out);
/* stralg/remap.c:8-31,102-114 build_remap_table + remap: d_out[0..n) = dense order-preserving codes 1..k of
 * d_in, d_out[n] = 0; table_out (host, 256 entries, optional): code of every byte value, -1 for absent ones;
 * *alphabet_size_out = k + 1.  Fails when more than 127 distinct symbols occur (remap.h:14-18). */
int sx_remap_dev(sx_ctx *ctx, const uint8_t *d_in, uint64_t n, uint8_t *d_out, int16_t *table_out,
                 uint32_t *alphabet_size_out);
/* stralg/bwt.c:147-151: the reversed copy of a remapped string that build_complete_table sorts for the RO table:
 * d_out[i] = d_in[n - 1 - i], d_out[n] = 0 (n + 1 bytes; the buffers must not overlap) */
int sx_reverse_dev(sx_ctx *ctx, const uint8_t *d_in, uint64_t n, uint8_t *d_out);

/* ---- measurement ------------------------------------------------------------ */
int sx_profile_enable(sx_ctx *ctx, int on);       /* bracket every launch with HIP events */
int sx_profile_only(sx_ctx *ctx, int kclass);     /* ... only launches of this class (kclass < 0: all): two event records per
                                                     launch cost ~5 % on a build of 300 short launches */
int sx_profile_reset(sx_ctx *ctx);
int sx_profile_read(sx_ctx *ctx, sx_kernel_stat *out /* SX_KC_COUNT entries */);
const char *sx_kernel_class_name(int kclass);
int sx_last_stats(const sx_ctx *ctx, sx_build_stats *out);

/* Synthetic input on the device: symbol i = 1 + (splitmix64(seed, i) >> 33) % (sigma - 1)
 * (same stream as oracle_synth / stralg_amd.synth). */
int sx_synth_dev(sx_ctx *ctx, uint8_t *d_out, uint64_t n, uint32_t sigma, uint64_t seed);

/* The box's memory ceiling (measurement aid; SURVEY.md section 8d "confirm on the box"): four streaming shapes over two
 * device buffers of `bytes` each (16-byte aligned; use far more than the 256 MB last-level cache), HIP-event timed on the
 * context's stream, best of `reps` after a warm-up.  out_GBps[0] read (16 B a lane), [1] fill, [2] copy (bytes counted both
 * ways), [3] four-way split of 4-byte entries (4 B in + 4 B out an entry: the store shape of the induced-sort scatters with
 * no ranking work).  d_b is overwritten. */
int sx_membw_probe(sx_ctx *ctx, void *d_a, void *d_b, uint64_t bytes, int reps, double *out_GBps /* 4 */);

/* ---- primitives, exported for the kernel-level tests ---------------------- */
/* stable LSD radix sort of (u64 key, u32 value) pairs on bits [begin_bit, end_bit);
 * all four device buffers hold n entries; *result_in_b tells where the output is. */
int sx_prim_sort_pairs_dev(sx_ctx *ctx, uint64_t *d_keys_a, uint32_t *d_vals_a, uint64_t *d_keys_b,
                           uint32_t *d_vals_b, uint64_t n, int begin_bit, int end_bit,
                           int *result_in_b);
/* exclusive prefix sum of n u32; d_total (optional) receives the grand total */
int sx_prim_exclusive_sum_dev(sx_ctx *ctx, const uint32_t *d_in, uint32_t *d_out, uint64_t n,
                              uint32_t *d_total);
/* S/L classification products: LMS flags as one byte per position (n+1) and the
 * three per-symbol histograms (256 entries each): all symbols incl. sentinel,
 * L-type symbols, LMS symbols. */
int sx_prim_classify_dev(sx_ctx *ctx, const uint8_t *d_text, uint64_t n, uint8_t *d_lms_flags,
                         uint32_t *d_hist_all, uint32_t *d_hist_l, uint32_t *d_hist_lms);

#ifdef __cplusplus
}
#endif
#endif
