/*
 * stralg_amd_readmapper -- a read mapper on libstralg_amd.so that takes the command line and the index file of
 * stralg's tools/readmappers/bwt_readmapper.
 *
 *   stralg_amd_readmapper -p genome.fa              writes genome.fa.bwttables (options may stand between -p and the
 *                                                   file: -p --compact genome.fa)
 *   stralg_amd_readmapper -d K genome.fa reads.fq [more.fq ...]
 *                                                   prints the SAM lines of every match with at most K edits, file after
 *                                                   file; the index is loaded once and stays on the device
 *   stralg_amd_readmapper -i -d K genome.fa reads.fq [more.fq ...]
 *                                                   the same with the index built on the device from genome.fa: no
 *                                                   genome.fa.bwttables is read or written
 *   --compact                                       with -d (and -i or a saved index): the index keeps BWT blocks with
 *                                                   sampled counts in place of the O / RO tables, a fifth of the device
 *                                                   memory for DNA; the output is the same.  -p writes the same file
 *                                                   with or without it
 *   --sa-sample S                                   with --compact and -d (and -i or a saved index): SA values at every
 *                                                   S-th text position (a power of two in 2 .. 1024) in place of the
 *                                                   suffix array, the others located by walks over the blocks: 5.4 bytes
 *                                                   a symbol at S = 32 where --compact alone takes 9; the output is the
 *                                                   same.  -p writes the same file with or without it
 *   --packed                                        with --compact and -d (and -i or a saved index), with or without
 *                                                   --sa-sample: a nibble a row in the blocks, for genomes whose records
 *                                                   have at most 7 letters (ACGT and N fit): 7 bytes a symbol where
 *                                                   --compact alone takes 9, 3.4 at S = 32 where it takes 5.4; the
 *                                                   output is the same.  A record of more letters ends the run.  -p
 *                                                   writes the same file with or without it
 *   --both-strands                                  with -d: behind the lines of every read come the lines of its reverse
 *                                                   complement (sequence reversed and complemented, qualities reversed),
 *                                                   with FLAG 16 in place of 0; goes with -i, --compact, --sa-sample,
 *                                                   --packed and several FASTQ files
 *   --best                                          with -d K: per read only the lines of its best stratum, those that
 *                                                   -d e* prints for it, e* the smallest edit count in 0 .. K at which
 *                                                   any are printed (with --both-strands: over both strands of the read
 *                                                   together); a read without a match within K edits prints nothing
 *   --no-indels                                     with -d K: mismatches only -- of the lines of -d K those whose CIGAR is
 *                                                   "<read length>M", i.e. every placement of a read within K
 *                                                   substitutions, once; with --best the strata are the smallest number
 *                                                   of substitutions; goes with --both-strands, --compact, --packed,
 *                                                   --sa-sample and -i
 *   --tags                                          with -d: every line gets "\tNM:i:<nm>\tMD:Z:<md>" behind QUAL, the edit
 *                                                   distance and the mismatch string of its POS, CIGAR and SEQ over the
 *                                                   record's letters, rendered on the device; goes with every other
 *                                                   switch
 *   --unmapped                                      with -d: a read (with --both-strands: a read and its reverse complement)
 *                                                   that prints no line gets one, where its lines would stand:
 *                                                   "<name>\t4\t*\t0\t0\t*\t*\t0\t0\t<seq>\t<qual>", no tags; goes with
 *                                                   every other switch but -2
 *   --header                                        with -d: the SAM header in front of the lines, "@HD VN:1.6 SO:unsorted"
 *                                                   and an "@SQ SN:<name> LN:<length>" a record; once, with several FASTQ
 *                                                   files too; goes with every other switch, -2 included
 *   --mapq                                          with -d and --best: FLAG and MAPQ from the read's best stratum.  Of the n
 *                                                   lines of a read (with --both-strands: of the read and its reverse
 *                                                   complement) the first keeps its FLAG, every other one has 256 added
 *                                                   (secondary: 256 or 272), and all carry MAPQ 50 (n = 1), 3 (n = 2),
 *                                                   1 (n = 3 or 4) or 0 (n >= 5).  n counts lines, and the search with indels
 *                                                   reports some placements twice: --no-indels is what it is meant to be
 *                                                   used with.  Goes with every other switch but -2; without --best it is
 *                                                   refused before any output
 *   -2 mates.fq (--mates)                           with -d and one reads.fq: paired-end reads.  Read p of reads.fq and read p of
 *                                                   mates.fq are the mates of pair p; the output is the two lines of every
 *                                                   proper pair of their placements -- same record, one mate on either
 *                                                   strand, the forward one in front, the distance from its first base to
 *                                                   the reverse one's last in the window -- with FLAG 99 / 147 or 83 / 163,
 *                                                   RNEXT "=", PNEXT and TLEN; a pair without one prints nothing.  Both
 *                                                   strands are implied.  Goes with -i, --compact, --sa-sample, --packed,
 *                                                   --best and --no-indels (which is what it is meant to be used with: the
 *                                                   search reports some placements with indels more than once); not with
 *                                                   --tags, --unmapped, --mapq or several read files
 *   --min-insert N, --max-insert N                  with -2: the window of that distance (0 and 1000)
 *   (--preprocess, --edits and --in-memory are accepted for -p, -d and -i)
 *
 * Index file: u32 record count; per record, last FASTA record first, its name as u32 length + bytes + NUL, then the
 * table image of stralg/serialise.c.  Indexing packs the FASTA image with sx_fasta_pack and lets the library stream
 * each record's tables from the device into the file; mapping is stralg_amd_index_read / stralg_amd_index_map.
 */
#include "stralg_amd.h"
#include "stralg_compat.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define INDEX_EXT ".bwttables"

static void fail(const char *what, const char *detail)
{
    fprintf(stderr, "stralg_amd_readmapper: %s%s%s\n", what, detail ? ": " : "", detail ? detail : "");
    exit(EXIT_FAILURE);
}

static char *index_path(const char *fasta)
{
    char *p = malloc(strlen(fasta) + sizeof INDEX_EXT);
    if (!p) fail("out of memory", NULL);
    strcpy(p, fasta);
    strcat(p, INDEX_EXT);
    return p;
}

static uint8_t *slurp(const char *path, size_t *len)
{
    FILE *f = fopen(path, "rb");
    if (!f) fail("cannot read", path);
    size_t cap = 1 << 16, n = 0;
    uint8_t *buf = malloc(cap);
    while (buf) {
        n += fread(buf + n, 1, cap - n, f);
        if (n < cap) break;
        buf = realloc(buf, cap *= 2);
    }
    if (!buf) fail("out of memory", path);
    fclose(f);
    *len = n;
    return buf;
}

static void put_u32(FILE *f, uint32_t v)
{
    if (fwrite(&v, sizeof v, 1, f) != 1) fail("write error", NULL);
}

static int build_index(const char *fasta)
{
    size_t len = 0;
    uint8_t *image = slurp(fasta, &len);
    uint8_t *packed = malloc(len + 1);
    uint32_t *term = malloc((len + 2) * sizeof *term);
    if (!packed || !term) fail("out of memory", fasta);
    sx_ctx *ctx = NULL;
    if (sx_ctx_create(0, &ctx) != 0) fail("no usable GPU", NULL);
    uint64_t packed_len = 0;
    uint32_t n_rec = 0;
    const int rc = sx_fasta_pack(ctx, image, len, packed, &packed_len, term, len + 2, &n_rec);
    if (rc != 0) fail(rc == SX_E_MALFORMED ? "not a FASTA file" : sx_last_error(ctx), fasta);
    sx_ctx_destroy(ctx);
    char *path = index_path(fasta);
    FILE *out = fopen(path, "wb");
    if (!out) fail("cannot write", path);
    put_u32(out, n_rec);
    for (uint32_t r = n_rec; r-- > 0;) { /* last record first */
        const uint8_t *name = packed + (r ? term[2 * r - 1] + 1 : 0), *seq = packed + term[2 * r] + 1;
        const uint32_t name_bytes = (uint32_t)strlen((const char *)name) + 1;
        fprintf(stderr, "%s: %u symbols\n", (const char *)name, term[2 * r + 1] - term[2 * r] - 1);
        put_u32(out, name_bytes);
        if (fwrite(name, 1, name_bytes, out) != name_bytes) fail("write error", path);
        if (stralg_amd_write_complete_bwt_info_stream(out, seq, true) != 0) fail("could not build the tables of", (const char *)name);
    }
    if (fclose(out) != 0) fail("write error", path);
    free(path);
    free(term);
    free(packed);
    free(image);
    stralg_amd_release();
    return EXIT_SUCCESS;
}

/* -d: the index is loaded once (from genome.fa.bwttables, or, with -i, built on the device from genome.fa itself) and
 * stays on the device; every FASTQ file is mapped against it, stdout is the files' texts one behind the other */
static int map_reads(const char *fasta, char *const *reads, int n_reads, int k, int in_memory, uint32_t flags, uint32_t map_flags,
                     const char *mates, const sx_pair_opts *window)
{
    struct sx_index *idx = NULL;
    if (in_memory) {
        size_t len = 0;
        uint8_t *image = slurp(fasta, &len);
        idx = stralg_amd_index_from_fasta_image_ex(image, len, true, flags);
        free(image);
        if (!idx) fail("could not index", fasta);
    } else {
        char *path = index_path(fasta);
        FILE *in = fopen(path, "rb");
        if (!in) fail("cannot read (run -p first)", path);
        idx = stralg_amd_index_read_ex(in, flags);
        if (!idx) fail("empty or truncated index", path);
        fclose(in);
        free(path);
    }
    int rc = 0;
    if (mates) { /* -2: reads[0] and mates are the two files of the pairs */
        FILE *fq1 = fopen(reads[0], "rb"), *fq2 = fopen(mates, "rb");
        if (!fq1 || !fq2) fail("cannot read", fq1 ? mates : reads[0]);
        rc = stralg_amd_index_map_pairs(idx, fq1, fq2, k, window, map_flags, stdout);
        fclose(fq1);
        fclose(fq2);
        n_reads = 0;
    }
    for (int f = 0; f < n_reads && rc == 0; ++f) {
        FILE *fq = fopen(reads[f], "rb");
        if (!fq) fail("cannot read", reads[f]);
        rc = stralg_amd_index_map_ex(idx, fq, k, f == 0 ? map_flags : map_flags & ~(uint32_t)SX_MAP_HEADER, stdout); /* (one header) */
        fclose(fq);
    }
    stralg_amd_index_free(idx);
    stralg_amd_release();
    return rc == 0 && fflush(stdout) == 0 ? EXIT_SUCCESS : EXIT_FAILURE;
}

static int usage(const char *self, int status)
{
    fprintf(stderr, "usage: %s -p genome.fa               build genome.fa" INDEX_EXT "\n", self);
    fprintf(stderr, "       %s -d K genome.fa reads.fq ...  SAM lines of all matches within K edits, on stdout\n", self);
    fprintf(stderr, "       %s -i -d K genome.fa reads.fq ...  the same, the index built in memory from genome.fa\n", self);
    fprintf(stderr, "       --compact                          with -d: BWT blocks in place of the O tables on the device\n");
    fprintf(stderr, "       --sa-sample S                      with --compact and -d: SA values at every S-th position (a power of\n");
    fprintf(stderr, "                                          two in 2 .. 1024) in place of the suffix array on the device\n");
    fprintf(stderr, "       --packed                           with --compact and -d: a nibble a row in the blocks (records of at\n");
    fprintf(stderr, "                                          most 7 letters)\n");
    fprintf(stderr, "       --both-strands                     with -d: every read's reverse complement is mapped too, its lines\n");
    fprintf(stderr, "                                          have FLAG 16\n");
    fprintf(stderr, "       --best                             with -d K: per read only the matches of the smallest edit count\n");
    fprintf(stderr, "                                          in 0 .. K that has any (with --both-strands: over both strands)\n");
    fprintf(stderr, "       --no-indels                        with -d K: mismatches only, every placement within K substitutions\n");
    fprintf(stderr, "                                          once (with --best: the smallest number of substitutions)\n");
    fprintf(stderr, "       --tags                             with -d: NM:i and MD:Z behind QUAL on every line\n");
    fprintf(stderr, "       --unmapped                         with -d: a FLAG 4 line for every read that prints no line\n");
    fprintf(stderr, "       --header                           with -d: @HD and @SQ lines in front of the text, once\n");
    fprintf(stderr, "       --mapq                             with -d and --best: per read the first line keeps its FLAG, the others\n");
    fprintf(stderr, "                                          get 256 added; MAPQ 50, 3, 1, 0 for 1, 2, 3-4, 5 or more lines of the\n");
    fprintf(stderr, "                                          read (meant for --no-indels); not without --best, not with -2\n");
    fprintf(stderr, "       -2 mates.fq, --mates mates.fq      with -d and one reads.fq: paired-end reads, the lines of the proper\n");
    fprintf(stderr, "                                          pairs (FLAG 99 / 147, 83 / 163); not with --tags, --unmapped or --mapq\n");
    fprintf(stderr, "       --min-insert N, --max-insert N     with -2: the window of a pair's length (0, 1000)\n");
    return status;
}

int main(int argc, char **argv)
{
    const char *to_index = NULL, *mates = NULL;
    sx_pair_opts window = {0, 1000};
    char **rest = calloc((size_t)argc + 1, sizeof *rest);
    int k = -1, n_rest = 0, in_memory = 0, indexing = 0;
    uint32_t flags = 0, sa_log2 = 0, map_flags = 0;
    if (!rest) fail("out of memory", NULL);
    for (int a = 1; a < argc; ++a) {
        const char *s = argv[a];
        const int wants_p = !strcmp(s, "-p") || !strcmp(s, "--preprocess"), wants_d = !strcmp(s, "-d") || !strcmp(s, "--edits");
        if (!strcmp(s, "-h") || !strcmp(s, "--help")) return usage(argv[0], EXIT_SUCCESS);
        if (!strcmp(s, "-i") || !strcmp(s, "--in-memory")) {
            in_memory = 1;
        } else if (!strcmp(s, "--compact")) {
            flags |= SX_INDEX_COMPACT;
        } else if (!strcmp(s, "--packed")) {
            flags |= SX_INDEX_PACKED;
        } else if (!strcmp(s, "--both-strands")) {
            map_flags |= SX_MAP_BOTH_STRANDS;
        } else if (!strcmp(s, "--best")) {
            map_flags |= SX_MAP_BEST_STRATUM;
        } else if (!strcmp(s, "--no-indels")) {
            map_flags |= SX_MAP_NO_INDELS;
        } else if (!strcmp(s, "--tags")) {
            map_flags |= SX_MAP_TAGS;
        } else if (!strcmp(s, "--unmapped")) {
            map_flags |= SX_MAP_UNMAPPED;
        } else if (!strcmp(s, "--header")) {
            map_flags |= SX_MAP_HEADER;
        } else if (!strcmp(s, "--mapq")) {
            map_flags |= SX_MAP_MAPQ;
        } else if (!strcmp(s, "-2") || !strcmp(s, "--mates")) {
            if (++a >= argc) return usage(argv[0], EXIT_FAILURE);
            mates = argv[a];
        } else if (!strcmp(s, "--min-insert") || !strcmp(s, "--max-insert")) {
            if (++a >= argc) return usage(argv[0], EXIT_FAILURE);
            char *end = NULL;
            const unsigned long long v = strtoull(argv[a], &end, 10);
            if (argv[a][0] < '0' || argv[a][0] > '9' || *end || v > 0xFFFFFFFFull) fail("an insert size is a number below 2^32, not", argv[a]);
            *(s[3] == 'i' ? &window.min_insert : &window.max_insert) = (uint32_t)v;
        } else if (!strcmp(s, "--sa-sample")) {
            if (++a >= argc) return usage(argv[0], EXIT_FAILURE);
            const long dist = strtol(argv[a], NULL, 10);
            for (sa_log2 = 1; sa_log2 <= 10 && (1L << sa_log2) != dist; ++sa_log2) {}
            if (sa_log2 > 10) fail("--sa-sample takes a power of two in 2 .. 1024, not", argv[a]);
        } else if (wants_p) { /* the file follows, or, where options come first (-p --compact genome.fa), stands behind them */
            indexing = 1;
            if (a + 1 < argc && argv[a + 1][0] != '-') to_index = argv[++a];
        } else if (wants_d) {
            if (++a >= argc) return usage(argv[0], EXIT_FAILURE);
            k = (int)strtol(argv[a], NULL, 10);
        } else if (s[0] == '-' && s[1] == 'd' && s[2]) { /* -dK */
            k = (int)strtol(s + 2, NULL, 10);
        } else if (s[0] == '-' && s[1]) {
            return usage(argv[0], EXIT_FAILURE);
        } else {
            rest[n_rest++] = argv[a];
        }
    }
    if (sa_log2 && !(flags & SX_INDEX_COMPACT)) fail("--sa-sample needs --compact", NULL);
    if ((flags & SX_INDEX_PACKED) && !(flags & SX_INDEX_COMPACT)) fail("--packed needs --compact", NULL);
    flags |= SX_INDEX_SA_SAMPLE_LOG2(sa_log2);
    if (indexing && !to_index && n_rest) to_index = rest[0];
    if (indexing) return to_index ? build_index(to_index) : usage(argv[0], EXIT_FAILURE);
    if (n_rest < 2 || k < 0) return usage(argv[0], EXIT_FAILURE);
    if (mates && (map_flags & SX_MAP_TAGS)) fail("-2 does not go with --tags", NULL);
    if (mates && (map_flags & SX_MAP_UNMAPPED)) {
        fprintf(stderr, "%s: -2 does not go with --unmapped\n", argv[0]);
        return usage(argv[0], EXIT_FAILURE);
    }
    if ((map_flags & SX_MAP_MAPQ) && (mates || !(map_flags & SX_MAP_BEST_STRATUM))) {
        fprintf(stderr, "%s: --mapq %s\n", argv[0], mates ? "does not go with -2" : "needs --best");
        return usage(argv[0], EXIT_FAILURE);
    }
    if (mates && n_rest != 2) fail("-2 takes one reads file beside the mates' file", NULL);
    if (mates && window.min_insert > window.max_insert) fail("--min-insert must not exceed --max-insert", NULL);
    return map_reads(rest[0], rest + 1, n_rest - 1, k, in_memory, flags, map_flags, mates, &window);
}
