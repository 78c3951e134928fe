/*
 * stralg_amd_readmapper -- a read mapper on libstralg_amd.so that takes the command line and the index file of
 * stralg's tools/readmappers/bwt_readmapper.
 *
 *   stralg_amd_readmapper -p genome.fa              writes genome.fa.bwttables
 *   stralg_amd_readmapper -d K genome.fa reads.fq   prints the SAM lines of every match with at most K edits
 *   (--preprocess and --edits are accepted for -p and -d)
 *
 * Index file: u32 record count; per record, last FASTA record first, its name as u32 length + bytes + NUL, then the
 * table image of stralg/serialise.c.  Indexing packs the FASTA image with sx_fasta_pack and lets the library stream
 * each record's tables from the device into the file; mapping is stralg_amd_map_reads.
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

static int map_reads(const char *fasta, const char *reads, int k)
{
    char *path = index_path(fasta);
    FILE *in = fopen(path, "rb");
    if (!in) fail("cannot read (run -p first)", path);
    uint32_t n = 0;
    if (fread(&n, sizeof n, 1, in) != 1) fail("empty index", path);
    struct bwt_table **tables = calloc((size_t)n + 1, sizeof *tables);
    char **names = calloc((size_t)n + 1, sizeof *names);
    if (!tables || !names) fail("out of memory", path);
    /* the lines of one read list the records last-in-file first */
    for (uint32_t at = n; at-- > 0;) {
        uint32_t name_bytes = 0;
        if (fread(&name_bytes, sizeof name_bytes, 1, in) != 1 || name_bytes == 0 || !(names[at] = malloc(name_bytes)) ||
            fread(names[at], 1, name_bytes, in) != name_bytes || names[at][name_bytes - 1] != '\0' ||
            !(tables[at] = read_complete_bwt_info(in)))
            fail("truncated index", path);
    }
    fclose(in);
    FILE *fq = fopen(reads, "rb");
    if (!fq) fail("cannot read", reads);
    const int rc = stralg_amd_map_reads(tables, (const char *const *)names, n, fq, k, stdout);
    fclose(fq);
    for (uint32_t r = 0; r < n; ++r) {
        completely_free_bwt_table(tables[r]);
        free(names[r]);
    }
    free(tables);
    free(names);
    free(path);
    stralg_amd_release();
    return rc == 0 && fflush(stdout) == 0 ? EXIT_SUCCESS : EXIT_FAILURE;
}

static int usage(const char *self, int status)
{
    fprintf(stderr, "usage: %s -p genome.fa               build genome.fa" INDEX_EXT "\n", self);
    fprintf(stderr, "       %s -d K genome.fa reads.fq    SAM lines of all matches within K edits, on stdout\n", self);
    return status;
}

int main(int argc, char **argv)
{
    const char *to_index = NULL, *rest[2] = {NULL, NULL};
    int k = -1, n_rest = 0;
    for (int a = 1; a < argc; ++a) {
        const char *s = argv[a];
        const int wants_p = !strcmp(s, "-p") || !strcmp(s, "--preprocess"), wants_d = !strcmp(s, "-d") || !strcmp(s, "--edits");
        if (!strcmp(s, "-h") || !strcmp(s, "--help")) return usage(argv[0], EXIT_SUCCESS);
        if (wants_p || wants_d) {
            if (++a >= argc) return usage(argv[0], EXIT_FAILURE);
            if (wants_p) to_index = argv[a];
            else k = (int)strtol(argv[a], NULL, 10);
        } else if (s[0] == '-' && s[1] == 'd' && s[2]) { /* -dK */
            k = (int)strtol(s + 2, NULL, 10);
        } else if (s[0] == '-' && s[1]) {
            return usage(argv[0], EXIT_FAILURE);
        } else if (n_rest < 2) {
            rest[n_rest++] = s;
        } else {
            return usage(argv[0], EXIT_FAILURE);
        }
    }
    if (to_index) return build_index(to_index);
    if (n_rest != 2 || k < 0) return usage(argv[0], EXIT_FAILURE);
    return map_reads(rest[0], rest[1], k);
}
