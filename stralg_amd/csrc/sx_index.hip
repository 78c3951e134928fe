// sx_index.hip -- a device-resident index (build from FASTA once, map many read sets) and the FASTQ ingest on the
// device.
//
// The index holds, for every FASTA record, the remapped string, SA, C, O and RO in device allocations of its own (not
// slabs of a context's cache), so that a context can be trimmed or used for other builds while an index lives.
//
// sx_fastq_index_dev restates the host's sx_fastq_index (stralg_host.c; bioinf/fastq.c:17-35) as data-parallel passes
// over 4096-byte tiles of the image.  A byte's line is the number of newlines in front of it; the line at rank j belongs
// to record j / 4 and has role j % 4 (name, sequence, '+' line, quality):
//   1. every tile counts its newlines (16 bytes a lane, classified in their words) and flags NUL bytes,
//   2. a scan of the tile counts gives every tile the rank of its first line,
//   3. the line-end table: the position of every line's newline (the image's end for a last line without one),
//   4. one lane a record checks its four lines and writes the three lengths (or an error bit),
//   5. three exclusive scans turn the lengths into the offset arrays,
//   6. a pass over the image in order sends every byte of a first, second or fourth line to its place: a workgroup
//      holds its tile's line starts in LDS, a lane finds the line of its four bytes by a search in them.
// Where a byte goes is a function of the scans alone (no atomics place anything): the same image gives the same bytes.
#include "sx_common.hpp"
#include "sx_device.hpp"
#include "sx_bytes16.hpp"
#include "sx_hostio.hpp"
#include "sx_scan.hpp"
#include "sx_index.hpp"
#include "sx_occ.hpp"
#include "sx_locate.hpp"

#include <stdlib.h>

#include <atomic>
#include <new>

namespace sx {

// ---- FASTQ image -> the six arrays of sx_fastq ---------------------------------------------------------------------
constexpr int kFqPer = kBytes16, kFqTile = kBlock * kFqPer;
constexpr uint32_t kFqLineMax = 2047; // fgets(buffer, 2048): a line's content must be shorter than this
enum { FQ_ERR_NUL = 1, FQ_ERR_LINE = 2 };

// which of the lane's 16 bytes (those in front of `len`) are newlines / NULs: bit k for byte k (sx_bytes16.hpp)
__device__ __forceinline__ void fq_masks16(const uint8_t *__restrict__ img, uint64_t i0, uint64_t len, uint32_t &nl, uint32_t &zero)
{
    nl = 0, zero = 0;
    if (i0 >= len) return;
    uint4 v = {0, 0, 0, 0};
    if (fetch16(img, i0, len, v)) {
        nl = eq16(v, 0x0A0A0A0Au);
        zero = eq16(v, 0u);
    } else { // (nothing beyond `len` counts as a NUL here)
        for (int k = 0; k < kFqPer && i0 + k < len; ++k) {
            const uint32_t c = img[i0 + k];
            nl |= (c == '\n' ? 1u : 0u) << k;
            zero |= (c == 0u ? 1u : 0u) << k;
        }
    }
}

// pass 1: newlines of every tile; scal[0] |= FQ_ERR_NUL for a NUL byte; scal[1] <- 1 when the last byte is no newline
__global__ __launch_bounds__(kBlock) void fq_count_kernel(const uint8_t *__restrict__ img, uint64_t len, uint32_t *__restrict__ tile_nl,
                                                          uint32_t *__restrict__ scal)
{
    __shared__ uint32_t lds[kWavesPerBlock];
    const uint64_t i0 = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) * kFqPer;
    uint32_t nl, zero;
    fq_masks16(img, i0, len, nl, zero);
    if (zero) atomicOr(&scal[0], (uint32_t)FQ_ERR_NUL);
    if (i0 < len && len - i0 <= (uint64_t)kFqPer) scal[1] = ((nl >> (uint32_t)(len - 1 - i0)) & 1u) ? 0u : 1u;
    const uint32_t tot = block_reduce<OpAdd>((uint32_t)__popc(nl), lds);
    if (threadIdx.x == 0) tile_nl[blockIdx.x] = tot;
}

// pass 3: line_end[j] <- position of the newline that ends line j; the last line of an image without a final newline
// ends at len (n_lines > the number of newlines then)
__global__ __launch_bounds__(kBlock) void fq_line_end_kernel(const uint8_t *__restrict__ img, uint64_t len, const uint32_t *__restrict__ tile_base,
                                                             uint32_t *__restrict__ line_end, uint32_t n_newlines, uint32_t n_lines)
{
    __shared__ uint32_t lds[kWavesPerBlock];
    const uint64_t i0 = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) * kFqPer;
    uint32_t nl, zero;
    fq_masks16(img, i0, len, nl, zero);
    uint32_t tot;
    uint32_t rank = tile_base[blockIdx.x] + block_exclusive_scan<OpAdd>((uint32_t)__popc(nl), lds, tot);
    while (nl) {
        const uint32_t k = (uint32_t)__ffs(nl) - 1u;
        if (rank < n_newlines) line_end[rank] = (uint32_t)(i0 + k);
        ++rank;
        nl &= nl - 1u;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && n_lines > n_newlines) line_end[n_newlines] = (uint32_t)len;
}

// pass 4: record r's lines end at e[0 .. 4); lens[k][r] <- the bytes of its name, sequence and quality; entry `count`
// of each is 0 so that the scans' entry `count` is the total
__global__ __launch_bounds__(kBlock) void fq_record_kernel(const uint32_t *__restrict__ line_end, uint32_t count, uint32_t *__restrict__ name_len,
                                                           uint32_t *__restrict__ seq_len, uint32_t *__restrict__ qual_len, uint32_t *__restrict__ scal)
{
    const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r > count) return;
    uint32_t nlen = 0, slen = 0, qlen = 0;
    if (r < count) {
        const uint32_t start = r ? line_end[4 * r - 1] + 1u : 0u;
        const uint32_t e0 = line_end[4 * r], e1 = line_end[4 * r + 1], e2 = line_end[4 * r + 2], e3 = line_end[4 * r + 3];
        const uint32_t l0 = e0 - start, l1 = e1 - e0 - 1u, l2 = e2 - e1 - 1u, l3 = e3 - e2 - 1u;
        // a line of 2047 bytes or more; a first line of fewer than 2 bytes; an empty second or fourth line
        const bool bad = l0 >= kFqLineMax || l1 >= kFqLineMax || l2 >= kFqLineMax || l3 >= kFqLineMax || l0 < 2u || l1 == 0u || l3 == 0u;
        if (bad) atomicOr(&scal[0], (uint32_t)FQ_ERR_LINE);
        else nlen = l0 - 1u, slen = l1, qlen = l3;
    }
    name_len[r] = nlen;
    seq_len[r] = slen;
    qual_len[r] = qlen;
}

// pass 6: every byte to its place.  ls[m]: the first byte of the m-th line that touches this tile (ls[0]: the line
// the tile's first byte lies in, which may start in an earlier tile).
__global__ __launch_bounds__(kBlock) void fq_scatter_kernel(const uint8_t *__restrict__ img, uint64_t len, const uint32_t *__restrict__ tile_base,
                                                            const uint32_t *__restrict__ tile_nl, const uint32_t *__restrict__ line_end,
                                                            const uint32_t *__restrict__ name_off, const uint32_t *__restrict__ seq_off,
                                                            const uint32_t *__restrict__ qual_off, uint8_t *__restrict__ names,
                                                            uint8_t *__restrict__ seqs, uint8_t *__restrict__ quals, uint32_t n_lines)
{
    __shared__ uint32_t ls[kFqTile + 1];
    const uint64_t tile0 = (uint64_t)blockIdx.x * kFqTile;
    const uint32_t rank0 = tile_base[blockIdx.x], cnt = tile_nl[blockIdx.x]; // cnt <= kFqTile
    for (uint32_t m = threadIdx.x; m <= cnt; m += kBlock) {
        const uint32_t j = rank0 + m; // ls[m] = the start of line j = the end of line j - 1, plus one
        ls[m] = j ? line_end[j - 1] + 1u : 0u;
    }
    __syncthreads();
    const bool words = ((uintptr_t)img & 3u) == 0;
    for (uint32_t it = 0; it < (uint32_t)kFqTile / (4u * kBlock); ++it) {
        const uint64_t i = tile0 + 4ull * ((uint64_t)it * kBlock + threadIdx.x);
        if (i >= len) break;
        uint32_t w = 0;
        if (words && i + 4 <= len) {
            w = *reinterpret_cast<const uint32_t *>(img + i);
        } else {
            for (uint32_t k = 0; k < 4 && i + k < len; ++k) w |= (uint32_t)img[i + k] << (8u * k);
        }
        uint32_t m = 0;
        { // the last m with ls[m] <= i (ls[0] <= tile0)
            uint32_t hi = cnt + 1u;
            while (hi - m > 1u) {
                const uint32_t mid = (m + hi) / 2u;
                if ((uint64_t)ls[mid] <= i) m = mid;
                else hi = mid;
            }
        }
        for (uint32_t k = 0; k < 4; ++k) {
            const uint64_t pos = i + k;
            if (pos >= len) break;
            if (m < cnt && (uint64_t)ls[m + 1] <= pos) ++m;
            const uint32_t c = (w >> (8u * k)) & 0xFFu;
            const uint32_t j = rank0 + m;
            if (c == '\n' || j >= n_lines) continue;
            const uint32_t rec = j >> 2, role = j & 3u, off = (uint32_t)(pos - ls[m]);
            if (role == 0) {
                if (off) names[name_off[rec] + off - 1u] = (uint8_t)c; // (the record's first byte is dropped whatever it is)
            } else if (role == 1) {
                seqs[seq_off[rec] + off] = (uint8_t)c;
            } else if (role == 3) {
                quals[qual_off[rec] + off] = (uint8_t)c;
            }
        }
    }
}

static std::atomic<int> g_live_indexes{0};
static void free_rec(sx_index_rec &R)
{
    (void)hipFree(R.d_string), (void)hipFree(R.d_sa), (void)hipFree(R.d_c), (void)hipFree(R.d_o), (void)hipFree(R.d_ro);
    (void)hipFree(R.d_occ), (void)hipFree(R.d_rocc), (void)hipFree(R.d_sa_marks), (void)hipFree(R.d_sa_values);
    R.d_string = R.d_occ = R.d_rocc = R.d_sa_marks = nullptr, R.d_sa = R.d_c = R.d_o = R.d_ro = R.d_sa_values = nullptr;
}

static void free_view(sx_index *idx)
{
    (void)hipFree(idx->d_rnames), (void)hipFree(idx->d_tabs), (void)hipFree(idx->d_rname_off), (void)hipFree((void *)idx->d_sa_list),
        (void)hipFree(idx->d_sa_lens), (void)hipFree(idx->d_loc_list);
    idx->d_loc_list = nullptr;
    idx->d_rnames = idx->d_tabs = nullptr, idx->d_rname_off = nullptr, idx->d_sa_list = nullptr, idx->d_sa_lens = nullptr;
    idx->device_bytes -= idx->view_bytes;
    idx->view_bytes = 0;
}

// what the mapper's kernels read of the records, uploaded again after every change of the record list
static int make_view(sx_ctx *ctx, sx_index *idx)
{
    free_view(idx);
    const size_t n = idx->recs.size();
    std::vector<uint8_t> rnames, tabs(n * 256 + 1);
    std::vector<uint32_t> rname_off(n + 1);
    std::vector<const uint32_t *> sa_ptrs(n + 1);
    std::vector<uint64_t> sa_lens(n + 1);
    std::vector<LocRec> locs(idx->sa_log2 ? n : 0);
    for (size_t r = 0; r < n; ++r) {
        const sx_index_rec &R = idx->recs[r];
        rname_off[r] = (uint32_t)rnames.size();
        rnames.insert(rnames.end(), R.name.begin(), R.name.end());
        // remap.c:102-114: a byte the table lacks makes remap() return NULL and the mapper skip the record for this
        // read; here it becomes symbol 0, for which the search has no hits
        for (int b = 0; b < 256; ++b) tabs[r * 256 + b] = R.remap[b] > 0 && (uint32_t)R.remap[b] < R.sigma ? (uint8_t)R.remap[b] : 0;
        sa_ptrs[r] = R.d_sa;
        sa_lens[r] = R.N;
        if (idx->sa_log2) locs[r] = loc_rec_of(R.d_c, R.d_occ, R.N, R.sigma, R.d_sa_marks, R.d_sa_values, R.sa_log2);
    }
    rname_off[n] = (uint32_t)rnames.size();
    rnames.push_back(0);
    sx_dev_scope S;
    size_t bytes = 0;
    uint8_t *d_rnames, *d_tabs;
    uint32_t *d_rname_off;
    const uint32_t **d_sa_list;
    uint64_t *d_sa_lens;
    SX_TRY(S.take(ctx, &d_rnames, rnames.size(), &bytes));
    SX_TRY(S.take(ctx, &d_tabs, tabs.size(), &bytes));
    SX_TRY(S.take(ctx, &d_rname_off, rname_off.size(), &bytes));
    SX_TRY(S.take(ctx, &d_sa_list, sa_ptrs.size(), &bytes));
    SX_TRY(S.take(ctx, &d_sa_lens, sa_lens.size(), &bytes));
    LocRec *d_locs = nullptr;
    if (!locs.empty()) {
        SX_TRY(S.take(ctx, &d_locs, locs.size(), &bytes));
        SX_CHECK(hipMemcpyAsync(d_locs, locs.data(), locs.size() * sizeof(LocRec), hipMemcpyHostToDevice, ctx->stream));
    }
    SX_CHECK(hipMemcpyAsync(d_rnames, rnames.data(), rnames.size(), hipMemcpyHostToDevice, ctx->stream));
    SX_CHECK(hipMemcpyAsync(d_tabs, tabs.data(), tabs.size(), hipMemcpyHostToDevice, ctx->stream));
    SX_CHECK(hipMemcpyAsync(d_rname_off, rname_off.data(), rname_off.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    SX_CHECK(hipMemcpyAsync(d_sa_list, sa_ptrs.data(), sa_ptrs.size() * sizeof(void *), hipMemcpyHostToDevice, ctx->stream));
    SX_CHECK(hipMemcpyAsync(d_sa_lens, sa_lens.data(), sa_lens.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    SX_TRY(sx_sync(ctx)); // (the host vectors are pageable: their copies are done)
    S.keep();
    idx->d_rnames = d_rnames, idx->d_tabs = d_tabs, idx->d_rname_off = d_rname_off, idx->d_sa_list = d_sa_list, idx->d_sa_lens = d_sa_lens;
    idx->d_loc_list = d_locs;
    idx->view_bytes = bytes;
    idx->device_bytes += bytes;
    return 0;
}

// the flags of the _ex builders: SX_INDEX_COMPACT, and in bits 8 .. 15 the log2 of a sampling distance, which needs it
static bool index_flags_ok(uint32_t flags)
{
    const uint32_t q = (flags >> 8) & 0xFFu;
    if (flags & ~((uint32_t)SX_INDEX_COMPACT | 0xFF00u)) return false;
    return q == 0 || (sa_sample_log2_ok(q) && (flags & SX_INDEX_COMPACT));
}

static sx_index *new_index(sx_ctx *ctx, uint32_t flags)
{
    const bool compact = (flags & SX_INDEX_COMPACT) != 0;
    sx_index *idx = new (std::nothrow) sx_index;
    if (!idx) return nullptr;
    idx->device = ctx->device;
    idx->compact = compact;
    idx->sa_log2 = (flags >> 8) & 0xFFu;
    g_live_indexes.fetch_add(1);
    return idx;
}

// one record of host tables (the copies are queued; the caller syncs before the host arrays may go)
static int add_tables(sx_ctx *ctx, sx_index *idx, const sx_map_record &M, const uint8_t *string, bool at_front)
{
    sx_index_rec R;
    R.name = M.name;
    R.N = M.N;
    R.sigma = M.sigma;
    memcpy(R.remap, M.remap, 256);
    const size_t o_words = (size_t)(M.N + 1) * M.sigma;
    sx_dev_scope S;
    size_t bytes = 0;
    R.sa_log2 = idx->sa_log2;
    if (R.sa_log2) {
        SX_TRY(S.take(ctx, &R.d_sa_marks, (size_t)sa_mark_bytes(M.N), &bytes));
        SX_TRY(S.take(ctx, &R.d_sa_values, (size_t)sa_sample_count(M.N, R.sa_log2), &bytes));
    } else {
        SX_TRY(S.take(ctx, &R.d_sa, (size_t)M.N, &bytes));
    }
    SX_TRY(S.take(ctx, &R.d_c, (size_t)M.sigma, &bytes));
    if (idx->compact) {
        SX_TRY(S.take(ctx, &R.d_occ, (size_t)occ_bytes(M.N, M.sigma), &bytes));
        if (M.ro_table) SX_TRY(S.take(ctx, &R.d_rocc, (size_t)occ_bytes(M.N, M.sigma), &bytes));
    } else {
        SX_TRY(S.take(ctx, &R.d_o, o_words, &bytes));
        if (M.ro_table) SX_TRY(S.take(ctx, &R.d_ro, o_words, &bytes));
    }
    if (string) SX_TRY(S.take(ctx, &R.d_string, (size_t)M.N, &bytes));
    // (a sampled record's suffix array comes up in windows and leaves as marks and values: it is never resident)
    if (R.sa_log2) SX_TRY(sx_nomem_of(sx_sa_sample_host_impl(ctx, M.sa, M.N, R.sa_log2, R.d_sa_marks, R.d_sa_values)));
    if (!R.sa_log2) SX_CHECK(hipMemcpyAsync(R.d_sa, M.sa, (size_t)M.N * 4, hipMemcpyHostToDevice, ctx->stream));
    SX_CHECK(hipMemcpyAsync(R.d_c, M.c_table, (size_t)M.sigma * 4, hipMemcpyHostToDevice, ctx->stream));
    if (idx->compact) { // the full rows come up in windows and leave as blocks: no table of o_words exists on the device
        SX_TRY(sx_nomem_of(sx_occ_from_rows_impl(ctx, M.o_table, M.N, M.sigma, R.d_occ)));
        if (M.ro_table) SX_TRY(sx_nomem_of(sx_occ_from_rows_impl(ctx, M.ro_table, M.N, M.sigma, R.d_rocc)));
    } else {
        SX_CHECK(hipMemcpyAsync(R.d_o, M.o_table, o_words * 4, hipMemcpyHostToDevice, ctx->stream));
        if (M.ro_table) SX_CHECK(hipMemcpyAsync(R.d_ro, M.ro_table, o_words * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    if (string) {
        if (M.N > 1) SX_CHECK(hipMemcpyAsync(R.d_string, string, (size_t)M.N - 1, hipMemcpyHostToDevice, ctx->stream));
        SX_CHECK(hipMemsetAsync(R.d_string + (M.N - 1), 0, 1, ctx->stream));
    }
    S.keep();
    idx->device_bytes += bytes;
    if (at_front) idx->recs.insert(idx->recs.begin(), R);
    else idx->recs.push_back(R);
    return 0;
}

static int record_check(sx_ctx *ctx, const sx_map_record &R)
{
    if (sx_map_record_check(R, 1)) return 0;
    return sx_fail_msg(ctx, SX_E_ARG, "index: a record lacks its name, suffix array, tables or remap table");
}

// an index of host tables, given as records (no strings) or as sources; every record is checked first
static int from_sources(sx_ctx *ctx, const sx_map_record *records, const sx_index_source *sources, uint32_t n, uint32_t flags, sx_index **out)
{
    for (uint32_t r = 0; r < n; ++r) SX_TRY(record_check(ctx, records ? records[r] : sources[r].record));
    SX_CHECK(hipSetDevice(ctx->device));
    sx_index *idx = new_index(ctx, flags);
    if (!idx) return sx_fail_msg(ctx, SX_E_NOMEM, "index");
    int rc = 0;
    for (uint32_t r = 0; r < n && rc == 0; ++r)
        rc = add_tables(ctx, idx, records ? records[r] : sources[r].record, records ? nullptr : sources[r].string, false);
    if (rc == 0) rc = make_view(ctx, idx); // (ends with a sync: the tables' copies are done too)
    if (rc != 0) {
        (void)hipStreamSynchronize(ctx->stream);
        sx_index_destroy(idx);
        return rc;
    }
    *out = idx;
    return 0;
}

// one FASTA record on the device -> its tables
static int build_record(sx_ctx *ctx, sx_index *idx, const uint8_t *d_seq, uint64_t n, const std::string &name, bool include_reverse)
{
    sx_index_rec R;
    R.name = name;
    R.N = n + 1;
    sx_dev_scope S, T; // S: what the record keeps, T: temporaries
    size_t bytes = 0;
    int16_t t16[256];
    SX_TRY(S.take(ctx, &R.d_string, (size_t)n + 1, &bytes));
    SX_TRY(sx_remap_dev(ctx, d_seq, n, R.d_string, t16, &R.sigma));
    for (int b = 0; b < 256; ++b) R.remap[b] = (signed char)t16[b];
    const uint64_t N = n + 1;
    const uint32_t sigma = R.sigma;
    const size_t o_words = (size_t)(N + 1) * sigma;
    uint8_t *d_bwt;
    // sampled: the suffix array is an allocation of this call, sampled and released before the reverse is built
    uint32_t *d_sa;
    R.sa_log2 = idx->sa_log2;
    if (R.sa_log2) {
        SX_TRY(T.take(ctx, &d_sa, (size_t)N));
    } else {
        SX_TRY(S.take(ctx, &R.d_sa, (size_t)N, &bytes));
        d_sa = R.d_sa;
    }
    SX_TRY(S.take(ctx, &R.d_c, (size_t)sigma, &bytes));
    // compact: the BWT goes straight into the block builder and the table call makes C alone
    const bool compact = idx->compact;
    const size_t occ_b = (size_t)occ_bytes(N, sigma);
    if (compact) SX_TRY(S.take(ctx, &R.d_occ, occ_b, &bytes));
    else SX_TRY(S.take(ctx, &R.d_o, o_words, &bytes));
    SX_TRY(T.take(ctx, &d_bwt, (size_t)N));
    SX_TRY(sx_nomem_of(sx_sa_bwt_build_dev(ctx, R.d_string, n, sigma, d_sa, d_bwt)));
    SX_TRY(sx_nomem_of(sx_bwt_tables_from_bwt_dev(ctx, d_bwt, N, sigma, R.d_c, R.d_o)));
    if (compact) SX_TRY(sx_nomem_of(sx_occ_build_impl(ctx, d_bwt, N, sigma, R.d_occ)));
    if (R.sa_log2) {
        SX_TRY(S.take(ctx, &R.d_sa_marks, (size_t)sa_mark_bytes(N), &bytes));
        SX_TRY(S.take(ctx, &R.d_sa_values, (size_t)sa_sample_count(N, R.sa_log2), &bytes));
        SX_TRY(sx_nomem_of(sx_sa_sample_dev_impl(ctx, d_sa, N, R.sa_log2, R.d_sa_marks, R.d_sa_values))); // (ends with a sync)
        T.drop(d_sa);
    }
    if (include_reverse) { // bwt.c:147-158: the reversed string's suffix array is temporary, its O table is RO
        uint8_t *d_rev;
        uint32_t *d_rsa, *d_rc;
        if (compact) SX_TRY(S.take(ctx, &R.d_rocc, occ_b, &bytes));
        else SX_TRY(S.take(ctx, &R.d_ro, o_words, &bytes));
        SX_TRY(T.take(ctx, &d_rev, (size_t)N));
        SX_TRY(T.take(ctx, &d_rsa, (size_t)N));
        SX_TRY(T.take(ctx, &d_rc, (size_t)sigma));
        SX_TRY(sx_reverse_dev(ctx, R.d_string, n, d_rev));
        SX_TRY(sx_nomem_of(sx_sa_bwt_build_dev(ctx, d_rev, n, sigma, d_rsa, d_bwt)));
        SX_TRY(sx_nomem_of(sx_bwt_tables_from_bwt_dev(ctx, d_bwt, N, sigma, d_rc, R.d_ro)));
        if (compact) SX_TRY(sx_nomem_of(sx_occ_build_impl(ctx, d_bwt, N, sigma, R.d_rocc)));
    }
    SX_TRY(sx_sync(ctx));
    S.keep();
    idx->device_bytes += bytes;
    idx->recs.push_back(R);
    return 0;
}

static int build_fasta(sx_ctx *ctx, sx_index *idx, const uint8_t *fasta, uint64_t len, bool include_reverse)
{
    // every record but the first starts at a '>', and every record has two terminators: a bound for the table
    uint64_t starts = 1;
    for (const uint8_t *p = fasta, *end = fasta + len; p < end && (p = (const uint8_t *)memchr(p, '>', (size_t)(end - p))) != nullptr; ++p) ++starts;
    const uint64_t term_cap = 2 * starts + 2;
    sx_dev_scope T;
    uint8_t *d_file, *d_packed;
    uint32_t *d_term;
    SX_TRY(T.take(ctx, &d_file, (size_t)len + 16));
    SX_TRY(T.take(ctx, &d_packed, (size_t)len + 17));
    SX_TRY(T.take(ctx, &d_term, (size_t)term_cap));
    SX_TRY(sx_upload_staged(ctx, d_file, fasta, (size_t)len));
    uint64_t packed_len = 0;
    uint32_t n_rec = 0;
    SX_TRY(sx_nomem_of(sx_fasta_pack_dev(ctx, d_file, len, d_packed, &packed_len, d_term, term_cap, &n_rec)));
    T.drop(d_file);
    if (2ull * n_rec > term_cap) return sx_fail_msg(ctx, SX_E_INTERNAL, "index: more records than '>' bytes");
    std::vector<uint32_t> term(2 * (size_t)n_rec + 1);
    if (n_rec) SX_CHECK(hipMemcpyAsync(term.data(), d_term, 2 * (size_t)n_rec * 4, hipMemcpyDeviceToHost, ctx->stream));
    SX_TRY(sx_sync(ctx));
    for (uint32_t r = 0; r < n_rec; ++r) {
        const uint32_t name_at = r ? term[2 * r - 1] + 1 : 0, name_len = term[2 * r] - name_at;
        const uint32_t seq_at = term[2 * r] + 1, seq_len = term[2 * r + 1] - seq_at;
        std::string name(name_len, '\0');
        if (name_len) SX_CHECK(hipMemcpyAsync(&name[0], d_packed + name_at, name_len, hipMemcpyDeviceToHost, ctx->stream));
        SX_TRY(sx_sync(ctx));
        SX_TRY(build_record(ctx, idx, d_packed + seq_at, seq_len, name, include_reverse));
    }
    return make_view(ctx, idx);
}

} // namespace sx

using namespace sx;

int sx_index_from_records_impl(sx_ctx *ctx, const sx_map_record *records, uint32_t n_records, sx_index **out)
{
    return from_sources(ctx, records, nullptr, n_records, 0, out);
}

extern "C" {

void sx_fastq_dev_free(sx_fastq_dev *fq)
{
    if (!fq) return;
    (void)hipFree(fq->d_names), (void)hipFree(fq->d_seqs), (void)hipFree(fq->d_quals);
    (void)hipFree(fq->d_name_off), (void)hipFree(fq->d_seq_off), (void)hipFree(fq->d_qual_off);
    memset(fq, 0, sizeof *fq);
}

static int fastq_index_dev(sx_ctx *ctx, const uint8_t *d_image, uint64_t len, sx_fastq_dev *out)
{
    sx_dev_scope S;
    const uint32_t ntiles = sx_div_up(len, kFqTile);
    // scratch: a few scalars and two u32 a tile (slab M); the line ends and the lengths (slab N, sized once the lines are counted)
    SX_TRY(sx_slab_ensure(ctx, SX_SLAB_M, 256 + 2 * (size_t)(ntiles + 1) * sizeof(uint32_t)));
    uint32_t *scal = (uint32_t *)ctx->slab[SX_SLAB_M].p; // [0] error bits, [1] no final newline, [2] newlines, [4..6] totals
    uint32_t *tile_nl = scal + 64, *tile_base = tile_nl + ntiles + 1;
    SX_CHECK(hipMemsetAsync(scal, 0, 256, ctx->stream));
    uint32_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (len) {
        sx_launch(ctx, SX_KC_FASTA, len, fq_count_kernel, dim3(ntiles), dim3(kBlock), d_image, len, tile_nl, scal);
        SX_TRY((device_scan<OpAdd>(ctx, ntiles, InU32{tile_nl}, OutExclusive{tile_base}, scal + 2, SX_KC_FASTA, 0)));
        SX_TRY(sx_readback(ctx, scal, 3, h));
    }
    const uint64_t n_newlines = h[2], n_lines = n_newlines + h[1];
    // a NUL inside a record; a line count that is no multiple of four (a record cut off, a blank line somewhere)
    if (h[0] || (n_lines & 3u)) return sx_fail_msg(ctx, SX_E_MALFORMED, "malformed FASTQ image (see sx_fastq_index)");
    const uint32_t count = (uint32_t)(n_lines / 4);
    SX_TRY(S.take(ctx, &out->d_name_off, (size_t)count + 1));
    SX_TRY(S.take(ctx, &out->d_seq_off, (size_t)count + 1));
    SX_TRY(S.take(ctx, &out->d_qual_off, (size_t)count + 1));
    if (count == 0) {
        SX_CHECK(hipMemsetAsync(out->d_name_off, 0, 4, ctx->stream));
        SX_CHECK(hipMemsetAsync(out->d_seq_off, 0, 4, ctx->stream));
        SX_CHECK(hipMemsetAsync(out->d_qual_off, 0, 4, ctx->stream));
        SX_TRY(S.take(ctx, &out->d_names, 16));
        SX_TRY(S.take(ctx, &out->d_seqs, 16));
        SX_TRY(S.take(ctx, &out->d_quals, 16));
        SX_TRY(sx_sync(ctx));
        S.keep();
        return 0;
    }
    const size_t lens_b = (((size_t)count + 1) * 4 + 255) & ~(size_t)255;
    int rc = sx_slab_ensure(ctx, SX_SLAB_N, (((size_t)n_lines * 4 + 255) & ~(size_t)255) + 3 * lens_b);
    uint32_t *line_end = nullptr, *lens[3] = {nullptr, nullptr, nullptr};
    if (rc == 0) {
        line_end = (uint32_t *)ctx->slab[SX_SLAB_N].p;
        for (int k = 0; k < 3; ++k) lens[k] = (uint32_t *)((char *)line_end + (((size_t)n_lines * 4 + 255) & ~(size_t)255) + (size_t)k * lens_b);
        sx_launch(ctx, SX_KC_FASTA, len + n_lines * 4, fq_line_end_kernel, dim3(ntiles), dim3(kBlock), d_image, len,
                  (const uint32_t *)tile_base, line_end, (uint32_t)n_newlines, (uint32_t)n_lines);
        sx_launch(ctx, SX_KC_FASTA, (uint64_t)count * 28, fq_record_kernel, dim3(sx_div_up((uint64_t)count + 1, kBlock)), dim3(kBlock),
                  (const uint32_t *)line_end, count, lens[0], lens[1], lens[2], scal);
        uint32_t *offs[3] = {out->d_name_off, out->d_seq_off, out->d_qual_off};
        for (int k = 0; k < 3 && rc == 0; ++k)
            rc = device_scan<OpAdd>(ctx, (uint64_t)count + 1, InU32{lens[k]}, OutExclusive{offs[k]}, scal + 4 + k, SX_KC_FASTA, 0);
        if (rc == 0) rc = sx_readback(ctx, scal, 7, h);
        if (rc == 0 && h[0]) rc = sx_fail_msg(ctx, SX_E_MALFORMED, "malformed FASTQ image (see sx_fastq_index)");
    }
    if (rc == 0) rc = S.take(ctx, &out->d_names, (size_t)h[4] + 16);
    if (rc == 0) rc = S.take(ctx, &out->d_seqs, (size_t)h[5] + 16);
    if (rc == 0) rc = S.take(ctx, &out->d_quals, (size_t)h[6] + 16);
    if (rc == 0) {
        // (every line has passed its checks: each byte's place lies inside the three totals)
        sx_launch(ctx, SX_KC_FASTA, 2 * len, fq_scatter_kernel, dim3(ntiles), dim3(kBlock), d_image, len, (const uint32_t *)tile_base,
                  (const uint32_t *)tile_nl, (const uint32_t *)line_end, (const uint32_t *)out->d_name_off, (const uint32_t *)out->d_seq_off,
                  (const uint32_t *)out->d_qual_off, out->d_names, out->d_seqs, out->d_quals, (uint32_t)n_lines);
        rc = sx_sync(ctx);
    }
    if (rc != 0) return rc; // (S releases what was taken)
    out->count = count;
    out->name_bytes = h[4], out->seq_bytes = h[5], out->qual_bytes = h[6];
    S.keep();
    return 0;
}

int sx_fastq_index_dev(sx_ctx *ctx, const uint8_t *d_image, uint64_t len, sx_fastq_dev *out)
{
    if (!ctx || !out || (len && !d_image)) return SX_E_ARG;
    memset(out, 0, sizeof *out);
    if (len > 0xFFFFFFFEull) return sx_fail_msg(ctx, SX_E_ARG, "FASTQ image must be shorter than 2^32 - 1 bytes");
    SX_CHECK(hipSetDevice(ctx->device));
    const int rc = fastq_index_dev(ctx, d_image, len, out);
    if (rc != 0) memset(out, 0, sizeof *out); // (what was allocated has been released)
    return sx_nomem_of(rc);
}

int sx_index_live_count(void) { return g_live_indexes.load(); }

int sx_download(sx_ctx *ctx, void *h_dst, const void *d_src, size_t bytes)
{
    if (!ctx || (bytes && (!h_dst || !d_src))) return SX_E_ARG;
    SX_CHECK(hipSetDevice(ctx->device));
    if (bytes) SX_CHECK(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return sx_sync(ctx);
}

void sx_index_destroy(sx_index *idx)
{
    if (!idx) return;
    int before = 0;
    const bool switched = hipGetDevice(&before) == hipSuccess && before != idx->device && hipSetDevice(idx->device) == hipSuccess;
    for (sx_index_rec &R : idx->recs) free_rec(R);
    free_view(idx);
    if (switched) (void)hipSetDevice(before);
    delete idx;
    g_live_indexes.fetch_sub(1);
}

int sx_index_build_fasta(sx_ctx *ctx, const uint8_t *fasta, uint64_t len, int include_reverse, sx_index **out)
{
    return sx_index_build_fasta_ex(ctx, fasta, len, include_reverse, 0, out);
}

int sx_index_build_fasta_ex(sx_ctx *ctx, const uint8_t *fasta, uint64_t len, int include_reverse, uint32_t flags, sx_index **out)
{
    if (!ctx || !out || (len && !fasta)) return SX_E_ARG;
    *out = nullptr;
    if (!index_flags_ok(flags)) return sx_fail_msg(ctx, SX_E_ARG, "index: unknown flags, or a sampling distance without SX_INDEX_COMPACT or outside 2^1 .. 2^10");
    if (len >= 0x7FFFFFFFull) return sx_fail_msg(ctx, SX_E_ARG, "FASTA image must be shorter than 2^31 - 1 bytes");
    SX_CHECK(hipSetDevice(ctx->device));
    sx_index *idx = new_index(ctx, flags);
    if (!idx) return sx_fail_msg(ctx, SX_E_NOMEM, "index");
    const int rc = build_fasta(ctx, idx, fasta, len, include_reverse != 0);
    if (rc != 0) {
        (void)hipStreamSynchronize(ctx->stream);
        sx_index_destroy(idx);
        return sx_nomem_of(rc);
    }
    *out = idx;
    return 0;
}

int sx_index_from_tables(sx_ctx *ctx, const sx_map_record *records, uint32_t n_records, sx_index **out)
{
    if (!ctx || !out || (n_records && !records)) return SX_E_ARG;
    *out = nullptr;
    return from_sources(ctx, records, nullptr, n_records, 0, out);
}

int sx_index_from_sources(sx_ctx *ctx, const sx_index_source *sources, uint32_t n_records, sx_index **out)
{
    if (!ctx || !out || (n_records && !sources)) return SX_E_ARG;
    *out = nullptr;
    return from_sources(ctx, nullptr, sources, n_records, 0, out);
}

int sx_index_from_sources_ex(sx_ctx *ctx, const sx_index_source *sources, uint32_t n_records, uint32_t flags, sx_index **out)
{
    if (!ctx || !out || (n_records && !sources)) return SX_E_ARG;
    *out = nullptr;
    if (!index_flags_ok(flags)) return sx_fail_msg(ctx, SX_E_ARG, "index: unknown flags, or a sampling distance without SX_INDEX_COMPACT or outside 2^1 .. 2^10");
    return sx_nomem_of(from_sources(ctx, nullptr, sources, n_records, flags, out));
}

int sx_index_add_record(sx_ctx *ctx, sx_index *idx, const sx_index_source *source, int at_front)
{
    if (!ctx || !idx || !source) return SX_E_ARG;
    if (idx->device != ctx->device) return sx_fail_msg(ctx, SX_E_ARG, "index: it lives on another device than this context");
    SX_TRY(record_check(ctx, source->record));
    SX_CHECK(hipSetDevice(ctx->device));
    const int rc = add_tables(ctx, idx, source->record, source->string, at_front != 0);
    if (rc != 0) {
        (void)hipStreamSynchronize(ctx->stream);
        return sx_nomem_of(rc);
    }
    return make_view(ctx, idx);
}

int sx_index_info(const sx_index *idx, uint32_t *n_records_out, int *device_out, int *has_ro_out, uint64_t *device_bytes_out)
{
    if (!idx) return SX_E_ARG;
    if (n_records_out) *n_records_out = (uint32_t)idx->recs.size();
    if (device_out) *device_out = idx->device;
    if (has_ro_out) {
        *has_ro_out = idx->recs.empty() ? 0 : 1;
        for (const sx_index_rec &R : idx->recs)
            if (!R.has_ro()) *has_ro_out = 0;
    }
    if (device_bytes_out) *device_bytes_out = idx->device_bytes;
    return 0;
}

int sx_index_record_info(const sx_index *idx, uint32_t record, sx_index_record *out)
{
    if (!idx || !out || record >= idx->recs.size()) return SX_E_ARG;
    const sx_index_rec &R = idx->recs[record];
    out->name = R.name.c_str();
    out->N = R.N;
    out->sigma = R.sigma;
    out->has_ro = R.has_ro() ? 1 : 0;
    out->has_string = R.d_string ? 1 : 0;
    out->remap = R.remap;
    out->d_string = R.d_string;
    out->d_sa = R.d_sa, out->d_c = R.d_c, out->d_o = R.d_o, out->d_ro = R.d_ro;
    return 0;
}

int sx_index_record_occ(const sx_index *idx, uint32_t record, sx_index_occ *out)
{
    if (!idx || !out || record >= idx->recs.size()) return SX_E_ARG;
    const sx_index_rec &R = idx->recs[record];
    memset(out, 0, sizeof *out);
    out->compact = R.d_occ ? 1 : 0;
    if (R.d_occ) {
        out->d_occ = R.d_occ, out->d_rocc = R.d_rocc;
        out->stride = occ_stride(R.sigma), out->sigma_pad = occ_sigma_pad(R.sigma);
        out->n_blocks = occ_blocks(R.N);
    }
    return 0;
}

int sx_index_is_compact(const sx_index *idx) { return idx && idx->compact ? 1 : 0; }

int sx_index_record_samples(const sx_index *idx, uint32_t record, sx_index_samples *out)
{
    if (!idx || !out || record >= idx->recs.size()) return SX_E_ARG;
    const sx_index_rec &R = idx->recs[record];
    memset(out, 0, sizeof *out);
    if (R.sa_log2) {
        out->d_marks = R.d_sa_marks, out->d_values = R.d_sa_values;
        out->sa_log2 = R.sa_log2;
        out->n_samples = sa_sample_count(R.N, R.sa_log2);
        out->n_blocks = occ_blocks(R.N);
    }
    return 0;
}

static int expand_sink(void *user, int, const void *data, size_t bytes)
{
    char **at = (char **)user;
    memcpy(*at, data, bytes);
    *at += bytes;
    return 0;
}

int sx_index_expand_o(sx_ctx *ctx, const sx_index *idx, uint32_t record, int reverse, uint64_t row_lo, uint64_t row_hi, uint32_t *rows_out)
{
    if (!ctx || !idx || record >= idx->recs.size()) return SX_E_ARG;
    if (idx->device != ctx->device) return sx_fail_msg(ctx, SX_E_ARG, "index: it lives on another device than this context");
    const sx_index_rec &R = idx->recs[record];
    const uint8_t *blocks = reverse ? R.d_rocc : R.d_occ;
    if (!blocks) return sx_fail_msg(ctx, SX_E_ARG, "index: the record has no blocks of this table");
    if (row_lo > row_hi || row_hi > R.N + 1 || (row_hi > row_lo && !rows_out)) return sx_fail_msg(ctx, SX_E_ARG, "index: the rows to expand lie in [0, N]");
    SX_CHECK(hipSetDevice(ctx->device));
    char *at = (char *)rows_out;
    return sx_nomem_of(sx_occ_stream_rows(ctx, SX_SECTION_INDEX, blocks, R.N, R.sigma, row_lo, row_hi, expand_sink, &at));
}

int sx_index_expand_sa(sx_ctx *ctx, const sx_index *idx, uint32_t record, uint64_t row_lo, uint64_t row_hi, uint32_t *rows_out)
{
    if (!ctx || !idx || record >= idx->recs.size()) return SX_E_ARG;
    if (idx->device != ctx->device) return sx_fail_msg(ctx, SX_E_ARG, "index: it lives on another device than this context");
    const sx_index_rec &R = idx->recs[record];
    if (!R.sa_log2) return sx_fail_msg(ctx, SX_E_ARG, "index: the record keeps its whole suffix array");
    if (row_lo > row_hi || row_hi > R.N || (row_hi > row_lo && !rows_out)) return sx_fail_msg(ctx, SX_E_ARG, "index: the rows to expand lie in [0, N)");
    SX_CHECK(hipSetDevice(ctx->device));
    char *at = (char *)rows_out;
    return sx_nomem_of(sx_sa_stream_rows(ctx, SX_SECTION_INDEX, loc_rec_of(R.d_c, R.d_occ, R.N, R.sigma, R.d_sa_marks, R.d_sa_values, R.sa_log2), row_lo,
                                         row_hi, expand_sink, &at));
}

int sx_index_map_reads(sx_ctx *ctx, const sx_index *idx, const uint8_t *fastq, size_t fastq_len, int edits, sx_sink_fn sink, void *user)
{
    if (!ctx || !idx || !sink || (fastq_len && !fastq)) return SX_E_ARG;
    if (idx->device != ctx->device) return sx_fail_msg(ctx, SX_E_ARG, "index: it lives on another device than this context");
    if (edits < 0 || edits > SX_APPROX_MAX_EDITS) return sx_fail_msg(ctx, SX_E_ARG, "read mapping: edits must be in [0, 8]");
    if (fastq_len > 0xFFFFFFFEull) return sx_fail_msg(ctx, SX_E_ARG, "read mapping: malformed FASTQ image (see sx_fastq_index)");
    SX_CHECK(hipSetDevice(ctx->device));
    sx_fastq_dev fq;
    memset(&fq, 0, sizeof fq);
    {
        sx_dev_scope T;
        uint8_t *d_image;
        SX_TRY(T.take(ctx, &d_image, fastq_len + 16));
        SX_TRY(sx_upload_staged(ctx, d_image, fastq, fastq_len));
        const int frc = sx_fastq_index_dev(ctx, d_image, fastq_len, &fq);
        if (frc == SX_E_MALFORMED || frc == SX_E_ARG) return sx_fail_msg(ctx, frc, "read mapping: malformed FASTQ image (see sx_fastq_index)");
        if (frc != 0) return frc;
    }
    sx_reads_dev reads;
    reads.count = fq.count;
    reads.d_names = fq.d_names, reads.d_seqs = fq.d_seqs, reads.d_quals = fq.d_quals;
    reads.d_name_off = fq.d_name_off, reads.d_seq_off = fq.d_seq_off, reads.d_qual_off = fq.d_qual_off;
    reads.seq_bytes = fq.seq_bytes;
    const int rc = sx_map_reads_core(ctx, idx, reads, edits, sink, user);
    sx_fastq_dev_free(&fq);
    return rc;
}

int sx_index_write(sx_ctx *ctx, const sx_index *idx, sx_sink_fn sink, void *user)
{
    if (!ctx || !idx || !sink) return SX_E_ARG;
    if (idx->device != ctx->device) return sx_fail_msg(ctx, SX_E_ARG, "index: it lives on another device than this context");
    for (const sx_index_rec &R : idx->recs)
        if (!R.d_string) return sx_fail_msg(ctx, SX_E_ARG, "index: a record was given without its string and cannot be written");
    SX_CHECK(hipSetDevice(ctx->device));
    auto put = [&](const void *p, size_t n) { return sink(user, SX_SECTION_INDEX, p, n) != 0 ? sx_fail_msg(ctx, SX_E_ARG, "the sink refused a chunk") : 0; };
    const uint32_t n_rec = (uint32_t)idx->recs.size();
    SX_TRY(put(&n_rec, 4));
    for (uint32_t r = n_rec; r-- > 0;) { // last record first, as the mapper's -p writes them
        const sx_index_rec &R = idx->recs[r];
        const uint32_t name_bytes = (uint32_t)R.name.size() + 1, n = (uint32_t)(R.N - 1);
        const size_t o_bytes = (size_t)(R.N + 1) * R.sigma * 4;
        SX_TRY(put(&name_bytes, 4));
        SX_TRY(put(R.name.c_str(), name_bytes));
        // stralg/serialise.c:7-18: string (u32 length, bytes), suffix array, remap table, C, O, flag, RO
        SX_TRY(put(&n, 4));
        SX_TRY(sx_stream_to_sink(ctx, SX_SECTION_INDEX, R.d_string, n, sink, user));
        // (a sampled record's suffix array is located window by window: the same bytes)
        if (R.sa_log2)
            SX_TRY(sx_nomem_of(sx_sa_stream_rows(ctx, SX_SECTION_INDEX, loc_rec_of(R.d_c, R.d_occ, R.N, R.sigma, R.d_sa_marks, R.d_sa_values, R.sa_log2),
                                                 0, R.N, sink, user)));
        if (!R.sa_log2) SX_TRY(sx_stream_to_sink(ctx, SX_SECTION_INDEX, R.d_sa, (size_t)R.N * 4, sink, user));
        struct { // stralg/remap.h:9-19
            uint32_t alphabet_size;
            signed char table[256], rev_table[128];
        } rt;
        rt.alphabet_size = R.sigma;
        memcpy(rt.table, R.remap, 256);
        memset(rt.rev_table, -1, 128);
        rt.rev_table[0] = 0;
        for (int c = 1; c < 256; ++c)
            if (R.remap[c] > 0) rt.rev_table[(int)R.remap[c]] = (signed char)c;
        SX_TRY(put(&rt, sizeof rt));
        SX_TRY(sx_stream_to_sink(ctx, SX_SECTION_INDEX, R.d_c, (size_t)R.sigma * 4, sink, user));
        // (a compact record's tables are expanded window by window: the same bytes)
        if (R.d_occ) SX_TRY(sx_nomem_of(sx_occ_stream_rows(ctx, SX_SECTION_INDEX, R.d_occ, R.N, R.sigma, 0, R.N + 1, sink, user)));
        else SX_TRY(sx_stream_to_sink(ctx, SX_SECTION_INDEX, R.d_o, o_bytes, sink, user));
        const uint8_t has_ro = R.has_ro() ? 1 : 0; // (a bool in the reference: one byte)
        SX_TRY(put(&has_ro, 1));
        if (R.d_rocc) SX_TRY(sx_nomem_of(sx_occ_stream_rows(ctx, SX_SECTION_INDEX, R.d_rocc, R.N, R.sigma, 0, R.N + 1, sink, user)));
        else if (R.d_ro) SX_TRY(sx_stream_to_sink(ctx, SX_SECTION_INDEX, R.d_ro, o_bytes, sink, user));
    }
    return sx_sync(ctx);
}

} // extern "C"
