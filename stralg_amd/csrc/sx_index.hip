// sx_index.hip -- a device-resident index: build from FASTA once, map many read sets.
//
// The index holds, for every FASTA record, the remapped string, SA, C, O and RO (in one of the three forms of
// sx_index.hpp) in device allocations of its own (not slabs of a context's cache), so that a context can be trimmed or
// used for other builds while an index lives.
#include "sx_common.hpp"
#include "sx_hostio.hpp"
#include "sx_index.hpp"

#include <atomic>
#include <new>

namespace sx {

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
        (void)hipFree(idx->d_sa_lens), (void)hipFree(idx->d_loc_list), (void)hipFree(idx->d_letters), (void)hipFree((void *)idx->d_text_list);
    idx->d_loc_list = nullptr;
    idx->d_text_list = nullptr;
    idx->d_rnames = idx->d_tabs = idx->d_letters = nullptr, idx->d_rname_off = nullptr, idx->d_sa_list = nullptr, idx->d_sa_lens = nullptr;
    idx->device_bytes -= idx->view_bytes;
    idx->view_bytes = 0;
}

// what the mapper's kernels read of the records, uploaded again after every change of the record list
static int make_view(sx_ctx *ctx, sx_index *idx)
{
    free_view(idx);
    const size_t n = idx->recs.size();
    std::vector<uint8_t> rnames, tabs(n * 256 + 1), letters(n * 256 + 1);
    std::vector<const uint8_t *> texts(n + 1);
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
        sx_map_letters_of(R.remap, R.sigma, &letters[r * 256]);
        texts[r] = R.d_string;
        sa_ptrs[r] = R.d_sa;
        sa_lens[r] = R.N;
        if (idx->sa_log2) locs[r] = R.loc();
    }
    rname_off[n] = (uint32_t)rnames.size();
    rnames.push_back(0);
    sx_dev_scope S;
    size_t bytes = 0;
    uint8_t *d_rnames, *d_tabs, *d_letters;
    const uint8_t **d_text_list;
    uint32_t *d_rname_off;
    const uint32_t **d_sa_list;
    uint64_t *d_sa_lens;
    SX_TRY(S.take(ctx, &d_rnames, rnames.size(), &bytes));
    SX_TRY(S.take(ctx, &d_tabs, tabs.size(), &bytes));
    SX_TRY(S.take(ctx, &d_rname_off, rname_off.size(), &bytes));
    SX_TRY(S.take(ctx, &d_sa_list, sa_ptrs.size(), &bytes));
    SX_TRY(S.take(ctx, &d_sa_lens, sa_lens.size(), &bytes));
    SX_TRY(S.take(ctx, &d_letters, letters.size(), &bytes));
    SX_TRY(S.take(ctx, &d_text_list, texts.size(), &bytes));
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
    SX_CHECK(hipMemcpyAsync(d_letters, letters.data(), letters.size(), hipMemcpyHostToDevice, ctx->stream));
    SX_CHECK(hipMemcpyAsync(d_text_list, texts.data(), texts.size() * sizeof(void *), hipMemcpyHostToDevice, ctx->stream));
    SX_TRY(sx_sync(ctx)); // (the host vectors are pageable: their copies are done)
    S.keep();
    idx->d_rnames = d_rnames, idx->d_tabs = d_tabs, idx->d_rname_off = d_rname_off, idx->d_sa_list = d_sa_list, idx->d_sa_lens = d_sa_lens;
    idx->d_loc_list = d_locs;
    idx->d_letters = d_letters, idx->d_text_list = d_text_list;
    idx->view_bytes = bytes;
    idx->device_bytes += bytes;
    return 0;
}

// the flags of the _ex builders: SX_INDEX_COMPACT, SX_INDEX_PACKED, which needs it, and in bits 8 .. 15 the log2 of a
// sampling distance, which needs it too
static int flags_check(sx_ctx *ctx, uint32_t flags)
{
    const uint32_t q = (flags >> 8) & 0xFFu;
    const bool known = !(flags & ~((uint32_t)SX_INDEX_COMPACT | (uint32_t)SX_INDEX_PACKED | 0xFF00u));
    const bool compact = (flags & SX_INDEX_COMPACT) != 0;
    if (known && (q == 0 || (sa_sample_log2_ok(q) && compact)) && (!(flags & SX_INDEX_PACKED) || compact)) return 0;
    return sx_fail_msg(ctx, SX_E_ARG,
                       "index: unknown flags, or SX_INDEX_PACKED or a sampling distance without SX_INDEX_COMPACT, or a distance outside 2^1 .. 2^10");
}

// a packed index holds records of at most 8 symbols (the sentinel among them): there is no other form for the others
static int packed_sigma_check(sx_ctx *ctx, const sx_index *idx, uint32_t sigma)
{
    if (!idx->packed || sigma <= kOccPackedMaxSigma) return 0;
    return sx_fail_msg(ctx, SX_E_ARG, "index: a record of more than 8 symbols (7 letters) does not fit the packed form");
}

static int device_check(sx_ctx *ctx, const sx_index *idx)
{
    return idx->device == ctx->device ? 0 : sx_fail_msg(ctx, SX_E_ARG, "index: it lives on another device than this context");
}

// the end of a call that makes an index: it goes to the caller, or goes altogether
static int finish_index(sx_ctx *ctx, sx_index *idx, int rc, sx_index **out)
{
    if (rc == 0) return *out = idx, 0;
    (void)hipStreamSynchronize(ctx->stream);
    sx_index_destroy(idx);
    return rc;
}

static sx_index *new_index(sx_ctx *ctx, uint32_t flags)
{
    sx_index *idx = new (std::nothrow) sx_index;
    if (!idx) return nullptr;
    idx->device = ctx->device;
    idx->compact = (flags & SX_INDEX_COMPACT) != 0;
    idx->packed = (flags & SX_INDEX_PACKED) != 0;
    idx->sa_log2 = (flags >> 8) & 0xFFu;
    g_live_indexes.fetch_add(1);
    return idx;
}

// Every array that a record of R's N, sigma and sa_log2 keeps in the given form (sx_index.hpp), taken into S; *bytes
// grows by what they occupy.  Both ways to a record (host tables, a build from FASTA) allocate through this.
static int take_arrays(sx_ctx *ctx, sx_dev_scope &S, sx_index_rec &R, bool compact, bool want_ro, bool want_string, size_t *bytes)
{
    const size_t o_words = (size_t)(R.N + 1) * R.sigma, occ_b = (size_t)occ_form_bytes(R.N, R.sigma, R.packed);
    if (R.sampled()) {
        SX_TRY(S.take(ctx, &R.d_sa_marks, (size_t)sa_mark_bytes(R.N), bytes));
        SX_TRY(S.take(ctx, &R.d_sa_values, (size_t)sa_sample_count(R.N, R.sa_log2), bytes));
    } else {
        SX_TRY(S.take(ctx, &R.d_sa, (size_t)R.N, bytes));
    }
    SX_TRY(S.take(ctx, &R.d_c, (size_t)R.sigma, bytes));
    if (compact) {
        SX_TRY(S.take(ctx, &R.d_occ, occ_b, bytes));
        if (want_ro) SX_TRY(S.take(ctx, &R.d_rocc, occ_b, bytes));
    } else {
        SX_TRY(S.take(ctx, &R.d_o, o_words, bytes));
        if (want_ro) SX_TRY(S.take(ctx, &R.d_ro, o_words, bytes));
    }
    if (want_string) SX_TRY(S.take(ctx, &R.d_string, (size_t)R.N, bytes));
    return 0;
}

// one record of host tables (the copies are queued; the caller syncs before the host arrays may go)
static int add_tables(sx_ctx *ctx, sx_index *idx, const sx_map_record &M, const uint8_t *string, bool at_front)
{
    sx_index_rec R;
    R.name = M.name;
    R.N = M.N, R.sigma = M.sigma, R.sa_log2 = idx->sa_log2, R.packed = idx->packed;
    SX_TRY(packed_sigma_check(ctx, idx, R.sigma));
    memcpy(R.remap, M.remap, 256);
    const size_t o_words = (size_t)(M.N + 1) * M.sigma;
    sx_dev_scope S;
    size_t bytes = 0;
    SX_TRY(take_arrays(ctx, S, R, idx->compact, M.ro_table != nullptr, string != nullptr, &bytes));
    // (a sampled record's suffix array comes up in windows and leaves as marks and values: it is never resident)
    if (R.sampled()) SX_TRY(sx_nomem_of(sx_sa_sample_host_impl(ctx, M.sa, M.N, R.sa_log2, R.d_sa_marks, R.d_sa_values)));
    else SX_CHECK(hipMemcpyAsync(R.d_sa, M.sa, (size_t)M.N * 4, hipMemcpyHostToDevice, ctx->stream));
    SX_CHECK(hipMemcpyAsync(R.d_c, M.c_table, (size_t)M.sigma * 4, hipMemcpyHostToDevice, ctx->stream));
    if (R.compact()) { // the full rows come up in windows and leave as blocks: no table of o_words exists on the device
        SX_TRY(sx_nomem_of(sx_occ_from_rows_impl(ctx, M.o_table, M.N, M.sigma, R.d_occ, R.packed)));
        if (M.ro_table) SX_TRY(sx_nomem_of(sx_occ_from_rows_impl(ctx, M.ro_table, M.N, M.sigma, R.d_rocc, R.packed)));
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
    idx->recs.insert(at_front ? idx->recs.begin() : idx->recs.end(), R);
    return 0;
}

static int record_check(sx_ctx *ctx, const sx_map_record &R)
{
    if (sx_map_record_check(R, 1)) return 0;
    return sx_fail_msg(ctx, SX_E_ARG, "index: a record lacks its name, suffix array, tables or remap table");
}

// The body of the from_* entry points: an index of host tables, given as records (no strings) or as sources; the
// arguments, the flags and every record are checked before anything is made
static int from_tables(sx_ctx *ctx, const sx_map_record *records, const sx_index_source *sources, uint32_t n, uint32_t flags, sx_index **out)
{
    if (!ctx || !out || (n && !records && !sources)) return SX_E_ARG;
    *out = nullptr;
    SX_TRY(flags_check(ctx, flags));
    for (uint32_t r = 0; r < n; ++r) SX_TRY(record_check(ctx, records ? records[r] : sources[r].record));
    if (flags & SX_INDEX_PACKED)
        for (uint32_t r = 0; r < n; ++r)
            if ((records ? records[r] : sources[r].record).sigma > kOccPackedMaxSigma)
                return sx_fail_msg(ctx, SX_E_ARG, "index: a record of more than 8 symbols (7 letters) does not fit the packed form");
    SX_CHECK(hipSetDevice(ctx->device));
    sx_index *idx = new_index(ctx, flags);
    if (!idx) return sx_fail_msg(ctx, SX_E_NOMEM, "index");
    int rc = 0;
    for (uint32_t r = 0; r < n && rc == 0; ++r)
        rc = add_tables(ctx, idx, records ? records[r] : sources[r].record, records ? nullptr : sources[r].string, false);
    if (rc == 0) rc = make_view(ctx, idx); // (ends with a sync: the tables' copies are done too)
    return finish_index(ctx, idx, rc, out);
}

// One FASTA record on the device -> its tables.  Everything the record keeps is taken before the first pass: the peak
// is that of the reverse pass (or, without one, of the forward pass's last step), which holds all of it either way.
static int build_record(sx_ctx *ctx, sx_index *idx, const uint8_t *d_seq, uint64_t n, const std::string &name, bool include_reverse)
{
    sx_index_rec R;
    R.name = name;
    R.N = n + 1, R.sa_log2 = idx->sa_log2, R.packed = idx->packed;
    sx_dev_scope S, T; // S: what the record keeps, T: temporaries
    size_t bytes = 0;
    int16_t t16[256];
    SX_TRY(S.take(ctx, &R.d_string, (size_t)n + 1, &bytes));
    SX_TRY(sx_remap_dev(ctx, d_seq, n, R.d_string, t16, &R.sigma));
    for (int b = 0; b < 256; ++b) R.remap[b] = (signed char)t16[b];
    SX_TRY(packed_sigma_check(ctx, idx, R.sigma)); // (the whole build fails: what it has made so far goes with the index)
    const uint64_t N = n + 1;
    const uint32_t sigma = R.sigma;
    SX_TRY(take_arrays(ctx, S, R, idx->compact, include_reverse, false, &bytes));
    uint8_t *d_bwt;
    // sampled: the suffix array is an allocation of this call, sampled and released before the reverse is built
    uint32_t *d_sa = R.d_sa;
    if (R.sampled()) SX_TRY(T.take(ctx, &d_sa, (size_t)N));
    SX_TRY(T.take(ctx, &d_bwt, (size_t)N));
    SX_TRY(sx_nomem_of(sx_sa_bwt_build_dev(ctx, R.d_string, n, sigma, d_sa, d_bwt)));
    // compact: the BWT goes straight into the block builder and the table call makes C alone (d_o and d_ro are null)
    SX_TRY(sx_nomem_of(sx_bwt_tables_from_bwt_dev(ctx, d_bwt, N, sigma, R.d_c, R.d_o)));
    if (R.compact()) SX_TRY(sx_nomem_of(sx_occ_build_impl(ctx, d_bwt, N, sigma, R.d_occ, R.packed)));
    if (R.sampled()) {
        SX_TRY(sx_nomem_of(sx_sa_sample_dev_impl(ctx, d_sa, N, R.sa_log2, R.d_sa_marks, R.d_sa_values))); // (ends with a sync)
        T.drop(d_sa);
    }
    if (include_reverse) { // bwt.c:147-158: the reversed string's suffix array is temporary, its O table is RO
        uint8_t *d_rev;
        uint32_t *d_rsa, *d_rc;
        SX_TRY(T.take(ctx, &d_rev, (size_t)N));
        SX_TRY(T.take(ctx, &d_rsa, (size_t)N));
        SX_TRY(T.take(ctx, &d_rc, (size_t)sigma));
        SX_TRY(sx_reverse_dev(ctx, R.d_string, n, d_rev));
        SX_TRY(sx_nomem_of(sx_sa_bwt_build_dev(ctx, d_rev, n, sigma, d_rsa, d_bwt)));
        SX_TRY(sx_nomem_of(sx_bwt_tables_from_bwt_dev(ctx, d_bwt, N, sigma, d_rc, R.d_ro)));
        if (R.compact()) SX_TRY(sx_nomem_of(sx_occ_build_impl(ctx, d_bwt, N, sigma, R.d_rocc, R.packed)));
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

// A record's suffix array rows [lo, hi), and its O (or RO) rows [lo, hi), to a sink as the index file has them, whichever
// form the record keeps them in: a sampled suffix array is located and compact blocks are expanded into a device window,
// a staging buffer's worth at a time (the same bytes)
static int send_sa_rows(sx_ctx *ctx, const sx_index_rec &R, uint64_t lo, uint64_t hi, sx_sink_fn sink, void *user)
{
    if (!R.sampled()) return sx_stream_to_sink(ctx, SX_SECTION_INDEX, R.d_sa + lo, (size_t)(hi - lo) * 4, sink, user);
    const auto fill = [&](uint64_t a, uint64_t b, uint32_t *d_win) { return sx_sa_locate_rows_impl(ctx, R.loc(), a, b, d_win); };
    return sx_nomem_of(sx_stream_windows(ctx, SX_SECTION_INDEX, lo, hi, 4, sink, user, fill));
}
static int send_o_rows(sx_ctx *ctx, const sx_index_rec &R, bool reverse, uint64_t lo, uint64_t hi, sx_sink_fn sink, void *user)
{
    const size_t row_bytes = (size_t)R.sigma * 4;
    if (!R.compact()) return sx_stream_to_sink(ctx, SX_SECTION_INDEX, (reverse ? R.d_ro : R.d_o) + lo * R.sigma, (hi - lo) * row_bytes, sink, user);
    const auto fill = [&](uint64_t a, uint64_t b, uint32_t *d_win) { return sx_occ_expand_impl(ctx, reverse ? R.d_rocc : R.d_occ, R.N, R.sigma, a, b, d_win, R.packed); };
    return sx_nomem_of(sx_stream_windows(ctx, SX_SECTION_INDEX, lo, hi, row_bytes, sink, user, fill));
}

} // namespace sx

using namespace sx;

extern "C" {

int sx_index_live_count(void) { return g_live_indexes.load(); }

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
    SX_TRY(flags_check(ctx, flags));
    if (len >= 0x7FFFFFFFull) return sx_fail_msg(ctx, SX_E_ARG, "FASTA image must be shorter than 2^31 - 1 bytes");
    SX_CHECK(hipSetDevice(ctx->device));
    sx_index *idx = new_index(ctx, flags);
    if (!idx) return sx_fail_msg(ctx, SX_E_NOMEM, "index");
    return finish_index(ctx, idx, sx_nomem_of(build_fasta(ctx, idx, fasta, len, include_reverse != 0)), out);
}

int sx_index_from_tables(sx_ctx *ctx, const sx_map_record *records, uint32_t n_records, sx_index **out)
{
    return from_tables(ctx, records, nullptr, n_records, 0, out);
}

int sx_index_from_sources(sx_ctx *ctx, const sx_index_source *sources, uint32_t n_records, sx_index **out)
{
    return from_tables(ctx, nullptr, sources, n_records, 0, out);
}

int sx_index_from_sources_ex(sx_ctx *ctx, const sx_index_source *sources, uint32_t n_records, uint32_t flags, sx_index **out)
{
    return sx_nomem_of(from_tables(ctx, nullptr, sources, n_records, flags, out));
}

int sx_index_add_record(sx_ctx *ctx, sx_index *idx, const sx_index_source *source, int at_front)
{
    if (!ctx || !idx || !source) return SX_E_ARG;
    SX_TRY(device_check(ctx, idx));
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
    out->compact = R.compact() ? (R.packed ? 2 : 1) : 0;
    if (R.compact()) {
        out->d_occ = R.d_occ, out->d_rocc = R.d_rocc;
        out->stride = occ_form_stride(R.sigma, R.packed), out->sigma_pad = R.packed ? kOccPackedMaxSigma : occ_sigma_pad(R.sigma);
        out->n_blocks = occ_blocks(R.N);
    }
    return 0;
}

int sx_index_is_compact(const sx_index *idx) { return idx && idx->compact ? 1 : 0; }
int sx_index_is_packed(const sx_index *idx) { return idx && idx->packed ? 1 : 0; }

int sx_index_record_samples(const sx_index *idx, uint32_t record, sx_index_samples *out)
{
    if (!idx || !out || record >= idx->recs.size()) return SX_E_ARG;
    const sx_index_rec &R = idx->recs[record];
    memset(out, 0, sizeof *out);
    if (R.sampled()) {
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
    SX_TRY(device_check(ctx, idx));
    const sx_index_rec &R = idx->recs[record];
    if (!(reverse ? R.d_rocc : R.d_occ)) return sx_fail_msg(ctx, SX_E_ARG, "index: the record has no blocks of this table");
    if (row_lo > row_hi || row_hi > R.N + 1 || (row_hi > row_lo && !rows_out)) return sx_fail_msg(ctx, SX_E_ARG, "index: the rows to expand lie in [0, N]");
    SX_CHECK(hipSetDevice(ctx->device));
    char *at = (char *)rows_out;
    return send_o_rows(ctx, R, reverse != 0, row_lo, row_hi, expand_sink, &at);
}

int sx_index_expand_sa(sx_ctx *ctx, const sx_index *idx, uint32_t record, uint64_t row_lo, uint64_t row_hi, uint32_t *rows_out)
{
    if (!ctx || !idx || record >= idx->recs.size()) return SX_E_ARG;
    SX_TRY(device_check(ctx, idx));
    const sx_index_rec &R = idx->recs[record];
    if (!R.sampled()) return sx_fail_msg(ctx, SX_E_ARG, "index: the record keeps its whole suffix array");
    if (row_lo > row_hi || row_hi > R.N || (row_hi > row_lo && !rows_out)) return sx_fail_msg(ctx, SX_E_ARG, "index: the rows to expand lie in [0, N)");
    SX_CHECK(hipSetDevice(ctx->device));
    char *at = (char *)rows_out;
    return send_sa_rows(ctx, R, row_lo, row_hi, expand_sink, &at);
}

int sx_index_map_reads(sx_ctx *ctx, const sx_index *idx, const uint8_t *fastq, size_t fastq_len, int edits, sx_sink_fn sink, void *user)
{
    return sx_index_map_reads_ex(ctx, idx, fastq, fastq_len, edits, 0, sink, user);
}

int sx_index_map_reads_ex(sx_ctx *ctx, const sx_index *idx, const uint8_t *fastq, size_t fastq_len, int edits, uint32_t flags, sx_sink_fn sink,
                          void *user)
{
    if (!ctx || !idx || !sink || (fastq_len && !fastq)) return SX_E_ARG;
    SX_TRY(device_check(ctx, idx));
    if (edits < 0 || edits > SX_APPROX_MAX_EDITS) return sx_fail_msg(ctx, SX_E_ARG, "read mapping: edits must be in [0, 8]");
    if (flags & ~sx_map_known_flags) return sx_fail_msg(ctx, SX_E_ARG, "read mapping: unknown flags");
    SX_TRY(sx_map_mapq_check(ctx, flags));
    if (fastq_len > 0xFFFFFFFEull) return sx_fail_msg(ctx, SX_E_ARG, "read mapping: malformed FASTQ image (see sx_fastq_index)");
    SX_TRY(sx_map_tags_check(ctx, idx, flags)); // (before the reads go up)
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
    const int rc = sx_map_reads_core(ctx, idx, fq, nullptr, edits, flags, sink, user);
    sx_fastq_dev_free(&fq);
    return rc;
}

// a FASTQ image through the staging buffers to the device, indexed there (the image is released again)
static int fastq_up(sx_ctx *ctx, const uint8_t *fastq, size_t fastq_len, sx_fastq_dev *fq)
{
    sx_dev_scope T;
    uint8_t *d_image;
    SX_TRY(T.take(ctx, &d_image, fastq_len + 16));
    SX_TRY(sx_upload_staged(ctx, d_image, fastq, fastq_len));
    const int frc = sx_fastq_index_dev(ctx, d_image, fastq_len, fq);
    if (frc == SX_E_MALFORMED || frc == SX_E_ARG) return sx_fail_msg(ctx, frc, "read mapping: malformed FASTQ image (see sx_fastq_index)");
    return frc;
}

int sx_index_map_pairs(sx_ctx *ctx, const sx_index *idx, const uint8_t *fastq1, size_t len1, const uint8_t *fastq2, size_t len2, int edits,
                       const sx_pair_opts *opts, uint32_t flags, sx_sink_fn sink, void *user)
{
    if (!ctx || !idx || !sink || !opts || (len1 && !fastq1) || (len2 && !fastq2)) return SX_E_ARG;
    SX_TRY(device_check(ctx, idx));
    if (edits < 0 || edits > SX_APPROX_MAX_EDITS) return sx_fail_msg(ctx, SX_E_ARG, "read mapping: edits must be in [0, 8]");
    if (flags & ~(uint32_t)(SX_MAP_BOTH_STRANDS | SX_MAP_BEST_STRATUM | SX_MAP_NO_INDELS | SX_MAP_HEADER))
        return sx_fail_msg(ctx, SX_E_ARG, "paired reads: the flags are SX_MAP_BOTH_STRANDS (implied), SX_MAP_BEST_STRATUM, SX_MAP_NO_INDELS and SX_MAP_HEADER");
    if (opts->min_insert > opts->max_insert) return sx_fail_msg(ctx, SX_E_ARG, "paired reads: min_insert must not exceed max_insert");
    if (len1 > 0xFFFFFFFEull || len2 > 0xFFFFFFFEull) return sx_fail_msg(ctx, SX_E_ARG, "read mapping: malformed FASTQ image (see sx_fastq_index)");
    SX_CHECK(hipSetDevice(ctx->device));
    sx_fastq_dev fq1, fq2;
    memset(&fq1, 0, sizeof fq1);
    memset(&fq2, 0, sizeof fq2);
    int rc = fastq_up(ctx, fastq1, len1, &fq1);
    if (rc == 0) rc = fastq_up(ctx, fastq2, len2, &fq2);
    if (rc == 0) rc = sx_map_pairs_core(ctx, idx, fq1, fq2, edits, *opts, flags, sink, user);
    sx_fastq_dev_free(&fq1);
    sx_fastq_dev_free(&fq2);
    return rc;
}

int sx_index_write(sx_ctx *ctx, const sx_index *idx, sx_sink_fn sink, void *user)
{
    if (!ctx || !idx || !sink) return SX_E_ARG;
    SX_TRY(device_check(ctx, idx));
    for (const sx_index_rec &R : idx->recs)
        if (!R.d_string) return sx_fail_msg(ctx, SX_E_ARG, "index: a record was given without its string and cannot be written");
    SX_CHECK(hipSetDevice(ctx->device));
    auto put = [&](const void *p, size_t n) { return sink(user, SX_SECTION_INDEX, p, n) != 0 ? sx_fail_msg(ctx, SX_E_ARG, "the sink refused a chunk") : 0; };
    const uint32_t n_rec = (uint32_t)idx->recs.size();
    SX_TRY(put(&n_rec, 4));
    for (uint32_t r = n_rec; r-- > 0;) { // last record first, as the mapper's -p writes them
        const sx_index_rec &R = idx->recs[r];
        const uint32_t name_bytes = (uint32_t)R.name.size() + 1, n = (uint32_t)(R.N - 1);
        SX_TRY(put(&name_bytes, 4));
        SX_TRY(put(R.name.c_str(), name_bytes));
        // stralg/serialise.c:7-18: string (u32 length, bytes), suffix array, remap table, C, O, flag, RO
        SX_TRY(put(&n, 4));
        SX_TRY(sx_stream_to_sink(ctx, SX_SECTION_INDEX, R.d_string, n, sink, user));
        SX_TRY(send_sa_rows(ctx, R, 0, R.N, sink, user));
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
        SX_TRY(send_o_rows(ctx, R, false, 0, R.N + 1, sink, user));
        const uint8_t has_ro = R.has_ro() ? 1 : 0; // (a bool in the reference: one byte)
        SX_TRY(put(&has_ro, 1));
        if (has_ro) SX_TRY(send_o_rows(ctx, R, true, 0, R.N + 1, sink, user));
    }
    return sx_sync(ctx);
}

} // extern "C"
