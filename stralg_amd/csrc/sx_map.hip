// sx_map.hip -- the read mapper's loop (tools/readmappers/bwt_readmapper/bwt_readmapper.c map_read, :130-160, 257-266) over
// reads and an index that lie on the device: what sx_map_reads_stream and sx_index_map_reads share (DESIGN.md sections 11,
// 12, 16, 17).  The reads go through in batches.  A batch: its searches, record after record, and its hits put in (read,
// record, hit) order (on capacity: the hits' room grows or the batch is halved, and it runs again; sx_map_plan.hpp has
// the arithmetic), then its SAM text (sx_sam.hip), window after window, to the sink.  Paired reads (sx_map_pairs_core, DESIGN.md
// section 21) go through the same loop in batches of whole pairs; their text is that of the join's line descriptors (sx_pairs.hip).
// With SX_MAP_MAPQ a best-stratum batch's merged hits go through the quality pass before their text.
#include "sx_common.hpp"
#include "sx_device.hpp"
#include "sx_scan.hpp"
#include "sx_hostio.hpp"
#include "sx_index.hpp"
#include "sx_locate.hpp"
#include "sx_sam.hpp"
#include "sx_pairs.hpp"
#include "sx_map_plan.hpp"

#include <vector>

namespace sx {

// ---- remap per record, hits of all records in (read, record rank, hit) order -------------------------------------------
__global__ __launch_bounds__(kBlock) void sam_remap_kernel(const uint8_t *seqs, const uint8_t *table, uint8_t *out, uint64_t lo,
                                                           uint64_t hi)
{
    const uint64_t i = lo + (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < hi) out[i] = table[seqs[i]];
}

// cnt[q * n_rec + r] = hits of read q in record r (ho: n_rec arrays of stride entries, the searches' hit offsets)
__global__ __launch_bounds__(kBlock) void sam_vq_count_kernel(const uint64_t *ho, uint64_t stride, uint32_t batch, uint32_t n_rec,
                                                              uint64_t *cnt)
{
    const uint64_t idx = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= (uint64_t)batch * n_rec) return;
    const uint32_t q = (uint32_t)(idx / n_rec), r = (uint32_t)(idx - (uint64_t)q * n_rec);
    cnt[idx] = ho[r * stride + q + 1] - ho[r * stride + q];
}

// ---- unmapped read groups (SX_MAP_UNMAPPED) ------------------------------------------------------
// cnt as sam_vq_count_kernel leaves it (or best_vq_count_kernel): a group of gsize reads whose counts are all 0 gets one
// slot, the one of its first read and record 0, for its placeholder
__global__ __launch_bounds__(kBlock) void sam_unmapped_count_kernel(uint64_t *cnt, uint32_t groups, uint32_t gsize, uint32_t n_rec)
{
    const uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= groups) return;
    const uint64_t first = g * gsize * n_rec;
    uint64_t sum = 0;
    for (uint64_t k = 0; k < (uint64_t)gsize * n_rec; ++k) sum += cnt[first + k];
    if (sum == 0) cnt[first] = 1;
}

// vbase: those counts scanned.  A group with exactly one slot gets the placeholder there, an empty interval of its first
// read and record 0 -- before the merge, which overwrites it where that slot is a real hit's (the group's one hit lands on
// the group's first slot as well)
__global__ __launch_bounds__(kBlock) void sam_unmapped_place_kernel(const uint64_t *vbase, uint32_t groups, uint32_t gsize, uint32_t n_rec, uint4 *dst,
                                                                    uint64_t n_dst, uint32_t *err)
{
    const uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= groups) return;
    const uint64_t first = g * gsize * n_rec, at = vbase[first];
    if (vbase[first + (uint64_t)gsize * n_rec] - at != 1) return;
    if (at >= n_dst) {
        atomicOr(err, 2u);
        return;
    }
    const uint4 h0 = {(uint32_t)first, 0u, 0u, 0u}, h1 = {0u, 0u, 0u, 0u};
    dst[2 * at] = h0;
    dst[2 * at + 1] = h1;
}

// hit j of the searches' hit arrays (record r's at seg[r] .. seg[r + 1]) goes behind the hits of its read in the
// records before r: query <- read * n_rec + r (n_dst: the merged array's entries, the hits and the placeholders)
__global__ __launch_bounds__(kBlock) void sam_merge_kernel(const uint4 *src, uint64_t n_hits, const uint64_t *seg, uint32_t n_rec,
                                                           const uint64_t *ho, uint64_t stride, uint32_t batch, const uint64_t *vbase,
                                                           uint4 *dst, uint64_t n_dst, uint32_t *err)
{
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n_hits) return;
    uint32_t r = 0;
    {
        uint32_t b = n_rec; // seg[r] <= j < seg[b]
        while (b - r > 1) {
            const uint32_t mid = (r + b) / 2;
            if (seg[mid] <= j) r = mid;
            else b = mid;
        }
    }
    uint4 h0 = src[2 * j];
    const uint32_t q = h0.x;
    if (q >= batch) {
        atomicOr(err, 2u);
        return;
    }
    const uint64_t at = vbase[(uint64_t)q * n_rec + r] + (j - seg[r] - ho[r * stride + q]);
    if (at >= n_dst) {
        atomicOr(err, 2u);
        return;
    }
    h0.x = q * n_rec + r;
    dst[2 * at] = h0;
    dst[2 * at + 1] = src[2 * j + 1];
}

// ---- MAPQ and secondary lines (SX_MAP_MAPQ) -------------------------------------------------------
// The quality pass over a best-stratum batch's merged hits (its groups' hits are consecutive there: vbase).  No lane walks
// over a group and there are no atomics: a group's line count is a difference of the scanned row counts.
// rows[h] <- R - L of merged hit h (a placeholder: 0), to be scanned
__global__ __launch_bounds__(kBlock) void mapq_rows_kernel(const uint4 *hits, uint64_t n_hits, uint64_t *rows)
{
    const uint64_t h = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (h >= n_hits) return;
    const uint4 h0 = hits[2 * h];
    rows[h] = h0.z > h0.y ? h0.z - h0.y : 0u;
}

// ext[g] <- 1 where the first hit of group g (gslots consecutive entries of vbase) has more than one row: that hit is split
// into its first row, the group's primary line, and the rest; to be scanned
__global__ __launch_bounds__(kBlock) void mapq_split_count_kernel(const uint4 *hits, uint64_t n_hits, const uint64_t *vbase, uint32_t groups,
                                                                  uint32_t gslots, uint64_t *ext)
{
    const uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= groups) return;
    const uint64_t first = vbase[g * gslots], end = vbase[(g + 1) * gslots];
    uint64_t e = 0;
    if (first < end && first < n_hits) {
        const uint4 h0 = hits[2 * first];
        e = h0.z > h0.y && h0.z - h0.y > 1u ? 1u : 0u;
    }
    ext[g] = e;
}

// the MAPQ of a group of n lines: -10 log10(1 - 1/n) as TopHat and STAR round it
__device__ __forceinline__ uint32_t mapq_of_lines(uint64_t n) { return n <= 1 ? 50u : n == 2 ? 3u : n <= 4 ? 1u : 0u; }

// One lane a merged hit h: its group from its query, the group's lines n from the scanned rows at the group's slot range, and
// the hit goes to dst behind the split entries of the groups in front (ext, scanned) -- a group's first hit as its first
// row (primary) and, where it has more, the rest; every other entry is secondary (bit 8 of its quality word)
__global__ __launch_bounds__(kBlock) void mapq_split_kernel(const uint4 *hits, uint64_t n_hits, const uint64_t *rows, const uint64_t *vbase,
                                                            const uint64_t *ext, uint32_t groups, uint32_t gslots, uint4 *dst, uint16_t *quality,
                                                            uint64_t n_dst, uint32_t *err)
{
    const uint64_t h = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (h >= n_hits) return;
    uint4 h0 = hits[2 * h];
    const uint4 h1 = hits[2 * h + 1];
    const uint32_t g = h0.x / gslots;
    if (g >= groups) {
        atomicOr(err, 2u);
        return;
    }
    const uint64_t first = vbase[(uint64_t)g * gslots], end = vbase[((uint64_t)g + 1) * gslots];
    const uint64_t x = ext[g], split = ext[g + 1] - x;
    if (h < first || h >= end || end > n_hits || split > 1) {
        atomicOr(err, 2u);
        return;
    }
    const uint32_t q = mapq_of_lines(rows[end] - rows[first]);
    uint64_t at = h + x + (h > first ? split : 0u);
    if (at + (h == first ? split : 0u) >= n_dst) {
        atomicOr(err, 2u);
        return;
    }
    if (h == first && split) {
        uint4 p = h0;
        p.z = h0.y + 1u;
        dst[2 * at] = p;
        dst[2 * at + 1] = h1;
        quality[at] = (uint16_t)q;
        h0.y += 1u;
        ++at;
        dst[2 * at] = h0;
        dst[2 * at + 1] = h1;
        quality[at] = (uint16_t)(q | 0x100u);
        return;
    }
    dst[2 * at] = h0;
    dst[2 * at + 1] = h1;
    quality[at] = (uint16_t)(h == first ? q : q | 0x100u);
}

// ---- the pieces of the loop ---------------------------------------------------------------------------------------------
template <class T> static int upload(sx_ctx *ctx, sx_dev_scope &B, T **d, const T *h, size_t count)
{
    SX_TRY(B.take(ctx, d, count));
    if (count) SX_CHECK(hipMemcpyAsync(*d, h, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return 0;
}

// what a mapping call asks of its reads and records; records_ok: sx_map_dims_ok / sx_map_record_check with sigma >= 2
static int map_check(sx_ctx *ctx, uint64_t n_reads, uint64_t n_records, uint32_t flags, bool records_ok)
{
    if (flags & ~sx_map_known_flags) return sx_fail_msg(ctx, SX_E_ARG, "read mapping: unknown flags");
    SX_TRY(sx_map_mapq_check(ctx, flags));
    if (sx_map_reads_limit(n_reads, n_records, flags) != 0)
        return sx_fail_msg(ctx, SX_E_ARG, "read mapping: reads x records (twice that for both strands) must stay below 2^32");
    if (!records_ok) return sx_fail_msg(ctx, SX_E_ARG, "read mapping: a record lacks its name, suffix array, tables or remap table");
    return 0;
}

// Room for the hits of a batch's searches: a guess to start with; a batch that needs more makes it
// grow, up to what map_room_largest allows, before the batch is halved
struct HitRoom {
    uint64_t cap = 0, cap_max = 0;
    sx_approx_hit *d_raw = nullptr;
    sx_dev_scope own;
    int init(sx_ctx *ctx, uint32_t batch_max, uint32_t n_records)
    {
        size_t free_b = 0, total_b = 0;
        const bool known = hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b;
        if (!known) (void)hipGetLastError();
        cap_max = map_room_largest(known, free_b, ctx->sam_room_hits);
        cap = map_room_first(batch_max, n_records, cap_max, ctx->sam_room_hits);
        return own.take(ctx, &d_raw, (size_t)cap);
    }
    // the searches of `groups` groups of reads need room for `need` hits: it grows, or *halve, and the caller goes on with
    // half the groups
    int grow_or_halve(sx_ctx *ctx, uint64_t need, uint32_t groups, bool *halve)
    {
        const map_room_step s = map_room_next(cap, cap_max, need, groups);
        *halve = s.halve;
        if (s.halve) return 0;
        cap = s.cap;
        own.drop(d_raw);
        return own.take(ctx, &d_raw, (size_t)cap);
    }
};

// the reads of a mapping call as the loop sees them
struct MapReads {
    const sx_fastq_dev *fq;
    const uint32_t *h_seq_off; // the host's copy of fq->d_seq_off, or null (the two entries a batch needs are read back)
    const uint16_t *d_flags;   // a FLAG per read, or null
    uint32_t group; // 0, or (SX_MAP_BEST_STRATUM) the reads that share a stratum: 1, or 2 for the strands of a read
    uint32_t search_flags; // SX_SEARCH_* of every search of the call (SX_MAP_NO_INDELS)
    bool tags;             // NM and MD behind QUAL (SX_MAP_TAGS)
    // paired reads, or null: the reads are 4 x pairs, read 4p + 2m + s, a batch holds whole pairs and its
    // text is that of the join's line descriptors
    const sx_pair_opts *pairs = nullptr;
    // 0, or (SX_MAP_UNMAPPED) the reads of a group that gets a FLAG 4 line where it has none: 1, or 2
    // for the strands of a read
    uint32_t unmapped = 0;
    bool mapq = false; // MAPQ and secondary lines from the best stratum (SX_MAP_MAPQ; group != 0)
};

struct MapBufs { // what a mapping call holds on the device beside the hits' room
    uint8_t *d_pat, *d_win[2];
    uint64_t *d_ho, *d_vbase, *d_seg, *d_byte_off = nullptr;
    uint32_t *d_err;
    sx_approx_hit *d_merged = nullptr;
    // an index with a sampled suffix array: the lines in front of every hit of the batch, the positions of a run of hits
    uint64_t *d_pos_off = nullptr;
    uint32_t *d_positions = nullptr;
    uint64_t pos_cap = 0;
    uint64_t merged_cap = 0, stride = 0; // stride: entries of a record's hit offsets in d_ho
    size_t window = 0;
    std::vector<uint64_t> seg; // (the plain batch) where record r's hits start in the room; last, how many there are
    // SX_MAP_MAPQ: the merged hits with every group's first hit split, a quality word each; a split count a group
    bool mapq = false;
    sx_approx_hit *d_split = nullptr;
    uint16_t *d_quality = nullptr;
    uint64_t *d_ext = nullptr;
    sx_dev_scope own;
};

// [*p_lo, *p_hi): the sequence bytes of reads q0 .. q0 + batch
static int batch_bytes(sx_ctx *ctx, const MapReads &R, uint32_t q0, uint32_t batch, uint64_t *p_lo, uint64_t *p_hi)
{
    if (R.h_seq_off) {
        *p_lo = R.h_seq_off[q0], *p_hi = R.h_seq_off[q0 + batch];
    } else { // (the offsets were made on the device: the two this batch needs come back)
        const uint32_t *src[2] = {R.fq->d_seq_off + q0, R.fq->d_seq_off + q0 + batch};
        const uint32_t one[2] = {1, 1};
        uint32_t got[2];
        SX_TRY(sx_readback_ranges(ctx, src, one, 2, got));
        *p_lo = got[0], *p_hi = got[1];
    }
    return 0;
}

// The searches of reads q0 .. q0 + batch, record after record, into the room: M.seg[r] <- where record r's hits start,
// M.seg[records] and *hits_out <- how many there are.  SX_E_CAPACITY: the room is too small for the *hits_out hits known of
// so far
static int search_batch(sx_ctx *ctx, const sx_index *idx, const MapReads &R, MapBufs &M, const HitRoom &room, uint32_t q0, uint32_t batch,
                        int edits, uint32_t search_flags, uint64_t *hits_out)
{
    uint64_t p_lo, p_hi;
    SX_TRY(batch_bytes(ctx, R, q0, batch, &p_lo, &p_hi));
    const uint32_t n_records = (uint32_t)idx->recs.size();
    uint64_t used = 0;
    for (uint32_t r = 0; r < n_records; ++r) {
        if (p_hi > p_lo)
            sx_launch(ctx, SX_KC_REMAP, 2 * (p_hi - p_lo), sam_remap_kernel, dim3(sx_div_up(p_hi - p_lo, kBlock)), dim3(kBlock),
                      (const uint8_t *)R.fq->d_seqs, (const uint8_t *)(idx->d_tabs + (size_t)r * 256), M.d_pat, p_lo, p_hi);
        uint64_t tot = 0;
        // (whichever form the record has: the hits and their order are the same)
        const int rc = sx_approx_search_record(ctx, idx->recs[r], M.d_pat, R.fq->d_seq_off + q0, batch, edits, M.d_ho + r * M.stride,
                                               room.d_raw + used, room.cap - used, &tot, search_flags);
        if (rc == SX_E_CAPACITY) *hits_out = used + tot;
        if (rc != 0) return rc;
        M.seg[r] = used;
        used += tot;
    }
    M.seg[n_records] = *hits_out = used;
    return 0;
}

// room for `used` hits in (read, record, hit) order and for their byte offsets
static int merged_room(sx_ctx *ctx, MapBufs &M, const HitRoom &room, uint64_t used)
{
    if (used > M.merged_cap) {
        if (M.d_merged) M.own.drop(M.d_merged), M.own.drop(M.d_byte_off), M.own.drop(M.d_pos_off);
        if (M.d_split) M.own.drop(M.d_split), M.own.drop(M.d_quality);
        M.d_pos_off = nullptr, M.d_split = nullptr, M.d_quality = nullptr;
        M.merged_cap = used > room.cap ? used : room.cap;
        SX_TRY(M.own.take(ctx, &M.d_merged, (size_t)M.merged_cap));
        SX_TRY(M.own.take(ctx, &M.d_byte_off, (size_t)M.merged_cap + 1));
        if (M.mapq) {
            SX_TRY(M.own.take(ctx, &M.d_split, (size_t)M.merged_cap));
            SX_TRY(M.own.take(ctx, &M.d_quality, (size_t)M.merged_cap));
        }
    }
    return 0;
}

// The hits of the batch's searches in (read, record rank, hit) order: M.d_merged, query <- read x records + rank.
// ugroup (SX_MAP_UNMAPPED): the reads of a group, and every group without a hit gets its placeholder in that order too;
// *merged_out <- the entries of M.d_merged
static int merge_batch(sx_ctx *ctx, MapBufs &M, const HitRoom &room, uint32_t batch, uint32_t ugroup, uint64_t *merged_out)
{
    const uint32_t n_records = (uint32_t)M.seg.size() - 1;
    const uint64_t used = M.seg[n_records], groups = ugroup ? batch / ugroup : 0;
    SX_TRY(merged_room(ctx, M, room, used + groups)); // (with placeholders: one a group at the most)
    SX_CHECK(hipMemcpyAsync(M.d_seg, M.seg.data(), M.seg.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    SX_CHECK(hipStreamSynchronize(ctx->stream)); // (seg is reused by the next batch)
    const uint64_t nvq = (uint64_t)batch * n_records;
    sx_launch(ctx, SX_KC_SAM, nvq * 24, sam_vq_count_kernel, dim3(sx_div_up(nvq, kBlock)), dim3(kBlock), (const uint64_t *)M.d_ho, M.stride,
              batch, n_records, M.d_vbase);
    if (ugroup) sx_map_unmapped_count(ctx, M.d_vbase, (uint32_t)groups, ugroup, n_records);
    SX_TRY(device_scan64_inplace(ctx, M.d_vbase, nvq, SX_KC_SAM));
    uint64_t merged = used;
    if (ugroup) {
        uint32_t w[2] = {0, 0};
        SX_TRY(sx_readback(ctx, (const uint32_t *)(M.d_vbase + nvq), 2, w));
        merged = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
        if (merged < used || merged > used + groups) return sx_fail_msg(ctx, SX_E_INTERNAL, "read mapping: the hits of a batch do not add up");
        sx_map_unmapped_place(ctx, M.d_vbase, (uint32_t)groups, ugroup, n_records, M.d_merged, merged, M.d_err);
    }
    if (used)
        sx_launch(ctx, SX_KC_SAM, used * 64, sam_merge_kernel, dim3(sx_div_up(used, kBlock)), dim3(kBlock), (const uint4 *)room.d_raw, used,
                  (const uint64_t *)M.d_seg, n_records, (const uint64_t *)M.d_ho, M.stride, batch, (const uint64_t *)M.d_vbase,
                  (uint4 *)M.d_merged, merged, M.d_err);
    uint32_t e = 0;
    SX_TRY(sx_readback(ctx, M.d_err, 1, &e));
    if (e) return sx_fail_msg(ctx, SX_E_INTERNAL, "read mapping: the hits of a batch do not add up");
    *merged_out = merged;
    return 0;
}

// A batch of either kind, reads q0 .. q0 + batch: on success its hits are in M.d_merged in (read, record, hit) order and
// *hits_out is their count (SX_MAP_UNMAPPED: with the placeholders); SX_E_CAPACITY: the room is too small for the
// *hits_out hits known of so far.
// The plain batch: every record's search, then the merge (with placeholders also where there is no hit)
static int plain_batch(sx_ctx *ctx, const sx_index *idx, const MapReads &R, MapBufs &M, const HitRoom &room, int edits, uint32_t q0,
                       uint32_t batch, uint64_t *hits_out)
{
    SX_TRY(search_batch(ctx, idx, R, M, room, q0, batch, edits, R.search_flags, hits_out));
    return *hits_out || R.unmapped ? merge_batch(ctx, M, room, batch, R.unmapped, hits_out) : 0;
}

// The best-stratum batch (whole groups): the rounds of sx_best.hip into the room, then its place step
static int best_batch(sx_ctx *ctx, const sx_index *idx, const MapReads &R, MapBufs &M, const HitRoom &room, sx_best_state &S, int edits,
                      uint32_t q0, uint32_t batch, uint64_t *hits_out)
{
    sx_best_batch B = {};
    B.recs = idx->recs.data(), B.n_rec = (uint32_t)idx->recs.size(), B.d_tabs = idx->d_tabs, B.d_pat = M.d_pat;
    B.d_bytes = R.fq->d_seqs, B.bytes_total = R.fq->seq_bytes, B.d_off = R.fq->d_seq_off + q0;
    SX_TRY(batch_bytes(ctx, R, q0, batch, &B.p_lo, &B.p_hi));
    B.count = batch, B.gsize = R.group, B.k = edits, B.search_flags = R.search_flags;
    B.d_ho = M.d_ho, B.ho_stride = M.stride, B.d_stratum = S.d_stratum;
    B.d_raw = room.d_raw, B.raw_cap = room.cap, B.go_on_counting = false;
    SX_TRY(sx_best_rounds(ctx, S, B, hits_out));
    if (*hits_out == 0 && !R.unmapped) return 0;
    const uint64_t split = R.mapq ? batch / R.group : 0; // (SX_MAP_MAPQ: a group's first hit may become two entries)
    if (!R.unmapped) {
        SX_TRY(merged_room(ctx, M, room, *hits_out + split));
        return sx_best_place(ctx, S, B, *hits_out, M.d_vbase, M.d_merged);
    }
    SX_TRY(merged_room(ctx, M, room, *hits_out + batch / R.group + split)); // (a placeholder a group at the most)
    return sx_best_place(ctx, S, B, *hits_out, M.d_vbase, M.d_merged, true, hits_out);
}

// The quality pass (SX_MAP_MAPQ) over the `hits` merged entries of a best-stratum batch of `batch` reads in
// groups of `gsize`: M.d_split <- the entries with every group's first hit split where it has more than one row, M.d_quality
// <- a quality word an entry, *split_out <- how many there are (at most one more a group; merged_room has seen to the room)
static int quality_pass(sx_ctx *ctx, MapBufs &M, uint64_t hits, uint32_t batch, uint32_t gsize, uint32_t n_records, uint64_t *split_out)
{
    const uint32_t groups = batch / gsize, gslots = gsize * n_records;
    const uint4 *src = (const uint4 *)M.d_merged;
    uint64_t *d_rows = M.d_byte_off; // (the layout's array, which the layout fills after this pass: hits + 1 entries here)
    sx_launch(ctx, SX_KC_MAPQ, hits * 24, mapq_rows_kernel, dim3(sx_div_up(hits, kBlock)), dim3(kBlock), src, hits, d_rows);
    SX_TRY(device_scan64_inplace(ctx, d_rows, hits, SX_KC_MAPQ));
    sx_launch(ctx, SX_KC_MAPQ, (uint64_t)groups * 40, mapq_split_count_kernel, dim3(sx_div_up(groups, kBlock)), dim3(kBlock), src, hits,
              (const uint64_t *)M.d_vbase, groups, gslots, M.d_ext);
    SX_TRY(device_scan64_inplace(ctx, M.d_ext, groups, SX_KC_MAPQ));
    uint32_t w[2] = {0, 0};
    SX_TRY(sx_readback(ctx, (const uint32_t *)(M.d_ext + groups), 2, w));
    const uint64_t n_split = hits + ((uint64_t)w[0] | ((uint64_t)w[1] << 32));
    if (n_split > hits + groups || n_split > M.merged_cap) return sx_fail_msg(ctx, SX_E_INTERNAL, "read mapping: the hits of a batch do not add up");
    sx_launch(ctx, SX_KC_MAPQ, hits * 106, mapq_split_kernel, dim3(sx_div_up(hits, kBlock)), dim3(kBlock), src, hits, (const uint64_t *)d_rows,
              (const uint64_t *)M.d_vbase, (const uint64_t *)M.d_ext, groups, gslots, (uint4 *)M.d_split, M.d_quality, n_split, M.d_err);
    uint32_t e = 0;
    SX_TRY(sx_readback(ctx, M.d_err, 1, &e));
    if (e) return sx_fail_msg(ctx, SX_E_INTERNAL, "read mapping: the hits of a batch do not add up");
    *split_out = n_split;
    return 0;
}

// The text of A's hits: its layout, then window after window through the two device windows and the context's staging
// buffers: emit and copy of window w are queued, then the sink works on window w - 1
// (emit(lo, hi, d_out): bytes [lo, hi) of a text of `total` bytes)
template <class Emit> static int emit_windows_of(sx_ctx *ctx, uint64_t total, const MapBufs &M, const sx_stage_events &E, sx_sink_fn sink, void *user, Emit emit)
{
    const uint64_t window = M.window, n_win = (total + window - 1) / window;
    for (uint64_t w = 0; w <= n_win; ++w) {
        if (w < n_win) {
            const uint64_t lo = w * window, hi = total - lo < window ? total : lo + window;
            SX_TRY(emit(lo, hi, M.d_win[w & 1]));
            SX_CHECK(hipMemcpyAsync(ctx->h_stage[w & 1], M.d_win[w & 1], (size_t)(hi - lo), hipMemcpyDeviceToHost, ctx->stream));
            SX_CHECK(hipEventRecord(E.ev[w & 1], ctx->stream));
        }
        if (w > 0) {
            const uint64_t lo = (w - 1) * window, hi = total - lo < window ? total : lo + window;
            SX_CHECK(hipEventSynchronize(E.ev[(w - 1) & 1]));
            if (sink(user, SX_SECTION_SAM, ctx->h_stage[(w - 1) & 1], (size_t)(hi - lo)) != 0) {
                (void)hipStreamSynchronize(ctx->stream);
                return sx_fail_msg(ctx, SX_E_ARG, "the sink refused a chunk");
            }
        }
    }
    return sx_sync(ctx);
}

// (unmapped: the hits have placeholders, SX_MAP_UNMAPPED; quality: a quality word a hit, SX_MAP_MAPQ, or null)
static int emit_windows(sx_ctx *ctx, const SamTagArgs &A, const MapBufs &M, const sx_stage_events &E, sx_sink_fn sink, void *user, bool unmapped,
                        const uint16_t *quality)
{
    uint64_t total = 0;
    SX_TRY(sam_layout(ctx, A, M.d_byte_off, &total, unmapped, quality));
    return emit_windows_of(ctx, total, M, E, sink, user,
                           [&](uint64_t lo, uint64_t hi, uint8_t *d_out) { return sam_emit(ctx, A, M.d_byte_off, lo, hi, d_out, unmapped, quality); });
}

// The text of a batch (`text`: its hits, reads and records) against an index with a sampled suffix array: its hits are taken
// in runs of consecutive hits whose lines fit the cap (SX_FLAG_LOCATE_CHUNK_ROWS; a hit is never split: one with more lines
// gets a buffer of its own length); a run is located, laid out and emitted through its windows before the next one starts
static int emit_located(sx_ctx *ctx, const sx_index *idx, const SamTagArgs &text, MapBufs &M, const sx_stage_events &E, sx_sink_fn sink, void *user,
                        bool unmapped, const uint16_t *quality)
{
    const LocRec *d_recs = (const LocRec *)idx->d_loc_list;
    const uint64_t n_hits = text.n_hits, cap = map_located_rows(ctx->locate_chunk_rows);
    if (!M.d_pos_off) SX_TRY(M.own.take(ctx, &M.d_pos_off, (size_t)M.merged_cap + 1));
    uint64_t total = 0;
    SX_TRY(sx_sa_hits_offsets(ctx, d_recs, text.n_records, (uint64_t)text.n_reads * text.n_records, text.hits, n_hits, M.d_pos_off, &total));
    uint32_t *d_loc_err = M.d_err + 4, *d_run = M.d_err + 8;
    for (uint64_t h_lo = 0, base = 0; h_lo < n_hits;) {
        uint64_t h_hi = n_hits, rows = total - base;
        if (rows > cap) SX_TRY(sx_sa_hits_run(ctx, M.d_pos_off, n_hits, h_lo, base, cap, d_run, &h_hi, &rows));
        if (rows > M.pos_cap) {
            if (M.d_positions) M.own.drop(M.d_positions);
            M.d_positions = nullptr, M.pos_cap = 0;
            SX_TRY(M.own.take(ctx, &M.d_positions, (size_t)rows));
            M.pos_cap = rows;
        }
        if (!M.d_positions) SX_TRY(M.own.take(ctx, &M.d_positions, 1)); // (hits without a line: the kernels still want an address)
        SX_TRY(sx_sa_locate_hits(ctx, d_recs, text.n_records, idx->packed, text.hits, M.d_pos_off, h_lo, h_hi, base, rows, M.d_positions, d_loc_err));
        uint32_t e = 0;
        SX_TRY(sx_readback(ctx, d_loc_err, 1, &e));
        if (e) return sx_fail_msg(ctx, SX_E_INTERNAL, "read mapping: a walk over a sampled suffix array met its bound");
        SamTagArgs A = text;
        A.hits = text.hits + 2 * h_lo, A.n_hits = h_hi - h_lo;
        A.positions = M.d_positions, A.pos_off = M.d_pos_off + h_lo, A.pos_base = base;
        SX_TRY(emit_windows(ctx, A, M, E, sink, user, unmapped, quality ? quality + h_lo : nullptr));
        base += rows;
        h_lo = h_hi;
    }
    return 0;
}

// ---- paired reads -----------------------------------------------------------------------------------
struct PairBufs { // what the join of a batch holds on the device; every array grows to what the largest batch so far needed
    uint64_t largest = 0; // lines of the batch, and line descriptors, that a batch of several pairs may have
    PairLines L = {nullptr, nullptr, nullptr, 0};
    uint64_t *d_cnt = nullptr, *d_byte_off = nullptr;
    sx_pair_line *d_desc = nullptr;
    uint64_t hits_cap = 0, lines_cap = 0, desc_cap = 0;
    sx_dev_scope own;
    template <class T> int grow(sx_ctx *ctx, T **d, size_t count)
    {
        if (*d) own.drop(*d);
        *d = nullptr;
        return own.take(ctx, d, count);
    }
};

// The text of a batch of whole pairs from its merged hits (A: the batch as the emitter sees it): the lines of the batch, their
// positions, count, scan, fill, then the descriptors' text through the windows.  SX_E_CAPACITY (a batch of several pairs
// only): its lines or its descriptors are more than P.largest; the caller halves the batch
static int pairs_text(sx_ctx *ctx, const sx_index *idx, const SamTagArgs &A, MapBufs &M, PairBufs &P, const sx_pair_opts &opts, bool lone,
                      const sx_stage_events &E, sx_sink_fn sink, void *user)
{
    PairJoin J = {A.hits, A.n_hits, M.d_vbase, A.n_reads, A.n_records, idx->d_sa_list, idx->d_sa_lens, nullptr, opts.min_insert,
                  opts.max_insert > 0x7FFFFFFFu ? 0x7FFFFFFFu : opts.max_insert}; // (TLEN is a signed 32-bit number)
    if (A.n_hits + 1 > P.hits_cap) {
        SX_TRY(P.grow(ctx, &P.L.line_off, (size_t)M.merged_cap + 1));
        P.hits_cap = M.merged_cap + 1;
    }
    SX_TRY(pair_lines_count(ctx, J, P.L));
    const uint64_t n_lines = P.L.n_lines;
    if (n_lines == 0) return 0;
    if (n_lines > P.largest && !lone) return SX_E_CAPACITY;
    if (n_lines + 1 > P.lines_cap) {
        SX_TRY(P.grow(ctx, &P.L.ps, (size_t)n_lines));
        SX_TRY(P.grow(ctx, &P.L.hit, (size_t)n_lines));
        SX_TRY(P.grow(ctx, &P.d_cnt, (size_t)n_lines + 1));
        P.lines_cap = n_lines + 1;
    }
    if (idx->sa_log2) { // the positions of every line of the batch, located in runs of hits whose lines fit the cap
        const LocRec *d_recs = (const LocRec *)idx->d_loc_list;
        const uint64_t cap = map_located_rows(ctx->locate_chunk_rows);
        if (n_lines > M.pos_cap) {
            if (M.d_positions) M.own.drop(M.d_positions);
            M.d_positions = nullptr, M.pos_cap = 0;
            SX_TRY(M.own.take(ctx, &M.d_positions, (size_t)n_lines));
            M.pos_cap = n_lines;
        }
        uint32_t *d_loc_err = M.d_err + 4, *d_run = M.d_err + 8;
        for (uint64_t h_lo = 0, base = 0; h_lo < A.n_hits;) {
            uint64_t h_hi = A.n_hits, rows = n_lines - base;
            if (rows > cap) SX_TRY(sx_sa_hits_run(ctx, P.L.line_off, A.n_hits, h_lo, base, cap, d_run, &h_hi, &rows));
            SX_TRY(sx_sa_locate_hits(ctx, d_recs, A.n_records, idx->packed, A.hits, P.L.line_off, h_lo, h_hi, base, rows, M.d_positions + base, d_loc_err));
            base += rows;
            h_lo = h_hi;
        }
        uint32_t e = 0;
        SX_TRY(sx_readback(ctx, d_loc_err, 1, &e));
        if (e) return sx_fail_msg(ctx, SX_E_INTERNAL, "read mapping: a walk over a sampled suffix array met its bound");
        J.positions = M.d_positions;
    }
    SX_TRY(pair_lines_expand(ctx, J, P.L));
    uint64_t combos = 0;
    SX_TRY(pair_count(ctx, J, P.L, P.d_cnt, &combos));
    if (combos == 0) return 0;
    const uint64_t n_desc = 2 * combos;
    if (n_desc > P.largest && !lone) return SX_E_CAPACITY;
    if (n_desc + 1 > P.desc_cap) {
        SX_TRY(P.grow(ctx, &P.d_desc, (size_t)n_desc));
        SX_TRY(P.grow(ctx, &P.d_byte_off, (size_t)n_desc + 1));
        P.desc_cap = n_desc + 1;
    }
    SX_TRY(pair_fill(ctx, J, P.L, P.d_cnt, P.d_desc));
    uint64_t total = 0;
    const SamArgs &S = A;
    SX_TRY(sam_layout_pairs(ctx, S, P.d_desc, n_desc, P.d_byte_off, &total));
    return emit_windows_of(ctx, total, M, E, sink, user,
                           [&](uint64_t lo, uint64_t hi, uint8_t *d_out) { return sam_emit_pairs(ctx, S, P.d_desc, n_desc, P.d_byte_off, lo, hi, d_out); });
}

// The loop.  A batch: its hits (on capacity: grow_or_halve, again), their text, on to the next reads
static int map_reads_loop(sx_ctx *ctx, const sx_index *idx, const MapReads &R, int edits, sx_sink_fn sink, void *user)
{
    const sx_fastq_dev &fq = *R.fq;
    const uint32_t n_reads = fq.count, n_records = (uint32_t)idx->recs.size();
    // the reads that a batch keeps together: a pair's four, a best group, or (SX_MAP_UNMAPPED) the strands of a read, whose
    // placeholder stands for both
    const uint32_t kept = R.group ? R.group : R.unmapped, g = R.pairs ? 4 : kept ? kept : 1;
    SX_CHECK(hipSetDevice(ctx->device));
    sx_map_stats &T = ctx->map_stats; // (host counts: sx_map_last_stats)
    T = {};
    MapBufs M;
    SX_TRY(M.own.take(ctx, &M.d_pat, (size_t)fq.seq_bytes));
    SX_TRY(sx_sync(ctx)); // (the callers' uploads from pageable memory are done)

    const uint32_t batch_max = R.pairs ? map_pairs_batch_max(ctx->sam_batch_reads, n_reads) : map_batch_max(ctx->sam_batch_reads, kept, n_reads);
    M.window = map_window_bytes(ctx->sam_window_bytes, sx_stage_bytes);
    SX_TRY(sx_stage_ensure(ctx));
    sx_stage_events E;
    for (uint8_t *&w : M.d_win) SX_TRY(M.own.take(ctx, &w, M.window));
    SX_TRY(E.create(ctx));
    M.stride = (uint64_t)batch_max + 1;
    SX_TRY(M.own.take(ctx, &M.d_ho, (size_t)M.stride * n_records));
    SX_TRY(M.own.take(ctx, &M.d_vbase, (size_t)batch_max * n_records + 1));
    SX_TRY(M.own.take(ctx, &M.d_seg, (size_t)n_records + 1));
    SX_TRY(M.own.take(ctx, &M.d_err, 64));
    SX_CHECK(hipMemsetAsync(M.d_err, 0, 256, ctx->stream));
    M.seg.resize(n_records + 1);
    HitRoom room;
    SX_TRY(room.init(ctx, batch_max, n_records));
    T.room_first = T.room_final = room.cap, T.batch_first = T.batch_final = batch_max;
    sx_best_state S;
    if (R.group) SX_TRY(S.init(ctx, batch_max, fq.seq_bytes, n_records, edits, true));
    M.mapq = R.mapq && R.group;
    if (M.mapq) SX_TRY(M.own.take(ctx, &M.d_ext, (size_t)batch_max / R.group + 1));
    SamTagArgs A = {}; // the batch whose text is emitted: what is the same for every batch here
    A.sa_list = idx->d_sa_list, A.sa_len_list = idx->d_sa_lens;
    A.names = fq.d_names, A.seqs = fq.d_seqs, A.quals = fq.d_quals;
    A.rnames = idx->d_rnames, A.rname_off = idx->d_rname_off, A.n_records = n_records;
    if (R.tags) A.text_list = idx->d_text_list, A.letters = idx->d_letters; // (emit_windows and emit_located carry them in A)

    PairBufs P;
    if (R.pairs) {
        size_t free_b = 0, total_b = 0;
        const bool known = hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b;
        if (!known) (void)hipGetLastError();
        P.largest = map_pairs_largest(known, free_b, ctx->pairs_room_lines > 0 ? ctx->pairs_room_lines : ctx->sam_room_hits);
    }

    uint32_t q0 = 0, batch = batch_max;
    while (q0 < n_reads) {
        if (batch > n_reads - q0) batch = n_reads - q0;
        uint64_t hits = 0;
        const int rc = R.group ? best_batch(ctx, idx, R, M, room, S, edits, q0, batch, &hits) : plain_batch(ctx, idx, R, M, room, edits, q0, batch, &hits);
        if (rc == SX_E_CAPACITY) { // (a group alone gets whatever it needs; a batch of groups is halved to whole groups)
            bool halve;
            SX_TRY(room.grow_or_halve(ctx, hits, batch / g, &halve));
            ++T.retries, ++(halve ? T.halved : batch / g == 1 ? T.lone_grown : T.room_grown);
            if (halve) batch = map_batch_halved(batch, g); // (it is not tried longer again)
            T.room_final = room.cap, T.batch_final = batch;
            continue;
        }
        if (rc != 0) return rc;
        if (hits) {
            A.hits = (const uint4 *)M.d_merged, A.n_hits = hits;
            A.name_off = fq.d_name_off + q0, A.seq_off = fq.d_seq_off + q0, A.qual_off = fq.d_qual_off + q0;
            A.n_reads = batch;
            A.flags = R.d_flags ? R.d_flags + q0 : nullptr; // (the offsets are this batch's: so are the flags)
            if (R.pairs) {
                const int prc = pairs_text(ctx, idx, A, M, P, *R.pairs, batch == g, E, sink, user);
                if (prc == SX_E_CAPACITY) { // (the lines or the descriptors of several pairs do not fit: half of them are tried)
                    ++T.retries, ++T.halved;
                    T.batch_final = batch = map_batch_halved(batch, g);
                    continue;
                }
                SX_TRY(prc);
            } else {
                const bool unm = R.unmapped != 0;
                const uint16_t *quality = nullptr;
                if (M.mapq) { // (the text is that of the split entries and their quality words)
                    uint64_t n_split = 0;
                    SX_TRY(quality_pass(ctx, M, hits, batch, R.group, n_records, &n_split));
                    A.hits = (const uint4 *)M.d_split, A.n_hits = n_split;
                    quality = M.d_quality;
                }
                SX_TRY(idx->sa_log2 ? emit_located(ctx, idx, A, M, E, sink, user, unm, quality) : emit_windows(ctx, A, M, E, sink, user, unm, quality));
            }
        }
        ++T.batches;
        q0 += batch;
    }
    return sx_sync(ctx);
}

} // namespace sx

using namespace sx;

// out[i] = table[seqs[i]] for i in [lo, hi) (sx_best.hip remaps its pattern sets with the loop's kernel)
void sx_sam_remap(sx_ctx *ctx, const uint8_t *d_seqs, const uint8_t *d_table, uint8_t *d_out, uint64_t lo, uint64_t hi)
{
    if (hi > lo) sx_launch(ctx, SX_KC_REMAP, 2 * (hi - lo), sam_remap_kernel, dim3(sx_div_up(hi - lo, kBlock)), dim3(kBlock), d_seqs, d_table, d_out, lo, hi);
}

void sx_map_unmapped_count(sx_ctx *ctx, uint64_t *d_cnt, uint32_t groups, uint32_t gsize, uint32_t n_rec)
{
    if (groups)
        sx_launch(ctx, SX_KC_SAM, (uint64_t)groups * gsize * n_rec * 8, sam_unmapped_count_kernel, dim3(sx_div_up(groups, kBlock)), dim3(kBlock), d_cnt,
                  groups, gsize, n_rec);
}

void sx_map_unmapped_place(sx_ctx *ctx, const uint64_t *d_vbase, uint32_t groups, uint32_t gsize, uint32_t n_rec, sx_approx_hit *d_dst, uint64_t n_dst,
                           uint32_t *d_err)
{
    if (groups)
        sx_launch(ctx, SX_KC_SAM, (uint64_t)groups * 16, sam_unmapped_place_kernel, dim3(sx_div_up(groups, kBlock)), dim3(kBlock), d_vbase, groups, gsize,
                  n_rec, (uint4 *)d_dst, n_dst, d_err);
}

// The SAM header of SX_MAP_HEADER in one sink call: @HD, then an @SQ line a record in the list's order,
// SN the record's name as the lines' RNAME has it, LN its symbols (N - 1)
template <class NameOf, class LenOf> static int map_header(sx_ctx *ctx, uint32_t n_records, NameOf name_of, LenOf len_of, sx_sink_fn sink, void *user)
{
    std::string h = "@HD\tVN:1.6\tSO:unsorted\n";
    for (uint32_t r = 0; r < n_records; ++r) {
        h += "@SQ\tSN:";
        h += name_of(r);
        h += "\tLN:";
        h += std::to_string(len_of(r));
        h += "\n";
    }
    if (sink(user, SX_SECTION_SAM, h.data(), h.size()) != 0) return sx_fail_msg(ctx, SX_E_ARG, "the sink refused a chunk");
    return 0;
}

static int index_header(sx_ctx *ctx, const sx_index *idx, sx_sink_fn sink, void *user)
{
    return map_header(
        ctx, (uint32_t)idx->recs.size(), [&](uint32_t r) -> const std::string & { return idx->recs[r].name; },
        [&](uint32_t r) { return (unsigned long long)(idx->recs[r].N - 1); }, sink, user);
}

int sx_map_mapq_check(sx_ctx *ctx, uint32_t flags)
{
    if ((flags & SX_MAP_MAPQ) && !(flags & SX_MAP_BEST_STRATUM))
        return sx_fail_msg(ctx, SX_E_ARG, "read mapping: SX_MAP_MAPQ needs SX_MAP_BEST_STRATUM (a read's first line must be one of its best)");
    return 0;
}

int sx_map_tags_check(sx_ctx *ctx, const sx_index *idx, uint32_t flags)
{
    if (!(flags & SX_MAP_TAGS)) return 0;
    for (const sx_index_rec &R : idx->recs)
        if (!R.d_string) return sx_fail_msg(ctx, SX_E_ARG, "read mapping: NM and MD need every record's string, and a record was given without it");
    return 0;
}

// A mapping call over reads and an index on ctx's device.  Both strands: the read set of 2 x count
// reads, read 2q + strand, is made once and searched like any read set, so its hits come in (read, strand, record, hit)
// order, which is the text's; the FLAGs go with the batches.
int sx_map_reads_core(sx_ctx *ctx, const sx_index *idx, const sx_fastq_dev &reads, const uint32_t *h_seq_off, int edits, uint32_t flags,
                      sx_sink_fn sink, void *user)
{
    const uint32_t n_records = (uint32_t)idx->recs.size();
    const bool header = (flags & SX_MAP_HEADER) != 0;
    if ((reads.count == 0 || n_records == 0) && !header) return 0;
    bool records_ok = true;
    for (const sx_index_rec &R : idx->recs) records_ok = records_ok && sx_map_dims_ok(R.N, R.sigma, 2);
    SX_TRY(map_check(ctx, reads.count, n_records, flags, records_ok)); // (SX_MAP_TAGS: the callers have seen to the strings)
    if (header) SX_TRY(index_header(ctx, idx, sink, user));
    if (reads.count == 0 || n_records == 0) return 0;
    const bool best = (flags & SX_MAP_BEST_STRATUM) != 0, tags = (flags & SX_MAP_TAGS) != 0, unmapped = (flags & SX_MAP_UNMAPPED) != 0;
    const uint32_t sflags = sx_map_search_flags(flags);
    if (!(flags & SX_MAP_BOTH_STRANDS)) {
        MapReads R = {&reads, h_seq_off, nullptr, best ? 1u : 0u, sflags, tags};
        R.unmapped = unmapped ? 1u : 0u;
        R.mapq = (flags & SX_MAP_MAPQ) != 0;
        return map_reads_loop(ctx, idx, R, edits, sink, user);
    }
    SX_CHECK(hipSetDevice(ctx->device));
    sx_fastq_dev both = {};
    sx_dev_scope F;
    uint16_t *d_flags;
    SX_TRY(F.take(ctx, &d_flags, 2 * (size_t)reads.count));
    SX_TRY(sx_fastq_strands_dev(ctx, &reads, &both, d_flags)); // (syncs: the callers' uploads from pageable memory are done)
    MapReads R = {&both, nullptr, d_flags, best ? 2u : 0u, sflags, tags};
    R.unmapped = unmapped ? 2u : 0u;
    R.mapq = (flags & SX_MAP_MAPQ) != 0;
    const int rc = map_reads_loop(ctx, idx, R, edits, sink, user);
    sx_fastq_dev_free(&both);
    return rc;
}

// A paired mapping call over the two mates' read sets and an index on ctx's device: the mates as one
// set, read 2p + m, then its strands, read 4p + 2m + s, searched like any read set in batches of whole pairs
int sx_map_pairs_core(sx_ctx *ctx, const sx_index *idx, const sx_fastq_dev &reads1, const sx_fastq_dev &reads2, int edits, const sx_pair_opts &opts,
                      uint32_t flags, sx_sink_fn sink, void *user)
{
    const uint32_t n_records = (uint32_t)idx->recs.size();
    if (reads1.count != reads2.count) return sx_fail_msg(ctx, SX_E_ARG, "paired reads: the two FASTQ images differ in their read counts");
    const bool header = (flags & SX_MAP_HEADER) != 0;
    if ((reads1.count == 0 || n_records == 0) && !header) return 0;
    if (sx_map_pairs_limit(reads1.count, n_records) != 0) return sx_fail_msg(ctx, SX_E_ARG, "paired reads: 4 x pairs x records must stay below 2^32");
    for (const sx_index_rec &R : idx->recs)
        if (!sx_map_dims_ok(R.N, R.sigma, 2)) return sx_fail_msg(ctx, SX_E_ARG, "read mapping: a record lacks its name, suffix array, tables or remap table");
    if (header) SX_TRY(index_header(ctx, idx, sink, user));
    if (reads1.count == 0 || n_records == 0) return 0;
    SX_CHECK(hipSetDevice(ctx->device));
    sx_fastq_dev mates = {}, both = {};
    int rc = sx_fastq_mates_dev(ctx, &reads1, &reads2, &mates);
    if (rc != 0) return sx_nomem_of(rc);
    sx_dev_scope F;
    uint16_t *d_flags = nullptr;
    rc = F.take(ctx, &d_flags, 2 * (size_t)mates.count);
    if (rc == 0) rc = sx_fastq_strands_dev(ctx, &mates, &both, d_flags);
    sx_fastq_dev_free(&mates);
    if (rc != 0) return rc;
    MapReads R = {&both, nullptr, nullptr, (flags & SX_MAP_BEST_STRATUM) ? 2u : 0u, sx_map_search_flags(flags), false};
    R.pairs = &opts;
    rc = map_reads_loop(ctx, idx, R, edits, sink, user);
    sx_fastq_dev_free(&both);
    return rc;
}

extern "C" {

int sx_map_pairs_limit(uint64_t n_pairs, uint64_t n_records)
{
    // (no product is formed before it is known to fit)
    if (n_pairs > 0xFFFFFFFFull / 4) return SX_E_ARG;
    if (n_records && n_pairs * 4 > 0xFFFFFFFFull / n_records) return SX_E_ARG;
    return 0;
}

int sx_map_reads_limit(uint64_t n_reads, uint64_t n_records, uint32_t flags)
{
    if (flags & ~sx_map_known_flags) return SX_E_ARG;
    const uint64_t strands = (flags & SX_MAP_BOTH_STRANDS) ? 2 : 1;
    // (no product is formed before it is known to fit)
    if (n_reads > 0xFFFFFFFFull / strands) return SX_E_ARG;
    if (n_records && n_reads * strands > 0xFFFFFFFFull / n_records) return SX_E_ARG;
    return 0;
}

int sx_map_reads_stream(sx_ctx *ctx, const sx_map_record *records, uint32_t n_records, const uint8_t *fastq, size_t fastq_len,
                        int edits, sx_sink_fn sink, void *user)
{
    return sx_map_reads_stream_ex(ctx, records, n_records, fastq, fastq_len, edits, 0, sink, user);
}

int sx_map_reads_stream_ex(sx_ctx *ctx, const sx_map_record *records, uint32_t n_records, const uint8_t *fastq, size_t fastq_len,
                           int edits, uint32_t flags, sx_sink_fn sink, void *user)
{
    if (!ctx || !sink || (n_records && !records) || (fastq_len && !fastq)) return SX_E_ARG;
    if (edits < 0 || edits > SX_APPROX_MAX_EDITS)
        return sx_fail_msg(ctx, SX_E_ARG, "read mapping: edits must be in [0, 8]");
    if (flags & ~sx_map_known_flags) return sx_fail_msg(ctx, SX_E_ARG, "read mapping: unknown flags");
    SX_TRY(sx_map_mapq_check(ctx, flags));
    if (flags & SX_MAP_TAGS) // (the rule of sx_index_write for a record without its string)
        return sx_fail_msg(ctx, SX_E_ARG, "read mapping: NM and MD need every record's string, and these records are tables alone (map through an index)");
    sx_fastq fq;
    const int frc = sx_fastq_index(fastq, fastq_len, &fq);
    if (frc != 0) return sx_fail_msg(ctx, frc, "read mapping: malformed FASTQ image (see sx_fastq_index)");
    struct FqFree {
        sx_fastq *f;
        ~FqFree() { sx_fastq_free(f); }
    } fq_free{&fq};
    const bool header = (flags & SX_MAP_HEADER) != 0;
    if ((fq.count == 0 || n_records == 0) && !header) return 0;
    bool records_ok = true;
    for (uint32_t r = 0; r < n_records; ++r) records_ok = records_ok && sx_map_record_check(records[r], 2);
    SX_TRY(map_check(ctx, fq.count, n_records, flags, records_ok));
    if (fq.count == 0 || n_records == 0) // (the header alone; otherwise the loop's call sinks it from the index)
        return map_header(
            ctx, n_records, [&](uint32_t r) { return records[r].name; }, [&](uint32_t r) { return (unsigned long long)(records[r].N - 1); }, sink, user);
    SX_CHECK(hipSetDevice(ctx->device));
    // the reads of this call, then a temporary index of the host tables (every record's suffix array and tables:
    // N x (4 + 8 sigma) bytes a record with its RO table), the loop, and the index goes again
    const uint32_t n_reads = fq.count;
    sx_dev_scope B; // (it owns the reads' arrays: they are not released with sx_fastq_dev_free)
    sx_fastq_dev reads = {};
    reads.count = n_reads;
    reads.name_bytes = fq.name_off[n_reads], reads.seq_bytes = fq.seq_off[n_reads], reads.qual_bytes = fq.qual_off[n_reads];
    SX_TRY(upload(ctx, B, &reads.d_names, fq.names, (size_t)reads.name_bytes));
    SX_TRY(upload(ctx, B, &reads.d_seqs, fq.seqs, (size_t)reads.seq_bytes));
    SX_TRY(upload(ctx, B, &reads.d_quals, fq.quals, (size_t)reads.qual_bytes));
    SX_TRY(upload(ctx, B, &reads.d_name_off, fq.name_off, (size_t)n_reads + 1));
    SX_TRY(upload(ctx, B, &reads.d_seq_off, fq.seq_off, (size_t)n_reads + 1));
    SX_TRY(upload(ctx, B, &reads.d_qual_off, fq.qual_off, (size_t)n_reads + 1));
    sx_index *idx = nullptr;
    SX_TRY(sx_index_from_tables(ctx, records, n_records, &idx));
    const int rc = sx_map_reads_core(ctx, idx, reads, fq.seq_off, edits, flags, sink, user);
    sx_index_destroy(idx);
    return rc;
}

} // extern "C"
