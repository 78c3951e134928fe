// sx_fastq.hip -- the FASTQ ingest on the device.
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
// sx_fastq_strands_dev makes the read set of both strands of these arrays (below).
// Where a byte goes is a function of the scans alone (no atomics place anything): the same image gives the same bytes.
#include "sx_common.hpp"
#include "sx_device.hpp"
#include "sx_bytes16.hpp"
#include "sx_hostio.hpp"
#include "sx_scan.hpp"

#include <algorithm>

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

// ---- the read set of both strands -------------------------------------------------------------
// Read 2q of the output is read q, read 2q + 1 its reverse complement, so pair q takes the bytes [2 off[q], 2 off[q + 1]) of
// an output array and nothing needs a scan.  The work is cut by output bytes, not by reads: a workgroup makes a tile of
// 4096 bytes of one of the three arrays (blockIdx.y: names, sequences, qualities), a lane 16 of them in one store, whatever
// the reads' lengths are (10 to 2046 bytes: a lane a read would leave a wave waiting for its longest read, a wave a read
// would leave five lanes in six idle on a short one).  The workgroup finds the pairs at its tile's ends by a search in the
// offsets, a lane the pair of its first byte by a search between them, and walks on from there.
constexpr uint32_t kStrandPer = 16, kStrandTile = kBlock * kStrandPer;

struct StrandArgs {
    const uint8_t *names, *seqs, *quals;
    const uint32_t *name_off, *seq_off, *qual_off;
    uint8_t *names_out, *seqs_out, *quals_out;
    uint32_t name_bytes, seq_bytes, qual_bytes; // of the input; the doubled ones fit 32 bits
    uint32_t count;
};

// the complement of a FASTQ byte: letters keep their case, every byte outside the table stays
__device__ __forceinline__ uint32_t strand_complement(uint32_t c)
{
    const uint32_t low = c | 0x20u;
    if (low < 'a' || low > 'z') return c;
    uint32_t v;
    switch (c & 0xDFu) {
    case 'A': v = 'T'; break;
    case 'C': v = 'G'; break;
    case 'G': v = 'C'; break;
    case 'T': v = 'A'; break;
    case 'U': v = 'A'; break;
    case 'R': v = 'Y'; break;
    case 'Y': v = 'R'; break;
    case 'K': v = 'M'; break;
    case 'M': v = 'K'; break;
    case 'B': v = 'V'; break;
    case 'V': v = 'B'; break;
    case 'D': v = 'H'; break;
    case 'H': v = 'D'; break;
    default: v = c & 0xDFu; break;
    }
    return v | (c & 0x20u);
}

// the last q in [lo, hi] with 2 off[q] <= j (2 off[lo] <= j)
__device__ __forceinline__ uint32_t strand_pair_of(const uint32_t *__restrict__ off, uint32_t lo, uint32_t hi, uint64_t j)
{
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1u) / 2u;
        if (2ull * off[mid] <= j) lo = mid;
        else hi = mid - 1u;
    }
    return lo;
}

__global__ __launch_bounds__(kBlock) void fq_strand_bytes_kernel(StrandArgs A)
{
    __shared__ uint8_t tab[kBlock]; // the second read's byte of a source byte (kBlock == 256)
    static_assert(kBlock == 256, "one lane a table entry");
    const uint32_t which = blockIdx.y, t = threadIdx.x;
    const uint8_t *__restrict__ in = which == 0 ? A.names : which == 1 ? A.seqs : A.quals;
    const uint32_t *__restrict__ off = which == 0 ? A.name_off : which == 1 ? A.seq_off : A.qual_off;
    uint8_t *__restrict__ out = which == 0 ? A.names_out : which == 1 ? A.seqs_out : A.quals_out;
    const uint32_t in_bytes = which == 0 ? A.name_bytes : which == 1 ? A.seq_bytes : A.qual_bytes;
    const bool reversed = which != 0; // (a name is repeated as it is)
    const uint64_t total = 2ull * in_bytes, tile0 = (uint64_t)blockIdx.x * kStrandTile;
    if (tile0 >= total) return; // (the whole workgroup: the grid is the longest array's)
    tab[t] = (uint8_t)(which == 1 ? strand_complement(t) : t);
    const uint64_t tile_last = total - tile0 < kStrandTile ? total - 1u : tile0 + kStrandTile - 1u;
    const uint32_t p0 = strand_pair_of(off, 0u, A.count - 1u, tile0), p1 = strand_pair_of(off, p0, A.count - 1u, tile_last);
    __syncthreads();
    const uint64_t j0 = tile0 + (uint64_t)t * kStrandPer;
    if (j0 >= total) return;
    uint32_t q = strand_pair_of(off, p0, p1, j0);
    uint32_t b = off[q], e = off[q + 1];
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t k = 0; k < kStrandPer; ++k) {
        const uint64_t j = j0 + k;
        if (j >= total) break; // (the bytes behind the array's end are zeros: they lie in its 16 spare bytes)
        while (j >= 2ull * e && q + 1u < A.count) { // (the next pair; more than one step only over reads without a byte)
            ++q;
            b = e;
            e = off[q + 1];
        }
        const uint32_t len = e >= b ? e - b : 0u, r = (uint32_t)(j - 2ull * b);
        uint32_t c = 0;
        if (r < len) { // the read itself
            if (b + r < in_bytes) c = in[b + r];
        } else if (r - len < len) { // its second strand
            const uint32_t at = reversed ? e - 1u - (r - len) : b + (r - len);
            if (at < in_bytes) c = tab[in[at]];
        }
        w[k >> 2] |= c << (8u * (k & 3u));
    }
    const uint4 v = {w[0], w[1], w[2], w[3]};
    *reinterpret_cast<uint4 *>(out + j0) = v;
}

// off_out[2q] = 2 off[q], off_out[2q + 1] = 2 off[q] + the read's length, off_out[2 count] = 2 off[count]; the flags
__global__ __launch_bounds__(kBlock) void fq_strand_offsets_kernel(StrandArgs A, uint32_t *__restrict__ name_off_out,
                                                                   uint32_t *__restrict__ seq_off_out, uint32_t *__restrict__ qual_off_out,
                                                                   uint16_t *__restrict__ flags_out)
{
    const uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q > A.count) return;
    const uint32_t nb = A.name_off[q], sb = A.seq_off[q], qb = A.qual_off[q];
    name_off_out[2 * q] = 2u * nb;
    seq_off_out[2 * q] = 2u * sb;
    qual_off_out[2 * q] = 2u * qb;
    if (q == A.count) return;
    name_off_out[2 * q + 1] = nb + A.name_off[q + 1];
    seq_off_out[2 * q + 1] = sb + A.seq_off[q + 1];
    qual_off_out[2 * q + 1] = qb + A.qual_off[q + 1];
    flags_out[2 * q] = 0;
    flags_out[2 * q + 1] = 16;
}

// ---- the read set of the mates of two images ------------------------------------------------------
// Read 2p of the output is read p of image 1, read 2p + 1 read p of image 2: pair p takes the bytes [off1[p] + off2[p],
// off1[p + 1] + off2[p + 1]) of an output array, so the offsets need no scan here either.  The bytes are cut like those of the
// strands: a lane makes 16 output bytes in one store; it finds the read of its first byte by a search in the new offsets and
// walks on from there.  sx_fastq_strands_dev of this set is the set of 4 x pairs reads, read 4p + 2m + s, that the mapper searches.
struct MateArgs {
    const uint8_t *names1, *seqs1, *quals1, *names2, *seqs2, *quals2;
    const uint32_t *name_off1, *seq_off1, *qual_off1, *name_off2, *seq_off2, *qual_off2;
    uint8_t *names_out, *seqs_out, *quals_out;
    uint32_t *name_off_out, *seq_off_out, *qual_off_out;
    uint32_t count; // pairs
};

__global__ __launch_bounds__(kBlock) void fq_mate_offsets_kernel(MateArgs A)
{
    const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p > A.count) return;
    const uint32_t n1 = A.name_off1[p], n2 = A.name_off2[p], s1 = A.seq_off1[p], s2 = A.seq_off2[p], q1 = A.qual_off1[p], q2 = A.qual_off2[p];
    A.name_off_out[2 * p] = n1 + n2;
    A.seq_off_out[2 * p] = s1 + s2;
    A.qual_off_out[2 * p] = q1 + q2;
    if (p == A.count) return;
    A.name_off_out[2 * p + 1] = A.name_off1[p + 1] + n2;
    A.seq_off_out[2 * p + 1] = A.seq_off1[p + 1] + s2;
    A.qual_off_out[2 * p + 1] = A.qual_off1[p + 1] + q2;
}

__global__ __launch_bounds__(kBlock) void fq_mate_bytes_kernel(MateArgs A)
{
    const uint32_t which = blockIdx.y;
    const uint8_t *__restrict__ in1 = which == 0 ? A.names1 : which == 1 ? A.seqs1 : A.quals1;
    const uint8_t *__restrict__ in2 = which == 0 ? A.names2 : which == 1 ? A.seqs2 : A.quals2;
    const uint32_t *__restrict__ off1 = which == 0 ? A.name_off1 : which == 1 ? A.seq_off1 : A.qual_off1;
    const uint32_t *__restrict__ off2 = which == 0 ? A.name_off2 : which == 1 ? A.seq_off2 : A.qual_off2;
    const uint32_t *__restrict__ off = which == 0 ? A.name_off_out : which == 1 ? A.seq_off_out : A.qual_off_out;
    uint8_t *__restrict__ out = which == 0 ? A.names_out : which == 1 ? A.seqs_out : A.quals_out;
    const uint32_t n = 2u * A.count;
    const uint64_t total = off[n], j0 = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) * kStrandPer;
    if (j0 >= total) return;
    uint32_t i = 0;
    { // the last read i in [0, n - 1] with off[i] <= j0
        uint32_t hi = n - 1u;
        while (i < hi) {
            const uint32_t mid = i + (hi - i + 1u) / 2u;
            if ((uint64_t)off[mid] <= j0) i = mid;
            else hi = mid - 1u;
        }
    }
    uint32_t b = off[i], e = off[i + 1];
    uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
#pragma unroll
    for (uint32_t k = 0; k < kStrandPer; ++k) {
        const uint64_t j = j0 + k;
        if (j >= total) break; // (the bytes behind the array's end are zeros: they lie in its 16 spare bytes)
        while (j >= e && i + 1u < n) {
            ++i;
            b = e;
            e = off[i + 1];
        }
        const uint32_t r = (uint32_t)(j - b), p = i >> 1;
        const uint32_t c = (i & 1u) ? in2[off2[p] + r] : in1[off1[p] + r];
        (k < 8 ? (k < 4 ? w0 : w1) : (k < 12 ? w2 : w3)) |= c << (8u * (k & 3u));
    }
    const uint4 v = {w0, w1, w2, w3};
    *reinterpret_cast<uint4 *>(out + j0) = v;
}

} // namespace sx

using namespace sx;

// the mates of two read sets of the same count as one: read 2p <- read p of in1, read 2p + 1 <- read p of in2 (the contract of
// sx_fastq_dev holds for *out, which sx_fastq_dev_free releases; after an error it holds no memory)
int sx_fastq_mates_dev(sx_ctx *ctx, const sx_fastq_dev *in1, const sx_fastq_dev *in2, sx_fastq_dev *out)
{
    memset(out, 0, sizeof *out);
    const uint32_t count = in1->count;
    if (in2->count != count) return sx_fail_msg(ctx, SX_E_ARG, "paired reads: the two read sets differ in their counts");
    const uint64_t nb = in1->name_bytes + in2->name_bytes, sb = in1->seq_bytes + in2->seq_bytes, qb = in1->qual_bytes + in2->qual_bytes;
    if (count > 0x3FFFFFFFu || nb > 0x7FFFFFFFull || sb > 0x7FFFFFFFull || qb > 0x7FFFFFFFull)
        return sx_fail_msg(ctx, SX_E_ARG, "paired reads: four times the pairs and twice the bytes of both images must fit 32 bits");
    sx_dev_scope S;
    SX_TRY(S.take(ctx, &out->d_name_off, 2 * (size_t)count + 1));
    SX_TRY(S.take(ctx, &out->d_seq_off, 2 * (size_t)count + 1));
    SX_TRY(S.take(ctx, &out->d_qual_off, 2 * (size_t)count + 1));
    SX_TRY(S.take(ctx, &out->d_names, (size_t)nb + 16));
    SX_TRY(S.take(ctx, &out->d_seqs, (size_t)sb + 16));
    SX_TRY(S.take(ctx, &out->d_quals, (size_t)qb + 16));
    const MateArgs A = {in1->d_names,    in1->d_seqs,    in1->d_quals,    in2->d_names,    in2->d_seqs,    in2->d_quals,
                        in1->d_name_off, in1->d_seq_off, in1->d_qual_off, in2->d_name_off, in2->d_seq_off, in2->d_qual_off,
                        out->d_names,    out->d_seqs,    out->d_quals,    out->d_name_off, out->d_seq_off, out->d_qual_off, count};
    sx_launch(ctx, SX_KC_REMAP, (uint64_t)count * 48, fq_mate_offsets_kernel, dim3(sx_div_up((uint64_t)count + 1, kBlock)), dim3(kBlock), A);
    const uint64_t most = std::max(nb, std::max(sb, qb));
    if (count && most) // (every byte is read once and written once)
        sx_launch(ctx, SX_KC_REMAP, 2 * (nb + sb + qb), fq_mate_bytes_kernel, dim3(sx_div_up(most, kStrandTile), 3), dim3(kBlock), A);
    const int rc = sx_sync(ctx);
    if (rc != 0) {
        memset(out, 0, sizeof *out); // (S releases what was taken)
        return rc;
    }
    out->count = 2 * count;
    out->name_bytes = nb, out->seq_bytes = sb, out->qual_bytes = qb;
    S.keep();
    return 0;
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

static int fastq_strands_dev(sx_ctx *ctx, const sx_fastq_dev *in, sx_fastq_dev *out, uint16_t *d_flags_out)
{
    sx_dev_scope S;
    const uint32_t count = in->count;
    SX_TRY(S.take(ctx, &out->d_name_off, 2 * (size_t)count + 1));
    SX_TRY(S.take(ctx, &out->d_seq_off, 2 * (size_t)count + 1));
    SX_TRY(S.take(ctx, &out->d_qual_off, 2 * (size_t)count + 1));
    SX_TRY(S.take(ctx, &out->d_names, 2 * (size_t)in->name_bytes + 16));
    SX_TRY(S.take(ctx, &out->d_seqs, 2 * (size_t)in->seq_bytes + 16));
    SX_TRY(S.take(ctx, &out->d_quals, 2 * (size_t)in->qual_bytes + 16));
    if (count == 0) {
        SX_CHECK(hipMemsetAsync(out->d_name_off, 0, 4, ctx->stream));
        SX_CHECK(hipMemsetAsync(out->d_seq_off, 0, 4, ctx->stream));
        SX_CHECK(hipMemsetAsync(out->d_qual_off, 0, 4, ctx->stream));
        SX_TRY(sx_sync(ctx));
        S.keep();
        return 0;
    }
    // the totals the kernels' bounds rest on are the caller's: they must be the offsets' last entries
    const uint32_t *last[3] = {in->d_name_off + count, in->d_seq_off + count, in->d_qual_off + count};
    const uint32_t one[3] = {1, 1, 1};
    uint32_t h[3] = {0, 0, 0};
    SX_TRY(sx_readback_ranges(ctx, last, one, 3, h));
    if (h[0] != in->name_bytes || h[1] != in->seq_bytes || h[2] != in->qual_bytes)
        return sx_fail_msg(ctx, SX_E_ARG, "both strands: the byte counts of the read set are not its offsets' last entries");
    const StrandArgs A = {in->d_names,    in->d_seqs,     in->d_quals,    in->d_name_off,          in->d_seq_off,          in->d_qual_off,
                          out->d_names,   out->d_seqs,    out->d_quals,   (uint32_t)in->name_bytes, (uint32_t)in->seq_bytes, (uint32_t)in->qual_bytes,
                          count};
    sx_launch(ctx, SX_KC_REMAP, (uint64_t)count * 38, fq_strand_offsets_kernel, dim3(sx_div_up((uint64_t)count + 1, kBlock)), dim3(kBlock), A,
              out->d_name_off, out->d_seq_off, out->d_qual_off, d_flags_out);
    const uint64_t most = std::max(in->name_bytes, std::max(in->seq_bytes, in->qual_bytes));
    // (every byte of the input is read twice and written twice)
    if (most)
        sx_launch(ctx, SX_KC_REMAP, 4 * (in->name_bytes + in->seq_bytes + in->qual_bytes), fq_strand_bytes_kernel,
                  dim3(sx_div_up(2 * most, kStrandTile), 3), dim3(kBlock), A);
    SX_TRY(sx_sync(ctx));
    out->count = 2 * count;
    out->name_bytes = 2 * in->name_bytes, out->seq_bytes = 2 * in->seq_bytes, out->qual_bytes = 2 * in->qual_bytes;
    S.keep();
    return 0;
}

int sx_fastq_strands_dev(sx_ctx *ctx, const sx_fastq_dev *in, sx_fastq_dev *out, uint16_t *d_flags_out)
{
    if (!ctx || !in || !out || in == out) return SX_E_ARG;
    memset(out, 0, sizeof *out);
    if (!in->d_name_off || !in->d_seq_off || !in->d_qual_off || (in->count && (!in->d_names || !in->d_seqs || !in->d_quals || !d_flags_out)) ||
        ((uintptr_t)d_flags_out & 1))
        return sx_fail_msg(ctx, SX_E_ARG, "both strands: the six arrays of a read set and room for the flags are needed");
    if (in->count > 0x7FFFFFFFu || in->name_bytes > 0x7FFFFFFFull || in->seq_bytes > 0x7FFFFFFFull || in->qual_bytes > 0x7FFFFFFFull)
        return sx_fail_msg(ctx, SX_E_ARG, "both strands: twice the reads' count and bytes must fit 32 bits");
    SX_CHECK(hipSetDevice(ctx->device));
    const int rc = fastq_strands_dev(ctx, in, out, d_flags_out);
    if (rc != 0) memset(out, 0, sizeof *out); // (what was allocated has been released)
    return sx_nomem_of(rc);
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

} // extern "C"
