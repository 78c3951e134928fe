// sx_sam.hip -- SAM text of k-edit search hits on the device (bioinf/sam.c print_sam_line); the read mapper's loop
// (sx_map.hip) calls its layout and emit through sx_sam.hpp.
//
// One hit (sx_approx_hit) is an interval of a suffix array; it prints R - L lines
//     <qname>\t0\t<rname>\t<sa[i]+1>\t0\t<cigar>\t*\t0\t0\t<seq>\t<qual>\n          i = L .. R-1
// that differ in the position's digits only.  The second field is 0, or, where the batch brings a FLAG per read (the
// kernels' kFlags form: the reads of both strands), that FLAG in decimal.  Two steps (DESIGN.md
// section 11, "SAM text"):
//  * layout: a size pass gives every hit its byte count, (R - L) x (the fixed part for this read, record name and
//    CIGAR) plus the digits of every sa[i] + 1 (hits of more than 32 matches are summed by their whole workgroup),
//    and a 64-bit exclusive scan turns the counts into each hit's first output byte and the total.
//  * emit: writes the bytes of a window [byte_lo, byte_hi) of the output.  A workgroup owns a slice of the window,
//    finds the hit at its first byte by a search in the scanned offsets and the match inside the hit by a walk over
//    the interval (1024 matches a step), lays lines out in LDS, one lane a line, 256 lines a step (the CIGAR of a hit
//    is rendered once into LDS, not once per match), and stores the slice in 16-byte vector stores.  The last < 16
//    bytes of a window whose length is not a multiple of 16 are the only bytes stored singly.  Where a byte goes is
//    fixed by the scan alone (no atomics), so the text does not depend on scheduling.
// With the texts of the records (the kernels' kTags form) every line has "\tNM:i:<nm>\tMD:Z:<md>" between
// its quality string and its newline: one walk a hit over its edit string, the read and the text window at its first
// position (md_render), in the size pass for the length and in the emit pass into LDS, beside the CIGAR.
// Unmapped read groups (SX_MAP_UNMAPPED): a hit with an empty interval (R == L, which no search
// gives) is the placeholder of a read group without a line and prints "<qname>\t4\t*\t0\t0\t*\t*\t0\t0\t<seq>\t<qual>\n"
// -- in the kernels' kUnmapped forms alone, their fourth template parameter; the forms without it keep their code.
// MAPQ and secondary lines (SX_MAP_MAPQ): a 16-bit quality word a hit gives the MAPQ printed where
// the "0" behind POS stands and, by its bit 8, 256 on top of the FLAG of every line of the hit -- in the kernels' kMapq
// forms alone, their fifth template parameter, which take the FLAG array (null: 0) and the placeholders at run time.
// The output does not fit the device in general: the caller fills a fixed buffer window after window; lines may start
// in one window (or slice) and end in the next, the concatenation of the windows is the file.
#include "sx_common.hpp"
#include "sx_device.hpp"
#include "sx_scan.hpp"
#include "sx_sam.hpp"

namespace sx {

#ifndef SX_SAM_SLICE_BYTES
#define SX_SAM_SLICE_BYTES 16384u // output bytes a workgroup lays out in LDS (a multiple of 16)
#endif
static_assert(SX_SAM_SLICE_BYTES % 16 == 0 && SX_SAM_SLICE_BYTES >= 16 && SX_SAM_SLICE_BYTES <= 32768, "slice");

constexpr uint32_t kSlice = SX_SAM_SLICE_BYTES;
constexpr uint32_t kCigarMax = 80;  // 9 runs of M (5 digits) and 8 of I / D (1 digit) take 70 bytes; longer ones are cut
// MD:Z of a hit: a search of at most SX_APPROX_MAX_EDITS = 8 operations gives at most 8 items (a mismatch: its letter; a
// deletion: '^', or nothing behind another deletion, and its letter) between at most 9 numbers of at most 5 digits (the
// edit string has fewer than 2^15 + 8 entries): 9 x 5 + 8 x 2 = 61 bytes.  NM is one digit.
constexpr uint32_t kMdMax = 64;
static_assert(SX_APPROX_MAX_EDITS == 8 && 9 * 5 + 8 * 2 <= kMdMax, "MD:Z of 8 edits fits its buffer");
constexpr uint32_t kInlineMatches = 32;
constexpr uint32_t kWalk = 4; // matches per lane in one step of the walk inside a long hit

struct HitInfo {
    const uint32_t *pos; // the hit's positions: pos[0 .. cnt)
    uint32_t cnt, fixed, cig_len, m, flag;
    uint32_t name_b, name_l, seq_b, seq_l, qual_b, qual_l, rn_b, rn_l;
    uint4 gaps;
    uint32_t n_gaps;
    uint32_t rec, nm, md_len; // (kTags) the record's rank; NM and the bytes of MD once tags_render has run
    uint32_t mapq;            // (kMapq) the MAPQ of the hit's lines
};

__device__ __forceinline__ uint32_t dec_digits(uint32_t v)
{
    return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u
           : v < 10000000u ? 7u : v < 100000000u ? 8u : v < 1000000000u ? 9u : 10u;
}

// decimal digits of v into out[at ..) as far as cap allows (out == nullptr: count only); returns the new length
__device__ __forceinline__ uint32_t put_dec(uint8_t *out, uint32_t at, uint32_t cap, uint32_t v)
{
    const uint32_t nd = dec_digits(v);
    for (uint32_t d = 0; d < nd; ++d) {
        const uint32_t where = at + nd - 1u - d;
        if (out && where < cap) out[where] = (uint8_t)('0' + v % 10u);
        v /= 10u;
    }
    return at + nd < cap ? at + nd : cap;
}

// cigar.c edits_to_cigar of the hit's edit string in pattern order (stralg_host.c approx_cigar): runs of equal
// operations, "%d%c" each; at most cap bytes
__device__ __forceinline__ uint32_t cigar_render(uint8_t *out, uint32_t cap, uint32_t m, uint4 gaps, uint32_t ng)
{
    const uint32_t gw[4] = {gaps.x, gaps.y, gaps.z, gaps.w};
    uint32_t n_d = 0;
    for (uint32_t g = 0; g < ng; ++g) n_d += ((gw[g >> 1] >> (16u * (g & 1u))) & SX_APPROX_GAP_D) ? 1u : 0u;
    const uint32_t len = m + n_d;
    uint32_t w = 0, pos = 0, g = 0;
    while (pos < len) {
        const uint32_t e = g < ng ? (gw[g >> 1] >> (16u * (g & 1u))) & 0xFFFFu : 0u;
        uint32_t run = 0;
        uint8_t op = 'M';
        if (g < ng && (e & 0x7FFFu) == pos) {
            op = (e & SX_APPROX_GAP_D) ? 'D' : 'I';
            while (g < ng && pos < len) {
                const uint32_t e2 = (gw[g >> 1] >> (16u * (g & 1u))) & 0xFFFFu;
                if ((e2 & 0x7FFFu) != pos || (e2 & SX_APPROX_GAP_D) != (e & SX_APPROX_GAP_D)) break;
                ++g;
                ++pos;
                ++run;
            }
        } else {
            const uint32_t next = (g < ng && (e & 0x7FFFu) > pos && (e & 0x7FFFu) < len) ? (e & 0x7FFFu) : len;
            run = next - pos;
            pos = next;
        }
        w = put_dec(out, w, cap, run);
        if (w < cap) {
            if (out) out[w] = op;
            ++w;
        }
    }
    return w;
}

// ---- NM:i and MD:Z ----------------------------------------------------------------------------------
// entry g of a hit's gap[] (selects, not an indexed array: that would go to scratch or LDS)
__device__ __forceinline__ uint32_t gap_at(uint4 gaps, uint32_t g)
{
    const uint32_t w = g < 4 ? (g < 2 ? gaps.x : gaps.y) : (g < 6 ? gaps.z : gaps.w);
    return (w >> (16u * (g & 1u))) & 0xFFFFu;
}
__device__ __forceinline__ uint32_t gap_deletions(uint4 gaps, uint32_t ng)
{
    uint32_t n_d = 0;
#pragma unroll
    for (uint32_t g = 0; g < SX_APPROX_MAX_EDITS; ++g) n_d += (g < ng && (gap_at(gaps, g) & SX_APPROX_GAP_D)) ? 1u : 0u;
    return n_d;
}

// The bytes of a text [lo, hi) one at a time, through the 16 aligned bytes around the last one asked for: a chunk that lies
// inside the text is one 16-byte load, the chunks across its first and its last byte are read byte by byte
// (at: the chunk's address, an odd number while there is none; b: its four words, kept apart so that they stay registers)
__device__ __forceinline__ uint32_t text_symbol(const uint8_t *lo, const uint8_t *hi, const uint8_t *p, uintptr_t &at, uint32_t &b0, uint32_t &b1,
                                                uint32_t &b2, uint32_t &b3)
{
    const uintptr_t a = (uintptr_t)p & ~(uintptr_t)15;
    if (a != at) {
        at = a;
        if (a >= (uintptr_t)lo && a + 16 <= (uintptr_t)hi) {
            const uint4 v = *(const uint4 *)a;
            b0 = v.x, b1 = v.y, b2 = v.z, b3 = v.w;
        } else {
            b0 = b1 = b2 = b3 = 0;
#pragma unroll
            for (uint32_t k = 0; k < 16; ++k) {
                const uint8_t *q = (const uint8_t *)a + k;
                const uint32_t v = (q >= lo && q < hi) ? (uint32_t)*q << (8u * (k & 3u)) : 0u;
                (k < 8 ? (k < 4 ? b0 : b1) : (k < 12 ? b2 : b3)) |= v;
            }
        }
    }
    const uint32_t k = (uint32_t)((uintptr_t)p & 15);
    const uint32_t w = k < 8 ? (k < 4 ? b0 : b1) : (k < 12 ? b2 : b3);
    return (w >> (8u * (k & 3u))) & 0xFFu;
}

// One walk over a hit's edit string (pattern order), the read's bytes and the text from the hit's first position on: an M
// step compares the read's byte with the letter behind the text's code, an I step takes a read byte, a D step a text
// symbol.  Returns the bytes of MD:Z (at most cap; out == nullptr: the length only, as cigar_render) and *nm <- the
// mismatches, inserted and deleted symbols.  The window is win[0 .. tlen) inside the text [lo, hi); the walk stays inside
// the read's m bytes and the window whatever the edit string holds.
__device__ __forceinline__ uint32_t md_render(uint8_t *out, uint32_t cap, uint32_t m, uint4 gaps, uint32_t ng, const uint8_t *read,
                                              const uint8_t *lo, const uint8_t *hi, const uint8_t *win, uint32_t tlen, const uint8_t *letters,
                                              uint32_t *nm)
{
    const uint32_t len = m + gap_deletions(gaps, ng);
    uintptr_t at = 1;
    uint32_t b0 = 0, b1 = 0, b2 = 0, b3 = 0;
    uint32_t w = 0, run = 0, edits = 0, ri = 0, ti = 0, g = 0;
    bool in_del = false; // the step before was a D: this one's letter joins its '^' group
    for (uint32_t pos = 0; pos < len; ++pos) {
        const uint32_t e = g < ng ? gap_at(gaps, g) : 0u;
        if (g < ng && (e & 0x7FFFu) == pos) {
            ++g;
            ++edits;
            if (e & SX_APPROX_GAP_D) {
                if (ti >= tlen) break;
                if (!in_del) {
                    w = put_dec(out, w, cap, run);
                    if (w < cap) {
                        if (out) out[w] = '^';
                        ++w;
                    }
                    run = 0;
                }
                if (w < cap) {
                    if (out) out[w] = letters[text_symbol(lo, hi, win + ti, at, b0, b1, b2, b3)];
                    ++w;
                }
                ++ti;
                in_del = true;
            } else {
                ++ri;
                in_del = false;
            }
            continue;
        }
        if (ri >= m || ti >= tlen) break;
        const uint8_t a = letters[text_symbol(lo, hi, win + ti, at, b0, b1, b2, b3)];
        if (a == read[ri]) {
            ++run;
        } else {
            w = put_dec(out, w, cap, run);
            if (w < cap) {
                if (out) out[w] = a;
                ++w;
            }
            run = 0;
            ++edits;
        }
        ++ri;
        ++ti;
        in_del = false;
    }
    *nm = edits;
    return put_dec(out, w, cap, run);
}

// what the lines of hit h are made of; false: the hit does not fit the batch (its query, interval or offsets).
// kUnmapped: a hit with R == L is the placeholder of a read group without a line, and has one line,
// the FLAG 4 line of its read: I.pos == nullptr, I.cnt == 1 (no position, CIGAR or tags are read for it)
// kMapq: quality[h] gives the hit's MAPQ and, by bit 8, 256 on top of its FLAG; the FLAG array may
// be null (FLAG 0) and a placeholder's quality word is not looked at
template <bool kLocated, bool kFlags, bool kUnmapped = false, bool kMapq = false>
__device__ __forceinline__ bool hit_info(const SamArgs &A, uint64_t h, HitInfo &I, const uint16_t *quality = nullptr)
{
    const uint4 h0 = A.hits[2 * h];
    I.gaps = A.hits[2 * h + 1];
    I.cnt = 0;
    I.fixed = 0;
    I.cig_len = 0;
    I.flag = 0;
    I.pos = nullptr;
    const uint32_t vq = h0.x, L = h0.y, R = h0.z;
    if ((uint64_t)vq >= (uint64_t)A.n_reads * A.n_records || L > R) return false;
    const uint32_t read = vq / A.n_records, rec = vq - read * A.n_records;
    const uint32_t *sa = kLocated ? nullptr : A.sa_list ? A.sa_list[rec] : A.sa;
    const uint64_t sa_len = A.sa_list ? A.sa_len_list[rec] : A.sa_len;
    if ((uint64_t)R > sa_len) return false;
    I.name_b = A.name_off[read];
    I.seq_b = A.seq_off[read];
    I.qual_b = A.qual_off[read];
    I.rn_b = A.rname_off[rec];
    const uint32_t name_e = A.name_off[read + 1], seq_e = A.seq_off[read + 1], qual_e = A.qual_off[read + 1],
                   rn_e = A.rname_off[rec + 1];
    if (name_e < I.name_b || seq_e < I.seq_b || qual_e < I.qual_b || rn_e < I.rn_b) return false;
    I.name_l = name_e - I.name_b;
    I.seq_l = seq_e - I.seq_b;
    I.qual_l = qual_e - I.qual_b;
    I.rn_l = rn_e - I.rn_b;
    I.m = I.seq_l;
    I.rec = rec;
    I.n_gaps = h0.w >> 16;
    if (I.n_gaps > SX_APPROX_MAX_EDITS) I.n_gaps = SX_APPROX_MAX_EDITS;
    if (kUnmapped && L == R) {
        I.n_gaps = 0;
        I.cnt = 1;
        I.flag = 4;
        return true;
    }
    I.pos = kLocated ? A.positions + (A.pos_off[h] - A.pos_base) : sa + L;
    I.cnt = R - L;
    if (kMapq) {
        const uint32_t w = quality[h];
        I.flag = (A.flags ? A.flags[read] : 0u) | (w & 0x100u);
        I.mapq = w & 0xFFu;
    } else if (kFlags) {
        I.flag = A.flags[read];
    }
    return true;
}

// NM and MD of hit I, which has a line (I.cnt > 0): the text window starts at the hit's first position and has as many
// symbols as the edit string takes of the text.  false: the window leaves the text in front of its sentinel, [0, N - 1),
// or the walk finds more than SX_APPROX_MAX_EDITS differences -- such a hit is malformed, like one outside the batch
__device__ __forceinline__ bool tags_render(const SamTagArgs &A, HitInfo &I, uint8_t *out)
{
    const uint32_t n_d = gap_deletions(I.gaps, I.n_gaps), n_i = I.n_gaps - n_d;
    const uint64_t N = A.sa_list ? A.sa_len_list[I.rec] : A.sa_len;
    I.nm = 0, I.md_len = 0;
    if (I.m + n_d < n_i) return false;
    const uint64_t tlen = I.m + n_d - n_i, p = I.pos[0];
    const uint8_t *text = A.text_list[I.rec];
    if (!text || N == 0 || p + tlen > N - 1) return false;
    I.md_len = md_render(out, kMdMax, I.m, I.gaps, I.n_gaps, A.seqs + I.seq_b, text, text + N, text + p, (uint32_t)tlen, A.letters + (size_t)I.rec * 256, &I.nm);
    return I.nm <= SX_APPROX_MAX_EDITS;
}

// "\t0\t" + "\t" + "\t0\t" + "\t*\t0\t0\t" + "\t" + "\n": the 16 bytes of a line beside its fields and digits; a FLAG
// takes its digits in place of the first "0" (without kFlags I.flag is the constant 0: one digit, 16 bytes)
template <bool kTags = false, bool kMapq = false> __device__ __forceinline__ uint32_t fixed_bytes(const HitInfo &I)
{
    // (kTags) "\tNM:i:" + "\tMD:Z:" and the one digit of NM <= 8: 13 bytes beside the bytes of MD
    // (kMapq) the MAPQ takes its digits in place of the "0" behind POS
    if (kMapq) return I.name_l + I.rn_l + I.cig_len + I.seq_l + I.qual_l + 14u + dec_digits(I.flag) + dec_digits(I.mapq) + (kTags ? 13u + I.md_len : 0u);
    return I.name_l + I.rn_l + I.cig_len + I.seq_l + I.qual_l + 15u + dec_digits(I.flag) + (kTags ? 13u + I.md_len : 0u);
}

// "\t4\t*\t0\t0\t*\t*\t0\t0\t" + "\t" + "\n": the whole FLAG 4 line of a placeholder beside its QNAME, SEQ and QUAL (no tags)
constexpr uint32_t kUnmappedFixed = 19;
__device__ __forceinline__ uint32_t unmapped_bytes(const HitInfo &I) { return I.name_l + I.seq_l + I.qual_l + kUnmappedFixed; }

// ---- layout: bytes per hit ---------------------------------------------------------------------
// what a kernel takes of a batch: the tagged forms alone carry the texts and the letters
// and the kMapq forms, with tags or without, the quality words as well
template <bool kTags, bool kMapq = false> struct KernelArgs { typedef SamArgs type; };
template <> struct KernelArgs<true, false> { typedef SamTagArgs type; };
template <bool kTags> struct KernelArgs<kTags, true> { typedef SamMapqArgs type; };
__device__ __forceinline__ const uint16_t *quality_of(const SamArgs &) { return nullptr; }
__device__ __forceinline__ const uint16_t *quality_of(const SamMapqArgs &A) { return A.quality; }
// (the forms without tags never get there)
__device__ __forceinline__ bool tags_render(const SamArgs &, HitInfo &, uint8_t *) { return true; }

// kUnmapped: the forms of SX_MAP_UNMAPPED (placeholders print a FLAG 4 line); with it false the code is the one from before
// kMapq: the forms of SX_MAP_MAPQ (kFlags and kUnmapped set: both are looked at at run time); the same holds of it
template <bool kLocated, bool kFlags, bool kTags, bool kUnmapped, bool kMapq = false>
__global__ __launch_bounds__(kBlock) void sam_size_kernel(typename KernelArgs<kTags, kMapq>::type A, uint64_t *len_out, uint32_t *err)
{
    __shared__ uint64_t red[kWavesPerBlock];
    __shared__ uint32_t long_cnt[kBlock];
    __shared__ const uint32_t *long_pos[kBlock];
    const uint32_t t = threadIdx.x;
    const uint64_t h = (uint64_t)blockIdx.x * kBlock + t;
    uint64_t bytes = 0;
    long_cnt[t] = 0;
    if (h < A.n_hits) {
        HitInfo I = {};
        if (!hit_info<kLocated, kFlags, kUnmapped, kMapq>(A, h, I, quality_of(A))) {
            atomicOr(err, 1u);
        } else if (kUnmapped && !I.pos) {
            bytes = unmapped_bytes(I);
        } else {
            I.cig_len = cigar_render(nullptr, kCigarMax, I.m, I.gaps, I.n_gaps);
            if (kTags && I.cnt && !tags_render(A, I, nullptr)) {
                atomicOr(err, 1u);
                I.cnt = 0;
            }
            bytes = (uint64_t)I.cnt * fixed_bytes<kTags, kMapq>(I);
            if (I.cnt <= kInlineMatches) {
                for (uint32_t i = 0; i < I.cnt; ++i) bytes += dec_digits(I.pos[i] + 1u);
            } else {
                long_cnt[t] = I.cnt;
                long_pos[t] = I.pos;
            }
        }
    }
    __syncthreads();
    // long intervals (up to 10^5 matches and more): the whole workgroup sums one's digits
    for (uint32_t u = 0; u < (uint32_t)kBlock; ++u) {
        const uint32_t cnt = long_cnt[u]; // (the same for every lane)
        if (cnt == 0) continue;
        const uint32_t *pos = long_pos[u];
        uint64_t d = 0;
        for (uint32_t i = t; i < cnt; i += kBlock) d += dec_digits(pos[i] + 1u);
        uint64_t tot;
        (void)block_exclusive_sum_u64(d, red, tot);
        if (u == t) bytes += tot;
    }
    if (h < A.n_hits) len_out[h] = bytes;
}

// ---- emit ---------------------------------------------------------------------------------------
struct HitLds {
    const uint32_t *pos;
    uint32_t cnt, fixed, cig_len;
    uint32_t name_b, name_l, seq_b, seq_l, qual_b, qual_l, rn_b, rn_l;
    uint32_t tags; // (kTags) the bytes of MD, and NM from bit 8 on (it fills the struct's 8-byte alignment)
};

// n bytes of a line that begins at slice offset `off` (may be negative), clipped to the slice
__device__ __forceinline__ void put_bytes(uint8_t *obuf, int64_t &off, int64_t slice_len, const uint8_t *src, uint32_t n)
{
    int64_t k0 = off < 0 ? -off : 0, k1 = (int64_t)n < slice_len - off ? (int64_t)n : slice_len - off;
    for (int64_t k = k0; k < k1; ++k) obuf[off + k] = src[k];
    off += n;
}

// kUnmapped: as in sam_size_kernel; a placeholder is kept as a hit of 1 line with HitLds::pos == nullptr and HitLds::fixed
// the line's whole length
// kMapq: as in sam_size_kernel; the MAPQ of the step's hits lies beside their FLAGs
template <bool kLocated, bool kFlags, bool kTags, bool kUnmapped, bool kMapq = false>
__global__ __launch_bounds__(kBlock) void sam_emit_kernel(typename KernelArgs<kTags, kMapq>::type A, const uint64_t *byte_off, uint64_t lo, uint64_t hi, uint8_t *out)
{
    __shared__ uint4 obuf4[kSlice / 16];
    __shared__ uint8_t cig[kBlock * kCigarMax];
    __shared__ HitLds hl[kBlock];
    __shared__ uint32_t mo[kBlock + 1];
    __shared__ uint64_t red[kWavesPerBlock];
    __shared__ uint32_t red32[kWavesPerBlock];
    __shared__ uint64_t nxt[2];
    __shared__ uint16_t hflag[kFlags ? kBlock : 1]; // (kFlags) the FLAG of the step's hits
    __shared__ uint8_t md[kTags ? kBlock * kMdMax : 1]; // (kTags) MD:Z of the step's hits, rendered once a hit like the CIGAR
    __shared__ uint8_t hmapq[kMapq ? kBlock : 1];       // (kMapq) the MAPQ of the step's hits
    uint8_t *obuf = (uint8_t *)obuf4;
    const uint32_t t = threadIdx.x;
    const uint64_t s_lo = lo + (uint64_t)blockIdx.x * kSlice;
    if (s_lo >= hi) return; // (the whole workgroup)
    const uint64_t s_hi = hi - s_lo < kSlice ? hi : s_lo + kSlice;
    const int64_t slice_len = (int64_t)(s_hi - s_lo);

    // the hit at the slice's first byte: the last h with byte_off[h] <= s_lo (byte_off[n_hits] = total > s_lo)
    uint64_t h = 0;
    {
        uint64_t b = A.n_hits;
        while (b - h > 1) {
            const uint64_t mid = h + (b - h) / 2;
            if (byte_off[mid] <= s_lo) h = mid;
            else b = mid;
        }
    }
    uint64_t pos = byte_off[h]; // first byte of line (h, i)
    uint32_t i = 0;
    {   // the walk inside the hit: whole steps of 1024 lines that end at or before the slice's first byte are skipped
        HitInfo I = {};
        if (hit_info<kLocated, kFlags, kUnmapped, kMapq>(A, h, I, quality_of(A))) { // (a placeholder has 1 line: no walk)
            I.cig_len = cigar_render(nullptr, kCigarMax, I.m, I.gaps, I.n_gaps);
            // (the tags' length is needed by the steps below alone: a hit of up to 1024 lines, which is nearly every hit,
            //  is not walked here, only by its lane in the loop further down)
            if (kTags && I.cnt > kWalk * kBlock && !tags_render(A, I, nullptr)) I.cnt = 0;
            const uint32_t fixed = fixed_bytes<kTags, kMapq>(I);
            while (I.cnt - i > kWalk * kBlock) {
                uint64_t b = 0;
#pragma unroll
                for (uint32_t k = 0; k < kWalk; ++k) b += fixed + dec_digits(I.pos[i + k * kBlock + t] + 1u);
                uint64_t tot;
                (void)block_exclusive_sum_u64(b, red, tot);
                if (pos + tot > s_lo) break;
                pos += tot;
                i += kWalk * kBlock;
            }
        }
    }

    while (pos < s_hi && h < A.n_hits) {
        // hits h .. h + 255: how many lines each has left, the first 256 lines' hits, their CIGARs
        HitInfo I = {};
        uint32_t c = 0;
        if (h + t < A.n_hits && hit_info<kLocated, kFlags, kUnmapped, kMapq>(A, h + t, I, quality_of(A))) c = I.cnt - (t == 0 ? (i < I.cnt ? i : I.cnt) : 0u);
        const uint32_t cc = c < (uint32_t)kBlock ? c : (uint32_t)kBlock;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan<OpAdd>(cc, red32, total);
        mo[t] = ex;
        if (t == 0) mo[kBlock] = total;
        if (kUnmapped && cc && ex < (uint32_t)kBlock && !I.pos) {
            HitLds &H = hl[t];
            H.pos = nullptr;
            H.cnt = 1;
            H.fixed = unmapped_bytes(I);
            H.name_b = I.name_b, H.name_l = I.name_l, H.seq_b = I.seq_b, H.seq_l = I.seq_l;
            H.qual_b = I.qual_b, H.qual_l = I.qual_l;
        } else if (cc && ex < (uint32_t)kBlock) {
            I.cig_len = cigar_render(cig + t * kCigarMax, kCigarMax, I.m, I.gaps, I.n_gaps);
            HitLds &H = hl[t];
            H.pos = I.pos;
            H.cnt = I.cnt;
            H.cig_len = I.cig_len;
            if (kTags) {
                (void)tags_render(A, I, md + t * kMdMax); // (a hit that the layout refused never gets here)
                H.tags = I.md_len | (I.nm << 8);
            }
            H.fixed = fixed_bytes<kTags, kMapq>(I);
            H.name_b = I.name_b, H.name_l = I.name_l, H.seq_b = I.seq_b, H.seq_l = I.seq_l;
            H.qual_b = I.qual_b, H.qual_l = I.qual_l, H.rn_b = I.rn_b, H.rn_l = I.rn_l;
            if (kFlags) hflag[t] = (uint16_t)I.flag;
            if (kMapq) hmapq[t] = (uint8_t)I.mapq;
        }
        __syncthreads();
        const uint32_t nlines = total < (uint32_t)kBlock ? total : (uint32_t)kBlock;
        if (nlines == 0) { // 256 hits without a line (malformed ones): on to the next
            h += kBlock;
            i = 0;
            __syncthreads();
            continue;
        }
        // line t of this step
        uint32_t u = 0, mi = 0, p1 = 0, len = 0;
        if (t < nlines) {
            uint32_t a = 0, b = kBlock; // mo[a] <= t < mo[b]
            while (b - a > 1) {
                const uint32_t mid = (a + b) / 2;
                if (mo[mid] <= t) a = mid;
                else b = mid;
            }
            u = a;
            mi = t - mo[u] + (u == 0 ? i : 0u);
            if (kUnmapped && !hl[u].pos) {
                len = hl[u].fixed;
            } else {
                p1 = hl[u].pos[mi] + 1u;
                len = hl[u].fixed + dec_digits(p1);
            }
        }
        uint32_t step_bytes;
        const uint32_t lstart = block_exclusive_scan<OpAdd>(len, red32, step_bytes);
        const uint64_t line_abs = pos + lstart;
        if (kUnmapped && t < nlines && line_abs < s_hi && line_abs + len > s_lo && !hl[u].pos) {
            const HitLds &H = hl[u];
            int64_t off = (int64_t)line_abs - (int64_t)s_lo;
            put_bytes(obuf, off, slice_len, A.names + H.name_b, H.name_l);
            put_bytes(obuf, off, slice_len, (const uint8_t *)"\t4\t*\t0\t0\t*\t*\t0\t0\t", 17);
            put_bytes(obuf, off, slice_len, A.seqs + H.seq_b, H.seq_l);
            put_bytes(obuf, off, slice_len, (const uint8_t *)"\t", 1);
            put_bytes(obuf, off, slice_len, A.quals + H.qual_b, H.qual_l);
            put_bytes(obuf, off, slice_len, (const uint8_t *)"\n", 1);
        } else if (t < nlines && line_abs < s_hi && line_abs + len > s_lo) {
            const HitLds &H = hl[u];
            int64_t off = (int64_t)line_abs - (int64_t)s_lo;
            uint8_t dig[10];
            const uint32_t nd = put_dec(dig, 0, 10, p1);
            put_bytes(obuf, off, slice_len, A.names + H.name_b, H.name_l);
            if (kFlags) {
                uint8_t fdig[5];
                const uint32_t nf = put_dec(fdig, 0, 5, hflag[u]);
                put_bytes(obuf, off, slice_len, (const uint8_t *)"\t", 1);
                put_bytes(obuf, off, slice_len, fdig, nf);
                put_bytes(obuf, off, slice_len, (const uint8_t *)"\t", 1);
            } else {
                put_bytes(obuf, off, slice_len, (const uint8_t *)"\t0\t", 3);
            }
            put_bytes(obuf, off, slice_len, A.rnames + H.rn_b, H.rn_l);
            put_bytes(obuf, off, slice_len, (const uint8_t *)"\t", 1);
            put_bytes(obuf, off, slice_len, dig, nd);
            if (kMapq) {
                uint8_t qdig[3];
                const uint32_t nq = put_dec(qdig, 0, 3, hmapq[u]);
                put_bytes(obuf, off, slice_len, (const uint8_t *)"\t", 1);
                put_bytes(obuf, off, slice_len, qdig, nq);
                put_bytes(obuf, off, slice_len, (const uint8_t *)"\t", 1);
            } else {
                put_bytes(obuf, off, slice_len, (const uint8_t *)"\t0\t", 3);
            }
            put_bytes(obuf, off, slice_len, cig + u * kCigarMax, H.cig_len);
            put_bytes(obuf, off, slice_len, (const uint8_t *)"\t*\t0\t0\t", 7);
            put_bytes(obuf, off, slice_len, A.seqs + H.seq_b, H.seq_l);
            put_bytes(obuf, off, slice_len, (const uint8_t *)"\t", 1);
            put_bytes(obuf, off, slice_len, A.quals + H.qual_b, H.qual_l);
            if (kTags) {
                const uint8_t nm = (uint8_t)('0' + (H.tags >> 8)); // (at most SX_APPROX_MAX_EDITS: the layout refuses the others)
                put_bytes(obuf, off, slice_len, (const uint8_t *)"\tNM:i:", 6);
                put_bytes(obuf, off, slice_len, &nm, 1);
                put_bytes(obuf, off, slice_len, (const uint8_t *)"\tMD:Z:", 6);
                put_bytes(obuf, off, slice_len, md + u * kMdMax, H.tags & 0xFFu);
            }
            put_bytes(obuf, off, slice_len, (const uint8_t *)"\n", 1);
        }
        if (t == nlines - 1u) { // the line behind this step's last one
            const bool more = mi + 1u < hl[u].cnt;
            nxt[0] = h + u + (more ? 0u : 1u);
            nxt[1] = more ? mi + 1u : 0u;
        }
        __syncthreads();
        h = nxt[0];
        i = (uint32_t)nxt[1];
        pos += step_bytes;
        __syncthreads();
    }
    __syncthreads();
    // the slice leaves in 16-byte stores; a window that does not end on a 16-byte boundary has up to 15 single bytes
    uint8_t *dst = out + (s_lo - lo);
    const uint32_t full = (uint32_t)(slice_len / 16);
    for (uint32_t k = t; k < full; k += kBlock) stream_store16((uint4 *)dst + k, obuf4[k]);
    const uint32_t tail = (uint32_t)slice_len - full * 16u;
    if (t < tail) dst[full * 16u + t] = obuf[full * 16u + t];
}

// ---- lines with a mate ---------------------------------------------------------------------------
// A line descriptor (sx_pair_line) names a hit and brings POS, FLAG, PNEXT and TLEN; the hit gives the read, the record and
// the CIGAR.  One lane a line in both passes: a line's first byte is its entry of the scanned sizes, so the emit needs no walk
// inside a hit and no step over 256 hits.  The kernels are separate from the ones above, which keep their registers and LDS.
struct PairHit {
    uint32_t name_b, name_l, seq_b, seq_l, qual_b, qual_l, rn_b, rn_l, n_gaps;
    uint4 gaps;
};

// what line descriptors take of hit h (hit_info without the positions); false: the hit does not fit the batch
__device__ __forceinline__ bool pair_hit(const SamArgs &A, uint64_t h, PairHit &P)
{
    if (h >= A.n_hits) return false;
    const uint4 h0 = A.hits[2 * h];
    P.gaps = A.hits[2 * h + 1];
    const uint32_t vq = h0.x;
    if ((uint64_t)vq >= (uint64_t)A.n_reads * A.n_records) return false;
    const uint32_t read = vq / A.n_records, rec = vq - read * A.n_records;
    P.name_b = A.name_off[read];
    P.seq_b = A.seq_off[read];
    P.qual_b = A.qual_off[read];
    P.rn_b = A.rname_off[rec];
    const uint32_t name_e = A.name_off[read + 1], seq_e = A.seq_off[read + 1], qual_e = A.qual_off[read + 1], rn_e = A.rname_off[rec + 1];
    if (name_e < P.name_b || seq_e < P.seq_b || qual_e < P.qual_b || rn_e < P.rn_b) return false;
    P.name_l = name_e - P.name_b;
    P.seq_l = seq_e - P.seq_b;
    P.qual_l = qual_e - P.qual_b;
    P.rn_l = rn_e - P.rn_b;
    P.n_gaps = h0.w >> 16;
    if (P.n_gaps > SX_APPROX_MAX_EDITS) P.n_gaps = SX_APPROX_MAX_EDITS;
    return true;
}

__device__ __forceinline__ uint32_t tlen_magnitude(int32_t t) { return t < 0 ? 0u - (uint32_t)t : (uint32_t)t; }

// the digits of v at slice offset `off` (may be negative), clipped to the slice; no buffer of the lane's own
__device__ __forceinline__ void put_dec_clipped(uint8_t *obuf, int64_t &off, int64_t slice_len, uint32_t v)
{
    const uint32_t nd = dec_digits(v);
    for (uint32_t d = 0; d < nd; ++d) {
        const int64_t where = off + (int64_t)(nd - 1u - d);
        if (where >= 0 && where < slice_len) obuf[where] = (uint8_t)('0' + v % 10u);
        v /= 10u;
    }
    off += nd;
}

// 10 tabs, the newline, MAPQ "0" and RNEXT "=": the 13 bytes of a line beside its fields and numbers
__global__ __launch_bounds__(kBlock) void sam_pair_size_kernel(SamArgs A, const sx_pair_line *lines, uint64_t n_lines, uint64_t *len_out, uint32_t *err)
{
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n_lines) return;
    const sx_pair_line D = lines[j];
    PairHit P;
    uint64_t bytes = 0;
    if (!pair_hit(A, D.hit, P)) {
        atomicOr(err, 1u);
    } else {
        bytes = (uint64_t)P.name_l + P.rn_l + cigar_render(nullptr, kCigarMax, P.seq_l, P.gaps, P.n_gaps) + P.seq_l + P.qual_l + 13u +
                dec_digits(D.flag) + dec_digits(D.pos) + dec_digits(D.pnext) + (D.tlen < 0 ? 1u : 0u) + dec_digits(tlen_magnitude(D.tlen));
    }
    len_out[j] = bytes;
}

__global__ __launch_bounds__(kBlock) void sam_pair_emit_kernel(SamArgs A, const sx_pair_line *lines, uint64_t n_lines, const uint64_t *byte_off,
                                                               uint64_t lo, uint64_t hi, uint8_t *out)
{
    __shared__ uint4 obuf4[kSlice / 16];
    __shared__ uint8_t cig[kBlock * kCigarMax]; // a lane's CIGAR: rendered once, then copied like a field
    uint8_t *obuf = (uint8_t *)obuf4;
    const uint32_t t = threadIdx.x;
    const uint64_t s_lo = lo + (uint64_t)blockIdx.x * kSlice;
    if (s_lo >= hi) return; // (the whole workgroup)
    const uint64_t s_hi = hi - s_lo < kSlice ? hi : s_lo + kSlice;
    const int64_t slice_len = (int64_t)(s_hi - s_lo);
    // the line at the slice's first byte: the last j with byte_off[j] <= s_lo (byte_off[n_lines] = total > s_lo)
    uint64_t j0 = 0;
    {
        uint64_t b = n_lines;
        while (b - j0 > 1) {
            const uint64_t mid = j0 + (b - j0) / 2;
            if (byte_off[mid] <= s_lo) j0 = mid;
            else b = mid;
        }
    }
    // lines j0 + t, j0 + 256 + t, ... as far as they begin inside the slice (a line has 19 bytes at least)
    for (uint64_t j = j0 + t; j < n_lines; j += kBlock) {
        const uint64_t line_abs = byte_off[j];
        if (line_abs >= s_hi) break;
        const sx_pair_line D = lines[j];
        PairHit P;
        if (!pair_hit(A, D.hit, P)) continue; // (the layout refused it)
        const uint32_t cig_len = cigar_render(cig + t * kCigarMax, kCigarMax, P.seq_l, P.gaps, P.n_gaps);
        int64_t off = (int64_t)line_abs - (int64_t)s_lo;
        put_bytes(obuf, off, slice_len, A.names + P.name_b, P.name_l);
        put_bytes(obuf, off, slice_len, (const uint8_t *)"\t", 1);
        put_dec_clipped(obuf, off, slice_len, D.flag);
        put_bytes(obuf, off, slice_len, (const uint8_t *)"\t", 1);
        put_bytes(obuf, off, slice_len, A.rnames + P.rn_b, P.rn_l);
        put_bytes(obuf, off, slice_len, (const uint8_t *)"\t", 1);
        put_dec_clipped(obuf, off, slice_len, D.pos);
        put_bytes(obuf, off, slice_len, (const uint8_t *)"\t0\t", 3);
        put_bytes(obuf, off, slice_len, cig + t * kCigarMax, cig_len);
        put_bytes(obuf, off, slice_len, (const uint8_t *)"\t=\t", 3);
        put_dec_clipped(obuf, off, slice_len, D.pnext);
        put_bytes(obuf, off, slice_len, (const uint8_t *)"\t-", D.tlen < 0 ? 2 : 1);
        put_dec_clipped(obuf, off, slice_len, tlen_magnitude(D.tlen));
        put_bytes(obuf, off, slice_len, (const uint8_t *)"\t", 1);
        put_bytes(obuf, off, slice_len, A.seqs + P.seq_b, P.seq_l);
        put_bytes(obuf, off, slice_len, (const uint8_t *)"\t", 1);
        put_bytes(obuf, off, slice_len, A.quals + P.qual_b, P.qual_l);
        put_bytes(obuf, off, slice_len, (const uint8_t *)"\n", 1);
    }
    __syncthreads();
    uint8_t *dst = out + (s_lo - lo);
    const uint32_t full = (uint32_t)(slice_len / 16);
    for (uint32_t k = t; k < full; k += kBlock) stream_store16((uint4 *)dst + k, obuf4[k]);
    const uint32_t tail = (uint32_t)slice_len - full * 16u;
    if (t < tail) dst[full * 16u + t] = obuf[full * 16u + t];
}

int sam_layout_pairs(sx_ctx *ctx, const SamArgs &A, const sx_pair_line *d_lines, uint64_t n_lines, uint64_t *d_byte_off, uint64_t *total_out)
{
    *total_out = 0;
    SX_TRY(sx_slab_ensure(ctx, SX_SLAB_SORT, 4096));
    uint32_t *d_err = (uint32_t *)ctx->slab[SX_SLAB_SORT].p;
    SX_CHECK(hipMemsetAsync(d_err, 0, 16, ctx->stream));
    if (n_lines) // (a descriptor in, a size out, 32 bytes of its hit and the offsets of its read)
        sx_launch(ctx, SX_KC_PAIR_LAYOUT, n_lines * 76, sam_pair_size_kernel, dim3(sx_div_up(n_lines, kBlock)), dim3(kBlock), A, d_lines, n_lines,
                  d_byte_off, d_err);
    SX_TRY(device_scan64_inplace(ctx, d_byte_off, n_lines, SX_KC_PAIR_LAYOUT));
    uint32_t h[2] = {0, 0}, e = 0;
    SX_TRY(sx_readback(ctx, (const uint32_t *)(d_byte_off + n_lines), 2, h));
    SX_TRY(sx_readback(ctx, d_err, 1, &e));
    if (e) return sx_fail_msg(ctx, SX_E_ARG, "SAM text: a line descriptor's hit, or that hit's query or offsets, lie outside the batch");
    *total_out = (uint64_t)h[0] | ((uint64_t)h[1] << 32);
    return 0;
}

// (asynchronous: the caller syncs)
int sam_emit_pairs(sx_ctx *ctx, const SamArgs &A, const sx_pair_line *d_lines, uint64_t n_lines, const uint64_t *d_byte_off, uint64_t lo,
                   uint64_t hi, uint8_t *d_out)
{
    if (hi <= lo) return 0;
    const uint64_t slices = (hi - lo + kSlice - 1) / kSlice;
    if (slices > 0x7FFFFFFFull) return sx_fail_msg(ctx, SX_E_ARG, "SAM text: window too long");
    sx_launch(ctx, SX_KC_PAIR_EMIT, hi - lo, sam_pair_emit_kernel, dim3((uint32_t)slices), dim3(kBlock), A, d_lines, n_lines, d_byte_off, lo, hi,
              d_out);
    return 0;
}

// what the kernels get of a batch (SamArgs has sx_sam_batch's fields in its order)
static SamArgs sam_args_of(const sx_sam_batch &b)
{
    return SamArgs{(const uint4 *)b.d_hits, b.n_hits,     b.d_sa,       b.sa_len,     b.d_sa_list, b.d_sa_len_list, b.d_names,   b.d_seqs,
                   b.d_quals,               b.d_name_off, b.d_seq_off,  b.d_qual_off, b.n_reads,   b.d_rnames,      b.d_rname_off, b.n_records,
                   nullptr,                 nullptr,      0,            nullptr};
}

static int sam_args(sx_ctx *ctx, const sx_sam_batch *b, SamTagArgs &A)
{
    if (!ctx || !b) return SX_E_ARG;
    if (b->n_hits && (!b->d_hits || ((uintptr_t)b->d_hits & 15) || !(b->d_sa || (b->d_sa_list && b->d_sa_len_list))))
        return sx_fail_msg(ctx, SX_E_ARG, "SAM text: hits (16-byte aligned) and a suffix array are needed");
    if (!b->d_name_off || !b->d_seq_off || !b->d_qual_off || !b->d_rname_off || b->n_records == 0 ||
        (uint64_t)b->n_reads * b->n_records > 0xFFFFFFFFull)
        return sx_fail_msg(ctx, SX_E_ARG, "SAM text: offsets of the reads and record names; reads x records below 2^32");
    static_cast<SamArgs &>(A) = sam_args_of(*b);
    return 0;
}

// the same of a batch that may bring a FLAG per read
static int sam_args_ex(sx_ctx *ctx, const sx_sam_batch_ex *b, SamTagArgs &A)
{
    if (!b) return SX_E_ARG;
    SX_TRY(sam_args(ctx, &b->batch, A));
    if ((uintptr_t)b->d_read_flags & 1) return sx_fail_msg(ctx, SX_E_ARG, "SAM text: the reads' flags are 16-bit entries");
    A.flags = b->d_read_flags;
    return 0;
}

// the same of a batch whose lines carry NM and MD; its positions may have been located beforehand
static int sam_args_tags(sx_ctx *ctx, const sx_sam_batch_tags *b, SamTagArgs &A)
{
    if (!b) return SX_E_ARG;
    SX_TRY(sam_args_ex(ctx, &b->ex, A));
    if (!b->d_text_list || !b->d_letters || ((uintptr_t)b->d_text_list & 7))
        return sx_fail_msg(ctx, SX_E_ARG, "SAM text: NM and MD need every record's text and its table of letters");
    if ((b->d_positions != nullptr) != (b->d_pos_off != nullptr) || ((uintptr_t)b->d_positions & 3) || ((uintptr_t)b->d_pos_off & 7))
        return sx_fail_msg(ctx, SX_E_ARG, "SAM text: located positions come with their offsets");
    A.text_list = b->d_text_list, A.letters = b->d_letters;
    A.positions = b->d_positions, A.pos_off = b->d_pos_off, A.pos_base = b->pos_base;
    return 0;
}

// the forms of the two kernels: positions located beforehand or read from a suffix array, a FLAG per read or none, each of
// the four with NM and MD behind QUAL (T), and each of the eight with placeholders (U)
#define SX_SAM_KERNEL_T(kernel, A, T, U) \
    ((A).positions ? ((A).flags ? kernel<true, true, T, U> : kernel<true, false, T, U>) : ((A).flags ? kernel<false, true, T, U> : kernel<false, false, T, U>))

// the kMapq forms: positions located beforehand or not, tags or not; the FLAG array and the placeholders are run-time matters
#define SX_SAM_KERNEL_Q(kernel, Q) \
    ((Q).positions ? ((Q).text_list ? kernel<true, true, true, true, true> : kernel<true, true, false, true, true>) \
                   : ((Q).text_list ? kernel<false, true, true, true, true> : kernel<false, true, false, true, true>))

static SamMapqArgs mapq_args_of(const SamTagArgs &A, const uint16_t *quality)
{
    SamMapqArgs Q;
    static_cast<SamTagArgs &>(Q) = A;
    Q.quality = quality;
    return Q;
}

int sam_layout(sx_ctx *ctx, const SamTagArgs &A, uint64_t *d_byte_off, uint64_t *total_out, bool unmapped, const uint16_t *quality)
{
    *total_out = 0;
    SX_TRY(sx_slab_ensure(ctx, SX_SLAB_SORT, 4096));
    uint32_t *d_err = (uint32_t *)ctx->slab[SX_SLAB_SORT].p;
    SX_CHECK(hipMemsetAsync(d_err, 0, 16, ctx->stream));
    if (A.n_hits && quality) // (SX_MAP_MAPQ: kernels of their own again; 2 bytes more a hit)
        sx_launch(ctx, SX_KC_SAM, A.n_hits * 42, SX_SAM_KERNEL_Q(sam_size_kernel, A), dim3(sx_div_up(A.n_hits, kBlock)), dim3(kBlock),
                  mapq_args_of(A, quality), d_byte_off, d_err);
    else if (A.n_hits && unmapped && A.text_list) // (SX_MAP_UNMAPPED: the same passes in kernels of their own)
        sx_launch(ctx, SX_KC_SAM, A.n_hits * 40, SX_SAM_KERNEL_T(sam_size_kernel, A, true, true), dim3(sx_div_up(A.n_hits, kBlock)),
                  dim3(kBlock), A, d_byte_off, d_err);
    else if (A.n_hits && unmapped)
        sx_launch(ctx, SX_KC_SAM, A.n_hits * 40, SX_SAM_KERNEL_T(sam_size_kernel, A, false, true), dim3(sx_div_up(A.n_hits, kBlock)),
                  dim3(kBlock), static_cast<const SamArgs &>(A), d_byte_off, d_err);
    else if (A.n_hits && A.text_list) // (a text window of about a read's length a hit beside its 32 bytes)
        sx_launch(ctx, SX_KC_SAM, A.n_hits * 40, SX_SAM_KERNEL_T(sam_size_kernel, A, true, false), dim3(sx_div_up(A.n_hits, kBlock)),
                  dim3(kBlock), A, d_byte_off, d_err);
    else if (A.n_hits)
        sx_launch(ctx, SX_KC_SAM, A.n_hits * 40, SX_SAM_KERNEL_T(sam_size_kernel, A, false, false), dim3(sx_div_up(A.n_hits, kBlock)),
                  dim3(kBlock), static_cast<const SamArgs &>(A), d_byte_off, d_err);
    SX_TRY(device_scan64_inplace(ctx, d_byte_off, A.n_hits, SX_KC_SAM));
    uint32_t h[2] = {0, 0}, e = 0;
    SX_TRY(sx_readback(ctx, (const uint32_t *)(d_byte_off + A.n_hits), 2, h));
    SX_TRY(sx_readback(ctx, d_err, 1, &e));
    if (e && A.text_list)
        return sx_fail_msg(ctx, SX_E_ARG, "SAM text: a hit's query, interval, offsets or text window lie outside the batch, or it has more than 8 differences");
    if (e) return sx_fail_msg(ctx, SX_E_ARG, "SAM text: a hit's query, interval or offsets lie outside the batch");
    *total_out = (uint64_t)h[0] | ((uint64_t)h[1] << 32);
    return 0;
}

// (asynchronous: the caller syncs)
int sam_emit(sx_ctx *ctx, const SamTagArgs &A, const uint64_t *d_byte_off, uint64_t lo, uint64_t hi, uint8_t *d_out, bool unmapped, const uint16_t *quality)
{
    if (hi <= lo) return 0;
    const uint64_t slices = (hi - lo + kSlice - 1) / kSlice;
    if (slices > 0x7FFFFFFFull) return sx_fail_msg(ctx, SX_E_ARG, "SAM text: window too long");
    // per line: its bytes out, 4 bytes of position in; the read's fields once a slice
    if (quality)
        sx_launch(ctx, SX_KC_SAM, hi - lo, SX_SAM_KERNEL_Q(sam_emit_kernel, A), dim3((uint32_t)slices), dim3(kBlock), mapq_args_of(A, quality),
                  d_byte_off, lo, hi, d_out);
    else if (unmapped && A.text_list)
        sx_launch(ctx, SX_KC_SAM, hi - lo, SX_SAM_KERNEL_T(sam_emit_kernel, A, true, true), dim3((uint32_t)slices), dim3(kBlock), A,
                  d_byte_off, lo, hi, d_out);
    else if (unmapped)
        sx_launch(ctx, SX_KC_SAM, hi - lo, SX_SAM_KERNEL_T(sam_emit_kernel, A, false, true), dim3((uint32_t)slices), dim3(kBlock),
                  static_cast<const SamArgs &>(A), d_byte_off, lo, hi, d_out);
    else if (A.text_list)
        sx_launch(ctx, SX_KC_SAM, hi - lo, SX_SAM_KERNEL_T(sam_emit_kernel, A, true, false), dim3((uint32_t)slices), dim3(kBlock), A,
                  d_byte_off, lo, hi, d_out);
    else
        sx_launch(ctx, SX_KC_SAM, hi - lo, SX_SAM_KERNEL_T(sam_emit_kernel, A, false, false), dim3((uint32_t)slices), dim3(kBlock),
                  static_cast<const SamArgs &>(A), d_byte_off, lo, hi, d_out);
    return 0;
}

} // namespace sx

using namespace sx;

extern "C" {

int sx_sam_layout_dev_ex(sx_ctx *ctx, const sx_sam_batch_ex *batch, uint64_t *d_byte_offsets, uint64_t *total_bytes_out)
{
    SamTagArgs A;
    SX_TRY(sam_args_ex(ctx, batch, A));
    if (!d_byte_offsets || !total_bytes_out) return SX_E_ARG;
    SX_CHECK(hipSetDevice(ctx->device));
    return sam_layout(ctx, A, d_byte_offsets, total_bytes_out);
}

int sx_sam_emit_dev_ex(sx_ctx *ctx, const sx_sam_batch_ex *batch, const uint64_t *d_byte_offsets, uint64_t total_bytes, uint64_t byte_lo,
                       uint64_t byte_hi, uint8_t *d_out)
{
    SamTagArgs A;
    SX_TRY(sam_args_ex(ctx, batch, A));
    if (!d_byte_offsets || byte_lo > byte_hi || byte_hi > total_bytes || (A.n_hits == 0 && byte_hi > byte_lo) || (byte_hi > byte_lo && (!d_out || ((uintptr_t)d_out & 15))))
        return sx_fail_msg(ctx, SX_E_ARG, "SAM text: a window inside [0, total) and a 16-byte aligned buffer are needed");
    SX_CHECK(hipSetDevice(ctx->device));
    SX_TRY(sam_emit(ctx, A, d_byte_offsets, byte_lo, byte_hi, d_out));
    return sx_sync(ctx);
}

int sx_sam_layout_dev_tags(sx_ctx *ctx, const sx_sam_batch_tags *batch, uint64_t *d_byte_offsets, uint64_t *total_bytes_out)
{
    SamTagArgs A;
    SX_TRY(sam_args_tags(ctx, batch, A));
    if (!d_byte_offsets || !total_bytes_out) return SX_E_ARG;
    SX_CHECK(hipSetDevice(ctx->device));
    return sam_layout(ctx, A, d_byte_offsets, total_bytes_out);
}

int sx_sam_emit_dev_tags(sx_ctx *ctx, const sx_sam_batch_tags *batch, const uint64_t *d_byte_offsets, uint64_t total_bytes, uint64_t byte_lo,
                         uint64_t byte_hi, uint8_t *d_out)
{
    SamTagArgs A;
    SX_TRY(sam_args_tags(ctx, batch, A));
    if (!d_byte_offsets || byte_lo > byte_hi || byte_hi > total_bytes || (A.n_hits == 0 && byte_hi > byte_lo) || (byte_hi > byte_lo && (!d_out || ((uintptr_t)d_out & 15))))
        return sx_fail_msg(ctx, SX_E_ARG, "SAM text: a window inside [0, total) and a 16-byte aligned buffer are needed");
    SX_CHECK(hipSetDevice(ctx->device));
    SX_TRY(sam_emit(ctx, A, d_byte_offsets, byte_lo, byte_hi, d_out));
    return sx_sync(ctx);
}

// a batch whose placeholders print FLAG 4 lines: the fields of sx_sam_batch_tags, the texts and letters optional (both or
// neither: with them the mapped lines carry NM and MD)
static int sam_args_unmapped(sx_ctx *ctx, const sx_sam_batch_tags *b, SamTagArgs &A)
{
    if (!b) return SX_E_ARG;
    if (b->d_text_list || b->d_letters) return sam_args_tags(ctx, b, A);
    SX_TRY(sam_args_ex(ctx, &b->ex, A));
    if ((b->d_positions != nullptr) != (b->d_pos_off != nullptr) || ((uintptr_t)b->d_positions & 3) || ((uintptr_t)b->d_pos_off & 7))
        return sx_fail_msg(ctx, SX_E_ARG, "SAM text: located positions come with their offsets");
    A.positions = b->d_positions, A.pos_off = b->d_pos_off, A.pos_base = b->pos_base;
    return 0;
}

int sx_sam_layout_dev_unmapped(sx_ctx *ctx, const sx_sam_batch_tags *batch, uint64_t *d_byte_offsets, uint64_t *total_bytes_out)
{
    SamTagArgs A;
    SX_TRY(sam_args_unmapped(ctx, batch, A));
    if (!d_byte_offsets || !total_bytes_out) return SX_E_ARG;
    SX_CHECK(hipSetDevice(ctx->device));
    return sam_layout(ctx, A, d_byte_offsets, total_bytes_out, true);
}

int sx_sam_emit_dev_unmapped(sx_ctx *ctx, const sx_sam_batch_tags *batch, const uint64_t *d_byte_offsets, uint64_t total_bytes, uint64_t byte_lo,
                             uint64_t byte_hi, uint8_t *d_out)
{
    SamTagArgs A;
    SX_TRY(sam_args_unmapped(ctx, batch, A));
    if (!d_byte_offsets || byte_lo > byte_hi || byte_hi > total_bytes || (A.n_hits == 0 && byte_hi > byte_lo) || (byte_hi > byte_lo && (!d_out || ((uintptr_t)d_out & 15))))
        return sx_fail_msg(ctx, SX_E_ARG, "SAM text: a window inside [0, total) and a 16-byte aligned buffer are needed");
    SX_CHECK(hipSetDevice(ctx->device));
    SX_TRY(sam_emit(ctx, A, d_byte_offsets, byte_lo, byte_hi, d_out, true));
    return sx_sync(ctx);
}

// The emitter of SX_MAP_MAPQ over hits that the caller made up: the batch of sx_sam_layout_dev_unmapped and a quality word a hit
static int sam_args_mapq(sx_ctx *ctx, const sx_sam_batch_mapq *b, SamTagArgs &A)
{
    if (!b) return SX_E_ARG;
    SX_TRY(sam_args_unmapped(ctx, &b->tags, A));
    if (!b->d_hit_quality || ((uintptr_t)b->d_hit_quality & 1)) return sx_fail_msg(ctx, SX_E_ARG, "SAM text: MAPQ needs a 16-bit quality word a hit");
    return 0;
}

int sx_sam_layout_dev_mapq(sx_ctx *ctx, const sx_sam_batch_mapq *batch, uint64_t *d_byte_offsets, uint64_t *total_bytes_out)
{
    SamTagArgs A;
    SX_TRY(sam_args_mapq(ctx, batch, A));
    if (!d_byte_offsets || !total_bytes_out) return SX_E_ARG;
    SX_CHECK(hipSetDevice(ctx->device));
    return sam_layout(ctx, A, d_byte_offsets, total_bytes_out, true, batch->d_hit_quality);
}

int sx_sam_emit_dev_mapq(sx_ctx *ctx, const sx_sam_batch_mapq *batch, const uint64_t *d_byte_offsets, uint64_t total_bytes, uint64_t byte_lo,
                         uint64_t byte_hi, uint8_t *d_out)
{
    SamTagArgs A;
    SX_TRY(sam_args_mapq(ctx, batch, A));
    if (!d_byte_offsets || byte_lo > byte_hi || byte_hi > total_bytes || (A.n_hits == 0 && byte_hi > byte_lo) || (byte_hi > byte_lo && (!d_out || ((uintptr_t)d_out & 15))))
        return sx_fail_msg(ctx, SX_E_ARG, "SAM text: a window inside [0, total) and a 16-byte aligned buffer are needed");
    SX_CHECK(hipSetDevice(ctx->device));
    SX_TRY(sam_emit(ctx, A, d_byte_offsets, byte_lo, byte_hi, d_out, true, batch->d_hit_quality));
    return sx_sync(ctx);
}

// a batch for line descriptors: hits, reads and records; no suffix array is asked for
static int sam_args_pairs(sx_ctx *ctx, const sx_sam_batch *b, const sx_pair_line *d_lines, uint64_t n_lines, SamArgs &A)
{
    if (!ctx || !b) return SX_E_ARG;
    if (n_lines && (!d_lines || ((uintptr_t)d_lines & 3) || !b->d_hits || ((uintptr_t)b->d_hits & 15)))
        return sx_fail_msg(ctx, SX_E_ARG, "SAM text: line descriptors (4-byte aligned) and hits (16-byte aligned) are needed");
    if (!b->d_name_off || !b->d_seq_off || !b->d_qual_off || !b->d_rname_off || b->n_records == 0 ||
        (uint64_t)b->n_reads * b->n_records > 0xFFFFFFFFull)
        return sx_fail_msg(ctx, SX_E_ARG, "SAM text: offsets of the reads and record names; reads x records below 2^32");
    A = sam_args_of(*b);
    return 0;
}

int sx_sam_layout_dev_pairs(sx_ctx *ctx, const sx_sam_batch *batch, const sx_pair_line *d_lines, uint64_t n_lines, uint64_t *d_byte_offsets,
                            uint64_t *total_bytes_out)
{
    SamArgs A;
    SX_TRY(sam_args_pairs(ctx, batch, d_lines, n_lines, A));
    if (!d_byte_offsets || !total_bytes_out) return SX_E_ARG;
    SX_CHECK(hipSetDevice(ctx->device));
    return sam_layout_pairs(ctx, A, d_lines, n_lines, d_byte_offsets, total_bytes_out);
}

int sx_sam_emit_dev_pairs(sx_ctx *ctx, const sx_sam_batch *batch, const sx_pair_line *d_lines, uint64_t n_lines, const uint64_t *d_byte_offsets,
                          uint64_t total_bytes, uint64_t byte_lo, uint64_t byte_hi, uint8_t *d_out)
{
    SamArgs A;
    SX_TRY(sam_args_pairs(ctx, batch, d_lines, n_lines, A));
    if (!d_byte_offsets || byte_lo > byte_hi || byte_hi > total_bytes || (n_lines == 0 && byte_hi > byte_lo) || (byte_hi > byte_lo && (!d_out || ((uintptr_t)d_out & 15))))
        return sx_fail_msg(ctx, SX_E_ARG, "SAM text: a window inside [0, total) and a 16-byte aligned buffer are needed");
    SX_CHECK(hipSetDevice(ctx->device));
    SX_TRY(sam_emit_pairs(ctx, A, d_lines, n_lines, d_byte_offsets, byte_lo, byte_hi, d_out));
    return sx_sync(ctx);
}

int sx_sam_layout_dev(sx_ctx *ctx, const sx_sam_batch *batch, uint64_t *d_byte_offsets, uint64_t *total_bytes_out)
{
    if (!batch) return SX_E_ARG;
    const sx_sam_batch_ex ex = {*batch, nullptr};
    return sx_sam_layout_dev_ex(ctx, &ex, d_byte_offsets, total_bytes_out);
}

int sx_sam_emit_dev(sx_ctx *ctx, const sx_sam_batch *batch, const uint64_t *d_byte_offsets, uint64_t total_bytes, uint64_t byte_lo,
                    uint64_t byte_hi, uint8_t *d_out)
{
    if (!batch) return SX_E_ARG;
    const sx_sam_batch_ex ex = {*batch, nullptr};
    return sx_sam_emit_dev_ex(ctx, &ex, d_byte_offsets, total_bytes, byte_lo, byte_hi, d_out);
}

} // extern "C"
