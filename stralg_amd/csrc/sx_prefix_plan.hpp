// sx_prefix_plan.hpp -- what the prefix-key sort (sx_lmssort.hip) decides before an attempt's first launch: the prefix
// length, dense or base-b keys, whether and how the hybrid sort runs, what the keys embed for the induction, which key
// kernel runs or none.  Plain arithmetic on the text's size, its symbol counts and the context's switches: host only, no
// HIP runtime call, so that tests/test_prefix_plan.py checks it at the sizes where the decisions matter.
#pragma once
#include <math.h>

#include "sx_common.hpp"
#include "sx_internal.hpp"
#include "sx_window.hpp"
#include "sx_lmskey.hpp"

// ---- the text's symbol statistics: one walk over the counts of the symbols 1 .. 255 (N - 1 of them in all)
struct sx_symbol_stats {
    double sum_p2; // the chance that two positions hold the same symbol; 1 / sum_p2: the effective alphabet
    double pmax;   // share of the most frequent symbol
    uint32_t used; // symbols that occur
};
static inline sx_symbol_stats sx_symbol_stats_of(const uint32_t h_all[256], uint64_t N)
{
    sx_symbol_stats s = {0.0, 0.0, 0};
    const double n_sym = (double)N - 1.0;
    for (int c = 1; c < 256 && n_sym > 0; ++c) {
        if (!h_all[c]) continue;
        const double pc = (double)h_all[c] / n_sym;
        if (pc > s.pmax) s.pmax = pc;
        s.sum_p2 += pc * pc;
        ++s.used;
    }
    return s;
}

// longest prefix whose number fits 63 bits
static inline uint32_t sx_prefix_cmax(uint32_t base)
{
    uint32_t Cmax = 0;
    for (double cap63 = 9.2e18, v = 1.0; v * base <= cap63 && Cmax < 63; v *= base) ++Cmax;
    return Cmax < 1 ? 1 : Cmax;
}
// bits of the largest key of C symbols in base `base`, base^C - 1 (C <= sx_prefix_cmax(base)); at least 1
static inline int sx_prefix_key_bits(uint32_t base, uint32_t C)
{
    uint64_t top = 1;
    for (uint32_t i = 0; i < C; ++i) top *= base;
    return sx_bitlen(top - 1) > 0 ? sx_bitlen(top - 1) : 1;
}

namespace sx {

// top bits of the hybrid sort of dense keys that are tried first
constexpr int SX_DENSE4_TOP = 22; // (1 GiB of DNA, whole step: base-5 keys 23.30 ms; dense keys with 24 top bits 22.79, 22: 22.71, 21: 22.73, 20: 22.79)

// what the decisions read
struct prefix_inputs {
    uint64_t N, m;  // positions of the text; suffixes to sort (all_suffixes: N, else the LMS suffixes)
    uint32_t maxc;  // largest symbol present: keys are numbers in base maxc + 1
    uint32_t ntiles; // classification tiles
    bool all_suffixes;
    sx_symbol_stats st;
    int prefix_symbols, sort_mode; // SX_FLAG_PREFIX_SYMBOLS, SX_FLAG_SORT_MODE
    bool text_keys_off;            // SX_FLAG_TEXT_KEYS_OFF
    bool long_list;  // sub-buckets too long for a workgroup can be listed (SX_FLAG_LONG_SUBBUCKETS_OFF: not)
    bool ls_tiles;   // the local sort's tile arrays were obtained
    int digit_bits;  // of the radix passes (sx_sort_digit_bits)
};

// the first attempt's prefix length
struct prefix_first {
    uint32_t C;
    bool one_more; // the extra symbol of four-letter texts is in it (taken back if the hybrid sort does not follow)
};
static inline prefix_first prefix_first_length(const prefix_inputs &in)
{
    const uint64_t m = in.m;
    const uint32_t base = in.maxc + 1, Cmax = sx_prefix_cmax(base);
    // shortest prefix that tells ~97 % of m suffixes of a uniformly random text apart
    uint32_t C = 1;
    {
        // (the direct sort of all suffixes accepts twice the ties to stay within 40 key bits at 32, 128, ... symbols)
        const double eff = in.maxc > 2 ? (double)in.maxc : 2.0, target = (in.all_suffixes ? 16.0 : 32.0) * (double)m;
        double v = eff;
        while (v < target && C < Cmax) {
            v *= eff;
            ++C;
        }
        // Skewed symbol frequencies (a genome with 5 % N, a GC-poor one): two suffixes agree on a symbol with
        // probability sum p^2, not 1 / maxc.  A prefix that is too short costs a whole second sort with the longest
        // key; one symbol too many costs at most a pass.  So the prefix is also made long enough for <= ~6 % ties
        // under the text's own collision rate (uniform text: never the larger of the two; symbols that only occur
        // in long runs, like N, hardly enter the rate but do enter maxc: that case needs the margin).
        const double sum_p2 = in.st.sum_p2;
        if (sum_p2 > 0.0 && sum_p2 < 1.0) {
            const double eff_c = 1.0 / sum_p2, target_c = 16.0 * (double)m;
            uint32_t Cc = 1;
            for (double u = eff_c; u < target_c && Cc < Cmax; u *= eff_c) ++Cc;
            if (Cc > C) C = Cc;
        }
    }
    // Round 4: four-letter texts take one symbol more where the dense key still leaves at most 19 bits to the local sort
    // (2 C + length field <= 41).  The prefix above leaves ~1.8 % of uniformly random suffixes tied, one symbol more a
    // quarter of that, and the tied suffixes' refinement -- random reads of the text -- cost more than the symbol: same box,
    // 1 GiB 22.13 -> 21.13 ms (refinement 1.00 -> 0.28 ms, every other class unchanged), 256 MiB 6.36 -> 6.19; a symbol
    // less: 23.21.  Taken back by the plan if the text turns out not to take the hybrid sort (plain passes would pay a pass for it).
    bool one_more = false;
    if (!in.all_suffixes && base == 5 && in.prefix_symbols <= 0 && in.sort_mode != 1 && C + 1 <= Cmax &&
        2 * (C + 1) + (uint32_t)sx_bitlen(C + 1) <= 41) {
        ++C;
        one_more = true;
    }
    // (the direct sort of all suffixes likewise, while the key stays within 40 bits -- five 8-bit digits either way, at most
    //  16 bits for the local sort: 1 GiB of 20 symbols 58.5 -> 56.3 ms, ties refined in 0.19 instead of 2.7 ms; bytes stay at
    //  five symbols, six would be 48 bits)
    if (in.all_suffixes && in.prefix_symbols <= 0 && C + 1 <= Cmax) {
        double top = 1.0;
        for (uint32_t i = 0; i <= C; ++i) top *= (double)base;
        if (top <= 1099511627776.0) ++C; // base^(C+1) <= 2^40
    }
    if (in.prefix_symbols > 0) C = (uint32_t)in.prefix_symbols < Cmax ? (uint32_t)in.prefix_symbols : Cmax; // (tests)
    return {C, one_more};
}

// everything an attempt decides before its first launch
struct prefix_plan {
    uint32_t C;       // symbols of the key
    uint32_t lenbits; // length field of dense keys: that of the attempt's C as it came in -- the value stays when the extra
                      // symbol is taken back (the keys are not dense then)
    int kbits;        // sorted key bits
    int kbits_base;   // those of the base-b key of C symbols (dense keys: more than it needs)
    bool dense4;      // four symbols and the sentinel: dense keys of two bits a symbol and a length field (dense4_finish)
    int top_bits;     // of the hybrid sort; 0: plain passes over all key bits
    wnd_cfg wcfg;     // the windows the keys carry above bit kbits; CW = 0: none
    bool embed;
    uint32_t embed_chars; // symbols of the windows the keys carry (embed) for the induction
    uint64_t kmask;
    uint32_t dig_shift, dig_mask; // the first pass's digit of a key, left by the key kernels
    bool text_keyed, lms_keyed;   // the hybrid sort's first pass computes the keys itself: no key kernel
    uint32_t lms_shape;           // lms_key_shape of the static form of the LMS keys; 0: none
    uint32_t longest_expected;    // the longest sub-bucket the local sort is told to expect; 0: not known
    bool took_back;               // the extra symbol (prefix_first::one_more) was taken back: C is one less than asked for
    bool hybrid() const { return top_bits != 0; }
};

// The keys of C symbols in one form, dense (dense4) or base-b: their bits, the windows they carry, and the hybrid sort's
// top bits for them.
static inline void prefix_plan_keys(const prefix_inputs &in, uint32_t C, bool dense4, prefix_plan &p)
{
    const uint64_t m = in.m;
    const uint32_t base = in.maxc + 1;
    p.C = C;
    p.dense4 = dense4;
    p.kbits_base = sx_prefix_key_bits(base, C); // base^C - 1 is the largest key
    p.kbits = dense4 ? (int)(2 * C + p.lenbits) : p.kbits_base;
    if (p.kbits < 1) p.kbits = 1;
    const int kbits = p.kbits;
    const int kbits_wnd = kbits > p.kbits_base ? kbits : p.kbits_base; // (dense keys: the windows of the base-5 keys, for which the static kernels are built)
    // Symbol windows in the unsorted key bits, when at least four symbols fit.  Texts of more than 16 symbols, whose
    // induction windows are 64-bit words, take part since round 4: the sort hands the windows on as 32-bit words (the
    // same layout with fewer symbols: code fields of B bits above a 4-bit count), so up to 28 / B symbols, and from
    // two on they are worth it -- an LMS seed's first symbol is its entry's bucket, its second the symbol byte of
    // the entry it induces, and the text is read again where that entry is scanned.  (Without them every seed's
    // window was gathered from the text in suffix order before the L pass: 3.6 * 10^8 random 16-byte reads, 8.3 of
    // the 94 ms of 1 GiB of bytes through the induced-sort passes.)
    const bool wide = sx_window_cfg(in.maxc, p.wcfg);
    uint32_t wchars = 0;
    if (64 - kbits_wnd > kCntBits) wchars = (uint32_t)(64 - kbits_wnd - kCntBits) / p.wcfg.B;
    if (wchars > p.wcfg.CW) wchars = p.wcfg.CW;
    if (wide && wchars > (32u - (uint32_t)kCntBits) / p.wcfg.B) wchars = (32u - (uint32_t)kCntBits) / p.wcfg.B;
    p.embed = wide ? wchars >= 2 : wchars >= 4;
    p.embed_chars = p.embed ? wchars : 0;
    if (in.all_suffixes) {
        // no induction follows a direct sort; one symbol of window is the BWT symbol of the suffix, for free
        wchars = 64 - kbits >= (int)(kCntBits + p.wcfg.B) ? 1u : 0u;
        p.embed = wchars == 1;
    }
    p.wcfg.CW = p.embed ? wchars : 0;
    p.kmask = kbits >= 64 ? ~0ull : ((1ull << kbits) - 1ull);
    // Hybrid sort (sx_localsort.hip): only the top 24 key bits go through HBM passes, the sub-buckets they leave are
    // ordered in LDS.  It needs sub-buckets that fit a workgroup: a prefix of 24 / log2(base) symbols must not be too
    // frequent.  Judged here from the text's most frequent symbol (a run of it is the most frequent prefix of a text
    // without repeats); repeats show when the kernel finds a sub-bucket that does not fit, and LSD passes finish the job.
    p.top_bits = 0;
    if (in.sort_mode == 1 || in.digit_bits != 8 || !in.ls_tiles) return;
    // Sub-buckets the top bits leave: the low L = kbits - top bits span base^(L / log2 base) key values, so the
    // top bits tell apart prefixes of C - L / log2(base) symbols (A C G T in base 5, 17 symbols, L = 16: 10.1) -- and
    // a text has about (effective alphabet)^(that many) of those, the effective alphabet being 1 / sum p^2 (4,
    // not 5: a fifth of the key space per symbol is never used).  Also: the copies of the most frequent one.
    // Three passes (24 bits).  Four passes (32 bits) leave short sub-buckets in texts of 2 Gi symbols and more and
    // with skewed frequencies too (2 GiB of uniform DNA: 40.3 against 43.2 ms for six plain passes), but are only
    // taken when asked for (SX_FLAG_SORT_MODE 3): texts that long are genomes, their repeat families overflow a
    // workgroup whatever the symbol counts promise, and a failed attempt costs more than a good one saves
    // (the genome-like 1 GiB text: 58 instead of 44 ms).  (Four-letter texts with dense keys: see cand0 below -- their
    // sub-buckets' lengths are known, and 2 GiB ... 8 GiB of uniform DNA take the hybrid sort with 22 / 24 top bits.)
    const double pmax = in.st.pmax, eff = in.st.sum_p2 > 0.0 ? 1.0 / in.st.sum_p2 : 1.0;
    // Dense keys: a sub-bucket is a prefix of top_bits / 2 symbols, so its mean length (m / eff^symbols) and that of
    // the most frequent symbol's run (m * pmax^symbols) are known better than for base-b keys; LMS suffixes favour
    // some prefixes (the fullest sub-bucket of uniform text holds 3.6 times the mean, measured), so 4.5 times the
    // larger of the two, with half as much again for safety, has to fit the 1024 pairs between a span's end and the
    // reach.  Skewed symbol counts (a genome: 30 % A) give the run of the most frequent symbol many times the mean:
    // such texts have repeat families too, and are left to plain passes as before.  22 top bits where they do
    // (1 GiB ... 2 GiB of uniform DNA), else 24 (up to 8 GiB).
    int cand0 = dense4 ? SX_DENSE4_TOP : 24;
    bool dense_fits = false;
    if (dense4 && in.sort_mode == 0) {
        for (int tb = SX_DENSE4_TOP; tb <= 24 && !dense_fits; tb += 2) {
            const double sy = (double)tb / 2.0, mean_d = (double)m / pow(eff, sy), top_d = (double)m * pow(pmax, sy);
            if (top_d <= 1.5 * mean_d && 4.5 * top_d * 1.5 <= 1024.0 && sx_local_sort_applies(m, kbits, tb)) cand0 = tb, dense_fits = true;
        }
        // Round 4: skewed symbol counts and repeat families no longer rule the hybrid sort out -- the sub-buckets that
        // do not fit a workgroup are listed and ordered by HBM passes of their own (sx_long_subbuckets) --, so what
        // counts is the mean sub-bucket (the genome-like 1 GiB text: 115 pairs at 22 bits, 6 % of the pairs in long
        // sub-buckets): three HBM passes and the LDS step instead of five passes, a key kernel and the pass that marks
        // the ties.  (A text whose long sub-buckets hold a quarter of the pairs falls back as before.)
        for (int tb = SX_DENSE4_TOP; tb <= 24 && !dense_fits && in.long_list; tb += 2) {
            const double mean_d = (double)m / pow(eff, (double)tb / 2.0);
            if (mean_d <= 256.0 && sx_local_sort_applies(m, kbits, tb)) cand0 = tb, dense_fits = true;
        }
    }
    for (int ci = 0; ci < 2 && p.top_bits == 0; ++ci) {
        const int cand = ci == 0 ? cand0 : 32;
        if (!sx_local_sort_applies(m, kbits, cand)) continue;
        if (in.sort_mode >= 2) { // forced (tests): 2 three passes, 3 four
            if ((in.sort_mode == 2) == (ci == 0)) p.top_bits = cand;
            continue;
        }
        const double syms = (double)C - (double)(p.kbits_base - (ci == 0 ? 24 : 32)) / log2((double)base);
        const double mean_bucket = syms > 0.0 ? (double)m / pow(eff, syms) : (double)m;
        const double top_bucket = syms > 0.0 ? (double)m * pow(pmax, syms) : (double)m;
        if (ci == 0 && m >= (1u << 22) && (dense4 ? dense_fits : (mean_bucket <= 300.0 && top_bucket <= 400.0))) p.top_bits = cand; // (a workgroup owns the sub-buckets that start in its span and end within its reach: one that starts
                                                                                                                                   //  at the span's last pair may hold kLsCap - kLsSpan = 1024 pairs, one that starts earlier more)
    }
}

// The plan of an attempt with C symbols.  take_back: C holds the extra symbol (prefix_first::one_more, first attempt).
static inline prefix_plan prefix_plan_for(const prefix_inputs &in, uint32_t C, bool take_back)
{
    const uint64_t m = in.m;
    const uint32_t base = in.maxc + 1;
    prefix_plan p = {};
    // four symbols and the sentinel: dense keys of two bits a symbol and a length field (dense4_finish); the plain-passes
    // mode keeps the base-5 keys (tests run both)
    p.lenbits = (uint32_t)sx_bitlen(C);
    // (dense keys only with the hybrid sort: plain passes run faster on the base-5 keys' uneven digits -- the genome-like
    //  text 41.9 against 40.5 ms --, so the decisions are taken for the dense keys first and, if they end without
    //  the hybrid sort, once more for the base-5 keys)
    const bool dense4 = !in.all_suffixes && base == 5 && in.sort_mode != 1 && 2 * C + p.lenbits <= 60;
    prefix_plan_keys(in, C, dense4, p);
    if (dense4 && !p.hybrid()) {
        p.took_back = take_back; // (no hybrid sort after all: the shorter key, as before)
        prefix_plan_keys(in, take_back ? C - 1 : C, false, p);
    }
    const int kbits = p.kbits;
    p.dig_shift = p.hybrid() ? (uint32_t)(kbits - p.top_bits) : 0u;
    p.dig_mask = kbits - (int)p.dig_shift >= 8 ? 0xFFu : (1u << (kbits - (int)p.dig_shift)) - 1u;
    // The direct sort's keys are a function of the text alone, so where the hybrid sort applies its first HBM pass computes
    // them itself (sx_textkey, sx_radix.hip): no key kernel, and 8 bytes a suffix that are neither written nor read back
    // (1 GiB of bytes: 2.4 ms of key kernel and 7.5 GB of the first scatter's reads).  Switch for the A/B and the
    // tests: SX_FLAG_TEXT_KEYS_OFF keeps the key kernel.
    p.text_keyed = in.all_suffixes && p.C <= 12 && p.hybrid() && in.digit_bits == 8 && !in.text_keys_off;
    // The LMS sort of a four-letter text likewise (sx_lmskey, round 4): the hybrid sort's first pass lists the LMS
    // suffixes of its piece of the text and computes their dense keys itself -- no key kernel, and 13 bytes an LMS suffix
    // (key, position, first digit) that are neither written nor read back.  Same switch.
    const pkey_cfg lms_kc = pkey_make(p.dense4 ? 4u : base, p.C);
    p.lms_shape = (!in.all_suffixes && lms_kc.dot && p.wcfg.B == 2 && p.wcfg.CW) ? lms_key_shape(p.C, p.wcfg.CW, 2) : 0u;
    p.lms_keyed = !in.all_suffixes && p.hybrid() && p.dense4 && in.digit_bits == 8 && !in.text_keys_off && p.lms_shape != 0 &&
                  sx_sort_lms_keys_applies(m, in.ntiles, p.lms_shape);
    // (dense keys: a sub-bucket is a prefix of top_bits / 2 symbols; LMS suffixes favour some prefixes -- two thirds of
    //  them begin with the smallest symbol -- so the fullest sub-bucket of uniform text holds 3.6 times the mean: 4.5 times
    //  the most frequent symbol's share to that power, for the local sort's choice of its span)
    p.longest_expected = 0;
    if (p.hybrid() && (p.dense4 || in.all_suffixes) && in.sort_mode == 0) {
        // (all suffixes of a wide alphabet, the direct sort: no favoured prefixes, a sub-bucket is a prefix of
        //  top_bits / log2(base) symbols -- three bytes at 256 symbols --: the most frequent symbol's run and what
        //  chance adds to the fullest of 2^24 sub-buckets)
        const double run = (double)m * pow(in.st.pmax, p.dense4 ? (double)p.top_bits / 2.0 : (double)p.top_bits / log2((double)base));
        const double est = p.dense4 ? 4.5 * run : 1.2 * run + 8.0 * sqrt(run) + 16.0;
        p.longest_expected = est < 1.0 ? 1u : (est > 1e9 ? 1000000000u : (uint32_t)est);
    }
    return p;
}

} // namespace sx
