// The prefix-key sort's plan (stralg_amd/csrc/sx_prefix_plan.hpp) over a grid of text sizes, alphabets, symbol counts and
// switches, one line a case: what tests/test_prefix_plan.py compares with tests/golden/prefix_plans.txt.  No GPU, no
// launch: the plan is arithmetic.  Linked with the CPU harness library for sx_local_sort_applies and
// sx_sort_lms_keys_applies.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include "sx_prefix_plan.hpp"

using namespace sx;

struct text_kind {
    const char *name;
    uint32_t base;
    bool all_suffixes;
    double share[5]; // of the first symbols; all 0: equal counts of the base - 1 symbols
};

// symbol counts that add up to N - 1: the shares given, or equal ones; what rounding leaves goes to symbol 1
static void counts_of(const text_kind &k, uint64_t N, uint32_t h_all[256])
{
    memset(h_all, 0, 256 * sizeof(uint32_t));
    const uint64_t n = N - 1;
    const uint32_t syms = k.base - 1;
    uint64_t given = 0;
    for (uint32_t c = 1; c <= syms; ++c) {
        const uint64_t cnt = k.share[0] > 0.0 ? (uint64_t)(k.share[c - 1] * (double)n) : n / syms;
        h_all[c] = (uint32_t)cnt;
        given += cnt;
    }
    h_all[1] += (uint32_t)(n - given);
}

static void row(const char *label, const text_kind &k, uint64_t N, uint64_t m, int sort_mode, int prefix_symbols, int attempt, bool long_list)
{
    uint32_t h_all[256];
    counts_of(k, N, h_all);
    prefix_inputs in = {};
    in.N = N, in.m = k.all_suffixes ? N : m, in.maxc = k.base - 1, in.ntiles = sx_div_up(N, kClsTile), in.all_suffixes = k.all_suffixes;
    in.st = sx_symbol_stats_of(h_all, N);
    in.prefix_symbols = prefix_symbols, in.sort_mode = sort_mode, in.text_keys_off = false;
    in.long_list = long_list, in.ls_tiles = true, in.digit_bits = 8;
    const prefix_first f = prefix_first_length(in);
    // the second attempt: the longest key, nothing to take back
    const uint32_t C = attempt == 0 ? f.C : sx_prefix_cmax(k.base);
    const prefix_plan p = prefix_plan_for(in, C, f.one_more && attempt == 0);
    printf("%s %s N=%" PRIu64 " m=%" PRIu64 " mode=%d symbols=%d attempt=%d long_list=%d :", label, k.name, N, in.m, sort_mode, prefix_symbols,
           attempt, (int)long_list);
    printf(" first=%u one_more=%d C=%u took_back=%d lenbits=%u kbits=%d kbits_base=%d dense4=%d top_bits=%d", f.C, (int)f.one_more, p.C,
           (int)p.took_back, p.lenbits, p.kbits, p.kbits_base, (int)p.dense4, p.top_bits);
    printf(" B=%u CW=%u embed=%d embed_chars=%u kmask=%" PRIx64 " dig_shift=%u dig_mask=%x text_keyed=%d lms_keyed=%d lms_shape=%u longest=%u\n",
           p.wcfg.B, p.wcfg.CW, (int)p.embed, p.embed_chars, p.kmask, p.dig_shift, p.dig_mask, (int)p.text_keyed, (int)p.lms_keyed,
           p.lms_shape, p.longest_expected);
}

static void grid_row(const text_kind &k, uint64_t m, int sort_mode, int prefix_symbols, int attempt, bool long_list)
{
    // LMS sorts: N = ceil(3.43 m), at most 2^32; direct sorts: N = m
    uint64_t N = m;
    if (!k.all_suffixes) {
        N = (uint64_t)((double)m * 3.43) + 1;
        if (N > (1ull << 32)) N = 1ull << 32;
    }
    row("grid", k, N, m, sort_mode, prefix_symbols, attempt, long_list);
}

int main()
{
    const text_kind lms3 = {"lms3", 3, false, {0}}, lms5 = {"lms5", 5, false, {0}}, lms5a = {"lms5-55-25-15-5", 5, false, {0.55, 0.25, 0.15, 0.05}},
                    lms5b = {"lms5-30-20-20-30", 5, false, {0.3, 0.2, 0.2, 0.3}}, lms6 = {"lms6", 6, false, {0}},
                    lms6n = {"lms6-fifth-5", 6, false, {0.2375, 0.2375, 0.2375, 0.2375, 0.05}}, lms21 = {"lms21", 21, false, {0}},
                    lms256 = {"lms256", 256, false, {0}}, all5 = {"all5", 5, true, {0}}, all21 = {"all21", 21, true, {0}},
                    all256 = {"all256", 256, true, {0}};
    // the rows the project has recorded (profiles/r05_final_bench_*.json, build_stats): equal counts, the recorded n_lms as m
    const uint64_t G = 1ull << 30;
    row("dna-2^30", lms5, G + 1, 313178366, 0, 0, 0, true);
    row("dna-2^26", lms5, (1ull << 26) + 1, 19574071, 0, 0, 0, true);
    row("bytes-2^30-direct", all256, G + 1, 0, 0, 0, 0, true);
    row("bytes-2^30-induced", lms256, G + 1, 357204340, 0, 0, 0, true);
    row("sigma21-2^30-direct", all21, G + 1, 0, 0, 0, 0, true);
    row("sigma21-2^30-induced", lms21, G + 1, 348980281, 0, 0, 0, true);
    row("sigma6-2^30", lms6, G + 1, 322126801, 0, 0, 0, true);
    row("dna-2^22-direct", all5, (1ull << 22) + 1, 0, 0, 0, 0, true);

    const uint64_t ms[9] = {1ull << 20, (1ull << 22) - 1, 1ull << 22, 1ull << 24, 1ull << 26, 313178366, 1ull << 30, 1ull << 31, (1ull << 32) - 2};
    const text_kind *kinds[11] = {&lms3, &lms5, &lms5a, &lms5b, &lms6, &lms6n, &lms21, &lms256, &all5, &all21, &all256};
    // the default mode, both attempts, every size
    for (const text_kind *k : kinds)
        for (uint64_t m : ms)
            for (int attempt = 0; attempt < 2; ++attempt) grid_row(*k, m, 0, 0, attempt, true);
    // without the list of long sub-buckets: read by the dense keys' choice in the default mode only
    for (const text_kind *k : {&lms5, &lms5a, &lms5b})
        for (uint64_t m : ms)
            for (int attempt = 0; attempt < (k == &lms5 ? 1 : 2); ++attempt) grid_row(*k, m, 0, 0, attempt, false);
    // the forced modes: plain passes, three HBM passes, four
    for (const text_kind *k : {&lms5, &lms5a, &lms6, &lms256, &all21, &all256})
        for (uint64_t m : {ms[0], ms[2], ms[4], ms[6], ms[8]})
            for (int mode = 1; mode <= 3; ++mode) grid_row(*k, m, mode, 0, 0, true);
    // a forced prefix length
    for (const text_kind *k : {&lms3, &lms5, &lms6n, &all5})
        for (uint64_t m : {ms[0], ms[3], ms[6]})
            for (int mode = 0; mode <= 1; ++mode) grid_row(*k, m, mode, 17, 0, true);
    return 0;
}
