// reuse_main.cpp -- one context through calls of changing size, a scribble over its workspace, the look-back epoch's
// wrap and a trim, by the C API alone (include/stralg_amd.h).  A stand-alone program: tests/test_reuse_cpu.py links it with
// the CPU execution harness's objects, everything compiled with -fsanitize=address,undefined, and runs it; a slab freed
// under a running call, or an index past a slab's end, is the sanitizer's report.  It checks what it computes by brute
// force (neighbouring suffixes compared, occurrences counted) and exits non-zero on any mismatch.  TEST INFRASTRUCTURE ONLY.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "stralg_amd.h"

static sx_ctx *g_ctx = nullptr;

#define MUST(expr)                                                                                                     \
    do {                                                                                                               \
        int rc_ = (expr);                                                                                              \
        if (rc_ != 0) {                                                                                                \
            fprintf(stderr, "%s:%d: %s -> %d (%s)\n", __FILE__, __LINE__, #expr, rc_, sx_last_error(g_ctx));           \
            exit(2);                                                                                                   \
        }                                                                                                              \
    } while (0)

#define CHECK(cond, what)                                                                                              \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, what, #cond);                                       \
            exit(1);                                                                                                   \
        }                                                                                                              \
    } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t below)
{
    g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
    return (uint32_t)((g_rng >> 33) % below);
}

static std::vector<uint8_t> text_of(size_t n, uint32_t sigma)
{
    std::vector<uint8_t> x(n + 1, 0); // (the terminator behind it, for the comparisons below)
    for (size_t i = 0; i < n; ++i) x[i] = (uint8_t)(1 + rnd(sigma - 1));
    if (n > 400) memcpy(&x[n / 2], &x[10], n / 8); // a duplication: long common prefixes
    return x;
}

// suffix a < suffix b of x[0 .. n] (x[n] = 0, smaller than every symbol)
static bool suffix_less(const std::vector<uint8_t> &x, uint32_t a, uint32_t b)
{
    const size_t n = x.size() - 1;
    while (a <= n && b <= n && x[a] == x[b]) ++a, ++b;
    return x[a] < x[b];
}

static void check_sa(const std::vector<uint8_t> &x, const std::vector<uint32_t> &sa, const char *what)
{
    const size_t N = x.size();
    std::vector<uint8_t> seen(N, 0);
    for (size_t i = 0; i < N; ++i) {
        CHECK(sa[i] < N && !seen[sa[i]], what);
        seen[sa[i]] = 1;
        if (i) CHECK(suffix_less(x, sa[i - 1], sa[i]), what);
    }
}

static std::vector<uint32_t> build(uint32_t sigma, size_t n, const char *what, std::vector<uint8_t> *text_out = nullptr)
{
    std::vector<uint8_t> x = text_of(n, sigma);
    std::vector<uint32_t> sa(n + 1, 0xDDDDDDDDu);
    MUST(sx_sa_build(g_ctx, x.data(), n, sigma, sa.data()));
    check_sa(x, sa, what);
    if (text_out) *text_out = x;
    return sa;
}

static void lcp(size_t N, const char *what)
{
    std::vector<uint8_t> x;
    g_rng += N;
    std::vector<uint32_t> sa = build(5, N - 1, what, &x), inv(N, 0xDDDDDDDDu), l(N, 0xDDDDDDDDu);
    MUST(sx_sa_lcp_dev(g_ctx, x.data(), sa.data(), N, inv.data(), l.data())); // (the harness's device memory is the host's)
    CHECK(l[0] == 0, what);
    for (size_t j = 0; j < N; ++j) {
        CHECK(inv[sa[j]] == j, what);
        if (!j) continue;
        uint32_t a = sa[j - 1], b = sa[j], k = 0;
        while (a + k < N - 1 && b + k < N - 1 && x[a + k] == x[b + k]) ++k;
        CHECK(l[j] == k, what);
    }
}

static void search(const char *what)
{
    const uint32_t sigma = 5, n = 1200, count = 300, m = 9; // (more patterns than the harness's 256 lanes)
    std::vector<uint8_t> x = text_of(n, sigma);
    std::vector<uint32_t> sa(n + 1), c(sigma), o((size_t)(n + 2) * sigma);
    MUST(sx_build_tables(g_ctx, x.data(), n, sigma, sa.data(), c.data(), o.data()));
    check_sa(x, sa, what);
    std::vector<uint8_t> pat((size_t)count * m + 16, 0);
    std::vector<uint32_t> off(count + 1);
    for (uint32_t q = 0; q <= count; ++q) off[q] = q * m;
    for (uint32_t q = 0; q < count; ++q) memcpy(&pat[(size_t)q * m], &x[rnd(n - m)], m);
    for (int k = 0; k <= 1; ++k) {
        std::vector<uint64_t> ho(count + 1, ~0ull), ho2(count + 1, ~0ull);
        uint64_t total = 0, again = 0;
        MUST(sx_bwt_approx_search_dev(g_ctx, c.data(), o.data(), nullptr, n + 1, sigma, pat.data(), off.data(), count, k, ho.data(), nullptr, 0, &total));
        CHECK(total >= count && ho[0] == 0 && ho[count] == total, what);
        std::vector<sx_approx_hit> hits(total);
        MUST(sx_bwt_approx_search_dev(g_ctx, c.data(), o.data(), nullptr, n + 1, sigma, pat.data(), off.data(), count, k, ho2.data(), hits.data(), total, &again));
        CHECK(again == total && ho == ho2, what);
        for (uint32_t q = 0; q < count; ++q) {
            CHECK(ho[q] <= ho[q + 1], what);
            for (uint64_t h = ho[q]; h < ho[q + 1]; ++h) CHECK(hits[h].query == q && hits[h].L < hits[h].R && hits[h].R <= n + 1, what);
            if (k == 0) { // one interval: the pattern's occurrences, counted by brute force
                uint32_t occ = 0;
                for (uint32_t a = 0; a + m <= n; ++a) occ += memcmp(&x[a], &pat[(size_t)q * m], m) == 0;
                CHECK(ho[q + 1] - ho[q] == 1 && hits[ho[q]].R - hits[ho[q]].L == occ && hits[ho[q]].match_length == m, what);
                for (uint32_t r = hits[ho[q]].L; r < hits[ho[q]].R; ++r) CHECK(memcmp(&x[sa[r]], &pat[(size_t)q * m], m) == 0, what);
            }
        }
    }
}

static void epoch_is_sane(const char *what)
{
    sx_ctx_counts k;
    MUST(sx_ctx_counters(g_ctx, &k));
    CHECK(k.chain_slab_max_epoch <= k.chain_epoch && k.chain_epoch < (1u << 24), what);
    CHECK(k.child_chain_slab_max_epoch <= k.child_chain_epoch, what);
}

int main(void)
{
    MUST(sx_ctx_create(0, &g_ctx));
    MUST(sx_ctx_set_flag(g_ctx, SX_FLAG_SMALL_DIRECT_MAX, 0)); // (the SA-IS kernels, not the direct sort of short records)
    build(5, 3000, "small build");
    build(5, 70000, "large build"); // (the slabs proportional to n grow past their first MiB)
    epoch_is_sane("after the builds");
    MUST(sx_ctx_scribble(g_ctx, 0xFF));
    lcp(2999, "lcp, small");   // the plain inverse
    lcp(6337, "lcp, large");   // the three-pass inverse and Kasai's chunks (the harness's thresholds: 3000, 6000)
    lcp(2999, "lcp, small again");
    lcp(5000, "lcp by phi");
    MUST(sx_ctx_scribble(g_ctx, 0xA5));
    search("k-edit search");
    MUST(sx_ctx_set_flag(g_ctx, SX_FLAG_CHAIN_EPOCH, (1 << 24) - 2));
    MUST(sx_ctx_scribble(g_ctx, 0xFF));
    build(5, 9000, "build across the epoch's wrap");
    epoch_is_sane("after the wrap");
    build(12, 3000, "second build behind the wrap");
    sx_ctx_counts k;
    MUST(sx_ctx_counters(g_ctx, &k));
    CHECK(k.chain_epoch >= 1 && k.chain_epoch < 1000, "the epoch wrapped");
    sx_ctx_trim(g_ctx);
    MUST(sx_ctx_counters(g_ctx, &k));
    for (int i = 0; i < 7; ++i) CHECK(k.slab_bytes[i] == 0, "trim");
    build(5, 5000, "build after trim");
    epoch_is_sane("at the end");
    sx_ctx_destroy(g_ctx);
    printf("reuse ok\n");
    return 0;
}
