// sx_approx.hip -- batched k-edit BWT search (stralg/bwt.c:226-422 init_bwt_approx_iter / next_bwt_approx_match).
//
// One lane searches one pattern at a time, depth first, in the reference's order: at a node the children are M over
// a = 1 .. sigma-1 (cost 0 where a is the pattern symbol), then I, then D over a = 1 .. sigma-1 (the root has no D);
// a node whose pattern is used up (i < 0) is a hit.  Two passes over the same search: the first counts every
// pattern's hits, a scan turns the counts into offsets, the second writes the hits at their pattern's offset -- the
// output depends on nothing but the pattern numbers, so it is the same from run to run however lanes pick up work.
//
// Design ("k-edit search"):
//  * Frames only where edits are left.  A node with no edit left has one child that can lead anywhere, the exact M,
//    so its whole subtree is the exact backward search of the rest of the pattern: the lane walks it in a loop of
//    its own (the "chain") and pushes nothing.  A node with edits left is pushed as one 16-byte frame {L, R, next
//    child | edits_left, i | match_length}; nodes with edits left form a prefix of the path, so frame d is the node
//    at search depth d, and a path holds at most m + k - 1 of them.  Frames live in a workspace in device memory,
//    frame d of lane t at stack[d * lanes + t] (a per-lane array indexed at run time would go to scratch anyway).
//  * The edit string is never stored: matches and mismatches are both 'M' in the reference's CIGARs, so a path's
//    CIGAR is fixed by its I/D operations, which a 128-bit shift register of 16-bit entries holds (push on the way
//    down, pop on the way back).
//  * D table in registers: it is non-decreasing and a node is cut when edits_left < D[i], i.e. when i >= brk[e]
//    with brk[e] the first i where D[i] > e; only brk[0 .. k] matter.
//  * Load balance: hit counts (and search trees) differ by orders of magnitude between patterns.  The lane's loop is
//    flat -- one step of the search, of the chain or of starting a pattern per iteration -- and a lane that finishes
//    its pattern takes the next one from a counter, so it does not wait for the rest of its wave.
#include "sx_common.hpp"
#include "sx_device.hpp"
#include "sx_index.hpp"
#include "sx_occ.hpp"
#include "sx_scan.hpp"

#include <stdlib.h>

namespace sx {

#ifndef SX_APPROX_LANES
#define SX_APPROX_LANES (1u << 18) // persistent lanes (1024 a CU); each holds a stack of (longest pattern + k) frames
#endif

constexpr int kApproxBlock = 256;
constexpr int kMaxEdits = SX_APPROX_MAX_EDITS;

// Occ: how O(a, row) is read (sx_occ.hpp); OccFull is one pointer, so ApproxArgs is laid out as it was before the
// accessor came
template <class Occ> struct ApproxArgsT {
    const uint32_t *c;
    Occ o, ro;
    uint64_t N;
    uint32_t sigma;
    const uint8_t *pat;
    const uint32_t *off;
    uint32_t count;
    int k;
    uint32_t lanes, frames; // frames per lane
    uint4 *stack;
    uint32_t *next;         // [0] work counter, [1] error word (a stack that would overflow)
    uint32_t *counts;       // count pass: hits per pattern
    unsigned long long *total;
    const uint64_t *hit_off; // emit pass
    uint4 *hits;
    uint64_t cap;
};

using ApproxArgs = ApproxArgsT<OccFull>;

enum : uint32_t { kFetch = 0, kScan = 1, kChain = 2 };

__device__ __forceinline__ uint4 u4(uint32_t x, uint32_t y, uint32_t z, uint32_t w)
{
    uint4 v;
    v.x = x;
    v.y = y;
    v.z = z;
    v.w = w;
    return v;
}

template <bool kEmit, class Occ>
__global__ __launch_bounds__(kApproxBlock) void bwt_approx_kernel(ApproxArgsT<Occ> A)
{
    const uint32_t t = blockIdx.x * kApproxBlock + threadIdx.x;
    if (t >= A.lanes) return;
    const uint32_t sigma = A.sigma;
    const uint32_t nI = sigma - 1; // child index of I; M(a) is a - 1, D(a) is sigma - 1 + a
    const uint32_t *__restrict__ C = A.c;
    const Occ O = A.o;
    uint4 *stack = A.stack + t;

    uint32_t mode = kFetch, q = 0, m = 0, cnt = 0;
    const uint8_t *p = nullptr;
    uint64_t out_base = 0;
    uint32_t brk[kMaxEdits + 1];
    // current node
    uint32_t L = 0, R = 0, c = 0, depth = 0;
    int32_t i = 0, e = 0;
    uint32_t ml = 0;
    // I/D operations on the path: 16-bit entries (search depth | D bit), the latest in the low bits
    uint64_t g_lo = 0, g_hi = 0;
    uint32_t ng = 0;
    // chain (the exact search below a child with no edit left, or a hit right away)
    uint32_t L2 = 0, R2 = 0, hml = 0, hlen = 0;
    int32_t j = 0;

    for (;;) {
        if (mode == kChain) {
            if (j >= 0 && L2 < R2) {
                const uint32_t a = p[j];
                L2 = C[a] + O.rank(a, L2, sigma);
                R2 = C[a] + O.rank(a, R2, sigma);
                --j;
                continue;
            }
            if (L2 < R2) { // a hit: the interval, its match length, its I/D operations in pattern order
                if (kEmit) {
                    const uint64_t idx = out_base + cnt;
                    if (idx < A.cap) {
                        uint32_t gw[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                        for (int s = 0; s < kMaxEdits; ++s) {
                            if ((uint32_t)s < ng) {
                                const uint32_t g = (uint32_t)((s < 4 ? g_lo >> (16 * s) : g_hi >> (16 * (s - 4))) & 0xFFFFu);
                                const uint32_t v = ((hlen - 1u - (g & 0x7FFFu)) & 0x7FFFu) | (g & SX_APPROX_GAP_D);
                                gw[s >> 1] |= v << (16 * (s & 1));
                            }
                        }
                        A.hits[2 * idx] = u4(q, L2, R2, (hml & 0xFFFFu) | (ng << 16));
                        A.hits[2 * idx + 1] = u4(gw[0], gw[1], gw[2], gw[3]);
                    }
                }
                ++cnt;
            }
            if (c >= nI) { // back from an I or D child: its operation leaves the path
                g_lo = (g_lo >> 16) | (g_hi << 48);
                g_hi >>= 16;
                --ng;
            }
            ++c;
            mode = kScan;
            continue;
        }
        if (mode == kScan) {
            const uint32_t nchild = depth == 0 ? sigma : 2 * sigma - 1;
            if (c < nchild) {
                uint32_t nL = L, nR = R;
                int32_t ci = i - 1, ce = e - 1;
                bool take = false;
                if (c != nI) { // M(a) or D(a): the same child interval
                    const uint32_t a = c < nI ? c + 1 : c - nI;
                    if (c < nI) ce = e - (a == (uint32_t)p[i] ? 0 : 1);
                    else ci = i;
                    if (ce >= 0) {
                        nL = C[a] + O.rank(a, L, sigma);
                        nR = C[a] + O.rank(a, R, sigma);
                        take = nL < nR;
                    }
                } else {
                    take = ce >= 0;
                }
                if (take && ci >= 0) { // the reference's cut at the child: edits_left < D[i]
                    uint32_t b = brk[0];
#pragma unroll
                    for (int s = 1; s <= kMaxEdits; ++s)
                        if (s == ce) b = brk[s];
                    take = (uint32_t)ci < b;
                }
                if (!take) {
                    ++c;
                    continue;
                }
                const uint32_t cml = ml + (c == nI ? 0u : 1u);
                if (c >= nI) { // I or D: onto the path's list of operations
                    g_hi = (g_hi << 16) | (g_lo >> 48);
                    g_lo = (g_lo << 16) | (uint64_t)(depth | (c > nI ? SX_APPROX_GAP_D : 0u));
                    ++ng;
                }
                if (ci < 0 || ce == 0) { // a hit, or the exact search of the rest: no frame
                    L2 = nL;
                    R2 = nR;
                    j = ci;
                    hml = cml + (uint32_t)(ci + 1);
                    hlen = depth + 1u + (uint32_t)(ci + 1);
                    mode = kChain;
                    continue;
                }
                if (depth >= A.frames) { // (cannot happen: frames = longest pattern + k)
                    atomicOr(A.next + 1, 1u);
                    mode = kFetch;
                    if (!kEmit) A.counts[q] = cnt;
                    continue;
                }
                stack[(uint64_t)depth * A.lanes] = u4(L, R, c | ((uint32_t)e << 16), (uint32_t)i | (ml << 16));
                L = nL;
                R = nR;
                i = ci;
                e = ce;
                ml = cml;
                c = 0;
                ++depth;
                continue;
            }
            if (depth > 0) { // the node is done: back to its parent, on to the parent's next child
                --depth;
                const uint4 f = stack[(uint64_t)depth * A.lanes];
                L = f.x;
                R = f.y;
                c = f.z & 0xFFFFu;
                e = (int32_t)(f.z >> 16);
                i = (int32_t)(f.w & 0xFFFFu);
                ml = f.w >> 16;
                if (c >= nI) {
                    g_lo = (g_lo >> 16) | (g_hi << 48);
                    g_hi >>= 16;
                    --ng;
                }
                ++c;
                continue;
            }
            // the root is done
            if (!kEmit) {
                A.counts[q] = cnt;
                if (cnt) atomicAdd(A.total, (unsigned long long)cnt);
            }
            mode = kFetch;
            continue;
        }
        // kFetch: the next pattern
        q = atomicAdd(A.next, 1u);
        if (q >= A.count) break;
        const uint32_t begin = A.off[q];
        m = A.off[q + 1] - begin;
        p = A.pat + begin;
        cnt = 0;
        if (kEmit) out_base = A.hit_off[q];
        // symbols in [1, sigma) (the reference asserts it) and the D table's break points (bwt.c:319-338)
        bool ok = m > 0;
#pragma unroll
        for (int s = 0; s <= kMaxEdits; ++s) brk[s] = m;
        uint32_t rL = 0, rR = (uint32_t)A.N;
        int32_t me = 0;
        for (uint32_t s = 0; s < m; ++s) {
            const uint32_t a = p[s];
            if (a == 0 || a >= sigma) {
                ok = false;
                break;
            }
            if (A.ro.present() && me <= A.k) {
                rL = C[a] + A.ro.rank(a, rL, sigma);
                rR = C[a] + A.ro.rank(a, rR, sigma);
                if (rL >= rR) {
                    ++me;
#pragma unroll
                    for (int b = 0; b <= kMaxEdits; ++b)
                        if (b == me - 1) brk[b] = s;
                    rL = 0;
                    rR = (uint32_t)A.N;
                }
            }
        }
        if (!ok) {
            if (!kEmit) A.counts[q] = 0;
            continue;
        }
        L = 0;
        R = (uint32_t)A.N;
        i = (int32_t)m - 1;
        e = A.k;
        ml = 0;
        c = 0;
        depth = 0;
        g_lo = g_hi = 0;
        ng = 0;
        mode = kScan;
    }
}

// The search without I and D (SX_SEARCH_NO_INDELS): the same walk with the M children only, so its
// hits are those of bwt_approx_kernel whose path took no I or D child, in that kernel's order.  A node at search depth
// d stands at pattern index m - 1 - d with match length d, so neither is kept; a frame is {L, R} and {next child |
// edits_left | the node's pattern symbol}, 12 bytes in two planes of the same workspace (frame d of lane t at
// lr[d * lanes + t], ce[d * lanes + t]); there is no list of operations, and a hit's match length is m and its gap[]
// zeros.  The D table cuts as it does there: a bound on the edits of any kind that the rest of the pattern needs is one
// on its substitutions too.
// A step of the loop has one place where it reads the table: a step of the chain and a child of a node both come down
// to "the interval of a in front of [lo, hi)", so the step first says what it looks up, then every lane of the wave that
// looks anything up does so together (with the pattern symbol the next step will need), then the step's state moves on.
// The loop has one back edge; the kernel above, whose steps each read on their own, is laid out by the compiler as
// nested loops in which the lanes of a wave wait for each other's chains.
template <bool kEmit, class Occ>
__global__ __launch_bounds__(kApproxBlock) void bwt_hamming_kernel(ApproxArgsT<Occ> A)
{
    const uint32_t t = blockIdx.x * kApproxBlock + threadIdx.x;
    if (t >= A.lanes) return;
    const uint32_t sigma = A.sigma;
    const uint32_t nM = sigma - 1; // children of a node: M(a) is a - 1
    const uint32_t *__restrict__ C = A.c;
    const Occ O = A.o;
    uint2 *lr = reinterpret_cast<uint2 *>(A.stack) + t;
    uint32_t *ce_plane = reinterpret_cast<uint32_t *>(reinterpret_cast<uint2 *>(A.stack) + (uint64_t)A.frames * A.lanes) + t;

    uint32_t mode = kFetch, q = 0, m = 0, cnt = 0;
    const uint8_t *p = nullptr;
    uint64_t out_base = 0;
    uint32_t brk[kMaxEdits + 1];
    // current node: its interval, next child, search depth, edits left, and the pattern symbol it stands at
    uint32_t L = 0, R = 0, c = 0, depth = 0, pa = 0;
    int32_t e = 0;
    // chain (the exact search below a child with no edit left, or a hit right away): interval, next index and its symbol
    uint32_t L2 = 0, R2 = 0, pj = 0;
    int32_t j = 0;

    for (bool live = true; live;) {
        // what this step looks up: a of [lo, hi), and the pattern index whose symbol the step behind it stands at
        uint32_t a = 0, lo = 0, hi = 0;
        int32_t ni = -1, ce = 0;
        bool look = false;
        if (mode == kChain) {
            look = j >= 0 && L2 < R2;
            a = pj, lo = L2, hi = R2, ni = j - 1;
        } else if (mode == kScan && c < nM) {
            a = c + 1, lo = L, hi = R, ni = (int32_t)(m - 1u - depth) - 1;
            ce = e - (a == pa ? 0 : 1);
            look = ce >= 0;
        }
        uint32_t nL = lo, nR = hi, nx = 0;
        if (look) {
            const uint32_t base = C[a];
            nL = base + O.rank(a, lo, sigma);
            nR = base + O.rank(a, hi, sigma);
            if (ni >= 0) nx = p[ni];
        }
        if (mode == kChain) {
            if (look) {
                L2 = nL, R2 = nR, j = ni, pj = nx;
            } else {
                if (L2 < R2) { // a hit: the interval; the pattern is aligned to m symbols, with no I/D operation
                    if (kEmit) {
                        const uint64_t idx = out_base + cnt;
                        if (idx < A.cap) {
                            A.hits[2 * idx] = u4(q, L2, R2, m & 0xFFFFu);
                            A.hits[2 * idx + 1] = u4(0u, 0u, 0u, 0u);
                        }
                    }
                    ++cnt;
                }
                ++c;
                mode = kScan;
            }
        } else if (mode == kScan) {
            if (c < nM) {
                bool take = look && nL < nR;
                if (take && ni >= 0) { // the reference's cut at the child: edits_left < D[i]
                    uint32_t b = brk[0];
#pragma unroll
                    for (int s = 1; s <= kMaxEdits; ++s)
                        if (s == ce) b = brk[s];
                    take = (uint32_t)ni < b;
                }
                if (!take) {
                    ++c;
                } else if (ni < 0 || ce == 0) { // a hit, or the exact search of the rest: no frame
                    L2 = nL, R2 = nR, j = ni, pj = nx;
                    mode = kChain;
                } else if (depth >= A.frames) { // (cannot happen: frames >= longest pattern)
                    atomicOr(A.next + 1, 1u);
                    mode = kFetch;
                    if (!kEmit) A.counts[q] = cnt;
                } else {
                    uint2 f;
                    f.x = L;
                    f.y = R;
                    lr[(uint64_t)depth * A.lanes] = f;
                    ce_plane[(uint64_t)depth * A.lanes] = c | ((uint32_t)e << 16) | (pa << 24);
                    L = nL, R = nR, e = ce, pa = nx;
                    c = 0;
                    ++depth;
                }
            } else if (depth > 0) { // the node is done: back to its parent, on to the parent's next child
                --depth;
                const uint2 f = lr[(uint64_t)depth * A.lanes];
                const uint32_t w = ce_plane[(uint64_t)depth * A.lanes];
                L = f.x, R = f.y;
                c = (w & 0xFFFFu) + 1u;
                e = (int32_t)((w >> 16) & 0xFFu);
                pa = w >> 24;
            } else { // the root is done
                if (!kEmit) {
                    A.counts[q] = cnt;
                    if (cnt) atomicAdd(A.total, (unsigned long long)cnt);
                }
                mode = kFetch;
            }
        } else { // kFetch: the next pattern
            q = atomicAdd(A.next, 1u);
            if (q >= A.count) {
                live = false;
            } else {
                const uint32_t begin = A.off[q];
                m = A.off[q + 1] - begin;
                p = A.pat + begin;
                cnt = 0;
                if (kEmit) out_base = A.hit_off[q];
                // symbols in [1, sigma) and the D table's break points, as in bwt_approx_kernel
                bool ok = m > 0;
#pragma unroll
                for (int s = 0; s <= kMaxEdits; ++s) brk[s] = m;
                uint32_t rL = 0, rR = (uint32_t)A.N;
                int32_t me = 0;
                for (uint32_t s = 0; s < m; ++s) {
                    const uint32_t x = p[s];
                    if (x == 0 || x >= sigma) {
                        ok = false;
                        break;
                    }
                    if (A.ro.present() && me <= A.k) {
                        rL = C[x] + A.ro.rank(x, rL, sigma);
                        rR = C[x] + A.ro.rank(x, rR, sigma);
                        if (rL >= rR) {
                            ++me;
#pragma unroll
                            for (int b = 0; b <= kMaxEdits; ++b)
                                if (b == me - 1) brk[b] = s;
                            rL = 0;
                            rR = (uint32_t)A.N;
                        }
                    }
                }
                if (!ok) {
                    if (!kEmit) A.counts[q] = 0;
                } else {
                    L = 0;
                    R = (uint32_t)A.N;
                    e = A.k;
                    c = 0;
                    depth = 0;
                    pa = p[m - 1u];
                    mode = kScan;
                }
            }
        }
    }
}

// the pass over A's patterns, with or without I and D
template <bool kEmit, class Occ> static void approx_launch(sx_ctx *ctx, const ApproxArgsT<Occ> &A, uint32_t search_flags, uint64_t bytes)
{
    if (search_flags & SX_SEARCH_NO_INDELS)
        sx_launch(ctx, SX_KC_SEARCH, bytes, bwt_hamming_kernel<kEmit, Occ>, dim3(A.lanes / kApproxBlock), dim3(kApproxBlock), A);
    else
        sx_launch(ctx, SX_KC_SEARCH, bytes, bwt_approx_kernel<kEmit, Occ>, dim3(A.lanes / kApproxBlock), dim3(kApproxBlock), A);
}

struct InLen {
    const uint32_t *off;
    __device__ __forceinline__ uint32_t operator()(uint64_t q) const { return off[q + 1] - off[q]; }
};
struct OutNone {
    __device__ __forceinline__ void operator()(uint64_t, uint32_t, uint32_t) const {}
};
struct OutOffsets64 {
    uint64_t *p;
    __device__ __forceinline__ void operator()(uint64_t q, uint32_t excl, uint32_t) const { p[q] = excl; }
};

__global__ void approx_finish_offsets_kernel(const unsigned long long *total, uint64_t *hit_off, uint32_t count)
{
    if (threadIdx.x == 0) hit_off[count] = *total;
}

static uint32_t approx_lanes(uint32_t count)
{
    const uint32_t want = ((count + kApproxBlock - 1) / kApproxBlock) * kApproxBlock;
    return want < SX_APPROX_LANES ? want : SX_APPROX_LANES;
}

// the workspace of a pass over A's patterns (stack, counts, counters: the BWT and N slabs)
template <class Occ> static int approx_workspace(sx_ctx *ctx, ApproxArgsT<Occ> &A)
{
    // the longest pattern (the stack's depth, the 2^15 limit)
    SX_TRY(sx_slab_ensure(ctx, SX_SLAB_BWT, 4096));
    uint32_t *scal = (uint32_t *)ctx->slab[SX_SLAB_BWT].p; // [0] longest, [2..3] u64 total, [4] counter, [5] error
    SX_CHECK(hipMemsetAsync(scal, 0, 64, ctx->stream));
    SX_TRY((device_scan<OpMax>(ctx, A.count, InLen{A.off}, OutNone{}, scal, SX_KC_SEARCH, (uint64_t)A.count * 8)));
    uint32_t longest = 0;
    SX_TRY(sx_readback(ctx, scal, 1, &longest));
    if ((uint64_t)longest + (uint64_t)A.k >= (1u << 15))
        return sx_fail_msg(ctx, SX_E_ARG, "approximate search: pattern length + max_edits must stay below 2^15");
    A.lanes = approx_lanes(A.count);
    A.frames = longest + (uint32_t)A.k + 1u;
    const size_t cnt_b = ((size_t)A.count * 4 + 255) & ~(size_t)255;
    SX_TRY(sx_slab_ensure(ctx, SX_SLAB_N, cnt_b + (size_t)A.lanes * A.frames * sizeof(uint4)));
    A.counts = (uint32_t *)ctx->slab[SX_SLAB_N].p;
    A.stack = (uint4 *)((char *)ctx->slab[SX_SLAB_N].p + cnt_b);
    A.total = (unsigned long long *)(scal + 2);
    A.next = scal + 4;
    return 0;
}

// count pass + offsets; the workspace stays where it is for the emit pass
template <class Occ> static int approx_count(sx_ctx *ctx, ApproxArgsT<Occ> &A, uint32_t search_flags, uint64_t *d_hit_off, uint64_t *total_out)
{
    SX_TRY(approx_workspace(ctx, A));
    uint32_t *scal = (uint32_t *)ctx->slab[SX_SLAB_BWT].p;
    approx_launch<false>(ctx, A, search_flags, 0);
    SX_TRY((device_scan<OpAdd>(ctx, A.count, InU32{A.counts}, OutOffsets64{d_hit_off}, nullptr, SX_KC_SEARCH, (uint64_t)A.count * 12)));
    sx_launch(ctx, SX_KC_SEARCH, 0, approx_finish_offsets_kernel, dim3(1), dim3(64), (const unsigned long long *)A.total, d_hit_off, A.count);
    uint32_t h[4] = {0, 0, 0, 0};
    SX_TRY(sx_readback(ctx, scal + 2, 4, h));
    if (h[3]) return sx_fail_msg(ctx, SX_E_INTERNAL, "approximate search: a search stack overflowed");
    const uint64_t total = (uint64_t)h[0] | ((uint64_t)h[1] << 32);
    if (total >= (1ull << 32)) return sx_fail_msg(ctx, SX_E_ARG, "approximate search: 2^32 hits or more in one call");
    *total_out = total;
    return 0;
}

template <class Occ>
static int approx_emit(sx_ctx *ctx, ApproxArgsT<Occ> &A, uint32_t search_flags, const uint64_t *d_hit_off, sx_approx_hit *d_hits, uint64_t total)
{
    A.hit_off = d_hit_off;
    A.hits = (uint4 *)d_hits;
    A.cap = total;
    SX_CHECK(hipMemsetAsync(A.next, 0, 8, ctx->stream));
    approx_launch<true>(ctx, A, search_flags, total * sizeof(sx_approx_hit));
    uint32_t h[2] = {0, 0};
    SX_TRY(sx_readback(ctx, A.next, 2, h));
    if (h[1]) return sx_fail_msg(ctx, SX_E_INTERNAL, "approximate search: a search stack overflowed");
    return 0;
}

template <class Occ>
static int approx_args(sx_ctx *ctx, ApproxArgsT<Occ> &A, const uint32_t *c, Occ o, Occ ro, uint64_t N, uint32_t sigma, const uint8_t *pat,
                       const uint32_t *off, uint32_t count, int k, uint32_t search_flags)
{
    (void)ctx;
    if (search_flags & ~(uint32_t)SX_SEARCH_NO_INDELS) return SX_E_ARG;
    if (!c || !o.p || !off || N == 0 || N > 0xFFFFFFFFull || sigma < 2 || sigma > 256 || k > kMaxEdits) return SX_E_ARG;
    A = ApproxArgsT<Occ>{};
    A.c = c;
    A.o = o;
    A.ro = ro;
    A.N = N;
    A.sigma = sigma;
    A.pat = pat;
    A.off = off;
    A.count = count;
    A.k = k;
    return 0;
}

} // namespace sx

using namespace sx;

// sx_bwt_approx_search_dev in any form of the tables
template <class Occ>
static int approx_search_dev(sx_ctx *ctx, const uint32_t *d_c_table, Occ o, Occ ro, uint64_t N, uint32_t sigma, const uint8_t *d_patterns,
                             const uint32_t *d_offsets, uint32_t count, int max_edits, uint64_t *d_hit_offsets, sx_approx_hit *d_hits,
                             uint64_t hit_capacity, uint64_t *total_hits_out, uint32_t search_flags)
{
    if (!ctx || !d_hit_offsets || !total_hits_out || ((uintptr_t)d_hits & 15)) return SX_E_ARG;
    ApproxArgsT<Occ> A;
    SX_TRY(approx_args(ctx, A, d_c_table, o, ro, N, sigma, d_patterns, d_offsets, count, max_edits, search_flags));
    SX_CHECK(hipSetDevice(ctx->device));
    *total_hits_out = 0;
    if (max_edits < 0 || count == 0) { // no search: every offset 0
        SX_CHECK(hipMemsetAsync(d_hit_offsets, 0, ((size_t)count + 1) * sizeof(uint64_t), ctx->stream));
        return sx_sync(ctx);
    }
    uint64_t total = 0;
    SX_TRY(approx_count(ctx, A, search_flags, d_hit_offsets, &total));
    *total_hits_out = total;
    if (!d_hits) return sx_sync(ctx);
    if (total > hit_capacity) {
        SX_TRY(sx_sync(ctx));
        sx_fail_msg(ctx, SX_E_CAPACITY, "approximate search: more hits than hit_capacity");
        return SX_E_CAPACITY;
    }
    if (total) SX_TRY(approx_emit(ctx, A, search_flags, d_hit_offsets, d_hits, total));
    return sx_sync(ctx);
}

// the search over a record of an index in whichever form its tables have (the mapper's loop, sx_map.hip)
int sx_approx_search_record(sx_ctx *ctx, const sx_index_rec &R, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t count, int max_edits,
                            uint64_t *d_hit_offsets, sx_approx_hit *d_hits, uint64_t hit_capacity, uint64_t *total_hits_out, uint32_t search_flags)
{
    if (R.packed)
        return sx_bwt_approx_search_packed_dev_ex(ctx, R.d_c, R.d_occ, R.d_rocc, R.N, R.sigma, d_patterns, d_offsets, count, max_edits, d_hit_offsets,
                                                  d_hits, hit_capacity, total_hits_out, search_flags);
    return R.compact() ? sx_bwt_approx_search_compact_dev_ex(ctx, R.d_c, R.d_occ, R.d_rocc, R.N, R.sigma, d_patterns, d_offsets, count, max_edits,
                                                             d_hit_offsets, d_hits, hit_capacity, total_hits_out, search_flags)
                       : sx_bwt_approx_search_dev_ex(ctx, R.d_c, R.d_o, R.d_ro, R.N, R.sigma, d_patterns, d_offsets, count, max_edits, d_hit_offsets,
                                                     d_hits, hit_capacity, total_hits_out, search_flags);
}

// f(o, ro): the accessors of a record's tables in whichever form they have
template <class F> static int with_record_occ(const sx_index_rec &R, F f)
{
    if (R.compact() && (((uintptr_t)R.d_occ | (uintptr_t)R.d_rocc) & 15u)) return SX_E_ARG; // (the layout of sx_occ.hpp)
    if (R.packed) return R.sigma > kOccPackedMaxSigma ? SX_E_ARG : f(OccPacked{R.d_occ}, OccPacked{R.d_rocc});
    if (R.compact()) {
        if (R.sigma > 128) return SX_E_ARG;
        const uint32_t stride = occ_stride(R.sigma);
        return f(OccCompact{R.d_occ, stride}, OccCompact{R.d_rocc, stride});
    }
    return f(OccFull{R.d_o}, OccFull{R.d_ro});
}

// the two passes on their own, for the rounds of sx_best.hip: they launch what the passes of approx_search_dev launch
int sx_approx_count_record(sx_ctx *ctx, const sx_index_rec &R, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t count, int max_edits,
                           uint64_t *d_hit_offsets, uint64_t *total_hits_out, uint32_t search_flags)
{
    if (!ctx || !d_hit_offsets || !total_hits_out || count == 0 || max_edits < 0) return SX_E_ARG;
    return with_record_occ(R, [&](auto o, auto ro) -> int {
        ApproxArgsT<decltype(o)> A;
        SX_TRY(approx_args(ctx, A, R.d_c, o, ro, R.N, R.sigma, d_patterns, d_offsets, count, max_edits, search_flags));
        return approx_count(ctx, A, search_flags, d_hit_offsets, total_hits_out);
    });
}

int sx_approx_emit_record(sx_ctx *ctx, const sx_index_rec &R, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t count, int max_edits,
                          const uint64_t *d_hit_offsets, sx_approx_hit *d_hits, uint64_t total_hits, uint32_t search_flags)
{
    if (!ctx || !d_hit_offsets || !d_hits || ((uintptr_t)d_hits & 15) || count == 0 || max_edits < 0 || total_hits == 0) return SX_E_ARG;
    return with_record_occ(R, [&](auto o, auto ro) -> int {
        ApproxArgsT<decltype(o)> A;
        SX_TRY(approx_args(ctx, A, R.d_c, o, ro, R.N, R.sigma, d_patterns, d_offsets, count, max_edits, search_flags));
        SX_TRY(approx_workspace(ctx, A));
        return approx_emit(ctx, A, search_flags, d_hit_offsets, d_hits, total_hits);
    });
}

extern "C" {

int sx_bwt_approx_search_dev_ex(sx_ctx *ctx, const uint32_t *d_c_table, const uint32_t *d_o_table, const uint32_t *d_ro_table, uint64_t N,
                                uint32_t sigma, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t count, int max_edits,
                                uint64_t *d_hit_offsets, sx_approx_hit *d_hits, uint64_t hit_capacity, uint64_t *total_hits_out,
                                uint32_t search_flags)
{
    return approx_search_dev(ctx, d_c_table, OccFull{d_o_table}, OccFull{d_ro_table}, N, sigma, d_patterns, d_offsets, count, max_edits,
                             d_hit_offsets, d_hits, hit_capacity, total_hits_out, search_flags);
}

int sx_bwt_approx_search_dev(sx_ctx *ctx, const uint32_t *d_c_table, const uint32_t *d_o_table,
                             const uint32_t *d_ro_table, uint64_t N, uint32_t sigma, const uint8_t *d_patterns,
                             const uint32_t *d_offsets, uint32_t count, int max_edits, uint64_t *d_hit_offsets,
                             sx_approx_hit *d_hits, uint64_t hit_capacity, uint64_t *total_hits_out)
{
    return sx_bwt_approx_search_dev_ex(ctx, d_c_table, d_o_table, d_ro_table, N, sigma, d_patterns, d_offsets, count, max_edits, d_hit_offsets,
                                       d_hits, hit_capacity, total_hits_out, 0);
}

int sx_bwt_approx_search_compact_dev_ex(sx_ctx *ctx, const uint32_t *d_c_table, const uint8_t *d_occ, const uint8_t *d_rocc, uint64_t N,
                                        uint32_t sigma, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t count, int max_edits,
                                        uint64_t *d_hit_offsets, sx_approx_hit *d_hits, uint64_t hit_capacity, uint64_t *total_hits_out,
                                        uint32_t search_flags)
{
    if (sigma > 128 || (((uintptr_t)d_occ | (uintptr_t)d_rocc) & 15u)) return SX_E_ARG; // (the layout of sx_occ.hpp)
    const uint32_t stride = occ_stride(sigma);
    return approx_search_dev(ctx, d_c_table, OccCompact{d_occ, stride}, OccCompact{d_rocc, stride}, N, sigma, d_patterns, d_offsets, count,
                             max_edits, d_hit_offsets, d_hits, hit_capacity, total_hits_out, search_flags);
}

int sx_bwt_approx_search_compact_dev(sx_ctx *ctx, const uint32_t *d_c_table, const uint8_t *d_occ, const uint8_t *d_rocc, uint64_t N,
                                     uint32_t sigma, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t count, int max_edits,
                                     uint64_t *d_hit_offsets, sx_approx_hit *d_hits, uint64_t hit_capacity, uint64_t *total_hits_out)
{
    return sx_bwt_approx_search_compact_dev_ex(ctx, d_c_table, d_occ, d_rocc, N, sigma, d_patterns, d_offsets, count, max_edits, d_hit_offsets,
                                               d_hits, hit_capacity, total_hits_out, 0);
}

int sx_bwt_approx_search_packed_dev_ex(sx_ctx *ctx, const uint32_t *d_c_table, const uint8_t *d_occ, const uint8_t *d_rocc, uint64_t N,
                                       uint32_t sigma, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t count, int max_edits,
                                       uint64_t *d_hit_offsets, sx_approx_hit *d_hits, uint64_t hit_capacity, uint64_t *total_hits_out,
                                       uint32_t search_flags)
{
    if (sigma > kOccPackedMaxSigma || (((uintptr_t)d_occ | (uintptr_t)d_rocc) & 15u)) return SX_E_ARG; // (the layout of sx_occ.hpp)
    return approx_search_dev(ctx, d_c_table, OccPacked{d_occ}, OccPacked{d_rocc}, N, sigma, d_patterns, d_offsets, count, max_edits,
                             d_hit_offsets, d_hits, hit_capacity, total_hits_out, search_flags);
}

int sx_bwt_approx_search_packed_dev(sx_ctx *ctx, const uint32_t *d_c_table, const uint8_t *d_occ, const uint8_t *d_rocc, uint64_t N,
                                    uint32_t sigma, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t count, int max_edits,
                                    uint64_t *d_hit_offsets, sx_approx_hit *d_hits, uint64_t hit_capacity, uint64_t *total_hits_out)
{
    return sx_bwt_approx_search_packed_dev_ex(ctx, d_c_table, d_occ, d_rocc, N, sigma, d_patterns, d_offsets, count, max_edits, d_hit_offsets,
                                              d_hits, hit_capacity, total_hits_out, 0);
}

int sx_bwt_approx_search(sx_ctx *ctx, const uint32_t *c_table, const uint32_t *o_table, const uint32_t *ro_table,
                         uint64_t N, uint32_t sigma, const uint8_t *patterns, const uint32_t *offsets, uint32_t count,
                         int max_edits, uint64_t *hit_offsets, sx_approx_hit **hits_out, uint64_t *total_hits_out)
{
    return sx_bwt_approx_search_ex(ctx, c_table, o_table, ro_table, N, sigma, patterns, offsets, count, max_edits, hit_offsets, hits_out,
                                   total_hits_out, 0);
}

int sx_bwt_approx_search_ex(sx_ctx *ctx, const uint32_t *c_table, const uint32_t *o_table, const uint32_t *ro_table, uint64_t N,
                            uint32_t sigma, const uint8_t *patterns, const uint32_t *offsets, uint32_t count, int max_edits,
                            uint64_t *hit_offsets, sx_approx_hit **hits_out, uint64_t *total_hits_out, uint32_t search_flags)
{
    if (!ctx || !hit_offsets || !hits_out || !total_hits_out) return SX_E_ARG;
    *hits_out = nullptr;
    *total_hits_out = 0;
    ApproxArgs A;
    SX_TRY(approx_args(ctx, A, c_table, OccFull{o_table}, OccFull{ro_table}, N, sigma, patterns, offsets, count, max_edits, search_flags));
    if (max_edits < 0 || count == 0) {
        memset(hit_offsets, 0, ((size_t)count + 1) * sizeof(uint64_t));
        return 0;
    }
    SX_CHECK(hipSetDevice(ctx->device));
    // staging: C, O, RO, patterns, offsets, hit offsets (the hits themselves go to the M slab once their number is known)
    const uint64_t plen = offsets[count];
    const size_t c_b = ((size_t)sigma * 4 + 255) & ~(size_t)255, o_b = (((N + 1) * sigma * 4) + 255) & ~(size_t)255,
                 p_b = (plen + 16 + 255) & ~(size_t)255, off_b = (((size_t)count + 1) * 4 + 255) & ~(size_t)255,
                 ho_b = (((size_t)count + 1) * 8 + 255) & ~(size_t)255;
    SX_TRY(sx_slab_ensure(ctx, SX_SLAB_IO, c_b + o_b * (ro_table ? 2 : 1) + p_b + off_b + ho_b));
    char *base = (char *)ctx->slab[SX_SLAB_IO].p;
    uint32_t *d_c = (uint32_t *)base, *d_o = (uint32_t *)(base + c_b);
    uint32_t *d_ro = ro_table ? (uint32_t *)(base + c_b + o_b) : nullptr;
    char *rest = base + c_b + o_b * (ro_table ? 2 : 1);
    uint8_t *d_p = (uint8_t *)rest;
    uint32_t *d_off = (uint32_t *)(rest + p_b);
    uint64_t *d_ho = (uint64_t *)(rest + p_b + off_b);
    SX_CHECK(hipMemcpyAsync(d_c, c_table, (size_t)sigma * 4, hipMemcpyHostToDevice, ctx->stream));
    SX_CHECK(hipMemcpyAsync(d_o, o_table, (size_t)(N + 1) * sigma * 4, hipMemcpyHostToDevice, ctx->stream));
    if (ro_table) SX_CHECK(hipMemcpyAsync(d_ro, ro_table, (size_t)(N + 1) * sigma * 4, hipMemcpyHostToDevice, ctx->stream));
    if (plen) SX_CHECK(hipMemcpyAsync(d_p, patterns, plen, hipMemcpyHostToDevice, ctx->stream));
    SX_CHECK(hipMemcpyAsync(d_off, offsets, ((size_t)count + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    A.c = d_c;
    A.o = OccFull{d_o};
    A.ro = OccFull{d_ro};
    A.pat = d_p;
    A.off = d_off;
    uint64_t total = 0;
    SX_TRY(approx_count(ctx, A, search_flags, d_ho, &total));
    SX_CHECK(hipMemcpyAsync(hit_offsets, d_ho, ((size_t)count + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (total) {
        SX_TRY(sx_slab_ensure(ctx, SX_SLAB_M, total * sizeof(sx_approx_hit)));
        sx_approx_hit *d_hits = (sx_approx_hit *)ctx->slab[SX_SLAB_M].p;
        SX_TRY(approx_emit(ctx, A, search_flags, d_ho, d_hits, total));
        sx_approx_hit *h = (sx_approx_hit *)malloc(total * sizeof(sx_approx_hit));
        if (!h) return sx_fail_msg(ctx, SX_E_NOMEM, "approximate search: host hit array");
        const hipError_t e = hipMemcpyAsync(h, d_hits, total * sizeof(sx_approx_hit), hipMemcpyDeviceToHost, ctx->stream);
        if (e != hipSuccess || sx_sync(ctx) != 0) {
            free(h);
            return sx_fail_msg(ctx, SX_E_INTERNAL, "approximate search: hit download");
        }
        *hits_out = h;
    }
    *total_hits_out = total;
    return sx_sync(ctx);
}

} // extern "C"
