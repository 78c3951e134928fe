"""The consumers of a resident suffix array on the MI355X at the sizes where their forms change (sx_extras.hip,
sx_approx.hip): inverse and LCP through sa_inverse_dev / sa_lcp_dev on both sides of the plain / three-pass threshold
(N = 2^23) and of the coarse-window step at N = 2^28, a long-repeat text at 2^28, batched exact search at sigma = 256 and
on 2^28 DNA tables, and the k-edit search with several patterns a lane and wide alphabets.  Exact comparisons with the
oracle where the host can afford them, stralg_amd.verify.verify_inverse_lcp_on_device elsewhere."""
import numpy as np
import pytest

import approx_model
import oracle
from next_rows_cases import exact_patterns
from stralg_amd import api, synth, verify

pytestmark = pytest.mark.gpu


def _dna_sa(ctx, n, seed):
    import torch
    text = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctx.synth_dev(text, n, 5, seed)
    sa = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    ctx.sa_build_dev(text, n, 5, sa)
    return text, sa


def _inverse_lcp_all_entries(ctx, text, sa, n):
    """(inv, lcp) from sa_inverse_dev, and sa_lcp_dev with and without the inverse output, the three agreeing"""
    import torch
    N = n + 1
    inv = torch.empty(N, dtype=torch.int32, device="cuda")
    ctx.sa_inverse_dev(sa, N, inv)
    inv2 = torch.empty(N, dtype=torch.int32, device="cuda")
    lcp = torch.empty(N, dtype=torch.int32, device="cuda")
    ctx.sa_lcp_dev(text, sa, N, inv2, lcp)
    assert torch.equal(inv, inv2)
    del inv2
    lcp2 = torch.empty(N, dtype=torch.int32, device="cuda")
    ctx.sa_lcp_dev(text, sa, N, None, lcp2)
    assert torch.equal(lcp, lcp2)
    return inv, lcp


def test_inverse_lcp_at_the_plain_three_pass_threshold(gpu_ctx):
    """n = 2^23 - 2 (N = 2^23 - 1: the last plain inverse and Kasai chunks) and n = 2^23 - 1 (the first three-pass inverse
    and Phi), exactly against the oracle"""
    for n in ((1 << 23) - 2, (1 << 23) - 1):
        text, sa = _dna_sa(gpu_ctx, n, 17 + n)
        inv, lcp = _inverse_lcp_all_entries(gpu_ctx, text, sa, n)
        h_sa = sa.cpu().numpy().view(np.uint32)
        x = text.cpu().numpy()
        assert (inv.cpu().numpy().view(np.uint32) == oracle.inverse(h_sa)).all(), n
        assert (lcp.cpu().numpy().view(np.uint32) == oracle.lcp(x, h_sa)).all(), n


def test_inverse_lcp_around_2p28(gpu_ctx):
    """n = 2^28 - 1 (N = 2^28: the last size with coarse windows of 2^21) exactly against the oracle, and n = 2^28
    (N = 2^28 + 1: coarse windows of 2^22, the size the README quotes) by the device check"""
    import torch
    for n, exact in (((1 << 28) - 1, True), (1 << 28, False)):
        text, sa = _dna_sa(gpu_ctx, n, 28)
        inv, lcp = _inverse_lcp_all_entries(gpu_ctx, text, sa, n)
        gpu_ctx.trim()
        verify.verify_sa_on_device(text, sa, n)
        verify.verify_inverse_lcp_on_device(text, sa, inv, lcp, n)
        if exact:
            h_sa = sa.cpu().numpy().view(np.uint32)
            assert (inv.cpu().numpy().view(np.uint32) == oracle.inverse(h_sa)).all()
            assert (lcp.cpu().numpy().view(np.uint32) == oracle.lcp(text.cpu().numpy(), h_sa)).all()
        del text, sa, inv, lcp
        torch.cuda.empty_cache()


def test_lcp_of_a_long_repeat_text_at_2p28(gpu_ctx):
    """a 2^20-symbol random block repeated 256 times: from the second copy on every position shares a prefix of up to
    2^28 symbols with its neighbour, so every chunk takes plcp_kernel's long path and the samples carry huge values"""
    import torch
    n = 1 << 28
    block = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    gpu_ctx.synth_dev(block, 1 << 20, 5, 2028)
    text = block.repeat(n >> 20)
    torch.cuda.synchronize()  # (torch copies on its own stream; the library's stream does not wait for it)
    sa = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    gpu_ctx.sa_build_dev(text, n, 5, sa)
    inv, lcp = _inverse_lcp_all_entries(gpu_ctx, text, sa, n)
    gpu_ctx.trim()
    verify.verify_sa_on_device(text, sa, n)
    verify.verify_inverse_lcp_on_device(text, sa, inv, lcp, n)
    assert int((lcp.long() & 0xFFFFFFFF).max()) == n - (1 << 20)
    del text, sa, inv, lcp
    torch.cuda.empty_cache()


def _exact_on_device(ctx, ct, d_c, d_o, N, sigma, pats):
    import torch
    off = np.concatenate([[0], np.cumsum([p.size for p in pats])]).astype(np.uint32)
    flat = np.concatenate(pats).astype(np.uint8)
    d_pat = torch.from_numpy(flat).cuda()
    d_off = torch.from_numpy(off.view(np.int32)).cuda()
    d_l = torch.full((len(pats),), 7, dtype=torch.int32, device="cuda")
    d_r = torch.full((len(pats),), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()  # (the fills are on torch's stream)
    ctx.bwt_exact_search_dev(d_c, d_o, N, sigma, d_pat, d_off, len(pats), d_l, d_r)
    return d_l.cpu().numpy().view(np.uint32), d_r.cpu().numpy().view(np.uint32)


def test_exact_search_sigma_256(gpu_ctx):
    """a 2^20-symbol text over 255 symbols (the device builds O tables up to sigma = 128 only: these come from the oracle);
    the CPU harness's pattern set (lengths around the 16-symbol words and the text's length, invalid symbols at every
    position of a word), every (L, R) exact"""
    import torch
    rng = np.random.default_rng(256)
    n, sigma = 1 << 20, 256
    x = rng.integers(1, sigma, n).astype(np.uint8)
    x[700_000:900_000] = x[100_000:300_000]
    N = n + 1
    sa = oracle.sa_is(x, sigma)
    ct, ot = oracle.c_table(x, sigma), oracle.o_table(x, sa, sigma)
    d_c = torch.from_numpy(ct.view(np.int32)).cuda()
    d_o = torch.from_numpy(ot.view(np.int32).reshape(-1)).cuda()
    pats, want = exact_patterns(x, sigma, rng)
    l, r = _exact_on_device(gpu_ctx, ct, d_c, d_o, N, sigma, pats)
    for k, p in enumerate(pats):
        w = want[k] if want[k] is not None else oracle.bwt_exact_search(ct, ot, sigma, p)
        assert (int(l[k]), int(r[k])) == w, (k, p.size)


def test_exact_search_2p28_dna(gpu_ctx):
    """10^4 patterns (text substrings, mutated, random; 1 to 120 symbols) on the tables of 2^28 random DNA"""
    import torch
    n, sigma = 1 << 28, 5
    N = n + 1
    text, d_sa = _dna_sa(gpu_ctx, n, 4)
    d_c = torch.zeros(sigma, dtype=torch.int32, device="cuda")
    d_o = torch.empty((N + 1) * sigma, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gpu_ctx.bwt_tables_dev(text, d_sa, N, sigma, d_c, d_o)
    del d_sa
    ct = d_c.cpu().numpy().view(np.uint32)
    ot = np.ascontiguousarray(d_o.cpu().numpy().view(np.uint32).reshape(N + 1, sigma))  # (once: every oracle call uses it)
    rng = np.random.default_rng(28)
    starts = rng.integers(0, n - 200, 10_000)
    x = text.cpu().numpy()
    pats = []
    for q, a in enumerate(starts.tolist()):
        m = int(rng.integers(1, 121))
        p = x[a:a + m].copy() if q % 3 else rng.integers(1, sigma, m).astype(np.uint8)
        if q % 3 == 1:
            p[int(rng.integers(0, m))] = int(rng.integers(1, sigma))
        pats.append(p)
    l, r = _exact_on_device(gpu_ctx, ct, d_c, d_o, N, sigma, pats)
    for k, p in enumerate(pats):
        assert (int(l[k]), int(r[k])) == oracle.bwt_exact_search(ct, ot, sigma, p), (k, p.size)
    del text, d_c, d_o
    torch.cuda.empty_cache()


def _device_tables(ctx, sym, sigma):
    from test_gpu_approx import device_tables
    return device_tables(ctx, sym, sigma)


def _device_search(ctx, d_c, d_o, d_ro, N, sigma, pats, k):
    from test_gpu_approx import device_search
    off = np.concatenate([[0], np.cumsum([p.size for p in pats])]).astype(np.uint32)
    return device_search(ctx, d_c, d_o, d_ro, N, sigma, np.concatenate(pats).astype(np.uint8), off, k)


def test_approx_several_patterns_a_lane(gpu_ctx):
    """3 x 10^5 reads (more than the 2^18 lanes: lanes take several patterns each) on 2^24 DNA tables built on the device,
    made of 1000 planted reads repeated and shuffled, k = 1 and 2 with RO: every copy's hit records equal its original's,
    a sample of the originals' streams equal the model's, and a second run gives the same bytes"""
    import torch
    from test_gpu_approx import plant_reads
    rng = np.random.default_rng(2424)
    n, sigma = 1 << 24, 5
    x = synth(n, sigma, 24)
    d_sa, d_c, d_o, d_ro = _device_tables(gpu_ctx, x, sigma)
    distinct, _, _ = plant_reads(x, 1000, 100, 2, rng)
    order = rng.permutation(np.repeat(np.arange(1000), 300))
    pats = [distinct[q] for q in order]
    first = np.full(1000, -1)
    for i, q in enumerate(order):
        if first[q] < 0:
            first[q] = i
    sa = c = o = ro = None
    for k in (1, 2):
        hit_off, hits = _device_search(gpu_ctx, d_c, d_o, d_ro, n + 1, sigma, pats, k)
        hit_off2, hits2 = _device_search(gpu_ctx, d_c, d_o, d_ro, n + 1, sigma, pats, k)
        assert (hit_off == hit_off2).all() and hits.tobytes() == hits2.tobytes(), k
        counts = np.diff(hit_off).astype(np.int64)
        assert (hits["query"] == np.repeat(np.arange(len(pats)), counts)).all()
        assert (counts == counts[first[order]]).all(), k
        rec = hits.view(np.uint32).reshape(-1, 8)[:, 1:]
        starts = hit_off[:-1].astype(np.int64)
        for j in range(counts.max()):  # (the j-th record of every copy against the j-th of its original's first copy)
            has = counts > j
            assert (rec[starts[has] + j] == rec[starts[first[order[has]]] + j]).all(), (k, j)
        if sa is None:
            sa = d_sa.cpu().numpy().view(np.uint32)
            c = d_c.cpu().numpy().view(np.uint32)
            o = d_o.cpu().numpy().view(np.uint32).reshape(n + 2, sigma)
            ro = d_ro.cpu().numpy().view(np.uint32).reshape(n + 2, sigma)
        sample = rng.choice(1000, 40, replace=False)
        sel = [first[q] for q in sample]
        got = api.approx_matches(np.concatenate([hits[hit_off[i]:hit_off[i + 1]] for i in sel]),
                                 np.concatenate([[0], np.cumsum(counts[sel])]).astype(np.uint64), [pats[i].size for i in sel], sa)
        assert got == [approx_model.matches(c, o, ro, sa, distinct[q], k) for q in sample], k
    del d_sa, d_c, d_o, d_ro
    torch.cuda.empty_cache()


def test_approx_wide_alphabets_many_edits(gpu_ctx):
    """sigma = 21 and sigma = 256 (up to 511 children a node) with short patterns at k up to 8, with RO and without, against
    the model; sigma = 21 on device-built tables"""
    import torch
    rng = np.random.default_rng(821)
    for sigma, n, ks, lengths in ((21, 600, (0, 1, 3, 8), (1, 4)), (256, 2000, (0, 1, 2), (1, 5))):
        x = rng.integers(1, sigma, n).astype(np.uint8)
        sa, c, o, ro = approx_model.tables(x, sigma)
        if sigma <= 128:
            d_sa, d_c, d_o, d_ro = _device_tables(gpu_ctx, x, sigma)
            assert (d_sa.cpu().numpy().view(np.uint32) == sa).all() and (d_ro.cpu().numpy().view(np.uint32) == ro.reshape(-1)).all()
        else:  # (the device builds O tables up to sigma = 128 only)
            d_c, d_o, d_ro = (torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1)).cuda() for a in (c, o, ro))
        pats = []
        for _ in range(12):
            m = int(rng.integers(*lengths))
            a = int(rng.integers(0, n - m))
            p = x[a:a + m].copy()
            p[int(rng.integers(0, m))] = int(rng.integers(1, sigma))
            pats.append(p)
        for k in ks:
            if k >= 4:
                pats = pats[:3]  # (the model's search trees grow as sigma^k)
            for with_ro in (True, False):
                hit_off, hits = _device_search(gpu_ctx, d_c, d_o, d_ro if with_ro else None, n + 1, sigma, pats, k)
                got = api.approx_matches(hits, hit_off, [p.size for p in pats], sa)
                assert got == [approx_model.matches(c, o, ro if with_ro else None, sa, p, k) for p in pats], (sigma, k, with_ro)
