"""The k-edit BWT search on the MI355X: the reference iterator's streams (tests/golden/golden_approx.npz) through
sx_bwt_approx_search_dev on tables built on the device and through stralg_amd_bwt_approx_batch, and a 2^26-symbol DNA
text with 10^5 reads against planted origins, the alignments themselves, the exact search, the model and the reference."""
import ctypes as C

import numpy as np
import pytest

import approx_model
import oracle
from approx_cases import approx_cases, cigar_ok, reference_matches, remapped
from stralg_amd import _lib, api, synth

pytestmark = pytest.mark.gpu


def dev(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a)
    if dtype is not None:
        a = a.view(dtype)
    return torch.from_numpy(a).cuda()


def device_tables(ctx, sym, sigma):
    """(d_sa, d_c, d_o, d_ro) built on the device by sa_build_dev / bwt_tables_dev / reverse_dev"""
    import torch
    n = sym.size
    N = n + 1
    d_text = dev(np.concatenate([sym, np.zeros(16, np.uint8)]))
    d_sa = torch.zeros(N, dtype=torch.int32, device="cuda")
    d_c = torch.zeros(sigma, dtype=torch.int32, device="cuda")
    d_o = torch.zeros((N + 1) * sigma, dtype=torch.int32, device="cuda")
    d_rev = torch.zeros(N + 16, dtype=torch.uint8, device="cuda")
    d_rsa = torch.zeros(N, dtype=torch.int32, device="cuda")
    d_c2 = torch.zeros_like(d_c)
    d_ro = torch.zeros_like(d_o)
    # (torch fills these on its own stream; the library's stream does not wait for it: a fill that ran late overwrote the
    #  reversed text the library had written)
    torch.cuda.synchronize()
    ctx.sa_build_dev(d_text, n, sigma, d_sa)
    ctx.bwt_tables_dev(d_text, d_sa, N, sigma, d_c, d_o)
    ctx.reverse_dev(d_text, n, d_rev)
    ctx.sa_build_dev(d_rev, n, sigma, d_rsa)
    ctx.bwt_tables_dev(d_rev, d_rsa, N, sigma, d_c2, d_ro)
    del d_rsa, d_c2, d_rev, d_text
    return d_sa, d_c, d_o, d_ro


def device_search(ctx, d_c, d_o, d_ro, N, sigma, pat, off, k):
    """count, then emit: (hit offsets, hits) on the host"""
    import torch
    count = off.size - 1
    d_pat = dev(np.concatenate([pat, np.zeros(16, np.uint8)]))
    d_off = dev(off, np.int32)
    d_hoff = torch.zeros(count + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()  # (the fill above is on torch's stream)
    total = ctx.bwt_approx_search_dev(d_c, d_o, d_ro, N, sigma, d_pat, d_off, count, k, d_hoff)
    d_hits = torch.zeros(max(total, 1) * 32, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert ctx.bwt_approx_search_dev(d_c, d_o, d_ro, N, sigma, d_pat, d_off, count, k, d_hoff, d_hits, total) == total
    hits = d_hits.cpu().numpy()[:total * 32].view(_lib.APPROX_HIT_DTYPE)
    return d_hoff.cpu().numpy().view(np.uint64), hits


def test_fixture_streams_on_device_tables(gpu_ctx):
    for name, cs in approx_cases().items():
        sym, sigma = remapped(cs["raw"])
        d_sa, d_c, d_o, d_ro = device_tables(gpu_ctx, sym, sigma)
        sa = d_sa.cpu().numpy().view(np.uint32)
        for mode, r in (("ro", d_ro), ("noro", None)):
            hoff, hits = device_search(gpu_ctx, d_c, d_o, r, sym.size + 1, sigma, cs["pat"], cs["pat_off"], cs["k"])
            got = api.approx_matches(hits, hoff, np.diff(cs["pat_off"]), sa)
            assert got == cs["streams"][mode], (name, mode)


def test_fixture_streams_through_the_c_batch(gpu_ctx):
    """stralg_amd_bwt_approx_batch on build_complete_table(raw, true), the caller's own entry points"""
    from oracle.pyoracle import _RefBwt

    class Match(C.Structure):
        _fields_ = [("position", C.c_uint32), ("match_length", C.c_uint32), ("cigar", C.c_char_p)]

    class Result(C.Structure):
        _fields_ = [("count", C.c_size_t), ("first", C.POINTER(C.c_size_t)), ("matches", C.POINTER(Match)),
                    ("cigars", C.c_void_p)]

    lib = C.CDLL(_lib.PRODUCT_LIB)
    lib.build_complete_table.argtypes = [C.c_char_p, C.c_bool]
    lib.build_complete_table.restype = C.POINTER(_RefBwt)
    lib.completely_free_bwt_table.argtypes = [C.POINTER(_RefBwt)]
    lib.stralg_amd_bwt_approx_batch.argtypes = [C.POINTER(_RefBwt), C.POINTER(C.c_char_p), C.c_size_t, C.c_int]
    lib.stralg_amd_bwt_approx_batch.restype = C.POINTER(Result)
    lib.stralg_amd_free_approx_result.argtypes = [C.POINTER(Result)]
    for name, cs in approx_cases().items():
        for include_reverse, mode in ((True, "ro"), (False, "noro")):
            t = lib.build_complete_table(cs["raw"], include_reverse)
            pats = (C.c_char_p * len(cs["patterns"]))(*[p.tobytes() for p in cs["patterns"]])
            r = lib.stralg_amd_bwt_approx_batch(t, pats, len(cs["patterns"]), cs["k"])
            assert r, name
            res = r.contents
            got = []
            for q in range(res.count):
                got.append([(res.matches[i].position, res.matches[i].match_length, res.matches[i].cigar.decode())
                            for i in range(res.first[q], res.first[q + 1])])
            lib.stralg_amd_free_approx_result(r)
            lib.completely_free_bwt_table(t)
            assert got == cs["streams"][mode], (name, mode)


def plant_reads(text, count, length, max_edits, rng):
    """reads of text[a : a + length] with up to max_edits substitutions / insertions / deletions inside (none in the
    first or last 10 symbols, so that the origin's alignment starts at a): (reads, origins, planted edits)"""
    starts = rng.integers(0, text.size - length - max_edits - 1, count)
    nedits = rng.integers(0, max_edits + 1, count)
    reads = []
    for a, ne in zip(starts.tolist(), nedits.tolist()):
        r = text[a:a + length].copy()
        for _ in range(ne):
            op, at = int(rng.integers(0, 3)), int(rng.integers(10, r.size - 10))
            if op == 0:
                r[at] = 1 + (int(r[at]) % 4)
            elif op == 1:
                r = np.delete(r, at)
            else:
                r = np.insert(r, at, int(rng.integers(1, 5)))
        reads.append(r.astype(np.uint8))
    return reads, starts, nedits


def test_dna_2p26_reads(gpu_ctx):
    import torch
    n, sigma = 1 << 26, 5
    text = synth(n, sigma, 2026)
    d_sa, d_c, d_o, d_ro = device_tables(gpu_ctx, text, sigma)
    N = n + 1
    rng = np.random.default_rng(26)
    reads, origins, planted = plant_reads(text, 100_000, 100, 2, rng)
    off = np.concatenate([[0], np.cumsum([r.size for r in reads])]).astype(np.uint32)
    flat = np.concatenate(reads).astype(np.uint8)
    sa = d_sa.cpu().numpy().view(np.uint32)
    c = d_c.cpu().numpy().view(np.uint32)
    o = d_o.cpu().numpy().view(np.uint32).reshape(N + 1, sigma)
    ro = d_ro.cpu().numpy().view(np.uint32).reshape(N + 1, sigma)
    # the exact search on the same patterns
    d_l = torch.zeros(len(reads), dtype=torch.int32, device="cuda")
    d_r = torch.zeros_like(d_l)
    torch.cuda.synchronize()  # (the fills are on torch's stream)
    gpu_ctx.bwt_exact_search_dev(d_c, d_o, N, sigma, dev(np.concatenate([flat, np.zeros(16, np.uint8)])), dev(off, np.int32),
                                 len(reads), d_l, d_r)
    ex_l, ex_r = d_l.cpu().numpy().view(np.uint32), d_r.cpu().numpy().view(np.uint32)
    sample = rng.choice(len(reads), 120, replace=False)
    for k in (0, 1, 2):
        hoff, hits = device_search(gpu_ctx, d_c, d_o, d_ro, N, sigma, flat, off, k)
        hoff2, hits2 = device_search(gpu_ctx, d_c, d_o, d_ro, N, sigma, flat, off, k)
        assert (hoff == hoff2).all() and hits.tobytes() == hits2.tobytes(), k  # the same bytes from run to run
        counts = np.diff(hoff).astype(np.int64)
        assert (hits["query"] == np.repeat(np.arange(len(reads)), counts)).all()
        if k == 0:  # one interval a read, the exact search's
            found = ex_l < ex_r
            assert (counts == found.astype(np.int64)).all()
            assert (hits["L"] == ex_l[found]).all() and (hits["R"] == ex_r[found]).all()
            assert (hits["n_gaps"] == 0).all() and (hits["match_length"] == np.diff(off)[found]).all()
        matches = api.approx_matches(hits, hoff, np.diff(off), sa)
        for q in range(len(reads)):
            if planted[q] <= k:
                assert int(origins[q]) in {pos for pos, _, _ in matches[q]}, (k, q)
            for pos, ml, cigar in matches[q]:
                assert cigar_ok(reads[q], text, pos, ml, cigar, k), (k, q, pos, ml, cigar)
        model = [approx_model.matches(c, o, ro, sa, reads[q], k) for q in sample]
        assert [matches[q] for q in sample] == model, k
        if oracle.have_ref():
            want = reference_matches(sa, c, o, ro, sigma, [reads[q] for q in sample[:40]], k)
            assert [matches[q] for q in sample[:40]] == want, k
