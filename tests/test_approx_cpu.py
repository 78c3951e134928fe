"""The k-edit BWT search (sx_approx.hip) through the CPU execution harness, and its Python restatement
(tests/approx_model.py), against the reference iterator's streams in tests/golden/golden_approx.npz."""
import numpy as np
import pytest

import approx_model
from approx_cases import approx_cases, remapped
from stralg_amd import _lib, api


@pytest.fixture(scope="module")
def cases():
    return approx_cases()


@pytest.fixture(scope="module")
def tables(cases):
    """name -> (sa, c, o, ro, sigma) of build_complete_table(raw, true), from the oracle's restatement"""
    out = {}
    for name, c in cases.items():
        sym, sigma = remapped(c["raw"])
        out[name] = approx_model.tables(sym, sigma) + (sigma,)
    return out


def search(ctx, c, o, ro, sigma, pat, off, k, capacity=None):
    """the device entry, count then emit: (offsets, hits)"""
    count = off.size - 1
    hit_off = np.zeros(count + 1, np.uint64)
    pat = pat if pat.size else np.zeros(1, np.uint8)
    total = ctx.bwt_approx_search_dev(c, o, ro, o.shape[0] - 1, sigma, pat, off, count, k, hit_off)
    hits = np.zeros(max(total, 1), dtype=_lib.APPROX_HIT_DTYPE)
    again = ctx.bwt_approx_search_dev(c, o, ro, o.shape[0] - 1, sigma, pat, off, count, k, hit_off, hits,
                                      total if capacity is None else capacity)
    assert again == total
    return hit_off, hits[:total]


def test_fixture_streams_through_the_kernels(emu_ctx, cases, tables):
    for name, cs in cases.items():
        sa, c, o, ro, sigma = tables[name]
        for mode, r in (("ro", ro), ("noro", None)):
            hit_off, hits = search(emu_ctx, c, o, r, sigma, cs["pat"], cs["pat_off"], cs["k"])
            got = api.approx_matches(hits, hit_off, np.diff(cs["pat_off"]), sa)
            assert got == cs["streams"][mode], (name, mode)
            assert (hits["query"] == np.repeat(np.arange(hit_off.size - 1), np.diff(hit_off).astype(np.int64))).all()


def test_model_matches_fixture(cases, tables):
    for name, cs in cases.items():
        sa, c, o, ro, sigma = tables[name]
        for mode, r in (("ro", ro), ("noro", None)):
            got = [approx_model.matches(c, o, r, sa, p, cs["k"]) for p in cs["patterns"]]
            assert got == cs["streams"][mode], (name, mode)


def test_capacity_edges_and_limits(emu_ctx, cases, tables):
    name = "struct/binary-dups"
    sa, c, o, ro, sigma = tables[name]
    cs = cases[name]
    count = cs["pat_off"].size - 1
    hit_off = np.zeros(count + 1, np.uint64)
    total = emu_ctx.bwt_approx_search_dev(c, o, ro, o.shape[0] - 1, sigma, cs["pat"], cs["pat_off"], count, cs["k"], hit_off)
    assert total > 1000 and int(hit_off[-1]) == total
    # too small a buffer: SX_E_CAPACITY, the offsets and the total all the same, no hit written
    hits = np.zeros(total - 1, dtype=_lib.APPROX_HIT_DTYPE)
    hit_off[:] = 0
    with pytest.raises(api.StralgAmdError, match=str(_lib.SX_E_CAPACITY)):
        emu_ctx.bwt_approx_search_dev(c, o, ro, o.shape[0] - 1, sigma, cs["pat"], cs["pat_off"], count, cs["k"], hit_off, hits,
                                      total - 1)
    assert int(hit_off[-1]) == total and not hits.view(np.uint8).any()
    # no-hit edge cases: empty pattern, symbol 0, symbol >= sigma, max_edits < 0
    pats = [np.zeros(0, np.uint8), np.array([1, 0, 1], np.uint8), np.array([1, sigma], np.uint8), np.array([1, 2, 1], np.uint8)]
    flat = np.concatenate(pats).astype(np.uint8)
    off = np.array([0, 0, 3, 5, 8], np.uint32)
    h_off, h = search(emu_ctx, c, o, ro, sigma, flat, off, 2)
    n = np.diff(h_off)
    assert n[0] == 0 and n[1] == 0 and n[2] == 0 and n[3] > 0
    h_off, h = search(emu_ctx, c, o, ro, sigma, flat, off, -1)
    assert not h_off.any() and h.size == 0
    # beyond the limits: SX_E_ARG
    with pytest.raises(api.StralgAmdError, match=str(_lib.SX_E_ARG)):
        search(emu_ctx, c, o, ro, sigma, flat, off, _lib.APPROX_MAX_EDITS + 1)
    long = np.ones(1 << 15, np.uint8)
    with pytest.raises(api.StralgAmdError, match=str(_lib.SX_E_ARG)):
        search(emu_ctx, c, o, ro, sigma, long, np.array([0, long.size], np.uint32), 1)


def test_random_against_model(emu_ctx):
    """patterns of the text with planted edits, k up to 8 on short patterns, against the model"""
    rng = np.random.default_rng(11)
    for sigma, n in ((3, 400), (5, 3000), (9, 1500)):
        sym = rng.integers(1, sigma, n).astype(np.uint8)
        sa, c, o, ro = approx_model.tables(sym, sigma)
        for k in ((0, 1, 2, 3, 5, 8) if sigma == 3 else (0, 1, 2, 3)):
            pats = []
            for q in range(24):
                m = int(rng.integers(1, 4 if k >= 5 else 40))
                a = int(rng.integers(0, n - m))
                p = sym[a:a + m].copy()
                for _ in range(int(rng.integers(0, k + 1))):
                    p[int(rng.integers(0, m))] = int(rng.integers(1, sigma))
                pats.append(p)
            if k >= 5:
                pats = pats[:4]
            off = np.concatenate([[0], np.cumsum([p.size for p in pats])]).astype(np.uint32)
            flat = np.concatenate(pats).astype(np.uint8)
            for r in (ro, None):
                hit_off, hits = search(emu_ctx, c, o, r, sigma, flat, off, k)
                got = api.approx_matches(hits, hit_off, np.diff(off), sa)
                want = [approx_model.matches(c, o, r, sa, p, k) for p in pats]
                assert got == want, (sigma, k, r is None)


def test_host_entry_and_python_api(emu_ctx, cases, tables):
    """sx_bwt_approx_search (host buffers, staged through the context) and the module-level bwt_approx_search"""
    for name in ("ref/s3/k2", "rand/s5/n700/k2", "struct/runs", "genome/reads-100-100-2.fq/k2"):
        sa, c, o, ro, sigma = tables[name]
        cs = cases[name]
        for mode, r in (("ro", ro), ("noro", None)):
            hit_off, hits = emu_ctx.bwt_approx_search(c, o, r, sigma, cs["pat"], cs["pat_off"], cs["k"])
            assert api.approx_matches(hits, hit_off, np.diff(cs["pat_off"]), sa) == cs["streams"][mode], (name, mode)
            table = api.BwtTable(api.RemapTable(sigma, None, None), api.SuffixArray(None, sa), c, o, r)
            assert api.bwt_approx_search(table, cs["patterns"], cs["k"], ctx=emu_ctx) == cs["streams"][mode], (name, mode)
