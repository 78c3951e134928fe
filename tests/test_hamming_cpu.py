"""The search without indels (SX_SEARCH_NO_INDELS, SX_MAP_NO_INDELS) through the CPU execution
harness (tests/hamming_cases.py): the search calls against the reference iterator's recorded streams with every entry
dropped whose CIGAR is not pure M, and against a sliding-window Hamming scan; the best-stratum search under the mode; the
mapper's loop against the reference mapper's recorded texts filtered the same way.

The harness runs the search with 256 lanes, so the fixture's pattern sets are larger than a launch here, too."""
import ctypes as C

import numpy as np
import pytest

import approx_model
import best_cases as bc
import hamming_cases as hc
from approx_cases import approx_cases, remapped
from device_memory import HarnessMemory
from stralg_amd import _lib, api
from test_sam_cpu import records_of

MEM = HarnessMemory()
APPROX = approx_cases()
NAMES = sorted(APPROX)


@pytest.fixture(scope="module")
def cases():
    return bc.best_cases()


@pytest.fixture(scope="module")
def tables():
    """name -> (sa, c, o, ro, sigma), made when first asked for"""
    made = {}

    def get(name):
        if name not in made:
            sym, sigma = remapped(APPROX[name]["raw"])
            made[name] = approx_model.tables(sym, sigma) + (sigma,)
        return made[name]
    return get


# ---- the guards: a filter that empties everything cannot hide a failure -------------------------------------------------------
def test_filtered_streams_hold_mismatches():
    assert APPROX["rand/s3/n3000/k1"]["k"] == 1 and hc.mismatches_in(APPROX["rand/s3/n3000/k1"]) == 91
    assert APPROX["struct/periodic-acgta"]["k"] == 2 and hc.mismatches_in(APPROX["struct/periodic-acgta"]) == 898
    assert APPROX["rand/s8/n60/k3"]["k"] == 3 and hc.mismatches_in(APPROX["rand/s8/n60/k3"]) == 168
    cs = APPROX["struct/all-a"]
    assert sum(len(hc.pure_stream(s, len(p))) for s, p in zip(cs["streams"]["ro"], cs["patterns"])) == 406 and hc.mismatches_in(cs) == 0


def test_filtered_texts_hold_lines(cases):
    assert hc.want_of(cases["two-records-best"], 2, False, False).count(b"\n") == 87
    assert hc.want_of(cases["hg38/reads-100-10-0"], 1, False, False).count(b"\n") == 4616
    assert [hc.pure_text(t).count(b"\n") for t in cases["two-records-best"]["fwd"]] == [34, 73, 87]
    assert [hc.pure_text(t).count(b"\n") for t in cases["two-records-best"]["rev"]] == [8, 18, 19]
    assert [hc.pure_text(t).count(b"\n") for t in cases["test-out"]["fwd"]] == [4, 13, 29]
    strata = bc.strata_of(cases["two-records-best"]["fastq"], [hc.pure_text(t) for t in cases["two-records-best"]["fwd"]], None, 2)
    assert [strata.count(e) for e in (0, 1, 2, None)] == [32, 38, 11, 159]


def test_filtered_streams_are_the_scan(tables):
    """the expected outputs themselves: the pure-M entries of every recorded stream are the scan's positions, each once"""
    for name in NAMES:
        cs = APPROX[name]
        sym, _ = remapped(cs["raw"])
        for mode in ("ro", "noro"):
            for p, s in zip(cs["patterns"], cs["streams"][mode]):
                pure = hc.pure_stream(s, len(p))
                assert sorted(pos for pos, _, _ in pure) == hc.brute(sym, p, cs["k"])[0], (name, mode)
                assert all(ml == len(p) for _, ml, _ in pure)


# ---- 1, 2: the fixture, in every form of the tables ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fixture_streams(emu_ctx, tables, name):
    want = hc.check_fixture_case(emu_ctx, MEM, APPROX[name], tables(name))
    sigma = tables(name)[4]
    assert hc.check_forms(emu_ctx, MEM, api.Index, APPROX[name], tables(name), want) == (sigma <= 128) + (sigma <= 8)


# ---- 3: random texts against the scan -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma,n", hc.RANDOM_SHAPES)
def test_random_against_the_scan(emu_ctx, sigma, n):
    hc.check_random(emu_ctx, MEM, sigma, n)


# ---- 4: edges -----------------------------------------------------------------------------------------------------------------
def test_no_edits_is_the_exact_search(emu_ctx, tables):
    for name in ("rand/s5/n700/k2", "struct/runs", "struct/all-a"):
        sa, c, o, ro, sigma = tables(name)
        cs = APPROX[name]
        T = hc.Tables(MEM, c, o, ro, sigma, cs["pat"], cs["pat_off"])
        ho, hits, failure = T.hamming(emu_ctx, 0)
        assert failure is None
        d_l, d_r = MEM.zeros(T.count, np.uint32), MEM.zeros(T.count, np.uint32)
        emu_ctx.bwt_exact_search_dev(T.c, T.o, T.N, sigma, T.pat, T.off, T.count, d_l, d_r)
        lo, hi = MEM.to_host(d_l, np.uint32), MEM.to_host(d_r, np.uint32)
        found = np.nonzero(lo < hi)[0]
        assert found.size and hits["query"].tolist() == found.tolist()
        assert hits["L"].tolist() == lo[found].tolist() and hits["R"].tolist() == hi[found].tolist()
        plain_ho, plain_hits = T.approx(emu_ctx, 0)
        assert ho.tolist() == plain_ho.tolist() and hits.tobytes() == plain_hits.tobytes()
        ho, hits, failure = T.hamming(emu_ctx, -1)
        assert failure is None and not ho.any() and hits.size == 0


def test_short_patterns(emu_ctx):
    """m = 1 at k = 0 and 1; k >= m (m = 3, k = 8, sigma = 3): every window of the text, each once"""
    rng = np.random.default_rng(5)
    sigma, n = 3, 400
    sym = rng.integers(1, sigma, n).astype(np.uint8)
    sa, c, o, ro = approx_model.tables(sym, sigma)
    pats = [np.array([1], np.uint8), np.array([2], np.uint8)]
    flat, off = hc.flat_of(pats)
    for k in (0, 1):
        for r in (ro, None):
            ho, hits, _ = hc.Tables(MEM, c, o, r, sigma, flat, off).hamming(emu_ctx, k)
            assert hc.positions_of(hits, ho, sa) == [hc.brute(sym, p, k)[0] for p in pats]
            hc.check_pure(hits, ho, [1, 1])
    assert hc.brute(sym, pats[0], 1)[0] == list(range(n))
    flat, off = hc.flat_of([np.array([1, 2, 1], np.uint8)])
    for r in (ro, None):
        ho, hits, _ = hc.Tables(MEM, c, o, r, sigma, flat, off).hamming(emu_ctx, 8)
        assert hc.positions_of(hits, ho, sa) == [list(range(n - 2))]
        hc.check_pure(hits, ho, [3])


def test_one_child_a_node(emu_ctx, tables):
    """sigma = 2: the only child is the exact one"""
    sa, c, o, ro, sigma = tables("struct/all-a")
    assert sigma == 2
    ho, hits = hc.check_fixture_case(emu_ctx, MEM, APPROX["struct/all-a"], tables("struct/all-a"))
    assert sum(int(h["R"]) - int(h["L"]) for h in hits) == 406


def test_capacity_edges_and_limits(emu_ctx, tables):
    name = "struct/periodic-acgta"
    sa, c, o, ro, sigma = tables(name)
    cs = APPROX[name]
    T = hc.Tables(MEM, c, o, ro, sigma, cs["pat"], cs["pat_off"])
    want_ho, want_hits, failure = T.hamming(emu_ctx, cs["k"])
    total = int(want_ho[-1])
    assert failure is None and total > 1  # (intervals: periodic text, many positions a hit)
    # too small a buffer: SX_E_CAPACITY, the offsets and the total all the same, no hit written
    hit_off = np.zeros(T.count + 1, np.uint64)
    hits = np.zeros(total - 1, dtype=_lib.APPROX_HIT_DTYPE)
    got = C.c_uint64(0)
    rc = emu_ctx.lib.sx_bwt_approx_search_dev_ex(emu_ctx.h, T.c.ctypes.data, T.o.ctypes.data, T.ro.ctypes.data, T.N, sigma, T.pat.ctypes.data,
                                                 T.off.ctypes.data, T.count, cs["k"], hit_off.ctypes.data, hits.ctypes.data, total - 1,
                                                 C.byref(got), _lib.SX_SEARCH_NO_INDELS)
    assert rc == _lib.SX_E_CAPACITY and got.value == total
    assert hit_off.tolist() == want_ho.tolist() and not hits.view(np.uint8).any()
    # patterns without hits: empty, symbol 0, symbol >= sigma
    pats = [np.zeros(0, np.uint8), np.array([1, 0, 1], np.uint8), np.array([1, sigma], np.uint8), np.array([1, 2, 1], np.uint8)]
    flat = np.concatenate(pats).astype(np.uint8)
    off = np.array([0, 0, 3, 5, 8], np.uint32)
    E = hc.Tables(MEM, c, o, ro, sigma, flat, off)
    ho, hits, _ = E.hamming(emu_ctx, 2)
    assert np.diff(ho).tolist()[:3] == [0, 0, 0] and ho[4] > ho[3] and (hits["query"] == 3).all()
    # beyond the limits: SX_E_ARG
    with pytest.raises(api.StralgAmdError, match="code -1"):
        E.hamming(emu_ctx, _lib.APPROX_MAX_EDITS + 1)
    long = np.ones(1 << 15, np.uint8)
    with pytest.raises(api.StralgAmdError, match="code -1"):
        hc.Tables(MEM, c, o, ro, sigma, long, np.array([0, long.size], np.uint32)).hamming(emu_ctx, 1)


def test_unknown_search_flags(emu_ctx, tables):
    """search_flags = 2: SX_E_ARG from every _ex call, nothing written"""
    sa, c, o, ro, sigma = tables("struct/runs")
    cs = APPROX["struct/runs"]
    T = hc.Tables(MEM, c, o, ro, sigma, cs["pat"], cs["pat_off"])
    lib, h = emu_ctx.lib, emu_ctx.h
    ho = np.zeros(T.count + 1, np.uint64)
    stratum = np.zeros(T.count, np.uint8)
    total, hp = C.c_uint64(0), C.c_void_p()
    head = (h, T.c.ctypes.data, T.o.ctypes.data, T.ro.ctypes.data, T.N, sigma, T.pat.ctypes.data, T.off.ctypes.data, T.count, 1)
    for flags in (2, 3, 1 << 31):
        assert lib.sx_bwt_approx_search_dev_ex(*head, ho.ctypes.data, None, 0, C.byref(total), flags) == _lib.SX_E_ARG
        assert lib.sx_bwt_approx_search_compact_dev_ex(*head, ho.ctypes.data, None, 0, C.byref(total), flags) == _lib.SX_E_ARG
        assert lib.sx_bwt_approx_search_packed_dev_ex(*head, ho.ctypes.data, None, 0, C.byref(total), flags) == _lib.SX_E_ARG
        assert lib.sx_bwt_best_search_dev_ex(*head, stratum.ctypes.data, ho.ctypes.data, None, 0, C.byref(total), flags) == _lib.SX_E_ARG
        assert lib.sx_bwt_approx_search_ex(h, c.ctypes.data, o.ctypes.data, ro.ctypes.data, T.N, sigma, cs["pat"].ctypes.data, cs["pat_off"].ctypes.data,
                                           T.count, 1, ho.ctypes.data, C.byref(hp), C.byref(total), flags) == _lib.SX_E_ARG
    assert not ho.any() and not stratum.any() and total.value == 0 and not hp.value
    # and the flags that exist
    assert lib.sx_bwt_approx_search_dev_ex(*head, ho.ctypes.data, None, 0, C.byref(total), 0) == 0
    plain = total.value
    assert lib.sx_bwt_approx_search_dev_ex(*head, ho.ctypes.data, None, 0, C.byref(total), 1) == 0
    assert 0 < total.value < plain


# ---- 5: best stratum ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_best_search(emu_ctx, tables, name):
    hc.check_best(emu_ctx, MEM, APPROX[name], tables(name))


# ---- 6: the host-buffer entry and the module-level call -----------------------------------------------------------------------
def test_host_entry_and_python_api(emu_ctx, tables):
    for name in ("rand/s5/n700/k2", "struct/runs"):
        sa, c, o, ro, sigma = tables(name)
        cs = APPROX[name]
        for mode, r in (("ro", ro), ("noro", None)):
            want = [hc.pure_stream(s, len(p)) for s, p in zip(cs["streams"][mode], cs["patterns"])]
            hit_off, hits = emu_ctx.bwt_approx_search(c, o, r, sigma, cs["pat"], cs["pat_off"], cs["k"], indels=False)
            assert api.approx_matches(hits, hit_off, np.diff(cs["pat_off"]), sa) == want, (name, mode)
            hc.check_pure(hits, hit_off, np.diff(cs["pat_off"]))
            table = api.BwtTable(api.RemapTable(sigma, None, None), api.SuffixArray(None, sa), c, o, r)
            assert api.bwt_approx_search(table, cs["patterns"], cs["k"], ctx=emu_ctx, indels=False) == want, (name, mode)
            assert api.bwt_approx_search(table, cs["patterns"], cs["k"], ctx=emu_ctx) == cs["streams"][mode], (name, mode)


# ---- 7: the mapper ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,both,best", hc.MAP_PARAMS, ids=hc.MAP_IDS)
def test_cases_whole_text(emu_ctx, cases, name, k, both, best):
    c = cases[name]
    chunks, st = hc.stream(emu_ctx, records_of(emu_ctx, c["fasta"]), c["fastq"], k, both, best)
    bc.check_text(b"".join(chunks), hc.want_of(c, k, both, best))
    assert st["retries"] == 0


def test_module_level_map_reads(emu_ctx, cases):
    c = cases["test-out"]
    for both in (False, True):
        for best in (False, True):
            bc.check_text(api.map_reads(c["fasta"], c["fastq"], 2, ctx=emu_ctx, both_strands=both, best=best, indels=False),
                          hc.want_of(c, 2, both, best))


@pytest.mark.parametrize("form", hc.FORMS, ids=hc.FORM_IDS)
def test_index_forms(emu_ctx, cases, form):
    hc.check_index_forms(emu_ctx, api.Index, cases["two-records-best"], form)


def test_no_edits_with_the_flag_is_the_plain_text(emu_ctx, cases):
    c = cases["two-records-best"]
    records = records_of(emu_ctx, c["fasta"])
    for both in (False, True):
        for best in (False, True):
            got = b"".join(hc.stream(emu_ctx, records, c["fastq"], 0, both, best)[0])
            assert got == b"".join(hc.stream(emu_ctx, records, c["fastq"], 0, both, False, indels=True)[0]) == bc.plain_of(c, 0, both)


def test_without_the_flag_nothing_changes(emu_ctx, cases):
    """the same index, mapped with the flag and then without it"""
    c = cases["two-records-best"]
    with api.Index.from_fasta(c["fasta"], ctx=emu_ctx) as idx:
        bc.check_text(idx.map_reads(c["fastq"], 2, indels=False), hc.want_of(c, 2, False, False))
        bc.check_text(idx.map_reads(c["fastq"], 2), c["fwd"][2])
        bc.check_text(idx.map_reads(c["fastq"], 2, both_strands=True, best=True), bc.want_of(c, 2, True))


# ---- 8: the flags word --------------------------------------------------------------------------------------------------------
def test_flags_word(emu_ctx, cases):
    """16, 17, 24 and 25 are accepted by the places that take a flags word; 2, 4, 18, 20, 22 and 32 are refused"""
    c = cases["test-out"]
    recs = (_lib.MapRecord * 8)()
    keep = []
    records = records_of(emu_ctx, c["fasta"])
    for r, (rname, t) in enumerate(records):
        recs[r] = api._map_record(rname, t, keep)
    chunks = []

    def sink(user, section, data, n):
        chunks.append(C.string_at(data, n))
        return 0

    cb = _lib.SINK_FN(sink)
    buf = np.frombuffer(c["fastq"], np.uint8)
    lib, h = emu_ctx.lib, emu_ctx.h
    limit = lib.sx_map_reads_limit
    with api.Index.from_fasta(c["fasta"], ctx=emu_ctx) as idx:
        for flags in (16, 17, 24, 25):
            both, best = bool(flags & 1), bool(flags & 8)
            assert flags == _lib.map_flags(both, best, indels=False)
            del chunks[:]
            assert lib.sx_map_reads_stream_ex(h, recs, len(records), buf.ctypes.data, buf.size, 2, flags, cb, None) == 0
            bc.check_text(b"".join(chunks), hc.want_of(c, 2, both, best))
            del chunks[:]
            assert lib.sx_index_map_reads_ex(h, idx._handle(), buf.ctypes.data, buf.size, 2, flags, cb, None) == 0
            bc.check_text(b"".join(chunks), hc.want_of(c, 2, both, best))
            assert limit(5, 5, flags) == 0
        del chunks[:]
        for flags in (2, 4, 18, 20, 22, 32):
            assert lib.sx_map_reads_stream_ex(h, recs, len(records), buf.ctypes.data, buf.size, 2, flags, cb, None) == _lib.SX_E_ARG
            assert lib.sx_index_map_reads_ex(h, idx._handle(), buf.ctypes.data, buf.size, 2, flags, cb, None) == _lib.SX_E_ARG
            assert limit(5, 5, flags) == _lib.SX_E_ARG
        assert not chunks
    # the limit is the plain call's: the flag does not change it
    assert limit(2 ** 32 - 1, 1, 16) == 0 and limit(2 ** 32, 1, 16) == _lib.SX_E_ARG
    assert limit(2 ** 31 - 1, 1, 17) == 0 and limit(2 ** 31, 1, 17) == _lib.SX_E_ARG
    assert (_lib.SX_MAP_NO_INDELS, _lib.SX_SEARCH_NO_INDELS) == (16, 1)


# ---- 9: windows and batches, in a room that has to grow -----------------------------------------------------------------------
@pytest.mark.parametrize("window,batch", hc.WINDOWS)
def test_windows_and_batches(emu_ctx, cases, window, batch):
    c = cases["two-records-best"]
    hc.check_windows(emu_ctx, records_of(emu_ctx, c["fasta"]), c, window, batch)
