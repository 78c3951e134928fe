"""Best-stratum mapping through the CPU execution harness (tests/best_cases.py): sx_patterns_select_dev against a Python
list comprehension, sx_bwt_best_search_dev against the plain search at every edit count and against the search's Python
restatement (tests/approx_model.py), and the mapper's loop with SX_MAP_BEST_STRATUM against the text composed from the
reference mapper's recorded outputs at -d 0, 1, 2 (tests/golden/golden_sam_best.npz).

The harness builds the SAM kernels with a slice of 256 bytes a workgroup and the search with 256 lanes, so the rounds'
sets are larger than a launch here, too."""
import ctypes as C

import numpy as np
import pytest

import approx_model
import best_cases as bc
from approx_cases import approx_cases, remapped
from device_memory import HarnessMemory
from stralg_amd import _lib, api
from test_sam_cpu import records_of

MEM = HarnessMemory()


@pytest.fixture(scope="module")
def cases():
    return bc.best_cases()


def run(ctx, fasta, fastq, k, window=0, batch=0, both_strands=False, best=True):
    chunks = []
    ctx.set_sam_window_bytes(window)
    ctx.set_sam_batch_reads(batch)
    try:
        ctx.map_reads_stream(records_of(ctx, fasta), fastq, k, chunks.append, both_strands=both_strands, best=best)
    finally:
        ctx.set_sam_window_bytes(0)
        ctx.set_sam_batch_reads(0)
    return chunks


# ---- the fixture ----------------------------------------------------------------------------------------------------------
def test_fixture_has_every_outcome(cases):
    """20 reads at least of each outcome, one strand and both (what the generator asserted)"""
    c = cases["two-records-best"]
    for rev in (None, c["rev"]):
        strata = bc.strata_of(c["fastq"], c["fwd"], rev, 2)
        assert min(strata.count(e) for e in (0, 1, 2, None)) >= 20
    c = cases["hg38/reads-100-10-0"]
    strata = bc.strata_of(c["fastq"], c["fwd"], None, 1)
    assert (strata.count(0), strata.count(1)) == (51, 49)
    c = cases["test-out"]
    strata = bc.strata_of(c["fastq"], c["fwd"], None, 2)
    assert (strata.count(0), strata.count(None)) == (3, 1)


# ---- sx_patterns_select_dev -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.SELECT_NAMES)
def test_select(emu_ctx, name):
    bc.check_select(emu_ctx, MEM, bc.select_cases()[name])


def test_select_names_are_the_modules():
    assert list(bc.select_cases()) == bc.SELECT_NAMES


def test_select_with_offsets_that_descend(emu_ctx):
    """wrong bytes or SX_E_ARG, never an access outside the arrays (the harness's memory is the process's own)"""
    off = np.array([0, 40, 10, 30, 20], np.uint32)
    d_bytes, d_off, d_keep = MEM.to_dev(bytes(range(1, 41))), MEM.to_dev(off), MEM.to_dev(np.ones(4, np.uint8))
    d_out, d_off_out, d_ids = MEM.zeros(20 + 16), MEM.zeros(5, np.uint32), MEM.zeros(4, np.uint32)
    with pytest.raises(api.StralgAmdError, match="code -1"):
        emu_ctx.patterns_select_dev(d_bytes, d_off, 4, d_keep, d_out, d_off_out, d_ids)
    assert not MEM.to_host(d_out).any()


# ---- sx_bwt_best_search_dev -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def approx():
    return approx_cases()


@pytest.fixture(scope="module")
def tables(approx):
    out = {}
    for name, c in approx.items():
        sym, sigma = remapped(c["raw"])
        out[name] = approx_model.tables(sym, sigma) + (sigma,)
    return out


@pytest.mark.parametrize("k", [0, 1, 2])
def test_best_search_on_the_approx_fixture(emu_ctx, approx, tables, k):
    for name, cs in approx.items():
        sa, c, o, ro, sigma = tables[name]
        for r in (ro, None):
            T = bc.Tables(MEM, c, o, r, sigma, cs["pat"], cs["pat_off"])
            strata, ho, hits, per_d = bc.check_best_search(emu_ctx, T, k)
            # against the search's restatement at d = 0 .. k
            lens = np.diff(cs["pat_off"])
            got = api.approx_matches(hits, ho, lens, sa)
            for q, p in enumerate(cs["patterns"]):
                per = [approx_model.matches(c, o, r, sa, p, d) for d in range(k + 1)]
                e = next((d for d in range(k + 1) if per[d]), None)
                assert strata[q] == (0xFF if e is None else e), (name, q)
                assert got[q] == ([] if e is None else per[e]), (name, q)


def test_best_search_edge_patterns(emu_ctx, approx, tables):
    """an empty pattern, a symbol 0, a symbol the text lacks: 0xFF and no hits; max_edits < 0: all 0xFF"""
    sa, c, o, ro, sigma = tables["struct/binary-dups"]
    pats = [np.zeros(0, np.uint8), np.array([1, 0, 1], np.uint8), np.array([1, sigma], np.uint8), np.array([1, 2, 1], np.uint8)]
    off = np.array([0, 0, 3, 5, 8], np.uint32)
    T = bc.Tables(MEM, c, o, ro, sigma, np.concatenate(pats).astype(np.uint8), off)
    strata, ho, hits, _ = bc.check_best_search(emu_ctx, T, 2)
    assert strata.tolist()[:3] == [0xFF] * 3 and strata[3] == 0
    assert np.diff(ho).tolist()[:3] == [0, 0, 0] and (hits["query"] == 3).all()
    strata, ho, hits, failure = T.best(emu_ctx, -1)
    assert failure is None and strata.tolist() == [0xFF] * 4 and not ho.any() and hits.size == 0
    with pytest.raises(api.StralgAmdError, match="code -1"):
        emu_ctx.bwt_best_search_dev(T.c, T.o, T.ro, T.N, T.sigma, T.pat, T.off, 4, _lib.APPROX_MAX_EDITS + 1, MEM.zeros(4), MEM.zeros(5, np.uint64))


# ---- the loop -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,both", bc.BEST_PARAMS, ids=bc.BEST_IDS)
def test_cases_whole_text(emu_ctx, cases, name, k, both):
    c = cases[name]
    bc.check_text(b"".join(run(emu_ctx, c["fasta"], c["fastq"], k, both_strands=both)), bc.want_of(c, k, both))


@pytest.mark.parametrize("window", [16, 4096])
@pytest.mark.parametrize("batch", [1, 7, 33])
def test_batches_and_windows(emu_ctx, cases, batch, window):
    """odd batches: with both strands a batch still holds both strands of every read of it"""
    for name, k in (("two-records-best", 1), ("test-out", 2)):
        c = cases[name]
        for both in (False, True):
            chunks = run(emu_ctx, c["fasta"], c["fastq"], k, window=window, batch=batch, both_strands=both)
            assert max(len(x) for x in chunks) <= window
            bc.check_text(b"".join(chunks), bc.want_of(c, k, both))


def test_sampled_index(emu_ctx, cases):
    """a compact index with a sampled suffix array, its hits located in runs of at most 64 rows"""
    c = cases["two-records-best"]
    emu_ctx.set_locate_chunk_rows(64)
    try:
        with api.Index.from_fasta(c["fasta"], ctx=emu_ctx, compact=True, sa_sample=32) as idx:
            for both in (False, True):
                bc.check_text(idx.map_reads(c["fastq"], 2, both_strands=both, best=True), bc.want_of(c, 2, both))
            want = bc.want_of(c, 1, True)
            assert sum(n for _, n in idx.map_reads_discard(c["fastq"], 1, both_strands=True, best=True)) == len(want)
    finally:
        emu_ctx.set_locate_chunk_rows(0)


def test_best_at_no_edits_is_the_plain_text(emu_ctx, cases):
    c = cases["two-records-best"]
    for both in (False, True):
        best = b"".join(run(emu_ctx, c["fasta"], c["fastq"], 0, both_strands=both))
        plain = b"".join(run(emu_ctx, c["fasta"], c["fastq"], 0, both_strands=both, best=False))
        assert best == plain == bc.plain_of(c, 0, both)


def test_without_the_flag_nothing_changes(emu_ctx, cases):
    c = cases["two-records-best"]
    bc.check_text(b"".join(run(emu_ctx, c["fasta"], c["fastq"], 2, best=False)), c["fwd"][2])


def test_flags_word(emu_ctx, cases):
    """8 and 9 are accepted by the three places that take a flags word, 10 and 12 refused (2, 4 and 6 stay refused:
    tests/test_strands_cpu.py)"""
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
    limit = emu_ctx.lib.sx_map_reads_limit
    with api.Index.from_fasta(c["fasta"], ctx=emu_ctx) as idx:
        for flags in (8, 9):
            both = bool(flags & 1)
            del chunks[:]
            assert emu_ctx.lib.sx_map_reads_stream_ex(emu_ctx.h, recs, len(records), buf.ctypes.data, buf.size, 2, flags, cb, None) == 0
            bc.check_text(b"".join(chunks), bc.want_of(c, 2, both))
            del chunks[:]
            assert emu_ctx.lib.sx_index_map_reads_ex(emu_ctx.h, idx._handle(), buf.ctypes.data, buf.size, 2, flags, cb, None) == 0
            bc.check_text(b"".join(chunks), bc.want_of(c, 2, both))
            assert limit(5, 5, flags) == 0
        for flags in (10, 12):
            assert emu_ctx.lib.sx_map_reads_stream_ex(emu_ctx.h, recs, len(records), buf.ctypes.data, buf.size, 2, flags, cb, None) == _lib.SX_E_ARG
            assert emu_ctx.lib.sx_index_map_reads_ex(emu_ctx.h, idx._handle(), buf.ctypes.data, buf.size, 2, flags, cb, None) == _lib.SX_E_ARG
            assert limit(5, 5, flags) == _lib.SX_E_ARG
    # the limit is the plain call's: the flag does not change it
    assert limit(2 ** 32 - 1, 1, 8) == 0 and limit(2 ** 32, 1, 8) == _lib.SX_E_ARG
    assert limit(2 ** 31 - 1, 1, 9) == 0 and limit(2 ** 31, 1, 9) == _lib.SX_E_ARG
