"""Unmapped reads and the SAM header (SX_MAP_UNMAPPED, SX_MAP_HEADER) through the CPU execution harness
(tests/unmapped_cases.py): the oracle's own counts, the mapper against the oracle on the fixture cases, under the other flags,
in every form of the index, in batches, windows and a room of one hit, on reads that all fail to map, at a batch's edges, on
an empty FASTQ, on a fresh and a used context; the paired call with a header; the exported emitter over made-up hits.

The harness lays a slice of 256 bytes out in a workgroup, so FLAG 4 lines break across slices here at every size.  The
digest-only case (hg38/reads-100-10-0/k2) and the tool run on the GPU only (tests/test_gpu_unmapped.py)."""
import ctypes as C

import numpy as np
import pytest

import best_cases as bc
import pairs_cases as pc
import unmapped_cases as uc
from conftest import EMU_LIB
from device_memory import HarnessMemory
from stralg_amd import _lib, api
from test_sam_cpu import records_of

MEM = HarnessMemory()


@pytest.fixture(scope="module")
def cases():
    return uc.fixture_cases()


@pytest.fixture(scope="module")
def flag_cases():
    return bc.best_cases()


def stream(ctx, case, k, both=False, best=False, header=False, window=0, batch=0, room=0):
    """(text, map_stats) of map_reads_stream with SX_MAP_UNMAPPED and the switches set; every switch back at 0 behind it"""
    chunks = []
    ctx.set_sam_window_bytes(window)
    ctx.set_sam_batch_reads(batch)
    ctx.set_sam_room_hits(room)
    try:
        ctx.map_reads_stream(records_of(ctx, case["fasta"]), case["fastq"], k, chunks.append, both_strands=both, best=best, unmapped=True,
                             header=header)
        return chunks, ctx.map_stats()
    finally:
        ctx.set_sam_window_bytes(0)
        ctx.set_sam_batch_reads(0)
        ctx.set_sam_room_hits(0)


# ---- the oracle -------------------------------------------------------------------------------------------------------------
def test_oracle_counts(cases):
    uc.check_added(cases)


def test_oracle_on_reads_by_hand():
    fastq = b"@a\nACGT\n+\nIIII\n@b b\nGG\n+\n!#\n@c\nT\n+\n~\n"
    text = b"a\t0\tchr\t3\t0\t4M\t*\t0\t0\tACGT\tIIII\na\t16\tchr\t9\t0\t4M\t*\t0\t0\tACGT\tIIII\nc\t0\tchr\t1\t0\t1M\t*\t0\t0\tT\t~\n"
    got, n = uc.with_unmapped(fastq, text)
    assert n == 1 and got == text[:text.index(b"c\t")] + b"b b\t4\t*\t0\t0\t*\t*\t0\t0\tGG\t!#\n" + text[text.index(b"c\t"):]
    assert uc.header_of(b">left slice\nAC GT\nA\n>r\n\n") == b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:leftslice\tLN:5\n@SQ\tSN:r\tLN:0\n"


def test_header_names_and_lengths_are_the_index_records(emu_ctx, cases):
    """the oracle's @SQ fields against what the index holds: SN = the record's name (the lines' RNAME), LN = N - 1"""
    for key in (("test-out/k0", 0, False, False), ("two-records/k1", 1, False, False)):
        c = cases[key]
        n = C.c_uint32(0)
        with api.Index.from_fasta(c["fasta"], ctx=emu_ctx) as idx:
            assert emu_ctx.lib.sx_index_info(idx._handle(), C.byref(n), None, None, None) == 0
            got = [(idx.record_info(r).name, idx.record_info(r).N - 1) for r in range(n.value)]
        assert got == uc.fasta_sq(c["fasta"]), key


# ---- the fixture cases -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", uc.ADDED, ids=uc.ADDED_IDS)
@pytest.mark.parametrize("header", [False, True], ids=["text", "header"])
def test_fixture_cases(emu_ctx, cases, row, header):
    name, k, both, best, added = row
    c = cases[row[:4]]
    chunks, st = stream(emu_ctx, c, k, both, best, header)
    got = b"".join(chunks)
    bc.check_text(got, uc.want_of(c, header))
    if header:
        assert chunks[0] == uc.header_of(c["fasta"])  # (one sink call, in front of the first window)
    assert st["retries"] == 0


# ---- the other flags and the index forms --------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", uc.FLAG_SETS, ids=uc.FLAG_SET_IDS)
def test_with_the_other_flags(emu_ctx, flag_cases, flags):
    k, both, best, indels, tags = flags
    for name in ("test-out", "two-records-best"):
        c = flag_cases[name]
        with api.Index.from_fasta(c["fasta"], ctx=emu_ctx) as idx:
            for header in (False, True):
                got = idx.map_reads(c["fastq"], k, both_strands=both, best=best, indels=indels, tags=tags, unmapped=True, header=header)
                bc.check_text(got, uc.want_flags(c, k, both, best, indels, tags, header))


@pytest.mark.parametrize("form", [dict(), dict(compact=True), dict(compact=True, sa_sample=32), dict(compact=True, packed=True, sa_sample=32)],
                         ids=["full", "compact", "sampled", "packed-sampled"])
def test_index_forms(emu_ctx, cases, flag_cases, form):
    for key in (("test-out/k2", 2, False, False), ("two-records/k1", 1, False, False)):
        c = cases[key]
        with api.Index.from_fasta(c["fasta"], ctx=emu_ctx, **form) as idx:
            bc.check_text(idx.map_reads(c["fastq"], c["k"], unmapped=True, header=True), uc.want_of(c, True))
            bc.check_text(idx.map_reads(c["fastq"], c["k"]), c["plain"])  # (the plain call is what it was)
    c = flag_cases["two-records-best"]
    with api.Index.from_fasta(c["fasta"], ctx=emu_ctx, **form) as idx:
        got = idx.map_reads(c["fastq"], 2, both_strands=True, best=True, indels=False, tags=True, unmapped=True)
        bc.check_text(got, uc.want_flags(c, 2, True, True, False, True))
        assert sum(n for _, n in idx.map_reads_discard(c["fastq"], 2, both_strands=True, best=True, indels=False, tags=True, unmapped=True)) == len(got)


def test_sampled_index_located_in_runs_of_five(emu_ctx, cases, flag_cases):
    emu_ctx.set_locate_chunk_rows(5)
    try:
        c = cases[("two-records/k1", 1, False, False)]
        with api.Index.from_fasta(c["fasta"], ctx=emu_ctx, compact=True, sa_sample=16) as idx:
            bc.check_text(idx.map_reads(c["fastq"], 1, unmapped=True), uc.want_of(c))
        c = flag_cases["two-records-best"]
        with api.Index.from_fasta(c["fasta"], ctx=emu_ctx, compact=True, sa_sample=16) as idx:
            bc.check_text(idx.map_reads(c["fastq"], 1, both_strands=True, tags=True, unmapped=True), uc.want_flags(c, 1, True, False, True, True))
    finally:
        emu_ctx.set_locate_chunk_rows(0)


# ---- batches, windows, the room ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 3, 33])
def test_batches(emu_ctx, cases, flag_cases, batch):
    c = cases[("two-records/k1", 1, False, False)]
    chunks, st = stream(emu_ctx, c, 1, batch=batch, header=True)
    bc.check_text(b"".join(chunks), uc.want_of(c, True))
    assert st["batches"] == -(-200 // batch)
    c = flag_cases["two-records-best"]
    for best in (False, True):
        chunks, st = stream(emu_ctx, dict(c), 2, True, best, batch=batch)
        bc.check_text(b"".join(chunks), uc.want_flags(c, 2, True, best, True, False))


def test_sixteen_byte_windows(emu_ctx, cases):
    """windows of 16 bytes over two-records/k1, and over 16 unmapped reads whose FLAG 4 fields start at every offset of a
    window"""
    c = cases[("two-records/k1", 1, False, False)]
    want = uc.want_of(c)
    chunks, _ = stream(emu_ctx, c, 1, window=16)
    assert max(len(x) for x in chunks) <= 16
    bc.check_text(b"".join(chunks), want)
    # and over 16 unmapped reads whose lines have 33 bytes: line q's fields start at q + 8 modulo 16, every offset once
    reads = uc.fastq_reads(uc.all_unmapped_fastq(16, 3))
    fastq = uc.fastq_image([(b"n%07d" % q, s, qq) for q, (_, s, qq) in enumerate(reads)])  # (lines of 33 bytes)
    d = dict(c, fastq=fastq)
    chunks, _ = stream(emu_ctx, d, 1, window=16)
    text = b"".join(chunks)
    assert text == b"".join(uc.unmapped_line(r) for r in uc.fastq_reads(fastq))
    starts = {(text.index(uc.UNMAPPED_FIELDS, sum(len(uc.unmapped_line(r)) for r in uc.fastq_reads(fastq)[:q]))) % 16 for q in range(16)}
    assert len(starts) == 16, starts


def test_room_of_one_hit(emu_ctx, flag_cases):
    c = flag_cases["two-records-best"]
    for best in (False, True):
        chunks, st = stream(emu_ctx, c, 2, True, best, room=1, window=1000)
        assert st["retries"] > 0, st
        bc.check_text(b"".join(chunks), uc.want_flags(c, 2, True, best, True, False))


# ---- edges -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [dict(), dict(compact=True, sa_sample=32)], ids=["full", "sampled"])
def test_reads_that_all_fail_to_map(emu_ctx, cases, form):
    c = cases[("test-out/k2", 2, False, False)]
    fastq = uc.all_unmapped_fastq()
    want = b"".join(uc.unmapped_line(r) for r in uc.fastq_reads(fastq))
    with api.Index.from_fasta(c["fasta"], ctx=emu_ctx, **form) as idx:
        assert idx.map_reads(fastq, 2) == b""
        for batch in (0, 1):
            emu_ctx.set_sam_batch_reads(batch)
            try:
                for both in (False, True):
                    for best in (False, True):
                        assert idx.map_reads(fastq, 2, both_strands=both, best=best, unmapped=True) == want, (batch, both, best)
                st = emu_ctx.map_stats()
                assert st["batches"] == (40 if batch == 1 else 1)
            finally:
                emu_ctx.set_sam_batch_reads(0)


def test_first_and_last_read_of_a_batch(emu_ctx, cases):
    c = cases[("two-records/k1", 1, False, False)]
    fastq = uc.edges_fastq(c)
    d = dict(c, fastq=fastq)
    want, added = uc.with_unmapped(fastq, c["plain"])
    assert added == 12
    for batch in (0, 1, 2, 101, 102):
        chunks, _ = stream(emu_ctx, d, 1, batch=batch)
        bc.check_text(b"".join(chunks), want)


def test_empty_fastq(emu_ctx, cases):
    c = cases[("test-out/k1", 1, False, False)]
    records = records_of(emu_ctx, c["fasta"])
    for header in (False, True):
        chunks = []
        emu_ctx.map_reads_stream(records, b"", 1, chunks.append, unmapped=True, header=header)
        assert b"".join(chunks) == (uc.header_of(c["fasta"]) if header else b"")
    with api.Index.from_fasta(c["fasta"], ctx=emu_ctx) as idx:
        assert idx.map_reads(b"", 1, unmapped=True) == b""
        assert idx.map_reads(b"", 1, unmapped=True, header=True) == uc.header_of(c["fasta"])
        assert idx.map_reads(b"", 1, both_strands=True, header=True) == uc.header_of(c["fasta"])
        assert idx.map_pairs(b"", b"", 1, header=True) == uc.header_of(c["fasta"])
        assert idx.map_pairs(b"", b"", 1) == b""


def test_refused_calls_sink_nothing(emu_ctx, cases):
    c = cases[("test-out/k1", 1, False, False)]
    chunks = []

    def sink(user, section, data, n):
        chunks.append(C.string_at(data, n))
        return 0

    cb = _lib.SINK_FN(sink)
    buf = np.frombuffer(c["fastq"], np.uint8)
    lib, h = emu_ctx.lib, emu_ctx.h
    U, H = _lib.SX_MAP_UNMAPPED, _lib.SX_MAP_HEADER
    with api.Index.from_fasta(c["fasta"], ctx=emu_ctx) as idx, api.Index.from_tables(records_of(emu_ctx, c["fasta"]), ctx=emu_ctx) as bare:
        for flags in (H | 2, H | U | 4, H | 32, H | (1 << 9)):
            assert lib.sx_index_map_reads_ex(h, idx._handle(), buf.ctypes.data, buf.size, 1, flags, cb, None) == _lib.SX_E_ARG
        assert lib.sx_index_map_reads_ex(h, idx._handle(), buf.ctypes.data, buf.size, 9, H | U, cb, None) == _lib.SX_E_ARG
        assert lib.sx_index_map_reads_ex(h, bare._handle(), buf.ctypes.data, buf.size, 1, H | U | _lib.SX_MAP_TAGS, cb, None) == _lib.SX_E_ARG
        bad = np.frombuffer(b"@r\nACGT\n+\n", np.uint8)
        assert lib.sx_index_map_reads_ex(h, idx._handle(), bad.ctypes.data, bad.size, 1, H | U, cb, None) == _lib.SX_E_MALFORMED
        p = pc.pair_case(("test-out/k1", "overlap", 0, 500))
        for flags in (U, U | H, H | _lib.SX_MAP_TAGS):
            assert pc.raw_call(emu_ctx, idx, p["fastq1"], p["fastq2"], 1, 0, 500, flags) == (_lib.SX_E_ARG, b""), flags
        one_less = pc.sc.fastq_image(pc.sc.fastq_reads(p["fastq2"])[:-1])
        assert pc.raw_call(emu_ctx, idx, p["fastq1"], one_less, 1, 0, 500, H) == (_lib.SX_E_ARG, b"")
    assert not chunks
    limit = lib.sx_map_reads_limit
    assert limit(2 ** 32 - 1, 1, U | H) == 0 and limit(2 ** 32, 1, U | H) == _lib.SX_E_ARG
    assert limit(2 ** 31 - 1, 1, U | 1) == 0 and limit(2 ** 31, 1, U | 1) == _lib.SX_E_ARG
    assert (U, H) == (128, 256) and _lib.map_flags(unmapped=True, header=True) == 384 and _lib.pair_flags(header=True) == 256


# ---- the paired call with a header -------------------------------------------------------------------------------------------
def test_pairs_with_header(emu_ctx):
    p = pc.pair_case(("test-out/k1", "overlap", 0, 500))
    assert p["want"]
    with api.Index.from_fasta(p["fasta"], ctx=emu_ctx) as idx:
        got = idx.map_pairs(p["fastq1"], p["fastq2"], p["k"], p["lo"], p["hi"], header=True)
        assert got == uc.header_of(p["fasta"]) + p["want"]
        assert idx.map_pairs(p["fastq1"], p["fastq2"], p["k"], p["lo"], p["hi"]) == p["want"]
    assert api.map_pairs(p["fasta"], p["fastq1"], p["fastq2"], p["k"], p["lo"], p["hi"], ctx=emu_ctx, header=True) == got


# ---- the same bytes from call to call, the module-level call -----------------------------------------------------------------
def test_second_call_and_fresh_context(emu_ctx, flag_cases):
    c = flag_cases["two-records-best"]
    want = uc.want_flags(c, 1, True, True, True, False, True)
    with api.Index.from_fasta(c["fasta"], ctx=emu_ctx, compact=True, sa_sample=32) as idx:
        first = idx.map_reads(c["fastq"], 1, both_strands=True, best=True, unmapped=True, header=True)
        plain = idx.map_reads(c["fastq"], 1, both_strands=True, best=True)
        assert idx.map_reads(c["fastq"], 1, both_strands=True, best=True, unmapped=True, header=True) == first == want
        assert plain == bc.want_of(c, 1, True)
    fresh = api.Context(0, lib_path=EMU_LIB)
    try:
        fresh.set_small_direct_max(0)
        with api.Index.from_fasta(c["fasta"], ctx=fresh) as other:
            assert other.map_reads(c["fastq"], 1, both_strands=True, best=True, unmapped=True, header=True) == want
    finally:
        fresh.close()


def test_module_level_map_reads(emu_ctx, cases, flag_cases):
    c = cases[("test-out/k2", 2, False, False)]
    bc.check_text(api.map_reads(c["fasta"], c["fastq"], 2, ctx=emu_ctx, unmapped=True, header=True), uc.want_of(c, True))
    c = flag_cases["test-out"]
    bc.check_text(api.map_reads(c["fasta"], c["fastq"], 2, ctx=emu_ctx, both_strands=True, indels=False, tags=True, unmapped=True, header=True),
                  uc.want_flags(c, 2, True, False, False, True, True))


# ---- the exported emitter over made-up hits ---------------------------------------------------------------------------------
def test_emitter_made_up(emu_ctx):
    uc.check_made_up(emu_ctx, MEM, uc.made_up_case())


def test_emitter_made_up_holds_what_it_was_built_for():
    c = uc.made_up_case()
    text = uc.made_up_text(c, c["flags"])
    pos = [l.split(b"\t")[3] for l in text.split(b"\n")[:-1]]
    flags = [l.split(b"\t")[1] for l in text.split(b"\n")[:-1]]
    assert b"1" in pos and b"4294967295" in pos and flags[0] == b"4" and flags[-1] == b"4" and b"16" in flags
    assert flags.count(b"4") == 4
