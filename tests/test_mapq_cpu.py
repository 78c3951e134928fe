"""MAPQ and secondary lines from the best stratum (SX_MAP_MAPQ) through the CPU execution harness
(tests/mapq_cases.py): the oracle's own counts, the mapper against the oracle on the table's cases, under the other flags, in
every form of the index, in batches, windows and a room of one hit, at a batch's edges, on an empty FASTQ, on a fresh and a
used context; the refusals; the exported emitter over made-up hits.

The harness lays a slice of 256 bytes out in a workgroup, so lines break across slices here at every size.  The tool and the
case at size run on the GPU only (tests/test_gpu_mapq.py)."""
import ctypes as C

import numpy as np
import pytest

import best_cases as bc
import mapq_cases as mc
import pairs_cases as pc
import unmapped_cases as uc
from conftest import EMU_LIB
from device_memory import HarnessMemory
from stralg_amd import _lib, api
from test_sam_cpu import records_of

MEM = HarnessMemory()


@pytest.fixture(scope="module")
def cases():
    return bc.best_cases()


def stream(ctx, case, k, both=False, indels=True, unmapped=False, header=False, window=0, batch=0, room=0):
    """(chunks, map_stats) of map_reads_stream with best and SX_MAP_MAPQ and the switches set; every switch back at 0 behind it"""
    chunks = []
    ctx.set_sam_window_bytes(window)
    ctx.set_sam_batch_reads(batch)
    ctx.set_sam_room_hits(room)
    try:
        ctx.map_reads_stream(records_of(ctx, case["fasta"]), case["fastq"], k, chunks.append, both_strands=both, best=True, indels=indels,
                             unmapped=unmapped, header=header, mapq=True)
        return chunks, ctx.map_stats()
    finally:
        ctx.set_sam_window_bytes(0)
        ctx.set_sam_batch_reads(0)
        ctx.set_sam_room_hits(0)


# ---- the oracle -------------------------------------------------------------------------------------------------------------
def test_oracle_counts(cases):
    mc.check_table(cases)


def test_oracle_on_reads_by_hand():
    fastq = b"@a\nACGT\n+\nIIII\n@b b\nGG\n+\n!#\n@c\nT\n+\n~\n@d\nA\n+\n!\n"
    line = b"%s\t%d\tchr\t%d\t%d\t4M\t*\t0\t0\tACGT\tIIII\n"
    text = (b"@HD\tVN:1.6\tSO:unsorted\n" + line % (b"a", 0, 3, 0) + line % (b"a", 16, 9, 0) + b"b b\t4\t*\t0\t0\t*\t*\t0\t0\tGG\t!#\n" +
            line % (b"c", 16, 1, 0) + b"".join(line % (b"d", 0, p, 0) for p in range(5)))
    want = (b"@HD\tVN:1.6\tSO:unsorted\n" + line % (b"a", 0, 3, 3) + line % (b"a", 272, 9, 3) + b"b b\t4\t*\t0\t0\t*\t*\t0\t0\tGG\t!#\n" +
            line % (b"c", 16, 1, 50) + line % (b"d", 0, 0, 0) + b"".join(line % (b"d", 256, p, 0) for p in range(1, 5)))
    got, n = mc.with_mapq(fastq, text)
    assert got == want and mc.without_mapq(got) == text
    assert (n["lines"], n["secondary"], n["first16"], n["groups"]) == (8, 5, 1, {50: 1, 3: 1, 1: 0, 0: 1})
    assert [mc.mapq_of(n) for n in (1, 2, 3, 4, 5, 6, 7600)] == [50, 3, 1, 1, 0, 0, 0]


# ---- the table's cases ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", mc.TABLE, ids=mc.TABLE_IDS)
def test_table_cases(emu_ctx, cases, row):
    name, k, both, indels = row[:4]
    c = cases[name]
    chunks, st = stream(emu_ctx, c, k, both, indels)
    bc.check_text(b"".join(chunks), mc.want_of(c, k, both, indels))
    assert st["retries"] == 0


# ---- the other flags and the index forms --------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", mc.FLAG_SETS, ids=mc.FLAG_SET_IDS)
def test_with_the_other_flags(emu_ctx, cases, flags):
    tags, unmapped, header, indels = flags
    c = cases["two-records-best"]
    with api.Index.from_fasta(c["fasta"], ctx=emu_ctx) as idx:
        got = idx.map_reads(c["fastq"], 2, both_strands=True, best=True, indels=indels, tags=tags, unmapped=unmapped, header=header, mapq=True)
        bc.check_text(got, mc.want_of(c, 2, True, indels, tags, unmapped, header))
        # (the same call without the bit is what it was)
        plain = idx.map_reads(c["fastq"], 2, both_strands=True, best=True, indels=indels, tags=tags, unmapped=unmapped, header=header)
        bc.check_text(plain, mc.plain_of(c, 2, True, indels, tags, unmapped, header))
        seen = idx.map_reads_discard(c["fastq"], 2, both_strands=True, best=True, indels=indels, tags=tags, unmapped=unmapped, header=header, mapq=True)
        assert sum(n for _, n in seen) == len(got)


@pytest.mark.parametrize("form", mc.FORMS, ids=mc.FORM_IDS)
def test_index_forms(emu_ctx, cases, form):
    c = cases["two-records-best"]
    with api.Index.from_fasta(c["fasta"], ctx=emu_ctx, **form) as idx:
        bc.check_text(idx.map_reads(c["fastq"], 1, best=True, mapq=True), mc.want_of(c, 1, False))
        got = idx.map_reads(c["fastq"], 2, both_strands=True, best=True, indels=False, tags=True, unmapped=True, header=True, mapq=True)
        bc.check_text(got, mc.want_of(c, 2, True, False, True, True, True))
    c = cases["test-out"]
    with api.Index.from_fasta(c["fasta"], ctx=emu_ctx, **form) as idx:
        bc.check_text(idx.map_reads(c["fastq"], 2, both_strands=True, best=True, mapq=True), mc.want_of(c, 2, True))


def test_sampled_index_located_in_runs_of_five(emu_ctx, cases):
    emu_ctx.set_locate_chunk_rows(5)
    try:
        c = cases["two-records-best"]
        with api.Index.from_fasta(c["fasta"], ctx=emu_ctx, compact=True, sa_sample=16) as idx:
            bc.check_text(idx.map_reads(c["fastq"], 1, best=True, mapq=True), mc.want_of(c, 1, False))
            got = idx.map_reads(c["fastq"], 2, both_strands=True, best=True, tags=True, unmapped=True, mapq=True)
            bc.check_text(got, mc.want_of(c, 2, True, True, True, True))
    finally:
        emu_ctx.set_locate_chunk_rows(0)


# ---- batches, windows, the room ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 3, 33])
def test_batches(emu_ctx, cases, batch):
    c = cases["two-records-best"]
    for both, unmapped in ((False, False), (True, True)):
        chunks, st = stream(emu_ctx, c, 2, both, unmapped=unmapped, header=True, batch=batch)
        bc.check_text(b"".join(chunks), mc.want_of(c, 2, both, unmapped=unmapped, header=True))
        # (a batch counts the reads of the search: with both strands two a read, and an odd number is rounded up to whole groups)
        assert st["batches"] == (-(-2 * 240 // (batch + batch % 2)) if both else -(-240 // batch))


def test_sixteen_byte_windows(emu_ctx, cases):
    c = cases["two-records-best"]
    chunks, _ = stream(emu_ctx, c, 1, True, window=16)
    assert max(len(x) for x in chunks) <= 16
    bc.check_text(b"".join(chunks), mc.want_of(c, 1, True))


def test_room_of_one_hit(emu_ctx, cases):
    """every batch is halved down to a group, which then gets what it needs"""
    c = cases["two-records-best"]
    for unmapped in (False, True):
        chunks, st = stream(emu_ctx, c, 2, True, unmapped=unmapped, room=1, window=1000)
        assert st["retries"] > 0 and st["halved"] > 0, st
        bc.check_text(b"".join(chunks), mc.want_of(c, 2, True, unmapped=unmapped))


# ---- edges -------------------------------------------------------------------------------------------------------------------
def test_unmapped_reads_first_middle_and_last(emu_ctx, cases):
    c = cases["two-records-best"]
    fastq = mc.edges_fastq(c)
    plain, added = uc.with_unmapped(fastq, bc.want_of(c, 1, True))
    want, n = mc.with_mapq(fastq, plain)
    assert added >= 3 and want.startswith(b"first-lost\t4\t") and want.split(b"\n")[-2].startswith(b"last-lost\t4\t") and n["secondary"] > 0
    for batch in (0, 1, 2, 3):
        chunks, _ = stream(emu_ctx, dict(c, fastq=fastq), 1, True, unmapped=True, batch=batch)
        bc.check_text(b"".join(chunks), want)


def test_empty_fastq(emu_ctx, cases):
    c = cases["test-out"]
    records = records_of(emu_ctx, c["fasta"])
    for header in (False, True):
        chunks = []
        emu_ctx.map_reads_stream(records, b"", 1, chunks.append, best=True, unmapped=True, header=header, mapq=True)
        assert b"".join(chunks) == (uc.header_of(c["fasta"]) if header else b"")
    with api.Index.from_fasta(c["fasta"], ctx=emu_ctx) as idx:
        assert idx.map_reads(b"", 1, best=True, mapq=True) == b""
        assert idx.map_reads(b"", 1, best=True, header=True, mapq=True) == uc.header_of(c["fasta"])


def test_second_call_and_fresh_context(emu_ctx, cases):
    c = cases["two-records-best"]
    want = mc.want_of(c, 1, True, unmapped=True, header=True)
    with api.Index.from_fasta(c["fasta"], ctx=emu_ctx, compact=True, sa_sample=32) as idx:
        first = idx.map_reads(c["fastq"], 1, both_strands=True, best=True, unmapped=True, header=True, mapq=True)
        assert idx.map_reads(c["fastq"], 1, both_strands=True, best=True) == bc.want_of(c, 1, True)
        assert idx.map_reads(c["fastq"], 1, both_strands=True, best=True, unmapped=True, header=True, mapq=True) == first == want
    fresh = api.Context(0, lib_path=EMU_LIB)
    try:
        fresh.set_small_direct_max(0)
        with api.Index.from_fasta(c["fasta"], ctx=fresh) as other:
            assert other.map_reads(c["fastq"], 1, both_strands=True, best=True, unmapped=True, header=True, mapq=True) == want
    finally:
        fresh.close()


def test_module_level_map_reads(emu_ctx, cases):
    c = cases["test-out"]
    bc.check_text(api.map_reads(c["fasta"], c["fastq"], 2, ctx=emu_ctx, both_strands=True, best=True, mapq=True), mc.want_of(c, 2, True))
    got = api.map_reads(c["fasta"], c["fastq"], 2, ctx=emu_ctx, both_strands=True, best=True, indels=False, tags=True, unmapped=True, header=True,
                        mapq=True)
    bc.check_text(got, mc.want_of(c, 2, True, False, True, True, True))


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refused_calls_sink_nothing(emu_ctx, cases):
    c = cases["test-out"]
    chunks = []

    def sink(user, section, data, n):
        chunks.append(C.string_at(data, n))
        return 0

    cb = _lib.SINK_FN(sink)
    buf = np.frombuffer(c["fastq"], np.uint8)
    lib, h = emu_ctx.lib, emu_ctx.h
    Q, H, B = _lib.SX_MAP_MAPQ, _lib.SX_MAP_HEADER, _lib.SX_MAP_BEST_STRATUM
    assert Q == 1024 and _lib.map_flags(best=True, mapq=True) == 1032 and _lib.map_flags(unmapped=True, header=True) == 384
    records = records_of(emu_ctx, c["fasta"])
    recs = (_lib.MapRecord * len(records))()
    keep = []
    for r, (name, t) in enumerate(records):
        recs[r] = api._map_record(name, t, keep)
    with api.Index.from_fasta(c["fasta"], ctx=emu_ctx) as idx:
        for flags in (Q, H | Q, Q | _lib.SX_MAP_BOTH_STRANDS | _lib.SX_MAP_UNMAPPED | H, Q | B | (1 << 9)):
            assert lib.sx_index_map_reads_ex(h, idx._handle(), buf.ctypes.data, buf.size, 1, flags, cb, None) == _lib.SX_E_ARG, flags
            assert lib.sx_map_reads_stream_ex(h, recs, len(records), buf.ctypes.data, buf.size, 1, flags, cb, None) == _lib.SX_E_ARG, flags
        assert lib.sx_index_map_reads_ex(h, idx._handle(), buf.ctypes.data, buf.size, 1, Q, cb, None) == _lib.SX_E_ARG
        assert b"SX_MAP_BEST_STRATUM" in lib.sx_last_error(h)
        with pytest.raises(api.StralgAmdError):
            idx.map_reads(c["fastq"], 1, mapq=True, header=True, sink=chunks.append)
        p = pc.pair_case(("test-out/k1", "overlap", 0, 500))
        for flags in (Q, Q | B, Q | B | H):
            assert pc.raw_call(emu_ctx, idx, p["fastq1"], p["fastq2"], 1, 0, 500, flags) == (_lib.SX_E_ARG, b""), flags
    assert not chunks
    limit = lib.sx_map_reads_limit
    for n, other in ((2 ** 32 - 1, B), (2 ** 32, B), (2 ** 31 - 1, B | 1), (2 ** 31, B | 1)):
        assert limit(n, 1, other | Q) == limit(n, 1, other)
    assert limit(2 ** 32 - 1, 1, B | Q) == 0 and limit(2 ** 31, 1, B | Q | 1) == _lib.SX_E_ARG and limit(1, 1, Q | 512) == _lib.SX_E_ARG


# ---- the exported emitter over made-up hits ---------------------------------------------------------------------------------
@pytest.mark.parametrize("with_flags", [False, True], ids=["no-flags", "flags"])
def test_emitter_small(emu_ctx, with_flags):
    """every quality word, placeholders first and last, POS of 1 and 10 digits; windows of 16 bytes; a cut at every offset
    from FLAG to MAPQ of a line with three digits in both"""
    case = mc.small_case()
    flags = case["flags"] if with_flags else None
    b, want = mc.check_emitter(emu_ctx, MEM, case, flags, sixteen=True)
    fields = [l.split(b"\t") for l in want.split(b"\n")[:-1]]
    assert fields[0][1] == b"4" and fields[-1][1] == b"4" and sum(f[1] == b"4" for f in fields) == 4
    assert {f[4] for f in fields} >= {b"50", b"3", b"0", b"255"} and {f[3] for f in fields} >= {b"1", b"4294967295"}
    needle = b"272" if with_flags else b"256"
    assert mc.check_cuts(b, want, needle) >= 9
    located, _ = mc.check_emitter(emu_ctx, MEM, case, flags, located=True, sixteen=True)
    assert located.text() == want


@pytest.mark.parametrize("with_flags", [False, True], ids=["no-flags", "flags"])
@pytest.mark.parametrize("located", [False, True], ids=["rows", "located"])
def test_emitter_intervals(emu_ctx, with_flags, located):
    case = mc.interval_case()
    _, want = mc.check_emitter(emu_ctx, MEM, case, case["flags"] if with_flags else None, located)
    flags = {l.split(b"\t")[1] for l in want.split(b"\n")[:-1]}
    assert flags == ({b"0", b"16", b"256", b"272", b"4"} if with_flags else {b"0", b"256", b"4"})
    assert {l.split(b"\t")[4] for l in want.split(b"\n")[:-1]} == {b"50", b"3", b"1", b"0", b"255"}


@pytest.mark.parametrize("located", [False, True], ids=["rows", "located"])
def test_emitter_tagged(emu_ctx, located):
    case = mc.tagged_case()
    for flags in (None, case["flags"]):
        _, want = mc.check_emitter(emu_ctx, MEM, case, flags, located)
        assert b"\tNM:i:" in want and want.count(b"\t4\t*\t0\t0\t*\t*\t0\t0\t") == 3


def test_emitter_without_quality_words_is_refused(emu_ctx):
    mc.check_refused_without_quality(emu_ctx, MEM, mc.small_case())
