"""MAPQ and secondary lines from the best stratum on the GPU (tests/mapq_cases.py): the cases of tests/test_mapq_cpu.py at the
same shapes (the device lays a slice of 16 KiB out in a workgroup where the harness has 256 bytes), one case at size (a
2^22-symbol record with a segment planted twice, 10^4 reads of 100), and the command-line tool with --mapq."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import best_cases as bc
import mapq_cases as mc
import pairs_cases as pc
import stralg_amd
import unmapped_cases as uc
from device_memory import GpuMemory
from sam_cases import ROOT
from stralg_amd import _lib, api

pytestmark = pytest.mark.gpu

MAPPER = os.path.join(ROOT, "tools", "stralg_amd_readmapper")


@pytest.fixture(scope="module")
def cases():
    return bc.best_cases()


@pytest.fixture(scope="module")
def mem():
    return GpuMemory()


@pytest.fixture(scope="module")
def mapper():
    if not os.path.exists(MAPPER):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "stralg_amd", "csrc"), "mapper"])
    return MAPPER


@pytest.fixture(scope="module")
def indexes(gpu_ctx):
    """(fasta, form) -> a resident index, built once"""
    made = {}

    def get(fasta, **form):
        key = (fasta, tuple(sorted(form.items())))
        if key not in made:
            made[key] = stralg_amd.Index.from_fasta(fasta, ctx=gpu_ctx, **form)
        return made[key]

    yield get
    for idx in made.values():
        idx.close()


def switched(ctx, window=0, batch=0, room=0, locate=0):
    """a context manager that sets the loop's switches and puts them back at 0"""
    class _S:
        def __enter__(self):
            ctx.set_sam_window_bytes(window)
            ctx.set_sam_batch_reads(batch)
            ctx.set_sam_room_hits(room)
            ctx.set_locate_chunk_rows(locate)

        def __exit__(self, *exc):
            ctx.set_sam_window_bytes(0)
            ctx.set_sam_batch_reads(0)
            ctx.set_sam_room_hits(0)
            ctx.set_locate_chunk_rows(0)
    return _S()


# ---- the table's cases ---------------------------------------------------------------------------------------------------------
def test_oracle_counts(cases):
    mc.check_table(cases)


@pytest.mark.parametrize("row", mc.TABLE, ids=mc.TABLE_IDS)
def test_table_cases(gpu_ctx, indexes, cases, row):
    """through the stream call (tables of the module-level call) and through a resident index"""
    name, k, both, indels = row[:4]
    c = cases[name]
    want = mc.want_of(c, k, both, indels)
    bc.check_text(stralg_amd.map_reads(c["fasta"], c["fastq"], k, ctx=gpu_ctx, both_strands=both, best=True, indels=indels, mapq=True), want)
    bc.check_text(indexes(c["fasta"]).map_reads(c["fastq"], k, both_strands=both, best=True, indels=indels, mapq=True), want)
    assert gpu_ctx.map_stats()["retries"] == 0


# ---- the other flags and the index forms --------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", mc.FLAG_SETS, ids=mc.FLAG_SET_IDS)
def test_with_the_other_flags(gpu_ctx, indexes, cases, flags):
    tags, unmapped, header, indels = flags
    c = cases["two-records-best"]
    idx = indexes(c["fasta"])
    got = idx.map_reads(c["fastq"], 2, both_strands=True, best=True, indels=indels, tags=tags, unmapped=unmapped, header=header, mapq=True)
    bc.check_text(got, mc.want_of(c, 2, True, indels, tags, unmapped, header))
    plain = idx.map_reads(c["fastq"], 2, both_strands=True, best=True, indels=indels, tags=tags, unmapped=unmapped, header=header)
    bc.check_text(plain, mc.plain_of(c, 2, True, indels, tags, unmapped, header))


@pytest.mark.parametrize("form", mc.FORMS, ids=mc.FORM_IDS)
def test_index_forms(gpu_ctx, indexes, cases, form):
    c = cases["two-records-best"]
    idx = indexes(c["fasta"], **form)
    bc.check_text(idx.map_reads(c["fastq"], 1, best=True, mapq=True), mc.want_of(c, 1, False))
    got = idx.map_reads(c["fastq"], 2, both_strands=True, best=True, indels=False, tags=True, unmapped=True, header=True, mapq=True)
    bc.check_text(got, mc.want_of(c, 2, True, False, True, True, True))
    c = cases["test-out"]
    bc.check_text(indexes(c["fasta"], **form).map_reads(c["fastq"], 2, both_strands=True, best=True, mapq=True), mc.want_of(c, 2, True))


def test_sampled_index_located_in_runs_of_five(gpu_ctx, indexes, cases):
    c = cases["two-records-best"]
    idx = indexes(c["fasta"], compact=True, sa_sample=16)
    with switched(gpu_ctx, locate=5):
        bc.check_text(idx.map_reads(c["fastq"], 1, best=True, mapq=True), mc.want_of(c, 1, False))
        got = idx.map_reads(c["fastq"], 2, both_strands=True, best=True, tags=True, unmapped=True, mapq=True)
        bc.check_text(got, mc.want_of(c, 2, True, True, True, True))


# ---- batches, windows, the room ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 3, 33])
def test_batches(gpu_ctx, indexes, cases, batch):
    c = cases["two-records-best"]
    idx = indexes(c["fasta"])
    with switched(gpu_ctx, batch=batch):
        for both, unmapped in ((False, False), (True, True)):
            got = idx.map_reads(c["fastq"], 2, both_strands=both, best=True, unmapped=unmapped, header=True, mapq=True)
            bc.check_text(got, mc.want_of(c, 2, both, unmapped=unmapped, header=True))
            assert gpu_ctx.map_stats()["batches"] == (-(-2 * 240 // (batch + batch % 2)) if both else -(-240 // batch))


def test_sixteen_byte_windows(gpu_ctx, indexes, cases):
    c = cases["two-records-best"]
    chunks = []
    with switched(gpu_ctx, window=16):
        indexes(c["fasta"]).map_reads(c["fastq"], 0, sink=chunks.append, both_strands=True, best=True, mapq=True)
    assert max(len(x) for x in chunks) <= 16
    bc.check_text(b"".join(chunks), mc.want_of(c, 0, True))


def test_room_of_one_hit(gpu_ctx, indexes, cases):
    c = cases["two-records-best"]
    with switched(gpu_ctx, room=1, window=1000):
        for unmapped in (False, True):
            got = indexes(c["fasta"]).map_reads(c["fastq"], 2, both_strands=True, best=True, unmapped=unmapped, mapq=True)
            st = gpu_ctx.map_stats()
            assert st["retries"] > 0 and st["halved"] > 0, st
            bc.check_text(got, mc.want_of(c, 2, True, unmapped=unmapped))


# ---- edges -------------------------------------------------------------------------------------------------------------------
def test_unmapped_reads_first_middle_and_last(gpu_ctx, indexes, cases):
    c = cases["two-records-best"]
    fastq = mc.edges_fastq(c)
    plain, added = uc.with_unmapped(fastq, bc.want_of(c, 1, True))
    want, n = mc.with_mapq(fastq, plain)
    assert added >= 3 and want.startswith(b"first-lost\t4\t") and n["secondary"] > 0
    for batch in (0, 1, 2, 3):
        with switched(gpu_ctx, batch=batch):
            bc.check_text(indexes(c["fasta"]).map_reads(fastq, 1, both_strands=True, best=True, unmapped=True, mapq=True), want)


def test_empty_fastq_and_refusals(gpu_ctx, indexes, cases):
    c = cases["test-out"]
    idx = indexes(c["fasta"])
    head = uc.header_of(c["fasta"])
    assert idx.map_reads(b"", 1, best=True, mapq=True) == b"" and idx.map_reads(b"", 1, best=True, header=True, mapq=True) == head
    chunks = []

    def sink(user, section, data, n):
        chunks.append(C.string_at(data, n))
        return 0

    cb = _lib.SINK_FN(sink)
    buf = np.frombuffer(c["fastq"], np.uint8)
    Q, H, B = _lib.SX_MAP_MAPQ, _lib.SX_MAP_HEADER, _lib.SX_MAP_BEST_STRATUM
    records = [(name, stralg_amd.build_complete_table(seq, True, gpu_ctx)) for name, seq in gpu_ctx.fasta_records(c["fasta"])]
    recs = (_lib.MapRecord * len(records))()
    keep = []
    for r, (name, t) in enumerate(records):
        recs[r] = api._map_record(name, t, keep)
    for flags in (Q, H | Q):
        assert gpu_ctx.lib.sx_index_map_reads_ex(gpu_ctx.h, idx._handle(), buf.ctypes.data, buf.size, 1, flags, cb, None) == _lib.SX_E_ARG
        assert gpu_ctx.lib.sx_map_reads_stream_ex(gpu_ctx.h, recs, len(records), buf.ctypes.data, buf.size, 1, flags, cb, None) == _lib.SX_E_ARG
    p = pc.pair_case(("test-out/k1", "overlap", 0, 500))
    for flags in (Q, Q | B, Q | B | H):
        assert pc.raw_call(gpu_ctx, idx, p["fastq1"], p["fastq2"], 1, 0, 500, flags) == (_lib.SX_E_ARG, b""), flags
    assert not chunks
    limit = gpu_ctx.lib.sx_map_reads_limit
    for n, other in ((2 ** 32 - 1, B), (2 ** 32, B), (2 ** 31 - 1, B | 1), (2 ** 31, B | 1)):
        assert limit(n, 1, other | Q) == limit(n, 1, other)


def test_second_call_and_fresh_context(gpu_ctx, cases):
    c = cases["two-records-best"]
    want = mc.want_of(c, 1, True, unmapped=True, header=True)
    with stralg_amd.Index.from_fasta(c["fasta"], ctx=gpu_ctx, compact=True, sa_sample=32) as idx:
        first = idx.map_reads(c["fastq"], 1, both_strands=True, best=True, unmapped=True, header=True, mapq=True)
        assert idx.map_reads(c["fastq"], 1, both_strands=True, best=True) == bc.want_of(c, 1, True)
        assert idx.map_reads(c["fastq"], 1, both_strands=True, best=True, unmapped=True, header=True, mapq=True) == first == want
    fresh = api.Context(0)
    try:
        with stralg_amd.Index.from_fasta(c["fasta"], ctx=fresh) as other:
            assert other.map_reads(c["fastq"], 1, both_strands=True, best=True, unmapped=True, header=True, mapq=True) == want
    finally:
        fresh.close()


# ---- the exported emitter over made-up hits ---------------------------------------------------------------------------------
@pytest.mark.parametrize("with_flags", [False, True], ids=["no-flags", "flags"])
def test_emitter_small(gpu_ctx, mem, with_flags):
    case = mc.small_case()
    flags = case["flags"] if with_flags else None
    b, want = mc.check_emitter(gpu_ctx, mem, case, flags, sixteen=True)
    assert mc.check_cuts(b, want, b"272" if with_flags else b"256") >= 9
    located, _ = mc.check_emitter(gpu_ctx, mem, case, flags, located=True, sixteen=True)
    assert located.text() == want


@pytest.mark.parametrize("with_flags", [False, True], ids=["no-flags", "flags"])
@pytest.mark.parametrize("located", [False, True], ids=["rows", "located"])
def test_emitter_intervals(gpu_ctx, mem, with_flags, located):
    case = mc.interval_case()
    _, want = mc.check_emitter(gpu_ctx, mem, case, case["flags"] if with_flags else None, located)
    flags = {l.split(b"\t")[1] for l in want.split(b"\n")[:-1]}
    assert flags == ({b"0", b"16", b"256", b"272", b"4"} if with_flags else {b"0", b"256", b"4"})
    assert {l.split(b"\t")[4] for l in want.split(b"\n")[:-1]} == {b"50", b"3", b"1", b"0", b"255"}


@pytest.mark.parametrize("located", [False, True], ids=["rows", "located"])
def test_emitter_tagged(gpu_ctx, mem, located):
    case = mc.tagged_case()
    for flags in (None, case["flags"]):
        _, want = mc.check_emitter(gpu_ctx, mem, case, flags, located)
        assert b"\tNM:i:" in want and want.count(b"\t4\t*\t0\t0\t*\t*\t0\t0\t") == 3


def test_emitter_without_quality_words_is_refused(gpu_ctx, mem):
    mc.check_refused_without_quality(gpu_ctx, mem, mc.small_case())


# ---- one case at size ----------------------------------------------------------------------------------------------------------
def test_at_size(gpu_ctx):
    """a record of 2^22 symbols with a segment planted twice, 10^4 reads of 100, every tenth from the segment; k = 1, no indels,
    both strands, batches of 1 000 reads: the oracle applied to the same call's text without the bit"""
    fasta, fastq = mc.planted_case()
    with stralg_amd.Index.from_fasta(fasta, ctx=gpu_ctx) as idx, switched(gpu_ctx, batch=1000):
        plain = idx.map_reads(fastq, 1, both_strands=True, best=True, indels=False)
        got = idx.map_reads(fastq, 1, both_strands=True, best=True, indels=False, mapq=True)
        assert gpu_ctx.map_stats()["batches"] == 20
    want, n = mc.with_mapq(fastq, plain)
    assert n["groups"][3] >= 1000 and n["groups"][50] >= 8000 and n["lines"] == plain.count(b"\n") >= 11000, n["groups"]
    bc.check_text(got, want)


# ---- the tool -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_memory", [True, False], ids=["in-memory", "index-file"])
def test_tool(mapper, tmp_path, cases, in_memory):
    c = cases["two-records-best"]
    fa, fq = tmp_path / "genome.fa", tmp_path / "reads.fq"
    fa.write_bytes(c["fasta"])
    fq.write_bytes(c["fastq"])
    if not in_memory:
        subprocess.run([mapper, "-p", str(fa)], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    base = (["-i"] if in_memory else []) + ["-d", "2", str(fa)]
    got = subprocess.run([mapper, "--best", "--mapq", "--unmapped", "--header"] + base + [str(fq)], check=True, stdout=subprocess.PIPE,
                         stderr=subprocess.DEVNULL, timeout=300).stdout
    bc.check_text(got, mc.want_of(c, 2, False, unmapped=True, header=True))
    for args in (["--mapq"] + base + [str(fq)], ["--best", "--mapq"] + base + [str(fq), "-2", str(fq)]):
        r = subprocess.run([mapper] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode != 0 and r.stdout == b"" and b"--mapq" in r.stderr and b"usage" in r.stderr, args
