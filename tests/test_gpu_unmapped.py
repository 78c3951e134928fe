"""Unmapped reads and the SAM header on the GPU (tests/unmapped_cases.py): the cases of tests/test_unmapped_cpu.py at the same
shapes (the device lays a slice of 16 KiB out in a workgroup where the harness has 256 bytes), the digest-only fixture case,
one case at size (a 2^22-symbol record, 10^4 reads of which about half are random), and the command-line tool with
--unmapped and --header."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import best_cases as bc
import pairs_cases as pc
import stralg_amd
import unmapped_cases as uc
from device_memory import GpuMemory
from sam_cases import ROOT, sam_cases
from stralg_amd import _lib, api

pytestmark = pytest.mark.gpu

MAPPER = os.path.join(ROOT, "tools", "stralg_amd_readmapper")


@pytest.fixture(scope="module")
def cases():
    return uc.fixture_cases()


@pytest.fixture(scope="module")
def flag_cases():
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


# ---- the fixture cases -------------------------------------------------------------------------------------------------------
def test_oracle_counts(cases):
    uc.check_added(cases)


@pytest.mark.parametrize("row", uc.ADDED, ids=uc.ADDED_IDS)
def test_fixture_cases(gpu_ctx, indexes, cases, row):
    """through the stream call (tables of the module-level call), with and without the header, and through a resident index"""
    name, k, both, best, added = row
    c = cases[row[:4]]
    for header in (False, True):
        got = stralg_amd.map_reads(c["fasta"], c["fastq"], k, ctx=gpu_ctx, both_strands=both, best=best, unmapped=True, header=header)
        bc.check_text(got, uc.want_of(c, header))
    bc.check_text(indexes(c["fasta"]).map_reads(c["fastq"], k, both_strands=both, best=best, unmapped=True, header=True), uc.want_of(c, True))


def test_digest_case_keeps_its_digest(gpu_ctx, indexes):
    """hg38/reads-100-10-0/k2 has no unmapped read: with the bit and without the header its recorded SHA-256"""
    c = sam_cases()[uc.BY_DIGEST]
    got = indexes(c["fasta"]).map_reads(c["fastq"], c["k"], unmapped=True)
    assert len(got) == c["bytes"] and got.count(b"\n") == c["lines"]
    assert hashlib.sha256(got).digest() == c["sha256"]


# ---- the other flags and the index forms --------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", uc.FLAG_SETS, ids=uc.FLAG_SET_IDS)
def test_with_the_other_flags(gpu_ctx, indexes, flag_cases, flags):
    k, both, best, indels, tags = flags
    for name in ("test-out", "two-records-best"):
        c = flag_cases[name]
        idx = indexes(c["fasta"])
        for header in (False, True):
            got = idx.map_reads(c["fastq"], k, both_strands=both, best=best, indels=indels, tags=tags, unmapped=True, header=header)
            bc.check_text(got, uc.want_flags(c, k, both, best, indels, tags, header))


@pytest.mark.parametrize("form", [dict(), dict(compact=True), dict(compact=True, sa_sample=32), dict(compact=True, packed=True, sa_sample=32)],
                         ids=["full", "compact", "sampled", "packed-sampled"])
def test_index_forms(gpu_ctx, indexes, cases, flag_cases, form):
    for key in (("test-out/k2", 2, False, False), ("two-records/k1", 1, False, False)):
        c = cases[key]
        idx = indexes(c["fasta"], **form)
        bc.check_text(idx.map_reads(c["fastq"], c["k"], unmapped=True, header=True), uc.want_of(c, True))
        bc.check_text(idx.map_reads(c["fastq"], c["k"]), c["plain"])
    c = flag_cases["two-records-best"]
    idx = indexes(c["fasta"], **form)
    got = idx.map_reads(c["fastq"], 2, both_strands=True, best=True, indels=False, tags=True, unmapped=True)
    bc.check_text(got, uc.want_flags(c, 2, True, True, False, True))


def test_sampled_index_located_in_runs_of_five(gpu_ctx, indexes, cases, flag_cases):
    with switched(gpu_ctx, locate=5):
        c = cases[("two-records/k1", 1, False, False)]
        bc.check_text(indexes(c["fasta"], compact=True, sa_sample=16).map_reads(c["fastq"], 1, unmapped=True), uc.want_of(c))
        c = flag_cases["two-records-best"]
        bc.check_text(indexes(c["fasta"], compact=True, sa_sample=16).map_reads(c["fastq"], 1, both_strands=True, tags=True, unmapped=True),
                      uc.want_flags(c, 1, True, False, True, True))


# ---- batches, windows, the room ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 3, 33])
def test_batches(gpu_ctx, indexes, cases, flag_cases, batch):
    c = cases[("two-records/k1", 1, False, False)]
    with switched(gpu_ctx, batch=batch):
        bc.check_text(indexes(c["fasta"]).map_reads(c["fastq"], 1, unmapped=True, header=True), uc.want_of(c, True))
        assert gpu_ctx.map_stats()["batches"] == -(-200 // batch)
        c = flag_cases["two-records-best"]
        for best in (False, True):
            bc.check_text(indexes(c["fasta"]).map_reads(c["fastq"], 2, both_strands=True, best=best, unmapped=True),
                          uc.want_flags(c, 2, True, best, True, False))


def test_sixteen_byte_windows(gpu_ctx, indexes, cases):
    c = cases[("two-records/k1", 1, False, False)]
    reads = uc.fastq_reads(uc.all_unmapped_fastq(16, 3))
    fastq = uc.fastq_image([(b"n%07d" % q, s, qq) for q, (_, s, qq) in enumerate(reads)])  # (lines of 33 bytes)
    with switched(gpu_ctx, window=16):
        chunks = []
        indexes(c["fasta"]).map_reads(c["fastq"], 1, sink=chunks.append, unmapped=True)
        assert max(len(x) for x in chunks) <= 16
        bc.check_text(b"".join(chunks), uc.want_of(c))
        chunks = []
        indexes(c["fasta"]).map_reads(fastq, 1, sink=chunks.append, unmapped=True)
    assert b"".join(chunks) == b"".join(uc.unmapped_line(r) for r in uc.fastq_reads(fastq))


def test_room_of_one_hit(gpu_ctx, indexes, flag_cases):
    c = flag_cases["two-records-best"]
    with switched(gpu_ctx, room=1, window=1000):
        for best in (False, True):
            got = indexes(c["fasta"]).map_reads(c["fastq"], 2, both_strands=True, best=best, unmapped=True)
            assert gpu_ctx.map_stats()["retries"] > 0
            bc.check_text(got, uc.want_flags(c, 2, True, best, True, False))


# ---- edges -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [dict(), dict(compact=True, sa_sample=32)], ids=["full", "sampled"])
def test_reads_that_all_fail_to_map(gpu_ctx, indexes, cases, form):
    c = cases[("test-out/k2", 2, False, False)]
    fastq = uc.all_unmapped_fastq()
    want = b"".join(uc.unmapped_line(r) for r in uc.fastq_reads(fastq))
    idx = indexes(c["fasta"], **form)
    assert idx.map_reads(fastq, 2) == b""
    for batch in (0, 1):
        with switched(gpu_ctx, batch=batch):
            for both in (False, True):
                for best in (False, True):
                    assert idx.map_reads(fastq, 2, both_strands=both, best=best, unmapped=True) == want, (batch, both, best)


def test_first_and_last_read_of_a_batch(gpu_ctx, indexes, cases):
    c = cases[("two-records/k1", 1, False, False)]
    fastq = uc.edges_fastq(c)
    want, added = uc.with_unmapped(fastq, c["plain"])
    assert added == 12
    for batch in (0, 1, 2, 101, 102):
        with switched(gpu_ctx, batch=batch):
            bc.check_text(indexes(c["fasta"]).map_reads(fastq, 1, unmapped=True), want)


def test_empty_fastq_and_pairs_with_header(gpu_ctx, indexes):
    p = pc.pair_case(("test-out/k1", "overlap", 0, 500))
    idx = indexes(p["fasta"])
    head = uc.header_of(p["fasta"])
    assert idx.map_reads(b"", 1, unmapped=True) == b"" and idx.map_reads(b"", 1, unmapped=True, header=True) == head
    assert idx.map_pairs(b"", b"", 1, header=True) == head and idx.map_pairs(b"", b"", 1) == b""
    assert p["want"] and idx.map_pairs(p["fastq1"], p["fastq2"], p["k"], p["lo"], p["hi"], header=True) == head + p["want"]
    assert pc.raw_call(gpu_ctx, idx, p["fastq1"], p["fastq2"], 1, 0, 500, _lib.SX_MAP_UNMAPPED) == (_lib.SX_E_ARG, b"")
    assert pc.raw_call(gpu_ctx, idx, p["fastq1"], p["fastq2"], 1, 0, 500, _lib.SX_MAP_UNMAPPED | _lib.SX_MAP_HEADER) == (_lib.SX_E_ARG, b"")


def test_second_call_and_fresh_context(gpu_ctx, flag_cases):
    c = flag_cases["two-records-best"]
    want = uc.want_flags(c, 1, True, True, True, False, True)
    with stralg_amd.Index.from_fasta(c["fasta"], ctx=gpu_ctx, compact=True, sa_sample=32) as idx:
        first = idx.map_reads(c["fastq"], 1, both_strands=True, best=True, unmapped=True, header=True)
        assert idx.map_reads(c["fastq"], 1, both_strands=True, best=True) == bc.want_of(c, 1, True)
        assert idx.map_reads(c["fastq"], 1, both_strands=True, best=True, unmapped=True, header=True) == first == want
    fresh = api.Context(0)
    try:
        with stralg_amd.Index.from_fasta(c["fasta"], ctx=fresh) as other:
            assert other.map_reads(c["fastq"], 1, both_strands=True, best=True, unmapped=True, header=True) == want
    finally:
        fresh.close()


def test_emitter_made_up(gpu_ctx, mem):
    uc.check_made_up(gpu_ctx, mem, uc.made_up_case())


# ---- one case at size ----------------------------------------------------------------------------------------------------------
def test_at_size(gpu_ctx):
    """a record of 2^22 symbols, 10^4 reads of 100: every second one a substring of the record with at most one
    substitution (it maps), the others random (they do not, within one edit, but for odds of about 10^-50); k = 1, batches of 1 000 reads.  The plain call's text with the FLAG 4 lines inserted
    by the oracle"""
    rng = np.random.default_rng(2024)
    dna = np.frombuffer(b"ACGT", np.uint8)
    genome = rng.choice(dna, 1 << 22)
    fasta = b">big record\n" + b"\n".join(genome[i:i + 80].tobytes() for i in range(0, genome.size, 80)) + b"\n"
    reads = []
    for q in range(10000):
        if q % 2:
            seq = rng.choice(dna, 100)
        else:
            at = int(rng.integers(0, genome.size - 100))
            seq = genome[at:at + 100].copy()
            for j in rng.integers(0, 100, int(rng.integers(0, 2))):
                seq[j] = dna[(np.flatnonzero(dna == seq[j])[0] + 1) % 4]
        reads.append((b"r%d" % q, seq.tobytes(), bytes(rng.integers(33, 74, 100, dtype=np.uint8).tolist())))
    fastq = uc.fastq_image(reads)
    with stralg_amd.Index.from_fasta(fasta, ctx=gpu_ctx) as idx, switched(gpu_ctx, batch=1000):
        plain = idx.map_reads(fastq, 1)
        got = idx.map_reads(fastq, 1, unmapped=True, header=True)
    want, added = uc.with_unmapped(fastq, plain)
    assert added == 5000, added
    bc.check_text(got, uc.header_of(fasta) + want)


# ---- the tool -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_memory", [True, False], ids=["in-memory", "index-file"])
def test_tool(mapper, tmp_path, cases, in_memory):
    c = cases[("two-records/k1", 1, False, False)]
    fa, fq, fq2 = tmp_path / "genome.fa", tmp_path / "reads.fq", tmp_path / "more.fq"
    fa.write_bytes(c["fasta"])
    fq.write_bytes(c["fastq"])
    fq2.write_bytes(uc.all_unmapped_fastq(5, 7))
    if not in_memory:
        subprocess.run([mapper, "-p", str(fa)], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    base = (["-i"] if in_memory else []) + ["-d", "1", str(fa)]
    got = subprocess.run([mapper, "--unmapped", "--header"] + base + [str(fq), str(fq2)], check=True, stdout=subprocess.PIPE,
                         stderr=subprocess.DEVNULL, timeout=300).stdout
    more = b"".join(uc.unmapped_line(r) for r in uc.fastq_reads(uc.all_unmapped_fastq(5, 7)))
    bc.check_text(got, uc.want_of(c, True) + more)  # (the header once, at the top)
    got = subprocess.run([mapper, "--header", "--compact", "--sa-sample", "32"] + base + [str(fq)], check=True, stdout=subprocess.PIPE,
                         stderr=subprocess.DEVNULL, timeout=300).stdout
    bc.check_text(got, uc.header_of(c["fasta"]) + c["plain"])
    r = subprocess.run([mapper, "--unmapped"] + base + [str(fq), "-2", str(fq)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode != 0 and r.stdout == b"" and b"usage" in r.stderr
