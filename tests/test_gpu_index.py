"""The device-resident index on the GPU (sx_index.hip: stralg_amd.Index, sx_fastq.hip: sx_fastq_index_dev, the tool's -i and several
FASTQ files) against the reference mapper's stdout (tests/golden/golden_sam.npz), the reference's tables
(tests/golden/golden_genomes.npz), and, at size, against what numpy says about reads cut at known places."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from conftest import check_against_sha, genome_cases
import index_form_cases as forms
from sam_cases import ROOT, check_case, sam_cases
import stralg_amd
from stralg_amd import Index, api

pytestmark = pytest.mark.gpu

MAPPER = os.path.join(ROOT, "tools", "stralg_amd_readmapper")
NAMES = ["test-out/k0", "test-out/k1", "test-out/k2", "hg38/reads-100-10-0/k0", "hg38/reads-100-10-0/k1",
         "hg38/reads-100-10-0/k2", "hg38/reads-1000-100-2/k2", "hg38/reads-1000-200-1/k1", "two-records/k1"]  # test_gpu_sam.NAMES


@pytest.fixture(scope="module")
def cases():
    return sam_cases()


@pytest.fixture(scope="module")
def mapper():
    if not os.path.exists(MAPPER):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "stralg_amd", "csrc"), "mapper"])
    return MAPPER


_INDEXES = {}


@pytest.fixture(scope="module")
def index_of(gpu_ctx):
    def get(fasta):
        if fasta not in _INDEXES:
            _INDEXES[fasta] = Index.from_fasta(fasta, ctx=gpu_ctx)
        return _INDEXES[fasta]
    yield get
    for idx in _INDEXES.values():
        idx.close()
    _INDEXES.clear()


@pytest.mark.parametrize("name", NAMES)
def test_from_fasta_equals_the_reference(gpu_ctx, cases, index_of, name):
    c = cases[name]
    check_case(c, index_of(c["fasta"]).map_reads(c["fastq"], c["k"]))


@pytest.mark.parametrize("form", list(forms.FORMS))
@pytest.mark.parametrize("name", forms.CASES)
def test_built_and_loaded_agree_in_every_form(gpu_ctx, cases, name, form):
    forms.check_built_and_loaded_agree(gpu_ctx, Index, cases[name], form)


@pytest.mark.parametrize("name", NAMES)
def test_tool_in_memory_equals_the_reference(mapper, cases, name, tmp_path):
    c = cases[name]
    fa, fq = tmp_path / "genome.fa", tmp_path / "reads.fq"
    fa.write_bytes(c["fasta"])
    fq.write_bytes(c["fastq"])
    got = subprocess.run([mapper, "-i", "-d", str(c["k"]), str(fa), str(fq)], check=True, stdout=subprocess.PIPE,
                         stderr=subprocess.DEVNULL, timeout=300).stdout
    check_case(c, got)
    assert not os.path.exists(str(fa) + ".bwttables")


def test_tool_several_read_files(mapper, cases, tmp_path):
    a, b = cases["test-out/k1"], cases["test-out/k2"]
    assert a["fasta"] == b["fasta"]
    fa, fqa, fqb = tmp_path / "genome.fa", tmp_path / "a.fq", tmp_path / "b.fq"
    fa.write_bytes(a["fasta"])
    fqa.write_bytes(a["fastq"])
    fqb.write_bytes(b["fastq"])
    subprocess.run([mapper, "-p", str(fa)], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    run = lambda *files: subprocess.run([mapper, "-d", "1", str(fa)] + [str(f) for f in files], check=True,
                                        stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=300).stdout
    one, two = run(fqa), run(fqb)
    assert one == a["sam"] and two
    assert run(fqa, fqb) == one + two
    assert run(fqb, fqa, fqb) == two + one + two


def test_device_tables_of_a_genome(gpu_ctx):
    """SA, O and RO by digest, C and the remapped string directly, against the reference's (golden_genomes.npz)"""
    g = genome_cases()["hg38-10000.fa"]
    with Index.from_fasta(g["file"], ctx=gpu_ctx) as idx:
        assert len(idx.records) == g["records"]
        total = 0
        for r, want in enumerate(g["recs"]):
            name, N, sigma, has_ro = idx.records[r]
            assert name == want["name"] and N == want["sym"].size + 1 and sigma == want["sigma"] and has_ro
            got = idx.device_tables(r)
            check_against_sha(got["sa"], want, "sa", "hg38-10000.fa")
            check_against_sha(got["o"], want, "o", "hg38-10000.fa")
            check_against_sha(got["ro"], want, "ro", "hg38-10000.fa")
            assert (got["c"] == want["c"]).all()
            assert (got["string"][:-1] == want["sym"]).all() and got["string"][-1] == 0
            total += N * (5 + 8 * sigma)
        assert total <= idx.device_bytes <= total + 4096 * (5 * g["records"] + 5)


def fasta_of(records, width=60):
    out = []
    for name, seq in records:
        full = seq.size - seq.size % width
        rows = seq[:full].reshape(-1, width)
        lines = np.empty((rows.shape[0], width + 1), np.uint8)
        lines[:, :width] = rows
        lines[:, width] = 10
        out.append(b">" + name + b"\n" + lines.tobytes() + (seq[full:].tobytes() + b"\n" if full < seq.size else b""))
    return b"".join(out)


def fastq_of(names, seqs, qual=ord("I")):
    """reads of one length m: '@' name '\\n' seq '\\n+\\n' qual '\\n' (names: equal-length byte rows)"""
    n, m = seqs.shape
    w = names.shape[1]
    rec = np.empty((n, 1 + w + 1 + m + 3 + m + 1), np.uint8)
    rec[:, 0] = ord("@")
    rec[:, 1:1 + w] = names
    rec[:, 1 + w] = 10
    rec[:, 2 + w:2 + w + m] = seqs
    rec[:, 2 + w + m:5 + w + m] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, 5 + w + m:5 + w + 2 * m] = qual
    rec[:, -1] = 10
    return rec.tobytes()


def read_names(n):
    return np.frombuffer(b"".join(b"r%07d" % i for i in range(n)), np.uint8).reshape(n, 8)


def test_at_size_exact_matches_checked_with_numpy(gpu_ctx):
    """two records of 2^26 symbols of synthetic DNA, 10^5 reads of 100 symbols cut at known (record, position) pairs, k = 0:
    every read has exactly one line, with its record's name, position + 1 and 100M (a second occurrence of 100 symbols
    among 2^27 random ones has probability about 10^5 x 2^27 / 4^100)"""
    n, m, reads = 1 << 26, 100, 100_000
    letters = np.frombuffer(b"\0ACGT", np.uint8)
    recs = [(b"chrA", letters[stralg_amd.synth(n, 5, 101)]), (b"chrB", letters[stralg_amd.synth(n, 5, 202)])]
    rng = np.random.default_rng(7)
    which = rng.integers(0, 2, reads)
    pos = rng.integers(0, n - m, reads)
    seqs = np.stack([recs[0][1], recs[1][1]])[which[:, None], pos[:, None] + np.arange(m)[None, :]]
    names = read_names(reads)
    fastq = fastq_of(names, seqs)
    with Index.from_fasta(fasta_of(recs), ctx=gpu_ctx) as idx:
        assert [r[:3] for r in idx.records] == [(b"chrA", n + 1, 5), (b"chrB", n + 1, 5)]
        text = idx.map_reads(fastq, 0)
    lines = text.split(b"\n")
    assert lines.pop() == b"" and len(lines) == reads
    fields = [l.split(b"\t") for l in lines]
    assert all(len(f) == 11 for f in fields)
    assert [f[0] for f in fields] == [names[i].tobytes() for i in range(reads)]
    assert [f[2] for f in fields] == [(b"chrA", b"chrB")[w] for w in which]
    assert (np.array([int(f[3]) for f in fields]) == pos + 1).all()
    assert all(f[1] == b"0" and f[4] == b"0" and f[5] == b"100M" and f[6:9] == [b"*", b"0", b"0"] for f in fields)
    assert [f[9] for f in fields] == [seqs[i].tobytes() for i in range(reads)]
    assert all(f[10] == b"I" * m for f in fields)


def test_write_streams_several_chunks(gpu_ctx):
    """one record of 2^22 symbols of synthetic DNA (sigma 5) with RO: its O and RO tables are 84 MB each, three chunks of
    the 32 MiB staging buffers, so both buffers are used a second time.  The written stream, walked by the layout of
    the reference's serialise.c, holds at each array's place what single copies of the device buffers give."""
    n = 1 << 22
    seq = np.frombuffer(b"\0ACGT", np.uint8)[stralg_amd.synth(n, 5, 303)]
    chunks = []
    with Index.from_fasta(fasta_of([(b"chrW", seq)]), ctx=gpu_ctx) as idx:
        assert idx.records == [(b"chrW", n + 1, 5, True)]
        idx.write(chunks.append)
        want = idx.device_tables(0)
    stream = np.frombuffer(b"".join(chunks), np.uint8)
    N, sigma, at = n + 1, 5, 0

    def take(count, dtype=np.uint8):
        nonlocal at
        out = stream[at:at + count * np.dtype(dtype).itemsize].view(dtype)
        assert out.size == count, "the stream ends early"
        at += out.nbytes
        return out

    assert take(1, np.uint32)[0] == 1  # records
    assert take(1, np.uint32)[0] == 5 and take(5).tobytes() == b"chrW\0"  # the name with its terminator
    assert take(1, np.uint32)[0] == n and (take(n) == want["string"][:-1]).all()
    assert (take(N, np.uint32) == want["sa"]).all()
    remap = take(4 + 256 + 128)  # remap.h: alphabet size, table, reverse table
    assert remap[:4].view(np.uint32)[0] == sigma and remap[4 + 256:4 + 256 + sigma].tobytes() == b"\0ACGT"
    assert (take(sigma, np.uint32) == want["c"]).all()
    assert (take((N + 1) * sigma, np.uint32) == want["o"].ravel()).all()
    assert take(1)[0] == 1  # the flag: RO follows
    assert (take((N + 1) * sigma, np.uint32) == want["ro"].ravel()).all()
    assert at == stream.size
    assert (N + 1) * sigma * 4 > 2 * (32 << 20)  # (a third chunk)


def test_at_size_agrees_with_the_stream_call(gpu_ctx):
    """a record of 2^24 symbols, 10^5 reads with up to one substitution, k = 1: the index path's text has the SHA-256 of
    Context.map_reads_stream's, fed host tables from build_complete_table"""
    n, m, reads = 1 << 24, 100, 100_000
    letters = np.frombuffer(b"\0ACGT", np.uint8)
    seq = letters[stralg_amd.synth(n, 5, 303)]
    rng = np.random.default_rng(9)
    pos = rng.integers(0, n - m, reads)
    seqs = seq[pos[:, None] + np.arange(m)[None, :]].copy()
    hit = rng.integers(0, 2, reads).astype(bool)
    at = rng.integers(0, m, reads)
    seqs[hit, at[hit]] = letters[1 + (np.searchsorted(letters[1:], seqs[hit, at[hit]]) + 1) % 4]
    fastq = fastq_of(read_names(reads), seqs)
    fasta = fasta_of([(b"chrS", seq)])
    with Index.from_fasta(fasta, ctx=gpu_ctx) as idx:
        h = hashlib.sha256()
        size = [0]

        def sink(chunk):
            h.update(chunk)
            size[0] += len(chunk)

        idx.map_reads(fastq, 1, sink=sink)
    records = [(name, stralg_amd.build_complete_table(s, True, gpu_ctx)) for name, s in gpu_ctx.fasta_records(fasta)]
    h2 = hashlib.sha256()
    gpu_ctx.map_reads_stream(records, fastq, 1, h2.update)
    assert size[0] > reads * 200 and h.digest() == h2.digest()


def big_fastq(reads, rng):
    m = 90
    seqs = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (reads, m))]
    return fastq_of(read_names(reads), seqs, qual=ord("#"))


def test_fastq_index_dev_at_size(gpu_ctx):
    """10^6 records (about 200 MB): the six device arrays equal the host function's; one defect near the end: malformed"""
    import torch
    reads = 1_000_000
    data = big_fastq(reads, np.random.default_rng(3))
    assert len(data) > 190_000_000
    d = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    got, count = gpu_ctx.fastq_index_dev(d, len(data))
    want = gpu_ctx.fastq_index(data)
    assert count == reads
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.size == w.size and (g == w).all()
    again, _ = gpu_ctx.fastq_index_dev(d, len(data))
    assert all((a == g).all() for a, g in zip(again, got))
    rec = len(data) // reads
    bad = bytearray(data)
    at = (reads - 3) * rec + 1 + 8 + 1  # the first byte of a sequence line near the end ...
    bad[at] = 10  # ... becomes a newline: an empty sequence, five lines
    d2 = torch.from_numpy(np.frombuffer(bytes(bad), np.uint8).copy()).cuda()
    with pytest.raises(api.StralgAmdError) as e:
        gpu_ctx.fastq_index_dev(d2, len(bad))
    assert "code -4" in str(e.value)
    with pytest.raises(api.StralgAmdError) as e:
        gpu_ctx.fastq_index(bytes(bad))
    assert "code -4" in str(e.value)


def test_two_builds_are_identical(cases):
    """two builds of the same FASTA from fresh contexts: identical device SA, O and RO digests and identical SAM text"""
    c = cases["hg38/reads-1000-100-2/k2"]
    out = []
    for _ in range(2):
        ctx = stralg_amd.Context(0)
        try:
            with Index.from_fasta(c["fasta"], ctx=ctx) as idx:
                digests = []
                for r in range(len(idx.records)):
                    t = idx.device_tables(r)
                    digests.append(tuple(hashlib.sha256(t[k].tobytes()).hexdigest() for k in ("sa", "o", "ro")))
                out.append((digests, idx.map_reads(c["fastq"], c["k"])))
        finally:
            ctx.close()
    assert out[0] == out[1]
    check_case(c, out[0][1])


def test_live_count_on_the_gpu(gpu_ctx, cases):
    start = gpu_ctx.lib.sx_index_live_count()
    with Index.from_fasta(cases["test-out/k0"]["fasta"], ctx=gpu_ctx):
        assert gpu_ctx.lib.sx_index_live_count() == start + 1
    with pytest.raises(api.StralgAmdError):
        Index.from_fasta(b">cut off", ctx=gpu_ctx)
    assert gpu_ctx.lib.sx_index_live_count() == start
