"""The sampled suffix array of the compact index on the GPU (sx_locate.hip, Index(compact=True, sa_sample=s): SA values at
a sampling distance in place of the suffix array, the others located by LF walks over the BWT blocks): the kernels' edge
cases of tests/sa_sample_cases.py (the CPU harness runs the same list), the reference mapper's stdout through a sampled
index and through the tool's --sa-sample, long hits in runs, the index file out of one, its memory, its failure paths, and
a record of 2^24 symbols."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import occ_cases as oc
import sa_sample_cases as sc
import stralg_amd
from device_memory import GpuMemory
from sam_cases import ROOT, check_case, sam_cases
from stralg_amd import Index, _lib, api
from test_gpu_index import NAMES, fasta_of, fastq_of, read_names
from test_index_cpu import oracle_records

pytestmark = pytest.mark.gpu

MAPPER = os.path.join(ROOT, "tools", "stralg_amd_readmapper")


@pytest.fixture(scope="module")
def cases():
    return sam_cases()


@pytest.fixture(scope="module")
def mem():
    return GpuMemory()


@pytest.fixture(scope="module")
def mapper():
    if not os.path.exists(MAPPER):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "stralg_amd", "csrc"), "mapper"])
    return MAPPER


_INDEXES = {}


@pytest.fixture(scope="module")
def sampled_of(gpu_ctx):
    yield lambda how, fasta, sa_sample: sc.sampled_index(_INDEXES, gpu_ctx, Index, oracle_records, how, fasta, sa_sample)
    for idx in _INDEXES.values():
        if hasattr(idx, "close"):
            idx.close()
    _INDEXES.clear()


# ---- kernel edge cases -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letters", oc.LETTERS)
def test_records_at_the_block_edges(gpu_ctx, letters):
    seen = set()
    for symbols, l, fasta in oc.record_cases():
        if l == letters:
            N, sigma = sc.check_record(gpu_ctx, Index, fasta, api, gpu=True)
            assert N == symbols + 1 and sigma == min(symbols, letters) + 1
            seen.add(sigma)
    assert max(seen) == letters + 1 and 1 in seen


@pytest.mark.parametrize("name", sorted(sc.odd_texts()))
def test_texts_that_walk_oddly(gpu_ctx, name):
    N, sigma = sc.check_record(gpu_ctx, Index, sc.odd_texts()[name], api, gpu=True)
    assert (N, sigma) == {"one-letter": (1001, 2), "acgt": (1201, 5)}[name]


def test_the_record_without_symbols(gpu_ctx):
    with Index.from_fasta(b">empty\n>full\nACGT\n", ctx=gpu_ctx, compact=True, sa_sample=32) as idx:
        assert idx.records == [(b"empty", 1, 1, True), (b"full", 5, 5, True)] and idx.sa_sample == 32
        assert idx.record_samples(0).n_samples == 1 and idx.expand_sa(0).tolist() == [0]
        with pytest.raises(api.StralgAmdError) as e:
            idx.map_reads(b"@r\nAC\n+\nII\n", 0)
        assert "code -1" in str(e.value)


@pytest.mark.parametrize("N,sigma,q", sc.KERNEL_SHAPES)
def test_sample_and_locate_on_their_own(gpu_ctx, mem, N, sigma, q):
    sc.check_kernels(gpu_ctx, mem, api, N, sigma, q)


# ---- index, end to end -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sa_sample", [4, 32])
@pytest.mark.parametrize("name", NAMES)
def test_sampled_indexes_equal_the_reference(gpu_ctx, cases, sampled_of, name, sa_sample):
    c = cases[name]
    for how in ("from_fasta", "from_tables", "load"):
        idx = sampled_of(how, c["fasta"], sa_sample)
        assert idx.sa_sample == sa_sample and all(idx.record_samples(r).sa_log2 for r in range(len(idx.records)))
        check_case(c, idx.map_reads(c["fastq"], c["k"]))


@pytest.mark.parametrize("name", NAMES)
def test_tool_sampled_in_memory_equals_the_reference(mapper, cases, name, tmp_path):
    c = cases[name]
    fa, fq = tmp_path / "genome.fa", tmp_path / "reads.fq"
    fa.write_bytes(c["fasta"])
    fq.write_bytes(c["fastq"])
    got = subprocess.run([mapper, "-i", "--compact", "--sa-sample", "32", "-d", str(c["k"]), str(fa), str(fq)], check=True,
                         stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=300).stdout
    check_case(c, got)
    assert not os.path.exists(str(fa) + ".bwttables")


def test_long_hits_and_runs(gpu_ctx):
    sc.check_long_hits(gpu_ctx, Index)


# ---- saving ----------------------------------------------------------------------------------------------------------
def test_write_and_the_tool_on_a_saved_index(gpu_ctx, mapper, cases, sampled_of, tmp_path):
    """write() of a sampled index equals the full index's bytes; -p writes the same file with and without --compact
    --sa-sample; -d on it prints the reference's text; refused options"""
    c = cases["two-records/k1"]
    fa, fq = tmp_path / "genome.fa", tmp_path / "reads.fq"
    fa.write_bytes(c["fasta"])
    fq.write_bytes(c["fastq"])
    run = lambda *args: subprocess.run([mapper] + list(args), check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=300).stdout
    run("-p", str(fa))
    plain = (tmp_path / "genome.fa.bwttables").read_bytes()
    run("-p", "--compact", "--sa-sample", "32", str(fa))
    assert (tmp_path / "genome.fa.bwttables").read_bytes() == plain
    check_case(c, run("--compact", "--sa-sample", "32", "-d", str(c["k"]), str(fa), str(fq)))
    with Index.from_fasta(c["fasta"], ctx=gpu_ctx) as full:
        assert sc.written(full) == plain
    assert sc.written(sampled_of("from_fasta", c["fasta"], 32)) == plain
    for bad in (["--sa-sample", "32"], ["--compact", "--sa-sample", "3"]):
        assert subprocess.run([mapper] + bad + ["-d", "1", str(fa), str(fq)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                              timeout=300).returncode != 0


# ---- memory ----------------------------------------------------------------------------------------------------------
def test_device_bytes_of_a_sampled_index(gpu_ctx, cases, sampled_of):
    for name in ("test-out/k0", "two-records/k1", "hg38/reads-100-10-0/k0"):
        for q in (2, 5):
            idx = sampled_of("from_fasta", cases[name]["fasta"], 1 << q)
            least, most = sc.memory_bounds(idx.records, q)
            assert least <= idx.device_bytes <= most, (name, q)


# ---- failure paths ---------------------------------------------------------------------------------------------------
def test_failure_paths_leave_nothing(gpu_ctx):
    sc.check_failure_paths(gpu_ctx, Index, api, _lib)


# ---- at size ---------------------------------------------------------------------------------------------------------
def test_at_size_agrees_with_the_compact_index(gpu_ctx):
    """a record of 2^24 symbols, 10^5 reads of 100 with up to one substitution, k = 1 (test_gpu_occ's
    test_at_size_agrees_with_the_full_index): the text and the written index of the sampled index (s = 32) have the SHA-256
    of the compact index's from the same context (the suffix array section is 64 MB: two staging windows); its
    device_bytes are below 0.62 of the compact index's (the layout gives 5.375 N against 9 N, 0.597; the margin covers the
    per-buffer rounding); two sampled builds from fresh contexts have the same marks and values digests"""
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
    text, image, sizes, nbytes = [], [], [], []
    for sa_sample in (0, 32):
        with Index.from_fasta(fasta, ctx=gpu_ctx, compact=True, sa_sample=sa_sample) as idx:
            assert idx.sa_sample == sa_sample
            for out, call in ((text, lambda sink: idx.map_reads(fastq, 1, sink=sink)), (image, idx.write)):
                h, size = hashlib.sha256(), [0]

                def sink(chunk):
                    h.update(chunk)
                    size[0] += len(chunk)

                call(sink)
                out.append(h.digest())
                sizes.append(size[0])
            nbytes.append(idx.device_bytes)
    assert sizes[0] == sizes[2] > reads * 200 and text[0] == text[1]
    assert sizes[1] == sizes[3] > 4 * (n + 1) and image[0] == image[1]
    assert 4 * (n + 1) > (32 << 20)  # (the suffix array section: a second staging window)
    print("device_bytes compact %d sampled %d ratio %.4f" % (nbytes[0], nbytes[1], nbytes[1] / nbytes[0]))
    assert nbytes[1] < 0.62 * nbytes[0]
    digests = []
    for _ in range(2):
        ctx = stralg_amd.Context(0)
        try:
            with Index.from_fasta(fasta, ctx=ctx, compact=True, sa_sample=32) as idx:
                digests.append(tuple(hashlib.sha256(x.tobytes()).hexdigest() for x in idx.device_samples(0)))
        finally:
            ctx.close()
    assert digests[0] == digests[1] and digests[0][0] != digests[0][1]
