"""The compact index on the GPU (sx_occ.hip, Index(compact=True): BWT blocks with occurrence counts sampled every 64 rows
in place of the O / RO tables): the kernels' edge cases of tests/occ_cases.py (the CPU harness runs the same list), the
searches over blocks against the searches over full tables, the reference mapper's stdout through a compact index and
through the tool's --compact, the index file out of one, its memory, its failure paths, and a record of 2^24 symbols."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import approx_model
import occ_cases as oc
import stralg_amd
from approx_cases import approx_cases, remapped
from conftest import genome_cases
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
def compact_of(gpu_ctx):
    def get(fasta):
        if fasta not in _INDEXES:
            _INDEXES[fasta] = Index.from_fasta(fasta, ctx=gpu_ctx, compact=True)
        return _INDEXES[fasta]
    yield get
    for idx in _INDEXES.values():
        idx.close()
    _INDEXES.clear()


# ---- kernel edge cases -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letters", oc.LETTERS)
def test_records_at_the_block_edges(gpu_ctx, letters):
    seen = set()
    for symbols, l, fasta in oc.record_cases():
        if l == letters:
            N, sigma = oc.check_record(gpu_ctx, Index, fasta, api, gpu=True)
            assert N == symbols + 1 and sigma == min(symbols, letters) + 1
            seen.add(sigma)
    assert max(seen) == letters + 1 and 1 in seen


def test_build_dev_and_expand_dev_on_a_raw_bwt(gpu_ctx, mem):
    """sx_occ_compact_build_dev / _expand_dev on their own, several tiles of 64 blocks, against numpy's running counts;
    twice: the same bytes"""
    import torch
    rng = np.random.default_rng(4)
    for N, sigma in ((37 * 4096 + 77, 5), (4096, 2), (4097, 21), (130, 128)):
        bwt = rng.integers(0, sigma, N).astype(np.uint8)
        want = np.zeros((N + 1, sigma), np.uint32)
        want[1:] = np.cumsum(bwt[:, None] == np.arange(sigma)[None, :], axis=0)
        nbytes = gpu_ctx.occ_compact_bytes(N, sigma)
        d_bwt = torch.from_numpy(bwt).cuda()
        both = []
        for _ in range(2):
            d_blocks = torch.full((nbytes + 256,), 0x5A, dtype=torch.uint8, device="cuda")
            assert d_blocks.data_ptr() % 256 == 0
            d_rows = torch.zeros((N + 1) * sigma, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            gpu_ctx.occ_compact_build_dev(d_bwt, N, sigma, d_blocks)
            gpu_ctx.occ_compact_expand_dev(d_blocks, N, sigma, 0, N + 1, d_rows)
            raw = d_blocks.cpu().numpy()
            assert (raw[nbytes:] == 0x5A).all()  # (nothing behind the last block is written)
            assert (raw[:nbytes].reshape(-1, oc.stride(sigma)) == oc.reference_blocks(want, N, sigma)).all(), (N, sigma)
            assert (d_rows.cpu().numpy().view(np.uint32).reshape(N + 1, sigma) == want).all(), (N, sigma)
            both.append(raw.tobytes())
        assert both[0] == both[1]
        with pytest.raises(api.StralgAmdError, match=str(_lib.SX_E_ARG)):
            gpu_ctx.occ_compact_expand_dev(d_blocks[8:], N, sigma, 0, 1, d_rows)
        with pytest.raises(api.StralgAmdError, match=str(_lib.SX_E_ARG)):
            gpu_ctx.occ_compact_expand_dev(d_blocks, N, sigma, 0, N + 2, d_rows)


# ---- search ----------------------------------------------------------------------------------------------------------
_APPROX = approx_cases()


@pytest.mark.parametrize("name", sorted(_APPROX))
def test_searches_over_blocks_equal_the_full_tables(gpu_ctx, mem, name):
    cs = _APPROX[name]
    sym, sigma = remapped(cs["raw"])
    oc.check_searches(gpu_ctx, mem, Index, cs, approx_model.tables(sym, sigma) + (sigma,), _lib.APPROX_HIT_DTYPE, api)


# ---- index, end to end -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_compact_from_fasta_equals_the_reference(gpu_ctx, cases, compact_of, name):
    c = cases[name]
    idx = compact_of(c["fasta"])
    assert idx.compact
    check_case(c, idx.map_reads(c["fastq"], c["k"]))


@pytest.mark.parametrize("name", NAMES)
def test_compact_from_tables_equals_the_reference(gpu_ctx, cases, name):
    c = cases[name]
    with Index.from_tables(oracle_records(gpu_ctx, c["fasta"]), ctx=gpu_ctx, compact=True) as idx:
        assert idx.compact
        check_case(c, idx.map_reads(c["fastq"], c["k"]))


@pytest.mark.parametrize("name", NAMES)
def test_tool_compact_in_memory_equals_the_reference(mapper, cases, name, tmp_path):
    c = cases[name]
    fa, fq = tmp_path / "genome.fa", tmp_path / "reads.fq"
    fa.write_bytes(c["fasta"])
    fq.write_bytes(c["fastq"])
    got = subprocess.run([mapper, "-i", "--compact", "-d", str(c["k"]), str(fa), str(fq)], check=True, stdout=subprocess.PIPE,
                         stderr=subprocess.DEVNULL, timeout=300).stdout
    check_case(c, got)
    assert not os.path.exists(str(fa) + ".bwttables")


def test_tool_compact_on_a_saved_index(gpu_ctx, mapper, cases, tmp_path):
    """-p writes the same file with and without --compact; -d --compact on it prints the reference's text"""
    c = cases["two-records/k1"]
    fa, fq = tmp_path / "genome.fa", tmp_path / "reads.fq"
    fa.write_bytes(c["fasta"])
    fq.write_bytes(c["fastq"])
    run = lambda *args: subprocess.run([mapper] + list(args), check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                                       timeout=300).stdout
    run("-p", str(fa))
    plain = (tmp_path / "genome.fa.bwttables").read_bytes()
    run("--compact", "-p", str(fa))
    assert (tmp_path / "genome.fa.bwttables").read_bytes() == plain
    check_case(c, run("--compact", "-d", str(c["k"]), str(fa), str(fq)))
    with Index.from_fasta(c["fasta"], ctx=gpu_ctx, compact=True) as idx:
        chunks = []
        idx.write(chunks.append)
    assert b"".join(chunks) == plain


# ---- saving and loading ----------------------------------------------------------------------------------------------
def test_write_of_a_compact_index_streams_several_windows(gpu_ctx):
    """one record of 2^22 symbols (sigma 5, with RO): O and RO are 84 MB each, three windows of the 32 MiB staging
    buffers; the stream's SHA-256 is that of a full index's stream of the same FASTA"""
    n = 1 << 22
    fasta = fasta_of([(b"chrW", np.frombuffer(b"\0ACGT", np.uint8)[stralg_amd.synth(n, 5, 303)])])
    digests, sizes = [], []
    for compact in (False, True):
        h, size, longest = hashlib.sha256(), [0], [0]

        def sink(chunk):
            h.update(chunk)
            size[0] += len(chunk)
            longest[0] = max(longest[0], len(chunk))

        with Index.from_fasta(fasta, ctx=gpu_ctx, compact=compact) as idx:
            assert idx.records == [(b"chrW", n + 1, 5, True)] and idx.compact == compact
            idx.write(sink)
        digests.append(h.digest())
        sizes.append(size[0])
        assert longest[0] <= 32 << 20
    assert (n + 2) * 5 * 4 > 2 * (32 << 20)  # (a third window)
    assert sizes[0] == sizes[1] > 2 * (n + 2) * 5 * 4 and digests[0] == digests[1]


def test_load_compact_maps_the_same(gpu_ctx, cases, compact_of):
    c = cases["two-records/k1"]
    chunks = []
    compact_of(c["fasta"]).write(chunks.append)
    image = b"".join(chunks)
    with Index.load(image, ctx=gpu_ctx, compact=True) as loaded:
        assert loaded.compact and loaded.records == compact_of(c["fasta"]).records
        for r in range(len(loaded.records)):
            for rev in (False, True):
                assert (loaded.device_occ(r, reverse=rev) == compact_of(c["fasta"]).device_occ(r, reverse=rev)).all()
        check_case(c, loaded.map_reads(c["fastq"], c["k"]))


# ---- memory ----------------------------------------------------------------------------------------------------------
def test_device_bytes_of_a_compact_index(gpu_ctx, cases, compact_of):
    for name in ("test-out/k0", "two-records/k1"):
        idx = compact_of(cases[name]["fasta"])
        least, most = oc.memory_bounds(idx.records)
        assert least <= idx.device_bytes <= most, name
    g = genome_cases()["hg38-10000.fa"]
    with Index.from_fasta(g["file"], ctx=gpu_ctx) as full, Index.from_fasta(g["file"], ctx=gpu_ctx, compact=True) as comp:
        least, most = oc.memory_bounds(comp.records)
        assert least <= comp.device_bytes <= most
        assert comp.device_bytes < full.device_bytes / 4


# ---- failure paths ---------------------------------------------------------------------------------------------------
def test_failed_compact_builds_leave_nothing(gpu_ctx):
    start = gpu_ctx.lib.sx_index_live_count()
    with pytest.raises(api.StralgAmdError) as e:
        Index.from_fasta(b">cut off", ctx=gpu_ctx, compact=True)
    assert "code -4" in str(e.value)
    assert gpu_ctx.lib.sx_index_live_count() == start


def test_the_record_without_symbols_in_a_compact_index(gpu_ctx):
    with Index.from_fasta(b">empty\n>full\nACGT\n", ctx=gpu_ctx, compact=True) as idx:
        assert idx.records == [(b"empty", 1, 1, True), (b"full", 5, 5, True)]
        with pytest.raises(api.StralgAmdError) as e:
            idx.map_reads(b"@r\nAC\n+\nII\n", 0)
        assert "code -1" in str(e.value)


def test_a_compact_index_refuses_a_context_on_another_device(gpu_ctx, cases, compact_of):
    if gpu_ctx.lib.sx_device_count() < 2:
        pytest.skip("one device: a context on another one cannot be made")
    other = api.Context(1)
    try:
        with pytest.raises(api.StralgAmdError) as e:
            compact_of(cases["test-out/k0"]["fasta"]).map_reads(b"@r\nA\n+\nI\n", 0, ctx=other)
        assert "code -1" in str(e.value)
    finally:
        other.close()


# ---- at size ---------------------------------------------------------------------------------------------------------
def test_at_size_agrees_with_the_full_index(gpu_ctx):
    """a record of 2^24 symbols, 10^5 reads of 100 with up to one substitution, k = 1 (test_gpu_index's
    test_at_size_agrees_with_the_stream_call): the compact index's text has the SHA-256 of the full index's from the same
    context; two compact builds from fresh contexts have the same block digests"""
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
    digests, sizes, nbytes = [], [], []
    for compact in (False, True):
        with Index.from_fasta(fasta, ctx=gpu_ctx, compact=compact) as idx:
            h, size = hashlib.sha256(), [0]

            def sink(chunk):
                h.update(chunk)
                size[0] += len(chunk)

            idx.map_reads(fastq, 1, sink=sink)
            digests.append(h.digest())
            sizes.append(size[0])
            nbytes.append(idx.device_bytes)
    assert sizes[0] == sizes[1] > reads * 200 and digests[0] == digests[1]
    assert nbytes[1] < nbytes[0] / 4
    blocks = []
    for _ in range(2):
        ctx = stralg_amd.Context(0)
        try:
            with Index.from_fasta(fasta, ctx=ctx, compact=True) as idx:
                blocks.append(tuple(hashlib.sha256(idx.device_occ(0, reverse=rev).tobytes()).hexdigest() for rev in (False, True)))
        finally:
            ctx.close()
    assert blocks[0] == blocks[1] and blocks[0][0] != blocks[0][1]
