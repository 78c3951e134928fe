"""The packed form of the compact index on the GPU (sx_occ.hpp OccPacked, Index(compact=True, packed=True): the 64-row
blocks with a nibble a row, for alphabets of up to 8 symbols): the kernels' edge cases of tests/packed_cases.py (the CPU
harness runs the same list), the raw calls, the searches over packed blocks against the searches over full tables, the
reference mapper's stdout through a packed index and through the tool's --packed, the index file out of one, its
memory, its failure paths, and a record of 2^22 symbols."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import approx_model
import packed_cases as pc
import stralg_amd
from approx_cases import approx_cases, remapped
from conftest import genome_cases, serial_cases
from device_memory import GpuMemory
from sam_cases import ROOT, check_case, sam_cases
from stralg_amd import Index, _lib, api
from test_gpu_index import fasta_of, fastq_of, read_names
from test_index_cpu import NAMES, oracle_records

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
def packed_of(gpu_ctx):
    def get(fasta, sa_sample=0):
        if (fasta, sa_sample) not in _INDEXES:
            _INDEXES[(fasta, sa_sample)] = Index.from_fasta(fasta, ctx=gpu_ctx, compact=True, packed=True, sa_sample=sa_sample)
        return _INDEXES[(fasta, sa_sample)]
    yield get
    for idx in _INDEXES.values():
        idx.close()
    _INDEXES.clear()


def written(idx):
    chunks = []
    idx.write(chunks.append)
    return b"".join(chunks)


# ---- 1. block edges --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letters", pc.LETTERS)
def test_records_at_the_block_edges(gpu_ctx, letters):
    seen = set()
    for symbols, l, fasta in pc.record_cases():
        if l == letters:
            N, sigma = pc.check_record(gpu_ctx, Index, fasta, api, gpu=True)
            assert N == symbols + 1 and sigma == min(symbols, letters) + 1
            seen.add(sigma)
    assert max(seen) == letters + 1 and 1 in seen


# ---- 2. raw calls ----------------------------------------------------------------------------------------------------
def test_build_dev_and_expand_dev_on_a_raw_bwt(gpu_ctx, mem):
    pc.check_raw_calls(gpu_ctx, mem, api, pc.RAW_SHAPES_GPU)


# ---- 3. searches -----------------------------------------------------------------------------------------------------
_APPROX = approx_cases()
_SMALL, _LARGE = pc.split_cases(_APPROX, remapped)


def test_the_cases_that_fit_the_packed_form():
    assert len(_SMALL) >= 31 and _LARGE


@pytest.mark.parametrize("name", _SMALL)
def test_searches_over_packed_blocks_equal_the_full_tables(gpu_ctx, mem, name):
    cs = _APPROX[name]
    sym, sigma = remapped(cs["raw"])
    pc.check_searches(gpu_ctx, mem, Index, cs, approx_model.tables(sym, sigma) + (sigma,), _lib.APPROX_HIT_DTYPE, api)


@pytest.mark.parametrize("name", _LARGE)
def test_more_than_8_symbols_are_refused(gpu_ctx, name):
    sym, sigma = remapped(_APPROX[name]["raw"])
    pc.check_refuses_large_sigma(gpu_ctx, Index, approx_model.tables(sym, sigma) + (sigma,), api)


# ---- 4. end to end ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_packed_indexes_equal_the_reference(gpu_ctx, cases, packed_of, name):
    """from_fasta, from_fasta with a suffix array sampled at 2 and at 32, from_tables: the reference mapper's recorded stdout"""
    c = cases[name]
    ran = 0
    for sa_sample in (0, 2, 32):
        idx = packed_of(c["fasta"], sa_sample)
        assert idx.compact and idx.packed and idx.sa_sample == sa_sample
        assert all(sigma <= 6 for _, _, sigma, _ in idx.records)
        check_case(c, idx.map_reads(c["fastq"], c["k"]))
        ran += 1
    with Index.from_tables(oracle_records(gpu_ctx, c["fasta"]), ctx=gpu_ctx, compact=True, packed=True) as idx:
        assert idx.packed and all(idx.record_occ(r).compact == 2 for r in range(len(idx.records)))
        check_case(c, idx.map_reads(c["fastq"], c["k"]))
        ran += 1
    assert ran == 4


def test_tool_packed_equals_the_reference(gpu_ctx, mapper, cases, tmp_path):
    """-i --compact --packed and --compact --packed --sa-sample 32 (on a saved index) print the reference's text; -p writes
    the same file with and without --packed; --packed without --compact fails as --sa-sample does"""
    c = cases["two-records/k1"]
    fa, fq = tmp_path / "genome.fa", tmp_path / "reads.fq"
    fa.write_bytes(c["fasta"])
    fq.write_bytes(c["fastq"])
    run = lambda *args: subprocess.run([mapper] + list(args), check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                                       timeout=300).stdout
    check_case(c, run("-i", "--compact", "--packed", "-d", str(c["k"]), str(fa), str(fq)))
    assert not os.path.exists(str(fa) + ".bwttables")
    run("-p", str(fa))
    plain = (tmp_path / "genome.fa.bwttables").read_bytes()
    run("--compact", "--packed", "-p", str(fa))
    assert (tmp_path / "genome.fa.bwttables").read_bytes() == plain
    check_case(c, run("--compact", "--packed", "--sa-sample", "32", "-d", str(c["k"]), str(fa), str(fq)))
    check_case(c, run("-i", "--compact", "--packed", "--sa-sample", "32", "-d", str(c["k"]), str(fa), str(fq)))
    for args in (["--packed"], ["--sa-sample", "32"]):
        bad = subprocess.run([mapper, "-i"] + args + ["-d", str(c["k"]), str(fa), str(fq)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             timeout=300)
        assert bad.returncode != 0 and not bad.stdout and b"needs --compact" in bad.stderr
    with Index.from_fasta(c["fasta"], ctx=gpu_ctx, compact=True, packed=True) as idx:
        assert written(idx) == plain


# ---- 5. saving and loading -------------------------------------------------------------------------------------------
def test_save_of_a_packed_index_equals_the_reference_writer(gpu_ctx):
    import struct
    ran = 0
    for name, c in serial_cases().items():
        fasta = b">" + name.encode() + b"\n" + c["raw"] + b"\n"
        head = struct.pack("<I", 1) + struct.pack("<I", len(name) + 1) + name.encode() + b"\0"
        if remapped(c["raw"])[1] > pc.MAX_SIGMA:  # (ref-serialise: 9 letters)
            start = gpu_ctx.lib.sx_index_live_count()
            with pytest.raises(api.StralgAmdError, match="code -1"):
                Index.from_fasta(fasta, ctx=gpu_ctx, compact=True, packed=True)
            assert gpu_ctx.lib.sx_index_live_count() == start
            continue
        for sa_sample in (0, 4):
            with Index.from_fasta(fasta, ctx=gpu_ctx, compact=True, packed=True, sa_sample=sa_sample) as idx:
                assert written(idx) == head + c["with_reverse"], (name, sa_sample)
                ran += 1
    assert ran >= 2 and remapped(serial_cases()["ref-serialise"]["raw"])[1] == 10


def test_load_packed_maps_the_same(gpu_ctx, cases, packed_of):
    c = cases["two-records/k1"]
    with Index.from_fasta(c["fasta"], ctx=gpu_ctx) as full:
        image = written(full)
    for sa_sample in (0, 32):
        built = packed_of(c["fasta"], sa_sample)
        assert written(built) == image
        with Index.load(image, ctx=gpu_ctx, compact=True, packed=True, sa_sample=sa_sample) as loaded:
            assert loaded.packed and loaded.sa_sample == sa_sample and loaded.records == built.records
            for r in range(len(loaded.records)):
                for rev in (False, True):
                    assert loaded.device_occ(r, reverse=rev).tobytes() == built.device_occ(r, reverse=rev).tobytes()
            check_case(c, loaded.map_reads(c["fastq"], c["k"]))


# ---- 6. expand_sa ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letters", pc.LETTERS)
def test_expand_sa_of_a_packed_sampled_index(gpu_ctx, letters):
    for _, l, fasta in pc.record_cases():
        if l == letters:
            pc.check_expand_sa(gpu_ctx, Index, fasta)


# ---- 7. memory -------------------------------------------------------------------------------------------------------
def test_device_bytes_of_a_packed_index(gpu_ctx, cases, packed_of):
    for name in ("test-out/k0", "two-records/k1", "hg38/reads-100-10-0/k0"):
        for sa_sample in (0, 32):
            idx = packed_of(cases[name]["fasta"], sa_sample)
            least, most = pc.memory_bounds(gpu_ctx, idx.records, sa_sample)
            assert least <= idx.device_bytes <= most, (name, sa_sample)
    g = genome_cases()["hg38-10000.fa"]
    with Index.from_fasta(g["file"], ctx=gpu_ctx, compact=True) as comp:
        assert packed_of(g["file"]).device_bytes < comp.device_bytes


# ---- 8. failure paths ------------------------------------------------------------------------------------------------
def test_failure_paths_leave_nothing(gpu_ctx):
    pc.check_failure_paths(gpu_ctx, Index, api, _lib)


def test_the_record_without_symbols_in_a_packed_index(gpu_ctx):
    pc.check_the_record_without_symbols(gpu_ctx, Index, api, written)


# ---- 9. at size ------------------------------------------------------------------------------------------------------
def test_at_size_agrees_with_the_full_index(gpu_ctx):
    """a record of 2^22 symbols, 10^4 reads of 100 with up to one substitution, k = 1: the text's SHA-256 through the packed
    index, and through packed + sa_sample=32, is the full index's from the same context; write streams in chunks of at most
    32 MiB with the full index's digest; two packed builds from fresh contexts have equal block digests"""
    n, m, reads = 1 << 22, 100, 10_000
    letters = np.frombuffer(b"\0ACGT", np.uint8)
    seq = letters[stralg_amd.synth(n, 5, 303)]
    rng = np.random.default_rng(9)
    pos = rng.integers(0, n - m, reads)
    seqs = seq[pos[:, None] + np.arange(m)[None, :]].copy()
    hit = rng.integers(0, 2, reads).astype(bool)
    at = rng.integers(0, m, reads)
    seqs[hit, at[hit]] = letters[1 + (np.searchsorted(letters[1:], seqs[hit, at[hit]]) + 1) % 4]
    fastq = fastq_of(read_names(reads), seqs)
    fasta = fasta_of([(b"chrP", seq)])
    text, image, nbytes = [], [], []
    for kwargs in (dict(), dict(compact=True, packed=True), dict(compact=True, packed=True, sa_sample=32)):
        with Index.from_fasta(fasta, ctx=gpu_ctx, **kwargs) as idx:
            assert idx.records == [(b"chrP", n + 1, 5, True)] and idx.packed == bool(kwargs)
            h, size = hashlib.sha256(), [0]

            def sink(chunk):
                h.update(chunk)
                size[0] += len(chunk)

            idx.map_reads(fastq, 1, sink=sink)
            text.append((h.hexdigest(), size[0]))
            w, longest = hashlib.sha256(), [0]

            def wsink(chunk):
                w.update(chunk)
                longest[0] = max(longest[0], len(chunk))

            idx.write(wsink)
            assert longest[0] <= 32 << 20
            image.append(w.hexdigest())
            nbytes.append(idx.device_bytes)
    assert text[0][1] > reads * 200 and text[1] == text[0] and text[2] == text[0]
    assert image[1] == image[0] and image[2] == image[0]
    assert (n + 2) * 5 * 4 > 2 * (32 << 20)  # (O and RO each leave in three windows)
    assert nbytes[2] < nbytes[1] < nbytes[0] / 5
    blocks = []
    for _ in range(2):
        ctx = stralg_amd.Context(0)
        try:
            with Index.from_fasta(fasta, ctx=ctx, compact=True, packed=True) as idx:
                blocks.append(tuple(hashlib.sha256(idx.device_occ(0, reverse=rev).tobytes()).hexdigest() for rev in (False, True)))
        finally:
            ctx.close()
    assert blocks[0] == blocks[1] and blocks[0][0] != blocks[0][1]
