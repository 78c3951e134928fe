"""The sampled suffix array of the compact index (sx_locate.hip, Index(compact=True, sa_sample=s): SA values at a sampling
distance in place of the suffix array, the others located by LF walks over the BWT blocks) through the CPU execution
harness: the kernels' edge cases (tests/sa_sample_cases.py; the GPU runs the same list), the reference mapper's stdout
through a sampled index, long hits in runs, the index file out of one, its memory, its failure paths.  (The harness stages
4096 bytes a chunk: a suffix array from the host takes a window every 16 blocks, a saved one a window every 1024 rows.)"""
import numpy as np
import pytest

import occ_cases as oc
import sa_sample_cases as sc
from device_memory import HarnessMemory
from sam_cases import check_case, sam_cases
from stralg_amd import Index, _lib, api
from test_index_cpu import NAMES, oracle_records

MEM = HarnessMemory()


@pytest.fixture(scope="module")
def cases():
    return sam_cases()


_INDEXES = {}


@pytest.fixture(scope="module")
def sampled_of(emu_ctx):
    """(how, fasta bytes, sa_sample) -> the sampled index of it, made by from_fasta, from_tables or load (one build each for
    the whole module)"""
    yield lambda how, fasta, sa_sample: sc.sampled_index(_INDEXES, emu_ctx, Index, oracle_records, how, fasta, sa_sample)
    for idx in _INDEXES.values():
        if hasattr(idx, "close"):
            idx.close()
    _INDEXES.clear()


# ---- kernel edge cases -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symbols,letters", [(n, l) for n, l, _ in oc.record_cases()])
def test_records_at_the_block_edges(emu_ctx, symbols, letters):
    fasta = [f for n, l, f in oc.record_cases() if (n, l) == (symbols, letters)][0]
    N, sigma = sc.check_record(emu_ctx, Index, fasta, api)
    assert N == symbols + 1 and sigma == min(symbols, letters) + 1


@pytest.mark.parametrize("name", sorted(sc.odd_texts()))
def test_texts_that_walk_oddly(emu_ctx, name):
    N, sigma = sc.check_record(emu_ctx, Index, sc.odd_texts()[name], api)
    assert (N, sigma) == {"one-letter": (1001, 2), "acgt": (1201, 5)}[name]


def test_the_record_without_symbols(emu_ctx):
    fasta = b">empty\n>full\nACGT\n"
    with Index.from_fasta(fasta, ctx=emu_ctx, compact=True, sa_sample=32) as idx, Index.from_fasta(fasta, ctx=emu_ctx) as full:
        assert idx.records == [(b"empty", 1, 1, True), (b"full", 5, 5, True)] and idx.sa_sample == 32
        assert idx.record_samples(0).n_samples == 1 and idx.expand_sa(0).tolist() == [0]
        assert (idx.expand_sa(1) == full.device_tables(1)["sa"]).all()
        assert sc.written(idx) == sc.written(full)
        with pytest.raises(api.StralgAmdError) as e:
            idx.map_reads(b"@r\nAC\n+\nII\n", 0)
        assert "code -1" in str(e.value)


@pytest.mark.parametrize("N,sigma,q", sc.KERNEL_SHAPES)
def test_sample_and_locate_on_their_own(emu_ctx, N, sigma, q):
    sc.check_kernels(emu_ctx, MEM, api, N, sigma, q)


# ---- index, end to end -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sa_sample", [4, 32])
@pytest.mark.parametrize("name", NAMES)
def test_sampled_indexes_map_the_fixture_cases(emu_ctx, cases, sampled_of, name, sa_sample):
    """from_fasta, from_tables and load of the same genome: the reference mapper's recorded stdout, byte for byte"""
    c = cases[name]
    for how in ("from_fasta", "from_tables", "load"):
        idx = sampled_of(how, c["fasta"], sa_sample)
        assert idx.sa_sample == sa_sample and all(idx.record_samples(r).sa_log2 for r in range(len(idx.records)))
        check_case(c, idx.map_reads(c["fastq"], c["k"]))


def test_small_batches_windows_and_runs(emu_ctx, cases):
    c = cases["two-records/k1"]
    emu_ctx.set_sam_batch_reads(7)
    emu_ctx.set_sam_window_bytes(4096)
    emu_ctx.set_locate_chunk_rows(5)
    try:
        with Index.from_fasta(c["fasta"], ctx=emu_ctx, compact=True, sa_sample=8) as idx:
            check_case(c, idx.map_reads(c["fastq"], c["k"]))
    finally:
        emu_ctx.set_sam_batch_reads(0)
        emu_ctx.set_sam_window_bytes(0)
        emu_ctx.set_locate_chunk_rows(0)


def test_long_hits_and_runs(emu_ctx):
    sc.check_long_hits(emu_ctx, Index)


# ---- saving ----------------------------------------------------------------------------------------------------------
def test_write_of_a_sampled_index_equals_the_full_index(emu_ctx, cases):
    c = cases["two-records/k1"]
    with Index.from_fasta(c["fasta"], ctx=emu_ctx) as full:
        image = sc.written(full)
    for s in (2, 32, 1024):
        with Index.from_fasta(c["fasta"], ctx=emu_ctx, compact=True, sa_sample=s) as idx:
            chunks = []
            idx.write(chunks.append)
            assert b"".join(chunks) == image, s
            assert max(len(x) for x in chunks) <= 4096  # (the harness's staging chunk: the suffix array left in many windows)
        with Index.load(image, ctx=emu_ctx, compact=True, sa_sample=s) as loaded:
            assert sc.written(loaded) == image, s


# ---- memory ----------------------------------------------------------------------------------------------------------
def test_device_bytes_of_a_sampled_index(emu_ctx, cases, sampled_of):
    for name in ("test-out/k0", "two-records/k1", "hg38/reads-100-10-0/k0"):
        for q in (2, 5):
            idx = sampled_of("from_fasta", cases[name]["fasta"], 1 << q)
            least, most = sc.memory_bounds(idx.records, q)
            assert least <= idx.device_bytes <= most, (name, q)


# ---- failure paths ---------------------------------------------------------------------------------------------------
def test_failure_paths_leave_nothing(emu_ctx):
    sc.check_failure_paths(emu_ctx, Index, api, _lib)
