"""The packed form of the compact index (sx_occ.hpp OccPacked, Index(compact=True, packed=True): the 64-row blocks with a
nibble a row, for alphabets of up to 8 symbols) through the CPU execution harness: the kernels' edge cases
(tests/packed_cases.py; the GPU runs the same list), the raw calls, the searches over packed blocks against the searches
over full tables and the reference iterator's streams, the reference mapper's stdout through a packed index with and
without a sampled suffix array, the reference writer's byte streams out of one, its memory, its failure paths.  (The
harness stages 4096 bytes a chunk: every table here crosses many windows.)"""
import struct

import pytest

import approx_model
import packed_cases as pc
from approx_cases import approx_cases, remapped
from conftest import genome_cases, serial_cases
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
def packed_of(emu_ctx):
    """(fasta bytes, sa_sample) -> Index.from_fasta(compact=True, packed=True, sa_sample=..) of it (one build each)"""
    def get(fasta, sa_sample=0):
        if (fasta, sa_sample) not in _INDEXES:
            _INDEXES[(fasta, sa_sample)] = Index.from_fasta(fasta, ctx=emu_ctx, compact=True, packed=True, sa_sample=sa_sample)
        return _INDEXES[(fasta, sa_sample)]
    yield get
    for idx in _INDEXES.values():
        idx.close()
    _INDEXES.clear()


def written(idx):
    chunks = []
    idx.write(chunks.append)
    assert max(len(x) for x in chunks) <= 4096  # (the harness's staging chunk: the tables left in many windows)
    return b"".join(chunks)


# ---- 1. block edges --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symbols,letters", [(n, l) for n, l, _ in pc.record_cases()])
def test_records_at_the_block_edges(emu_ctx, symbols, letters):
    fasta = [f for n, l, f in pc.record_cases() if (n, l) == (symbols, letters)][0]
    N, sigma = pc.check_record(emu_ctx, Index, fasta, api)
    assert N == symbols + 1 and sigma == min(symbols, letters) + 1


# ---- 2. raw calls ----------------------------------------------------------------------------------------------------
def test_build_dev_and_expand_dev_on_a_raw_bwt(emu_ctx):
    pc.check_raw_calls(emu_ctx, MEM, api, pc.RAW_SHAPES_HARNESS)


# ---- 3. searches -----------------------------------------------------------------------------------------------------
_APPROX = approx_cases()
_SMALL, _LARGE = pc.split_cases(_APPROX, remapped)


def test_the_cases_that_fit_the_packed_form():
    assert len(_SMALL) >= 31 and _LARGE
    for name in _APPROX:
        if name.startswith(("rand/s4", "rand/s5", "rand/s8", "ref/", "struct/")):
            assert name in _SMALL, name
        if name.startswith("rand/s13"):
            assert name in _LARGE, name


@pytest.mark.parametrize("name", _SMALL)
def test_searches_over_packed_blocks_equal_the_full_tables(emu_ctx, name):
    cs = _APPROX[name]
    sym, sigma = remapped(cs["raw"])
    pc.check_searches(emu_ctx, MEM, Index, cs, approx_model.tables(sym, sigma) + (sigma,), _lib.APPROX_HIT_DTYPE, api)


@pytest.mark.parametrize("name", _LARGE)
def test_more_than_8_symbols_are_refused(emu_ctx, name):
    sym, sigma = remapped(_APPROX[name]["raw"])
    pc.check_refuses_large_sigma(emu_ctx, Index, approx_model.tables(sym, sigma) + (sigma,), api)


# ---- 4. end to end ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_packed_indexes_map_the_fixture_cases(emu_ctx, cases, packed_of, name):
    """from_fasta, from_fasta with a suffix array sampled at 2 and at 32, from_tables: the reference mapper's recorded stdout"""
    c = cases[name]
    ran = 0
    for sa_sample in (0, 2, 32):
        idx = packed_of(c["fasta"], sa_sample)
        assert idx.compact and idx.packed and idx.sa_sample == sa_sample
        assert all(sigma <= 6 for _, _, sigma, _ in idx.records)
        check_case(c, idx.map_reads(c["fastq"], c["k"]))
        ran += 1
    with Index.from_tables(oracle_records(emu_ctx, c["fasta"]), ctx=emu_ctx, compact=True, packed=True) as idx:
        assert idx.packed and all(idx.record_occ(r).compact == 2 for r in range(len(idx.records)))
        check_case(c, idx.map_reads(c["fastq"], c["k"]))
        ran += 1
    assert ran == 4


@pytest.mark.parametrize("sa_sample", [0, 32])
def test_small_batches_and_windows_through_a_packed_index(emu_ctx, cases, packed_of, sa_sample):
    c = cases["two-records/k1"]
    emu_ctx.set_sam_batch_reads(7)
    emu_ctx.set_sam_window_bytes(4096)
    try:
        check_case(c, packed_of(c["fasta"], sa_sample).map_reads(c["fastq"], c["k"]))
    finally:
        emu_ctx.set_sam_batch_reads(0)
        emu_ctx.set_sam_window_bytes(0)


# ---- 5. saving and loading -------------------------------------------------------------------------------------------
def test_save_of_a_packed_index_equals_the_reference_writer(emu_ctx):
    ran = 0
    for name, c in serial_cases().items():
        fasta = b">" + name.encode() + b"\n" + c["raw"] + b"\n"
        head = struct.pack("<I", 1) + struct.pack("<I", len(name) + 1) + name.encode() + b"\0"
        sigma = remapped(c["raw"])[1]
        if sigma > pc.MAX_SIGMA:  # (ref-serialise: 9 letters)
            start = emu_ctx.lib.sx_index_live_count()
            with pytest.raises(api.StralgAmdError, match="code -1"):
                Index.from_fasta(fasta, ctx=emu_ctx, compact=True, packed=True)
            assert emu_ctx.lib.sx_index_live_count() == start
            with Index.from_fasta(fasta, ctx=emu_ctx) as full:
                with pytest.raises(api.StralgAmdError, match="code -1"):
                    Index.load(written(full), ctx=emu_ctx, compact=True, packed=True)
            assert emu_ctx.lib.sx_index_live_count() == start
            continue
        for rev, want in ((True, c["with_reverse"]), (False, c["forward_only"])):
            for sa_sample in (0, 4):
                with Index.from_fasta(fasta, include_reverse=rev, ctx=emu_ctx, compact=True, packed=True, sa_sample=sa_sample) as idx:
                    assert written(idx) == head + want, (name, rev, sa_sample)
                    assert [r[3] for r in idx.records] == [rev]
                    ran += 1
    assert ran >= 4 and remapped(serial_cases()["ref-serialise"]["raw"])[1] == 10


def test_load_packed_maps_and_saves_the_same(emu_ctx, cases, packed_of, tmp_path):
    c = cases["two-records/k1"]
    with Index.from_fasta(c["fasta"], ctx=emu_ctx) as full:
        image = written(full)
    for sa_sample in (0, 32):
        built = packed_of(c["fasta"], sa_sample)
        assert written(built) == image
        with Index.load(image, ctx=emu_ctx, compact=True, packed=True, sa_sample=sa_sample) as loaded:
            assert loaded.packed and loaded.sa_sample == sa_sample and loaded.records == built.records
            for r in range(len(loaded.records)):
                for rev in (False, True):
                    assert loaded.device_occ(r, reverse=rev).tobytes() == built.device_occ(r, reverse=rev).tobytes()
            check_case(c, loaded.map_reads(c["fastq"], c["k"]))
            assert written(loaded) == image
    with Index.load(image, ctx=emu_ctx, compact=True) as plain:
        assert plain.compact and not plain.packed


# ---- 6. expand_sa ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symbols,letters", [(n, l) for n, l, _ in pc.record_cases()])
def test_expand_sa_of_a_packed_sampled_index(emu_ctx, symbols, letters):
    fasta = [f for n, l, f in pc.record_cases() if (n, l) == (symbols, letters)][0]
    pc.check_expand_sa(emu_ctx, Index, fasta)


# ---- 7. memory -------------------------------------------------------------------------------------------------------
def test_device_bytes_of_a_packed_index(emu_ctx, cases, packed_of):
    for name in ("test-out/k0", "two-records/k1", "hg38/reads-100-10-0/k0"):
        for sa_sample in (0, 32):
            idx = packed_of(cases[name]["fasta"], sa_sample)
            least, most = pc.memory_bounds(emu_ctx, idx.records, sa_sample)
            assert least <= idx.device_bytes <= most, (name, sa_sample)
    fasta = cases["hg38/reads-100-10-0/k0"]["fasta"]
    assert fasta == genome_cases()["hg38-10000.fa"]["file"]
    with Index.from_fasta(fasta, ctx=emu_ctx, compact=True) as comp:
        assert packed_of(fasta).device_bytes < comp.device_bytes


# ---- 8. failure paths ------------------------------------------------------------------------------------------------
def test_failure_paths_leave_nothing(emu_ctx):
    pc.check_failure_paths(emu_ctx, Index, api, _lib)


def test_the_record_without_symbols_in_a_packed_index(emu_ctx):
    pc.check_the_record_without_symbols(emu_ctx, Index, api, written)
