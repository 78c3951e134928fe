"""The compact index (sx_occ.hip, Index(compact=True): BWT blocks with occurrence counts sampled every 64 rows in place of
the O / RO tables) through the CPU execution harness: the kernels' edge cases (tests/occ_cases.py; the GPU runs the same
list), the searches over blocks against the searches over full tables and the reference iterator's streams, the
reference mapper's stdout through a compact index, the reference writer's byte streams out of one, its memory, its
failure paths.  (The harness stages 4096 bytes a chunk: every table here crosses many windows.)"""
import struct

import numpy as np
import pytest

import approx_model
import occ_cases as oc
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
def compact_of(emu_ctx):
    """fasta bytes -> Index.from_fasta(compact=True) of it (one build a genome for the whole module)"""
    def get(fasta):
        if fasta not in _INDEXES:
            _INDEXES[fasta] = Index.from_fasta(fasta, ctx=emu_ctx, compact=True)
        return _INDEXES[fasta]
    yield get
    for idx in _INDEXES.values():
        idx.close()
    _INDEXES.clear()


# ---- kernel edge cases -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symbols,letters", [(n, l) for n, l, _ in oc.record_cases()])
def test_records_at_the_block_edges(emu_ctx, symbols, letters):
    fasta = [f for n, l, f in oc.record_cases() if (n, l) == (symbols, letters)][0]
    N, sigma = oc.check_record(emu_ctx, Index, fasta, api)
    assert N == symbols + 1 and sigma == min(symbols, letters) + 1


def test_build_dev_and_expand_dev_on_a_raw_bwt(emu_ctx):
    """sx_occ_compact_build_dev / _expand_dev on their own: a BWT that is no text's (every symbol count is fine for them),
    several tiles of 64 blocks, expanded against numpy's running counts; misaligned blocks and rows out of range: SX_E_ARG"""
    rng = np.random.default_rng(4)
    for N, sigma in ((3 * 4096 + 77, 5), (4096, 2), (4097, 21), (130, 128)):
        bwt = rng.integers(0, sigma, N).astype(np.uint8)
        want = np.zeros((N + 1, sigma), np.uint32)
        want[1:] = np.cumsum(bwt[:, None] == np.arange(sigma)[None, :], axis=0)
        nbytes = emu_ctx.occ_compact_bytes(N, sigma)
        raw = np.zeros(nbytes + 512, np.uint8)
        at = (-raw.ctypes.data) % 256  # (as a device allocation starts)
        blocks = raw[at:at + nbytes]
        emu_ctx.occ_compact_build_dev(bwt, N, sigma, blocks)
        assert (blocks.reshape(-1, oc.stride(sigma)) == oc.reference_blocks(want, N, sigma)).all(), (N, sigma)
        assert not raw[:at].any() and not raw[at + nbytes:].any()
        rows = np.zeros((N + 1, sigma), np.uint32)
        emu_ctx.occ_compact_expand_dev(blocks, N, sigma, 0, N + 1, rows)
        assert (rows == want).all(), (N, sigma)
        one = np.zeros((1, sigma), np.uint32)
        emu_ctx.occ_compact_expand_dev(blocks, N, sigma, 65, 66, one)
        assert (one == want[65:66]).all()
        with pytest.raises(api.StralgAmdError, match=str(_lib.SX_E_ARG)):
            emu_ctx.occ_compact_expand_dev(raw[at + 8:], N, sigma, 0, 1, one)
        with pytest.raises(api.StralgAmdError, match=str(_lib.SX_E_ARG)):
            emu_ctx.occ_compact_expand_dev(blocks, N, sigma, 0, N + 2, rows)
    assert emu_ctx.occ_compact_bytes(0, 5) == 0 and emu_ctx.occ_compact_bytes(10, 129) == 0


# ---- search ----------------------------------------------------------------------------------------------------------
_APPROX = approx_cases()


@pytest.mark.parametrize("name", sorted(_APPROX))
def test_searches_over_blocks_equal_the_full_tables(emu_ctx, name):
    cs = _APPROX[name]
    sym, sigma = remapped(cs["raw"])
    oc.check_searches(emu_ctx, MEM, Index, cs, approx_model.tables(sym, sigma) + (sigma,), _lib.APPROX_HIT_DTYPE, api)


# ---- index, end to end -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_compact_from_fasta_maps_the_fixture_cases(emu_ctx, cases, compact_of, name):
    c = cases[name]
    idx = compact_of(c["fasta"])
    assert idx.compact
    check_case(c, idx.map_reads(c["fastq"], c["k"]))


@pytest.mark.parametrize("name", NAMES)
def test_compact_from_tables_maps_the_fixture_cases(emu_ctx, cases, name):
    c = cases[name]
    with Index.from_tables(oracle_records(emu_ctx, c["fasta"]), ctx=emu_ctx, compact=True) as idx:
        assert idx.compact and all(idx.record_occ(r).compact for r in range(len(idx.records)))
        check_case(c, idx.map_reads(c["fastq"], c["k"]))


def test_small_batches_and_windows_through_a_compact_index(emu_ctx, cases, compact_of):
    c = cases["two-records/k1"]
    emu_ctx.set_sam_batch_reads(7)
    emu_ctx.set_sam_window_bytes(4096)
    try:
        check_case(c, compact_of(c["fasta"]).map_reads(c["fastq"], c["k"]))
    finally:
        emu_ctx.set_sam_batch_reads(0)
        emu_ctx.set_sam_window_bytes(0)


# ---- saving and loading ----------------------------------------------------------------------------------------------
def written(idx):
    chunks = []
    idx.write(chunks.append)
    return b"".join(chunks), max(len(x) for x in chunks)


def test_save_of_a_compact_index_equals_the_reference_writer(emu_ctx):
    for name, c in serial_cases().items():
        fasta = b">" + name.encode() + b"\n" + c["raw"] + b"\n"
        head = struct.pack("<I", 1) + struct.pack("<I", len(name) + 1) + name.encode() + b"\0"
        for rev, want in ((True, c["with_reverse"]), (False, c["forward_only"])):
            with Index.from_fasta(fasta, include_reverse=rev, ctx=emu_ctx, compact=True) as idx:
                stream, longest = written(idx)
                assert stream == head + want, (name, rev)  # (what a full index writes: test_index_cpu)
                assert longest <= 4096  # (the harness's staging chunk: the tables left in many windows)
                assert [r[3] for r in idx.records] == [rev]
                if not rev:
                    with pytest.raises(api.StralgAmdError):
                        idx.expand_o(0, reverse=True)


def test_load_compact_maps_and_saves_the_same(emu_ctx, cases, compact_of, tmp_path):
    c = cases["two-records/k1"]
    with Index.from_fasta(c["fasta"], ctx=emu_ctx) as full:
        image = written(full)[0]
    assert written(compact_of(c["fasta"]))[0] == image
    path = tmp_path / "two.fa.bwttables"
    path.write_bytes(image)
    with Index.load(image, ctx=emu_ctx, compact=True) as loaded, Index.load(str(path), ctx=emu_ctx, compact=True) as from_file:
        assert loaded.compact and from_file.compact and loaded.records == compact_of(c["fasta"]).records
        for r in range(len(loaded.records)):
            for rev in (False, True):
                assert (loaded.device_occ(r, reverse=rev) == compact_of(c["fasta"]).device_occ(r, reverse=rev)).all()
        check_case(c, loaded.map_reads(c["fastq"], c["k"]))
        check_case(c, from_file.map_reads(c["fastq"], c["k"]))
        assert written(loaded)[0] == image
    with Index.load(image, ctx=emu_ctx) as plain:
        assert not plain.compact
    with pytest.raises(api.StralgAmdError):
        Index.load(image[:-5], ctx=emu_ctx, compact=True)


# ---- memory ----------------------------------------------------------------------------------------------------------
def test_device_bytes_of_a_compact_index(emu_ctx, cases, compact_of):
    for name in ("test-out/k0", "two-records/k1"):
        idx = compact_of(cases[name]["fasta"])
        least, most = oc.memory_bounds(idx.records)
        assert least <= idx.device_bytes <= most, name
    # the hg38 fixture genome: below a quarter of the least a full index of it takes (test_index_cpu: N (5 + 8 sigma) a
    # record is a lower bound of a full index's device_bytes; the GPU test builds both)
    c = cases["hg38/reads-100-10-0/k0"]
    assert c["fasta"] == genome_cases()["hg38-10000.fa"]["file"]
    comp = compact_of(c["fasta"])
    least, most = oc.memory_bounds(comp.records)
    assert least <= comp.device_bytes <= most
    assert comp.device_bytes < sum(N * (5 + 8 * sigma) for _, N, sigma, _ in comp.records) / 4


# ---- failure paths ---------------------------------------------------------------------------------------------------
def test_failed_compact_builds_leave_nothing(emu_ctx):
    lib = emu_ctx.lib
    start = lib.sx_index_live_count()
    with pytest.raises(api.StralgAmdError) as e:
        Index.from_fasta(b">cut off", ctx=emu_ctx, compact=True)
    assert "code -4" in str(e.value)
    with pytest.raises(api.StralgAmdError) as e:
        Index.from_fasta(b">one\nACGT\n>cut off inside the header", ctx=emu_ctx, compact=True)
    assert "code -4" in str(e.value)
    assert lib.sx_index_live_count() == start
    h = api.C.c_void_p()
    assert lib.sx_index_build_fasta_ex(emu_ctx.h, None, 0, 1, 2, api.C.byref(h)) == _lib.SX_E_ARG and not h  # (unknown flags)
    with Index.from_tables([], ctx=emu_ctx, compact=True) as empty:
        assert empty.compact and empty.records == [] and empty.map_reads(b"@r\nA\n+\nI\n", 0) == b""
    assert lib.sx_index_live_count() == start


def test_the_record_without_symbols_in_a_compact_index(emu_ctx, tmp_path):
    fasta = b">empty\n>full\nACGT\n"
    with Index.from_fasta(fasta, ctx=emu_ctx, compact=True) as idx, Index.from_fasta(fasta, ctx=emu_ctx) as full:
        assert idx.records == [(b"empty", 1, 1, True), (b"full", 5, 5, True)]
        assert (idx.expand_o(0) == full.device_tables(0)["o"]).all() and idx.expand_o(0).shape == (2, 1)
        assert written(idx)[0] == written(full)[0]
        with pytest.raises(api.StralgAmdError) as e:
            idx.map_reads(b"@r\nAC\n+\nII\n", 0)
        assert "code -1" in str(e.value)


def test_a_compact_index_refuses_a_context_on_another_device(emu_ctx, cases, compact_of):
    if emu_ctx.lib.sx_device_count() < 2:
        pytest.skip("the harness has one device: a context on another one cannot be made")
    other = api.Context(1, lib_path=emu_ctx.lib._name)
    try:
        idx = compact_of(cases["test-out/k0"]["fasta"])
        for call in (lambda: idx.map_reads(b"@r\nA\n+\nI\n", 0, ctx=other), lambda: idx.write(lambda chunk: None, ctx=other),
                     lambda: idx.expand_o(0, ctx=other)):
            with pytest.raises(api.StralgAmdError) as e:
                call()
            assert "code -1" in str(e.value)
    finally:
        other.close()
