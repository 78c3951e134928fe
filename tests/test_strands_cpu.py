"""Both strands through the CPU execution harness (tests/strand_cases.py): sx_fastq_strands_dev against the contract's
rc() restated in Python, sx_sam_layout_dev_ex / sx_sam_emit_dev_ex over made-up hits, and the mapper's loop with
SX_MAP_BOTH_STRANDS against the text composed from the reference mapper's two recorded outputs
(tests/golden/golden_sam_strands.npz).

The harness builds the SAM kernels with a slice of 256 bytes a workgroup, so a FLAG is cut by slices here and, with
windows of 16 bytes, by windows.  The 45 MB case (reads-100-10-0.fq, 2 edits) is not run whole here: its first reads
are, against the fixture's first 200 lines; tests/test_gpu_strands.py checks that case by its SHA-256."""
import pytest

import strand_cases as sc
from device_memory import HarnessMemory
from sam_cases import check_case, sam_cases, subset_fastq
from stralg_amd import _lib, api
from test_sam_cpu import records_of

MEM = HarnessMemory()


@pytest.fixture(scope="module")
def cases():
    return sc.strand_cases()


@pytest.fixture(scope="module")
def images():
    return sc.strand_images()


def run(ctx, fasta, fastq, k, window=0, batch=0, both_strands=True):
    chunks = []
    ctx.set_sam_window_bytes(window)
    ctx.set_sam_batch_reads(batch)
    try:
        ctx.map_reads_stream(records_of(ctx, fasta), fastq, k, chunks.append, both_strands=both_strands)
    finally:
        ctx.set_sam_window_bytes(0)
        ctx.set_sam_batch_reads(0)
    return chunks


# ---- sx_fastq_strands_dev ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.STRAND_IMAGE_NAMES)
def test_strands_of_an_image(emu_ctx, images, name):
    sc.check_strand_image(emu_ctx, MEM, *images[name])


def test_image_names_are_the_modules(images):
    assert list(images) == sc.STRAND_IMAGE_NAMES


def test_strands_of_the_fixtures_reads(emu_ctx):
    for c in sam_cases().values():
        if c["k"] == 1:
            sc.check_strand_image(emu_ctx, MEM, c["fastq"], 0)


def test_rc_restated():
    """the helper's table against the contract's, spelled out"""
    pairs = "AT CG GC TA UA NN RY YR KM MK BV VB DH HD SS WW"
    for p in pairs.split():
        assert sc.rc((b"n", p[:1].encode(), b"!"))[1] == p[1:].encode()
        assert sc.rc((b"n", p[:1].lower().encode(), b"!"))[1] == p[1:].lower().encode()
    assert sc.rc((b"n a", b"AAC*-\x80g", b"123456\xff")) == (b"n a", b"c\x80-*GTT", b"\xff654321")


# ---- the FLAG of the SAM emitter --------------------------------------------------------------------------------------
def test_flags_on_neighbouring_reads(emu_ctx):
    sc.check_flags(emu_ctx, MEM, sc.flag_case())


def test_flags_cut_by_windows_of_16_bytes(emu_ctx):
    sc.check_flags(emu_ctx, MEM, sc.small_flag_case())


def test_flags_with_several_records(emu_ctx):
    sc.check_flags(emu_ctx, MEM, sc.several_records_flag_case())


def test_flags_must_be_aligned(emu_ctx):
    case = sc.flag_case()
    b = sc.FlagBatch(emu_ctx, MEM, case, case["flags"])
    b.batch.d_read_flags += 1
    with pytest.raises(api.StralgAmdError) as e:
        emu_ctx.sam_layout_dev(b.batch, b.d_off)
    assert "code -1" in str(e.value)


# ---- the loop ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.WHOLE_TEXT)
def test_fixture_cases_whole_text(emu_ctx, cases, name):
    c = cases[name]
    sc.check_strands(c, b"".join(run(emu_ctx, c["fasta"], c["fastq"], c["k"])))


def test_skewed_case_first_lines(emu_ctx, cases):
    c = cases[sc.BY_DIGEST]
    got = b"".join(run(emu_ctx, c["fasta"], subset_fastq(c["fastq"], range(3)), c["k"]))
    assert got.count(b"\n") >= 200
    assert got.startswith(c["head"])


@pytest.mark.parametrize("window", [16, 4096])
@pytest.mark.parametrize("batch", [1, 7, 33])
def test_batches_and_windows(emu_ctx, cases, batch, window):
    """odd batches part a read from its reverse complement; windows of 16 bytes cut a "16" """
    for name in ("test-out/k1", "two-records-flipped/k1"):
        c = cases[name]
        chunks = run(emu_ctx, c["fasta"], c["fastq"], c["k"], window=window, batch=batch)
        assert max(len(x) for x in chunks) <= window
        sc.check_strands(c, b"".join(chunks))


def test_sampled_index_both_strands(emu_ctx, cases):
    """the located form of the kernels takes the flags too: a compact index with a sampled suffix array, its hits located
    in runs of at most 64 rows"""
    c = cases["two-records-flipped/k1"]
    emu_ctx.set_locate_chunk_rows(64)
    try:
        with api.Index.from_fasta(c["fasta"], ctx=emu_ctx, compact=True, sa_sample=32) as idx:
            sc.check_strands(c, idx.map_reads(c["fastq"], c["k"], both_strands=True))
            assert idx.map_reads(c["fastq"], c["k"]) == c["forward"]
            assert sum(n for _, n in idx.map_reads_discard(c["fastq"], c["k"], both_strands=True)) == len(c["want"])
    finally:
        emu_ctx.set_locate_chunk_rows(0)


def test_one_strand_through_the_new_entry_points(emu_ctx):
    """flags == 0 through sx_map_reads_stream_ex and sx_index_map_reads_ex: the text of golden_sam.npz"""
    import ctypes as C
    import numpy as np
    base = sam_cases()
    for name in ("test-out/k1", "two-records/k1"):
        c = base[name]
        recs = (_lib.MapRecord * 8)()
        keep = []
        records = records_of(emu_ctx, c["fasta"])
        for r, (rname, t) in enumerate(records):
            recs[r] = api._map_record(rname, t, keep)
        chunks = []

        def sink(user, section, data, n):
            chunks.append(C.string_at(data, n))
            return 0

        cb = _lib.SINK_FN(sink)
        buf = np.frombuffer(c["fastq"], np.uint8)
        assert emu_ctx.lib.sx_map_reads_stream_ex(emu_ctx.h, recs, len(records), buf.ctypes.data, buf.size, c["k"], 0, cb, None) == 0
        check_case(c, b"".join(chunks))
        with api.Index.from_fasta(c["fasta"], ctx=emu_ctx) as idx:
            del chunks[:]
            assert emu_ctx.lib.sx_index_map_reads_ex(emu_ctx.h, idx._handle(), buf.ctypes.data, buf.size, c["k"], 0, cb, None) == 0
            check_case(c, b"".join(chunks))
            # unknown flag bits are refused by both
            assert emu_ctx.lib.sx_index_map_reads_ex(emu_ctx.h, idx._handle(), buf.ctypes.data, buf.size, c["k"], 2, cb, None) == _lib.SX_E_ARG
        assert emu_ctx.lib.sx_map_reads_stream_ex(emu_ctx.h, recs, len(records), buf.ctypes.data, buf.size, c["k"], 6, cb, None) == _lib.SX_E_ARG


def test_the_limit_counts_both_strands(emu_ctx):
    """2 x reads x records < 2^32 (sx_map_reads_limit holds the arithmetic that the loop asks)"""
    limit = emu_ctx.lib.sx_map_reads_limit
    both = _lib.SX_MAP_BOTH_STRANDS
    assert limit(2 ** 32 - 1, 1, 0) == 0 and limit(2 ** 32, 1, 0) == _lib.SX_E_ARG
    assert limit(2 ** 31 - 1, 1, both) == 0 and limit(2 ** 31, 1, both) == _lib.SX_E_ARG
    assert limit(2 ** 16, 2 ** 15 - 1, both) == 0 and limit(2 ** 16, 2 ** 15, both) == _lib.SX_E_ARG
    assert limit(2 ** 16, 2 ** 16 - 1, 0) == 0 and limit(2 ** 16, 2 ** 16, 0) == _lib.SX_E_ARG
    assert limit(3, 1431655765, 0) == 0 and limit(3, 1431655765, both) == _lib.SX_E_ARG
    assert limit(2 ** 63, 2, both) == _lib.SX_E_ARG and limit(2 ** 64 - 1, 2 ** 64 - 1, 0) == _lib.SX_E_ARG  # (no wrap-around)
    assert limit(0, 0, both) == 0 and limit(5, 5, 2) == _lib.SX_E_ARG


def test_limits_and_empty_sets(emu_ctx, cases):
    c = cases["test-out/k0"]
    for k in (-1, 9):
        with pytest.raises(api.StralgAmdError) as e:
            run(emu_ctx, c["fasta"], c["fastq"], k)
        assert "code -1" in str(e.value)
    assert run(emu_ctx, c["fasta"], b"", 1) == []
    # a read equal to its own reverse complement prints both groups
    got = b"".join(run(emu_ctx, c["fasta"], b"@pal\nAT\n+\nI#\n", 0))
    lines = got.split(b"\n")[:-1]
    fwd = [l for l in lines if l.split(b"\t")[1] == b"0"]
    rev = [l for l in lines if l.split(b"\t")[1] == b"16"]
    assert fwd and len(fwd) == len(rev) and lines == fwd + rev
    assert [sc.with_flag(l, b"0").replace(b"\tI#", b"\t#I") for l in rev] == [l.replace(b"\tI#", b"\t#I") for l in fwd]
