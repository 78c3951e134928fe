"""The device-resident index (sx_index.hip: stralg_amd.Index) and the FASTQ ingest on the device (sx_fastq.hip: sx_fastq_index_dev)
through the CPU execution harness: the reference read mapper's stdout in tests/golden/golden_sam.npz, the reference
writer's byte streams in tests/golden/golden_fasta.npz, and, on every FASTQ image (tests/fastq_cases.py), the contract
restated in Python and the host's sx_fastq_index beside the device function."""
import struct

import numpy as np
import pytest

import approx_model
from approx_cases import remapped
import fastq_cases as fq
import index_form_cases as forms
from conftest import serial_cases
from device_memory import HarnessMemory
from sam_cases import check_case, sam_cases, subset_fastq
from stralg_amd import Index, api

NAMES = ["test-out/k0", "test-out/k1", "test-out/k2", "hg38/reads-100-10-0/k0", "hg38/reads-100-10-0/k1",
         "hg38/reads-1000-100-2/k2", "hg38/reads-1000-200-1/k1", "two-records/k1"]  # test_sam_cpu's whole-text cases


@pytest.fixture(scope="module")
def cases():
    return sam_cases()


_INDEXES = {}


@pytest.fixture(scope="module")
def index_of(emu_ctx):
    """fasta bytes -> Index.from_fasta of it (one build a genome for the whole module)"""
    def get(fasta):
        if fasta not in _INDEXES:
            _INDEXES[fasta] = Index.from_fasta(fasta, ctx=emu_ctx)
        return _INDEXES[fasta]
    yield get
    for idx in _INDEXES.values():
        idx.close()
    _INDEXES.clear()


def oracle_records(ctx, fasta):
    """[(name, BwtTable)] with tables from the oracle's restatement (as test_sam_cpu.records_of), the string included"""
    recs = []
    for name, seq in ctx.fasta_records(fasta):
        sym, sigma = remapped(seq)
        sa, c, o, ro = approx_model.tables(sym, sigma)
        string = np.concatenate([np.asarray(sym, np.uint8), np.zeros(1, np.uint8)])
        recs.append((name, api.BwtTable(api.alloc_remap_table(seq), api.SuffixArray(string, sa), c, o, ro)))
    return recs


# ---- mapping ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_from_fasta_maps_the_fixture_cases(emu_ctx, cases, index_of, name):
    c = cases[name]
    check_case(c, index_of(c["fasta"]).map_reads(c["fastq"], c["k"]))


@pytest.mark.parametrize("name", NAMES)
def test_from_tables_maps_the_fixture_cases(emu_ctx, cases, name):
    c = cases[name]
    with Index.from_tables(oracle_records(emu_ctx, c["fasta"]), ctx=emu_ctx) as idx:
        check_case(c, idx.map_reads(c["fastq"], c["k"]))


def test_device_tables_equal_the_oracle(emu_ctx, cases, index_of):
    for name in ("test-out/k0", "two-records/k1"):
        fasta = cases[name]["fasta"]
        idx = index_of(fasta)
        want = oracle_records(emu_ctx, fasta)
        assert [r[0] for r in idx.records] == [n for n, _ in want]
        total = 0
        for r, (_, t) in enumerate(want):
            got = idx.device_tables(r)
            N, sigma = idx.records[r][1:3]
            assert (N, sigma) == (t.sa.array.size, t.remap_table.alphabet_size) and idx.records[r][3]
            assert (got["string"] == t.sa.string).all() and (got["sa"] == t.sa.array).all() and (got["c"] == t.c_table).all()
            assert (got["o"] == t.o_table).all() and (got["ro"] == t.ro_table).all()
            total += N * (5 + 8 * sigma)
        assert total <= idx.device_bytes <= total + 4096 * (5 * len(want) + 5)  # (allocations are rounded up to 256 + 256)


@pytest.mark.parametrize("form", list(forms.FORMS))
@pytest.mark.parametrize("name", forms.CASES)
def test_built_and_loaded_agree_in_every_form(emu_ctx, cases, name, form):
    forms.check_built_and_loaded_agree(emu_ctx, Index, cases[name], form)


def test_one_index_several_read_sets(emu_ctx, cases, index_of):
    """three different FASTQ images one after the other, then the first again; between two of the calls an unrelated
    build and a trim on the same context"""
    a, b, c = cases["test-out/k0"], cases["test-out/k1"], cases["test-out/k2"]
    assert a["fasta"] == b["fasta"] == c["fasta"]
    idx = index_of(a["fasta"])
    sets = [(a["fastq"], a["k"], a), (subset_fastq(b["fastq"], range(2)), 1, None), (c["fastq"], c["k"], c)]
    first = idx.map_reads(*sets[0][:2])
    check_case(a, first)
    second = idx.map_reads(*sets[1][:2])
    assert second and b["sam"].startswith(second)
    x = np.random.default_rng(5).integers(1, 5, 5000).astype(np.uint8)
    assert emu_ctx.sa_build(x, 5)[0] == 5000
    emu_ctx.trim()
    check_case(c, idx.map_reads(*sets[2][:2]))
    check_case(b, idx.map_reads(b["fastq"], b["k"]))
    assert idx.map_reads(*sets[0][:2]) == first


@pytest.mark.parametrize("window", [16, 4096])
def test_windows_through_the_index(emu_ctx, cases, index_of, window):
    for name in ("test-out/k1", "two-records/k1") + (("hg38/reads-100-10-0/k0",) if window > 16 else ()):
        c = cases[name]
        chunks = []
        emu_ctx.set_sam_window_bytes(window)
        try:
            index_of(c["fasta"]).map_reads(c["fastq"], c["k"], sink=chunks.append)
        finally:
            emu_ctx.set_sam_window_bytes(0)
        assert max(len(x) for x in chunks) <= window and len(chunks) >= len(c["sam"]) // window
        check_case(c, b"".join(chunks))


def test_small_read_batches_through_the_index(emu_ctx, cases, index_of):
    for name, batch in (("two-records/k1", 7), ("test-out/k2", 1), ("hg38/reads-100-10-0/k0", 33)):
        c = cases[name]
        emu_ctx.set_sam_batch_reads(batch)
        emu_ctx.set_sam_window_bytes(4096)
        try:
            check_case(c, index_of(c["fasta"]).map_reads(c["fastq"], c["k"]))
        finally:
            emu_ctx.set_sam_batch_reads(0)
            emu_ctx.set_sam_window_bytes(0)


def test_limits_and_errors_are_those_of_the_stream_call(emu_ctx, cases, index_of):
    c = cases["test-out/k0"]
    idx = index_of(c["fasta"])
    for k in (-1, 9):
        with pytest.raises(api.StralgAmdError) as e:
            idx.map_reads(c["fastq"], k)
        assert "code -1" in str(e.value)
    assert idx.map_reads(b"", 1) == b""
    with pytest.raises(api.StralgAmdError) as e:
        idx.map_reads(b"@r\nA\n+\n", 1)
    assert "code -4" in str(e.value)

    def refuse(chunk):
        raise KeyError("sink")

    with pytest.raises(KeyError):
        idx.map_reads(c["fastq"], 0, sink=refuse)
    check_case(c, idx.map_reads(c["fastq"], c["k"]))  # (and it still works)


# ---- sx_fastq_index_dev against the contract's restatement and the host's sx_fastq_index (tests/fastq_cases.py; the GPU
# runs the same images) ------------------------------------------------------------------------------------------------
MEM = HarnessMemory()


def test_fastq_reference_reproduces_the_golden_sam_text(cases):
    """every line of the reference mapper's SAM text shows a read's name, sequence and quality: fastq_reference gives
    exactly those for the golden FASTQ images, reads in the text's order (the 24 MB case: its first 200 lines)"""
    checked = 0
    for name, c in cases.items():
        ref = fq.fastq_reference(c["fastq"])
        assert ref is not None, name
        names, seqs, quals, no, so, qo = ref
        reads = [(names[no[i]:no[i + 1]], seqs[so[i]:so[i + 1]], quals[qo[i]:qo[i + 1]]) for i in range(len(no) - 1)]
        at = 0
        for line in (c["sam"] if "sam" in c else c["head"]).split(b"\n")[:-1]:
            f = line.split(b"\t")
            while reads[at][0] != f[0]:  # (reads without a line are passed over; the order is the file's)
                at += 1
            assert (f[0], f[9], f[10]) == reads[at], (name, f[0])
            checked += 1
    assert checked > 1000


def test_fastq_dev_on_the_fixture_images(emu_ctx, cases):
    images = fq.fixture_images(cases)
    for case in images:
        fq.check_image(emu_ctx, MEM, case)
    assert len(images) >= 2 * 4


def test_fastq_dev_in_contract(emu_ctx):
    for case in fq.in_contract_images():
        fq.check_image(emu_ctx, MEM, case)
    fq.check_in_contract_fields(emu_ctx, MEM)


@pytest.mark.parametrize("data", fq.OUT_OF_CONTRACT)
def test_fastq_dev_out_of_contract(emu_ctx, data, cases, index_of):
    assert fq.agree(emu_ctx, MEM, data, expect=False) == "-4"
    with pytest.raises(api.StralgAmdError) as e:
        index_of(cases["test-out/k0"]["fasta"]).map_reads(data, 1)
    assert "code -4" in str(e.value)


def test_fastq_dev_generated_images(emu_ctx):
    for case in fq.generated_images():
        fq.check_image(emu_ctx, MEM, case)


def test_fastq_dev_soups_with_one_defect(emu_ctx):
    fq.check_defects(emu_ctx, MEM, fq.soups())


@pytest.mark.parametrize("family", ["line_role_edge_images", "long_line_images", "dense_tile_images",
                                    "shifted_tile_multiple_images"])
def test_fastq_dev_at_the_tiles_edges(emu_ctx, family):
    for case in getattr(fq, family)():
        fq.check_image(emu_ctx, MEM, case)


def test_fastq_dev_defects_at_the_tiles_edges(emu_ctx):
    fq.check_defects(emu_ctx, MEM, fq.defects_at_tile_edges())


def test_fastq_dev_twice_the_same_bytes(emu_ctx):
    for case in fq.determinism_images():
        fq.check_deterministic(emu_ctx, MEM, case)


# ---- saving and loading -----------------------------------------------------------------------------------------------
def test_save_equals_the_reference_writer(emu_ctx, tmp_path):
    for name, c in serial_cases().items():
        fasta = b">" + name.encode() + b"\n" + c["raw"] + b"\n"
        assert emu_ctx.fasta_records(fasta) == [(name.encode(), c["raw"])], name  # (the raw string survives FASTA packing)
        head = struct.pack("<I", 1) + struct.pack("<I", len(name) + 1) + name.encode() + b"\0"
        for rev, want in ((True, c["with_reverse"]), (False, c["forward_only"])):
            with Index.from_fasta(fasta, include_reverse=rev, ctx=emu_ctx) as idx:
                path = tmp_path / f"{name}-{int(rev)}"
                idx.save(path)
                assert path.read_bytes() == head + want, (name, rev)
                assert [r[3] for r in idx.records] == [rev]


def test_load_of_the_reference_writers_streams(emu_ctx, tmp_path):
    """an index file put together from the reference writer's own byte streams, as
    test_gpu_sam.test_tool_reads_tables_of_the_reference_writer builds it: it maps like Index.from_fasta"""
    sc = serial_cases()
    recs = [(b"fasta0", sc["ref-fasta0"]), (b"periodic", sc["struct-periodic"])]  # FASTA order
    fasta = b"".join(b">" + n + b"\n" + c["raw"] + b"\n" for n, c in recs)
    image = struct.pack("<I", len(recs))
    for n, c in reversed(recs):
        image += struct.pack("<I", len(n) + 1) + n + b"\0" + c["with_reverse"]
    reads = []
    for n, c in recs:
        raw = c["raw"]
        for at in range(0, len(raw) - 12, max(1, len(raw) // 40)):
            reads.append(raw[at:at + 12])
    reads += [b"ACGTACGTAC", b"abcd", b"zz"]
    fastq = b"".join(b"@q%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads))
    path = tmp_path / "two.fa.bwttables"
    path.write_bytes(image)
    with Index.from_fasta(fasta, ctx=emu_ctx) as built, Index.load(image, ctx=emu_ctx) as loaded, \
            Index.load(str(path), ctx=emu_ctx) as from_file:
        assert loaded.records == built.records == from_file.records
        assert [r[0] for r in loaded.records] == [b"fasta0", b"periodic"]
        for k in (0, 1):
            want = built.map_reads(fastq, k)
            assert want.count(b"\n") > 80
            assert loaded.map_reads(fastq, k) == want and from_file.map_reads(fastq, k) == want
        out = tmp_path / "again"
        loaded.save(out)
        assert out.read_bytes() == image
        built.save(out)
        assert out.read_bytes() == image
    with pytest.raises(api.StralgAmdError):
        Index.load(image[:-5], ctx=emu_ctx)


def test_an_index_without_strings_cannot_be_saved(emu_ctx, cases, tmp_path):
    c = cases["test-out/k0"]
    recs = oracle_records(emu_ctx, c["fasta"])
    for _, t in recs:
        t.sa.string = None
    with Index.from_tables(recs, ctx=emu_ctx) as idx:
        with pytest.raises(api.StralgAmdError) as e:
            idx.save(tmp_path / "x")
        assert "code -1" in str(e.value)
        check_case(c, idx.map_reads(c["fastq"], c["k"]))


def test_empty_sequence_record(emu_ctx, tmp_path):
    """a record without symbols is what build_complete_table makes of an empty string (N = 1, sigma = 1): it builds and
    saves; mapping answers SX_E_ARG as sx_map_reads_stream does for such a table"""
    fasta = b">empty\n>full\nACGT\n"
    assert emu_ctx.fasta_records(fasta) == [(b"empty", b""), (b"full", b"ACGT")]
    with Index.from_fasta(fasta, ctx=emu_ctx) as idx:
        assert idx.records == [(b"empty", 1, 1, True), (b"full", 5, 5, True)]
        assert idx.device_tables(0)["sa"].tolist() == [0]
        idx.save(tmp_path / "e")
        with pytest.raises(api.StralgAmdError) as e:
            idx.map_reads(b"@r\nAC\n+\nII\n", 0)
        assert "code -1" in str(e.value)
    t = api.build_complete_table(b"", True, emu_ctx)
    with pytest.raises(api.StralgAmdError) as e:
        emu_ctx.map_reads_stream([(b"empty", t)], b"@r\nAC\n+\nII\n", 0, lambda chunk: None)
    assert "code -1" in str(e.value)


# ---- lifetime --------------------------------------------------------------------------------------------------------
def test_live_count_and_failed_builds(emu_ctx, cases):
    lib = emu_ctx.lib
    start = lib.sx_index_live_count()
    idx = Index.from_fasta(cases["test-out/k0"]["fasta"], ctx=emu_ctx)
    assert lib.sx_index_live_count() == start + 1
    idx.close()
    idx.close()
    assert lib.sx_index_live_count() == start
    with pytest.raises(api.StralgAmdError):
        idx.map_reads(b"", 0)
    with pytest.raises(api.StralgAmdError) as e:
        Index.from_fasta(b">one\nACGT\n>cut off inside the header", ctx=emu_ctx)
    assert "code -4" in str(e.value)
    too_many = b">wide\n" + bytes(range(0x40, 0x40 + 130)) + b"\n"
    with pytest.raises(api.StralgAmdError) as e:
        Index.from_fasta(too_many, ctx=emu_ctx)
    assert "code -1" in str(e.value)
    assert lib.sx_index_live_count() == start
    with pytest.raises(api.StralgAmdError) as e:  # (an empty image ends inside a header line: fasta.c:121-124)
        Index.from_fasta(b"", ctx=emu_ctx)
    assert "code -4" in str(e.value)
    with Index.from_tables([], ctx=emu_ctx) as empty:
        assert empty.records == [] and empty.map_reads(b"@r\nA\n+\nI\n", 0) == b""
    assert lib.sx_index_live_count() == start


def test_a_context_on_another_device_is_refused(emu_ctx, cases, index_of):
    if emu_ctx.lib.sx_device_count() < 2:
        pytest.skip("the harness has one device: a context on another one cannot be made")
    other = api.Context(1, lib_path=emu_ctx.lib._name)
    try:
        with pytest.raises(api.StralgAmdError) as e:
            index_of(cases["test-out/k0"]["fasta"]).map_reads(b"@r\nA\n+\nI\n", 0, ctx=other)
        assert "code -1" in str(e.value)
    finally:
        other.close()
