"""The SAM text of search hits (sx_sam.hip) and the mapper's loop (sx_map_reads_stream) through the CPU execution
harness, against the reference read mapper's stdout in tests/golden/golden_sam.npz.

The harness builds the kernels with a slice of 256 bytes a workgroup (SX_SAM_SLICE_BYTES in the Makefile's EMUGRIDS), so
lines straddle slices in every case here; windows are set per test (SX_FLAG_SAM_WINDOW_BYTES).

The 24 MB case (reads-100-10-0.fq, 2 edits) is not run whole here: its first reads are, and their lines are compared with
the fixture's first 200 lines.  tests/test_gpu_sam.py checks that case by its SHA-256."""
import pytest

import approx_model
import sam_kernel_cases as skc
from approx_cases import remapped
from device_memory import HarnessMemory
from sam_cases import check_case, sam_cases, subset_fastq
from stralg_amd import api


@pytest.fixture(scope="module")
def cases():
    return sam_cases()


_TABLES = {}


def records_of(ctx, fasta):
    """[(name, BwtTable)] in the mapper's list order (the file's), tables from the oracle's restatement"""
    if fasta not in _TABLES:
        recs = []
        for name, seq in ctx.fasta_records(fasta):
            sym, sigma = remapped(seq)
            sa, c, o, ro = approx_model.tables(sym, sigma)
            t = api.BwtTable(api.alloc_remap_table(seq), api.SuffixArray(None, sa), c, o, ro)
            recs.append((name, t))
        _TABLES[fasta] = recs
    return _TABLES[fasta]


def run(ctx, fasta, fastq, k, window=0, batch=0):
    chunks = []
    ctx.set_sam_window_bytes(window)
    ctx.set_sam_batch_reads(batch)
    try:
        ctx.map_reads_stream(records_of(ctx, fasta), fastq, k, chunks.append)
    finally:
        ctx.set_sam_window_bytes(0)
        ctx.set_sam_batch_reads(0)
    return chunks


@pytest.mark.parametrize("name", ["test-out/k0", "test-out/k1", "test-out/k2", "hg38/reads-100-10-0/k0",
                                  "hg38/reads-100-10-0/k1", "hg38/reads-1000-100-2/k2", "hg38/reads-1000-200-1/k1",
                                  "two-records/k1"])
def test_fixture_cases_whole_text(emu_ctx, cases, name):
    c = cases[name]
    check_case(c, b"".join(run(emu_ctx, c["fasta"], c["fastq"], c["k"])))


def test_skewed_case_first_lines(emu_ctx, cases):
    c = cases["hg38/reads-100-10-0/k2"]
    got = b"".join(run(emu_ctx, c["fasta"], subset_fastq(c["fastq"], range(3)), c["k"]))
    lines = got.split(b"\n")[:-1]
    assert len(lines) >= 200
    assert got.startswith(c["head"])


@pytest.mark.parametrize("window", [16, 4096])
def test_windows_concatenate(emu_ctx, cases, window):
    for name in ("test-out/k1", "two-records/k1") + (("hg38/reads-100-10-0/k0",) if window > 16 else ()):
        c = cases[name]
        chunks = run(emu_ctx, c["fasta"], c["fastq"], c["k"], window=window)
        assert max(len(x) for x in chunks) <= window and len(chunks) >= len(c["sam"]) // window
        check_case(c, b"".join(chunks))


def test_small_read_batches(emu_ctx, cases):
    for name, batch in (("two-records/k1", 7), ("test-out/k2", 1), ("hg38/reads-100-10-0/k0", 33)):
        c = cases[name]
        check_case(c, b"".join(run(emu_ctx, c["fasta"], c["fastq"], c["k"], batch=batch, window=4096)))


# ---- sx_sam_layout_dev / sx_sam_emit_dev on made-up hits (tests/sam_kernel_cases.py; the GPU runs the same cases) -------------
MEM = HarnessMemory()


def test_cigar_on_the_device(emu_ctx):
    skc.check_cigars(emu_ctx, MEM, skc.cigar_case())


def test_position_digits(emu_ctx):
    skc.check_position_digits(emu_ctx, MEM, skc.digit_case())


@pytest.mark.parametrize("window", skc.WINDOWS)
def test_emit_window_sizes(emu_ctx, window):
    skc.check_window(emu_ctx, MEM, skc.digit_case(), window)


def test_layout_rejects_hits_outside_the_batch(emu_ctx):
    for case in skc.refused_cases():
        skc.check_refused(emu_ctx, MEM, case)


def test_empty_batch(emu_ctx):
    skc.check_empty(emu_ctx, MEM, skc.empty_case())


@pytest.fixture(scope="module")
def text_cases():
    return skc.text_cases()


@pytest.mark.parametrize("name", skc.TEXT_CASE_NAMES)
def test_layout_and_emit_at_the_kernels_thresholds(emu_ctx, text_cases, name):
    case = text_cases[name]
    assert not case.get("gpu_only")
    skc.check_text(emu_ctx, MEM, case)


def test_text_case_names_are_the_modules(text_cases):
    assert list(text_cases) == skc.TEXT_CASE_NAMES


# ---- sx_fastq_index --------------------------------------------------------------------------------------------------
def test_fastq_index_in_contract(emu_ctx):
    data = b"@r0 desc x\nCC\n+\n~~\n@r1\nAAA\n+r1 again\nIII\n@@\n@\n+\n+\n@last\tname\nNN\n\n##"
    names, no, seqs, so, quals, qo = emu_ctx.fastq_index(data)
    split = lambda d, o: [d[o[i]:o[i + 1]].tobytes() for i in range(o.size - 1)]
    assert split(names, no) == [b"r0 desc x", b"r1", b"@", b"last\tname"]
    assert split(seqs, so) == [b"CC", b"AAA", b"@", b"NN"]
    assert split(quals, qo) == [b"~~", b"III", b"+", b"##"]
    assert emu_ctx.fastq_index(data + b"\n")[0].tobytes() == names.tobytes()
    assert emu_ctx.fastq_index(b"")[1].tolist() == [0]
    longest = b"@" + b"n" * 2045 + b"\n" + b"A" * 2046 + b"\n+\n" + b"I" * 2046
    assert emu_ctx.fastq_index(longest)[3].tolist() == [0, 2046]


@pytest.mark.parametrize("data", [
    b"@" + b"n" * 2046 + b"\nA\n+\nI\n",          # a line of 2047 bytes
    b"@r\n" + b"A" * 2047 + b"\n+\n" + b"I" * 2047 + b"\n",
    b"@\nA\n+\nI\n",                               # an empty name
    b"@r\n\n+\nI\n",                               # an empty sequence
    b"@r\nA\n+\n\n",                               # an empty quality line
    b"@r\nA\n+\n",                                 # cut off before the fourth line
    b"@r\nA\n+",
    b"@r\nA\n",
    b"@r\n",
    b"@r\nA\n+\nI\n\n",                            # a blank line behind the records
    b"\n@r\nA\n+\nI\n",
    b"@r\nA\0\n+\nI\n",                            # a NUL inside a record
])
def test_fastq_index_out_of_contract(emu_ctx, data):
    with pytest.raises(api.StralgAmdError) as e:
        emu_ctx.fastq_index(data)
    assert "code -4" in str(e.value)
    with pytest.raises(api.StralgAmdError) as e:
        emu_ctx.map_reads_stream([], data, 1, lambda chunk: None)
    assert "code -4" in str(e.value)


def test_map_reads_limits(emu_ctx, cases):
    c = cases["test-out/k0"]
    for k in (-1, 9):
        with pytest.raises(api.StralgAmdError) as e:
            run(emu_ctx, c["fasta"], c["fastq"], k)
        assert "code -1" in str(e.value)
    assert run(emu_ctx, c["fasta"], b"", 1) == []

    def refuse(chunk):
        raise KeyError("sink")

    with pytest.raises(KeyError):
        emu_ctx.map_reads_stream(records_of(emu_ctx, c["fasta"]), c["fastq"], 0, refuse)
