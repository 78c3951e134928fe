"""The three forms of an index record (full tables, compact blocks, compact blocks with a sampled suffix array) through both
ways to a record: a build from FASTA, and host tables that come up one record at a time (what Index.load does).  Shared
by the CPU-harness suite (tests/test_index_cpu.py) and the GPU suite (tests/test_gpu_index.py)."""

FORMS = {"full": dict(), "compact": dict(compact=True), "sampled": dict(compact=True, sa_sample=4)}
# the smallest fixture genome with more than one record (42 bytes, three records: every allocation is its 256-byte
# rounding and tail), and the two-record genome of 70 KB, whose arrays are larger than the rounding
CASES = ["test-out/k1", "two-records/k1"]


def check_built_and_loaded_agree(ctx, Index, case, form):
    """an index built from FASTA and the one loaded from its saved bytes, in the same form: the same bytes on the device,
    the same SAM text of the fixture's reads (the reference's), and the same file saved again"""
    from sam_cases import check_case
    assert case["fasta"].count(b">") > 1
    with Index.from_fasta(case["fasta"], ctx=ctx, **FORMS[form]) as built:
        chunks = []
        built.write(chunks.append)
        saved = b"".join(chunks)
        with Index.load(saved, ctx=ctx, **FORMS[form]) as loaded:
            assert len(built.records) > 1 and loaded.records == built.records
            assert built.device_bytes == loaded.device_bytes
            sam = built.map_reads(case["fastq"], case["k"])
            check_case(case, sam)
            assert loaded.map_reads(case["fastq"], case["k"]) == sam
            again = []
            loaded.write(again.append)
            assert b"".join(again) == saved
