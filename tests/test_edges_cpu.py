"""Edge-case genomes (tests/edge_cases.py) through the CPU execution harness: 69 records, records
around the 64-row blocks and shorter than the sampling distance, reads at the FASTQ limit and k up to 8, through every flag
set, the index forms, the loop's switches and the pair join.  The same cases at the same shapes run on the GPU
(tests/test_gpu_edges.py); the harness lays a slice of 256 bytes out in a workgroup where the device has 16 KiB.  The tool runs
on the GPU only."""
import pytest

import best_cases as bc
import edge_cases as ec
from conftest import EMU_LIB
from stralg_amd import api
from test_sam_cpu import records_of


@pytest.fixture(scope="module")
def cases():
    return ec.edge_cases()


@pytest.fixture(scope="module")
def indexes(emu_ctx):
    """(fasta, form) -> a resident index, built once"""
    made = {}

    def get(fasta, **form):
        key = (fasta, tuple(sorted(form.items())))
        if key not in made:
            made[key] = api.Index.from_fasta(fasta, ctx=emu_ctx, **form)
        return made[key]

    yield get
    for idx in made.values():
        idx.close()


# ---- the oracle -------------------------------------------------------------------------------------------------------------
def test_oracle_counts(cases):
    ec.check_table(cases)
    ec.check_pairs_table(cases)


def test_recordings_cover_the_edges(cases):
    ec.coverage(cases)


# ---- every case, every k, every flag set --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", ec.KS, ids=ec.KS_IDS)
def test_flag_sets(emu_ctx, indexes, cases, name, k):
    c = cases[name]

    def stream(case, k, **flags):
        chunks = []
        emu_ctx.map_reads_stream(records_of(emu_ctx, case["fasta"]), case["fastq"], k, chunks.append, **flags)
        return b"".join(chunks)

    ec.check_flag_sets(emu_ctx, indexes(c["fasta"]), stream, c, name, k)


def test_module_level_map_reads(emu_ctx, cases):
    """stralg_amd.map_reads itself (it builds the tables of every record through the context) on the two small genomes"""
    for name in ("block-edges", "deep-k"):
        c, K = cases[name], ec.CASES[name]
        for f in ec.STREAMED:
            bc.check_text(api.map_reads(c["fasta"], c["fastq"], K, ctx=emu_ctx, **ec.call_flags(**ec.FLAG_SETS[f])), ec.want(c, K, **ec.FLAG_SETS[f]))


# ---- the index forms ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(ec.FORMS))
@pytest.mark.parametrize("name", ["block-edges", "deep-k"])
def test_index_forms(emu_ctx, indexes, cases, name, form):
    ec.check_form(indexes(cases[name]["fasta"], **ec.FORMS[form]), cases[name], name)


@pytest.mark.parametrize("form", ec.MANY_FORMS)
def test_index_forms_of_many_records(emu_ctx, indexes, cases, form):
    ec.check_form(indexes(cases["many-records"]["fasta"], **ec.FORMS[form]), cases["many-records"], "many-records")


def test_many_records_cannot_be_packed(emu_ctx, cases):
    ec.check_packed_refused(emu_ctx, api.Index, cases["many-records"])


# ---- the loop's switches ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 3, 33])
def test_batches(emu_ctx, indexes, cases, batch):
    c = cases["many-records"]
    ec.check_batches(emu_ctx, indexes(c["fasta"]), c, batch)


def test_sixteen_byte_windows(emu_ctx, indexes, cases):
    c = cases["many-records"]
    ec.check_sixteen_byte_windows(emu_ctx, indexes(c["fasta"]), c)


def test_room_of_one_hit(emu_ctx, indexes, cases):
    c = cases["many-records"]
    ec.check_room_of_one_hit(emu_ctx, indexes(c["fasta"]), c)


def test_sampled_index_located_in_runs_of_five(emu_ctx, indexes, cases):
    c = cases["many-records"]
    ec.check_located_in_runs_of_five(emu_ctx, indexes(c["fasta"], **ec.FORMS["sampled-1024"]), c)


@pytest.mark.parametrize("window", [16, 4099])
def test_reads_of_2046_symbols_with_tags(emu_ctx, indexes, cases, window):
    c = cases["block-edges"]
    ec.check_longest_reads(emu_ctx, indexes(c["fasta"]), c, window)


# ---- pairs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,batch", [(k, b) for k in ec.PAIRS for b in ((0, 3) if k[1] == 2 else (0,))],
                         ids=lambda v: "%s-k%d" % v[:2] if isinstance(v, tuple) else "batch%d" % v)
def test_pairs(emu_ctx, indexes, cases, key, batch):
    c = cases[key[0]]
    ec.check_pairs(emu_ctx, indexes(c["fasta"]), c, key, batch)


# ---- the same bytes from run to run ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ec.CASES))
def test_second_call_and_fresh_context(emu_ctx, indexes, cases, name):
    fresh = api.Context(0, lib_path=EMU_LIB)
    try:
        fresh.set_small_direct_max(0)
        ec.check_same_bytes(indexes(cases[name]["fasta"]), fresh, api.Index, cases[name], name)
    finally:
        fresh.close()
