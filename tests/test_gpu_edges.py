"""Edge-case genomes on the GPU (tests/edge_cases.py): the cases of tests/test_edges_cpu.py at the same
shapes -- 69 records (the scans over reads x records slots cross waves and workgroups), records around the 64-row blocks and
shorter than the sampling distance, reads at the FASTQ limit, k up to 8 -- where the device lays a slice of 16 KiB out in a
workgroup and the harness 256 bytes; and the command-line tool on the 69 records.  It reads the recorded fixture alone."""
import os
import subprocess

import pytest

import best_cases as bc
import edge_cases as ec
import stralg_amd
from sam_cases import ROOT
from stralg_amd import api

pytestmark = pytest.mark.gpu

MAPPER = os.path.join(ROOT, "tools", "stralg_amd_readmapper")


@pytest.fixture(scope="module")
def cases():
    return ec.edge_cases()


@pytest.fixture(scope="module")
def mapper():
    if not os.path.exists(MAPPER):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "stralg_amd", "csrc"), "mapper"])
    return MAPPER


@pytest.fixture(scope="module")
def indexes(gpu_ctx):
    """(fasta, form) -> a resident index, built once"""
    made = {}

    def get(fasta, **form):
        key = (fasta, tuple(sorted(form.items())))
        if key not in made:
            made[key] = stralg_amd.Index.from_fasta(fasta, ctx=gpu_ctx, **form)
        return made[key]

    yield get
    for idx in made.values():
        idx.close()


# ---- the oracle -------------------------------------------------------------------------------------------------------------
def test_oracle_counts(cases):
    ec.check_table(cases)
    ec.check_pairs_table(cases)


# ---- every case, every k, every flag set --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", ec.KS, ids=ec.KS_IDS)
def test_flag_sets(gpu_ctx, indexes, cases, name, k):
    c = cases[name]

    def stream(case, k, **flags):
        return stralg_amd.map_reads(case["fasta"], case["fastq"], k, ctx=gpu_ctx, **flags)

    ec.check_flag_sets(gpu_ctx, indexes(c["fasta"]), stream, c, name, k)


# ---- the index forms ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(ec.FORMS))
@pytest.mark.parametrize("name", ["block-edges", "deep-k"])
def test_index_forms(gpu_ctx, indexes, cases, name, form):
    ec.check_form(indexes(cases[name]["fasta"], **ec.FORMS[form]), cases[name], name)


@pytest.mark.parametrize("form", ec.MANY_FORMS)
def test_index_forms_of_many_records(gpu_ctx, indexes, cases, form):
    ec.check_form(indexes(cases["many-records"]["fasta"], **ec.FORMS[form]), cases["many-records"], "many-records")


def test_many_records_cannot_be_packed(gpu_ctx, cases):
    ec.check_packed_refused(gpu_ctx, stralg_amd.Index, cases["many-records"])


# ---- the loop's switches ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 3, 33])
def test_batches(gpu_ctx, indexes, cases, batch):
    c = cases["many-records"]
    ec.check_batches(gpu_ctx, indexes(c["fasta"]), c, batch)


def test_sixteen_byte_windows(gpu_ctx, indexes, cases):
    c = cases["many-records"]
    ec.check_sixteen_byte_windows(gpu_ctx, indexes(c["fasta"]), c)


def test_room_of_one_hit(gpu_ctx, indexes, cases):
    c = cases["many-records"]
    ec.check_room_of_one_hit(gpu_ctx, indexes(c["fasta"]), c)


def test_sampled_index_located_in_runs_of_five(gpu_ctx, indexes, cases):
    c = cases["many-records"]
    ec.check_located_in_runs_of_five(gpu_ctx, indexes(c["fasta"], **ec.FORMS["sampled-1024"]), c)


@pytest.mark.parametrize("window", [16, 4099])
def test_reads_of_2046_symbols_with_tags(gpu_ctx, indexes, cases, window):
    c = cases["block-edges"]
    ec.check_longest_reads(gpu_ctx, indexes(c["fasta"]), c, window)


# ---- pairs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,batch", [(k, b) for k in ec.PAIRS for b in ((0, 3) if k[1] == 2 else (0,))],
                         ids=lambda v: "%s-k%d" % v[:2] if isinstance(v, tuple) else "batch%d" % v)
def test_pairs(gpu_ctx, indexes, cases, key, batch):
    c = cases[key[0]]
    ec.check_pairs(gpu_ctx, indexes(c["fasta"]), c, key, batch)


# ---- the same bytes from run to run ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ec.CASES))
def test_second_call_and_fresh_context(gpu_ctx, indexes, cases, name):
    fresh = api.Context(0)
    try:
        ec.check_same_bytes(indexes(cases[name]["fasta"]), fresh, stralg_amd.Index, cases[name], name)
    finally:
        fresh.close()


# ---- the tool -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_memory", [True, False], ids=["in-memory", "index-file"])
def test_tool(mapper, tmp_path, cases, in_memory):
    c = cases["many-records"]
    fa, fq = tmp_path / "genome.fa", tmp_path / "reads.fq"
    fa.write_bytes(c["fasta"])
    fq.write_bytes(c["fastq"])
    if not in_memory:
        subprocess.run([mapper, "-p", str(fa)], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    args = ["--best", "--mapq", "--unmapped", "--header"] + (["-i"] if in_memory else []) + ["-d", "2", str(fa), str(fq)]
    got = subprocess.run([mapper] + args, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=300).stdout
    bc.check_text(got, ec.want(c, 2, best=True, unmapped=True, header=True, mapq=True))
