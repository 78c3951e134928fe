"""Best-stratum mapping on the GPU (tests/best_cases.py): the mapper with best=True against the text composed from the
reference mapper's recorded outputs at -d 0, 1, 2 (tests/golden/golden_sam_best.npz) through stralg_amd.map_reads, a resident
index in its four forms and the command-line tool; sx_patterns_select_dev and sx_bwt_best_search_dev at the shapes of
tests/test_best_cpu.py (the device runs the search with 2^18 lanes where the harness has 256)."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import approx_model
import best_cases as bc
import stralg_amd
from approx_cases import approx_cases, remapped
from device_memory import GpuMemory
from sam_cases import ROOT

pytestmark = pytest.mark.gpu

MAPPER = os.path.join(ROOT, "tools", "stralg_amd_readmapper")


@pytest.fixture(scope="module")
def cases():
    return bc.best_cases()


@pytest.fixture(scope="module")
def mem():
    return GpuMemory()


@pytest.fixture(scope="module")
def mapper():
    if not os.path.exists(MAPPER):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "stralg_amd", "csrc"), "mapper"])
    return MAPPER


@pytest.mark.parametrize("name,k,both", bc.BEST_PARAMS, ids=bc.BEST_IDS)
def test_map_reads_best(gpu_ctx, cases, name, k, both):
    c = cases[name]
    bc.check_text(stralg_amd.map_reads(c["fasta"], c["fastq"], k, ctx=gpu_ctx, both_strands=both, best=True), bc.want_of(c, k, both))


@pytest.mark.parametrize("name,k,both", bc.BEST_PARAMS, ids=bc.BEST_IDS)
def test_index_best(gpu_ctx, cases, name, k, both):
    c = cases[name]
    with stralg_amd.Index.from_fasta(c["fasta"], ctx=gpu_ctx) as idx:
        bc.check_text(idx.map_reads(c["fastq"], k, both_strands=both, best=True), bc.want_of(c, k, both))


@pytest.mark.parametrize("form", [dict(), dict(compact=True), dict(compact=True, sa_sample=32),
                                  dict(compact=True, packed=True, sa_sample=32)], ids=["full", "compact", "sampled", "packed-sampled"])
def test_index_forms(gpu_ctx, cases, form):
    c = cases["two-records-best"]
    want = bc.want_of(c, 2, True)
    with stralg_amd.Index.from_fasta(c["fasta"], ctx=gpu_ctx, **form) as idx:
        bc.check_text(idx.map_reads(c["fastq"], 2, both_strands=True, best=True), want)
        bc.check_text(idx.map_reads(c["fastq"], 2, both_strands=True), bc.plain_of(c, 2, True))  # (and the plain call is what it was)
        assert sum(n for _, n in idx.map_reads_discard(c["fastq"], 2, both_strands=True, best=True)) == len(want)


def test_best_at_no_edits_is_the_plain_text(gpu_ctx, cases):
    c = cases["two-records-best"]
    for both in (False, True):
        best = stralg_amd.map_reads(c["fasta"], c["fastq"], 0, ctx=gpu_ctx, both_strands=both, best=True)
        assert best == stralg_amd.map_reads(c["fasta"], c["fastq"], 0, ctx=gpu_ctx, both_strands=both) == bc.plain_of(c, 0, both)


@pytest.mark.parametrize("window,batch", [(1000, 0), (1 << 16, 7), (1 << 20, 33), (1 << 20, 1)])
def test_windows_and_batches(gpu_ctx, cases, window, batch):
    c = cases["two-records-best"]
    records = [(n, stralg_amd.build_complete_table(s, True, gpu_ctx)) for n, s in gpu_ctx.fasta_records(c["fasta"])]
    for both in (False, True):
        want = bc.want_of(c, 2, both)
        chunks = []
        gpu_ctx.set_sam_window_bytes(window)
        gpu_ctx.set_sam_batch_reads(batch)
        try:
            gpu_ctx.map_reads_stream(records, c["fastq"], 2, chunks.append, both_strands=both, best=True)
        finally:
            gpu_ctx.set_sam_window_bytes(0)
            gpu_ctx.set_sam_batch_reads(0)
        assert max(len(x) for x in chunks) <= (window + 15) // 16 * 16
        bc.check_text(b"".join(chunks), want)


def test_same_text_from_fresh_contexts(cases):
    c = cases["two-records-best"]
    digests = []
    for _ in range(2):
        ctx = stralg_amd.Context(0)
        try:
            digests.append(hashlib.sha256(stralg_amd.map_reads(c["fasta"], c["fastq"], 2, ctx=ctx, both_strands=True, best=True)).digest())
        finally:
            ctx.close()
    assert digests[0] == digests[1] == hashlib.sha256(bc.want_of(c, 2, True)).digest()


@pytest.mark.parametrize("in_memory", [True, False], ids=["-i", "bwttables"])
def test_tool_best(mapper, cases, tmp_path, in_memory):
    c = cases["two-records-best"]
    fa, fq = tmp_path / "genome.fa", tmp_path / "reads.fq"
    fa.write_bytes(c["fasta"])
    fq.write_bytes(c["fastq"])
    if not in_memory:
        subprocess.run([mapper, "-p", str(fa)], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    args = (["-i"] if in_memory else []) + ["--best", "-d", "2", str(fa), str(fq)]
    got = subprocess.run([mapper] + args, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=300).stdout
    bc.check_text(got, bc.want_of(c, 2, False))
    got = subprocess.run([mapper, "--both-strands"] + args, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=300).stdout
    bc.check_text(got, bc.want_of(c, 2, True))
    # with the other options; without the option the text is the plain text
    got = subprocess.run([mapper, "--compact", "--packed", "--sa-sample", "32", "--both-strands"] + args, check=True, stdout=subprocess.PIPE,
                         stderr=subprocess.DEVNULL, timeout=300).stdout
    bc.check_text(got, bc.want_of(c, 2, True))
    args.remove("--best")
    got = subprocess.run([mapper] + args, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=300).stdout
    assert got == c["fwd"][2]


# ---- the kernels at the shapes of the CPU list ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.SELECT_NAMES)
def test_select(gpu_ctx, mem, name):
    bc.check_select(gpu_ctx, mem, bc.select_cases()[name])


def test_best_search_on_the_approx_fixture(gpu_ctx, mem):
    for name, cs in approx_cases().items():
        sym, sigma = remapped(cs["raw"])
        sa, c, o, ro = approx_model.tables(sym, sigma)
        for r in (ro, None):
            T = bc.Tables(mem, c, o, r, sigma, cs["pat"], cs["pat_off"])
            strata, ho, hits, _ = bc.check_best_search(gpu_ctx, T, 2)
            assert np.diff(ho.astype(np.int64)).sum() == hits.size
