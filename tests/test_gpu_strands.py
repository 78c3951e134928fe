"""Both strands on the GPU (tests/strand_cases.py): the mapper with both_strands=True against the text composed from the
reference mapper's two recorded outputs (tests/golden/golden_sam_strands.npz) through stralg_amd.map_reads, a resident
index in its four forms and the command-line tool; sx_fastq_strands_dev and the flagged SAM emitter at the shapes of
tests/test_strands_cpu.py (the device builds the emitter with slices of 16 KiB where the harness has 256 bytes)."""
import hashlib
import os
import subprocess

import pytest

import strand_cases as sc
import stralg_amd
from device_memory import GpuMemory
from sam_cases import ROOT

pytestmark = pytest.mark.gpu

MAPPER = os.path.join(ROOT, "tools", "stralg_amd_readmapper")


@pytest.fixture(scope="module")
def cases():
    return sc.strand_cases()


@pytest.fixture(scope="module")
def mem():
    return GpuMemory()


@pytest.fixture(scope="module")
def images():
    return sc.strand_images()


@pytest.fixture(scope="module")
def mapper():
    if not os.path.exists(MAPPER):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "stralg_amd", "csrc"), "mapper"])
    return MAPPER


def test_fixture_holds_every_case(cases):
    assert sorted(cases) == sorted(sc.ALL_CASES)


@pytest.mark.parametrize("name", sc.ALL_CASES)
def test_map_reads_both_strands(gpu_ctx, cases, name):
    c = cases[name]
    sc.check_strands(c, stralg_amd.map_reads(c["fasta"], c["fastq"], c["k"], ctx=gpu_ctx, both_strands=True))


@pytest.mark.parametrize("name", sc.ALL_CASES)
def test_index_both_strands(gpu_ctx, cases, name):
    c = cases[name]
    with stralg_amd.Index.from_fasta(c["fasta"], ctx=gpu_ctx) as idx:
        sc.check_strands(c, idx.map_reads(c["fastq"], c["k"], both_strands=True))


@pytest.mark.parametrize("form", [dict(), dict(compact=True), dict(compact=True, sa_sample=32),
                                  dict(compact=True, packed=True, sa_sample=32)], ids=["full", "compact", "sampled", "packed-sampled"])
def test_index_forms(gpu_ctx, cases, form):
    c = cases["two-records-flipped/k2"]
    with stralg_amd.Index.from_fasta(c["fasta"], ctx=gpu_ctx, **form) as idx:
        sc.check_strands(c, idx.map_reads(c["fastq"], c["k"], both_strands=True))
        assert idx.map_reads(c["fastq"], c["k"]) == c["forward"]  # (and one strand is what it was)
        assert sum(n for _, n in idx.map_reads_discard(c["fastq"], c["k"], both_strands=True)) == len(c["want"])


@pytest.mark.parametrize("window,batch", [(1000, 0), (1 << 16, 0), (1 << 20, 9)])
def test_windows_and_batches(gpu_ctx, cases, window, batch):
    c = cases["two-records-flipped/k1"]
    records = [(n, stralg_amd.build_complete_table(s, True, gpu_ctx)) for n, s in gpu_ctx.fasta_records(c["fasta"])]
    chunks = []
    gpu_ctx.set_sam_window_bytes(window)
    gpu_ctx.set_sam_batch_reads(batch)
    try:
        gpu_ctx.map_reads_stream(records, c["fastq"], c["k"], chunks.append, both_strands=True)
    finally:
        gpu_ctx.set_sam_window_bytes(0)
        gpu_ctx.set_sam_batch_reads(0)
    assert len(chunks) > (1 if window < len(c["want"]) else 0) and max(len(x) for x in chunks) <= (window + 15) // 16 * 16
    sc.check_strands(c, b"".join(chunks))


def test_same_text_from_fresh_contexts(cases):
    c = cases["two-records-flipped/k2"]
    digests = []
    for _ in range(2):
        ctx = stralg_amd.Context(0)
        try:
            digests.append(hashlib.sha256(stralg_amd.map_reads(c["fasta"], c["fastq"], c["k"], ctx=ctx, both_strands=True)).digest())
        finally:
            ctx.close()
    assert digests[0] == digests[1] == hashlib.sha256(c["want"]).digest()


@pytest.mark.parametrize("in_memory", [True, False], ids=["-i", "bwttables"])
def test_tool_both_strands(mapper, cases, tmp_path, in_memory):
    c = cases["two-records-flipped/k1"]
    fa, fq = tmp_path / "genome.fa", tmp_path / "reads.fq"
    fa.write_bytes(c["fasta"])
    fq.write_bytes(c["fastq"])
    if not in_memory:
        subprocess.run([mapper, "-p", str(fa)], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    args = (["-i"] if in_memory else []) + ["--both-strands", "-d", str(c["k"]), str(fa), str(fq)]
    got = subprocess.run([mapper] + args, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=300).stdout
    sc.check_strands(c, got)
    # with the other options and two FASTQ files; without the option the text is the one-strand text
    got = subprocess.run([mapper, "--compact", "--packed", "--sa-sample", "32"] + args + [str(fq)], check=True, stdout=subprocess.PIPE,
                         stderr=subprocess.DEVNULL, timeout=300).stdout
    assert got == c["want"] + c["want"]
    args.remove("--both-strands")
    got = subprocess.run([mapper] + args, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=300).stdout
    assert got == c["forward"]


# ---- the kernels at the shapes of the CPU list ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.STRAND_IMAGE_NAMES)
def test_strands_of_an_image(gpu_ctx, mem, images, name):
    sc.check_strand_image(gpu_ctx, mem, *images[name])


def test_strands_of_the_fixtures_reads(gpu_ctx, mem, cases):
    for name in ("hg38/reads-100-10-0/k1", "hg38/reads-1000-200-1/k1", "two-records-flipped/k1"):
        sc.check_strand_image(gpu_ctx, mem, cases[name]["fastq"], 0)


def test_flags_on_neighbouring_reads(gpu_ctx, mem):
    sc.check_flags(gpu_ctx, mem, sc.flag_case())


def test_flags_cut_by_windows_of_16_bytes(gpu_ctx, mem):
    sc.check_flags(gpu_ctx, mem, sc.small_flag_case())


def test_flags_with_several_records(gpu_ctx, mem):
    sc.check_flags(gpu_ctx, mem, sc.several_records_flag_case())
