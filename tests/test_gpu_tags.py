"""NM:i and MD:Z behind QUAL on the GPU (tests/tags_cases.py): the cases of tests/test_tags_cpu.py at the same shapes through
the same helpers (the device lays a slice of 16 KB out in a workgroup where the harness has 256 bytes), the text's digest from
two fresh contexts, and the command-line tool with --tags."""
import hashlib
import os
import subprocess

import pytest

import best_cases as bc
import hamming_cases as hc
import stralg_amd
import tags_cases as tc
from device_memory import GpuMemory
from sam_cases import ROOT

pytestmark = pytest.mark.gpu

MAPPER = os.path.join(ROOT, "tools", "stralg_amd_readmapper")
KERNEL = tc.kernel_cases()
REFUSED = {c["name"]: c for c in tc.refused_cases()}


@pytest.fixture(scope="module")
def cases():
    return tc.whole_cases()


@pytest.fixture(scope="module")
def flag_cases():
    return bc.best_cases()


@pytest.fixture(scope="module")
def mem():
    return GpuMemory()


@pytest.fixture(scope="module")
def mapper():
    if not os.path.exists(MAPPER):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "stralg_amd", "csrc"), "mapper"])
    return MAPPER


# ---- the kernels' entries on made-up hits ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.KERNEL_CASE_NAMES)
def test_kernel_text(gpu_ctx, mem, name):
    tc.check_tag_text(gpu_ctx, mem, KERNEL[name])


@pytest.mark.parametrize("name", tc.REFUSED_NAMES)
def test_kernel_refuses(gpu_ctx, mem, name):
    tc.check_tag_refused(gpu_ctx, mem, REFUSED[name])


# ---- the mapper -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.WHOLE_TEXT)
def test_whole_text(gpu_ctx, cases, name):
    c = cases[name]
    chunks, st = tc.stream_tagged(gpu_ctx, stralg_amd.Index, c, c["k"])
    bc.check_text(b"".join(chunks), tc.want_whole(c))
    assert st["retries"] == 0


@pytest.mark.parametrize("name,k,both,best,indels", tc.FLAG_PARAMS, ids=tc.FLAG_IDS)
def test_with_the_other_flags(gpu_ctx, flag_cases, name, k, both, best, indels):
    c = flag_cases[name]
    chunks, _ = tc.stream_tagged(gpu_ctx, stralg_amd.Index, c, k, both, best, indels)
    bc.check_text(b"".join(chunks), tc.want_flags(c, k, both, best, indels))


@pytest.mark.parametrize("form", hc.FORMS, ids=hc.FORM_IDS)
def test_index_forms(gpu_ctx, cases, flag_cases, form):
    tc.check_index_form(gpu_ctx, stralg_amd.Index, cases, flag_cases, form)


@pytest.mark.parametrize("window,batch", hc.WINDOWS)
def test_windows_and_batches(gpu_ctx, flag_cases, window, batch):
    tc.check_windows(gpu_ctx, stralg_amd.Index, flag_cases["two-records-best"], window, batch)


def test_module_level_map_reads_and_the_refusals(gpu_ctx, cases, flag_cases):
    c = cases["test-out/k2"]
    bc.check_text(stralg_amd.map_reads(c["fasta"], c["fastq"], 2, ctx=gpu_ctx, tags=True), tc.want_whole(c))
    assert stralg_amd.map_reads(c["fasta"], c["fastq"], 2, ctx=gpu_ctx) == c["sam"]
    records = [(n, stralg_amd.build_complete_table(s, True, gpu_ctx)) for n, s in gpu_ctx.fasta_records(c["fasta"])]
    chunks = []
    with pytest.raises(stralg_amd.api.StralgAmdError, match="code -1"):
        gpu_ctx.map_reads_stream(records, c["fastq"], 2, chunks.append, tags=True)
    with stralg_amd.Index.from_tables(records, ctx=gpu_ctx) as idx:  # (these tables bring their strings)
        bc.check_text(idx.map_reads(c["fastq"], 2, tags=True), tc.want_whole(c))
    api = stralg_amd.api
    records = [(n, api.BwtTable(t.remap_table, api.SuffixArray(None, t.sa.array), t.c_table, t.o_table, t.ro_table)) for n, t in records]
    with stralg_amd.Index.from_tables(records, ctx=gpu_ctx) as bare:
        with pytest.raises(stralg_amd.api.StralgAmdError, match="code -1"):
            bare.map_reads(c["fastq"], 2, sink=chunks.append, tags=True)
        assert not chunks
        assert bare.map_reads(c["fastq"], 2) == c["sam"]
    lib = gpu_ctx.lib
    assert [lib.sx_map_reads_limit(5, 5, f) for f in (64, 65, 72, 80, 89, 66, 68, 96)] == [0] * 5 + [stralg_amd._lib.SX_E_ARG] * 3


def test_same_text_from_fresh_contexts(flag_cases):
    c = flag_cases["two-records-best"]
    digests = []
    for _ in range(2):
        ctx = stralg_amd.Context(0)
        try:
            got = stralg_amd.map_reads(c["fasta"], c["fastq"], 2, ctx=ctx, both_strands=True, tags=True)
            digests.append(hashlib.sha256(got).digest())
            assert stralg_amd.map_reads(c["fasta"], c["fastq"], 2, ctx=ctx, both_strands=True, tags=True) == got  # (and a second call)
        finally:
            ctx.close()
    assert digests[0] == digests[1] == hashlib.sha256(tc.want_flags(c, 2, True, False, True)).digest()


@pytest.mark.parametrize("in_memory", [True, False], ids=["-i", "bwttables"])
def test_tool_tags(mapper, flag_cases, tmp_path, in_memory):
    c = flag_cases["two-records-best"]
    fa, fq = tmp_path / "genome.fa", tmp_path / "reads.fq"
    fa.write_bytes(c["fasta"])
    fq.write_bytes(c["fastq"])
    if not in_memory:
        subprocess.run([mapper, "-p", str(fa)], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    args = (["-i"] if in_memory else []) + ["--tags", "-d", "2", str(fa), str(fq)]
    got = subprocess.run([mapper] + args, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=300).stdout
    bc.check_text(got, tc.want_flags(c, 2, False, False, True))
    got = subprocess.run([mapper, "--best", "--both-strands", "--no-indels"] + args, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                         timeout=300).stdout
    bc.check_text(got, tc.want_flags(c, 2, True, True, False))
    got = subprocess.run([mapper, "--compact", "--packed", "--sa-sample", "32"] + args, check=True, stdout=subprocess.PIPE,
                         stderr=subprocess.DEVNULL, timeout=300).stdout
    bc.check_text(got, tc.want_flags(c, 2, False, False, True))
    args.remove("--tags")
    got = subprocess.run([mapper] + args, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=300).stdout
    assert got == c["fwd"][2]
