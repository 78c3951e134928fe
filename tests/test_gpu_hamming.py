"""The search without indels on the GPU (tests/hamming_cases.py): the cases of tests/test_hamming_cpu.py at the same shapes
through the same helpers (the device runs the search with 2^18 lanes where the harness has 256), a pattern set larger
than the lanes, the text's digest from two fresh contexts, and the command-line tool with --no-indels."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import approx_model
import best_cases as bc
import hamming_cases as hc
import stralg_amd
from approx_cases import approx_cases, remapped
from device_memory import GpuMemory
from sam_cases import ROOT

pytestmark = pytest.mark.gpu

MAPPER = os.path.join(ROOT, "tools", "stralg_amd_readmapper")
APPROX = approx_cases()
NAMES = sorted(APPROX)


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


@pytest.fixture(scope="module")
def tables():
    made = {}

    def get(name):
        if name not in made:
            sym, sigma = remapped(APPROX[name]["raw"])
            made[name] = approx_model.tables(sym, sigma) + (sigma,)
        return made[name]
    return get


# ---- the search calls -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fixture_streams(gpu_ctx, mem, tables, name):
    want = hc.check_fixture_case(gpu_ctx, mem, APPROX[name], tables(name))
    sigma = tables(name)[4]
    assert hc.check_forms(gpu_ctx, mem, stralg_amd.Index, APPROX[name], tables(name), want) == (sigma <= 128) + (sigma <= 8)


@pytest.mark.parametrize("sigma,n", hc.RANDOM_SHAPES)
def test_random_against_the_scan(gpu_ctx, mem, sigma, n):
    hc.check_random(gpu_ctx, mem, sigma, n)


def test_edges(gpu_ctx, mem, tables):
    """k = 0: the plain call's hits; max_edits = -1; m = 1; k >= m; patterns without hits; a capacity one short; the limits"""
    sa, c, o, ro, sigma = tables("rand/s5/n700/k2")
    cs = APPROX["rand/s5/n700/k2"]
    T = hc.Tables(mem, c, o, ro, sigma, cs["pat"], cs["pat_off"])
    ho, hits, failure = T.hamming(gpu_ctx, 0)
    plain_ho, plain_hits = T.approx(gpu_ctx, 0)
    assert failure is None and hits.size and ho.tolist() == plain_ho.tolist() and hits.tobytes() == plain_hits.tobytes()
    ho, hits, failure = T.hamming(gpu_ctx, -1)
    assert failure is None and not ho.any() and hits.size == 0
    want_ho, want_hits, _ = T.hamming(gpu_ctx, 2)
    total = int(want_ho[-1])
    ho, hits, failure = T.hamming(gpu_ctx, 2, capacity=total - 1)
    assert failure is not None and "code %d" % stralg_amd._lib.SX_E_CAPACITY in str(failure)
    assert ho.tolist() == want_ho.tolist() and not hits.view(np.uint8).any()
    # short patterns on a text of two letters
    rng = np.random.default_rng(5)
    n = 400
    sym = rng.integers(1, 3, n).astype(np.uint8)
    sa, c, o, ro = approx_model.tables(sym, 3)
    pats = [np.array([1], np.uint8), np.array([2], np.uint8), np.array([1, 2, 1], np.uint8), np.zeros(0, np.uint8), np.array([1, 0, 1], np.uint8),
            np.array([1, 3], np.uint8)]
    flat, off = hc.flat_of(pats)
    for k in (0, 1, 8):
        ho, hits, _ = hc.Tables(mem, c, o, ro, 3, flat, off).hamming(gpu_ctx, k)
        got = hc.positions_of(hits, ho, sa)
        assert got[:3] == [hc.brute(sym, p, k)[0] for p in pats[:3]] and got[3:] == [[], [], []]
    assert got[2] == list(range(n - 2))
    with pytest.raises(stralg_amd.api.StralgAmdError, match="code -1"):
        T.hamming(gpu_ctx, 9)
    long = np.ones(1 << 15, np.uint8)
    with pytest.raises(stralg_amd.api.StralgAmdError, match="code -1"):
        hc.Tables(mem, c, o, ro, 3, long, np.array([0, long.size], np.uint32)).hamming(gpu_ctx, 1)


@pytest.mark.parametrize("name", NAMES)
def test_best_search(gpu_ctx, mem, tables, name):
    hc.check_best(gpu_ctx, mem, APPROX[name], tables(name))


def test_more_patterns_than_lanes(gpu_ctx, mem):
    """2^18 + 257 patterns from a pool of 64: lanes take a second pattern from the counter"""
    rng = np.random.default_rng(23)
    sigma, n, m, k = 5, 3000, 12, 1
    sym = rng.integers(1, sigma, n).astype(np.uint8)
    sa, c, o, ro = approx_model.tables(sym, sigma)
    pool = []
    for q in range(64):
        a = int(rng.integers(0, n - m))
        p = sym[a:a + m].copy()
        if q & 1:
            p[int(rng.integers(0, m))] = int(rng.integers(1, sigma))
        pool.append(p)
    want = [hc.brute(sym, p, k)[0] for p in pool]
    assert all(want[q] for q in range(0, 64, 2))
    count = (1 << 18) + 257
    pick = rng.integers(0, 64, count)
    flat = np.stack(pool)[pick].reshape(-1)
    off = (np.arange(count + 1, dtype=np.uint64) * m).astype(np.uint32)
    ho, hits, failure = hc.Tables(mem, c, o, ro, sigma, flat, off).hamming(gpu_ctx, k)
    assert failure is None
    hc.check_pure(hits, ho, np.full(count, m))
    # per pattern of the pool the sorted positions, from its first copy; every copy then has that copy's intervals
    sizes = np.diff(ho.astype(np.int64))
    lr = np.stack([hits["L"], hits["R"]], axis=1)
    body = []
    for j in range(64):
        q = int(np.nonzero(pick == j)[0][0])
        body.append(lr[int(ho[q]):int(ho[q + 1])])
        assert sorted(int(p) for lo, hi in body[j].tolist() for p in sa[lo:hi]) == want[j], j
    assert (sizes == np.array([len(b) for b in body])[pick]).all()
    assert (lr == np.concatenate([body[j] for j in pick.tolist()])).all()


# ---- the mapper -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,both,best", hc.MAP_PARAMS, ids=hc.MAP_IDS)
def test_map_reads(gpu_ctx, cases, name, k, both, best):
    c = cases[name]
    got = stralg_amd.map_reads(c["fasta"], c["fastq"], k, ctx=gpu_ctx, both_strands=both, best=best, indels=False)
    bc.check_text(got, hc.want_of(c, k, both, best))


@pytest.mark.parametrize("form", hc.FORMS, ids=hc.FORM_IDS)
def test_index_forms(gpu_ctx, cases, form):
    hc.check_index_forms(gpu_ctx, stralg_amd.Index, cases["two-records-best"], form)


def test_no_edits_with_the_flag_is_the_plain_text(gpu_ctx, cases):
    c = cases["two-records-best"]
    for both in (False, True):
        got = stralg_amd.map_reads(c["fasta"], c["fastq"], 0, ctx=gpu_ctx, both_strands=both, indels=False)
        assert got == stralg_amd.map_reads(c["fasta"], c["fastq"], 0, ctx=gpu_ctx, both_strands=both) == bc.plain_of(c, 0, both)


@pytest.mark.parametrize("window,batch", hc.WINDOWS)
def test_windows_and_batches(gpu_ctx, cases, window, batch):
    c = cases["two-records-best"]
    records = [(n, stralg_amd.build_complete_table(s, True, gpu_ctx)) for n, s in gpu_ctx.fasta_records(c["fasta"])]
    hc.check_windows(gpu_ctx, records, c, window, batch)


def test_same_text_from_fresh_contexts(cases):
    c = cases["two-records-best"]
    digests = []
    for _ in range(2):
        ctx = stralg_amd.Context(0)
        try:
            digests.append(hashlib.sha256(stralg_amd.map_reads(c["fasta"], c["fastq"], 2, ctx=ctx, both_strands=True, indels=False)).digest())
        finally:
            ctx.close()
    assert digests[0] == digests[1] == hashlib.sha256(hc.want_of(c, 2, True, False)).digest()


@pytest.mark.parametrize("in_memory", [True, False], ids=["-i", "bwttables"])
def test_tool_no_indels(mapper, cases, tmp_path, in_memory):
    c = cases["two-records-best"]
    fa, fq = tmp_path / "genome.fa", tmp_path / "reads.fq"
    fa.write_bytes(c["fasta"])
    fq.write_bytes(c["fastq"])
    if not in_memory:
        subprocess.run([mapper, "-p", str(fa)], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    args = (["-i"] if in_memory else []) + ["--no-indels", "-d", "2", str(fa), str(fq)]
    got = subprocess.run([mapper] + args, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=300).stdout
    bc.check_text(got, hc.want_of(c, 2, False, False))
    got = subprocess.run([mapper, "--best", "--both-strands"] + args, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=300).stdout
    bc.check_text(got, hc.want_of(c, 2, True, True))
    got = subprocess.run([mapper, "--compact", "--packed", "--sa-sample", "32"] + args, check=True, stdout=subprocess.PIPE,
                         stderr=subprocess.DEVNULL, timeout=300).stdout
    bc.check_text(got, hc.want_of(c, 2, False, False))
    args.remove("--no-indels")
    got = subprocess.run([mapper] + args, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=300).stdout
    assert got == c["fwd"][2]
