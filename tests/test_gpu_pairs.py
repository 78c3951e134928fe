"""Paired-end reads on the GPU (tests/pairs_cases.py): every case of the oracle's table through stralg_amd.map_pairs and a
resident index (the 2.1 M-line case by its digest), the four forms of the index, batches and windows, best and no indels,
the command-line tool with -2, and the descriptor emitter at the shapes of tests/test_pairs_cpu.py (the device builds the
emitter with slices of 16 KiB where the harness has 256 bytes)."""
import hashlib
import os
import subprocess

import pytest

import pairs_cases as pc
import stralg_amd
from device_memory import GpuMemory
from sam_cases import ROOT

pytestmark = pytest.mark.gpu

MAPPER = os.path.join(ROOT, "tools", "stralg_amd_readmapper")


@pytest.fixture(scope="module")
def mem():
    return GpuMemory()


@pytest.fixture(scope="module")
def mapper():
    if not os.path.exists(MAPPER):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "stralg_amd", "csrc"), "mapper"])
    return MAPPER


@pytest.fixture(scope="module")
def indexes(gpu_ctx):
    """fasta -> a full resident index, built once"""
    made = {}

    def get(fasta):
        if fasta not in made:
            made[fasta] = stralg_amd.Index.from_fasta(fasta, ctx=gpu_ctx)
        return made[fasta]

    yield get
    for idx in made.values():
        idx.close()


@pytest.mark.parametrize("key", pc.CASES, ids=pc.case_id)
def test_cases(gpu_ctx, indexes, key):
    c = pc.pair_case(key)
    assert c["want"].count(b"\n") == pc.COUNTS[key][0]
    check = pc.check_digest if key == pc.BIG else pc.check_text
    check(indexes(c["fasta"]).map_pairs(c["fastq1"], c["fastq2"], c["k"], min_insert=c["lo"], max_insert=c["hi"]), c["want"])
    if key != pc.BIG:  # (the module-level call builds an index of its own)
        check(stralg_amd.map_pairs(c["fasta"], c["fastq1"], c["fastq2"], c["k"], min_insert=c["lo"], max_insert=c["hi"], ctx=gpu_ctx), c["want"])


@pytest.mark.parametrize("form", [dict(), dict(compact=True), dict(compact=True, sa_sample=32),
                                  dict(compact=True, packed=True, sa_sample=32)], ids=["full", "compact", "sampled", "packed-sampled"])
def test_index_forms(gpu_ctx, form):
    c = pc.pair_case(pc.GRID)
    with stralg_amd.Index.from_fasta(c["fasta"], ctx=gpu_ctx, **form) as idx:
        pc.check_text(idx.map_pairs(c["fastq1"], c["fastq2"], c["k"], min_insert=c["lo"], max_insert=c["hi"]), c["want"])
        gpu_ctx.set_locate_chunk_rows(5)  # (a sampled index: runs shorter than one pair's lines)
        try:
            seen = idx.map_pairs_discard(c["fastq1"], c["fastq2"], c["k"], c["lo"], c["hi"])
        finally:
            gpu_ctx.set_locate_chunk_rows(0)
        assert sum(n for _, n in seen) == len(c["want"])


@pytest.mark.parametrize("window", [16, 4096])
@pytest.mark.parametrize("batch", [1, 3, 33])
def test_batches_and_windows(gpu_ctx, indexes, batch, window):
    c = pc.pair_case(pc.GRID)
    chunks = pc.run(gpu_ctx, indexes(c["fasta"]), c, window=window, batch=batch)
    assert max(len(x) for x in chunks) <= window
    pc.check_text(b"".join(chunks), c["want"])
    stats = gpu_ctx.map_stats()
    assert stats["batch_first"] == 4 * batch and stats["batches"] == -(-200 // batch)


def test_small_room_halves_to_single_pairs(gpu_ctx, indexes):
    c = pc.pair_case(("test-out/k1", "overlap", 0, 500))
    pc.check_text(b"".join(pc.run(gpu_ctx, indexes(c["fasta"]), c, room=1)), c["want"])
    stats = gpu_ctx.map_stats()
    assert stats["halved"] >= 2 and stats["batch_final"] == 4


def test_descriptors_halve_a_batch_whose_lines_fit(gpu_ctx, indexes):
    """a room of lines and descriptors alone: the lines of the batch of all four pairs of test-out/k1 overlap (118), fewer
    than its 658 descriptors; the hits' room stays by the free memory"""
    key = ("test-out/k1", "overlap", 0, 500)
    room = pc.batch_lines(key)
    assert room == 118
    _, st = pc.check_pairs_room(gpu_ctx, indexes(pc.pair_case(key)["fasta"]), key, room)
    assert st["batch_first"] == 16


def test_lines_halve_a_batch_whose_hits_fit(gpu_ctx, indexes):
    _, st = pc.check_pairs_room(gpu_ctx, indexes(pc.pair_case(pc.GRID)["fasta"]), pc.GRID, 1, batch=33)
    assert st["batch_first"] == 4 * 33


@pytest.mark.parametrize("best,indels", [(True, True), (False, False), (True, False)])
def test_best_and_no_indels(gpu_ctx, indexes, best, indels):
    """on two-records-best, the reads on the two-records genome whose texts are recorded at every stratum (best_cases())"""
    c = pc.flagged_case("two-records-best", 2, best, indels)
    assert c["pairs"] > 0
    pc.check_text(b"".join(pc.run(gpu_ctx, indexes(c["fasta"]), c, best=best, indels=indels)), c["want"])


def test_no_indels_on_two_records_flipped_k2(gpu_ctx, indexes):
    """indels=False (best off) on two-records-flipped/k2 overlap [30, 3000]: the oracle over the recorded lines of pure M
    (best needs the strata of every edit count, which two-records-flipped does not record: test_best_and_no_indels)"""
    c = pc.no_indels_case("two-records-flipped/k2", "overlap", 30, 3000)
    assert c["want"].count(b"\n") == 184 and c["pairs"] == 87
    pc.check_text(indexes(c["fasta"]).map_pairs(c["fastq1"], c["fastq2"], c["k"], min_insert=30, max_insert=3000, indels=False), c["want"])
    pc.check_text(stralg_amd.map_pairs(c["fasta"], c["fastq1"], c["fastq2"], c["k"], min_insert=30, max_insert=3000, indels=False, ctx=gpu_ctx),
                  c["want"])


def test_same_text_from_fresh_contexts():
    c = pc.pair_case(("two-records-flipped/k1", "overlap", 0, 500))
    digests = []
    for _ in range(2):
        ctx = stralg_amd.Context(0)
        try:
            digests.append(hashlib.sha256(stralg_amd.map_pairs(c["fasta"], c["fastq1"], c["fastq2"], c["k"], c["lo"], c["hi"], ctx=ctx)).digest())
        finally:
            ctx.close()
    assert digests[0] == digests[1] == hashlib.sha256(c["want"]).digest()


@pytest.mark.parametrize("in_memory", [True, False], ids=["-i", "bwttables"])
def test_tool_with_mates(mapper, tmp_path, in_memory):
    c = pc.pair_case(pc.GRID)
    fa, fq1, fq2 = tmp_path / "genome.fa", tmp_path / "reads.fq", tmp_path / "mates.fq"
    fa.write_bytes(c["fasta"])
    fq1.write_bytes(c["fastq1"])
    fq2.write_bytes(c["fastq2"])
    if not in_memory:
        subprocess.run([mapper, "-p", str(fa)], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    args = (["-i"] if in_memory else []) + ["-d", str(c["k"]), "-2", str(fq2), "--min-insert", str(c["lo"]), "--max-insert", str(c["hi"]), str(fa), str(fq1)]
    got = subprocess.run([mapper] + args, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=300).stdout
    pc.check_text(got, c["want"])
    got = subprocess.run([mapper, "--compact", "--packed", "--sa-sample", "32"] + args, check=True, stdout=subprocess.PIPE,
                         stderr=subprocess.DEVNULL, timeout=300).stdout
    pc.check_text(got, c["want"])
    # refused: with --tags, with a second reads file, with a window the wrong way round
    for extra in (["--tags"], [str(fq1)], ["--min-insert", "4000"]):
        r = subprocess.run([mapper] + args + extra, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=300)
        assert r.returncode != 0 and r.stdout == b"", extra


def test_descriptors_made_up(gpu_ctx, mem):
    pc.check_descriptors(gpu_ctx, mem, pc.descriptor_case())
