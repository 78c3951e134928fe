"""Paired-end reads through the CPU execution harness (tests/pairs_cases.py): the oracle's own counts, sx_index_map_pairs
against the oracle on every case but the 2.1 M-line one (tests/test_gpu_pairs.py checks that one by its digest), batches
and windows, best and no indels, a sampled index, the window's edges, the refused calls, and the descriptor emitter over
made-up descriptors.  The harness builds the SAM kernels with a slice of 256 bytes a workgroup."""
import pytest

import pairs_cases as pc
from conftest import EMU_LIB
from device_memory import HarnessMemory
from stralg_amd import _lib, api

MEM = HarnessMemory()


@pytest.fixture(scope="module")
def indexes(emu_ctx):
    """fasta -> a full index on the harness, built once"""
    made = {}

    def get(fasta):
        if fasta not in made:
            made[fasta] = api.Index.from_fasta(fasta, ctx=emu_ctx)
        return made[fasta]

    yield get
    for idx in made.values():
        idx.close()


# ---- the oracle ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", pc.SMALL_CASES, ids=pc.case_id)
def test_oracle_counts(key):
    c = pc.pair_case(key)
    lines, pairs = pc.COUNTS[key]
    assert c["want"].count(b"\n") == lines
    assert pairs is None or c["pairs"] == pairs
    n = len(pc.sc.fastq_reads(c["fastq1"]))
    assert len(pc.sc.fastq_reads(c["fastq2"])) == n
    if key[0] == "test-out/k0":
        assert n == 4
    if key[0].startswith("two-records-flipped"):
        assert n == 200


def test_oracle_count_of_the_large_case():
    c = pc.pair_case(pc.BIG)
    assert c["want"].count(b"\n") == pc.COUNTS[pc.BIG][0]
    by_pair = {}
    for line in c["want"].split(b"\n")[:-1]:
        f = line.split(b"\t", 2)
        if int(f[1]) & 64:
            by_pair[f[0]] = by_pair.get(f[0], 0) + 2
    assert max(by_pair.values()) == 96272


def test_oracle_on_a_pair_by_hand():
    a = [b"m\t0\tchr\t10\t0\t5M\t*\t0\t0\tACGTA\tIIIII", b"m\t16\tchr\t40\t0\t2M1D3M\t*\t0\t0\tACGTA\tIIIII"]
    b = [b"n\t0\tchr\t7\t0\t1I3M\t*\t0\t0\tTTTT\t####", b"n\t16\tchr\t12\t0\t4M\t*\t0\t0\tTTTT\t####", b"n\t16\tother\t12\t0\t4M\t*\t0\t0\tTTTT\t####"]
    assert pc.span_of(b"2M1D3M") == 6 and pc.span_of(b"1I3M") == 3
    want = (b"m\t99\tchr\t10\t0\t5M\t=\t12\t6\tACGTA\tIIIII\n" b"n\t147\tchr\t12\t0\t4M\t=\t10\t-6\tTTTT\t####\n"
            b"m\t83\tchr\t40\t0\t2M1D3M\t=\t7\t-39\tACGTA\tIIIII\n" b"n\t163\tchr\t7\t0\t1I3M\t=\t40\t39\tTTTT\t####\n")
    assert pc.pair_text(a, b, 0, 500) == want
    assert pc.pair_text(a, b, 7, 38) == b"" and pc.pair_text(a, b, 6, 6) == want[:want.index(b"m\t83")]
    # the forward line must not end behind the reverse one, nor start behind it
    assert pc.pair_text([b"m\t0\tchr\t10\t0\t9M\t*\t0\t0\tA\tI"], [b"n\t16\tchr\t12\t0\t4M\t*\t0\t0\tT\t#"], 0, 500) == b""
    assert pc.pair_text([b"m\t0\tchr\t13\t0\t9M\t*\t0\t0\tA\tI"], [b"n\t16\tchr\t12\t0\t40M\t*\t0\t0\tT\t#"], 0, 500) == b""


# ---- the call against the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", pc.SMALL_CASES, ids=pc.case_id)
def test_cases_whole_text(emu_ctx, indexes, key):
    c = pc.pair_case(key)
    got = indexes(c["fasta"]).map_pairs(c["fastq1"], c["fastq2"], c["k"], min_insert=c["lo"], max_insert=c["hi"])
    pc.check_text(got, c["want"])


def test_downstream_pairing(emu_ctx, indexes):
    c0 = pc.sc.strand_cases()["two-records-flipped/k1"]
    fastq2, want, pairs = pc.paired(c0["fastq"], c0["want"], "downstream", 0, 2 ** 31)
    assert pairs > 0
    got = indexes(c0["fasta"]).map_pairs(c0["fastq"], fastq2, 1, min_insert=0, max_insert=2 ** 31)
    pc.check_text(got, want)


@pytest.mark.parametrize("window", [16, 4096])
@pytest.mark.parametrize("batch", [1, 3, 33])
def test_batches_and_windows(emu_ctx, indexes, batch, window):
    """a pair's lines cross windows; a pair never crosses a batch"""
    c = pc.pair_case(pc.GRID)
    chunks = pc.run(emu_ctx, indexes(c["fasta"]), c, window=window, batch=batch)
    assert max(len(x) for x in chunks) <= window
    pc.check_text(b"".join(chunks), c["want"])
    stats = emu_ctx.map_stats()
    assert stats["batch_first"] == 4 * batch and stats["batches"] == -(-200 // batch)


def test_small_room_halves_to_single_pairs(emu_ctx, indexes):
    """a room of one hit (which sets the room of lines and descriptors to 1 as well): the hits halve every batch down to a
    pair, which gets what it needs"""
    c = pc.pair_case(("test-out/k1", "overlap", 0, 500))
    chunks = pc.run(emu_ctx, indexes(c["fasta"]), c, room=1)
    pc.check_text(b"".join(chunks), c["want"])
    stats = emu_ctx.map_stats()
    assert stats["halved"] >= 2 and stats["batch_final"] == 4


def test_descriptors_halve_a_batch_whose_lines_fit(emu_ctx, indexes):
    """a room of lines and descriptors alone, exactly the lines of the batch of all four pairs of test-out/k1 overlap (118) and
    fewer than its 658 descriptors: that batch passes the lines' check and is halved by its descriptors"""
    key = ("test-out/k1", "overlap", 0, 500)
    room = pc.batch_lines(key)
    c = pc.pair_case(key)
    assert room == 118 and c["want"].count(b"\n") == 658
    _, st = pc.check_pairs_room(emu_ctx, indexes(c["fasta"]), key, room)
    assert st["batch_first"] == 16


def test_lines_halve_a_batch_whose_hits_fit(emu_ctx, indexes):
    """a room of one line and descriptor, the hits' room by the free memory: batches of 33 pairs are halved by their lines"""
    c = pc.pair_case(pc.GRID)
    _, st = pc.check_pairs_room(emu_ctx, indexes(c["fasta"]), pc.GRID, 1, batch=33)
    assert st["batch_first"] == 4 * 33


@pytest.mark.parametrize("best,indels", [(True, True), (False, False), (True, False)])
def test_best_and_no_indels(emu_ctx, indexes, best, indels):
    for name, k in (("two-records-best", 2), ("test-out", 2)):
        c = pc.flagged_case(name, k, best, indels)
        assert c["pairs"] > 0
        chunks = pc.run(emu_ctx, indexes(c["fasta"]), c, batch=7, best=best, indels=indels)
        pc.check_text(b"".join(chunks), c["want"])


def test_no_indels_on_two_records_flipped_k2(emu_ctx, indexes):
    """indels=False on two-records-flipped/k2 overlap [30, 3000]: the oracle over the recorded lines of pure M"""
    c = pc.no_indels_case("two-records-flipped/k2", "overlap", 30, 3000)
    assert c["want"].count(b"\n") == 184 and c["pairs"] == 87
    pc.check_text(b"".join(pc.run(emu_ctx, indexes(c["fasta"]), c, batch=33, indels=False)), c["want"])


def test_sampled_index_with_a_small_locate_chunk(emu_ctx):
    """a compact index with a sampled suffix array; the batch's positions are located in runs of at most 5 rows, fewer than one
    pair's lines"""
    c = pc.pair_case(pc.GRID)
    emu_ctx.set_locate_chunk_rows(5)
    try:
        with api.Index.from_fasta(c["fasta"], ctx=emu_ctx, compact=True, sa_sample=32) as idx:
            pc.check_text(b"".join(pc.run(emu_ctx, idx, c, batch=33)), c["want"])
            assert sum(n for _, n in idx.map_pairs_discard(c["fastq1"], c["fastq2"], c["k"], c["lo"], c["hi"])) == len(c["want"])
    finally:
        emu_ctx.set_locate_chunk_rows(0)


def test_window_edges(emu_ctx, indexes):
    c = pc.pair_case(("test-out/k0", "overlap", 0, 500))
    idx = indexes(c["fasta"])
    ts = sorted({int(l.split(b"\t")[8]) for l in c["want"].split(b"\n")[:-1] if int(l.split(b"\t")[8]) > 0})
    t = ts[0]
    reads = pc.sc.fastq_reads(c["fastq1"])
    by_name = pc.sc.lines_of(pc.sc.strand_cases()["test-out/k0"]["want"])
    want = b"".join(pc.pair_text(by_name.get(r[0], []), pc.lines_of_rc(by_name.get(r[0], [])), t, t) for r in reads)
    assert want and want.count(b"\n") < c["want"].count(b"\n") or len(ts) == 1
    pc.check_text(idx.map_pairs(c["fastq1"], c["fastq2"], 0, min_insert=t, max_insert=t), want)
    assert idx.map_pairs(c["fastq1"], c["fastq2"], 0, min_insert=0, max_insert=0) == b""
    assert idx.map_pairs(c["fastq1"], c["fastq2"], 0, min_insert=2 ** 32 - 1, max_insert=2 ** 32 - 1) == b""


def test_refused_calls_reach_no_sink(emu_ctx, indexes):
    c = pc.pair_case(("test-out/k1", "overlap", 0, 500))
    idx = indexes(c["fasta"])
    one_less = pc.sc.fastq_image(pc.sc.fastq_reads(c["fastq2"])[:-1])
    E = _lib.SX_E_ARG
    assert pc.raw_call(emu_ctx, idx, c["fastq1"], one_less, 1, 0, 500, 0) == (E, b"")
    assert pc.raw_call(emu_ctx, idx, c["fastq1"], b"", 1, 0, 500, 0) == (E, b"")
    assert pc.raw_call(emu_ctx, idx, c["fastq1"], c["fastq2"], 1, 501, 500, 0) == (E, b"")
    for flags in (_lib.SX_MAP_TAGS, 2, 4, 32, 128, 1 << 31, _lib.SX_MAP_TAGS | 1):
        assert pc.raw_call(emu_ctx, idx, c["fastq1"], c["fastq2"], 1, 0, 500, flags) == (E, b""), flags
    for k in (-1, 9):
        assert pc.raw_call(emu_ctx, idx, c["fastq1"], c["fastq2"], k, 0, 500, 0) == (E, b"")
    # SX_MAP_BOTH_STRANDS is implied: set or not, the same text
    rc, text = pc.raw_call(emu_ctx, idx, c["fastq1"], c["fastq2"], 1, 0, 500, _lib.SX_MAP_BOTH_STRANDS)
    assert rc == 0 and text == c["want"]


def test_the_limit(emu_ctx):
    """4 x pairs x records < 2^32"""
    limit = emu_ctx.lib.sx_map_pairs_limit
    assert limit(2 ** 30 - 1, 1) == 0 and limit(2 ** 30, 1) == _lib.SX_E_ARG
    assert limit(2 ** 15, 2 ** 15 - 1) == 0 and limit(2 ** 15, 2 ** 15) == _lib.SX_E_ARG
    assert limit(3, 357913941) == 0 and limit(3, 357913942) == _lib.SX_E_ARG
    assert limit(2 ** 63, 2) == _lib.SX_E_ARG and limit(2 ** 64 - 1, 2 ** 64 - 1) == _lib.SX_E_ARG  # (no wrap-around)
    assert limit(0, 0) == 0 and limit(0, 2 ** 40) == 0


def test_empty_images(emu_ctx, indexes):
    c = pc.pair_case(("test-out/k0", "overlap", 0, 500))
    assert indexes(c["fasta"]).map_pairs(b"", b"", 1) == b""


# ---- the descriptor emitter -----------------------------------------------------------------------------------------------
def test_descriptors_made_up(emu_ctx):
    pc.check_descriptors(emu_ctx, MEM, pc.descriptor_case())


def test_descriptor_text_by_hand():
    c = pc.descriptor_case()
    lines = pc.descriptor_text(c)
    flags = [l.split(b"\t")[1] for l in lines[:4]]
    assert flags == [b"83", b"99", b"147", b"163"]
    tl = {l.split(b"\t")[8] for l in lines}
    assert {b"-2147483647", b"-1", b"0", b"1", b"2147483647"} <= tl
    assert {len(l.split(b"\t")[7]) for l in lines} >= {1, 10}


def test_sixteen_byte_windows_cut_the_mate_fields():
    """windows of 16 bytes over the made-up descriptors' text: one starts on the "=" of RNEXT, one on the "-" of a TLEN, and
    one inside the digits of a PNEXT or a TLEN"""
    c = pc.descriptor_case()
    assert 16 in c["windows"]
    on_eq = on_minus = in_number = 0
    at = 0
    for line in pc.descriptor_text(c):
        f = line.split(b"\t")
        rnext = at + sum(len(x) + 1 for x in f[:6])
        pnext = rnext + 2
        tlen = pnext + len(f[7]) + 1
        for cut in range(-(-at // 16) * 16, at + len(line), 16):
            on_eq += cut == rnext
            on_minus += cut == tlen and f[8].startswith(b"-")
            in_number += pnext < cut < pnext + len(f[7]) or tlen < cut < tlen + len(f[8])
        at += len(line)
    assert on_eq and on_minus and in_number, (on_eq, on_minus, in_number)


# ---- the same bytes from call to call ---------------------------------------------------------------------------------------
def test_second_call_and_fresh_context(emu_ctx, indexes):
    c = pc.pair_case(("two-records-flipped/k1", "overlap", 0, 500))
    idx = indexes(c["fasta"])
    first = idx.map_pairs(c["fastq1"], c["fastq2"], c["k"], c["lo"], c["hi"])
    assert idx.map_pairs(c["fastq1"], c["fastq2"], c["k"], c["lo"], c["hi"]) == first == c["want"]
    fresh = api.Context(0, lib_path=EMU_LIB)
    try:
        fresh.set_small_direct_max(0)
        with api.Index.from_fasta(c["fasta"], ctx=fresh) as other:
            assert other.map_pairs(c["fastq1"], c["fastq2"], c["k"], c["lo"], c["hi"]) == first
    finally:
        fresh.close()
