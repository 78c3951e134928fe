"""Paired-end reads (sx_index_map_pairs, sx_sam_layout_dev_pairs / sx_sam_emit_dev_pairs): the contract
restated over parsed SAM lines, the second images and the expected texts composed from the both-strands texts that the
fixtures determine (strand_cases, best_cases, hamming_cases: no new run of the reference), and the cases that the CPU-harness
suite (tests/test_pairs_cpu.py) and the GPU suite (tests/test_gpu_pairs.py) share.  `mem` is one of the two objects of
tests/device_memory.py.  TEST INFRASTRUCTURE ONLY."""
import hashlib
import re

import numpy as np

import best_cases as bc
import hamming_cases as hc
import sam_kernel_cases as skc
import strand_cases as sc
from stralg_amd import _lib, api


# ---- the contract, restated -----------------------------------------------------------------------------------------------
def span_of(cigar):
    """the M and D lengths of a CIGAR: the symbols of the reference that the line covers"""
    return sum(int(n) for n, op in re.findall(rb"(\d+)([MID])", cigar) if op in b"MD")


def _parsed(lines):
    out = []
    for line in lines:
        f = line.split(b"\t")
        out.append((f, int(f[1]), f[2], int(f[3]), span_of(f[5])))
    return out


def _mate_line(f, flag, pnext, tlen):
    return b"\t".join(f[:1] + [b"%d" % flag] + f[2:6] + [b"=", b"%d" % pnext, b"%d" % tlen] + f[9:]) + b"\n"


def pair_text(lines1, lines2, lo, hi):
    """the text of one pair: for a over lines1 (the both-strands lines of mate 1) and b over lines2 (of mate 2), both in order,
    a's line and then b's line of every proper (a, b)"""
    out = []
    second = _parsed(lines2)
    for fa, flag_a, rname_a, pos_a, span_a in _parsed(lines1):
        for fb, flag_b, rname_b, pos_b, span_b in second:
            if rname_a != rname_b or {flag_a, flag_b} != {0, 16}:
                continue
            a_forward = flag_a == 0
            pos_f, span_f, pos_r, span_r = (pos_a, span_a, pos_b, span_b) if a_forward else (pos_b, span_b, pos_a, span_a)
            t = pos_r + span_r - pos_f
            if not (pos_f <= pos_r and pos_f + span_f <= pos_r + span_r and lo <= t <= hi):
                continue
            out.append(_mate_line(fa, 1 + 2 + 64 + (32 if a_forward else 16), pos_b, t if a_forward else -t))
            out.append(_mate_line(fb, 1 + 2 + 128 + (16 if a_forward else 32), pos_a, -t if a_forward else t))
    return b"".join(out)


def lines_of_rc(lines):
    """the both-strands lines of rc(read) from those of the read: its FLAG-16 group first, with FLAG 0, then its FLAG-0 group
    with FLAG 16 (SEQ and QUAL of a FLAG-16 line are rc(read)'s own: the forward orientation)"""
    fwd = [l for l in lines if l.split(b"\t", 2)[1] == b"0"]
    rev = [l for l in lines if l.split(b"\t", 2)[1] == b"16"]
    assert lines == fwd + rev
    return [sc.with_flag(l, b"0") for l in rev] + [sc.with_flag(l, b"16") for l in fwd]


# ---- the second image: a selection of the recorded reads, reverse complemented -------------------------------------------------
def _first_forward(lines):
    for l in lines:
        f = l.split(b"\t")
        if f[1] == b"0":
            return f[2], int(f[3])
    return None


def partners(pairing, reads, by_name):
    """q[p]: mate 2 of pair p is rc(read q[p])"""
    n = len(reads)
    if pairing == "overlap":
        return list(range(n))
    if pairing == "next":
        return [(p + 1) % n for p in range(n)]
    assert pairing == "downstream"
    first = [_first_forward(by_name.get(r[0], [])) for r in reads]
    out = []
    for p in range(n):
        behind = [(first[q][1], q) for q in range(n) if q != p and first[p] and first[q] and first[q][0] == first[p][0] and first[q][1] >= first[p][1]]
        out.append(min(behind)[1] if behind else p)
    return out


def paired(fastq, both_text, pairing, lo, hi):
    """(image 2, the expected text, pairs with lines) of image 1 = fastq, whose both-strands text is both_text"""
    reads = sc.fastq_reads(fastq)
    by_name = sc.lines_of(both_text)
    q = partners(pairing, reads, by_name)
    texts = [pair_text(by_name.get(reads[p][0], []), lines_of_rc(by_name.get(reads[q[p]][0], [])), lo, hi) for p in range(len(reads))]
    return sc.fastq_image([sc.rc(reads[j]) for j in q]), b"".join(texts), sum(1 for t in texts if t)


# ---- the cases ----------------------------------------------------------------------------------------------------------------
# (fixture, pairing, min_insert, max_insert) -> lines (and pairs with lines, where that was recorded): the counts of a
# prototype of this oracle, asserted so that no case passes on an empty text
COUNTS = {
    ("test-out/k0", "overlap", 0, 500): (12, 3),
    ("test-out/k1", "overlap", 0, 500): (658, 3),
    ("test-out/k1", "next", 0, 500): (152, None),
    ("test-out/k2", "overlap", 0, 500): (11398, None),
    ("two-records-flipped/k1", "overlap", 0, 500): (3380, 191),
    ("two-records-flipped/k1", "overlap", 30, 3000): (2332, 140),
    ("two-records-flipped/k1", "next", 0, 2 ** 31): (14, None),
    ("two-records-flipped/k2", "overlap", 30, 3000): (2164872, None),
    ("hg38/reads-100-10-0/k0", "overlap", 0, 500): (14792, None),
    ("hg38/reads-100-10-0/k0", "next", 30, 3000): (28, None),
}
BIG = ("two-records-flipped/k2", "overlap", 30, 3000)  # 2.1 M lines: by length and SHA-256, on the GPU only
CASES = list(COUNTS)
SMALL_CASES = [c for c in CASES if c != BIG]
GRID = ("two-records-flipped/k1", "overlap", 30, 3000)  # the case of the batch and window grid and of the index forms


def case_id(c):
    return "%s/%s/%d-%d" % c


_memo = {}


def pair_case(key):
    """dict(fasta, fastq1, fastq2, k, lo, hi, want, pairs) of a case of COUNTS (computed once a process)"""
    if key not in _memo:
        name, pairing, lo, hi = key
        if "strands" not in _memo:
            _memo["strands"] = sc.strand_cases()
        c = _memo["strands"][name]
        fastq2, want, pairs = paired(c["fastq"], c["want"], pairing, lo, hi)
        _memo[key] = dict(fasta=c["fasta"], fastq1=c["fastq"], fastq2=fastq2, k=c["k"], lo=lo, hi=hi, want=want, pairs=pairs)
    return _memo[key]


def check_text(got, want):
    assert len(got) == len(want), (len(got), len(want), skc.first_difference(got, want))
    assert got == want, skc.first_difference(got, want)


def check_digest(got, want):
    assert len(got) == len(want) and got.count(b"\n") == want.count(b"\n")
    assert hashlib.sha256(got).digest() == hashlib.sha256(want).digest()


def flagged_case(name, k, best, indels, pairing="overlap", lo=0, hi=500):
    """a case of best_cases() with best and / or indels=False: the oracle over the both-strands text those modules compose"""
    if "best" not in _memo:
        _memo["best"] = bc.best_cases()
    c = _memo["best"][name]
    both = bc.want_of(c, k, True) if best and indels else bc.plain_of(c, k, True) if indels else hc.want_of(c, k, True, best)
    fastq2, want, pairs = paired(c["fastq"], both, pairing, lo, hi)
    return dict(fasta=c["fasta"], fastq1=c["fastq"], fastq2=fastq2, k=k, lo=lo, hi=hi, want=want, pairs=pairs)


def no_indels_case(name, pairing, lo, hi):
    """indels=False (best off) on a fixture of strand_cases(): the oracle over the lines of its recorded both-strands text whose
    CIGAR is pure M (hamming_cases.pure_text)"""
    if "strands" not in _memo:
        _memo["strands"] = sc.strand_cases()
    c = _memo["strands"][name]
    fastq2, want, pairs = paired(c["fastq"], hc.pure_text(c["want"]), pairing, lo, hi)
    return dict(fasta=c["fasta"], fastq1=c["fastq"], fastq2=fastq2, k=c["k"], lo=lo, hi=hi, want=want, pairs=pairs)


def batch_lines(key):
    """the lines of a batch of every pair of an overlap case: the both-strands lines of its reads, twice (mate 2 of pair p is
    rc(read p), which has as many)"""
    assert key[1] == "overlap"
    c = pair_case(key)
    by_name = sc.lines_of(_memo["strands"][key[0]]["want"])
    return 2 * sum(len(by_name.get(r[0], [])) for r in sc.fastq_reads(c["fastq1"]))


def run(ctx, idx, c, window=0, batch=0, room=0, pairs_room=0, **flags):
    """the chunks of idx.map_pairs on case c with the context's switches set (batch counts pairs)"""
    chunks = []
    ctx.set_sam_window_bytes(window)
    ctx.set_sam_batch_reads(batch)
    ctx.set_sam_room_hits(room)
    ctx.set_pairs_room_lines(pairs_room)
    try:
        idx.map_pairs(c["fastq1"], c["fastq2"], c["k"], min_insert=c["lo"], max_insert=c["hi"], sink=chunks.append, **flags)
    finally:
        ctx.set_sam_window_bytes(0)
        ctx.set_sam_batch_reads(0)
        ctx.set_sam_room_hits(0)
        ctx.set_pairs_room_lines(0)
    return chunks


def check_pairs_room(ctx, idx, key, pairs_room, batch=0):
    """a room for lines and descriptors alone (the hits' room stays by the free memory: no hit stage grows or halves): the
    batches of several pairs that exceed it are halved by the join, the text is unchanged"""
    c = pair_case(key)
    check_text(b"".join(run(ctx, idx, c, batch=batch, pairs_room=pairs_room)), c["want"])
    st = ctx.map_stats()
    assert st["room_grown"] == st["lone_grown"] == 0 and st["halved"] >= 1 and st["retries"] == st["halved"], st
    assert st["batch_final"] < st["batch_first"] and st["batch_final"] % 4 == 0, st
    return c, st


def raw_call(ctx, idx, fastq1, fastq2, k, lo, hi, flags):
    """(return code, bytes that reached the sink) of sx_index_map_pairs itself"""
    import ctypes as C
    seen = []

    def sink(user, section, data, n):
        seen.append(C.string_at(data, n))
        return 0

    b1, b2 = np.frombuffer(fastq1, np.uint8), np.frombuffer(fastq2, np.uint8)
    opts = _lib.PairOpts(lo, hi)
    rc = ctx.lib.sx_index_map_pairs(ctx.h, idx._handle(), b1.ctypes.data if b1.size else None, b1.size, b2.ctypes.data if b2.size else None,
                                    b2.size, k, C.byref(opts), flags, _lib.SINK_FN(sink), None)
    return rc, b"".join(seen)


# ---- sx_sam_layout_dev_pairs / sx_sam_emit_dev_pairs over made-up descriptors ------------------------------------------------
def descriptor_case():
    """hits of skc's several-records case under made-up descriptors: FLAGs 83, 99, 147 and 163 on neighbouring lines, TLEN at
    both ends of its range and around 0, PNEXT and POS of 1 and 10 digits; windows of 16 bytes cut "=", a "-" and numbers"""
    c = dict(skc.several_records_case())
    n = len(c["rows"])
    tl = [-2147483647, -1, 0, 1, 2147483647, -30, 250, -2147483647]
    lines = [(j % n, [1, 4294967295, 77, 1000000000][j % 4], [4294967295, 1, 123456, 9][j % 4], tl[j % len(tl)], [83, 99, 147, 163][j % 4])
             for j in range(3 * n + 5)]
    c["lines"] = lines
    c["windows"] = [16, 100, 4099]
    return c


def descriptor_text(case):
    sas, rnames = skc._as_lists(case["sa"], case["rnames"])
    out = []
    for h, pos, pnext, tlen, flag in case["lines"]:
        q, L, R, gaps = case["rows"][h]
        read, rec = q // len(rnames), q % len(rnames)
        cigar = api.approx_cigar(len(case["seqs"][read]), gaps).encode()
        out.append(b"\t".join([case["names"][read], b"%d" % flag, rnames[rec], b"%d" % pos, b"0", cigar, b"=", b"%d" % pnext, b"%d" % tlen,
                               case["seqs"][read], case["quals"][read]]) + b"\n")
    return out


def check_descriptors(ctx, mem, case):
    """offsets, total and text against the Python rendering, whole and window by window; a descriptor whose hit lies outside
    the batch is refused"""
    want_lines = descriptor_text(case)
    want = b"".join(want_lines)
    b = skc.batch_of(ctx, mem, case)
    lines = np.array(case["lines"], dtype=np.int64)
    rec = np.zeros(len(lines), dtype=_lib.PAIR_LINE_DTYPE)
    for k, f in enumerate(("hit", "pos", "pnext", "tlen", "flag")):
        rec[f] = lines[:, k]
    n = len(lines)
    d_lines = mem.to_dev(rec.view(np.uint8))
    d_off = mem.zeros(n + 1, np.uint64)
    mem.fill(d_off, 0xEE)
    mem.sync()
    total = ctx.sam_layout_dev_pairs(b.batch, d_lines, n, d_off)
    off = mem.to_host(d_off, np.uint64)
    assert total == len(want)
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(l) for l in want_lines])]).tolist()
    for window in [total] + case["windows"]:
        d_out = mem.zeros(window + 16)
        got = []
        for lo in range(0, total, window):
            hi = min(total, lo + window)
            mem.fill(d_out, 0xEE)
            mem.sync()
            ctx.sam_emit_dev_pairs(b.batch, d_lines, n, d_off, total, lo, hi, d_out)
            chunk = mem.to_host(d_out)
            assert (chunk[hi - lo:] == 0xEE).all(), (window, lo)
            got.append(chunk[:hi - lo].tobytes())
        assert b"".join(got) == want, (window, skc.first_difference(b"".join(got), want))
    rec["hit"][n // 2] = len(case["rows"])
    d_bad = mem.to_dev(rec.view(np.uint8))
    mem.sync()
    try:
        ctx.sam_layout_dev_pairs(b.batch, d_bad, n, d_off)
    except api.StralgAmdError as e:
        assert "code -1" in str(e)
    else:
        raise AssertionError("a descriptor outside the batch was accepted")
