"""Made-up hits for sx_sam_layout_dev / sx_sam_emit_dev (sx_sam.hip), shared by the CPU-harness suite
(tests/test_sam_cpu.py) and the GPU suite (tests/test_gpu_sam_kernels.py).  The expected text is formatted in Python from
the hit rows and the input lists (expected_text), the expected offsets are a numpy cumulative sum of the expected line
lengths (expected_offsets); no device result feeds either.  `mem` is one of the two objects of tests/device_memory.py.
TEST INFRASTRUCTURE ONLY."""
import itertools

import numpy as np
import pytest

from stralg_amd import _lib, api

FRONT = 48  # guard bytes in front of a window (a multiple of 16: the window itself stays 16-byte aligned)
BEHIND = 48


def flat(items):
    off = np.zeros(len(items) + 1, np.uint32)
    off[1:] = np.cumsum([len(x) for x in items])
    data = np.frombuffer(b"".join(items) + b"\0", np.uint8).copy()
    return data, off


class Batch:
    """the device copies of a batch and its layout.  sa: one suffix array (a sequence of numbers) with one record name, or
    a list of suffix arrays, one per record name (the d_sa_list form; a hit's query is read x records + record rank)"""

    def __init__(self, ctx, mem, hits, sa, names, seqs, quals, rnames):
        self.ctx, self.mem = ctx, mem
        several = len(rnames) > 1
        hits = np.ascontiguousarray(hits)
        self.n_hits = hits.size
        host = list(flat(names) + flat(seqs) + flat(quals) + flat(rnames))
        self.keep = [mem.to_dev(hits)] + [mem.to_dev(a) for a in host]
        h, nm, no, sq, so, ql, qo, rn, ro = self.keep
        if several:
            arrays = [np.ascontiguousarray(s, dtype=np.uint32) for s in sa]
            d_sas = [mem.to_dev(a) for a in arrays]
            d_list = mem.to_dev(np.array([api._ptr(d) for d in d_sas], np.uint64))
            d_lens = mem.to_dev(np.array([a.size for a in arrays], np.uint64))
            self.keep += d_sas + [d_list, d_lens]
            d_sa, sa_len = None, 0
        else:
            s = np.ascontiguousarray(sa, dtype=np.uint32)
            d_sa, sa_len, d_list, d_lens = mem.to_dev(s), s.size, None, None
            self.keep.append(d_sa)
        self.batch = ctx.sam_batch(h, hits.size, d_sa, sa_len, nm, no, sq, so, ql, qo, len(names), rn, ro, len(rnames), d_list,
                                   d_lens)
        self.d_off = mem.zeros(hits.size + 1, np.uint64)
        mem.sync()
        self.total = ctx.sam_layout_dev(self.batch, self.d_off)
        self.off = mem.to_host(self.d_off, np.uint64)

    def text(self, window=None):
        """the text, window after window; every window lies between guard bytes inside a larger buffer"""
        mem = self.mem
        window = window or max(self.total, 1)
        room = (min(window, max(self.total, 1)) + 15) // 16 * 16
        buf = mem.zeros(FRONT + room + BEHIND)
        out = []
        for lo in range(0, self.total, window):
            hi = min(self.total, lo + window)
            mem.fill(buf, 0xEE)
            mem.sync()
            self.ctx.sam_emit_dev(self.batch, self.d_off, self.total, lo, hi, buf[FRONT:])
            got = mem.to_host(buf)
            assert (got[:FRONT] == 0xEE).all(), "bytes in front of the window were written"
            assert (got[FRONT + hi - lo:] == 0xEE).all(), "bytes behind the window were written"
            out.append(got[FRONT:FRONT + hi - lo].tobytes())
        return b"".join(out)


def make_hits(rows):
    """rows: (query, L, R, gaps)"""
    hits = np.zeros(len(rows), dtype=_lib.APPROX_HIT_DTYPE)
    if rows:
        hits["query"], hits["L"], hits["R"] = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
    for k, (q, L, R, gaps) in enumerate(rows):
        if gaps:
            hits[k]["n_gaps"] = len(gaps)
            hits[k]["gap"][:len(gaps)] = gaps
    return hits


def gap_patterns(m, max_gaps):
    """every edit string over M / I / D of a pattern of m symbols with at most max_gaps I / D: its gap[] list"""
    out = []
    for n_i in range(max_gaps + 1):
        for n_d in range(max_gaps + 1 - n_i):
            length = m + n_d
            for where in itertools.combinations(range(length), n_i + n_d):
                for d_set in itertools.combinations(where, n_d):
                    out.append([w | (_lib.APPROX_GAP_D if w in d_set else 0) for w in where])
    return out


def _as_lists(sa, rnames):
    """(list of suffix arrays, list of record names) of either form of a batch's suffix arrays"""
    if isinstance(rnames, bytes):
        return [sa], [rnames]
    return (list(sa), list(rnames)) if len(rnames) > 1 else ([sa], list(rnames))


def expected_text(sa, rows, names, seqs, quals, rnames):
    """the lines of the hit rows, formatted here: query = read x records + record rank, positions sa[L .. R) + 1 of that
    record's suffix array, the CIGAR from api.approx_cigar (pure Python)"""
    sas, rnames = _as_lists(sa, rnames)
    out, cigars = [], {}
    for q, L, R, g in rows:
        read, rec = divmod(q, len(rnames))
        key = (len(seqs[read]), tuple(g))
        if key not in cigars:
            cigars[key] = api.approx_cigar(len(seqs[read]), g).encode()
        for i in range(L, R):
            out.append(b"%s\t0\t%s\t%d\t0\t%s\t*\t0\t0\t%s\t%s\n" % (names[read], rnames[rec], int(sas[rec][i]) + 1, cigars[key],
                                                                 seqs[read], quals[read]))
    return b"".join(out)


def expected_offsets(sa, rows, names, seqs, quals, rnames):
    """every hit's first byte and the total (n_hits + 1 entries): a cumulative sum of the expected line lengths -- per
    line its fields, CIGAR, 16 bytes of tabs, zeros, '*' and newline, and the decimal digits of its position"""
    sas, rnames = _as_lists(sa, rnames)
    digit_sums = []
    for s in sas:
        p1 = np.asarray(s, dtype=np.int64) + 1
        digits = 1 + sum((p1 >= 10 ** k).astype(np.int64) for k in range(1, 11))
        digit_sums.append(np.concatenate([[0], np.cumsum(digits)]))
    cigars = {}
    lengths = np.zeros(len(rows) + 1, np.int64)
    for h, (q, L, R, g) in enumerate(rows):
        read, rec = divmod(q, len(rnames))
        key = (len(seqs[read]), tuple(g))
        if key not in cigars:
            cigars[key] = len(api.approx_cigar(len(seqs[read]), g))
        fixed = len(names[read]) + len(rnames[rec]) + cigars[key] + len(seqs[read]) + len(quals[read]) + 16
        lengths[h + 1] = (R - L) * fixed + digit_sums[rec][R] - digit_sums[rec][L]
    return np.cumsum(lengths).astype(np.uint64)


# ---- the CIGAR of every edit string ------------------------------------------------------------------------------------------
def cigar_case():
    """every CIGAR of a 6-symbol pattern with up to 3 gaps, and 40 of a 300-symbol pattern with 8"""
    rng = np.random.default_rng(8)
    gaps6 = gap_patterns(6, 3)
    rows = [(0, 0, 1, g) for g in gaps6]
    want = [api.approx_cigar(6, g) for g in gaps6]
    long_m = 300
    for _ in range(40):  # k = 8
        n_d = int(rng.integers(0, 9))
        where = sorted(rng.choice(long_m + n_d, 8, replace=False).tolist())
        if _ % 4 == 0:  # (runs of adjacent operations)
            where = list(range(where[0] % 200, where[0] % 200 + 8))
        d_set = set(rng.choice(where, n_d, replace=False).tolist())
        g = [w | (_lib.APPROX_GAP_D if w in d_set else 0) for w in where]
        rows.append((1, 0, 1, g))
        want.append(api.approx_cigar(long_m, g))
    return dict(rows=rows, want=want, sa=[41], names=[b"six", b"long"], seqs=[b"ACGTAC", b"A" * long_m],
                quals=[b"~" * 6, b"!" * long_m], rnames=[b"rec"])


def check_cigars(ctx, mem, case):
    rows, want = case["rows"], case["want"]
    b = Batch(ctx, mem, make_hits(rows), case["sa"], case["names"], case["seqs"], case["quals"], case["rnames"])
    lines = b.text().split(b"\n")[:-1]
    assert len(lines) == len(rows)
    for line, cigar, row in zip(lines, want, rows):
        f = line.split(b"\t")
        assert f[5].decode() == cigar, row
        assert f[0] == (b"six", b"long")[row[0]] and f[2] == b"rec" and f[3] == b"42"
        assert line == b"\t".join([f[0], b"0", b"rec", b"42", b"0", cigar.encode(), b"*", b"0", b"0", f[9], f[10]])
    assert sum(len(l) + 1 for l in lines) == b.total
    assert b.off[-1] == b.total and (np.diff(b.off.astype(np.int64)) == [len(l) + 1 for l in lines]).all()


# ---- positions of 1 to 10 digits; the small batch for the windows ------------------------------------------------------------
POSITIONS = [1, 9, 10, 99_999, 100_000, 2 ** 32 - 1]
WINDOWS = [1, 15, 16, 17, 255, 256, 257]


def digit_case():
    sa = [p - 1 for p in POSITIONS] + [7] * 70 + [123456]
    rows = [(1, 0, 6, []), (0, 2, 4, [2]), (1, 6, 77, [1 | _lib.APPROX_GAP_D])]  # (the last: a long interval)
    return dict(name="digits", rows=rows, sa=sa, names=[b"a b", b"r1"], seqs=[b"ACG", b"TT"], quals=[b"III", b"##"], rnames=[b"chr"])


def batch_of(ctx, mem, case):
    return Batch(ctx, mem, make_hits(case["rows"]), case["sa"], case["names"], case["seqs"], case["quals"], case["rnames"])


def text_of(case):
    return expected_text(case["sa"], case["rows"], case["names"], case["seqs"], case["quals"], case["rnames"])


def check_position_digits(ctx, mem, case):
    b = batch_of(ctx, mem, case)
    want = expected_text(case["sa"], case["rows"], [b"a b", b"r1"], [b"ACG", b"TT"], [b"III", b"##"], b"chr")
    got = b.text()
    assert got == want
    assert [l.split(b"\t")[3] for l in got.split(b"\n")[:6]] == [str(p).encode() for p in POSITIONS]
    assert b.total == len(want)


def check_window(ctx, mem, case, window):
    """the windows' concatenation is the one-window text, and both are the expected text"""
    b = batch_of(ctx, mem, case)
    whole = b.text()
    assert b.text(window) == whole
    assert whole == text_of(case)


# ---- hits that the layout refuses, and the empty batch ------------------------------------------------------------------------
def refused_cases():
    """a query, an interval's end and an interval's order outside the batch; with several records, an interval that
    exceeds its own record's suffix array but not another's.  hit_info answers before it reads what such a hit points
    to; emit is never called on these."""
    one = dict(sa=[1, 2, 3], names=[b"a", b"b"], seqs=[b"A", b"C"], quals=[b"!", b"!"], rnames=[b"r"])
    out = [dict(one, name="refused-%d" % k, rows=[row]) for k, row in enumerate([(2, 0, 1, []), (0, 0, 9, []), (0, 3, 2, [])])]
    three = dict(sa=[list(range(5)), list(range(50)), list(range(20))], names=[b"a", b"b"], seqs=[b"A", b"C"], quals=[b"!", b"!"],
                 rnames=[b"r0", b"r1", b"r2"])
    out.append(dict(three, name="refused-other-records-length", rows=[(1, 0, 4, []), (3 * 1 + 0, 2, 10, [])]))
    out.append(dict(three, name="refused-query-of-three-records", rows=[(6, 0, 1, [])]))
    return out


def check_refused(ctx, mem, case):
    with pytest.raises(api.StralgAmdError) as e:
        batch_of(ctx, mem, case)
    assert "code -1" in str(e.value)


def empty_case():
    return dict(name="empty", rows=[], sa=[0], names=[b"a"], seqs=[b"A"], quals=[b"!"], rnames=[b"r"])


def check_empty(ctx, mem, case):
    b = batch_of(ctx, mem, case)
    assert b.total == 0 and b.text() == b""


# ---- the layout's and the emit's thresholds ------------------------------------------------------------------------------------
BIG_WINDOWS = [4099, 16383, 16384, 16385, 16400]
INTERVALS = [1, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025, 2049, 5000]


def mixed_sa(rng, n):
    """suffix-array values whose positions have 1 to 10 digits in no order"""
    d = rng.integers(1, 10, n)
    sa = (rng.random(n) * (10.0 ** d - 10.0 ** (d - 1)) + 10.0 ** (d - 1)).astype(np.int64) - 1
    sa[rng.integers(0, n, n // 50)] = 2 ** 32 - 2
    sa[rng.integers(0, n, n // 50)] = 0
    return sa.astype(np.uint32)


def threshold_case():
    """interval lengths around the size pass's inline limit (32), the emit's step (256 lines) and its walk's step (1024
    lines), several long ones in one workgroup of the size pass, short ones before, between and behind them"""
    rng = np.random.default_rng(21)
    sa = mixed_sa(rng, 6000)
    gaps = [[], [1], [2 | _lib.APPROX_GAP_D], [0, 1]]
    rows = []
    for k, n in enumerate([1, 31] + INTERVALS + [33, 2049, 1, 1024, 31, 5000, 2]):
        L = int(rng.integers(0, sa.size - n + 1))
        rows.append((k % 2, L, L + n, gaps[k % 4]))
    return dict(name="thresholds", rows=rows, sa=sa, names=[b"q0", b"read1"], seqs=[b"ACG", b"TTGA"], quals=[b"III", b"#!#!"],
                rnames=[b"c"], windows=BIG_WINDOWS)


def empty_interval_cases():
    """hits with L == R (no lines): single ones and runs of 255, 256, 257 and 600 in front of, between and behind real
    hits; a batch of nothing else"""
    rng = np.random.default_rng(22)
    sa = mixed_sa(rng, 700)
    base = dict(sa=sa, names=[b"e", b"name two"], seqs=[b"AC", b"GGT"], quals=[b"II", b"###"], rnames=[b"rec"])
    out = []
    for run in (1, 255, 256, 257, 600):
        rows = []
        for k, real in enumerate((3, 300, 1, 40)):
            at = int(rng.integers(0, sa.size))
            rows += [(k % 2, at, at, [])] * run
            L = int(rng.integers(0, sa.size - real))
            rows.append(((k + 1) % 2, L, L + real, [1] if k == 2 else []))
        rows += [(0, sa.size, sa.size, [])] * run  # (behind the last real hit; L == R == the suffix array's length)
        out.append(dict(base, name="empty-runs-%d" % run, rows=rows, windows=[100, 4099]))
    out.append(dict(base, name="only-empty-intervals", rows=[(1, 5, 5, [])] * 300))
    return out


def long_field_cases():
    """a read with the longest name, sequence and quality the FASTQ contract allows and a record name of 300 bytes
    (lines of about 6.4 KB); a pattern of 30 000 symbols with eight gaps far apart: nine M runs, one of five digits"""
    rng = np.random.default_rng(23)
    sa = mixed_sa(rng, 64)
    letters = np.frombuffer(b"ACGT", np.uint8)
    names = [b"N" * 2045, b"s"]
    seqs = [letters[rng.integers(0, 4, 2046)].tobytes(), b"ACGT"]
    quals = [(33 + rng.integers(0, 90, 2046)).astype(np.uint8).tobytes(), b"!~!~"]
    rows = [(1, 0, 2, []), (0, 3, 10, []), (1, 9, 10, [2]), (0, 20, 33, [5 | _lib.APPROX_GAP_D, 2000]), (1, 0, 1, [])]
    out = [dict(name="longest-fastq-fields", rows=rows, sa=sa, names=names, seqs=seqs, quals=quals, rnames=[b"R" * 300],
                windows=[4099, 16384])]
    m = 30_000
    where = [700, 11_000, 12_500, 15_000, 19_999, 23_000, 26_000, 29_990]
    gaps = [w | (_lib.APPROX_GAP_D if k % 3 == 0 else 0) for k, w in enumerate(where)]
    assert len(api.approx_cigar(m, gaps)) > 50
    out.append(dict(name="pattern-of-30000", rows=[(0, 1, 4, gaps), (1, 0, 2, []), (0, 7, 8, gaps[:3])], sa=sa, names=[b"long", b"s"],
                    seqs=[letters[rng.integers(0, 4, m)].tobytes(), b"AC"], quals=[b"J" * m, b"!!"], rnames=[b"chrL"],
                    windows=[16385]))
    return out


def several_records_case():
    """three records with a suffix array each, of different lengths; query = read x 3 + record rank"""
    rng = np.random.default_rng(24)
    sas = [mixed_sa(rng, 40), mixed_sa(rng, 900), mixed_sa(rng, 7)]
    rows = []
    for read in range(4):
        for rec in range(3):
            n = sas[rec].size
            for _ in range(int(rng.integers(0, 3))):
                L = int(rng.integers(0, n))
                R = int(rng.integers(L, n + 1))
                rows.append((read * 3 + rec, L, R, [1] if read == 2 else []))
    rows.append((3 * 3 + 1, 0, 900, []))  # (a whole suffix array, longer than the other records' ones)
    rows.append((0 * 3 + 2, 0, 7, []))
    return dict(name="three-records", rows=rows, sa=sas, names=[b"r0", b"r1 x", b"r2", b"r3"], seqs=[b"ACGT", b"A", b"GATTACA", b"TT"],
                quals=[b"IIII", b"#", b"1234567", b"~~"], rnames=[b"first", b"2", b"the third"], windows=[17, 4099])


def scan_edge_cases():
    """hit counts around the 64-bit scan's tile (2048 entries) and its spine's second round (from 257 tiles on): one line a
    hit.  At the largest count only offsets and total are checked."""
    rng = np.random.default_rng(25)
    sa = mixed_sa(rng, 5000)
    out = []
    for n in (2047, 2048, 2049, 2048 * 256 + 1):
        L = rng.integers(0, sa.size, n)
        q = rng.integers(0, 2, n)
        rows = [(int(q[k]), int(L[k]), int(L[k]) + 1, []) for k in range(n)]
        out.append(dict(name="scan-%d-hits" % n, rows=rows, sa=sa, names=[b"a", b"bc"], seqs=[b"A", b"CG"], quals=[b"!", b"##"],
                        rnames=[b"r"], offsets_only=n > 4096))
    return out


def text_cases():
    """the cases of check_text, by name"""
    cases = [threshold_case()] + empty_interval_cases() + long_field_cases() + [several_records_case()] + scan_edge_cases()
    return {c["name"]: c for c in cases}


TEXT_CASE_NAMES = ["thresholds", "empty-runs-1", "empty-runs-255", "empty-runs-256", "empty-runs-257", "empty-runs-600",
                   "only-empty-intervals", "longest-fastq-fields", "pattern-of-30000", "three-records", "scan-2047-hits",
                   "scan-2048-hits", "scan-2049-hits", "scan-524289-hits"]


def check_text(ctx, mem, case):
    """offsets and total against expected_offsets; the one-window text and every window size's concatenation against
    expected_text"""
    b = batch_of(ctx, mem, case)
    args = (case["sa"], case["rows"], case["names"], case["seqs"], case["quals"], case["rnames"])
    want_off = expected_offsets(*args)
    assert b.off.size == want_off.size and b.total == int(want_off[-1]), (case["name"], b.total, int(want_off[-1]))
    wrong = np.flatnonzero(b.off != want_off)
    assert wrong.size == 0, (case["name"], "first wrong offset at hit", int(wrong[0]))
    if case.get("offsets_only"):
        return
    want = expected_text(*args)
    assert len(want) == b.total
    got = b.text()
    assert len(got) == len(want) and got == want, (case["name"], "one window", first_difference(got, want))
    for window in case.get("windows", ()):
        got = b.text(window)
        assert len(got) == len(want) and got == want, (case["name"], window, first_difference(got, want))


def first_difference(a, b):
    n = min(len(a), len(b))
    x, y = np.frombuffer(a[:n], np.uint8), np.frombuffer(b[:n], np.uint8)
    d = np.flatnonzero(x != y)
    return int(d[0]) if d.size else n
