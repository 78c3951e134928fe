"""The SAM text of search hits (sx_sam.hip) and the mapper's loop (sx_map_reads_stream) through the CPU execution
harness, against the reference read mapper's stdout in tests/golden/golden_sam.npz.

The harness builds the kernels with a slice of 256 bytes a workgroup (SX_SAM_SLICE_BYTES in the Makefile's EMUGRIDS), so
lines straddle slices in every case here; windows are set per test (SX_FLAG_SAM_WINDOW_BYTES).

The 24 MB case (reads-100-10-0.fq, 2 edits) is not run whole here: its first reads are, and their lines are compared with
the fixture's first 200 lines.  tests/test_gpu_sam.py checks that case by its SHA-256."""
import itertools

import numpy as np
import pytest

import approx_model
from approx_cases import remapped
from sam_cases import check_case, sam_cases, subset_fastq
from stralg_amd import _lib, api


@pytest.fixture(scope="module")
def cases():
    return sam_cases()


_TABLES = {}


def records_of(ctx, fasta):
    """[(name, BwtTable)] in the mapper's list order (the file's), tables from the oracle's restatement"""
    if fasta not in _TABLES:
        recs = []
        for name, seq in ctx.fasta_records(fasta):
            sym, sigma = remapped(seq)
            sa, c, o, ro = approx_model.tables(sym, sigma)
            t = api.BwtTable(api.alloc_remap_table(seq), api.SuffixArray(None, sa), c, o, ro)
            recs.append((name, t))
        _TABLES[fasta] = recs
    return _TABLES[fasta]


def run(ctx, fasta, fastq, k, window=0, batch=0):
    chunks = []
    ctx.set_sam_window_bytes(window)
    ctx.set_sam_batch_reads(batch)
    try:
        ctx.map_reads_stream(records_of(ctx, fasta), fastq, k, chunks.append)
    finally:
        ctx.set_sam_window_bytes(0)
        ctx.set_sam_batch_reads(0)
    return chunks


@pytest.mark.parametrize("name", ["test-out/k0", "test-out/k1", "test-out/k2", "hg38/reads-100-10-0/k0",
                                  "hg38/reads-100-10-0/k1", "hg38/reads-1000-100-2/k2", "hg38/reads-1000-200-1/k1",
                                  "two-records/k1"])
def test_fixture_cases_whole_text(emu_ctx, cases, name):
    c = cases[name]
    check_case(c, b"".join(run(emu_ctx, c["fasta"], c["fastq"], c["k"])))


def test_skewed_case_first_lines(emu_ctx, cases):
    c = cases["hg38/reads-100-10-0/k2"]
    got = b"".join(run(emu_ctx, c["fasta"], subset_fastq(c["fastq"], range(3)), c["k"]))
    lines = got.split(b"\n")[:-1]
    assert len(lines) >= 200
    assert got.startswith(c["head"])


@pytest.mark.parametrize("window", [16, 4096])
def test_windows_concatenate(emu_ctx, cases, window):
    for name in ("test-out/k1", "two-records/k1") + (("hg38/reads-100-10-0/k0",) if window > 16 else ()):
        c = cases[name]
        chunks = run(emu_ctx, c["fasta"], c["fastq"], c["k"], window=window)
        assert max(len(x) for x in chunks) <= window and len(chunks) >= len(c["sam"]) // window
        check_case(c, b"".join(chunks))


def test_small_read_batches(emu_ctx, cases):
    for name, batch in (("two-records/k1", 7), ("test-out/k2", 1), ("hg38/reads-100-10-0/k0", 33)):
        c = cases[name]
        check_case(c, b"".join(run(emu_ctx, c["fasta"], c["fastq"], c["k"], batch=batch, window=4096)))


# ---- sx_sam_layout_dev / sx_sam_emit_dev on made-up hits ------------------------------------------------------------
def aligned_bytes(n):
    raw = np.zeros(n + 32, np.uint8)
    at = (-raw.ctypes.data) % 16
    return raw[at:at + n]


def flat(items):
    off = np.zeros(len(items) + 1, np.uint32)
    off[1:] = np.cumsum([len(x) for x in items])
    data = np.frombuffer(b"".join(items) + b"\0", np.uint8).copy()
    return data, off


class Batch:
    def __init__(self, ctx, hits, sa, names, seqs, quals, rnames):
        self.ctx = ctx
        self.keep = [np.ascontiguousarray(hits), np.ascontiguousarray(sa, dtype=np.uint32)]
        self.keep += list(flat(names) + flat(seqs) + flat(quals) + flat(rnames))
        h, s, nm, no, sq, so, ql, qo, rn, ro = self.keep
        self.n_hits = h.size
        self.batch = ctx.sam_batch(h, h.size, s, s.size, nm, no, sq, so, ql, qo, len(names), rn, ro, len(rnames))
        self.off = np.zeros(h.size + 1, np.uint64)
        self.total = ctx.sam_layout_dev(self.batch, self.off)

    def text(self, window=None):
        window = window or max(self.total, 1)
        out = b""
        for lo in range(0, self.total, window):
            hi = min(self.total, lo + window)
            buf = aligned_bytes(hi - lo + 16)
            buf[:] = 0xEE
            self.ctx.sam_emit_dev(self.batch, self.off, self.total, lo, hi, buf)
            assert (buf[hi - lo:] == 0xEE).all(), "bytes behind the window were written"
            out += buf[:hi - lo].tobytes()
        return out


def make_hits(rows):
    """rows: (query, L, R, gaps)"""
    hits = np.zeros(len(rows), dtype=_lib.APPROX_HIT_DTYPE)
    for k, (q, L, R, gaps) in enumerate(rows):
        hits[k]["query"], hits[k]["L"], hits[k]["R"] = q, L, R
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


def test_cigar_on_the_device(emu_ctx):
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
    b = Batch(emu_ctx, make_hits(rows), [41], [b"six", b"long"], [b"ACGTAC", b"A" * long_m], [b"~" * 6, b"!" * long_m], [b"rec"])
    lines = b.text().split(b"\n")[:-1]
    assert len(lines) == len(rows)
    for line, cigar, row in zip(lines, want, rows):
        f = line.split(b"\t")
        assert f[5].decode() == cigar, row
        assert f[0] == (b"six", b"long")[row[0]] and f[2] == b"rec" and f[3] == b"42"
        assert line == b"\t".join([f[0], b"0", b"rec", b"42", b"0", cigar.encode(), b"*", b"0", b"0", f[9], f[10]])
    assert sum(len(l) + 1 for l in lines) == b.total
    assert b.off[-1] == b.total and (np.diff(b.off.astype(np.int64)) == [len(l) + 1 for l in lines]).all()


POSITIONS = [1, 9, 10, 99_999, 100_000, 2 ** 32 - 1]


def digit_batch(ctx):
    sa = [p - 1 for p in POSITIONS] + [7] * 70 + [123456]
    rows = [(1, 0, 6, []), (0, 2, 4, [2]), (1, 6, 77, [1 | _lib.APPROX_GAP_D])]  # (the last: a long interval)
    return Batch(ctx, make_hits(rows), sa, [b"a b", b"r1"], [b"ACG", b"TT"], [b"III", b"##"], [b"chr"]), sa, rows


def expected_text(sa, rows, names, seqs, quals, rname):
    out = b""
    for q, L, R, g in rows:
        for i in range(L, R):
            out += b"%s\t0\t%s\t%d\t0\t%s\t*\t0\t0\t%s\t%s\n" % (names[q], rname, sa[i] + 1,
                                                             api.approx_cigar(len(seqs[q]), g).encode(), seqs[q], quals[q])
    return out


def test_position_digits(emu_ctx):
    b, sa, rows = digit_batch(emu_ctx)
    want = expected_text(sa, rows, [b"a b", b"r1"], [b"ACG", b"TT"], [b"III", b"##"], b"chr")
    got = b.text()
    assert got == want
    assert [l.split(b"\t")[3] for l in got.split(b"\n")[:6]] == [str(p).encode() for p in POSITIONS]
    assert b.total == len(want)


@pytest.mark.parametrize("window", [1, 15, 16, 17, 255, 256, 257])
def test_emit_window_sizes(emu_ctx, window):
    b, sa, rows = digit_batch(emu_ctx)
    assert b.text(window) == b.text()


def test_layout_rejects_hits_outside_the_batch(emu_ctx):
    for row in [(2, 0, 1, []), (0, 0, 9, []), (0, 3, 2, [])]:
        with pytest.raises(api.StralgAmdError) as e:
            Batch(emu_ctx, make_hits([row]), [1, 2, 3], [b"a", b"b"], [b"A", b"C"], [b"!", b"!"], [b"r"])
        assert "code -1" in str(e.value)


def test_empty_batch(emu_ctx):
    b = Batch(emu_ctx, make_hits([]), [0], [b"a"], [b"A"], [b"!"], [b"r"])
    assert b.total == 0 and b.text() == b""


# ---- sx_fastq_index --------------------------------------------------------------------------------------------------
def test_fastq_index_in_contract(emu_ctx):
    data = b"@r0 desc x\nCC\n+\n~~\n@r1\nAAA\n+r1 again\nIII\n@@\n@\n+\n+\n@last\tname\nNN\n\n##"
    names, no, seqs, so, quals, qo = emu_ctx.fastq_index(data)
    split = lambda d, o: [d[o[i]:o[i + 1]].tobytes() for i in range(o.size - 1)]
    assert split(names, no) == [b"r0 desc x", b"r1", b"@", b"last\tname"]
    assert split(seqs, so) == [b"CC", b"AAA", b"@", b"NN"]
    assert split(quals, qo) == [b"~~", b"III", b"+", b"##"]
    assert emu_ctx.fastq_index(data + b"\n")[0].tobytes() == names.tobytes()
    assert emu_ctx.fastq_index(b"")[1].tolist() == [0]
    longest = b"@" + b"n" * 2045 + b"\n" + b"A" * 2046 + b"\n+\n" + b"I" * 2046
    assert emu_ctx.fastq_index(longest)[3].tolist() == [0, 2046]


@pytest.mark.parametrize("data", [
    b"@" + b"n" * 2046 + b"\nA\n+\nI\n",          # a line of 2047 bytes
    b"@r\n" + b"A" * 2047 + b"\n+\n" + b"I" * 2047 + b"\n",
    b"@\nA\n+\nI\n",                               # an empty name
    b"@r\n\n+\nI\n",                               # an empty sequence
    b"@r\nA\n+\n\n",                               # an empty quality line
    b"@r\nA\n+\n",                                 # cut off before the fourth line
    b"@r\nA\n+",
    b"@r\nA\n",
    b"@r\n",
    b"@r\nA\n+\nI\n\n",                            # a blank line behind the records
    b"\n@r\nA\n+\nI\n",
    b"@r\nA\0\n+\nI\n",                            # a NUL inside a record
])
def test_fastq_index_out_of_contract(emu_ctx, data):
    with pytest.raises(api.StralgAmdError) as e:
        emu_ctx.fastq_index(data)
    assert "code -4" in str(e.value)
    with pytest.raises(api.StralgAmdError) as e:
        emu_ctx.map_reads_stream([], data, 1, lambda chunk: None)
    assert "code -4" in str(e.value)


def test_map_reads_limits(emu_ctx, cases):
    c = cases["test-out/k0"]
    for k in (-1, 9):
        with pytest.raises(api.StralgAmdError) as e:
            run(emu_ctx, c["fasta"], c["fastq"], k)
        assert "code -1" in str(e.value)
    assert run(emu_ctx, c["fasta"], b"", 1) == []

    def refuse(chunk):
        raise KeyError("sink")

    with pytest.raises(KeyError):
        emu_ctx.map_reads_stream(records_of(emu_ctx, c["fasta"]), c["fastq"], 0, refuse)
