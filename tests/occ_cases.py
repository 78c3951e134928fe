"""The cases of the compact occurrence table (sx_occ.hpp: BWT blocks with counts sampled every 64 rows) that the CPU
harness (tests/test_occ_cpu.py) and the GPU (tests/test_gpu_occ.py) run alike: records whose N = symbols + 1 falls
before, on and behind the block boundaries, over alphabets whose sigma sits on both sides of the counters' padding, and
the checks of one record.  TEST INFRASTRUCTURE ONLY.  (The library is imported inside the functions, never when the
module is.)"""
import numpy as np
import pytest

SYMBOLS = [0, 1, 62, 63, 64, 65, 127, 128, 129, 1000]  # N = symbols + 1: 1 (the sigma = 1 record), ..., 63 .. 66, 128 .. 130
LETTERS = [1, 4, 15, 16, 127]  # sigma = 2, 5, 16, 17 (the first sigma_pad of 32), 128 (the largest)
ROWS = 64


def sigma_pad(sigma):
    return (sigma + 15) // 16 * 16


def stride(sigma):
    return 4 * sigma_pad(sigma) + ROWS


def blocks(N):
    return N // ROWS + 1


def alphabet(letters):
    """`letters` distinct bytes that a FASTA sequence line may hold (no '>', no white space, no NUL)"""
    pool = [b for b in range(0x21, 0x100) if b != ord(">") and not bytes([b]).isspace()]
    assert len(pool) >= 127
    return np.array(pool[:letters], np.uint8)


def record(symbols, letters, seed=0):
    """a sequence of `symbols` bytes in which every one of `letters` letters occurs when there is room for them"""
    rng = np.random.default_rng(1000 * letters + symbols + seed)
    abc = alphabet(letters)
    seq = abc[rng.integers(0, letters, symbols)]
    first = min(symbols, letters)
    seq[rng.permutation(symbols)[:first]] = abc[:first]
    return seq.tobytes()


def record_cases():
    """[(symbols, letters, fasta bytes)]: one record a FASTA image"""
    return [(n, l, b">rec-%d-%d\n" % (n, l) + record(n, l) + b"\n") for l in LETTERS for n in SYMBOLS]


def reference_blocks(o, N, sigma):
    """the layout restated from the full table o ((N + 1, sigma)): a uint8 array (blocks, stride)"""
    nb, st, pad = blocks(N), stride(sigma), sigma_pad(sigma)
    out = np.zeros((nb, st), np.uint8)
    sym = np.full(nb * ROWS, 0xFF, np.uint8)
    sym[:N] = np.argmax(o[1:] != o[:-1], axis=1).astype(np.uint8)
    out[:, 4 * pad:] = sym.reshape(nb, ROWS)
    counters = np.zeros((nb, pad), np.uint32)
    counters[:, :sigma] = o[::ROWS][:nb]
    out[:, :4 * pad] = counters.view(np.uint8)
    return out


def check_record(ctx, Index, fasta, api, gpu=False):
    """everything the issue asks of one record: both tables expanded equal the full index's entry for entry, the blocks
    are the layout restated in numpy, the blocks built from full rows equal them byte for byte, windows of the expansion"""
    with Index.from_fasta(fasta, ctx=ctx) as full, Index.from_fasta(fasta, ctx=ctx, compact=True) as comp:
        assert comp.compact and not full.compact
        assert comp.records == full.records and len(full.records) == 1
        _, N, sigma, has_ro = full.records[0]
        assert has_ro
        want = full.device_tables(0)
        got = comp.device_tables(0)
        assert got["o"] is None and got["ro"] is None
        for f in ("string", "sa", "c"):
            assert (got[f] == want[f]).all(), f
        occ = comp.record_occ(0)
        assert (occ.compact, occ.stride, occ.sigma_pad, occ.n_blocks) == (1, stride(sigma), sigma_pad(sigma), blocks(N))
        align = 256 if gpu else 16  # (a device allocation; the harness allocates with malloc)
        assert occ.d_occ % align == 0 and occ.d_rocc % align == 0
        assert ctx.occ_compact_bytes(N, sigma) == blocks(N) * stride(sigma)
        with pytest.raises(api.StralgAmdError):
            full.device_occ(0)
        by_table = {}
        for reverse, field in ((False, "o"), (True, "ro")):
            o = comp.expand_o(0, reverse=reverse)
            assert o.shape == (N + 1, sigma) and (o == want[field]).all(), (field, N, sigma)  # (row N, column 0 and all)
            raw = comp.device_occ(0, reverse=reverse)
            assert raw.shape == (blocks(N), stride(sigma))
            assert (raw == reference_blocks(want[field], N, sigma)).all(), (field, N, sigma)
            by_table[field] = raw
            # windows: neither end on a block boundary, one row, the last row, nothing
            for lo, hi in {(min(N, 3), N + 1 - min(N, 2)), (N // 2, N // 2 + 1), (N, N + 1), (min(N, 70), min(N + 1, 131)), (1, 1)}:
                if lo <= hi:
                    assert (comp.expand_o(0, reverse=reverse, rows=(lo, hi)) == want[field][lo:hi]).all(), (field, lo, hi)
        # the same blocks from full rows (tables that arrive as tables)
        name = full.records[0][0]
        table = api.BwtTable(api.RemapTable(sigma, np.zeros(256, np.int16), None), api.SuffixArray(want["string"], want["sa"]),
                             want["c"], want["o"], want["ro"])
        with Index.from_tables([(name, table)], ctx=ctx, compact=True) as rows:
            assert rows.compact
            assert (rows.device_occ(0) == by_table["o"]).all() and (rows.device_occ(0, reverse=True) == by_table["ro"]).all()
            assert (rows.expand_o(0) == want["o"]).all()
        with pytest.raises(api.StralgAmdError):
            comp.expand_o(0, rows=(0, N + 2))
        return N, sigma


def memory_bounds(records):
    """(least, most) device_bytes of a compact index with RO over [(name, N, sigma, has_ro)]: what the issue sets"""
    least = sum(N * 5 + 2 * blocks(N) * stride(sigma) + 4 * sigma for _, N, sigma, _ in records)
    return least, least + 4096 * (5 * len(records) + 5)


def table_of(sa, c, o, ro, sigma, string=None):
    """a BwtTable over these arrays as Index.from_tables takes it"""
    from stralg_amd import api
    return api.BwtTable(api.RemapTable(sigma, np.zeros(256, np.int16), None), api.SuffixArray(string, sa), c, o, ro)


class BothForms:
    """one record's tables on the device in both forms (two indexes from the same host tables), for the search calls"""

    def __init__(self, ctx, Index, sa, c, o, ro, sigma):
        t = table_of(sa, c, o, ro, sigma)
        self.full = Index.from_tables([(b"r", t)], ctx=ctx)
        self.comp = Index.from_tables([(b"r", t)], ctx=ctx, compact=True)
        self.N, self.sigma = int(sa.size), sigma
        self.rec, self.occ = self.full.record_info(0), self.comp.record_occ(0)

    def close(self):
        self.full.close()
        self.comp.close()

    def approx(self, ctx, mem, pat, off, k, with_ro, hits_dtype):
        """the approximate search over full tables and over blocks, count then emit: [(offsets, hits)] of both"""
        count = off.size - 1
        d_pat, d_off = mem.to_dev(np.concatenate([pat, np.zeros(16, np.uint8)])), mem.to_dev(off)
        out = []
        for compact in (False, True):
            d_ho = mem.zeros(count + 1, np.uint64)
            mem.sync()
            call = ctx.bwt_approx_search_compact_dev if compact else ctx.bwt_approx_search_dev
            o, ro = (self.occ.d_occ, self.occ.d_rocc) if compact else (self.rec.d_o, self.rec.d_ro)
            args = (self.rec.d_c, o, ro if with_ro else None, self.N, self.sigma, d_pat, d_off, count, k, d_ho)
            total = call(*args)
            d_hits = mem.zeros(max(total, 1) * 32)
            mem.sync()
            assert call(*args, d_hits, total) == total
            out.append((mem.to_host(d_ho, np.uint64), mem.to_host(d_hits)[:total * 32].view(hits_dtype)))
        return out

    def exact(self, ctx, mem, pat, off):
        count = off.size - 1
        d_pat, d_off = mem.to_dev(np.concatenate([pat, np.zeros(16, np.uint8)])), mem.to_dev(off)
        out = []
        for compact in (False, True):
            d_l, d_r = mem.zeros(count, np.uint32), mem.zeros(count, np.uint32)
            mem.sync()
            call = ctx.bwt_exact_search_compact_dev if compact else ctx.bwt_exact_search_dev
            call(self.rec.d_c, self.occ.d_occ if compact else self.rec.d_o, self.N, self.sigma, d_pat, d_off, count, d_l, d_r)
            out.append((mem.to_host(d_l, np.uint32), mem.to_host(d_r, np.uint32)))
        return out


def check_searches(ctx, mem, Index, case, tables, hits_dtype, api, ks=(0, 1, 2)):
    """one case of tests/approx_cases.py: at every k the compact calls return the full-table calls' offsets and hits, byte
    for byte (so also their order); at the case's own k both give the reference iterator's stream"""
    sa, c, o, ro, sigma = tables
    both = BothForms(ctx, Index, sa, c, o, ro, sigma)
    try:
        pat, off = case["pat"], case["pat_off"]
        for k in sorted(set(ks) | {case["k"]}):
            for with_ro, mode in ((True, "ro"), (False, "noro")):
                (f_off, f_hits), (c_off, c_hits) = both.approx(ctx, mem, pat, off, k, with_ro, hits_dtype)
                assert (f_off == c_off).all() and f_hits.tobytes() == c_hits.tobytes(), (k, mode)
                if k == case["k"]:
                    assert api.approx_matches(c_hits, c_off, np.diff(off), sa) == case["streams"][mode], (k, mode)
        (f_l, f_r), (c_l, c_r) = both.exact(ctx, mem, pat, off)
        assert (f_l == c_l).all() and (f_r == c_r).all()
        assert (f_l < f_r).any()
    finally:
        both.close()
