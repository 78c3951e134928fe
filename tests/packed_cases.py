"""The cases of the packed occurrence table (sx_occ.hpp: the 64-row blocks of the compact table with a nibble a row, for
alphabets of up to 8 symbols) that the CPU harness (tests/test_packed_cpu.py) and the GPU (tests/test_gpu_packed.py) run
alike: records whose N = symbols + 1 falls before, on and behind the block boundaries over alphabets of 2, 5 and 8
symbols, the layout restated in numpy, and the checks of one record, of the raw calls, of the searches and of the failure
paths.  TEST INFRASTRUCTURE ONLY.  (The library is imported inside the functions, never when the module is.)"""
import numpy as np
import pytest

import occ_cases as oc
import sa_sample_cases as sc

SYMBOLS = [0, 1, 62, 63, 64, 65, 127, 128, 129, 1000]  # N = symbols + 1
LETTERS = [1, 4, 7]  # sigma = 2, 5, 8 (the largest)
ROWS, STRIDE, COUNTERS, MAX_SIGMA = 64, 64, 8, 8
RAW_SHAPES_GPU = [(37 * 4096 + 77, 5), (4096, 2), (4097, 8), (130, 8)]  # (N, sigma): several tiles of 64 blocks, tile edges
RAW_SHAPES_HARNESS = [(3 * 4096 + 77, 5), (4096, 2), (4097, 8), (130, 8)]
SX_E_ARG = -1


def record_cases():
    """[(symbols, letters, fasta bytes)]: one record a FASTA image"""
    return [(n, l, b">rec-%d-%d\n" % (n, l) + oc.record(n, l) + b"\n") for l in LETTERS for n in SYMBOLS]


def reference_blocks(o, N, sigma):
    """the layout restated from the full table o ((N + 1, sigma)): a uint8 array (blocks, 64): 8 u32 counters (zero from
    sigma on), then row 64 b + j in byte j / 2, the low nibble for even j, 0xF from row N on"""
    nb = oc.blocks(N)
    out = np.zeros((nb, STRIDE), np.uint8)
    sym = np.full(nb * ROWS, 0xF, np.uint8)
    sym[:N] = np.argmax(o[1:] != o[:-1], axis=1).astype(np.uint8)
    assert sym[:N].max() < MAX_SIGMA
    out[:, 4 * COUNTERS:] = (sym[0::2] | (sym[1::2] << 4)).reshape(nb, ROWS // 2)
    counters = np.zeros((nb, COUNTERS), np.uint32)
    counters[:, :sigma] = o[::ROWS][:nb]
    out[:, :4 * COUNTERS] = counters.view(np.uint8)
    return out


def running_counts(bwt, sigma):
    want = np.zeros((bwt.size + 1, sigma), np.uint32)
    want[1:] = np.cumsum(bwt[:, None] == np.arange(sigma)[None, :], axis=0)
    return want


def check_record(ctx, Index, fasta, api, gpu=False):
    """one record: both tables expanded from the packed index equal the full index's entry for entry, the blocks are the
    layout restated in numpy, the blocks built from full rows equal them byte for byte, windows of the expansion, what
    record_occ reports, the alignment"""
    with Index.from_fasta(fasta, ctx=ctx) as full, Index.from_fasta(fasta, ctx=ctx, compact=True, packed=True) as pk:
        assert pk.compact and pk.packed and not full.packed
        assert pk.records == full.records and len(full.records) == 1
        _, N, sigma, has_ro = full.records[0]
        assert has_ro and sigma <= MAX_SIGMA
        want = full.device_tables(0)
        got = pk.device_tables(0)
        assert got["o"] is None and got["ro"] is None
        for f in ("string", "sa", "c"):
            assert (got[f] == want[f]).all(), f
        occ = pk.record_occ(0)
        assert (occ.compact, occ.stride, occ.sigma_pad, occ.n_blocks) == (2, 64, 8, N // 64 + 1)
        align = 256 if gpu else 16  # (a device allocation; the harness allocates with malloc)
        assert occ.d_occ % align == 0 and occ.d_rocc % align == 0
        assert ctx.occ_packed_bytes(N, sigma) == (N // 64 + 1) * 64
        by_table = {}
        for reverse, field in ((False, "o"), (True, "ro")):
            o = pk.expand_o(0, reverse=reverse)
            assert o.shape == (N + 1, sigma) and (o == want[field]).all(), (field, N, sigma)
            raw = pk.device_occ(0, reverse=reverse)
            assert raw.shape == (N // 64 + 1, 64)
            assert (raw == reference_blocks(want[field], N, sigma)).all(), (field, N, sigma)
            by_table[field] = raw
            for lo, hi in {(min(N, 3), N + 1 - min(N, 2)), (N // 2, N // 2 + 1), (N, N + 1), (min(N, 70), min(N + 1, 131)), (1, 1)}:
                if lo <= hi:
                    assert (pk.expand_o(0, reverse=reverse, rows=(lo, hi)) == want[field][lo:hi]).all(), (field, lo, hi)
        name = full.records[0][0]
        table = oc.table_of(want["sa"], want["c"], want["o"], want["ro"], sigma, want["string"])
        with Index.from_tables([(name, table)], ctx=ctx, compact=True, packed=True) as rows:
            assert rows.compact and rows.packed and rows.record_occ(0).compact == 2
            assert (rows.device_occ(0) == by_table["o"]).all() and (rows.device_occ(0, reverse=True) == by_table["ro"]).all()
            assert (rows.expand_o(0) == want["o"]).all()
        with pytest.raises(api.StralgAmdError):
            pk.expand_o(0, rows=(0, N + 2))
        return N, sigma


def check_expand_sa(ctx, Index, fasta, samplings=(2, 32, 1024)):
    """expand_sa of a packed sampled index equals the full suffix array, whole and in windows off the block boundaries"""
    with Index.from_fasta(fasta, ctx=ctx) as full:
        sa = full.device_tables(0)["sa"]
        N = int(sa.size)
    for s in samplings:
        with Index.from_fasta(fasta, ctx=ctx, compact=True, packed=True, sa_sample=s) as idx:
            assert idx.packed and idx.sa_sample == s and idx.record_occ(0).compact == 2
            assert (idx.expand_sa(0) == sa).all(), (N, s)
            for lo, hi in sc.row_windows(N):
                assert (idx.expand_sa(0, rows=(lo, hi)) == sa[lo:hi]).all(), (N, s, lo, hi)


def check_raw_calls(ctx, mem, api, shapes):
    """occ_packed_build_dev / occ_packed_expand_dev on their own over BWTs that are no text's: the layout and numpy's running
    counts, guard bytes behind the last block, two builds with the same bytes, the arguments that are refused"""
    rng = np.random.default_rng(4)
    for N, sigma in shapes:
        bwt = rng.integers(0, sigma, N).astype(np.uint8)
        want = running_counts(bwt, sigma)
        nbytes = ctx.occ_packed_bytes(N, sigma)
        assert nbytes == (N // 64 + 1) * 64
        d_bwt = mem.to_dev(bwt)
        both = []
        for _ in range(2):
            d_blocks, d_rows = mem.zeros(nbytes + 256), mem.zeros((N + 1) * sigma, np.uint32)
            mem.fill(d_blocks, 0x5A)
            mem.sync()
            ctx.occ_packed_build_dev(d_bwt, N, sigma, d_blocks)
            ctx.occ_packed_expand_dev(d_blocks, N, sigma, 0, N + 1, d_rows)
            raw = mem.to_host(d_blocks)
            assert (raw[nbytes:] == 0x5A).all()  # (nothing behind the last block is written)
            assert (raw[:nbytes].reshape(-1, STRIDE) == reference_blocks(want, N, sigma)).all(), (N, sigma)
            assert (mem.to_host(d_rows, np.uint32).reshape(N + 1, sigma) == want).all(), (N, sigma)
            both.append(raw.tobytes())
        assert both[0] == both[1]
        d_win = mem.zeros(3 * sigma, np.uint32)
        mem.sync()
        ctx.occ_packed_expand_dev(d_blocks, N, sigma, 63, 66, d_win)  # (across a block boundary)
        assert (mem.to_host(d_win, np.uint32).reshape(3, sigma) == want[63:66]).all()
        refused = [lambda: ctx.occ_packed_expand_dev(d_blocks[8:], N, sigma, 0, 1, d_rows),
                   lambda: ctx.occ_packed_build_dev(d_bwt, N, sigma, d_blocks[8:]),
                   lambda: ctx.occ_packed_expand_dev(d_blocks, N, sigma, 0, N + 2, d_rows),
                   lambda: ctx.occ_packed_expand_dev(d_blocks, N, 9, 0, 1, d_rows),
                   lambda: ctx.occ_packed_build_dev(d_bwt, N, 9, d_blocks)]
        for call in refused:
            with pytest.raises(api.StralgAmdError, match="code %d" % SX_E_ARG):
                call()
        assert mem.to_host(d_blocks).tobytes() == both[1]  # (a refused call writes nothing)
    assert ctx.occ_packed_bytes(10, 9) == 0 and ctx.occ_packed_bytes(0, 5) == 0 and ctx.occ_packed_bytes(10, 8) == 64


def split_cases(cases, remapped):
    """(names of the approx cases with sigma <= 8, names of the others), each sorted"""
    small, large = [], []
    for name in sorted(cases):
        (small if remapped(cases[name]["raw"])[1] <= MAX_SIGMA else large).append(name)
    return small, large


class FullAndPacked:
    """one record's tables on the device as full tables and as packed blocks (two indexes from the same host tables)"""

    def __init__(self, ctx, Index, sa, c, o, ro, sigma):
        t = oc.table_of(sa, c, o, ro, sigma)
        self.full = Index.from_tables([(b"r", t)], ctx=ctx)
        try:
            self.pk = Index.from_tables([(b"r", t)], ctx=ctx, compact=True, packed=True)
        except Exception:
            self.full.close()
            raise
        self.N, self.sigma = int(sa.size), sigma
        self.rec, self.occ = self.full.record_info(0), self.pk.record_occ(0)
        assert self.occ.compact == 2

    def close(self):
        self.full.close()
        self.pk.close()

    def approx(self, ctx, mem, pat, off, k, with_ro, hits_dtype):
        count = off.size - 1
        d_pat, d_off = mem.to_dev(np.concatenate([pat, np.zeros(16, np.uint8)])), mem.to_dev(off)
        out = []
        for packed in (False, True):
            d_ho = mem.zeros(count + 1, np.uint64)
            mem.sync()
            call = ctx.bwt_approx_search_packed_dev if packed else ctx.bwt_approx_search_dev
            o, ro = (self.occ.d_occ, self.occ.d_rocc) if packed else (self.rec.d_o, self.rec.d_ro)
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
        for packed in (False, True):
            d_l, d_r = mem.zeros(count, np.uint32), mem.zeros(count, np.uint32)
            mem.sync()
            call = ctx.bwt_exact_search_packed_dev if packed else ctx.bwt_exact_search_dev
            call(self.rec.d_c, self.occ.d_occ if packed else self.rec.d_o, self.N, self.sigma, d_pat, d_off, count, d_l, d_r)
            out.append((mem.to_host(d_l, np.uint32), mem.to_host(d_r, np.uint32)))
        return out


def check_searches(ctx, mem, Index, case, tables, hits_dtype, api, ks=(0, 1, 2)):
    """one case of tests/approx_cases.py with sigma <= 8: at every k, with and without RO, the packed calls return the
    full-table calls' offsets and hits byte for byte; at the case's own k the hits are the reference stream; the exact
    search's intervals are equal and some interval is non-empty"""
    sa, c, o, ro, sigma = tables
    both = FullAndPacked(ctx, Index, sa, c, o, ro, sigma)
    try:
        pat, off = case["pat"], case["pat_off"]
        for k in sorted(set(ks) | {case["k"]}):
            for with_ro, mode in ((True, "ro"), (False, "noro")):
                (f_off, f_hits), (p_off, p_hits) = both.approx(ctx, mem, pat, off, k, with_ro, hits_dtype)
                assert (f_off == p_off).all() and f_hits.tobytes() == p_hits.tobytes(), (k, mode)
                if k == case["k"]:
                    assert api.approx_matches(p_hits, p_off, np.diff(off), sa) == case["streams"][mode], (k, mode)
        (f_l, f_r), (p_l, p_r) = both.exact(ctx, mem, pat, off)
        assert (f_l == p_l).all() and (f_r == p_r).all()
        assert (f_l < f_r).any()
    finally:
        both.close()


def check_refuses_large_sigma(ctx, Index, tables, api):
    """a record of more than 8 symbols has no packed form: from_tables raises with SX_E_ARG and nothing stays alive"""
    sa, c, o, ro, sigma = tables
    assert sigma > MAX_SIGMA
    start = ctx.lib.sx_index_live_count()
    with pytest.raises(api.StralgAmdError, match="code %d" % SX_E_ARG):
        Index.from_tables([(b"r", oc.table_of(sa, c, o, ro, sigma))], ctx=ctx, compact=True, packed=True)
    assert ctx.lib.sx_index_live_count() == start


def memory_bounds(ctx, records, sa_sample=0):
    """(least, most) device_bytes of a packed index with RO over [(name, N, sigma, has_ro)]: N bytes of string, the suffix
    array (or its marks and values as sx_sa_sample_bytes counts them), two tables of 64-byte blocks, C; the slack is the
    compact index's (occ_cases.memory_bounds)"""
    least = 0
    for _, N, sigma, _ in records:
        sa_bytes = 4 * N if not sa_sample else sum(ctx.sa_sample_bytes(N, sa_sample))
        least += N + sa_bytes + 2 * (N // 64 + 1) * 64 + 4 * sigma
    return least, least + 4096 * (5 * len(records) + 5)


def nine_symbol_source(_lib, keep):
    """an sx_index_source of a record of 8 letters (sigma = 9) over numpy tables that `keep` holds alive"""
    import approx_model
    sym = np.array([1, 2, 3, 4, 5, 6, 7, 8, 1, 2, 3], np.uint8)
    sa, c, o, ro = approx_model.tables(sym, 9)
    arrays = [np.ascontiguousarray(a, np.uint32) for a in (sa, c, o, ro)] + [np.full(256, -1, np.int8),
                                                                           np.concatenate([sym, np.zeros(1, np.uint8)])]
    keep.extend(arrays)
    sa, c, o, ro, tab, string = arrays
    rec = _lib.MapRecord(b"nine", sa.ctypes.data, c.ctypes.data, o.ctypes.data, ro.ctypes.data, sa.size, 9, tab.ctypes.data)
    return _lib.IndexSource(rec, string.ctypes.data)


def check_failure_paths(ctx, Index, api, _lib):
    """flags that are refused before anything is built, a cut-off FASTA, a record that does not fit: nothing stays alive"""
    import ctypes as C
    lib = ctx.lib
    start = lib.sx_index_live_count()
    fasta = b">r\nACGTACGT\n"
    buf = np.frombuffer(fasta, np.uint8)
    h = C.c_void_p()
    assert _lib.SX_INDEX_PACKED == 4
    for flags in (_lib.SX_INDEX_PACKED, 2, 1 << 16, _lib.SX_INDEX_COMPACT | 8, _lib.SX_INDEX_PACKED | (5 << 8)):
        assert lib.sx_index_build_fasta_ex(ctx.h, buf.ctypes.data, buf.size, 1, flags, C.byref(h)) == SX_E_ARG and not h
        assert lib.sx_index_from_sources_ex(ctx.h, None, 0, flags, C.byref(h)) == SX_E_ARG and not h
    for make in (lambda: Index.from_fasta(fasta, ctx=ctx, packed=True), lambda: Index.from_tables([], ctx=ctx, packed=True),
                 lambda: Index.load(b"\0\0\0\0", ctx=ctx, packed=True), lambda: _lib.index_flags(False, 0, True),
                 lambda: Index.from_fasta(fasta, ctx=ctx, sa_sample=32, packed=True)):
        with pytest.raises(ValueError):
            make()
    assert _lib.index_flags(True, 32, True) == 1 | 4 | (5 << 8) and _lib.index_flags(True) == 1 and _lib.index_flags(True, 4) == 1 | (2 << 8)
    assert lib.sx_index_live_count() == start
    for cut in (b">cut off", b">one\nACGT\n>cut off inside the header"):
        with pytest.raises(api.StralgAmdError) as e:
            Index.from_fasta(cut, ctx=ctx, compact=True, packed=True)
        assert "code -4" in str(e.value)
        assert lib.sx_index_live_count() == start
    # a record of 8 letters behind one that fits: the whole build fails, and what the first record took goes with it
    with pytest.raises(api.StralgAmdError, match="code %d" % SX_E_ARG):
        Index.from_fasta(b">fits\nACGTACGT\n>too-many\nABCDEFGH\n", ctx=ctx, compact=True, packed=True)
    assert lib.sx_index_live_count() == start
    with Index.from_fasta(b">seven\nABCDEFG\n", ctx=ctx, compact=True, packed=True) as seven:
        assert seven.records == [(b"seven", 8, 8, True)]
    with Index.from_tables([], ctx=ctx, compact=True, packed=True) as empty:
        assert empty.packed and empty.records == [] and empty.map_reads(b"@r\nA\n+\nI\n", 0) == b""
    # add_record of a sigma = 9 record: SX_E_ARG, and the index still maps
    with Index.from_fasta(fasta, ctx=ctx) as full, Index.from_fasta(fasta, ctx=ctx, compact=True, packed=True) as idx:
        fastq = b"@q\nCGTA\n+\nIIII\n"
        want = full.map_reads(fastq, 1)
        assert want and idx.map_reads(fastq, 1) == want
        keep, nbytes = [], idx.device_bytes
        src = nine_symbol_source(_lib, keep)
        assert lib.sx_index_add_record(ctx.h, idx.h, C.byref(src), 0) == SX_E_ARG
        assert len(idx.records) == 1 and idx.device_bytes == nbytes and idx.map_reads(fastq, 1) == want
        assert lib.sx_index_add_record(ctx.h, full.h, C.byref(src), 0) == 0 and len(full.records) == 2  # (the record itself is sound)
    assert lib.sx_index_live_count() == start


def check_the_record_without_symbols(ctx, Index, api, written):
    """the empty record beside a full one: sigma = 1, one block"""
    fasta = b">empty\n>full\nACGT\n"
    with Index.from_fasta(fasta, ctx=ctx, compact=True, packed=True) as idx, Index.from_fasta(fasta, ctx=ctx) as full:
        assert idx.records == [(b"empty", 1, 1, True), (b"full", 5, 5, True)]
        assert (idx.expand_o(0) == full.device_tables(0)["o"]).all() and idx.expand_o(0).shape == (2, 1)
        assert (idx.device_occ(0) == reference_blocks(full.device_tables(0)["o"], 1, 1)).all()
        assert written(idx) == written(full)
        with pytest.raises(api.StralgAmdError) as e:
            idx.map_reads(b"@r\nAC\n+\nII\n", 0)
        assert "code -1" in str(e.value)
