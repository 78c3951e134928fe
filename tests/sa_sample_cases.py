"""The cases of the sampled suffix array (sx_locate.hpp: SA values at a sampling distance, the others located by LF walks
over the BWT blocks) that the CPU harness (tests/test_sa_sample_cpu.py) and the GPU (tests/test_gpu_sa_sample.py) run
alike, the layout restated in numpy, and the checks of one record.  TEST INFRASTRUCTURE ONLY.  (The library is imported
inside the functions, never when the module is.)"""
import hashlib

import numpy as np
import pytest

import occ_cases as oc

LOG2S = (1, 5, 10)  # the sampling distances 2, 32 and 1024: the shortest walks, the default, the longest
KERNEL_SHAPES = [(37 * 4096 + 77, 5, 5), (4097, 21, 1), (130, 128, 10)]  # (N, sigma, q)
SX_E_ARG, SX_E_INTERNAL = -1, -3


def samples(N, q):
    return (N + (1 << q) - 1) >> q


def reference_samples(sa, q):
    """the layout restated: (marks, a (blocks, 2) uint64 array of (bits, before); values, SA of the marked rows in row order)"""
    sa = np.asarray(sa, np.uint32)
    N, nb = sa.size, oc.blocks(sa.size)
    marked = np.zeros(nb * oc.ROWS, bool)
    marked[:N] = (sa & ((1 << q) - 1)) == 0
    rows = marked.reshape(nb, oc.ROWS)
    bits = (rows.astype(np.uint64) << np.arange(oc.ROWS, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
    count = rows.sum(axis=1).astype(np.uint64)
    marks = np.zeros((nb, 2), np.uint64)
    marks[:, 0] = bits
    marks[:, 1] = np.cumsum(count) - count  # (u32 before, u32 zero: one little-endian u64)
    return marks, sa[marked[:N]]


def numpy_sa(sym):
    """the suffix array of sym + [0] (symbols >= 1) by prefix doubling"""
    t = np.concatenate([np.asarray(sym, np.int64), np.zeros(1, np.int64)])
    N, rank, k = t.size, t.copy(), 1
    while True:
        second = np.zeros(N, np.int64)
        second[:N - k] = rank[k:] + 1
        order = np.lexsort((second, rank))
        a, b = rank[order], second[order]
        fresh = np.zeros(N, np.int64)
        fresh[order] = np.cumsum(np.concatenate([[0], (a[1:] != a[:-1]) | (b[1:] != b[:-1])]))
        rank = fresh
        if rank.max() == N - 1:
            return order.astype(np.uint32)
        k *= 2


def odd_texts():
    """texts whose walks are odd: one letter repeated (every LF step stays in one run), a short period"""
    return {"one-letter": b">a\n" + b"A" * 1000 + b"\n", "acgt": b">p\n" + b"ACGT" * 300 + b"\n"}


def row_windows(N):
    """windows of rows: neither end on a block boundary, one row, the last row, rows across the first boundaries, nothing"""
    want = {(min(N, 3), N - min(N, 2)), (N // 2, N // 2 + 1), (N - 1, N), (min(N, 70), min(N, 131)), (1, 1)}
    return sorted((lo, hi) for lo, hi in want if 0 <= lo <= hi <= N)


def written(idx):
    chunks = []
    idx.write(chunks.append)
    return b"".join(chunks)


def sampled_index(cache, ctx, Index, oracle_records, how, fasta, sa_sample):
    """the sampled index of a FASTA image by one of the three constructors, kept in `cache` (whose owner closes what it
    holds): the tables of from_tables and the image of load are made once a genome"""
    key = (how, fasta, sa_sample)
    if key not in cache:
        if how == "from_fasta":
            cache[key] = Index.from_fasta(fasta, ctx=ctx, compact=True, sa_sample=sa_sample)
        elif how == "from_tables":
            if ("tables", fasta) not in cache:
                cache[("tables", fasta)] = oracle_records(ctx, fasta)
            cache[key] = Index.from_tables(cache[("tables", fasta)], ctx=ctx, compact=True, sa_sample=sa_sample)
        else:
            if ("image", fasta) not in cache:
                cache[("image", fasta)] = written(sampled_index(cache, ctx, Index, oracle_records, "from_fasta", fasta, sa_sample))
            cache[key] = Index.load(cache[("image", fasta)], ctx=ctx, compact=True, sa_sample=sa_sample)
    return cache[key]


def check_record(ctx, Index, fasta, api, log2s=LOG2S, gpu=False):
    """everything the issue asks of one record, at every sampling distance: the expansion equals the full index's suffix
    array, marks and values are the layout restated in numpy, windows of rows, rows out of range, and the same marks and
    values from tables that arrive from the host (from_tables, load: the windowed path)"""
    with Index.from_fasta(fasta, ctx=ctx) as full:
        assert full.sa_sample == 0 and len(full.records) == 1
        name, N, sigma, _ = full.records[0]
        want = full.device_tables(0)
        image = written(full)
        with pytest.raises(api.StralgAmdError):
            full.expand_sa(0)
        with pytest.raises(api.StralgAmdError):
            full.device_samples(0)
    sa = want["sa"]
    table = api.BwtTable(api.RemapTable(sigma, np.zeros(256, np.int16), None), api.SuffixArray(want["string"], sa), want["c"], want["o"],
                         want["ro"])
    for q in log2s:
        s = 1 << q
        ref_marks, ref_values = reference_samples(sa, q)
        with Index.from_fasta(fasta, ctx=ctx, compact=True, sa_sample=s) as idx:
            assert idx.compact and idx.sa_sample == s and idx.records == [(name, N, sigma, True)]
            got = idx.device_tables(0)
            assert got["sa"] is None and got["o"] is None and not idx.record_info(0).d_sa
            assert (got["string"] == want["string"]).all() and (got["c"] == want["c"]).all()
            smp = idx.record_samples(0)
            assert (smp.sa_log2, smp.n_samples, smp.n_blocks) == (q, samples(N, q), oc.blocks(N))
            align = 256 if gpu else 16  # (a device allocation; the harness allocates with malloc)
            assert smp.d_marks % align == 0 and smp.d_values % align == 0
            assert ctx.sa_sample_bytes(N, s) == (16 * oc.blocks(N), 4 * samples(N, q))
            marks, values = idx.device_samples(0)
            assert marks.tobytes() == ref_marks.tobytes() and values.tobytes() == ref_values.tobytes(), (N, sigma, q)
            if q == 10 and N <= 1001:
                assert values.tolist() == [0]  # (one sample: the walks are as long as they get)
            assert (idx.expand_sa(0) == sa).all(), (N, sigma, q)
            for lo, hi in row_windows(N):
                assert (idx.expand_sa(0, rows=(lo, hi)) == sa[lo:hi]).all(), (N, sigma, q, lo, hi)
            with pytest.raises(api.StralgAmdError):
                idx.expand_sa(0, rows=(0, N + 1))
            with pytest.raises(api.StralgAmdError):
                idx.expand_sa(0, rows=(2, 1))
        # the same marks and values from a suffix array that arrives from the host, in windows
        with Index.from_tables([(name, table)], ctx=ctx, compact=True, sa_sample=s) as rows, \
                Index.load(image, ctx=ctx, compact=True, sa_sample=s) as loaded:
            for other in (rows, loaded):
                assert other.sa_sample == s
                m, v = other.device_samples(0)
                assert m.tobytes() == ref_marks.tobytes() and v.tobytes() == ref_values.tobytes(), (N, sigma, q)
            assert (rows.expand_sa(0) == sa).all()
    return N, sigma


def check_kernels(ctx, mem, api, N, sigma, q):
    """sa_sample_build_dev and sa_locate_rows_dev on their own, over a real suffix array with its blocks: twice into 0x5A-filled
    buffers (the same bytes, nothing behind the last entry), a misaligned marks pointer and a row behind the last (SX_E_ARG),
    marks that do not belong to the blocks (SX_E_INTERNAL: the walks end at their bound)"""
    s = 1 << q
    rng = np.random.default_rng(N + sigma)
    sym = rng.integers(1, sigma, N - 1).astype(np.uint8)
    sym[rng.permutation(N - 1)[:sigma - 1]] = np.arange(1, sigma, dtype=np.uint8)
    sa = numpy_sa(sym)
    text = np.concatenate([sym, np.zeros(1, np.uint8)])
    bwt = text[sa.astype(np.int64) - 1]  # (the row of suffix 0 gets the sentinel)
    counts = np.bincount(text, minlength=sigma)
    c = (np.cumsum(counts) - counts).astype(np.uint32)
    ref_marks, ref_values = reference_samples(sa, q)
    marks_b, values_b = ctx.sa_sample_bytes(N, s)
    assert (marks_b, values_b) == (ref_marks.nbytes, ref_values.nbytes)
    d_bwt, d_sa, d_c = mem.to_dev(bwt), mem.to_dev(sa), mem.to_dev(c)
    d_blocks = mem.zeros(ctx.occ_compact_bytes(N, sigma))
    mem.sync()
    ctx.occ_compact_build_dev(d_bwt, N, sigma, d_blocks)
    both = []
    for _ in range(2):
        d_marks, d_values, d_out = mem.zeros(marks_b + 64), mem.zeros(values_b + 64), mem.zeros(4 * N + 64)
        for buf in (d_marks, d_values, d_out):
            mem.fill(buf, 0x5A)
        mem.sync()
        ctx.sa_sample_build_dev(d_sa, N, s, d_marks, d_values)
        ctx.sa_locate_rows_dev(d_c, d_blocks, N, sigma, d_marks, d_values, s, 0, N, d_out)
        marks, values, out = mem.to_host(d_marks), mem.to_host(d_values), mem.to_host(d_out)
        assert marks[:marks_b].tobytes() == ref_marks.tobytes() and values[:values_b].tobytes() == ref_values.tobytes(), (N, sigma, q)
        assert (out[:4 * N].view(np.uint32) == sa).all(), (N, sigma, q)
        for raw, used in ((marks, marks_b), (values, values_b), (out, 4 * N)):
            assert (raw[used:] == 0x5A).all()  # (nothing behind the last entry is written)
        both.append(marks.tobytes() + values.tobytes() + out.tobytes())
    assert both[0] == both[1]
    one = mem.zeros(16)
    mem.sync()
    ctx.sa_locate_rows_dev(d_c, d_blocks, N, sigma, d_marks, d_values, s, N - 1, N, one)
    assert mem.to_host(one, np.uint32)[0] == sa[N - 1]
    ctx.sa_locate_rows_dev(d_c, d_blocks, N, sigma, d_marks, d_values, s, 5, 5, None)  # (nothing: a success)
    with pytest.raises(api.StralgAmdError, match="code %d" % SX_E_ARG):
        ctx.sa_locate_rows_dev(d_c, d_blocks, N, sigma, d_marks[8:], d_values, s, 0, 1, d_out)
    with pytest.raises(api.StralgAmdError, match="code %d" % SX_E_ARG):
        ctx.sa_sample_build_dev(d_sa, N, s, d_marks[8:], d_values)
    with pytest.raises(api.StralgAmdError, match="code %d" % SX_E_ARG):
        ctx.sa_locate_rows_dev(d_c, d_blocks, N, sigma, d_marks, d_values, s, 0, N + 1, d_out)
    # marks all clear: no row is ever marked, every walk runs to its bound and the call says so
    d_clear = mem.zeros(marks_b)
    mem.sync()
    with pytest.raises(api.StralgAmdError, match="code %d" % SX_E_INTERNAL):
        ctx.sa_locate_rows_dev(d_c, d_blocks, N, sigma, d_clear, d_values, s, 0, N, d_out)
    # ... and the context goes on working
    ctx.sa_locate_rows_dev(d_c, d_blocks, N, sigma, d_marks, d_values, s, 0, N, d_out)
    assert (mem.to_host(d_out)[:4 * N].view(np.uint32) == sa).all()


def long_hits_case():
    """a genome of 5000 x A and 3000 random letters behind them; reads AA and A at k = 0 and one read at k = 1: a hit of
    more matches than the emit kernel's walk takes in a step (4 x 1024), several of more than 32"""
    rng = np.random.default_rng(77)
    genome = b"A" * 5000 + bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 3000)])
    fasta = b">long\n" + genome + b"\n"
    exact = b"@aa\nAA\n+\nII\n@a\nA\n+\nI\n"
    one_edit = b"@aaca\nAACA\n+\nIIII\n"
    return fasta, [(exact, 0), (one_edit, 1)]


def check_long_hits(ctx, Index, caps=(0, 64, 1)):
    """the text of a sampled index equals the full index's from the same context, whatever the cap of a run: the default
    (one run), 64 and 1 (many runs; hits longer than the cap get a buffer of their own)"""
    fasta, read_sets = long_hits_case()
    with Index.from_fasta(fasta, ctx=ctx) as full, Index.from_fasta(fasta, ctx=ctx, compact=True, sa_sample=32) as idx:
        for fastq, k in read_sets:
            want = full.map_reads(fastq, k)
            counts = {}
            for line in want.split(b"\n")[:-1]:
                key = (line.split(b"\t")[0], line.split(b"\t")[5])
                counts[key] = counts.get(key, 0) + 1
            if k == 0:
                assert max(counts.values()) > 4 * 1024
            else:
                assert sum(1 for v in counts.values() if v > 32) >= 2
            digests = {hashlib.sha256(want).hexdigest()}
            for cap in caps:
                ctx.set_locate_chunk_rows(cap)
                try:
                    h, chunks = hashlib.sha256(), []

                    def sink(chunk):
                        h.update(chunk)
                        chunks.append(chunk)

                    idx.map_reads(fastq, k, sink=sink)
                finally:
                    ctx.set_locate_chunk_rows(0)
                assert b"".join(chunks) == want, (k, cap)
                digests.add(h.hexdigest())
            assert len(digests) == 1


def memory_bounds(records, q):
    """(least, most) device_bytes of a sampled compact index with RO over [(name, N, sigma, has_ro)]: the layout restated"""
    least = sum(N + 4 * sigma + 2 * oc.blocks(N) * oc.stride(sigma) + 16 * oc.blocks(N) + 4 * samples(N, q) for _, N, sigma, _ in records)
    return least, least + 4096 * (7 * len(records) + 5)


def check_failure_paths(ctx, Index, api, _lib):
    """arguments that are refused before anything is built, a FASTA cut off with the flag set: no index stays alive"""
    import ctypes as C
    lib = ctx.lib
    start = lib.sx_index_live_count()
    fasta = b">r\nACGTACGT\n"
    for kwargs in (dict(sa_sample=32), dict(compact=True, sa_sample=2048), dict(compact=True, sa_sample=3), dict(compact=True, sa_sample=1),
                   dict(compact=False, sa_sample=4)):
        for make in (lambda: Index.from_fasta(fasta, ctx=ctx, **kwargs), lambda: Index.from_tables([], ctx=ctx, **kwargs),
                     lambda: Index.load(b"\0\0\0\0", ctx=ctx, **kwargs)):
            with pytest.raises((ValueError, api.StralgAmdError)):
                make()
    h = C.c_void_p()
    buf = np.frombuffer(fasta, np.uint8)
    for flags in (5 << 8, _lib.SX_INDEX_COMPACT | (11 << 8), _lib.SX_INDEX_COMPACT | (255 << 8), _lib.SX_INDEX_COMPACT | (1 << 16)):
        assert lib.sx_index_build_fasta_ex(ctx.h, buf.ctypes.data, buf.size, 1, flags, C.byref(h)) == SX_E_ARG and not h
        assert lib.sx_index_from_sources_ex(ctx.h, None, 0, flags, C.byref(h)) == SX_E_ARG and not h
    assert lib.sx_index_live_count() == start
    for cut in (b">cut off", b">one\nACGT\n>cut off inside the header"):
        with pytest.raises(api.StralgAmdError) as e:
            Index.from_fasta(cut, ctx=ctx, compact=True, sa_sample=32)
        assert "code -4" in str(e.value)
        assert lib.sx_index_live_count() == start
    with Index.from_fasta(fasta, ctx=ctx) as full, Index.from_fasta(fasta, ctx=ctx, compact=True) as comp:
        for idx in (full, comp):
            assert idx.sa_sample == 0 and idx.record_samples(0).sa_log2 == 0 and not idx.record_samples(0).d_marks
            with pytest.raises(api.StralgAmdError) as e:
                idx.expand_sa(0)
            assert "code -1" in str(e.value)
    with Index.from_tables([], ctx=ctx, compact=True, sa_sample=32) as empty:
        assert empty.records == [] and empty.map_reads(b"@r\nA\n+\nI\n", 0) == b""
    assert lib.sx_index_live_count() == start
