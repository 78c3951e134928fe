"""What a context carries from call to call ("What a context carries from call to call"): the operations that
tests/test_reuse_cpu.py (the CPU execution harness) and tests/test_gpu_reuse.py (the GPU) run one behind the other in one
context -- after a scribble over its workspace (Context.scribble), around the look-back epoch's and the read-back
sequence's wraps, across regrowth and trim, after failed calls, and from two contexts in turn.  TEST INFRASTRUCTURE ONLY.

Every expected value comes from the oracle, from the search's Python restatement (tests/approx_model.py) or from the
reference mapper's recorded texts (best_cases.want_of / plain_of); none from a run of the library.  The inputs and
expected values are made once per process (Cases caches them) and never written to.

`mem` is one of the two objects of tests/device_memory.py.  An operation is run(ctx) -> True; it sets the switches it
needs and puts them back, and a wrong result is an AssertionError that says what differed.

Shapes.  The harness's are those of tests/test_emu_pipeline.py, cut where a launch costs more there than its entries: the
induced build of a wide alphabet takes 3000 symbols of 9 letters (a byte text's 255 buckets took 20 s), the recursion one
level.  The GPU's are the smallest that put several tiles into a chained launch and cross the thresholds that only the
harness build lowers: an induce round scans tiles of kIndTile = 2048 entries (sx_induce_common.hpp) and is one chained launch
up to 256 tiles for at most 8 buckets, so a DNA text of 2^20 + 3 symbols has rounds of 2^18 entries = 128 look-back tiles a
bucket (the harness's 17 001 symbols: 3 tiles); the three-pass inverse starts at N = 2^23 on the GPU
(SX_INVERSE_TWO_PASS_FROM), at 3000 in the harness."""
import threading

import numpy as np

import approx_model
import best_cases as bc
import oracle
from oracle import pyoracle
from next_rows_cases import fibonacci
from stralg_amd import _lib, api
from stralg_amd.synth import synth

IND_TILE = 2048  # kIndTile

HARNESS = dict(dna=17_001, bytes_direct=9_000, bytes_induced=3_000, induced_sigma=10, general=3_000, fib=5_000, recurse_min=1_500,
               tables=3_001, inverse=(2_999, 6_337), search_text=2_500, patterns=300, pattern_len=12, modelled=40,
               sort_pairs=5_000, exclusive_sum=70_000, dna_small=4_097, dna_large=100_000, tables_small=700, tables_large=20_000,
               search_small=600, search_large=30_000, packed_case="test-out", map_large="two-records-best")
GPU = dict(dna=(1 << 20) + 3, bytes_direct=(1 << 18) + 1, bytes_induced=1 << 18, induced_sigma=256, general=1 << 18, fib=1 << 18,
           recurse_min=5000, packed_case="two-records-best", map_large="hg38/reads-100-10-0",
           tables=70_001, inverse=((1 << 20) + 5, 1 << 23), search_text=1 << 16, patterns=2_000, pattern_len=30, modelled=40,
           sort_pairs=300_001, exclusive_sum=1_000_003, dna_small=70_001, dna_large=(1 << 20) + 3, tables_small=4_097, tables_large=70_001,
           search_small=4_096, search_large=1 << 16)

FILLS = (0x00, 0xFF, 0xA5)
EPOCH_LIMIT = _lib.CHAIN_EPOCH_LIMIT


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not (got == want).all():
        at = int(np.flatnonzero(got.reshape(-1) != want.reshape(-1))[0])
        raise AssertionError((what, "first difference at", at, int(got.reshape(-1)[at]), int(want.reshape(-1)[at])))
    return True


def invariant(ctx, what=""):
    """no status word of the look-back slab carries an epoch above the context's, in the context and in its child; returns
    the counters"""
    k = ctx.counters()
    assert k["chain_slab_max_epoch"] <= k["chain_epoch"] < EPOCH_LIMIT, (what, k)
    assert k["child"]["chain_slab_max_epoch"] <= k["child"]["chain_epoch"] < EPOCH_LIMIT, (what, k)
    return k


class Cases:
    """the operations over one kind of memory at one set of shapes"""

    def __init__(self, mem, shapes, records_of=None):
        self.mem, self.s, self.records_of = mem, shapes, records_of
        self._cache, self._lock = {}, threading.RLock()
        self.ops = {
            "sa-dna": self.sa_dna,
            "sa-bytes-direct": self.sa_bytes_direct,
            "sa-bytes-induced": self.sa_bytes_induced,
            "sa-general-path": self.sa_general,
            "sa-fibonacci-child": self.sa_fibonacci,
            "build-tables": self.build_tables,
            "inverse-lcp": self.inverse_lcp,
            "exact-search": self.exact_search,
            "approx-search-k2": self.approx_search,
            "best-search": self.best_search,
            "fasta-records": self.fasta_records,
            "map-reads": self.map_reads,
            "packed-sampled-index": self.packed_index,
            "primitives": self.primitives,
        }

    def made(self, key, make):
        with self._lock:
            if key not in self._cache:
                self._cache[key] = make()
            return self._cache[key]

    # ---- suffix arrays ------------------------------------------------------------------------------------------------------
    def dna_text(self, n, seed):
        def make():
            x = synth(n, 5, seed)
            return x, oracle.sa_is(x, 5)
        return self.made(("dna", n, seed), make)

    def sa_dna(self, ctx, seed=7, n=None):
        """a DNA text through the small-alphabet induce rounds (several look-back tiles a round: see the module's text)"""
        n = n or self.s["dna"]
        x, want = self.dna_text(n, seed)
        ctx.set_small_direct_max(0)
        try:
            sa = ctx.sa_build(x, 5)
            st = ctx.last_stats()
        finally:
            ctx.set_small_direct_max(-1)
        assert st["lms_path"] != 3 and st["induce_rounds"] > 0, st
        if n == self.s["dna"]:
            assert n // 4 >= 2 * IND_TILE  # (several tiles a round)
        return same(sa, want, ("sa-dna", n, seed))

    def bytes_text(self, n, seed=3, sigma=256):
        def make():
            x = synth(n, sigma, seed)
            x[100:112] = x[1000:1012]  # ties beyond the first key
            return x, oracle.sa_is(x, sigma)
        return self.made(("bytes", n, seed, sigma), make)

    def sa_bytes_direct(self, ctx):
        x, want = self.bytes_text(self.s["bytes_direct"])
        sa = ctx.sa_build(x, 256)
        assert ctx.last_stats()["lms_path"] == 3, ctx.last_stats()
        return same(sa, want, "sa-bytes-direct")

    def sa_bytes_induced(self, ctx):
        """wide induce rounds and the hoisted other-region rounds"""
        sigma = self.s["induced_sigma"]
        x, want = self.bytes_text(self.s["bytes_induced"], 5, sigma)
        ctx.set_no_direct_sort(True)
        ctx.set_small_direct_max(0)
        try:
            sa = ctx.sa_build(x, sigma)
            st = ctx.last_stats()
        finally:
            ctx.set_no_direct_sort(False)
            ctx.set_small_direct_max(-1)
        assert st["lms_path"] != 3 and st["induce_rounds"] > 0, st
        return same(sa, want, "sa-bytes-induced")

    def sa_general(self, ctx):
        def make():
            n = self.s["general"]
            x = synth(n, 5, 9)
            L = n // 60
            x[n // 2:n // 2 + L] = x[100:100 + L]  # a long duplication
            x[3 * n // 4:3 * n // 4 + L] = x[100:100 + L]
            return x, oracle.sa_is(x, 5)
        x, want = self.made("general", make)
        ctx.set_small_direct_max(0)
        ctx.force_general_path(True)
        try:
            sa = ctx.sa_build(x, 5)
            st = ctx.last_stats()
        finally:
            ctx.force_general_path(False)
            ctx.set_small_direct_max(-1)
        assert st["lms_path"] == 2, st
        return same(sa, want, "sa-general-path")

    def sa_fibonacci(self, ctx):
        """the reduced string of a Fibonacci text recurses: the child context exists afterwards"""
        def make():
            x = fibonacci(self.s["fib"])
            return x, oracle.sa_is_strict(x, 3)
        x, want = self.made("fib", make)
        ctx.set_small_direct_max(0)
        ctx.set_recurse_min(self.s["recurse_min"])
        try:
            sa = ctx.sa_build(x, 3)
            st = ctx.last_stats()
        finally:
            ctx.set_recurse_min(-1)
            ctx.set_small_direct_max(-1)
        assert st["recursion_levels"] >= 1, st
        assert ctx.counters()["has_child"]
        return same(sa, want, "sa-fibonacci-child")

    # ---- tables -------------------------------------------------------------------------------------------------------------
    def tables_text(self, sigma, n):
        def make():
            x = np.random.default_rng(sigma + n).integers(1, sigma, size=n, dtype=np.uint8)
            sa = oracle.sa_is(x, sigma)
            return x, sa, oracle.c_table(x, sigma), oracle.o_table(x, sa, sigma)
        return self.made(("tables", sigma, n), make)

    def build_tables(self, ctx, sigmas=(5, 21, 128), n=None):
        n = n or self.s["tables"]
        for sigma in sigmas:
            x, want_sa, want_c, want_o = self.tables_text(sigma, n)
            sa, c, o = ctx.build_tables(x, sigma)
            same(sa, want_sa, ("build-tables sa", sigma, n))
            same(c, want_c, ("build-tables c", sigma, n))
            same(o, want_o, ("build-tables o", sigma, n))
        return True

    # ---- inverse and LCP ----------------------------------------------------------------------------------------------------
    def inverse_text(self, N):
        def make():
            n = N - 1
            x = synth(n, 5, N % 1000)
            L = min(n // 3, 3000)
            x[n // 2:n // 2 + L] = x[10:10 + L]
            sa = oracle.sa_is(x, 5)
            mem = self.mem
            d = (mem.to_dev(x), mem.to_dev(sa))
            mem.sync()
            return x, sa, oracle.inverse(sa), oracle.lcp(x, sa), d
        return self.made(("inverse", N), make)

    def inverse_lcp(self, ctx, sizes=None):
        """sx_sa_lcp_dev on both sides of the three-pass threshold: the inverse by the plain kernel and by the window passes,
        the LCP by Kasai's chunks and (the harness: below SX_LCP_PHI_MAX) by Phi"""
        mem = self.mem
        for N in sizes or self.s["inverse"]:
            x, sa, want_inv, want_lcp, (d_x, d_sa) = self.inverse_text(N)
            d_inv, d_lcp = mem.zeros(N, np.uint32), mem.zeros(N, np.uint32)
            mem.fill(d_inv, 0x5A)
            mem.fill(d_lcp, 0x5A)
            mem.sync()
            ctx.sa_lcp_dev(d_x, d_sa, N, d_inv, d_lcp)
            same(mem.to_host(d_inv, np.uint32), want_inv, ("inverse", N))
            same(mem.to_host(d_lcp, np.uint32), want_lcp, ("lcp", N))
        return True

    # ---- searches -----------------------------------------------------------------------------------------------------------
    def search_tables(self, n=None):
        """(x, sa, c, o, ro, patterns, bc.Tables in device memory) of a DNA text with a duplication and patterns cut from it,
        some of them changed in up to three places"""
        n = n or self.s["search_text"]

        def make():
            rng = np.random.default_rng(41 + n)
            x = rng.integers(1, 5, n).astype(np.uint8)
            x[n - n // 4:n - n // 4 + n // 8] = x[n // 10:n // 10 + n // 8]
            sa, c, o, ro = approx_model.tables(x, 5)
            m, count = self.s["pattern_len"], self.s["patterns"]
            pats = []
            for q in range(count):
                a = int(rng.integers(0, n - m))
                p = x[a:a + m].copy()
                for _ in range(q % 4):
                    p[int(rng.integers(0, m))] = int(rng.integers(1, 5))
                pats.append(p)
            off = (np.arange(count + 1) * m).astype(np.uint32)
            T = bc.Tables(self.mem, c, o, ro, 5, np.concatenate(pats).astype(np.uint8), off)
            return x, sa, c, o, ro, pats, T
        return self.made(("search", n), make)

    def modelled(self, n=None):
        """per modelled pattern [the model's matches at d = 0, 1, 2]"""
        x, sa, c, o, ro, pats, T = self.search_tables(n)
        return self.made(("model", n), lambda: [[approx_model.matches(c, o, ro, sa, p, d) for d in range(3)] for p in pats[:self.s["modelled"]]])

    def exact_search(self, ctx, n=None):
        x, sa, c, o, ro, pats, T = self.search_tables(n)
        want = self.made(("exact", n), lambda: np.array([oracle.bwt_exact_search(c, o, 5, p) for p in pats], np.int64))
        mem = self.mem
        d_l, d_r = mem.zeros(T.count, np.uint32), mem.zeros(T.count, np.uint32)
        mem.fill(d_l, 0x77)
        mem.fill(d_r, 0x77)
        mem.sync()
        ctx.bwt_exact_search_dev(T.c, T.o, T.N, 5, T.pat, T.off, T.count, d_l, d_r)
        same(mem.to_host(d_l, np.uint32), want[:, 0], "exact-search L")
        return same(mem.to_host(d_r, np.uint32), want[:, 1], "exact-search R")

    def approx_search(self, ctx, k=2, n=None):
        """count, then emit; the modelled patterns' streams against the model, every pattern's records under its own number"""
        x, sa, c, o, ro, pats, T = self.search_tables(n)
        model = self.modelled(n)
        ho, hits = T.approx(ctx, k)
        assert int(ho[0]) == 0 and int(ho[-1]) == hits.size and (np.diff(ho.astype(np.int64)) >= 0).all()
        same(hits["query"], np.repeat(np.arange(T.count), np.diff(ho).astype(np.int64)), "approx-search query numbers")
        m = len(model)
        got = api.approx_matches(hits[:int(ho[m])], ho[:m + 1], [p.size for p in pats[:m]], sa)
        assert got == [per[k] for per in model], "approx-search: the streams differ from the model's"
        assert sum(len(g) for g in got) > 0
        return True

    def approx_search_host(self, ctx, k, n):
        """sx_bwt_approx_search: tables, patterns and hits through the staging slab"""
        x, sa, c, o, ro, pats, T = self.search_tables(n)
        model = self.modelled(n)
        flat, off = np.concatenate(pats).astype(np.uint8), (np.arange(len(pats) + 1) * pats[0].size).astype(np.uint32)
        ho, hits = ctx.bwt_approx_search(c, o, ro, 5, flat, off, k)
        m = len(model)
        got = api.approx_matches(hits[:int(ho[m])], ho[:m + 1], [p.size for p in pats[:m]], sa)
        assert got == [per[k] for per in model], "approx-search over host buffers: the streams differ from the model's"
        return int(ho[-1]) == hits.size

    def best_search(self, ctx, k=2, n=None):
        x, sa, c, o, ro, pats, T = self.search_tables(n)
        model = self.modelled(n)
        strata, ho, hits, failure = T.best(ctx, k)
        assert failure is None, failure
        assert int(ho[-1]) == hits.size
        m = len(model)
        want_e = [next((d for d in range(k + 1) if per[d]), None) for per in model]
        same(strata[:m], [0xFF if e is None else e for e in want_e], "best-search strata")
        got = api.approx_matches(hits[:int(ho[m])], ho[:m + 1], [p.size for p in pats[:m]], sa)
        assert got == [[] if e is None else per[e] for per, e in zip(model, want_e)], "best-search: the streams differ from the model's"
        assert len(set(want_e)) >= 3  # (the fixture has several strata)
        return True

    # ---- ingest and mapping -------------------------------------------------------------------------------------------------
    def fasta_records(self, ctx):
        import conftest
        conftest.check_fasta(ctx.fasta_records, self.made("fasta", conftest.fasta_cases))
        return True

    def records(self, ctx, fasta):
        """the tables the mapper reads: the harness's from the oracle (tests/test_sam_cpu.py records_of), the GPU's built by
        the context itself, every time"""
        if self.records_of is not None:
            return self.records_of(ctx, fasta)
        return [(name, api.build_complete_table(seq, True, ctx)) for name, seq in ctx.fasta_records(fasta)]

    def map_text(self, ctx, k, both, best, name="two-records-best"):
        c = self.made("best-cases", bc.best_cases)[name]
        chunks = []
        ctx.map_reads_stream(self.records(ctx, c["fasta"]), c["fastq"], k, chunks.append, both_strands=both, best=best)
        bc.check_text(b"".join(chunks), (bc.want_of if best else bc.plain_of)(c, k, both))
        return True

    def map_reads(self, ctx):
        """two-records-best: plain on one strand, best-stratum on both"""
        return self.map_text(ctx, 1, False, False) and self.map_text(ctx, 2, True, True)

    def map_index(self, ctx, k, name):
        """an index that the context builds from the FASTA itself (nothing cached: ingest, builds and tables are the
        context's work every time), then the plain mapping on one strand"""
        c = self.made("best-cases", bc.best_cases)[name]
        with api.Index.from_fasta(c["fasta"], ctx=ctx) as idx:
            bc.check_text(idx.map_reads(c["fastq"], k), bc.plain_of(c, k, False))
        return True

    def packed_index(self, ctx, k=1):
        c = self.made("best-cases", bc.best_cases)[self.s["packed_case"]]
        with api.Index.from_fasta(c["fasta"], ctx=ctx, compact=True, packed=True, sa_sample=32) as idx:
            bc.check_text(idx.map_reads(c["fastq"], k), bc.plain_of(c, k, False))
        return True

    # ---- primitives ---------------------------------------------------------------------------------------------------------
    def primitives(self, ctx):
        mem = self.mem

        def make():
            rng = np.random.default_rng(1)
            keys = rng.integers(0, 1 << 62, size=self.s["sort_pairs"], dtype=np.uint64)
            keys[::7] = keys[3]  # duplicates: stability matters
            x = rng.integers(0, 800, size=self.s["exclusive_sum"], dtype=np.uint32)
            return keys, np.argsort(keys, kind="stable"), x, np.concatenate(([0], np.cumsum(x, dtype=np.uint64)[:-1])).astype(np.uint32)
        keys, order, x, sums = self.made("prims", make)
        n = keys.size
        ka, va = mem.to_dev(keys), mem.to_dev(np.arange(n, dtype=np.uint32))
        kb, vb = mem.zeros(n, np.uint64), mem.zeros(n, np.uint32)
        mem.sync()
        in_b = ctx.prim_sort_pairs_dev(ka, va, kb, vb, n, 0, 64)
        same(mem.to_host(kb if in_b else ka, np.uint64)[:n], keys[order], "sort-pairs keys")
        same(mem.to_host(vb if in_b else va, np.uint32)[:n], order, "sort-pairs values")
        d_in, d_out, d_tot = mem.to_dev(x), mem.zeros(x.size, np.uint32), mem.zeros(1, np.uint32)
        mem.fill(d_out, 0x33)
        mem.fill(d_tot, 0x33)
        mem.sync()
        ctx.prim_exclusive_sum_dev(d_in, d_out, x.size, d_tot)
        same(mem.to_host(d_out, np.uint32), sums, "exclusive-sum")
        assert int(mem.to_host(d_tot, np.uint32)[0]) == int(x.sum())
        return True

    # ---- calls that fail ----------------------------------------------------------------------------------------------------
    def failures(self):
        """name -> run(ctx): a call outside its contract, which must fail with its code and nothing else"""
        return {
            "sa-build-symbol-beyond-sigma": lambda ctx: self._fails(lambda: ctx.sa_build(self._bad_text(7), 5), _lib.SX_E_ARG),
            "sa-build-interior-zero": lambda ctx: self._fails(lambda: ctx.sa_build(self._bad_text(0), 5), _lib.SX_E_ARG),
            "inverse-of-a-non-permutation": self._fail_inverse,
            "fasta-ends-in-a-header": self._fail_fasta,
            "fastq-empty-sequence": self._fail_fastq,
            "approx-search-capacity": lambda ctx: self._fail_capacity(ctx, False),
            "best-search-capacity": lambda ctx: self._fail_capacity(ctx, True),
            "packed-index-eight-letters": self._fail_packed,
        }

    @staticmethod
    def _fails(call, code):
        try:
            call()
        except api.StralgAmdError as e:
            assert "code %d" % code in str(e), e
            return True
        raise AssertionError("the call did not fail")

    def _bad_text(self, symbol):
        x = synth(self.s["dna_small"], 5, 2).copy()
        x[x.size // 2] = symbol
        return x

    def _fail_inverse(self, ctx):
        N = self.s["inverse"][0]
        x, sa, _, _, _ = self.inverse_text(N)
        bad = sa.copy()
        bad[5] = 0xFFFFFFF0  # a value beyond N: every form of the inverse counts it and stores nothing for it
        mem = self.mem
        d_bad, d_inv = mem.to_dev(bad), mem.zeros(N, np.uint32)
        mem.sync()
        return self._fails(lambda: ctx.sa_inverse_dev(d_bad, N, d_inv), _lib.SX_E_ARG)

    def _fail_fasta(self, ctx):
        data = b">one\nACGTACGT\nGGCC\n>two"  # (edge/ends-in-header of the fixture: no newline behind the last header)
        assert pyoracle.fasta_pack(np.frombuffer(data, np.uint8))[0]  # (the reference's verdict: malformed)
        return self._fails(lambda: ctx.fasta_records(data), _lib.SX_E_MALFORMED)

    def _fail_fastq(self, ctx):
        import fastq_cases
        data = b"@r0\nACGT\n+\nIIII\n@r1\n\n+\n\n@r2\nGG\n+\nII\n"
        assert fastq_cases.fastq_reference(data) is None  # (the contract's restatement: malformed)
        d_image = self.mem.to_dev(data)
        self.mem.sync()
        return self._fails(lambda: ctx.fastq_index_dev(d_image, len(data)), _lib.SX_E_MALFORMED)

    def _fail_capacity(self, ctx, best):
        """a hit buffer one short of what the count-only call asks for: SX_E_CAPACITY, the offsets written all the same"""
        x, sa, c, o, ro, pats, T = self.search_tables()
        mem = self.mem
        extra = (mem.zeros(T.count),) if best else ()
        call = ctx.bwt_best_search_dev if best else ctx.bwt_approx_search_dev
        d_ho = mem.zeros(T.count + 1, np.uint64)
        mem.sync()
        total = call(T.c, T.o, T.ro, T.N, T.sigma, T.pat, T.off, T.count, 2, *extra, d_ho)
        assert total > 1
        d_hits = mem.zeros(total * 32)
        mem.fill(d_ho, 0xEE)
        mem.sync()
        self._fails(lambda: call(T.c, T.o, T.ro, T.N, T.sigma, T.pat, T.off, T.count, 2, *extra, d_ho, d_hits, total - 1), _lib.SX_E_CAPACITY)
        assert int(mem.to_host(d_ho, np.uint64)[T.count]) == total
        return True

    def _fail_packed(self, ctx):
        fasta = b">wide\nACGTNRYKACGTNRYKMMAC\n"  # eight letters: one more than a nibble's codes hold beside the sentinel
        return self._fails(lambda: api.Index.from_fasta(fasta, ctx=ctx, compact=True, packed=True), _lib.SX_E_ARG)


# ---- the tests' bodies (one per test of the two files) ---------------------------------------------------------------------
def run_op(cases, ctx, name):
    assert cases.ops[name](ctx), name
    return invariant(ctx, name)


def check_dirty_workspace(cases, ctx):
    """every operation once, then every operation behind a scribble with each fill"""
    for name in cases.ops:
        run_op(cases, ctx, name)
    k = ctx.counters()
    # not vacuous: every slab is there to scribble on.  The child only ever sorts a reduced string that is in device memory
    # already: it has no use for the BWT slab (2) and the staging slab (5), the others it has
    assert all(k["slab_bytes"]) and k["has_child"], k
    assert all(k["child"]["slab_bytes"][i] for i in (0, 1, 3, 4, _lib.SLAB_CHAIN)), k
    for fill in FILLS:
        for name in cases.ops:
            ctx.scribble(fill)
            invariant(ctx, ("scribble", fill))
            try:
                run_op(cases, ctx, name)
            except AssertionError as e:
                raise AssertionError(("after scribble(0x%02X)" % fill, name, e))


def check_pairs(cases, make_ctx, first):
    """in one context: `first`, then each operation; then `first` on one context, each operation on another, `first` again"""
    ctx = make_ctx()
    try:
        for name in cases.ops:
            run_op(cases, ctx, first)
            run_op(cases, ctx, name)
    finally:
        ctx.close()
    one, two = make_ctx(), make_ctx()
    try:
        for name in cases.ops:
            run_op(cases, one, first)
            run_op(cases, two, name)
            run_op(cases, one, first)
    finally:
        one.close()
        two.close()


def check_after_failure(cases, ctx, failure):
    names = list(cases.ops)
    at = list(cases.failures()).index(failure)
    assert cases.failures()[failure](ctx), failure
    invariant(ctx, failure)
    for j in range(3):
        run_op(cases, ctx, names[(3 * at + 5 * j + 1) % len(names)])  # (three different ones: 5 and 14 are coprime)


def check_epoch_wrap(cases, ctx):
    """the epoch set to 2^24 - 1 - j for j around the epochs a build takes: the wrap falls behind, inside, at the end of and
    just past the DNA build; the byte text and the Fibonacci text (the child's wrap) follow.  A chained launch takes one
    epoch and the launches of a build follow from its text alone, so the three builds take the same P epochs of the context
    and C of its child every time: a counter set to 2^24 - 1 - j ends at that plus its count where the count is at most j,
    and at count - j (the launch behind 2^24 - 1 takes epoch 1) where it is more"""
    cases.sa_dna(ctx, seed=7)
    E = invariant(ctx)["chain_epoch"]
    assert E >= 4, E  # (a DNA build takes a round per bucket and pass at least)
    cases.sa_fibonacci(ctx)  # (the child exists from here on: the switch reaches it)
    k0 = invariant(ctx)
    cases.sa_dna(ctx, seed=8)
    cases.sa_bytes_induced(ctx)
    cases.sa_fibonacci(ctx)
    k1 = invariant(ctx)
    P, C = k1["chain_epoch"] - k0["chain_epoch"], k1["child"]["chain_epoch"] - k0["child"]["chain_epoch"]
    assert P > E and C >= 1, (E, P, C)  # (P: a DNA build of the same size and two more; C: the child's first launch is chained)

    def after(start, count, j):
        return start + count if count <= j else count - j

    for j in (0, E // 2, E - 1, E):
        start = EPOCH_LIMIT - 1 - j
        ctx.set_chain_epoch(start)
        ctx.scribble(0xFF)
        k = invariant(ctx, ("set", j))
        assert k["chain_epoch"] == start and k["child"]["chain_epoch"] == start and k["chain_slab_max_epoch"] == start, k
        cases.sa_dna(ctx, seed=8)
        invariant(ctx, ("dna", j))
        cases.sa_bytes_induced(ctx)
        invariant(ctx, ("bytes", j))
        cases.sa_fibonacci(ctx)
        k = invariant(ctx, ("fibonacci", j))
        assert 1 <= k["chain_epoch"] < start, (j, k)  # the wrap happened
        assert k["chain_epoch"] == after(start, P, j) == P - j, (j, P, k)
        # the child takes fewer epochs than the parent: it wraps for every j below them (j = 0 always: its first launch is
        # the wrap) and stops short of the limit otherwise
        child = k["child"]["chain_epoch"]
        assert child == after(start, C, j) and 1 <= child < EPOCH_LIMIT, (j, C, k)
        assert (child < start) == (C > j), (j, C, k)


def check_readback_sequence(cases, ctx):
    ctx.set_readback_seq(0xFFFFFFFD)
    assert ctx.counters()["readback_seq"] == 0xFFFFFFFD
    cases.sa_dna(ctx)  # (more than three read-backs: a pass reads its stop record back for every bucket region)
    k = invariant(ctx)
    assert 1 <= k["readback_seq"] < 1000, k


def regrowth_families(cases):
    """family -> (small call, large call), each against the oracle, the model or the recorded text.  A slab is a whole number
    of MiB, so the large call is one whose workspace passes the MiB of some slab that the small call took, or takes a slab
    that the small call had no use for (the three-pass inverse's pairs)"""
    s = cases.s
    return {
        "sa-build": (lambda ctx: cases.sa_dna(ctx, seed=5, n=s["dna_small"]), lambda ctx: cases.sa_dna(ctx, n=s["dna_large"])),
        "build-tables": (lambda ctx: cases.build_tables(ctx, (5, 21), s["tables_small"]), lambda ctx: cases.build_tables(ctx, (5, 21), s["tables_large"])),
        "inverse-lcp": (lambda ctx: cases.inverse_lcp(ctx, s["inverse"][:1]), lambda ctx: cases.inverse_lcp(ctx, s["inverse"][1:])),
        "approx-search": (lambda ctx: cases.approx_search_host(ctx, 1, s["search_small"]), lambda ctx: cases.approx_search_host(ctx, 2, s["search_large"])),
        # (the mapper's loop keeps its hits in allocations of its own, and the tables of map_text may come from a cache: the
        #  family goes from the FASTA to the text in the context, so that what grows is the context's own work)
        "map-reads": (lambda ctx: cases.map_index(ctx, 2, "test-out"), lambda ctx: cases.map_index(ctx, 1, s["map_large"])),
    }


def check_regrowth(cases, make_ctx, family):
    """small, large, small in a fresh context: some slab grows under the large call; then trim() and small once more.  The
    trim follows in the same context, not in a fresh one: what stands around it is small, trim, small all the same, and the
    small call behind the trim meets counters that have moved on and a child that has no slab left"""
    small, large = regrowth_families(cases)[family]
    ctx = make_ctx()
    try:
        assert small(ctx)
        before = invariant(ctx, (family, "small"))
        assert large(ctx)
        after = invariant(ctx, (family, "large"))
        grown = [a > b for a, b in zip(after["slab_bytes"], before["slab_bytes"])]
        assert any(grown), (family, before["slab_bytes"], after["slab_bytes"])
        assert small(ctx)
        invariant(ctx, (family, "small again"))
        ctx.trim()
        k = invariant(ctx, (family, "trim"))
        assert not any(k["slab_bytes"]) and not any(k["child"]["slab_bytes"]), k
        assert small(ctx)
        invariant(ctx, (family, "small after trim"))
    finally:
        ctx.close()


def check_interleaved(cases, make_ctx):
    """two contexts take the operations in opposite orders, turn by turn, on one thread"""
    one, two = make_ctx(), make_ctx()
    try:
        names = list(cases.ops)
        for a, b in zip(names, reversed(names)):
            run_op(cases, one, a)
            run_op(cases, two, b)
    finally:
        one.close()
        two.close()


def check_two_threads(cases, make_ctx):
    """two threads, a context each, the operations in opposite orders"""
    names = list(cases.ops)
    warm = make_ctx()  # (the inputs and expected values are made before the threads start)
    try:
        for name in names:
            run_op(cases, warm, name)
    finally:
        warm.close()
    errors = []

    def work(order):
        ctx = make_ctx()
        try:
            for name in order:
                run_op(cases, ctx, name)
        except BaseException as e:  # noqa: BLE001 -- reported by the test's thread
            errors.append((order[0], e))
        finally:
            ctx.close()

    threads = [threading.Thread(target=work, args=(order,)) for order in (names, names[::-1])]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
