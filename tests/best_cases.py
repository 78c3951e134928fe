"""Best-stratum mapping (SX_MAP_BEST_STRATUM, sx_bwt_best_search_dev, sx_patterns_select_dev): the
contract's composition written out over the reference mapper's recorded outputs at -d 0, 1, 2 (tests/golden/
golden_sam_best.npz, written by tests/golden/make_golden_sam_best.py, and the texts of golden_sam.npz and
golden_sam_strands.npz), and the kernel-level cases that the CPU-harness suite (tests/test_best_cpu.py) and the GPU suite
(tests/test_gpu_best.py) share.  `mem` is one of the two objects of tests/device_memory.py.  TEST INFRASTRUCTURE ONLY."""
import os

import numpy as np

import sam_kernel_cases as skc
from sam_cases import ROOT, sam_cases
from strand_cases import compose, fastq_reads, lines_of
from stralg_amd import _lib, api


# ---- the contract, restated -----------------------------------------------------------------------------------------------
def strata_of(fastq, fwd, rev, k):
    """per read in file order: the first d in 0 .. k whose recorded text(s) (fwd[d], and rev[d] on the rc image unless rev is
    None) have a line for its name, or None"""
    names = [r[0] for r in fastq_reads(fastq)]
    seen = [set(lines_of(fwd[d])) | (set(lines_of(rev[d])) if rev is not None else set()) for d in range(k + 1)]
    return [next((d for d in range(k + 1) if n in seen[d]), None) for n in names]


def compose_best(fastq, fwd, rev, k):
    """the contract's text: per read in file order the lines the plain call prints for it at edits = e*(read); with rev,
    those are the both-strands lines (the forward group, then the FLAG-16 group) at e*"""
    reads = fastq_reads(fastq)
    strata = strata_of(fastq, fwd, rev, k)
    plain = [compose(fastq, fwd[d], rev[d] if rev is not None else b"") for d in range(k + 1)]
    by_read = [lines_of(t) for t in plain]
    out = []
    for (name, _, _), e in zip(reads, strata):
        if e is not None:
            out += by_read[e][name]
    return b"".join(l + b"\n" for l in out)


# ---- the mapper's cases ---------------------------------------------------------------------------------------------------
# (name, k): each runs one-strand and both
BEST_CASES = [("two-records-best", 0), ("two-records-best", 1), ("two-records-best", 2), ("hg38/reads-100-10-0", 1), ("test-out", 2)]
BEST_IDS = ["%s/k%d/%s" % (n, k, "both" if both else "one") for n, k in BEST_CASES for both in (False, True)]
BEST_PARAMS = [(n, k, both) for n, k in BEST_CASES for both in (False, True)]


def best_cases():
    """name -> dict(fasta, fastq, fwd [texts at -d 0 ..], rev [texts on the rc image at -d 0 ..])"""
    base = sam_cases()
    z = np.load(os.path.join(ROOT, "tests", "golden", "golden_sam_best.npz"))
    strands = np.load(os.path.join(ROOT, "tests", "golden", "golden_sam_strands.npz"))
    name = "two-records-best"
    out = {name: dict(fasta=base[z[name + "/base"].tobytes().decode()]["fasta"], fastq=z[name + "/fastq"].tobytes(),
                      fwd=[z["%s/fwd%d" % (name, d)].tobytes() for d in range(3)], rev=[z["%s/rev%d" % (name, d)].tobytes() for d in range(3)])}
    for name, kmax in (("hg38/reads-100-10-0", 1), ("test-out", 2)):
        c0 = base[name + "/k0"]
        out[name] = dict(fasta=c0["fasta"], fastq=c0["fastq"], fwd=[base["%s/k%d" % (name, d)]["sam"] for d in range(kmax + 1)],
                         rev=[strands["%s/k%d/rev" % (name, d)].tobytes() for d in range(kmax + 1)])
        assert all(base["%s/k%d" % (name, d)]["fastq"] == c0["fastq"] for d in range(kmax + 1))
    return out


def want_of(case, k, both):
    return compose_best(case["fastq"], case["fwd"], case["rev"] if both else None, k)


def plain_of(case, k, both):
    """the text of the same call without the flag"""
    return compose(case["fastq"], case["fwd"][k], case["rev"][k]) if both else case["fwd"][k]


def check_text(got, want):
    assert len(got) == len(want), (len(got), len(want), skc.first_difference(got, want))
    assert got == want, skc.first_difference(got, want)


# ---- sx_patterns_select_dev -----------------------------------------------------------------------------------------------
def select_cases():
    """name -> dict(lengths, keep, shift: the source's first byte off a 16-byte boundary, base: the first offset)"""
    rng = np.random.default_rng(17)
    out = {}
    for n in (0, 1, 255, 256, 257):
        lengths = rng.integers(1, 40, n).tolist()
        for mode, keep in (("none", [0] * n), ("all", [1] * n), ("every-other", [q & 1 for q in range(n)]), ("last", [0] * max(n - 1, 0) + [7] * min(n, 1))):
            out["%d-patterns/keep-%s" % (n, mode)] = dict(lengths=lengths, keep=keep, shift=0, base=0)
    edges = [1, 15, 16, 17, 2046, 1, 16, 2046, 17, 15, 1]
    out["edge-lengths/keep-all"] = dict(lengths=edges, keep=[1] * len(edges), shift=0, base=0)
    out["edge-lengths/keep-every-other"] = dict(lengths=edges, keep=[(q + 1) & 1 for q in range(len(edges))], shift=0, base=0)
    out["edge-lengths/keep-the-others"] = dict(lengths=edges, keep=[q & 1 for q in range(len(edges))], shift=0, base=0)
    # kept bytes 4086 .. 4106 are one pattern's: it lies across the first tile's edge; so does one across 8192, and the
    # patterns dropped in front of them put source and output out of step
    tile = [2046, 9, 2040, 5, 20, 2046, 3, 2046, 30, 100]
    out["across-a-tile-edge"] = dict(lengths=tile, keep=[1, 0, 1, 0, 1, 1, 0, 1, 1, 1], shift=0, base=0)
    out["across-a-tile-edge/keep-all"] = dict(lengths=tile, keep=[1] * len(tile), shift=0, base=0)
    mixed = rng.integers(1, 300, 70).tolist()
    out["source-shifted"] = dict(lengths=mixed, keep=(rng.integers(0, 3, 70) > 0).astype(int).tolist(), shift=5, base=0)
    out["offsets-from-the-middle"] = dict(lengths=mixed, keep=(rng.integers(0, 2, 70)).tolist(), shift=3, base=1237)
    return out


SELECT_NAMES = list(select_cases())


def check_select(ctx, mem, case):
    """kept count, offsets, ids and bytes against a Python list comprehension; the 16 spare bytes zero; a second run the same"""
    lengths, keep, base = case["lengths"], case["keep"], case["base"]
    n = len(lengths)
    rng = np.random.default_rng(n + base)
    pats = [bytes(rng.integers(1, 256, m, dtype=np.uint8).tolist()) for m in lengths]
    data = bytes(rng.integers(1, 256, base, dtype=np.uint8).tolist()) + b"".join(pats)
    off = (np.concatenate([[0], np.cumsum(lengths)]) + base).astype(np.uint32)
    kept = [q for q in range(n) if keep[q]]
    want = b"".join(pats[q] for q in kept)
    want_off = np.concatenate([[0], np.cumsum([lengths[q] for q in kept])]).astype(np.uint32)
    d_bytes, d_off, d_keep = mem.to_dev(data, case["shift"]), mem.to_dev(off), mem.to_dev(np.asarray(keep, np.uint8))
    results = []
    for fill in (0xEE, 0x55):
        d_out, d_off_out, d_ids = mem.zeros(len(data) - base + 16), mem.zeros(n + 1, np.uint32), mem.zeros(max(n, 1), np.uint32)
        for b in (d_out, d_off_out, d_ids):
            mem.fill(b, fill)
        mem.sync()
        got_n, got_bytes = ctx.patterns_select_dev(d_bytes, d_off, n, d_keep, d_out, d_off_out, d_ids)
        assert (got_n, got_bytes) == (len(kept), len(want))
        assert mem.to_host(d_off_out, np.uint32)[:got_n + 1].tolist() == want_off.tolist()
        assert mem.to_host(d_ids, np.uint32)[:got_n].tolist() == kept
        out = mem.to_host(d_out)
        assert out[:got_bytes].tobytes() == want, skc.first_difference(out[:got_bytes].tobytes(), want)
        assert not out[got_bytes:got_bytes + 16].any()  # the spare bytes
        assert (out[got_bytes + 16:] == fill).all()  # and nothing behind them
        results.append(out[:got_bytes + 16].tobytes())
    assert results[0] == results[1]


# ---- sx_bwt_best_search_dev -----------------------------------------------------------------------------------------------
class Tables:
    """a text's tables and a pattern set in device memory"""

    def __init__(self, mem, c, o, ro, sigma, pat, off):
        self.mem, self.N, self.sigma, self.count = mem, o.shape[0] - 1, sigma, off.size - 1
        self.c, self.o = mem.to_dev(np.ascontiguousarray(c, np.uint32)), mem.to_dev(np.ascontiguousarray(o, np.uint32))
        self.ro = None if ro is None else mem.to_dev(np.ascontiguousarray(ro, np.uint32))
        self.pat = mem.to_dev(np.ascontiguousarray(pat, np.uint8) if len(pat) else np.zeros(1, np.uint8))
        self.off = mem.to_dev(np.ascontiguousarray(off, np.uint32))
        mem.sync()

    def _run(self, call, k, extra, capacity):
        mem = self.mem
        d_ho = mem.zeros(self.count + 1, np.uint64)
        mem.sync()
        total = call(self.c, self.o, self.ro, self.N, self.sigma, self.pat, self.off, self.count, k, *extra, d_ho)
        d_hits = mem.zeros(max(total, 1) * 32)
        for b in (d_ho,) + tuple(extra):  # (the second call writes offsets and strata again, also where it ends with SX_E_CAPACITY)
            mem.fill(b, 0xEE)
        mem.sync()
        failure = None
        try:
            again = call(self.c, self.o, self.ro, self.N, self.sigma, self.pat, self.off, self.count, k, *extra, d_ho, d_hits,
                         total if capacity is None else capacity)
            assert again == total
        except api.StralgAmdError as e:
            failure = e
        return mem.to_host(d_ho, np.uint64), mem.to_host(d_hits).view(_lib.APPROX_HIT_DTYPE)[:total], failure

    def approx(self, ctx, k):
        """(offsets, hits) of sx_bwt_approx_search_dev"""
        ho, hits, failure = self._run(ctx.bwt_approx_search_dev, k, (), None)
        assert failure is None
        return ho, hits

    def best(self, ctx, k, capacity=None):
        """(strata, offsets, hits, the exception a too small capacity gave) of sx_bwt_best_search_dev: count-only, then emit"""
        d_stratum = self.mem.zeros(max(self.count, 1))
        self.mem.fill(d_stratum, 0x77)
        ho, hits, failure = self._run(ctx.bwt_best_search_dev, k, (d_stratum,), capacity)
        return self.mem.to_host(d_stratum)[:self.count], ho, hits, failure


def expected_best(per_d):
    """from [(offsets, hits) of the plain search at d = 0 ..]: (strata, offsets, hits) of the best-stratum search"""
    count = per_d[0][0].size - 1
    strata, chunks, sizes = [], [], []
    for q in range(count):
        e = next((d for d, (ho, _) in enumerate(per_d) if ho[q + 1] > ho[q]), None)
        strata.append(0xFF if e is None else e)
        if e is not None:
            ho, hits = per_d[e]
            chunks.append(hits[int(ho[q]):int(ho[q + 1])])
        sizes.append(0 if e is None else len(chunks[-1]))
    hits = np.concatenate(chunks) if chunks else np.zeros(0, _lib.APPROX_HIT_DTYPE)
    return np.array(strata, np.uint8), np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64), hits


def check_best_search(ctx, T, k):
    """strata, offsets and hits against the plain search at every d; the count-only form; a capacity one short.  Returns
    (strata, offsets, hits, [the plain searches])"""
    per_d = [T.approx(ctx, d) for d in range(k + 1)]
    want_s, want_off, want_hits = expected_best(per_d)
    strata, ho, hits, failure = T.best(ctx, k)
    assert failure is None
    assert strata.tolist() == want_s.tolist()
    assert ho.tolist() == want_off.tolist()
    assert hits.tobytes() == want_hits.tobytes()
    total = int(want_off[-1])
    if total:
        strata, ho, hits, failure = T.best(ctx, k, capacity=total - 1)
        assert failure is not None and "code %d" % _lib.SX_E_CAPACITY in str(failure)
        assert strata.tolist() == want_s.tolist() and ho.tolist() == want_off.tolist()
    return want_s, want_off, want_hits, per_d
