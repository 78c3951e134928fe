"""The search without indels (SX_SEARCH_NO_INDELS, SX_MAP_NO_INDELS): its expected outputs as filters
of the reference's recorded ones (a path of the reference's search has a CIGAR of pure M exactly when it took no I or D
child), a sliding-window Hamming scan that knows nothing of the search, and the cases that the CPU-harness suite
(tests/test_hamming_cpu.py) and the GPU suite (tests/test_gpu_hamming.py) share.  `mem` is one of the two objects of
tests/device_memory.py.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import approx_model
import best_cases as bc
import occ_cases as oc
import packed_cases as pc
import strand_cases as sc
from approx_cases import approx_cases, remapped
from stralg_amd import _lib, api


# ---- the contract, restated -----------------------------------------------------------------------------------------------
def pure_stream(stream, m):
    """of a pattern's recorded (position, match_length, cigar) entries those whose CIGAR is "<m>M", in order"""
    return [(pos, ml, cigar) for pos, ml, cigar in stream if cigar == "%dM" % m]


def pure_text(sam):
    """of a SAM text the lines whose CIGAR is "<length of SEQ>M", in order"""
    out = []
    for line in sam.split(b"\n")[:-1]:
        f = line.split(b"\t")
        if f[5] == b"%dM" % len(f[9]):
            out.append(line)
    return b"".join(l + b"\n" for l in out)


def want_of(case, k, both, best):
    """the text of a mapping call with the flag on a case of best_cases(): every recorded text filtered, then the unchanged
    compositions"""
    fwd, rev = [pure_text(t) for t in case["fwd"]], [pure_text(t) for t in case["rev"]]
    if best:
        return bc.compose_best(case["fastq"], fwd, rev if both else None, k)
    return sc.compose(case["fastq"], fwd[k], rev[k]) if both else fwd[k]


def brute(sym, pattern, k):
    """the positions at which the pattern lies in sym with at most k mismatches, ascending, with the mismatches of each:
    (positions, distances)"""
    sym, pattern = np.asarray(sym, np.uint8), np.asarray(pattern, np.uint8)
    m = pattern.size
    if m == 0 or m > sym.size:
        return [], []
    windows = np.lib.stride_tricks.sliding_window_view(sym, m)
    d = (windows != pattern).sum(axis=1)
    at = np.nonzero(d <= k)[0]
    return at.tolist(), d[at].tolist()


def mismatches_in(case, mode="ro"):
    """hits with at least one mismatch among a case's filtered streams"""
    sym, _ = remapped(case["raw"])
    n = 0
    for p, stream in zip(case["patterns"], case["streams"][mode]):
        for pos, ml, _ in pure_stream(stream, len(p)):
            n += int((np.asarray(sym[pos:pos + ml]) != p).any())
    return n


# (name, k): each runs one strand and both, best off and on
MAP_CASES = [("two-records-best", 0), ("two-records-best", 1), ("two-records-best", 2), ("hg38/reads-100-10-0", 1), ("test-out", 2)]
MAP_PARAMS = [(n, k, both, best) for n, k in MAP_CASES for both in (False, True) for best in (False, True)]
MAP_IDS = ["%s/k%d/%s/%s" % (n, k, "both" if both else "one", "best" if best else "all") for n, k, both, best in MAP_PARAMS]
FORMS = [dict(), dict(compact=True), dict(compact=True, sa_sample=32), dict(compact=True, packed=True, sa_sample=32)]
FORM_IDS = ["full", "compact", "sampled", "packed-sampled"]
WINDOWS = [(1000, 0), (1 << 16, 7), (1 << 20, 1)]
ROOM_HITS = 1  # the room of a mapping call that has to grow it or halve its batches: a hit


# ---- the search calls -----------------------------------------------------------------------------------------------------
class Tables(bc.Tables):
    """best_cases.Tables with the calls of this mode"""

    def hamming(self, ctx, k, capacity=None):
        """(offsets, hits, the exception a too small capacity gave) of the search with indels=False: count-only, then emit"""
        return self._run(lambda *a: ctx.bwt_approx_search_dev(*a, indels=False), k, (), capacity)

    def best_hamming(self, ctx, k, capacity=None):
        d_stratum = self.mem.zeros(max(self.count, 1))
        self.mem.fill(d_stratum, 0x77)
        ho, hits, failure = self._run(lambda *a: ctx.bwt_best_search_dev(*a, indels=False), k, (d_stratum,), capacity)
        return self.mem.to_host(d_stratum)[:self.count], ho, hits, failure


def check_pure(hits, ho, lens):
    """what every hit of the mode looks like; queries ascend"""
    assert not hits["n_gaps"].any() and not hits["gap"].any()
    counts = np.diff(ho.astype(np.int64))
    assert (hits["query"] == np.repeat(np.arange(counts.size), counts)).all()
    assert (hits["match_length"] == np.repeat(np.asarray(lens), counts)).all()


def check_fixture_case(ctx, mem, cs, tables):
    """a case of golden_approx.npz, with and without RO: the filtered stream, in order; returns the hits' bytes"""
    sa, c, o, ro, sigma = tables
    lens = np.diff(cs["pat_off"])
    out = []
    for mode, r in (("ro", ro), ("noro", None)):
        T = Tables(mem, c, o, r, sigma, cs["pat"], cs["pat_off"])
        ho, hits, failure = T.hamming(ctx, cs["k"])
        assert failure is None
        got = api.approx_matches(hits, ho, lens, sa)
        assert got == [pure_stream(s, len(p)) for s, p in zip(cs["streams"][mode], cs["patterns"])], mode
        check_pure(hits, ho, lens)
        out.append((ho, hits))
    assert out[0][0].tolist() == out[1][0].tolist() and out[0][1].tobytes() == out[1][1].tobytes()  # (the D table changes nothing)
    return out[0]


def check_forms(ctx, mem, Index, cs, tables, want):
    """compact blocks (sigma <= 128) and packed blocks (sigma <= 8) return the full table's (offsets, hits) `want`, byte for
    byte, with and without the reverse blocks"""
    sa, c, o, ro, sigma = tables
    count = cs["pat_off"].size - 1
    d_pat, d_off = mem.to_dev(np.concatenate([cs["pat"], np.zeros(16, np.uint8)])), mem.to_dev(cs["pat_off"])
    forms = []
    if sigma <= 128:
        forms.append((oc.BothForms(ctx, Index, sa, c, o, ro, sigma), "comp", ctx.bwt_approx_search_compact_dev))
    if sigma <= pc.MAX_SIGMA:
        forms.append((pc.FullAndPacked(ctx, Index, sa, c, o, ro, sigma), "pk", ctx.bwt_approx_search_packed_dev))
    try:
        for pair, _, call in forms:
            for with_ro in (True, False):
                d_ho = mem.zeros(count + 1, np.uint64)
                mem.sync()
                args = (pair.rec.d_c, pair.occ.d_occ, pair.occ.d_rocc if with_ro else None, pair.N, sigma, d_pat, d_off, count, cs["k"], d_ho)
                total = call(*args, indels=False)
                d_hits = mem.zeros(max(total, 1) * 32)
                mem.sync()
                assert call(*args, d_hits, total, indels=False) == total
                assert mem.to_host(d_ho, np.uint64).tolist() == want[0].tolist()
                assert mem.to_host(d_hits)[:total * 32].tobytes() == want[1].tobytes()
    finally:
        for pair, _, _ in forms:
            pair.close()
    return len(forms)


def planted_patterns(rng, sym, sigma, k, count=24):
    """patterns of the text of length 1 .. 40 with up to k planted substitutions; the last two have their only mismatch at
    the first and at the last symbol"""
    n = sym.size
    pats = []
    for q in range(count):
        m = int(rng.integers(1, 40))
        a = int(rng.integers(0, n - m))
        p = sym[a:a + m].copy()
        for _ in range(int(rng.integers(0, k + 1))):
            p[int(rng.integers(0, m))] = int(rng.integers(1, sigma))
        pats.append(p)
    for at in (0, -1):
        a = int(rng.integers(0, n - 20))
        p = sym[a:a + 20].copy()
        p[at] = p[at] % (sigma - 1) + 1  # (another symbol of 1 .. sigma - 1)
        pats.append(p)
    return pats


def flat_of(pats):
    off = np.concatenate([[0], np.cumsum([p.size for p in pats])]).astype(np.uint32)
    return (np.concatenate(pats).astype(np.uint8) if off[-1] else np.zeros(0, np.uint8)), off


def positions_of(hits, ho, sa):
    """per pattern the sorted positions of its hits"""
    return [sorted(int(p) for h in hits[int(ho[q]):int(ho[q + 1])] for p in sa[int(h["L"]):int(h["R"])]) for q in range(ho.size - 1)]


RANDOM_SHAPES = [(3, 400), (5, 3000), (9, 1500)]


def check_random(ctx, mem, sigma, n):
    """random texts against the scan: positions as sorted lists per pattern (a duplicate shows), k = 0 .. 3"""
    rng = np.random.default_rng(100 * sigma + 7)
    sym = rng.integers(1, sigma, n).astype(np.uint8)
    sa, c, o, ro = approx_model.tables(sym, sigma)
    for k in range(4):
        pats = planted_patterns(rng, sym, sigma, k)
        flat, off = flat_of(pats)
        want = [brute(sym, p, k)[0] for p in pats]  # (sym lacks the terminator: no window holds it)
        assert sum(len(w) for w in want) >= len(pats)
        for r in (ro, None):
            ho, hits, failure = Tables(mem, c, o, r, sigma, flat, off).hamming(ctx, k)
            assert failure is None
            assert positions_of(hits, ho, sa) == want, (sigma, k, r is None)
            check_pure(hits, ho, np.diff(off))


def check_best(ctx, mem, cs, tables, k=2):
    """the best-stratum search with indels=False on a fixture case, with and without RO"""
    sa, c, o, ro, sigma = tables
    sym, _ = remapped(cs["raw"])
    lens = np.diff(cs["pat_off"])
    dist = [brute(sym, p, k)[1] for p in cs["patterns"]]
    want_s = [min(d) if d else 0xFF for d in dist]
    for r in (ro, None):
        T = Tables(mem, c, o, r, sigma, cs["pat"], cs["pat_off"])
        per_d = [T.hamming(ctx, d)[:2] for d in range(k + 1)]
        _, want_off, want_hits = bc.expected_best(per_d)
        strata, ho, hits, failure = T.best_hamming(ctx, k)
        assert failure is None
        assert strata.tolist() == want_s
        assert ho.tolist() == want_off.tolist() and hits.tobytes() == want_hits.tobytes()
        check_pure(hits, ho, lens)
        total = int(want_off[-1])
        if total:
            strata, ho, hits, failure = T.best_hamming(ctx, k, capacity=total - 1)
            assert failure is not None and "code %d" % _lib.SX_E_CAPACITY in str(failure)
            assert strata.tolist() == want_s and ho.tolist() == want_off.tolist()


# ---- the mapper -----------------------------------------------------------------------------------------------------------
def stream(ctx, records, fastq, k, both, best, indels=False, window=0, batch=0, room=0):
    """(chunks, map_stats) of map_reads_stream with the switches set, and every switch back at 0 behind it"""
    chunks = []
    ctx.set_sam_window_bytes(window)
    ctx.set_sam_batch_reads(batch)
    ctx.set_sam_room_hits(room)
    try:
        ctx.map_reads_stream(records, fastq, k, chunks.append, both_strands=both, best=best, indels=indels)
        return chunks, ctx.map_stats()
    finally:
        ctx.set_sam_window_bytes(0)
        ctx.set_sam_batch_reads(0)
        ctx.set_sam_room_hits(0)


def check_windows(ctx, records, case, window, batch):
    """two-records-best, k = 2, both strands, best off and on, in a room that every batch outgrows"""
    for best in (False, True):
        chunks, st = stream(ctx, records, case["fastq"], 2, True, best, window=window, batch=batch, room=ROOM_HITS)
        assert st["retries"] > 0, st
        assert max(len(x) for x in chunks) <= (window + 15) // 16 * 16
        bc.check_text(b"".join(chunks), want_of(case, 2, True, best))


def check_index_forms(ctx, Index, case, form):
    """a resident index in one of its forms: every combination of the flags at k = 2, and the plain text afterwards"""
    with Index.from_fasta(case["fasta"], ctx=ctx, **form) as idx:
        for both in (False, True):
            for best in (False, True):
                want = want_of(case, 2, both, best)
                bc.check_text(idx.map_reads(case["fastq"], 2, both_strands=both, best=best, indels=False), want)
        assert sum(n for _, n in idx.map_reads_discard(case["fastq"], 2, both_strands=True, best=True, indels=False)) == len(want)
        bc.check_text(idx.map_reads(case["fastq"], 2, both_strands=True), bc.plain_of(case, 2, True))  # (the plain call is what it was)
