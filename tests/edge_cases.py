"""Edge-case genomes through every flag and form of the read mapper: three recorded inputs
(tests/golden/golden_sam_edges.npz, written by tests/golden/make_golden_sam_edges.py: inputs and the reference mapper's stdout
at -d 0 .. K on the FASTQ image and on its rc image) and the expected text of every call, composed only from the
restatements that the other suites already use.  Shared by the CPU-harness suite (tests/test_edges_cpu.py) and the GPU suite
(tests/test_gpu_edges.py).  TEST INFRASTRUCTURE ONLY.

Out of scope: duplicate read names.  Every oracle below keys a read's lines on its name (strand_cases.lines_of), so two reads
of one name cannot be told apart; the generator asserts that the names are unique."""
import os
import re

import numpy as np

import best_cases as bc
import hamming_cases as hc
import mapq_cases as mc
import pairs_cases as pc
import strand_cases as sc
import tags_cases as tc
import unmapped_cases as uc
from sam_cases import ROOT

# name -> K: texts are recorded at -d 0 .. K
CASES = {"many-records": 3, "block-edges": 1, "deep-k": 8}
FIXTURE = os.path.join(ROOT, "tests", "golden", "golden_sam_edges.npz")


def edge_cases():
    """name -> dict(fasta, fastq, fwd [texts at -d 0 ..], rev [texts on the rc image at -d 0 ..]), as best_cases.best_cases()"""
    z = np.load(FIXTURE)
    return {name: dict(fasta=z[name + "/fasta"].tobytes(), fastq=z[name + "/fastq"].tobytes(),
                       fwd=[z["%s/fwd%d" % (name, d)].tobytes() for d in range(K + 1)],
                       rev=[z["%s/rev%d" % (name, d)].tobytes() for d in range(K + 1)]) for name, K in CASES.items()}


# ---- the expected text ------------------------------------------------------------------------------------------------------
def want(case, k, both=False, best=False, indels=True, tags=False, unmapped=False, header=False, mapq=False):
    """the text of a mapping call, in the contract's order: the recorded texts filtered to pure M (indels=False), composed
    over strands and strata, the FLAG 4 lines put in, FLAG and MAPQ rewritten, the tags appended to every mapped line, the
    header in front"""
    fwd, rev = case["fwd"], case["rev"]
    if not indels:
        fwd, rev = [hc.pure_text(t) for t in fwd], [hc.pure_text(t) for t in rev]
    if best:
        text = bc.compose_best(case["fastq"], fwd, rev if both else None, k)
    else:
        text = sc.compose(case["fastq"], fwd[k], rev[k]) if both else fwd[k]
    if unmapped:
        text, _ = uc.with_unmapped(case["fastq"], text)
    if mapq:
        assert best
        plain = text
        text, _ = mc.with_mapq(case["fastq"], plain)
        assert mc.without_mapq(text) == plain
    if tags:
        letters = tc.fasta_letters(case["fasta"])
        text = b"".join(l + b"\n" if l.split(b"\t")[1] == b"4" else tc.tag_line(l, letters) + b"\n" for l in text.split(b"\n")[:-1])
    return (uc.header_of(case["fasta"]) if header else b"") + text


# the flag sets of the suites: every case runs each at every recorded k
ALL = dict(both=True, best=True, indels=False, tags=True, unmapped=True, header=True, mapq=True)
ALL_INDELS = dict(both=True, best=True, tags=True, unmapped=True, mapq=True)
FLAG_SETS = {"plain": dict(), "both": dict(both=True), "best": dict(best=True), "both-best": dict(both=True, best=True),
             "no-indels": dict(indels=False), "all": ALL, "all-indels": ALL_INDELS}
STREAMED = ["plain", "both", "best"]  # these also go through the stream entry (the others need an index, or say nothing new)
SWITCHES = dict(both=True, best=True, unmapped=True, mapq=True)  # the call of the loop's switches, at k = 2 on many-records


def call_flags(both=False, best=False, indels=True, tags=False, unmapped=False, header=False, mapq=False):
    """the flags of want() under the names of Index.map_reads"""
    return dict(both_strands=both, best=best, indels=indels, tags=tags, unmapped=unmapped, header=header, mapq=mapq)


def counts_of(text):
    """(lines, FLAG 16 lines, FLAG 4 lines, secondary lines) of a text, header lines left out"""
    flags = [int(l.split(b"\t")[1]) for l in text.split(b"\n")[:-1] if not re.match(rb"@(HD|SQ)\t", l)]
    return len(flags), sum(1 for f in flags if f & 16), sum(1 for f in flags if f == 4), sum(1 for f in flags if f & 256)


# (case, k, flag set) -> (lines, FLAG 16 lines, FLAG 4 lines, secondary lines): the counts that the generator printed
TABLE = {
    ('many-records', 0, 'plain'): (11, 0, 0, 0), ('many-records', 0, 'both'): (14, 3, 0, 0), ('many-records', 0, 'best'): (11, 0, 0, 0), ('many-records', 0, 'both-best'): (14, 3, 0, 0), ('many-records', 0, 'no-indels'): (11, 0, 0, 0), ('many-records', 0, 'all'): (48, 3, 34, 0), ('many-records', 0, 'all-indels'): (48, 3, 34, 0),
    ('many-records', 1, 'plain'): (69, 0, 0, 0), ('many-records', 1, 'both'): (97, 28, 0, 0), ('many-records', 1, 'best'): (39, 0, 0, 0), ('many-records', 1, 'both-best'): (52, 13, 0, 0), ('many-records', 1, 'no-indels'): (19, 0, 0, 0), ('many-records', 1, 'all'): (49, 6, 24, 1), ('many-records', 1, 'all-indels'): (69, 13, 17, 21),
    ('many-records', 2, 'plain'): (885, 0, 0, 0), ('many-records', 2, 'both'): (1249, 364, 0, 0), ('many-records', 2, 'best'): (82, 0, 0, 0), ('many-records', 2, 'both-best'): (70, 16, 0, 0), ('many-records', 2, 'no-indels'): (64, 0, 0, 0), ('many-records', 2, 'all'): (55, 10, 13, 7), ('many-records', 2, 'all-indels'): (76, 16, 6, 28),
    ('many-records', 3, 'plain'): (7788, 0, 0, 0), ('many-records', 3, 'both'): (12594, 4806, 0, 0), ('many-records', 3, 'best'): (155, 0, 0, 0), ('many-records', 3, 'both-best'): (111, 29, 0, 0), ('many-records', 3, 'no-indels'): (288, 0, 0, 0), ('many-records', 3, 'all'): (65, 17, 4, 17), ('many-records', 3, 'all-indels'): (114, 29, 3, 66),
    ('block-edges', 0, 'plain'): (143, 0, 0, 0), ('block-edges', 0, 'both'): (259, 116, 0, 0), ('block-edges', 0, 'best'): (143, 0, 0, 0), ('block-edges', 0, 'both-best'): (259, 116, 0, 0), ('block-edges', 0, 'no-indels'): (143, 0, 0, 0), ('block-edges', 0, 'all'): (269, 116, 10, 227), ('block-edges', 0, 'all-indels'): (269, 116, 10, 227),
    ('block-edges', 1, 'plain'): (3007, 0, 0, 0), ('block-edges', 1, 'both'): (5902, 2895, 0, 0), ('block-edges', 1, 'best'): (156, 0, 0, 0), ('block-edges', 1, 'both-best'): (272, 116, 0, 0), ('block-edges', 1, 'no-indels'): (1261, 0, 0, 0), ('block-edges', 1, 'all'): (269, 116, 9, 227), ('block-edges', 1, 'all-indels'): (272, 116, 0, 230),
    ('deep-k', 0, 'plain'): (5, 0, 0, 0), ('deep-k', 0, 'both'): (10, 5, 0, 0), ('deep-k', 0, 'best'): (5, 0, 0, 0), ('deep-k', 0, 'both-best'): (10, 5, 0, 0), ('deep-k', 0, 'no-indels'): (5, 0, 0, 0), ('deep-k', 0, 'all'): (14, 5, 4, 7), ('deep-k', 0, 'all-indels'): (14, 5, 4, 7),
    ('deep-k', 1, 'plain'): (32, 0, 0, 0), ('deep-k', 1, 'both'): (64, 32, 0, 0), ('deep-k', 1, 'best'): (5, 0, 0, 0), ('deep-k', 1, 'both-best'): (10, 5, 0, 0), ('deep-k', 1, 'no-indels'): (13, 0, 0, 0), ('deep-k', 1, 'all'): (14, 5, 4, 7), ('deep-k', 1, 'all-indels'): (14, 5, 4, 7),
    ('deep-k', 2, 'plain'): (122, 0, 0, 0), ('deep-k', 2, 'both'): (259, 137, 0, 0), ('deep-k', 2, 'best'): (38, 0, 0, 0), ('deep-k', 2, 'both-best'): (95, 57, 0, 0), ('deep-k', 2, 'no-indels'): (26, 0, 0, 0), ('deep-k', 2, 'all'): (26, 13, 1, 19), ('deep-k', 2, 'all-indels'): (96, 57, 1, 89),
    ('deep-k', 3, 'plain'): (388, 0, 0, 0), ('deep-k', 3, 'both'): (816, 428, 0, 0), ('deep-k', 3, 'best'): (68, 0, 0, 0), ('deep-k', 3, 'both-best'): (95, 57, 0, 0), ('deep-k', 3, 'no-indels'): (33, 0, 0, 0), ('deep-k', 3, 'all'): (26, 13, 1, 19), ('deep-k', 3, 'all-indels'): (96, 57, 1, 89),
    ('deep-k', 4, 'plain'): (964, 0, 0, 0), ('deep-k', 4, 'both'): (2071, 1107, 0, 0), ('deep-k', 4, 'best'): (68, 0, 0, 0), ('deep-k', 4, 'both-best'): (95, 57, 0, 0), ('deep-k', 4, 'no-indels'): (38, 0, 0, 0), ('deep-k', 4, 'all'): (26, 13, 1, 19), ('deep-k', 4, 'all-indels'): (96, 57, 1, 89),
    ('deep-k', 5, 'plain'): (1965, 0, 0, 0), ('deep-k', 5, 'both'): (4140, 2175, 0, 0), ('deep-k', 5, 'best'): (68, 0, 0, 0), ('deep-k', 5, 'both-best'): (95, 57, 0, 0), ('deep-k', 5, 'no-indels'): (38, 0, 0, 0), ('deep-k', 5, 'all'): (26, 13, 1, 19), ('deep-k', 5, 'all-indels'): (96, 57, 1, 89),
    ('deep-k', 6, 'plain'): (3367, 0, 0, 0), ('deep-k', 6, 'both'): (6880, 3513, 0, 0), ('deep-k', 6, 'best'): (68, 0, 0, 0), ('deep-k', 6, 'both-best'): (95, 57, 0, 0), ('deep-k', 6, 'no-indels'): (38, 0, 0, 0), ('deep-k', 6, 'all'): (26, 13, 1, 19), ('deep-k', 6, 'all-indels'): (96, 57, 1, 89),
    ('deep-k', 7, 'plain'): (5039, 0, 0, 0), ('deep-k', 7, 'both'): (10051, 5012, 0, 0), ('deep-k', 7, 'best'): (68, 0, 0, 0), ('deep-k', 7, 'both-best'): (95, 57, 0, 0), ('deep-k', 7, 'no-indels'): (38, 0, 0, 0), ('deep-k', 7, 'all'): (26, 13, 1, 19), ('deep-k', 7, 'all-indels'): (96, 57, 1, 89),
    ('deep-k', 8, 'plain'): (6616, 0, 0, 0), ('deep-k', 8, 'both'): (13089, 6473, 0, 0), ('deep-k', 8, 'best'): (68, 0, 0, 0), ('deep-k', 8, 'both-best'): (95, 57, 0, 0), ('deep-k', 8, 'no-indels'): (38, 0, 0, 0), ('deep-k', 8, 'all'): (26, 13, 1, 19), ('deep-k', 8, 'all-indels'): (96, 57, 1, 89),
}

# (case, k, best, indels) -> (lines, pairs with lines) of Index.map_pairs: image 2 is the rc of image 1, insert window [0, 5000]
PAIRS = {
    ('many-records', 1, True, False): (50, 24),
    ('many-records', 2, True, False): (84, 35),
    ('block-edges', 1, True, False): (11658, 33),
}
INSERT = (0, 5000)


def check_table(cases):
    """the oracle's own counts for every row (no case passes on an empty or an unchanged text); with_unmapped and with_mapq
    invert"""
    assert sorted(TABLE) == sorted((n, k, f) for n, K in CASES.items() for k in range(K + 1) for f in FLAG_SETS)
    for (name, k, flags), row in TABLE.items():
        c = cases[name]
        text = want(c, k, **FLAG_SETS[flags])
        assert counts_of(text) == row, (name, k, flags, counts_of(text))
        assert row[0] > 0
    for name, K in CASES.items():
        c = cases[name]
        plain = want(c, K, both=True, best=True)
        filled, added = uc.with_unmapped(c["fastq"], plain)
        assert added == TABLE[name, K, "all-indels"][2]
        assert b"".join(l + b"\n" for l in filled.split(b"\n")[:-1] if l.split(b"\t")[1] != b"4") == plain
        text, n = mc.with_mapq(c["fastq"], filled)
        assert mc.without_mapq(text) == filled and text != filled
        assert n["secondary"] == TABLE[name, K, "all-indels"][3] and n["lines"] == plain.count(b"\n")


def pair_case(case, k, best, indels):
    """dict(fastq1, fastq2, k, lo, hi, want, pairs) in the shape of pairs_cases.pair_case: the "overlap" selection (mate 2 of
    pair p is rc(read p)) over the both-strands lines of the same call"""
    both = want(case, k, both=True, best=best, indels=indels)
    fastq2, text, pairs = pc.paired(case["fastq"], both, "overlap", *INSERT)
    assert fastq2 == sc.rc_fastq(case["fastq"])
    return dict(fasta=case["fasta"], fastq1=case["fastq"], fastq2=fastq2, k=k, lo=INSERT[0], hi=INSERT[1], want=text, pairs=pairs)


def check_pairs_table(cases):
    for (name, k, best, indels), row in PAIRS.items():
        p = pair_case(cases[name], k, best, indels)
        assert (p["want"].count(b"\n"), p["pairs"]) == row and row[0] > 0, (name, k, best, indels, p["want"].count(b"\n"), p["pairs"])


# ---- what the recordings have to cover ------------------------------------------------------------------------------------
def gap_runs(cigar):
    return len(re.findall(rb"\d+[ID]", cigar))


def records_of(fasta):
    """[(RNAME, letters)] in file order"""
    return list(tc.fasta_letters(fasta).items())


def coverage(cases):
    """asserts the conditions of DESIGN.md section 24 on the recorded texts and returns what it counted"""
    seen = {}
    c = cases["many-records"]
    K = CASES["many-records"]
    assert len(records_of(c["fasta"])) == 69
    for both in (False, True):
        strata = bc.strata_of(c["fastq"], c["fwd"], c["rev"] if both else None, K)
        n = {e: strata.count(e) for e in (0, 1, 2, 3, None)}
        assert min(n.values()) >= 3, (both, n)
        seen["strata-both" if both else "strata-one"] = n
    _, n = mc.with_mapq(c["fastq"], want(c, K, both=True, best=True))
    assert min(n["groups"].values()) >= 1, n["groups"]
    seen["mapq-groups"] = n["groups"]
    plain = want(c, K, both=True)
    fields = [l.split(b"\t") for l in plain.split(b"\n")[:-1]]
    rnames = {}
    for f in fields:
        rnames.setdefault(f[0], set()).add(f[2])
    seen["reads-in-three-records"] = sum(1 for r in rnames.values() if len(r) >= 3)
    assert seen["reads-in-three-records"] >= 1
    # a read that lacks a letter in some records and has lines in another
    letters = dict(records_of(c["fasta"]))
    seen["reads-lacking-letters"] = 0
    for name, seq, _ in sc.fastq_reads(c["fastq"]):
        lacking = [r for r, t in letters.items() if not set(seq) <= set(t)]
        if lacking and rnames.get(name) and not rnames[name] <= set(lacking):
            seen["reads-lacking-letters"] += 1
    assert seen["reads-lacking-letters"] >= 1
    seen["flag16"] = sum(1 for f in fields if f[1] == b"16")
    seen["cigar-I"] = sum(1 for f in fields if b"I" in f[5])
    seen["cigar-D"] = sum(1 for f in fields if b"D" in f[5])
    seen["two-gap-runs"] = sum(1 for f in fields if gap_runs(f[5]) >= 2)
    assert min(seen["flag16"], seen["cigar-I"], seen["cigar-D"], seen["two-gap-runs"]) >= 1, seen
    text = want(c, K, both=True, unmapped=True)
    assert text.split(b"\n")[0].split(b"\t")[1] == b"4" and text.split(b"\n")[-2].split(b"\t")[1] == b"4"  # unmapped first and last

    c = cases["block-edges"]
    lengths = dict((r, len(t)) for r, t in records_of(c["fasta"]))
    assert sorted(lengths.values()) == [1, 2, 62, 63, 64, 126, 127, 128, 700, 1023, 1024, 5000]
    fields = [l.split(b"\t") for l in c["fwd"][1].split(b"\n")[:-1]]
    first = {lengths[f[2]] for f in fields if f[3] == b"1"}
    last = {lengths[f[2]] for f in fields if int(f[3]) - 1 + pc.span_of(f[5]) == lengths[f[2]]}
    edges = {62, 63, 64, 126, 127, 128, 1023, 1024}
    assert edges <= first and edges <= last, (sorted(first), sorted(last))
    seen["pos-1-records"], seen["last-symbol-records"] = sorted(first), sorted(last)
    by = sc.lines_of(c["fwd"][1])
    reads = sc.fastq_reads(c["fastq"])
    longer = [r for r in reads if r[0].startswith(b"longer-")]
    assert len(longer) == 9
    for name, seq, _ in longer:
        cigars = [l.split(b"\t")[5] for l in by[name]]
        assert cigars and all(b"I" in g and b"D" not in g for g in cigars), (name, cigars)
        assert name not in sc.lines_of(c["fwd"][0])
    seen["longer-read-lines"] = sum(len(by[r[0]]) for r in longer)
    long_reads = [r for r in reads if len(r[1]) == 2046]
    assert len(long_reads) == 2 and all(r[0] in by for r in long_reads) and long_reads[0][0] in sc.lines_of(c["fwd"][0])
    assert long_reads[1][0] not in sc.lines_of(c["fwd"][0])
    assert max(len(r[0]) for r in reads) == 2045
    seen["longest-line"] = max(len(l) for l in want(c, 1, **ALL_INDELS).split(b"\n"))

    c = cases["deep-k"]
    assert [t for _, t in records_of(c["fasta"])] == [b"ACGTTGCA", b"TT"]
    by = sc.lines_of(c["fwd"][8])
    seen["deep-k-acg-tt-lines"] = sum(len(by[r[0]]) for r in sc.fastq_reads(c["fastq"]) if r[1] in (b"ACG", b"TT"))
    assert seen["deep-k-acg-tt-lines"] == 880
    seen["deep-k-most-gap-runs"] = max(gap_runs(l.split(b"\t")[5]) for l in c["fwd"][8].split(b"\n")[:-1])
    for case in cases.values():
        names = [r[0] for r in sc.fastq_reads(case["fastq"])]
        assert len(set(names)) == len(names)
    return seen


# ---- the calls both suites make -----------------------------------------------------------------------------------------
KS = [(name, k) for name, K in CASES.items() for k in range(K + 1)]
KS_IDS = ["%s/k%d" % nk for nk in KS]
FORMS = {"full": dict(), "compact": dict(compact=True), "sampled-2": dict(compact=True, sa_sample=2),
         "sampled-1024": dict(compact=True, sa_sample=1024), "packed-32": dict(compact=True, packed=True, sa_sample=32),
         "packed-1024": dict(compact=True, packed=True, sa_sample=1024)}
MANY_FORMS = ["full", "compact", "sampled-1024"]  # (the protein record has more letters than a packed index takes)


class switched:
    """sets the loop's switches and puts them back at 0"""

    def __init__(self, ctx, window=0, batch=0, room=0, locate=0):
        self.ctx, self.values = ctx, (window, batch, room, locate)

    def _set(self, window, batch, room, locate):
        self.ctx.set_sam_window_bytes(window)
        self.ctx.set_sam_batch_reads(batch)
        self.ctx.set_sam_room_hits(room)
        self.ctx.set_locate_chunk_rows(locate)

    def __enter__(self):
        self._set(*self.values)

    def __exit__(self, *exc):
        self._set(0, 0, 0, 0)


def check_flag_sets(ctx, idx, stream, case, name, k):
    """every flag set through the resident index `idx`, the first three also through stream(case, k, **call flags); the
    table's counts on what came back; no retry at the default room"""
    for f, flags in FLAG_SETS.items():
        text = want(case, k, **flags)
        got = idx.map_reads(case["fastq"], k, **call_flags(**flags))
        assert ctx.map_stats()["retries"] == 0, (f, ctx.map_stats())
        bc.check_text(got, text)
        assert counts_of(got) == TABLE[name, k, f], f
        if f in STREAMED:
            bc.check_text(stream(case, k, **call_flags(**flags)), text)
            assert ctx.map_stats()["retries"] == 0, (f, ctx.map_stats())


def check_form(idx, case, name):
    """plain at every k and the all-flags call at the largest"""
    K = CASES[name]
    for k in range(K + 1):
        bc.check_text(idx.map_reads(case["fastq"], k), case["fwd"][k])
    bc.check_text(idx.map_reads(case["fastq"], K, **call_flags(**ALL)), want(case, K, **ALL))


def check_packed_refused(ctx, Index, case):
    """the protein record does not fit a packed index: SX_E_ARG, and the context builds and maps the full form afterwards"""
    from stralg_amd import api
    try:
        Index.from_fasta(case["fasta"], ctx=ctx, compact=True, packed=True, sa_sample=32).close()
    except api.StralgAmdError as e:
        assert "code -1" in str(e), e
    else:
        raise AssertionError("a record of 20 letters was packed")
    with Index.from_fasta(case["fasta"], ctx=ctx) as idx:
        bc.check_text(idx.map_reads(case["fastq"], 2, **call_flags(**ALL)), want(case, 2, **ALL))


def check_batches(ctx, idx, case, batch):
    reads = len(sc.fastq_reads(case["fastq"]))
    with switched(ctx, batch=batch):
        bc.check_text(idx.map_reads(case["fastq"], 2, **call_flags(**SWITCHES)), want(case, 2, **SWITCHES))
        # (a batch counts the reads of the search: with both strands two a read, and an odd number is rounded up to whole groups)
        assert ctx.map_stats()["batches"] == -(-2 * reads // (batch + batch % 2))


def check_sixteen_byte_windows(ctx, idx, case):
    chunks = []
    with switched(ctx, window=16):
        idx.map_reads(case["fastq"], 2, sink=chunks.append, **call_flags(**SWITCHES))
    assert max(len(x) for x in chunks) <= 16
    bc.check_text(b"".join(chunks), want(case, 2, **SWITCHES))


def check_room_of_one_hit(ctx, idx, case):
    with switched(ctx, room=1, window=1000):
        got = idx.map_reads(case["fastq"], 2, **call_flags(**SWITCHES))
        st = ctx.map_stats()
    assert st["retries"] > 0 and st["halved"] > 0, st
    bc.check_text(got, want(case, 2, **SWITCHES))


def check_located_in_runs_of_five(ctx, idx, case):
    with switched(ctx, locate=5):
        bc.check_text(idx.map_reads(case["fastq"], 2, **call_flags(**SWITCHES)), want(case, 2, **SWITCHES))


def check_longest_reads(ctx, idx, case, window):
    """the two reads of 2046 symbols alone, with tags: lines of 4 KB and an MD walk over 2046 symbols, cut by the windows"""
    reads = [r for r in sc.fastq_reads(case["fastq"]) if len(r[1]) == 2046]
    names = {r[0] for r in reads}
    assert len(reads) == 2
    text = b"".join(l + b"\n" for l in want(case, 1, tags=True).split(b"\n")[:-1] if l.split(b"\t", 1)[0] in names)
    assert text.count(b"\n") >= 2 and b"MD:Z:1023" in text and min(len(l) for l in text.split(b"\n")[:-1]) > 4096
    chunks = []
    with switched(ctx, window=window):
        idx.map_reads(sc.fastq_image(reads), 1, sink=chunks.append, tags=True)
    assert max(len(x) for x in chunks) <= (window + 15) // 16 * 16
    bc.check_text(b"".join(chunks), text)


def check_pairs(ctx, idx, case, key, batch=0):
    name, k, best, indels = key
    p = pair_case(case, k, best, indels)
    assert (p["want"].count(b"\n"), p["pairs"]) == PAIRS[key]
    pc.check_text(b"".join(pc.run(ctx, idx, p, batch=batch, best=best, indels=indels)), p["want"])
    if batch:
        assert ctx.map_stats()["batches"] == -(-len(sc.fastq_reads(case["fastq"])) // batch)


def check_same_bytes(idx, fresh, Index, case, name):
    """the all-flags call twice through an index on a used context, a plain call between them, and once on a fresh context"""
    K = min(CASES[name], 3)
    text = want(case, K, **ALL)
    first = idx.map_reads(case["fastq"], K, **call_flags(**ALL))
    bc.check_text(idx.map_reads(case["fastq"], K), case["fwd"][K])
    assert idx.map_reads(case["fastq"], K, **call_flags(**ALL)) == first == text
    with Index.from_fasta(case["fasta"], ctx=fresh) as other:
        assert other.map_reads(case["fastq"], K, **call_flags(**ALL)) == text
