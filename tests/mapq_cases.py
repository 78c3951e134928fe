"""MAPQ and secondary lines from the best stratum (SX_MAP_MAPQ): the contract restated in Python over
texts that the fixtures already determine -- best_cases.want_of, hamming_cases.want_of(best=True), unmapped_cases.with_unmapped of
those, the tag walk of tags_cases -- and the cases that the CPU-harness suite (tests/test_mapq_cpu.py) and the GPU suite
(tests/test_gpu_mapq.py) share.  `mem` is one of the two objects of tests/device_memory.py.  TEST INFRASTRUCTURE ONLY."""
import numpy as np
import pytest

import best_cases as bc
import hamming_cases as hc
import sam_kernel_cases as skc
import tags_cases as tc
import unmapped_cases as uc
from strand_cases import fastq_image, fastq_reads, with_flag
from stralg_amd import _lib, api

SECONDARY = 256
QBIT = 0x100  # bit 8 of a hit's quality word: its lines are secondary


# ---- the contract, restated -----------------------------------------------------------------------------------------------
def mapq_of(n):
    """-10 log10(1 - 1/n) as TopHat and STAR round it"""
    assert n >= 1
    return 50 if n == 1 else 3 if n == 2 else 1 if n <= 4 else 0


def with_mapq(fastq, text):
    """(the text of the same call with SX_MAP_MAPQ, its counts).  The lines of a read (every strand: they share the name) stand
    together in `text`, in FASTQ order; n is how many there are.  The first keeps its FLAG, every other one has 256 added, all
    carry the MAPQ of n.  FLAG 4 lines and header lines stay as they are.  counts: lines, secondary, first lines with FLAG 16,
    first lines per RNAME, groups per MAPQ, the largest n"""
    names = [r[0] for r in fastq_reads(fastq)]
    assert len(set(names)) == len(names)
    order = {n: i for i, n in enumerate(names)}
    lines = text.split(b"\n")[:-1]
    out = []
    counts = dict(lines=0, secondary=0, first16=0, first_rname={}, groups={50: 0, 3: 0, 1: 0, 0: 0}, sizes=set())
    at, last = 0, -1
    while at < len(lines):
        f = lines[at].split(b"\t")
        if lines[at].startswith(b"@") or f[1] == b"4":
            if f[1] == b"4" and not lines[at].startswith(b"@"):
                assert order[f[0]] > last
                last = order[f[0]]
            out.append(lines[at])
            at += 1
            continue
        end = at
        while end < len(lines) and lines[end].split(b"\t", 1)[0] == f[0]:
            end += 1
        assert order[f[0]] > last, "a read's lines stand together, in file order"
        last = order[f[0]]
        n = end - at
        q = mapq_of(n)
        for i in range(at, end):
            g = lines[i].split(b"\t")
            assert g[1] in (b"0", b"16") and g[4] == b"0", lines[i]
            if i > at:
                g[1] = b"%d" % (int(g[1]) + SECONDARY)
            g[4] = b"%d" % q
            out.append(b"\t".join(g))
        counts["lines"] += n
        counts["secondary"] += n - 1
        counts["first16"] += f[1] == b"16"
        counts["first_rname"][f[2]] = counts["first_rname"].get(f[2], 0) + 1
        counts["groups"][q] += 1
        counts["sizes"].add(n)
        at = end
    return b"".join(l + b"\n" for l in out), counts


def without_mapq(text):
    """the inverse: 256 cleared and MAPQ set to 0 on every line (header lines and FLAG 4 lines have neither)"""
    out = []
    for line in text.split(b"\n")[:-1]:
        if not line.startswith(b"@"):
            f = line.split(b"\t")
            f[1] = b"%d" % (int(f[1]) & ~SECONDARY)
            f[4] = b"0"
            line = b"\t".join(f)
        out.append(line)
    return b"".join(l + b"\n" for l in out)


# ---- the fixture cases ----------------------------------------------------------------------------------------------------
# (case of best_cases(), k, both, indels, lines, secondary, groups with MAPQ 50 / 3 / 1 / 0): the table of the issue
TABLE = [("two-records-best", 0, False, True, 34, 2, (30, 2, 0, 0)),
         ("two-records-best", 1, False, True, 226, 94, (86, 20, 21, 5)),
         ("two-records-best", 2, True, True, 359, 159, (127, 35, 29, 9)),
         ("two-records-best", 2, True, False, 105, 5, (96, 3, 1, 0)),
         ("hg38/reads-100-10-0", 1, False, True, 3181, 3081, (19, 10, 9, 62)),
         ("hg38/reads-100-10-0", 1, True, False, 2604, 2504, (22, 8, 16, 54)),
         ("test-out", 2, True, True, 5, 2, (1, 2, 0, 0))]
TABLE_IDS = ["%s/k%d/%s/%s" % (n, k, "both" if both else "one", "indels" if indels else "no-indels") for n, k, both, indels, *_ in TABLE]


def plain_of(case, k, both, indels=True, tags=False, unmapped=False, header=False):
    """the text of the call with best and without SX_MAP_MAPQ, under the other flags"""
    if unmapped:
        return uc.want_flags(case, k, both, True, indels, tags, header)
    text = tc.want_flags(case, k, both, True, indels) if tags else hc.want_of(case, k, both, True) if not indels else bc.want_of(case, k, both)
    return (uc.header_of(case["fasta"]) if header else b"") + text


def want_of(case, k, both, indels=True, tags=False, unmapped=False, header=False):
    plain = plain_of(case, k, both, indels, tags, unmapped, header)
    text, _ = with_mapq(case["fastq"], plain)
    assert without_mapq(text) == plain
    return text


def check_table(cases):
    """the oracle's own counts for every row of the table (no case passes on an unchanged text), what the rows cover between
    them, and the inverse"""
    sizes = set()
    for name, k, both, indels, lines, secondary, groups in TABLE:
        c = cases[name]
        plain = plain_of(c, k, both, indels)
        text, n = with_mapq(c["fastq"], plain)
        assert (n["lines"], n["secondary"]) == (lines, secondary), (name, k, both, indels, n)
        assert tuple(n["groups"][q] for q in (50, 3, 1, 0)) == groups, (name, k, both, indels, n["groups"])
        assert plain.count(b"\n") == lines and without_mapq(text) == plain and (text != plain) == (lines > 0)
        flags = [l.split(b"\t")[1] for l in text.split(b"\n")[:-1]]
        assert sum(f in (b"256", b"272") for f in flags) == secondary and sum(f in (b"0", b"16") for f in flags) == sum(groups)
        sizes |= n["sizes"]
        if (name, k, both, indels) == ("two-records-best", 2, True, True):
            assert n["first16"] == 40 and n["first_rname"].get(b"right") == 76 and b"272" in flags
    assert {1, 2, 3, 4, 5, 6, 326, 600} <= sizes, sorted(sizes)


# (tags, unmapped, header, indels): each alone, and all together -- on two-records-best, k = 2, both strands
FLAG_SETS = [(True, False, False, True), (False, True, False, True), (False, False, True, True), (False, False, False, False),
             (True, True, True, False)]
FLAG_SET_IDS = ["tags", "unmapped", "header", "no-indels", "all"]
FORMS = [dict(), dict(compact=True), dict(compact=True, sa_sample=32), dict(compact=True, packed=True, sa_sample=32)]
FORM_IDS = ["full", "compact", "sampled", "packed-sampled"]


def edges_fastq(case):
    """the reads of a case with an unmapped read first and last, and in between (unmapped_cases.edges_fastq)"""
    return uc.edges_fastq(case)


def planted_case(n_reads=10000, m=100, log2n=22, seed=2025):
    """(fasta, fastq): a record of 2^log2n random symbols in which a segment of 4 m symbols stands twice; every tenth read is
    copied from the segment (two placements: MAPQ 3), the others from anywhere, each with at most one substitution"""
    rng = np.random.default_rng(seed)
    dna = np.frombuffer(b"ACGT", np.uint8)
    genome = rng.choice(dna, 1 << log2n)
    a, b = genome.size // 5, 3 * genome.size // 5
    genome[b:b + 4 * m] = genome[a:a + 4 * m]
    fasta = b">planted twice\n" + b"\n".join(genome[i:i + 80].tobytes() for i in range(0, genome.size, 80)) + b"\n"
    reads = []
    for q in range(n_reads):
        at = a + int(rng.integers(0, 3 * m)) if q % 10 == 0 else int(rng.integers(0, genome.size - m))
        seq = genome[at:at + m].copy()
        if q % 10 and rng.integers(0, 2):
            j = int(rng.integers(0, m))
            seq[j] = dna[(np.flatnonzero(dna == seq[j])[0] + 1) % 4]
        reads.append((b"r%d" % q, seq.tobytes(), bytes(rng.integers(33, 74, m, dtype=np.uint8).tolist())))
    return fasta, fastq_image(reads)


# ---- the exported emitter over made-up hits ----------------------------------------------------------------------------------
WORDS = [50, 3, 1, 0, 255]  # the MAPQs of the contract, and one of three digits (the size pass counts them)


def quality_line(line, word, flag):
    """a mapped line as the emitter prints it for a hit with this quality word and a read with this FLAG"""
    f = line.split(b"\t")
    f[1] = b"%d" % (flag | (word & QBIT))
    f[4] = b"%d" % (word & 0xFF)
    return b"\t".join(f)


def small_case():
    """unmapped_cases.made_up_case (placeholders first and last, positions of 1 and 10 digits, reads with FLAG 16) with a
    quality word a hit: every MAPQ with and without bit 8; the placeholders' words are junk"""
    c = uc.made_up_case()
    c["names"], c["seqs"], c["quals"] = ([r[i] for r in c["reads"]] for i in range(3))
    c["quality"] = [0xFFFF, 50 | QBIT, 0x1FF, 255, 3 | QBIT, 0xABCD, 0, 7]
    c["name"] = "small"
    return c


def interval_case():
    """intervals of 1, 2, 33, 257, 1 025 and 5 000 rows (the size pass's inline limit, the emit's step, the walk's step) over
    positions of 1 to 10 digits, every quality word of WORDS with and without bit 8, placeholders first, between and last"""
    rng = np.random.default_rng(29)
    sa = skc.mixed_sa(rng, 6000).astype(np.uint64)
    sa[:3] = [0, 4294967294, 7]
    sa = sa.astype(np.uint32)
    reads = uc.READS
    gaps = [[], [1], [2 | _lib.APPROX_GAP_D], [0, 1]]
    rows, quality = [(4, 9, 9, [])], [0x1234]
    for k, n in enumerate([1, 2, 33, 257, 1025, 5000, 2, 33, 1, 1025]):
        L = 0 if k < 2 else int(rng.integers(0, sa.size - n + 1))
        rows.append((k % 4, L, L + n, gaps[k % 4]))
        quality.append(WORDS[k % 5] | (QBIT if (k // 2) % 2 else 0))  # (reads k % 4: FLAG 0 and 16, each with and without bit 8)
        if k in (3, 5):
            rows.append((2, 40, 40, []))
            quality.append(0xFFFF)
    rows.append((0, 0, 0, []))
    quality.append(0)
    return dict(name="intervals", sa=sa, rows=rows, reads=reads, names=[r[0] for r in reads], seqs=[r[1] for r in reads],
                quals=[r[2] for r in reads], rnames=[b"chr"], flags=[0, 16, 0, 16, 0], quality=quality, windows=[4099, 16384])


def tagged_case():
    """tags_cases.interval_case with placeholders and quality words: tagged lines of several lengths under MAPQ and FLAG"""
    c = tc.interval_case()
    rows = [(1, 5, 5, [])] + list(c["rows"]) + [(3, 0, 0, [])]
    rows.insert(4, (0, 77, 77, []))
    rng = np.random.default_rng(31)
    quality = [int(WORDS[i % 5]) | (QBIT if rng.integers(0, 2) else 0) for i in range(len(rows))]
    return dict(c, name="tagged", rows=rows, quality=quality, flags=[16, 0, 16, 0], windows=[4099])


def expected_lines(case, flags):
    """per hit row the lines it prints"""
    tagged = "texts" in case
    records = dict(zip(case["rnames"], case["texts"])) if tagged else None
    reads = list(zip(case["names"], case["seqs"], case["quals"]))
    out = []
    for (q, L, R, g), word in zip(case["rows"], case["quality"]):
        read = q // len(case["rnames"])
        if L == R:
            out.append([uc.unmapped_line(reads[read])[:-1]])
            continue
        lines = skc.expected_text(case["sa"], [(q, L, R, g)], case["names"], case["seqs"], case["quals"], case["rnames"]).split(b"\n")[:-1]
        lines = [quality_line(l, word, flags[read] if flags is not None else 0) for l in lines]
        out.append([tc.tag_line(l, records) for l in lines] if tagged else lines)
    return out


class MapqBatch(skc.Batch):
    """skc.Batch through sx_sam_layout_dev_mapq / sx_sam_emit_dev_mapq: with a FLAG per read or without, with the records' texts
    (case["texts"]: tags) or without, the positions located beforehand (the suffix arrays' device copies are overwritten) or not"""

    def __init__(self, ctx, mem, case, flags=None, located=False, quality=True):
        super().__init__(ctx, mem, skc.make_hits(case["rows"]), case["sa"], case["names"], case["seqs"], case["quals"], case["rnames"])
        batch = self.batch
        if flags is not None:
            self.d_flags = mem.to_dev(np.asarray(flags, np.uint16))
            batch = _lib.SamBatchEx(batch, api._ptr(self.d_flags))
        text_list = letters = None
        if "texts" in case:
            texts, tables = zip(*(tc.codes_of(t) for t in case["texts"]))
            self.d_texts = [mem.to_dev(t, (3 * r + 5) % 16) for r, t in enumerate(texts)]
            text_list = self.d_text_list = mem.to_dev(np.array([api._ptr(d) for d in self.d_texts], np.uint64))
            letters = self.d_letters = mem.to_dev(np.concatenate(tables))
        loc = (None, None, 0)
        if located:
            assert len(case["rnames"]) == 1
            rows = [np.asarray(case["sa"][L:R], np.uint32) for q, L, R, g in case["rows"]]
            base = 1000
            self.d_positions = mem.to_dev(np.concatenate(rows + [np.zeros(1, np.uint32)]))
            self.d_pos_off = mem.to_dev((base + np.concatenate([[0], np.cumsum([r.size for r in rows])])).astype(np.uint64))
            loc = (self.d_positions, self.d_pos_off, base)
            mem.fill(self.keep[-1], 0xFF)  # (the one suffix array's device copy: its rows are not to be read)
        ex = batch if isinstance(batch, _lib.SamBatchEx) else _lib.SamBatchEx(batch, None)
        self.batch = _lib.SamBatchTags(ex, api._ptr(text_list), api._ptr(letters), api._ptr(loc[0]), api._ptr(loc[1]), loc[2])
        self.d_quality = mem.to_dev(np.asarray(case["quality"], np.uint16)) if quality else None
        mem.fill(self.d_off, 0xEE)
        mem.sync()
        self.total = ctx.sam_layout_dev_mapq(self.batch, self.d_quality, self.d_off)
        self.off = mem.to_host(self.d_off, np.uint64)

    def window(self, lo, hi, fill=0xEE):
        mem = self.mem
        buf = mem.zeros(skc.FRONT + (hi - lo + 15) // 16 * 16 + skc.BEHIND)
        mem.fill(buf, fill)
        mem.sync()
        self.ctx.sam_emit_dev_mapq(self.batch, self.d_quality, self.d_off, self.total, lo, hi, buf[skc.FRONT:])
        got = mem.to_host(buf)
        assert (got[:skc.FRONT] == fill).all(), "bytes in front of the window were written"
        assert (got[skc.FRONT + hi - lo:] == fill).all(), "bytes behind the window were written"
        return got[skc.FRONT:skc.FRONT + hi - lo].tobytes()

    def text(self, window=None, fill=0xEE):
        window = window or max(self.total, 1)
        return b"".join(self.window(lo, min(self.total, lo + window), fill) for lo in range(0, self.total, window))


def check_emitter(ctx, mem, case, flags, located=False, sixteen=False):
    """offsets hit by hit, the total, the text in one window (twice, over differently pre-filled buffers), in the case's
    windows and, where asked for, in windows of 16 bytes"""
    per_hit = expected_lines(case, flags)
    want = b"".join(l + b"\n" for lines in per_hit for l in lines)
    want_off = np.concatenate([[0], np.cumsum([sum(len(l) + 1 for l in lines) for lines in per_hit])]).astype(np.uint64)
    b = MapqBatch(ctx, mem, case, flags, located)
    assert b.total == len(want) == int(want_off[-1]), (case["name"], b.total, len(want))
    wrong = np.flatnonzero(b.off != want_off)
    assert wrong.size == 0, (case["name"], "first wrong offset at hit", int(wrong[0]))
    got, again = b.text(), b.text(fill=0x11)
    assert got == want, (case["name"], "one window", skc.first_difference(got, want))
    assert again == got, "the same bytes from run to run"
    for window in list(case.get("windows", ())) + ([16] if sixteen else []):
        got = b.text(window)
        assert got == want, (case["name"], window, skc.first_difference(got, want))
    return b, want


def check_cuts(b, want, needle):
    """a window boundary at every offset of the FLAG-through-MAPQ span of the first line that holds `needle` in its FLAG field:
    from the tab in front of FLAG to the tab behind MAPQ"""
    at = 0
    for line in want.split(b"\n")[:-1]:
        f = line.split(b"\t")
        if f[1] == needle:
            break
        at += len(line) + 1
    else:
        raise AssertionError("no line with FLAG %r" % needle)
    lo = at + len(f[0])
    span = sum(len(x) + 1 for x in f[1:5]) + 1
    for cut in range(span + 1):
        parts = [b.window(a, z) for a, z in ((0, lo + cut), (lo + cut, b.total)) if z > a]
        assert b"".join(parts) == want, (needle, cut)
    return span


def check_refused_without_quality(ctx, mem, case):
    with pytest.raises(api.StralgAmdError) as e:
        MapqBatch(ctx, mem, case, quality=False)
    assert "code -1" in str(e.value) and "sx_sam_layout_dev_mapq" in str(e.value)
