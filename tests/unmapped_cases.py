"""Unmapped reads and the SAM header (SX_MAP_UNMAPPED, SX_MAP_HEADER): the contract restated in Python
over texts that the fixtures already determine -- the recorded texts of golden_sam.npz, strand_cases for both strands,
best_cases.want_of for best, hamming_cases.want_of for indels=False, tags_cases for tags -- and the cases that the CPU-harness
suite (tests/test_unmapped_cpu.py) and the GPU suite (tests/test_gpu_unmapped.py) share.  `mem` is one of the two objects of
tests/device_memory.py.  TEST INFRASTRUCTURE ONLY."""
import hashlib

import numpy as np

import best_cases as bc
import hamming_cases as hc
import sam_kernel_cases as skc
import tags_cases as tc
from sam_cases import sam_cases
from strand_cases import fastq_image, fastq_reads, lines_of, strand_cases, with_flag
from stralg_amd import _lib, api

# ---- the contract, restated -----------------------------------------------------------------------------------------------
UNMAPPED_FIELDS = b"\t4\t*\t0\t0\t*\t*\t0\t0\t"  # FLAG, RNAME, POS, MAPQ, CIGAR, RNEXT, PNEXT, TLEN between QNAME and SEQ


def unmapped_line(read):
    name, seq, qual = read
    return name + UNMAPPED_FIELDS + seq + b"\t" + qual + b"\n"


def with_unmapped(fastq, text):
    """(the text of the same call with SX_MAP_UNMAPPED, the lines added): per read in FASTQ order its lines of `text` (every
    strand: they share the name), or its FLAG 4 line where it has none.  The names are unique, and the reads' lines stand in
    file order in `text` already: taking the added lines out gives `text` back"""
    reads = fastq_reads(fastq)
    names = [r[0] for r in reads]
    by = lines_of(text)
    assert len(set(names)) == len(names) and set(by) <= set(names)
    assert b"".join(l + b"\n" for n in names for l in by.get(n, [])) == text
    out, added = [], 0
    for r in reads:
        if r[0] in by:
            out += [l + b"\n" for l in by[r[0]]]
        else:
            out.append(unmapped_line(r))
            added += 1
    return b"".join(out), added


WHITE = b" \t\n\r\v\f"


def fasta_sq(fasta):
    """[(name, symbols)] of a FASTA image in file order, as the mapper's records have them: the name is the header line
    behind '>' and the sequence the lines up to the next header, blanks taken out of both"""
    recs = []
    for line in fasta.split(b"\n"):
        if line.startswith(b">"):
            recs.append([line[1:].translate(None, WHITE), 0])
        elif recs:
            recs[-1][1] += len(line.translate(None, WHITE))
    return [tuple(r) for r in recs]


def header_of(fasta):
    return b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % r for r in fasta_sq(fasta))


def rnames_of(text):
    return {l.split(b"\t")[2] for l in text.split(b"\n")[:-1]} - {b"*"}


# ---- the fixture cases ----------------------------------------------------------------------------------------------------
# (case, k, both, best, lines added): the table of the issue; the plain texts are the recorded ones
ADDED = [("test-out/k0", 0, False, False, 1), ("test-out/k1", 1, False, False, 1), ("test-out/k2", 2, False, False, 1),
         ("two-records/k1", 1, False, False, 9), ("hg38/reads-100-10-0/k0", 0, False, False, 49),
         ("hg38/reads-100-10-0/k0", 0, True, False, 34), ("hg38/reads-100-10-0/k1", 1, False, False, 0),
         ("hg38/reads-1000-100-2/k2", 2, False, False, 988), ("hg38/reads-1000-200-1/k1", 1, False, False, 9896),
         ("two-records-flipped/k2", 2, True, False, 5),
         ("two-records-best", 0, False, True, 208), ("two-records-best", 1, False, True, 108), ("two-records-best", 2, False, True, 80),
         ("two-records-best", 0, True, True, 200), ("two-records-best", 1, True, True, 76), ("two-records-best", 2, True, True, 40)]
ADDED_IDS = ["%s/k%d/%s/%s" % (n, k, "both" if both else "one", "best" if best else "all") for n, k, both, best, _ in ADDED]
BY_DIGEST = "hg38/reads-100-10-0/k2"


def fixture_cases():
    """name -> dict(fasta, fastq, k, plain: the text of the call without the flag) for every row of ADDED"""
    base, strands, best = sam_cases(), strand_cases(), bc.best_cases()
    out = {}
    for name, k, both, is_best, _ in ADDED:
        key = (name, k, both, is_best)
        if is_best:
            c = best[name]
            out[key] = dict(fasta=c["fasta"], fastq=c["fastq"], k=k, plain=bc.want_of(c, k, both))
        elif both:
            c = strands[name]
            out[key] = dict(fasta=c["fasta"], fastq=c["fastq"], k=c["k"], plain=c["want"])
        else:
            c = base[name]
            out[key] = dict(fasta=c["fasta"], fastq=c["fastq"], k=c["k"], plain=c["sam"])
    return out


def want_of(case, header=False):
    text, _ = with_unmapped(case["fastq"], case["plain"])
    return (header_of(case["fasta"]) if header else b"") + text


def check_added(cases):
    """the oracle's count of added lines for every case of the table (no case passes on an empty insertion), and the
    header's names are the RNAMEs of the lines"""
    for (name, k, both, best, added), key in zip(ADDED, [a[:4] for a in ADDED]):
        c = cases[key]
        text, n = with_unmapped(c["fastq"], c["plain"])
        assert n == added, (key, n, added)
        assert text.count(b"\t4\t*\t0\t0\t*\t*\t0\t0\t") == added
        assert rnames_of(c["plain"]) <= {sn for sn, _ in fasta_sq(c["fasta"])}, key


# ---- the other flags, on cases of best_cases() ----------------------------------------------------------------------------
def want_flags(case, k, both, best, indels, tags, header=False):
    """the text with SX_MAP_UNMAPPED of a case of best_cases() under the other flags (the FLAG 4 lines carry no tags)"""
    if not indels:
        plain = hc.want_of(case, k, both, best)
    elif best:
        plain = bc.want_of(case, k, both)
    else:
        plain = bc.plain_of(case, k, both)
    text, _ = with_unmapped(case["fastq"], plain)
    if tags:
        letters = tc.fasta_letters(case["fasta"])
        text = b"".join(l + b"\n" if l.split(b"\t")[1] == b"4" else tc.tag_line(l, letters) + b"\n" for l in text.split(b"\n")[:-1])
    return (header_of(case["fasta"]) if header else b"") + text


# (k, both, best, indels, tags): each alone, and all four
FLAG_SETS = [(2, True, False, True, False), (2, False, True, True, False), (2, False, False, False, False), (2, False, False, True, True),
             (2, True, True, False, True), (1, True, True, False, True)]
FLAG_SET_IDS = ["both", "best", "no-indels", "tags", "all-four-k2", "all-four-k1"]


# ---- FASTQ images made for the edges ----------------------------------------------------------------------------------------
def all_unmapped_fastq(n=40, m=30, seed=5):
    """n reads of m letters that no record of test-out holds within 2 edits (X is in no record's alphabet)"""
    rng = np.random.default_rng(seed)
    reads = [(b"u%d" % q, b"X" * m, bytes(rng.integers(33, 127, m, dtype=np.uint8).tolist())) for q in range(n)]
    return fastq_image(reads)


def edges_fastq(case):
    """the reads of a case with an unmapped read first and last, and in between"""
    reads = fastq_reads(case["fastq"])
    lost = [(b"first-lost", b"XXXXXXXX", b"IIIIIIII"), (b"middle lost", b"XQX", b"!!!"), (b"last-lost", b"X", b"#")]
    return fastq_image([lost[0]] + reads[:len(reads) // 2] + [lost[1]] + reads[len(reads) // 2:] + [lost[2]])


# ---- the exported emitter over made-up hits ----------------------------------------------------------------------------------
READS = [(b"q0", b"ACG", b"III"), (b"read one", b"TTGAC", b"#!#!#"), (b"r2", b"GG", b"~~"), (b"three", b"ACGTACGT", b"12345678"),
         (b"lost", b"NNNN", b"!!!!")]


def made_up_case():
    """placeholders (R == L) of reads 0, 2, 4 and 2 again between hits whose positions print 1 digit (sa value 0) and 10 digits
    (4294967294 + 1), reads with FLAG 16 beside them, placeholders first and last"""
    rng = np.random.default_rng(23)
    sa = skc.mixed_sa(rng, 60).astype(np.uint64)
    sa[:3] = [0, 4294967294, 7]
    sa = sa.astype(np.uint32)
    rows = [(0, 5, 5, []), (1, 0, 2, [2]), (2, 9, 9, []), (3, 1, 3, []), (1, 2, 3, [1 | 0x8000]), (4, 0, 0, []), (3, 0, 1, [0, 1]),
            (2, 12, 12, [])]
    return dict(sa=sa, rows=rows, reads=READS, rnames=[b"chr"], flags=[0, 16, 0, 16, 0])


def made_up_text(case, flags=None):
    names, seqs, quals = ([r[i] for r in case["reads"]] for i in range(3))
    out = []
    for q, L, R, g in case["rows"]:
        if L == R:
            out.append(unmapped_line(case["reads"][q]))
            continue
        lines = skc.expected_text(case["sa"], [(q, L, R, g)], names, seqs, quals, case["rnames"]).split(b"\n")[:-1]
        out += [(with_flag(l, b"%d" % flags[q]) if flags else l) + b"\n" for l in lines]
    return b"".join(out)


class UnmappedBatch(skc.Batch):
    """skc.Batch through sx_sam_layout_dev_unmapped / sx_sam_emit_dev_unmapped, with a FLAG per read or without"""

    def __init__(self, ctx, mem, case, flags=None):
        names, seqs, quals = ([r[i] for r in case["reads"]] for i in range(3))
        super().__init__(ctx, mem, skc.make_hits(case["rows"]), case["sa"], names, seqs, quals, case["rnames"])
        self.plain_total = self.total
        if flags is not None:
            self.d_flags = mem.to_dev(np.asarray(flags, np.uint16))
            self.batch = _lib.SamBatchEx(self.batch, api._ptr(self.d_flags))
        mem.fill(self.d_off, 0xEE)
        mem.sync()
        self.total = ctx.sam_layout_dev_unmapped(self.batch, self.d_off)
        self.off = mem.to_host(self.d_off, np.uint64)

    def text(self, window=None):
        mem = self.mem
        window = window or max(self.total, 1)
        room = (min(window, max(self.total, 1)) + 15) // 16 * 16
        buf = mem.zeros(skc.FRONT + room + skc.BEHIND)
        out = []
        for lo in range(0, self.total, window):
            hi = min(self.total, lo + window)
            mem.fill(buf, 0xEE)
            mem.sync()
            self.ctx.sam_emit_dev_unmapped(self.batch, self.d_off, self.total, lo, hi, buf[skc.FRONT:])
            got = mem.to_host(buf)
            assert (got[:skc.FRONT] == 0xEE).all() and (got[skc.FRONT + hi - lo:] == 0xEE).all()
            out.append(got[skc.FRONT:skc.FRONT + hi - lo].tobytes())
        return b"".join(out)


def check_made_up(ctx, mem, case):
    """offsets, total and text, whole and in windows of 16 bytes shifted so that every offset of the FLAG 4 fields is a
    window's first byte; with flags (FLAG 16 neighbours, the placeholders stay FLAG 4); the plain entry prints nothing for
    a placeholder"""
    for flags in (None, case["flags"]):
        want = made_up_text(case, flags)
        b = UnmappedBatch(ctx, mem, case, flags)
        assert b.total == len(want) and int(b.off[-1]) == len(want)
        assert b.text() == want, skc.first_difference(b.text(), want)
        assert want.count(UNMAPPED_FIELDS) == 4
        got = b.text(16)
        assert got == want, skc.first_difference(got, want)
        # every cut: a window boundary at each of the 17 offsets of the fields of the first placeholder after the first line
        at = want.index(UNMAPPED_FIELDS, 1)
        for cut in range(len(UNMAPPED_FIELDS) + 1):
            lo = at + cut
            parts = []
            for a, z in ((0, lo), (lo, b.total)):
                if z > a:
                    parts.append(window_text(ctx, mem, b, a, z))
            assert b"".join(parts) == want, cut
    names, seqs, quals = ([r[i] for r in case["reads"]] for i in range(3))
    plain = skc.Batch(ctx, mem, skc.make_hits(case["rows"]), case["sa"], names, seqs, quals, case["rnames"])
    want = b"".join(l + b"\n" for l in made_up_text(case).split(b"\n")[:-1] if UNMAPPED_FIELDS not in l + b"\n")
    assert plain.total == len(want) and plain.text() == want


def window_text(ctx, mem, b, lo, hi):
    buf = mem.zeros(skc.FRONT + (hi - lo + 15) // 16 * 16 + skc.BEHIND)
    mem.fill(buf, 0xEE)
    mem.sync()
    ctx.sam_emit_dev_unmapped(b.batch, b.d_off, b.total, lo, hi, buf[skc.FRONT:])
    got = mem.to_host(buf)
    assert (got[:skc.FRONT] == 0xEE).all() and (got[skc.FRONT + hi - lo:] == 0xEE).all()
    return got[skc.FRONT:skc.FRONT + hi - lo].tobytes()


def sha256(b):
    return hashlib.sha256(b).digest()
