"""NM:i and MD:Z behind QUAL (SX_MAP_TAGS, sx_sam_layout_dev_tags / sx_sam_emit_dev_tags): the contract
restated as a walk in pure Python over a line's own POS, CIGAR and SEQ and the FASTA record's letters (md_walk knows nothing
of the library), the recorded texts extended by it, and the cases that the CPU-harness suite (tests/test_tags_cpu.py) and
the GPU suite (tests/test_gpu_tags.py) share.  `mem` is one of the two objects of tests/device_memory.py.
TEST INFRASTRUCTURE ONLY."""
import re

import numpy as np
import pytest

import best_cases as bc
import hamming_cases as hc
import sam_kernel_cases as skc
import strand_cases as sc
from sam_cases import sam_cases
from stralg_amd import _lib, api

D = _lib.APPROX_GAP_D


# ---- the contract, restated -----------------------------------------------------------------------------------------------
def md_walk(pos, cigar, seq, letters):
    """(NM, MD) of a line: the CIGAR walked from POS - 1 over the record's letters.  M: equal bytes extend the run, unequal
    ones print "<run><letter of the text>", reset the run and count 1; I: counts its length; D: prints "<run>^<the deleted
    letters>", resets the run and counts its length; the last run ends the string.  Bytes as they are."""
    ops = re.findall(rb"(\d+)([MID])", cigar)
    assert b"".join(n + op for n, op in ops) == cigar, cigar
    t, r, nm, run, md = pos - 1, 0, 0, 0, b""
    for n, op in ops:
        n = int(n)
        if op == b"M":
            for _ in range(n):
                if seq[r] == letters[t]:
                    run += 1
                else:
                    md += b"%d%c" % (run, letters[t])
                    run, nm = 0, nm + 1
                r, t = r + 1, t + 1
        elif op == b"I":
            r, nm = r + n, nm + n
        else:
            md += b"%d^%s" % (run, letters[t:t + n])
            run, nm, t = 0, nm + n, t + n
    assert r == len(seq) and 0 <= pos - 1 and t <= len(letters), (pos, cigar)
    return nm, md + b"%d" % run


def fasta_letters(fasta):
    """RNAME -> the record's letters: the header behind '>' with its blanks dropped, the sequence lines without white space"""
    out = {}
    for block in fasta.split(b">")[1:]:
        head, _, body = block.partition(b"\n")
        out[b"".join(head.split())] = b"".join(body.split())
    return out


def tag_line(line, records):
    f = line.split(b"\t")
    assert f[2] in records, f[2]  # (every line resolves to a record)
    nm, md = md_walk(int(f[3]), f[5], f[9], records[f[2]])
    return line + b"\tNM:i:%d\tMD:Z:%s" % (nm, md)


def tagged(sam, records):
    """the text with every line extended by its two fields (records: fasta_letters, or RNAME -> letters)"""
    return b"".join(tag_line(line, records) + b"\n" for line in sam.split(b"\n")[:-1])


def tag_counts(text):
    """what the guards count in a tagged text"""
    c = dict(lines=0, mismatch=0, insertion=0, deletion=0, behind_deletion=0, md_starts_0=0, md_ends_0=0, md_longest=0, nm_max=0)
    for line in text.split(b"\n")[:-1]:
        f = line.split(b"\t")
        assert f[11].startswith(b"NM:i:") and f[12].startswith(b"MD:Z:") and len(f) == 13
        md, nm = f[12][5:], int(f[11][5:])
        assert re.fullmatch(rb"\d+(?:(?:\^[^\d^]+|[^\d^])\d+)*", md), md  # (begins and ends with a number)
        c["lines"] += 1
        c["mismatch"] += bool(re.search(rb"\d[^\d^]", md))  # (a number with a letter behind it; a deletion has its '^' there)
        c["insertion"] += b"I" in f[5]
        c["deletion"] += b"^" in md
        c["behind_deletion"] += bool(re.search(rb"\^[^\d^]+0[^\d^]", md))
        c["md_starts_0"] += bool(re.match(rb"0\D", md))  # (an item first: a read of insertions alone has the MD "0")
        c["md_ends_0"] += bool(re.search(rb"\D0$", md))
        c["md_longest"] = max(c["md_longest"], len(md))
        c["nm_max"] = max(c["nm_max"], nm)
    return c


# ---- the mapper's cases ---------------------------------------------------------------------------------------------------
# every case of golden_sam.npz with a recorded text; the ninth (hg38/reads-100-10-0/k2) has a digest alone and is left out
WHOLE_TEXT = ["test-out/k0", "test-out/k1", "test-out/k2", "hg38/reads-100-10-0/k0", "hg38/reads-100-10-0/k1",
              "hg38/reads-1000-100-2/k2", "hg38/reads-1000-200-1/k1", "two-records/k1"]
FLAG_PARAMS = [p + (indels,) for p in hc.MAP_PARAMS for indels in (True, False)]
FLAG_IDS = ["%s/%s" % (i, "indels" if p[4] else "no-indels") for i, p in zip([i for i in hc.MAP_IDS for _ in range(2)], FLAG_PARAMS)]


def whole_cases():
    base = sam_cases()
    assert len(base) == 9 and sorted(n for n, c in base.items() if "sam" in c) == sorted(WHOLE_TEXT)
    return {n: base[n] for n in WHOLE_TEXT}


def want_whole(case):
    return tagged(case["sam"], fasta_letters(case["fasta"]))


def want_flags(case, k, both, best, indels):
    """the tagged text of a case of best_cases() under the other three flags"""
    if not indels:
        plain = hc.want_of(case, k, both, best)
    elif best:
        plain = bc.want_of(case, k, both)
    else:
        plain = bc.plain_of(case, k, both)
    return tagged(plain, fasta_letters(case["fasta"]))


def check_guards(cases):
    """the oracle is not vacuous: the recorded texts hold what the walk has to tell apart"""
    c = tag_counts(want_whole(cases["test-out/k2"]))
    assert (c["lines"], c["mismatch"], c["insertion"], c["deletion"]) == (184, 83, 142, 38), c
    assert (c["behind_deletion"], c["md_starts_0"], c["md_ends_0"]) == (5, 72, 69) and c["nm_max"] <= 2, c
    c = tag_counts(want_whole(cases["hg38/reads-100-10-0/k1"]))
    assert (c["lines"], c["mismatch"], c["deletion"], c["insertion"]) == (22493, 3734, 6254, 11623) and c["nm_max"] <= 1, c
    c = tag_counts(want_whole(cases["hg38/reads-1000-100-2/k2"]))
    assert (c["lines"], c["deletion"], c["md_longest"]) == (46, 30, 9) and c["nm_max"] <= 2, c
    c = tag_counts(want_whole(cases["hg38/reads-1000-200-1/k1"]))
    assert (c["lines"], c["deletion"]) == (265, 113) and c["nm_max"] <= 1, c
    want = want_whole(cases["two-records/k1"])
    assert tag_counts(want)["lines"] == 605 and len({l.split(b"\t")[2] for l in want.split(b"\n")[:-1]}) == 2


def stream_tagged(ctx, Index, case, k, both=False, best=False, indels=True, window=0, batch=0, room=0, records=None, **form):
    """(text, map_stats) of Index.from_fasta(...).map_reads(..., tags=True) with the switches set, and every switch back at
    0 behind it.  records: [(name, BwtTable with its string)], and the index is Index.from_tables of them (the CPU harness
    takes half a minute to build the tables of a genome file; its suite brings them from numpy for those)"""
    ctx.set_sam_window_bytes(window)
    ctx.set_sam_batch_reads(batch)
    ctx.set_sam_room_hits(room)
    try:
        with (Index.from_fasta(case["fasta"], ctx=ctx, **form) if records is None else Index.from_tables(records, ctx=ctx, **form)) as idx:
            chunks = []
            idx.map_reads(case["fastq"], k, sink=chunks.append, both_strands=both, best=best, indels=indels, tags=True)
            return chunks, ctx.map_stats()
    finally:
        ctx.set_sam_window_bytes(0)
        ctx.set_sam_batch_reads(0)
        ctx.set_sam_room_hits(0)


def check_windows(ctx, Index, case, window, batch):
    """two-records-best, k = 2, both strands, best off and on, in a room of one hit: grown rooms and halved batches print
    the same text"""
    for best in (False, True):
        chunks, st = stream_tagged(ctx, Index, case, 2, True, best, window=window, batch=batch, room=hc.ROOM_HITS)
        assert st["retries"] > 0, st
        assert max(len(x) for x in chunks) <= (window + 15) // 16 * 16
        bc.check_text(b"".join(chunks), want_flags(case, 2, True, best, True))


def check_index_form(ctx, Index, cases, best_cases, form):
    """test-out k = 2 and two-records/k1 through an index of the given form (the sampled ones go through located positions)"""
    for name in ("test-out/k2", "two-records/k1"):
        c = cases[name]
        with Index.from_fasta(c["fasta"], ctx=ctx, **form) as idx:
            bc.check_text(idx.map_reads(c["fastq"], c["k"], tags=True), want_whole(c))
            bc.check_text(idx.map_reads(c["fastq"], c["k"]), c["sam"])  # (and the plain call is what it was)
    c = best_cases["test-out"]
    with Index.from_fasta(c["fasta"], ctx=ctx, **form) as idx:
        got = idx.map_reads(c["fastq"], 2, both_strands=True, best=True, tags=True)
        bc.check_text(got, want_flags(c, 2, True, True, True))
        assert sum(n for _, n in idx.map_reads_discard(c["fastq"], 2, both_strands=True, best=True, tags=True)) == len(got)


# ---- synthetic hits for the kernel-level entries --------------------------------------------------------------------------
def codes_of(text):
    """(the remapped text with its sentinel, the 256 letters behind the codes) of a record's letters: codes 1 .. in byte order"""
    letters = sorted(set(text))
    table = np.zeros(256, np.uint8)
    table[letters] = np.arange(1, len(letters) + 1)
    inverse = np.zeros(256, np.uint8)
    inverse[1:len(letters) + 1] = letters
    return np.concatenate([table[np.frombuffer(text, np.uint8)], np.zeros(1, np.uint8)]).astype(np.uint8), inverse


def padded(positions, text):
    """a suffix array of the text's length (symbols and sentinel) whose first rows are the given positions"""
    sa = np.zeros(len(text) + 1, np.uint32)
    sa[:len(positions)] = positions
    return sa


def edited(window, ops, other):
    """(read, gap[] list, symbols of the window taken) of an edit string over M (match), X (mismatch), I and D in pattern
    order, applied to the text at `window`; other(letter) is a letter that differs from it"""
    read, gaps, t = bytearray(), [], 0
    for at, op in enumerate(ops):
        if op in "MX":
            read.append(window[t] if op == "M" else other(window[t]))
            t += 1
        elif op == "I":
            read.append(other(window[t % len(window)]))
            gaps.append(at)
        else:
            gaps.append(at | D)
            t += 1
    return bytes(read), gaps, t


def dna_other(b):
    return b"CGTA"[b"ACGT".index(bytes([b]))]


class TagBatch(skc.Batch):
    """skc.Batch through sx_sam_layout_dev_tags / sx_sam_emit_dev_tags.  case["texts"]: the records' letters (one per record
    name); case["shift"]: the first text's first byte off a 16-byte boundary; case["flags"]: a FLAG per read; case["located"]:
    the positions go in located beforehand (with a base that is not 0) and the suffix arrays' rows are never read"""

    def __init__(self, ctx, mem, case):
        super().__init__(ctx, mem, skc.make_hits(case["rows"]), case["sa"], case["names"], case["seqs"], case["quals"], case["rnames"])
        texts, tables = zip(*(codes_of(t) for t in case["texts"]))
        self.d_texts = [mem.to_dev(t, case.get("shift", 0) if r == 0 else (3 * r) % 16) for r, t in enumerate(texts)]
        self.d_text_list = mem.to_dev(np.array([api._ptr(d) for d in self.d_texts], np.uint64))
        self.d_letters = mem.to_dev(np.concatenate(tables))
        batch = self.batch
        if case.get("flags") is not None:
            self.d_flags = mem.to_dev(np.asarray(case["flags"], np.uint16))
            batch = _lib.SamBatchEx(batch, api._ptr(self.d_flags))
        located = ()
        if case.get("located"):
            sas, _ = skc._as_lists(case["sa"], case["rnames"])
            n_rec = len(case["rnames"])
            rows = [np.asarray(sas[q % n_rec][L:R], np.uint32) for q, L, R, g in case["rows"]]
            base = 1000
            pos_off = base + np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.uint64)
            self.d_positions = mem.to_dev(np.concatenate(rows + [np.zeros(1, np.uint32)]))
            self.d_pos_off = mem.to_dev(pos_off.astype(np.uint64))
            located = (self.d_positions, self.d_pos_off, base)
            # the rows themselves are not to be read: the device copies of the suffix arrays, found by the addresses the
            # batch holds (its one array, or the entries of its list), are overwritten
            held = {int(self.batch.d_sa or 0)}
            for buf in self.keep:
                if self.batch.d_sa_list and api._ptr(buf) == self.batch.d_sa_list:
                    held |= {int(p) for p in mem.to_host(buf, np.uint64)[:n_rec]}
            d_sas = [buf for buf in self.keep if api._ptr(buf) in held]
            assert len(d_sas) == n_rec
            for d_sa in d_sas:
                mem.fill(d_sa, 0xFF)
        self.batch = ctx.sam_batch_tags(batch, self.d_text_list, self.d_letters, *located)
        mem.fill(self.d_off, 0xEE)
        mem.sync()
        self.total = ctx.sam_layout_dev(self.batch, self.d_off)
        self.off = mem.to_host(self.d_off, np.uint64)


def expected_lines(case):
    """per hit row the tagged lines it prints: formatted by sam_kernel_cases, the FLAG rewritten, the fields from md_walk"""
    plain = skc.text_of(case).split(b"\n")[:-1]
    records = dict(zip(case["rnames"], case["texts"]))
    assert len(records) == len(case["rnames"])
    out, at = [], 0
    for q, L, R, g in case["rows"]:
        lines = plain[at:at + R - L]
        at += R - L
        if case.get("flags") is not None:
            lines = [sc.with_flag(l, b"%d" % case["flags"][q // len(case["rnames"])]) for l in lines]
        out.append([tag_line(l, records) for l in lines])
    assert at == len(plain)
    return out


def check_tag_text(ctx, mem, case):
    """the layout's offsets against the expected lines' lengths, hit by hit; the one-window text and every window size's
    concatenation against the expected text"""
    per_hit = expected_lines(case)
    want = b"".join(l + b"\n" for lines in per_hit for l in lines)
    want_off = np.concatenate([[0], np.cumsum([sum(len(l) + 1 for l in lines) for lines in per_hit])]).astype(np.uint64)
    b = TagBatch(ctx, mem, case)
    assert b.total == len(want) == int(want_off[-1]), (case["name"], b.total, len(want))
    wrong = np.flatnonzero(b.off != want_off)
    assert wrong.size == 0, (case["name"], "first wrong offset at hit", int(wrong[0]))
    got = b.text()
    assert len(got) == len(want) and got == want, (case["name"], "one window", skc.first_difference(got, want))
    for window in case.get("windows", ()):
        got = b.text(window)
        assert len(got) == len(want) and got == want, (case["name"], window, skc.first_difference(got, want))
    return want


def check_tag_refused(ctx, mem, case):
    """the plain layout takes the hits; the tagged one answers SX_E_ARG"""
    with pytest.raises(api.StralgAmdError) as e:
        TagBatch(ctx, mem, case)
    assert "code -1" in str(e.value) and "sx_sam_layout_dev_tags" in str(e.value)


def _case(name, text, reads, rows, positions=None, **more):
    """one record `text`; reads: [read bytes]; rows: (read, L, R, gaps) over the suffix array `positions` (default: row i is
    position i)"""
    sa = padded(positions if positions is not None else np.arange(len(text)), text)
    names = [b"q%d" % i if i % 2 else b"read %d" % i for i in range(len(reads))]
    quals = [bytes(33 + (i + j) % 60 for j in range(len(r))) for i, r in enumerate(reads)]
    return dict(dict(name=name, rows=rows, sa=sa, names=names, seqs=list(reads), quals=quals, rnames=[b"rec"], texts=[text]), **more)


def small_cases():
    """reads of one symbol; windows at position 0 and up to the last symbol; eight edits of every kind; a mismatch straight
    behind a deletion; an insertion between two deletions; bytes that differ in case alone"""
    rng = np.random.default_rng(61)
    out = [_case("one-symbol", b"ACGT", [b"C", b"G", b"A", b"T", b"GT", b"a"],
                 [(0, 1, 2, []), (1, 1, 2, []), (2, 0, 1, []), (3, 3, 4, []), (4, 2, 3, []), (1, 0, 1, []), (5, 0, 1, [])], shift=7)]
    text = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 400)].tobytes()
    reads, rows = [], []
    for ops, at in [("X" + "MMMX" * 7, 0), ("MMM" + "DMMM" * 8, 11), ("MMMM" + "D" * 8 + "MMMM", 30), ("XMIMMDMMIIMDDMMX", 50),
                    ("MMDDXMM", 70), ("MDIDM", 90), ("MMIIM", 100), ("M" * 37, 363), ("M" * 30 + "DDDDDDDX", 362), ("IMMMM", 5), ("MMMMI", 396)]:
        read, gaps, took = edited(text[at:], ops, dna_other)
        assert at + took <= 400
        rows.append((len(reads), at, at + 1, gaps))
        reads.append(read)
    out.append(_case("eight-edits", text, reads, rows, windows=skc.WINDOWS, shift=1))
    # the reference prints what the files hold: no case folding
    out.append(_case("letter-case", b"ACgtNNac", [b"ACGT", b"acgt", b"nNAC"], [(0, 0, 1, []), (1, 0, 1, []), (2, 4, 5, [])]))
    return out


def refused_cases():
    """a window one symbol beyond the last one in front of the sentinel (by its length, and by a deletion at its end); nine
    differences (nine mismatches; eight gaps and a mismatch)"""
    text = b"ACGTACGTACGTACGTACGTACGTACGTACGT"
    out = [_case("window-one-too-far", b"ACGT", [b"GT"], [(0, 3, 4, [])]),
           _case("window-into-the-sentinel", b"ACGT", [b"T"], [(0, 4, 5, [])], np.arange(5)),
           _case("deletion-one-too-far", b"ACGT", [b"CG"], [(0, 1, 2, [1 | D, 3 | D])])]
    read, gaps, _ = edited(text, "X" * 9 + "MMM", dna_other)
    out.append(_case("nine-mismatches", text, [read], [(0, 0, 1, gaps)]))
    read, gaps, _ = edited(text, "MDMDMIMIMDMDMIMIMX", dna_other)
    assert len(gaps) == 8
    out.append(_case("eight-gaps-and-a-mismatch", text, [read], [(0, 0, 1, gaps)]))
    return out


def long_read_case():
    """reads of 2046 symbols at window starts 0 .. 15 off a 16-byte boundary, a mismatch at the first, the 1000th or the last
    symbol (runs of four digits), and one with a deletion in the middle"""
    rng = np.random.default_rng(62)
    m = 2046
    text = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, m + 40)].tobytes()
    reads, rows = [], []
    for start in range(16):
        at = (0, 999, m - 1)[start % 3]
        read, gaps, _ = edited(text[start:], "M" * at + "X" + "M" * (m - 1 - at), dna_other)
        rows.append((len(reads), start, start + 1, gaps))
        reads.append(read)
    read, gaps, _ = edited(text[3:], "X" + "M" * 1022 + "DD" + "M" * 1022 + "X", dna_other)
    rows.append((len(reads), 3, 4, gaps))
    reads.append(read)
    return _case("reads-of-2046", text, reads, rows, windows=[16383, 16384, 16385])


def periodic(unit, n):
    return (unit * (n // len(unit) + 2))[:n]


def interval_case():
    """intervals around the size pass's inline limit, the emit's step and its walk's step: every row of a hit is a copy of
    the same window of a periodic text; tagged lines of several lengths between them"""
    unit = b"GATTACAGCT"
    text = periodic(unit, 10 * 2100 + 64)
    positions = (3 + 10 * np.arange(2100)).astype(np.uint32)  # (positions of 1 to 5 digits)
    specs = ["MMMMMMMMMMMM", "MXMMMDMMMMMX", "XIMMMMMMM", "MMMMDDXMMMM"]
    reads, gapsets = [], []
    for ops in specs:
        read, gaps, _ = edited(text[3:], ops, dna_other)
        reads.append(read)
        gapsets.append(gaps)
    rng = np.random.default_rng(63)
    rows = []
    for k, n in enumerate([1, 32, 33, 256, 257, 1024, 1025, 2049, 2, 2049, 31]):
        L = int(rng.integers(0, positions.size - n + 1))
        rows.append((k % 4, L, L + n, gapsets[k % 4]))
    return _case("intervals", text, reads, rows, positions, windows=[4099, 16383, 16384, 16385])


def many_hits_cases():
    """257 and 600 hits (more than a step of a workgroup) with empty intervals between them"""
    unit = b"TTGACCA"
    text = periodic(unit, 7 * 300 + 40)
    positions = (2 + 7 * np.arange(300)).astype(np.uint32)
    specs = ["MMMMMMMM", "MMXMMMMM", "MDMMMMMX", "MMMIMMM"]
    reads, gapsets = zip(*(edited(text[2:], ops, dna_other)[:2] for ops in specs))
    rng = np.random.default_rng(64)
    out = []
    for n in (257, 600):
        rows = []
        for h in range(n):
            L = int(rng.integers(0, 290))
            rows.append((h % 4, L, L + (0 if h % 3 == 1 else int(rng.integers(1, 4))), list(gapsets[h % 4])))
        out.append(_case("%d-hits" % n, text, list(reads), rows, positions, windows=[257, 4099]))
    return out


def several_records_case():
    """three records with alphabets of their own (one is not DNA, one has both cases): the letters go by record rank; one
    suffix array per record; a FLAG per read"""
    texts = [periodic(b"FOOBARBAZ", 90), periodic(b"acgtACGT", 64), periodic(b"AC", 41)]
    sas = [padded(np.arange(len(t)), t) for t in texts]
    others = [lambda b: b"Z"[0] if b != b"Z"[0] else b"F"[0], lambda b: bytes([b]).swapcase()[0], lambda b: b"CA"[b"AC".index(bytes([b]))]]
    reads, rows = [], []
    for rec, at, ops in [(0, 9, "MMXMMDMMM"), (1, 8, "XMMMMIMMX"), (2, 6, "MMMMMDMMX"), (1, 3, "MMMMMMMM"), (0, 1, "DMMMXX"), (2, 0, "XMIIM")]:
        read, gaps, _ = edited(texts[rec][at:], ops, others[rec])
        rows.append((len(reads) * 3 + rec, at, at + 1, gaps))
        reads.append(read)
    names = [b"r%d" % i for i in range(len(reads))]
    quals = [b"I" * len(r) for r in reads]
    return dict(name="three-alphabets", rows=rows, sa=sas, names=names, seqs=reads, quals=quals, rnames=[b"foo", b"mixedCase", b"ac"],
                texts=texts, flags=[0, 16, 256, 65535, 16, 0], windows=[17, 255])


def form_cases():
    """kFlags and kLocated, each with tags and both together, on the intervals and on the three records"""
    a, b = interval_case(), several_records_case()
    return [dict(a, name="intervals/flags", flags=[16, 0, 65535, 256]), dict(a, name="intervals/located", located=True),
            dict(a, name="intervals/located-flags", located=True, flags=[0, 16, 16, 0], windows=[4099]),
            dict(b, name="three-alphabets/located", located=True), dict(b, name="three-alphabets/no-flags", flags=None)]


def kernel_cases():
    cases = small_cases() + [long_read_case(), interval_case()] + many_hits_cases() + [several_records_case()] + form_cases()
    return {c["name"]: c for c in cases}


KERNEL_CASE_NAMES = ["one-symbol", "eight-edits", "letter-case", "reads-of-2046", "intervals", "257-hits", "600-hits", "three-alphabets",
                     "intervals/flags", "intervals/located", "intervals/located-flags", "three-alphabets/located", "three-alphabets/no-flags"]
REFUSED_NAMES = ["window-one-too-far", "window-into-the-sentinel", "deletion-one-too-far", "nine-mismatches", "eight-gaps-and-a-mismatch"]


def check_expected_fields():
    """the expected texts of the synthetic cases say what they were built to say"""
    lines = [l for hit in expected_lines(kernel_cases()["eight-edits"]) for l in hit]
    fields = [tuple(l.split(b"\t")[11:]) for l in lines]
    assert fields[0][0] == b"NM:i:8" and fields[0][1].count(b"0") >= 1 and len(re.findall(rb"[ACGT]", fields[0][1])) == 8
    assert fields[1][0] == b"NM:i:8" and fields[1][1].count(b"^") == 8
    assert fields[2][0] == b"NM:i:8" and re.fullmatch(rb"MD:Z:4\^[ACGT]{8}4", fields[2][1])
    assert fields[3][0] == b"NM:i:8" and fields[3][1].startswith(b"MD:Z:0") and fields[3][1].endswith(b"0")
    assert re.fullmatch(rb"MD:Z:2\^[ACGT]{2}0[ACGT]2", fields[4][1])  # (^AC0T)
    assert re.fullmatch(rb"MD:Z:1\^[ACGT]0\^[ACGT]1", fields[5][1])  # (an insertion parts two deletions)
    one = [tuple(l.split(b"\t")[11:]) for hit in expected_lines(kernel_cases()["one-symbol"]) for l in hit]
    assert one[:4] == [(b"NM:i:0", b"MD:Z:1"), (b"NM:i:1", b"MD:Z:0C0"), (b"NM:i:0", b"MD:Z:1"), (b"NM:i:0", b"MD:Z:1")]
    assert one[6] == (b"NM:i:1", b"MD:Z:0A0")
    long = [l.split(b"\t")[12] for hit in expected_lines(long_read_case()) for l in hit]
    assert re.fullmatch(rb"MD:Z:0[ACGT]2045", long[0]) and re.fullmatch(rb"MD:Z:999[ACGT]1046", long[1]) and re.fullmatch(rb"MD:Z:2045[ACGT]0", long[2])
