"""Both strands (sx_fastq_strands_dev, the FLAG of the SAM emitter, the mapper's loop with SX_MAP_BOTH_STRANDS): the
contract's rc() restated with bytes.translate and slicing, the expected text composed from the reference mapper's two
recorded outputs (tests/golden/golden_sam_strands.npz, written by tests/golden/make_golden_sam_strands.py), and the
kernel-level cases that the CPU-harness suite (tests/test_strands_cpu.py) and the GPU suite (tests/test_gpu_strands.py)
share.  `mem` is one of the two objects of tests/device_memory.py.  TEST INFRASTRUCTURE ONLY."""
import hashlib
import os

import numpy as np

import sam_kernel_cases as skc
from sam_cases import ROOT, sam_cases
from stralg_amd import _lib, api

# ---- the contract, restated -----------------------------------------------------------------------------------------------
COMPLEMENT = bytes.maketrans(b"ACGTURYKMBVDHacgturykmbvdh", b"TGCAAYRMKVBHDtgcaayrmkvbhd")


def rc(read):
    """rc of a (name, sequence, quality) triple: the same name, the sequence reversed and complemented (on the raw bytes:
    case kept, every byte outside the table maps to itself), the quality string reversed"""
    name, seq, qual = read
    return name, seq.translate(COMPLEMENT)[::-1], qual[::-1]


def fastq_reads(fastq):
    """[(name, sequence, quality)] of a well-formed FASTQ image (the name: the first line behind its first byte)"""
    lines = fastq.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    assert len(lines) % 4 == 0
    return [(lines[i][1:], lines[i + 1], lines[i + 3]) for i in range(0, len(lines), 4)]


def fastq_image(reads):
    return b"".join(b"@%s\n%s\n+\n%s\n" % r for r in reads)


def rc_fastq(fastq):
    return fastq_image([rc(r) for r in fastq_reads(fastq)])


def interleaved_fastq(fastq):
    """read0, rc(read0), read1, rc(read1), ..."""
    return fastq_image([x for r in fastq_reads(fastq) for x in (r, rc(r))])


def with_flag(line, flag):
    name, _, rest = line.split(b"\t", 2)
    return name + b"\t" + flag + b"\t" + rest


def lines_of(sam):
    """qname -> its lines, in order (a read's lines stand together)"""
    out = {}
    for line in sam.split(b"\n")[:-1]:
        out.setdefault(line.split(b"\t", 1)[0], []).append(line)
    return out


def compose(fastq, forward_sam, reverse_sam, flag=b"16"):
    """the contract's text: per read in file order its lines of the forward run, then its lines of the run on rc(fastq)
    with the second field rewritten to `flag`"""
    fwd, rev = lines_of(forward_sam), lines_of(reverse_sam)
    names = [r[0] for r in fastq_reads(fastq)]
    assert len(set(names)) == len(names) and not any(b"\t" in n for n in names)
    out = []
    for n in names:
        out += fwd.get(n, [])
        out += [with_flag(l, flag) for l in rev.get(n, [])]
    return b"".join(l + b"\n" for l in out)


# ---- the fixture ----------------------------------------------------------------------------------------------------------
WHOLE_TEXT = ["test-out/k0", "test-out/k1", "test-out/k2", "hg38/reads-100-10-0/k0", "hg38/reads-100-10-0/k1",
              "two-records-flipped/k1", "two-records-flipped/k2"]
BY_DIGEST = "hg38/reads-100-10-0/k2"
NOTHING_REVERSE = ["hg38/reads-1000-100-2/k2", "hg38/reads-1000-200-1/k1", "two-records/k1"]
ALL_CASES = WHOLE_TEXT + [BY_DIGEST] + NOTHING_REVERSE


def flipped_fastq(fastq):
    """every read q % 3 == 1 replaced by its rc"""
    return fastq_image([rc(r) if q % 3 == 1 else r for q, r in enumerate(fastq_reads(fastq))])


def strand_cases():
    """name -> dict(fasta, fastq, k, and `want`, the composed text, or sha256 / lines / bytes / head / tail of it)"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "golden_sam_strands.npz"))
    base = sam_cases()
    groups = {}
    for key in z.files:
        name, field = key.rsplit("/", 1)
        groups.setdefault(name, {})[field] = z[key]
    out = {}
    for name, g in groups.items():
        src = base[g["base"].tobytes().decode()] if "base" in g else base[name]
        c = dict(k=int(g["k"][0]) if "k" in g else src["k"], fasta=src["fasta"])
        c["fastq"] = g["fastq"].tobytes() if "fastq" in g else src["fastq"]
        if "rev" in g:
            forward = g["fwd"].tobytes() if "fwd" in g else src["sam"]
            c["want"] = compose(c["fastq"], forward, g["rev"].tobytes())
            c["forward"] = forward
        else:
            c.update(sha256=g["sha256"].tobytes(), lines=int(g["lines"][0]), bytes=int(g["bytes"][0]), head=g["head"].tobytes(),
                     tail=g["tail"].tobytes())
        out[name] = c
    return out


def check_strands(case, got):
    """the text of a both-strands run against the fixture: the whole text, or its digest, counts, first and last 200 lines"""
    if "want" in case:
        assert len(got) == len(case["want"]), (len(got), len(case["want"]), skc.first_difference(got, case["want"]))
        assert got == case["want"], skc.first_difference(got, case["want"])
        return
    assert len(got) == case["bytes"]
    assert got.count(b"\n") == case["lines"]
    assert got.startswith(case["head"]) and got.endswith(case["tail"])
    assert hashlib.sha256(got).digest() == case["sha256"]


# ---- sx_fastq_strands_dev against rc() ------------------------------------------------------------------------------------
def expected_strands(fastq):
    """(names, name_off, seqs, seq_off, quals, qual_off, flags) of the read set of both strands, from rc()"""
    reads = [x for r in fastq_reads(fastq) for x in (r, rc(r))]
    out = []
    for k in range(3):
        data, off = skc.flat([r[k] for r in reads])
        out += [data[:-1].tobytes(), off.tolist()]
    return out + [[0, 16] * (len(reads) // 2)]


def _random_reads(rng, lengths, alphabet):
    reads = []
    for q, m in enumerate(lengths):
        name = b"read %d / x" % q if q % 3 else b"r%d" % q
        seq = bytes(rng.choice(alphabet, m).tolist())
        qual = bytes(rng.integers(33, 127, m, dtype=np.uint8).tolist())
        reads.append((name, seq, qual))
    return reads


def strand_images():
    """name -> (FASTQ image, shift of its first byte off a 16-byte boundary)"""
    rng = np.random.default_rng(31)
    dna = np.frombuffer(b"ACGT", np.uint8)
    iupac = np.frombuffer(b"ACGTURYKMBVDHSWNacgturykmbvdhswn*-.xZ", np.uint8)
    edges = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 2046]
    out = {"one-read-of-one-byte": (b"@r\nA\n+\n!\n", 0),
           "lengths-at-the-lanes-edges": (fastq_image(_random_reads(rng, edges, dna)), 0),
           "257-reads-mixed": (fastq_image(_random_reads(rng, rng.integers(1, 300, 257).tolist(), dna)), 0),
           "even-count": (fastq_image(_random_reads(rng, rng.integers(10, 120, 64).tolist(), dna)), 5),
           "iupac-and-case": (fastq_image(_random_reads(rng, [len(iupac)] + rng.integers(1, 80, 40).tolist(), iupac)), 0),
           "empty": (b"", 0)}
    # every letter of the table once, in both cases, and bytes outside it: in the sequence '*', '-' and 0x80 .. 0xFF; in the
    # quality line 0x80 .. 0xFF (a quality byte is never complemented: these must come out reversed and unchanged)
    every = bytes(iupac.tolist()) + bytes(range(0x80, 0x100)) + b"\x01\x7f@[`{"
    qual = bytes(range(0x80, 0x100)) + bytes(rng.integers(33, 127, len(every) - 128, dtype=np.uint8).tolist())
    out["bytes-outside-the-table"] = (fastq_image([(b"name with  blanks ", every, qual), (b"t\tab", b"ACGU", b"AC\x80T")]), 3)
    no_newline = fastq_image(_random_reads(rng, [7, 2046, 1, 33, 100], dna))
    out["no-final-newline"] = (no_newline[:-1], 1)
    # long reads only: every tile of 4096 output bytes lies inside one or two pairs
    out["longest-reads"] = (fastq_image([(b"n" * 2045, bytes(rng.choice(dna, 2046).tolist()), b"I" * 2045 + b"#")] * 5), 0)
    return out


STRAND_IMAGE_NAMES = ["one-read-of-one-byte", "lengths-at-the-lanes-edges", "257-reads-mixed", "even-count", "iupac-and-case", "empty",
                      "bytes-outside-the-table", "no-final-newline", "longest-reads"]


def check_strand_image(ctx, mem, image, shift):
    """sx_fastq_strands_dev of the image's device arrays against expected_strands; the 16 bytes behind each byte array are
    read with it (the harness's memory is the process's own: a read behind an allocation is what its sanitizer run sees)"""
    d_image = mem.to_dev(image, shift)
    d_flags = mem.zeros(max(2, len(image) // 4), np.uint16)
    mem.sync()
    arrays, flags, count = ctx.fastq_strands_dev(d_image, len(image), d_flags, spare=16)
    want = expected_strands(image)
    assert count == len(want[6])
    assert flags.tolist() == want[6]
    for k in range(3):
        data, off = arrays[2 * k], arrays[2 * k + 1]
        assert off.tolist() == want[2 * k + 1], k
        assert data.size == len(want[2 * k]) + 16
        assert data[:-16].tobytes() == want[2 * k], (k, skc.first_difference(data[:-16].tobytes(), want[2 * k]))
    again, flags2, _ = ctx.fastq_strands_dev(d_image, len(image), d_flags)  # the same bytes from run to run
    assert all(a.tobytes() == b[:a.size].tobytes() for a, b in zip(again, arrays)) and flags2.tolist() == want[6]


# ---- sx_sam_layout_dev_ex / sx_sam_emit_dev_ex over made-up hits -----------------------------------------------------------
FLAGS = [0, 16, 256, 65535]  # 1, 2, 3 and 5 digits, on neighbouring reads


class FlagBatch(skc.Batch):
    """skc.Batch through sx_sam_layout_dev_ex / sx_sam_emit_dev_ex: a FLAG per read, or the NULL that means FLAG 0"""

    def __init__(self, ctx, mem, case, flags):
        super().__init__(ctx, mem, skc.make_hits(case["rows"]), case["sa"], case["names"], case["seqs"], case["quals"], case["rnames"])
        self.d_flags = mem.to_dev(np.asarray(flags, np.uint16)) if flags is not None else None
        self.batch = _lib.SamBatchEx(self.batch, api._ptr(self.d_flags))
        mem.fill(self.d_off, 0xEE)
        mem.sync()
        self.total = ctx.sam_layout_dev(self.batch, self.d_off)
        self.off = mem.to_host(self.d_off, np.uint64)


def flagged_text(case, flags):
    """expected_text with every line's second field replaced by its read's FLAG"""
    sas, rnames = skc._as_lists(case["sa"], case["rnames"])
    lines = skc.text_of(case).split(b"\n")[:-1]
    reads = [q // len(rnames) for q, L, R, g in case["rows"] for _ in range(L, R)]
    assert len(reads) == len(lines)
    return b"".join(with_flag(l, b"%d" % flags[r]) + b"\n" for l, r in zip(lines, reads))


def flag_case():
    """four neighbouring reads with flags of 1, 2, 3 and 5 digits; a hit of 300 matches and one of 3000 on flagged reads
    (the size pass's long-interval path, and about 140 KB of lines: slices of either size in the hit's second half skip the
    emit's walk steps of 1024 lines), short hits around them"""
    rng = np.random.default_rng(41)
    sa = skc.mixed_sa(rng, 4000)
    rows = [(0, 3, 5, []), (1, 10, 310, [2]), (2, 0, 3, []), (3, 100, 3100, []), (1, 7, 8, [1 | 0x8000]), (0, 20, 21, []),
            (3, 5, 38, [0, 1]), (2, 40, 41, [])]
    return dict(name="flags", rows=rows, sa=sa, names=[b"q0", b"read one", b"r2", b"three"], seqs=[b"ACG", b"TTGAC", b"GG", b"ACGTACGT"],
                quals=[b"III", b"#!#!#", b"~~", b"12345678"], rnames=[b"chr"], flags=FLAGS, windows=[4099])


def small_flag_case():
    """the same reads with a few short hits: windows of 16 bytes, so that a "16" and a "65535" are cut by a window and, at the
    harness's 256 bytes, by a slice"""
    c = flag_case()
    rows = [(1, 10, 14, [2]), (0, 3, 5, []), (3, 100, 140, []), (2, 0, 3, []), (1, 7, 8, []), (3, 5, 9, [0, 1])]
    return dict(c, name="flags-small", rows=rows, windows=[16, 100])


def several_records_flag_case():
    """three records: the flag goes by read = query / records"""
    c = dict(skc.several_records_case())
    c["flags"] = [16, 0, 65535, 256]
    c["windows"] = [16, 4099]
    return c


def check_flags(ctx, mem, case):
    """offsets, total and text with flags against the Python rendering, window by window; without flags the bytes of
    the old entry points"""
    flags = case["flags"]
    want = flagged_text(case, flags)
    b = FlagBatch(ctx, mem, case, flags)
    # every hit's bytes: the unflagged offsets plus, per line, the flag's digits beyond the one of "0"
    plain = skc.expected_offsets(case["sa"], case["rows"], case["names"], case["seqs"], case["quals"], case["rnames"]).astype(np.int64)
    n_rec = len(skc._as_lists(case["sa"], case["rnames"])[1])
    extra = np.array([0] + [(R - L) * (len(b"%d" % flags[q // n_rec]) - 1) for q, L, R, g in case["rows"]], np.int64)
    want_off = plain + np.cumsum(extra)
    assert b.total == len(want) == int(want_off[-1])
    assert (b.off.astype(np.int64) == want_off).all()
    got = b.text()
    assert got == want, skc.first_difference(got, want)
    for window in case["windows"]:
        got = b.text(window)
        assert got == want, (window, skc.first_difference(got, want))
    none = FlagBatch(ctx, mem, case, None)
    old = skc.batch_of(ctx, mem, case)
    assert none.total == old.total and (none.off == old.off).all()
    assert none.text() == old.text() == skc.text_of(case)
    zeros = FlagBatch(ctx, mem, case, [0] * len(flags))
    assert zeros.text(case["windows"][0]) == old.text()
