"""Generates tests/golden/golden_sam_best.npz: what the UNMODIFIED reference read mapper (compiled by plain gcc from where
its sources lie into a temporary directory outside the repository, as tests/golden/make_golden_sam.py does) prints at
-d 0, -d 1 and -d 2 for a read set whose reads differ in their best stratum.  The fixture holds inputs and recorded output
only.

    python tests/golden/make_golden_sam_best.py

One case, two-records-best: the genome of two-records/k1 in golden_sam.npz and 240 planted reads of 30 .. 60 symbols from
a fixed seed, read q cut from record q % 2 and edited by q % 6: exact; one substitution to a different letter; one deletion;
one insertion; one substitution and one deletion; four substitutions.  Every read q % 5 == 1 is replaced by its reverse
complement (strand_cases.rc).  Recorded: the mapper's stdout at -d 0, 1, 2 on the FASTQ image (fwd0 .. fwd2) and on its rc
image (rev0 .. rev2).  The expected text of a best-stratum run is composed from these per read (tests/best_cases.py).

The generator fails unless, one strand and both strands alike, each of the four outcomes (e* = 0, 1, 2, none) has 20 reads
at least, and the file stays under 1 MiB.
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import best_cases as bc  # noqa: E402
import strand_cases as sc  # noqa: E402
from make_golden_sam import build_mapper, run_mapper  # noqa: E402
from sam_cases import sam_cases  # noqa: E402

SEED = 20261019
BASE = "two-records/k1"


def fasta_sequences(fasta):
    """the records' sequences, line breaks removed"""
    out = []
    for rec in fasta.split(b">")[1:]:
        out.append(b"".join(rec.split(b"\n")[1:]))
    return out


def other_letter(rng, c):
    return ord([x for x in "ACGT" if ord(x) != c][int(rng.integers(0, 3))])


def planted_reads(fasta):
    rng = np.random.default_rng(SEED)
    seqs = fasta_sequences(fasta)
    assert len(seqs) == 2
    reads = []
    for q in range(240):
        src = seqs[q % 2]
        m = int(rng.integers(30, 61))
        while True:
            at = int(rng.integers(0, len(src) - m))
            r = bytearray(src[at:at + m])
            if b"N" not in r:
                break
        kind = q % 6
        if kind in (1, 4):
            p = int(rng.integers(0, m))
            r[p] = other_letter(rng, r[p])
        if kind in (2, 4):
            del r[int(rng.integers(1, len(r) - 1))]
        if kind == 3:
            r.insert(int(rng.integers(1, m - 1)), ord("ACGT"[int(rng.integers(0, 4))]))
        if kind == 5:
            for p in rng.choice(m, 4, replace=False):
                r[int(p)] = other_letter(rng, r[int(p)])
        qual = bytes(33 + int(v) for v in rng.integers(0, 40, len(r))).replace(b"@", b"A")
        read = (b"best%d src=%d kind=%d" % (q, q % 2, kind), bytes(r), qual)
        reads.append(sc.rc(read) if q % 5 == 1 else read)
    return sc.fastq_image(reads)


def main():
    fasta = sam_cases()[BASE]["fasta"]
    fastq = planted_reads(fasta)
    out = {"two-records-best/base": np.frombuffer(BASE.encode(), np.uint8), "two-records-best/fastq": np.frombuffer(fastq, np.uint8)}
    with tempfile.TemporaryDirectory() as tmp:
        assert not os.path.abspath(tmp).startswith(ROOT)
        exe = build_mapper(tmp)
        fwd = [run_mapper(exe, tmp, fasta, fastq, k) for k in (0, 1, 2)]
        rev = [run_mapper(exe, tmp, fasta, sc.rc_fastq(fastq), k) for k in (0, 1, 2)]
    for k in (0, 1, 2):
        out["two-records-best/fwd%d" % k] = np.frombuffer(fwd[k], np.uint8)
        out["two-records-best/rev%d" % k] = np.frombuffer(rev[k], np.uint8)
        print("-d %d: forward %d bytes, rc %d bytes" % (k, len(fwd[k]), len(rev[k])))
    for both in (False, True):
        strata = bc.strata_of(fastq, fwd, rev if both else None, 2)
        counts = {e: strata.count(e) for e in (0, 1, 2, None)}
        text = bc.compose_best(fastq, fwd, rev if both else None, 2)
        print("both strands" if both else "one strand", counts, "best text: %d lines" % text.count(b"\n"))
        assert min(counts.values()) >= 20, counts
    path = os.path.join(HERE, "golden_sam_best.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    sys.exit(main())
