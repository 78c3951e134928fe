"""Generates tests/golden/golden_sam_edges.npz: what the UNMODIFIED reference read mapper (compiled by plain gcc from where
its sources lie into a temporary directory outside the repository, as tests/golden/make_golden_sam.py does) prints for three
inputs made for the edges of the mapper's loop.  The fixture holds inputs and recorded output only.

    python tests/golden/make_golden_sam_edges.py

Per case <name>/: fasta, fastq, fwd0 .. fwdK (the mapper's stdout at -d k on the FASTQ image) and rev0 .. revK (the same on
strand_cases.rc_fastq of the image).  The expected text of every call is composed from these (tests/edge_cases.py).

many-records (K = 3): 69 records -- one symbol; 300 symbols over the 20 amino-acid letters; 400 over ACGTacgt; 300 over
ACGTRYKMN; 64 ACGT records of 1 .. 119 symbols; two symbols -- in lines of 60.  An unmapped read first and last; 40 planted reads
of 10 .. 13 symbols, read q edited by q % 6 (exact; 1, 2, 3 substitutions; one insertion; one deletion), every q % 5 == 1
replaced by its reverse complement; 30 symbols of the soft-masked record; 20 of the protein record; the first 15 and the last
15 of the IUPAC record; a whole short record; XXXX.
block-edges (K = 1): ACGT records of 1, 2, 62, 63, 64, 126, 127, 128, 1023, 1024 and 5000 symbols and one of 700 over ACGTNRY, in
lines of 70.  For each record of 62 .. 1024 symbols: the whole record, its first 20, its last 20, the record with a letter
appended (the 5000-symbol record is longer than a FASTQ read may be: its first and last 20 alone); two reads of 2046 symbols
from the 5000-symbol record, the second with a substitution in the middle; 30 symbols under a name of 2045 bytes; ACG.
deep-k (K = 8): the records ACGTTGCA and TT, reads of 1 .. 4 symbols.

The generator fails unless the recordings cover what the cases are for (edge_cases.coverage) and the file stays under 1 MiB
(the largest text has 0.57 MB and the file 0.25 MB, so every text is stored whole and none by its digest).
It prints the counts that edge_cases.TABLE and edge_cases.PAIRS assert.
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

import edge_cases as ec  # noqa: E402
import strand_cases as sc  # noqa: E402
from make_golden_sam import build_mapper, run_mapper  # noqa: E402

SEED = 20261021
AMINO = b"ACDEFGHIKLMNPQRSTVWY"


def letters(rng, alphabet, n):
    return bytes(rng.choice(np.frombuffer(alphabet, np.uint8), n).tolist())


def fasta_image(records, width):
    return b"".join(b">%s\n" % name + b"".join(seq[i:i + width] + b"\n" for i in range(0, len(seq), width)) for name, seq in records)


def quality(rng, m):
    return bytes(33 + int(v) for v in rng.integers(0, 40, m)).replace(b"@", b"A")


def other_letter(rng, c, alphabet):
    rest = [x for x in alphabet if x != c]
    return rest[int(rng.integers(0, len(rest)))]


def many_records():
    rng = np.random.default_rng(SEED)
    records = [(b"single", b"G"), (b"protein", letters(rng, AMINO, 300))]
    records += [(b"short%d" % r, letters(rng, b"ACGT", int(rng.integers(1, 120)))) for r in range(32)]
    records += [(b"soft masked", letters(rng, b"ACGTacgt", 400))]
    records += [(b"short%d" % r, letters(rng, b"ACGT", int(rng.integers(1, 120)))) for r in range(32, 64)]
    records += [(b"iupac", letters(rng, b"ACGTRYKMN", 300)), (b"pair", b"CA")]
    by = dict(records)
    shorts = [seq for name, seq in records if name.startswith(b"short") and len(seq) >= 30]
    reads = [(b"lost-first", b"XQXQXQXQXQ")]
    for q in range(40):
        kind = q % 6
        m = 13 if kind in (2, 3) else int(rng.integers(10, 14))
        src = shorts[int(rng.integers(0, len(shorts)))]
        at = int(rng.integers(0, len(src) - m - 1))
        r = bytearray(src[at:at + m])
        if kind in (1, 2, 3):
            for p in rng.choice(m, kind, replace=False):
                r[int(p)] = other_letter(rng, r[int(p)], b"ACGT")
        elif kind == 4:
            r.insert(int(rng.integers(1, m - 1)), b"ACGT"[int(rng.integers(0, 4))])
        elif kind == 5:
            del r[int(rng.integers(1, m - 1))]
        reads.append((b"planted%d kind=%d" % (q, kind), bytes(r)))
    reads.append((b"soft30", by[b"soft masked"][200:230]))
    reads.append((b"protein20", by[b"protein"][100:120]))
    reads.append((b"iupac-first15", by[b"iupac"][:15]))
    reads.append((b"iupac-last15", by[b"iupac"][-15:]))
    whole = next(seq for name, seq in records if name.startswith(b"short") and 14 <= len(seq) <= 40)
    reads += [(b"whole-record", whole), (b"in-no-record", b"XXXX"), (b"lost-last", b"ZZZZZZZZZZZZ")]
    reads = [(name, seq, quality(rng, len(seq))) for name, seq in reads]
    reads = [sc.rc(r) if r[0].startswith(b"planted") and q % 5 == 2 else r for q, r in enumerate(reads)]  # (planted q: reads[q + 1])
    return fasta_image(records, 60), sc.fastq_image(reads)


def block_edges():
    rng = np.random.default_rng(SEED + 1)
    records = [(b"n%d" % n, letters(rng, b"ACGT", n)) for n in (1, 2, 62, 63, 64, 126, 127, 128, 1023, 1024)]
    records.insert(5, (b"n5000", letters(rng, b"ACGT", 5000)))
    records.insert(9, (b"n700 of seven", letters(rng, b"ACGTNRY", 700)))
    reads = []
    for name, seq in records:
        n = len(seq)
        if n < 62:
            continue
        alphabet = b"ACGTNRY" if n == 700 else b"ACGT"
        if n <= 2045:
            reads.append((b"whole-%d" % n, seq))
            reads.append((b"longer-%d" % n, seq + letters(rng, alphabet, 1)))
        reads += [(b"first20-%d" % n, seq[:20]), (b"last20-%d" % n, seq[-20:])]
    big = dict(records)[b"n5000"]
    cut = bytearray(big[1500:1500 + 2046])
    reads.append((b"cut-2046", bytes(cut)))
    cut[1023] = other_letter(rng, cut[1023], b"ACGT")
    reads.append((b"cut-2046 one substitution", bytes(cut)))
    reads.append((b"long-name-" + b"n" * 2035, big[4000:4030]))
    reads.append((b"acg", b"ACG"))
    return fasta_image(records, 70), sc.fastq_image([(name, seq, quality(rng, len(seq))) for name, seq in reads])


def deep_k():
    rng = np.random.default_rng(SEED + 2)
    reads = [(b"acg", b"ACG"), (b"tt", b"TT"), (b"one", b"A"), (b"three g", b"GGG"), (b"in no record", b"X"), (b"four a", b"AAAA"),
             (b"ctag", b"CTAG")]
    return b">eight\nACGTTGCA\n>two\nTT\n", sc.fastq_image([(name, seq, quality(rng, len(seq))) for name, seq in reads])


def main():
    inputs = {"many-records": many_records(), "block-edges": block_edges(), "deep-k": deep_k()}
    assert list(inputs) == list(ec.CASES)
    out, cases = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        assert not os.path.abspath(tmp).startswith(ROOT)
        exe = build_mapper(tmp)
        for name, (fasta, fastq) in inputs.items():
            ks = range(ec.CASES[name] + 1)
            fwd = [run_mapper(exe, tmp, fasta, fastq, k) for k in ks]
            rev = [run_mapper(exe, tmp, fasta, sc.rc_fastq(fastq), k) for k in ks]
            cases[name] = dict(fasta=fasta, fastq=fastq, fwd=fwd, rev=rev)
            out[name + "/fasta"], out[name + "/fastq"] = np.frombuffer(fasta, np.uint8), np.frombuffer(fastq, np.uint8)
            for k in ks:
                out["%s/fwd%d" % (name, k)], out["%s/rev%d" % (name, k)] = np.frombuffer(fwd[k], np.uint8), np.frombuffer(rev[k], np.uint8)
                print("%s -d %d: forward %d bytes, rc %d bytes" % (name, k, len(fwd[k]), len(rev[k])))
    for what, n in ec.coverage(cases).items():
        print("%-24s %s" % (what, n))
    print("TABLE = {")
    for name, K in ec.CASES.items():
        for k in range(K + 1):
            print("    " + " ".join("(%r, %d, %r): %r," % (name, k, f, ec.counts_of(ec.want(cases[name], k, **flags))) for f, flags in ec.FLAG_SETS.items()))
    print("}\nPAIRS = {")
    for key in (("many-records", 1, True, False), ("many-records", 2, True, False), ("block-edges", 1, True, False)):
        p = ec.pair_case(cases[key[0]], *key[1:])
        print("    %r: %r," % (key, (p["want"].count(b"\n"), p["pairs"])))
    print("}")
    path = os.path.join(HERE, "golden_sam_edges.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    sys.exit(main())
