"""Generates tests/golden/golden_sam.npz: the stdout of the UNMODIFIED reference read mapper
(tools/readmappers/bwt_readmapper/bwt_readmapper.c), compiled by plain gcc from where its sources lie into a temporary
directory outside the repository, run with -p and then -d K.  The fixture holds inputs (FASTA / FASTQ images) and the
recorded output only.

    python tests/golden/make_golden_sam.py

Per case <name>/: genome (the name of a file in golden_genomes.npz) or fasta (the image), fastq (the image), k, and
either sam (the whole text) or, for the 24 MB case, sha256 / lines / bytes / head / tail (first and last 200 lines).
"""
import glob
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("STRALG_REFERENCE", "/root/reference")
DATA = os.path.join(REF, "tools", "readmappers", "data")


def build_mapper(tmp):
    exe = os.path.join(tmp, "bwt_readmapper")
    src = [os.path.join(REF, "tools", "readmappers", "bwt_readmapper", "bwt_readmapper.c")]
    src += sorted(glob.glob(os.path.join(REF, "stralg", "*.c"))) + sorted(glob.glob(os.path.join(REF, "bioinf", "*.c")))
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-w", "-I" + os.path.join(REF, "stralg"),
                           "-I" + os.path.join(REF, "bioinf"), "-o", exe] + src)
    return exe


def run_mapper(exe, tmp, fasta, fastq, k):
    fa = os.path.join(tmp, "genome.fa")
    fq = os.path.join(tmp, "reads.fq")
    open(fa, "wb").write(fasta)
    open(fq, "wb").write(fastq)
    subprocess.check_call([exe, "-p", fa], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return subprocess.run([exe, "-d", str(k), fa, fq], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True).stdout


HAND_FASTQ = b"@r0 desc x\nCC\n+\n~~\n@r1\nAAA\n+anything\nIII\n@r2\nOO\n+\n!!\n@r3\nNN\n+\n##"


def two_record_case(hg):
    """a two-record genome cut from hg38-10000.fa's sequence (the second slice gets a few N) and 200 planted reads"""
    seq = b"".join(l.strip() for l in hg.splitlines() if not l.startswith(b">"))
    rng = np.random.default_rng(20261016)
    a = bytearray(seq[1000:31000])
    b = bytearray(seq[200000:240000])
    for p in rng.choice(len(b), 40, replace=False):
        b[int(p)] = ord("N")
    fasta = b">left slice\n" + bytes(a) + b"\n>right\n"
    fasta += b"\n".join(bytes(b[i:i + 60]) for i in range(0, len(b), 60)) + b"\n"
    reads = []
    for q in range(200):
        src = a if q % 2 == 0 else b
        m = int(rng.integers(20, 61))
        at = int(rng.integers(0, len(src) - m))
        r = bytearray(src[at:at + m])
        kind = q % 5
        if kind == 1:
            r[int(rng.integers(0, m))] = ord("ACGT"[int(rng.integers(0, 4))])
        elif kind == 2:
            del r[int(rng.integers(1, m - 1))]
        elif kind == 3:
            r.insert(int(rng.integers(1, m - 1)), ord("ACGT"[int(rng.integers(0, 4))]))
        if q % 17 == 0:
            r[int(rng.integers(0, len(r)))] = ord("N")
        qual = bytes(33 + int(v) for v in rng.integers(0, 40, len(r)))
        qual = qual.replace(b"@", b"A")
        reads.append(b"@planted%d src=%d\n%s\n+\n%s\n" % (q, q % 2, bytes(r), qual))
    return fasta, b"".join(reads)


def main():
    genomes = np.load(os.path.join(ROOT, "tests", "golden", "golden_genomes.npz"))
    hg = genomes["hg38-10000.fa/file"].tobytes()
    assert hg == open(os.path.join(DATA, "genomes", "hg38-10000.fa"), "rb").read()
    test_out = open(os.path.join(DATA, "genomes", "test-out.fa"), "rb").read()

    def reads(name):
        return open(os.path.join(DATA, "reads", name), "rb").read()

    two_fa, two_fq = two_record_case(hg)
    cases = [("test-out/k%d" % k, None, test_out, HAND_FASTQ, k, True) for k in (0, 1, 2)]
    cases += [("hg38/reads-100-10-0/k%d" % k, "hg38-10000.fa", hg, reads("reads-100-10-0.fq"), k, k < 2) for k in (0, 1, 2)]
    cases += [("hg38/reads-1000-100-2/k2", "hg38-10000.fa", hg, reads("reads-1000-100-2.fq"), 2, True),
              ("hg38/reads-1000-200-1/k1", "hg38-10000.fa", hg, reads("reads-1000-200-1.fq"), 1, True),
              ("two-records/k1", None, two_fa, two_fq, 1, True)]
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        assert not os.path.abspath(tmp).startswith(ROOT)
        exe = build_mapper(tmp)
        for name, genome, fasta, fastq, k, full in cases:
            sam = run_mapper(exe, tmp, fasta, fastq, k)
            lines = sam.count(b"\n")
            print("%-28s k=%d lines=%d bytes=%d sha256=%s" % (name, k, lines, len(sam), hashlib.sha256(sam).hexdigest()[:16]))
            if genome:
                out[name + "/genome"] = np.frombuffer(genome.encode(), np.uint8)
            else:
                out[name + "/fasta"] = np.frombuffer(fasta, np.uint8)
            out[name + "/fastq"] = np.frombuffer(fastq, np.uint8)
            out[name + "/k"] = np.array([k], np.int32)
            if full:
                out[name + "/sam"] = np.frombuffer(sam, np.uint8)
            else:
                ls = sam.split(b"\n")[:-1]
                out[name + "/sha256"] = np.frombuffer(hashlib.sha256(sam).digest(), np.uint8)
                out[name + "/lines"] = np.array([lines], np.uint64)
                out[name + "/bytes"] = np.array([len(sam)], np.uint64)
                out[name + "/head"] = np.frombuffer(b"".join(l + b"\n" for l in ls[:200]), np.uint8)
                out[name + "/tail"] = np.frombuffer(b"".join(l + b"\n" for l in ls[-200:]), np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "golden_sam.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    sys.exit(main())
