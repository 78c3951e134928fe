"""Generates tests/golden/golden_sam_strands.npz: what the UNMODIFIED reference read mapper (compiled by plain gcc from
where its sources lie into a temporary directory outside the repository, as tests/golden/make_golden_sam.py does) prints
for the reverse complements of the reads of tests/golden/golden_sam.npz.  The fixture holds inputs and recorded output
only.

    python tests/golden/make_golden_sam_strands.py

Per case the mapper runs on the FASTQ image and on its rc image (tests/strand_cases.py rc_fastq: every read replaced by
its reverse complement under the same name).  The expected text of a both-strands run is the per-read composition of the
two outputs with FLAG 16 in the lines of the second (strand_cases.compose).  That this composition is what the reference
itself prints for both orientations is asserted here: its stdout on the interleaved image read0, rc(read0), read1, ... is
the composition with the FLAG left at 0.

Per case <name>/: rev (the stdout on the rc image); for the case that is not in golden_sam.npz (two-records-flipped: the
genome and reads of two-records/k1, every read q % 3 == 1 replaced by its rc) also base, fastq, k and fwd (the stdout on
the image itself); for the 45 MB case sha256 / lines / bytes / head / tail (first and last 200 lines) of the composition.
"""
import hashlib
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import strand_cases as sc  # noqa: E402
from make_golden_sam import build_mapper, run_mapper  # noqa: E402
from sam_cases import sam_cases  # noqa: E402


def main():
    base = sam_cases()
    flipped = sc.flipped_fastq(base["two-records/k1"]["fastq"])
    cases = [(name, name, base[name]["fastq"], base[name]["k"]) for name in sc.ALL_CASES if name in base]
    cases += [("two-records-flipped/k%d" % k, "two-records/k1", flipped, k) for k in (1, 2)]
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        assert not os.path.abspath(tmp).startswith(ROOT)
        exe = build_mapper(tmp)
        for name, src, fastq, k in cases:
            fasta = base[src]["fasta"]
            names = [r[0] for r in sc.fastq_reads(fastq)]
            assert len(set(names)) == len(names) and not any(b"\t" in n for n in names), name
            fwd = run_mapper(exe, tmp, fasta, fastq, k)
            if name in base and "sam" in base[name]:
                assert fwd == base[name]["sam"], name
            rev = run_mapper(exe, tmp, fasta, sc.rc_fastq(fastq), k)
            both = run_mapper(exe, tmp, fasta, sc.interleaved_fastq(fastq), k)
            assert both == sc.compose(fastq, fwd, rev, flag=b"0"), name
            want = sc.compose(fastq, fwd, rev)
            print("%-28s k=%d forward=%d reverse=%d lines, %d bytes composed" % (name, k, fwd.count(b"\n"), rev.count(b"\n"), len(want)))
            if name not in base:
                out[name + "/base"] = np.frombuffer(src.encode(), np.uint8)
                out[name + "/fastq"] = np.frombuffer(fastq, np.uint8)
                out[name + "/k"] = np.array([k], np.int32)
                out[name + "/fwd"] = np.frombuffer(fwd, np.uint8)
            if name == sc.BY_DIGEST:
                ls = want.split(b"\n")[:-1]
                out[name + "/sha256"] = np.frombuffer(hashlib.sha256(want).digest(), np.uint8)
                out[name + "/lines"] = np.array([len(ls)], np.uint64)
                out[name + "/bytes"] = np.array([len(want)], np.uint64)
                out[name + "/head"] = np.frombuffer(b"".join(l + b"\n" for l in ls[:200]), np.uint8)
                out[name + "/tail"] = np.frombuffer(b"".join(l + b"\n" for l in ls[-200:]), np.uint8)
            else:
                out[name + "/rev"] = np.frombuffer(rev, np.uint8)
    path = os.path.join(HERE, "golden_sam_strands.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    sys.exit(main())
