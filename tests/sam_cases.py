"""tests/golden/golden_sam.npz (tests/golden/make_golden_sam.py): the reference read mapper's stdout for a set of genomes,
reads and edit counts, and the helpers the CPU and GPU tests share.  TEST INFRASTRUCTURE ONLY."""
import hashlib
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sam_cases():
    """name -> dict(fasta bytes, fastq bytes, k, and sam bytes or sha256 / lines / bytes / head / tail)"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "golden_sam.npz"))
    genomes = np.load(os.path.join(ROOT, "tests", "golden", "golden_genomes.npz"))
    groups = {}
    for key in z.files:
        name, field = key.rsplit("/", 1)
        groups.setdefault(name, {})[field] = z[key]
    out = {}
    for name, g in groups.items():
        c = dict(k=int(g["k"][0]), fastq=g["fastq"].tobytes())
        c["fasta"] = genomes[g["genome"].tobytes().decode() + "/file"].tobytes() if "genome" in g else g["fasta"].tobytes()
        if "sam" in g:
            c["sam"] = g["sam"].tobytes()
        else:
            c.update(sha256=g["sha256"].tobytes(), lines=int(g["lines"][0]), bytes=int(g["bytes"][0]),
                     head=g["head"].tobytes(), tail=g["tail"].tobytes())
        out[name] = c
    return out


def check_case(case, got):
    """the text of a run against the fixture: the whole text, or its digest, counts, first and last 200 lines"""
    if "sam" in case:
        assert len(got) == len(case["sam"])
        assert got == case["sam"]
        return
    assert len(got) == case["bytes"]
    assert got.count(b"\n") == case["lines"]
    assert got.startswith(case["head"]) and got.endswith(case["tail"])
    assert hashlib.sha256(got).digest() == case["sha256"]


def subset_fastq(fastq, keep):
    """the records (four lines each) of a well-formed FASTQ image whose index is in `keep`"""
    lines = fastq.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    recs = [lines[i:i + 4] for i in range(0, len(lines), 4)]
    return b"".join(b"\n".join(recs[i]) + b"\n" for i in keep)


def lines_by_read(sam):
    """qname -> the concatenated lines of that read, in order"""
    out = {}
    for line in sam.split(b"\n")[:-1]:
        out.setdefault(line.split(b"\t", 1)[0], []).append(line)
    return out
