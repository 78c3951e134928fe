"""Generates tests/golden/golden_approx.npz by running the UNMODIFIED reference's k-edit BWT search
(init_bwt_approx_iter / next_bwt_approx_match, stralg/bwt.c:226-422, in oracle/_ref/libstralg_ref.so built by
oracle/Makefile) in the build container.  The fixture holds inputs and the reference's outputs only; no tables (the
product builds them).

    python tests/golden/make_golden_approx.py

Cases (k in 0 .. 3):
  * the strings and patterns of the reference's own test (tests/stralg/approx_match_test.c:505-525), k = 1, 2
  * seeded random texts, sigma 2 .. 20, periodic and run-heavy ones among them, patterns of 1 .. ~120 symbols
    (pieces of the text, mutated pieces, random ones, and a few that give thousands of duplicate hits)
  * the caller's data: the record of tools/readmappers/data/genomes/hg38-10000.fa (its file is in golden_genomes.npz,
    so only its name is stored here) with reads of reads-1000-100-1.fq and reads-100-100-2.fq

Per case: raw (the text, or genome = file name), k, pat / pat_off (remapped patterns), and for mode "ro"
(build_complete_table(raw, true)) and "noro" (build_complete_table(raw, false)) the stream: q, pos, ml (per match, in
the iterator's order), cig_id (index into cig, the distinct CIGARs joined by NULs).
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import oracle  # noqa: E402
from oracle import pyoracle  # noqa: E402

REF = "/root/reference"


class Match(C.Structure):
    # stralg/bwt.h struct bwt_approx_match
    _fields_ = [("cigar", C.c_char_p), ("position", C.c_uint32), ("match_length", C.c_uint32)]


def reference_stream(ref, raw, patterns_raw, k, include_reverse):
    """remapped patterns (None where a letter is not in the text) and [(q, pos, ml, cigar)] of the reference iterator"""
    lib = ref.lib
    lib.init_bwt_approx_iter.argtypes = [C.c_void_p, C.POINTER(pyoracle._RefBwt), C.POINTER(C.c_uint8), C.c_int]
    lib.init_bwt_approx_iter.restype = None
    lib.next_bwt_approx_match.argtypes = [C.c_void_p, C.POINTER(Match)]
    lib.next_bwt_approx_match.restype = C.c_bool
    lib.dealloc_bwt_approx_iter.argtypes = [C.c_void_p]
    lib.dealloc_bwt_approx_iter.restype = None
    lib.remap.argtypes = [C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(pyoracle._RefRemap)]
    lib.remap.restype = C.c_void_p
    buf = np.zeros(len(raw) + 1, np.uint8)
    buf[:len(raw)] = np.frombuffer(raw, np.uint8)
    t = lib.build_complete_table(buf.ctypes.data_as(C.POINTER(C.c_uint8)), include_reverse)
    it = (C.c_uint8 * 512)()
    rems, stream = [], []
    for q, pr in enumerate(patterns_raw):
        pb = np.zeros(len(pr) + 1, np.uint8)
        pb[:len(pr)] = np.frombuffer(pr, np.uint8)
        rp = np.zeros(len(pr) + 1, np.uint8)
        if not lib.remap(rp.ctypes.data_as(C.POINTER(C.c_uint8)), pb.ctypes.data_as(C.POINTER(C.c_uint8)), t.contents.remap_table):
            rems.append(None)
            continue
        rems.append(rp[:len(pr)].copy())
        lib.init_bwt_approx_iter(it, t, rp.ctypes.data_as(C.POINTER(C.c_uint8)), k)
        mt = Match()
        while lib.next_bwt_approx_match(it, C.byref(mt)):
            stream.append((q, mt.position, mt.match_length, mt.cigar))
        lib.dealloc_bwt_approx_iter(it)
    lib.completely_free_bwt_table(t)
    return rems, stream


def fasta_sequence(data):
    return b"".join(l.strip() for l in data.splitlines() if not l.startswith(b">"))


def fastq_reads(path, count):
    lines = open(path, "rb").read().splitlines()
    return [lines[4 * r + 1].strip() for r in range(count)]


def main():
    oracle.build(ref=True)
    ref = oracle.ref()
    out = {}

    def add(name, raw, pats, k, genome=None):
        raw = bytes(raw)
        rems, ro = reference_stream(ref, raw, pats, k, True)
        keep = [q for q, r in enumerate(rems) if r is not None]
        assert keep, name
        pats = [pats[q] for q in keep]
        rems, ro = reference_stream(ref, raw, pats, k, True)
        _, noro = reference_stream(ref, raw, pats, k, False)
        if genome:
            out[name + "/genome"] = np.frombuffer(genome.encode(), np.uint8)
        else:
            out[name + "/raw"] = np.frombuffer(raw, np.uint8)
        out[name + "/k"] = np.array([k], np.int32)
        out[name + "/pat"] = np.concatenate(rems).astype(np.uint8)
        out[name + "/pat_off"] = np.concatenate([[0], np.cumsum([r.size for r in rems])]).astype(np.uint32)
        for mode, st in (("ro", ro), ("noro", noro)):
            cigs = sorted({s[3] for s in st})
            ids = {c: n for n, c in enumerate(cigs)}
            out[f"{name}/{mode}/q"] = np.array([s[0] for s in st], np.uint32)
            out[f"{name}/{mode}/pos"] = np.array([s[1] for s in st], np.uint32)
            out[f"{name}/{mode}/ml"] = np.array([s[2] for s in st], np.uint32)
            out[f"{name}/{mode}/cig_id"] = np.array([ids[s[3]] for s in st], np.uint32)
            out[f"{name}/{mode}/cig"] = np.frombuffer(b"\0".join(cigs) + b"\0", np.uint8)
        print(name, "k", k, "patterns", len(pats), "hits", len(ro), "same without RO" if ro == noro else "DIFFERENT without RO")

    # the reference's own test (approx_match_test.c:505-525)
    strings = [b"gacacacag", b"acacacag", b"acacaca", b"acactgaca", b"acataca", b"ccgc", b"acgc"]
    patterns = [b"acg", b"ac", b"a", b"g", b"c", b"acgc", b"aaa", b"acggc"]
    for s_i, s in enumerate(strings):
        for k in (1, 2):
            add(f"ref/s{s_i}/k{k}", s, patterns, k)

    rng = np.random.default_rng(20261016)
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", np.uint8)

    def pieces(text, count, lmin, lmax, mutate):
        out_p = []
        for _ in range(count):
            m = int(rng.integers(lmin, lmax + 1))
            a = int(rng.integers(0, max(1, text.size - m)))
            p = text[a:a + m].copy()
            if p.size < m:
                p = np.concatenate([p, rng.choice(text, m - p.size)])
            for _ in range(int(rng.integers(0, mutate + 1))):
                op, at = int(rng.integers(0, 3)), int(rng.integers(0, p.size))
                if op == 0:
                    p[at] = rng.choice(text)
                elif op == 1 and p.size > 1:
                    p = np.delete(p, at)
                else:
                    p = np.insert(p, at, rng.choice(text))
            out_p.append(p.tobytes())
        return out_p

    # seeded random texts, sigma 2 .. 20 (sigma counts the sentinel: sigma - 1 letters)
    # (patterns on small alphabets stay short: a binary text has a hit in every interval of a few symbols)
    for sigma in (2, 3, 4, 5, 8, 13, 20):
        for n, k in ((60, 3), (700, 2), (3000, 1), (3000, 0)):
            if sigma == 2:  # one letter: every piece of the text is everywhere
                n = max(12, n // 50)
            text = rng.choice(letters[:sigma - 1], n)
            lmax = 6 if sigma == 2 else {2: 14, 3: 20, 4: 30}.get(sigma, 40) if k >= 2 else (24 if sigma == 2 else 120)
            pats = pieces(text, 12, 1, lmax, k + 1) + [rng.choice(letters[:sigma - 1], 8).tobytes()]
            add(f"rand/s{sigma}/n{text.size}/k{k}", text.tobytes(), pats, k)
    # periodic and run-heavy texts (many duplicate hits)
    for name, text, k, lmax in (("periodic-ab", np.tile(np.frombuffer(b"ab", np.uint8), 100), 2, 12),
                                ("periodic-acgta", np.tile(np.frombuffer(b"acgtacgga", np.uint8), 60), 2, 30),
                                ("runs", np.repeat(rng.choice(letters[:4], 40), rng.integers(1, 20, 40)), 2, 16),
                                ("all-a", np.full(40, ord("a"), np.uint8), 2, 6)):
        pats = pieces(text, 10, 2, lmax, k) + [text[:8].tobytes()]
        add(f"struct/{name}", text.tobytes(), pats, k)
    # binary text, 12-symbol pattern, k = 3: tens of thousands of hits with duplicates
    text = rng.choice(letters[:2], 2000)
    add("struct/binary-dups", text.tobytes(), [text[100:112].tobytes()], 3)

    # the caller's data (bwt_readmapper -d 1 / 2 on hg38-10000.fa)
    gdir = f"{REF}/tools/readmappers/data"
    genome = fasta_sequence(open(f"{gdir}/genomes/hg38-10000.fa", "rb").read())
    # (the reads were sampled from a longer genome, hg38-1000000.fa, so most have no hit here: pieces of this record with
    #  up to k planted edits are searched beside them)
    gtext = np.frombuffer(genome, np.uint8)
    for fq, count, k in (("reads-1000-100-1.fq", 16, 1), ("reads-100-100-2.fq", 8, 2)):
        pats = fastq_reads(f"{gdir}/reads/{fq}", count) + pieces(gtext, 8, 100, 100, k)
        add(f"genome/{fq}/k{k}", genome, pats, k, genome="hg38-10000.fa")

    path = os.path.join(ROOT, "tests", "golden", "golden_approx.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
