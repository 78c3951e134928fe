"""tests/golden/golden_approx.npz (tests/golden/make_golden_approx.py): the reference iterator's k-edit search streams,
and the helpers the CPU and GPU tests share to compare a search's hits with them.  TEST INFRASTRUCTURE ONLY."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _genome_raw(fname):
    z = np.load(os.path.join(ROOT, "tests", "golden", "golden_genomes.npz"))
    data = z[fname + "/file"].tobytes()
    return b"".join(l.strip() for l in data.splitlines() if not l.startswith(b">"))


def approx_cases():
    """name -> dict(raw bytes, k, patterns [uint8 arrays], pat, pat_off, streams {"ro": [...], "noro": [...]}) with a stream
    per pattern: [(position, match_length, cigar str)]"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "golden_approx.npz"))
    groups = {}
    for key in z.files:
        parts = key.split("/")
        if parts[-2] in ("ro", "noro"):
            name, mode, field = "/".join(parts[:-2]), parts[-2], parts[-1]
            groups.setdefault(name, {}).setdefault(mode, {})[field] = z[key]
        else:
            groups.setdefault("/".join(parts[:-1]), {})[parts[-1]] = z[key]
    genomes = {}
    out = {}
    for name, g in groups.items():
        if "genome" in g:
            fname = g["genome"].tobytes().decode()
            raw = genomes.setdefault(fname, _genome_raw(fname))
        else:
            raw = g["raw"].tobytes()
        off = g["pat_off"]
        pats = [g["pat"][off[q]:off[q + 1]] for q in range(off.size - 1)]
        streams = {}
        for mode in ("ro", "noro"):
            s = g[mode]
            cigs = s["cig"].tobytes().split(b"\0")
            per = [[] for _ in pats]
            for q, pos, ml, cid in zip(s["q"].tolist(), s["pos"].tolist(), s["ml"].tolist(), s["cig_id"].tolist()):
                per[q].append((pos, ml, cigs[cid].decode()))
            streams[mode] = per
        out[name] = dict(raw=raw, k=int(g["k"][0]), patterns=pats, pat=g["pat"], pat_off=off, streams=streams)
    return out


def remapped(raw):
    """(remapped symbols, alphabet_size) as stralg/remap.c builds them"""
    from stralg_amd import api
    t = api.alloc_remap_table(raw)
    return api.remap(raw, t), t.alphabet_size


def cigar_ok(pattern, text, pos, ml, cigar, k):
    """the CIGAR aligns the pattern to text[pos : pos + ml] with at most k edits (mismatches, I, D)"""
    import re
    ops = re.findall(r"(\d+)([MID])", cigar)
    p = t = edits = 0
    for n, op in ops:
        n = int(n)
        if op == "M":
            seg_p, seg_t = pattern[p:p + n], text[pos + t:pos + t + n]
            if len(seg_p) != n or len(seg_t) != n:
                return False
            edits += int(np.count_nonzero(np.asarray(seg_p) != np.asarray(seg_t)))
            p += n
            t += n
        elif op == "I":
            p += n
            edits += n
        else:
            t += n
            edits += n
    return p == len(pattern) and t == ml and pos + ml <= len(text) and edits <= k


def reference_matches(sa, c, o, ro, sigma, patterns, k):
    """the reference iterator (oracle/_ref, init_bwt_approx_iter / next_bwt_approx_match) over tables built by this
    library (stralg/bwt.h's struct layouts are the library's): per pattern [(position, match_length, cigar)].
    Needs oracle.have_ref()."""
    return reference_table(sa, c, o, ro, sigma)(patterns, k)


def reference_table(sa, c, o, ro, sigma):
    """the reference's struct bwt_table over these arrays; returns search(patterns, k) (reference_matches)"""
    import ctypes as C
    from oracle import pyoracle
    ref = pyoracle.ref()
    lib = ref.lib

    class Match(C.Structure):
        _fields_ = [("cigar", C.c_char_p), ("position", C.c_uint32), ("match_length", C.c_uint32)]

    lib.init_bwt_approx_iter.argtypes = [C.c_void_p, C.POINTER(pyoracle._RefBwt), C.POINTER(C.c_uint8), C.c_int]
    lib.init_bwt_approx_iter.restype = None
    lib.next_bwt_approx_match.argtypes = [C.c_void_p, C.POINTER(Match)]
    lib.next_bwt_approx_match.restype = C.c_bool
    lib.dealloc_bwt_approx_iter.argtypes = [C.c_void_p]
    lib.dealloc_bwt_approx_iter.restype = None
    sa = np.ascontiguousarray(sa, np.uint32)
    c = np.ascontiguousarray(c, np.uint32)
    o = np.ascontiguousarray(o, np.uint32)
    keep = [sa, c, o]
    rows = o.shape[0]

    def indices(tab):
        idx = (np.uint64(tab.ctypes.data) + np.arange(rows, dtype=np.uint64) * np.uint64(sigma * 4)).astype(np.uint64)
        keep.append(idx)
        return C.cast(idx.ctypes.data, C.POINTER(C.POINTER(C.c_uint32)))

    s = pyoracle._RefSA()
    s.length = sa.size
    s.array = sa.ctypes.data_as(C.POINTER(C.c_uint32))
    rt = pyoracle._RefRemap()
    rt.alphabet_size = sigma
    t = pyoracle._RefBwt()
    t.remap_table = C.pointer(rt)
    t.sa = C.pointer(s)
    t.c_table = c.ctypes.data_as(C.POINTER(C.c_uint32))
    t.o_table = o.ctypes.data_as(C.POINTER(C.c_uint32))
    t.o_indices = indices(o)
    if ro is not None:
        ro = np.ascontiguousarray(ro, np.uint32)
        keep.append(ro)
        t.ro_table = ro.ctypes.data_as(C.POINTER(C.c_uint32))
        t.ro_indices = indices(ro)
    def search(patterns, k):
        return _reference_run(lib, Match, t, keep, patterns, k)
    return search


def _reference_run(lib, Match, t, keep, patterns, k):
    import ctypes as C
    it = (C.c_uint8 * 512)()
    out = []
    for p in patterns:
        buf = np.zeros(len(p) + 1, np.uint8)
        buf[:len(p)] = p
        lib.init_bwt_approx_iter(it, C.byref(t), buf.ctypes.data_as(C.POINTER(C.c_uint8)), k)
        mt, res = Match(), []
        while lib.next_bwt_approx_match(it, C.byref(mt)):
            res.append((int(mt.position), int(mt.match_length), mt.cigar.decode()))
        lib.dealloc_bwt_approx_iter(it)
        out.append(res)
    return out
