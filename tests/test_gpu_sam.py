"""The read mapper on the GPU (sx_sam.hip, sx_map_reads_stream, tools/stralg_amd_readmapper.c) against the reference
mapper's stdout in tests/golden/golden_sam.npz: through stralg_amd.map_reads and through the command-line tool."""
import hashlib
import os
import struct
import subprocess

import numpy as np
import pytest

from sam_cases import ROOT, check_case, lines_by_read, sam_cases
import stralg_amd

pytestmark = pytest.mark.gpu

MAPPER = os.path.join(ROOT, "tools", "stralg_amd_readmapper")
NAMES = ["test-out/k0", "test-out/k1", "test-out/k2", "hg38/reads-100-10-0/k0", "hg38/reads-100-10-0/k1",
         "hg38/reads-100-10-0/k2", "hg38/reads-1000-100-2/k2", "hg38/reads-1000-200-1/k1", "two-records/k1"]


@pytest.fixture(scope="module")
def cases():
    return sam_cases()


@pytest.fixture(scope="module")
def mapper():
    if not os.path.exists(MAPPER):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "stralg_amd", "csrc"), "mapper"])
    return MAPPER


@pytest.mark.parametrize("name", NAMES)
def test_map_reads_equals_the_reference(gpu_ctx, cases, name):
    c = cases[name]
    check_case(c, stralg_amd.map_reads(c["fasta"], c["fastq"], c["k"], ctx=gpu_ctx))


@pytest.mark.parametrize("name", NAMES)
def test_tool_equals_the_reference(mapper, cases, name, tmp_path):
    c = cases[name]
    fa, fq = tmp_path / "genome.fa", tmp_path / "reads.fq"
    fa.write_bytes(c["fasta"])
    fq.write_bytes(c["fastq"])
    subprocess.run([mapper, "-p", str(fa)], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    got = subprocess.run([mapper, "-d", str(c["k"]), str(fa), str(fq)], check=True, stdout=subprocess.PIPE,
                         stderr=subprocess.DEVNULL, timeout=300).stdout
    check_case(c, got)


def test_tool_writes_the_reference_tables_file(mapper, tmp_path):
    """-p: record count, name (length + bytes with the NUL), then the serialisation whose digest golden_genomes.npz
    holds from the reference writer"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "golden_genomes.npz"))
    fa = tmp_path / "hg38-10000.fa"
    fa.write_bytes(z["hg38-10000.fa/file"].tobytes())
    subprocess.run([mapper, "-p", str(fa)], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    data = open(str(fa) + ".bwttables", "rb").read()
    name = z["hg38-10000.fa/rec0/name"].tobytes()
    head = struct.pack("<I", 1) + struct.pack("<I", len(name) + 1) + name + b"\0"
    assert data.startswith(head)
    body = data[len(head):]
    assert len(body) == int(z["hg38-10000.fa/rec0/serial_with_reverse_len"][0])
    assert hashlib.sha256(body).digest() == z["hg38-10000.fa/rec0/serial_with_reverse_sha256"].tobytes()


def test_tool_reads_tables_of_the_reference_writer(mapper, gpu_ctx, tmp_path):
    """-d on a .bwttables file put together from the reference writer's own byte streams (tests/golden/golden_fasta.npz
    serial/*: two records, the file lists them last first), never on one the tool wrote: the lines equal map_reads' on the
    same genome, and for k = 0 the positions equal the occurrences that bytes.find gives"""
    from conftest import serial_cases
    sc = serial_cases()
    recs = [(b"fasta0", sc["ref-fasta0"]), (b"periodic", sc["struct-periodic"])]  # FASTA order
    fasta = b"".join(b">" + n + b"\n" + c["raw"] + b"\n" for n, c in recs)
    image = struct.pack("<I", len(recs))
    for n, c in reversed(recs):
        image += struct.pack("<I", len(n) + 1) + n + b"\0" + c["with_reverse"]
    fa, fq = tmp_path / "two.fa", tmp_path / "reads.fq"
    (tmp_path / "two.fa.bwttables").write_bytes(image)  # (two.fa itself is not written: -d reads the tables only)
    reads = []
    for n, c in recs:
        raw = c["raw"]
        for at in range(0, len(raw) - 12, max(1, len(raw) // 40)):
            reads.append(raw[at:at + 12])
    reads += [b"ACGTACGTAC", b"abcd", b"zz"]
    fq.write_bytes(b"".join(b"@q%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads)))
    for k in (0, 1):
        got = subprocess.run([mapper, "-d", str(k), str(fa), str(fq)], check=True, stdout=subprocess.PIPE,
                             stderr=subprocess.DEVNULL, timeout=300).stdout
        assert got == stralg_amd.map_reads(fasta, fq.read_bytes(), k, ctx=gpu_ctx)
        if k == 0:
            want = []
            for i, r in enumerate(reads):
                for n, c in recs:
                    at, found = c["raw"].find(r), []
                    while at >= 0:
                        found.append(at + 1)
                        at = c["raw"].find(r, at + 1)
                    want += [(b"q%d" % i, n, p) for p in found]
            lines = [l.split(b"\t") for l in got.split(b"\n")[:-1]]
            assert sorted((f[0], f[2], int(f[3])) for f in lines) == sorted(want) and len(want) > 80
            assert [(f[0], f[2]) for f in lines] == sorted(((f[0], f[2]) for f in lines),
                                                           key=lambda t: (int(t[0][1:]), t[1] != b"fasta0"))


def test_at_size_checked_without_the_code_under_test(gpu_ctx):
    """2^26 symbols of synthetic DNA, 10^5 reads of about 100 symbols, k = 1, through sx_sam_layout_dev / sx_sam_emit_dev in
    the default 32 MiB windows.  The hits are test_gpu_approx.py's; the text is split with numpy and every field is
    compared with what the hits, the suffix array and the reads say: positions with sa[L .. R), CIGARs with approx_cigar,
    names, sequences and qualities with the input, the line count with the sum of R - L."""
    import torch
    from test_gpu_approx import dev, device_tables, plant_reads
    from stralg_amd import _lib, api, synth
    n, sigma = 1 << 26, 5
    text = synth(n, sigma, 2026)
    d_sa, d_c, d_o, d_ro = device_tables(gpu_ctx, text, sigma)
    N = n + 1
    rng = np.random.default_rng(26)
    reads, _, _ = plant_reads(text, 100_000, 100, 2, rng)
    R = len(reads)
    off = np.concatenate([[0], np.cumsum([r.size for r in reads])]).astype(np.uint32)
    flat = np.concatenate(reads).astype(np.uint8)
    pad = np.zeros(16, np.uint8)
    letters = np.frombuffer(b"\0ACGT", np.uint8)[flat]
    quals = (33 + rng.integers(0, 60, flat.size)).astype(np.uint8)
    names = [b"read %d/%d" % (q, R) for q in range(R)]
    name_off = np.concatenate([[0], np.cumsum([len(x) for x in names])]).astype(np.uint32)
    rname = b"chrSynthetic26"
    d_pat, d_off = dev(np.concatenate([flat, pad])), dev(off, np.int32)
    d_names, d_name_off = dev(np.concatenate([np.frombuffer(b"".join(names), np.uint8), pad])), dev(name_off, np.int32)
    d_seqs, d_quals = dev(np.concatenate([letters, pad])), dev(np.concatenate([quals, pad]))
    d_rname, d_rname_off = dev(np.concatenate([np.frombuffer(rname, np.uint8), pad])), dev(np.array([0, len(rname)], np.int32))
    d_hoff = torch.zeros(R + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    total = gpu_ctx.bwt_approx_search_dev(d_c, d_o, d_ro, N, sigma, d_pat, d_off, R, 1, d_hoff)
    d_hits = torch.zeros(max(total, 1) * 32, dtype=torch.uint8, device="cuda")
    d_boff = torch.zeros(total + 1, dtype=torch.int64, device="cuda")
    window = 32 << 20
    d_win = torch.zeros(window, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert gpu_ctx.bwt_approx_search_dev(d_c, d_o, d_ro, N, sigma, d_pat, d_off, R, 1, d_hoff, d_hits, total) == total
    batch = gpu_ctx.sam_batch(d_hits, total, d_sa, N, d_names, d_name_off, d_seqs, d_off, d_quals, d_off, R, d_rname, d_rname_off)
    nbytes = gpu_ctx.sam_layout_dev(batch, d_boff)
    parts = []
    for lo in range(0, nbytes, window):
        hi = min(nbytes, lo + window)
        gpu_ctx.sam_emit_dev(batch, d_boff, nbytes, lo, hi, d_win)
        parts.append(d_win[:hi - lo].cpu().numpy().copy())
    sam = np.concatenate(parts)
    assert len(parts) >= 2 and sam.size == nbytes
    hits = d_hits.cpu().numpy()[:total * 32].view(_lib.APPROX_HIT_DTYPE)
    sa = d_sa.cpu().numpy().view(np.uint32)
    boff = d_boff.cpu().numpy().view(np.uint64)
    cnt = hits["R"].astype(np.int64) - hits["L"]
    n_lines = int(cnt.sum())
    assert total > 100_000 and (cnt > 0).all()
    # lines and fields: one '\n' a line at its end, ten '\t' a line
    nl = np.flatnonzero(sam == 10)
    tabs = np.flatnonzero(sam == 9)
    assert nl.size == n_lines and nl[-1] == nbytes - 1 and tabs.size == 10 * n_lines
    tabs = tabs.reshape(n_lines, 10)
    start = np.concatenate([[0], nl[:-1] + 1])
    assert (tabs[:, 0] > start).all() and (tabs[:, 9] < nl).all()
    hit_of_line = np.repeat(np.arange(total), cnt)
    first_line = np.concatenate([[0], np.cumsum(cnt)])
    assert (boff[:-1] == start[first_line[:-1]]).all() and boff[-1] == nbytes
    q = hits["query"][hit_of_line].astype(np.int64)
    # expected positions: sa[L + i] + 1
    within = np.arange(n_lines) - first_line[hit_of_line]
    want_pos = sa[hits["L"][hit_of_line].astype(np.int64) + within].astype(np.int64) + 1

    def field(k):  # (begin, end) of field k of every line
        b = start if k == 0 else tabs[:, k - 1] + 1
        e = tabs[:, k] if k < 10 else nl
        return b, e

    def equals(k, data, data_off, index):
        """field k of every line is data[data_off[index] : data_off[index + 1]]"""
        b, e = field(k)
        lo, hi = data_off[index].astype(np.int64), data_off[index + 1].astype(np.int64)
        assert ((e - b) == (hi - lo)).all(), k
        ln = (e - b)
        rows = np.repeat(np.arange(n_lines), ln)
        inner = np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln, ln)
        assert (sam[b[rows] + inner] == data[lo[rows] + inner]).all(), k

    equals(0, np.frombuffer(b"".join(names), np.uint8), name_off, q)
    equals(9, letters, off, q)
    equals(10, quals, off, q)
    rn = np.frombuffer(rname, np.uint8)
    equals(2, rn, np.array([0, rn.size]), np.zeros(n_lines, np.int64))
    for k, lit in ((1, b"0"), (4, b"0"), (6, b"*"), (7, b"0"), (8, b"0")):
        b, e = field(k)
        assert ((e - b) == 1).all() and (sam[b] == lit[0]).all(), k
    b, e = field(3)
    got_pos = np.zeros(n_lines, np.int64)
    for d in range(int((e - b).max())):
        live = b + d < e
        assert ((sam[b[live] + d] >= 48) & (sam[b[live] + d] <= 57)).all()
        got_pos[live] = got_pos[live] * 10 + (sam[b[live] + d] - 48)
    assert (got_pos == want_pos).all() and (sam[b] != 48).all()
    # CIGARs: one rendering per distinct (pattern length, gaps), compared as bytes
    b, e = field(5)
    lens = np.diff(off)
    cache = {}
    cig = []
    for h in range(total):
        key = (int(lens[hits["query"][h]]), tuple(int(g) for g in hits["gap"][h][:int(hits["n_gaps"][h])]))
        if key not in cache:
            cache[key] = api.approx_cigar(key[0], list(key[1])).encode()
        cig.append(cache[key])
    assert len(cache) > 100
    cig_off = np.concatenate([[0], np.cumsum([len(c) for c in cig])])
    equals(5, np.frombuffer(b"".join(cig), np.uint8), cig_off, hit_of_line)


def test_same_text_from_fresh_contexts(cases):
    c = cases["hg38/reads-100-10-0/k2"]
    digests = []
    for _ in range(2):
        ctx = stralg_amd.Context(0)
        try:
            digests.append(hashlib.sha256(stralg_amd.map_reads(c["fasta"], c["fastq"], c["k"], ctx=ctx)).digest())
        finally:
            ctx.close()
    assert digests[0] == digests[1] == c["sha256"]


@pytest.mark.parametrize("window,batch", [(1 << 16, 0), (1000, 0), (1 << 20, 9)])
def test_streamed_windows_and_batches(gpu_ctx, cases, window, batch):
    c = cases["hg38/reads-100-10-0/k1"]
    records = [(n, stralg_amd.build_complete_table(s, True, gpu_ctx)) for n, s in gpu_ctx.fasta_records(c["fasta"])]
    chunks = []
    gpu_ctx.set_sam_window_bytes(window)
    gpu_ctx.set_sam_batch_reads(batch)
    try:
        gpu_ctx.map_reads_stream(records, c["fastq"], c["k"], chunks.append)
    finally:
        gpu_ctx.set_sam_window_bytes(0)
        gpu_ctx.set_sam_batch_reads(0)
    assert len(chunks) > 1 and max(len(x) for x in chunks) <= (window + 15) // 16 * 16
    check_case(c, b"".join(chunks))


def test_skewed_batch_twenty_copies(gpu_ctx, cases):
    """the 2-edit case (two of its 100 reads own 102 395 lines each), 20 copies of the reads under distinct names: about
    0.5 GB of text; every copy's lines equal the single copy's but for the name"""
    c = cases["hg38/reads-100-10-0/k2"]
    single = stralg_amd.map_reads(c["fasta"], c["fastq"], c["k"], ctx=gpu_ctx)
    check_case(c, single)
    recs = c["fastq"].split(b"\n@")
    recs = [recs[0][1:]] + recs[1:]
    many = b"".join(b"@c%02d_" % copy + r.rstrip(b"\n") + b"\n" for copy in range(20) for r in recs)
    got = stralg_amd.map_reads(c["fasta"], many, c["k"], ctx=gpu_ctx)
    assert got.count(b"\n") == 20 * c["lines"]
    assert len(got) == 20 * (c["bytes"] + 4 * c["lines"])
    want = {name: hashlib.sha256(b"\n".join(ls)).digest() for name, ls in lines_by_read(single).items()}
    per = lines_by_read(got)
    assert len(per) == 20 * len(want)
    order = list(per)
    assert order == [b"c%02d_" % copy + name for copy in range(20) for name in lines_by_read(single)]
    for name, ls in per.items():
        assert hashlib.sha256(b"\n".join(l[4:] for l in ls)).digest() == want[name[4:]], name
