"""k-edit BWT search on the device (sx_bwt_approx_search_dev): 10^6 reads of 100 symbols with up to two planted
substitutions against a 2^28-symbol DNA record (tables of build_complete_table(rec, true) built on the device), at
k = 1 and 2.  Prints one JSON line: reads/s and hits per k, kernel ms of the count pass and of the whole call (HIP
events of the SX_KC_SEARCH class), the exact-search kernel's row look-up rate on the same reads in the same run, and the
reference iterator's rate on a sample of the reads (oracle/_ref over this library's tables, one CPU core).
--no-indels adds, per k and on the same reads, the search with indels=False (SX_SEARCH_NO_INDELS) beside the plain one, and
both again over the compact form of the tables (BWT blocks, sx_bwt_approx_search_compact_dev): hits, matches, the count
pass, the emit pass and the whole call; whether the flagged call at k = 0 returns the plain call's hits, and whether every
read has a hit with the flag (kept in profiles/no_indels_bench_2p28.json).

    python tools/approx_bench.py [--log2n 28] [--reads 1000000] [--ref-sample 200] [--ks 0,1,2 --no-indels]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--length", type=int, default=100)
    ap.add_argument("--ref-sample", type=int, default=200)
    ap.add_argument("--ks", default="1,2")
    ap.add_argument("--no-indels", action="store_true", help="also the search with indels=False, and both over compact blocks")
    args = ap.parse_args()
    import torch

    from stralg_amd import Context, synth
    import oracle

    ctx = Context(0)
    n, sigma, L = 1 << args.log2n, 5, args.length
    text = synth(n, sigma, 28)
    N = n + 1
    d_text = torch.from_numpy(np.concatenate([text, np.zeros(16, np.uint8)])).cuda()
    d_sa = torch.zeros(N, dtype=torch.int32, device="cuda")
    d_c = torch.zeros(sigma, dtype=torch.int32, device="cuda")
    d_o = torch.zeros((N + 1) * sigma, dtype=torch.int32, device="cuda")
    ctx.sa_build_dev(d_text, n, sigma, d_sa)
    d_bwt = torch.zeros(N + 16, dtype=torch.uint8, device="cuda") if args.no_indels else None
    d_occ = d_rocc = None

    def blocks():
        """the compact form of the table whose BWT is in d_bwt"""
        d_blocks = torch.zeros(ctx.occ_compact_bytes(N, sigma) + 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.occ_compact_build_dev(d_bwt, N, sigma, d_blocks)
        return d_blocks

    ctx.bwt_tables_dev(d_text, d_sa, N, sigma, d_c, d_o, d_bwt)
    if args.no_indels:
        d_occ = blocks()
    d_rev = torch.zeros(N + 16, dtype=torch.uint8, device="cuda")
    ctx.reverse_dev(d_text, n, d_rev)
    d_rsa = torch.zeros(N, dtype=torch.int32, device="cuda")
    d_c2 = torch.zeros_like(d_c)
    d_ro = torch.zeros_like(d_o)
    ctx.sa_build_dev(d_rev, n, sigma, d_rsa)
    ctx.bwt_tables_dev(d_rev, d_rsa, N, sigma, d_c2, d_ro, d_bwt)
    if args.no_indels:
        d_rocc = blocks()
    del d_rsa, d_c2, d_rev, d_text, d_bwt
    torch.cuda.empty_cache()

    # reads: text[a : a + L] with 0, 1 or 2 substitutions (a substitution moves a symbol to another of 1 .. 4)
    rng = np.random.default_rng(100)
    R = args.reads
    starts = rng.integers(0, n - L, R)
    reads = text[starts[:, None] + np.arange(L)[None, :]]
    for e in range(2):
        hit = rng.random(R) < (0.5 if e == 0 else 0.25)
        at = rng.integers(0, L, R)
        rows = np.flatnonzero(hit)
        reads[rows, at[rows]] = 1 + (reads[rows, at[rows]] % 4)
    flat = np.ascontiguousarray(reads.reshape(-1))
    off = (np.arange(R + 1, dtype=np.uint64) * L).astype(np.uint32)
    d_pat = torch.from_numpy(np.concatenate([flat, np.zeros(16, np.uint8)])).cuda()
    d_off = torch.from_numpy(off.view(np.int32)).cuda()
    d_hoff = torch.zeros(R + 1, dtype=torch.int64, device="cuda")

    def profiled(fn):
        ctx.profile_only("search")
        ctx.profile_enable(True)
        ctx.profile_reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        ms = ctx.profile_read()["search"]["ms"]
        ctx.profile_enable(False)
        return out, wall, ms

    # the exact search on the same reads: its rate of dependent row look-ups (2 a symbol)
    d_l = torch.zeros(R, dtype=torch.int32, device="cuda")
    d_r = torch.zeros_like(d_l)
    ctx.bwt_exact_search_dev(d_c, d_o, N, sigma, d_pat, d_off, R, d_l, d_r)
    _, _, ex_ms = profiled(lambda: ctx.bwt_exact_search_dev(d_c, d_o, N, sigma, d_pat, d_off, R, d_l, d_r))
    out = {"bench": "approx_search", "n": n, "sigma": sigma, "reads": R, "read_length": L,
           "exact": {"kernel_ms": round(ex_ms, 3), "row_lookups_per_s": round(2 * R * L / (ex_ms * 1e-3), 1)}}

    def measure(search, k):
        """(the figures of search(k, d_hoff[, d_hits, capacity]) on the reads, its hits on the host)"""
        total = search(k, d_hoff)  # warm-up, the count
        d_hits = torch.zeros(max(total, 1) * 32, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        search(k, d_hoff, d_hits, total)
        count_runs = [profiled(lambda: search(k, d_hoff)) for _ in range(3)]
        count_wall, count_ms = min(r[1] for r in count_runs), min(r[2] for r in count_runs)
        walls, mss = [], []
        for _ in range(3):
            _, wall, ms = profiled(lambda: search(k, d_hoff, d_hits, total))
            walls.append(wall)
            mss.append(ms)
        wall = min(walls)
        entry = {"hits": int(total), "matches": None, "wall_s": round(wall, 4), "reads_per_s": round(R / wall, 1),
                 "kernel_ms_count_pass": round(count_ms, 3), "kernel_ms_total": round(min(mss), 3),
                 "kernel_ms_emit_pass": round(min(mss) - count_ms, 3), "wall_ms_count_only": round(count_wall * 1e3, 3),
                 "kernel_ms_count_pass_runs": [round(r[2], 3) for r in count_runs], "kernel_ms_total_runs": [round(x, 3) for x in mss]}
        raw = d_hits[:total * 32].cpu().numpy()
        hits = raw.view([("q", "<u4"), ("L", "<u4"), ("R", "<u4"), ("rest", "V20")])
        entry["matches"] = int((hits["R"].astype(np.int64) - hits["L"]).sum())
        entry["reads_with_a_hit"] = int((d_hoff[1:] > d_hoff[:-1]).sum().item())
        del d_hits
        torch.cuda.empty_cache()
        return entry, raw

    def full(indels):
        return lambda k, *rest: ctx.bwt_approx_search_dev(d_c, d_o, d_ro, N, sigma, d_pat, d_off, R, k, *rest, indels=indels)

    def compact(indels):
        return lambda k, *rest: ctx.bwt_approx_search_compact_dev(d_c, d_occ, d_rocc, N, sigma, d_pat, d_off, R, k, *rest, indels=indels)

    for k in [int(x) for x in args.ks.split(",")]:
        entry, raw = measure(full(True), k)
        if args.no_indels:
            entry["no_indels"], flagged = measure(full(False), k)
            if k == 0:
                entry["no_indels"]["equals_the_plain_hits"] = bool(np.array_equal(flagged, raw))
            entry["no_indels"]["every_read_has_a_hit"] = entry["no_indels"]["reads_with_a_hit"] == R
            del flagged
            entry["compact"], c_raw = measure(compact(True), k)
            entry["compact"]["equals_the_full_tables_hits"] = bool(np.array_equal(c_raw, raw))
            del c_raw
            entry["compact"]["no_indels"], _ = measure(compact(False), k)
        del raw
        out[f"k{k}"] = entry

    # the reference iterator on a sample, one core, over this library's tables
    if oracle.have_ref() and args.ref_sample:
        from approx_cases import reference_table
        sa = d_sa.cpu().numpy().view(np.uint32)
        c = d_c.cpu().numpy().view(np.uint32)
        o = d_o.cpu().numpy().view(np.uint32).reshape(N + 1, sigma)
        ro = d_ro.cpu().numpy().view(np.uint32).reshape(N + 1, sigma)
        sample = [reads[q] for q in range(args.ref_sample)]
        search = reference_table(sa, c, o, ro, sigma)
        for k in [int(x) for x in args.ks.split(",")]:
            search(sample[:2], k)  # (page faults)
            t0 = time.perf_counter()
            search(sample, k)
            dt = time.perf_counter() - t0
            ref_rate = len(sample) / dt
            out[f"k{k}"]["reference_reads_per_s_one_core"] = round(ref_rate, 1)
            out[f"k{k}"]["speedup_vs_one_core"] = round(out[f"k{k}"]["reads_per_s"] / ref_rate, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
