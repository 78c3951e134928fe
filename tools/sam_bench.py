"""SAM text of k-edit search hits on the device (sx_sam_layout_dev / sx_sam_emit_dev): the reads and the 2^28-symbol DNA
record of tools/approx_bench.py, k = 1 and 2.  Prints one JSON line (kept in profiles/sam_bench_2p28.json): per k the hits,
lines and bytes of text, ms and GB/s of the layout pass and of the emit pass into device memory (HIP events of the
SX_KC_SAM class; the emit pass fills one window buffer again and again) next to the bytes each moves, the search's kernel
ms on the same batch, the box's fill rate (sx_membw_probe), the rate of a plain pinned device-to-host copy, and the
streamed form (sx_map_reads_stream from host tables through a sink that discards) as wall time and as the rate of its
windows, a fraction of that copy rate; the host's FASTQ index pass.  --repeats N times every figure N times (the runs stand
next to their best as *_runs: the run-to-run spread that a comparison between two builds has to exceed).  --both-strands
adds the strand kernel (sx_fastq_strands_dev: ms, bytes moved, against the probe's copy rate) and the streamed call with
SX_MAP_BOTH_STRANDS (kept in profiles/strands_bench_2p28.json).  --best adds, per k, sx_bwt_best_search_dev on the same
batch (wall, kernel ms of the search and of the select class, hits and lines), its rounds replayed through the public
calls (per round: groups in and found; the count pass, the two selects with their bytes against the probe's copy rate, the
emit pass as the difference of the search over the found set with and without its hits) and the streamed call with
SX_MAP_BEST_STRATUM beside the plain one of the same run (kept in profiles/best_bench_2p28.json).  --no-indels adds, per k
and on the same reads, the search with indels=False (SX_SEARCH_NO_INDELS): its hits, lines and text bytes, the search's
kernel ms (every run: the spread), layout and emit over its hits, and the streamed call with SX_MAP_NO_INDELS (with --best:
also with both flags) beside the plain one (kept in profiles/no_indels_bench_2p28.json).  --tags adds, per k (and per
no-indels entry), layout and emit over the same hits with NM:i and MD:Z behind QUAL (sx_sam_layout_dev_tags /
sx_sam_emit_dev_tags), and the call through a resident index with its strings (Index.map_reads_discard) with and without
tags=True (kept in profiles/tags_bench_2p28.json).  --pairs adds paired-end reads: every read gets a
mate drawn 200 - 499 symbols downstream on the other strand, with the same substitution rates, and per k Index.map_pairs_discard
with indels=False, and with best=True as well, on the two files: the call's wall time, the kernel ms of its five classes
(pair_count, pair_scan, pair_fill, pair_layout, pair_emit; a run of their own with every launch timed), the emit's rate over
its text against the plain emit's, and the wall time of the two both_strands calls on the two files with the same flags
(kept in profiles/pairs_bench_2p28.json).  --unmapped adds FLAG 4 lines for the reads without a hit (SX_MAP_UNMAPPED, DESIGN.md
section 22): per k the reads without a hit and the bytes their lines add, layout and emit over the same hits with a
placeholder a read without one (sx_sam_layout_dev_unmapped / sx_sam_emit_dev_unmapped) and the cost per added byte against
the plain passes' rate, and the streamed call with and without unmapped=True, its kernel ms of the search and of the sam
class each in a run of its own (kept in profiles/unmapped_bench_2p28.json).  --mapq adds MAPQ and secondary flags from the best
stratum (SX_MAP_MAPQ): per k (and per no-indels entry) the best-stratum hits of the batch with every read's
first hit split and a quality word a hit, made here as the mapper's quality pass makes them, layout and emit of their text
through sx_sam_layout_dev_mapq / sx_sam_emit_dev_mapq beside the plain passes over the same hits, and the streamed call with
best=True with and without mapq=True: wall, bytes, and the kernel ms of its mapq class (the quality pass: two scans and three
kernels a batch) and of its sam class, each in a run of its own (kept in profiles/mapq_bench_2p28.json).

    python tools/sam_bench.py [--log2n 28] [--reads 1000000] [--window-mib 1024] [--repeats 5] [--both-strands] [--best] [--no-indels] [--tags] [--pairs] [--unmapped] [--mapq]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--length", type=int, default=100)
    ap.add_argument("--window-mib", type=int, default=1024)
    ap.add_argument("--ks", default="1,2")
    ap.add_argument("--reference-lines-per-s", type=float, default=0.0,
                    help="the reference mapper's rate measured elsewhere, recorded in the line as given")
    ap.add_argument("--repeats", type=int, default=1, help="time layout, emit and the streamed call so many times")
    ap.add_argument("--both-strands", action="store_true", help="also the strand kernel and the streamed call on both strands")
    ap.add_argument("--best", action="store_true", help="also the best-stratum search, its rounds and the streamed call with best=True")
    ap.add_argument("--no-indels", action="store_true", help="also the search, the text and the streamed call without indels")
    ap.add_argument("--tags", action="store_true", help="also layout, emit and the index call with NM:i and MD:Z on every line")
    ap.add_argument("--pairs", action="store_true", help="also the paired call on the reads and their mates, indels=False without and with best=True")
    ap.add_argument("--unmapped", action="store_true", help="also layout, emit and the streamed call with a FLAG 4 line for every read without a hit")
    ap.add_argument("--mapq", action="store_true", help="also layout, emit and the streamed best call with MAPQ and secondary flags")
    args = ap.parse_args()
    import torch

    from stralg_amd import Context, synth

    ctx = Context(0)
    n, sigma, L = 1 << args.log2n, 5, args.length
    text = synth(n, sigma, 28)
    N = n + 1
    d_text = torch.from_numpy(np.concatenate([text, np.zeros(16, np.uint8)])).cuda()
    d_sa = torch.zeros(N, dtype=torch.int32, device="cuda")
    d_c = torch.zeros(sigma, dtype=torch.int32, device="cuda")
    d_o = torch.zeros((N + 1) * sigma, dtype=torch.int32, device="cuda")
    ctx.sa_build_dev(d_text, n, sigma, d_sa)
    ctx.bwt_tables_dev(d_text, d_sa, N, sigma, d_c, d_o)
    d_rev = torch.zeros(N + 16, dtype=torch.uint8, device="cuda")
    ctx.reverse_dev(d_text, n, d_rev)
    d_rsa = torch.zeros(N, dtype=torch.int32, device="cuda")
    d_c2 = torch.zeros_like(d_c)
    d_ro = torch.zeros_like(d_o)
    ctx.sa_build_dev(d_rev, n, sigma, d_rsa)
    ctx.bwt_tables_dev(d_rev, d_rsa, N, sigma, d_c2, d_ro)
    # (--tags: the remapped text, its sentinel behind it, stays; its letters are those of the reads below)
    d_texts = torch.tensor([d_text.data_ptr()], dtype=torch.int64, device="cuda") if args.tags else None
    d_letters = torch.from_numpy(np.frombuffer(b"\0ACGT" + bytes(251), np.uint8).copy()).cuda() if args.tags else None
    d_text_kept = d_text if args.tags else None
    del d_rsa, d_c2, d_rev, d_text
    torch.cuda.empty_cache()

    # the reads of tools/approx_bench.py; as a FASTQ file they are named read<q>, letters ACGT, quality '~'
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
    names = [b"read%d" % q for q in range(R)]
    name_off = np.zeros(R + 1, np.uint32)
    name_off[1:] = np.cumsum([len(x) for x in names])
    pad = np.zeros(16, np.uint8)
    d_pat = torch.from_numpy(np.concatenate([flat, pad])).cuda()
    d_off = torch.from_numpy(off.view(np.int32)).cuda()
    d_names = torch.from_numpy(np.concatenate([np.frombuffer(b"".join(names), np.uint8), pad])).cuda()
    d_name_off = torch.from_numpy(name_off.view(np.int32)).cuda()
    d_seqs = torch.from_numpy(np.concatenate([np.frombuffer(b"\0ACGT", np.uint8)[flat], pad])).cuda()
    d_quals = torch.full((R * L + 16,), ord("~"), dtype=torch.uint8, device="cuda")
    d_rname = torch.from_numpy(np.concatenate([np.frombuffer(b"chr1", np.uint8), pad])).cuda()
    d_rname_off = torch.tensor([0, 4], dtype=torch.int32, device="cuda")
    d_hoff = torch.zeros(R + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()  # (torch fills on its own stream)

    def profiled(kclass, fn):
        ctx.profile_only(kclass)
        ctx.profile_enable(True)
        ctx.profile_reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        ms = ctx.profile_read()[kclass]["ms"]
        ctx.profile_enable(False)
        return res, wall, ms

    window = args.window_mib << 20
    d_win = torch.zeros(window + 16, dtype=torch.uint8, device="cuda")
    d_other = torch.zeros(window + 16, dtype=torch.uint8, device="cuda")
    probe = ctx.membw_probe(d_win, d_other, window, 5)
    del d_other
    h_pin = torch.empty(min(window, 256 << 20), dtype=torch.uint8).pin_memory()
    link = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h_pin.copy_(d_win[:h_pin.numel()], non_blocking=True)
        torch.cuda.synchronize()
        link.append(h_pin.numel() / (time.perf_counter() - t0) / 1e9)
    out = {"bench": "sam_text", "n": n, "sigma": sigma, "reads": R, "read_length": L, "window_bytes": window,
           "membw_probe_GBps": {"read": round(probe["read"], 1), "fill": round(probe["fill"], 1), "copy": round(probe["copy"], 1)},
           "pinned_d2h_copy_GBps": round(max(link), 2)}

    def text_of_search(k, indels):
        """the figures of the search and of the text of its hits"""
        total = ctx.bwt_approx_search_dev(d_c, d_o, d_ro, N, sigma, d_pat, d_off, R, k, d_hoff, indels=indels)
        d_hits = torch.zeros(max(total, 1) * 32, dtype=torch.uint8, device="cuda")
        d_boff = torch.zeros(total + 1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        search_runs = [profiled("search", lambda: ctx.bwt_approx_search_dev(d_c, d_o, d_ro, N, sigma, d_pat, d_off, R, k,
                                                                           d_hoff, d_hits, total, indels=indels))
                       for _ in range(args.repeats)]
        search_ms = min(r[2] for r in search_runs)
        batch = ctx.sam_batch(d_hits, total, d_sa, N, d_names, d_name_off, d_seqs, d_off, d_quals, d_off, R, d_rname,
                              d_rname_off, 1)
        ctx.sam_layout_dev(batch, d_boff)  # warm-up
        layout_runs = [profiled("sam", lambda: ctx.sam_layout_dev(batch, d_boff)) for _ in range(args.repeats)]
        nbytes, layout_ms = layout_runs[0][0], min(r[2] for r in layout_runs)
        words = d_hits[:total * 32].view(torch.int32).reshape(-1, 8)  # (query, L, R, ...)
        lines = int(((words[:, 2].to(torch.int64) & 0xFFFFFFFF) - (words[:, 1].to(torch.int64) & 0xFFFFFFFF)).sum().item())
        del words

        def emit_all():
            for lo in range(0, nbytes, window):
                ctx.sam_emit_dev(batch, d_boff, nbytes, lo, min(nbytes, lo + window), d_win)

        ctx.sam_emit_dev(batch, d_boff, nbytes, 0, min(nbytes, window), d_win)  # warm-up
        emit_runs = [profiled("sam", emit_all) for _ in range(args.repeats)]
        emit_wall, emit_ms = min(r[1] for r in emit_runs), min(r[2] for r in emit_runs)
        layout_bytes = total * (32 + 16) + lines * 4
        emit_bytes = nbytes + lines * 4 + total * 32
        entry = {"hits": int(total), "lines": lines, "text_bytes": int(nbytes),
                 "search_kernel_ms": round(search_ms, 3),
                 "layout_ms": round(layout_ms, 3), "layout_bytes": int(layout_bytes),
                 "layout_GBps": round(layout_bytes / (layout_ms * 1e-3) / 1e9, 1),
                 "emit_ms": round(emit_ms, 3), "emit_wall_ms": round(emit_wall * 1e3, 3), "emit_bytes": int(emit_bytes),
                 "emit_GBps": round(emit_bytes / (emit_ms * 1e-3) / 1e9, 1),
                 "emit_fraction_of_fill": round(emit_bytes / (emit_ms * 1e-3) / 1e9 / probe["fill"], 3),
                 "lines_per_s": round(lines / ((layout_ms + emit_ms) * 1e-3), 1)}
        if args.repeats > 1:
            entry["search_kernel_ms_runs"] = [round(r[2], 3) for r in search_runs]
            entry["layout_ms_runs"] = [round(r[2], 3) for r in layout_runs]
            entry["emit_ms_runs"] = [round(r[2], 3) for r in emit_runs]
        if args.tags:  # the same hits with the two fields on every line
            tb = ctx.sam_batch_tags(batch, d_texts, d_letters)
            ctx.sam_layout_dev(tb, d_boff)  # warm-up
            t_layout = [profiled("sam", lambda: ctx.sam_layout_dev(tb, d_boff)) for _ in range(args.repeats)]
            t_bytes = t_layout[0][0]

            def emit_tagged():
                for lo in range(0, t_bytes, window):
                    ctx.sam_emit_dev(tb, d_boff, t_bytes, lo, min(t_bytes, lo + window), d_win)

            ctx.sam_emit_dev(tb, d_boff, t_bytes, 0, min(t_bytes, window), d_win)  # warm-up
            t_emit = [profiled("sam", emit_tagged) for _ in range(args.repeats)]
            tl, te = min(r[2] for r in t_layout), min(r[2] for r in t_emit)
            # beside the untagged passes' bytes: a text window of the read's length a hit in either pass
            t_emit_bytes = t_bytes + lines * 4 + total * (32 + L)
            entry["tags"] = {"text_bytes": int(t_bytes), "layout_ms": round(tl, 3), "layout_ms_runs": [round(r[2], 3) for r in t_layout],
                             "emit_ms": round(te, 3), "emit_ms_runs": [round(r[2], 3) for r in t_emit], "emit_bytes": int(t_emit_bytes),
                             "emit_GBps": round(t_emit_bytes / (te * 1e-3) / 1e9, 1),
                             "layout_plus_emit_over_untagged": round((tl + te) / (layout_ms + emit_ms), 3),
                             "layout_plus_emit_over_search": round((tl + te) / search_ms, 4)}
        if args.unmapped:
            entry["unmapped"] = unmapped_passes(total, d_hits, layout_ms, emit_ms, nbytes)
        del d_hits, d_boff
        torch.cuda.empty_cache()
        if args.mapq:
            entry["mapq"] = mapq_passes(k, indels)
        return entry

    def mapq_passes(k, indels):
        """the best-stratum hits of the batch (one record: they stand in (read, hit) order) as the mapper's quality pass leaves
        them -- every read's first hit split where it has more than one row, a quality word an entry --, then layout and emit
        of that text with the quality words and, over the same entries, without"""
        d_stratum = torch.zeros(R, dtype=torch.uint8, device="cuda")
        d_bho = torch.zeros(R + 1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        total = ctx.bwt_best_search_dev(d_c, d_o, d_ro, N, sigma, d_pat, d_off, R, k, d_stratum, d_bho, indels=indels)
        d_hits = torch.zeros(max(total, 1) * 32, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.bwt_best_search_dev(d_c, d_o, d_ro, N, sigma, d_pat, d_off, R, k, d_stratum, d_bho, d_hits, total, indels=indels)
        words = d_hits[:total * 32].view(torch.int32).reshape(-1, 8)
        q = words[:, 0].to(torch.int64)
        rows = (words[:, 2].to(torch.int64) & 0xFFFFFFFF) - (words[:, 1].to(torch.int64) & 0xFFFFFFFF)
        cum = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(rows, 0)])
        first, end = d_bho[:-1], d_bho[1:]
        n_lines = cum[end] - cum[first]  # (a read's lines)
        split = ((end > first) & (rows[first.clamp(max=max(total - 1, 0))] > 1)).to(torch.int64)
        ext = torch.cumsum(split, 0) - split
        n_all = total + int(split.sum().item())
        h = torch.arange(total, device="cuda")
        is_first = h == first[q]
        at = h + ext[q] + (~is_first).to(torch.int64) * split[q]
        d_all = torch.zeros(max(n_all, 1) * 8, dtype=torch.int32, device="cuda")
        d_all.view(-1, 8)[at] = words
        two = torch.nonzero(is_first & (split[q] == 1)).flatten()
        d_all.view(-1, 8)[at[two] + 1] = words[two]
        d_all.view(-1, 8)[at[two], 2] = words[two, 1] + 1  # (the primary: row L alone)
        d_all.view(-1, 8)[at[two] + 1, 1] = words[two, 1] + 1
        n = n_lines[q]
        cls = torch.where(n <= 1, 50, torch.where(n == 2, 3, torch.where(n <= 4, 1, 0)))
        quality = torch.zeros(max(n_all, 1), dtype=torch.int16, device="cuda")
        quality[at] = (cls | (~is_first).to(torch.int64) * 256).to(torch.int16)
        quality[at[two] + 1] = (cls[two] | 256).to(torch.int16)
        groups = torch.bincount(torch.where(n_lines == 0, 4, torch.where(n_lines == 1, 0, torch.where(n_lines == 2, 1, torch.where(n_lines <= 4, 2, 3)))),
                                minlength=5).cpu().tolist()
        del words, q, rows, cum, at, two, n, cls, h, is_first
        d_qoff = torch.zeros(n_all + 1, dtype=torch.int64, device="cuda")
        batch = ctx.sam_batch(d_all, n_all, d_sa, N, d_names, d_name_off, d_seqs, d_off, d_quals, d_off, R, d_rname, d_rname_off, 1)
        res = {"hits": int(total), "entries": int(n_all), "split": int(n_all - total), "lines": int(n_lines.sum().item()),
               "reads_by_mapq_50_3_1_0": groups[:4], "reads_without_a_line": groups[4]}
        for name, layout, emit in (("plain", lambda: ctx.sam_layout_dev(batch, d_qoff),
                                    lambda nb, lo, hi: ctx.sam_emit_dev(batch, d_qoff, nb, lo, hi, d_win)),
                                   ("mapq", lambda: ctx.sam_layout_dev_mapq(batch, quality, d_qoff),
                                    lambda nb, lo, hi: ctx.sam_emit_dev_mapq(batch, quality, d_qoff, nb, lo, hi, d_win))):
            layout()  # warm-up
            l_runs = [profiled("sam", layout) for _ in range(args.repeats)]
            nb = l_runs[0][0]

            def emit_all():
                for lo in range(0, nb, window):
                    emit(nb, lo, min(nb, lo + window))

            emit(nb, 0, min(nb, window))  # warm-up
            e_runs = [profiled("sam", emit_all) for _ in range(args.repeats)]
            res[name] = {"text_bytes": int(nb), "layout_ms": round(min(r[2] for r in l_runs), 3), "layout_ms_runs": [round(r[2], 3) for r in l_runs],
                         "emit_ms": round(min(r[2] for r in e_runs), 3), "emit_ms_runs": [round(r[2], 3) for r in e_runs]}
        res["layout_plus_emit_over_plain"] = round((res["mapq"]["layout_ms"] + res["mapq"]["emit_ms"]) /
                                                   max(res["plain"]["layout_ms"] + res["plain"]["emit_ms"], 1e-9), 3)
        del d_hits, d_all, d_qoff, quality
        torch.cuda.empty_cache()
        return res

    def unmapped_passes(total, d_hits, layout_ms, emit_ms, nbytes):
        """the same hits with a placeholder (query = the read, L = R = 0) in front of where every read without a hit would
        have its hits, as the mapper's merge places them; layout and emit of that text"""
        cnt = d_hoff[1:] - d_hoff[:-1]
        lost = (cnt == 0).to(torch.int64)
        shift = torch.cumsum(lost, 0) - lost  # (reads without a hit in front of every read)
        n_lost = int(lost.sum().item())
        d_all = torch.zeros((total + n_lost) * 8, dtype=torch.int32, device="cuda")
        if total:
            words = d_hits[:total * 32].view(torch.int32).reshape(-1, 8)
            q = words[:, 0].to(torch.int64)
            d_all.view(-1, 8)[torch.arange(total, device="cuda") + shift[q]] = words
        lost_q = torch.nonzero(lost).flatten()
        d_all.view(-1, 8)[d_hoff[:-1][lost_q] + shift[lost_q], 0] = lost_q.to(torch.int32)
        n_all = total + n_lost
        d_uoff = torch.zeros(n_all + 1, dtype=torch.int64, device="cuda")
        ub = ctx.sam_batch(d_all, n_all, d_sa, N, d_names, d_name_off, d_seqs, d_off, d_quals, d_off, R, d_rname, d_rname_off, 1)
        ctx.sam_layout_dev_unmapped(ub, d_uoff)  # warm-up
        u_layout = [profiled("sam", lambda: ctx.sam_layout_dev_unmapped(ub, d_uoff)) for _ in range(args.repeats)]
        u_bytes = u_layout[0][0]

        def emit_unmapped():
            for lo in range(0, u_bytes, window):
                ctx.sam_emit_dev_unmapped(ub, d_uoff, u_bytes, lo, min(u_bytes, lo + window), d_win)

        ctx.sam_emit_dev_unmapped(ub, d_uoff, u_bytes, 0, min(u_bytes, window), d_win)  # warm-up
        u_emit = [profiled("sam", emit_unmapped) for _ in range(args.repeats)]
        ul, ue = min(r[2] for r in u_layout), min(r[2] for r in u_emit)
        added = u_bytes - nbytes
        plain_ns_per_byte = (layout_ms + emit_ms) * 1e6 / max(nbytes, 1)
        return {"reads_without_hit": n_lost, "added_lines": n_lost, "text_bytes": int(u_bytes), "added_bytes": int(added),
                "layout_ms": round(ul, 3), "layout_ms_runs": [round(r[2], 3) for r in u_layout],
                "emit_ms": round(ue, 3), "emit_ms_runs": [round(r[2], 3) for r in u_emit],
                "plain_ns_per_text_byte": round(plain_ns_per_byte, 4),
                "added_ns_per_added_byte": None if added <= 0 else round((ul + ue - layout_ms - emit_ms) * 1e6 / added, 4)}

    for k in [int(x) for x in args.ks.split(",")]:
        out[f"k{k}"] = text_of_search(k, True)
        if args.no_indels:
            out[f"k{k}"]["no_indels"] = text_of_search(k, False)
        if args.best:
            out[f"k{k}"]["best"] = best_rounds(ctx, torch, profiled, probe, d_c, d_o, d_ro, N, sigma, d_pat, d_off, R, L, k, args.repeats)
    # ---- the streamed form: sx_map_reads_stream (host tables and FASTQ image in, SAM text out through a sink that discards)
    from stralg_amd import _lib, api
    fastq = b"".join(b"@%s\n%s\n+\n%s\n" % (names[q], row.tobytes(), b"~" * L)
                     for q, row in enumerate(np.frombuffer(b"\0ACGT", np.uint8)[reads]))
    fq = _lib.Fastq()
    img = np.frombuffer(fastq, np.uint8)
    t0 = time.perf_counter()
    assert ctx.lib.sx_fastq_index(img.ctypes.data, img.size, C.byref(fq)) == 0 and fq.count == R
    index_s = time.perf_counter() - t0
    ctx.lib.sx_fastq_free(C.byref(fq))
    out["fastq_index_host"] = {"image_bytes": len(fastq), "ms": round(index_s * 1e3, 2), "GBps": round(len(fastq) / index_s / 1e9, 2)}
    torch.cuda.synchronize()
    table = np.full(256, -1, np.int16)
    table[0] = 0
    table[np.frombuffer(b"ACGT", np.uint8)] = [1, 2, 3, 4]
    rev = np.full(128, -1, np.int16)
    string = d_text_kept[:N].cpu().numpy() if args.tags else None  # (symbols and sentinel: the index then has its string)
    del d_text_kept, d_texts
    rec = api.BwtTable(api.RemapTable(sigma, table, rev), api.SuffixArray(string, d_sa.cpu().numpy().view(np.uint32)),
                       d_c.cpu().numpy().view(np.uint32), d_o.cpu().numpy().view(np.uint32),
                       d_ro.cpu().numpy().view(np.uint32))
    del d_sa, d_o, d_ro, d_win
    torch.cuda.empty_cache()
    def streamed(k, **kw):
        """(wall seconds, the windows) of the fastest of the repeated calls, and every call's wall time in ms"""
        runs = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            seen = ctx.map_reads_stream([(b"chr1", rec)], fastq, k, None, **kw)
            runs.append((time.perf_counter() - t0, seen))
        best = min(runs, key=lambda r: r[0])
        return best[0], best[1], [round(r[0] * 1e3, 1) for r in runs]

    for k in [int(x) for x in args.ks.split(",")]:
        wall, seen, walls = streamed(k)
        nbytes = sum(b for _, b in seen)
        assert nbytes == out[f"k{k}"]["text_bytes"], (nbytes, out[f"k{k}"]["text_bytes"])
        # the windows' own rate: from the first window's arrival at the sink to the last one's (the first window's
        # emit and copy, the table upload and the search of the first batch lie in front of it)
        span = seen[-1][0] - seen[0][0]
        rate = (nbytes - seen[0][1]) / span / 1e9 if span > 0 else None
        out[f"k{k}"]["streamed"] = {"call_wall_ms": round(wall * 1e3, 1), "windows": len(seen),
                                    "first_to_last_window_ms": round(span * 1e3, 2),
                                    "windows_GBps": None if rate is None else round(rate, 2),
                                    "fraction_of_pinned_copy": None if rate is None else round(rate / max(link), 3),
                                    "call_GBps": round(nbytes / wall / 1e9, 2)}
        if args.repeats > 1:
            out[f"k{k}"]["streamed"]["call_wall_ms_runs"] = walls
        if args.no_indels:
            for key, kw in [("streamed", dict(indels=False))] + ([("streamed_best", dict(indels=False, best=True))] if args.best else []):
                f_wall, f_seen, f_walls = streamed(k, **kw)
                out[f"k{k}"]["no_indels"][key] = {"call_wall_ms": round(f_wall * 1e3, 1), "call_wall_ms_runs": f_walls,
                                                  "text_bytes": int(sum(b for _, b in f_seen)), "windows": len(f_seen),
                                                  "plain_call_wall_ms": round(wall * 1e3, 1)}
            assert out[f"k{k}"]["no_indels"]["streamed"]["text_bytes"] == out[f"k{k}"]["no_indels"]["text_bytes"]
        if args.best:
            for key, kw in [("streamed_best", dict(best=True))] + ([("streamed_best_both_strands", dict(best=True, both_strands=True))] if args.both_strands else []):
                b_wall, b_seen, b_walls = streamed(k, **kw)
                out[f"k{k}"][key] = {"call_wall_ms": round(b_wall * 1e3, 1), "call_wall_ms_runs": b_walls,
                                     "text_bytes": int(sum(b for _, b in b_seen)), "windows": len(b_seen),
                                     "plain_call_wall_ms": round(wall * 1e3, 1)}
        if args.unmapped:  # the call with and without the bit: wall, bytes, and its search and sam kernel ms in runs of their own
            res = {}
            for name, kw in (("plain", {}), ("unmapped", dict(unmapped=True))):
                call = lambda: ctx.map_reads_stream([(b"chr1", rec)], fastq, k, None, **kw)  # noqa: E731
                u_wall, u_seen, u_walls = (wall, seen, walls) if not kw else streamed(k, **kw)  # (the plain runs: those above)
                search = [profiled("search", call)[2] for _ in range(args.repeats)]
                sam = [profiled("sam", call)[2] for _ in range(args.repeats)]
                res[name] = {"call_wall_ms": round(u_wall * 1e3, 1), "call_wall_ms_runs": u_walls, "text_bytes": int(sum(b for _, b in u_seen)),
                             "search_ms": round(min(search), 3), "search_ms_runs": [round(x, 3) for x in search],
                             "sam_class_ms": round(min(sam), 3), "sam_class_ms_runs": [round(x, 3) for x in sam]}
            assert res["unmapped"]["text_bytes"] == out[f"k{k}"]["unmapped"]["text_bytes"]
            out[f"k{k}"]["unmapped"]["streamed"] = res
        if args.mapq:  # the best call with and without the bit: wall, bytes, the kernel ms of the quality pass and of the sam class
            for where, more in [(out[f"k{k}"]["mapq"], {})] + ([(out[f"k{k}"]["no_indels"]["mapq"], dict(indels=False))] if args.no_indels else []):
                res = {}
                for name, kw in (("best", dict(best=True, **more)), ("best_mapq", dict(best=True, mapq=True, **more))):
                    call = lambda: ctx.map_reads_stream([(b"chr1", rec)], fastq, k, None, **kw)  # noqa: E731
                    q_wall, q_seen, q_walls = streamed(k, **kw)
                    sam = [profiled("sam", call)[2] for _ in range(args.repeats)]
                    res[name] = {"call_wall_ms": round(q_wall * 1e3, 1), "call_wall_ms_runs": q_walls, "text_bytes": int(sum(b for _, b in q_seen)),
                                 "sam_class_ms": round(min(sam), 3), "sam_class_ms_runs": [round(x, 3) for x in sam]}
                    if "mapq" in kw:
                        qp = [profiled("mapq", call)[2] for _ in range(args.repeats)]
                        res[name]["quality_pass_ms"] = round(min(qp), 3)
                        res[name]["quality_pass_ms_runs"] = [round(x, 3) for x in qp]
                assert res["best_mapq"]["text_bytes"] == where["mapq"]["text_bytes"] and res["best"]["text_bytes"] == where["plain"]["text_bytes"]
                where["streamed"] = res
        if args.both_strands:
            both_wall, both_seen, both_walls = streamed(k, both_strands=True)
            out[f"k{k}"]["streamed_both_strands"] = {"call_wall_ms": round(both_wall * 1e3, 1), "call_wall_ms_runs": both_walls,
                                                    "text_bytes": int(sum(b for _, b in both_seen)), "windows": len(both_seen),
                                                    "over_one_strand_call": round(both_wall / wall, 3)}
    if args.tags:
        # the call through a resident index that has its string (the tables go up once), with and without the fields
        with api.Index.from_tables([(b"chr1", rec)], ctx=ctx) as idx:
            for k in [int(x) for x in args.ks.split(",")]:
                variants = [("", {})] + ([("no_indels", dict(indels=False))] if args.no_indels else []) + \
                           ([("best", dict(best=True))] if args.best else [])
                for key, kw in variants:
                    res = {}
                    for name, tags in (("plain", False), ("tags", True)):
                        runs = []
                        for _ in range(args.repeats):
                            t0 = time.perf_counter()
                            seen = idx.map_reads_discard(fastq, k, tags=tags, **kw)
                            runs.append((time.perf_counter() - t0, sum(b for _, b in seen)))
                        res[name] = {"call_wall_ms": round(min(r[0] for r in runs) * 1e3, 1), "call_wall_ms_runs": [round(r[0] * 1e3, 1) for r in runs],
                                     "text_bytes": int(runs[0][1])}
                    where = out[f"k{k}"] if not key else out[f"k{k}"].setdefault(key, {})
                    where["index_call"] = res
    if args.pairs:
        # the mates: 200 - 499 symbols downstream of their reads, on the other strand, substitutions drawn like the reads'
        prng = np.random.default_rng(101)
        gap = prng.integers(200, 500, R)
        m_starts = np.minimum(starts + gap, n - L)
        mates = text[m_starts[:, None] + np.arange(L)[None, :]]
        for e in range(2):
            hit = prng.random(R) < (0.5 if e == 0 else 0.25)
            at = prng.integers(0, L, R)
            rows = np.flatnonzero(hit)
            mates[rows, at[rows]] = 1 + (mates[rows, at[rows]] % 4)
        rc_letters = np.frombuffer(b"\0TGCA", np.uint8)  # (the complement of the letter behind every code)
        fastq2 = b"".join(b"@%s\n%s\n+\n%s\n" % (names[q], row.tobytes(), b"~" * L) for q, row in enumerate(rc_letters[mates[:, ::-1]]))
        pair_classes = ["pair_count", "pair_scan", "pair_fill", "pair_layout", "pair_emit"]
        with api.Index.from_tables([(b"chr1", rec)], ctx=ctx) as idx:
            for k in [int(x) for x in args.ks.split(",")]:
                res = {}
                for key, kw in [("no_indels", dict(indels=False)), ("no_indels_best", dict(indels=False, best=True))]:
                    runs = []
                    for _ in range(args.repeats):
                        t0 = time.perf_counter()
                        seen = idx.map_pairs_discard(fastq, fastq2, k, 0, 1000, **kw)
                        runs.append((time.perf_counter() - t0, sum(b for _, b in seen)))
                    singles = []
                    for _ in range(args.repeats):
                        t0 = time.perf_counter()
                        b1 = sum(b for _, b in idx.map_reads_discard(fastq, k, both_strands=True, **kw))
                        b2 = sum(b for _, b in idx.map_reads_discard(fastq2, k, both_strands=True, **kw))
                        singles.append((time.perf_counter() - t0, b1 + b2))
                    # the five classes' kernel time: one more call with every launch between events
                    ctx.profile_only(None)
                    ctx.profile_enable(True)
                    ctx.profile_reset()
                    idx.map_pairs_discard(fastq, fastq2, k, 0, 1000, **kw)
                    prof = ctx.profile_read()
                    ctx.profile_enable(False)
                    text_bytes, wall = int(runs[0][1]), min(r[0] for r in runs)
                    emit_ms = prof["pair_emit"]["ms"]
                    res[key] = {"text_bytes": text_bytes, "call_wall_ms": round(wall * 1e3, 1), "call_wall_ms_runs": [round(r[0] * 1e3, 1) for r in runs],
                                "two_both_strands_calls_wall_ms": round(min(r[0] for r in singles) * 1e3, 1),
                                "two_both_strands_calls_wall_ms_runs": [round(r[0] * 1e3, 1) for r in singles],
                                "two_both_strands_calls_text_bytes": int(singles[0][1]),
                                "over_two_both_strands_calls": round(wall / min(r[0] for r in singles), 3),
                                "kernel_ms": {c: round(prof[c]["ms"], 3) for c in pair_classes + ["search", "sam", "remap"]},
                                "launches": {c: int(prof[c]["launches"]) for c in pair_classes},
                                "emit_GBps_of_text": round(text_bytes / (emit_ms * 1e-3) / 1e9, 1) if emit_ms > 0 else None}
                out[f"k{k}"]["pairs"] = res
    if args.both_strands:
        # the strand kernel alone: the image indexed on the device, then sx_fastq_strands_dev (launches of the remap class)
        d_img = torch.from_numpy(np.concatenate([img, pad])).cuda()
        d_flags = torch.zeros(2 * R, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        one, both = _lib.FastqDev(), _lib.FastqDev()
        assert ctx.lib.sx_fastq_index_dev(ctx.h, d_img.data_ptr(), img.size, C.byref(one)) == 0 and one.count == R

        def strands():
            assert ctx.lib.sx_fastq_strands_dev(ctx.h, C.byref(one), C.byref(both), d_flags.data_ptr()) == 0
            ctx.lib.sx_fastq_dev_free(C.byref(both))

        strands()  # warm-up
        runs = [profiled("remap", strands) for _ in range(max(3, args.repeats))]
        ms = min(r[2] for r in runs)
        moved = 4 * (int(one.name_bytes) + int(one.seq_bytes) + int(one.qual_bytes)) + 3 * 12 * R + 4 * R
        ctx.lib.sx_fastq_dev_free(C.byref(one))
        out["strand_kernel"] = {"ms": round(ms, 3), "ms_runs": [round(r[2], 3) for r in runs], "call_wall_ms": round(min(r[1] for r in runs) * 1e3, 3),
                                "bytes_moved": moved, "GBps": round(moved / (ms * 1e-3) / 1e9, 1),
                                "fraction_of_copy": round(moved / (ms * 1e-3) / 1e9 / probe["copy"], 3)}
    if args.reference_lines_per_s:
        out["reference_mapper_one_core"] = {"lines_per_s": args.reference_lines_per_s,
                                            "what": "unmodified bwt_readmapper -d 2, hg38-10000.fa, reads-100-10-0.fq (408 980 lines, "
                                                    "24.1 MB), whole program, page cache warm",
                                            "host": "the CPU-only build machine, not the GPU box"}
    print(json.dumps(out))


def best_rounds(ctx, torch, profiled, probe, d_c, d_o, d_ro, N, sigma, d_pat, d_off, R, L, k, repeats):
    """sx_bwt_best_search_dev on the batch, and its rounds replayed through the public calls"""
    d_hoff = torch.zeros(R + 1, dtype=torch.int64, device="cuda")
    d_stratum = torch.zeros(R, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    total = ctx.bwt_best_search_dev(d_c, d_o, d_ro, N, sigma, d_pat, d_off, R, k, d_stratum, d_hoff)
    d_hits = torch.zeros(max(total, 1) * 32, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    call = lambda: ctx.bwt_best_search_dev(d_c, d_o, d_ro, N, sigma, d_pat, d_off, R, k, d_stratum, d_hoff, d_hits, total)
    runs = [profiled("search", call) for _ in range(repeats)]
    sel_runs = [profiled("remap", call) for _ in range(repeats)]
    words = d_hits[:total * 32].view(torch.int32).reshape(-1, 8)
    lines = int(((words[:, 2].to(torch.int64) & 0xFFFFFFFF) - (words[:, 1].to(torch.int64) & 0xFFFFFFFF)).sum().item())
    strata = torch.bincount(d_stratum.to(torch.int64), minlength=256).cpu().tolist()
    res = {"hits": int(total), "lines": lines, "call_wall_ms": round(min(r[1] for r in runs) * 1e3, 2),
           "call_wall_ms_runs": [round(r[1] * 1e3, 2) for r in runs], "search_kernel_ms": round(min(r[2] for r in runs), 3),
           "select_kernel_ms": round(min(r[2] for r in sel_runs), 3), "without_a_hit": strata[255], "rounds": []}
    del words, d_hits
    # the rounds again, one public call a step
    cur_pat, cur_off, cur_n = d_pat, d_off, R
    for d in range(k + 1):
        if cur_n == 0:
            break
        d_ho = torch.zeros(cur_n + 1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        tot, count_wall, count_ms = profiled("search", lambda: ctx.bwt_approx_search_dev(d_c, d_o, d_ro, N, sigma, cur_pat, cur_off, cur_n, d, d_ho))
        found = (d_ho[1:] > d_ho[:-1])
        sets, sel = [], []
        for keep in (found, ~found):
            d_keep = keep.to(torch.uint8).contiguous()
            d_out = torch.zeros(cur_n * L + 32, dtype=torch.uint8, device="cuda")
            d_oo = torch.zeros(cur_n + 1, dtype=torch.int32, device="cuda")
            d_ids = torch.zeros(max(cur_n, 1), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            (kept, nbytes), wall, ms = profiled("remap", lambda: ctx.patterns_select_dev(cur_pat, cur_off, cur_n, d_keep, d_out, d_oo, d_ids))
            moved = 2 * nbytes + cur_n * 9 + kept * 16
            sel.append({"kept": kept, "bytes": nbytes, "kernel_ms": round(ms, 3), "wall_ms": round(wall * 1e3, 3), "bytes_moved": moved,
                        "fraction_of_copy": round(moved / (ms * 1e-3) / 1e9 / probe["copy"], 3) if ms > 0 else None})
            sets.append((d_out, d_oo, kept))
        emit_ms = None
        f_pat, f_off, f_n = sets[0]
        if f_n:
            d_fho = torch.zeros(f_n + 1, dtype=torch.int64, device="cuda")
            d_fh = torch.zeros(max(tot, 1) * 32, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            _, _, both_ms = profiled("search", lambda: ctx.bwt_approx_search_dev(d_c, d_o, d_ro, N, sigma, f_pat, f_off, f_n, d, d_fho, d_fh, tot))
            _, _, only_ms = profiled("search", lambda: ctx.bwt_approx_search_dev(d_c, d_o, d_ro, N, sigma, f_pat, f_off, f_n, d, d_fho))
            emit_ms = round(both_ms - only_ms, 3)
            del d_fho, d_fh
        res["rounds"].append({"d": d, "groups_in": cur_n, "found": int(f_n), "hits": int(tot), "count_kernel_ms": round(count_ms, 3),
                              "count_wall_ms": round(count_wall * 1e3, 2), "select_found": sel[0], "select_open": sel[1],
                              "emit_kernel_ms_by_difference": emit_ms})
        cur_pat, cur_off, cur_n = sets[1]
        torch.cuda.empty_cache()
    return res


if __name__ == "__main__":
    main()
