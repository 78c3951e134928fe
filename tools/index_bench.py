"""The device-resident index (stralg_amd.Index) against the route it replaces, on the inputs of tools/sam_bench.py: a
2^28-symbol DNA record, 10^6 reads of 100 symbols, k = 1 and 2.  Prints one JSON line (kept in
profiles/index_bench_2p28.json), everything measured in this one run:

  build      Index.from_fasta (FASTA image in, tables stay on the device) against the parent route's table production in
             stralg_amd.map_reads: fasta_records + build_complete_table per record (tables come back to the host)
  map        a repeated Index.map_reads on the resident index with a sink that discards, against sx_map_reads_stream's
             whole call on the same inputs (host tables uploaded in every call), per k; the difference next to the table
             upload measured alone (Index.from_tables of the same host tables)
  fastq      sx_fastq_index_dev, kernels only (HIP events of the class) and upload + kernels (wall), against the host's
             sx_fastq_index on the same image; the device pass as a fraction of sx_membw_probe's read rate

  --compact --sa-sample 8,32,128  the compact index against the same with a sampled suffix array
  --compact  the full index against the compact one (BWT blocks with sampled counts in place of O / RO, DESIGN.md section
             13) of the same record and reads, in one run: resident bytes, build time, a mapping call per k, the search
             kernels' share of it (HIP events of the class), and the ratio of the two forms' search times; nothing else
             is measured then (kept in profiles/compact_index_2p28.json)

  --compact --packed [--sa-sample 32]  the compact index against its packed form (a nibble a row in the blocks, DESIGN.md
             section 15) of the same record and reads, in one run; with --sa-sample both forms keep a suffix array sampled at
             these distances (kept in profiles/packed_index_2p28.json)

    python tools/index_bench.py [--log2n 28] [--reads 1000000] [--reps 3]
    python tools/index_bench.py --compact [--form compact --trace-only]
    rocprofv3 --kernel-trace --stats -d out -- python tools/index_bench.py --trace-only     (profiles/index_rocprofv3_summary.txt)
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


def best(fn, reps):
    times = []
    res = None
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fn()
        times.append(time.perf_counter() - t0)
    return res, min(times), times


def compact_leg(args, ctx, Index, fasta, fastq, out):
    """both forms of the index of the same record, one after the other in this process: what each keeps resident, what its
    build takes, a mapping call per k and the search kernels' part of one such call"""
    out["bench"] = "compact_index"
    ks = [int(x) for x in args.ks.split(",")]
    forms = ("full", "compact") if args.form == "both" else (args.form,)
    samplings = [int(x) for x in args.sa_sample.split(",")] if args.sa_sample else []
    if args.packed:  # every byte-block form beside its packed form: the same searches and walks over the other blocks
        out["bench"] = "packed_index"
        pairs = [f"sampled{s}" for s in samplings] if samplings else ["compact"]
        if args.form == "packed":
            forms = tuple("packed_" + f if f != "compact" else "packed" for f in pairs)
        else:
            forms = tuple(f for pair in pairs for f in (pair, "packed_" + pair if pair != "compact" else "packed"))
    elif samplings:  # the compact index beside the sampled ones: the searches are the same, the locate pass is what differs
        out["bench"] = "sampled_sa"
        forms = (() if args.form == "sampled" else ("compact",)) + tuple(f"sampled{s}" for s in samplings)
    for form in forms:
        compact = form != "full"
        packed = form.startswith("packed")
        sa_sample = int(form.split("sampled")[1]) if "sampled" in form else 0
        if args.trace_only:
            with Index.from_fasta(fasta, ctx=ctx, compact=compact, sa_sample=sa_sample, packed=packed) as idx:
                for _ in range(2):
                    idx.map_reads_discard(fastq, ks[0])
            continue

        def build():
            Index.from_fasta(fasta, ctx=ctx, compact=compact, sa_sample=sa_sample, packed=packed).close()

        build()  # warm-up (workspace)
        _, build_s, build_all = best(build, args.reps)
        res = {"build_ms": round(build_s * 1e3, 1), "build_all_ms": [round(t * 1e3, 1) for t in build_all]}
        with Index.from_fasta(fasta, ctx=ctx, compact=compact, sa_sample=sa_sample, packed=packed) as idx:
            res["device_bytes"] = idx.device_bytes
            res["device_bytes_a_symbol"] = round(idx.device_bytes / sum(N for _, N, _, _ in idx.records), 4)
            for k in ks:
                seen = idx.map_reads_discard(fastq, k)  # warm-up
                _, call_s, call_all = best(lambda: idx.map_reads_discard(fastq, k), args.reps if k < 2 else max(1, args.reps - 1))
                ctx.profile_only("search")
                ctx.profile_enable(True)
                ctx.profile_reset()
                t0 = time.perf_counter()
                idx.map_reads_discard(fastq, k)
                timed_s = time.perf_counter() - t0
                stat = ctx.profile_read()["search"]
                ctx.profile_enable(False)
                ctx.profile_only(None)
                res[f"k{k}"] = {"text_bytes": sum(b for _, b in seen), "call_ms": round(call_s * 1e3, 1),
                                "call_all_ms": [round(t * 1e3, 1) for t in call_all], "search_kernels_ms": round(stat["ms"], 2),
                                "search_launches": stat["launches"], "profiled_call_ms": round(timed_s * 1e3, 1),
                                "search_share_of_call": round(stat["ms"] * 1e-3 / timed_s, 4)}
                if sa_sample and not args.packed and "compact" in out:
                    # the locate kernel is timed in the searches' class: what that class takes beyond the compact index's same
                    # searches is the locate pass (a launch a run beside the count, the scan and the run kernels)
                    locate_ms = stat["ms"] - out["compact"][f"k{k}"]["search_kernels_ms"]
                    res[f"k{k}"].update(locate_ms=round(locate_ms, 2), locate_share_of_call=round(locate_ms * 1e-3 / timed_s, 4),
                                        locate_launches=stat["launches"] - out["compact"][f"k{k}"]["search_launches"])
        out[form] = res
        ctx.trim()
    if not args.trace_only:
        if args.packed and args.form != "packed":
            out["packed_over_bytes"] = {}
            for base in forms[0::2]:
                pk = "packed" if base == "compact" else "packed_" + base
                out["packed_over_bytes"][pk] = {
                    "device_bytes": round(out[pk]["device_bytes"] / out[base]["device_bytes"], 4),
                    "build": round(out[pk]["build_ms"] / out[base]["build_ms"], 3),
                    **{f"k{k}_search_kernels": round(out[pk][f"k{k}"]["search_kernels_ms"] / out[base][f"k{k}"]["search_kernels_ms"], 3) for k in ks},
                    **{f"k{k}_call": round(out[pk][f"k{k}"]["call_ms"] / out[base][f"k{k}"]["call_ms"], 3) for k in ks}}
                assert all(out[pk][f"k{k}"]["text_bytes"] == out[base][f"k{k}"]["text_bytes"] for k in ks)
        elif samplings and "compact" in out:
            out["sampled_over_compact"] = {
                f"sampled{s}": {"device_bytes": round(out[f"sampled{s}"]["device_bytes"] / out["compact"]["device_bytes"], 4),
                                "build": round(out[f"sampled{s}"]["build_ms"] / out["compact"]["build_ms"], 3),
                                **{f"k{k}_call": round(out[f"sampled{s}"][f"k{k}"]["call_ms"] / out["compact"][f"k{k}"]["call_ms"], 3) for k in ks}}
                for s in samplings}
            assert all(out[f"sampled{s}"][f"k{k}"]["text_bytes"] == out["compact"][f"k{k}"]["text_bytes"] for k in ks for s in samplings)
        elif len(forms) == 2:
            out["compact_over_full"] = {
                "device_bytes": round(out["compact"]["device_bytes"] / out["full"]["device_bytes"], 4),
                "build": round(out["compact"]["build_ms"] / out["full"]["build_ms"], 3),
                **{f"k{k}_search_kernels": round(out["compact"][f"k{k}"]["search_kernels_ms"] / out["full"][f"k{k}"]["search_kernels_ms"], 3)
                   for k in ks},
                **{f"k{k}_call": round(out["compact"][f"k{k}"]["call_ms"] / out["full"][f"k{k}"]["call_ms"], 3) for k in ks}}
            assert all(out["compact"][f"k{k}"]["text_bytes"] == out["full"][f"k{k}"]["text_bytes"] for k in ks)
        print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--length", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ks", default="1,2")
    ap.add_argument("--skip-parent", action="store_true", help="no host tables: only the index's own figures")
    ap.add_argument("--trace-only", action="store_true",
                    help="build the index, map the reads twice at the first k and stop (for a rocprofv3 --kernel-trace --stats run)")
    ap.add_argument("--compact", action="store_true", help="the full and the compact index side by side, nothing else")
    ap.add_argument("--form", default="both", choices=["both", "full", "compact", "sampled", "packed"],
                    help="with --compact: only this form (sampled: with --sa-sample, without the compact index beside it; packed: with "
                    "--packed, without the byte blocks beside it)")
    ap.add_argument("--packed", action="store_true", help="with --compact: the compact index beside its packed form (DESIGN.md section 15), "
                    "both with a sampled suffix array where --sa-sample is given; kept in profiles/packed_index_2p28.json")
    ap.add_argument("--sa-sample", default="", help="with --compact: the compact index beside indexes with a suffix array sampled at "
                    "these distances (8,32,128): DESIGN.md section 14, kept in profiles/sampled_sa_2p28.json")
    args = ap.parse_args()
    if args.packed and not args.compact:
        ap.error("--packed needs --compact")
    import torch

    import stralg_amd
    from stralg_amd import Context, Index, _lib, synth

    ctx = Context(0)
    n, L, R = 1 << args.log2n, args.length, args.reads
    letters = np.frombuffer(b"\0ACGT", np.uint8)
    text = synth(n, 5, 28)
    seq = letters[text]
    full = n - n % 60
    rows = np.empty((full // 60, 61), np.uint8)
    rows[:, :60] = seq[:full].reshape(-1, 60)
    rows[:, 60] = 10
    fasta = b">chr1\n" + rows.tobytes() + (seq[full:].tobytes() + b"\n" if full < n else b"")
    del rows
    # the reads of tools/sam_bench.py
    rng = np.random.default_rng(100)
    starts = rng.integers(0, n - L, R)
    reads = text[starts[:, None] + np.arange(L)[None, :]]
    for e in range(2):
        hit = rng.random(R) < (0.5 if e == 0 else 0.25)
        at = rng.integers(0, L, R)
        rws = np.flatnonzero(hit)
        reads[rws, at[rws]] = 1 + (reads[rws, at[rws]] % 4)
    fastq = b"".join(b"@read%d\n%s\n+\n%s\n" % (q, row.tobytes(), b"~" * L) for q, row in enumerate(letters[reads]))
    out = {"bench": "index", "n": n, "reads": R, "read_length": L, "fasta_bytes": len(fasta), "fastq_bytes": len(fastq),
           "reps": args.reps}

    if args.compact:
        return compact_leg(args, ctx, Index, fasta, fastq, out)

    if args.trace_only:
        with Index.from_fasta(fasta, ctx=ctx) as idx:
            k = int(args.ks.split(",")[0])
            for _ in range(2):
                idx.map_reads_discard(fastq, k)
        return

    # ---- the box: read rate of device memory, rate of a pinned upload
    nb = 1 << 30
    d_a = torch.zeros(nb + 16, dtype=torch.uint8, device="cuda")
    d_b = torch.zeros(nb + 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    probe = ctx.membw_probe(d_a, d_b, nb, 5)
    del d_a, d_b
    torch.cuda.empty_cache()
    out["membw_probe_GBps"] = {k: round(v, 1) for k, v in probe.items()}

    # ---- 3. FASTQ ingest
    img = np.frombuffer(fastq, np.uint8)
    fq = _lib.Fastq()

    def host_index():
        assert ctx.lib.sx_fastq_index(img.ctypes.data, img.size, C.byref(fq)) == 0 and fq.count == R
        ctx.lib.sx_fastq_free(C.byref(fq))

    _, host_s, _ = best(host_index, args.reps)
    h_pin = torch.from_numpy(img.copy()).pin_memory()
    d_img = torch.zeros(img.size + 16, dtype=torch.uint8, device="cuda")
    fqd = _lib.FastqDev()

    def dev_index():
        rc = ctx.lib.sx_fastq_index_dev(ctx.h, d_img.data_ptr(), img.size, C.byref(fqd))
        assert rc == 0 and fqd.count == R, rc
        ctx.lib.sx_fastq_dev_free(C.byref(fqd))

    def upload_and_index():
        d_img[:img.size].copy_(h_pin, non_blocking=True)
        torch.cuda.synchronize()
        dev_index()

    upload_and_index()  # warm-up (the context's scratch grows once)
    _, dev_wall_s, _ = best(dev_index, args.reps)
    _, both_s, _ = best(upload_and_index, args.reps)
    ctx.profile_only("fasta")
    ctx.profile_enable(True)
    ctx.profile_reset()
    dev_index()
    stat = ctx.profile_read()["fasta"]
    ctx.profile_enable(False)
    ctx.profile_only(None)
    kernel_s = stat["ms"] * 1e-3
    out["fastq_index"] = {"image_bytes": img.size, "host_ms": round(host_s * 1e3, 2),
                          "device_kernels_ms": round(kernel_s * 1e3, 3), "device_kernel_launches": stat["launches"],
                          "device_call_wall_ms": round(dev_wall_s * 1e3, 3),
                          "pinned_upload_plus_call_ms": round(both_s * 1e3, 2),
                          "device_kernels_GBps": round(img.size / kernel_s / 1e9, 1),
                          "fraction_of_probe_read": round(img.size / kernel_s / 1e9 / probe["read"], 4)}
    del d_img, h_pin
    torch.cuda.empty_cache()

    # ---- 1. build
    def build_index():
        idx = Index.from_fasta(fasta, ctx=ctx)
        idx.close()

    build_index()  # warm-up (workspace)
    _, build_s, build_all = best(build_index, args.reps)
    out["build"] = {"index_from_fasta_ms": round(build_s * 1e3, 1), "index_from_fasta_all_ms": [round(t * 1e3, 1) for t in build_all]}
    records = None
    if not args.skip_parent:
        def parent_tables():
            return [(name, stralg_amd.build_complete_table(s, True, ctx)) for name, s in ctx.fasta_records(fasta)]

        records, parent_s, parent_all = best(parent_tables, max(1, args.reps - 1))
        out["build"].update(parent_tables_ms=round(parent_s * 1e3, 1), parent_tables_all_ms=[round(t * 1e3, 1) for t in parent_all])
        ctx.trim()

    # ---- 2. repeated mapping
    idx = Index.from_fasta(fasta, ctx=ctx)
    out["device_bytes"] = idx.device_bytes
    for k in [int(x) for x in args.ks.split(",")]:
        seen = idx.map_reads_discard(fastq, k)  # warm-up
        nbytes = sum(b for _, b in seen)
        _, res_s, res_all = best(lambda: idx.map_reads_discard(fastq, k), args.reps)
        out[f"k{k}"] = {"text_bytes": nbytes, "resident_call_ms": round(res_s * 1e3, 1),
                        "resident_call_all_ms": [round(t * 1e3, 1) for t in res_all]}
    idx.close()
    if records is not None:
        def upload_only():
            Index.from_tables(records, ctx=ctx).close()

        upload_only()
        _, up_s, _ = best(upload_only, args.reps)
        out["table_upload_alone_ms"] = round(up_s * 1e3, 1)
        for k in [int(x) for x in args.ks.split(",")]:
            ctx.map_reads_stream(records, fastq, k, None) if k == 1 else None  # warm-up once
            seen, par_s, par_all = best(lambda: ctx.map_reads_stream(records, fastq, k, None), args.reps if k < 2 else 1)
            assert sum(b for _, b in seen) == out[f"k{k}"]["text_bytes"]
            out[f"k{k}"].update(stream_call_ms=round(par_s * 1e3, 1), stream_call_all_ms=[round(t * 1e3, 1) for t in par_all],
                                difference_ms=round((par_s - out[f"k{k}"]["resident_call_ms"] * 1e-3) * 1e3, 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
