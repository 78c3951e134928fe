"""A/B of SX_FLAG_INDUCE_EARLY_S_OFF in one process, on the same buffers (bench.py's step: suffix array + BWT + C/O tables
of one DNA record): the switch alternates off / on for `--pairs` pairs of steps after warm-up, every step timed on its
own between synchronisations; then one profiled step of each setting (HIP events around every launch) for the per-class
table.  Buffer placement moves a step by up to 1 ms from one process to the next, which is why
the two settings are compared here and not across processes.

    python tools/early_s_ab.py [--log2n 30] [--pairs 12] [--warmup 4] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=30)
    ap.add_argument("--pairs", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import torch
    import stralg_amd
    from stralg_amd import workloads

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    ctx = stralg_amd.Context(0)
    ctx.bind_to_numa_node()
    n = 1 << args.log2n
    N = n + 1
    text, sigma = workloads.make_text(ctx, "dna", n, 0, 42, dev)
    torch.cuda.synchronize()
    sa = torch.empty(N, dtype=torch.int32, device=dev)
    bwt = torch.empty(N, dtype=torch.uint8, device=dev)
    c_tab = torch.zeros(sigma, dtype=torch.int32, device=dev)
    o_tab = torch.empty((N + 1) * sigma, dtype=torch.int32, device=dev)

    def step():
        ctx.sa_bwt_build_dev(text, n, sigma, sa, bwt)
        ctx.bwt_tables_from_bwt_dev(bwt, N, sigma, c_tab, o_tab)

    def timed(on):
        ctx.set_induce_early_s(on)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for i in range(args.warmup):
        timed(bool(i & 1))
    off, on = [], []
    for _ in range(args.pairs):
        off.append(timed(False))
        on.append(timed(True))
    placed = ctx.last_stats()["induce_early_s"]
    for i, (a, b) in enumerate(zip(off, on)):
        print(f"pair {i:2d}: off {a:8.3f} ms   on {b:8.3f} ms")
    m_off, m_on, sd_off = statistics.mean(off), statistics.mean(on), statistics.stdev(off)
    print(f"mean off {m_off:.3f} ms (sd {sd_off:.3f}), mean on {m_on:.3f} ms (sd {statistics.stdev(on):.3f}): "
          f"on is {m_off - m_on:+.3f} ms below off = {(m_off - m_on) / sd_off:.1f} sd of the off-steps; induce_early_s {placed}")

    tables = {}
    for label, flag in (("off", False), ("on", True)):
        ctx.set_induce_early_s(flag)
        ctx.profile_reset()
        ctx.profile_only(None)
        ctx.profile_enable(True)
        step()
        torch.cuda.synchronize()
        ctx.profile_enable(False)
        tables[label] = ctx.profile_read()
    print(f"{'class':<18}{'off: n':>8}{'ms':>9}{'GB/s':>8}{'on: n':>9}{'ms':>9}{'GB/s':>8}")
    for k in sorted(tables["off"], key=lambda k: -tables["off"][k]["ms"]):
        a, b = tables["off"][k], tables["on"].get(k, {"launches": 0, "ms": 0.0, "alg_bytes": 0})
        if a["launches"] == 0 and b["launches"] == 0:
            continue
        gb = lambda r: r["alg_bytes"] / r["ms"] / 1e6 if r["ms"] > 0 else 0.0
        print(f"{k:<18}{a['launches']:>8}{a['ms']:>9.3f}{gb(a):>8.0f}{b['launches']:>9}{b['ms']:>9.3f}{gb(b):>8.0f}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"n": n, "pairs": args.pairs, "off_ms": off, "on_ms": on, "mean_off_ms": m_off, "mean_on_ms": m_on,
                       "sd_off_ms": sd_off, "induce_early_s": placed, "per_class": tables}, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
