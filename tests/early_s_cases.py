"""Cases for the S-type predecessors that the L pass of the induced sort places itself (sx_induce_small.hpp, early_s;
SX_FLAG_INDUCE_EARLY_S_OFF): texts of at most 8 symbols with the settings that make every large round place, a prefix of
the rounds, or none.  Shared by the CPU-harness run (tests/test_early_s_cpu.py) and the GPU run (tests/test_gpu_early_s.py):
every case is built with the switch on and off, through one of the two device entry points, and both results must be the
oracle's suffix array and BWT."""
import numpy as np

import oracle


def ascents_into_l(x):
    """positions q with x[q] < x[q + 1] whose right neighbour q + 1 is L-type: what the L pass can place at the most"""
    x = np.asarray(x, dtype=np.int64)
    n = x.size
    t = np.concatenate([x, [0]])
    is_s = np.zeros(n + 1, dtype=bool)
    is_s[n] = True
    for i in range(n - 1, -1, -1):
        is_s[i] = t[i] < t[i + 1] or (t[i] == t[i + 1] and is_s[i + 1])
    q = np.nonzero(x[:-1] < x[1:])[0]
    return int((~is_s[q + 1]).sum())


def uniform(n, sigma, seed):
    return np.random.default_rng(seed).integers(1, sigma, size=n, dtype=np.uint8)


def skewed(n, sigma, heavy, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(1, sigma, size=n, dtype=np.uint8)
    x[rng.random(n) < 0.9] = heavy
    return x


def poly_a(n, seed):
    """random DNA with poly-A runs of differing lengths, 200 to 5000"""
    rng = np.random.default_rng(seed)
    x = rng.integers(1, 5, size=n, dtype=np.uint8)
    at = 1000
    for length in (200, 317, 1000, 2500, 5000, 4099, 640):
        if at + length + 500 > n:
            break
        x[at:at + length] = 1
        at += length + int(rng.integers(300, 3000))
    return x


class Setting:
    """chain_max (None: default), the eight-rounds form on / off, attended passes, expectation on induce_early_s,
    the eight-rounds form's lower bound (None: default)"""

    def __init__(self, chain_max=None, batch=True, attended=0, expect=None, batch_min=None):
        self.chain_max, self.batch, self.attended, self.expect, self.batch_min = chain_max, batch, attended, expect, batch_min


def cases(full_size=True):
    """name -> (text, sigma, Setting, entry point: 'sa' (the BWT bytes live in the arena) or 'sa_bwt').
    full_size: the default-settings text has 2^20 symbols (the GPU run) and not 2^17 (the CPU harness, for its time)"""
    out = {}
    # every round places: one tile, a tile boundary, a ragged last tile, several tiles
    for k, n in enumerate((2047, 2048, 2049, 6143, 65537)):
        out[f"all_rounds_n{n}"] = (uniform(n, 5, 100 + k), 5, Setting(0, False, expect="all"), "sa_bwt" if k % 2 else "sa")
    # a prefix of the rounds places, the S pass scans the rest
    for n in (1 << 16, 1 << 18):
        for cm in (4096, 16384):
            for batch in (True, False):
                out[f"prefix_n{n}_cm{cm}_{'batch' if batch else 'rounds'}"] = (
                    uniform(n, 5, n + cm), 5, Setting(cm, batch, expect="some" if not batch and n // 8 > 2 * cm else None), "sa_bwt" if batch else "sa")
    # (the eight-rounds form on, as by default, takes every round of a region this short; with its lower bound set the
    #  rounds expected beyond the bound are launches of their own in front of it, as the large rounds of a long text are)
    for n, cm, bmin in ((1 << 16, 0, 3000), (1 << 18, 4096, 5000)):
        out[f"prefix_n{n}_cm{cm}_batchmin{bmin}"] = (uniform(n, 5, n + bmin), 5, Setting(cm, True, expect="some", batch_min=bmin), "sa_bwt")
    # nothing places: every region is below the default threshold
    out["default_settings"] = (uniform(1 << 20 if full_size else 1 << 17, 5, 7), 5, Setting(expect="none"), "sa_bwt")
    # alphabets and shapes
    n = 30011
    for sigma in (2, 3, 4, 8):
        out[f"sigma{sigma}"] = (uniform(n, sigma, 40 + sigma), sigma, Setting(0, False, expect="all" if sigma > 2 else "none"), "sa_bwt")
        out[f"sigma{sigma}_cm4096"] = (uniform(n, sigma, 50 + sigma), sigma, Setting(4096, False), "sa")
    out["largest_at_90"] = (skewed(n, 5, 4, 61), 5, Setting(0, False), "sa_bwt")
    out["smallest_at_90"] = (skewed(n, 5, 1, 62), 5, Setting(0, False), "sa_bwt")
    out["largest_at_90_cm4096"] = (skewed(n, 5, 4, 63), 5, Setting(4096, True), "sa")
    out["smallest_at_90_cm4096"] = (skewed(n, 5, 1, 64), 5, Setting(4096, True), "sa")
    x = uniform(n, 5, 65)
    x[x == 2] = 3
    out["middle_symbol_absent"] = (x, 5, Setting(0, False, expect="some"), "sa_bwt")
    out["acgt_repeated"] = (np.tile(np.array([1, 2, 3, 4], np.uint8), 3000), 5, Setting(0, False), "sa_bwt")
    out["tgca_repeated"] = (np.tile(np.array([4, 3, 2, 1], np.uint8), 3000), 5, Setting(0, False), "sa")
    out["one_symbol"] = (np.full(5000, 3, np.uint8), 5, Setting(0, False, expect="none"), "sa_bwt")
    out["two_alternating"] = (np.tile(np.array([2, 4], np.uint8), 4000), 5, Setting(0, False), "sa_bwt")
    # stops and carry-ons: unattended (the tail kernel leaves word), then attended
    for attended in (0, 1):
        for cm in (0, 4096):
            out[f"poly_a_{'attended' if attended else 'unattended'}_cm{cm}"] = (
                poly_a(60000, 70 + cm), 5, Setting(cm, cm != 0, attended), "sa_bwt" if attended else "sa")
    return out


def run_case(ctx, case, to_dev, to_host, new_dev):
    """both settings of the switch through the case's entry point; returns induce_early_s of the run with the switch on"""
    x, sigma, setting, entry = case
    n = x.size
    want = oracle.sa_is(x, sigma)
    bw_want = oracle.bwt(x, want)
    placed = None
    try:
        ctx.set_small_direct_max(0)
        ctx.set_chain_max_entries(-1 if setting.chain_max is None else setting.chain_max)
        ctx.set_induce_batch(setting.batch)
        ctx.set_induce_attended(setting.attended)
        ctx.set_induce_batch_min(-1 if setting.batch_min is None else setting.batch_min)
        d_text = to_dev(x)
        for on in (True, False):
            ctx.set_induce_early_s(on)
            sa = new_dev(n + 1, np.uint32)
            if entry == "sa_bwt":
                bw = new_dev(n + 1, np.uint8)
                ctx.sa_bwt_build_dev(d_text, n, sigma, sa, bw)
                assert (to_host(bw, np.uint8) == bw_want).all(), ("bwt", on)
            else:
                ctx.sa_build_dev(d_text, n, sigma, sa)
            assert (to_host(sa, np.uint32) == want).all(), ("sa", on)
            st = ctx.last_stats()
            if on:
                placed = st["induce_early_s"]
            else:
                assert st["induce_early_s"] == 0, st
    finally:
        ctx.set_induce_early_s(True)
        ctx.set_chain_max_entries(-1)
        ctx.set_induce_batch(True)
        ctx.set_induce_attended(0)
        ctx.set_induce_batch_min(-1)
    most = ascents_into_l(x)
    print(f"induce_early_s {placed} of {most} ascents into L-type positions")
    assert placed <= most
    if setting.expect == "all":
        assert placed == most
    elif setting.expect == "some":
        assert placed > 0
    elif setting.expect == "none":
        assert placed == 0
    return placed
