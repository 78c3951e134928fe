"""Inputs shared by the CPU-harness and GPU tests of the inverse, LCP and exact-search kernels (sx_extras.hip).
TEST INFRASTRUCTURE ONLY."""
import numpy as np


def fibonacci(n):
    """the first n symbols of the Fibonacci word over {1, 2}"""
    a, b = np.array([1], np.uint8), np.array([1, 2], np.uint8)
    while b.size < n:
        a, b = b, np.concatenate([b, a])
    return b[:n].copy()


def exact_patterns(x, sigma, rng):
    """(patterns, expected (L, R) or None for the oracle's): substrings of x at lengths around the kernel's 16-symbol words
    and the text's length, the same with one symbol changed, random ones, and one symbol 0 or >= sigma at every position of
    a word (inside a stretch of the text, so the interval is not empty when the search reaches it: (1, 0))"""
    n = x.size
    pats, want = [], []
    lengths = [0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, n - 1, n, n + 1, n + 2, 2 * n + 5]
    for m in lengths:
        for _ in range(3):
            if m <= n:
                a = int(rng.integers(0, n - m + 1))
                p = x[a:a + m].copy()
            else:  # longer than the text: the text with more symbols around it
                p = rng.integers(1, sigma, m).astype(np.uint8)
                p[:n] = x
            pats.append(p)
            want.append(None)
            if m:
                q = p.copy()
                q[int(rng.integers(0, m))] = int(rng.integers(1, sigma))
                pats.append(q)
                want.append(None)
                pats.append(rng.integers(1, sigma, m).astype(np.uint8))
                want.append(None)
    bad_symbols = (0,) if sigma == 256 else (0, sigma, 255)
    for m in (16, 17, 33):
        a = int(rng.integers(0, n - m + 1))
        for pos in range(m):
            for b in bad_symbols:
                p = x[a:a + m].copy()
                p[pos] = b
                pats.append(p)
                want.append((1, 0))
    # the last pattern ends where the (unpadded) pattern buffer ends, its last 16 symbols one whole word
    pats.append(x[n - 40:n - 1].copy())
    want.append(None)
    return pats, want

