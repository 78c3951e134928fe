"""A restatement of the reference's k-edit BWT search (stralg/bwt.c:226-422) over numpy C / O / RO tables.
TEST INFRASTRUCTURE ONLY: the checker for inputs too large for the fixture, pinned to the fixture by
tests/test_approx_cpu.py.

o and ro are position-major (N+1, sigma) arrays (O(a, i) = o[i, a]); patterns are remapped symbols.
"""
import numpy as np


def _cigar(edits):
    out, k = [], 0
    while k < len(edits):
        r = k
        while r < len(edits) and edits[r] == edits[k]:
            r += 1
        out.append(f"{r - k}{edits[k]}")
        k = r
    return "".join(out)


def d_table(c, ro, N, pattern):
    """bwt.c:319-338: the least number of edits pattern[0 .. i] needs, from the reversed text's O table."""
    out, me, L, R = [], 0, 0, N
    for a in pattern:
        L = int(c[a]) + int(ro[L, a])
        R = int(c[a]) + int(ro[R, a])
        if L >= R:
            me += 1
            L, R = 0, N
        out.append(me)
    return out


def intervals(c, o, ro, pattern, k):
    """The reference iterator's hit list: [(L, R, match_length, cigar)] in its order (bwt.c:226-348).  Empty for an
    empty pattern, a symbol 0 or >= sigma, or k < 0 (the reference asserts or reads out of bounds on the first two)."""
    p = [int(x) for x in pattern]
    sigma = c.size
    N = o.shape[0] - 1
    if not p or k < 0 or min(p) == 0 or max(p) >= sigma:
        return []
    m = len(p)
    D = d_table(c, ro, N, p) if ro is not None else None
    cc = [int(x) for x in c]
    hits = []
    edits = []

    def rec(L, R, i, ml, e):
        lower = D[i] if (i >= 0 and D is not None) else 0
        if e < lower:
            return
        if i < 0:
            hits.append((L, R, ml, _cigar(edits[::-1])))
            return
        rowL, rowR = o[L], o[R]
        for a in range(1, sigma):
            nL, nR = cc[a] + int(rowL[a]), cc[a] + int(rowR[a])
            cost = 0 if a == p[i] else 1
            if e - cost < 0 or nL >= nR:
                continue
            edits.append("M")
            rec(nL, nR, i - 1, ml + 1, e - cost)
            edits.pop()
        edits.append("I")
        rec(L, R, i - 1, ml, e - 1)
        edits.pop()
        for a in range(1, sigma):
            nL, nR = cc[a] + int(rowL[a]), cc[a] + int(rowR[a])
            if nL >= nR:
                continue
            edits.append("D")
            rec(nL, nR, i, ml + 1, e - 1)
            edits.pop()

    # the root: M and I only (bwt.c:364-394)
    i = m - 1
    rowL, rowR = o[0], o[N]
    for a in range(1, sigma):
        nL, nR = cc[a] + int(rowL[a]), cc[a] + int(rowR[a])
        cost = 0 if a == p[i] else 1
        if k - cost < 0 or nL >= nR:
            continue
        edits.append("M")
        rec(nL, nR, i - 1, 1, k - cost)
        edits.pop()
    edits.append("I")
    rec(0, N, i - 1, 0, k - 1)
    edits.pop()
    return hits


def matches(c, o, ro, sa, pattern, k):
    """[(position, match_length, cigar)] as next_bwt_approx_match yields them"""
    out = []
    for L, R, ml, cigar in intervals(c, o, ro, pattern, k):
        out.extend((int(pos), ml, cigar) for pos in sa[L:R])
    return out


def tables(sym, sigma):
    """(sa, c, o, ro) of build_complete_table(.., true) from the oracle's restatement (test infrastructure)."""
    import oracle
    sym = np.asarray(sym, np.uint8)
    sa = oracle.sa_is(sym, sigma)
    rsym = sym[::-1].copy()
    rsa = oracle.sa_is(rsym, sigma)
    return sa, oracle.c_table(sym, sigma), oracle.o_table(sym, sa, sigma), oracle.o_table(rsym, rsa, sigma)
