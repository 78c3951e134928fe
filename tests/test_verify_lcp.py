"""stralg_amd.verify.verify_inverse_lcp_on_device on CPU tensors: it accepts the oracle's inverse and LCP arrays and
rejects each single-entry corruption of them (the check the GPU tests use where a host LCP would take minutes)."""
import numpy as np
import pytest

import oracle
from stralg_amd.synth import synth
from stralg_amd.verify import verify_inverse_lcp_on_device


def _texts():
    rng = np.random.default_rng(5)
    fib_a, fib_b = np.array([1], np.uint8), np.array([1, 2], np.uint8)
    while fib_b.size < 3000:
        fib_a, fib_b = fib_b, np.concatenate([fib_b, fib_a])
    dup = synth(5000, 5, 8)
    dup[3000:4500] = dup[200:1700]
    return {
        "random": (rng.integers(1, 5, 4000).astype(np.uint8), 5),
        "random256": (rng.integers(1, 256, 1500).astype(np.uint8), 256),
        "periodic": (np.tile(np.array([1, 2, 2, 1, 3], np.uint8), 600), 4),
        "one-symbol": (np.ones(2500, np.uint8), 2),
        "fibonacci": (fib_b, 3),
        "duplicated": (dup, 5),
        "one": (np.array([3], np.uint8), 4),
    }


def _arrays(x, sigma):
    import torch
    sa = oracle.sa_is(x, sigma)
    inv, lcp = oracle.inverse(sa), oracle.lcp(x, sa)
    t = lambda a: torch.from_numpy(a.view(np.int32).copy())
    return torch.from_numpy(x.copy()), t(sa), t(inv), t(lcp), lcp


@pytest.mark.parametrize("name", list(_texts()))
def test_accepts_the_oracle(name):
    x, sigma = _texts()[name]
    text, sa, inv, lcp, _ = _arrays(x, sigma)
    assert verify_inverse_lcp_on_device(text, sa, inv, lcp, x.size, chunk=997)  # (several chunks, one cut mid-way)
    assert verify_inverse_lcp_on_device(text, sa, inv, lcp, x.size)


@pytest.mark.parametrize("name", ["random", "periodic", "one-symbol", "fibonacci", "duplicated"])
def test_rejects_each_mutant(name):
    x, sigma = _texts()[name]
    text, sa, inv, lcp, lcp_np = _arrays(x, sigma)
    rng = np.random.default_rng(len(name))
    pos = np.flatnonzero(lcp_np[1:] > 0) + 1
    j = int(pos[rng.integers(0, pos.size)])  # an entry with a common prefix, so that -1 and 0 both change it
    mutants = {
        "lcp+1": lambda l, i: l.__setitem__(j, l[j] + 1),
        "lcp-1": lambda l, i: l.__setitem__(j, l[j] - 1),
        "lcp=0": lambda l, i: l.__setitem__(j, 0),
        "lcp[0]=1": lambda l, i: l.__setitem__(0, 1),
        "last+1": lambda l, i: l.__setitem__(x.size, l[x.size] + 1),
        "inv swap": lambda l, i: i.__setitem__([3, 7], i[[7, 3]]),
    }
    for what, mutate in mutants.items():
        l2, i2 = lcp.clone(), inv.clone()
        mutate(l2, i2)
        with pytest.raises(AssertionError):
            verify_inverse_lcp_on_device(text, sa, i2, l2, x.size, chunk=997)
        assert (l2 != lcp).any() or (i2 != inv).any(), what
