"""The L pass's placing of S-type predecessors (tests/early_s_cases.py) over the CPU execution harness, which is built with
the tail kernel's short step limit, so the poly-A cases reach the stop record of an unattended pass."""
import numpy as np
import pytest

import early_s_cases as ec

CASES = ec.cases(full_size=False)


@pytest.mark.parametrize("name", sorted(CASES))
def test_early_s(emu_ctx, name):
    ec.run_case(emu_ctx, CASES[name], to_dev=lambda a: np.ascontiguousarray(a), to_host=lambda d, dt: d,
                new_dev=lambda count, dt: np.zeros(count, dtype=dt))


def test_poly_a_reaches_the_stop_record(emu_ctx):
    x, sigma, _, _ = CASES["poly_a_unattended_cm4096"]
    emu_ctx.set_chain_max_entries(4096)
    try:
        emu_ctx.sa_build(x, sigma)
        assert emu_ctx.last_stats()["induce_redo"] >= 1
    finally:
        emu_ctx.set_chain_max_entries(-1)
