"""The L pass's placing of S-type predecessors (tests/early_s_cases.py) on the GPU: every case with the switch on and
off against the oracle's suffix array and BWT, and the count of placed entries where the case fixes it."""
import numpy as np
import pytest

import early_s_cases as ec

pytestmark = pytest.mark.gpu

CASES = ec.cases(full_size=True)


@pytest.mark.parametrize("name", sorted(CASES))
def test_early_s(gpu_ctx, name):
    import torch
    tdt = {np.uint32: torch.int32, np.uint8: torch.uint8}
    ec.run_case(gpu_ctx, CASES[name], to_dev=lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda(),
                to_host=lambda d, dt: d.cpu().numpy().view(dt),
                new_dev=lambda count, dt: torch.zeros(count, dtype=tdt[dt], device="cuda"))
