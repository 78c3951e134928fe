"""A context's second call on the GPU (tests/reuse_cases.py; DESIGN.md, "What a context carries from call to call"): what
tests/test_reuse_cpu.py runs through the CPU execution harness, at shapes that put 128 look-back tiles into a chained launch
and cross the thresholds that the harness build lowers (reuse_cases.GPU).  Here a look-back can meet a predecessor tile that
has started and not yet published, so a status word of an earlier launch -- the scribble writes the worst ones: ready
inclusive prefixes of the last epoch with a wrong value -- is read by the kernels that must ignore it.

Every test makes its own context and closes it.  The library works on a stream of its own: the cases call
torch.cuda.synchronize() (GpuMemory.sync) between torch's fills and a library call, as the other GPU tests do."""
import pytest

import reuse_cases as rc
from stralg_amd.api import Context

pytestmark = pytest.mark.gpu

_CASES = []


@pytest.fixture(scope="module")
def cases():
    if not _CASES:
        import torch
        assert torch.cuda.is_available(), "gpu tests need a GPU"
        from device_memory import GpuMemory
        _CASES.append(rc.Cases(GpuMemory(), rc.GPU))
    return _CASES[0]


OPS = list(rc.Cases(None, rc.GPU).ops)
FAILURES = list(rc.Cases(None, rc.GPU).failures())
FAMILIES = list(rc.regrowth_families(rc.Cases(None, rc.GPU)))


@pytest.fixture
def make_ctx():
    made = []

    def make():
        made.append(Context(0))
        return made[-1]

    yield make
    for ctx in made:
        ctx.close()


def test_dirty_workspace(cases, make_ctx):
    rc.check_dirty_workspace(cases, make_ctx())


@pytest.mark.parametrize("first", OPS)
def test_ordered_pairs(cases, make_ctx, first):
    rc.check_pairs(cases, make_ctx, first)


@pytest.mark.parametrize("failure", FAILURES)
def test_after_a_failure(cases, make_ctx, failure):
    rc.check_after_failure(cases, make_ctx(), failure)


def test_epoch_wrap(cases, make_ctx):
    rc.check_epoch_wrap(cases, make_ctx())


def test_readback_sequence_wrap(cases, make_ctx):
    rc.check_readback_sequence(cases, make_ctx())


@pytest.mark.parametrize("family", FAMILIES)
def test_regrowth_and_trim(cases, make_ctx, family):
    rc.check_regrowth(cases, make_ctx, family)


def test_two_threads(cases, make_ctx):
    rc.check_two_threads(cases, make_ctx)
