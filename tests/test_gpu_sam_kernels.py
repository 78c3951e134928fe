"""sx_sam_layout_dev / sx_sam_emit_dev on the GPU with made-up hits: every case of tests/sam_kernel_cases.py, the ones
tests/test_sam_cpu.py runs on the CPU execution harness.  The harness runs workgroups one after the other and lanes as
fibers; a missing barrier, an LDS table reused a step early or a vector store to an odd address shows only here."""
import pytest

import sam_kernel_cases as skc
from device_memory import GpuMemory

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mem():
    return GpuMemory()


@pytest.fixture(scope="module")
def text_cases():
    return skc.text_cases()


def test_cigar_on_the_device(gpu_ctx, mem):
    skc.check_cigars(gpu_ctx, mem, skc.cigar_case())


def test_position_digits(gpu_ctx, mem):
    skc.check_position_digits(gpu_ctx, mem, skc.digit_case())


@pytest.mark.parametrize("window", skc.WINDOWS)
def test_emit_window_sizes(gpu_ctx, mem, window):
    skc.check_window(gpu_ctx, mem, skc.digit_case(), window)


def test_layout_rejects_hits_outside_the_batch(gpu_ctx, mem):
    for case in skc.refused_cases():
        skc.check_refused(gpu_ctx, mem, case)


def test_empty_batch(gpu_ctx, mem):
    skc.check_empty(gpu_ctx, mem, skc.empty_case())


@pytest.mark.parametrize("name", skc.TEXT_CASE_NAMES)
def test_layout_and_emit_at_the_kernels_thresholds(gpu_ctx, mem, text_cases, name):
    skc.check_text(gpu_ctx, mem, text_cases[name])


def test_text_case_names_are_the_modules(text_cases):
    assert list(text_cases) == skc.TEXT_CASE_NAMES
