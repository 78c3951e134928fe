"""sx_fastq_index_dev on the GPU: every image of tests/fastq_cases.py, the ones tests/test_index_cpu.py runs on the CPU
execution harness, put to the contract's restatement in Python, the host's sx_fastq_index and the device function."""
import pytest

import fastq_cases as fq
from device_memory import GpuMemory
from sam_cases import sam_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mem():
    return GpuMemory()


def test_fastq_dev_on_the_fixture_images(gpu_ctx, mem):
    images = fq.fixture_images(sam_cases())
    for case in images:
        fq.check_image(gpu_ctx, mem, case)
    assert len(images) >= 2 * 4


def test_fastq_dev_in_contract(gpu_ctx, mem):
    for case in fq.in_contract_images():
        fq.check_image(gpu_ctx, mem, case)
    fq.check_in_contract_fields(gpu_ctx, mem)


@pytest.mark.parametrize("data", fq.OUT_OF_CONTRACT)
def test_fastq_dev_out_of_contract(gpu_ctx, mem, data):
    assert fq.agree(gpu_ctx, mem, data, expect=False) == "-4"


def test_fastq_dev_generated_images(gpu_ctx, mem):
    for case in fq.generated_images():
        fq.check_image(gpu_ctx, mem, case)


def test_fastq_dev_soups_with_one_defect(gpu_ctx, mem):
    fq.check_defects(gpu_ctx, mem, fq.soups())


@pytest.mark.parametrize("family", ["line_role_edge_images", "long_line_images", "dense_tile_images",
                                    "shifted_tile_multiple_images"])
def test_fastq_dev_at_the_tiles_edges(gpu_ctx, mem, family):
    for case in getattr(fq, family)():
        fq.check_image(gpu_ctx, mem, case)


def test_fastq_dev_defects_at_the_tiles_edges(gpu_ctx, mem):
    fq.check_defects(gpu_ctx, mem, fq.defects_at_tile_edges())


def test_fastq_dev_twice_the_same_bytes(gpu_ctx, mem):
    for case in fq.determinism_images():
        fq.check_deterministic(gpu_ctx, mem, case)
