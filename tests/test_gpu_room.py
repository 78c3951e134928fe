"""The retries of the read mapper's loop on the GPU (tests/room_cases.py): the cases of tests/test_room_cpu.py, none cut, on
tables built on the device.  With SX_FLAG_SAM_ROOM_HITS the room of a batch's hits is small enough for the fixtures to make it
grow and to halve batches, the counters of sx_map_last_stats prove that they did, and every text is the reference mapper's
recorded one.  The device runs the search with 2^18 lanes where the harness has 256."""
import pytest

import room_cases as rc
import stralg_amd

pytestmark = pytest.mark.gpu

_TABLES = {}


@pytest.fixture
def tables(gpu_ctx):
    def records_of(fasta):
        if fasta not in _TABLES:
            _TABLES[fasta] = [(n, stralg_amd.build_complete_table(s, True, gpu_ctx)) for n, s in gpu_ctx.fasta_records(fasta)]
        return _TABLES[fasta]
    return records_of


@pytest.mark.parametrize("best,both", rc.MODES, ids=rc.MODE_IDS)
@pytest.mark.parametrize("room", rc.ROOMS)
def test_stream_rooms(gpu_ctx, tables, room, best, both):
    rc.check_stream_room(gpu_ctx, tables, room, best, both)


def test_rooms_batches_and_windows_interleave(gpu_ctx, tables):
    rc.check_interleaved(gpu_ctx, tables)


@pytest.mark.parametrize("best", [False, True], ids=["plain", "best"])
def test_one_record_tight(gpu_ctx, tables, best):
    rc.check_one_record(gpu_ctx, tables, best)


@pytest.mark.parametrize("best", [False, True], ids=["plain", "best"])
@pytest.mark.parametrize("form", rc.FORMS, ids=rc.FORM_IDS)
def test_index_forms_lone(gpu_ctx, form, best):
    rc.check_index_form(gpu_ctx, stralg_amd.Index, form, best)


def test_discard_and_the_switch_back_at_zero(gpu_ctx):
    rc.check_discard_and_back(gpu_ctx, stralg_amd.Index, rc.FORMS[2])


@pytest.mark.parametrize("best,both", rc.MODES, ids=rc.MODE_IDS)
def test_no_edits_in_a_room_of_one(gpu_ctx, tables, best, both):
    rc.check_no_edits(gpu_ctx, tables, best, both)
