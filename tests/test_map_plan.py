"""The read mapper's batch plan (stralg_amd/csrc/sx_map_plan.hpp): how much room the hits of a batch get, when the room grows
and when the batch is halved instead, the reads of a batch, the text's window, the rows of a located run.  It is arithmetic
on the free memory, four switches and counts, so tests/map_plan_grid.cpp computes it over a grid without a GPU and without
the library; its output is compared with tests/golden/map_plans.txt, recorded from the expressions as they stood inside the
mapper's loop before the plan was cut out of it.  The loop's retries themselves -- the room growing, the batch halved, the
batch run again -- are reached end to end by tests/test_room_cpu.py and tests/test_gpu_room.py through the room switch
(SX_FLAG_SAM_ROOM_HITS).

The grid: free memory unknown, 0, 2^20, 2^30, 80 x 2^30 bytes; 1, 2, 200 records; 1, 7, 2^20, 2^21 + 1 reads; groups of 0, 1, 2;
the batch switch at 0, 1, 7, 8; the window switch at 0, 1, 4096, 2^40.  Every room of (memory, records, switch 0 or 7) takes a
chain of needs: below twice the room, above it, between 4/5 of the largest room and the largest, above the largest with
several groups and with one, and at the largest with several.

The room switch's rows stand behind those (every line in front of them is what it was before the switch: with the switch at 0
no expression changed): the switch at 1, 4, 100, 400, 2^20, 2^40 over the same memory, records, reads, groups and batch
switches for the largest room and the first one, and chains from those rooms for batches of 240 and of 8 reads."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stralg_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "map_plans.txt")


def _build(out, extra):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", *extra, "-I" + CSRC, os.path.join(ROOT, "tests", "map_plan_grid.cpp"),
                           "-o", out])
    return out


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = _build(str(tmp_path_factory.mktemp("map_plan") / "grid"), [])
    return subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout


def test_plans_as_recorded(plans):
    with open(GOLDEN) as f:
        want = f.read()
    assert len(want.splitlines()) < 300
    got_lines, want_lines = plans.splitlines(), want.splitlines()
    assert len(got_lines) == len(want_lines)
    for g, w in zip(got_lines, want_lines):
        assert g == w
    assert plans == want


def _rows(plans, kind):
    return [line[len(kind) + 1:].split(" : ") for line in plans.splitlines() if line.startswith(kind + " ")]


def test_rows_worked_out_by_hand(plans):
    largest = {case: int(v) for case, v in _rows(plans, "largest")}
    assert largest["free=80*2^30"] == 1 << 27
    assert largest["free=2^30"] == 3728270
    assert largest["free=unknown"] == 1 << 26
    assert largest["free=2^20"] == 1 << 16

    nxt = {}
    for case, v in _rows(plans, "next"):
        c, r = dict(kv.split("=") for kv in case.split()), dict(kv.split("=") for kv in v.split())
        assert int(c["largest"]) == 1 << 27
        nxt[int(c["cap"]), int(c["need"]), int(c["groups"])] = (r["halve"] == "1", int(r["cap"]))
    assert nxt[1 << 16, 70000, 1] == (False, 131072)
    assert nxt[1 << 16, 200000, 1] == (False, 250000)
    assert nxt[1 << 26, 120000000, 1] == (False, 1 << 27)
    assert nxt[1 << 26, 140000000, 1] == (False, 175000000)
    assert nxt[1 << 26, 140000000, 2][0]

    # the room switch: the largest room is the switch whatever the memory, and the first room may be as small as one hit
    for case, v in _rows(plans, "switch_largest"):
        assert {kv.split("->")[1] for kv in v.split()} == {case.split("=")[1]}
    first = {}
    for case, v in _rows(plans, "room_first"):
        c = dict(kv.split("=") for kv in case.split())
        first[int(c["switch"]), int(c["batch_max"])] = int(v)
    assert first[1, 8] == 1 and first[1, 240] == 1
    assert first[100, 8] == 64 and first[100, 240] == 100  # (the guess: 4 hits x 8 reads x 2 records; 1920 is cut to the switch)
    assert first[400, 8] == 64 and first[400, 240] == 400
    assert first[1 << 20, 8] == 64 and first[1 << 20, 240] == 1920
    room = {}
    for case, v in _rows(plans, "room_next"):
        c, r = dict(kv.split("=") for kv in case.split()), dict(kv.split("=") for kv in v.split())
        room[int(c["cap"]), int(c["largest"]), int(c["need"]), int(c["groups"])] = (r["halve"] == "1", int(r["cap"]))
    assert room[1, 1, 5, 2] == (True, 1)
    assert room[1, 1, 5, 1] == (False, 6)  # (one group alone: 5 + 5 / 4, above the largest)
    assert room[6, 1, 7, 1] == (False, 12)  # (twice the room is more than 7 + 7 / 4)
    assert room[64, 100, 90, 4] == (False, 100)  # (twice 64 is cut to the largest: the need fits it)
    assert room[100, 100, 332, 2] == (True, 100)
    assert room[100, 100, 332, 1] == (False, 415)
    assert room[64, 1 << 20, 200, 4] == (False, 250)
    chains = dict(_rows(plans, "switch_chain"))
    assert chains["switch=100 n_records=2 flag=8 largest=100 cap=64"] == "96/4->100 300/4->halve 1100/3->halve 1100/1->1375 100/2->100"
    assert chains["switch=1 n_records=2 flag=0 largest=1 cap=1"] == "1/4->1 3/4->halve 1001/3->halve 1001/1->1251 1/2->1"
    assert len(_rows(plans, "switch_first")) == 6 * 5 * 3 and len(chains) == 6 * 3 * 2

    halved = {case: dict(kv.split("->") for kv in v.split()) for case, v in _rows(plans, "halved")}
    assert halved["g=1"]["7"] == "4"
    assert halved["g=2"]["6"] == "4"
    assert halved["g=2"]["10"] == "6"


def test_plan_under_sanitizers(plans, tmp_path):
    """the plan casts 64-bit switches to 32 bits and multiplies counts: the same program under AddressSanitizer and
    UndefinedBehaviorSanitizer"""
    exe = _build(str(tmp_path / "grid_san"), ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.stdout == plans
