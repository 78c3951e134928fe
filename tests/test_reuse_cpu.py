"""A context's second call, through the CPU execution harness (tests/reuse_cases.py; DESIGN.md, "What a context carries from
call to call"): every operation behind a scribble over the workspace, every ordered pair of operations in one context and
across two, operations behind failed calls, the look-back epoch's and the read-back sequence's wraps, regrowth and trim.
Every test makes its own context and closes it; after every operation no status word carries an epoch above the context's.

The harness runs the workgroups of a launch one after the other, so a look-back never meets a predecessor that has started
and not yet published: what a stale status word would do shows on the GPU only (tests/test_gpu_reuse.py).  The counters, the
zeroing at the wrap and everything the scribble overwrites are the same code on both.

The last test compiles the harness and a stand-alone program (tests/reuse_main.cpp) with AddressSanitizer and
UndefinedBehaviorSanitizer and runs the program: regrowth frees a slab that an earlier step of the same call may still hold a
pointer into, and only a sanitizer sees such a read."""
import os
import subprocess

import pytest

import conftest
import reuse_cases as rc
from device_memory import HarnessMemory
from stralg_amd.api import Context
from test_sam_cpu import records_of

CASES = rc.Cases(HarnessMemory(), rc.HARNESS, records_of)
OPS = list(CASES.ops)


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(conftest.ROOT, "stralg_amd", "csrc"), "emu"])
    return conftest.EMU_LIB


@pytest.fixture
def make_ctx(emu_lib):
    made = []

    def make():
        made.append(Context(0, lib_path=emu_lib))
        return made[-1]

    yield make
    for ctx in made:
        ctx.close()


def test_there_are_fourteen_operations_and_eight_failures():
    assert len(OPS) == 14 and len(CASES.failures()) == 8


def test_hooks_do_what_they_say(make_ctx):
    """scribble fills the status words with ready prefixes of the context's epoch and never a later one; the switches set what
    counters() reads; a fresh context has nothing"""
    ctx = make_ctx()
    k = ctx.counters()
    assert k["chain_epoch"] == 0 and k["readback_seq"] == 0 and not any(k["slab_bytes"]) and not k["has_child"]
    ctx.scribble(0xFF)  # (nothing to scribble on yet)
    CASES.sa_dna(ctx)
    k = rc.invariant(ctx)
    assert 0 < k["chain_slab_max_epoch"] <= k["chain_epoch"] and k["slab_bytes"][6] > 0
    ctx.scribble(0x01)
    assert ctx.counters()["chain_slab_max_epoch"] == k["chain_epoch"]
    ctx.set_chain_epoch(5)
    ctx.scribble(0x01)
    assert ctx.counters()["chain_slab_max_epoch"] == 5
    ctx.set_readback_seq(0xFFFFFFFF)
    assert ctx.counters()["readback_seq"] == 0xFFFFFFFF
    for bad in (-1, 256):
        with pytest.raises(Exception, match="code -1"):
            ctx.scribble(bad)
    with pytest.raises(Exception, match="code -1"):
        ctx.set_chain_epoch(1 << 24)
    CASES.sa_dna(ctx)
    rc.invariant(ctx)


def test_dirty_workspace(make_ctx):
    rc.check_dirty_workspace(CASES, make_ctx())


@pytest.mark.parametrize("first", OPS)
def test_ordered_pairs(make_ctx, first):
    rc.check_pairs(CASES, make_ctx, first)


@pytest.mark.parametrize("failure", list(CASES.failures()))
def test_after_a_failure(make_ctx, failure):
    rc.check_after_failure(CASES, make_ctx(), failure)


def test_epoch_wrap(make_ctx):
    rc.check_epoch_wrap(CASES, make_ctx())


def test_readback_sequence_wrap(make_ctx):
    rc.check_readback_sequence(CASES, make_ctx())


@pytest.mark.parametrize("family", list(rc.regrowth_families(CASES)))
def test_regrowth_and_trim(make_ctx, family):
    rc.check_regrowth(CASES, make_ctx, family)


def test_two_contexts_interleaved(make_ctx):
    """(the harness keeps __shared__ arrays as statics: two contexts take turns on one thread; the GPU suite uses two threads)"""
    rc.check_interleaved(CASES, make_ctx)


def test_reuse_program_under_sanitizers(tmp_path):
    """tests/reuse_main.cpp and the harness's objects with AddressSanitizer and UndefinedBehaviorSanitizer, objects and program
    in a temporary directory (not tests/emu/build_asan: conftest's child may be building there); the runtime comes with the
    executable, nothing is preloaded"""
    san = "-fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer"
    objd, lib, exe = str(tmp_path / "obj"), str(tmp_path / "libreuse_emu.so"), str(tmp_path / "reuse_main")
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(conftest.ROOT, "stralg_amd", "csrc"), "emu", "EMUOBJD=" + objd,
                           "EMUOUT=" + lib, "EMUFLAGS=-O1 -g " + san])
    objects = sorted(os.path.join(objd, f) for f in os.listdir(objd) if f.endswith(".o"))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g"] + san.split() + ["-I", os.path.join(conftest.ROOT, "include"),
                           os.path.join(conftest.ROOT, "tests", "reuse_main.cpp")] + objects + ["-o", exe, "-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.returncode, r.stderr[-4000:])
    assert r.stdout == "reuse ok\n"
