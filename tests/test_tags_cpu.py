"""NM:i and MD:Z behind QUAL (SX_MAP_TAGS) through the CPU execution harness (tests/tags_cases.py): the
mapper's texts against the reference mapper's recorded ones with every line extended by a walk over its own POS, CIGAR and
SEQ, under the other flags, in every form of the index, in rooms that have to grow; the flags word; the kernels' public
entries on made-up hits.

The harness lays a slice of 256 bytes out in a workgroup, so lines break inside the new fields here at every size."""
import ctypes as C

import numpy as np
import pytest

import best_cases as bc
import hamming_cases as hc
import tags_cases as tc
from approx_cases import remapped
from device_memory import HarnessMemory
from stralg_amd import _lib, api
from test_sam_cpu import records_of

MEM = HarnessMemory()
KERNEL = tc.kernel_cases()
REFUSED = {c["name"]: c for c in tc.refused_cases()}


def with_strings(ctx, case, name):
    """None for the small genomes (the index is built from the FASTA image); for the genome files the records of
    test_sam_cpu.records_of, each with its remapped string and terminator, for Index.from_tables"""
    if not name.startswith("hg38"):
        return None
    out = []
    for (rname, t), (_, seq) in zip(records_of(ctx, case["fasta"]), ctx.fasta_records(case["fasta"])):
        string = np.concatenate([remapped(seq)[0], np.zeros(1, np.uint8)]).astype(np.uint8)
        out.append((rname, api.BwtTable(t.remap_table, api.SuffixArray(string, t.sa.array), t.c_table, t.o_table, t.ro_table)))
    return out


@pytest.fixture(scope="module")
def cases():
    return tc.whole_cases()


@pytest.fixture(scope="module")
def flag_cases():
    return bc.best_cases()


# ---- the guards: an oracle that prints "NM:i:0 MD:Z:<length>" everywhere cannot hide a failure ----------------------------
def test_recorded_texts_hold_what_the_walk_tells_apart(cases):
    tc.check_guards(cases)


def test_made_up_hits_say_what_they_were_built_for():
    tc.check_expected_fields()
    assert sorted(KERNEL) == sorted(tc.KERNEL_CASE_NAMES) and sorted(REFUSED) == sorted(tc.REFUSED_NAMES)


# ---- the mapper -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.WHOLE_TEXT)
def test_whole_text(emu_ctx, cases, name):
    c = cases[name]
    chunks, st = tc.stream_tagged(emu_ctx, api.Index, c, c["k"], records=with_strings(emu_ctx, c, name))
    bc.check_text(b"".join(chunks), tc.want_whole(c))
    assert st["retries"] == 0


@pytest.mark.parametrize("name,k,both,best,indels", tc.FLAG_PARAMS, ids=tc.FLAG_IDS)
def test_with_the_other_flags(emu_ctx, flag_cases, name, k, both, best, indels):
    c = flag_cases[name]
    chunks, _ = tc.stream_tagged(emu_ctx, api.Index, c, k, both, best, indels, records=with_strings(emu_ctx, c, name))
    bc.check_text(b"".join(chunks), tc.want_flags(c, k, both, best, indels))


@pytest.mark.parametrize("form", hc.FORMS, ids=hc.FORM_IDS)
def test_index_forms(emu_ctx, cases, flag_cases, form):
    tc.check_index_form(emu_ctx, api.Index, cases, flag_cases, form)


@pytest.mark.parametrize("window,batch", hc.WINDOWS)
def test_windows_and_batches(emu_ctx, flag_cases, window, batch):
    tc.check_windows(emu_ctx, api.Index, flag_cases["two-records-best"], window, batch)


def test_two_calls_on_one_context(emu_ctx, cases):
    c = cases["test-out/k2"]
    with api.Index.from_fasta(c["fasta"], ctx=emu_ctx, compact=True, sa_sample=32) as idx:
        first = idx.map_reads(c["fastq"], 2, tags=True)
        plain = idx.map_reads(c["fastq"], 2)
        assert idx.map_reads(c["fastq"], 2, tags=True) == first == tc.want_whole(c) and plain == c["sam"]


def test_module_level_map_reads(emu_ctx, cases, flag_cases):
    c = cases["test-out/k2"]
    bc.check_text(api.map_reads(c["fasta"], c["fastq"], 2, ctx=emu_ctx, tags=True), tc.want_whole(c))
    c = flag_cases["test-out"]
    bc.check_text(api.map_reads(c["fasta"], c["fastq"], 2, ctx=emu_ctx, both_strands=True, best=True, indels=False, tags=True),
                  tc.want_flags(c, 2, True, True, False))


# ---- the flags word -------------------------------------------------------------------------------------------------------
def test_flags_word(emu_ctx, flag_cases):
    """64, 65, 72, 80 and 89 are accepted where an index has its strings; records of tables alone answer SX_E_ARG with
    nothing sunk; 66, 68 and 96 are refused everywhere"""
    c = flag_cases["test-out"]
    records = records_of(emu_ctx, c["fasta"])
    recs = (_lib.MapRecord * 8)()
    keep = []
    for r, (rname, t) in enumerate(records):
        recs[r] = api._map_record(rname, t, keep)
    chunks = []

    def sink(user, section, data, n):
        chunks.append(C.string_at(data, n))
        return 0

    cb = _lib.SINK_FN(sink)
    buf = np.frombuffer(c["fastq"], np.uint8)
    lib, h = emu_ctx.lib, emu_ctx.h
    limit = lib.sx_map_reads_limit
    with api.Index.from_fasta(c["fasta"], ctx=emu_ctx) as idx, api.Index.from_tables(records, ctx=emu_ctx) as bare:
        assert not any(bare.record_info(r).has_string for r in range(len(records)))
        for flags in (64, 65, 72, 80, 89):
            both, best, indels = bool(flags & 1), bool(flags & 8), not flags & 16
            assert flags == _lib.map_flags(both, best, indels, tags=True)
            del chunks[:]
            assert lib.sx_index_map_reads_ex(h, idx._handle(), buf.ctypes.data, buf.size, 2, flags, cb, None) == 0
            bc.check_text(b"".join(chunks), tc.want_flags(c, 2, both, best, indels))
            assert limit(5, 5, flags) == 0
            del chunks[:]
            assert lib.sx_map_reads_stream_ex(h, recs, len(records), buf.ctypes.data, buf.size, 2, flags, cb, None) == _lib.SX_E_ARG
            assert b"string" in lib.sx_last_error(h)
            assert lib.sx_index_map_reads_ex(h, bare._handle(), buf.ctypes.data, buf.size, 2, flags, cb, None) == _lib.SX_E_ARG
            assert b"string" in lib.sx_last_error(h) and not chunks
            # without the bit both still map
            assert lib.sx_index_map_reads_ex(h, bare._handle(), buf.ctypes.data, buf.size, 2, flags & ~64, cb, None) == 0
            plain = hc.want_of(c, 2, both, best) if not indels else bc.want_of(c, 2, both) if best else bc.plain_of(c, 2, both)
            bc.check_text(b"".join(chunks), plain)
        del chunks[:]
        for flags in (66, 68, 96):
            assert lib.sx_map_reads_stream_ex(h, recs, len(records), buf.ctypes.data, buf.size, 2, flags, cb, None) == _lib.SX_E_ARG
            assert lib.sx_index_map_reads_ex(h, idx._handle(), buf.ctypes.data, buf.size, 2, flags, cb, None) == _lib.SX_E_ARG
            assert limit(5, 5, flags) == _lib.SX_E_ARG
        assert not chunks
        with pytest.raises(api.StralgAmdError, match="code -1"):
            bare.map_reads(c["fastq"], 2, tags=True)
        with pytest.raises(api.StralgAmdError, match="code -1"):
            emu_ctx.map_reads_stream(records, c["fastq"], 2, chunks.append, tags=True)
    assert limit(2 ** 32 - 1, 1, 64) == 0 and limit(2 ** 32, 1, 64) == _lib.SX_E_ARG
    assert limit(2 ** 31 - 1, 1, 65) == 0 and limit(2 ** 31, 1, 65) == _lib.SX_E_ARG
    assert _lib.SX_MAP_TAGS == 64 and _lib.map_flags() == 0 and _lib.map_flags(True, True, False) == 25


# ---- the kernels' entries on made-up hits ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.KERNEL_CASE_NAMES)
def test_kernel_text(emu_ctx, name):
    tc.check_tag_text(emu_ctx, MEM, KERNEL[name])


@pytest.mark.parametrize("name", tc.REFUSED_NAMES)
def test_kernel_refuses(emu_ctx, name):
    tc.check_tag_refused(emu_ctx, MEM, REFUSED[name])


def test_kernel_entry_arguments(emu_ctx):
    """texts or letters missing, positions without their offsets: SX_E_ARG; a tagged batch of no hits is empty"""
    case = KERNEL["one-symbol"]
    b = tc.TagBatch(emu_ctx, MEM, case)
    ex = b.batch.ex
    for bad in (_lib.SamBatchTags(ex, None, api._ptr(b.d_letters), None, None, 0),
                _lib.SamBatchTags(ex, api._ptr(b.d_text_list), None, None, None, 0),
                _lib.SamBatchTags(ex, api._ptr(b.d_text_list), api._ptr(b.d_letters), api._ptr(b.d_off), None, 0)):
        with pytest.raises(api.StralgAmdError, match="code -1"):
            emu_ctx.sam_layout_dev(bad, b.d_off)
    empty = tc.TagBatch(emu_ctx, MEM, dict(case, rows=[]))
    assert empty.total == 0 and empty.text() == b""
