"""Host-side mirror of stralg's interface for the suffix-array / BWT-table path.

Names, argument meaning and results follow the reference declarations cited on
each function; arrays come back as numpy arrays instead of malloc'd pointers.
All work happens in libstralg_amd.so (include/stralg_amd.h); a missing library
or GPU raises -- there is no CPU fallback.
"""
import ctypes as C
import threading
import time

import numpy as np

from . import _lib


class StralgAmdError(RuntimeError):
    pass


def _ptr(x):
    """Raw address of a numpy array, a torch tensor, an int address or None."""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    raise TypeError(f"cannot take the address of {type(x)!r}")


class Context:
    """One device context (sx_ctx): a HIP stream plus cached workspace on one GPU."""

    def __init__(self, device=0, lib_path=None):
        self.lib = _lib.load(lib_path)
        self.device = device
        h = C.c_void_p()
        rc = self.lib.sx_ctx_create(device, C.byref(h))
        if rc != 0 or not h:
            raise StralgAmdError(
                f"sx_ctx_create(device={device}) failed with code {rc}: no usable GPU "
                "(stralg_amd has no CPU fallback)")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.sx_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            msg = self.lib.sx_last_error(self.h)
            raise StralgAmdError(f"{what} failed with code {rc}: {msg.decode() if msg else ''}")

    # ---- host-buffer entry points ------------------------------------------------
    def sa_build(self, text, alphabet_size):
        """sx_sa_build: text = uint8 symbols in [1, alphabet_size) without terminator."""
        text = np.ascontiguousarray(text, dtype=np.uint8)
        out = np.empty(text.size + 1, dtype=np.uint32)
        self._check(self.lib.sx_sa_build(self.h, _ptr(text), text.size, alphabet_size, _ptr(out)), "sx_sa_build")
        return out

    def bwt_tables(self, text, sa, sigma, want_o=True):
        """sx_bwt_tables: returns (c_table[sigma], o_table[(N+1), sigma] or None)."""
        text = np.ascontiguousarray(text, dtype=np.uint8)
        sa = np.ascontiguousarray(sa, dtype=np.uint32)
        N = sa.size
        if text.size != N - 1:
            raise ValueError("sa must have len(text) + 1 entries")
        c = np.zeros(sigma, dtype=np.uint32)
        o = np.empty((N + 1, sigma), dtype=np.uint32) if want_o else None
        self._check(self.lib.sx_bwt_tables(self.h, _ptr(text), _ptr(sa), N, sigma, _ptr(c), _ptr(o)), "sx_bwt_tables")
        return c, o

    def build_tables(self, text, sigma, want_sa=True, want_o=True):
        """sx_build_tables: (sa or None, c_table, o_table or None) with one text upload."""
        text = np.ascontiguousarray(text, dtype=np.uint8)
        N = text.size + 1
        sa = np.empty(N, dtype=np.uint32) if want_sa else None
        c = np.zeros(sigma, dtype=np.uint32)
        o = np.empty((N + 1, sigma), dtype=np.uint32) if want_o else None
        self._check(self.lib.sx_build_tables(self.h, _ptr(text), text.size, sigma, _ptr(sa), _ptr(c), _ptr(o)),
                    "sx_build_tables")
        return sa, c, o

    # ---- device-buffer entry points (torch tensors or raw addresses) --------------
    def sa_build_dev(self, d_text, n, alphabet_size, d_sa_out):
        self._check(self.lib.sx_sa_build_dev(self.h, _ptr(d_text), n, alphabet_size, _ptr(d_sa_out)), "sx_sa_build_dev")

    def sa_bwt_build_dev(self, d_text, n, alphabet_size, d_sa_out, d_bwt_out):
        self._check(self.lib.sx_sa_bwt_build_dev(self.h, _ptr(d_text), n, alphabet_size, _ptr(d_sa_out),
                                                 _ptr(d_bwt_out)), "sx_sa_bwt_build_dev")

    def bwt_tables_from_bwt_dev(self, d_bwt, N, sigma, d_c_out, d_o_out=None):
        self._check(self.lib.sx_bwt_tables_from_bwt_dev(self.h, _ptr(d_bwt), N, sigma, _ptr(d_c_out), _ptr(d_o_out)),
                    "sx_bwt_tables_from_bwt_dev")

    def bwt_tables_dev(self, d_text, d_sa, N, sigma, d_c_out, d_o_out=None, d_bwt_out=None):
        self._check(self.lib.sx_bwt_tables_dev(self.h, _ptr(d_text), _ptr(d_sa), N, sigma, _ptr(d_c_out),
                                               _ptr(d_o_out), _ptr(d_bwt_out)), "sx_bwt_tables_dev")

    def synth_dev(self, d_out, n, sigma, seed):
        self._check(self.lib.sx_synth_dev(self.h, _ptr(d_out), n, sigma, seed), "sx_synth_dev")

    # ---- consumers of a resident suffix array / table ---------------------------------
    def membw_probe(self, d_a, d_b, nbytes, reps=5):
        """the box's streaming rates in GB/s over two device buffers of nbytes each: read, fill, copy, four-way split"""
        out = (C.c_double * 4)()
        self._check(self.lib.sx_membw_probe(self.h, _ptr(d_a), _ptr(d_b), nbytes, reps, out), "sx_membw_probe")
        return dict(zip(("read", "fill", "copy", "split4"), (float(v) for v in out)))

    def inverse_lcp(self, text, sa, want_lcp=True):
        """sx_sa_inverse_lcp: (inverse, lcp or None) as compute_inverse / compute_lcp (suffix_array.c:53-85)."""
        text = np.ascontiguousarray(text, dtype=np.uint8)
        sa = np.ascontiguousarray(sa, dtype=np.uint32)
        inv = np.empty(sa.size, dtype=np.uint32)
        lcp = np.empty(sa.size, dtype=np.uint32) if want_lcp else None
        self._check(self.lib.sx_sa_inverse_lcp(self.h, _ptr(text), _ptr(sa), sa.size, _ptr(inv), _ptr(lcp)),
                    "sx_sa_inverse_lcp")
        return inv, lcp

    def sa_inverse_dev(self, d_sa, N, d_inv):
        self._check(self.lib.sx_sa_inverse_dev(self.h, _ptr(d_sa), N, _ptr(d_inv)), "sx_sa_inverse_dev")

    def sa_lcp_dev(self, d_text, d_sa, N, d_inv, d_lcp):
        self._check(self.lib.sx_sa_lcp_dev(self.h, _ptr(d_text), _ptr(d_sa), N, _ptr(d_inv), _ptr(d_lcp)), "sx_sa_lcp_dev")

    def bwt_exact_search_dev(self, d_c, d_o, N, sigma, d_patterns, d_offsets, count, d_l, d_r):
        self._check(self.lib.sx_bwt_exact_search_dev(self.h, _ptr(d_c), _ptr(d_o), N, sigma, _ptr(d_patterns),
                                                     _ptr(d_offsets), count, _ptr(d_l), _ptr(d_r)),
                    "sx_bwt_exact_search_dev")

    def bwt_approx_search_dev(self, d_c, d_o, d_ro, N, sigma, d_patterns, d_offsets, count, max_edits, d_hit_offsets,
                              d_hits=None, hit_capacity=0, indels=True):
        """sx_bwt_approx_search_dev: fills d_hit_offsets (count + 1 uint64) and, when d_hits is given and large enough,
        d_hits (hit_capacity records of _lib.APPROX_HIT_DTYPE); returns the number of hits.  More hits than
        hit_capacity raise StralgAmdError with code SX_E_CAPACITY (-5); the offsets are written all the same.
        indels=False (sx_bwt_approx_search_dev_ex, SX_SEARCH_NO_INDELS): mismatches only -- the hits of the call whose
        n_gaps is 0, in its order."""
        total = C.c_uint64(0)
        if indels:
            rc = self.lib.sx_bwt_approx_search_dev(self.h, _ptr(d_c), _ptr(d_o), _ptr(d_ro), N, sigma, _ptr(d_patterns),
                                                   _ptr(d_offsets), count, max_edits, _ptr(d_hit_offsets), _ptr(d_hits),
                                                   hit_capacity, C.byref(total))
        else:
            rc = self.lib.sx_bwt_approx_search_dev_ex(self.h, _ptr(d_c), _ptr(d_o), _ptr(d_ro), N, sigma, _ptr(d_patterns),
                                                      _ptr(d_offsets), count, max_edits, _ptr(d_hit_offsets), _ptr(d_hits),
                                                      hit_capacity, C.byref(total), _lib.search_flags(indels))
        self._check(rc, "sx_bwt_approx_search_dev" if indels else "sx_bwt_approx_search_dev_ex")
        return int(total.value)

    def bwt_best_search_dev(self, d_c, d_o, d_ro, N, sigma, d_patterns, d_offsets, count, max_edits, d_stratum, d_hit_offsets,
                            d_hits=None, hit_capacity=0, indels=True):
        """sx_bwt_best_search_dev: Context.bwt_approx_search_dev by iterative deepening.  d_stratum (count bytes) <- the
        smallest edit count at which each pattern has a hit (0xFF: none within max_edits); a pattern's hits are those of
        bwt_approx_search_dev at that edit count, in its order.  Returns the number of hits; on SX_E_CAPACITY (raised) the
        offsets and strata are written all the same.  indels=False (sx_bwt_best_search_dev_ex): strata and hits are
        those of the search with indels=False, so a stratum is the smallest number of mismatches."""
        total = C.c_uint64(0)
        if indels:
            rc = self.lib.sx_bwt_best_search_dev(self.h, _ptr(d_c), _ptr(d_o), _ptr(d_ro), N, sigma, _ptr(d_patterns),
                                                 _ptr(d_offsets), count, max_edits, _ptr(d_stratum), _ptr(d_hit_offsets),
                                                 _ptr(d_hits), hit_capacity, C.byref(total))
        else:
            rc = self.lib.sx_bwt_best_search_dev_ex(self.h, _ptr(d_c), _ptr(d_o), _ptr(d_ro), N, sigma, _ptr(d_patterns),
                                                    _ptr(d_offsets), count, max_edits, _ptr(d_stratum), _ptr(d_hit_offsets),
                                                    _ptr(d_hits), hit_capacity, C.byref(total), _lib.search_flags(indels))
        self._check(rc, "sx_bwt_best_search_dev" if indels else "sx_bwt_best_search_dev_ex")
        return int(total.value)

    def patterns_select_dev(self, d_bytes, d_off, count, d_keep, d_bytes_out, d_off_out, d_ids_out):
        """sx_patterns_select_dev: the patterns q with d_keep[q] != 0, in order and flat, into d_bytes_out (16-byte aligned,
        the input's bytes + 16), d_off_out (count + 1, from 0) and d_ids_out (count: a kept pattern's number in the
        input); returns (kept patterns, their bytes)"""
        kept, nbytes = C.c_uint32(0), C.c_uint64(0)
        self._check(self.lib.sx_patterns_select_dev(self.h, _ptr(d_bytes), _ptr(d_off), count, _ptr(d_keep), _ptr(d_bytes_out),
                                                    _ptr(d_off_out), _ptr(d_ids_out), C.byref(kept), C.byref(nbytes)),
                    "sx_patterns_select_dev")
        return int(kept.value), int(nbytes.value)

    def bwt_approx_search(self, c, o, ro, sigma, patterns, offsets, max_edits, indels=True):
        """sx_bwt_approx_search over host arrays (o, ro: (N+1, sigma); ro may be None): (hit offsets[count + 1], hits as a
        structured array of _lib.APPROX_HIT_DTYPE).  indels=False: sx_bwt_approx_search_ex with SX_SEARCH_NO_INDELS."""
        c = np.ascontiguousarray(c, dtype=np.uint32)
        o = np.ascontiguousarray(o, dtype=np.uint32)
        ro = None if ro is None else np.ascontiguousarray(ro, dtype=np.uint32)
        patterns = np.ascontiguousarray(patterns, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
        count = offsets.size - 1
        hit_off = np.zeros(count + 1, dtype=np.uint64)
        hp, total = C.c_void_p(), C.c_uint64(0)
        args = (self.h, _ptr(c), _ptr(o), _ptr(ro), o.shape[0] - 1, sigma, _ptr(patterns) if patterns.size else None,
                _ptr(offsets), count, max_edits, _ptr(hit_off), C.byref(hp), C.byref(total))
        if indels:
            self._check(self.lib.sx_bwt_approx_search(*args), "sx_bwt_approx_search")
        else:
            self._check(self.lib.sx_bwt_approx_search_ex(*args, _lib.search_flags(indels)), "sx_bwt_approx_search_ex")
        n = int(total.value)
        hits = np.zeros(n, dtype=_lib.APPROX_HIT_DTYPE)
        if hp.value:
            C.memmove(hits.ctypes.data, hp.value, n * hits.dtype.itemsize)
            _libc_free(hp.value)
        return hit_off, hits

    # ---- the compact form of the O table (sx_occ.hpp) ------------------------------------------
    def occ_compact_bytes(self, N, sigma):
        """sx_occ_compact_bytes: bytes of the blocks of a table of N + 1 rows"""
        return int(self.lib.sx_occ_compact_bytes(N, sigma))

    def occ_compact_build_dev(self, d_bwt, N, sigma, d_blocks):
        self._check(self.lib.sx_occ_compact_build_dev(self.h, _ptr(d_bwt), N, sigma, _ptr(d_blocks)), "sx_occ_compact_build_dev")

    def occ_compact_expand_dev(self, d_blocks, N, sigma, row_lo, row_hi, d_rows):
        self._check(self.lib.sx_occ_compact_expand_dev(self.h, _ptr(d_blocks), N, sigma, row_lo, row_hi, _ptr(d_rows)),
                    "sx_occ_compact_expand_dev")

    def bwt_exact_search_compact_dev(self, d_c, d_occ, N, sigma, d_patterns, d_offsets, count, d_l, d_r):
        self._check(self.lib.sx_bwt_exact_search_compact_dev(self.h, _ptr(d_c), _ptr(d_occ), N, sigma, _ptr(d_patterns),
                                                             _ptr(d_offsets), count, _ptr(d_l), _ptr(d_r)),
                    "sx_bwt_exact_search_compact_dev")

    def bwt_approx_search_compact_dev(self, d_c, d_occ, d_rocc, N, sigma, d_patterns, d_offsets, count, max_edits, d_hit_offsets,
                                      d_hits=None, hit_capacity=0, indels=True):
        """sx_bwt_approx_search_compact_dev: Context.bwt_approx_search_dev over blocks in place of the full tables
        (indels=False: sx_bwt_approx_search_compact_dev_ex with SX_SEARCH_NO_INDELS)"""
        total = C.c_uint64(0)
        args = (self.h, _ptr(d_c), _ptr(d_occ), _ptr(d_rocc), N, sigma, _ptr(d_patterns), _ptr(d_offsets), count, max_edits,
                _ptr(d_hit_offsets), _ptr(d_hits), hit_capacity, C.byref(total))
        if indels:
            self._check(self.lib.sx_bwt_approx_search_compact_dev(*args), "sx_bwt_approx_search_compact_dev")
        else:
            self._check(self.lib.sx_bwt_approx_search_compact_dev_ex(*args, _lib.search_flags(indels)),
                        "sx_bwt_approx_search_compact_dev_ex")
        return int(total.value)

    # ---- the packed form of the compact table (sx_occ.hpp: a nibble a row, sigma <= 8) ---------
    def occ_packed_bytes(self, N, sigma):
        """sx_occ_packed_bytes: bytes of the packed blocks of a table of N + 1 rows (0 for sigma > 8)"""
        return int(self.lib.sx_occ_packed_bytes(N, sigma))

    def occ_packed_build_dev(self, d_bwt, N, sigma, d_blocks):
        self._check(self.lib.sx_occ_packed_build_dev(self.h, _ptr(d_bwt), N, sigma, _ptr(d_blocks)), "sx_occ_packed_build_dev")

    def occ_packed_expand_dev(self, d_blocks, N, sigma, row_lo, row_hi, d_rows):
        self._check(self.lib.sx_occ_packed_expand_dev(self.h, _ptr(d_blocks), N, sigma, row_lo, row_hi, _ptr(d_rows)),
                    "sx_occ_packed_expand_dev")

    def bwt_exact_search_packed_dev(self, d_c, d_occ, N, sigma, d_patterns, d_offsets, count, d_l, d_r):
        self._check(self.lib.sx_bwt_exact_search_packed_dev(self.h, _ptr(d_c), _ptr(d_occ), N, sigma, _ptr(d_patterns),
                                                            _ptr(d_offsets), count, _ptr(d_l), _ptr(d_r)),
                    "sx_bwt_exact_search_packed_dev")

    def bwt_approx_search_packed_dev(self, d_c, d_occ, d_rocc, N, sigma, d_patterns, d_offsets, count, max_edits, d_hit_offsets,
                                     d_hits=None, hit_capacity=0, indels=True):
        """sx_bwt_approx_search_packed_dev: Context.bwt_approx_search_dev over packed blocks in place of the full tables
        (indels=False: sx_bwt_approx_search_packed_dev_ex with SX_SEARCH_NO_INDELS)"""
        total = C.c_uint64(0)
        args = (self.h, _ptr(d_c), _ptr(d_occ), _ptr(d_rocc), N, sigma, _ptr(d_patterns), _ptr(d_offsets), count, max_edits,
                _ptr(d_hit_offsets), _ptr(d_hits), hit_capacity, C.byref(total))
        if indels:
            self._check(self.lib.sx_bwt_approx_search_packed_dev(*args), "sx_bwt_approx_search_packed_dev")
        else:
            self._check(self.lib.sx_bwt_approx_search_packed_dev_ex(*args, _lib.search_flags(indels)),
                        "sx_bwt_approx_search_packed_dev_ex")
        return int(total.value)

    # ---- SAM text of search hits (the read mapper's output) ---------------------------------
    def sam_batch(self, d_hits, n_hits, d_sa, sa_len, d_names, d_name_off, d_seqs, d_seq_off, d_quals, d_qual_off, n_reads,
                  d_rnames, d_rname_off, n_records=1, d_sa_list=None, d_sa_len_list=None, d_read_flags=None):
        """sx_sam_batch over device tensors (the caller keeps them alive): hits as sx_bwt_approx_search_dev leaves them,
        the suffix array, the reads' flat name / sequence / quality bytes with n_reads + 1 offsets each (uint32), the
        record names likewise.  d_read_flags (uint16, n_reads entries): a FLAG per read, and the batch is an
        sx_sam_batch_ex that sam_layout_dev / sam_emit_dev send to the _ex calls."""
        batch = _lib.SamBatch(_ptr(d_hits), n_hits, _ptr(d_sa), sa_len, _ptr(d_sa_list), _ptr(d_sa_len_list), _ptr(d_names),
                              _ptr(d_seqs), _ptr(d_quals), _ptr(d_name_off), _ptr(d_seq_off), _ptr(d_qual_off), n_reads,
                              _ptr(d_rnames), _ptr(d_rname_off), n_records)
        return batch if d_read_flags is None else _lib.SamBatchEx(batch, _ptr(d_read_flags))

    def sam_batch_tags(self, batch, d_text_list, d_letters, d_positions=None, d_pos_off=None, pos_base=0):
        """sx_sam_batch_tags of a batch of sam_batch (with flags or without): every line gets NM:i and MD:Z behind QUAL.
        d_text_list (uint64, one device address per record rank): the records' remapped texts, the sentinel last;
        d_letters (uint8, 256 per record rank): the letter behind every code.  d_positions (uint32) with d_pos_off (uint64,
        a first line per hit) and pos_base: positions located beforehand, in place of the suffix arrays' rows.
        sam_layout_dev / sam_emit_dev send it to the _tags calls."""
        ex = batch if isinstance(batch, _lib.SamBatchEx) else _lib.SamBatchEx(batch, None)
        return _lib.SamBatchTags(ex, _ptr(d_text_list), _ptr(d_letters), _ptr(d_positions), _ptr(d_pos_off), pos_base)

    @staticmethod
    def _sam_call(batch, stem):
        return stem + ("_tags" if isinstance(batch, _lib.SamBatchTags) else "_ex" if isinstance(batch, _lib.SamBatchEx) else "")

    def sam_layout_dev(self, batch, d_byte_offsets):
        """sx_sam_layout_dev (sx_sam_layout_dev_ex for a batch with flags, sx_sam_layout_dev_tags for one with tags):
        d_byte_offsets (n_hits + 1 uint64) <- every hit's first output byte; returns the text's length"""
        total = C.c_uint64(0)
        name = self._sam_call(batch, "sx_sam_layout_dev")
        self._check(getattr(self.lib, name)(self.h, C.byref(batch), _ptr(d_byte_offsets), C.byref(total)), name)
        return int(total.value)

    def sam_emit_dev(self, batch, d_byte_offsets, total_bytes, byte_lo, byte_hi, d_out):
        """sx_sam_emit_dev (sx_sam_emit_dev_ex for a batch with flags, sx_sam_emit_dev_tags for one with tags): bytes
        [byte_lo, byte_hi) of the text into d_out (uint8, 16-byte aligned)"""
        name = self._sam_call(batch, "sx_sam_emit_dev")
        self._check(getattr(self.lib, name)(self.h, C.byref(batch), _ptr(d_byte_offsets), total_bytes, byte_lo, byte_hi, _ptr(d_out)),
                    name)

    @staticmethod
    def _unmapped_batch(batch):
        if isinstance(batch, _lib.SamBatchTags):
            return batch
        ex = batch if isinstance(batch, _lib.SamBatchEx) else _lib.SamBatchEx(batch, None)
        return _lib.SamBatchTags(ex, None, None, None, None, 0)

    def sam_layout_dev_unmapped(self, batch, d_byte_offsets):
        """sx_sam_layout_dev_unmapped: sam_layout_dev of a batch (of sam_batch, with flags or not, or of sam_batch_tags)
        whose hits with R == L are placeholders, one FLAG 4 line each; returns the text's length"""
        total = C.c_uint64(0)
        b = self._unmapped_batch(batch)
        self._check(self.lib.sx_sam_layout_dev_unmapped(self.h, C.byref(b), _ptr(d_byte_offsets), C.byref(total)), "sx_sam_layout_dev_unmapped")
        return int(total.value)

    def sam_emit_dev_unmapped(self, batch, d_byte_offsets, total_bytes, byte_lo, byte_hi, d_out):
        """sx_sam_emit_dev_unmapped: bytes [byte_lo, byte_hi) of that text into d_out (uint8, 16-byte aligned)"""
        b = self._unmapped_batch(batch)
        self._check(self.lib.sx_sam_emit_dev_unmapped(self.h, C.byref(b), _ptr(d_byte_offsets), total_bytes, byte_lo, byte_hi, _ptr(d_out)),
                    "sx_sam_emit_dev_unmapped")

    def _mapq_batch(self, batch, d_hit_quality):
        return _lib.SamBatchMapq(self._unmapped_batch(batch), _ptr(d_hit_quality))

    def sam_layout_dev_mapq(self, batch, d_hit_quality, d_byte_offsets):
        """sx_sam_layout_dev_mapq: sam_layout_dev_unmapped of a batch with a quality word a hit (d_hit_quality, uint16, n_hits
        entries: the low 8 bits the MAPQ of the hit's lines, bit 8 set for 256 on top of their FLAG; None: SX_E_ARG);
        returns the text's length"""
        total = C.c_uint64(0)
        b = self._mapq_batch(batch, d_hit_quality)
        self._check(self.lib.sx_sam_layout_dev_mapq(self.h, C.byref(b), _ptr(d_byte_offsets), C.byref(total)), "sx_sam_layout_dev_mapq")
        return int(total.value)

    def sam_emit_dev_mapq(self, batch, d_hit_quality, d_byte_offsets, total_bytes, byte_lo, byte_hi, d_out):
        """sx_sam_emit_dev_mapq: bytes [byte_lo, byte_hi) of that text into d_out (uint8, 16-byte aligned)"""
        b = self._mapq_batch(batch, d_hit_quality)
        self._check(self.lib.sx_sam_emit_dev_mapq(self.h, C.byref(b), _ptr(d_byte_offsets), total_bytes, byte_lo, byte_hi, _ptr(d_out)),
                    "sx_sam_emit_dev_mapq")

    def sam_layout_dev_pairs(self, batch, d_lines, n_lines, d_byte_offsets):
        """sx_sam_layout_dev_pairs: d_lines (n_lines entries of _lib.PAIR_LINE_DTYPE in device memory) over the hits, reads
        and records of a plain sam_batch; d_byte_offsets (n_lines + 1 uint64) <- every line's first byte; returns the
        text's length"""
        total = C.c_uint64(0)
        self._check(self.lib.sx_sam_layout_dev_pairs(self.h, C.byref(batch), _ptr(d_lines), n_lines, _ptr(d_byte_offsets), C.byref(total)),
                    "sx_sam_layout_dev_pairs")
        return int(total.value)

    def sam_emit_dev_pairs(self, batch, d_lines, n_lines, d_byte_offsets, total_bytes, byte_lo, byte_hi, d_out):
        """sx_sam_emit_dev_pairs: bytes [byte_lo, byte_hi) of the described lines' text into d_out (uint8, 16-byte aligned)"""
        self._check(self.lib.sx_sam_emit_dev_pairs(self.h, C.byref(batch), _ptr(d_lines), n_lines, _ptr(d_byte_offsets), total_bytes, byte_lo,
                                                   byte_hi, _ptr(d_out)), "sx_sam_emit_dev_pairs")

    def fastq_index(self, data):
        """sx_fastq_index of the bytes of a FASTQ file: (names, name_off, seqs, seq_off, quals, qual_off) as numpy arrays
        (uint8 bytes, uint32 offsets of count + 1 entries); raises StralgAmdError (code SX_E_MALFORMED = -4) outside the
        contract (include/stralg_amd.h)."""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        fq = _lib.Fastq()
        rc = self.lib.sx_fastq_index(_ptr(buf) if buf.size else None, buf.size, C.byref(fq))
        if rc != 0:
            raise StralgAmdError(f"sx_fastq_index failed with code {rc}")
        try:
            n = int(fq.count)
            out = []
            for data_p, off_p in ((fq.names, fq.name_off), (fq.seqs, fq.seq_off), (fq.quals, fq.qual_off)):
                off = np.ctypeslib.as_array(C.cast(off_p, C.POINTER(C.c_uint32)), (n + 1,)).copy()
                nbytes = int(off[n])
                out.append(np.ctypeslib.as_array(C.cast(data_p, C.POINTER(C.c_uint8)), (nbytes,)).copy() if nbytes
                           else np.zeros(0, np.uint8))
                out.append(off)
            return tuple(out)
        finally:
            self.lib.sx_fastq_free(C.byref(fq))

    def download(self, address, count, dtype=np.uint8):
        """sx_download: `count` entries of `dtype` of device memory at a raw address, as a numpy array"""
        out = np.empty(int(count), dtype=dtype)
        if out.size:
            self._check(self.lib.sx_download(self.h, _ptr(out), int(address), out.nbytes), "sx_download")
        return out

    def fastq_index_dev(self, d_image, length):
        """sx_fastq_index_dev of a FASTQ image in device memory (a tensor, an array the device can read, or an address):
        ((names, name_off, seqs, seq_off, quals, qual_off), count) -- the six device arrays, read back as numpy arrays as
        Context.fastq_index returns the host function's; raises StralgAmdError with the host function's code outside
        the contract."""
        fq = _lib.FastqDev()
        self._check(self.lib.sx_fastq_index_dev(self.h, _ptr(d_image) if length else None, int(length), C.byref(fq)),
                    "sx_fastq_index_dev")
        try:
            return self._fastq_dev_arrays(fq), int(fq.count)
        finally:
            self.lib.sx_fastq_dev_free(C.byref(fq))

    def _fastq_dev_arrays(self, fq, spare=0):
        """the six arrays of an sx_fastq_dev read back; spare: so many bytes behind each byte array come with it"""
        n = int(fq.count)
        out = []
        for data_p, off_p, nbytes in ((fq.d_names, fq.d_name_off, fq.name_bytes), (fq.d_seqs, fq.d_seq_off, fq.seq_bytes),
                                      (fq.d_quals, fq.d_qual_off, fq.qual_bytes)):
            out.append(self.download(data_p, nbytes + spare, np.uint8))
            out.append(self.download(off_p, n + 1, np.uint32))
        return tuple(out)

    def fastq_strands_dev(self, d_image, length, d_flags, spare=0):
        """sx_fastq_index_dev of a FASTQ image in device memory, then sx_fastq_strands_dev of its arrays:
        ((names, name_off, seqs, seq_off, quals, qual_off), flags, count) of the read set of both strands (read 2q is read q,
        read 2q + 1 its reverse complement), read back as numpy arrays as fastq_index_dev returns them.  d_flags: device
        memory of the caller for the flags, uint16, twice as many entries as the image has reads at least (length // 4
        entries are enough for any image); flags: its first `count` entries read back, 0 and 16.  spare: so many of the readable bytes
        behind each byte array are read back with it (the contract promises 16)."""
        fq, both = _lib.FastqDev(), _lib.FastqDev()
        self._check(self.lib.sx_fastq_index_dev(self.h, _ptr(d_image) if length else None, int(length), C.byref(fq)),
                    "sx_fastq_index_dev")
        try:
            room = d_flags.numel() * d_flags.element_size() if hasattr(d_flags, "numel") else d_flags.nbytes
            if room < 4 * int(fq.count):
                raise ValueError(f"d_flags has {room} bytes, the image's {int(fq.count)} reads take four each")
            self._check(self.lib.sx_fastq_strands_dev(self.h, C.byref(fq), C.byref(both), _ptr(d_flags)), "sx_fastq_strands_dev")
            try:
                flags = self.download(_ptr(d_flags), int(both.count), np.uint16)
                return self._fastq_dev_arrays(both, spare), flags, int(both.count)
            finally:
                self.lib.sx_fastq_dev_free(C.byref(both))
        finally:
            self.lib.sx_fastq_dev_free(C.byref(fq))

    def set_sam_batch_reads(self, reads):
        """sx_map_reads_stream: at most this many reads in one search batch (0: the default)"""
        self._check(self.lib.sx_ctx_set_flag(self.h, _lib.SX_FLAG_SAM_BATCH_READS, int(reads)), "sx_ctx_set_flag")

    def set_sam_window_bytes(self, nbytes):
        """sx_map_reads_stream: bytes of SAM text per window (0: the default, 32 MiB)"""
        self._check(self.lib.sx_ctx_set_flag(self.h, _lib.SX_FLAG_SAM_WINDOW_BYTES, int(nbytes)), "sx_ctx_set_flag")

    def set_locate_chunk_rows(self, rows):
        """mapping against an index with a sampled suffix array: the hits of a batch are located and printed in runs whose
        lines fit this many positions (0: the default, 2^28)"""
        self._check(self.lib.sx_ctx_set_flag(self.h, _lib.SX_FLAG_LOCATE_CHUNK_ROWS, int(rows)), "sx_ctx_set_flag")

    def set_sam_room_hits(self, hits):
        """read mapping, a test switch: the largest room for the hits of a batch's searches, in place of what the free memory
        gives, and a first room as small as 1 hit (0: the default, by the free memory).  Small values make the room grow and
        the batches halve on small inputs; map_stats() says what happened"""
        self._check(self.lib.sx_ctx_set_flag(self.h, _lib.SX_FLAG_SAM_ROOM_HITS, int(hits)), "sx_ctx_set_flag")

    def set_pairs_room_lines(self, lines):
        """paired reads, a test switch: the lines, and the line descriptors, that a batch of several pairs may have before it
        is halved, in place of what the free memory gives; the hits' room stays (0: the default; set_sam_room_hits sets it
        too where this is 0)"""
        self._check(self.lib.sx_ctx_set_flag(self.h, _lib.SX_FLAG_PAIRS_ROOM_LINES, int(lines)), "sx_ctx_set_flag")

    def map_stats(self):
        """sx_map_last_stats: what the loop of the last mapping call on this context did with its batches, as a dict (batches,
        retries, room_grown, lone_grown, halved, room_first, room_final, batch_first, batch_final)"""
        st = _lib.MapStats()
        self._check(self.lib.sx_map_last_stats(self.h, C.byref(st)), "sx_map_last_stats")
        return st.as_dict()

    # ---- the sampled suffix array (sx_locate.hpp) -----------------------------------------------
    def sa_sample_bytes(self, N, sa_sample):
        """sx_sa_sample_bytes: (bytes of the marks, bytes of the values) of a record of N rows sampled at this distance"""
        marks, values = C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.sx_sa_sample_bytes(N, int(sa_sample).bit_length() - 1, C.byref(marks), C.byref(values)), "sx_sa_sample_bytes")
        return int(marks.value), int(values.value)

    def sa_sample_build_dev(self, d_sa, N, sa_sample, d_marks, d_values):
        self._check(self.lib.sx_sa_sample_build_dev(self.h, _ptr(d_sa), N, int(sa_sample).bit_length() - 1, _ptr(d_marks), _ptr(d_values)),
                    "sx_sa_sample_build_dev")

    def sa_locate_rows_dev(self, d_c, d_occ, N, sigma, d_marks, d_values, sa_sample, row_lo, row_hi, d_out):
        self._check(self.lib.sx_sa_locate_rows_dev(self.h, _ptr(d_c), _ptr(d_occ), N, sigma, _ptr(d_marks), _ptr(d_values),
                                                   int(sa_sample).bit_length() - 1, row_lo, row_hi, _ptr(d_out)), "sx_sa_locate_rows_dev")

    def map_reads_stream(self, records, fastq, edits, sink, both_strands=False, best=False, indels=True, tags=False, unmapped=False,
                         header=False, mapq=False):
        """sx_map_reads_stream: records = [(name bytes, BwtTable), ...] in the mapper's list order; sink(bytes) receives the
        SAM text window after window.  sink=None discards the text without touching it and returns [(time.perf_counter(),
        bytes)] per window (measurement).  both_strands (sx_map_reads_stream_ex, SX_MAP_BOTH_STRANDS): behind the lines of
        every read come those of its reverse complement, with FLAG 16.  best (SX_MAP_BEST_STRATUM): per read only the
        lines of the smallest edit count in 0 .. edits that has any (with both_strands: over both strands together).
        indels=False (SX_MAP_NO_INDELS): mismatches only -- the lines whose CIGAR is "<length of SEQ>M", each placement
        once; with best the strata are the smallest number of mismatches.  tags (SX_MAP_TAGS) asks for NM:i and MD:Z, which
        need the records' strings on the device: records of tables alone have none and the call raises StralgAmdError
        (code SX_E_ARG = -1) before anything runs; map through an Index (Index.from_fasta) instead.  unmapped
        (SX_MAP_UNMAPPED): every read (with both_strands: read and reverse complement) that prints no line gets one FLAG 4
        line "<name>\t4\t*\t0\t0\t*\t*\t0\t0\t<seq>\t<qual>" where its lines would stand.  header (SX_MAP_HEADER): the @HD
        line and an @SQ line per record in front of the text.  mapq (SX_MAP_MAPQ, needs best; else StralgAmdError, code SX_E_ARG = -1): per read (with both_strands: read and reverse
        complement) the first line keeps its FLAG and every other one has 256 added; MAPQ on all of them is 50, 3, 1 or 0 for
        1, 2, 3 to 4 or more lines of the read.  The count is of lines, so indels=False is what to combine it with."""
        recs = (_lib.MapRecord * max(1, len(records)))()
        keep = []
        for r, (name, t) in enumerate(records):
            recs[r] = _map_record(name, t, keep)
        buf = np.frombuffer(bytes(fastq), dtype=np.uint8)
        failure = []

        seen = []

        def _sink(user, section, data, nbytes):
            try:
                if sink is None:
                    seen.append((time.perf_counter(), nbytes))
                else:
                    sink(C.string_at(data, nbytes))
                return 0
            except Exception as e:  # (an exception must not cross the C frames)
                failure.append(e)
                return 1

        cb = _lib.SINK_FN(_sink)
        flags = _lib.map_flags(both_strands, best, indels, tags, unmapped, header, mapq)
        if flags:
            rc = self.lib.sx_map_reads_stream_ex(self.h, recs, len(records), _ptr(buf) if buf.size else None, buf.size, edits,
                                                 flags, cb, None)
        else:
            rc = self.lib.sx_map_reads_stream(self.h, recs, len(records), _ptr(buf) if buf.size else None, buf.size, edits, cb, None)
        if failure:
            raise failure[0]
        self._check(rc, "sx_map_reads_stream_ex" if flags else "sx_map_reads_stream")
        return seen if sink is None else None

    # ---- FASTA ingest and remap ------------------------------
    def fasta_pack_dev(self, d_file, file_len, d_packed, d_term=None, term_cap=0):
        """bioinf/fasta.c load_fasta_records' packing on the device: returns (packed_len, n_records); raises
        StralgAmdError (code SX_E_MALFORMED = -4) where the reference reports MALFORMED_FILE."""
        plen, nrec = C.c_uint64(0), C.c_uint32(0)
        self._check(self.lib.sx_fasta_pack_dev(self.h, _ptr(d_file), file_len, _ptr(d_packed), C.byref(plen), _ptr(d_term),
                                               term_cap, C.byref(nrec)), "sx_fasta_pack_dev")
        return int(plen.value), int(nrec.value)

    def remap_dev(self, d_in, n, d_out):
        """stralg/remap.c on the device: d_out[0..n) dense codes, d_out[n] = 0; returns (alphabet_size, table[256])."""
        table = np.zeros(256, dtype=np.int16)
        sigma = C.c_uint32(0)
        self._check(self.lib.sx_remap_dev(self.h, _ptr(d_in), n, _ptr(d_out), table.ctypes.data_as(C.POINTER(C.c_int16)),
                                          C.byref(sigma)), "sx_remap_dev")
        return int(sigma.value), table

    def reverse_dev(self, d_in, n, d_out):
        """sx_reverse_dev: d_out[0..n) = d_in reversed, d_out[n] = 0 (the string build_complete_table sorts for RO, bwt.c:147-151)"""
        self._check(self.lib.sx_reverse_dev(self.h, _ptr(d_in), n, _ptr(d_out)), "sx_reverse_dev")

    def fasta_records(self, data):
        """sx_fasta_pack (host buffers): [(name, sequence), ...] in file order from the bytes of a FASTA file"""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        packed = np.zeros(buf.size + 1, dtype=np.uint8)
        term = np.zeros(buf.size + 2, dtype=np.uint32)
        plen, nrec = C.c_uint64(0), C.c_uint32(0)
        self._check(self.lib.sx_fasta_pack(self.h, _ptr(buf) if buf.size else None, buf.size, _ptr(packed), C.byref(plen),
                                           _ptr(term), term.size, C.byref(nrec)), "sx_fasta_pack")
        out = []
        for r in range(nrec.value):
            n0 = 0 if r == 0 else int(term[2 * r - 1]) + 1
            s0 = int(term[2 * r]) + 1
            out.append((packed[n0:int(term[2 * r])].tobytes(), packed[s0:int(term[2 * r + 1])].tobytes()))
        return out

    # ---- primitives (kernel-level tests) ------------------------------------------
    def prim_sort_pairs_dev(self, ka, va, kb, vb, n, begin_bit, end_bit):
        flag = C.c_int(0)
        self._check(self.lib.sx_prim_sort_pairs_dev(self.h, _ptr(ka), _ptr(va), _ptr(kb), _ptr(vb), n, begin_bit,
                                                    end_bit, C.byref(flag)), "sx_prim_sort_pairs_dev")
        return bool(flag.value)

    def prim_exclusive_sum_dev(self, d_in, d_out, n, d_total=None):
        self._check(self.lib.sx_prim_exclusive_sum_dev(self.h, _ptr(d_in), _ptr(d_out), n, _ptr(d_total)),
                    "sx_prim_exclusive_sum_dev")

    def prim_classify_dev(self, d_text, n, d_flags, d_hist_all, d_hist_l, d_hist_lms):
        self._check(self.lib.sx_prim_classify_dev(self.h, _ptr(d_text), n, _ptr(d_flags), _ptr(d_hist_all),
                                                  _ptr(d_hist_l), _ptr(d_hist_lms)), "sx_prim_classify_dev")

    # ---- measurement -----------------------------------------------------------------
    def profile_only(self, kclass_name=None):
        """events only around launches of one kernel class (None: all classes)"""
        k = -1 if kclass_name is None else _lib.KC_NAMES.index(kclass_name)
        self._check(self.lib.sx_profile_only(self.h, k), "sx_profile_only")

    def profile_enable(self, on=True):
        self._check(self.lib.sx_profile_enable(self.h, 1 if on else 0), "sx_profile_enable")

    def profile_reset(self):
        self._check(self.lib.sx_profile_reset(self.h), "sx_profile_reset")

    def profile_read(self):
        arr = (_lib.KernelStat * len(_lib.KC_NAMES))()
        self._check(self.lib.sx_profile_read(self.h, arr), "sx_profile_read")
        return {name: {"launches": int(arr[i].launches), "ms": float(arr[i].ms), "alg_bytes": int(arr[i].alg_bytes)}
                for i, name in enumerate(_lib.KC_NAMES)}

    def last_stats(self):
        st = _lib.BuildStats()
        self._check(self.lib.sx_last_stats(self.h, C.byref(st)), "sx_last_stats")
        return st.as_dict()

    def force_general_path(self, on=True):
        """SX_FLAG_FORCE_GENERAL_PATH: pieces + names + prefix doubling even where the prefix-key sort would do."""
        self._check(self.lib.sx_ctx_set_flag(self.h, 1, 1 if on else 0), "sx_ctx_set_flag")

    def set_chain_max_entries(self, entries):
        """SX_FLAG_CHAIN_MAX_ENTRIES: longer induce rounds take the count / offsets / scatter launches."""
        self._check(self.lib.sx_ctx_set_flag(self.h, 2, int(entries)), "sx_ctx_set_flag")

    def set_no_direct_sort(self, on=True):
        """SX_FLAG_NO_DIRECT_SORT: wide alphabets take the LMS sort + induction even where the direct sort applies."""
        self._check(self.lib.sx_ctx_set_flag(self.h, 3, 1 if on else 0), "sx_ctx_set_flag")

    def set_prefix_symbols(self, symbols):
        """SX_FLAG_PREFIX_SYMBOLS: the prefix-key sort's first attempt takes this many symbols (0: by the size)."""
        self._check(self.lib.sx_ctx_set_flag(self.h, 4, int(symbols)), "sx_ctx_set_flag")

    def set_radix_digit_bits(self, bits):
        """SX_FLAG_RADIX_DIGIT_BITS: digit width of the LSD radix passes (8, 9, 10; 0: default)."""
        self._check(self.lib.sx_ctx_set_flag(self.h, 5, int(bits)), "sx_ctx_set_flag")

    def set_sort_mode(self, mode):
        """SX_FLAG_SORT_MODE: 0 choose, 1 LSD passes only, 2 hybrid sort wherever the key shape allows it (HBM passes on
        the top 24 key bits), 3 the same with the top 32 bits."""
        self._check(self.lib.sx_ctx_set_flag(self.h, 6, int(mode)), "sx_ctx_set_flag")

    def set_induce_batch(self, on=True):
        """SX_FLAG_INDUCE_BATCH_OFF: the self rounds of a bucket eight at a time (default) or a launch each"""
        self._check(self.lib.sx_ctx_set_flag(self.h, 7, 0 if on else 1), "sx_ctx_set_flag")

    def set_induce_batch_min(self, entries):
        """SX_FLAG_INDUCE_BATCH_MIN: ranges longer than this take the eight-rounds-at-a-time form (negative: default)"""
        self._check(self.lib.sx_ctx_set_flag(self.h, 8, int(entries)), "sx_ctx_set_flag")

    def set_induce_attended(self, mode=1):
        """SX_FLAG_INDUCE_ATTENDED: 0 default (buckets queued one behind the other, a bucket the tail kernel could not
        finish is carried on by the host), 1 the host looks at every bucket's last range"""
        self._check(self.lib.sx_ctx_set_flag(self.h, 9, int(mode)), "sx_ctx_set_flag")

    def set_induce_early_s(self, on=True):
        """SX_FLAG_INDUCE_EARLY_S_OFF: texts of at most 8 symbols -- the L pass's large rounds place the S-type predecessors of
        the entries they scan (default), or the S pass scans every L region again for them"""
        self._check(self.lib.sx_ctx_set_flag(self.h, _lib.SX_FLAG_INDUCE_EARLY_S_OFF, 0 if on else 1), "sx_ctx_set_flag")

    def set_induce_hoist(self, on=True):
        """SX_FLAG_INDUCE_NO_HOIST: texts of more than 8 symbols -- all buckets' LMS seeds / L-type entries scanned at once, up
        front, placed by the text's bigram counts (default), or by launches of each bucket's own (rounds 1 - 3)"""
        self._check(self.lib.sx_ctx_set_flag(self.h, 13, 0 if on else 1), "sx_ctx_set_flag")

    def set_text_keys(self, on=True):
        """SX_FLAG_TEXT_KEYS_OFF: the first radix pass of the direct sort, and of a four-letter text's LMS sort, computes
        its keys from the text (default) or reads them from a key kernel's output (rounds 1 - 3)"""
        self._check(self.lib.sx_ctx_set_flag(self.h, 14, 0 if on else 1), "sx_ctx_set_flag")

    def set_long_subbuckets(self, on=True):
        """SX_FLAG_LONG_SUBBUCKETS_OFF: the hybrid prefix-key sort lists sub-buckets too long for a workgroup and orders them
        by HBM passes of their own (default), or falls back to plain passes when it meets one (rounds 1 - 3)"""
        self._check(self.lib.sx_ctx_set_flag(self.h, 15, 0 if on else 1), "sx_ctx_set_flag")

    def set_local_sort_lean(self, on=True):
        """SX_FLAG_LOCAL_SORT_LEAN_OFF: the hybrid sort's LDS step by the lean kernel of round 5 (default), or every workgroup by
        the kernel of rounds 3 and 4 (the one the lean kernel leaves its crowded workgroups to)"""
        self._check(self.lib.sx_ctx_set_flag(self.h, 17, 0 if on else 1), "sx_ctx_set_flag")

    def set_small_direct_max(self, suffixes):
        """SX_FLAG_SMALL_DIRECT_MAX: texts of at most 16 symbols and at most this many suffixes are sorted directly
        (0: never; negative: default)"""
        self._check(self.lib.sx_ctx_set_flag(self.h, 16, int(suffixes)), "sx_ctx_set_flag")

    def set_recurse_min(self, symbols):
        """SX_FLAG_RECURSE_MIN: reduced strings of at most 255 names recurse from this length on (negative: default)"""
        self._check(self.lib.sx_ctx_set_flag(self.h, 11, int(symbols)), "sx_ctx_set_flag")

    def set_sample_min(self, suffixes):
        """SX_FLAG_SAMPLE_MIN: wide-alphabet texts of at least this many suffixes get the look at a sample (negative: default)"""
        self._check(self.lib.sx_ctx_set_flag(self.h, 12, int(suffixes)), "sx_ctx_set_flag")

    def set_copy_text_first(self, on=True):
        """SX_FLAG_COPY_TEXT_FIRST: a device copy of the text before the classification (True) or the copy made by the
        classification while it reads the caller's text (default)"""
        self._check(self.lib.sx_ctx_set_flag(self.h, 10, 1 if on else 0), "sx_ctx_set_flag")

    def trim(self):
        self.lib.sx_ctx_trim(self.h)

    # ---- test hooks: what the context carries from call to call ----------------------------
    def scribble(self, byte):
        """sx_ctx_scribble: every workspace slab, the staging buffers and the read-back page filled with `byte`, the look-back
        status words with ready prefixes of the last epoch and a wrong value; the child context likewise"""
        self._check(self.lib.sx_ctx_scribble(self.h, int(byte)), "sx_ctx_scribble")

    def set_chain_epoch(self, epoch):
        """SX_FLAG_CHAIN_EPOCH: the look-back epoch of the context and of its child (the next chained launch takes the next)"""
        self._check(self.lib.sx_ctx_set_flag(self.h, _lib.SX_FLAG_CHAIN_EPOCH, int(epoch)), "sx_ctx_set_flag")

    def set_readback_seq(self, seq):
        """SX_FLAG_READBACK_SEQ: the sequence number of the last read-back, as a 32-bit pattern, in the context and on its page"""
        seq = int(seq) & 0xFFFFFFFF
        self._check(self.lib.sx_ctx_set_flag(self.h, _lib.SX_FLAG_READBACK_SEQ, seq - (1 << 32) if seq >> 31 else seq), "sx_ctx_set_flag")

    def counters(self):
        """sx_ctx_counters: dict(chain_epoch, readback_seq, chain_slab_max_epoch, slab_bytes[7], has_child, child=dict of the
        same four); chain_slab_max_epoch copies the status words to the host: slow"""
        st = _lib.CtxCounts()
        self._check(self.lib.sx_ctx_counters(self.h, C.byref(st)), "sx_ctx_counters")
        return st.as_dict()

    def bind_to_numa_node(self):
        """pin the calling thread (and the threads it starts later) to the CPUs next to this context's GPU
        (stralg_amd_bind_thread_to_device); returns the NUMA node, or -1 when the box does not tell"""
        self.lib.stralg_amd_bind_thread_to_device.argtypes = [C.c_int]
        self.lib.stralg_amd_bind_thread_to_device.restype = C.c_int
        return int(self.lib.stralg_amd_bind_thread_to_device(self.device))


def _map_record(name, t, keep):
    """(name bytes, BwtTable) -> _lib.MapRecord over arrays that `keep` holds alive"""
    sa = np.ascontiguousarray(t.sa.array, dtype=np.uint32)
    c = np.ascontiguousarray(t.c_table, dtype=np.uint32)
    o = np.ascontiguousarray(t.o_table, dtype=np.uint32)
    ro = None if t.ro_table is None else np.ascontiguousarray(t.ro_table, dtype=np.uint32)
    tab = np.ascontiguousarray(np.clip(t.remap_table.table, -1, 127), dtype=np.int8)
    keep.append((sa, c, o, ro, tab))
    return _lib.MapRecord(bytes(name), _ptr(sa), _ptr(c), _ptr(o), _ptr(ro), sa.size, t.remap_table.alphabet_size, _ptr(tab))


class Index:
    """A device-resident index (sx_index): every FASTA record's remapped string, SA, C, O and RO stay on the GPU, in
    allocations of the index's own; build it once, map many read sets.  Use one index from one thread at a time, with
    contexts on its device."""

    def __init__(self, ctx, handle):
        self.ctx = ctx
        self.h = handle

    # ---- constructors -------------------------------------------------------------------------------------------
    @classmethod
    def from_fasta(cls, fasta_bytes, include_reverse=True, ctx=None, compact=False, sa_sample=0, packed=False):
        """sx_index_build_fasta_ex: the bytes of a FASTA file -> tables of every record, built on the device; compact=True:
        BWT blocks with sampled counts in place of the O / RO tables (a fifth of the memory for DNA, the same results);
        sa_sample=32 (a power of two in 2 .. 1024, with compact): SA values at that distance in place of the suffix array,
        the others located by walks over the blocks (5.4 bytes a symbol in place of 9 for DNA, the same results);
        packed=True (with compact): a nibble a row in the blocks, for records of at most 7 letters (7 bytes a symbol in
        place of 9 for DNA, 3.4 in place of 5.4 with sa_sample=32, the same results; a record of more letters fails the build)"""
        flags = _lib.index_flags(compact, sa_sample, packed)
        ctx = ctx or default_context()
        buf = np.frombuffer(bytes(fasta_bytes), dtype=np.uint8)
        h = C.c_void_p()
        ctx._check(ctx.lib.sx_index_build_fasta_ex(ctx.h, _ptr(buf) if buf.size else None, buf.size, 1 if include_reverse else 0,
                                                   flags, C.byref(h)), "sx_index_build_fasta")
        return cls(ctx, h)

    @classmethod
    def from_tables(cls, records, ctx=None, compact=False, sa_sample=0, packed=False):
        """sx_index_from_sources_ex: records = [(name bytes, BwtTable), ...] in the mapper's list order (the FASTA file's), as
        Context.map_reads_stream takes them; a table whose sa.string is set (remapped symbols + terminator) can be saved.
        compact=True: the tables go up in windows and stay as blocks; sa_sample: as from_fasta (the suffix arrays go up in
        windows too and stay as samples); packed: as from_fasta"""
        flags = _lib.index_flags(compact, sa_sample, packed)
        ctx = ctx or default_context()
        src = (_lib.IndexSource * max(1, len(records)))()
        keep = []
        for r, (name, t) in enumerate(records):
            src[r].record = _map_record(name, t, keep)
            string = getattr(t.sa, "string", None)
            if string is not None:
                string = np.ascontiguousarray(string, dtype=np.uint8)
                keep.append(string)
                src[r].string = _ptr(string)
        h = C.c_void_p()
        ctx._check(ctx.lib.sx_index_from_sources_ex(ctx.h, src, len(records), flags, C.byref(h)),
                   "sx_index_from_sources")
        return cls(ctx, h)

    @classmethod
    def load(cls, path_or_bytes, ctx=None, compact=False, sa_sample=0, packed=False):
        """the read mapper's index file (genome.fa.bwttables; what .save writes): a path, or the bytes.  The file is
        mapped, and its records go to the device one after the other (compact=True: as blocks; sa_sample and packed: as
        from_fasta)."""
        flags = _lib.index_flags(compact, sa_sample, packed)
        ctx = ctx or default_context()
        if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
            blob = np.frombuffer(bytes(path_or_bytes), dtype=np.uint8)
        else:
            blob = np.memmap(path_or_bytes, dtype=np.uint8, mode="r")
        at = [0]

        def take(nbytes, dtype=np.uint8):
            if at[0] + nbytes > blob.size:
                raise StralgAmdError("Index.load: truncated index")
            out = np.frombuffer(np.ascontiguousarray(blob[at[0]:at[0] + nbytes]).tobytes(), dtype=dtype)
            at[0] += nbytes
            return out

        h = C.c_void_p()
        ctx._check(ctx.lib.sx_index_from_sources_ex(ctx.h, None, 0, flags, C.byref(h)),
                   "sx_index_from_sources")
        idx = cls(ctx, h)
        try:
            n_rec = int(take(4, np.uint32)[0])
            for _ in range(n_rec):  # (last FASTA record first)
                name = take(int(take(4, np.uint32)[0])).tobytes()
                if not name or name[-1] != 0:
                    raise StralgAmdError("Index.load: a record's name lacks its terminator")
                n = int(take(4, np.uint32)[0])
                string = np.concatenate([take(n), np.zeros(1, np.uint8)])
                sa = take(4 * (n + 1), np.uint32)
                sigma = int(take(4, np.uint32)[0])
                table, _rev = take(256, np.int8), take(128, np.int8)
                if not 1 <= sigma <= 128:
                    raise StralgAmdError("Index.load: a remap table of more than 127 letters")
                c = take(4 * sigma, np.uint32)
                o = take(4 * sigma * (n + 2), np.uint32)
                ro = take(4 * sigma * (n + 2), np.uint32) if int(take(1)[0]) else None
                src = _lib.IndexSource(_lib.MapRecord(name[:-1], _ptr(sa), _ptr(c), _ptr(o), _ptr(ro), n + 1, sigma, _ptr(table)),
                                       _ptr(string))
                ctx._check(ctx.lib.sx_index_add_record(ctx.h, idx.h, C.byref(src), 1), "sx_index_add_record")
        except Exception:
            idx.close()
            raise
        return idx

    # ---- use ----------------------------------------------------------------------------------------------------
    def _handle(self):
        if not self.h:
            raise StralgAmdError("the index is closed")
        return self.h

    def map_reads(self, fastq, edits, sink=None, ctx=None, both_strands=False, best=False, indels=True, tags=False, unmapped=False,
                  header=False, mapq=False):
        """sx_index_map_reads: the SAM text of every match of every read of a FASTQ image within `edits` edits, byte for
        byte stralg_amd.map_reads' (the reference mapper's stdout).  sink=None returns the text; sink(bytes) receives it
        window after window and None is returned.  both_strands, best, indels, tags: as in stralg_amd.map_reads
        (sx_index_map_reads_ex); tags needs every record's string in the index (an index from_tables without strings
        raises StralgAmdError, code SX_E_ARG = -1).  unmapped, header, mapq: as in stralg_amd.map_reads."""
        ctx = ctx or self.ctx
        buf = np.frombuffer(bytes(fastq), dtype=np.uint8)
        chunks, failure = [], []
        put = chunks.append if sink is None else sink

        def _sink(user, section, data, nbytes):
            try:
                put(C.string_at(data, nbytes))
                return 0
            except Exception as e:  # (an exception must not cross the C frames)
                failure.append(e)
                return 1

        cb = _lib.SINK_FN(_sink)
        flags = _lib.map_flags(both_strands, best, indels, tags, unmapped, header, mapq)
        rc = self._map(ctx, buf, edits, flags, cb)
        if failure:
            raise failure[0]
        ctx._check(rc, "sx_index_map_reads_ex" if flags else "sx_index_map_reads")
        return b"".join(chunks) if sink is None else None

    def _map(self, ctx, buf, edits, flags, cb):
        """the return code of sx_index_map_reads, or of sx_index_map_reads_ex with a flags word that is not 0"""
        image = _ptr(buf) if buf.size else None
        if flags:
            return ctx.lib.sx_index_map_reads_ex(ctx.h, self._handle(), image, buf.size, edits, flags, cb, None)
        return ctx.lib.sx_index_map_reads(ctx.h, self._handle(), image, buf.size, edits, cb, None)

    def map_reads_discard(self, fastq, edits, ctx=None, both_strands=False, best=False, indels=True, tags=False, unmapped=False,
                          header=False, mapq=False):
        """the same with a sink that does not touch the text: [(time.perf_counter(), bytes)] per window (measurement)"""
        ctx = ctx or self.ctx
        buf = np.frombuffer(bytes(fastq), dtype=np.uint8)
        seen = []

        def _sink(user, section, data, nbytes):
            seen.append((time.perf_counter(), nbytes))
            return 0

        cb = _lib.SINK_FN(_sink)
        flags = _lib.map_flags(both_strands, best, indels, tags, unmapped, header, mapq)
        ctx._check(self._map(ctx, buf, edits, flags, cb), "sx_index_map_reads_ex" if flags else "sx_index_map_reads")
        return seen

    def _map_pairs(self, ctx, fastq1, fastq2, edits, min_insert, max_insert, flags, cb):
        """the return code of sx_index_map_pairs"""
        b1, b2 = (np.frombuffer(bytes(f), dtype=np.uint8) for f in (fastq1, fastq2))
        opts = _lib.PairOpts(min_insert, max_insert)
        return ctx.lib.sx_index_map_pairs(ctx.h, self._handle(), _ptr(b1) if b1.size else None, b1.size, _ptr(b2) if b2.size else None,
                                          b2.size, edits, C.byref(opts), flags, cb, None)

    def map_pairs(self, fastq1, fastq2, edits, min_insert=0, max_insert=1000, sink=None, best=False, indels=True, ctx=None, header=False):
        """sx_index_map_pairs: paired-end reads.  Read p of fastq1 and read p of fastq2 are the mates of pair p; the text
        is, per pair in file order, the two lines of every proper combination of a line of mate 1 and a line of mate 2
        (lines as map_reads(both_strands=True) prints them at the same edits, best and indels): same record, one on
        either strand, the forward one not behind the reverse one at either end, and min_insert <= t <= max_insert for
        t = the reverse line's end - the forward line's POS.  FLAG is 99 / 147 or 83 / 163, RNEXT "=", PNEXT the other
        line's POS, TLEN t or -t.  A pair without a proper combination prints nothing.  The search reports some
        placements more than once (1I99M beside 100M) and such lines multiply: best=True and indels=False are what
        this is meant to be combined with.  sink=None returns the text; sink(bytes) receives it window after window.
        header (SX_MAP_HEADER): the @HD line and an @SQ line per record in front of the text."""
        ctx = ctx or self.ctx
        chunks, failure = [], []
        put = chunks.append if sink is None else sink

        def _sink(user, section, data, nbytes):
            try:
                put(C.string_at(data, nbytes))
                return 0
            except Exception as e:  # (an exception must not cross the C frames)
                failure.append(e)
                return 1

        rc = self._map_pairs(ctx, fastq1, fastq2, edits, min_insert, max_insert, _lib.pair_flags(best, indels, header), _lib.SINK_FN(_sink))
        if failure:
            raise failure[0]
        ctx._check(rc, "sx_index_map_pairs")
        return b"".join(chunks) if sink is None else None

    def map_pairs_discard(self, fastq1, fastq2, edits, min_insert=0, max_insert=1000, best=False, indels=True, ctx=None, header=False):
        """the same with a sink that does not touch the text: [(time.perf_counter(), bytes)] per window (measurement)"""
        ctx = ctx or self.ctx
        seen = []

        def _sink(user, section, data, nbytes):
            seen.append((time.perf_counter(), nbytes))
            return 0

        ctx._check(self._map_pairs(ctx, fastq1, fastq2, edits, min_insert, max_insert, _lib.pair_flags(best, indels, header), _lib.SINK_FN(_sink)),
                   "sx_index_map_pairs")
        return seen

    def write(self, sink, ctx=None):
        """sx_index_write: the index file's bytes, chunk after chunk, to sink(bytes)"""
        ctx = ctx or self.ctx
        failure = []

        def _sink(user, section, data, nbytes):
            try:
                sink(C.string_at(data, nbytes))
                return 0
            except Exception as e:
                failure.append(e)
                return 1

        cb = _lib.SINK_FN(_sink)
        rc = ctx.lib.sx_index_write(ctx.h, self._handle(), cb, None)
        if failure:
            raise failure[0]
        ctx._check(rc, "sx_index_write")

    def save(self, path):
        """the read mapper's index file (what `stralg_amd_readmapper -p` writes), from the resident buffers"""
        with open(path, "wb") as f:
            self.write(f.write)

    def _info(self):
        n, dev, ro, nbytes = C.c_uint32(0), C.c_int(0), C.c_int(0), C.c_uint64(0)
        self.ctx._check(self.ctx.lib.sx_index_info(self._handle(), C.byref(n), C.byref(dev), C.byref(ro), C.byref(nbytes)),
                        "sx_index_info")
        return int(n.value), int(dev.value), bool(ro.value), int(nbytes.value)

    def record_info(self, r):
        """sx_index_record_info of record r: the _lib.IndexRecord with the record's device addresses (for tests)"""
        rec = _lib.IndexRecord()
        self.ctx._check(self.ctx.lib.sx_index_record_info(self._handle(), r, C.byref(rec)), "sx_index_record_info")
        return rec

    @property
    def records(self):
        """[(name, N, sigma, has_ro)] in FASTA file order"""
        out = []
        for r in range(self._info()[0]):
            rec = self.record_info(r)
            out.append((bytes(rec.name), int(rec.N), int(rec.sigma), bool(rec.has_ro)))
        return out

    @property
    def device(self):
        return self._info()[1]

    @property
    def device_bytes(self):
        return self._info()[3]

    def device_tables(self, r, ctx=None):
        """record r's device buffers read back (tests): dict(string, sa, c, o, ro) of numpy arrays; ro / string may be None
        (and o, in a compact index: see device_occ and expand_o; and sa, in a sampled one: see device_samples and expand_sa)"""
        ctx = ctx or self.ctx
        rec = self.record_info(r)
        N, sigma = int(rec.N), int(rec.sigma)
        return dict(string=ctx.download(rec.d_string, N, np.uint8) if rec.d_string else None,
                    sa=ctx.download(rec.d_sa, N, np.uint32) if rec.d_sa else None, c=ctx.download(rec.d_c, sigma, np.uint32),
                    o=ctx.download(rec.d_o, (N + 1) * sigma, np.uint32).reshape(N + 1, sigma) if rec.d_o else None,
                    ro=ctx.download(rec.d_ro, (N + 1) * sigma, np.uint32).reshape(N + 1, sigma) if rec.d_ro else None)

    def record_occ(self, r):
        """sx_index_record_occ of record r: the _lib.IndexOcc with the addresses and the shape of the record's blocks"""
        occ = _lib.IndexOcc()
        self.ctx._check(self.ctx.lib.sx_index_record_occ(self._handle(), r, C.byref(occ)), "sx_index_record_occ")
        return occ

    @property
    def compact(self):
        """whether the records keep BWT blocks with sampled counts in place of the O / RO tables"""
        return bool(self.ctx.lib.sx_index_is_compact(self._handle()))

    @property
    def packed(self):
        """whether the records' blocks keep a nibble a row (the packed form of a compact index)"""
        return bool(self.ctx.lib.sx_index_is_packed(self._handle()))

    def _occ_address(self, r, reverse):
        occ = self.record_occ(r)
        if not occ.compact:
            raise StralgAmdError("the index keeps full tables: it has no blocks")
        address = occ.d_rocc if reverse else occ.d_occ
        if not address:
            raise StralgAmdError("the record was built without the reverse")
        return occ, address

    def device_occ(self, r, reverse=False, ctx=None):
        """record r's raw blocks (of RO with reverse=True) read back: a uint8 array of n_blocks x stride (x 64 in a packed index)"""
        ctx = ctx or self.ctx
        occ, address = self._occ_address(r, reverse)
        return ctx.download(address, int(occ.n_blocks) * int(occ.stride), np.uint8).reshape(int(occ.n_blocks), int(occ.stride))

    def expand_o(self, r, reverse=False, rows=None, ctx=None):
        """sx_index_expand_o: the (N + 1, sigma) O table of record r (RO with reverse=True) from its blocks, through the
        expand kernel; rows=(lo, hi): only the rows [lo, hi)"""
        ctx = ctx or self.ctx
        rec = self.record_info(r)
        N, sigma = int(rec.N), int(rec.sigma)
        lo, hi = (0, N + 1) if rows is None else rows
        out = np.zeros((max(0, hi - lo), sigma), dtype=np.uint32)
        ctx._check(ctx.lib.sx_index_expand_o(ctx.h, self._handle(), r, 1 if reverse else 0, lo, hi, _ptr(out)), "sx_index_expand_o")
        return out

    def record_samples(self, r):
        """sx_index_record_samples of record r: the _lib.IndexSamples with the addresses of the record's marks and values,
        the log2 of its sampling distance, its samples and its blocks (all 0 for a record with its whole suffix array)"""
        smp = _lib.IndexSamples()
        self.ctx._check(self.ctx.lib.sx_index_record_samples(self._handle(), r, C.byref(smp)), "sx_index_record_samples")
        return smp

    @property
    def sa_sample(self):
        """the sampling distance of the records' suffix arrays, 0 when they are kept whole"""
        if self._info()[0] == 0:
            return 0
        q = int(self.record_samples(0).sa_log2)
        return 1 << q if q else 0

    def device_samples(self, r, ctx=None):
        """record r's marks, a (blocks, 2) uint64 array of (bits, before), and values read back"""
        ctx = ctx or self.ctx
        smp = self.record_samples(r)
        if not smp.sa_log2:
            raise StralgAmdError("the index keeps whole suffix arrays: it has no samples")
        return (ctx.download(smp.d_marks, 2 * int(smp.n_blocks), np.uint64).reshape(int(smp.n_blocks), 2),
                ctx.download(smp.d_values, int(smp.n_samples), np.uint32))

    def expand_sa(self, r, rows=None, ctx=None):
        """sx_index_expand_sa: the suffix array of a sampled record r, located on the device; rows=(lo, hi): SA[lo .. hi)"""
        ctx = ctx or self.ctx
        N = int(self.record_info(r).N)
        lo, hi = (0, N) if rows is None else rows
        out = np.zeros(max(0, hi - lo), dtype=np.uint32)
        ctx._check(ctx.lib.sx_index_expand_sa(ctx.h, self._handle(), r, lo, hi, _ptr(out)), "sx_index_expand_sa")
        return out

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.sx_index_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            if getattr(self.ctx, "h", None):  # (a closed context has taken the device's state with it)
                self.close()
        except Exception:
            pass


_tls = threading.local()


def _libc_free(address):
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    libc.free.restype = None
    libc.free(address)


def default_context(device=None):
    """The calling thread's context (created on first use, like the C host layer's)."""
    ctx = getattr(_tls, "ctx", None)
    if ctx is None or (device is not None and ctx.device != device):
        ctx = Context(device or 0)
        _tls.ctx = ctx
    return ctx


# ---------------------------------------------------------------------------
# reference-shaped results
# ---------------------------------------------------------------------------

class SuffixArray:
    """stralg/suffix_array.h:10-20: string (borrowed, with terminator), length, array."""

    def __init__(self, string, array):
        self.string = string
        self.length = int(array.size)
        self.array = array
        self.inverse = None
        self.lcp = None


class RemapTable:
    """stralg/remap.h:9-19."""

    def __init__(self, alphabet_size, table, rev_table):
        self.alphabet_size = alphabet_size
        self.table = table
        self.rev_table = rev_table


class BwtTable:
    """stralg/bwt.h:36-44; o_table / ro_table are (N+1, sigma) arrays: O(a, i) = o_table[i, a]."""

    def __init__(self, remap_table, sa, c_table, o_table, ro_table):
        self.remap_table = remap_table
        self.sa = sa
        self.c_table = c_table
        self.o_table = o_table
        self.ro_table = ro_table


def _symbols(x):
    """bytes-like or array without terminator -> uint8 array; stops at the first 0 like strlen."""
    a = np.frombuffer(bytes(x), dtype=np.uint8) if isinstance(x, (bytes, bytearray, memoryview)) else np.asarray(x, dtype=np.uint8)
    zero = np.flatnonzero(a == 0)
    return a[: zero[0]] if zero.size else a


def _with_terminator(a):
    out = np.zeros(a.size + 1, dtype=np.uint8)
    out[: a.size] = a
    return out


def sa_is_construction(remapped_string, alphabet_size, ctx=None):
    """stralg/suffix_array.h:31-35 (sa_is.c:466-509)."""
    ctx = ctx or default_context()
    text = _symbols(remapped_string)
    return SuffixArray(_with_terminator(text), ctx.sa_build(text, alphabet_size))


def sa_is_mem_construction(remapped_string, alphabet_size, ctx=None):
    """stralg/suffix_array.h:37-41 (sa_is_mem.c:471-494): same array, same device path."""
    return sa_is_construction(remapped_string, alphabet_size, ctx)


def skew_sa_construction(string, ctx=None):
    """stralg/suffix_array.h:26-29 (skew.c:388-395): raw bytes 1..255, alphabet fixed at 256."""
    return sa_is_construction(string, 256, ctx)


def alloc_remap_table(string):
    """stralg/remap.c:8-41: order-preserving dense codes, 0 reserved for the sentinel."""
    s = _symbols(string)
    present = np.zeros(256, dtype=bool)
    present[s] = True
    present[0] = False
    table = np.full(256, -1, dtype=np.int16)
    rev = np.full(128, -1, dtype=np.int16)
    table[0] = 0
    rev[0] = 0
    letters = np.flatnonzero(present)
    if letters.size > 127:
        raise StralgAmdError("more than 127 distinct letters: stralg's remap table cannot hold them (remap.h:14-18)")
    table[letters] = np.arange(1, letters.size + 1)
    rev[1: letters.size + 1] = letters
    return RemapTable(int(letters.size + 1), table, rev)


def remap(string, table):
    """stralg/remap.c:102-114; raises where the reference returns NULL (letter not in the table)."""
    s = _symbols(string)
    out = table.table[s]
    if (out < 0).any():
        raise StralgAmdError("remap: the string holds a letter that is not in the table")
    return out.astype(np.uint8)


def remap_string(string):
    """stralg/remap.c:155-165: returns (remapped symbols, alphabet_size)."""
    t = alloc_remap_table(string)
    return remap(string, t), t.alphabet_size


def init_bwt_table(sa, rsa, remap_table, ctx=None):
    """stralg/bwt.h:73-76 (bwt.c:22-89): C, O and (when rsa is given) RO tables."""
    ctx = ctx or default_context()
    sigma = remap_table.alphabet_size
    c, o = ctx.bwt_tables(sa.string[:-1], sa.array, sigma)
    ro = None
    if rsa is not None:
        _, ro = ctx.bwt_tables(rsa.string[:-1], rsa.array, sigma)
    return BwtTable(remap_table, sa, c, o, ro)


def build_complete_table(string, include_reverse=True, ctx=None):
    """stralg/bwt.h:156-160 (bwt.c:134-161): remap -> SA-IS -> [reverse, SA-IS] -> tables."""
    ctx = ctx or default_context()
    table = alloc_remap_table(string)
    remapped = remap(string, table)
    sigma = table.alphabet_size
    # one device pass per direction: the induced sort hands over the BWT with the suffix array
    sa_arr, c, o = ctx.build_tables(remapped, sigma)
    ro = None
    if include_reverse:
        _, _, ro = ctx.build_tables(remapped[::-1].copy(), sigma, want_sa=False)
    sa = SuffixArray(_with_terminator(remapped), sa_arr)
    return BwtTable(table, sa, c, o, ro)


def approx_cigar(m, gaps):
    """The reference's CIGAR (cigar.c edits_to_cigar of the reversed edit string) of a hit of a pattern of m symbols
    whose I/D operations are `gaps` (sx_approx_hit.gap[:n_gaps]: index in the edit string | APPROX_GAP_D for a D)."""
    ops = ["M"] * (m + sum(1 for g in gaps if g & _lib.APPROX_GAP_D))
    for g in gaps:
        ops[g & 0x7FFF] = "D" if g & _lib.APPROX_GAP_D else "I"
    out, k = [], 0
    while k < len(ops):
        r = k
        while r < len(ops) and ops[r] == ops[k]:
            r += 1
        out.append(f"{r - k}{ops[k]}")
        k = r
    return "".join(out)


def approx_matches(hits, hit_offsets, pattern_lengths, sa):
    """sx_approx_hit records -> per pattern the list next_bwt_approx_match yields: (position, match_length, cigar)"""
    out = []
    for q in range(len(hit_offsets) - 1):
        res = []
        for h in hits[int(hit_offsets[q]):int(hit_offsets[q + 1])]:
            cigar = approx_cigar(int(pattern_lengths[q]), [int(g) for g in h["gap"][:int(h["n_gaps"])]])
            ml = int(h["match_length"])
            res.extend((int(pos), ml, cigar) for pos in sa[int(h["L"]):int(h["R"])])
        out.append(res)
    return out


def bwt_approx_search(bwt_table, patterns, edits, ctx=None, indels=True):
    """stralg/bwt.c:226-422 (init_bwt_approx_iter / next_bwt_approx_match) for a batch of remapped patterns at once:
    per pattern the list of (position, match_length, cigar) the reference iterator yields, in its order.  The RO table
    (when the table has one) feeds the search's D table.  A pattern that is empty or holds a symbol 0 or >=
    alphabet_size has no matches.
    indels=False: mismatches only -- of that list the entries whose CIGAR is "<pattern length>M", in its order: every
    occurrence of a string at Hamming distance <= edits from the pattern, once."""
    ctx = ctx or default_context()
    pats = [np.asarray(p, dtype=np.uint8) if not isinstance(p, (bytes, bytearray)) else np.frombuffer(bytes(p), np.uint8)
            for p in patterns]
    offsets = np.zeros(len(pats) + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum([p.size for p in pats])
    flat = np.concatenate(pats).astype(np.uint8) if offsets[-1] else np.zeros(0, np.uint8)
    hit_off, hits = ctx.bwt_approx_search(bwt_table.c_table, bwt_table.o_table, bwt_table.ro_table,
                                          bwt_table.remap_table.alphabet_size, flat, offsets, edits, indels=indels)
    return approx_matches(hits, hit_off, [p.size for p in pats], bwt_table.sa.array)


def map_reads(fasta, fastq, edits, ctx=None, both_strands=False, best=False, indels=True, tags=False, unmapped=False, header=False,
              mapq=False):
    """The reference read mapper (tools/readmappers/bwt_readmapper: -p genome.fa, then -d edits genome.fa reads.fq) on the
    bytes of a FASTA and a FASTQ file: its stdout, the SAM lines of every match of every read in every record within
    `edits` edits, byte for byte.  Per read the records come in the mapper's list order, which is the FASTA file's order
    (the iterator yields the records last first, -p writes them so, and -d prepends each to its list).
    both_strands: behind the lines of every read come the lines of its reverse complement (the name, the sequence reversed
    and complemented, the quality string reversed) as the reference prints them for such a read, with FLAG 16 in place of 0;
    the reference itself maps one strand only.
    best: per read only the lines of its best stratum: those the mapper prints for it at -d e*, the smallest edit count in
    0 .. edits at which it prints any for that read (with both_strands: over both strands of the read together).
    indels=False: mismatches only -- of the mapper's lines those whose CIGAR is "<length of SEQ>M" (every placement of a read
    within `edits` substitutions, once); with best the strata are taken over these lines.
    tags: every line gets "\tNM:i:<nm>\tMD:Z:<md>" behind QUAL -- the edit distance and the mismatch string of the line's POS,
    CIGAR and SEQ over the record's letters (no case folding), rendered on the device once per hit.  The tags read the
    records' strings, so the call then maps through a temporary Index.from_fasta on ctx (the same lines).
    unmapped: every read (with both_strands: the read and its reverse complement) that prints no line gets one,
    "<name>\t4\t*\t0\t0\t*\t*\t0\t0\t<seq>\t<qual>", where its lines would stand (no tags on it).
    header: "@HD\tVN:1.6\tSO:unsorted" and "@SQ\tSN:<name>\tLN:<length>" per record in front of the text.
    mapq (needs best; without it StralgAmdError, code SX_E_ARG = -1): FLAG and MAPQ say which line stands for the read and how
    alone it is in its best stratum.  Of the n lines of a read (with both_strands: of the read and its reverse complement) the
    first keeps its FLAG, every other one has 256 added (secondary), and all carry MAPQ 50 (n = 1), 3 (n = 2), 1 (n = 3 or 4)
    or 0 (n >= 5).  n counts lines: with indels some placements print twice, so indels=False is what to combine this with."""
    ctx = ctx or default_context()
    if tags:
        with Index.from_fasta(fasta, ctx=ctx) as idx:
            return idx.map_reads(fastq, edits, both_strands=both_strands, best=best, indels=indels, tags=True, unmapped=unmapped,
                                 header=header, mapq=mapq)
    records = [(name, build_complete_table(seq, True, ctx)) for name, seq in ctx.fasta_records(fasta)]
    chunks = []
    ctx.map_reads_stream(records, fastq, edits, chunks.append, both_strands=both_strands, best=best, indels=indels, unmapped=unmapped,
                         header=header, mapq=mapq)
    return b"".join(chunks)


def map_pairs(fasta, fastq1, fastq2, edits, min_insert=0, max_insert=1000, ctx=None, best=False, indels=True, header=False):
    """Index.map_pairs through a temporary Index.from_fasta on ctx: the SAM text of the proper pairs of two FASTQ files
    (mate 1 and mate 2 of pair p are read p of either file)."""
    ctx = ctx or default_context()
    with Index.from_fasta(fasta, ctx=ctx) as idx:
        return idx.map_pairs(fastq1, fastq2, edits, min_insert=min_insert, max_insert=max_insert, best=best, indels=indels, header=header)
