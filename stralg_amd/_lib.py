"""ctypes binding of libstralg_amd.so (the C-ABI declared in include/stralg_amd.h).

The product library is stralg_amd/libstralg_amd.so, built in-tree by
stralg_amd/csrc/Makefile for gfx950.  There is no CPU fallback: if the library
is missing, or no GPU is visible when a context is created, the call raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
PRODUCT_LIB = os.path.join(_HERE, "libstralg_amd.so")

KC_NAMES = ["classify", "samples", "keys", "radix_hist", "radix_scatter", "scan", "names", "doubling",
            "induce_gather", "induce_scan", "induce_scatter", "induce_chain", "bwt_gather", "otable", "misc",
            "fasta", "remap", "lcp", "search", "local_sort", "sam",
            "pair_count", "pair_scan", "pair_fill", "pair_layout", "pair_emit", "mapq"]


class KernelStat(C.Structure):
    _fields_ = [("launches", C.c_uint64), ("ms", C.c_double), ("alg_bytes", C.c_uint64)]


class BuildStats(C.Structure):
    _fields_ = [("n", C.c_uint64), ("n_lms", C.c_uint64), ("n_samples", C.c_uint64),
                ("n_names", C.c_uint64), ("key_bits", C.c_uint32), ("key_slots", C.c_uint32),
                ("doubling_rounds", C.c_uint32), ("induce_rounds", C.c_uint32),
                ("sort_passes", C.c_uint32), ("lms_path", C.c_uint32), ("sort_local", C.c_uint32), ("refine_tiers", C.c_uint32),
                ("ms_total", C.c_double), ("induce_redo", C.c_uint32), ("long_runs", C.c_uint32),
                ("recursion_levels", C.c_uint32), ("sample_tied_permille", C.c_uint32), ("long_subbuckets", C.c_uint32),
                ("induce_early_s", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class MapStats(C.Structure):
    """include/stralg_amd.h sx_map_stats: what the loop of the last mapping call did with its batches"""
    _fields_ = [(k, C.c_uint64) for k in ("batches", "retries", "room_grown", "lone_grown", "halved", "room_first", "room_final",
                                          "batch_first", "batch_final")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class CtxCounts(C.Structure):
    """include/stralg_amd.h sx_ctx_counts: what a context carries from call to call (test hook)"""
    _fields_ = [("chain_epoch", C.c_uint32), ("readback_seq", C.c_uint32), ("chain_slab_max_epoch", C.c_uint32),
                ("has_child", C.c_uint32), ("slab_bytes", C.c_uint64 * 7),
                ("child_chain_epoch", C.c_uint32), ("child_readback_seq", C.c_uint32), ("child_chain_slab_max_epoch", C.c_uint32),
                ("child_reserved", C.c_uint32), ("child_slab_bytes", C.c_uint64 * 7)]

    def as_dict(self):
        own = dict(chain_epoch=int(self.chain_epoch), readback_seq=int(self.readback_seq),
                   chain_slab_max_epoch=int(self.chain_slab_max_epoch), slab_bytes=[int(b) for b in self.slab_bytes])
        child = dict(chain_epoch=int(self.child_chain_epoch), readback_seq=int(self.child_readback_seq),
                     chain_slab_max_epoch=int(self.child_chain_slab_max_epoch), slab_bytes=[int(b) for b in self.child_slab_bytes])
        return dict(own, has_child=bool(self.has_child), child=child)


# include/stralg_amd.h sx_approx_hit (32 bytes)
APPROX_MAX_EDITS = 8
APPROX_GAP_D = 0x8000
APPROX_HIT_DTYPE = [("query", "<u4"), ("L", "<u4"), ("R", "<u4"), ("match_length", "<u2"), ("n_gaps", "<u2"),
                    ("gap", "<u2", (APPROX_MAX_EDITS,))]
SX_E_ARG, SX_E_MALFORMED, SX_E_CAPACITY = -1, -4, -5
SX_E_INTERNAL = -3
SX_SECTION_SAM = 3
SX_FLAG_SAM_BATCH_READS, SX_FLAG_SAM_WINDOW_BYTES = 18, 19
SX_FLAG_LOCATE_CHUNK_ROWS = 20
SX_FLAG_INDUCE_EARLY_S_OFF = 21
SX_FLAG_SAM_ROOM_HITS = 22
SX_FLAG_CHAIN_EPOCH, SX_FLAG_READBACK_SEQ = 23, 24  # (test switches, as SX_FLAG_SAM_ROOM_HITS)
SX_FLAG_PAIRS_ROOM_LINES = 25  # (a test switch too)
N_SLABS = 7
SLAB_CHAIN = 6
CHAIN_EPOCH_LIMIT = 1 << 24  # the look-back epoch has 24 bits: the launch after 2^24 - 1 takes 1 again
SX_MAP_BOTH_STRANDS = 1
SX_MAP_BEST_STRATUM = 8
SX_MAP_NO_INDELS = 16
SX_MAP_TAGS = 64
SX_MAP_UNMAPPED = 128
SX_MAP_HEADER = 256
SX_MAP_MAPQ = 1024
SX_SEARCH_NO_INDELS = 1


def map_flags(both_strands=False, best=False, indels=True, tags=False, unmapped=False, header=False, mapq=False):
    """the flags word of sx_map_reads_stream_ex / sx_index_map_reads_ex"""
    return ((SX_MAP_BOTH_STRANDS if both_strands else 0) | (SX_MAP_BEST_STRATUM if best else 0)
            | (0 if indels else SX_MAP_NO_INDELS) | (SX_MAP_TAGS if tags else 0) | (SX_MAP_UNMAPPED if unmapped else 0)
            | (SX_MAP_HEADER if header else 0) | (SX_MAP_MAPQ if mapq else 0))


def pair_flags(best=False, indels=True, header=False):
    """the flags word of sx_index_map_pairs (both strands are implied)"""
    return (SX_MAP_BEST_STRATUM if best else 0) | (0 if indels else SX_MAP_NO_INDELS) | (SX_MAP_HEADER if header else 0)


def search_flags(indels=True):
    """the search_flags word of the _ex search calls"""
    return 0 if indels else SX_SEARCH_NO_INDELS


class SamBatch(C.Structure):
    """include/stralg_amd.h sx_sam_batch (device pointers)"""
    _fields_ = [("d_hits", C.c_void_p), ("n_hits", C.c_uint64), ("d_sa", C.c_void_p), ("sa_len", C.c_uint64),
                ("d_sa_list", C.c_void_p), ("d_sa_len_list", C.c_void_p),
                ("d_names", C.c_void_p), ("d_seqs", C.c_void_p), ("d_quals", C.c_void_p),
                ("d_name_off", C.c_void_p), ("d_seq_off", C.c_void_p), ("d_qual_off", C.c_void_p), ("n_reads", C.c_uint32),
                ("d_rnames", C.c_void_p), ("d_rname_off", C.c_void_p), ("n_records", C.c_uint32)]


class SamBatchEx(C.Structure):
    """include/stralg_amd.h sx_sam_batch_ex: a batch and a FLAG per read (device memory, uint16)"""
    _fields_ = [("batch", SamBatch), ("d_read_flags", C.c_void_p)]


class SamBatchTags(C.Structure):
    """include/stralg_amd.h sx_sam_batch_tags: a batch with flags (or none), every record's text and table of letters (NM
    and MD behind QUAL) and, optionally, positions located beforehand"""
    _fields_ = [("ex", SamBatchEx), ("d_text_list", C.c_void_p), ("d_letters", C.c_void_p), ("d_positions", C.c_void_p),
                ("d_pos_off", C.c_void_p), ("pos_base", C.c_uint64)]


class SamBatchMapq(C.Structure):
    """include/stralg_amd.h sx_sam_batch_mapq: the batch of the unmapped emitter and a 16-bit quality word a hit (device
    memory): the low 8 bits the MAPQ of the hit's lines, bit 8 set for 256 on top of their FLAG"""
    _fields_ = [("tags", SamBatchTags), ("d_hit_quality", C.c_void_p)]


# include/stralg_amd.h sx_pair_line (20 bytes)
PAIR_LINE_DTYPE = [("hit", "<u4"), ("pos", "<u4"), ("pnext", "<u4"), ("tlen", "<i4"), ("flag", "<u4")]


class PairOpts(C.Structure):
    """include/stralg_amd.h sx_pair_opts"""
    _fields_ = [("min_insert", C.c_uint32), ("max_insert", C.c_uint32)]


class Fastq(C.Structure):
    """include/stralg_amd.h sx_fastq"""
    _fields_ = [("count", C.c_uint32), ("names", C.c_void_p), ("seqs", C.c_void_p), ("quals", C.c_void_p),
                ("name_off", C.c_void_p), ("seq_off", C.c_void_p), ("qual_off", C.c_void_p)]


class MapRecord(C.Structure):
    """include/stralg_amd.h sx_map_record (host pointers)"""
    _fields_ = [("name", C.c_char_p), ("sa", C.c_void_p), ("c_table", C.c_void_p), ("o_table", C.c_void_p),
                ("ro_table", C.c_void_p), ("N", C.c_uint64), ("sigma", C.c_uint32), ("remap", C.c_void_p)]


class FastqDev(C.Structure):
    """include/stralg_amd.h sx_fastq_dev (device pointers)"""
    _fields_ = [("count", C.c_uint32), ("d_names", C.c_void_p), ("d_seqs", C.c_void_p), ("d_quals", C.c_void_p),
                ("d_name_off", C.c_void_p), ("d_seq_off", C.c_void_p), ("d_qual_off", C.c_void_p),
                ("name_bytes", C.c_uint64), ("seq_bytes", C.c_uint64), ("qual_bytes", C.c_uint64)]


class IndexSource(C.Structure):
    """include/stralg_amd.h sx_index_source"""
    _fields_ = [("record", MapRecord), ("string", C.c_void_p)]


class IndexRecord(C.Structure):
    """include/stralg_amd.h sx_index_record"""
    _fields_ = [("name", C.c_char_p), ("N", C.c_uint64), ("sigma", C.c_uint32), ("has_ro", C.c_int), ("has_string", C.c_int),
                ("remap", C.c_void_p), ("d_string", C.c_void_p), ("d_sa", C.c_void_p), ("d_c", C.c_void_p), ("d_o", C.c_void_p),
                ("d_ro", C.c_void_p)]


class IndexOcc(C.Structure):
    """include/stralg_amd.h sx_index_occ"""
    _fields_ = [("compact", C.c_int), ("d_occ", C.c_void_p), ("d_rocc", C.c_void_p), ("stride", C.c_uint32),
                ("sigma_pad", C.c_uint32), ("n_blocks", C.c_uint64)]


class IndexSamples(C.Structure):
    """include/stralg_amd.h sx_index_samples"""
    _fields_ = [("d_marks", C.c_void_p), ("d_values", C.c_void_p), ("sa_log2", C.c_uint32), ("n_samples", C.c_uint64),
                ("n_blocks", C.c_uint64)]


SX_SECTION_INDEX = 4
SX_INDEX_COMPACT = 1
SX_INDEX_PACKED = 4
SA_SAMPLE_MAX_LOG2 = 10


def index_flags(compact, sa_sample=0, packed=False):
    """the flags of sx_index_build_fasta_ex / sx_index_from_sources_ex; sa_sample: 0, or a power of two in 2 .. 1024 (with
    compact); packed: a nibble a row in the blocks (with compact): checked here, before anything is built"""
    if packed and not compact:
        raise ValueError("packed needs compact=True: it is a form of the BWT blocks")
    return _sample_flags(compact, sa_sample) | (SX_INDEX_PACKED if packed else 0)


def _sample_flags(compact, sa_sample):
    sa_sample = int(sa_sample)
    if sa_sample == 0:
        return SX_INDEX_COMPACT if compact else 0
    q = sa_sample.bit_length() - 1
    if sa_sample < 2 or sa_sample != 1 << q or q > SA_SAMPLE_MAX_LOG2:
        raise ValueError(f"sa_sample must be 0 or a power of two in 2 .. 1024, not {sa_sample}")
    if not compact:
        raise ValueError("sa_sample needs compact=True: the walks read the BWT blocks")
    return SX_INDEX_COMPACT | (q << 8)


SINK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t)


def load(path=None):
    """Load the shared library and declare every entry point of include/stralg_amd.h."""
    path = path or PRODUCT_LIB
    # PyTorch-ROCm bundles its own libamdhip64 (same SONAME as /opt/rocm's).  Whichever
    # is loaded first serves the whole process, and a second copy cannot open the GPU,
    # so torch -- the process's owner of device memory and streams -- must come first.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: build it with `make -C stralg_amd/csrc` "
            "(or python -c 'import __graft_entry__ as g; g.build()'); there is no CPU fallback")
    lib = C.CDLL(path)
    vp, u8p, u32p, u64p = C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p
    sig = {
        "sx_device_count": (C.c_int, []),
        "sx_device_numa_node": (C.c_int, [C.c_int]),
        "sx_ctx_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
        "sx_ctx_destroy": (None, [vp]),
        "sx_ctx_live_count": (C.c_int, []),
        "sx_last_error": (C.c_char_p, [vp]),
        "sx_ctx_trim": (None, [vp]),
        "sx_ctx_set_flag": (C.c_int, [vp, C.c_int, C.c_int]),
        "sx_ctx_scribble": (C.c_int, [vp, C.c_int]),
        "sx_ctx_counters": (C.c_int, [vp, C.POINTER(CtxCounts)]),
        "sx_sa_build": (C.c_int, [vp, u8p, C.c_uint64, C.c_uint32, u32p]),
        "sx_sa_build_dev": (C.c_int, [vp, u8p, C.c_uint64, C.c_uint32, u32p]),
        "sx_sa_bwt_build_dev": (C.c_int, [vp, u8p, C.c_uint64, C.c_uint32, u32p, u8p]),
        "sx_bwt_tables_from_bwt_dev": (C.c_int, [vp, u8p, C.c_uint64, C.c_uint32, u32p, u32p]),
        "sx_build_tables": (C.c_int, [vp, u8p, C.c_uint64, C.c_uint32, u32p, u32p, u32p]),
        "sx_bwt_tables": (C.c_int, [vp, u8p, u32p, C.c_uint64, C.c_uint32, u32p, u32p]),
        "sx_bwt_tables_dev": (C.c_int, [vp, u8p, u32p, C.c_uint64, C.c_uint32, u32p, u32p, u8p]),
        "sx_sa_inverse_dev": (C.c_int, [vp, u32p, C.c_uint64, u32p]),
        "sx_sa_lcp_dev": (C.c_int, [vp, u8p, u32p, C.c_uint64, u32p, u32p]),
        "sx_sa_inverse_lcp": (C.c_int, [vp, u8p, u32p, C.c_uint64, u32p, u32p]),
        "sx_bwt_exact_search_dev": (C.c_int, [vp, u32p, u32p, C.c_uint64, C.c_uint32, u8p, u32p, C.c_uint32, u32p, u32p]),
        "sx_bwt_approx_search_dev": (C.c_int, [vp, u32p, u32p, u32p, C.c_uint64, C.c_uint32, u8p, u32p, C.c_uint32, C.c_int,
                                               u64p, vp, C.c_uint64, C.POINTER(C.c_uint64)]),
        "sx_bwt_best_search_dev": (C.c_int, [vp, u32p, u32p, u32p, C.c_uint64, C.c_uint32, u8p, u32p, C.c_uint32, C.c_int, u8p,
                                             u64p, vp, C.c_uint64, C.POINTER(C.c_uint64)]),
        "sx_bwt_approx_search_dev_ex": (C.c_int, [vp, u32p, u32p, u32p, C.c_uint64, C.c_uint32, u8p, u32p, C.c_uint32, C.c_int,
                                                  u64p, vp, C.c_uint64, C.POINTER(C.c_uint64), C.c_uint32]),
        "sx_bwt_best_search_dev_ex": (C.c_int, [vp, u32p, u32p, u32p, C.c_uint64, C.c_uint32, u8p, u32p, C.c_uint32, C.c_int, u8p,
                                                u64p, vp, C.c_uint64, C.POINTER(C.c_uint64), C.c_uint32]),
        "sx_bwt_approx_search_ex": (C.c_int, [vp, u32p, u32p, u32p, C.c_uint64, C.c_uint32, u8p, u32p, C.c_uint32, C.c_int,
                                              u64p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.c_uint32]),
        "sx_bwt_approx_search_compact_dev_ex": (C.c_int, [vp, u32p, u8p, u8p, C.c_uint64, C.c_uint32, u8p, u32p, C.c_uint32, C.c_int,
                                                          u64p, vp, C.c_uint64, C.POINTER(C.c_uint64), C.c_uint32]),
        "sx_bwt_approx_search_packed_dev_ex": (C.c_int, [vp, u32p, u8p, u8p, C.c_uint64, C.c_uint32, u8p, u32p, C.c_uint32, C.c_int,
                                                         u64p, vp, C.c_uint64, C.POINTER(C.c_uint64), C.c_uint32]),
        "sx_patterns_select_dev": (C.c_int, [vp, u8p, u32p, C.c_uint32, u8p, u8p, u32p, u32p, C.POINTER(C.c_uint32),
                                             C.POINTER(C.c_uint64)]),
        "sx_bwt_approx_search": (C.c_int, [vp, u32p, u32p, u32p, C.c_uint64, C.c_uint32, u8p, u32p, C.c_uint32, C.c_int,
                                           u64p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
        "sx_build_tables_stream": (C.c_int, [vp, u8p, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]),
        "sx_sam_layout_dev": (C.c_int, [vp, C.POINTER(SamBatch), u64p, C.POINTER(C.c_uint64)]),
        "sx_sam_emit_dev": (C.c_int, [vp, C.POINTER(SamBatch), u64p, C.c_uint64, C.c_uint64, C.c_uint64, u8p]),
        "sx_sam_layout_dev_ex": (C.c_int, [vp, C.POINTER(SamBatchEx), u64p, C.POINTER(C.c_uint64)]),
        "sx_sam_emit_dev_ex": (C.c_int, [vp, C.POINTER(SamBatchEx), u64p, C.c_uint64, C.c_uint64, C.c_uint64, u8p]),
        "sx_sam_layout_dev_tags": (C.c_int, [vp, C.POINTER(SamBatchTags), u64p, C.POINTER(C.c_uint64)]),
        "sx_sam_emit_dev_tags": (C.c_int, [vp, C.POINTER(SamBatchTags), u64p, C.c_uint64, C.c_uint64, C.c_uint64, u8p]),
        "sx_sam_layout_dev_unmapped": (C.c_int, [vp, C.POINTER(SamBatchTags), u64p, C.POINTER(C.c_uint64)]),
        "sx_sam_emit_dev_unmapped": (C.c_int, [vp, C.POINTER(SamBatchTags), u64p, C.c_uint64, C.c_uint64, C.c_uint64, u8p]),
        "sx_sam_layout_dev_mapq": (C.c_int, [vp, C.POINTER(SamBatchMapq), u64p, C.POINTER(C.c_uint64)]),
        "sx_sam_emit_dev_mapq": (C.c_int, [vp, C.POINTER(SamBatchMapq), u64p, C.c_uint64, C.c_uint64, C.c_uint64, u8p]),
        "sx_sam_layout_dev_pairs": (C.c_int, [vp, C.POINTER(SamBatch), vp, C.c_uint64, u64p, C.POINTER(C.c_uint64)]),
        "sx_sam_emit_dev_pairs": (C.c_int, [vp, C.POINTER(SamBatch), vp, C.c_uint64, u64p, C.c_uint64, C.c_uint64, C.c_uint64, u8p]),
        "sx_index_map_pairs": (C.c_int, [vp, vp, u8p, C.c_size_t, u8p, C.c_size_t, C.c_int, C.POINTER(PairOpts), C.c_uint32, SINK_FN,
                                         C.c_void_p]),
        "sx_map_pairs_limit": (C.c_int, [C.c_uint64, C.c_uint64]),
        "sx_fastq_index": (C.c_int, [u8p, C.c_size_t, C.POINTER(Fastq)]),
        "sx_fastq_free": (None, [C.POINTER(Fastq)]),
        "sx_map_reads_stream": (C.c_int, [vp, C.POINTER(MapRecord), C.c_uint32, u8p, C.c_size_t, C.c_int, SINK_FN, C.c_void_p]),
        "sx_map_reads_stream_ex": (C.c_int, [vp, C.POINTER(MapRecord), C.c_uint32, u8p, C.c_size_t, C.c_int, C.c_uint32, SINK_FN,
                                             C.c_void_p]),
        "sx_map_reads_limit": (C.c_int, [C.c_uint64, C.c_uint64, C.c_uint32]),
        "sx_map_last_stats": (C.c_int, [vp, C.POINTER(MapStats)]),
        "sx_fastq_strands_dev": (C.c_int, [vp, C.POINTER(FastqDev), C.POINTER(FastqDev), vp]),
        "sx_fastq_index_dev": (C.c_int, [vp, u8p, C.c_uint64, C.POINTER(FastqDev)]),
        "sx_fastq_dev_free": (None, [C.POINTER(FastqDev)]),
        "sx_index_build_fasta": (C.c_int, [vp, u8p, C.c_uint64, C.c_int, C.POINTER(vp)]),
        "sx_index_from_tables": (C.c_int, [vp, C.POINTER(MapRecord), C.c_uint32, C.POINTER(vp)]),
        "sx_index_from_sources": (C.c_int, [vp, C.POINTER(IndexSource), C.c_uint32, C.POINTER(vp)]),
        "sx_index_add_record": (C.c_int, [vp, vp, C.POINTER(IndexSource), C.c_int]),
        "sx_index_map_reads": (C.c_int, [vp, vp, u8p, C.c_size_t, C.c_int, SINK_FN, C.c_void_p]),
        "sx_index_map_reads_ex": (C.c_int, [vp, vp, u8p, C.c_size_t, C.c_int, C.c_uint32, SINK_FN, C.c_void_p]),
        "sx_index_info": (C.c_int, [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint64)]),
        "sx_index_record_info": (C.c_int, [vp, C.c_uint32, C.POINTER(IndexRecord)]),
        "sx_index_destroy": (None, [vp]),
        "sx_index_live_count": (C.c_int, []),
        "sx_index_write": (C.c_int, [vp, vp, SINK_FN, C.c_void_p]),
        "sx_download": (C.c_int, [vp, vp, vp, C.c_size_t]),
        "sx_occ_compact_bytes": (C.c_uint64, [C.c_uint64, C.c_uint32]),
        "sx_occ_compact_build_dev": (C.c_int, [vp, u8p, C.c_uint64, C.c_uint32, u8p]),
        "sx_occ_compact_expand_dev": (C.c_int, [vp, u8p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, u32p]),
        "sx_bwt_exact_search_compact_dev": (C.c_int, [vp, u32p, u8p, C.c_uint64, C.c_uint32, u8p, u32p, C.c_uint32, u32p, u32p]),
        "sx_bwt_approx_search_compact_dev": (C.c_int, [vp, u32p, u8p, u8p, C.c_uint64, C.c_uint32, u8p, u32p, C.c_uint32, C.c_int,
                                                       u64p, vp, C.c_uint64, C.POINTER(C.c_uint64)]),
        "sx_occ_packed_bytes": (C.c_uint64, [C.c_uint64, C.c_uint32]),
        "sx_occ_packed_build_dev": (C.c_int, [vp, u8p, C.c_uint64, C.c_uint32, u8p]),
        "sx_occ_packed_expand_dev": (C.c_int, [vp, u8p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, u32p]),
        "sx_bwt_exact_search_packed_dev": (C.c_int, [vp, u32p, u8p, C.c_uint64, C.c_uint32, u8p, u32p, C.c_uint32, u32p, u32p]),
        "sx_bwt_approx_search_packed_dev": (C.c_int, [vp, u32p, u8p, u8p, C.c_uint64, C.c_uint32, u8p, u32p, C.c_uint32, C.c_int,
                                                      u64p, vp, C.c_uint64, C.POINTER(C.c_uint64)]),
        "sx_index_is_packed": (C.c_int, [vp]),
        "sx_index_build_fasta_ex": (C.c_int, [vp, u8p, C.c_uint64, C.c_int, C.c_uint32, C.POINTER(vp)]),
        "sx_index_from_sources_ex": (C.c_int, [vp, C.POINTER(IndexSource), C.c_uint32, C.c_uint32, C.POINTER(vp)]),
        "sx_index_record_occ": (C.c_int, [vp, C.c_uint32, C.POINTER(IndexOcc)]),
        "sx_index_is_compact": (C.c_int, [vp]),
        "sx_index_expand_o": (C.c_int, [vp, vp, C.c_uint32, C.c_int, C.c_uint64, C.c_uint64, u32p]),
        "sx_sa_sample_bytes": (C.c_int, [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "sx_sa_sample_build_dev": (C.c_int, [vp, u32p, C.c_uint64, C.c_uint32, vp, u32p]),
        "sx_sa_locate_rows_dev": (C.c_int, [vp, u32p, u8p, C.c_uint64, C.c_uint32, vp, u32p, C.c_uint32, C.c_uint64, C.c_uint64, u32p]),
        "sx_index_record_samples": (C.c_int, [vp, C.c_uint32, C.POINTER(IndexSamples)]),
        "sx_index_expand_sa": (C.c_int, [vp, vp, C.c_uint32, C.c_uint64, C.c_uint64, u32p]),
        "sx_fasta_pack_dev": (C.c_int, [vp, u8p, C.c_uint64, u8p, C.POINTER(C.c_uint64), u32p, C.c_uint64,
                                        C.POINTER(C.c_uint32)]),
        "sx_fasta_pack": (C.c_int, [vp, u8p, C.c_uint64, u8p, C.POINTER(C.c_uint64), u32p, C.c_uint64,
                                    C.POINTER(C.c_uint32)]),
        "sx_remap_dev": (C.c_int, [vp, u8p, C.c_uint64, u8p, C.POINTER(C.c_int16), C.POINTER(C.c_uint32)]),
        "sx_reverse_dev": (C.c_int, [vp, u8p, C.c_uint64, u8p]),
        "sx_profile_enable": (C.c_int, [vp, C.c_int]),
        "sx_profile_only": (C.c_int, [vp, C.c_int]),
        "sx_profile_reset": (C.c_int, [vp]),
        "sx_profile_read": (C.c_int, [vp, C.POINTER(KernelStat)]),
        "sx_kernel_class_name": (C.c_char_p, [C.c_int]),
        "sx_last_stats": (C.c_int, [vp, C.POINTER(BuildStats)]),
        "sx_synth_dev": (C.c_int, [vp, u8p, C.c_uint64, C.c_uint32, C.c_uint64]),
        "sx_membw_probe": (C.c_int, [vp, vp, vp, C.c_uint64, C.c_int, C.POINTER(C.c_double)]),
        "sx_prim_sort_pairs_dev": (C.c_int, [vp, u64p, u32p, u64p, u32p, C.c_uint64, C.c_int, C.c_int,
                                             C.POINTER(C.c_int)]),
        "sx_prim_exclusive_sum_dev": (C.c_int, [vp, u32p, u32p, C.c_uint64, u32p]),
        "sx_prim_classify_dev": (C.c_int, [vp, u8p, C.c_uint64, u8p, u32p, u32p, u32p]),
    }
    missing = []
    for name, (res, args) in sig.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            missing.append(name)
            continue
        fn.restype = res
        fn.argtypes = args
    if missing:
        raise RuntimeError(f"{path} lacks symbols declared in include/stralg_amd.h: {missing}")
    return lib


EXPORTS = ["sx_device_count", "sx_device_numa_node", "sx_ctx_create", "sx_ctx_destroy", "sx_ctx_live_count", "sx_last_error", "sx_ctx_trim", "sx_ctx_set_flag",
           "sx_ctx_scribble", "sx_ctx_counters",
           "sx_sa_build", "sx_sa_build_dev", "sx_sa_bwt_build_dev", "sx_bwt_tables", "sx_bwt_tables_dev",
           "sx_bwt_tables_from_bwt_dev", "sx_build_tables", "sx_sa_inverse_dev", "sx_sa_lcp_dev", "sx_sa_inverse_lcp",
           "sx_bwt_exact_search_dev", "sx_bwt_approx_search_dev", "sx_bwt_approx_search", "sx_build_tables_stream", "sx_sam_layout_dev", "sx_sam_emit_dev", "sx_fastq_index", "sx_fastq_free", "sx_map_reads_stream",
           "sx_fastq_index_dev", "sx_fastq_dev_free", "sx_index_build_fasta", "sx_index_from_tables", "sx_index_from_sources",
           "sx_index_add_record", "sx_index_map_reads", "sx_index_info", "sx_index_record_info", "sx_index_destroy",
           "sx_index_live_count", "sx_index_write", "sx_download", "sx_fasta_pack_dev", "sx_fasta_pack", "sx_remap_dev", "sx_reverse_dev", "sx_profile_enable", "sx_profile_only",
           "sx_profile_reset", "sx_profile_read", "sx_kernel_class_name", "sx_last_stats",
           "sx_occ_compact_bytes", "sx_occ_compact_build_dev", "sx_occ_compact_expand_dev", "sx_bwt_exact_search_compact_dev",
           "sx_bwt_approx_search_compact_dev", "sx_index_build_fasta_ex", "sx_index_from_sources_ex", "sx_index_record_occ",
           "sx_index_is_compact", "sx_index_expand_o",
           "sx_occ_packed_bytes", "sx_occ_packed_build_dev", "sx_occ_packed_expand_dev", "sx_bwt_exact_search_packed_dev",
           "sx_bwt_approx_search_packed_dev", "sx_index_is_packed",
           "sx_sa_sample_bytes", "sx_sa_sample_build_dev", "sx_sa_locate_rows_dev", "sx_index_record_samples", "sx_index_expand_sa",
           "sx_sam_layout_dev_ex", "sx_sam_emit_dev_ex", "sx_map_reads_stream_ex", "sx_map_reads_limit", "sx_fastq_strands_dev",
           "sx_index_map_reads_ex", "sx_bwt_best_search_dev", "sx_patterns_select_dev", "sx_map_last_stats",
           "sx_bwt_approx_search_dev_ex", "sx_bwt_approx_search_compact_dev_ex", "sx_bwt_approx_search_packed_dev_ex",
           "sx_bwt_best_search_dev_ex", "sx_bwt_approx_search_ex", "sx_sam_layout_dev_tags", "sx_sam_emit_dev_tags",
           "sx_sam_layout_dev_pairs", "sx_sam_emit_dev_pairs", "sx_index_map_pairs", "sx_map_pairs_limit",
           "sx_sam_layout_dev_unmapped", "sx_sam_emit_dev_unmapped", "sx_sam_layout_dev_mapq", "sx_sam_emit_dev_mapq",
           "sx_synth_dev", "sx_membw_probe", "sx_prim_sort_pairs_dev", "sx_prim_exclusive_sum_dev", "sx_prim_classify_dev"]


def kernel_sources_sha16():
    """SHA-256 (first 16 hex digits) over the kernel sources the product library is built from (stralg_amd/csrc/*.hip,
    *.hpp, in name order): what a rocprofv3 PMC pass is stamped with (tools/pmc_to_json.py) so that bench.py can tell when
    the kernels have changed since the committed traffic figures were measured (there is no .git on the GPU box)."""
    import glob
    import hashlib
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(here, "*.hip")) + glob.glob(os.path.join(here, "*.hpp"))):
        h.update(os.path.basename(f).encode() + b"\0")
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]
