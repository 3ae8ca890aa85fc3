"""rust-msbwt_amd -- MI355X-native batched k-mer counting over a run-length-encoded
multi-string BWT: the `RleBWT::count_kmer` path of HudsonAlpha/rust-msbwt, rebuilt for
gfx950 behind the reference's own interface.

The directory name carries a hyphen (it is fixed by the project layout), so import it with
    import importlib; msbwt = importlib.import_module("rust-msbwt_amd")
or through the `rust_msbwt_amd` alias module at the repo root.

Modules mirror the reference crate: msbwt_core (BWTRange, constants, BWT), rle_bwt (RleBWT),
string_util, bwt_converter, dynamic_bwt (create_from_fastx), bwt_util (pairwise_bwt_merge, multi_bwt_merge).  Everything that computes runs in libmsbwt_hip.so.
"""
from . import _lib
from ._lib import MERGE_MAX_INPUTS
from .msbwt_core import BWT, BWTRange, VC_LEN, LETTER_BITS, NUMBER_BITS, NUM_POWER, MASK, COUNT_MASK
from .rle_bwt import RleBWT, MsbwtError, RankComm, trace_plan, canonical_trace_plan, trace_sequences, walk_plan, walk_sequences, overlap_plan, overlap_edges, OverlapResult, bridge_plan, bridge_sequences
from . import string_util, bwt_converter, msbwt_core, rle_bwt, sharded, dynamic_bwt, bwt_util
from .dynamic_bwt import create_from_fastx

__all__ = ["BWT", "BWTRange", "RleBWT", "MsbwtError", "RankComm", "string_util", "bwt_converter", "msbwt_core",
           "rle_bwt", "sharded", "dynamic_bwt", "create_from_fastx", "build_reads_plan", "build_reads_sort_tile", "bwt_util", "merge_plan", "merge_many_plan", "merge_tile", "source_index_plan", "source_block_rows", "source_narrow_rows", "spectrum_plan", "canonical_plan", "kmers_by_source_plan", "kmer_graph_plan", "unitigs_plan", "canonical_unitigs_plan", "unitig_graph_plan", "unitig_graph_by_source_plan", "trace_plan", "canonical_trace_plan", "trace_sequences", "walk_plan", "walk_sequences", "overlap_plan", "overlap_edges", "OverlapResult", "bridge_plan", "bridge_sequences", "MERGE_MAX_INPUTS", "VC_LEN", "LETTER_BITS", "NUMBER_BITS", "NUM_POWER", "MASK", "COUNT_MASK"]


def version():
    return _lib.lib().msbwt_version().decode()


def auto_table_depths(total_symbols, free_hbm_bytes, pair_index=True):
    """(flat, packed) levels of the suffix table the library builds by default for an index of that size
    with that much HBM free after plane and pair blocks (packed 0 = the table stays flat).  Pure host logic."""
    import ctypes
    flat, packed = ctypes.c_int(0), ctypes.c_int(0)
    rc = _lib.lib().msbwt_auto_table_depths(int(total_symbols), int(free_hbm_bytes), 1 if pair_index else 0,
                                            ctypes.byref(flat), ctypes.byref(packed))
    if rc:
        raise MsbwtError(rc, "msbwt_auto_table_depths")
    return flat.value, packed.value


def auto_pair_stride(total_symbols, free_hbm_bytes, hbm_total_bytes, typical_width=-1.0):
    """Spacing of the pair blocks (96 or 128) the loader picks for an index of that size: `free_hbm_bytes` free once
    the plane blocks are in place, `typical_width` what the load-time probe reports about the data
    (RleBWT.get_typical_range_width; negative = unknown).  Pure host logic (csrc/table_policy.hpp)."""
    import ctypes
    stride = ctypes.c_int(0)
    rc = _lib.lib().msbwt_auto_pair_stride(int(total_symbols), int(free_hbm_bytes), int(hbm_total_bytes), float(typical_width), ctypes.byref(stride))
    if rc:
        raise MsbwtError(rc, "msbwt_auto_pair_stride")
    return stride.value


def auto_index_plan(total_symbols, free_hbm_bytes, hbm_total_bytes, typical_width=-1.0, budget_bytes=0):
    """What the loader builds under a memory budget (msbwt_rle_set_memory_budget; 0 = none) for an index of that size:
    {"pair_index", "pair_stride", "flat_depth", "packed_depth", "index_bytes"}.  Pure host logic (csrc/table_policy.hpp, plan_index)."""
    import ctypes
    pair, stride, flat, packed = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    size = ctypes.c_uint64(0)
    rc = _lib.lib().msbwt_auto_index_plan(int(total_symbols), int(free_hbm_bytes), int(hbm_total_bytes), float(typical_width), int(budget_bytes),
                                          ctypes.byref(pair), ctypes.byref(stride), ctypes.byref(flat), ctypes.byref(packed), ctypes.byref(size))
    if rc:
        raise MsbwtError(rc, "msbwt_auto_index_plan")
    return {"pair_index": bool(pair.value), "pair_stride": stride.value, "flat_depth": flat.value, "packed_depth": packed.value, "index_bytes": size.value}



def build_reads_plan(total_symbols, free_hbm_bytes, piece=0):
    """(automatic piece for that much free HBM, HBM bytes the build of `total_symbols` symbols needs with pieces of `piece` suffixes;
    0 = the automatic piece).  Pure host logic (csrc/reads_build.hip, plan_reads_build)."""
    import ctypes
    auto, size = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = _lib.lib().msbwt_build_reads_plan(int(total_symbols), int(free_hbm_bytes), int(piece), ctypes.byref(auto), ctypes.byref(size))
    if rc:
        raise MsbwtError(rc, "msbwt_build_reads_plan")
    return auto.value, size.value


def build_reads_sort_tile():
    """Suffixes one workgroup ranks and scatters per radix pass of the builder."""
    return int(_lib.lib().msbwt_build_reads_sort_tile())


def merge_plan(total0, total1):
    """HBM bytes the merge of two BWTs of `total0` and `total1` symbols needs: at most 2.5 bytes per merged symbol + 64 MiB.  Pure host
    logic (csrc/merge.hip, plan_merge)."""
    import ctypes
    size = ctypes.c_uint64(0)
    rc = _lib.lib().msbwt_merge_plan(int(total0), int(total1), ctypes.byref(size))
    if rc:
        raise MsbwtError(rc, "msbwt_merge_plan")
    return size.value


def merge_many_plan(totals):
    """HBM bytes the one-pass merge of BWTs of `totals` symbols needs: with T their sum, at least 2 T and at most 3.25 T + 64 MiB.  Pure
    host logic (csrc/merge_many.hip, plan_merge_many)."""
    import ctypes
    import numpy as np
    a = np.ascontiguousarray([int(t) for t in totals], dtype=np.uint64)
    size = ctypes.c_uint64(0)
    rc = _lib.lib().msbwt_merge_many_plan(a.ctypes.data_as(ctypes.c_void_p) if a.size else None, a.size, ctypes.byref(size))
    if rc:
        raise MsbwtError(rc, "msbwt_merge_many_plan")
    return size.value


def merge_tile():
    """Merged rows one workgroup counts and scatters per iteration of the merge."""
    return int(_lib.lib().msbwt_merge_tile())


def source_index_plan(total_rows, n_sources):
    """HBM bytes RleBWT.set_sources holds for `n_sources` sources over `total_rows` rows: the byte per row and the checkpoints, at most
    1.5 bytes per row + SOURCE_INDEX_SLACK.  Pure host logic (csrc/source_index.hip, source_sizes)."""
    import ctypes
    size = ctypes.c_uint64(0)
    rc = _lib.lib().msbwt_source_index_plan(int(total_rows), int(n_sources), ctypes.byref(size))
    if rc:
        raise MsbwtError(rc, "msbwt_source_index_plan")
    return size.value


def spectrum_plan(total_rows, free_hbm_bytes, records=0, sorted=False):
    """HBM bytes a RleBWT.kmer_spectrum / enumerate_kmers call allocates (and frees again) on an index of `total_rows` rows with
    `free_hbm_bytes` free: the frontiers, for a sorted dump the bitmap over the rows and its rank checkpoints, and `records` records
    staged for a host dump.  Pure host logic (csrc/spectrum.hip)."""
    import ctypes
    size = ctypes.c_uint64(0)
    rc = _lib.lib().msbwt_spectrum_plan(int(total_rows), int(free_hbm_bytes), int(records), 1 if sorted else 0, ctypes.byref(size))
    if rc:
        raise MsbwtError(rc, "msbwt_spectrum_plan")
    return size.value


def canonical_plan(total_rows, free_hbm_bytes, records=0):
    """HBM bytes a RleBWT.canonical_kmer_spectrum / enumerate_canonical_kmers call allocates (and frees again): the frontiers of
    spectrum_plan, 16 bytes per frontier node for the other strand, and `records` records staged for a host dump.  Pure host logic."""
    import ctypes
    size = ctypes.c_uint64(0)
    rc = _lib.lib().msbwt_canonical_plan(int(total_rows), int(free_hbm_bytes), int(records), ctypes.byref(size))
    if rc:
        raise MsbwtError(rc, "msbwt_canonical_plan")
    return size.value


def kmers_by_source_plan(total_rows, free_hbm_bytes, n_sources, records=0, sorted=False):
    """HBM bytes a RleBWT.kmer_spectrum_by_source / enumerate_kmers_by_source call allocates (and frees again): what spectrum_plan gives
    for the walk, the sink's fixed words, and `records` records of 2 + n_sources words staged for a host dump.  Nothing in it grows
    with frontier x n_sources.  Pure host logic."""
    import ctypes
    size = ctypes.c_uint64(0)
    rc = _lib.lib().msbwt_kmers_by_source_plan(int(total_rows), int(free_hbm_bytes), int(n_sources), int(records), 1 if sorted else 0, ctypes.byref(size))
    if rc:
        raise MsbwtError(rc, "msbwt_kmers_by_source_plan")
    return size.value


def kmer_graph_plan(total_rows, free_hbm_bytes, records=0):
    """HBM bytes a RleBWT.enumerate_kmer_graph call (the host dump of `records` nodes with words, counts and l) allocates and frees
    again: what spectrum_plan(total_rows, free_hbm_bytes, 0, sorted=True) gives, 256 bytes of degree counters, the edge bytes as whole
    32-bit words and 24 bytes per record staged; the device form and kmer_graph_degrees take 24 * records less.  Pure host logic."""
    import ctypes
    size = ctypes.c_uint64(0)
    rc = _lib.lib().msbwt_kmer_graph_plan(int(total_rows), int(free_hbm_bytes), int(records), ctypes.byref(size))
    if rc:
        raise MsbwtError(rc, "msbwt_kmer_graph_plan")
    return size.value


def unitigs_plan(total_rows, free_hbm_bytes, nodes=0, unitigs=0, symbols=0):
    """HBM bytes a RleBWT.enumerate_unitigs call over `nodes` nodes that fills every buffer with `unitigs` unitigs of `symbols` symbols
    allocates and frees again (include/msbwt_hip.h writes the sum out term by term); unitigs = symbols = 0: the counting call.  The
    device form stages no sums, symbols, ends and flags.  Pure host logic."""
    import ctypes
    size = ctypes.c_uint64(0)
    rc = _lib.lib().msbwt_unitigs_plan(int(total_rows), int(free_hbm_bytes), int(nodes), int(unitigs), int(symbols), ctypes.byref(size))
    if rc:
        raise MsbwtError(rc, "msbwt_unitigs_plan")
    return size.value


def canonical_unitigs_plan(total_rows, free_hbm_bytes, classes=0, unitigs=0, symbols=0):
    """HBM bytes a RleBWT.enumerate_canonical_unitigs call over `classes` classes that fills every buffer with `unitigs` unitigs of
    `symbols` symbols allocates and frees again (include/msbwt_hip.h writes the sum out term by term); unitigs = symbols = 0: the
    counting call.  The device form stages no sums, symbols, ends and flags.  Pure host logic."""
    import ctypes
    size = ctypes.c_uint64(0)
    rc = _lib.lib().msbwt_canonical_unitigs_plan(int(total_rows), int(free_hbm_bytes), int(classes), int(unitigs), int(symbols), ctypes.byref(size))
    if rc:
        raise MsbwtError(rc, "msbwt_canonical_unitigs_plan")
    return size.value


def unitig_graph_plan(total_rows, free_hbm_bytes, nodes=0, unitigs=0, symbols=0, links=0, canonical=False):
    """HBM bytes a RleBWT.enumerate_unitig_graph call over `nodes` nodes (canonical: classes) that fills every buffer with `unitigs`
    unitigs of `symbols` symbols and `links` link entries allocates and frees again: unitigs_plan or canonical_unitigs_plan and the
    link table (include/msbwt_hip.h writes the terms out); all three 0: the counting call.  The device form stages no targets either.
    Pure host logic."""
    import ctypes
    size = ctypes.c_uint64(0)
    name = "msbwt_canonical_unitig_graph_plan" if canonical else "msbwt_unitig_graph_plan"
    rc = getattr(_lib.lib(), name)(int(total_rows), int(free_hbm_bytes), int(nodes), int(unitigs), int(symbols), int(links), ctypes.byref(size))
    if rc:
        raise MsbwtError(rc, name)
    return size.value


def unitig_graph_by_source_plan(total_rows, free_hbm_bytes, nodes=0, unitigs=0, symbols=0, links=0, n_sources=1, canonical=False):
    """HBM bytes a RleBWT.enumerate_unitig_graph_by_source call on an index of `n_sources` inputs allocates and frees again:
    unitig_graph_plan of the same kind, the range words and the staged matrix (include/msbwt_hip.h writes the terms out); unitigs,
    symbols and links all 0: the counting call.  The device form stages no matrix.  Pure host logic."""
    import ctypes
    size = ctypes.c_uint64(0)
    name = "msbwt_canonical_unitig_graph_by_source_plan" if canonical else "msbwt_unitig_graph_by_source_plan"
    rc = getattr(_lib.lib(), name)(int(total_rows), int(free_hbm_bytes), int(nodes), int(unitigs), int(symbols), int(links), int(n_sources), ctypes.byref(size))
    if rc:
        raise MsbwtError(rc, name)
    return size.value


def source_block_rows():
    """Rows per checkpoint of the source index."""
    return int(_lib.lib().msbwt_source_block_rows())


def source_narrow_rows():
    """The widest range the by-source count takes from the source bytes alone, without a checkpoint."""
    return int(_lib.lib().msbwt_source_narrow_rows())
