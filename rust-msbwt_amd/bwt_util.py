"""Mirror of the reference's `bwt_util` merge helpers (src/bwt_util.rs:21-141): the interleave merge of Holt & McMillan 2014, run on
the MI355X through the C ABI (msbwt_rle_merge, msbwt_rle_merge_many).

    >>> from oracle.oracle import naive_bwt
    >>> data = ["CCGT", "ACG"]
    >>> bwt_stream = naive_bwt(data)
    >>> bwts = [naive_bwt([s]) for s in data]
    >>> pairwise_stream = pairwise_bwt_merge(bwts[0].encode(), bwts[1].encode())
    >>> assert bwt_stream.encode() == pairwise_stream
"""
import numpy as np

from . import bwt_converter, string_util
from ._lib import MERGE_MAX_INPUTS
from .rle_bwt import RleBWT, rle_decode, rle_total


def _to_rle(bwt):
    if isinstance(bwt, (str, bytes, bytearray)):
        return bwt_converter.convert_to_vec(bwt)
    codes = np.ascontiguousarray(bwt, dtype=np.uint8).ravel()
    return bwt_converter.convert_to_vec(string_util.convert_itos(codes)) if codes.size else np.empty(0, dtype=np.uint8)


def pairwise_bwt_merge(bwt0, bwt1, device=None):
    """The BWT of the union of the read sets behind `bwt0` and `bwt1` (pairwise_bwt_merge, src/bwt_util.rs:108-141).  The two BWTs
    are symbol strings over "$ACGNT" (str or bytes) or np.uint8 arrays of symbol codes; the merged one comes back in the form of
    `bwt0`.  Rows of equal rotations: those of `bwt0` first."""
    handle = RleBWT(device=-1 if device is None else device)
    codes = rle_decode(handle.merge(_to_rle(bwt0), _to_rle(bwt1)))
    if isinstance(bwt0, str):
        return string_util.convert_itos(codes)
    if isinstance(bwt0, (bytes, bytearray)):
        return string_util.convert_itos(codes).encode()
    return codes


def multi_bwt_merge(bwts, device=None):
    """The BWT of the union of the read sets behind every BWT of `bwts` (at most MERGE_MAX_INPUTS), merged in one pass: what a left
    fold of pairwise_bwt_merge gives.  The BWTs come in the forms pairwise_bwt_merge takes; the merged one comes back in the form
    of the first.  Rows of equal rotations: those of the earlier BWT first."""
    bwts = list(bwts)
    if not bwts:
        raise ValueError("no BWT to merge")
    handle = RleBWT(device=-1 if device is None else device)
    codes = rle_decode(handle.merge_many([_to_rle(b) for b in bwts]))
    if isinstance(bwts[0], str):
        return string_util.convert_itos(codes)
    if isinstance(bwts[0], (bytes, bytearray)):
        return string_util.convert_itos(codes).encode()
    return codes


# merge_numpy_files(method="auto") merges in one pass from this many inputs on and by the tree of pairwise merges below it
# ("Merge of any number of BWTs in one pass", has the measurements behind the number)
ONE_PASS_MIN_INPUTS = 4


def _one_pass_plan(level, device):
    """(HBM bytes the one-pass merge of `level` needs, free HBM bytes of the device)."""
    import torch
    from . import merge_many_plan
    index = torch.cuda.current_device() if device is None or device < 0 else device
    return merge_many_plan([rle_total(r) for r in level]), torch.cuda.mem_get_info(index)[0]


def merge_numpy_files(paths, out_path, device=None, method="auto", sources_out=None):
    """Merges the BWTs in the .npy files `paths` (RLE bytes, as save_bwt_numpy writes them) into `out_path`.  The file is the same
    whatever the method:
      "tree"      neighbours are merged round by round in a balanced tree, so a symbol takes part in ceil(log2 n) merges, not in
                  up to n - 1;
      "one_pass"  all of them in one merge_many call: at most MERGE_MAX_INPUTS files, and their plan (merge_many_plan) must fit
                  the free HBM;
      "auto"      one pass from ONE_PASS_MIN_INPUTS files on where it can be taken, else the tree.
    `sources_out`: a path that receives the source vector as a plain .npy of uint8 -- for every merged row the index in `paths` of the
    file it came from -- so that a later process can load_numpy_file(out_path) and set_sources(np.load(sources_out)).  It takes the one
    pass (method "auto" or "one_pass"): the tree has no such vector."""
    if method not in ("auto", "tree", "one_pass"):
        raise ValueError("method must be \"auto\", \"tree\" or \"one_pass\"")
    level = [np.load(p, mmap_mode="r") for p in paths]
    if not level:
        raise ValueError("no BWT to merge")
    handle = RleBWT(device=-1 if device is None else device)
    one_pass = method == "one_pass"
    if one_pass and len(level) > MERGE_MAX_INPUTS:
        raise ValueError("%d BWTs, one pass merges at most %d" % (len(level), MERGE_MAX_INPUTS))
    if one_pass or (method == "auto" and (ONE_PASS_MIN_INPUTS if sources_out is None else 1) <= len(level) <= MERGE_MAX_INPUTS):
        need, free = _one_pass_plan(level, device)
        if one_pass and need > free:
            raise MemoryError("the one-pass merge needs %d bytes of HBM, %d are free" % (need, free))
        one_pass = need <= free
    if sources_out is not None and not one_pass:
        raise ValueError("sources_out needs the one-pass merge: at most %d files whose plan fits the free HBM" % MERGE_MAX_INPUTS)
    if one_pass:
        level = [handle.merge_many(level, return_sources=sources_out is not None)]
        if sources_out is not None:
            merged, sources = level[0]
            level = [merged]
            with open(sources_out, "wb") as f:  # (the path as given: np.save would append ".npy" to one without it)
                np.save(f, sources)
    while len(level) > 1:
        merged = [handle.merge(level[i], level[i + 1]) for i in range(0, len(level) - 1, 2)]
        level = merged + ([level[-1]] if len(level) % 2 else [])
    bwt_converter.save_bwt_numpy(np.ascontiguousarray(level[0], dtype=np.uint8), out_path)
