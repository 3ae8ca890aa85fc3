"""Mirror of the reference's `bwt_util` merge helpers (src/bwt_util.rs:21-141): the interleave merge of Holt & McMillan 2014, run on
the MI355X through the C ABI (msbwt_rle_merge).

    >>> from oracle.oracle import naive_bwt
    >>> data = ["CCGT", "ACG"]
    >>> bwt_stream = naive_bwt(data)
    >>> bwts = [naive_bwt([s]) for s in data]
    >>> pairwise_stream = pairwise_bwt_merge(bwts[0].encode(), bwts[1].encode())
    >>> assert bwt_stream.encode() == pairwise_stream
"""
import numpy as np

from . import bwt_converter, string_util
from .rle_bwt import RleBWT, rle_decode


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


def merge_numpy_files(paths, out_path, device=None):
    """Merges the BWTs in the .npy files `paths` (RLE bytes, as save_bwt_numpy writes them) into `out_path`: neighbours are merged
    round by round in a balanced tree, so a symbol takes part in ceil(log2 n) merges, not in up to n - 1."""
    level = [np.load(p, mmap_mode="r") for p in paths]
    if not level:
        raise ValueError("no BWT to merge")
    handle = RleBWT(device=-1 if device is None else device)
    while len(level) > 1:
        merged = [handle.merge(level[i], level[i + 1]) for i in range(0, len(level) - 1, 2)]
        level = merged + ([level[-1]] if len(level) % 2 else [])
    bwt_converter.save_bwt_numpy(np.ascontiguousarray(level[0], dtype=np.uint8), out_path)
