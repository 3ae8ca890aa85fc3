"""`RleBWT` -- host-side mirror of the reference's `msbwt2::rle_bwt::RleBWT`
(src/rle_bwt.rs) whose queries run on the MI355X through the C ABI (include/msbwt_hip.h).

Same method names, argument meaning and error behaviour as the reference's `impl BWT for
RleBWT`; `count_kmers` / `constrain_ranges` are the batch forms (host arrays), and the
`*_device` forms take device pointers (e.g. `torch.Tensor.data_ptr()`) and a HIP stream.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from .msbwt_core import BWT, BWTRange, VC_LEN


class MsbwtError(Exception):
    def __init__(self, code, message=""):
        super().__init__("msbwt error %d: %s" % (code, message))
        self.code = code


def _raise(code, handle):
    msg = _lib.lib().msbwt_rle_last_error(handle)
    msg = msg.decode(errors="replace") if msg else ""
    if code in (_lib.ERR_IO, _lib.ERR_UNEXPECTED_EOF):
        # the reference returns io::Error for these (rle_bwt.rs:84-148)
        err = EOFError(msg) if code == _lib.ERR_UNEXPECTED_EOF else OSError(msg)
        err.code = code
        raise err
    raise MsbwtError(code, msg)


def pack_reads(reads, ascii=False):
    """A read set as the C ABI takes it: (flat uint8 array, uint64 offsets[n + 1]).  `reads`: a sequence of reads -- each a str or
    bytes of "ACGTN..." (ascii=True) or an array / bytes of symbol codes 1..5 -- or such a (flat, offsets) pair itself."""
    if isinstance(reads, tuple) and len(reads) == 2 and not isinstance(reads[0], (str, bytes, bytearray)) and np.ndim(reads[1]) == 1 \
            and np.asarray(reads[1]).dtype.kind in "ui" and np.ndim(reads[0]) == 1 and len(reads[1]) >= 1:
        flat = np.ascontiguousarray(reads[0], dtype=np.uint8)
        offsets = np.ascontiguousarray(reads[1], dtype=np.uint64)
    else:
        parts = []
        for r in reads:
            if isinstance(r, str):
                if not ascii:
                    raise TypeError("a str read needs ascii=True; symbol codes come as bytes or arrays")
                r = r.encode()
            parts.append(np.frombuffer(bytes(r), dtype=np.uint8) if isinstance(r, (bytes, bytearray)) else np.ascontiguousarray(r, dtype=np.uint8).ravel())
        offsets = np.zeros(len(parts) + 1, dtype=np.uint64)
        if parts:
            np.cumsum([p.size for p in parts], out=offsets[1:])
        flat = np.concatenate(parts) if parts else np.empty(0, dtype=np.uint8)
    if flat.size == 0:
        flat = np.zeros(1, dtype=np.uint8)  # (a pointer the library may not be handed as null)
    return flat, offsets


def rle_runs(rle):
    """(symbols, lengths) of the sub-runs of an RLE stream, one per byte: byte i stands for digit << 5 * (its index among the
    consecutive bytes of its symbol) symbols (src/msbwt_core.rs:3-14).  A digit from the ninth on counts as zero: the library
    refuses a stream of 2^40 symbols or more before it reads a length."""
    a = np.ascontiguousarray(rle, dtype=np.uint8).ravel()
    syms, digits = a & 7, (a >> 3).astype(np.uint64)
    idx = np.arange(a.size)
    starts = np.ones(a.size, dtype=bool)
    starts[1:] = syms[1:] != syms[:-1]
    place = idx - np.maximum.accumulate(np.where(starts, idx, 0))  # index of the byte inside its run
    lengths = np.where(place < 8, digits << (5 * np.minimum(place, 7)).astype(np.uint64), np.uint64(0))
    return syms, lengths.astype(np.uint64)


def rle_total(rle):
    """Symbols an RLE stream encodes."""
    return int(rle_runs(rle)[1].sum(dtype=np.uint64)) if len(rle) else 0


def rle_decode(rle):
    """The symbol codes (np.uint8[]) an RLE stream encodes."""
    syms, lengths = rle_runs(rle)
    return np.repeat(syms, lengths.astype(np.int64))


def _pack_rles(rles):
    """Several RLE streams as the C ABI takes them: (flat uint8 array, uint64 offsets[n + 1])."""
    parts = [np.ascontiguousarray(r, dtype=np.uint8).ravel() for r in rles]
    offsets = np.zeros(len(parts) + 1, dtype=np.uint64)
    if parts:
        np.cumsum([p.size for p in parts], out=offsets[1:])
    return (np.concatenate(parts) if parts else np.empty(0, dtype=np.uint8)), offsets


_U64_MAX = (1 << 64) - 1


def _call_growing(call, cap):
    """call(out, cap, &length) with an output buffer of `cap` bytes, once more with a larger one if the library says it needs more:
    (return code, the bytes written)."""
    length = C.c_uint64(0)
    for _ in range(2):
        out = np.empty(max(cap, 1), dtype=np.uint8)
        rc = call(out.ctypes.data_as(C.c_void_p), cap, C.byref(length))
        if rc != _lib.ERR_INVALID_ARG or length.value <= cap:
            break
        cap = int(length.value)
    return rc, out[:length.value]


_LETTERS = np.frombuffer(b"$ACGNT", dtype=np.uint8)  # a symbol code as text


def _sequences(symbols, offsets):
    """The ragged rows symbols[offsets[u]:offsets[u + 1]] of symbol codes as a list of str."""
    letters = _LETTERS[symbols].tobytes().decode()
    return [letters[int(a):int(b)] for a, b in zip(offsets[:-1], offsets[1:])]


class RleBWT(BWT):
    def __init__(self, bin_power=8, device=-1):
        """RleBWT::new() / with_bin_power (rle_bwt.rs:297-322). `device` = HIP ordinal."""
        self._h = None
        self._h = _lib.lib().msbwt_rle_new_on_device(bin_power, device)
        if not self._h:
            raise MemoryError("msbwt_rle_new failed")
        self.bin_power = bin_power

    @classmethod
    def with_bin_power(cls, bin_power, device=-1):
        return cls(bin_power, device)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                _lib.lib().msbwt_rle_free(h)
            except (TypeError, AttributeError):  # interpreter shutdown: module globals already gone
                pass

    # ---- trait BWT -------------------------------------------------------------------
    def load_vector(self, bwt):
        a = np.ascontiguousarray(bwt, dtype=np.uint8)
        rc = _lib.lib().msbwt_rle_load_vector(self._h, a.ctypes.data_as(C.c_void_p), a.size)
        if rc:
            _raise(rc, self._h)

    def load_numpy_file(self, filename):
        rc = _lib.lib().msbwt_rle_load_numpy_file(self._h, os.fsencode(filename))
        if rc:
            _raise(rc, self._h)

    def get_symbol_count(self, symbol):
        if not 0 <= symbol < VC_LEN:
            raise IndexError("symbol out of range")  # the reference panics (array index)
        return int(_lib.lib().msbwt_rle_get_symbol_count(self._h, symbol))

    def get_total_size(self):
        return int(_lib.lib().msbwt_rle_get_total_size(self._h))

    def constrain_range(self, sym, input_range):
        ol, oh = C.c_uint64(), C.c_uint64()
        rc = _lib.lib().msbwt_rle_constrain_range(self._h, sym, input_range.l, input_range.h,
                                                  C.byref(ol), C.byref(oh))
        if rc:
            _raise(rc, self._h)
        return BWTRange(int(ol.value), int(oh.value))

    def count_kmer(self, kmer):
        a = np.ascontiguousarray(kmer, dtype=np.uint8)
        out = C.c_uint64()
        rc = _lib.lib().msbwt_rle_count_kmer(self._h, a.ctypes.data_as(C.c_void_p), a.size, C.byref(out))
        if rc:
            _raise(rc, self._h)
        return int(out.value)

    # ---- construction from reads (DynamicBWT::create_from_fastx, src/dynamic_bwt.rs:453-473, built on the device) ----
    def build_from_reads(self, reads, ascii=False):
        """The RLE bytes (np.uint8[]) of the multi-string BWT of `reads` (pack_reads says what a read set may look like), with the
        semantics of naive_bwt (src/bwt_util.rs:154-171).  The handle's own index, if it has one, stays as it is."""
        flat, offsets = pack_reads(reads, ascii)
        n = offsets.size - 1
        cap = int(offsets[-1] - offsets[0]) + n
        out = np.empty(max(cap, 1), dtype=np.uint8)
        length = C.c_uint64(0)
        rc = _lib.lib().msbwt_rle_build_from_reads(self._h, flat.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p), n,
                                                   1 if ascii else 0, out.ctypes.data_as(C.c_void_p), cap, C.byref(length))
        if rc:
            _raise(rc, self._h)
        return out[:length.value]

    def load_reads(self, reads, ascii=False):
        """build_from_reads, then the result loaded as load_vector would load it."""
        flat, offsets = pack_reads(reads, ascii)
        rc = _lib.lib().msbwt_rle_load_reads(self._h, flat.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p), offsets.size - 1,
                                             1 if ascii else 0)
        if rc:
            _raise(rc, self._h)

    def set_build_piece(self, suffixes):
        """Most suffixes the builder sorts at once (0 = automatic, from the free HBM).  Results never depend on it."""
        rc = _lib.lib().msbwt_rle_set_build_piece(self._h, int(suffixes))
        if rc:
            _raise(rc, self._h)

    def build_stage_ms(self):
        """{stage: milliseconds} of the last build on this handle, and "pieces"."""
        ms = (C.c_double * len(_lib.BUILD_STAGES))()
        pieces = C.c_uint64(0)
        rc = _lib.lib().msbwt_rle_build_stage_ms(self._h, ms, C.byref(pieces))
        if rc:
            _raise(rc, self._h)
        out = {name: float(ms[i]) for i, name in enumerate(_lib.BUILD_STAGES)}
        out["pieces"] = int(pieces.value)
        return out

    # ---- merge (bwt_util::pairwise_bwt_merge, src/bwt_util.rs:21-141, iterated on the device) ----
    def merge(self, rle0, rle1, return_interleave=False):
        """The RLE bytes (np.uint8[]) of the BWT of the union of the read sets behind the BWTs `rle0` and `rle1` (RLE bytes, either
        may be empty).  With `return_interleave` a pair: those bytes and an np.uint8 array, one entry per merged row, 1 where the row
        came from `rle1` (rows of equal rotations: those of `rle0` first).  The handle's own index, if it has one, stays as it is."""
        a = np.ascontiguousarray(rle0, dtype=np.uint8).ravel()
        b = np.ascontiguousarray(rle1, dtype=np.uint8).ravel()
        bits, total = None, 0
        if return_interleave:
            total = rle_total(a) + rle_total(b)
            bits = np.zeros((total + 7) // 8 + 1 if total < 2 ** 40 else 1, dtype=np.uint8)  # (2^40 and more: the library refuses)
        args = (self._h, a.ctypes.data_as(C.c_void_p) if a.size else None, a.size, b.ctypes.data_as(C.c_void_p) if b.size else None, b.size)
        where = bits.ctypes.data_as(C.c_void_p) if return_interleave else None
        # inputs that were not canonical can merge into more bytes than they took
        rc, out = _call_growing(lambda *out: _lib.lib().msbwt_rle_merge(*args, *out, where), a.size + b.size)
        if rc:
            _raise(rc, self._h)
        return (out, np.unpackbits(bits, bitorder="little")[:total]) if return_interleave else out

    def load_merged(self, rle0, rle1):
        """merge, then the result loaded as load_vector would load it."""
        a = np.ascontiguousarray(rle0, dtype=np.uint8).ravel()
        b = np.ascontiguousarray(rle1, dtype=np.uint8).ravel()
        rc = _lib.lib().msbwt_rle_load_merged(self._h, a.ctypes.data_as(C.c_void_p) if a.size else None, a.size,
                                              b.ctypes.data_as(C.c_void_p) if b.size else None, b.size)
        if rc:
            _raise(rc, self._h)

    def merge_many(self, rles, return_sources=False):
        """The RLE bytes (np.uint8[]) of the BWT of the union of the read sets behind the BWTs `rles` (a sequence of at most
        MERGE_MAX_INPUTS arrays of RLE bytes, any of them may be empty), merged in one pass.  With `return_sources` a pair: those bytes
        and an np.uint8 array, one entry per merged row, the index of the input the row came from (rows of equal rotations: lower
        index first).  The handle's own index, if it has one, stays as it is."""
        flat, offsets = _pack_rles(rles)
        n = offsets.size - 1
        sources = None
        if return_sources:
            total = sum(rle_total(flat[offsets[i]:offsets[i + 1]]) for i in range(n)) if n <= _lib.MERGE_MAX_INPUTS else 0
            sources = np.zeros(total if total < 2 ** 40 else 0, dtype=np.uint8)  # (2^40 and more, too many inputs: the library refuses)
        args = (self._h, flat.ctypes.data_as(C.c_void_p) if flat.size else None, offsets.ctypes.data_as(C.c_void_p), n)
        where = sources.ctypes.data_as(C.c_void_p) if return_sources and sources.size else None
        # inputs that were not canonical can merge into more bytes than they took
        rc, out = _call_growing(lambda *out: _lib.lib().msbwt_rle_merge_many(*args, *out, where), flat.size)
        if rc:
            _raise(rc, self._h)
        return (out, sources) if return_sources else out

    def load_merged_many(self, rles, keep_sources=False):
        """merge_many, then the result loaded as load_vector would load it.  With `keep_sources` the merge's source vector stays
        attached (set_sources): count_kmers_by_source then counts a k-mer in every input."""
        flat, offsets = _pack_rles(rles)
        load = _lib.lib().msbwt_rle_load_merged_many_sources if keep_sources else _lib.lib().msbwt_rle_load_merged_many
        rc = load(self._h, flat.ctypes.data_as(C.c_void_p) if flat.size else None, offsets.ctypes.data_as(C.c_void_p), offsets.size - 1)
        if rc:
            _raise(rc, self._h)

    def merge_info(self):
        """{"iterations": those of the last merge on this handle (the last one found nothing to change), stage: milliseconds}."""
        ms = (C.c_double * len(_lib.MERGE_STAGES))()
        iterations = C.c_uint64(0)
        rc = _lib.lib().msbwt_rle_merge_info(self._h, C.byref(iterations), ms)
        if rc:
            _raise(rc, self._h)
        out = {name: float(ms[i]) for i, name in enumerate(_lib.MERGE_STAGES)}
        out["iterations"] = int(iterations.value)
        return out

    # ---- counts by source ------------------------------------------------------------
    def set_sources(self, sources, n_sources=None):
        """Attaches a source vector -- np.uint8, one entry per row of the loaded index, what merge_many(return_sources=True) returns or
        np.load of the file merge_numpy_files(sources_out=...) wrote -- so that count_kmers_by_source can answer.  `n_sources`: None =
        the largest entry + 1.  sources=None detaches."""
        if sources is None:
            rc = _lib.lib().msbwt_rle_set_sources(self._h, None, 0, 0)
        else:
            a = np.ascontiguousarray(sources, dtype=np.uint8).ravel()
            if n_sources is None:
                n_sources = int(a.max(initial=0)) + 1
            rc = _lib.lib().msbwt_rle_set_sources(self._h, a.ctypes.data_as(C.c_void_p) if a.size else None, a.size, int(n_sources))
        if rc:
            _raise(rc, self._h)

    def source_count(self):
        """Sources attached; 0 = none."""
        return int(_lib.lib().msbwt_rle_source_count(self._h))

    def source_totals(self):
        """uint64[source_count()]: the rows of every source."""
        out = np.zeros(max(self.source_count(), 1), dtype=np.uint64)
        rc = _lib.lib().msbwt_rle_source_totals(self._h, out.ctypes.data_as(C.c_void_p))
        if rc:
            _raise(rc, self._h)
        return out[:self.source_count()]

    def count_kmers_by_source(self, kmers):
        """kmers: (n, k) uint8 symbol codes -> uint64[n, source_count()]: out[i, s] = occurrences of row i in input s."""
        a = np.ascontiguousarray(kmers, dtype=np.uint8)
        if a.ndim != 2:
            raise ValueError("kmers must be (n, k)")
        n, k = a.shape
        out = np.empty((n, self.source_count()), dtype=np.uint64)
        rc = _lib.lib().msbwt_rle_count_kmers_by_source(self._h, a.ctypes.data_as(C.c_void_p), k, n, out.ctypes.data_as(C.c_void_p) if out.size else None)
        if rc:
            _raise(rc, self._h)
        return out

    def range_sources(self, l, h):
        """l, h: uint64[n] row ranges [l, h) -> uint64[n, source_count()]: the rows of every source inside each range."""
        l = np.ascontiguousarray(l, dtype=np.uint64)
        h = np.ascontiguousarray(h, dtype=np.uint64)
        if not (l.shape == h.shape and l.ndim == 1):
            raise ValueError("l, h must be 1-D and equally long")
        out = np.empty((l.size, self.source_count()), dtype=np.uint64)
        rc = _lib.lib().msbwt_rle_range_sources(self._h, l.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p), l.size,
                                                out.ctypes.data_as(C.c_void_p) if out.size else None)
        if rc:
            _raise(rc, self._h)
        return out

    def count_kmers_by_source_device(self, d_kmers, k, n, d_out, stream=0):
        """Device pointers (ints): n x k symbol codes -> n x source_count() u64; asynchronous on `stream`."""
        rc = _lib.lib().msbwt_rle_count_kmers_by_source_device(self._h, d_kmers, k, n, d_out, stream)
        if rc:
            _raise(rc, self._h)

    def range_sources_device(self, d_l, d_h, n, d_out, stream=0):
        """Device pointers (ints): l, h (n u64 each) -> n x source_count() u64; asynchronous on `stream`."""
        rc = _lib.lib().msbwt_rle_range_sources_device(self._h, d_l, d_h, n, d_out, stream)
        if rc:
            _raise(rc, self._h)

    # ---- the k-mers the index holds: spectrum and enumeration ----------------------------
    def _two_calls(self, fn, args, n_columns, columns):
        """The two-call pattern of a host dump fn(handle, *args, <a pointer per column>, capacity, &n): without buffers it counts;
        columns(n) then makes the n_columns numpy arrays (None: a column not wanted) that a second call fills when n > 0."""
        n = C.c_uint64(0)
        rc = fn(self._h, *args, *[None] * n_columns, 0, C.byref(n))
        if rc:
            _raise(rc, self._h)
        out = columns(n.value)
        if n.value:
            rc = fn(self._h, *args, *[None if a is None else a.ctypes.data_as(C.c_void_p) for a in out], n.value, C.byref(n))
            if rc:
                _raise(rc, self._h)
        return out

    def _device_dump(self, fn, *args, stream):
        """A device dump fn(handle, *args, &n, stream) -> n; an MsbwtError it raises carries n too (a capacity too small still learns it)."""
        n = C.c_uint64(0)
        rc = fn(self._h, *args, C.byref(n), stream)
        if rc:
            try:
                _raise(rc, self._h)
            except MsbwtError as err:
                err.n = n.value  # (set whatever the outcome)
                raise
        return n.value

    def kmer_spectrum(self, k, bins=256):
        """msbwt_rle_kmer_spectrum -> (hist, distinct, occurrences): hist[c] = distinct k-mers that occur exactly c times (hist[bins - 1]:
        bins - 1 times or more, hist[0] = 0) as uint64[bins]; their number; the sum of their counts."""
        hist = np.zeros(int(bins), dtype=np.uint64)
        distinct, occurrences = C.c_uint64(0), C.c_uint64(0)
        rc = _lib.lib().msbwt_rle_kmer_spectrum(self._h, int(k), hist.ctypes.data_as(C.c_void_p) if hist.size else None, hist.size, C.byref(distinct),
                                                C.byref(occurrences))
        if rc:
            _raise(rc, self._h)
        return hist, distinct.value, occurrences.value

    def enumerate_kmers(self, k, min_count=1, max_count=None, sorted=True, ranges=False):
        """msbwt_rle_enumerate_kmers, both calls of the two-call pattern -> (words, counts[, l]) as uint64[n]: the k-mers that occur
        min_count..max_count times (None: no upper limit) as 2-bit words (pack_2bit's layout; unpack_2bit gives the symbols), their
        counts and, with ranges=True, the start l of each one's range [l, l + count).  sorted: ascending k-mers."""
        words, counts, l = self._two_calls(_lib.lib().msbwt_rle_enumerate_kmers, (int(k), int(min_count), int(max_count or 0), 1 if sorted else 0), 3,
                                           lambda n: [np.empty(n, dtype=np.uint64), np.empty(n, dtype=np.uint64), np.empty(n, dtype=np.uint64) if ranges else None])
        return (words, counts, l) if ranges else (words, counts)

    def enumerate_kmers_device(self, k, d_words, d_counts, d_l, capacity, min_count=1, max_count=None, sorted=True, stream=0):
        """msbwt_rle_enumerate_kmers_device: device pointers (ints; d_counts, d_l may be None) of `capacity` u64 each -> n, the k-mers
        that qualify; capacity 0 only counts, 0 < capacity < n raises (nothing written).  Synchronises `stream`."""
        return self._device_dump(_lib.lib().msbwt_rle_enumerate_kmers_device, int(k), int(min_count), int(max_count or 0), 1 if sorted else 0, d_words, d_counts, d_l,
                                 int(capacity), stream=stream)

    # ---- the same with a k-mer and its reverse complement as one class ----
    def canonical_kmer_spectrum(self, k, bins=256):
        """msbwt_rle_canonical_kmer_spectrum -> (hist, distinct, occurrences) over the classes {q, rc(q)}: hist[c] = classes whose two
        strands occur c times together (a palindrome counted once), their number, the sum of their counts."""
        hist = np.zeros(int(bins), dtype=np.uint64)
        distinct, occurrences = C.c_uint64(0), C.c_uint64(0)
        rc = _lib.lib().msbwt_rle_canonical_kmer_spectrum(self._h, int(k), hist.ctypes.data_as(C.c_void_p) if hist.size else None, hist.size,
                                                          C.byref(distinct), C.byref(occurrences))
        if rc:
            _raise(rc, self._h)
        return hist, distinct.value, occurrences.value

    def enumerate_canonical_kmers(self, k, min_count=1, max_count=None, sorted=False, strands=False):
        """msbwt_rle_enumerate_canonical_kmers, both calls of the two-call pattern -> (words, counts), or with strands=True (words, own,
        other), as uint64[n]: the classes whose count own + other lies in min_count..max_count (None: no upper limit); words = the
        canonical (smaller) 2-bit word of each, own = its count, other = its reverse complement's (0 for a palindrome).  The library
        returns them in the order its walk produces; sorted=True orders them by word here, on the host."""
        words, own, other = self._two_calls(_lib.lib().msbwt_rle_enumerate_canonical_kmers, (int(k), int(min_count), int(max_count or 0)), 3,
                                            lambda n: [np.empty(n, dtype=np.uint64) for _ in range(3)])
        if sorted:
            order = np.argsort(words, kind="stable")
            words, own, other = words[order], own[order], other[order]
        return (words, own, other) if strands else (words, own + other)

    def enumerate_canonical_kmers_device(self, k, d_words, d_own, d_other, capacity, min_count=1, max_count=None, stream=0):
        """msbwt_rle_enumerate_canonical_kmers_device: device pointers (ints; d_own, d_other may be None) of `capacity` u64 each -> n, the
        classes that qualify; capacity 0 only counts, 0 < capacity < n raises (nothing written).  Synchronises `stream`."""
        return self._device_dump(_lib.lib().msbwt_rle_enumerate_canonical_kmers_device, int(k), int(min_count), int(max_count or 0), d_words, d_own, d_other,
                                 int(capacity), stream=stream)

    # ---- the k-mers of a merged index by source: one spectrum per input, and the dump filtered by per-source counts ----
    def _source_limits(self, min_counts, max_counts):
        """(min, max) as uint64[S] or None; in max_counts None or a negative entry is "no limit", 0 is "absent from this source"."""
        S = self.source_count()
        lo = hi = None
        if min_counts is not None:
            lo = np.ascontiguousarray(min_counts, dtype=np.uint64)
        if max_counts is not None:
            hi = np.array([_U64_MAX if m is None or int(m) < 0 else int(m) for m in max_counts], dtype=np.uint64)
        for a in (lo, hi):
            if a is not None and a.shape != (S,):
                raise ValueError("min_counts and max_counts hold one entry per source (%d)" % S)
        return lo, hi

    def _by_source_args(self, k, min_counts, max_counts, min_total, max_total, sorted):
        """(the arguments of both by-source dumps up to `sorted`, the limit arrays they point into -- to be kept alive)"""
        lo, hi = self._source_limits(min_counts, max_counts) if self.source_count() else (None, None)
        return (int(k), lo.ctypes.data_as(C.c_void_p) if lo is not None else None, hi.ctypes.data_as(C.c_void_p) if hi is not None else None, int(min_total),
                int(max_total or 0), 1 if sorted else 0), (lo, hi)

    def kmer_spectrum_by_source(self, k, bins=256):
        """msbwt_rle_kmer_spectrum_by_source -> (hist[S, bins], sharing[S + 1], distinct[S], occurrences[S]), uint64: hist[s, c] = k-mers
        of the merged index that input s holds exactly c times (hist[s, bins - 1]: bins - 1 times or more, hist[s, 0]: not at all);
        sharing[j] = k-mers held by exactly j inputs; per input the k-mers it holds and the sum of their counts."""
        S = self.source_count()
        hist = np.zeros((max(S, 1), int(bins)), dtype=np.uint64)
        sharing, distinct, occurrences = np.zeros(S + 1, dtype=np.uint64), np.zeros(max(S, 1), dtype=np.uint64), np.zeros(max(S, 1), dtype=np.uint64)
        rc = _lib.lib().msbwt_rle_kmer_spectrum_by_source(self._h, int(k), hist.ctypes.data_as(C.c_void_p) if hist.size else None, int(bins),
                                                          sharing.ctypes.data_as(C.c_void_p), distinct.ctypes.data_as(C.c_void_p),
                                                          occurrences.ctypes.data_as(C.c_void_p))
        if rc:
            _raise(rc, self._h)
        return hist[:S], sharing, distinct[:S], occurrences[:S]

    def enumerate_kmers_by_source(self, k, min_counts=None, max_counts=None, min_total=1, max_total=None, sorted=True, ranges=False):
        """msbwt_rle_enumerate_kmers_by_source, both calls of the two-call pattern -> (words, counts[n, S][, l]): the k-mers with
        min_counts[s] <= counts[:, s] <= max_counts[s] for every input s and min_total <= counts.sum(1) <= max_total.  In max_counts
        None (the whole argument or an entry) is no limit and 0 means ABSENT from that input: "private to input 0" is
        max_counts=[None, 0, 0, ...].  sorted: ascending k-mers; ranges=True adds the start l of each one's range."""
        S = self.source_count()
        args, _limits = self._by_source_args(k, min_counts, max_counts, min_total, max_total, sorted)
        words, counts, l = self._two_calls(_lib.lib().msbwt_rle_enumerate_kmers_by_source, args, 3,
                                           lambda n: [np.empty(n, dtype=np.uint64), np.empty((n, S), dtype=np.uint64), np.empty(n, dtype=np.uint64) if ranges else None])
        return (words, counts, l) if ranges else (words, counts)

    def enumerate_kmers_by_source_device(self, k, d_words, d_counts, d_l, capacity, min_counts=None, max_counts=None, min_total=1, max_total=None, sorted=True,
                                         stream=0):
        """msbwt_rle_enumerate_kmers_by_source_device: device pointers (ints; d_counts -- capacity x S u64 -- and d_l may be None) -> n,
        the k-mers that qualify; capacity 0 only counts, 0 < capacity < n raises (nothing written).  The limits are host arrays, as in
        enumerate_kmers_by_source.  Synchronises `stream`."""
        args, _limits = self._by_source_args(k, min_counts, max_counts, min_total, max_total, sorted)
        return self._device_dump(_lib.lib().msbwt_rle_enumerate_kmers_by_source_device, *args, d_words, d_counts, d_l, int(capacity), stream=stream)

    # ---- the k-mer graph: an edge byte per k-mer of the sorted dump, and the table of (in, out) degrees ----
    def enumerate_kmer_graph(self, k, min_count=1, min_edge=None, ranges=False):
        """msbwt_rle_enumerate_kmer_graph, both calls of the two-call pattern -> (words, counts, edges[, l]): the k-mers that occur at
        least min_count times, ascending, as enumerate_kmers gives them, and per k-mer q one uint8: bit j (A C G T -> 0..3) = the
        (k+1)-mer j.q occurs at least min_edge times (None: min_count) -- a predecessor --, bit 4 + j = q.j does -- a successor.
        graph_successors / graph_predecessors turn the bits into neighbour words."""
        words, counts, l, edges = self._two_calls(_lib.lib().msbwt_rle_enumerate_kmer_graph, (int(k), int(min_count), int(min_edge or 0)), 4,
                                                  lambda n: [np.empty(n, dtype=np.uint64), np.empty(n, dtype=np.uint64), np.empty(n, dtype=np.uint64) if ranges else None, np.zeros(n, dtype=np.uint8)])
        return (words, counts, edges, l) if ranges else (words, counts, edges)

    def enumerate_kmer_graph_device(self, k, d_words, d_counts, d_l, d_edges, capacity, min_count=1, min_edge=None, stream=0):
        """msbwt_rle_enumerate_kmer_graph_device: device pointers (ints, each may be None) of `capacity` u64 -- d_edges: bytes, any
        alignment -- -> n, the k-mers that qualify; capacity 0 only counts, 0 < capacity < n raises (nothing written).  Synchronises `stream`."""
        return self._device_dump(_lib.lib().msbwt_rle_enumerate_kmer_graph_device, int(k), int(min_count), int(min_edge or 0), d_words, d_counts, d_l, d_edges,
                                 int(capacity), stream=stream)

    def kmer_graph_degrees(self, k, min_count=1, min_edge=None):
        """msbwt_rle_kmer_graph_degrees -> (table, nodes, edges): table[i, o] (uint64, 5 x 5) = the k-mers with i predecessors and o
        successors, their number, and the number of (k+1)-mers that are edges.  No record leaves the device."""
        table = np.zeros((5, 5), dtype=np.uint64)
        nodes, edges = C.c_uint64(0), C.c_uint64(0)
        rc = _lib.lib().msbwt_rle_kmer_graph_degrees(self._h, int(k), int(min_count), int(min_edge or 0), table.ctypes.data_as(C.c_void_p), C.byref(nodes),
                                                     C.byref(edges))
        if rc:
            _raise(rc, self._h)
        return table, nodes.value, edges.value

    # ---- unitigs: the non-branching paths of the k-mer graph as ragged sequences ----
    def _unitigs(self, fn, k, min_count, min_edge, text, links=False, by_source=False):
        """Both calls of the two-call pattern of a unitig entry point -> (symbols, offsets, count_sums, ends, flags) and, as the entry
        point has them, (link_offsets, link_targets) and source_sums behind; with text=True the sequences in place of (symbols, offsets)."""
        args = (int(k), int(min_count), int(min_edge or 0))
        totals = [C.c_uint64(0) for _ in range(3 if links else 2)]  # U, S and, of a graph call, L
        refs = [C.byref(t) for t in totals]
        rc = fn(self._h, *args, *[None] * (5 + 2 * links + by_source), *[0] * len(totals), *refs)
        if rc:
            _raise(rc, self._h)
        U, S = totals[0].value, totals[1].value
        arrays = [np.zeros(S, dtype=np.uint8), np.zeros(U + 1, dtype=np.uint64), np.zeros(U, dtype=np.uint64), np.zeros(U, dtype=np.uint8), np.zeros(U, dtype=np.uint8)]
        if links:
            arrays += [np.zeros(2 * U + 1, dtype=np.uint64), np.zeros(totals[2].value, dtype=np.uint64)]
        if by_source:
            arrays.append(np.zeros((U, self.source_count()), dtype=np.uint64))
        if U:
            rc = fn(self._h, *args, *[a.ctypes.data_as(C.c_void_p) for a in arrays], *[t.value for t in totals], *refs)
            if rc:
                _raise(rc, self._h)
        if text:
            arrays[:2] = [_sequences(arrays[0], arrays[1])]
        return tuple(arrays)

    def _unitigs_device(self, fn, k, pointers, capacities, min_count, min_edge, stream):
        """A device form of a unitig entry point: its device pointers, and a total per capacity -> (U, S) or (U, S, L)."""
        totals = [C.c_uint64(0) for _ in capacities]
        rc = fn(self._h, int(k), int(min_count), int(min_edge or 0), *pointers, *[int(c) for c in capacities], *[C.byref(t) for t in totals], stream)
        if rc:
            try:
                _raise(rc, self._h)
            except MsbwtError as err:
                for name, t in zip(("n", "symbols", "links"), totals):
                    setattr(err, name, t.value)
                raise
        return tuple(t.value for t in totals)

    def _info(self, fn, names):
        w = np.zeros(len(names), dtype=np.uint64)
        rc = fn(self._h, w.ctypes.data_as(C.c_void_p))
        if rc:
            _raise(rc, self._h)
        return dict(zip(names, (int(x) for x in w)))

    def enumerate_unitigs(self, k, min_count=1, min_edge=None, text=False):
        """msbwt_rle_enumerate_unitigs, both calls of the two-call pattern -> (symbols, offsets, count_sums, ends, flags): unitig u is
        symbols[offsets[u]:offsets[u + 1]] in symbol codes (A C G T = 1 2 3 5; uint8), of offsets[u + 1] - offsets[u] - k + 1 nodes whose
        counts sum to count_sums[u]; ends[u]: low nibble = predecessor bits of its first node, high nibble = successor bits of its last;
        flags[u] bit 0 = circular.  Ascending by first k-mer.  text=True: the sequences as a list of str in place of (symbols, offsets),
        that is (sequences, count_sums, ends, flags)."""
        return self._unitigs(_lib.lib().msbwt_rle_enumerate_unitigs, k, min_count, min_edge, text)

    def enumerate_unitigs_device(self, k, d_symbols, d_offsets, d_count_sums, d_ends, d_flags, capacity_unitigs, capacity_symbols, min_count=1, min_edge=None,
                                 stream=0):
        """msbwt_rle_enumerate_unitigs_device: device pointers (ints, each may be None; the byte arrays at any alignment) -> (U, S);
        both capacities 0 only counts, a capacity too small raises (nothing written; the error carries .n = U and .symbols = S).
        Synchronises `stream`."""
        return self._unitigs_device(_lib.lib().msbwt_rle_enumerate_unitigs_device, k, (d_symbols, d_offsets, d_count_sums, d_ends, d_flags),
                                    (capacity_unitigs, capacity_symbols), min_count, min_edge, stream)

    def unitig_info(self):
        """What the last unitig call found: {"nodes", "edges", "links", "unitigs", "symbols", "circular", "longest", "rounds"}."""
        return self._info(_lib.lib().msbwt_rle_unitig_info, ("nodes", "edges", "links", "unitigs", "symbols", "circular", "longest", "rounds"))

    # ---- canonical unitigs: the same over the strand-merged graph, every class of {q, rc(q)} in one unitig once ----
    def enumerate_canonical_unitigs(self, k, min_count=1, min_edge=None, text=False):
        """msbwt_rle_enumerate_canonical_unitigs, both calls of the two-call pattern -> what enumerate_unitigs returns, for the
        strand-merged graph (1 <= k <= 31): count_sums are sums of class counts, ends the adjacency of the emitted orientation; of a
        unitig and its reverse complement the one with the smaller first k-mer is returned."""
        return self._unitigs(_lib.lib().msbwt_rle_enumerate_canonical_unitigs, k, min_count, min_edge, text)

    def enumerate_canonical_unitigs_device(self, k, d_symbols, d_offsets, d_count_sums, d_ends, d_flags, capacity_unitigs, capacity_symbols, min_count=1,
                                           min_edge=None, stream=0):
        """msbwt_rle_enumerate_canonical_unitigs_device: as enumerate_unitigs_device."""
        return self._unitigs_device(_lib.lib().msbwt_rle_enumerate_canonical_unitigs_device, k, (d_symbols, d_offsets, d_count_sums, d_ends, d_flags),
                                    (capacity_unitigs, capacity_symbols), min_count, min_edge, stream)

    def canonical_unitig_info(self):
        """What the last canonical unitig call found, for the emitted set: {"classes", "edge_classes", "links", "unitigs", "symbols",
        "circular", "longest", "rounds", "palindromes", "cut_links"}."""
        return self._info(_lib.lib().msbwt_rle_canonical_unitig_info,
                          ("classes", "edge_classes", "links", "unitigs", "symbols", "circular", "longest", "rounds", "palindromes", "cut_links"))

    # ---- unitig links: either unitig call with the compacted graph's edges behind its columns ----
    def enumerate_unitig_graph(self, k, min_count=1, min_edge=None, canonical=False, text=False):
        """msbwt_rle_enumerate_[canonical_]unitig_graph, both calls of the two-call pattern -> what enumerate_unitigs (canonical=True:
        enumerate_canonical_unitigs) returns, plus (link_offsets, link_targets): side 2u leaves unitig u forwards, side 2u + 1 leaves its
        reverse complement forwards, and side a holds link_targets[link_offsets[a]:link_offsets[a + 1]], one entry 2v + o per edge in
        A C G T order of the appended symbol: the edge reaches the first node of v (o = 0) or the reverse complement of its last node
        (o = 1).  canonical: flags[u] bit 1 = the unitig is its own reverse complement and has one side.  unitig_link_records keeps
        every edge once, write_gfa writes the graph."""
        fn = _lib.lib().msbwt_rle_enumerate_canonical_unitig_graph if canonical else _lib.lib().msbwt_rle_enumerate_unitig_graph
        return self._unitigs(fn, k, min_count, min_edge, text, links=True)

    def enumerate_unitig_graph_device(self, k, d_symbols, d_offsets, d_count_sums, d_ends, d_flags, d_link_offsets, d_link_targets, capacity_unitigs, capacity_symbols,
                                      capacity_links, min_count=1, min_edge=None, stream=0):
        """msbwt_rle_enumerate_unitig_graph_device: device pointers (ints, each may be None; the byte arrays at any alignment) ->
        (U, S, L); all three capacities 0 only counts, a capacity too small raises (nothing written; the error carries .n = U,
        .symbols = S and .links = L).  Synchronises `stream`."""
        return self._unitigs_device(_lib.lib().msbwt_rle_enumerate_unitig_graph_device, k, (d_symbols, d_offsets, d_count_sums, d_ends, d_flags, d_link_offsets, d_link_targets),
                                    (capacity_unitigs, capacity_symbols, capacity_links), min_count, min_edge, stream)

    def enumerate_canonical_unitig_graph_device(self, k, d_symbols, d_offsets, d_count_sums, d_ends, d_flags, d_link_offsets, d_link_targets, capacity_unitigs,
                                                capacity_symbols, capacity_links, min_count=1, min_edge=None, stream=0):
        """msbwt_rle_enumerate_canonical_unitig_graph_device: as enumerate_unitig_graph_device."""
        return self._unitigs_device(_lib.lib().msbwt_rle_enumerate_canonical_unitig_graph_device, k,
                                    (d_symbols, d_offsets, d_count_sums, d_ends, d_flags, d_link_offsets, d_link_targets),
                                    (capacity_unitigs, capacity_symbols, capacity_links), min_count, min_edge, stream)

    # ---- unitigs by source: either unitig graph call with the per-input sums of every unitig behind the link table ----
    def enumerate_unitig_graph_by_source(self, k, min_count=1, min_edge=None, canonical=False, text=False):
        """msbwt_rle_enumerate_[canonical_]unitig_graph_by_source, both calls of the two-call pattern, on an index with sources attached
        (load_merged_many(keep_sources=True), set_sources) -> what enumerate_unitig_graph returns with source_sums appended: U x S
        uint64, source_sums[u, s] = the rows of input s in the ranges of the nodes of unitig u (canonical: of both members of its
        classes, a palindrome once).  Row u sums to count_sums[u]; the thresholds meet the counts of all inputs together."""
        fn = _lib.lib().msbwt_rle_enumerate_canonical_unitig_graph_by_source if canonical else _lib.lib().msbwt_rle_enumerate_unitig_graph_by_source
        return self._unitigs(fn, k, min_count, min_edge, text, links=True, by_source=True)

    def enumerate_unitig_graph_by_source_device(self, k, d_symbols, d_offsets, d_count_sums, d_ends, d_flags, d_link_offsets, d_link_targets, d_source_sums,
                                                capacity_unitigs, capacity_symbols, capacity_links, min_count=1, min_edge=None, stream=0):
        """msbwt_rle_enumerate_unitig_graph_by_source_device: as enumerate_unitig_graph_device with d_source_sums (capacity_unitigs x
        source_count() u64, may be None) behind d_link_targets -> (U, S, L)."""
        return self._unitigs_device(_lib.lib().msbwt_rle_enumerate_unitig_graph_by_source_device, k,
                                    (d_symbols, d_offsets, d_count_sums, d_ends, d_flags, d_link_offsets, d_link_targets, d_source_sums),
                                    (capacity_unitigs, capacity_symbols, capacity_links), min_count, min_edge, stream)

    def enumerate_canonical_unitig_graph_by_source_device(self, k, d_symbols, d_offsets, d_count_sums, d_ends, d_flags, d_link_offsets, d_link_targets, d_source_sums,
                                                          capacity_unitigs, capacity_symbols, capacity_links, min_count=1, min_edge=None, stream=0):
        """msbwt_rle_enumerate_canonical_unitig_graph_by_source_device: as enumerate_unitig_graph_by_source_device."""
        return self._unitigs_device(_lib.lib().msbwt_rle_enumerate_canonical_unitig_graph_by_source_device, k,
                                    (d_symbols, d_offsets, d_count_sums, d_ends, d_flags, d_link_offsets, d_link_targets, d_source_sums),
                                    (capacity_unitigs, capacity_symbols, capacity_links), min_count, min_edge, stream)

    def spectrum_scratch_bytes(self):
        """Bytes of HBM scratch the last k-mer walk call of this handle allocated (and freed again before it returned)."""
        out = C.c_uint64(0)
        rc = _lib.lib().msbwt_rle_spectrum_scratch_bytes(self._h, C.byref(out))
        if rc:
            _raise(rc, self._h)
        return out.value

    # ---- traces: from seed k-mers through the k-mer graph, node by node, in batches ----
    def trace_kmers(self, seeds, k, max_steps, mode="unique", direction="right", min_count=1, min_edge=None, targets=None, symbols=None):
        """msbwt_rle_trace_kmers -> (symbols, steps, stops, edge_sums, last, fans).  seeds (and targets, optional): n packed k-mer words
        (pack_2bit), 1 <= k <= 31.  mode "unique" | "unitig" | "greedy", direction "right" | "left" (include/msbwt_hip.h, "traces", has
        the walk step by step).  symbols: (n, max_steps) uint8, row i holding steps[i] symbol codes (A C G T = 1 2 3 5) and zeros -- or
        what the `symbols` array passed in held -- behind them; stops: _lib.TRACE_STOPS names the codes; last: the node a walk ended
        on; fans: bit j = the edge by symbol j leaves it.  trace_sequences turns rows into sequences.
        numpy arrays go through the host form.  torch tensors on this handle's device (int64 or uint64 words) go through the _device
        form on torch's current stream, and torch tensors come back (words as int64)."""
        return self._trace_kmers(False, seeds, k, max_steps, mode, direction, min_count, min_edge, targets, symbols)

    def _trace_kmers(self, canonical, seeds, k, max_steps, mode, direction, min_count, min_edge, targets, symbols):
        """trace_kmers and trace_canonical_kmers: the arrays of either call"""
        mode, direction = _lib.TRACE_MODES[mode], _lib.TRACE_DIRECTIONS[direction]
        host_call = _lib.lib().msbwt_rle_trace_canonical_kmers if canonical else _lib.lib().msbwt_rle_trace_kmers
        device_call = self.trace_canonical_kmers_device if canonical else self.trace_kmers_device
        if hasattr(seeds, "data_ptr"):
            import torch
            n, dev = int(seeds.numel()), seeds.device
            if not seeds.is_contiguous() or seeds.element_size() != 8 or (targets is not None and (not targets.is_contiguous() or targets.element_size() != 8 or targets.numel() != n)):
                raise ValueError("seeds and targets are contiguous tensors of n 64-bit words")
            if symbols is None:
                symbols = torch.zeros((n, int(max_steps)), dtype=torch.uint8, device=dev)
            steps, edge_sums, last = (torch.zeros(n, dtype=torch.int64, device=dev) for _ in range(3))
            stops, fans = (torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(2))
            device_call(seeds.data_ptr(), k, n, max_steps, *[t.data_ptr() for t in (symbols, steps, stops, edge_sums, last, fans)], mode=mode, direction=direction,
                        min_count=min_count, min_edge=min_edge, d_targets=None if targets is None else targets.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
            return symbols, steps, stops, edge_sums, last, fans
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64).reshape(-1)
        n = len(seeds)
        if targets is not None:
            targets = np.ascontiguousarray(targets, dtype=np.uint64).reshape(-1)
            if len(targets) != n:
                raise ValueError("one target a seed")
        if symbols is None:
            symbols = np.zeros((n, int(max_steps)), dtype=np.uint8)
        elif symbols.dtype != np.uint8 or symbols.shape != (n, int(max_steps)) or not symbols.flags.c_contiguous:
            raise ValueError("symbols is a C-contiguous (n, max_steps) uint8 array")
        steps, edge_sums, last = (np.zeros(n, dtype=np.uint64) for _ in range(3))
        stops, fans = (np.zeros(n, dtype=np.uint8) for _ in range(2))
        rc = host_call(self._h, seeds.ctypes.data_as(C.c_void_p), None if targets is None else targets.ctypes.data_as(C.c_void_p), int(k), n, int(min_count),
                       int(min_edge or 0), mode, direction, int(max_steps), *[a.ctypes.data_as(C.c_void_p) for a in (symbols, steps, stops, edge_sums, last, fans)])
        if rc:
            _raise(rc, self._h)
        return symbols, steps, stops, edge_sums, last, fans

    def trace_kmers_device(self, d_seeds, k, n, max_steps, d_symbols, d_steps, d_stops, d_edge_sums, d_last, d_fans, mode=0, direction=0, min_count=1, min_edge=None,
                           d_targets=None, stream=0):
        """msbwt_rle_trace_kmers_device: device pointers (ints; every output and d_targets may be None; the byte arrays at any
        alignment), mode and direction as the header's numbers.  Synchronises `stream`; a device fault shows in device_status."""
        rc = _lib.lib().msbwt_rle_trace_kmers_device(self._h, d_seeds, d_targets, int(k), int(n), int(min_count), int(min_edge or 0), int(mode), int(direction),
                                                     int(max_steps), d_symbols, d_steps, d_stops, d_edge_sums, d_last, d_fans, stream)
        if rc:
            _raise(rc, self._h)

    def trace_info(self):
        """What the last trace call did: {"walks", "rounds", "queries", "steps", "longest", "pieces", "scratch_bytes", "not_nodes"}."""
        return self._info(_lib.lib().msbwt_rle_trace_info, ("walks", "rounds", "queries", "steps", "longest", "pieces", "scratch_bytes", "not_nodes"))

    # ---- canonical traces: the same through the strand-merged graph ----
    def trace_canonical_kmers(self, seeds, k, max_steps, mode="unique", direction="right", min_count=1, min_edge=None, targets=None, symbols=None):
        """msbwt_rle_trace_canonical_kmers -> (symbols, steps, stops, edge_sums, last, fans): trace_kmers through the strand-merged graph
        of the canonical unitigs (include/msbwt_hip.h, "canonical traces").  A k-mer counts with its reverse complement, so a seed may
        be a k-mer the index holds only on the other strand; edge_sums sums class counts; last is the word in the walk's orientation.
        stops: _lib.CANONICAL_TRACE_STOPS names the codes -- "unitig" mode has MIRROR, where the link chosen is a cut of the canonical
        unitigs.  Arguments, arrays and tensors as trace_kmers; trace_sequences serves both."""
        return self._trace_kmers(True, seeds, k, max_steps, mode, direction, min_count, min_edge, targets, symbols)

    def trace_canonical_kmers_device(self, d_seeds, k, n, max_steps, d_symbols, d_steps, d_stops, d_edge_sums, d_last, d_fans, mode=0, direction=0, min_count=1,
                                     min_edge=None, d_targets=None, stream=0):
        """msbwt_rle_trace_canonical_kmers_device: as trace_kmers_device."""
        rc = _lib.lib().msbwt_rle_trace_canonical_kmers_device(self._h, d_seeds, d_targets, int(k), int(n), int(min_count), int(min_edge or 0), int(mode), int(direction),
                                                               int(max_steps), d_symbols, d_steps, d_stops, d_edge_sums, d_last, d_fans, stream)
        if rc:
            _raise(rc, self._h)

    def canonical_trace_info(self):
        """What the last canonical trace call did: the words of trace_info."""
        return self._info(_lib.lib().msbwt_rle_canonical_trace_info, ("walks", "rounds", "queries", "steps", "longest", "pieces", "scratch_bytes", "not_nodes"))

    def set_trace_piece(self, walks):
        """Most walks a trace call of either kind advances at once (0 = automatic, 2^20): results never depend on it."""
        rc = _lib.lib().msbwt_rle_set_trace_piece(self._h, int(walks))
        if rc:
            _raise(rc, self._h)

    # ---- bridges: all bounded walks of the k-mer graph between two anchor k-mers ----
    def bridge_kmers(self, seeds, targets, k, max_steps, min_steps=0, max_paths=4, max_live=64, direction="right", min_count=1, min_edge=None, symbols=True):
        """msbwt_rle_bridge_kmers -> (symbols, lengths, edge_sums, found, stops, depths, live).  seeds and targets: n packed k-mer words
        each (pack_2bit), 1 <= k <= 31; include/msbwt_hip.h, "bridges", has the exploration level by level.  symbols: (n, max_paths,
        max_steps) uint8, row (i, j) holding lengths[i, j] symbol codes (A C G T = 1 2 3 5) in walk order and zeros -- or what the
        `symbols` array passed in held -- behind them; symbols=False is a counting call and returns None there.  lengths, edge_sums:
        (n, max_paths); found, depths, live: n words; stops: _lib.BRIDGE_STOPS names the codes.  bridge_sequences turns rows into
        sequences.
        numpy arrays go through the host form.  torch tensors on this handle's device (int64 or uint64 words) go through the _device
        form on torch's current stream, and torch tensors come back (words as int64)."""
        direction = _lib.TRACE_DIRECTIONS[direction]
        n_steps, n_paths = int(max_steps), int(max_paths)
        if hasattr(seeds, "data_ptr"):
            import torch
            n, dev = int(seeds.numel()), seeds.device
            if not hasattr(targets, "data_ptr") or any(not t.is_contiguous() or t.element_size() != 8 for t in (seeds, targets)) or targets.numel() != n:
                raise ValueError("seeds and targets are contiguous tensors of n 64-bit words")
            if symbols is True:
                symbols = torch.zeros((n, n_paths, n_steps), dtype=torch.uint8, device=dev)
            elif symbols is False:
                symbols = None
            lengths, edge_sums = (torch.zeros((n, n_paths), dtype=torch.int64, device=dev) for _ in range(2))
            found, depths, live = (torch.zeros(n, dtype=torch.int64, device=dev) for _ in range(3))
            stops = torch.zeros(n, dtype=torch.uint8, device=dev)
            self.bridge_kmers_device(seeds.data_ptr(), targets.data_ptr(), k, n, max_steps, None if symbols is None else symbols.data_ptr(),
                                     *[t.data_ptr() for t in (lengths, edge_sums, found, stops, depths, live)], min_steps=min_steps, max_paths=max_paths, max_live=max_live,
                                     direction=direction, min_count=min_count, min_edge=min_edge, stream=torch.cuda.current_stream(dev).cuda_stream)
            return symbols, lengths, edge_sums, found, stops, depths, live
        seeds, targets = (np.ascontiguousarray(a, dtype=np.uint64).reshape(-1) for a in (seeds, targets))
        n = len(seeds)
        if len(targets) != n:
            raise ValueError("one target a seed")
        if symbols is True:
            symbols = np.zeros((n, n_paths, n_steps), dtype=np.uint8)
        elif symbols is False:
            symbols = None
        elif symbols.dtype != np.uint8 or symbols.shape != (n, n_paths, n_steps) or not symbols.flags.c_contiguous:
            raise ValueError("symbols is a C-contiguous (n, max_paths, max_steps) uint8 array")
        lengths, edge_sums = (np.zeros((n, n_paths), dtype=np.uint64) for _ in range(2))
        found, depths, live = (np.zeros(n, dtype=np.uint64) for _ in range(3))
        stops = np.zeros(n, dtype=np.uint8)
        rc = _lib.lib().msbwt_rle_bridge_kmers(self._h, seeds.ctypes.data_as(C.c_void_p), targets.ctypes.data_as(C.c_void_p), int(k), n, int(min_count), int(min_edge or 0),
                                               direction, int(min_steps), n_steps, n_paths, int(max_live), None if symbols is None else symbols.ctypes.data_as(C.c_void_p),
                                               *[a.ctypes.data_as(C.c_void_p) for a in (lengths, edge_sums, found, stops, depths, live)])
        if rc:
            _raise(rc, self._h)
        return symbols, lengths, edge_sums, found, stops, depths, live

    def bridge_kmers_device(self, d_seeds, d_targets, k, n, max_steps, d_symbols, d_lengths, d_edge_sums, d_found, d_stops, d_depths, d_live, min_steps=0, max_paths=4,
                            max_live=64, direction=0, min_count=1, min_edge=None, stream=0):
        """msbwt_rle_bridge_kmers_device: device pointers (ints; every output may be None; the byte arrays at any alignment), direction
        as the header's number.  Synchronises `stream`; a device fault shows in device_status."""
        rc = _lib.lib().msbwt_rle_bridge_kmers_device(self._h, d_seeds, d_targets, int(k), int(n), int(min_count), int(min_edge or 0), int(direction), int(min_steps),
                                                      int(max_steps), int(max_paths), int(max_live), d_symbols, d_lengths, d_edge_sums, d_found, d_stops, d_depths, d_live,
                                                      stream)
        if rc:
            _raise(rc, self._h)

    def bridge_info(self):
        """What the last bridge call did: {"pairs", "rounds", "queries", "expanded", "found", "pieces", "scratch_bytes", "widest"}."""
        return self._info(_lib.lib().msbwt_rle_bridge_info, ("pairs", "rounds", "queries", "expanded", "found", "pieces", "scratch_bytes", "widest"))

    def set_bridge_slots(self, slots):
        """The frontier slots of a bridge call's piece (0 = automatic, 2^20; max_live where that is larger): results never depend on it."""
        rc = _lib.lib().msbwt_rle_set_bridge_slots(self._h, int(slots))
        if rc:
            _raise(rc, self._h)

    # ---- left walks: from BWT rows back to the text -- LF walks, locate, the reads themselves ----
    def walk_rows(self, rows, max_steps, symbols=True):
        """msbwt_rle_walk_rows -> (symbols, steps, stops, last, reads).  rows: n BWT rows.  Each is walked left by LF until it stands on
        a '$' or has taken max_steps steps (include/msbwt_hip.h, "left walks").  symbols: (n, max_steps) uint8 in WALK order -- row i
        holds steps[i] codes 1..5, the last symbol of the prefix first, and zeros (or what the `symbols` array passed in held) behind
        them; symbols=False: None, the call is locate.  stops: _lib.WALK_STOPS names the codes; last: the row a walk stands on; reads:
        the read for a DOLLAR stop (steps is then the offset in it), else 2^64 - 1.  A row at or beyond the total size stops BAD_ROW
        and raises MsbwtError(ERR_INVALID_RANGE).  walk_sequences turns rows into prefixes in reading order.
        numpy arrays go through the host form.  A torch tensor on this handle's device (int64 or uint64 words) goes through the
        _device form on torch's current stream, and torch tensors come back (words as int64); a bad row shows in device_status."""
        if hasattr(rows, "data_ptr"):
            import torch
            n, dev = int(rows.numel()), rows.device
            if not rows.is_contiguous() or rows.element_size() != 8:
                raise ValueError("rows is a contiguous tensor of n 64-bit words")
            if symbols is True:
                symbols = torch.zeros((n, int(max_steps)), dtype=torch.uint8, device=dev)
            elif symbols is False:
                symbols = None
            steps, last, reads = (torch.zeros(n, dtype=torch.int64, device=dev) for _ in range(3))
            stops = torch.zeros(n, dtype=torch.uint8, device=dev)
            self.walk_rows_device(rows.data_ptr(), n, max_steps, None if symbols is None else symbols.data_ptr(), steps.data_ptr(), stops.data_ptr(), last.data_ptr(),
                                  reads.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
            return symbols, steps, stops, last, reads
        rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
        n = len(rows)
        if symbols is True:
            symbols = np.zeros((n, int(max_steps)), dtype=np.uint8)
        elif symbols is False:
            symbols = None
        elif symbols.dtype != np.uint8 or symbols.shape != (n, int(max_steps)) or not symbols.flags.c_contiguous:
            raise ValueError("symbols is a C-contiguous (n, max_steps) uint8 array")
        steps, last, reads = (np.zeros(n, dtype=np.uint64) for _ in range(3))
        stops = np.zeros(n, dtype=np.uint8)
        rc = _lib.lib().msbwt_rle_walk_rows(self._h, rows.ctypes.data_as(C.c_void_p), n, int(max_steps), None if symbols is None else symbols.ctypes.data_as(C.c_void_p),
                                            *[a.ctypes.data_as(C.c_void_p) for a in (steps, stops, last, reads)])
        if rc:
            _raise(rc, self._h)
        return symbols, steps, stops, last, reads

    def walk_rows_device(self, d_rows, n, max_steps, d_symbols, d_steps, d_stops, d_last, d_reads, stream=0):
        """msbwt_rle_walk_rows_device: device pointers (ints; every output may be None; the rows of symbols at any alignment).
        Synchronises `stream`; a bad row shows in device_status."""
        rc = _lib.lib().msbwt_rle_walk_rows_device(self._h, d_rows, int(n), int(max_steps), d_symbols, d_steps, d_stops, d_last, d_reads, stream)
        if rc:
            _raise(rc, self._h)

    def locate_rows(self, rows, max_steps):
        """walk_rows without symbols -> (reads, offsets, stops): row i is the suffix at offsets[i] of read reads[i] where stops[i] is
        DOLLAR (1); elsewhere the walk did not reach the start of its read within max_steps and reads[i] is 2^64 - 1 (-1 in a tensor)."""
        _, steps, stops, _, reads = self.walk_rows(rows, max_steps, symbols=False)
        return reads, steps, stops

    def locate_kmer(self, kmer, max_steps):
        """Where a k-mer (symbol codes, uint8[k]) occurs: kmer_ranges, the rows of its range, locate_rows -> (reads, offsets), sorted by
        read and offset.  max_steps bounds the offsets that can be found; an occurrence further into its read raises MsbwtError."""
        l, h = self.kmer_ranges(np.ascontiguousarray(kmer, dtype=np.uint8).reshape(1, -1))
        reads, offsets, stops = self.locate_rows(np.arange(int(l[0]), int(h[0]), dtype=np.uint64), max_steps)
        if np.any(stops != _lib.WALK_STOPS.index("DOLLAR")):
            raise MsbwtError(_lib.ERR_INVALID_ARG, "locate_kmer: %d occurrences lie more than max_steps = %d symbols into their reads" % (int((stops != 1).sum()), max_steps))
        order = np.lexsort((offsets, reads))
        return reads[order], offsets[order]

    def extract_reads(self, read_ids=None, first=0, n=None, max_len=1024, truncate=False):
        """msbwt_rle_extract_reads -> (symbols, offsets): reads of the index as a ragged set in reading order, read j =
        symbols[offsets[j]:offsets[j + 1]] -- what count_ragged_read_kmers and build_from_reads take as they are.  read_ids: the reads
        wanted (each below get_symbol_count(0), repeats allowed), or None: the reads first .. first + n (n=None: all from `first` on).
        Read i is the i-th of the sorted read set (duplicates in input order).  A read longer than max_len comes back as its last
        max_len symbols with truncate=True and raises MsbwtError otherwise.  One walk: the buffer holds n x max_len symbols."""
        if read_ids is not None:
            ids = np.ascontiguousarray(read_ids, dtype=np.uint64).reshape(-1)
            n, where = len(ids), ids.ctypes.data_as(C.c_void_p)
        else:
            where = None
            if n is None:
                n = max(self.get_symbol_count(0) - int(first), 0)
        cap = int(n) * int(max_len)
        symbols = np.empty(max(cap, 1), dtype=np.uint8)
        offsets = np.zeros(int(n) + 1, dtype=np.uint64)
        total, truncated = C.c_uint64(0), C.c_uint64(0)
        rc = _lib.lib().msbwt_rle_extract_reads(self._h, where, int(first), int(n), int(max_len), symbols.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p),
                                                cap, C.byref(total), C.byref(truncated))
        if rc:
            _raise(rc, self._h)
        if truncated.value and not truncate:
            raise MsbwtError(_lib.ERR_INVALID_ARG, "extract_reads: %d reads are longer than max_len = %d (truncate=True keeps their last max_len symbols)"
                             % (truncated.value, max_len))
        return symbols[:total.value].copy(), offsets

    def extract_reads_device(self, d_read_ids, first, n, max_len, d_symbols, d_offsets, capacity_symbols, stream=0):
        """msbwt_rle_extract_reads_device: device pointers (ints; d_read_ids, d_symbols and d_offsets may each be None) -> (S, truncated).
        A capacity below S raises (the error carries .symbols = S).  Synchronises `stream`; a bad id shows in device_status."""
        total, truncated = C.c_uint64(0), C.c_uint64(0)
        rc = _lib.lib().msbwt_rle_extract_reads_device(self._h, d_read_ids, int(first), int(n), int(max_len), d_symbols, d_offsets, int(capacity_symbols), C.byref(total),
                                                       C.byref(truncated), stream)
        if rc:
            try:
                _raise(rc, self._h)
            except MsbwtError as e:
                e.symbols = int(total.value)
                raise
        return int(total.value), int(truncated.value)

    def walk_info(self):
        """What the last left-walk call did: {"walks", "steps", "dollar", "max_steps", "bad_row", "pieces", "scratch_bytes", "us"}."""
        return self._info(_lib.lib().msbwt_rle_walk_info, ("walks", "steps", "dollar", "max_steps", "bad_row", "pieces", "scratch_bytes", "us"))

    def set_walk_piece(self, walks):
        """Most left walks a launch takes (0 = automatic, 2^20; at most 2^28): results never depend on it."""
        rc = _lib.lib().msbwt_rle_set_walk_piece(self._h, int(walks))
        if rc:
            _raise(rc, self._h)

    # ---- read overlaps: the reads that begin with a suffix of a query, every length from one backward search ----
    def read_overlaps(self, reads, min_overlap, max_overlap=0, strand=0, records=True, ascii=False):
        """msbwt_rle_read_overlaps -> OverlapResult.  reads: the queries, as pack_reads takes them -- a list of strings (ascii=True) or of
        arrays of symbol codes, or a (symbols, offsets) pair of codes such as extract_reads returns.  Each is searched backwards
        (strand=1: its reverse complement), and for every length j >= min_overlap (and <= max_overlap, 0 = no limit) at which reads of
        the index begin with the query's last j symbols the result holds one record (length, first read, count): the records of query
        i are [offsets[i], offsets[i + 1]) of lengths / first / counts, in ascending length (include/msbwt_hip.h, "read overlaps").
        matched: the longest suffix found; edges: the sum of the query's counts; stops: _lib.OVERLAP_STOPS names the codes.
        records=False: a counting call, one search instead of two; lengths, first and counts are None.  A symbol that is no code 1..5
        stops its query BAD_SYMBOL and raises MsbwtError(ERR_INVALID_SYMBOL).  overlap_edges expands the result to edges."""
        flat, offsets = pack_reads(reads, ascii=ascii)
        if ascii:
            codes = np.empty_like(flat)
            _lib.lib().msbwt_convert_stoi(flat.ctypes.data_as(C.c_void_p), flat.size, codes.ctypes.data_as(C.c_void_p))
            flat = codes
        n = len(offsets) - 1
        out = OverlapResult(n, np.diff(offsets.astype(np.int64)).astype(np.uint64))
        total = C.c_uint64(0)

        def call(columns, capacity):
            return _lib.lib().msbwt_rle_read_overlaps(self._h, flat.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p), n, int(min_overlap), int(max_overlap),
                                                      int(strand), out.offsets.ctypes.data_as(C.c_void_p), *columns, capacity, C.byref(total),
                                                      out.matched.ctypes.data_as(C.c_void_p), out.edges.ctypes.data_as(C.c_void_p), out.stops.ctypes.data_as(C.c_void_p))

        rc = call((None, None, None), 0)
        if rc:
            _raise(rc, self._h)
        if records:
            R = int(total.value)
            out.lengths, out.first, out.counts = (np.zeros(R, dtype=np.uint64) for _ in range(3))
            if R:
                rc = call([a.ctypes.data_as(C.c_void_p) for a in (out.lengths, out.first, out.counts)], R)
                if rc:
                    _raise(rc, self._h)
        return out

    def read_overlaps_device(self, reads, offsets, min_overlap, max_overlap=0, strand=0, records=True, capacity=None):
        """msbwt_rle_read_overlaps_device on torch tensors of this handle's device, on torch's current stream -> OverlapResult of tensors
        (words as int64).  reads: uint8 symbol codes; offsets: n + 1 words (int64 or uint64), contiguous.  records=True counts first
        and fills tensors of exactly R records -- three searches in all -- unless `capacity` says how many records the columns are to
        hold: then one filling call, and MsbwtError (with .records = R) if R exceeds it.  A bad symbol shows in device_status."""
        import torch
        if not (reads.is_contiguous() and offsets.is_contiguous()) or reads.element_size() != 1 or offsets.element_size() != 8:
            raise ValueError("reads is a contiguous uint8 tensor, offsets a contiguous tensor of n + 1 64-bit words")
        n, dev = int(offsets.numel()) - 1, offsets.device
        stream = torch.cuda.current_stream(dev).cuda_stream
        out = OverlapResult(n, None, torch=torch, device=dev)
        total = C.c_uint64(0)

        def call(columns, cap):
            rc = _lib.lib().msbwt_rle_read_overlaps_device(self._h, reads.data_ptr() if reads.numel() else offsets.data_ptr(), offsets.data_ptr(), n, int(min_overlap),
                                                           int(max_overlap), int(strand), out.offsets.data_ptr(), *columns, cap, C.byref(total), out.matched.data_ptr(),
                                                           out.edges.data_ptr(), out.stops.data_ptr(), stream)
            if rc:
                try:
                    _raise(rc, self._h)
                except MsbwtError as e:
                    e.records = int(total.value)
                    raise

        if not records:
            call((None, None, None), 0)
        else:
            if capacity is None:
                call((None, None, None), 0)
                capacity = int(total.value)
            out.lengths, out.first, out.counts = (torch.zeros(max(int(capacity), 1), dtype=torch.int64, device=dev) for _ in range(3))
            call([a.data_ptr() for a in (out.lengths, out.first, out.counts)], int(capacity))
            R = int(total.value)
            out.lengths, out.first, out.counts = out.lengths[:R], out.first[:R], out.counts[:R]
        out.query_lengths = (offsets[1:] - offsets[:-1]) if n else offsets[:0]
        return out

    def overlap_info(self):
        """What the last read-overlap call did: {"queries", "symbols", "records", "edges", "end", "empty", "bad_symbol", "lines", "pieces",
        "scratch_bytes", "us", "piece_symbols", "piece_records"}."""
        return self._info(_lib.lib().msbwt_rle_overlap_info, ("queries", "symbols", "records", "edges", "end", "empty", "bad_symbol", "lines", "pieces", "scratch_bytes",
                                                              "us", "piece_symbols", "piece_records"))

    def set_overlap_piece(self, queries):
        """Most overlap queries a launch takes (0 = automatic, 2^20; at most 2^28): results never depend on it."""
        rc = _lib.lib().msbwt_rle_set_overlap_piece(self._h, int(queries))
        if rc:
            _raise(rc, self._h)

    def set_spectrum_frontier(self, nodes):
        """Most nodes per frontier buffer of the k-mer walks (0 = automatic, else at least _lib.SPECTRUM_MIN_FRONTIER): results never depend on it."""
        rc = _lib.lib().msbwt_rle_set_spectrum_frontier(self._h, int(nodes))
        if rc:
            _raise(rc, self._h)

    def spectrum_info(self):
        """What the last k-mer walk did: {"k", "seed_depth", "chunks", "retries", "descents", "nodes": uint64[33] per depth, "ms"}."""
        w = np.zeros(_lib.SPECTRUM_INFO_WORDS, dtype=np.uint64)
        rc = _lib.lib().msbwt_rle_spectrum_info(self._h, w.ctypes.data_as(C.c_void_p))
        if rc:
            _raise(rc, self._h)
        return {"k": int(w[0]), "seed_depth": int(w[1]), "chunks": int(w[2]), "retries": int(w[3]), "descents": int(w[39]), "nodes": w[4:37].copy(),
                "ms": int(w[38]) / 1000.0}

    # ---- batch forms -----------------------------------------------------------------
    def count_kmers(self, kmers, out=None):
        """kmers: (n, k) uint8 symbol codes -> uint64[n] (`out`: optional preallocated result array)."""
        a = np.ascontiguousarray(kmers, dtype=np.uint8)
        if a.ndim != 2:
            raise ValueError("kmers must be (n, k)")
        n, k = a.shape
        if out is None:
            out = np.empty(n, dtype=np.uint64)
        elif out.dtype != np.uint64 or out.shape != (n,) or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous uint64 array of length n")
        rc = _lib.lib().msbwt_rle_count_kmers(self._h, a.ctypes.data_as(C.c_void_p), k, n,
                                              out.ctypes.data_as(C.c_void_p))
        if rc:
            _raise(rc, self._h)
        return out

    def kmer_ranges(self, kmers):
        """kmers: (n, k) uint8 symbol codes -> (l, h), two uint64[n]: the FM range [l, h) of every k-mer
        (h - l == its count; (0, 0) when it does not occur; k = 0: [0, total))."""
        a = np.ascontiguousarray(kmers, dtype=np.uint8)
        if a.ndim != 2:
            raise ValueError("kmers must be (n, k)")
        n, k = a.shape
        ol = np.empty(n, dtype=np.uint64)
        oh = np.empty(n, dtype=np.uint64)
        rc = _lib.lib().msbwt_rle_kmer_ranges(self._h, a.ctypes.data_as(C.c_void_p), k, n,
                                              ol.ctypes.data_as(C.c_void_p), oh.ctypes.data_as(C.c_void_p))
        if rc:
            _raise(rc, self._h)
        return ol, oh

    def count_kmer_extensions(self, kmers):
        """kmers: (n, k) uint8 symbol codes -> uint64[n, 6]: out[i, c] = count_kmer([c] + row i), c = 0..5 ($ A C G N T)."""
        a = np.ascontiguousarray(kmers, dtype=np.uint8)
        if a.ndim != 2:
            raise ValueError("kmers must be (n, k)")
        n, k = a.shape
        out = np.empty((n, 6), dtype=np.uint64)
        rc = _lib.lib().msbwt_rle_count_kmer_extensions(self._h, a.ctypes.data_as(C.c_void_p), k, n,
                                                        out.ctypes.data_as(C.c_void_p))
        if rc:
            _raise(rc, self._h)
        return out

    def constrain_ranges(self, syms, l, h):
        s = np.ascontiguousarray(syms, dtype=np.uint8)
        l = np.ascontiguousarray(l, dtype=np.uint64)
        h = np.ascontiguousarray(h, dtype=np.uint64)
        if not (s.shape == l.shape == h.shape and s.ndim == 1):
            raise ValueError("syms, l, h must be 1-D and equally long")
        ol = np.empty(s.size, dtype=np.uint64)
        oh = np.empty(s.size, dtype=np.uint64)
        rc = _lib.lib().msbwt_rle_constrain_ranges(self._h, s.ctypes.data_as(C.c_void_p),
                                                   l.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p),
                                                   s.size, ol.ctypes.data_as(C.c_void_p), oh.ctypes.data_as(C.c_void_p))
        if rc:
            _raise(rc, self._h)
        return ol, oh

    def count_read_kmers(self, reads, k, ascii=None, forward=True, revcomp=False, out_fwd=None, out_rc=None):
        """Counts every k-mer window of every read, fused on the GPU (no n x k query matrix).

        reads: (n_reads, read_len) uint8 -- symbol codes, or ASCII bytes (`ascii=True`; a list of
        equal-length str/bytes is accepted and implies ASCII).  Returns (fwd, rc): uint64 arrays
        of shape (n_reads, read_len - k + 1), `None` for a strand that was not requested.
        rc[r, w] = count_kmer(reverse_complement_i(window))."""
        if not isinstance(reads, np.ndarray):
            reads = np.array([np.frombuffer(r.encode() if isinstance(r, str) else bytes(r), dtype=np.uint8) for r in reads])
            ascii = True if ascii is None else ascii
        a = np.ascontiguousarray(reads, dtype=np.uint8)
        if a.ndim != 2:
            raise ValueError("reads must be (n_reads, read_len)")
        n, length = a.shape
        w = length - k + 1
        fwd = (out_fwd if out_fwd is not None else np.empty((n, max(w, 0)), dtype=np.uint64)) if forward else None
        rc = (out_rc if out_rc is not None else np.empty((n, max(w, 0)), dtype=np.uint64)) if revcomp else None
        for o in (fwd, rc):
            if o is not None and (o.dtype != np.uint64 or o.shape != (n, max(w, 0)) or not o.flags.c_contiguous):
                raise ValueError("output arrays must be contiguous uint64 of shape (n_reads, read_len - k + 1)")
        code = _lib.lib().msbwt_rle_count_read_kmers(
            self._h, a.ctypes.data_as(C.c_void_p), length, n, k, 1 if ascii else 0,
            fwd.ctypes.data_as(C.c_void_p) if fwd is not None else None,
            rc.ctypes.data_as(C.c_void_p) if rc is not None else None)
        if code:
            _raise(code, self._h)
        return fwd, rc

    def count_ragged_read_kmers(self, reads, k, ascii=True, forward=True, revcomp=False):
        """Like count_read_kmers for reads of different lengths.  `reads`: list of str/bytes (ASCII)
        or of uint8 arrays (codes when ascii=False).  Returns (fwd, rc, window_offsets): flat
        uint64 arrays in read order, read r owning [window_offsets[r], window_offsets[r+1])."""
        arrs = [np.frombuffer(r.encode() if isinstance(r, str) else bytes(r), dtype=np.uint8)
                if isinstance(r, (str, bytes, bytearray)) else np.asarray(r, dtype=np.uint8) for r in reads]
        lens = np.array([len(a) for a in arrs], dtype=np.uint64)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        flat = np.ascontiguousarray(np.concatenate(arrs)) if arrs else np.zeros(0, dtype=np.uint8)
        woff = np.concatenate([[0], np.cumsum(np.where(lens >= k, lens - np.uint64(k) + np.uint64(1), 0))]).astype(np.uint64)
        total = int(woff[-1])
        fwd = np.empty(total, dtype=np.uint64) if forward else None
        rc = np.empty(total, dtype=np.uint64) if revcomp else None
        got = C.c_uint64()
        code = _lib.lib().msbwt_rle_count_ragged_read_kmers(
            self._h, flat.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p), len(arrs), k,
            1 if ascii else 0, fwd.ctypes.data_as(C.c_void_p) if fwd is not None else None,
            rc.ctypes.data_as(C.c_void_p) if rc is not None else None, C.byref(got))
        if code:
            _raise(code, self._h)
        assert int(got.value) == total
        return fwd, rc, woff

    def count_read_kmers_device(self, d_reads, read_len, n_reads, k, ascii, d_out_fwd, d_out_rc, stream=0):
        code = _lib.lib().msbwt_rle_count_read_kmers_device(self._h, d_reads, read_len, n_reads, k,
                                                            1 if ascii else 0, d_out_fwd, d_out_rc, stream)
        if code:
            _raise(code, self._h)

    def count_kmers_device(self, d_kmers, k, n, d_out, stream=0):
        """Device pointers (ints); asynchronous on `stream` (a hipStream_t as int)."""
        rc = _lib.lib().msbwt_rle_count_kmers_device(self._h, d_kmers, k, n, d_out, stream)
        if rc:
            _raise(rc, self._h)

    def kmer_ranges_device(self, d_kmers, k, n, d_out_l, d_out_h, stream=0):
        """Device pointers (ints): n x k symbol codes -> l, h (n u64 each); asynchronous on `stream`."""
        rc = _lib.lib().msbwt_rle_kmer_ranges_device(self._h, d_kmers, k, n, d_out_l, d_out_h, stream)
        if rc:
            _raise(rc, self._h)

    def count_kmer_extensions_device(self, d_kmers, k, n, d_out, stream=0):
        """Device pointers (ints): n x k symbol codes -> n x 6 u64 left-extension counts; asynchronous on `stream`."""
        rc = _lib.lib().msbwt_rle_count_kmer_extensions_device(self._h, d_kmers, k, n, d_out, stream)
        if rc:
            _raise(rc, self._h)

    def constrain_ranges_device(self, d_syms, d_l, d_h, n, d_out_l, d_out_h, stream=0):
        rc = _lib.lib().msbwt_rle_constrain_ranges_device(self._h, d_syms, d_l, d_h, n, d_out_l, d_out_h, stream)
        if rc:
            _raise(rc, self._h)

    def device_status(self, stream=0):
        """Synchronises `stream` and raises if a device batch saw invalid input."""
        rc = _lib.lib().msbwt_rle_device_status(self._h, stream)
        if rc:
            _raise(rc, self._h)

    def count_kmers_packed(self, words, k, count_bits=64, out=None):
        """msbwt_rle_count_kmers_packed: `words` = (n, ceil(k / 32)) uint64, two bits per symbol (pack_2bit); returns uint64[n]
        or, with count_bits=32, uint32[n] (`out`: optional preallocated result array of that type)."""
        w = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, 2 if k > 32 else 1)
        want = np.uint64 if count_bits == 64 else np.uint32
        if out is None:
            out = np.empty(len(w), dtype=want)
        elif out.dtype != want or out.shape != (len(w),) or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous array of n counts of the requested width")
        rc = _lib.lib().msbwt_rle_count_kmers_packed(self._h, w.ctypes.data_as(C.c_void_p), k, len(w), out.ctypes.data_as(C.c_void_p), count_bits)
        if rc:
            _raise(rc, self._h)
        return out

    def count_kmers_packed_device(self, d_words, k, n, d_out, stream=0):
        rc = _lib.lib().msbwt_rle_count_kmers_packed_device(self._h, d_words, k, n, d_out, stream)
        if rc:
            _raise(rc, self._h)

    def set_batch_order(self, mode):
        """-1 = automatic (default; today that means never, include/msbwt_hip.h), 0 = never, 1 = whenever the pass applies."""
        rc = _lib.lib().msbwt_rle_set_batch_order(self._h, int(mode))
        if rc:
            _raise(rc, self._h)

    def get_batch_order(self):
        return int(_lib.lib().msbwt_rle_get_batch_order(self._h))

    def batch_order_for(self, k, n):
        rc = int(_lib.lib().msbwt_rle_batch_order_for(self._h, int(k), int(n)))
        if rc < 0:
            _raise(rc, self._h)
        return bool(rc)

    def kmer_order_keys_device(self, d_kmers, k, n, d_out_keys, stream=0):
        """msbwt_rle_kmer_order_keys_device: u64 keys (device pointers); a batch sorted by them ascending walks the index in order."""
        rc = _lib.lib().msbwt_rle_kmer_order_keys_device(self._h, d_kmers, k, n, d_out_keys, stream)
        if rc:
            _raise(rc, self._h)

    def allgather_counts(self, comm, d_mine, n_mine, d_all, wire_bits=64, stream=0):
        """msbwt_rle_allgather_counts: d_all[r * n_mine + i] = rank r's d_mine[i] on every rank (device pointers,
        u64 counts), asynchronous on `stream`; wire_bits 16 / 32 narrows the payload (overflow -> device_status)."""
        rc = _lib.lib().msbwt_rle_allgather_counts(self._h, comm._c, d_mine, n_mine, d_all, wire_bits, stream)
        if rc:
            _raise(rc, self._h)

    def count_kmers_allgather_device(self, comm, d_kmers, k, n_mine, d_mine_counts, d_all, wire_bits=16, out_bits=64, pieces=4, stream=0):
        """msbwt_rle_count_kmers_allgather_device: this rank's shard counted piece by piece on `stream` while the finished pieces' counts
        are all-gathered on a second stream; d_all[r * n_mine + i] as out_bits-wide integers (64 or the wire width)."""
        rc = _lib.lib().msbwt_rle_count_kmers_allgather_device(self._h, comm._c, d_kmers, k, n_mine, d_mine_counts, d_all, wire_bits, out_bits, pieces, stream)
        if rc:
            _raise(rc, self._h)

    # ---- several GPUs of one node ---------------------------------------------------------
    def replicate(self, device):
        """A new RleBWT on `device` holding a GPU -> GPU copy of this index (no rebuild, no upload)."""
        h = _lib.lib().msbwt_rle_replicate(self._h, device)
        if not h:
            _raise(_lib.ERR_HIP, self._h)
        other = object.__new__(RleBWT)
        other._h = h
        other.bin_power = self.bin_power
        return other

    # ---- tuning / introspection --------------------------------------------------------
    def set_table_depth(self, depth):
        rc = _lib.lib().msbwt_rle_set_table_depth(self._h, depth)
        if rc:
            _raise(rc, self._h)

    def get_table_depth(self):
        return int(_lib.lib().msbwt_rle_get_table_depth(self._h))

    def set_table_packed(self, mode):
        """1 = packed table two levels deeper whenever a pair index exists, 0 = flat table only, -1 = automatic."""
        rc = _lib.lib().msbwt_rle_set_table_packed(self._h, mode)
        if rc:
            _raise(rc, self._h)

    def get_table_packed(self):
        return bool(_lib.lib().msbwt_rle_get_table_packed(self._h))

    def set_memory_budget(self, nbytes):
        """HBM the loaded index may hold (0 = no budget); rebuilds the optional structures of a loaded index under it."""
        rc = _lib.lib().msbwt_rle_set_memory_budget(self._h, int(nbytes))
        if rc:
            _raise(rc, self._h)

    def get_memory_budget(self):
        return int(_lib.lib().msbwt_rle_get_memory_budget(self._h))

    def set_table_side(self, mode):
        """1 = escape lines of the packed table keep flat entries in a side array (default), 0 = their queries search from scratch."""
        rc = _lib.lib().msbwt_rle_set_table_side(self._h, int(mode))
        if rc:
            _raise(rc, self._h)

    def table_info(self):
        """{"lines", "escape_lines", "side_bytes"} of the packed table in HBM (zeros without one)."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        rc = _lib.lib().msbwt_rle_table_info(self._h, C.byref(a), C.byref(b), C.byref(c))
        if rc:
            _raise(rc, self._h)
        return {"lines": a.value, "escape_lines": b.value, "side_bytes": c.value}

    COUNTER_NAMES = ("wave_steps", "lane_steps", "pair_steps", "second_lines", "sat_out", "escape_queries", "escape_restarts",
                     "table_decided", "searched", "first_lines", "table_steps", "table_displaced", "table_rides", "waves_worked", "tier_fallbacks")

    # ---- sparse suffix table (include/msbwt_hip.h, msbwt_rle_set_sparse_table) ----
    def set_sparse_table(self, depth):
        """-1 = automatic (default), 0 = off, 16..31 = exactly that depth (29: at least 2^29 buckets, 69 GB)."""
        rc = _lib.lib().msbwt_rle_set_sparse_table(self._h, int(depth))
        if rc:
            _raise(rc, self._h)

    def set_query_length(self, k):
        """The k this index will mostly be asked about (0 = unknown): the AUTOMATIC sparse table goes as deep as min(k, 31) -- where its table fits -- instead of 23
        -- a table of d-mers serves k >= d only.  Results never depend on it."""
        rc = _lib.lib().msbwt_rle_set_query_length(self._h, int(k))
        if rc:
            _raise(rc, self._h)

    def get_query_length(self):
        return int(_lib.lib().msbwt_rle_get_query_length(self._h))

    def set_sparse_tiers(self, mode):
        """Two-tier form of the sparse table (entries for the suffixes that occur at least twice, filter bits for the rest -- read sets with
        errors): -1 = where the complete table of a depth does not fit (default), 0 = never, 1 = always.  Results never depend on it."""
        rc = _lib.lib().msbwt_rle_set_sparse_tiers(self._h, int(mode))
        if rc:
            _raise(rc, self._h)

    def set_sparse_second(self, mode):
        """The second, shallower sparse level (17-symbol suffixes, for k undeclared): -1 = automatic (default), 0 = never."""
        rc = _lib.lib().msbwt_rle_set_sparse_second(self._h, int(mode))
        if rc:
            _raise(rc, self._h)

    def get_sparse_tiers(self):
        """True when the sparse table in HBM is of the two-tier form."""
        return bool(_lib.lib().msbwt_rle_get_sparse_tiers(self._h))

    def get_sparse_table(self):
        """Depth of the sparse suffix table in HBM, 0 = none."""
        return int(_lib.lib().msbwt_rle_get_sparse_table(self._h))

    def sparse_table_info(self):
        """What msbwt_rle_sparse_table_info reports, by name; "distinct" / "wide": {depth: count} for the depths the build passed."""
        out = (C.c_uint64 * _lib.SPARSE_INFO_WORDS)()
        rc = _lib.lib().msbwt_rle_sparse_table_info(self._h, out)
        if rc:
            _raise(rc, self._h)
        info = {"depth": int(out[0]), "entries": int(out[1]), "buckets": int(out[2]), "bytes": int(out[3]), "side_entries": int(out[4]),
                "side_bytes": int(out[5]), "displaced": int(out[6]), "parent_depth": int(out[7]), "two_tier": bool(out[8]), "probe": int(out[9]),
                "filtered": int(out[42]), "second_depth": int(out[43]), "second_bytes": int(out[44]),
                "second_tier": bool(out[112]),
                "sizing_chunks": int(out[113]), "sizing_retries": int(out[114]), "sizing_descents": int(out[115]),
                "fill_chunks": int(out[116]), "fill_retries": int(out[117]), "fill_descents": int(out[118])}
        info["distinct"] = {d: int(out[10 + d]) for d in range(32) if out[10 + d]}
        info["wide"] = {d: int(out[45 + d]) for d in range(32) if out[10 + d]}
        info["once"] = {d: int(out[80 + d]) for d in range(32) if out[10 + d]}
        return info

    def download_sparse_table(self):
        """(lines, side): the bucket lines as a (nlines, 32) uint32 array and the side array as (n, 2) uint64 -- for tests."""
        info = self.sparse_table_info()
        if not info["depth"]:
            return None, None
        lines = np.empty((info["bytes"] // 128, 32), dtype=np.uint32)
        side = np.empty((info["side_bytes"] // 16, 2), dtype=np.uint64)
        got = _lib.lib().msbwt_rle_download_sparse_table(self._h, lines.ctypes.data_as(C.c_void_p), lines.nbytes,
                                                         side.ctypes.data_as(C.c_void_p) if side.size else None, side.nbytes)
        if got == _lib.SIZE_MAX:
            _raise(_lib.ERR_HIP, self._h)
        return lines, side

    def set_search_counters(self, enabled):
        rc = _lib.lib().msbwt_rle_set_search_counters(self._h, 1 if enabled else 0)
        if rc:
            _raise(rc, self._h)

    def search_counters(self, stream=0):
        """The counters of the launches since the last call, by name (include/msbwt_hip.h); reads and zeroes them."""
        out = (C.c_uint64 * 16)()
        rc = _lib.lib().msbwt_rle_search_counters(self._h, out, stream)
        if rc:
            _raise(rc, self._h)
        return {name: int(out[i]) for i, name in enumerate(self.COUNTER_NAMES)}

    def set_presence_filter(self, mode):
        """0 = no presence filter, anything else = automatic (kept when it can reject something)."""
        rc = _lib.lib().msbwt_rle_set_presence_filter(self._h, mode)
        if rc:
            _raise(rc, self._h)

    def get_presence_filter(self):
        """Depth of the L2-resident presence filter in front of the suffix table, 0 if none."""
        return int(_lib.lib().msbwt_rle_get_presence_filter(self._h))

    def set_pair_index(self, mode):
        """1 = build the two-symbols-per-step index, 0 = drop it, -1 = automatic (default)."""
        rc = _lib.lib().msbwt_rle_set_pair_index(self._h, mode)
        if rc:
            _raise(rc, self._h)

    def get_pair_index(self):
        return bool(_lib.lib().msbwt_rle_get_pair_index(self._h))

    def set_pair_stride(self, stride):
        """128 = disjoint pair blocks, 96 = overlapping (one line for ranges up to 32 wide), 0 = automatic."""
        rc = _lib.lib().msbwt_rle_set_pair_stride(self._h, stride)
        if rc:
            _raise(rc, self._h)

    def get_pair_stride(self):
        return int(_lib.lib().msbwt_rle_get_pair_stride(self._h))

    def get_typical_range_width(self):
        """Median number of occurrences of a present 24-mer, probed at load time (-1.0: not probed)."""
        return float(_lib.lib().msbwt_rle_get_typical_range_width(self._h))

    BLOCK_FORMATS = {"planes": 0, "runs": 1}

    def set_block_format(self, fmt):
        """"planes" (default) or "runs" (memory-lean run blocks, no pair index); takes effect at the next load."""
        rc = _lib.lib().msbwt_rle_set_block_format(self._h, self.BLOCK_FORMATS.get(fmt, fmt))
        if rc:
            _raise(rc, self._h)

    def get_block_format(self):
        return {v: k for k, v in self.BLOCK_FORMATS.items()}[int(_lib.lib().msbwt_rle_get_block_format(self._h))]

    SEARCH_KERNELS = {"auto": 0, "groups": 1, "lanes": 2}

    def set_search_kernel(self, mode):
        """"auto" (default), "groups" (8 lanes per query) or "lanes" (one query per lane, LDS-staged lines)."""
        rc = _lib.lib().msbwt_rle_set_search_kernel(self._h, self.SEARCH_KERNELS.get(mode, mode))
        if rc:
            _raise(rc, self._h)

    def get_search_kernel(self):
        return {v: k for k, v in self.SEARCH_KERNELS.items()}[int(_lib.lib().msbwt_rle_get_search_kernel(self._h))]

    def search_kernel_for(self, k):
        """The kernel a batch of k-symbol queries runs on right now: "lanes", "groups" or "generic" (k > 64)."""
        rc = int(_lib.lib().msbwt_rle_search_kernel_for(self._h, int(k)))
        if rc < 0:
            _raise(rc, self._h)
        return {0: "generic", 1: "groups", 2: "lanes"}[rc]

    def set_line_streaming(self, mode):
        """-1 = automatic (index lines are fetched non-temporally once the random-access arrays reach 4 GiB), 0 = never, 1 = always."""
        rc = _lib.lib().msbwt_rle_set_line_streaming(self._h, int(mode))
        if rc:
            _raise(rc, self._h)

    def get_line_streaming(self):
        return bool(_lib.lib().msbwt_rle_get_line_streaming(self._h))

    PROBE_ARRAYS = {"blocks": 0, "pair_blocks": 1, "sparse_table": 2, "table": 3}

    def probe_line_rate(self, which):
        """Random 128-byte lines per second served right now from one of the index's arrays ("blocks", "pair_blocks",
        "sparse_table", "table"); 0.0 if there is no such array.  A placement diagnostic (msbwt_rle_probe_line_rate)."""
        out = C.c_double()
        rc = _lib.lib().msbwt_rle_probe_line_rate(self._h, self.PROBE_ARRAYS.get(which, which), C.byref(out))
        if rc:
            _raise(rc, self._h)
        return float(out.value)

    def device_bytes(self):
        return int(_lib.lib().msbwt_rle_device_bytes(self._h))

    def set_kernel_timing(self, enabled):
        _lib.lib().msbwt_rle_set_kernel_timing(self._h, 1 if enabled else 0)

    def kernel_time_ms(self):
        """(average ms per count-kernel launch, launches) since the last call; HIP events."""
        avg, cnt = C.c_double(), C.c_uint64()
        rc = _lib.lib().msbwt_rle_kernel_time_ms(self._h, C.byref(avg), C.byref(cnt))
        if rc:
            _raise(rc, self._h)
        return float(avg.value), int(cnt.value)

    def device_ordinal(self):
        return int(_lib.lib().msbwt_rle_device_ordinal(self._h))


class RankComm:
    """An RCCL communicator over the GPUs of a one-process-per-GPU job, made through the library
    (msbwt_comm_*): rank 0 calls RankComm.unique_id(), the bytes reach the other ranks by any channel
    (torch.distributed.broadcast in bench.py), every rank calls RankComm(nranks, id, rank) with its GPU current."""

    @staticmethod
    def unique_id():
        buf = (C.c_uint8 * _lib.COMM_ID_BYTES)()
        rc = _lib.lib().msbwt_comm_get_unique_id(buf)
        if rc:
            raise MsbwtError(rc, "msbwt_comm_get_unique_id (is librccl.so there?)")
        return bytes(buf)

    def __init__(self, nranks, unique_id, rank):
        self._c = C.c_void_p()
        self.nranks, self.rank = nranks, rank
        buf = (C.c_uint8 * _lib.COMM_ID_BYTES).from_buffer_copy(unique_id)
        rc = _lib.lib().msbwt_comm_init_rank(C.byref(self._c), nranks, buf, rank)
        if rc:
            raise MsbwtError(rc, "msbwt_comm_init_rank")

    def close(self):
        c, self._c = self._c, None
        if c:
            _lib.lib().msbwt_comm_destroy(c)

    def __del__(self):
        try:
            self.close()
        except (TypeError, AttributeError):
            pass


def kmer_order_keys(kmers):
    """msbwt_kmer_order_keys (host): the u64 key of every row of an (n, k) matrix of symbol codes; sort a batch by it
    (ascending) and its queries read the suffix table, and then the index, in ascending order."""
    a = np.ascontiguousarray(kmers, dtype=np.uint8)
    if a.ndim != 2:
        raise ValueError("kmers must be (n, k)")
    n, k = a.shape
    out = np.empty(n, dtype=np.uint64)
    rc = _lib.lib().msbwt_kmer_order_keys(a.ctypes.data_as(C.c_void_p), k, n, out.ctypes.data_as(C.c_void_p))
    if rc:
        raise MsbwtError(rc, "msbwt_kmer_order_keys")
    return out


def _handles(replicas):
    arr = (C.c_void_p * len(replicas))(*[r._h for r in replicas])
    return arr


def count_kmers_multi(replicas, kmers, out=None):
    """msbwt_rle_count_kmers_multi: a host batch sharded over the replicas (one per GPU)."""
    a = np.ascontiguousarray(kmers, dtype=np.uint8)
    if a.ndim != 2:
        raise ValueError("kmers must be (n, k)")
    n, k = a.shape
    if out is None:
        out = np.empty(n, dtype=np.uint64)
    rc = _lib.lib().msbwt_rle_count_kmers_multi(_handles(replicas), len(replicas), a.ctypes.data_as(C.c_void_p), k, n,
                                                out.ctypes.data_as(C.c_void_p))
    if rc:
        raise MsbwtError(rc, "; ".join(_lib.lib().msbwt_rle_last_error(r._h).decode(errors="replace") for r in replicas))
    return out


def pack_2bit(kmers):
    """(n, k) symbol codes over ACGT -> (n, ceil(k / 32)) uint64 words (msbwt_kmers_pack_2bit; include/msbwt_hip.h has the layout)."""
    a = np.ascontiguousarray(kmers, dtype=np.uint8)
    if a.ndim != 2:
        raise ValueError("kmers must be (n, k)")
    n, k = a.shape
    out = np.empty((n, 2 if k > 32 else 1), dtype=np.uint64)
    rc = _lib.lib().msbwt_kmers_pack_2bit(a.ctypes.data_as(C.c_void_p), k, n, out.ctypes.data_as(C.c_void_p))
    if rc:
        raise MsbwtError(rc, "a symbol outside A C G T cannot be packed into two bits")
    return out


def unpack_2bit(words, k):
    """uint64[n] 2-bit words of k-mers, k <= 32 (pack_2bit's layout: first symbol most significant, last in bits 0-1) -> (n, k) symbol
    codes (A C G T = 1 2 3 5)."""
    if not 1 <= k <= 32:
        raise ValueError("unpack_2bit takes one word per k-mer: 1 <= k <= 32")
    w = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
    shifts = (2 * np.arange(k - 1, -1, -1)).astype(np.uint64)
    return np.array([1, 2, 3, 5], dtype=np.uint8)[((w[:, None] >> shifts[None, :]) & np.uint64(3)).astype(np.intp)]


def trace_sequences(seeds, k, symbols, steps, direction="right", text=False):
    """The full sequence of every walk of RleBWT.trace_kmers, in reading order: the seed followed by its steps[i] symbols ("right"), or
    those symbols reversed followed by the seed ("left") -> a list of uint8 arrays of symbol codes, or (text=True) of str."""
    if direction not in _lib.TRACE_DIRECTIONS:
        raise ValueError("direction is 'right' or 'left'")
    heads = unpack_2bit(np.asarray(seeds, dtype=np.uint64) & np.uint64((1 << (2 * int(k))) - 1), int(k))
    symbols, steps = np.asarray(symbols, dtype=np.uint8), np.asarray(steps, dtype=np.uint64).reshape(-1)
    if symbols.ndim != 2 or len(symbols) != len(heads) or len(steps) != len(heads) or (len(steps) and int(steps.max()) > symbols.shape[1]):
        raise ValueError("symbols is (n, max_steps) and steps[i] <= max_steps")
    out = []
    for head, row, s in zip(heads, symbols, steps):
        row = row[:int(s)]
        out.append(np.concatenate([head, row]) if direction == "right" else np.concatenate([row[::-1], head]))
    if not text:
        return out
    return [_LETTERS[a].tobytes().decode() for a in out]


def bridge_sequences(seeds, k, symbols, lengths, direction="right", text=False):
    """The full sequence of every written bridge of RleBWT.bridge_kmers, in reading order: per pair a list with, for each row j of
    lengths[i, j] > 0 symbols, the seed followed by them ("right") or those symbols reversed followed by the seed ("left") -> lists of
    uint8 arrays of symbol codes, or (text=True) of str.  (A bridge has at least one symbol, so a length of 0 is an unused row.)"""
    if direction not in _lib.TRACE_DIRECTIONS:
        raise ValueError("direction is 'right' or 'left'")
    heads = unpack_2bit(np.asarray(seeds, dtype=np.uint64) & np.uint64((1 << (2 * int(k))) - 1), int(k))
    symbols, lengths = np.asarray(symbols, dtype=np.uint8), np.asarray(lengths, dtype=np.uint64)
    if symbols.ndim != 3 or lengths.shape != symbols.shape[:2] or len(symbols) != len(heads) or (lengths.size and int(lengths.max()) > symbols.shape[2]):
        raise ValueError("symbols is (n, max_paths, max_steps), lengths (n, max_paths) and lengths[i, j] <= max_steps")
    out = []
    for head, rows, lens in zip(heads, symbols, lengths):
        found = [row[:int(s)] for row, s in zip(rows, lens) if s]
        out.append([np.concatenate([head, row]) if direction == "right" else np.concatenate([row[::-1], head]) for row in found])
    if not text:
        return out
    return [[_LETTERS[a].tobytes().decode() for a in rows] for rows in out]


def bridge_plan(n, max_steps, max_paths=4, max_live=64, host=True, slots=0):
    """msbwt_bridge_plan: the bytes of HBM scratch a bridge call of n pairs allocates (and frees again) on an index that holds something."""
    out = C.c_uint64(0)
    rc = _lib.lib().msbwt_bridge_plan(int(n), int(max_steps), int(max_paths), int(max_live), int(bool(host)), int(slots), C.byref(out))
    if rc:
        raise MsbwtError(rc, "msbwt_bridge_plan: max_paths and max_live are at least 1, slots at most 2^28, max_steps at most 4096, max_live at most 2^24, "
                             "and n x max_paths x max_steps must stay below 2^40")
    return out.value


def canonical_trace_plan(n, max_steps, mode="unique", targets=False, host=True, piece=0):
    """msbwt_canonical_trace_plan: the bytes of HBM scratch a canonical trace call of n walks allocates (and frees again) on an index that holds something."""
    out = C.c_uint64(0)
    rc = _lib.lib().msbwt_canonical_trace_plan(int(n), int(max_steps), _lib.TRACE_MODES[mode], int(bool(targets)), int(bool(host)), int(piece), C.byref(out))
    if rc:
        raise MsbwtError(rc, "msbwt_canonical_trace_plan: max_steps and n x max_steps must stay below 2^40")
    return out.value


def walk_plan(n, max_steps, symbols=True, host=True, piece=0):
    """msbwt_walk_plan: the bytes of HBM scratch a RleBWT.walk_rows call of n walks allocates (and frees again) on an index that holds
    something; symbols=False: locate.  The device form allocates its counters only."""
    out = C.c_uint64(0)
    rc = _lib.lib().msbwt_walk_plan(int(n), int(max_steps), int(bool(symbols)), int(bool(host)), int(piece), C.byref(out))
    if rc:
        raise MsbwtError(rc, "msbwt_walk_plan: max_steps and n x max_steps must stay below 2^40, a piece is at most 2^28 walks")
    return out.value


def walk_sequences(symbols, steps, text=False):
    """The prefixes the walks of RleBWT.walk_rows went through, in READING order: for walk i the first steps[i] symbols of row i of
    `symbols` reversed -- the read's prefix [0, steps[i]) for a walk that stopped DOLLAR.  A list of uint8 arrays of symbol codes, or
    of str with text=True.  Pure host logic."""
    symbols = np.ascontiguousarray(symbols.cpu().numpy() if hasattr(symbols, "data_ptr") else symbols, dtype=np.uint8)
    steps = np.ascontiguousarray(steps.cpu().numpy() if hasattr(steps, "data_ptr") else steps).astype(np.uint64).reshape(-1)
    if symbols.ndim != 2 or symbols.shape[0] != steps.size or (steps.size and int(steps.max()) > symbols.shape[1]):
        raise ValueError("symbols is (n, max_steps) and steps[i] <= max_steps")
    out = [row[:int(s)][::-1].copy() for row, s in zip(symbols, steps)]
    if not text:
        return out
    return [_LETTERS[a].tobytes().decode() for a in out]


class OverlapResult:
    """What RleBWT.read_overlaps returns: offsets (n + 1), the record columns lengths / first / counts (None for a counting call),
    matched, edges, stops (n each) and query_lengths.  numpy arrays from the host form, torch tensors (words as int64) from the
    device form."""

    def __init__(self, n, query_lengths, torch=None, device=None):
        self.query_lengths = query_lengths
        self.lengths = self.first = self.counts = None
        if torch is None:
            self.offsets = np.zeros(n + 1, dtype=np.uint64)
            self.matched, self.edges = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
            self.stops = np.zeros(n, dtype=np.uint8)
        else:
            self.offsets = torch.zeros(n + 1, dtype=torch.int64, device=device)
            self.matched, self.edges = torch.zeros(n, dtype=torch.int64, device=device), torch.zeros(n, dtype=torch.int64, device=device)
            self.stops = torch.zeros(n, dtype=torch.uint8, device=device)


def overlap_edges(result, query_ids=None, drop_self=True, drop_contained=False):
    """The records of an OverlapResult expanded to edges: an (E, 3) uint64 array of (query, read, length) rows, by query, then length,
    then read.  query_ids: the read id of each query where the queries are reads of the index (extract_reads order: the ids
    themselves); with it, drop_self removes (i, query_ids[i], L_i), the query found as itself.  drop_contained removes every edge
    whose length equals its query's length: the reads that hold the whole query as a prefix, duplicates and self included.  Pure
    host logic in numpy."""
    def host(a):
        return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "data_ptr") else a).astype(np.uint64).reshape(-1)

    if result.lengths is None:
        raise ValueError("overlap_edges needs the records: read_overlaps(..., records=True)")
    offsets, lengths, first, counts, qlen = host(result.offsets), host(result.lengths), host(result.first), host(result.counts), host(result.query_lengths)
    per_query = np.diff(offsets.astype(np.int64))
    rec_query = np.repeat(np.arange(per_query.size, dtype=np.uint64), per_query)
    c = counts.astype(np.int64)
    query = np.repeat(rec_query, c)
    length = np.repeat(lengths, c)
    starts = np.cumsum(c) - c
    read = np.repeat(first, c) + (np.arange(int(c.sum()), dtype=np.int64) - np.repeat(starts, c)).astype(np.uint64)
    keep = np.ones(query.size, dtype=bool)
    whole = length == qlen[query.astype(np.int64)] if query.size else keep
    if drop_contained:
        keep &= ~whole
    elif drop_self and query_ids is not None:
        ids = host(query_ids)
        keep &= ~(whole & (read == ids[query.astype(np.int64)]))
    return np.stack([query[keep], read[keep], length[keep]], axis=1) if query.size else np.zeros((0, 3), dtype=np.uint64)


def overlap_plan(n, host=True, piece=0, piece_symbols=0, piece_records=0):
    """msbwt_overlap_plan: the peak bytes of HBM scratch a RleBWT.read_overlaps call of n queries allocates (and frees again) on an
    index that holds something; piece_symbols / piece_records: overlap_info's words of the same names (host form)."""
    out = C.c_uint64(0)
    rc = _lib.lib().msbwt_overlap_plan(int(n), int(bool(host)), int(piece), int(piece_symbols), int(piece_records), C.byref(out))
    if rc:
        raise MsbwtError(rc, "msbwt_overlap_plan: n, the symbols and the records of a piece must stay below 2^40, a piece is at most 2^28 queries")
    return out.value


def trace_plan(n, max_steps, mode="unique", targets=False, host=True, piece=0):
    """msbwt_trace_plan: the bytes of HBM scratch a trace call of n walks allocates (and frees again) on an index that holds something."""
    out = C.c_uint64(0)
    rc = _lib.lib().msbwt_trace_plan(int(n), int(max_steps), _lib.TRACE_MODES[mode], int(bool(targets)), int(bool(host)), int(piece), C.byref(out))
    if rc:
        raise MsbwtError(rc, "msbwt_trace_plan: max_steps and n x max_steps must stay below 2^40")
    return out.value


def reverse_complement_2bit(words, k):
    """uint64 2-bit words of k-mers, 1 <= k <= 32 -> the words of their reverse complements, same shape (msbwt_kmers_reverse_complement_2bit)."""
    w = np.ascontiguousarray(words, dtype=np.uint64)
    out = np.empty_like(w)
    rc = _lib.lib().msbwt_kmers_reverse_complement_2bit(w.ctypes.data_as(C.c_void_p), int(k), w.size, out.ctypes.data_as(C.c_void_p))
    if rc:
        raise ValueError("reverse_complement_2bit takes one word per k-mer: 1 <= k <= 32")
    return out


def _graph_neighbours(words, edges, k, successors):
    words, edges, k = np.ascontiguousarray(words, dtype=np.uint64), np.ascontiguousarray(edges, dtype=np.uint8), int(k)
    if not 1 <= k <= 32 or words.shape != edges.shape or words.ndim != 1:
        raise ValueError("graph neighbours need 1 <= k <= 32 and one edge byte per word")
    j = np.arange(4, dtype=np.uint64)
    bits = (edges[:, None] >> (np.arange(4, dtype=np.uint8) + np.uint8(4 if successors else 0))[None, :]) & np.uint8(1)
    mask = np.uint64((1 << (2 * k)) - 1)
    if successors:  # q.j: q loses its first symbol and gains j as the last
        if k == 32:
            shifted = (words << np.uint64(2))[:, None]
        else:
            shifted = ((words << np.uint64(2)) & mask)[:, None]
        grid = shifted | j[None, :]
    else:  # j.q: q loses its last symbol and gains j as the first
        grid = (words >> np.uint64(2))[:, None] | (j << np.uint64(2 * (k - 1)))[None, :]
    rec, sym = np.nonzero(bits)
    return rec.astype(np.int64), grid[rec, sym]


def graph_successors(words, edges, k):
    """(index, neighbours): for every successor bit 4 + j of edges[i], in the order of i then j, the record i and the 2-bit word of the
    node the edge words[i].j leads to (words[i] without its first symbol, with j appended).  Pure host logic."""
    return _graph_neighbours(words, edges, k, True)


def graph_predecessors(words, edges, k):
    """(index, neighbours): for every predecessor bit j of edges[i], in the order of i then j, the record i and the 2-bit word of the
    node the edge j.words[i] comes from (j, then words[i] without its last symbol).  Pure host logic."""
    return _graph_neighbours(words, edges, k, False)


def unitig_link_records(link_offsets, link_targets, flags):
    """(side, target): the records of a link table (RleBWT.enumerate_unitig_graph) with every bidirected edge kept once.  The record
    (a, e) -- side a holds entry e -- has the mirror (c(e ^ 1), c(a ^ 1)), the same edge from its other end, where c clears bit 0 for a
    unitig that is its own reverse complement (flags bit 1); a record stays when it is not above its mirror, compared as pairs.  In table
    order.  Pure host logic."""
    link_offsets, link_targets = np.ascontiguousarray(link_offsets, dtype=np.uint64), np.ascontiguousarray(link_targets, dtype=np.uint64)
    own_mirror = (np.ascontiguousarray(flags, dtype=np.uint8) & np.uint8(2)) != 0
    if link_offsets.size != 2 * own_mirror.size + 1 or int(link_offsets[-1]) != link_targets.size:
        raise ValueError("a link table has 2 U + 1 offsets, the last of which is the number of its targets")
    sides = np.repeat(np.arange(2 * own_mirror.size, dtype=np.uint64), np.diff(link_offsets).astype(np.int64))
    one = np.uint64(1)

    def c(x):
        return np.where(own_mirror[(x >> one).astype(np.int64)], x & ~one, x)

    mirror_side, mirror_target = c(link_targets ^ one), c(sides ^ one)
    keep = (sides < mirror_side) | ((sides == mirror_side) & (link_targets <= mirror_target))
    return sides[keep], link_targets[keep]


def write_gfa(file, k, symbols, offsets, count_sums, flags, link_offsets, link_targets, source_sums=None):
    """The compacted graph of RleBWT.enumerate_unitig_graph as GFA 1: a header, one `S <u> <sequence> KC:i:<count sum>` line a unitig
    (named by its number) and one `L <u> <+|-> <v> <+|-> <k-1>M` line per edge, each edge once (unitig_link_records): an odd side leaves
    the reverse complement (-), an odd entry reaches one.  With `source_sums` (U x S, RleBWT.enumerate_unitig_graph_by_source) every S
    line carries the tag `sc:Z:c0,c1,...` behind KC:i:, the unitig's sums by input in decimal.  `file`: a path, or an object with
    write().  -> (segments, links) written."""
    k = int(k)
    sides, targets = unitig_link_records(link_offsets, link_targets, flags)
    lines = ["H\tVN:Z:1.0\n"]
    for u, sequence in enumerate(_sequences(np.ascontiguousarray(symbols, dtype=np.uint8), offsets)):
        colours = "" if source_sums is None else "\tsc:Z:" + ",".join(str(int(c)) for c in source_sums[u])
        lines.append("S\t%d\t%s\tKC:i:%d%s\n" % (u, sequence, int(count_sums[u]), colours))
    for a, e in zip(sides.tolist(), targets.tolist()):
        lines.append("L\t%d\t%s\t%d\t%s\t%dM\n" % (a >> 1, "-" if a & 1 else "+", e >> 1, "-" if e & 1 else "+", k - 1))
    if hasattr(file, "write"):
        file.write("".join(lines))
    else:
        with open(file, "w") as out:
            out.write("".join(lines))
    return len(offsets) - 1, len(sides)


def count_read_kmers_multi(replicas, reads, k, ascii=False, forward=True, revcomp=False):
    """msbwt_rle_count_read_kmers_multi: reads sharded over the replicas, every k-mer window counted."""
    a = np.ascontiguousarray(reads, dtype=np.uint8)
    n, length = a.shape
    w = length - k + 1
    fwd = np.empty((n, w), dtype=np.uint64) if forward else None
    rc_arr = np.empty((n, w), dtype=np.uint64) if revcomp else None
    rc = _lib.lib().msbwt_rle_count_read_kmers_multi(
        _handles(replicas), len(replicas), a.ctypes.data_as(C.c_void_p), length, n, k, 1 if ascii else 0,
        fwd.ctypes.data_as(C.c_void_p) if fwd is not None else None, rc_arr.ctypes.data_as(C.c_void_p) if rc_arr is not None else None)
    if rc:
        raise MsbwtError(rc, "; ".join(_lib.lib().msbwt_rle_last_error(r._h).decode(errors="replace") for r in replicas))
    return fwd, rc_arr


def count_kmers_multi_device(replicas, d_kmers, k, n, d_out):
    """msbwt_rle_count_kmers_multi_device: device pointers on replicas[0]'s device; synchronous."""
    rc = _lib.lib().msbwt_rle_count_kmers_multi_device(_handles(replicas), len(replicas), d_kmers, k, n, d_out)
    if rc:
        raise MsbwtError(rc, "; ".join(_lib.lib().msbwt_rle_last_error(r._h).decode(errors="replace") for r in replicas))
