"""k-mer ranges and left-extension counts (msbwt_rle_kmer_ranges[_device], msbwt_rle_count_kmer_extensions[_device]) against the CPU oracle
and a brute-force count over the strings, in every index configuration whose search kernel has a range form (csrc/lanes_kernel.hpp,
csrc/kernels.hip) and with both block formats behind the extension kernel (csrc/extend.hip).  Each case asserts the configuration it
loaded before it asks anything.  Needs an MI355X: run with `pytest -m gpu`."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import rust_msbwt_amd as msbwt
from rust_msbwt_amd import RleBWT, _lib
from conftest import GOLDEN_DIR, ROOT
from oracle import oracle as orc
from test_gpu_sparse import ACGT, oracle_ranges, read_set, synth_bwt
from test_gpu_tier_fallback import GENOME_READS, high_copy_read_set, query_mix

pytestmark = pytest.mark.gpu
MsbwtError = msbwt.rle_bwt.MsbwtError

ALL_KS = (0, 1, 2, 5, 6, 15, 16, 17, 22, 23, 24, 29, 30, 31, 32, 33, 48, 64, 65, 80)
SOME_KS = (0, 2, 6, 16, 17, 23, 24, 27, 31, 32, 33, 64, 65)
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
_CACHE = {}


def plain_read_set():
    """Reads of a random genome with 0.5 % substitutions and a few repeats: counts 0, 1 and more at every k."""
    if "reads" not in _CACHE:
        reads = read_set(91, 20000, 3000, 100, repeats=6, err=0.005)
        _CACHE["reads"] = reads
        _CACHE["rle"] = synth_bwt(reads)
        ref = orc.OracleRleBWT()
        ref.load_vector(_CACHE["rle"])
        _CACHE["ref"] = ref
    return _CACHE["reads"], _CACHE["rle"], _CACHE["ref"]


def expected(ref, q):
    """(l, h, ext) by the oracle: ext[:, c] = count_kmers([c] ++ row); ranges by its constrain_range, empty ones as (0, 0)."""
    n = len(q)
    ext = np.stack([ref.count_kmers(np.ascontiguousarray(np.hstack([np.full((n, 1), c, dtype=np.uint8), q]))) for c in range(6)], axis=1)
    if q.shape[1] == 0:
        l = np.zeros(n, dtype=np.uint64)
        h = np.full(n, ref.get_total_size(), dtype=np.uint64)
    else:
        l, h = oracle_ranges(ref, q)
    empty = l == h
    l[empty] = 0
    h[empty] = 0
    return l, h, ext.astype(np.uint64)


def queries(reads, k, rng):
    if k == 0:
        return np.zeros((37, 0), dtype=np.uint8)
    return query_mix(reads, k, rng, GENOME_READS if len(reads) > GENOME_READS else None)


def check(b, ref, q, k):
    l, h = b.kmer_ranges(q)
    ext = b.count_kmer_extensions(q)
    cnt = b.count_kmers(q)
    # invariants among the library's own answers
    assert np.array_equal(h - l, cnt), k
    assert np.array_equal(ext.sum(axis=1), cnt), k
    assert np.all((cnt > 0) | ((l == 0) & (h == 0))), k
    el, eh, eext = expected(ref, q)
    assert np.array_equal(l, el) and np.array_equal(h, eh), k
    assert np.array_equal(ext, eext), k


def run_ks(b, ref, reads, ks, seed):
    rng = np.random.default_rng(seed)
    for k in ks:
        check(b, ref, queries(reads, k, rng), k)


def load(rle, monkeypatch, env=None, query_length=None):
    for key, v in (env or {}).items():
        monkeypatch.setenv(key, str(v))
    b = RleBWT()
    if query_length:
        b.set_query_length(query_length)
    b.load_vector(rle)
    return b


# ---- configurations ------------------------------------------------------------------------------------------------------------------
def test_automatic_index_every_k(monkeypatch):
    reads, rle, ref = plain_read_set()
    b = load(rle, monkeypatch)
    assert b.get_block_format() == "planes" and b.get_pair_index() and b.get_total_size() == ref.get_total_size()
    run_ks(b, ref, reads, ALL_KS, 1)


# name -> (environment, declared k, what the loaded index must look like)
CONFIGS = {
    "no_sparse": ({"MSBWT_SPARSE_TABLE": 0}, None, lambda b: b.get_sparse_table() == 0 and b.get_pair_index()),
    "declared_k31": ({}, 31, lambda b: b.get_query_length() == 31 and b.get_pair_index()),
    "xwide31": ({"MSBWT_SEARCH": "lanes", "MSBWT_SPARSE_TABLE": 31}, None, lambda b: b.get_sparse_table() == 31),
    "wide27": ({"MSBWT_SEARCH": "lanes", "MSBWT_SPARSE_TABLE": 27}, None, lambda b: b.get_sparse_table() == 27),
    "sparse20": ({"MSBWT_SEARCH": "lanes", "MSBWT_SPARSE_TABLE": 20}, None, lambda b: b.get_sparse_table() == 20),
    "groups": ({"MSBWT_SEARCH": "groups"}, None, lambda b: b.get_search_kernel() == "groups" and b.search_kernel_for(31) == "groups"),
    "lanes": ({"MSBWT_SEARCH": "lanes"}, None, lambda b: b.get_search_kernel() == "lanes" and b.search_kernel_for(31) == "lanes"),
    "no_pair": ({"MSBWT_PAIR_INDEX": 0}, None, lambda b: not b.get_pair_index()),
    "no_pair_lanes": ({"MSBWT_PAIR_INDEX": 0, "MSBWT_SEARCH": "lanes"}, None, lambda b: not b.get_pair_index()),
    "runs": ({"MSBWT_BLOCKS": "runs", "MSBWT_SPARSE_TABLE": 0}, None,
             lambda b: b.get_block_format() == "runs" and b.get_sparse_table() == 0 and not b.get_pair_index()),
    "runs_sparse": ({"MSBWT_BLOCKS": "runs", "MSBWT_SPARSE_TABLE": 20}, None,
                    lambda b: b.get_block_format() == "runs" and b.get_sparse_table() == 20),
    "host_build": ({"MSBWT_BUILD": "host"}, None, lambda b: b.get_block_format() == "planes"),
    "ordered": ({"MSBWT_ORDER": 1}, None, lambda b: b.get_batch_order() == 1 and b.batch_order_for(31, 8100) == 1),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_configuration(name, monkeypatch):
    env, qlen, looks_right = CONFIGS[name]
    reads, rle, ref = plain_read_set()
    b = load(rle, monkeypatch, env, qlen)
    assert looks_right(b), name
    run_ks(b, ref, reads, SOME_KS, zlib.crc32(name.encode()))


@pytest.mark.parametrize("tiers", [0, 1])
def test_high_copy_suffixes_escape_lines_and_two_tier(tiers, monkeypatch):
    """High-copy reads (escape lines of the packed direct table, side-array entries), with the complete sparse table of depth 17 or its
    two-tier form in front of a packed depth-15 direct table; k-mers of the junction reads fall back through the escape line."""
    reads, rle = high_copy_read_set()
    ref = orc.OracleRleBWT()
    ref.load_vector(rle)
    env = {"MSBWT_SEARCH": "lanes", "MSBWT_SPARSE_TABLE": 16 + tiers, "MSBWT_TABLE_DEPTH": 13, "MSBWT_TABLE_PACKED": 1, "MSBWT_SPARSE_TIERS": tiers}
    b = load(rle, monkeypatch, env)
    assert b.get_sparse_table() == 16 + tiers and bool(b.get_sparse_tiers()) == bool(tiers)
    assert b.get_table_depth() == 15 and b.get_table_packed()
    tinfo = b.table_info()
    assert tinfo["escape_lines"] > 0 and tinfo["side_bytes"] > 0, tinfo
    run_ks(b, ref, reads, (6, 15, 16, 17, 31, 33, 64), 17 + tiers)
    jq = np.ascontiguousarray(reads[-6:, 32:63])   # the junction 31-mers: each occurs once
    check(b, ref, np.ascontiguousarray(np.concatenate([jq] * 20)), 31)


# ---- brute force over the strings ------------------------------------------------------------------------------------------------------
SYM = "$ACGNT"


def brute_extensions(strings, q):
    """count([c] ++ q) by scanning the strings: c = '$' is a string that starts with q"""
    qs = "".join(SYM[x] for x in q)
    out = [sum(s.startswith(qs) for s in strings)]
    for c in SYM[1:]:
        p = c + qs
        out.append(sum(sum(1 for i in range(len(s) - len(p) + 1) if s[i:i + len(p)] == p) for s in strings))
    return out


@pytest.mark.parametrize("blocks", ["planes", "runs"])
def test_brute_force_on_toy_strings(blocks, monkeypatch):
    monkeypatch.setenv("MSBWT_BLOCKS", blocks)
    rng = np.random.default_rng(5)
    strings = ["".join(rng.choice(list("ACGTN"), p=[0.3, 0.2, 0.2, 0.25, 0.05], size=int(rng.integers(3, 40)))) for _ in range(60)]
    cases = [(["ACGT", "TGCA"], os.path.join(GOLDEN_DIR, "two_string.npy")), (strings, None)]
    for strs, npy in cases:
        b = RleBWT()
        if npy:
            b.load_numpy_file(npy)
        else:
            b.load_vector(orc.convert_to_vec(orc.naive_bwt(strs)))
        assert b.get_block_format() == blocks
        for k in (0, 1, 2, 3, 5, 8):
            q = np.array([rng.choice([1, 2, 3, 4, 5], size=k) for _ in range(150)], dtype=np.uint8).reshape(150, k)
            if k:   # and substrings that occur, the strings' first symbols among them
                subs = [s[i:i + k] for s in strs for i in range(len(s) - k + 1)][:200]
                q = np.concatenate([q, np.array([orc.convert_stoi(x) for x in subs], dtype=np.uint8).reshape(-1, k)])
            q = np.ascontiguousarray(q)
            ext = b.count_kmer_extensions(q)
            l, h = b.kmer_ranges(q)
            exp = np.array([brute_extensions(strs, row) for row in q], dtype=np.uint64)
            assert np.array_equal(ext, exp), (k, npy)
            assert np.array_equal(h - l, exp.sum(axis=1)), k


# ---- entry-point shapes -----------------------------------------------------------------------------------------------------------------
def _torch():
    import torch
    return torch


def test_batch_sizes_and_pipeline_chunks(monkeypatch):
    reads, rle, ref = plain_read_set()
    b = load(rle, monkeypatch)
    k = 31
    l, h = b.kmer_ranges(np.zeros((0, k), dtype=np.uint8))
    assert l.shape == h.shape == (0,) and b.count_kmer_extensions(np.zeros((0, k), dtype=np.uint8)).shape == (0, 6)
    one = np.ascontiguousarray(reads[3:4, 10:10 + k])
    check(b, ref, one, k)
    # 2^21 + 12 345 queries: the host forms cross a 2 Mi-query chunk of the pipeline
    rng = np.random.default_rng(3)
    windows = np.lib.stride_tricks.sliding_window_view(reads, k, axis=1).reshape(-1, k)
    n = (1 << 21) + 12345
    q = np.ascontiguousarray(windows[rng.integers(0, len(windows), size=n)])
    q[rng.integers(0, n, size=n // 4), rng.integers(0, k, size=n // 4)] = ACGT[rng.integers(0, 4, size=n // 4)]
    l, h = b.kmer_ranges(q)
    ext = b.count_kmer_extensions(q)
    cnt = b.count_kmers(q)
    assert np.array_equal(h - l, cnt) and np.array_equal(ext.sum(axis=1), cnt)
    around = np.r_[0:3000, (1 << 21) - 3000:(1 << 21) + 3000, n - 3000:n]   # both sides of the chunk border, and the ends
    el, eh, eext = expected(ref, np.ascontiguousarray(q[around]))
    assert np.array_equal(l[around], el) and np.array_equal(h[around], eh) and np.array_equal(ext[around], eext)


def test_device_forms_aligned_unaligned_and_on_a_side_stream(monkeypatch):
    torch = _torch()
    reads, rle, ref = plain_read_set()
    b = load(rle, monkeypatch)
    rng = np.random.default_rng(4)
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream(dev)
    for k in (5, 31, 33, 80):
        q = queries(reads, k, rng)
        n = len(q)
        el, eh, eext = expected(ref, q)
        for offset in (0, 1):   # 16-byte aligned, and one byte off (the generic kernel)
            raw = torch.zeros(n * k + 16, dtype=torch.uint8, device=dev)
            raw[offset:offset + n * k] = torch.from_numpy(q.reshape(-1)).to(dev)
            d_q = raw.data_ptr() + offset
            d_l = torch.full((n,), 7, dtype=torch.int64, device=dev)
            d_h = torch.full((n,), 7, dtype=torch.int64, device=dev)
            d_e = torch.full((n, 6), 7, dtype=torch.int64, device=dev)
            torch.cuda.synchronize(dev)
            with torch.cuda.stream(side):
                b.kmer_ranges_device(d_q, k, n, d_l.data_ptr(), d_h.data_ptr(), side.cuda_stream)
                b.count_kmer_extensions_device(d_q, k, n, d_e.data_ptr(), side.cuda_stream)
                b.device_status(side.cuda_stream)
            side.synchronize()
            assert np.array_equal(d_l.cpu().numpy().astype(np.uint64), el), (k, offset)
            assert np.array_equal(d_h.cpu().numpy().astype(np.uint64), eh), (k, offset)
            assert np.array_equal(d_e.cpu().numpy().astype(np.uint64), eext), (k, offset)


@pytest.mark.parametrize("k", [7, 31, 40, 70])
def test_invalid_symbol_row_is_all_ones_and_the_rest_exact(k, monkeypatch):
    torch = _torch()
    reads, rle, ref = plain_read_set()
    b = load(rle, monkeypatch)
    rng = np.random.default_rng(k)
    q = queries(reads, k, rng)[:3000].copy()
    bad = np.array([5, 700, 2999])
    q[bad, rng.integers(0, k, size=len(bad))] = np.array([6, 7, 200], dtype=np.uint8)
    good = np.setdiff1d(np.arange(len(q)), bad)
    el, eh, eext = expected(ref, np.ascontiguousarray(q[good]))
    dev = torch.device("cuda:0")
    d_q = torch.from_numpy(q).to(dev)
    d_l = torch.zeros(len(q), dtype=torch.int64, device=dev)
    d_h = torch.zeros(len(q), dtype=torch.int64, device=dev)
    d_e = torch.zeros((len(q), 6), dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for launch in (lambda: b.kmer_ranges_device(d_q.data_ptr(), k, len(q), d_l.data_ptr(), d_h.data_ptr(), stream),
                   lambda: b.count_kmer_extensions_device(d_q.data_ptr(), k, len(q), d_e.data_ptr(), stream)):
        launch()
        with pytest.raises(MsbwtError) as err:
            b.device_status(stream)
        assert err.value.code == _lib.ERR_INVALID_SYMBOL and "symbol" in str(err.value)
    l = d_l.cpu().numpy().astype(np.uint64)
    h = d_h.cpu().numpy().astype(np.uint64)
    e = d_e.cpu().numpy().astype(np.uint64)
    assert np.all(l[bad] == ALL_ONES) and np.all(h[bad] == ALL_ONES) and np.all(e[bad] == ALL_ONES)
    assert np.array_equal(l[good], el) and np.array_equal(h[good], eh) and np.array_equal(e[good], eext)
    with pytest.raises(MsbwtError) as err:   # the host forms report it too
        b.count_kmer_extensions(q)
    assert err.value.code == _lib.ERR_INVALID_SYMBOL


def test_replica_python_c_abi_and_cpp_mirror_agree(tmp_path, monkeypatch):
    import ctypes as C
    reads, rle, ref = plain_read_set()
    b = load(rle, monkeypatch)
    rng = np.random.default_rng(9)
    k = 31
    q = queries(reads, k, rng)
    n = len(q)
    l, h = b.kmer_ranges(q)
    ext = b.count_kmer_extensions(q)
    # a replica on the same device
    r = b.replicate(0)
    rl, rh = r.kmer_ranges(q)
    assert np.array_equal(rl, l) and np.array_equal(rh, h) and np.array_equal(r.count_kmer_extensions(q), ext)
    # the C ABI, called directly
    cl, ch, ce = np.empty(n, dtype=np.uint64), np.empty(n, dtype=np.uint64), np.empty((n, 6), dtype=np.uint64)
    lib = _lib.lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.msbwt_rle_kmer_ranges(b._h, vp(q), k, n, vp(cl), vp(ch)) == 0
    assert lib.msbwt_rle_count_kmer_extensions(b._h, vp(q), k, n, vp(ce)) == 0
    assert np.array_equal(cl, l) and np.array_equal(ch, h) and np.array_equal(ce, ext)
    # the C++ mirror, on the same index saved as a .npy
    npy = str(tmp_path / "idx.npy")
    orc.save_bwt_numpy(rle, npy)
    exe = str(tmp_path / "mirror")
    libdir = os.path.join(ROOT, "rust-msbwt_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "kmer_extensions_mirror.cpp"), "-o", exe, "-L", libdir, "-lmsbwt_hip",
                           "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])
    qfile, out = str(tmp_path / "q.bin"), str(tmp_path / "out.bin")
    q.tofile(qfile)
    res = subprocess.run([exe, npy, qfile, str(k), out], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    got = np.fromfile(out, dtype=np.uint64)
    assert np.array_equal(got[:n], l) and np.array_equal(got[n:2 * n], h) and np.array_equal(got[2 * n:].reshape(n, 6), ext)
