"""Unitigs (csrc/unitigs.hip, csrc/unitig_calls.cpp): the k-mer graph compacted into its non-branching paths on the device.

Expected values never come from the code under test.  The oracle is a few lines of Python over the reads as strings: Counters of the
ACGT-only windows at k and at k + 1 (test_gpu_kmer_graph.windows) give the nodes and the edges, the links follow from the definition
(out(p) = 1 and in(q) = 1), the heads are walked in sorted order and what is left then lies on cycles, opened at their smallest member.
Working on strings, k = 32 needs no 66-bit word.  Properties that need no oracle are checked beside it.

Shapes: ragged sets of 1-50 reads with N, duplicates and prefixes at every k; hand-made sets around k = 5 (a path of one, a branch, a
self-loop, isolated cycles, a cycle with a tail into it); a 20 000-base chain and a 5 000-base circle for the rounds of the pointer
jumping; the 4000-read sets with errors (4.0e5 symbols) under several thresholds; a frontier at its minimum; every index form.
Run with `pytest -m gpu`."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest

from test_gpu_kmer_graph import FORMS, check_graph, read_set_graph, thresholds, windows
from test_gpu_reads_build import naive_rle, ragged_set, read_set
from test_gpu_spectrum import loaded, word_of

pytestmark = pytest.mark.gpu

msbwt = importlib.import_module("rust-msbwt_amd")
_lib = msbwt._lib
MsbwtError = msbwt.MsbwtError
U64 = np.uint64
KS = (1, 2, 3, 4, 15, 16, 17, 30, 31, 32)
CODE = {"A": 1, "C": 2, "G": 3, "T": 5}
NAMES = ("symbols", "offsets", "count_sums", "ends", "flags")


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


# ---- the oracle: what the unitigs of a read set ARE, from its windows alone ----

def unitigs_of_texts(reads, k, min_count=1, min_edge=0):
    """{"seqs": [str], "symbols", "offsets", "count_sums", "ends", "flags", "info": nodes, edges, links, unitigs, symbols, circular, longest}"""
    m, me = thresholds(min_count, min_edge)
    nodes = {q: n for q, n in windows(reads, k).items() if n >= m}
    solid = {e for e, n in windows(reads, k + 1).items() if n >= me}
    succ = {q: [c for c in "ACGT" if q + c in solid] for q in nodes}
    pred = {q: [c for c in "ACGT" if c + q in solid] for q in nodes}
    up = {}  # the links: q -> the p whose only out-edge is q's only in-edge
    for q in nodes:
        if len(pred[q]) == 1:
            p = pred[q][0] + q[:-1]
            if len(succ[p]) == 1:
                up[q] = p
    down = {p: q for q, p in up.items()}
    assert len(down) == len(up)
    seen, found = set(), []

    def walk(first, circular):
        path = [first]
        while path[-1] in down and down[path[-1]] != first:
            path.append(down[path[-1]])
        assert not seen & set(path)
        seen.update(path)
        found.append((first, path, circular))

    for q in sorted(nodes):  # 2. the heads, in sorted order
        if q not in up:
            walk(q, False)
    for q in sorted(nodes):  # 3. what is left lies on cycles: each opened at its smallest member
        if q not in seen:
            walk(q, True)
    assert len(seen) == len(nodes)
    found.sort()  # ascending first node (strings over ACGT sort as their packed words do)
    seqs = [path[0] + "".join(q[-1] for q in path[1:]) for _, path, _ in found]
    ends = [sum(1 << "ACGT".index(c) for c in pred[path[0]]) | sum(16 << "ACGT".index(c) for c in succ[path[-1]]) for _, path, _ in found]
    lengths = [len(s) for s in seqs]
    out = {"seqs": seqs,
           "symbols": np.array([CODE[c] for s in seqs for c in s], dtype=np.uint8),
           "offsets": np.concatenate([[0], np.cumsum(lengths)]).astype(U64),
           "count_sums": np.array([sum(nodes[q] for q in path) for _, path, _ in found], dtype=U64),
           "ends": np.array(ends, dtype=np.uint8),
           "flags": np.array([int(c) for _, _, c in found], dtype=np.uint8),
           "first": [path[0] for _, path, _ in found], "last": [path[-1] for _, path, _ in found]}
    out["info"] = {"nodes": len(nodes), "edges": len(solid), "links": len(up), "unitigs": len(found), "symbols": int(sum(lengths)),
                   "circular": sum(int(c) for _, _, c in found), "longest": max([len(path) for _, path, _ in found], default=0)}
    assert out["info"]["symbols"] == len(nodes) + len(found) * (k - 1)  # S = n + U (k - 1)
    return out


def check_unitigs(b, k, want, min_count=1, min_edge=0):
    got = b.enumerate_unitigs(k, min_count=min_count, min_edge=min_edge or None)
    for name, g in zip(NAMES, got):
        assert g.dtype == want[name].dtype, name
        assert g.shape == want[name].shape and np.array_equal(g, want[name]), (k, min_count, min_edge, name, g[:8], want[name][:8])
    info = b.unitig_info()
    if want["info"]["nodes"]:
        assert {x: info[x] for x in want["info"]} == want["info"], (k, min_count, min_edge)
        n = info["nodes"]
        assert info["rounds"] <= 3 * (math.ceil(math.log2(n)) + 1) if n > 1 else info["rounds"] == 0
    else:
        assert not any(info.values())
    return got


def texts_of_codes(flat, offsets):
    text = np.frombuffer(b"$ACGNT", dtype=np.uint8)[flat].tobytes().decode()
    return [text[int(a):int(b)] for a, b in zip(offsets[:-1], offsets[1:])]


# ---- 1. exactness on small sets ----

@pytest.mark.parametrize("seed", [0, 1, 2, 5, 11])
def test_ragged_sets_at_every_k(orc, seed):
    reads = ragged_set(seed)
    b = loaded(naive_rle(orc, reads))
    longer = 0
    for k in KS:
        for min_count, min_edge in ((1, 0), (2, 0)):
            want = unitigs_of_texts(reads, k, min_count, min_edge)
            check_unitigs(b, k, want, min_count, min_edge)
            longer += sum(1 for a, z in zip(want["first"], want["last"]) if a != z)
    assert longer > 20  # (the sets do yield unitigs of more than one node)


def test_hand_made_sets(orc):
    k = 5

    def run(reads, kk=k, **thresholds):
        b = loaded(naive_rle(orc, reads))
        want = unitigs_of_texts(reads, kk, **thresholds)
        got = check_unitigs(b, kk, want, **thresholds)
        return want, dict(zip(NAMES, got)), b

    # a read of exactly k symbols: a unitig of one node with no neighbour
    want, got, _ = run(["ACGTA"])
    assert want["seqs"] == ["ACGTA"] and got["ends"].tolist() == [0] and got["flags"].tolist() == [0] and got["count_sums"].tolist() == [1]
    assert got["offsets"].tolist() == [0, 5] and got["symbols"].tolist() == [1, 2, 3, 5, 1]
    # a branch: GGCAT -> GCATC and GCATG ends TGGCAT; both branches are heads
    want, got, b = run(["TGGCATCAAAAAG", "TGGCATG"])
    assert want["seqs"] == ["GCATCAAAAAG", "GCATG", "TGGCAT"]  # (AAAAA occurs once: no loop; the chain runs through it)
    assert got["ends"].tolist() == [1 << 2, 1 << 2, 16 << 1 | 16 << 2]  # <- G, <- G; TGGCAT has no predecessor and the successors C and G
    assert got["count_sums"].tolist() == [7, 1, 4] and got["offsets"].tolist() == [0, 11, 16, 22] and not got["flags"].any()
    # with the loop beside it, AAAAA has two predecessors and two successors: a unitig of its own, and not circular
    loop = ["TGGCATCAAAAAG", "AAAAAAAA"]
    want, got, _ = run(loop)
    assert want["seqs"] == ["AAAAA", "AAAAG", "TGGCATCAAAA"] and not got["flags"].any() and got["ends"].tolist() == [0x53, 1, 16]
    for kk in (4, 6, 7):
        check_unitigs(b, kk, unitigs_of_texts(["TGGCATCAAAAAG", "TGGCATG"], kk))
    # the self-loop alone: one circular unitig of one node
    want, got, b = run(["AAAAAAAA"])
    assert want["seqs"] == ["AAAAA"] and got["ends"].tolist() == [0x11] and got["flags"].tolist() == [1] and got["count_sums"].tolist() == [4]
    assert b.unitig_info() == {"nodes": 1, "edges": 1, "links": 1, "unitigs": 1, "symbols": 5, "circular": 1, "longest": 1, "rounds": 0}
    # one isolated cycle of 9 nodes, opened at its smallest k-mer
    want, got, b = run(["ACGTTGCAGACGTT"])
    assert want["seqs"] == ["ACGTTGCAGACGT"] and got["flags"].tolist() == [1] and got["offsets"].tolist() == [0, 13]
    assert got["ends"].tolist() == [1 << 2 | 16 << 3]  # the closing edge GACGT -> ACGTT: predecessor G, successor T
    info = b.unitig_info()
    assert (info["nodes"], info["links"], info["unitigs"], info["circular"], info["longest"]) == (9, 9, 1, 1, 9) and info["rounds"] >= 4
    for kk in (3, 4, 6):
        check_unitigs(b, kk, unitigs_of_texts(["ACGTTGCAGACGTT"], kk))
    # a cycle with a tail running into it: the entry node has two predecessors and is a head; nothing is circular
    reads = ["TTCCACGTTGCAGACGTT"]
    want, got, _ = run(reads)
    assert not got["flags"].any() and want["info"]["circular"] == 0 and "ACGTTGCAGACGT" in want["seqs"] and want["info"]["unitigs"] == 2
    entry = want["seqs"].index("ACGTTGCAGACGT")
    assert got["ends"][entry] == (1 << 1 | 1 << 2 | 16 << 3)  # <- C (the tail) and G (the cycle); -> T: itself
    # two disjoint isolated cycles from two reads
    reads = ["ACGTTGCAGACGTT", "CCATGGATTCCCATGG"]
    want, got, b = run(reads)
    assert got["flags"].tolist() == [1, 1] and want["info"]["circular"] == 2 and want["info"]["links"] == want["info"]["nodes"]
    assert want["seqs"][0] == "ACGTTGCAGACGT" and all(s[:k - 1] == s[-(k - 1):] for s in want["seqs"])  # (each closes on itself)
    # a k-mer preceded only by '$' or 'N'
    reads = ["TTGACNCCGTTA", "CCGTTAG"]
    want, got, b = run(reads)
    assert got["ends"][want["seqs"].index("TTGAC")] == 0 and want["seqs"].count("CCGTTA") + want["seqs"].count("CCGTTAG") == 1
    for kk in (4, 6):
        check_unitigs(b, kk, unitigs_of_texts(reads, kk))
    # thresholds: the edge threshold above the node threshold cuts links
    reads = ["ACGTACCGGT", "ACGTACCGGT", "ACGTACC"]
    for min_count, min_edge in ((1, 0), (2, 0), (2, 3), (3, 0), (4, 0)):
        check_unitigs(loaded(naive_rle(orc, reads)), k, unitigs_of_texts(reads, k, min_count, min_edge), min_count, min_edge)


# ---- 2. long chains: the rounds of the pointer jumping ----

def _genome(n):
    return "".join("ACGT"[x] for x in np.random.default_rng(7).integers(0, 4, size=20000)[:n])


_chains = {}


def chain(circular):
    """(reads, a handle with them loaded): error-free 100-base reads every 50 bases of the 20 000-base genome, or of its first 5 000 as a circle"""
    if circular not in _chains:
        g = _genome(5000) if circular else _genome(20000)
        text = g + g[:200] if circular else g
        reads = [text[s:s + 100] for s in range(0, len(text) - 99, 50)]
        b = msbwt.RleBWT(device=0)
        b.load_reads(reads, ascii=True)
        _chains[circular] = (reads, b)
    return _chains[circular]


@pytest.mark.parametrize("k,nodes", [(15, 19986), (21, 19980), (31, 19970), (32, 19969)])
def test_one_long_chain(k, nodes):
    reads, b = chain(False)
    want = unitigs_of_texts(reads, k)
    assert want["info"]["unitigs"] == 1 and want["info"]["longest"] == nodes == want["info"]["nodes"] and want["info"]["circular"] == 0
    check_unitigs(b, k, want)
    info = b.unitig_info()
    print("k = %d: %d nodes in one unitig, %d rounds" % (k, nodes, info["rounds"]))
    assert info["longest"] == nodes and 14 <= info["rounds"] <= math.ceil(math.log2(nodes)) + 2


@pytest.mark.parametrize("k", [15, 21, 31, 32])
def test_one_long_circle(k):
    reads, b = chain(True)
    want = unitigs_of_texts(reads, k)
    assert want["info"]["unitigs"] == 1 and want["info"]["longest"] == 5000 == want["info"]["nodes"] and want["info"]["circular"] == 1
    symbols, offsets, sums, ends, flags = check_unitigs(b, k, want)
    first = want["seqs"][0][:k]
    assert first == min(windows(reads, k))  # opened at the smallest word
    last = want["seqs"][0][-k:]
    assert ends.tolist() == [1 << "ACGT".index(last[0]) | 16 << "ACGT".index(first[-1])] and flags.tolist() == [1]  # the closing edge last -> first
    info = b.unitig_info()
    print("k = %d: a circle of 5000 nodes, %d rounds" % (k, info["rounds"]))
    assert info["longest"] == 5000 and info["links"] == 5000 and 13 <= info["rounds"] <= 3 * 14


# ---- 3. reads with errors ----

_texts = {}


def read_set_texts(name):
    if name not in _texts:
        (flat, offsets), _ = read_set(name)
        _texts[name] = texts_of_codes(flat, offsets)
    return _texts[name]


_wants = {}


def read_set_unitigs(name, k, min_count=1, min_edge=0):
    key = (name, k, min_count, min_edge)
    if key not in _wants:
        _wants[key] = unitigs_of_texts(read_set_texts(name), k, min_count, min_edge)
    return _wants[key]


def windows_of_unitigs(symbols, offsets, k):
    """the packed words of all k-windows of the sequences, in order"""
    code = np.full(6, 255, dtype=np.uint8)
    code[[1, 2, 3, 5]] = [0, 1, 2, 3]
    two = code[symbols].astype(U64)
    assert (two < 4).all()
    starts = np.concatenate([np.arange(int(a), int(b) - k + 1) for a, b in zip(offsets[:-1], offsets[1:])]) if len(offsets) > 1 else np.zeros(0, dtype=np.int64)
    words = np.zeros(len(starts), dtype=U64)
    for j in range(k):
        words = (words << U64(2)) | two[starts + j]
    return words


@pytest.mark.parametrize("k", [15, 31])
@pytest.mark.parametrize("name", ["plain_100", "repeat_150"])
def test_read_sets_with_errors(orc, name, k):
    _, rle = read_set(name)
    b = loaded(rle)
    for min_count, min_edge in ((1, 0), (2, 0), (2, 3), (10 ** 9, 0)):
        want = read_set_unitigs(name, k, min_count, min_edge)
        symbols, offsets, sums, ends, flags = check_unitigs(b, k, want, min_count, min_edge)
        info = b.unitig_info()
        # without the oracle: the windows of the sequences are exactly the nodes, each once; the ends are the graph's bytes there
        words, counts, _, edges, n_edges = read_set_graph(orc, name, k, min_count, min_edge)
        got_words = windows_of_unitigs(symbols, offsets, k)
        assert len(got_words) == len(words) and np.array_equal(np.sort(got_words), words)
        U = len(sums)
        if min_count == 10 ** 9:
            assert U == 0 and len(symbols) == 0 and offsets.tolist() == [0]
            continue
        assert info["unitigs"] + info["links"] - info["circular"] == info["nodes"] == len(words) and info["edges"] == n_edges
        nodes_before = (offsets[:-1] - U64(k - 1) * np.arange(U, dtype=U64)).astype(np.int64)
        first, last = got_words[nodes_before], got_words[np.append(nodes_before[1:], len(got_words)) - 1]
        assert (first[1:] > first[:-1]).all()  # ascending first words
        assert np.array_equal(ends & 15, edges[np.searchsorted(words, first)] & 15) and np.array_equal(ends >> 4, edges[np.searchsorted(words, last)] >> 4)
        assert int(sums.sum()) == int(counts.sum())
        if min_count == 1:
            assert int(sums.sum()) == b.kmer_spectrum(k)[2]  # the plain spectrum's occurrences
        print("%s, k = %d, (%d, %d): %s" % (name, k, min_count, min_edge, info))
    assert read_set_unitigs(name, k)["info"]["longest"] > 50 and read_set_unitigs(name, k)["info"]["unitigs"] > 1000  # (the errors branch the graph)
    with pytest.raises(MsbwtError) as err:
        b.enumerate_unitigs(k, min_count=3, min_edge=2)
    assert err.value.code == _lib.ERR_INVALID_ARG and "min_edge" in str(err.value)


# ---- 4. chunks: the predecessor slots land in other chunks ----

@pytest.mark.parametrize("k", [15, 31])
def test_a_frontier_at_its_minimum_gives_the_same_bytes(k):
    name = "repeat_150"
    _, rle = read_set(name)
    b = loaded(rle)
    want = read_set_unitigs(name, k)
    auto = check_unitigs(b, k, want)
    b.set_spectrum_frontier(_lib.SPECTRUM_MIN_FRONTIER)
    first = b.enumerate_unitigs(k)
    info = b.spectrum_info()  # the writing walk
    second = b.enumerate_unitigs(k)
    assert info["k"] == k and info["chunks"] >= 1000 and info["nodes"][k] == want["info"]["nodes"]
    for x, y, z in zip(first, second, auto):
        assert np.array_equal(x, z) and np.array_equal(y, z)
    b.set_spectrum_frontier(0)


# ---- 5. every index form gives the same answer ----

@pytest.mark.parametrize("form", sorted(FORMS))
def test_every_index_form_gives_the_same_answer(form):
    name = "repeat_150"
    _, rle = read_set(name)
    b = loaded(rle, **FORMS[form])
    assert b.get_block_format() == FORMS[form].get("block_format", "planes")
    for k in (15, 31):
        check_unitigs(b, k, read_set_unitigs(name, k))
        check_unitigs(b, k, read_set_unitigs(name, k, 2, 3), 2, 3)


# ---- 6. capacity, NULL buffers, scratch ----

def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_capacity_and_null_buffers():
    import torch
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    name, k, min_count = "plain_100", 17, 2
    _, rle = read_set(name)
    want = read_set_unitigs(name, k, min_count)
    n, U, S = want["info"]["nodes"], want["info"]["unitigs"], want["info"]["symbols"]
    assert U > 50 and n > 10000
    b = loaded(rle)
    lib, got_u, got_s = _lib.lib(), C.c_uint64(0), C.c_uint64(0)
    total, before, free = b.get_total_size(), b.device_bytes(), torch.cuda.mem_get_info(0)[0]
    plan = lambda *a: msbwt.unitigs_plan(total, free, *a)
    sizes = {"symbols": S, "offsets": U + 1, "count_sums": U, "ends": U, "flags": U}
    staged = {"symbols": 8 * ((S + 7) // 8), "offsets": 0, "count_sums": 8 * U, "ends": 8 * ((U + 7) // 8), "flags": 8 * ((U + 7) // 8)}

    def host(cap_u, cap_s, skip=()):
        bufs = {x: np.full(sizes[x] + 3, 7, dtype=want[x].dtype) for x in NAMES}
        args = [_ptr(bufs[x]) if x not in skip else None for x in NAMES]
        return lib.msbwt_rle_enumerate_unitigs(b._h, k, min_count, 0, *args, cap_u, cap_s, C.byref(got_u), C.byref(got_s)), bufs

    # the two-call pattern; a capacity too small (each of the two) writes nothing and names U and S
    rc, bufs = host(0, 0)
    assert rc == 0 and (got_u.value, got_s.value) == (U, S) and all((a == 7).all() for a in bufs.values())
    assert b.spectrum_scratch_bytes() == plan(n) == plan(n, 0, 0)
    for cap_u, cap_s in ((U - 1, S), (U, S - 1), (1, 1), (0, S), (U, 0)):
        got_u.value = got_s.value = 0
        rc, bufs = host(cap_u, cap_s)
        message = lib.msbwt_rle_last_error(b._h)
        assert rc == _lib.ERR_INVALID_ARG and (got_u.value, got_s.value) == (U, S) and str(U).encode() in message and str(S).encode() in message
        assert all((a == 7).all() for a in bufs.values())
    # every output NULL in turn, and all at once; capacities above need
    for skip in ((),) + tuple((x,) for x in NAMES) + (NAMES,):
        rc, bufs = host(U + 2, S + 2, skip)
        assert rc == 0 and (got_u.value, got_s.value) == (U, S), skip
        for x in NAMES:
            assert (bufs[x][sizes[x]:] == 7).all() and (np.array_equal(bufs[x][:sizes[x]], want[x]) if x not in skip else (bufs[x] == 7).all()), (skip, x)
        assert b.spectrum_scratch_bytes() == plan(n, U, S) - sum(staged[x] for x in skip), skip
    rc, _ = host(U, 0, ("symbols",))  # no symbols wanted: their capacity does not matter
    assert rc == 0
    # the device form: the same, into buffers of the caller's; the byte arrays at odd addresses
    assert b.enumerate_unitigs_device(k, None, None, None, None, None, 0, 0, min_count=min_count, stream=stream) == (U, S)
    assert b.spectrum_scratch_bytes() == plan(n)
    words = ("offsets", "count_sums")
    for skip in ((),) + tuple((x,) for x in NAMES):
        bufs = {x: torch.full((sizes[x] + 9,), 7, dtype=torch.int64 if x in words else torch.uint8, device=dev) for x in NAMES}
        ptrs = [None if x in skip else bufs[x].data_ptr() + (0 if x in words else 1) for x in NAMES]
        for cap_u, cap_s in ((U - 1, S), (U, S - 1)):
            if cap_s < S and "symbols" in skip:
                continue
            with pytest.raises(MsbwtError) as err:
                b.enumerate_unitigs_device(k, *ptrs, cap_u, cap_s, min_count=min_count, stream=stream)
            assert err.value.code == _lib.ERR_INVALID_ARG and (err.value.n, err.value.symbols) == (U, S) and str(U) in str(err.value) and str(S) in str(err.value)
            assert all(bool((bufs[x] == 7).all()) for x in NAMES)
        assert b.enumerate_unitigs_device(k, *ptrs, U + 1, S + 1, min_count=min_count, stream=stream) == (U, S)
        b.device_status(stream)
        assert b.spectrum_scratch_bytes() == plan(n, U, S) - sum(staged.values())  # nothing staged
        for x in NAMES:
            got, lead = bufs[x].cpu().numpy(), 0 if x in words else 1
            if x in skip:
                assert (got == 7).all(), (skip, x)
            else:
                assert (got[:lead] == 7).all() and (got[lead + sizes[x]:] == 7).all() and np.array_equal(got[lead:lead + sizes[x]].astype(want[x].dtype), want[x]), (skip, x)
    assert b.device_bytes() == before
    # the guards behind "nothing loaded"
    for bad_k in (0, 33, 1000):
        assert lib.msbwt_rle_enumerate_unitigs(b._h, bad_k, 1, 0, None, None, None, None, None, 0, 0, C.byref(got_u), C.byref(got_s)) == _lib.ERR_INVALID_ARG
        assert lib.msbwt_rle_enumerate_unitigs_device(b._h, bad_k, 1, 0, None, None, None, None, None, 0, 0, C.byref(got_u), C.byref(got_s), None) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_enumerate_unitigs(b._h, k, 3, 2, None, None, None, None, None, 0, 0, C.byref(got_u), C.byref(got_s)) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_enumerate_unitigs(b._h, k, 1, 0, None, None, None, None, None, 0, 0, None, C.byref(got_s)) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_enumerate_unitigs(b._h, k, 0, 0, None, None, None, None, None, 0, 0, C.byref(got_u), None) == 0  # min_count 0 is 1; the total is optional
    # an empty index
    from test_gpu_merge_many import EMPTY
    empty = loaded(EMPTY)
    for kk in (1, 21, 32):
        got = empty.enumerate_unitigs(kk)
        assert [len(a) for a in got] == [0, 1, 0, 0, 0] and got[1].tolist() == [0] and not any(empty.unitig_info().values())
    assert empty.enumerate_unitigs(5, text=True)[0] == []


# ---- 7. round trip through the library's own calls ----

def test_round_trip_through_the_ragged_read_calls():
    name, k = "plain_100", 21
    _, rle = read_set(name)
    b = loaded(rle)
    want = read_set_unitigs(name, k)
    symbols, offsets, sums, ends, flags = b.enumerate_unitigs(k)
    seqs, sums2, ends2, flags2 = b.enumerate_unitigs(k, text=True)
    assert seqs == want["seqs"] and np.array_equal(sums, sums2) and np.array_equal(ends, ends2) and np.array_equal(flags, flags2)
    reads = [symbols[int(a):int(z)] for a, z in zip(offsets[:-1], offsets[1:])]
    # unitigs -> count_ragged_read_kmers at k: every window is a node, and its count the node's
    fwd, _, at = b.count_ragged_read_kmers(reads, k, ascii=False)
    counts = windows(read_set_texts(name), k)
    assert len(fwd) == len(counts) and fwd.tolist() == [counts[s[i:i + k]] for s in seqs for i in range(len(s) - k + 1)]
    assert np.array_equal(np.add.reduceat(fwd, at[:-1].astype(np.int64)), sums)
    # unitigs -> an index of their own -> its k-mers are the graph's nodes
    again = msbwt.RleBWT(device=0)
    again.load_reads((symbols, offsets), ascii=False)
    words, ones = again.enumerate_kmers(k)
    assert np.array_equal(words, b.enumerate_kmers(k)[0]) and words.tolist() == sorted(word_of(q) for q in counts) and (ones == 1).all()


# ---- 8. the graph calls are unchanged ----

def test_the_graph_calls_after_a_unitig_call(orc):
    import torch
    name, k = "plain_100", 15
    _, rle = read_set(name)
    b = loaded(rle)
    total, free = b.get_total_size(), torch.cuda.mem_get_info(0)[0]
    for min_count, min_edge in ((1, 0), (2, 3)):
        check_unitigs(b, k, read_set_unitigs(name, k, min_count, min_edge), min_count, min_edge)
        want = read_set_graph(orc, name, k, min_count, min_edge)
        check_graph(b, k, want, min_count, min_edge)  # the dump, then the degree table
        n = len(want[0])
        assert b.spectrum_scratch_bytes() == msbwt.kmer_graph_plan(total, free, n) - 24 * n
        b.enumerate_kmer_graph(k, min_count=min_count, min_edge=min_edge or None, ranges=True)
        assert b.spectrum_scratch_bytes() == msbwt.kmer_graph_plan(total, free, n)
    b.device_status()
