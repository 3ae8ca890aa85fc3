"""Bridges (csrc/bridges.hip, csrc/bridge_calls.cpp: msbwt_rle_bridge_kmers[_device]): all bounded walks between two anchor k-mers.

Expected values never come from the code under test: tests/bridge_oracle.py is the header's definition over strings (held against
brute force and the trace oracle in tests/test_bridge_oracle.py), and closed forms on a saturated graph and on a random chain.  All
seven outputs are compared word for word, the untouched tails of the rows included.

Shapes: ragged sets of 1-50 reads at k = 1, 2, 5, 16, 31 with pairs that bridge, pairs that do not, dirty, absent, below-threshold and
repeated anchors and seed == target; hand-made graphs at k = 5; a saturated graph at k = 4 whose frontier holds 2^19 to 4.2e6 states
(more than one trip of the grid, several levels of the scan, pair boundaries inside workgroups); pieces of 1 and 2 pairs; every index
form; host form, device form and torch tensors.  Run with `pytest -m gpu`."""
import ctypes as C
import importlib

import numpy as np
import pytest

import bridge_oracle as B
import trace_oracle as T
from test_gpu_merge_many import EMPTY
from test_gpu_reads_build import naive_rle, ragged_set
from test_gpu_spectrum import loaded
from test_gpu_trace import ALL_FORMS, chain, words_of

pytestmark = pytest.mark.gpu

msbwt = importlib.import_module("rust-msbwt_amd")
_lib = msbwt._lib
U64 = np.uint64
NAMES = ("symbols", "lengths", "edge_sums", "found", "stops", "depths", "live")
SENTINEL = 0xEE
DIRECTIONS = ("right", "left")


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def run(b, seeds, targets, k, max_steps, min_steps=0, max_paths=4, max_live=64, direction="right", min_count=1, min_edge=0):
    """the host form with the rows pre-filled with the sentinel"""
    symbols = np.full((len(seeds), max_paths, max_steps), SENTINEL, dtype=np.uint8)
    got = b.bridge_kmers(seeds, targets, k, max_steps, min_steps=min_steps, max_paths=max_paths, max_live=max_live, direction=direction, min_count=min_count,
                         min_edge=min_edge or None, symbols=symbols)
    assert got[0] is symbols
    assert [g.dtype for g in got] == [np.uint8, U64, U64, U64, np.uint8, U64, U64]
    return got


def check(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.flatnonzero((g != w).reshape(len(w), -1).any(axis=1))
        assert bad.size == 0, (what, name, bad[:5], g[bad[:3]], w[bad[:3]])


def check_info(b, res, pieces, max_steps, max_paths, max_live, host=True, slots=0):
    info, want = b.bridge_info(), B.expected_info(res, pieces)
    scratch = info.pop("scratch_bytes")
    assert info == want, (info, want)
    assert scratch == msbwt.bridge_plan(len(res), max_steps, max_paths, max_live, host=host, slots=slots)


def dirty(words, k, rng):
    """some of the words with garbage above bit 2k"""
    garbage = rng.integers(1, 1 << min(64 - 2 * k, 62), size=len(words), dtype=np.uint64) << U64(2 * k)
    return np.where(rng.random(len(words)) < 0.3, words | garbage, words)


def pairs_of(g, k, rng, direction):
    """(seed, target) as strings: ends of random walks through the graph (most bridge), seed == target, random pairs of nodes, anchors
    that are below the threshold or absent, and repeats"""
    nodes = sorted(g.nodes)
    absent = [q for q in ("".join(rng.choice(list("ACGT"), size=k)) for _ in range(6)) if q not in g.nodes and q not in g.below][:2]
    pairs = []
    for s in (nodes[i] for i in rng.integers(0, len(nodes), size=min(len(nodes), 14))) if nodes else ():
        cur = s
        for _ in range(int(rng.integers(1, 12))):
            fan = g.fan(cur, direction)
            if not fan:
                break
            cur = fan[int(rng.integers(0, len(fan)))][1]
            cur = cur[1:] if direction == "right" else cur[:-1]
        pairs.append((s, cur))
    pairs += [(q, q) for q in nodes[:4]]
    if nodes:
        pairs += [(nodes[i], nodes[j]) for i, j in rng.integers(0, len(nodes), size=(6, 2))]
        pairs += [(q, nodes[0]) for q in g.below[:2] + absent] + [(nodes[-1], q) for q in g.below[:2] + absent]
    else:
        pairs += [(q, q) for q in g.below[:2] + absent]
    return pairs + pairs[:3]


# ---- 1. exactness on small sets ----

WINDOWS = ((0, 0), (0, 1), (0, 7), (0, 40), (3, 7), (3, 40))  # min_steps in {0, 3} x max_steps in {0, 1, 7, 40}, min <= max


@pytest.mark.parametrize("k", (1, 2, 5, 16, 31))
@pytest.mark.parametrize("seed", [1, 2, 5])
def test_ragged_sets(orc, seed, k):
    reads = ragged_set(seed)
    b = loaded(naive_rle(orc, reads))
    rng = np.random.default_rng(seed * 100 + k)
    found, stops = 0, set()
    for min_count, min_edge in ((1, 0), (2, 3)):
        g = T.Graph(reads, k, min_count, min_edge)
        for direction in DIRECTIONS:
            pairs = pairs_of(g, k, rng, direction)
            seeds, targets = [s for s, _ in pairs], [t for _, t in pairs]
            ws, wt = dirty(words_of(seeds), k, rng), dirty(words_of(targets), k, rng)
            for min_steps, max_steps in WINDOWS:
                for max_paths in (1, 3):
                    for max_live in (1, 2, 8):
                        limits = (min_steps, max_steps, max_paths, max_live)
                        res = B.results(g, seeds, targets, direction, *limits)
                        want = B.expected_arrays(g, seeds, targets, direction, *limits, sentinel=SENTINEL, res=res)
                        got = run(b, ws, wt, k, max_steps, min_steps, max_paths, max_live, direction, min_count, min_edge)
                        check(got, want, (seed, k, min_count, min_edge, direction) + limits)
                        check_info(b, res, [range(len(pairs))], max_steps, max_paths, max_live)
                        found += int(want[3].sum())
                        stops |= set(want[4].tolist())
    assert found > 0 and len(stops) >= 3, stops  # (no vacuous case: which stops occur depends on k)


# ---- 2. hand-made graphs at k = 5 ----

def one(b, g, seed, target, direction="right", min_steps=0, max_steps=20, max_paths=4, max_live=64):
    """one pair, against the oracle -> (the bridges in reading order, found, stop name, depth, live)"""
    limits = (min_steps, max_steps, max_paths, max_live)
    want = B.expected_arrays(g, [seed], [target], direction, *limits, sentinel=SENTINEL)
    got = run(b, words_of([seed]), words_of([target]), g.k, max_steps, min_steps, max_paths, max_live, direction)
    check(got, want, (seed, target, direction) + limits)
    texts = msbwt.bridge_sequences(words_of([seed]), g.k, got[0], got[1], direction, text=True)[0]
    return texts, int(got[3][0]), B.STOP_NAMES[int(got[4][0])], int(got[5][0]), int(got[6][0])


def test_hand_made_graphs(orc):
    k = 5

    def graph(reads):
        return loaded(naive_rle(orc, reads)), T.Graph(reads, k)

    # a bubble: two bridges of equal length, in lexicographic order, from either side
    b, g = graph(["TTACGCATGGA", "TTACGGATGGA"])
    assert one(b, g, "TTACG", "ATGGA") == (["TTACGCATGGA", "TTACGGATGGA"], 2, "EXHAUSTED", 6, 0)
    assert one(b, g, "ATGGA", "TTACG", "left") == (["TTACGCATGGA", "TTACGGATGGA"], 2, "EXHAUSTED", 6, 0)
    assert one(b, g, "TTACG", "ATGGA", max_paths=1) == (["TTACGCATGGA"], 2, "FULL", 6, 0)
    assert one(b, g, "TTACG", "ATGGA", max_live=1) == ([], 0, "TOO_WIDE", 1, 2)
    assert got_edge_sums(b, g, "TTACG", "ATGGA") == [6, 6]
    # a bubble with arms of different length: the shorter first
    b, g = graph(["TTACGTCATGGA", "TTACGATGGA"])
    assert one(b, g, "TTACG", "ATGGA") == (["TTACGATGGA", "TTACGTCATGGA"], 2, "EXHAUSTED", 7, 0)
    assert one(b, g, "TTACG", "ATGGA", max_steps=6) == (["TTACGATGGA"], 1, "MAX_STEPS", 6, 1)
    assert one(b, g, "TTACG", "ATGGA", min_steps=6) == (["TTACGTCATGGA"], 1, "EXHAUSTED", 7, 0)  # (the short arm runs through the target into a dead end)
    # a tandem repeat: a walk ends where it first enters the target from lo on, and min_steps selects the second arrival
    b, g = graph(["GGACTTCACTTCACTTG"])
    assert one(b, g, "GGACT", "CACTT") == (["GGACTTCACTT"], 1, "EXHAUSTED", 6, 0)
    assert one(b, g, "GGACT", "CACTT", min_steps=7, max_paths=1) == (["GGACTTCACTTCACTT"], 1, "FULL", 11, 0)
    # a dead-end tip
    b, g = graph(["ACGTACCGGT", "TTTTTTT"])
    assert one(b, g, "ACGTA", "TTTTT") == ([], 0, "EXHAUSTED", 6, 0)
    assert one(b, g, "ACGTA", "GGGGG")[1:] == (0, "NO_TARGET", 0, 0) and one(b, g, "GGGGG", "ACGTA")[1:] == (0, "NO_SEED", 0, 0)
    assert one(b, g, "ACGTA", "TTTTT", max_steps=0)[1:] == (0, "MAX_STEPS", 0, 1)
    # seed == target on a self-loop and on a cycle
    b, g = graph(["AAAAAAAA"])
    assert one(b, g, "AAAAA", "AAAAA") == (["AAAAAA"], 1, "EXHAUSTED", 1, 0)
    assert one(b, g, "AAAAA", "AAAAA", min_steps=3, max_steps=5, max_paths=2) == (["AAAAAAAA"], 1, "EXHAUSTED", 3, 0)
    b, g = graph(["ACGTTGCAGACGTT"])
    for direction in DIRECTIONS:
        assert one(b, g, "ACGTT", "ACGTT", direction) == (["ACGTTGCAGACGTT"], 1, "EXHAUSTED", 9, 0)
    assert one(b, g, "ACGTT", "ACGTT", min_steps=10, max_steps=20, max_paths=1) == (["ACGTTGCAGACGTTGCAGACGTT"], 1, "FULL", 18, 0)


def got_edge_sums(b, g, seed, target):
    return run(b, words_of([seed]), words_of([target]), g.k, 20)[2][0, :2].tolist()


def test_guards_on_a_loaded_index(orc):
    b = loaded(naive_rle(orc, ["ACGTACCGGT"]))
    lib, words = _lib.lib(), words_of(["ACGTA", "CGTAC"])
    found = np.full(2, 77, dtype=U64)
    p = words.ctypes.data_as(C.c_void_p)

    def call(k=5, n=2, min_count=1, min_edge=0, direction=0, min_steps=0, max_steps=4, max_paths=2, max_live=8, seeds=p, targets=p):
        return lib.msbwt_rle_bridge_kmers(b._h, seeds, targets, k, n, min_count, min_edge, direction, min_steps, max_steps, max_paths, max_live, None, None, None,
                                          found.ctypes.data_as(C.c_void_p), None, None, None)

    def last_error():
        return lib.msbwt_rle_last_error(b._h).decode()

    for bad in (dict(k=0), dict(k=32), dict(min_count=3, min_edge=2), dict(direction=2), dict(direction=-1), dict(seeds=None), dict(targets=None), dict(max_paths=0),
                dict(max_live=0), dict(min_steps=5)):
        assert call(**bad) == _lib.ERR_INVALID_ARG, bad
        assert last_error() != ""
    assert "1 <= k <= 31" in (call(k=32), last_error())[1] and "min_steps" in (call(min_steps=5), last_error())[1]
    for bad in (dict(max_steps=_lib.BRIDGE_MAX_STEPS_CAP + 1), dict(max_live=_lib.BRIDGE_MAX_LIVE_CAP + 1), dict(n=2 ** 30, max_paths=2 ** 5, max_steps=2 ** 5),
                dict(n=2 ** 20, max_paths=2 ** 20, max_steps=0)):
        assert call(**bad) == _lib.ERR_TOO_LARGE, bad
    assert (found == 77).all()
    assert lib.msbwt_rle_bridge_kmers_device(b._h, None, None, 5, 2, 1, 0, 0, 0, 4, 2, 8, None, None, None, None, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert call(n=0, seeds=None, targets=None) == 0 and call(max_steps=_lib.BRIDGE_MAX_STEPS_CAP, max_live=2) == 0 and found.tolist() == [0, 0]
    with pytest.raises(msbwt.MsbwtError):
        b.set_bridge_slots(2 ** 28 + 1)
    b.set_bridge_slots(2 ** 28)
    b.set_bridge_slots(0)


# ---- 3. a saturated graph: every walk forks four ways a round ----

_saturated = {}


def saturated():
    """(a handle on the reads of a random text in which every 5-mer occurs, the oracle's graph at k = 4)"""
    if not _saturated:
        text = "".join("ACGT"[x] for x in np.random.default_rng(4).integers(0, 4, size=20000))
        reads = [text[s:s + 100] for s in range(0, len(text) - 99, 50)]
        g = T.Graph(reads, 4)
        assert len(g.edges) == 4 ** 5 and len(g.nodes) == 4 ** 4  # saturated: asserted from the oracle's own edge set
        _saturated.update(b=loaded(msbwt.RleBWT(device=0).build_from_reads(reads, ascii=True)), g=g)
    return _saturated["b"], _saturated["g"]


@pytest.mark.parametrize("pairs,steps,max_paths,slots", [(32, 8, 3, 0), (32, 8, 300, 0), (64, 9, 3, 2 ** 22)])
def test_a_saturated_graph_fills_the_frontier(pairs, steps, max_paths, slots):
    b, g = saturated()
    k, max_live = 4, 2 ** 16
    distinct = [("ACGT", "TTGA"), ("GGGG", "GGGG"), ("TACA", "ACAT"), ("CCCA", "AAAA")]
    seeds, targets = [distinct[i % 4][0] for i in range(pairs)], [distinct[i % 4][1] for i in range(pairs)]
    limits = (steps, steps, max_paths, max_live)
    res = B.results(g, seeds, targets, "right", *limits)
    want = B.expected_arrays(g, seeds, targets, "right", *limits, sentinel=SENTINEL, res=res)
    # the closed form: every string of `steps` symbols that ends in the target is a bridge
    assert (want[3] == 4 ** (steps - k)).all() and (want[5] == steps).all()
    assert (want[4] == (B.FULL if max_paths <= 4 ** (steps - k) else B.MAX_STEPS)).all() and (want[6] == 4 ** steps - 4 ** (steps - k)).all()
    b.set_bridge_slots(slots)
    try:
        got = run(b, words_of(seeds), words_of(targets), k, steps, steps, max_paths, max_live)
        check(got, want, (pairs, steps, max_paths))
        P = max(slots, 2 ** 20) // max_live
        check_info(b, res, [range(i, min(i + P, pairs)) for i in range(0, pairs, P)], steps, max_paths, max_live, slots=slots)
        info = b.bridge_info()
        assert info["widest"] == min(P, pairs) * 4 ** (steps - 1) and info["expanded"] == pairs * sum(4 ** r for r in range(1, steps + 1))
        if slots:
            assert info["widest"] > 4 * 2048 * 256  # several trips of the grid cap in every kernel, the scatter of children included
        # run to run: byte-equal, in the rows that are written and in which they are
        again = run(b, words_of(seeds), words_of(targets), k, steps, steps, max_paths, max_live)
        for name, x, y in zip(NAMES, got, again):
            assert x.tobytes() == y.tobytes(), name
    finally:
        b.set_bridge_slots(0)


def test_a_saturated_graph_with_small_limits_stops_at_known_rounds():
    b, g = saturated()
    k = 4
    seeds, targets = ["ACGT", "GGGG", "TACA"], ["TTGA", "GGGG", "ACAT"]
    for limits, stop, depth, found, live in (((20, 20, 4, 100), B.TOO_WIDE, 4, 0, 256), ((20, 20, 4, 256), B.TOO_WIDE, 5, 0, 1024),
                                             ((6, 10, 10, 2 ** 16), B.FULL, 6, 16, 4 ** 6 - 16)):
        want = B.expected_arrays(g, seeds, targets, "right", *limits, sentinel=SENTINEL)
        assert (want[4] == stop).all() and (want[5] == depth).all() and (want[3] == found).all() and (live is None or (want[6] == live).all())
        check(run(b, words_of(seeds), words_of(targets), k, limits[1], limits[0], limits[2], limits[3]), want, limits)


# ---- 4. pieces ----

@pytest.mark.parametrize("slots,max_live", [(16, 8), (16, 64), (1, 3)])
def test_pieces_give_the_same_bytes(orc, slots, max_live):
    reads = ragged_set(2)
    k, limits = 3, (2, 9, 3, max_live)
    b = loaded(naive_rle(orc, reads))
    g = T.Graph(reads, k)
    rng = np.random.default_rng(slots)
    pairs = pairs_of(g, k, rng, "right")
    seeds, targets = [s for s, _ in pairs], [t for _, t in pairs]
    res = B.results(g, seeds, targets, "right", *limits)
    want = B.expected_arrays(g, seeds, targets, "right", *limits, sentinel=SENTINEL, res=res)
    before = b.device_bytes()
    auto = run(b, words_of(seeds), words_of(targets), k, limits[1], limits[0], limits[2], max_live)
    check(auto, want, "one piece")
    check_info(b, res, [range(len(pairs))], limits[1], limits[2], max_live)
    b.set_bridge_slots(slots)
    try:
        pieces = run(b, words_of(seeds), words_of(targets), k, limits[1], limits[0], limits[2], max_live)
        P = max(1, slots // max_live)
        check_info(b, res, [range(i, min(i + P, len(pairs))) for i in range(0, len(pairs), P)], limits[1], limits[2], max_live, slots=slots)
        assert b.bridge_info()["pieces"] == -(-len(pairs) // P) > 10
        # the device form, whose arrays are the whole call's: a piece writes at its own rows
        import torch
        dev = torch.device("cuda:0")
        d_seeds, d_targets = (torch.from_numpy(words_of(x).view(np.int64)).to(dev) for x in (seeds, targets))
        d_symbols = torch.full((len(pairs), limits[2], limits[1]), SENTINEL, dtype=torch.uint8, device=dev)
        got = b.bridge_kmers(d_seeds, d_targets, k, limits[1], min_steps=limits[0], max_paths=limits[2], max_live=max_live, symbols=d_symbols)
        b.device_status(torch.cuda.current_stream(dev).cuda_stream)
        check([t.cpu().numpy().view(w.dtype) for t, w in zip(got, want)], want, "pieces, device form")
        check_info(b, res, [range(i, min(i + P, len(pairs))) for i in range(0, len(pairs), P)], limits[1], limits[2], max_live, host=False, slots=slots)
    finally:
        b.set_bridge_slots(0)
    check(pieces, auto, "pieces")
    assert b.device_bytes() == before


# ---- 5. every index form gives the same bytes ----

@pytest.mark.parametrize("form", sorted(ALL_FORMS))
def test_every_index_form_gives_the_same_bytes(orc, form):
    knobs = ALL_FORMS[form]
    reads = ragged_set(5)
    b = loaded(naive_rle(orc, reads), **knobs)
    assert b.get_block_format() == knobs.get("block_format", "planes")
    rng = np.random.default_rng(3)
    for k in (3, 16, 31):
        g = T.Graph(reads, k, 1, 0)
        for direction in DIRECTIONS:
            pairs = pairs_of(g, k, rng, direction)
            seeds, targets = [s for s, _ in pairs], [t for _, t in pairs]
            want = B.expected_arrays(g, seeds, targets, direction, 0, 30, 3, 8, sentinel=SENTINEL)
            check(run(b, words_of(seeds), words_of(targets), k, 30, 0, 3, 8, direction), want, (form, k, direction))
    # an index past one block: the 5 000-base chain, whose every k-mer is unique -- one bridge of 30 steps between k-mers 30 apart
    c = chain()
    b = loaded(c["rle"], **knobs)
    text = c["text"]
    positions = list(range(0, 4900, 64))
    for k, direction in ((21, "right"), (31, "left")):
        near, far = [text[p:p + k] for p in positions], [text[p + 30:p + 30 + k] for p in positions]
        seeds, targets = (near, far) if direction == "right" else (far, near)
        symbols, lengths, sums, found, stops, depths, live = run(b, words_of(seeds), words_of(targets), k, 40, 25, 2, 4, direction)
        assert (found == 1).all() and (stops == B.EXHAUSTED).all() and (depths == 30).all() and not live.any() and (lengths == [30, 0]).all()
        rows = msbwt.bridge_sequences(words_of(seeds), k, symbols, lengths, direction, text=True)
        assert rows == [[text[p:p + 30 + k]] for p in positions]
        assert (sums[:, 0] == [sum(c["edges"][k][text[j:j + k + 1]] for j in range(p, p + 30)) for p in positions]).all() and (symbols[:, 1] == SENTINEL).all()


# ---- 6. host form, device form, torch tensors; NULL outputs; n = 0; an empty index ----

def test_host_form_device_form_and_torch_tensors_give_the_same_bytes(orc):
    import torch
    reads = ragged_set(2)
    k, limits = 4, (0, 12, 3, 8)
    b = loaded(naive_rle(orc, reads))
    g = T.Graph(reads, k)
    dev = torch.device("cuda:0")
    before = b.device_bytes()
    for direction in DIRECTIONS:
        pairs = pairs_of(g, k, np.random.default_rng(9), direction)
        seeds, targets = [s for s, _ in pairs], [t for _, t in pairs]
        ws, wt = words_of(seeds), words_of(targets)
        n = len(pairs)
        want = B.expected_arrays(g, seeds, targets, direction, *limits, sentinel=SENTINEL)
        check(run(b, ws, wt, k, limits[1], limits[0], limits[2], limits[3], direction), want, ("host", direction))
        d_seeds, d_targets = (torch.from_numpy(w.view(np.int64)).to(dev) for w in (ws, wt))
        for stream in (torch.cuda.current_stream(dev), torch.cuda.Stream(dev)):
            with torch.cuda.stream(stream):
                d_symbols = torch.full((n, limits[2], limits[1]), SENTINEL, dtype=torch.uint8, device=dev)
                stream.synchronize()
                got = b.bridge_kmers(d_seeds, d_targets, k, limits[1], min_steps=limits[0], max_paths=limits[2], max_live=limits[3], direction=direction,
                                     symbols=d_symbols)
                b.device_status(stream.cuda_stream)
            assert got[0] is d_symbols and all(t.device == dev for t in got)
            check([t.cpu().numpy().view(w.dtype) for t, w in zip(got, want)], want, ("torch", direction))
            assert b.bridge_info()["scratch_bytes"] == msbwt.bridge_plan(n, limits[1], limits[2], limits[3], host=False)
        counted = b.bridge_kmers(d_seeds, d_targets, k, limits[1], min_steps=limits[0], max_paths=limits[2], max_live=limits[3], direction=direction, symbols=False)
        assert counted[0] is None
        check([t.cpu().numpy().view(w.dtype) for t, w in zip(counted[1:], want[1:])], want[1:], ("counting", direction))
        # NULL outputs: each alone, each missing alone, none -- what is asked for is what the full call gave, and nothing else is written
        d_full = [torch.from_numpy(w.copy()).to(dev) if w.dtype == np.uint8 else torch.from_numpy(w.view(np.int64).copy()).to(dev) for w in want]
        for wanted in [1 << j for j in range(7)] + [127 ^ 1 << j for j in range(7)] + [0]:
            outs = [np.full_like(w, SENTINEL) for w in want]
            ptrs = [o.ctypes.data_as(C.c_void_p) if wanted >> j & 1 else None for j, o in enumerate(outs)]
            rc = _lib.lib().msbwt_rle_bridge_kmers(b._h, ws.ctypes.data_as(C.c_void_p), wt.ctypes.data_as(C.c_void_p), k, n, 1, 0, _lib.TRACE_DIRECTIONS[direction],
                                                   *limits, *ptrs)
            assert rc == 0, _lib.lib().msbwt_rle_last_error(b._h)
            for j, (o, w) in enumerate(zip(outs, want)):
                assert np.array_equal(o, w) if wanted >> j & 1 else (o == SENTINEL).all(), (wanted, NAMES[j])
            d_outs = [torch.full_like(t, SENTINEL if t.dtype == torch.uint8 else -1) for t in d_full]
            b.bridge_kmers_device(d_seeds.data_ptr(), d_targets.data_ptr(), k, n, limits[1], *[t.data_ptr() if wanted >> j & 1 else None for j, t in enumerate(d_outs)],
                                  min_steps=limits[0], max_paths=limits[2], max_live=limits[3], direction=_lib.TRACE_DIRECTIONS[direction],
                                  stream=torch.cuda.current_stream(dev).cuda_stream)
            b.device_status(torch.cuda.current_stream(dev).cuda_stream)
            for j, (t, f) in enumerate(zip(d_outs, d_full)):
                assert torch.equal(t, f) if wanted >> j & 1 else bool((t == (SENTINEL if t.dtype == torch.uint8 else -1)).all()), (wanted, NAMES[j])
    assert b.device_bytes() == before
    # n = 0
    got = b.bridge_kmers(np.zeros(0, dtype=U64), np.zeros(0, dtype=U64), k, 5)
    assert [x.shape for x in got] == [(0, 4, 5), (0, 4), (0, 4), (0,), (0,), (0,), (0,)] and not any(b.bridge_info().values())
    got = b.bridge_kmers(torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int64, device=dev), k, 5)
    assert got[0].shape == (0, 4, 5) and got[3].numel() == 0


def test_an_empty_index():
    import torch
    b = loaded(EMPTY)
    k = 7
    words = np.array([0, 5, (1 << 14) - 1, 1 << 14 | 9, 2 ** 64 - 1], dtype=U64)
    symbols, lengths, sums, found, stops, depths, live = run(b, words, words[::-1].copy(), k, 6, max_paths=2)
    assert (symbols == SENTINEL).all() and not any(x.any() for x in (lengths, sums, found, depths, live)) and (stops == B.NO_SEED).all()
    assert b.bridge_info() == {"pairs": 5, "rounds": 0, "queries": 0, "expanded": 0, "found": 0, "pieces": 0, "scratch_bytes": 0, "widest": 0}
    dev = torch.device("cuda:0")
    d_words = torch.from_numpy(words.view(np.int64)).to(dev)
    got = b.bridge_kmers(d_words, d_words, k, 6)
    assert not got[0].any() and (got[4] == B.NO_SEED).all() and not any(bool(t.any()) for t in (got[1], got[2], got[3], got[5], got[6]))
    assert b.bridge_kmers(np.zeros(0, dtype=U64), np.zeros(0, dtype=U64), k, 6)[3].size == 0
