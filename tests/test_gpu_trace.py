"""Traces (csrc/trace.hip, csrc/trace_calls.cpp: msbwt_rle_trace_kmers[_device]): from seed k-mers through the k-mer graph, node by node.

Expected values never come from the code under test: tests/trace_oracle.py is the header's definition over strings (checked against
the unitig oracle in tests/test_trace_oracle.py), closed forms for a random chain, and -- where the issue asks for exactly that -- the
library's own enumerate_unitigs, which tests/test_gpu_unitigs.py holds to its oracle.

Shapes: ragged sets of 1-50 reads of 0-70 symbols with N, duplicates and prefixes at every k where a word's layout changes (1 .. 4,
15 .. 17, 30, 31), seeds that are nodes, below the threshold, absent, repeated and dirty above bit 2k, step limits 0, 1, 7 and past
every walk; hand-made sets at k = 5; the 4000-read set with errors (4.0e5 symbols) against its unitigs; a 5 000-base chain (5 000
rounds of one walk; 78 walks in one batch, which is no multiple of a wave; pieces of 64 walks); every index form; host form, device
form and torch tensors.  Run with `pytest -m gpu`."""
import ctypes as C
import importlib

import numpy as np
import pytest

import trace_oracle as T
from test_gpu_kmer_graph import FORMS, windows
from test_gpu_merge_many import EMPTY
from test_gpu_reads_build import naive_rle, ragged_set, read_set
from test_gpu_spectrum import loaded
from test_trace_oracle import HAND

pytestmark = pytest.mark.gpu

msbwt = importlib.import_module("rust-msbwt_amd")
_lib = msbwt._lib
MsbwtError = msbwt.MsbwtError
U64 = np.uint64
KS = (1, 2, 3, 4, 15, 16, 17, 30, 31)
MODES = ("unique", "unitig", "greedy")
DIRECTIONS = ("right", "left")
THRESHOLDS = ((1, 0), (2, 0), (1, 3))  # (min_count, min_edge)
NAMES = ("symbols", "steps", "stops", "edge_sums", "last", "fans")
SENTINEL = 0xEE
ALL_FORMS = dict(FORMS, **{"sparse table 16": dict(sparse_table=16), "no sparse table": dict(sparse_table=0)})


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def words_of(kmers):
    return np.array([T.word_of(q) for q in kmers], dtype=U64)


def run(b, words, k, max_steps, mode, direction, min_count=1, min_edge=0, targets=None):
    """the call with the rows pre-filled with the sentinel"""
    symbols = np.full((len(words), max_steps), SENTINEL, dtype=np.uint8)
    got = b.trace_kmers(words, k, max_steps, mode=mode, direction=direction, min_count=min_count, min_edge=min_edge or None, targets=targets, symbols=symbols)
    assert got[0] is symbols
    assert [g.dtype for g in got] == [np.uint8, U64, np.uint8, U64, U64, np.uint8]
    return got


def check(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        bad = np.flatnonzero((g != w).reshape(len(w), -1).any(axis=1))
        assert g.shape == w.shape and bad.size == 0, (what, name, bad[:5], g[bad[:3]], w[bad[:3]])


def seeds_of(g, k, rng):
    """every node, every k-mer below the threshold that occurs, a few absent ones, duplicates -- and the words, some dirty above bit 2k"""
    nodes = sorted(g.nodes)
    absent = [q for q in ("".join(rng.choice(list("ACGT"), size=k)) for _ in range(6)) if q not in g.nodes and q not in g.below][:3]
    kmers = nodes + g.below + absent + nodes[:5] + nodes[-2:]
    words = words_of(kmers)
    dirty = rng.random(len(words)) < 0.3
    garbage = rng.integers(1, 1 << min(64 - 2 * k, 62), size=len(words), dtype=np.uint64) << U64(2 * k)
    return kmers, np.where(dirty, words | garbage, words)


# ---- 1. exactness on small sets ----

@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("seed", [0, 1, 2, 5, 11])
def test_ragged_sets(orc, seed, k):
    reads = ragged_set(seed)
    b = loaded(naive_rle(orc, reads))
    rng = np.random.default_rng(seed * 100 + k)
    moved = 0
    for min_count, min_edge in THRESHOLDS:
        g = T.Graph(reads, k, min_count, min_edge)
        kmers, words = seeds_of(g, k, rng)
        for mode in MODES:
            for direction in DIRECTIONS:
                for max_steps in (0, 1, 7, 200):
                    want = T.expected_arrays(g, kmers, mode, direction, max_steps)
                    got = run(b, words, k, max_steps, mode, direction, min_count, min_edge)
                    check(got, want, (seed, k, min_count, min_edge, mode, direction, max_steps))
                    info = b.trace_info()
                    assert info["walks"] == len(words) and info["rounds"] <= max_steps + 1 and info["pieces"] == (1 if len(words) else 0)
                    assert info["steps"] == int(want[1].sum()) and info["longest"] == int(want[1].max(initial=0))
                    assert info["not_nodes"] == int((want[2] == T.NOT_A_NODE).sum())
                    moved += int(want[1].sum())
        # targets: a node a seed, drawn from the nodes; most lie off the seed's path, some on it, some are the seed
        if g.nodes:
            nodes = sorted(g.nodes)
            targets = [nodes[i] for i in rng.integers(0, len(nodes), size=len(kmers))]
            for mode, direction in (("greedy", "right"), ("unitig", "left")):
                want = T.expected_arrays(g, kmers, mode, direction, 200, targets)
                check(run(b, words, k, 200, mode, direction, min_count, min_edge, words_of(targets)), want, (seed, k, "targets", mode, direction))
    assert moved > 0 or k > 17 or seed == 0  # (the short k always move)


# ---- 2. hand-made sets at k = 5 ----

def one(b, g, seed, mode, direction, max_steps=50, target=None, **thresholds):
    """one walk, against the oracle -> (sequence in reading order, steps, stop name, edge_sum, last k-mer, fan bits)"""
    want = T.expected_arrays(g, [seed], mode, direction, max_steps, None if target is None else [target])
    got = run(b, words_of([seed]), g.k, max_steps, mode, direction, targets=None if target is None else words_of([target]), **thresholds)
    check(got, want, (seed, mode, direction, max_steps, target))
    text = msbwt.trace_sequences(words_of([seed]), g.k, got[0], got[1], direction, text=True)[0]
    return text, int(got[1][0]), T.STOP_NAMES[int(got[2][0])], int(got[3][0]), T.kmer_of(got[4][0], g.k), int(got[5][0])


def test_hand_made_sets(orc):
    k = 5

    def graph(reads, kk=k, **thresholds):
        return loaded(naive_rle(orc, reads)), T.Graph(reads, kk, **thresholds)

    # every set of the oracle's own test, every node and both directions, in all modes
    for reads in HAND:
        for min_count, min_edge in THRESHOLDS + ((2, 3),):
            b, g = graph(reads, min_count=min_count, min_edge=min_edge)
            kmers = sorted(g.nodes) + g.below + ["GGGGG"]
            for mode in MODES:
                for direction in DIRECTIONS:
                    check(run(b, words_of(kmers), k, 40, mode, direction, min_count, min_edge), T.expected_arrays(g, kmers, mode, direction, 40), (reads, mode, direction))
    # a read of exactly k symbols: a node with no edge
    b, g = graph(["ACGTA"])
    assert one(b, g, "ACGTA", "unitig", "right") == ("ACGTA", 0, "DEAD_END", 0, "ACGTA", 0)
    assert one(b, g, "CGTAC", "unitig", "right")[1:3] == (0, "NOT_A_NODE")
    # a dead end, with the sums of the edges on the way
    b, g = graph(["ACGTACCGGT", "ACGTACC"])
    assert one(b, g, "ACGTA", "unique", "right") == ("ACGTACCGGT", 5, "DEAD_END", 2 + 2 + 1 + 1 + 1, "CCGGT", 0)
    assert one(b, g, "CCGGT", "unique", "left") == ("ACGTACCGGT", 5, "DEAD_END", 7, "ACGTA", 0)
    assert one(b, T.Graph(["ACGTACCGGT", "ACGTACC"], k, min_count=2), "ACGTA", "unique", "right", min_count=2)[:3] == ("ACGTACC", 2, "DEAD_END")
    # a branch: UNIQUE and UNITIG stop with both fan bits; GREEDY takes the heavier side, and the smaller symbol on a tie
    b, g = graph(["TGGCATCA", "TGGCATCA", "TGGCATGA"])
    for mode in ("unique", "unitig"):
        assert one(b, g, "TGGCA", mode, "right") == ("TGGCAT", 1, "BRANCH", 3, "GGCAT", 0b0110)
    assert one(b, g, "TGGCA", "greedy", "right") == ("TGGCATCA", 3, "DEAD_END", 3 + 2 + 2, "CATCA", 0)
    b, g = graph(["TGGCATGA", "TGGCATGA", "TGGCATCA"])
    assert one(b, g, "TGGCA", "greedy", "right")[0] == "TGGCATGA"
    b, g = graph(["TGGCATGA", "TGGCATCA"])
    assert one(b, g, "TGGCA", "greedy", "right")[0] == "TGGCATCA"
    # a merge: MERGE in UNITIG mode, with the node not entered; entered in UNIQUE mode
    b, g = graph(["AACCGGTTAC", "TTCCGGTTAC"])
    assert one(b, g, "AACCG", "unitig", "right") == ("AACCGG", 1, "MERGE", 1, "ACCGG", 0b1000)  # CCGGT has the predecessors A and T
    assert one(b, g, "AACCG", "unique", "right") == ("AACCGGTTAC", 5, "DEAD_END", 1 + 1 + 2 + 2 + 2, "GTTAC", 0)
    assert one(b, g, "GTTAC", "unitig", "left") == ("CCGGTTAC", 3, "BRANCH", 6, "CCGGT", 0b1001)
    # A^k with its self-loop, alone and with a second in-edge
    b, g = graph(["AAAAAAAA"])
    for mode in MODES:
        for direction in DIRECTIONS:
            assert one(b, g, "AAAAA", mode, direction) == ("AAAAA", 0, "RETURNED", 0, "AAAAA", 1)
    b, g = graph(["AAAAAAAA", "CAAAAA"])
    assert one(b, g, "AAAAA", "unitig", "right")[1:3] == (0, "MERGE") and one(b, g, "AAAAA", "unique", "right")[1:3] == (0, "RETURNED")
    assert one(b, g, "CAAAA", "unitig", "right")[1:3] == (0, "MERGE") and one(b, g, "CAAAA", "unique", "right", 9)[1:3] == (9, "MAX_STEPS")
    # an isolated cycle of 9 nodes: RETURNED after 8 steps from every node
    b, g = graph(["ACGTTGCAGACGTT"])
    for mode in MODES:
        assert one(b, g, "ACGTT", mode, "right") == ("ACGTTGCAGACGT", 8, "RETURNED", 8, "GACGT", 0b1000)
        assert one(b, g, "GCAGA", mode, "left")[1:3] == (8, "RETURNED")
    # a cycle with a tail into it: MAX_STEPS in UNIQUE mode, MERGE in UNITIG mode
    b, g = graph(["TTCCACGTTGCAGACGTT"])
    assert one(b, g, "TTCCA", "unique", "right", 40)[1:3] == (40, "MAX_STEPS")
    assert one(b, g, "TTCCA", "unitig", "right", 40)[:3] == ("TTCCACGT", 3, "MERGE")
    # a target on the path, off the path, and equal to the seed
    b, g = graph(["ACGTACCGGT"])
    assert one(b, g, "ACGTA", "unique", "right", target="GTACC") == ("ACGTACC", 2, "TARGET", 2, "GTACC", 0b0100)
    assert one(b, g, "ACGTA", "unique", "right", target="GGGGG")[1:3] == (5, "DEAD_END")
    assert one(b, g, "ACGTA", "unique", "right", target="ACGTA")[1:3] == (5, "DEAD_END")
    assert one(b, g, "CCGGT", "greedy", "left", target="CGTAC")[:3] == ("CGTACCGGT", 4, "TARGET")
    # k = 31 reads rich in T: edge words with bit 63 set (RIGHT: the node's first symbol is T; LEFT: the symbol prepended is T)
    reads = ["T" * 20 + "GATTACATTTTGTTTCTTTATTTTTTGTTCTTTTTTTA", "T" * 20 + "GATTACATTTTGTTTCTTTATTTTTTGTTCTTTTC"]
    b, g = graph(reads, 31)
    first, last = reads[0][:31], reads[0][-31:]
    assert T.word_of(first) >> 60 == 3 and all(T.word_of(e) >> 63 for e in g.edges if e[0] == "T") and any(e[0] == "T" for e in g.edges)
    for mode in MODES:
        text, steps, stop, _, _, fan = one(b, g, first, mode, "right", 60)
        if mode == "greedy":  # C and T tie where the reads part: C, the second read's
            assert (text, stop, fan) == (reads[1], "DEAD_END", 0)
        else:
            assert reads[0].startswith(text) and reads[1].startswith(text) and (stop, fan) == ("BRANCH", 0b1010), (mode, text, stop)
        text, steps, stop, _, end, _ = one(b, g, last, mode, "left", 60)
        assert stop in ("DEAD_END", "MERGE") and reads[0].endswith(text) and steps > 0
    kmers = sorted(g.nodes)
    for mode in MODES:
        for direction in DIRECTIONS:
            check(run(b, words_of(kmers), 31, 60, mode, direction), T.expected_arrays(g, kmers, mode, direction, 60), ("T-rich", mode, direction))


def test_guards_on_a_loaded_index(orc):
    b = loaded(naive_rle(orc, ["ACGTACCGGT"]))
    lib, seeds = _lib.lib(), words_of(["ACGTA", "CGTAC"])
    steps = np.full(2, 77, dtype=U64)
    p = seeds.ctypes.data_as(C.c_void_p)

    def call(k=5, n=2, min_count=1, min_edge=0, mode=0, direction=0, max_steps=4, seeds=p):
        return lib.msbwt_rle_trace_kmers(b._h, seeds, None, k, n, min_count, min_edge, mode, direction, max_steps, None, steps.ctypes.data_as(C.c_void_p), None, None,
                                         None, None)

    def last_error():
        return lib.msbwt_rle_last_error(b._h).decode()

    for bad in (dict(k=0), dict(k=32), dict(k=33), dict(min_count=3, min_edge=2), dict(mode=3), dict(mode=-1), dict(direction=2), dict(direction=-1), dict(seeds=None)):
        assert call(**bad) == _lib.ERR_INVALID_ARG, bad
        assert last_error() != ""
    assert "1 <= k <= 31" in (call(k=32), last_error())[1] and "min_edge" in (call(min_count=3, min_edge=2), last_error())[1]
    for bad in (dict(max_steps=2 ** 40), dict(n=2 ** 30, max_steps=2 ** 10)):
        assert call(**bad) == _lib.ERR_TOO_LARGE, bad
    assert (steps == 77).all()
    assert lib.msbwt_rle_trace_kmers_device(b._h, None, None, 5, 2, 1, 0, 0, 0, 4, None, None, None, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert call(n=0, seeds=None) == 0 and call() == 0 and steps.tolist() == [4, 4]


# ---- 3. agreement with enumerate_unitigs on reads with errors ----

@pytest.mark.parametrize("min_count", [1, 2])
@pytest.mark.parametrize("k", [15, 31])
def test_unitig_mode_reproduces_the_unitigs(k, min_count):
    _, rle = read_set("plain_100")
    b = loaded(rle)
    symbols, offsets, sums, ends, flags = b.enumerate_unitigs(k, min_count=min_count)
    info = b.unitig_info()
    U, longest = len(sums), info["longest"]
    assert U > (1000 if min_count == 1 else 50) and longest > 50  # (the errors branch the graph; min_count = 2 drops most of them)
    code = np.zeros(6, dtype=U64)
    code[[1, 2, 3, 5]] = [0, 1, 2, 3]
    two = code[symbols]
    starts, ends_at = offsets[:-1].astype(np.int64), offsets[1:].astype(np.int64)
    first, last = np.zeros(U, dtype=U64), np.zeros(U, dtype=U64)
    for j in range(k):
        first = (first << U64(2)) | two[starts + j]
        last = (last << U64(2)) | two[ends_at - k + j]
    nodes = (ends_at - starts - (k - 1)).astype(U64)
    column = np.arange(longest)[None, :]
    for direction, seeds in (("right", first), ("left", last)):
        rows, steps, stops, edge_sums, end, fans = b.trace_kmers(seeds, k, longest, mode="unitig", direction=direction, min_count=min_count)
        assert np.array_equal(steps, nodes - U64(1)) and int(steps.sum()) + U == info["nodes"]
        assert np.array_equal(stops == T.RETURNED, flags & 1 == 1) and np.isin(stops[flags & 1 == 0], (T.DEAD_END, T.BRANCH, T.MERGE)).all()
        assert np.array_equal(end, last if direction == "right" else first)
        # every unitig's symbols: behind its first k (RIGHT), or before its last k, reversed (LEFT)
        valid = column < steps[:, None].astype(np.int64)
        at = (starts[:, None] + k + column) if direction == "right" else (ends_at[:, None] - k - 1 - column)
        assert np.array_equal(rows[valid], symbols[at[valid]]) and not rows[~valid].any()
        # the fans of the last node are the ends' bits on that side
        assert np.array_equal(fans, ends >> 4 if direction == "right" else ends & 15)
        t = b.trace_info()
        assert t["rounds"] <= longest + 1 and t["longest"] == longest - 1 and t["steps"] == info["nodes"] - U and t["not_nodes"] == 0
        print("k = %d, min_count = %d, %s: %d unitigs, %s" % (k, min_count, direction, U, t))


# ---- 4. rounds, compaction and pieces ----

_chain = {}


def chain():
    """(the 5 000-base random text, 100-base reads every 50 bases of it, their RLE, a handle with them loaded)"""
    if not _chain:
        text = "".join("ACGT"[x] for x in np.random.default_rng(77).integers(0, 4, size=5000))
        reads = [text[s:s + 100] for s in range(0, len(text) - 99, 50)]
        rle = msbwt.RleBWT(device=0).build_from_reads(reads, ascii=True)
        _chain.update(text=text, reads=reads, rle=rle, b=loaded(rle), edges={k: windows(reads, k + 1) for k in (21, 31)})
    return _chain


def chain_walks(k, positions, max_steps, direction):
    """closed forms for walks from the chain's k-mers at `positions`: every k-mer and (k+1)-mer of the text is unique"""
    c = chain()
    text, edges = c["text"], c["edges"][k]
    n_nodes = len(text) - k + 1
    symbols = np.full((len(positions), max_steps), SENTINEL, dtype=np.uint8)
    steps, sums, last, stops, fans = [], [], [], [], []
    for i, p in enumerate(positions):
        room = n_nodes - 1 - p if direction == "right" else p
        s = min(room, max_steps)
        path = text[p + k:p + k + s] if direction == "right" else text[p - s:p][::-1]
        symbols[i, :s] = [T.CODE[ch] for ch in path]
        end = p + s if direction == "right" else p - s
        crossed = range(p, p + s) if direction == "right" else range(p - s, p)
        steps.append(s)
        sums.append(sum(edges[text[j:j + k + 1]] for j in crossed))
        last.append(T.word_of(text[end:end + k]))
        stops.append(T.MAX_STEPS if s == max_steps else T.DEAD_END)  # (the step limit is looked at first)
        at_end = end == (n_nodes - 1 if direction == "right" else 0)
        fans.append(0 if at_end else 1 << "ACGT".index(text[end + k] if direction == "right" else text[end - 1]))
    return symbols, np.array(steps, dtype=U64), np.array(stops, dtype=np.uint8), np.array(sums, dtype=U64), np.array(last, dtype=U64), np.array(fans, dtype=np.uint8)


def check_round_structure(b, got, n, max_steps, mode, targets=False, piece=0):
    info = b.trace_info()
    assert info["walks"] == n and info["rounds"] <= (max_steps + 1) * info["pieces"] and info["pieces"] == -(-n // (piece or 2 ** 20))
    assert info["scratch_bytes"] == msbwt.trace_plan(n, max_steps, mode, targets=targets, host=True, piece=piece)
    # a finished walk is not searched again: 5 queries a walk in round 0, then 4 or 8 a live walk and round, and a walk that stops
    # DEAD_END, BRANCH, TARGET or MAX_STEPS is live in as many later rounds as it takes steps
    assert info["queries"] <= n + 8 * int((got[1] + U64(1)).sum())
    assert info["queries"] == 5 * n + (8 if mode == "unitig" else 4) * int(got[1].sum())
    return info


@pytest.mark.parametrize("k,direction,mode", [(21, "right", "unitig"), (31, "left", "unique")])
def test_one_walk_down_the_chain(k, direction, mode):
    b, text = chain()["b"], chain()["text"]
    assert len(set(windows([text], k))) == 5000 - k + 1  # a chain: no k-mer twice
    p = 0 if direction == "right" else 5000 - k
    want = chain_walks(k, [p], 5000, direction)
    assert int(want[1][0]) == 5000 - k and want[2][0] == T.DEAD_END
    got = run(b, words_of([text[p:p + k]]), k, 5000, mode, direction)
    check(got, want, (k, direction))
    assert msbwt.trace_sequences(words_of([text[p:p + k]]), k, got[0], got[1], direction, text=True) == [text]
    info = check_round_structure(b, got, 1, 5000, mode)
    assert info["rounds"] == 5000 - k + 1 and info["longest"] == info["steps"] == 5000 - k
    print("k = %d %s: %s" % (k, direction, info))


@pytest.mark.parametrize("mode", MODES)
def test_every_64th_node_in_one_batch(mode):
    k, max_steps = 21, 300
    b, text = chain()["b"], chain()["text"]
    positions = list(range(0, 5000 - k + 1, 64))
    assert len(positions) == 78 and len(positions) % 64
    for direction in DIRECTIONS:
        want = chain_walks(k, positions, max_steps, direction)
        assert set(want[2].tolist()) == {T.MAX_STEPS, T.DEAD_END} and len(set(want[1].tolist())) > 3  # the walks end in different rounds
        got = run(b, words_of([text[p:p + k] for p in positions]), k, max_steps, mode, direction)
        check(got, want, (mode, direction))
        info = check_round_structure(b, got, len(positions), max_steps, mode)
        assert info["rounds"] == max_steps + 1


@pytest.mark.parametrize("n", [200, 1])
def test_pieces_of_64_walks_give_the_same_bytes(n):
    k, max_steps = 21, 50
    b, text = chain()["b"], chain()["text"]
    positions = [(37 * i) % (5000 - k + 1) for i in range(n)]
    seeds, targets = words_of([text[p:p + k] for p in positions]), words_of([text[p + 30:p + 30 + k] if p + 30 + k <= 5000 else text[:k] for p in positions])
    for mode, direction, tg in (("unitig", "right", None), ("greedy", "left", None), ("unique", "right", targets)):
        auto = run(b, seeds, k, max_steps, mode, direction, targets=tg)
        if tg is None:
            check(auto, chain_walks(k, positions, max_steps, direction), (n, mode, direction))
        else:
            assert (auto[2] == T.TARGET).sum() >= n // 2 and (auto[1][auto[2] == T.TARGET] == 30).all()
        assert check_round_structure(b, auto, n, max_steps, mode, targets=tg is not None)["pieces"] == 1
        b.set_trace_piece(64)
        try:
            pieces = run(b, seeds, k, max_steps, mode, direction, targets=tg)
            info = check_round_structure(b, pieces, n, max_steps, mode, targets=tg is not None, piece=64)
        finally:
            b.set_trace_piece(0)
        assert info["pieces"] == (4 if n == 200 else 1)
        check(pieces, auto, (n, mode, direction, "pieces"))


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
        kmers, words = seeds_of(g, k, rng)
        for mode in MODES:
            for direction in DIRECTIONS:
                check(run(b, words, k, 80, mode, direction), T.expected_arrays(g, kmers, mode, direction, 80), (form, k, mode, direction))
    c = chain()
    b = loaded(c["rle"], **knobs)
    positions = list(range(0, 4970, 64))
    for k, direction in ((21, "right"), (31, "left")):
        got = run(b, words_of([c["text"][p:p + k] for p in positions]), k, 150, "unitig", direction)
        check(got, chain_walks(k, positions, 150, direction), (form, k, direction))


# ---- 6. host form, device form, torch tensors; NULL outputs; n = 0; an empty index ----

def test_host_form_device_form_and_torch_tensors_give_the_same_bytes(orc):
    import torch
    reads = ragged_set(2)
    k, max_steps = 4, 30
    b = loaded(naive_rle(orc, reads))
    g = T.Graph(reads, k)
    kmers, words = seeds_of(g, k, np.random.default_rng(9))
    nodes = sorted(g.nodes)
    targets = words_of([nodes[(7 * i) % len(nodes)] for i in range(len(kmers))])
    dev = torch.device("cuda:0")
    before = b.device_bytes()
    for mode, direction, tg in (("unitig", "right", None), ("greedy", "left", targets), ("unique", "left", None)):
        want = T.expected_arrays(g, kmers, mode, direction, max_steps, None if tg is None else [T.kmer_of(w, k) for w in tg])
        host = run(b, words, k, max_steps, mode, direction, targets=tg)
        check(host, want, ("host", mode, direction))
        d_seeds = torch.from_numpy(words.view(np.int64)).to(dev)
        d_targets = None if tg is None else torch.from_numpy(tg.view(np.int64)).to(dev)
        for stream in (torch.cuda.current_stream(dev), torch.cuda.Stream(dev)):
            with torch.cuda.stream(stream):
                d_symbols = torch.full((len(words), max_steps), SENTINEL, dtype=torch.uint8, device=dev)
                stream.synchronize()
                got = b.trace_kmers(d_seeds, k, max_steps, mode=mode, direction=direction, targets=d_targets, symbols=d_symbols)
                b.device_status(stream.cuda_stream)
            assert got[0] is d_symbols and all(t.device == dev for t in got)
            check([t.cpu().numpy().view(w.dtype) for t, w in zip(got, want)], want, ("torch", mode, direction))
            assert b.trace_info()["scratch_bytes"] == msbwt.trace_plan(len(words), max_steps, mode, targets=tg is not None, host=False)
        # NULL outputs in every combination: what is asked for is what the full call gave, and nothing else is written
        d_full = [torch.from_numpy(w.copy()).to(dev) if w.dtype == np.uint8 else torch.from_numpy(w.view(np.int64).copy()).to(dev) for w in want]
        for wanted in (range(64) if tg is None and mode == "unitig" else (0b101010, 0b010101, 0b000001)):
            outs = [np.full_like(w, SENTINEL) for w in want]
            ptrs = [o.ctypes.data_as(C.c_void_p) if wanted >> j & 1 else None for j, o in enumerate(outs)]
            rc = _lib.lib().msbwt_rle_trace_kmers(b._h, words.ctypes.data_as(C.c_void_p), None if tg is None else tg.ctypes.data_as(C.c_void_p), k, len(words), 1, 0,
                                                  _lib.TRACE_MODES[mode], _lib.TRACE_DIRECTIONS[direction], max_steps, *ptrs)
            assert rc == 0, _lib.lib().msbwt_rle_last_error(b._h)
            for j, (o, w) in enumerate(zip(outs, want)):
                assert np.array_equal(o, w) if wanted >> j & 1 else (o == SENTINEL).all(), (wanted, NAMES[j])
            if wanted % 9 == 0 or wanted == 0b101010:  # the device form, a few of them
                d_outs = [torch.full_like(t, SENTINEL if t.dtype == torch.uint8 else -1) for t in d_full]
                b.trace_kmers_device(d_seeds.data_ptr(), k, len(words), max_steps, *[t.data_ptr() if wanted >> j & 1 else None for j, t in enumerate(d_outs)],
                                     mode=_lib.TRACE_MODES[mode], direction=_lib.TRACE_DIRECTIONS[direction], d_targets=None if tg is None else d_targets.data_ptr(),
                                     stream=torch.cuda.current_stream(dev).cuda_stream)
                b.device_status(torch.cuda.current_stream(dev).cuda_stream)
                for j, (t, f) in enumerate(zip(d_outs, d_full)):
                    assert torch.equal(t, f) if wanted >> j & 1 else bool((t == (SENTINEL if t.dtype == torch.uint8 else -1)).all()), (wanted, NAMES[j])
    assert b.device_bytes() == before
    # n = 0
    got = b.trace_kmers(np.zeros(0, dtype=U64), k, 5)
    assert [g.shape for g in got] == [(0, 5), (0,), (0,), (0,), (0,), (0,)] and not any(b.trace_info().values())
    got = b.trace_kmers(torch.zeros(0, dtype=torch.int64, device=dev), k, 5)
    assert got[0].shape == (0, 5) and got[1].numel() == 0


def test_an_empty_index():
    import torch
    b = loaded(EMPTY)
    k = 7
    words = np.array([0, 5, (1 << 14) - 1, 1 << 14 | 9, 2 ** 64 - 1], dtype=U64)
    for mode in MODES:
        symbols, steps, stops, sums, last, fans = run(b, words, k, 6, mode, "left")
        assert (symbols == SENTINEL).all() and not steps.any() and not sums.any() and not fans.any() and (stops == T.NOT_A_NODE).all()
        assert last.tolist() == [0, 5, (1 << 14) - 1, 9, (1 << 14) - 1]
        info = b.trace_info()
        assert info == {"walks": 5, "rounds": 0, "queries": 0, "steps": 0, "longest": 0, "pieces": 0, "scratch_bytes": 0, "not_nodes": 5}
    dev = torch.device("cuda:0")
    got = b.trace_kmers(torch.from_numpy(words.view(np.int64)).to(dev), k, 6, mode="unitig")
    assert not got[0].any() and (got[2] == T.NOT_A_NODE).all() and got[4].cpu().numpy().view(U64).tolist() == [0, 5, (1 << 14) - 1, 9, (1 << 14) - 1]
    assert b.trace_kmers(np.zeros(0, dtype=U64), k, 6)[1].size == 0
