"""tests/bridge_oracle.py, the definition of a bridge call over strings, held against things that are not it: brute force over every
string of every length at k = 2 and 3, the trace oracle where a trace runs into its target, and the invariant the header states for
every stop code.  No GPU, nothing from the library."""
import itertools

import numpy as np
import pytest

import bridge_oracle as B
import trace_oracle as T
from test_gpu_reads_build import ragged_set
from test_trace_oracle import HAND

DIRECTIONS = ("right", "left")
seen_stops = set()


def is_walk(g, seed, row, direction):
    """the nodes of the walk from seed along the symbols of row, or None where an edge is missing"""
    nodes, cur = [], seed
    for c in row:
        e = cur + c if direction == "right" else c + cur
        if e not in g.edges:
            return None
        cur = e[1:] if direction == "right" else e[:-1]
        nodes.append(cur)
    return nodes


def brute_force(g, seed, target, direction, lo, length):
    """every bridge of exactly `length` symbols, in lexicographic order: a walk that ends on the target and did not stand on it at any
    earlier step from lo on (a bridge is not extended through its target)"""
    out = []
    for row in map("".join, itertools.product("ACGT", repeat=length)):
        nodes = is_walk(g, seed, row, direction)
        if nodes and nodes[-1] == target and target not in nodes[lo - 1:-1]:
            out.append((row, sum(g.edges[(n0 + c) if direction == "right" else (c + n0)] for n0, c in zip([seed] + nodes[:-1], row))))
    return out


def texts(seed, n, length):
    rng = np.random.default_rng(seed)
    return ["".join(rng.choice(list("ACGT"), size=length)) for _ in range(n)]


@pytest.mark.parametrize("k,reads", [(2, texts(1, 2, 14)), (2, texts(2, 1, 40)), (3, texts(3, 3, 30)), (3, texts(4, 2, 80)), (3, ["AAAAAAAC", "CAAAAG"])])
def test_against_every_string_of_every_length(k, reads):
    g = T.Graph(reads, k)
    nodes = sorted(g.nodes)
    rng = np.random.default_rng(len(nodes))
    pairs = [(nodes[i], nodes[j]) for i, j in rng.integers(0, len(nodes), size=(14, 2))] + [(nodes[0], nodes[0]), (nodes[-1], nodes[-1])]
    bridged = 0
    for direction in DIRECTIONS:
        for seed, target in pairs:
            for min_steps, max_steps in ((0, 6), (3, 5), (4, 4), (0, 1)):
                lo = max(min_steps, 1)
                want = [b for length in range(lo, max_steps + 1) for b in brute_force(g, seed, target, direction, lo, length)]
                got = B.bridges(g, seed, target, direction, min_steps, max_steps, max_paths=10 ** 6, max_live=10 ** 6)
                assert got.stop in (B.EXHAUSTED, B.MAX_STEPS) and got.found == len(want) and got.rows == want, (seed, target, direction, min_steps, max_steps)
                assert got.depth == max_steps or got.stop == B.EXHAUSTED
                seen_stops.add(got.stop)
                bridged += len(want)
                # a budget of rows: the first max_paths in the order (length, then symbols), and found counts every bridge up to depth
                for max_paths in (1, 3):
                    cut = B.bridges(g, seed, target, direction, min_steps, max_steps, max_paths=max_paths, max_live=10 ** 6)
                    upto = [b for b in want if len(b[0]) <= cut.depth]
                    assert cut.rows == want[:max_paths][:len(cut.rows)] == upto[:max_paths] and cut.found == len(upto)
                    assert (cut.stop == B.FULL) == (len(upto) >= max_paths)
                    seen_stops.add(cut.stop)
    assert bridged > 10  # (no vacuous case set)


def every_case():
    for seed in (0, 1, 2, 5, 11):
        reads = ragged_set(seed)
        for k in (1, 2, 3, 5, 16):
            for min_count, min_edge in ((1, 0), (2, 0), (1, 3)):
                yield reads, k, min_count, min_edge
    for reads in HAND:
        for min_count, min_edge in ((1, 0), (2, 3)):
            yield reads, 5, min_count, min_edge


def test_a_unique_trace_into_its_target_is_the_one_bridge():
    checked = 0
    for reads, k, min_count, min_edge in every_case():
        g = T.Graph(reads, k, min_count, min_edge)
        for direction in DIRECTIONS:
            for seed in sorted(g.nodes):
                # the node the UNIQUE trace ends on, made its target: a walk along a path that never branches
                row, steps, stop, edge_sum, last, _ = T.trace(g, seed, "unique", direction, 30)
                if steps == 0:
                    continue
                row2, steps2, stop2, edge_sum2, last2, _ = T.trace(g, seed, "unique", direction, 30, target=last)
                if stop2 != T.TARGET:
                    continue
                got = B.bridges(g, seed, last2, direction, 0, steps2, max_paths=4, max_live=64)
                assert got.rows == [(row2, edge_sum2)] and got.found == 1 and got.depth == steps2 and got.stop == B.EXHAUSTED and got.live == 0
                checked += 1
    assert checked > 500


def test_bridges_up_to_depth_are_all_counted_whatever_the_stop():
    """found against an exploration that knows no budget, cut at the depth the budgeted one reached"""
    stops = set()
    for reads, k, min_count, min_edge in every_case():
        g = T.Graph(reads, k, min_count, min_edge)
        nodes = sorted(g.nodes) + g.below[:1] + ["G" * k]
        rng = np.random.default_rng(k + len(nodes))
        for seed, target in ((nodes[i], nodes[j]) for i, j in rng.integers(0, len(nodes), size=(12, 2))):
            for direction in DIRECTIONS:
                for min_steps, max_steps, max_paths, max_live in ((0, 12, 2, 2), (3, 12, 1, 8), (0, 0, 3, 1), (2, 7, 3, 1), (0, 20, 50, 3)):
                    got = B.bridges(g, seed, target, direction, min_steps, max_steps, max_paths, max_live)
                    stops.add(got.stop)
                    assert 1 <= got.stop <= 6 and got.depth <= max_steps and len(got.rows) == min(got.found, max_paths)
                    if got.stop in (B.NO_SEED, B.NO_TARGET):
                        assert (got.found, got.depth, got.live, got.rows) == (0, 0, 0, []) and (seed not in g.nodes or target not in g.nodes)
                        continue
                    free = B.bridges(g, seed, target, direction, min_steps, got.depth, 10 ** 9, 10 ** 9)
                    assert got.found == free.found and got.rows == free.rows[:max_paths], (seed, target, direction, got.stop)
                    assert [len(r) for r, _ in got.rows] == sorted(len(r) for r, _ in got.rows) and all(len(r) >= max(min_steps, 1) for r, _ in got.rows)
                    assert all(is_walk(g, seed, r, direction)[-1] == target for r, _ in got.rows)
                    if got.stop == B.EXHAUSTED:  # no longer bridge exists
                        assert B.bridges(g, seed, target, direction, min_steps, got.depth + 6, 10 ** 9, 10 ** 9).found == got.found and got.live == 0
                    if got.stop == B.TOO_WIDE:
                        assert got.live > max_live and got.depth < max_steps and got.found < max_paths
                    if got.stop == B.MAX_STEPS:
                        assert got.depth == max_steps and got.found < max_paths and (got.live > 0)
                    if got.stop == B.FULL:
                        assert got.found >= max_paths
    # every stop code occurs in this file's cases: no case set can silently miss one
    assert stops == {B.EXHAUSTED, B.FULL, B.MAX_STEPS, B.TOO_WIDE, B.NO_SEED, B.NO_TARGET}, stops


def test_hand_made_graphs():
    k = 5
    # a bubble: two bridges of equal length, in lexicographic order
    g = T.Graph(["TTACGCATGGA", "TTACGGATGGA"], k)
    got = B.bridges(g, "TTACG", "ATGGA", "right", 0, 10)
    assert [r for r, _ in got.rows] == ["CATGGA", "GATGGA"] and (got.found, got.stop, got.depth) == (2, B.EXHAUSTED, 6)
    assert [B.sequence("TTACG", r, "right") for r, _ in got.rows] == ["TTACGCATGGA", "TTACGGATGGA"]
    got = B.bridges(g, "ATGGA", "TTACG", "left", 0, 10)
    assert [B.sequence("ATGGA", r, "left") for r, _ in got.rows] == ["TTACGCATGGA", "TTACGGATGGA"]
    # arms of different length: the shorter first
    g = T.Graph(["TTACGTCATGGA", "TTACGATGGA"], k)
    got = B.bridges(g, "TTACG", "ATGGA", "right", 0, 10)
    assert [r for r, _ in got.rows] == ["ATGGA", "TCATGGA"] and got.stop == B.EXHAUSTED
    assert B.bridges(g, "TTACG", "ATGGA", "right", 0, 10, max_paths=1).stop == B.FULL
    assert B.bridges(g, "TTACG", "ATGGA", "right", 0, 6).rows == got.rows[:1] and B.bridges(g, "TTACG", "ATGGA", "right", 0, 6).stop == B.MAX_STEPS
    # a tandem repeat: a walk ends where it first enters the target from lo on, and min_steps selects the second arrival
    g = T.Graph(["GGACTTCACTTCACTTG"], k)
    got = B.bridges(g, "GGACT", "CACTT", "right", 0, 20, max_paths=2)
    assert [r for r, _ in got.rows] == ["TCACTT"] and got.stop == B.EXHAUSTED
    assert [r for r, _ in B.bridges(g, "GGACT", "CACTT", "right", 7, 20, max_paths=1).rows] == ["TCACTTCACTT"]
    # a dead-end tip
    g = T.Graph(["ACGTACCGGT", "TTTTTTT"], k)
    got = B.bridges(g, "ACGTA", "TTTTT", "right", 0, 20)
    assert (got.found, got.stop, got.depth, got.rows) == (0, B.EXHAUSTED, 6, [])
    # seed == target on a self-loop and on a cycle
    assert B.bridges(T.Graph(["AAAAAAAA"], k), "AAAAA", "AAAAA", "right", 0, 5).rows == [("A", 3)]
    assert [r for r, _ in B.bridges(T.Graph(["ACGTTGCAGACGTT"], k), "ACGTT", "ACGTT", "right", 0, 20).rows] == ["GCAGACGTT"]
