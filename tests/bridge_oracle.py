"""What a bridge call IS (include/msbwt_hip.h, "bridges"), over strings: the header's steps 0-1 literally -- the levels W and E as lists of
walks in their defined order -- on the Graph of tests/trace_oracle.py.  Nothing here comes from the library."""
import numpy as np

from trace_oracle import CODE, Graph, word_of  # noqa: F401  (Graph and word_of are what the tests build their cases with)

EXHAUSTED, FULL, MAX_STEPS, TOO_WIDE, NO_SEED, NO_TARGET = 1, 2, 3, 4, 5, 6
STOP_NAMES = {1: "EXHAUSTED", 2: "FULL", 3: "MAX_STEPS", 4: "TOO_WIDE", 5: "NO_SEED", 6: "NO_TARGET"}
U64 = np.uint64


class Result:
    """one pair: rows = [(symbols in walk order, edge sum)] of the bridges WRITTEN; found, stop, depth, live; and what the call spends --
    levels[r] = |W(r)| of every level that goes on (levels[0] = 1 for a pair that starts), expanded = the sum of |E(r)|"""

    def __init__(self):
        self.rows, self.found, self.stop, self.depth, self.live, self.levels, self.expanded = [], 0, 0, 0, 0, [], 0

    def done(self, stop, live=0):
        self.stop, self.live = stop, live
        return self


def bridges(g, seed, target, direction="right", min_steps=0, max_steps=10, max_paths=4, max_live=64):
    """one pair -> Result"""
    res, right, lo = Result(), direction == "right", max(min_steps, 1)
    if seed not in g.nodes:
        return res.done(NO_SEED)                                             # 0
    if target not in g.nodes:
        return res.done(NO_TARGET)
    W = [("", seed, 0)]                                                      # 1: (symbols, the node stood on, edge sum)
    r = 0
    while True:
        r += 1
        if max_steps == 0:
            return res.done(MAX_STEPS, len(W))                               # expand
        res.levels.append(len(W))
        E = [(row + c, e[1:] if right else e[:-1], total + g.edges[e]) for row, node, total in W for c, e in g.fan(node, direction)]
        res.expanded += len(E)
        B = [w for w in E if w[1] == target] if r >= lo else []              # collect
        for row, _, total in B:
            if res.found < max_paths:
                res.rows.append((row, total))
            res.found += 1
        W = [w for w in E if w[1] != target] if r >= lo else E            # E \ B
        res.depth = r
        if res.found >= max_paths:                                           # stop
            return res.done(FULL, len(W))
        if not W:
            return res.done(EXHAUSTED, 0)
        if r == max_steps:
            return res.done(MAX_STEPS, len(W))
        if len(W) > max_live:
            return res.done(TOO_WIDE, len(W))


def sequence(seed, symbols, direction):
    """the full sequence of a bridge, in reading order"""
    return seed + symbols if direction == "right" else symbols[::-1] + seed


def results(g, seeds, targets, direction, min_steps, max_steps, max_paths, max_live):
    """a batch -> [Result]; a pair that occurs again is explored once"""
    seen = {}
    return [seen.get((s, t)) or seen.setdefault((s, t), bridges(g, s, t, direction, min_steps, max_steps, max_paths, max_live)) for s, t in zip(seeds, targets)]


def expected_arrays(g, seeds, targets, direction, min_steps, max_steps, max_paths, max_live, sentinel=0xEE, res=None):
    """The seven outputs of a batch as the library returns them, for seeds and targets given as strings: the tails of the rows of
    symbols, and the unused rows, hold `sentinel`."""
    n = len(seeds)
    res = res or results(g, seeds, targets, direction, min_steps, max_steps, max_paths, max_live)
    symbols = np.full((n, max_paths, max_steps), sentinel, dtype=np.uint8)
    lengths, edge_sums = np.zeros((n, max_paths), dtype=U64), np.zeros((n, max_paths), dtype=U64)
    found, depths, live, stops = np.zeros(n, dtype=U64), np.zeros(n, dtype=U64), np.zeros(n, dtype=U64), np.zeros(n, dtype=np.uint8)
    for i, p in enumerate(res):
        found[i], stops[i], depths[i], live[i] = p.found, p.stop, p.depth, p.live
        for j, (row, total) in enumerate(p.rows):
            symbols[i, j, :len(row)] = [CODE[c] for c in row]
            lengths[i, j], edge_sums[i, j] = len(row), total
    return symbols, lengths, edge_sums, found, stops, depths, live


def expected_info(res, pieces):
    """what msbwt_rle_bridge_info says of a batch whose pieces are the lists of indices `pieces`: queries (6 a pair, then 4 a state of
    every level that goes on), expanded, found, rounds (round 0 and every expansion a piece) and the widest frontier"""
    queries = 6 * len(res) + 4 * sum(sum(p.levels[1:]) for p in res)
    rounds = sum(1 + max(p.depth for p in (res[i] for i in piece)) for piece in pieces)
    widest = 0
    for piece in pieces:
        mine = [res[i] for i in piece]
        widest = max([widest, len(mine)] + [sum(p.levels[r] for p in mine if len(p.levels) > r) for r in range(1, max(len(p.levels) for p in mine))])
    return dict(pairs=len(res), rounds=rounds, queries=queries, expanded=sum(p.expanded for p in res), found=sum(p.found for p in res), pieces=len(pieces),
                widest=widest)
