"""What a trace IS (include/msbwt_hip.h, "traces"), over strings: the header's steps 0-8 literally, on the Counters of the reads'
windows at k and at k + 1.  Nothing here comes from the library."""
import numpy as np

from test_gpu_kmer_graph import thresholds, windows

DEAD_END, BRANCH, MERGE, RETURNED, TARGET, MAX_STEPS, NOT_A_NODE = 1, 2, 3, 4, 5, 6, 7
STOP_NAMES = {1: "DEAD_END", 2: "BRANCH", 3: "MERGE", 4: "RETURNED", 5: "TARGET", 6: "MAX_STEPS", 7: "NOT_A_NODE"}
CODE = {"A": 1, "C": 2, "G": 3, "T": 5}
U64 = np.uint64


class Graph:
    """G(k, m, me) of reads given as strings: the nodes with their counts, and the counts of the solid edges"""

    def __init__(self, reads, k, min_count=1, min_edge=0):
        m, me = thresholds(min_count, min_edge)
        self.k = k
        self.nodes = {q: n for q, n in windows(reads, k).items() if n >= m}
        self.below = sorted(q for q, n in windows(reads, k).items() if n < m)  # k-mers that occur and are no nodes
        self.edges = {e: n for e, n in windows(reads, k + 1).items() if n >= me}
        self._fans = {}

    def fan(self, q, direction, back=False):
        """[(symbol, edge)] of the edges that leave q in the walk direction (back: that enter it), in A C G T order"""
        right = (direction == "right") != back
        if (q, right) not in self._fans:  # (looked up once a node and side)
            self._fans[q, right] = [(c, q + c if right else c + q) for c in "ACGT" if (q + c if right else c + q) in self.edges]
        return self._fans[q, right]


def trace(g, seed, mode="unique", direction="right", max_steps=10, target=None):
    """one walk -> (symbols appended or prepended, as a str; steps; stop; edge_sum; last node; fan bits of the last node)"""
    def done(stop):
        bits = 0 if stop == NOT_A_NODE else sum(1 << "ACGT".index(c) for c, _ in g.fan(cur, direction))
        return "".join(symbols), steps, stop, edge_sum, cur, bits

    right = direction == "right"
    cur, steps, edge_sum, symbols = seed, 0, 0, []
    if seed not in g.nodes:
        return done(NOT_A_NODE)                                     # 0
    while True:
        if steps == max_steps:
            return done(MAX_STEPS)                                  # 1
        fan = g.fan(cur, direction)
        if not fan:
            return done(DEAD_END)                                   # 2
        if len(fan) >= 2 and mode != "greedy":
            return done(BRANCH)                                     # 3
        c, e = max(fan, key=lambda ce: (g.edges[ce[1]], -"ACGT".index(ce[0])))  # the largest count, on a tie the smallest symbol
        nxt = e[1:] if right else e[:-1]
        if mode == "unitig" and len(g.fan(nxt, direction, back=True)) >= 2:
            return done(MERGE)                                      # 4
        if nxt == seed:
            return done(RETURNED)                                   # 5
        symbols.append(c)                                           # 6
        edge_sum += g.edges[e]
        steps += 1
        cur = nxt
        if target is not None and cur == target:
            return done(TARGET)                                     # 7


def sequence(seed, symbols, direction):
    """the full sequence of a walk, in reading order"""
    return seed + symbols if direction == "right" else symbols[::-1] + seed


def word_of(kmer):
    w = 0
    for c in kmer:
        w = w << 2 | "ACGT".index(c)
    return w


def kmer_of(word, k):
    return "".join("ACGT"[(int(word) >> (2 * (k - 1 - i))) & 3] for i in range(k))


def expected_arrays(g, seeds, mode, direction, max_steps, targets=None, sentinel=0xEE):
    """The six outputs of a batch as the library returns them, for seeds (and targets) given as strings: the rows' tails hold `sentinel`."""
    n = len(seeds)
    symbols = np.full((n, max_steps), sentinel, dtype=np.uint8)
    steps, edge_sums, last = np.zeros(n, dtype=U64), np.zeros(n, dtype=U64), np.zeros(n, dtype=U64)
    stops, fans = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    for i, s in enumerate(seeds):
        row, steps[i], stops[i], edge_sums[i], end, fans[i] = trace(g, s, mode, direction, max_steps, None if targets is None else targets[i])
        symbols[i, :len(row)] = [CODE[c] for c in row]
        last[i] = word_of(end)
    return symbols, steps, stops, edge_sums, last, fans
