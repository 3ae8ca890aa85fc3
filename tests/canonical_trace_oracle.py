"""What a canonical trace IS (include/msbwt_hip.h, "canonical traces"), over strings: the traces' steps 0-8 with the section's changes,
literally, through the strand-merged graph D of the Counters of the reads' windows at k and at k + 1.  Nothing here comes from the
library; the words, the codes and the stops 1-7 are tests/trace_oracle.py's."""
import numpy as np

import trace_oracle as T
from test_gpu_kmer_graph import thresholds, windows
from trace_oracle import BRANCH, DEAD_END, MAX_STEPS, MERGE, NOT_A_NODE, RETURNED, TARGET, kmer_of, sequence, word_of  # noqa: F401 (for the tests)

MIRROR = 8
STOP_NAMES = {**T.STOP_NAMES, MIRROR: "MIRROR"}
COMPLEMENT = str.maketrans("ACGT", "TGCA")
U64 = np.uint64


def rc(s):
    return s.translate(COMPLEMENT)[::-1]


class Graph:
    """D(k, m, me) of reads given as strings: cc(x) = count(x) + count(rc(x)), a palindrome once; both members of every class with
    cc >= m are nodes; q -> q' by c is an edge when cc(q.c) >= me and q' is a node."""

    def __init__(self, reads, k, min_count=1, min_edge=0):
        self.m, self.me = thresholds(min_count, min_edge)
        self.k = k
        self.at_k, self.at_k1 = windows(reads, k), windows(reads, k + 1)
        occur = set(self.at_k) | {rc(q) for q in self.at_k}
        self.nodes = {q: self.cc(q) for q in occur if self.cc(q) >= self.m}
        self.below = sorted(q for q in occur if self.cc(q) < self.m)  # k-mers that occur on either strand and are no nodes
        self._fans = {}

    def cc(self, x):
        counter = self.at_k if len(x) == self.k else self.at_k1  # (a Counter answers 0 for what it does not hold)
        r = rc(x)
        return counter[x] if r == x else counter[x] + counter[r]

    def fan(self, q, direction, back=False):
        """[(symbol, edge, far end)] of the edges of D that leave q in the walk direction (back: that enter it), in A C G T order"""
        right = (direction == "right") != back
        if (q, right) not in self._fans:  # (looked up once a node and side)
            found = []
            for c in "ACGT":
                e = q + c if right else c + q
                far = e[1:] if right else e[:-1]
                if self.cc(e) >= self.me and far in self.nodes:
                    found.append((c, e, far))
            self._fans[q, right] = found
        return self._fans[q, right]


def trace(g, seed, mode="unique", direction="right", max_steps=10, target=None):
    """one walk -> (symbols appended or prepended, as a str; steps; stop; edge_sum; last node; fan bits of the last node)"""
    def done(stop):
        bits = 0 if stop == NOT_A_NODE else sum(1 << "ACGT".index(c) for c, _, _ in g.fan(cur, direction))
        return "".join(symbols), steps, stop, edge_sum, cur, bits

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
        c, e, nxt = max(fan, key=lambda f: (g.cc(f[1]), -"ACGT".index(f[0])))  # the largest cc, on a tie the smallest symbol
        if mode == "unitig" and (rc(cur) == cur or rc(nxt) == nxt or rc(e) == e):
            return done(MIRROR)                                     # 3b
        if mode == "unitig" and len(g.fan(nxt, direction, back=True)) >= 2:
            return done(MERGE)                                      # 4
        if nxt == seed:
            return done(RETURNED)                                   # 5
        symbols.append(c)                                           # 6
        edge_sum += g.cc(e)
        steps += 1
        cur = nxt
        if target is not None and cur == target:
            return done(TARGET)                                     # 7


def expected_arrays(g, seeds, mode, direction, max_steps, targets=None, sentinel=0xEE):
    """The six outputs of a batch as the library returns them, for seeds (and targets) given as strings: the rows' tails hold `sentinel`."""
    n = len(seeds)
    symbols = np.full((n, max_steps), sentinel, dtype=np.uint8)
    steps, edge_sums, last = np.zeros(n, dtype=U64), np.zeros(n, dtype=U64), np.zeros(n, dtype=U64)
    stops, fans = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    for i, s in enumerate(seeds):
        row, steps[i], stops[i], edge_sums[i], end, fans[i] = trace(g, s, mode, direction, max_steps, None if targets is None else targets[i])
        symbols[i, :len(row)] = [T.CODE[c] for c in row]
        last[i] = word_of(end)
    return symbols, steps, stops, edge_sums, last, fans


def mirrored(result):
    """the trace of rc(s) in the other direction, from the trace of s (UNIQUE and UNITIG): symbols complemented, last reverse-
    complemented, fan bits reversed"""
    symbols, steps, stop, edge_sum, last, fan = result
    return symbols.translate(COMPLEMENT), steps, stop, edge_sum, rc(last), sum(1 << (3 - j) for j in range(4) if fan >> j & 1)
