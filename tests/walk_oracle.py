"""The left walks of include/msbwt_hip.h ("left walks") on the BWT string alone, for the tests: nothing of the library, numpy only.

S is the decoded BWT of T rows, C[c] the rows holding a symbol below c, LF(r) = C[S[r]] + rank(S[r], r).  A walk from r0 emits S[r]
and goes to LF(r) until it stands on a '$' (code 0; neither emitted nor counted: DOLLAR, which wins at steps == max_steps) or has
taken max_steps steps (MAX_STEPS); r0 >= T is BAD_ROW.  `Decoded` holds S itself; `Runs` answers the same two questions -- the symbol
at a row, LF of a row -- from a run list in closed form, for streams too long to decode."""
import numpy as np

DOLLAR, MAX_STEPS, BAD_ROW = 1, 2, 3
STOP_NAMES = ("", "DOLLAR", "MAX_STEPS", "BAD_ROW")
NO_READ = np.uint64(2 ** 64 - 1)
U64 = np.uint64


class Decoded:
    """S as an array of symbol codes 0..5"""

    def __init__(self, symbols):
        self.S = np.ascontiguousarray(symbols, dtype=np.uint8)
        self.T = int(self.S.size)
        counts = np.bincount(self.S, minlength=6).astype(np.int64)
        self.C = np.concatenate([[0], np.cumsum(counts)[:-1]])
        self.reads = int(counts[0])
        self.lf = np.zeros(self.T, dtype=np.int64)
        for c in range(6):
            at = np.flatnonzero(self.S == c)
            self.lf[at] = self.C[c] + np.arange(at.size)  # rank(c, r) = how many c stand before r

    def step(self, r):
        return int(self.S[r]), int(self.lf[r])

    def step_many(self, r):
        return self.S[r].astype(np.int64), self.lf[r]


class Runs:
    """S as (symbol, length) runs: rows [starts[j], starts[j] + lens[j]) hold syms[j]"""

    def __init__(self, syms, lens):
        self.syms = np.asarray(syms, dtype=np.int64)
        self.lens = np.asarray(lens, dtype=np.int64)
        self.ends = np.cumsum(self.lens)
        self.starts = self.ends - self.lens
        self.T = int(self.ends[-1]) if self.lens.size else 0
        counts = np.array([int(self.lens[self.syms == c].sum()) for c in range(6)], dtype=np.int64)
        self.C = np.concatenate([[0], np.cumsum(counts)[:-1]])
        self.reads = int(counts[0])
        self.before = np.zeros(self.lens.size, dtype=np.int64)  # occurrences of a run's own symbol in the runs before it
        for c in range(6):
            mine = self.syms == c
            self.before[mine] = np.cumsum(self.lens[mine]) - self.lens[mine]

    def step(self, r):
        j = int(np.searchsorted(self.ends, r, side="right"))
        s = int(self.syms[j])
        return s, int(self.C[s] + self.before[j] + (r - self.starts[j]))

    def step_many(self, r):
        j = np.searchsorted(self.ends, r, side="right")
        s = self.syms[j]
        return s, self.C[s] + self.before[j] + (r - self.starts[j])


def walk(index, r0, max_steps):
    """-> (symbols emitted, in walk order; stop; the row the walk stands on; the read, or None)"""
    if r0 >= index.T:
        return [], BAD_ROW, r0, None
    out, r = [], int(r0)
    while True:
        s, nxt = index.step(r)
        if s == 0:
            return out, DOLLAR, r, nxt  # C['$'] = 0: LF of a '$' row is rank('$', r), the read
        if len(out) == max_steps:
            return out, MAX_STEPS, r, None
        out.append(s)
        r = nxt


def expected_arrays(index, rows, max_steps, fill=0):
    """(symbols, steps, stops, last, reads) as msbwt_rle_walk_rows leaves them, rows of symbols pre-filled with `fill`: walk() for
    every row, all rows a step at a time"""
    rows = np.array([int(r) for r in rows], dtype=U64)
    n = rows.size
    symbols = np.full((n, max_steps), fill, dtype=np.uint8)
    steps, reads = np.zeros(n, dtype=U64), np.full(n, NO_READ, dtype=U64)
    inside = rows < U64(index.T)
    stops = np.where(inside, 0, BAD_ROW).astype(np.uint8)
    cur, live = np.where(inside, rows, 0).astype(np.int64), inside.copy()
    for t in range(max_steps + 1):
        at = np.flatnonzero(live)
        if at.size == 0:
            break
        s, nxt = index.step_many(cur[at])
        dollar = s == 0
        stops[at[dollar]], reads[at[dollar]], live[at[dollar]] = DOLLAR, nxt[dollar], False
        go = at[~dollar]
        if t == max_steps:
            stops[go], live[go] = MAX_STEPS, False
            break
        symbols[go, t], cur[go] = s[~dollar], nxt[~dollar]
        steps[go] += U64(1)
    return symbols, steps, stops, np.where(inside, cur.astype(U64), rows), reads


def extract(index, ids, max_len):
    """(symbols, offsets, truncated) as msbwt_rle_extract_reads leaves them: read i in reading order, its last max_len symbols when it is longer"""
    parts, truncated = [], 0
    for i in ids:
        assert 0 <= int(i) < index.reads
        out, stop, _, _ = walk(index, int(i), max_len)
        truncated += stop == MAX_STEPS
        parts.append(np.array(out[::-1], dtype=np.uint8))
    offsets = np.zeros(len(parts) + 1, dtype=U64)
    if parts:
        np.cumsum([p.size for p in parts], out=offsets[1:])
    return (np.concatenate(parts) if parts else np.empty(0, dtype=np.uint8)), offsets, truncated


def locate(index, rows, max_steps):
    """(reads, offsets, stops) of RleBWT.locate_rows"""
    _, steps, stops, _, reads = expected_arrays(index, rows, max_steps)
    return reads, steps, stops
