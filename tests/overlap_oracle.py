"""The read overlaps of include/msbwt_hip.h ("read overlaps") on the BWT string alone, for the tests: nothing of the library, numpy only.

S is the decoded BWT of T rows, C[c] the rows holding a symbol below c, rank(c, r) the occurrences of c in S[0 .. r) and
constrain(c, [l, h)) = [C[c] + rank(c, l), C[c] + rank(c, h)).  A query Q of L codes is searched backwards (strand 1: its reverse
complement) from R_0 = [0, T), j = 0:
  1. j >= m and D_j = [rank('$', l_j), rank('$', h_j)) not empty: the record (j, D_j.l, D_j.h - D_j.l)
  2. j == E = min(L, M) (M = 0: L): END
  3. c = Q'[L - 1 - j] is 0 or above 5: BAD_SYMBOL
  4. R_(j+1) = constrain(c, R_j) empty: EMPTY; else j += 1, back to 1
An index of no rows answers EMPTY with nothing matched.  `Decoded` holds S itself; `Runs` answers rank from a run list in closed
form, for streams too long to decode."""
import numpy as np

END, EMPTY, BAD_SYMBOL = 1, 2, 3
STOP_NAMES = ("", "END", "EMPTY", "BAD_SYMBOL")
COMPLEMENT = (0, 5, 3, 2, 4, 1)
U64 = np.uint64


class Decoded:
    """S as an array of symbol codes 0..5"""

    def __init__(self, symbols):
        self.S = np.ascontiguousarray(symbols, dtype=np.uint8)
        self.T = int(self.S.size)
        counts = np.bincount(self.S, minlength=6).astype(np.int64)
        self.C = [0] + [int(x) for x in np.cumsum(counts)]  # C[6] = T
        self.before = [np.concatenate([[0], np.cumsum(self.S == c)]) for c in range(6)]

    def rank(self, c, r):
        return int(self.before[c][r])


class Runs:
    """S as (symbol, length) runs"""

    def __init__(self, syms, lens):
        self.syms = np.asarray(syms, dtype=np.int64)
        self.lens = np.asarray(lens, dtype=np.int64)
        self.ends = np.cumsum(self.lens)
        self.starts = self.ends - self.lens
        self.T = int(self.ends[-1]) if self.lens.size else 0
        counts = [int(self.lens[self.syms == c].sum()) for c in range(6)]
        self.C = [0] + [int(x) for x in np.cumsum(counts)]
        # occurrences of c before every run's start
        self.before = [np.cumsum(np.where(self.syms == c, self.lens, 0)) - np.where(self.syms == c, self.lens, 0) for c in range(6)]

    def rank(self, c, r):
        if r >= self.T:
            return self.C[c + 1] - self.C[c]
        j = int(np.searchsorted(self.ends, r, side="right"))  # the run that holds row r
        return int(self.before[c][j]) + (int(r - self.starts[j]) if int(self.syms[j]) == c else 0)


def searched(query, strand):
    """Q': the codes as given, or their reverse complement (a code above 5 stays what it is)"""
    q = [int(x) for x in query]
    return q if strand == 0 else [COMPLEMENT[x] if x < 6 else x for x in reversed(q)]


def search(index, query, m, M=0, strand=0, trace=None):
    """-> (records [(j, first, count)], matched, edges, stop); trace: a list that receives (j, l_j, h_j) of every step whose ranks are taken"""
    assert m >= 1
    if index.T == 0:
        return [], 0, 0, EMPTY
    q = searched(query, strand)
    L = len(q)
    E = min(L, M) if M else L
    l, h, j, records = 0, index.T, 0, []
    while True:
        if j >= m:
            a, b = index.rank(0, l), index.rank(0, h)
            if b > a:
                records.append((j, a, b - a))
        if j == E:
            stop = END
            break
        c = q[L - 1 - j]
        if c == 0 or c > 5:
            stop = BAD_SYMBOL
            break
        if trace is not None and j >= 1:
            trace.append((j, l, h))
        nl, nh = index.C[c] + index.rank(c, l), index.C[c] + index.rank(c, h)
        if nl >= nh:
            stop = EMPTY
            break
        l, h, j = nl, nh, j + 1
    return records, j, sum(r[2] for r in records), stop


class Expected:
    """what msbwt_rle_read_overlaps leaves for a batch: offsets (n + 1), the three columns, matched, edges, stops"""

    def __init__(self, index, queries, m, M=0, strand=0):
        got = [search(index, q, m, M, strand) for q in queries]
        n = len(got)
        self.offsets = np.zeros(n + 1, dtype=U64)
        if n:
            np.cumsum([len(g[0]) for g in got], out=self.offsets[1:])
        flat = [r for g in got for r in g[0]]
        self.lengths = np.array([r[0] for r in flat], dtype=U64)
        self.first = np.array([r[1] for r in flat], dtype=U64)
        self.counts = np.array([r[2] for r in flat], dtype=U64)
        self.matched = np.array([g[1] for g in got], dtype=U64)
        self.edges = np.array([g[2] for g in got], dtype=U64)
        self.stops = np.array([g[3] for g in got], dtype=np.uint8)
        self.total = len(flat)


def edges_by_strings(queries, reads_sorted, m, M=0, strand=0, letters=True):
    """{(query, read, length)}: every read of the sorted set that begins with the last `length` symbols of the query searched, by string
    comparison; a query stops being searched where a symbol is no A C G N T.  Strings over ACGNT."""
    comp = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
    out = set()
    for qi, q in enumerate(queries):
        if strand:
            q = "".join(comp.get(x, x) for x in reversed(q))
        E = min(len(q), M) if M else len(q)
        for j in range(m, E + 1):
            suffix = q[len(q) - j:]
            if any(x not in comp for x in suffix):
                break
            for ri, r in enumerate(reads_sorted):
                if r.startswith(suffix):
                    out.add((qi, ri, j))
    return out
