"""A numpy oracle for the link table of the unitig graph calls (include/msbwt_hip.h, "unitig links"), and the brute force it is held to.

link_table() works from the unitigs an oracle returned -- tests/graph_oracle.py's, or the string oracles' of test_gpu_unitigs.py and
test_gpu_canonical_unitigs.py -- through their first and last words and their ends bytes alone: the word an edge out of a side reaches
is looked up among the first words (entry 2v) and among the sorted reverse complements of the last words (entry 2v + 1), with
searchsorted.  brute_links() does not look at an ends byte: it takes the nodes and the edges from the reads' windows, as the string
oracles do, and walks every side of every sequence symbol by symbol with two dicts over strings.  tests/test_link_oracle.py holds the
first to the second.  Nothing here calls the library."""
import numpy as np

import graph_oracle as G
from test_gpu_kmer_graph import thresholds, windows
from test_gpu_spectrum import word_of

U64 = np.uint64
REVERSED = np.array([int("{:04b}".format(x)[::-1], 2) for x in range(16)], dtype=np.int64)  # a nibble with bit j at 3 - j
COMPLEMENT = str.maketrans("ACGT", "TGCA")


def rc(s):
    return s.translate(COMPLEMENT)[::-1]


def words_of(column):
    """a unitig oracle's "first" or "last": words already, or k-mers as strings"""
    if isinstance(column, np.ndarray):
        return column.astype(U64)
    return np.array([word_of(q) for q in column], dtype=U64)


def link_table(unitigs, k, canonical):
    """(link_offsets, link_targets, flags) of the unitigs of an oracle: 2 U + 1 offsets, L targets, and the flags with bit 1 set on a
    unitig that is its own reverse complement (canonical only)"""
    first, last, ends = words_of(unitigs["first"]), words_of(unitigs["last"]), unitigs["ends"].astype(np.int64)
    U = len(first)
    assert (first[1:] > first[:-1]).all()  # ascending by first word: searchsorted may look there
    mask = U64((1 << (2 * k)) - 1)
    own_mirror = (first == last) & (G.rc_words(first, k) == first) if canonical else np.zeros(U, dtype=bool)
    mirrored_last = G.rc_words(last, k)
    order = np.argsort(mirrored_last, kind="stable")
    mirrored_sorted = mirrored_last[order]
    # side 2u leaves last(u) along its out-bits; side 2u + 1 leaves rc(first(u)), whose out-bit c is in-bit 3 - c of first(u)
    leaves = np.stack([last, G.rc_words(first, k)], axis=1).reshape(2 * U)
    out_bits = np.stack([ends >> 4, np.where(own_mirror, 0, REVERSED[ends & 15])], axis=1).reshape(2 * U)
    present = ((out_bits[:, None] >> np.arange(4)[None, :]) & 1).astype(bool)
    side, c = np.nonzero(present)  # by side, then by symbol
    reached = ((leaves[side] << U64(2)) & mask) | c.astype(U64)
    at_first, is_first = G.slots_of(reached, first)
    at_last, is_last = G.slots_of(reached, mirrored_sorted)
    to_last = 2 * (order[at_last] if U else at_last) + 1
    if canonical:
        assert (is_first | is_last).all()  # the word an edge reaches lies at an end
        targets = np.where(is_first, 2 * at_first, to_last)
    else:  # rc(u) is no part of the strand-specific graph: an odd side is read through the mirrored edges
        even = side % 2 == 0
        assert is_first[even].all() and is_last[~even].all()
        targets = np.where(even, 2 * at_first, to_last)
    offsets = np.concatenate([[0], np.cumsum(present.sum(axis=1))]).astype(U64)
    flags = (unitigs["flags"] | (own_mirror.astype(np.uint8) << 1)).astype(np.uint8)
    return offsets, targets.astype(U64), flags


def brute_links(reads, k, seqs, canonical, min_count=1, min_edge=0):
    """[the entries of side a, for a < 2 U] of the unitigs `seqs` (strings) of the reads' graph, from the windows alone"""
    m, me = thresholds(min_count, min_edge)
    at_k, at_k1 = windows(reads, k), windows(reads, k + 1)

    def cc(counter, x):
        return counter[x] if rc(x) == x else counter[x] + counter[rc(x)]

    if canonical:
        def edge(x):
            return cc(at_k1, x) >= me and cc(at_k, x[:-1]) >= m and cc(at_k, x[1:]) >= m
    else:
        def edge(x):
            return at_k1[x] >= me
    starts = {s[:k]: v for v, s in enumerate(seqs)}
    mirrored_ends = {rc(s[-k:]): v for v, s in enumerate(seqs)}
    assert len(starts) == len(seqs) == len(mirrored_ends)
    sides = []
    for s in seqs:
        own_mirror = canonical and rc(s) == s
        for leaving, forwards in ((s[-k:], True), (rc(s[:k]), False)):
            entries = []
            for c in "ACGT":
                x = leaving + c
                if not forwards and own_mirror:
                    continue  # one side
                if not (edge(x) if canonical or forwards else edge(rc(x))):
                    continue
                reached = x[1:]
                if canonical:
                    entries.append(2 * starts[reached] if reached in starts else 2 * mirrored_ends[reached] + 1)
                else:
                    entries.append(2 * starts[reached] if forwards else 2 * mirrored_ends[reached] + 1)
            sides.append(entries)
    return sides


def sides_of(link_offsets, link_targets):
    """the table as brute_links returns it"""
    return [link_targets[int(a):int(z)].tolist() for a, z in zip(link_offsets[:-1], link_offsets[1:])]


def records_once(sides, own_mirror):
    """[(side, entry)] of a table given side by side, every bidirected edge once: a record stays when it is not above its mirror"""
    def c(x):
        return x & ~1 if own_mirror[x >> 1] else x

    return [(a, e) for a, entries in enumerate(sides) for e in entries if (a, e) <= (c(e ^ 1), c(a ^ 1))]


# ---- the hand-made sets of the link tests: (reads, the k to run them at, the threshold pairs) ----

def de_bruijn(order):
    """a read that holds every word of `order` symbols over ACGT exactly once"""
    a, out = [0] * (4 * order), []

    def db(t, p):
        if t > order:
            if order % p == 0:
                out.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, 4):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    text = "".join("ACGT"[x] for x in out)
    return text + text[:order - 1]


def _branch_at_a_high_word(k):
    """two reads that share one k-mer starting with T (the top bits of its word set) and differ on both sides of it"""
    rng = np.random.default_rng(32)
    node = "T" + "".join("ACGT"[x] for x in rng.integers(0, 4, size=k - 1))
    tail = lambda n: "".join("ACGT"[x] for x in rng.integers(0, 4, size=n))
    return [tail(9) + "G" + node + "A" + tail(9), tail(9) + "C" + node + "C" + tail(9)]


PAIRS = ((1, 0), (2, 3))
HAND_MADE = {
    "every edge present": [([de_bruijn(k + 1)], (k,), ((1, 0),)) for k in (2, 3, 4, 5)],
    "a circular unitig of one node": [(["A" * (k + 1)], (k,), ((1, 0),)) for k in (2, 3, 4, 5)],
    "an isolated circle": [(["ACGTTGCAGACGTT"], (2, 3, 4, 5), PAIRS), (["ACGTTGCAGACGTT", "CCATGGATTCCCATGG"] * 3, (5,), PAIRS)],
    "a hairpin edge": [(["AATT"], (3,), ((1, 0),)), (["AACGTT"], (2, 3, 5), ((1, 0),))],
    "a palindromic node with neighbours on both ends": [(["GGACGTCC"], (4,), ((1, 0),)), (["GGACGTCC", "TAACGTAT"], (2, 3, 4, 5), ((1, 0),))],
    "an edge by count that lacks an end": [(["CATG"], (2,), ((2, 0), (1, 0)))],
    "no node at all": [(["NNNN", "", "N"], (2, 3), ((1, 0),))],
    "k = 1": [(["ACGTTGCAGACGTT", "AAC"], (1,), PAIRS), (["A"], (1,), ((1, 0),)), (["AT"], (1,), ((1, 0),))],
    "branches and tips": [(["TGGCATCAAAAAG", "TGGCATG", "AAAAAAAA", "TTCCACGTTGCAGACGTT"], (2, 3, 4, 5), PAIRS)],
    "a branch at a word with its top bits set": [(_branch_at_a_high_word(32), (32,), ((1, 0),)), (_branch_at_a_high_word(31), (31,), ((1, 0),))],
}


def hand_made_cases():
    """(name, reads, k, min_count, min_edge, canonical) of every hand-made case; canonical stops at k = 31"""
    for name, sets in HAND_MADE.items():
        for reads, ks, pairs in sets:
            for k in ks:
                for min_count, min_edge in pairs:
                    for canonical in (False, True):
                        if not (canonical and k > 31):
                            yield name, reads, k, min_count, min_edge, canonical
