"""tests/overlap_oracle.py -- the read overlaps of include/msbwt_hip.h on the BWT string alone -- against strings: on ragged read sets
every record's interval of read ids is the set of sorted reads that begin with that suffix of the query, `matched` is the longest
suffix a string search finds, on both strands; two cases worked by hand on the two-string golden; and the closed form over a run
list against the decoded stream.  No GPU."""
import os

import numpy as np
import pytest

import overlap_oracle as O
from conftest import GOLDEN_DIR
from rle_random import random_runs, runs_to_bytes

CODE = {"$": 0, "A": 1, "C": 2, "G": 3, "N": 4, "T": 5}
LETTER = "$ACGNT"
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def codes_of(text):
    return np.array([CODE[c] for c in text], dtype=np.uint8)


def overlap_read_set(seed, n=250, genome=300, longest=40):
    """n reads of 0 .. longest symbols from a random genome, some with an N, then 20 duplicates, a read that is a 5-symbol prefix of
    another, and an empty read"""
    rng = np.random.default_rng(7000 + seed)
    g = "".join(rng.choice(list("ACGT"), size=genome))
    reads = []
    for _ in range(n):
        length = int(rng.integers(0, longest + 1))
        at = int(rng.integers(0, genome - length + 1))
        r = g[at:at + length]
        if length and rng.random() < 0.05:
            p = int(rng.integers(0, length))
            r = r[:p] + "N" + r[p + 1:]
        reads.append(r)
    reads += [reads[int(i)] for i in rng.integers(0, n, size=20)]
    long_one = max(reads, key=len)
    reads += [long_one[:5], ""]
    return reads, g


def occurs(reads, s):
    return any(s in r for r in reads)


@pytest.mark.parametrize("strand", [0, 1])
@pytest.mark.parametrize("seed", [0, 1])
def test_records_are_the_reads_that_begin_with_the_suffix(orc, seed, strand):
    reads, _ = overlap_read_set(seed)
    ordered = sorted(reads)
    index = O.Decoded([CODE[c] for c in orc.naive_bwt(reads)])
    assert index.T == sum(len(r) + 1 for r in reads) and index.C[1] == len(reads)
    wide = 0
    for q in reads:
        qs = "".join(COMP[c] for c in reversed(q)) if strand else q
        assert "".join(LETTER[c] for c in O.searched(codes_of(q), strand)) == qs
        records, matched, edges, stop = O.search(index, codes_of(q), 1, 0, strand)
        by_length = {j: (first, count) for j, first, count in records}
        assert [r[0] for r in records] == sorted(by_length) and edges == sum(c for _, c in by_length.values())
        longest = max(j for j in range(len(qs) + 1) if occurs(reads, qs[len(qs) - j:]))
        assert matched == longest and stop == (O.END if matched == len(qs) else O.EMPTY), (q, strand)
        for j in range(1, len(qs) + 1):
            ids = [i for i, r in enumerate(ordered) if r.startswith(qs[len(qs) - j:])]
            if j > matched or not ids:
                assert j not in by_length, (q, j)
            else:
                assert by_length[j] == (ids[0], len(ids)) and ids == list(range(ids[0], ids[0] + len(ids))), (q, j)
                wide += len(ids) > 1
    assert wide > 100  # intervals wider than one read: the duplicates and the shared prefixes
    # min_overlap and max_overlap only cut the records and the search short
    for m, M in ((5, 0), (1, 10), (5, 10), (12, 10)):
        for q in reads[:60]:
            records, matched, _, _ = O.search(index, codes_of(q), 1, 0, strand)
            cut, cut_matched, cut_edges, cut_stop = O.search(index, codes_of(q), m, M, strand)
            E = min(len(q), M) if M else len(q)
            assert cut == [r for r in records if m <= r[0] <= E] and cut_matched == min(matched, E) and cut_edges == sum(r[2] for r in cut)
            assert cut_stop == (O.END if cut_matched == E else O.EMPTY)
    # and the edges by strings are the records expanded
    sample = reads[:40]
    want = O.edges_by_strings(sample, ordered, 3, 0, strand)
    got = set()
    for qi, q in enumerate(sample):
        for j, first, count in O.search(index, codes_of(q), 3, 0, strand)[0]:
            got |= {(qi, first + i, j) for i in range(count)}
    assert got == want and want


def test_two_string_golden_by_hand(orc):
    rle = np.load(os.path.join(GOLDEN_DIR, "two_string.npy"))
    index = O.Decoded(orc.decompress(rle))
    assert "".join(LETTER[c] for c in index.S) == "TAC$GATCG$"  # the reads ACGT and TGCA
    assert O.search(index, codes_of("GGAC"), 1) == ([(2, 0, 1)], 2, 1, O.EMPTY)
    assert O.search(index, codes_of("ACGT"), 1) == ([(1, 1, 1), (4, 0, 1)], 4, 2, O.END)
    # the other strand of ACGT is ACGT; of TGCA, TGCA: the same records
    assert O.search(index, codes_of("ACGT"), 1, 0, 1) == ([(1, 1, 1), (4, 0, 1)], 4, 2, O.END)
    assert O.search(index, codes_of("GTCC"), 1, 0, 1) == ([(2, 0, 1)], 2, 1, O.EMPTY)
    # the bounds: min_overlap above every record, max_overlap below the whole read, the empty query
    assert O.search(index, codes_of("ACGT"), 5) == ([], 4, 0, O.END)
    assert O.search(index, codes_of("ACGT"), 1, 3) == ([(1, 1, 1)], 3, 1, O.END)
    assert O.search(index, codes_of(""), 1) == ([], 0, 0, O.END)
    # a symbol that is none: the records before it stand
    assert O.search(index, [1, 2, 0, 5], 1) == ([(1, 1, 1)], 1, 1, O.BAD_SYMBOL)
    assert O.search(index, [1, 2, 6, 5], 1, 0, 1) == ([(1, 1, 1)], 2, 1, O.BAD_SYMBOL)  # searched: A 6 G T, backwards T, G, then the 6
    assert O.search(index, [7], 1) == ([], 0, 0, O.BAD_SYMBOL)
    assert O.search(O.Decoded([]), [1, 2], 1) == ([], 0, 0, O.EMPTY)
    e = O.Expected(index, [codes_of("GGAC"), codes_of(""), codes_of("ACGT")], 1)
    assert e.offsets.tolist() == [0, 1, 1, 3] and e.lengths.tolist() == [2, 1, 4] and e.first.tolist() == [0, 1, 0] and e.counts.tolist() == [1, 1, 1]
    assert e.matched.tolist() == [2, 0, 4] and e.edges.tolist() == [1, 0, 2] and e.stops.tolist() == [O.EMPTY, O.END, O.END] and e.total == 3


@pytest.mark.parametrize("kind", ["ones", "short", "long", "mixed"])
def test_run_list_closed_form_equals_the_decoded_stream(orc, kind):
    rng = np.random.default_rng(5)
    syms, lens = random_runs(rng, 60, kind)
    lens = np.minimum(lens, 300)
    full, runs = O.Decoded(orc.decompress(runs_to_bytes(syms, lens))), O.Runs(syms, lens)
    assert (runs.T, runs.C) == (full.T, full.C)
    for c in range(6):
        assert [runs.rank(c, r) for r in range(full.T + 1)] == [full.rank(c, r) for r in range(full.T + 1)]
    queries = [rng.integers(1, 6, size=int(rng.integers(0, 9))) for _ in range(200)]
    for strand in (0, 1):
        for q in queries:
            assert O.search(runs, q, 1, 0, strand) == O.search(full, q, 1, 0, strand)
