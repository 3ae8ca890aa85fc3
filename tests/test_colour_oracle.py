"""The CPU check of tests/colour_oracle.py, the oracle behind tests/test_gpu_unitig_sources.py: on the hand-made sets of
tests/test_graph_oracle.py split into 2 and 3 sources -- dealt, all in the last source, and one split in which a source holds only
reverse-complemented reads -- rows sum to count_sums, one source gives count_sums, and permuting the sources permutes the columns.
Nothing here needs a GPU."""
import numpy as np
import pytest

import colour_oracle as CO
from test_gpu_canonical_unitigs import rc
from test_graph_oracle import HAND_MADE

KS = (1, 2, 3, 4, 5, 6)
THRESHOLDS = ((1, 0), (2, 0), (2, 3))


def splits(reads):
    """(name, sets): the reads dealt to 2 and 3 sources, all in the last of 3, and each read once as it is and once flipped in a source of its own"""
    yield "dealt to 2", CO.deal(reads, 2)
    yield "dealt to 3", CO.deal(reads, 3)
    yield "all in the last of 3", [[], [""], list(reads)]
    yield "a source of reverse complements only", [list(reads), [rc(r) for r in reads]]
    yield "three, the middle one flipped", [list(reads), [rc(r) for r in reads], list(reads)]


@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_rows_sum_and_columns_permute(name):
    reads = HAND_MADE[name]
    rows = 0
    for split, sets in splits(reads):
        for k in KS:
            for min_count, min_edge in THRESHOLDS:
                for canonical in (False, True):
                    where = (name, split, k, min_count, min_edge, canonical)
                    unitigs, m = CO.unitigs_by_source(sets, k, min_count, min_edge, canonical)
                    assert m.shape == (len(unitigs["seqs"]), len(sets)) and m.dtype == np.uint64, where
                    assert np.array_equal(m.sum(axis=1), unitigs["count_sums"]), where
                    # one source: the column is count_sums
                    one = CO.source_sums([[r for s in sets for r in s]], k, unitigs["seqs"], canonical)
                    assert np.array_equal(one[:, 0], unitigs["count_sums"]), where
                    # the sources in another order: the same unitigs, the columns in that order
                    order = list(range(len(sets)))[::-1] if len(sets) == 2 else [2, 0, 1]
                    again, pm = CO.unitigs_by_source([sets[i] for i in order], k, min_count, min_edge, canonical)
                    assert again["seqs"] == unitigs["seqs"] and np.array_equal(pm, m[:, order]), where
                    rows += len(m)
                    if split == "a source of reverse complements only" and canonical:  # a class is held alike by a strand and by its mirror
                        assert np.array_equal(m[:, 0], m[:, 1]), where
    assert rows > 0


def test_the_literal_cases():
    # the palindromic node mid-path: GGAC GACG | ACGT | CGTC GTCC; ACGT is its own mirror and counts once, GGAC = rc(GTCC)
    unitigs, m = CO.unitigs_by_source([["GGACGTCC"], ["GGACGTCC", "ACGT"]], 4, canonical=True)
    assert unitigs["seqs"] == ["ACGT", "CGTCC"] and m.tolist() == [[1, 2], [4, 4]]
    unitigs, m = CO.unitigs_by_source([["GGACGTCC"], ["GGACGTCC", "ACGT"]], 4)
    assert sorted(unitigs["seqs"]) == ["GGACGTCC"] and m.tolist() == [[5, 6]]
    # a source on the reverse strand only lands in the emitted unitig's row
    unitigs, m = CO.unitigs_by_source([["TTACG"], [rc("TTACG")], []], 5, canonical=True)
    assert unitigs["seqs"] == ["CGTAA"] and m.tolist() == [[1, 1, 0]]
    unitigs, m = CO.unitigs_by_source([["TTACG"], [rc("TTACG")], []], 5)
    assert unitigs["seqs"] == ["CGTAA", "TTACG"] and m.tolist() == [[0, 1, 0], [1, 0, 0]]


@pytest.mark.parametrize("seed", [0, 1, 2, 5, 11])
def test_the_numpy_matrix_is_the_string_matrix(seed):
    import graph_oracle as G
    from test_gpu_reads_build import ragged_set
    reads = ragged_set(seed) + ["GGACGTCCTAGCATGCTAGG"] * 2
    rows = 0
    for S in (1, 3, 4):
        sets = CO.deal(reads, S)
        codes = [G.codes_of_texts(s) for s in sets]
        for k in (1, 2, 4, 8, 17, 31):
            for canonical in (False, True):
                unitigs, m = CO.unitigs_by_source(sets, k, canonical=canonical)
                assert np.array_equal(CO.source_sums_of_codes(codes, k, unitigs["symbols"], unitigs["offsets"], canonical), m), (seed, S, k, canonical)
                rows += len(m)
    assert rows > 100
