"""The trace oracle (tests/trace_oracle.py) against the unitig oracle (test_gpu_unitigs.unitigs_of_texts), without a GPU: a trace in
unitig mode from a unitig's first node RIGHT, or from its last node LEFT, IS that unitig; and how the three modes order.  Ragged sets
of reads with N, duplicates and prefixes at every k of the GPU tests, and the hand-made sets of tests/test_gpu_trace.py."""
import pytest

import trace_oracle as T
from test_gpu_reads_build import ragged_set
from test_gpu_unitigs import unitigs_of_texts

KS = (1, 2, 3, 4, 15, 16, 17, 30, 31)
THRESHOLDS = ((1, 0), (2, 0), (1, 3))
# k = 5: a read of exactly k symbols; a branch; the self-loop of A^k beside a chain through it; the self-loop alone; an isolated cycle
# of 9 nodes; a cycle with a tail into it; two cycles; a k-mer preceded only by '$' or 'N'; reads for the thresholds
HAND = (["ACGTA"], ["TGGCATCAAAAAG", "TGGCATG"], ["TGGCATCAAAAAG", "AAAAAAAA"], ["AAAAAAAA"], ["ACGTTGCAGACGTT"], ["TTCCACGTTGCAGACGTT"],
        ["ACGTTGCAGACGTT", "CCATGGATTCCCATGG"], ["TTGACNCCGTTA", "CCGTTAG"], ["ACGTACCGGT", "ACGTACCGGT", "ACGTACC"])


def check_unitigs_are_traces(reads, k, min_count, min_edge):
    want = unitigs_of_texts(reads, k, min_count, min_edge)
    g = T.Graph(reads, k, min_count, min_edge)
    assert set(g.nodes) == {s[i:i + k] for s in want["seqs"] for i in range(len(s) - k + 1)}
    limit = want["info"]["longest"] + 1
    steps_sum = 0
    for seq, first, last, circular, count_sum in zip(want["seqs"], want["first"], want["last"], want["flags"], want["count_sums"]):
        v = len(seq) - k + 1
        for seed, direction in ((first, "right"), (last, "left")):
            symbols, steps, stop, edge_sum, end, fan = T.trace(g, seed, "unitig", direction, limit)
            assert T.sequence(seed, symbols, direction) == seq, (reads, k, seed, direction)
            assert steps == v - 1 and end == (last if direction == "right" else first)
            assert stop == T.RETURNED if circular else stop in (T.DEAD_END, T.BRANCH, T.MERGE), (seq, direction, stop)
            assert edge_sum == sum(g.edges[seq[i:i + k + 1]] for i in range(v - 1))
            if direction == "right":
                steps_sum += steps
    assert steps_sum + want["info"]["unitigs"] == want["info"]["nodes"]
    return len(want["seqs"])


def check_modes_order(reads, k, min_count, min_edge, max_steps):
    g = T.Graph(reads, k, min_count, min_edge)
    for direction in ("right", "left"):
        for seed in g.nodes:
            unitig, unique, greedy = (T.trace(g, seed, mode, direction, max_steps) for mode in ("unitig", "unique", "greedy"))
            assert unitig[1] <= unique[1] <= greedy[1] <= max_steps
            assert unique[0].startswith(unitig[0]) and greedy[0].startswith(unique[0])  # each goes the way of the one before it, and on
            if unitig[1] < unique[1]:
                assert unitig[2] == T.MERGE
            if unique[1] < greedy[1]:
                assert unique[2] == T.BRANCH
        for seed in g.below + ["A" * k, ("ACGT" * 8)[:k]]:
            if len(seed) == k and seed not in g.nodes:
                assert T.trace(g, seed, "greedy", direction, max_steps) == ("", 0, T.NOT_A_NODE, 0, seed, 0)


@pytest.mark.parametrize("seed", [0, 1, 2, 5, 11])
def test_ragged_sets(seed):
    reads = ragged_set(seed)
    unitigs = 0
    for k in KS:
        for min_count, min_edge in THRESHOLDS:
            unitigs += check_unitigs_are_traces(reads, k, min_count, min_edge)
            for max_steps in (0, 1, 7, 200):
                check_modes_order(reads, k, min_count, min_edge, max_steps)
    assert unitigs > 20


def test_hand_made_sets():
    k = 5
    for reads in HAND:
        for min_count, min_edge in THRESHOLDS + ((2, 3), (3, 0)):
            check_unitigs_are_traces(reads, k, min_count, min_edge)
            check_modes_order(reads, k, min_count, min_edge, 50)
    # the self-loop alone: RETURNED after 0 steps in every mode; with a second in-edge, a MERGE in unitig mode only
    g = T.Graph(["AAAAAAAA"], k)
    for mode in ("unique", "unitig", "greedy"):
        assert T.trace(g, "AAAAA", mode, "right", 9) == ("", 0, T.RETURNED, 0, "AAAAA", 1)
    g = T.Graph(["AAAAAAAA", "CAAAAA"], k)
    assert T.trace(g, "AAAAA", "unitig", "right", 9)[2] == T.MERGE and T.trace(g, "AAAAA", "unique", "right", 9)[2] == T.RETURNED
    # an isolated cycle of v = 9 nodes: RETURNED after v - 1 steps from any of its nodes, in both directions
    g = T.Graph(["ACGTTGCAGACGTT"], k)
    assert len(g.nodes) == 9
    for seed in g.nodes:
        for direction in ("right", "left"):
            symbols, steps, stop, _, end, fan = T.trace(g, seed, "unitig", direction, 50)
            assert (steps, stop) == (8, T.RETURNED) and bin(fan).count("1") == 1
            assert T.sequence(seed, symbols, direction).count(seed) == 1
    # a tail into that cycle: the walk from the tail turns until max_steps in unique mode and stops at the entry in unitig mode
    g = T.Graph(["TTCCACGTTGCAGACGTT"], k)
    assert T.trace(g, "TTCCA", "unique", "right", 40)[1:3] == (40, T.MAX_STEPS)
    assert T.trace(g, "TTCCA", "unitig", "right", 40)[1:5] == (3, T.MERGE, 3, "CACGT")  # TTCCA TCCAC CCACG CACGT | ACGTT
    # greedy takes the heavier side, and the smaller symbol on a tie
    g = T.Graph(["TGGCATCA", "TGGCATCA", "TGGCATGA"], k)
    assert T.trace(g, "TGGCA", "unique", "right", 9)[:3] == ("T", 1, T.BRANCH) and T.trace(g, "TGGCA", "greedy", "right", 9)[0] == "TCA"
    g = T.Graph(["TGGCATGA", "TGGCATCA"], k)
    assert T.trace(g, "TGGCA", "greedy", "right", 9)[0] == "TCA" and T.trace(g, "TGGCA", "unique", "right", 9)[5] == 0b0110
    # a target on the path stops the walk there; off the path, or equal to the seed, it does not
    g = T.Graph(["ACGTACCGGT"], k)
    assert T.trace(g, "ACGTA", "unique", "right", 9, target="GTACC")[:5] == ("CC", 2, T.TARGET, 2, "GTACC")
    assert T.trace(g, "ACGTA", "unique", "right", 9, target="GGGGG")[1:3] == (5, T.DEAD_END)
    assert T.trace(g, "ACGTA", "unique", "right", 9, target="ACGTA")[1:3] == (5, T.DEAD_END)
    assert T.trace(g, "CCGGT", "unique", "left", 9)[0] == "ATGCA" and T.sequence("CCGGT", "ATGCA", "left") == "ACGTACCGGT"


def test_words_and_strings():
    assert T.word_of("ACGT") == 0b00011011 and T.kmer_of(0b00011011, 4) == "ACGT" and T.kmer_of(T.word_of("T" * 31), 31) == "T" * 31
