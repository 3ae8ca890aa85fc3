"""The canonical trace oracle (tests/canonical_trace_oracle.py) against the canonical unitig oracle
(test_gpu_canonical_unitigs.canonical_unitigs_of_counters), without a GPU: a trace in unitig mode from a canonical unitig's first node
RIGHT, or from its last node LEFT, IS that unitig; how the three modes order; the mirror and strand symmetries; and the literal cases of
the definition -- the node clause at a palindromic far end, a seed the index holds on the other strand only, the hairpin edge,
MIRROR before MERGE, a palindromic seed."""
import pytest

import canonical_trace_oracle as CT
from canonical_trace_oracle import BRANCH, DEAD_END, MAX_STEPS, MERGE, MIRROR, NOT_A_NODE, RETURNED, TARGET, rc
from test_gpu_canonical_unitigs import canonical_unitigs_of_counters, flip_every_second
from test_gpu_reads_build import ragged_set

KS = (1, 2, 3, 4, 5, 6, 15, 16)
THRESHOLDS = ((1, 0), (2, 0), (1, 3), (3, 0))
MODES = ("unique", "unitig", "greedy")
R = "AAGCTCATTGGA"
# (reads, k, min_count, seed, modes, direction, extra arguments of the walk) -> (row, steps, stop, edge_sum, last, fans), or a prefix of it
LITERALS = (
    (["CATG"], 2, 2, "CA", ("unique",), "right", {}, ("", 0, DEAD_END, 0, "CA", 0)),  # cc(CAT) = 2, but AT is no node: cc(AT) = 1
    (["CATG"], 2, 2, "AT", ("unique",), "right", {}, ("", 0, NOT_A_NODE, 0, "AT", 0)),
    (["CATG"], 2, 1, "CA", ("unique",), "right", {}, ("TG", 2, DEAD_END, 4, "TG", 0)),
    ([R, rc(R)], 5, 2, "AAGCT", MODES, "right", {}, ("CATTGGA", 7, DEAD_END, 14, "TTGGA", 0)),
    ([R, rc(R)], 5, 2, "AGCTT", MODES, "left", {}, ("GTAACCT", 7, DEAD_END, 14, "TCCAA", 0)),
    ([R], 5, 2, "AAGCT", ("unique",), "right", {}, ("", 0, NOT_A_NODE, 0, "AAGCT", 0)),
    ([R], 5, 1, "TCCAA", ("unique",), "right", {}, ("TGAGCTT", 7, DEAD_END, 7, "AGCTT", 0)),  # a seed the index holds only as its reverse complement
    (["AACGTC"], 3, 1, "ACG", ("unitig",), "right", {}, ("", 0, MIRROR, 0, "ACG", 0b1000)),  # the hairpin edge ACGT
    (["AACGTC"], 3, 1, "ACG", ("unique",), "right", {}, ("T", 1, BRANCH, 1, "CGT", 0b1010)),
    (["AACGTC"], 3, 1, "AAC", ("unitig",), "right", {}, ("", 0, MERGE, 0, "AAC", 0b0100)),
    (["AACGTC"], 3, 1, "AAC", ("greedy",), "right", {}, ("GTC", 3, DEAD_END, 3, "GTC", 0)),
    (["TGGACGTAA"], 4, 1, "TGGA", ("unitig",), "right", {}, ("CG", 2, MIRROR, 2, "GACG", 0b1000)),  # nxt = ACGT: a palindrome with two predecessors
    (["TGGACGTAA"], 4, 1, "TGGA", ("unique",), "right", {}, ("CGT", 3, BRANCH, 3, "ACGT", 0b0011)),
    (["TGGACGTAA"], 4, 1, "TGGA", ("greedy",), "right", dict(target="ACGT"), ("CGT", 3, TARGET)),
    (["TGGACGTAA"], 4, 1, "TGGA", ("greedy",), "right", dict(max_steps=3), ("CGT", 3, MAX_STEPS)),
    (["GGACGTCA"], 4, 1, "ACGT", ("unitig",), "right", {}, ("", 0, MIRROR, 0, "ACGT", 0b0010)),  # a palindromic seed
    (["GGACGTCA"], 4, 1, "GGAC", ("greedy",), "right", {}, ("GTCA", 4, DEAD_END, 6, "GTCA", 0)),
)


def test_the_literal_cases():
    for reads, k, min_count, seed, modes, direction, more, want in LITERALS:
        g = CT.Graph(reads, k, min_count)
        for mode in modes:
            got = CT.trace(g, seed, mode, direction, **{**dict(max_steps=50), **more})
            assert got[:len(want)] == want, (reads, k, min_count, seed, mode, direction, got)


def check_unitigs_are_traces(g, k, min_count, min_edge):
    want = canonical_unitigs_of_counters(g.at_k, g.at_k1, k, min_count, min_edge)
    assert {min(q, rc(q)) for q in g.nodes} == {min(s[i:i + k], rc(s[i:i + k])) for s in want["seqs"] for i in range(len(s) - k + 1)}
    limit = want["info"]["longest"] + 1
    steps_sum = mirrors = 0
    for seq, first, last, circular, count_sum, ends in zip(want["seqs"], want["first"], want["last"], want["flags"], want["count_sums"], want["ends"]):
        v = len(seq) - k + 1
        for seed, direction in ((first, "right"), (last, "left")):
            symbols, steps, stop, edge_sum, end, fan = CT.trace(g, seed, "unitig", direction, limit)
            assert CT.sequence(seed, symbols, direction) == seq, (k, seed, direction)
            assert steps == v - 1 and end == (last if direction == "right" else first)
            assert stop == RETURNED if circular else stop in (DEAD_END, BRANCH, MERGE, MIRROR), (seq, direction, stop)
            assert edge_sum == sum(g.cc(seq[i:i + k + 1]) for i in range(v - 1))
            assert fan == (int(ends) >> 4 if direction == "right" else int(ends) & 15)
            mirrors += stop == MIRROR
            if direction == "right":
                steps_sum += steps
    assert steps_sum + want["info"]["unitigs"] == want["info"]["classes"]
    return len(want["seqs"]), mirrors


def check_modes_order_and_mirror(g, k, max_steps):
    for direction, other in (("right", "left"), ("left", "right")):
        for seed in g.nodes:
            unitig, unique, greedy = (CT.trace(g, seed, mode, direction, max_steps) for mode in ("unitig", "unique", "greedy"))
            assert unitig[1] <= unique[1] <= greedy[1] <= max_steps
            assert unique[0].startswith(unitig[0]) and greedy[0].startswith(unique[0])  # each goes the way of the one before it, and on
            if unitig[1] < unique[1]:
                assert unitig[2] in (MERGE, MIRROR)
            if unique[1] < greedy[1]:
                assert unique[2] == BRANCH
            # the trace of rc(s) in the other direction is the mirror of the trace of s
            for mode, result in (("unitig", unitig), ("unique", unique)):
                assert CT.trace(g, rc(seed), mode, other, max_steps) == CT.mirrored(result), (k, seed, mode, direction)
        for seed in g.below + ["A" * k, ("ACGT" * 8)[:k]]:
            if seed not in g.nodes:
                assert CT.trace(g, seed, "greedy", direction, max_steps) == ("", 0, NOT_A_NODE, 0, seed, 0)


@pytest.mark.parametrize("seed", [0, 1, 2, 5, 11])
def test_ragged_sets(seed):
    reads = ragged_set(seed)
    flipped = flip_every_second(reads)
    unitigs = mirrors = 0
    for k in KS:
        for min_count, min_edge in THRESHOLDS:
            g, f = CT.Graph(reads, k, min_count, min_edge), CT.Graph(flipped, k, min_count, min_edge)
            u, mi = check_unitigs_are_traces(g, k, min_count, min_edge)
            unitigs, mirrors = unitigs + u, mirrors + mi
            check_unitigs_are_traces(f, k, min_count, min_edge)
            for max_steps in (0, 1, 7, 200):
                check_modes_order_and_mirror(g, k, max_steps)
            # D does not see which strand a read came from
            assert g.nodes == f.nodes and g.below == f.below
            for mode in MODES:
                for q in g.nodes:
                    assert CT.trace(g, q, mode, "right", 200) == CT.trace(f, q, mode, "right", 200)
    assert unitigs > 20 and mirrors > 0


def test_planted_palindromes_and_hairpins():
    reads = ["TTGACGTCAAGGACGTCC", "GGAATTCCA", "GGAATTCCA", "CCAACGTTGG", "TGCATGCATG", "AATT", "ACGT" * 4, "GATCGATC" + "A" * 9]
    mirrors = 0
    for k in KS[:6]:
        for min_count, min_edge in THRESHOLDS:
            g = CT.Graph(reads, k, min_count, min_edge)
            mirrors += check_unitigs_are_traces(g, k, min_count, min_edge)[1]
            check_modes_order_and_mirror(g, k, 60)
    assert mirrors > 10
