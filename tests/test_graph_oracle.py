"""The CPU proof of tests/graph_oracle.py, the numpy oracle behind tests/test_gpu_graph_scale.py.  Nothing here needs a GPU.

1. On ragged and hand-made sets, at every k of the unitig tests and under four threshold pairs, every column and every info word of the
   numpy oracle equals the string oracles test_gpu_kmer_graph.graph_of_texts, test_gpu_unitigs.unitigs_of_texts and
   test_gpu_canonical_unitigs.canonical_unitigs_of_counters, which are imported, not restated.
2. Scaling carries over to graphs: the oracle's result on a set with every read c times, shuffled, under thresholds times c is its
   result on the set itself with the counts and count sums times c, and a threshold of c m - (c - 1) selects what c m selects.  That is
   what lets an index of 4.5e9 rows be predicted from a set of 1.1e6."""
import numpy as np
import pytest

import graph_oracle as G
from test_gpu_canonical_unitigs import canonical_unitigs_of_texts, flip_every_second
from test_gpu_kmer_graph import graph_of_texts
from test_gpu_reads_build import ragged_set
from test_gpu_spectrum import word_of
from test_gpu_unitigs import unitigs_of_texts
from test_scaled_copies import COPIES, U64, as_text, copy_set, shuffled_copies

KS = (1, 2, 3, 4, 15, 16, 17, 30, 31)
THRESHOLDS = ((1, 0), (2, 0), (2, 3), (3, 5))
# the hand-made sets of tests/test_gpu_unitigs.py and tests/test_gpu_canonical_unitigs.py
HAND_MADE = {
    "a palindromic node mid-path": ["GGACGTCC"],
    "a hairpin edge": ["AACGTT"],
    "an edge by count that lacks an end": ["CATG"],
    "a cycle with a tail": ["TTCCACGTTGCAGACGTT"],
    "a cycle with a tail, twice and flipped": flip_every_second(["TTCCACGTTGCAGACGTT"] * 4),
    "the self-loop": ["AAAAAAAA"],
    "a read of k": ["ACGTA"],
    "a read of k, emitted as its mirror": ["TTACG"],
    "one strand only": ["TTTGGCATC"],
    "a branch": ["TGGCATCAAAAAG", "TGGCATG"],
    "a branch beside the loop": ["TGGCATCAAAAAG", "AAAAAAAA"],
    "one cycle": ["ACGTTGCAGACGTT"],
    "two cycles": ["ACGTTGCAGACGTT", "CCATGGATTCCCATGG"],
    "preceded by $ or N only": ["TTGACNCCGTTA", "CCGTTAG"],
    "edge threshold above node threshold": ["ACGTACCGGT", "ACGTACCGGT", "ACGTACC"],
    "once per strand": ["ACGGTCATTGACAGCT", "AGCTGTCAATGACCGT"],
    "the graph test's set": ["ACGTA", "GGCATC", "TTGACNCCGTTA", "CCGTTAG", "AAAAAAAA", "TGGCATCAAAAAG", "TGGCATG"],
}
INPUTS = ["ragged %d%s" % (seed, flipped) for seed in (0, 1, 2, 5, 11) for flipped in ("", " flipped")] + sorted(HAND_MADE)


def texts_of(name):
    if name in HAND_MADE:
        return HAND_MADE[name]
    reads = ragged_set(int(name.split()[1]))
    if name.split()[1] == "0":
        reads = reads + ["GGACGTCCTAGCATGCTAGG", "GGACGTCCTAGCATGCTAGG"]  # palindromic nodes at every even k up to 8, twice
    return flip_every_second(reads) if name.endswith("flipped") else reads


def same_unitigs(got, want, where):
    for name in G.NAMES:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape and np.array_equal(got[name], want[name]), (where, name)
    assert got["info"] == want["info"], (where, got["info"], want["info"])
    assert got["first"].tolist() == [word_of(q) for q in want["first"]] and got["last"].tolist() == [word_of(q) for q in want["last"]], where


@pytest.mark.parametrize("name", INPUTS)
def test_the_numpy_oracle_is_the_string_oracles(name):
    texts = texts_of(name)
    reads = G.codes_of_texts(texts)
    assert [as_text(r) for r in reads] == texts
    seen = {"nodes": 0, "longer": 0, "canonical longer": 0, "circular": 0, "cut": 0}
    for k in KS + ((5, 6) if name in HAND_MADE else ()):
        cen = G.census(reads, k)
        for min_count, min_edge in THRESHOLDS:
            where = (name, k, min_count, min_edge)
            words, counts, edges, n_edges = graph_of_texts(texts, k, min_count, min_edge)
            got = G.graph_of_census(cen, k, min_count, min_edge)
            assert [a.dtype for a in got[:3]] == [U64, U64, np.uint8] and got[3] == n_edges, where
            assert np.array_equal(got[0], words) and np.array_equal(got[1], counts) and np.array_equal(got[2], edges), where
            want = unitigs_of_texts(texts, k, min_count, min_edge)
            plain = G.unitigs_of_census(cen, k, min_count, min_edge)
            same_unitigs(plain, want, where)
            want = canonical_unitigs_of_texts(texts, k, min_count, min_edge)
            canonical = G.canonical_unitigs_of_census(cen, k, min_count, min_edge)
            same_unitigs(canonical, want, where)
            assert canonical["slots"] == 2 * want["info"]["classes"] - want["info"]["palindromes"]
            seen["nodes"] += len(words)
            seen["longer"] += int((plain["first"] != plain["last"]).sum())
            seen["canonical longer"] += int((canonical["first"] != canonical["last"]).sum())
            seen["circular"] += plain["info"]["circular"] + canonical["info"]["circular"]
            seen["cut"] += want["info"]["cut_links"]
    assert seen["nodes"] > 0
    if name.startswith("ragged"):
        assert seen["longer"] > 20 and seen["canonical longer"] > 20
    if name in ("one cycle", "two cycles", "the self-loop"):
        assert seen["circular"] > 0
    if name in ("a palindromic node mid-path", "a hairpin edge"):
        assert seen["cut"] > 0


def test_the_literal_cases():
    """the oracle itself, pinned to sequences written out by hand"""
    text = lambda out: [as_text(out["symbols"][int(a):int(z)]) for a, z in zip(out["offsets"][:-1], out["offsets"][1:])]
    out = G.unitigs_of_codes(G.codes_of_texts(["TGGCATCAAAAAG", "TGGCATG"]), 5)
    assert text(out) == ["GCATCAAAAAG", "GCATG", "TGGCAT"] and out["ends"].tolist() == [1 << 2, 1 << 2, 16 << 1 | 16 << 2] and out["count_sums"].tolist() == [7, 1, 4]
    out = G.unitigs_of_codes(G.codes_of_texts(["ACGTTGCAGACGTT"]), 5)
    assert text(out) == ["ACGTTGCAGACGT"] and out["flags"].tolist() == [1] and out["ends"].tolist() == [1 << 2 | 16 << 3]
    out = G.canonical_unitigs_of_codes(G.codes_of_texts(["GGACGTCC"]), 4)
    assert text(out) == ["ACGT", "CGTCC"] and out["count_sums"].tolist() == [1, 4] and out["ends"].tolist() == [1 << 2 | 16 << 1, 1 << 0]
    assert out["info"] == {"classes": 3, "edge_classes": 2, "links": 1, "unitigs": 2, "symbols": 9, "circular": 0, "longest": 2, "palindromes": 1, "cut_links": 2}
    out = G.canonical_unitigs_of_codes(G.codes_of_texts(["TTTGGCATC"]), 5)
    assert text(out) == ["GATGCCAAA"] and out["count_sums"].tolist() == [5]
    out = G.canonical_unitigs_of_codes(G.codes_of_texts(["AAAAAAAA"]), 5)
    assert text(out) == ["AAAAA"] and out["ends"].tolist() == [0x11] and out["flags"].tolist() == [1] and out["count_sums"].tolist() == [4]
    empty = G.canonical_unitigs_of_codes(G.codes_of_texts(["ACG"]), 5)
    assert [len(empty[x]) for x in G.NAMES] == [0, 1, 0, 0, 0] and not any(empty["info"].values())


def test_words_of_reverse_complements():
    rng = np.random.default_rng(3)
    for k in (1, 2, 15, 16, 31, 32):
        texts = ["".join("ACGT"[x] for x in rng.integers(0, 4, size=k)) for _ in range(20)] + ["A" * k, "T" * k]
        words = np.array([word_of(t) for t in texts], dtype=U64)
        mirror = [t.translate(str.maketrans("ACGT", "TGCA"))[::-1] for t in texts]
        assert G.rc_words(words, k).tolist() == [word_of(t) for t in mirror]
    reads = G.codes_of_texts(["ACGNT", "", "GGA"])
    assert [as_text(r) for r in G.flip_every_second(reads)] == ["ACGNT", "", "GGA"] and as_text(G.reverse_complement(reads[0])) == "ANCGT"


# ---- scaling: a set with every read c times ----

@pytest.mark.parametrize("c", COPIES)
def test_the_graph_of_the_copies_is_the_graph_of_the_set(c):
    reads = copy_set(2500, 17) + G.codes_of_texts(["ACGTTGCAGACGTT", "TTCCACGTTGCAGACGTT", "GGACGTCCTAGCATGCTAGG"] + ["ACGGTCATTGACAGCTAACGTTGACA"] * 3)
    copies = shuffled_copies(reads, c, 70 + c)
    assert len(copies) == c * len(reads)
    seen = {"nodes": 0, "dropped": 0, "longer": 0}
    for k in (1, 3, 4, 12, 31):
        small, big = G.census(reads, k), G.census(copies, k)
        assert np.array_equal(big[0], small[0]) and np.array_equal(big[1], small[1] * U64(c))
        for m, me in THRESHOLDS:
            for big_m, big_me in ((c * m, c * me), (c * m - (c - 1), c * me)):
                where = (c, k, big_m, big_me)
                words, counts, edges, n_edges = G.graph_of_census(small, k, m, me)
                got = G.graph_of_census(big, k, big_m, big_me)
                assert np.array_equal(got[0], words) and np.array_equal(got[1], counts * U64(c)) and np.array_equal(got[2], edges) and got[3] == n_edges, where
                for unitigs in (G.unitigs_of_census, G.canonical_unitigs_of_census):
                    want, out = G.scaled(unitigs(small, k, m, me), c), unitigs(big, k, big_m, big_me)
                    for name in G.NAMES + ("first", "last"):
                        assert np.array_equal(out[name], want[name]), (where, name)
                    assert out["info"] == want["info"], where
                    seen["longer"] += int((want["first"] != want["last"]).sum())
            seen["nodes"] += len(words)
            seen["dropped"] += len(small[0]) - len(words)
    assert seen["nodes"] > 1000 and seen["dropped"] > 1000 and seen["longer"] > 100
