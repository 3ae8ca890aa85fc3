"""The CPU proof of tests/link_oracle.py, the oracle behind tests/test_gpu_unitig_links.py, and of the host helpers of the link table
(rle_bwt.unitig_link_records, rle_bwt.write_gfa).  Nothing here needs a GPU.

1. On the hand-made sets of link_oracle.HAND_MADE and on the ragged sets of the unitig tests, at their k and under (1, 0) and (2, 3),
   for both graphs, the numpy table equals the brute force over strings, side by side.
2. Every identity include/msbwt_hip.h states for the table holds: the sizes of the sides against the ends bytes, the parity of the
   plain call's entries, L against the info words, the sides of a circular unitig, the one side of a unitig that is its own reverse
   complement, the mirror of every record, and the number of records kept once.
3. unitig_link_records is the rule written out as a loop; write_gfa, parsed back, holds the brute force's edges, each once."""
import importlib
import io

import numpy as np
import pytest

import graph_oracle as G
import link_oracle as L
from test_gpu_canonical_unitigs import canonical_unitigs_of_texts
from test_gpu_reads_build import ragged_set
from test_gpu_unitigs import KS, unitigs_of_texts

rle_bwt = importlib.import_module("rust-msbwt_amd").rle_bwt
U64 = np.uint64
POP = G.POP


def unitigs_of(reads, k, min_count, min_edge, canonical):
    return (canonical_unitigs_of_texts if canonical else unitigs_of_texts)(reads, k, min_count, min_edge)


def check_identities(want, table, k, canonical, where):
    offsets, targets, flags = table
    U, sides = len(want["ends"]), L.sides_of(offsets, targets)
    ends, info = want["ends"].astype(np.int64), want["info"]
    own_mirror = (flags & 2) != 0
    assert offsets.dtype == U64 and targets.dtype == U64 and flags.dtype == np.uint8
    assert len(offsets) == 2 * U + 1 and offsets[0] == 0 and offsets[-1] == len(targets) and len(sides) == 2 * U
    assert np.array_equal(flags & 1, want["flags"]) and (canonical or not own_mirror.any()), where
    sizes = np.diff(offsets.astype(np.int64))
    assert np.array_equal(sizes[0::2], POP[ends >> 4]) and np.array_equal(sizes[1::2], np.where(own_mirror, 0, POP[ends & 15])), where
    seqs = want["seqs"]
    assert [canonical and L.rc(s) == s for s in seqs] == own_mirror.tolist(), where
    assert all(len(s) == k for s, own in zip(seqs, own_mirror) if own)  # a single palindromic node
    for u in range(U):
        if want["flags"][u]:  # circular: the closing link from both ends
            assert sides[2 * u] == [2 * u] and sides[2 * u + 1] == [2 * u + 1], where
    if not canonical:
        assert all(e % 2 == 0 for s in sides[0::2] for e in s) and all(e % 2 == 1 for s in sides[1::2] for e in s), where
        assert len(targets) == 2 * (info["edges"] - info["links"] + info["circular"]), where
        for u in range(U):  # 2v + 1 for the v whose last node precedes first(u), by descending predecessor symbol
            before = [c + seqs[u][:k - 1] for c in "TGCA" if ends[u] & (1 << "ACGT".index(c))]
            assert [seqs[e >> 1][-k:] for e in sides[2 * u + 1]] == before, where
    assert all(e % 2 == 0 for s in sides for e in s if own_mirror[e >> 1]), where  # entries that reach a unitig of one side carry o = 0
    # the mirror of every record is a record
    def c(x):
        return x & ~1 if own_mirror[x >> 1] else x

    records = [(a, e) for a, s in enumerate(sides) for e in s]
    assert len(set(records)) == len(records), where
    assert {(c(e ^ 1), c(a ^ 1)) for a, e in records} == set(records), where
    once = L.records_once(sides, own_mirror)
    assert len(once) == (info["edge_classes"] if canonical else info["edges"]) - info["links"] + info["circular"], where
    if not canonical:  # as many as the even sides hold (not those: (1, 3) stays, its mirror (2, 0) goes)
        assert len(once) == sum(len(s) for s in sides[0::2]), where
    got_sides, got_targets = rle_bwt.unitig_link_records(offsets, targets, flags)
    assert got_sides.dtype == U64 and got_targets.dtype == U64 and list(zip(got_sides.tolist(), got_targets.tolist())) == once, where
    return once


def check_gfa(want, table, k, once, where):
    offsets, targets, flags = table
    own_mirror = (flags & 2) != 0
    out = io.StringIO()
    written = rle_bwt.write_gfa(out, k, want["symbols"], want["offsets"], want["count_sums"], flags, offsets, targets)
    lines = out.getvalue().splitlines()
    assert lines[0] == "H\tVN:Z:1.0" and written == (len(want["seqs"]), len(once)), where
    segments = [x.split("\t") for x in lines if x.startswith("S\t")]
    assert [(s[1], s[2], s[3]) for s in segments] == [(str(u), q, "KC:i:%d" % n) for u, (q, n) in enumerate(zip(want["seqs"], want["count_sums"].tolist()))], where
    links = [x.split("\t") for x in lines if x.startswith("L\t")]
    assert len(lines) == 1 + len(segments) + len(links) and all(x[5] == "%dM" % (k - 1) for x in links), where

    def edge(u, minus_u, v, minus_v):  # an edge and the same edge from its other end, a unitig of one side always forwards
        minus_u, minus_v = minus_u and not own_mirror[u], minus_v and not own_mirror[v]
        back = (v, not minus_v and not own_mirror[v], u, not minus_u and not own_mirror[u])
        return min((u, minus_u, v, minus_v), back)

    parsed = [edge(int(x[1]), x[2] == "-", int(x[3]), x[4] == "-") for x in links]
    assert all(x[2] in "+-" and x[4] in "+-" for x in links) and len(set(parsed)) == len(parsed), where  # each edge once
    return set(parsed), edge


def check_case(reads, k, min_count, min_edge, canonical, where):
    want = unitigs_of(reads, k, min_count, min_edge, canonical)
    table = L.link_table(want, k, canonical)
    brute = L.brute_links(reads, k, want["seqs"], canonical, min_count, min_edge)
    assert L.sides_of(table[0], table[1]) == brute, where
    once = check_identities(want, table, k, canonical, where)
    parsed, edge = check_gfa(want, table, k, once, where)
    assert parsed == {edge(a >> 1, bool(a & 1), e >> 1, bool(e & 1)) for a, entries in enumerate(brute) for e in entries}, where
    if k <= 31:  # the numpy unitig oracle gives the same table through words
        cen = G.census(G.codes_of_texts(reads), k)
        again = (G.canonical_unitigs_of_census if canonical else G.unitigs_of_census)(cen, k, min_count, min_edge)
        for x, y in zip(L.link_table(again, k, canonical), table):
            assert np.array_equal(x, y), where
    return want, table


def test_the_hand_made_sets():
    seen = {"own mirror": 0, "circular": 0, "four": 0, "odd entries": 0, "empty": 0, "hairpins": 0}
    for name, reads, k, min_count, min_edge, canonical in L.hand_made_cases():
        want, (offsets, targets, flags) = check_case(reads, k, min_count, min_edge, canonical, (name, k, min_count, min_edge, canonical))
        sides = L.sides_of(offsets, targets)
        seen["own mirror"] += int(((flags & 2) != 0).sum())
        seen["circular"] += int((flags & 1).sum())
        seen["empty"] += len(want["seqs"]) == 0
        seen["odd entries"] += sum(1 for a, s in enumerate(sides) for e in s if canonical and a % 2 == 0 and e % 2 == 1)
        seen["hairpins"] += sum(1 for a, s in enumerate(sides) for e in s if canonical and e == a ^ 1 and not (flags[a >> 1] & 2))
        if name == "every edge present":
            assert canonical or len(want["seqs"]) == 4 ** k  # every node branches both ways: a unitig of its own
            assert all(len(s) == 4 for a, s in enumerate(sides) if not (flags[a >> 1] & 2 and a & 1))
            seen["four"] += 1
        if name == "a circular unitig of one node":
            assert want["seqs"] == ["A" * k] and sides == [[0], [1]] and flags.tolist() == [1]
        if name == "no node at all":
            assert offsets.tolist() == [0] and len(targets) == 0
    assert all(seen.values()), seen
    # the cases of the header, written out
    want, (offsets, targets, flags) = check_case(["CATG"], 2, 2, 0, True, "CATG")
    assert want["seqs"] == ["CA"] and L.sides_of(offsets, targets) == [[], []]  # AT is no node: ATG is no edge, whatever its count
    want, (offsets, targets, flags) = check_case(["AATT"], 3, 1, 0, True, "AATT")
    assert want["seqs"] == ["AAT"] and L.sides_of(offsets, targets) == [[1], []] and flags.tolist() == [0]  # AAT -> ATT = rc(AAT): its own mirror
    want, (offsets, targets, flags) = check_case(["GGACGTCC"], 4, 1, 0, True, "GGACGTCC")
    assert want["seqs"] == ["ACGT", "CGTCC"] and flags.tolist() == [2, 0]
    assert L.sides_of(offsets, targets) == [[2], [], [], [0]]  # ACGT -> CGTC; GACG -> ACGT read from rc(CGTCC) = GGACG, with o = 0


@pytest.mark.parametrize("seed", [0, 1, 2, 5, 11])
def test_ragged_sets_at_every_k(seed):
    reads = ragged_set(seed)
    entries = 0
    for k in KS:
        for min_count, min_edge in L.PAIRS:
            for canonical in (False, True) if k <= 31 else (False,):
                _, (offsets, targets, _) = check_case(reads, k, min_count, min_edge, canonical, (seed, k, min_count, min_edge, canonical))
                entries += len(targets)
    assert entries > 100


def test_link_records_refuse_a_table_that_is_none():
    with pytest.raises(ValueError):
        rle_bwt.unitig_link_records(np.zeros(2, dtype=U64), np.zeros(0, dtype=U64), np.zeros(1, dtype=np.uint8))
    with pytest.raises(ValueError):
        rle_bwt.unitig_link_records(np.array([0, 1, 2], dtype=U64), np.zeros(1, dtype=U64), np.zeros(1, dtype=np.uint8))
    sides, targets = rle_bwt.unitig_link_records(np.zeros(1, dtype=U64), np.zeros(0, dtype=U64), np.zeros(0, dtype=np.uint8))
    assert len(sides) == 0 and len(targets) == 0
