"""tests/walk_oracle.py -- the left walks of include/msbwt_hip.h on the BWT string alone -- against strings: reads recovered from the
'$' rows, locate against a suffix array of the doubled rotations computed naively, two goldens written out by hand, and the
closed form over a run list against the decoded stream.  No GPU."""
import os

import numpy as np
import pytest

import walk_oracle as W
from conftest import GOLDEN_DIR
from rle_random import random_runs, runs_to_bytes

CODE = {"$": 0, "A": 1, "C": 2, "G": 3, "N": 4, "T": 5}
LETTER = "$ACGNT"


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def decoded_of(text):
    return W.Decoded([CODE[c] for c in text])


def text_of(codes):
    return "".join(LETTER[int(c)] for c in codes)


def ragged(seed):
    """a few reads of 0-30 symbols over ACGTN with duplicates, prefixes and empty reads"""
    rng = np.random.default_rng(seed)
    reads = ["".join(rng.choice(list("ACGTN"), size=int(rng.integers(0, 31)), p=[0.3, 0.2, 0.2, 0.25, 0.05])) for _ in range(int(rng.integers(1, 15)))]
    for _ in range(3):
        r = reads[int(rng.integers(0, len(reads)))]
        reads += [r, r[:int(rng.integers(0, len(r) + 1))]]
    return reads + [""]


def naive_positions(reads):
    """(read, offset) of every row: the rotations of every read + '$', doubled as naive_bwt doubles them, sorted; ties -- equal reads --
    by the read's place among the sorted reads"""
    ordered = sorted(reads)
    rows = []
    for i, r in enumerate(ordered):
        ds = r + "$"
        rows += [(ds[p:] + ds + ds[:p], i, p) for p in range(len(ds))]
    rows.sort()
    return ordered, [(i, p) for _, i, p in rows]


@pytest.mark.parametrize("seed", range(8))
def test_dollar_rows_give_the_sorted_reads_reversed(orc, seed):
    reads = ragged(seed)
    index = decoded_of(orc.naive_bwt(reads))
    ordered = sorted(reads)
    assert index.reads == len(reads) and index.T == sum(len(r) + 1 for r in reads)
    for i, r in enumerate(ordered):
        out, stop, last, read = W.walk(index, i, 1000)
        assert (text_of(out), stop, read) == (r[::-1], W.DOLLAR, i) and index.S[last] == 0
        # at max_steps == len the '$' still wins; one step less is MAX_STEPS with the last len - 1 symbols
        assert W.walk(index, i, len(r))[:2] == (out, W.DOLLAR)
        if r:
            assert W.walk(index, i, len(r) - 1)[:2] == (out[:-1], W.MAX_STEPS) and W.walk(index, i, len(r) - 1)[3] is None
    symbols, offsets, truncated = W.extract(index, range(len(reads)), 1000)
    assert truncated == 0 and [text_of(symbols[int(a):int(b)]) for a, b in zip(offsets[:-1], offsets[1:])] == ordered
    symbols, offsets, truncated = W.extract(index, range(len(reads)), 7)
    assert truncated == sum(len(r) > 7 for r in reads)
    assert [text_of(symbols[int(a):int(b)]) for a, b in zip(offsets[:-1], offsets[1:])] == [r[-7:] if len(r) > 7 else r for r in ordered]


@pytest.mark.parametrize("seed", range(8))
def test_locate_of_every_row_is_the_suffix_array(orc, seed):
    reads = ragged(100 + seed)
    index = decoded_of(orc.naive_bwt(reads))
    ordered, positions = naive_positions(reads)
    got_reads, got_offsets, stops = W.locate(index, range(index.T), 1000)
    assert (stops == W.DOLLAR).all()
    assert list(zip(got_reads.tolist(), got_offsets.tolist())) == positions
    # and the symbols of a walk are the read's prefix before the offset, last symbol first
    for row, (i, p) in enumerate(positions):
        assert text_of(W.walk(index, row, 1000)[0]) == ordered[i][:p][::-1]


def test_golden_three_reads_by_hand(orc):
    reads, bwt = ["CCGT", "N", "ACG"], "GTN$$ACCC$G"
    assert orc.naive_bwt(reads) == bwt
    index = decoded_of(bwt)
    assert index.C.tolist() == [0, 3, 4, 7, 9, 10] and index.reads == 3
    assert index.lf.tolist() == [7, 10, 9, 0, 1, 3, 4, 5, 6, 2, 8]
    symbols, steps, stops, last, reads_at = W.expected_arrays(index, range(12), 4, fill=0xEE)
    E = 0xEE
    assert symbols.tolist() == [[3, 2, 1, E], [5, 3, 2, 2], [4, E, E, E], [E, E, E, E], [E, E, E, E], [1, E, E, E], [2, E, E, E], [2, 1, E, E], [2, 2, E, E],
                                [E, E, E, E], [3, 2, 2, E], [E, E, E, E]]
    assert steps.tolist() == [3, 4, 1, 0, 0, 1, 1, 2, 2, 0, 3, 0]
    assert stops.tolist() == [1] * 11 + [W.BAD_ROW]
    assert last.tolist() == [3, 4, 9, 3, 4, 3, 4, 3, 4, 9, 4, 11]
    assert reads_at.tolist() == [0, 1, 2, 0, 1, 0, 1, 0, 1, 2, 1, int(W.NO_READ)]
    # three steps do not finish CCGT from its '$' row
    assert W.walk(index, 1, 3) == ([5, 3, 2], W.MAX_STEPS, 6, None)
    symbols, offsets, truncated = W.extract(index, [2, 0, 1, 0], 3)
    assert text_of(symbols) == "N" + "ACG" + "CGT" + "ACG" and offsets.tolist() == [0, 1, 4, 7, 10] and truncated == 1


def test_golden_two_string_file_by_hand(orc):
    rle = np.load(os.path.join(GOLDEN_DIR, "two_string.npy"))
    index = W.Decoded(orc.decompress(rle))
    assert text_of(index.S) == "TAC$GATCG$"
    symbols, steps, stops, last, reads_at = W.expected_arrays(index, [0, 1, 3, 9, 8, 10], 4)
    assert symbols.tolist() == [[5, 3, 2, 1], [1, 2, 3, 5], [0, 0, 0, 0], [0, 0, 0, 0], [3, 2, 1, 0], [0, 0, 0, 0]]
    assert steps.tolist() == [4, 4, 0, 0, 3, 0] and stops.tolist() == [1, 1, 1, 1, 1, 3]
    assert last.tolist() == [3, 9, 3, 9, 3, 10] and reads_at.tolist() == [0, 1, 0, 1, 0, int(W.NO_READ)]
    symbols, offsets, truncated = W.extract(index, [0, 1], 4)
    assert (text_of(symbols), offsets.tolist(), truncated) == ("ACGTTGCA", [0, 4, 8], 0)


@pytest.mark.parametrize("kind", ["ones", "short", "long", "mixed"])
def test_run_list_closed_form_equals_the_decoded_stream(orc, kind):
    rng = np.random.default_rng(5)
    syms, lens = random_runs(rng, 60, kind)
    lens = np.minimum(lens, 300)
    full, runs = W.Decoded(orc.decompress(runs_to_bytes(syms, lens))), W.Runs(syms, lens)
    assert (runs.T, runs.reads, runs.C.tolist()) == (full.T, full.reads, full.C.tolist())
    assert [runs.step(r) for r in range(full.T)] == [full.step(r) for r in range(full.T)]
    rows = list(range(0, full.T, 7)) + [full.T - 1, full.T, 1 << 40]
    for a, b in zip(W.expected_arrays(runs, rows, 9), W.expected_arrays(full, rows, 9)):
        assert np.array_equal(a, b)
    # the batch form is walk() row by row
    symbols, steps, stops, last, reads = W.expected_arrays(full, rows, 9, fill=7)
    for i, r in enumerate(rows):
        out, stop, at, read = W.walk(full, r, 9)
        assert (symbols[i, :len(out)].tolist(), symbols[i, len(out):].tolist(), int(steps[i]), int(stops[i]), int(last[i])) == (out, [7] * (9 - len(out)), len(out), stop, at)
        assert int(reads[i]) == (int(W.NO_READ) if read is None else read)
