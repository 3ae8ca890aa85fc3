"""Seeded random RLE streams for parity tests (test infrastructure)."""
import numpy as np


def runs_to_bytes(syms, lens):
    """(symbol, length) runs -> RLE bytes: base-32 digits, least significant first, zero
    digits included, nothing for a zero-length run (bwt_converter.rs:151-184 semantics)."""
    syms = np.asarray(syms, dtype=np.uint8)
    lens = np.asarray(lens, dtype=np.uint64)
    ndig = 13
    shifts = (np.arange(ndig, dtype=np.uint64) * np.uint64(5))[None, :]
    rest = lens[:, None] >> shifts
    digits = (rest & np.uint64(31)).astype(np.uint8)
    keep = rest > 0
    out = (syms[:, None] | (digits << 3)).astype(np.uint8)
    return out[keep]


def random_runs(rng, nruns, kind="mixed", alphabet=(0, 1, 2, 3, 4, 5)):
    """Runs with no two neighbours of the same symbol."""
    alphabet = np.asarray(alphabet, dtype=np.uint8)
    first = rng.integers(0, len(alphabet))
    step = rng.integers(1, len(alphabet), size=nruns)  # 1..len-1: never the same symbol twice
    idx = (first + np.concatenate([[0], np.cumsum(step[1:])])) % len(alphabet)
    syms = alphabet[idx]
    if kind == "ones":
        lens = np.ones(nruns, dtype=np.uint64)
    elif kind == "short":
        lens = rng.geometric(0.2, size=nruns).astype(np.uint64)
    elif kind == "long":
        lens = rng.integers(1, 5000, size=nruns).astype(np.uint64)
    else:
        pick = rng.integers(0, 10, size=nruns)
        lens = rng.geometric(0.15, size=nruns).astype(np.uint64)
        special = np.array([32, 1024, 32768, 31, 33, 1023, 1025, 255, 256, 257], dtype=np.uint64)
        lens = np.where(pick == 0, special[rng.integers(0, len(special), size=nruns)], lens)
        lens = np.where(pick == 1, rng.integers(1, 100000, size=nruns).astype(np.uint64), lens)
    return syms, lens


def random_stream(seed, nruns, kind="mixed", alphabet=(0, 1, 2, 3, 4, 5)):
    rng = np.random.default_rng(seed)
    syms, lens = random_runs(rng, nruns, kind, alphabet)
    return runs_to_bytes(syms, lens)


def raw_byte_stream(seed, nbytes):
    """Arbitrary valid bytes: any symbol 0..5 with any digit 0..31 -- zero digits, zero-length
    runs and multi-digit runs appear by chance."""
    rng = np.random.default_rng(seed)
    sym = rng.integers(0, 6, size=nbytes).astype(np.uint8)
    # bias towards repeats so multi-byte runs are common
    rep = rng.random(nbytes) < 0.4
    chain = 1
    for i in range(1, nbytes):
        if rep[i] and chain < 3:  # at most 3 digits per run: lengths stay below 32^3
            sym[i] = sym[i - 1]
        chain = chain + 1 if sym[i] == sym[i - 1] else 1
        if chain > 3:
            sym[i] = (sym[i] + 1) % 6
            chain = 1
    digit = rng.integers(0, 32, size=nbytes).astype(np.uint8)
    digit[rng.random(nbytes) < 0.1] = 0
    return (sym | (digit << 3)).astype(np.uint8)


def run_across_byte(first_byte, length, tail=(3, 40)):
    """A stream in which the digits of ONE run of `length` symbols start at byte `first_byte`: that many alternating one-byte
    runs of A and C in front of it, the run itself of T, and a short run of `tail` = (symbol, length) behind it.  The device
    walks a stream 16 bytes to a thread and 4096 to a workgroup, and a byte's weight depends on the bytes of its run before it:
    a run whose digits lie on both sides of such a border has its weight carried across."""
    syms = [1 + i % 2 for i in range(first_byte)] + [5, tail[0]]
    stream = runs_to_bytes(syms, [1] * first_byte + [length, tail[1]])
    ndigits = (int(length).bit_length() + 4) // 5
    assert (stream[first_byte:first_byte + ndigits] & 7 == 5).all() and (stream[first_byte - 1] & 7, stream[first_byte + ndigits] & 7) == (1 + (first_byte - 1) % 2, tail[0])
    return stream


# four digits, the third of them zero: at bytes 4095 | 4096..4098 (a tile's last byte and the next tile's first three) and at bytes
# 15 | 16..18 (the same for two threads)
FOUR_DIGITS = 5 + 7 * 32 + 0 * 32 ** 2 + 3 * 32 ** 3
BORDER_STREAMS = {"tile border": lambda: run_across_byte(4095, FOUR_DIGITS), "thread border": lambda: run_across_byte(15, FOUR_DIGITS)}
# eight digits, the eighth the only one that is not zero, at bytes 13..15 | 16..20: the largest weight a byte can have, 32^7 -- so
# this stream has 2^35 symbols, and nothing that expands it is small
EIGHT_DIGITS = lambda: run_across_byte(13, 32 ** 7)


def canonical_runs(stream):
    """The canonical RLE bytes of what `stream` decodes to, from its runs alone (no symbol array): a run is a maximal group of
    bytes of one symbol, neighbouring runs of one symbol join, a run of no symbols vanishes."""
    stream = np.asarray(stream, dtype=np.uint8)
    if stream.size == 0:
        return stream
    sym = stream & 7
    head = np.flatnonzero(np.concatenate([[True], sym[1:] != sym[:-1]]))
    index = np.arange(stream.size) - np.repeat(head, np.diff(np.concatenate([head, [stream.size]])))
    assert index.max() < 12
    value = (stream >> 3).astype(np.uint64) << (np.uint64(5) * index.astype(np.uint64))
    lens, syms = np.add.reduceat(value, head), sym[head]
    syms, lens = syms[lens > 0], lens[lens > 0]
    if syms.size == 0:
        return np.empty(0, dtype=np.uint8)
    head = np.flatnonzero(np.concatenate([[True], syms[1:] != syms[:-1]]))
    return runs_to_bytes(syms[head], np.add.reduceat(lens, head))


def random_kmers(seed, n, k, alphabet=(1, 2, 3, 5)):
    rng = np.random.default_rng(seed)
    alphabet = np.asarray(alphabet, dtype=np.uint8)
    return alphabet[rng.integers(0, len(alphabet), size=(n, k))]
