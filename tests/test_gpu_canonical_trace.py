"""Canonical traces (csrc/canonical_trace.hip, csrc/trace_calls.cpp: msbwt_rle_trace_canonical_kmers[_device]): from seed k-mers through
the strand-merged k-mer graph, node by node.

Expected values never come from the code under test: tests/canonical_trace_oracle.py is the header's definition over strings (checked
against the canonical unitig oracle in tests/test_canonical_trace_oracle.py), closed forms for a random chain read from both strands,
and -- where exactly that is asked -- the library's own enumerate_canonical_unitigs, which tests/test_gpu_canonical_unitigs.py holds to
its oracle.  Two properties need no oracle: the trace of rc(s) in the other direction mirrors the trace of s, and an index does not see
which strand a read came from.

Shapes: ragged sets of 1-50 reads of 0-70 symbols with N, duplicates and prefixes, as they are and with every second read reverse-
complemented, at every k where a word's layout changes (1 .. 4, 15 .. 17, 30, 31) -- the even k with min_count >= 2 run the node
clause's queries --, seeds that are nodes (both members of a class), below the threshold, absent, repeated and dirty above bit 2k, step
limits 0, 1, 7 and past every walk; the hand-made sets of the definition; the 4000-read set with errors from both strands against its
canonical unitigs; a 5 000-base chain read from both strands (5 000 rounds of one walk; 78 walks in one batch, which is no multiple of
a wave; pieces of 64 walks); every index form; host form, device form and torch tensors.  Run with `pytest -m gpu`."""
import ctypes as C
import importlib

import numpy as np
import pytest

import canonical_trace_oracle as CT
from test_canonical_trace_oracle import LITERALS
from test_gpu_canonical_unitigs import both_strands, flip_every_second, rc
from test_gpu_merge_many import EMPTY
from test_gpu_reads_build import naive_rle, ragged_set
from test_gpu_spectrum import loaded
from test_gpu_trace import ALL_FORMS, DIRECTIONS, KS, MODES, NAMES, SENTINEL, chain, chain_walks, check, words_of

pytestmark = pytest.mark.gpu

msbwt = importlib.import_module("rust-msbwt_amd")
_lib = msbwt._lib
U64 = np.uint64
THRESHOLDS = ((1, 0), (2, 0), (1, 3), (3, 0))  # (min_count, min_edge)
INFO = ("walks", "rounds", "queries", "steps", "longest", "pieces", "scratch_bytes", "not_nodes")


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def run(b, words, k, max_steps, mode, direction, min_count=1, min_edge=0, targets=None):
    """the call with the rows pre-filled with the sentinel"""
    symbols = np.full((len(words), max_steps), SENTINEL, dtype=np.uint8)
    got = b.trace_canonical_kmers(words, k, max_steps, mode=mode, direction=direction, min_count=min_count, min_edge=min_edge or None, targets=targets, symbols=symbols)
    assert got[0] is symbols
    assert [g.dtype for g in got] == [np.uint8, U64, np.uint8, U64, U64, np.uint8]
    return got


def seeds_of(g, k, rng):
    """every node (both members of every class), every k-mer below the threshold that occurs on either strand, a few absent ones,
    duplicates -- and the words, some dirty above bit 2k"""
    nodes = sorted(g.nodes)
    absent = [q for q in ("".join(rng.choice(list("ACGT"), size=k)) for _ in range(6)) if q not in g.nodes and q not in g.below][:3]
    kmers = nodes + g.below + absent + nodes[:5] + nodes[-2:]
    words = words_of(kmers)
    dirty = rng.random(len(words)) < 0.3
    garbage = rng.integers(1, 1 << min(64 - 2 * k, 62), size=len(words), dtype=np.uint64) << U64(2 * k)
    return kmers, np.where(dirty, words | garbage, words)


def queries_of(got, n, k, min_count, mode):
    """Queries searched, exactly: (10 + E) n in round 0, then 8 + E (UNITIG: 16 + 2 E) a live walk and round; a walk of s steps is live in
    s later rounds, and in one more where MERGE or, in UNITIG mode, RETURNED stops it.  MIRROR costs no round."""
    E = 1 if k % 2 == 0 and min_count >= 2 else 0
    unitig = mode == "unitig"
    extra = (got[2] == CT.MERGE) | ((got[2] == CT.RETURNED) if unitig else np.zeros(len(got[2]), dtype=bool))
    live = int(got[1].sum()) + int(extra.sum())
    return (10 + E) * n + (16 + 2 * E if unitig else 8 + E) * live


def check_info(b, got, want, k, min_count, max_steps, mode, targets=False, piece=0):
    n = len(want[1])
    info = b.canonical_trace_info()
    assert tuple(info) == INFO
    assert info["walks"] == n and info["rounds"] <= (max_steps + 1) * info["pieces"] and info["pieces"] == -(-n // (piece or 2 ** 20))
    assert info["steps"] == int(want[1].sum()) and info["longest"] == int(want[1].max(initial=0))
    assert info["not_nodes"] == int((want[2] == CT.NOT_A_NODE).sum())
    assert info["queries"] == queries_of(got, n, k, min_count, mode), (info, k, min_count, mode)
    assert info["scratch_bytes"] == msbwt.canonical_trace_plan(n, max_steps, mode, targets=targets, host=True, piece=piece)
    return info


COMPLEMENT_CODE = np.zeros(256, dtype=np.uint8)
COMPLEMENT_CODE[[1, 2, 3, 5, SENTINEL]] = [5, 3, 2, 1, SENTINEL]


def rc_words(words, k):
    return words_of([rc(CT.kmer_of(w, k)) for w in (words & U64((1 << 2 * k) - 1))])


def mirrored(got, k):
    """the six outputs of the traces of the reverse complements in the other direction, from those of the seeds (UNIQUE and UNITIG)"""
    symbols, steps, stops, sums, last, fans = got
    flipped = np.zeros_like(fans)
    for j in range(4):
        flipped |= ((fans >> j) & 1) << (3 - j)
    return COMPLEMENT_CODE[symbols], steps, stops, sums, rc_words(last, k), flipped


# ---- 1. exactness on small sets, the two properties beside it ----

@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("seed", [0, 1, 2, 5, 11])
def test_ragged_sets(orc, seed, k):
    reads = ragged_set(seed)
    b, f = loaded(naive_rle(orc, reads)), loaded(naive_rle(orc, flip_every_second(reads)))
    rng = np.random.default_rng(seed * 100 + k)
    moved = 0
    for min_count, min_edge in THRESHOLDS:
        g = CT.Graph(reads, k, min_count, min_edge)
        kmers, words = seeds_of(g, k, rng)
        mirror_words = rc_words(words, k)
        for mode in MODES:
            for direction, other in (DIRECTIONS, DIRECTIONS[::-1]):
                for max_steps in (0, 1, 7, 200):
                    what = (seed, k, min_count, min_edge, mode, direction, max_steps)
                    want = CT.expected_arrays(g, kmers, mode, direction, max_steps)
                    got = run(b, words, k, max_steps, mode, direction, min_count, min_edge)
                    check(got, want, what)
                    check_info(b, got, want, k, min_count, max_steps, mode)
                    # the index of the same reads with every second one reverse-complemented returns the same bytes
                    check(run(f, words, k, max_steps, mode, direction, min_count, min_edge), got, what + ("flipped",))
                    if mode != "greedy" and max_steps in (7, 200):  # the trace of rc(s) in the other direction is the mirror
                        check(run(b, mirror_words, k, max_steps, mode, other, min_count, min_edge), mirrored(got, k), what + ("mirror",))
                    moved += int(want[1].sum())
        # targets: a node a seed, drawn from the nodes; most lie off the seed's path, some on it, some are the seed
        if g.nodes:
            nodes = sorted(g.nodes)
            targets = [nodes[i] for i in rng.integers(0, len(nodes), size=len(kmers))]
            for mode, direction in (("greedy", "right"), ("unitig", "left")):
                want = CT.expected_arrays(g, kmers, mode, direction, 200, targets)
                got = run(b, words, k, 200, mode, direction, min_count, min_edge, words_of(targets))
                check(got, want, (seed, k, "targets", mode, direction))
                check_info(b, got, want, k, min_count, 200, mode, targets=True)
    assert moved > 0 or k > 17 or seed == 0  # (the short k always move)


# ---- 2. the hand-made sets of the definition, through the library ----

def test_hand_made_sets(orc):
    for reads, k, min_count, seed, modes, direction, more, want in LITERALS:
        b, g = loaded(naive_rle(orc, reads)), CT.Graph(reads, k, min_count)
        for mode in modes:
            max_steps, target = more.get("max_steps", 50), more.get("target")
            got = run(b, words_of([seed]), k, max_steps, mode, direction, min_count, targets=None if target is None else words_of([target]))
            check(got, CT.expected_arrays(g, [seed], mode, direction, max_steps, None if target is None else [target]), (reads, seed, mode))
            row = "".join("?ACG?T"[c] for c in got[0][0, :int(got[1][0])])
            assert (row, int(got[1][0]), int(got[2][0]), int(got[3][0]), CT.kmer_of(got[4][0], k), int(got[5][0]))[:len(want)] == want, (reads, seed, mode)
        # every node of the set, in all modes and both directions
        kmers = sorted(g.nodes) + g.below
        for mode in MODES:
            for direction_ in DIRECTIONS:
                check(run(b, words_of(kmers), k, 40, mode, direction_, min_count), CT.expected_arrays(g, kmers, mode, direction_, 40), (reads, mode, direction_))


def test_guards_on_a_loaded_index(orc):
    b = loaded(naive_rle(orc, ["ACGTACCGGT"]))
    lib, seeds = _lib.lib(), words_of(["ACGTA", "CGTAC"])
    steps = np.full(2, 77, dtype=U64)
    p = seeds.ctypes.data_as(C.c_void_p)

    def call(k=5, n=2, min_count=1, min_edge=0, mode=0, direction=0, max_steps=4, seeds=p):
        return lib.msbwt_rle_trace_canonical_kmers(b._h, seeds, None, k, n, min_count, min_edge, mode, direction, max_steps, None, steps.ctypes.data_as(C.c_void_p),
                                                   None, None, None, None)

    def last_error():
        return lib.msbwt_rle_last_error(b._h).decode()

    for bad in (dict(k=0), dict(k=32), dict(k=33), dict(min_count=3, min_edge=2), dict(mode=3), dict(mode=-1), dict(direction=2), dict(direction=-1), dict(seeds=None)):
        assert call(**bad) == _lib.ERR_INVALID_ARG, bad
        assert last_error() != ""
    assert "1 <= k <= 31" in (call(k=32), last_error())[1] and "min_edge" in (call(min_count=3, min_edge=2), last_error())[1]
    assert "trace_canonical_kmers" in (call(mode=3), last_error())[1]
    # the order of the ladder: k before the thresholds before the mode before the direction before the seeds before the size
    assert "1 <= k" in (call(k=32, min_count=3, min_edge=2, mode=3), last_error())[1] and "min_edge" in (call(min_count=3, min_edge=2, mode=3), last_error())[1]
    assert "mode" in (call(mode=3, direction=2, seeds=None), last_error())[1] and "direction" in (call(direction=2, seeds=None, max_steps=2 ** 40), last_error())[1]
    assert call(seeds=None, max_steps=2 ** 40) == _lib.ERR_INVALID_ARG
    for bad in (dict(max_steps=2 ** 40), dict(n=2 ** 30, max_steps=2 ** 10)):
        assert call(**bad) == _lib.ERR_TOO_LARGE, bad
    assert (steps == 77).all()
    assert lib.msbwt_rle_trace_canonical_kmers_device(b._h, None, None, 5, 2, 1, 0, 0, 0, 4, None, None, None, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert call(n=0, seeds=None) == 0 and call() == 0 and steps.tolist() == [4, 4]


# ---- 3. agreement with enumerate_canonical_unitigs on reads with errors from both strands ----

@pytest.mark.parametrize("min_count", [1, 2])
@pytest.mark.parametrize("k", [15, 31])
def test_unitig_mode_reproduces_the_canonical_unitigs(k, min_count):
    _, rle, _ = both_strands("plain_100")
    b = loaded(rle)
    symbols, offsets, sums, ends, flags = b.enumerate_canonical_unitigs(k, min_count=min_count)
    info = b.canonical_unitig_info()
    U, longest = len(sums), info["longest"]
    assert U > (1000 if min_count == 1 else 50) and longest > 50  # (the errors branch the graph; min_count = 2 drops most of them)
    code = np.zeros(6, dtype=U64)
    code[[1, 2, 3, 5]] = [0, 1, 2, 3]
    two = code[symbols]
    starts, ends_at = offsets[:-1].astype(np.int64), offsets[1:].astype(np.int64)
    first, last = np.zeros(U, dtype=U64), np.zeros(U, dtype=U64)
    for j in range(k):
        first = (first << U64(2)) | two[starts + j]
        last = (last << U64(2)) | two[ends_at - k + j]
    nodes = (ends_at - starts - (k - 1)).astype(U64)
    column = np.arange(longest)[None, :]
    for direction, seeds in (("right", first), ("left", last)):
        rows, steps, stops, edge_sums, end, fans = b.trace_canonical_kmers(seeds, k, longest, mode="unitig", direction=direction, min_count=min_count)
        assert np.array_equal(steps, nodes - U64(1)) and int(steps.sum()) + U == info["classes"]
        assert np.array_equal(stops == CT.RETURNED, flags & 1 == 1) and np.isin(stops[flags & 1 == 0], (CT.DEAD_END, CT.BRANCH, CT.MERGE, CT.MIRROR)).all()
        assert np.array_equal(end, last if direction == "right" else first)
        # every unitig's symbols: behind its first k (RIGHT), or before its last k, reversed (LEFT)
        valid = column < steps[:, None].astype(np.int64)
        at = (starts[:, None] + k + column) if direction == "right" else (ends_at[:, None] - k - 1 - column)
        assert np.array_equal(rows[valid], symbols[at[valid]]) and not rows[~valid].any()
        # the fans of the last node are the ends' bits on that side
        assert np.array_equal(fans, ends >> 4 if direction == "right" else ends & 15)
        t = b.canonical_trace_info()
        assert t["rounds"] <= longest + 1 and t["longest"] == longest - 1 and t["steps"] == info["classes"] - U and t["not_nodes"] == 0
        assert t["queries"] == queries_of((rows, steps, stops), U, k, min_count, "unitig")
        print("k = %d, min_count = %d, %s: %d unitigs, %d MIRROR, %s" % (k, min_count, direction, U, int((stops == CT.MIRROR).sum()), t))


# ---- 4. rounds, compaction and pieces ----

_both = {}


def chain_of_both_strands():
    """A handle with the chain's reads loaded, every second one reverse-complemented.  No k-mer of the text is the reverse complement of
    one, so D along the text is the chain, and cc of an edge is its count among the reads as they were: chain_walks' closed forms hold."""
    if not _both:
        c = chain()
        for k in (21, 31):
            assert not set(CT.windows([c["text"]], k)) & set(CT.windows([rc(c["text"])], k))
        flipped = flip_every_second(c["reads"])
        assert flipped[1] == rc(c["reads"][1]) and flipped[0] == c["reads"][0]
        _both["rle"] = msbwt.RleBWT(device=0).build_from_reads(flipped, ascii=True)
        _both["b"] = loaded(_both["rle"])
    return _both["b"]


def check_round_structure(b, got, n, k, max_steps, mode, targets=False, piece=0):
    return check_info(b, got, got, k, 1, max_steps, mode, targets=targets, piece=piece)


@pytest.mark.parametrize("k,direction,mode", [(21, "right", "unitig"), (31, "left", "unique")])
def test_one_walk_down_the_chain(k, direction, mode):
    b, text = chain_of_both_strands(), chain()["text"]
    p = 0 if direction == "right" else 5000 - k
    want = chain_walks(k, [p], 5000, direction)
    assert int(want[1][0]) == 5000 - k and want[2][0] == CT.DEAD_END
    got = run(b, words_of([text[p:p + k]]), k, 5000, mode, direction)
    check(got, want, (k, direction))
    assert msbwt.trace_sequences(words_of([text[p:p + k]]), k, got[0], got[1], direction, text=True) == [text]
    info = check_round_structure(b, got, 1, k, 5000, mode)
    assert info["rounds"] == 5000 - k + 1 and info["longest"] == info["steps"] == 5000 - k
    assert info["queries"] == 10 + (16 if mode == "unitig" else 8) * (5000 - k)
    # the other strand of the same walk: the mirror, word for word
    back = run(b, rc_words(words_of([text[p:p + k]]), k), k, 5000, mode, "left" if direction == "right" else "right")
    check(back, mirrored(got, k), (k, direction, "mirror"))
    print("k = %d %s: %s" % (k, direction, info))


@pytest.mark.parametrize("mode", MODES)
def test_every_64th_node_in_one_batch(mode):
    k, max_steps = 21, 300
    b, text = chain_of_both_strands(), chain()["text"]
    positions = list(range(0, 5000 - k + 1, 64))
    assert len(positions) == 78 and len(positions) % 64
    for direction in DIRECTIONS:
        want = chain_walks(k, positions, max_steps, direction)
        assert set(want[2].tolist()) == {CT.MAX_STEPS, CT.DEAD_END} and len(set(want[1].tolist())) > 3  # the walks end in different rounds
        got = run(b, words_of([text[p:p + k] for p in positions]), k, max_steps, mode, direction)
        check(got, want, (mode, direction))
        info = check_round_structure(b, got, len(positions), k, max_steps, mode)
        assert info["rounds"] == max_steps + 1


@pytest.mark.parametrize("n", [200, 1])
def test_pieces_of_64_walks_give_the_same_bytes(n):
    k, max_steps = 21, 50
    b, text = chain_of_both_strands(), chain()["text"]
    positions = [(37 * i) % (5000 - k + 1) for i in range(n)]
    seeds, targets = words_of([text[p:p + k] for p in positions]), words_of([text[p + 30:p + 30 + k] if p + 30 + k <= 5000 else text[:k] for p in positions])
    for mode, direction, tg in (("unitig", "right", None), ("greedy", "left", None), ("unique", "right", targets)):
        auto = run(b, seeds, k, max_steps, mode, direction, targets=tg)
        if tg is None:
            check(auto, chain_walks(k, positions, max_steps, direction), (n, mode, direction))
        else:
            assert (auto[2] == CT.TARGET).sum() >= n // 2 and (auto[1][auto[2] == CT.TARGET] == 30).all()
        assert check_round_structure(b, auto, n, k, max_steps, mode, targets=tg is not None)["pieces"] == 1
        b.set_trace_piece(64)
        try:
            pieces = run(b, seeds, k, max_steps, mode, direction, targets=tg)
            info = check_round_structure(b, pieces, n, k, max_steps, mode, targets=tg is not None, piece=64)
        finally:
            b.set_trace_piece(0)
        assert info["pieces"] == (4 if n == 200 else 1)
        check(pieces, auto, (n, mode, direction, "pieces"))


def test_pieces_with_the_node_clause(orc):
    """even k and min_count = 2: the far ends' queries lie behind a PIECE's edge queries, whatever the piece"""
    reads = ["GGAATTCCA", "CATG", "TTACGTAA", "CATGC", "GGAATTC"]
    b = loaded(naive_rle(orc, reads))
    for k in (2, 4):
        g = CT.Graph(reads, k, 2)
        kmers, words = seeds_of(g, k, np.random.default_rng(k))
        assert len(words) > 6 and any(rc(q) == q for q in g.below)  # (a palindrome that occurs and is no node,
        assert any(g.cc(q + c) >= g.me and (q + c)[1:] not in g.nodes for q in g.nodes for c in "ACGT")  # and an edge by count that lacks it)
        for mode in MODES:
            for direction in DIRECTIONS:
                want = CT.expected_arrays(g, kmers, mode, direction, 60)
                for piece in (0, 3, 5):
                    b.set_trace_piece(piece)
                    try:
                        got = run(b, words, k, 60, mode, direction, 2)
                        check(got, want, (k, mode, direction, piece))
                        assert check_info(b, got, want, k, 2, 60, mode, piece=piece)["pieces"] == (-(-len(words) // piece) if piece else 1)
                    finally:
                        b.set_trace_piece(0)


# ---- 5. every index form gives the same bytes ----

@pytest.mark.parametrize("form", sorted(ALL_FORMS))
def test_every_index_form_gives_the_same_bytes(orc, form):
    knobs = ALL_FORMS[form]
    reads = ragged_set(5)
    b = loaded(naive_rle(orc, reads), **knobs)
    assert b.get_block_format() == knobs.get("block_format", "planes")
    rng = np.random.default_rng(3)
    for k, min_count in ((3, 1), (16, 2), (31, 1)):
        g = CT.Graph(reads, k, min_count, 0)
        kmers, words = seeds_of(g, k, rng)
        for mode in MODES:
            for direction in DIRECTIONS:
                check(run(b, words, k, 80, mode, direction, min_count), CT.expected_arrays(g, kmers, mode, direction, 80), (form, k, mode, direction))
    c = chain()
    chain_of_both_strands()
    b = loaded(_both["rle"], **knobs)
    positions = list(range(0, 4970, 64))
    for k, direction in ((21, "right"), (31, "left")):
        got = run(b, words_of([c["text"][p:p + k] for p in positions]), k, 150, "unitig", direction)
        check(got, chain_walks(k, positions, 150, direction), (form, k, direction))


# ---- 6. host form, device form, torch tensors; NULL outputs; n = 0; an empty index; the existing call ----

def test_host_form_device_form_and_torch_tensors_give_the_same_bytes(orc):
    import torch
    reads = ragged_set(2)
    k, max_steps, min_count = 4, 30, 2  # (the node clause's queries run)
    b = loaded(naive_rle(orc, reads))
    g = CT.Graph(reads, k, min_count)
    kmers, words = seeds_of(g, k, np.random.default_rng(9))
    nodes = sorted(g.nodes)
    targets = words_of([nodes[(7 * i) % len(nodes)] for i in range(len(kmers))])
    dev = torch.device("cuda:0")
    before = b.device_bytes()
    for mode, direction, tg in (("unitig", "right", None), ("greedy", "left", targets), ("unique", "left", None)):
        want = CT.expected_arrays(g, kmers, mode, direction, max_steps, None if tg is None else [CT.kmer_of(w, k) for w in tg])
        host = run(b, words, k, max_steps, mode, direction, min_count, targets=tg)
        check(host, want, ("host", mode, direction))
        d_seeds = torch.from_numpy(words.view(np.int64)).to(dev)
        d_targets = None if tg is None else torch.from_numpy(tg.view(np.int64)).to(dev)
        for stream in (torch.cuda.current_stream(dev), torch.cuda.Stream(dev)):
            with torch.cuda.stream(stream):
                d_symbols = torch.full((len(words), max_steps), SENTINEL, dtype=torch.uint8, device=dev)
                stream.synchronize()
                got = b.trace_canonical_kmers(d_seeds, k, max_steps, mode=mode, direction=direction, min_count=min_count, targets=d_targets, symbols=d_symbols)
                b.device_status(stream.cuda_stream)
            assert got[0] is d_symbols and all(t.device == dev for t in got)
            check([t.cpu().numpy().view(w.dtype) for t, w in zip(got, want)], want, ("torch", mode, direction))
            assert b.canonical_trace_info()["scratch_bytes"] == msbwt.canonical_trace_plan(len(words), max_steps, mode, targets=tg is not None, host=False)
        # NULL outputs in every combination: what is asked for is what the full call gave, and nothing else is written
        d_full = [torch.from_numpy(w.copy()).to(dev) if w.dtype == np.uint8 else torch.from_numpy(w.view(np.int64).copy()).to(dev) for w in want]
        for wanted in (range(64) if tg is None and mode == "unitig" else (0b101010, 0b010101, 0b000001)):
            outs = [np.full_like(w, SENTINEL) for w in want]
            ptrs = [o.ctypes.data_as(C.c_void_p) if wanted >> j & 1 else None for j, o in enumerate(outs)]
            rc_ = _lib.lib().msbwt_rle_trace_canonical_kmers(b._h, words.ctypes.data_as(C.c_void_p), None if tg is None else tg.ctypes.data_as(C.c_void_p), k, len(words),
                                                             min_count, 0, _lib.TRACE_MODES[mode], _lib.TRACE_DIRECTIONS[direction], max_steps, *ptrs)
            assert rc_ == 0, _lib.lib().msbwt_rle_last_error(b._h)
            for j, (o, w) in enumerate(zip(outs, want)):
                assert np.array_equal(o, w) if wanted >> j & 1 else (o == SENTINEL).all(), (wanted, NAMES[j])
            if wanted % 9 == 0 or wanted == 0b101010:  # the device form, a few of them
                d_outs = [torch.full_like(t, SENTINEL if t.dtype == torch.uint8 else -1) for t in d_full]
                b.trace_canonical_kmers_device(d_seeds.data_ptr(), k, len(words), max_steps, *[t.data_ptr() if wanted >> j & 1 else None for j, t in enumerate(d_outs)],
                                               mode=_lib.TRACE_MODES[mode], direction=_lib.TRACE_DIRECTIONS[direction], min_count=min_count,
                                               d_targets=None if tg is None else d_targets.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
                b.device_status(torch.cuda.current_stream(dev).cuda_stream)
                for j, (t, f) in enumerate(zip(d_outs, d_full)):
                    assert torch.equal(t, f) if wanted >> j & 1 else bool((t == (SENTINEL if t.dtype == torch.uint8 else -1)).all()), (wanted, NAMES[j])
    assert b.device_bytes() == before
    # n = 0
    got = b.trace_canonical_kmers(np.zeros(0, dtype=U64), k, 5)
    assert [g_.shape for g_ in got] == [(0, 5), (0,), (0,), (0,), (0,), (0,)] and not any(b.canonical_trace_info().values())
    got = b.trace_canonical_kmers(torch.zeros(0, dtype=torch.int64, device=dev), k, 5)
    assert got[0].shape == (0, 5) and got[1].numel() == 0


def test_an_empty_index():
    import torch
    b = loaded(EMPTY)
    k = 7
    words = np.array([0, 5, (1 << 14) - 1, 1 << 14 | 9, 2 ** 64 - 1], dtype=U64)
    for mode in MODES:
        symbols, steps, stops, sums, last, fans = run(b, words, k, 6, mode, "left")
        assert (symbols == SENTINEL).all() and not steps.any() and not sums.any() and not fans.any() and (stops == CT.NOT_A_NODE).all()
        assert last.tolist() == [0, 5, (1 << 14) - 1, 9, (1 << 14) - 1]
        info = b.canonical_trace_info()
        assert info == {"walks": 5, "rounds": 0, "queries": 0, "steps": 0, "longest": 0, "pieces": 0, "scratch_bytes": 0, "not_nodes": 5}
    dev = torch.device("cuda:0")
    got = b.trace_canonical_kmers(torch.from_numpy(words.view(np.int64)).to(dev), k, 6, mode="unitig")
    assert not got[0].any() and (got[2] == CT.NOT_A_NODE).all() and got[4].cpu().numpy().view(U64).tolist() == [0, 5, (1 << 14) - 1, 9, (1 << 14) - 1]
    assert b.trace_canonical_kmers(np.zeros(0, dtype=U64), k, 6)[1].size == 0


def test_the_existing_call_before_and_after(orc):
    """trace_kmers returns the same bytes before and after a canonical call, and each call's info words are its own"""
    import trace_oracle as T
    reads = ragged_set(11)
    k = 4
    b = loaded(naive_rle(orc, reads))
    plain, merged = T.Graph(reads, k, 2), CT.Graph(reads, k, 2)
    kmers, words = seeds_of(merged, k, np.random.default_rng(4))
    symbols = np.full((len(words), 40), SENTINEL, dtype=np.uint8)
    before = b.trace_kmers(words, k, 40, mode="unitig", min_count=2, symbols=symbols.copy())
    check(before, T.expected_arrays(plain, kmers, "unitig", "right", 40), "before")
    info = b.trace_info()
    assert not any(b.canonical_trace_info().values())
    got = run(b, words, k, 40, "unitig", "right", 2)
    check(got, CT.expected_arrays(merged, kmers, "unitig", "right", 40), "canonical")
    assert b.trace_info() == info and b.canonical_trace_info()["queries"] > info["queries"] and b.canonical_trace_info() != info
    canonical_info = b.canonical_trace_info()
    after = b.trace_kmers(words, k, 40, mode="unitig", min_count=2, symbols=symbols.copy())
    check(after, before, "after")
    assert b.trace_info() == info and b.canonical_trace_info() == canonical_info
