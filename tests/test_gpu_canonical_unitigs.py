"""Canonical unitigs (csrc/canonical_unitigs.hip, csrc/unitig_calls.cpp): the strand-merged k-mer graph compacted into its non-branching
paths on the device, every class of a k-mer and its reverse complement in exactly one unitig exactly once.

Expected values never come from the code under test.  The oracle is Python over the reads as strings, in the style of
test_gpu_unitigs.unitigs_of_texts: Counters of the ACGT-only windows at k and at k + 1 give the class counts cc(x) = count(x) +
count(rc(x)) (a palindrome once); the nodes are both members of every class with cc >= m; q -> q' is an edge when cc(q.c) >= me and both
ends are nodes; the links are the edges with out(p) = 1 and in(q) = 1 less the two cuts (a palindromic node has none; q -> rc(q) is never
one); heads are walked in sorted order, cycles opened at their smallest member, and of U and rc(U) the one with the smaller first word
is kept.  The literal cases pin the oracle itself.  Properties that need no oracle are checked on every case beside it.

Shapes: the hand-made sets of the definitions; ragged sets of 1-50 reads with N, duplicates and prefixes at every k, as they are and
with every second read reverse-complemented; a 20 000-base chain and a 600-base circle for the rounds; 4000 reads with errors from
both strands (4.0e5 symbols) under four thresholds; a frontier at its minimum; every index form.  Run with `pytest -m gpu`."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest

from test_gpu_kmer_graph import FORMS, thresholds, windows
from test_gpu_reads_build import naive_rle, ragged_set, read_set
from test_gpu_spectrum import loaded
from test_gpu_unitigs import CODE, NAMES, texts_of_codes, unitigs_of_texts

pytestmark = pytest.mark.gpu

msbwt = importlib.import_module("rust-msbwt_amd")
_lib = msbwt._lib
MsbwtError = msbwt.MsbwtError
U64 = np.uint64
KS = (1, 2, 3, 4, 15, 16, 17, 30, 31)
COMPLEMENT = str.maketrans("ACGT", "TGCA")
INFO = ("classes", "edge_classes", "links", "unitigs", "symbols", "circular", "longest", "palindromes", "cut_links")


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def rc(s):
    return s.translate(COMPLEMENT)[::-1]


def flip_every_second(reads):
    """the same reads with every second one reverse-complemented (N stays N)"""
    return [rc(r) if i % 2 else r for i, r in enumerate(reads)]


# ---- the oracle: what the canonical unitigs of a read set ARE, from its windows alone ----

def canonical_unitigs_of_counters(at_k, at_k1, k, min_count=1, min_edge=0):
    m, me = thresholds(min_count, min_edge)

    def cc(counter, x):  # (a Counter answers 0 for what it does not hold)
        r = rc(x)
        return counter[x] if r == x else counter[x] + counter[r]

    nodes = {}
    for q in at_k:
        n = cc(at_k, q)
        if n >= m:
            nodes[q] = nodes[rc(q)] = n
    succ = {q: [c for c in "ACGT" if q[1:] + c in nodes and cc(at_k1, q + c) >= me] for q in nodes}
    pred = {q: [c for c in "ACGT" if (c + q)[:-1] in nodes and cc(at_k1, c + q) >= me] for q in nodes}
    for q in nodes:  # D is symmetric: in-bit j of q is out-bit 3 - j of rc(q)
        assert sorted(pred[q]) == sorted(c.translate(COMPLEMENT) for c in succ[rc(q)])
    up, cut = {}, 0
    for q in nodes:
        if len(pred[q]) == 1:
            p = pred[q][0] + q[:-1]
            if len(succ[p]) == 1:
                if rc(q) == q or rc(p) == p or rc(p + q[-1]) == p + q[-1]:
                    cut += 1
                else:
                    up[q] = p
    down = {p: q for q, p in up.items()}
    assert len(down) == len(up)
    seen, found, head_of = set(), [], {}

    def walk(first, circular):
        path = [first]
        while path[-1] in down and down[path[-1]] != first:
            path.append(down[path[-1]])
        assert not seen & set(path)
        seen.update(path)
        head_of.update((q, first) for q in path)
        found.append((first, path, circular))

    for q in sorted(nodes):
        if q not in up:
            walk(q, False)
    for q in sorted(nodes):
        if q not in seen:
            walk(q, True)
    assert len(seen) == len(nodes)
    # the choice: of U and rc(U), the one whose head is smaller (a palindromic node is its own mirror)
    kept = [(first, path, circular) for first, path, circular in found if first <= head_of[rc(path[-1])]]
    for first, path, _ in found:
        mirror = head_of[rc(path[-1])]
        assert (mirror == first) == (len(path) == 1 and rc(first) == first), "a unitig is its own mirror exactly when it is a palindromic node"
    kept.sort()
    classes = {min(q, rc(q)) for q in nodes}
    assert sorted(min(q, rc(q)) for _, path, _ in kept for q in path) == sorted(classes)  # every class in exactly one unitig exactly once
    seqs = [path[0] + "".join(q[-1] for q in path[1:]) for _, path, _ in kept]
    ends = [sum(1 << "ACGT".index(c) for c in pred[path[0]]) | sum(16 << "ACGT".index(c) for c in succ[path[-1]]) for _, path, _ in kept]
    lengths = [len(s) for s in seqs]
    out = {"seqs": seqs,
           "symbols": np.array([CODE[c] for s in seqs for c in s], dtype=np.uint8),
           "offsets": np.concatenate([[0], np.cumsum(lengths)]).astype(U64),
           "count_sums": np.array([sum(nodes[q] for q in path) for _, path, _ in kept], dtype=U64),
           "ends": np.array(ends, dtype=np.uint8),
           "flags": np.array([int(c) for _, _, c in kept], dtype=np.uint8),
           "first": [path[0] for _, path, _ in kept], "last": [path[-1] for _, path, _ in kept]}
    circular = sum(int(c) for _, _, c in kept)
    out["info"] = {"classes": len(classes), "edge_classes": len({min(q + c, rc(q + c)) for q in nodes for c in succ[q]}),
                   "links": len(classes) + circular - len(kept), "unitigs": len(kept), "symbols": int(sum(lengths)), "circular": circular,
                   "longest": max([len(path) for _, path, _ in kept], default=0), "palindromes": sum(1 for q in nodes if rc(q) == q), "cut_links": cut}
    assert out["info"]["symbols"] == len(classes) + len(kept) * (k - 1)  # S = n + U (k - 1)
    assert len(nodes) == 2 * len(classes) - out["info"]["palindromes"]
    return out


def canonical_unitigs_of_texts(reads, k, min_count=1, min_edge=0):
    return canonical_unitigs_of_counters(windows(reads, k), windows(reads, k + 1), k, min_count, min_edge)


def check_properties(b, k, got, min_count=1):
    """what needs no oracle"""
    symbols, offsets, sums, ends, flags = got
    U, S = len(sums), len(symbols)
    seqs = texts_of_codes(symbols, offsets)
    words, counts = b.enumerate_canonical_kmers(k, min_count=min_count)
    n = len(words)
    assert S == n + U * (k - 1) and sum(len(s) - k + 1 for s in seqs) == n
    emitted = set(seqs)
    for s in seqs:
        assert rc(s) not in emitted or (len(s) == k and rc(s) == s), s
    assert all(a[:k] < z[:k] for a, z in zip(seqs, seqs[1:]))  # first words ascend
    if U:
        fwd, rev, at = b.count_ragged_read_kmers([symbols[int(a):int(z)] for a, z in zip(offsets[:-1], offsets[1:])], k, ascii=False, revcomp=True)
        own_mirror = np.array([rc(s[i:i + k]) == s[i:i + k] for s in seqs for i in range(len(s) - k + 1)])
        per_node = fwd + np.where(own_mirror, U64(0), rev)
        assert (per_node >= U64(max(min_count, 1))).all()
        assert np.array_equal(np.add.reduceat(per_node, at[:-1].astype(np.int64)), sums)
        assert int(sums.sum()) == int(counts.sum())


def check_canonical(b, k, want, min_count=1, min_edge=0):
    got = b.enumerate_canonical_unitigs(k, min_count=min_count, min_edge=min_edge or None)
    for name, g in zip(NAMES, got):
        assert g.dtype == want[name].dtype, name
        assert g.shape == want[name].shape and np.array_equal(g, want[name]), (k, min_count, min_edge, name, g[:8], want[name][:8])
    info = b.canonical_unitig_info()
    if want["info"]["classes"]:
        assert {x: info[x] for x in INFO} == want["info"], (k, min_count, min_edge)
        N = 2 * info["classes"] - info["palindromes"]
        assert info["rounds"] <= 3 * (math.ceil(math.log2(N)) + 1) if N > 1 else info["rounds"] == 0
    else:
        assert not any(info.values())
    check_properties(b, k, got, min_count)
    return got


def run(orc, reads, k, **thresholds_):
    b = loaded(naive_rle(orc, reads))
    want = canonical_unitigs_of_texts(reads, k, **thresholds_)
    got = check_canonical(b, k, want, **thresholds_)
    return want, dict(zip(NAMES, got)), b


# ---- 1. the definitions, case by case: the expectations written out, and the oracle held to them ----

def test_a_palindromic_node_mid_path(orc):
    # GGAC GACG ACGT CGTC GTCC: classes {GGAC, GTCC}, {GACG, CGTC}, {ACGT}; the palindrome ACGT has no links and cuts the path
    want, got, b = run(orc, ["GGACGTCC"], 4)
    assert want["seqs"] == ["ACGT", "CGTCC"] and got["offsets"].tolist() == [0, 4, 9] and got["count_sums"].tolist() == [1, 4] and not got["flags"].any()
    assert got["symbols"].tolist() == [1, 2, 3, 5, 2, 3, 5, 2, 2]
    # ACGT: <- G (GACG), -> C (CGTC); CGTCC: <- A (ACGT), nothing after GTCC (its mirror GGAC has no predecessor)
    assert got["ends"].tolist() == [1 << 2 | 16 << 1, 1 << 0]
    info = b.canonical_unitig_info()
    assert {x: info[x] for x in INFO} == {"classes": 3, "edge_classes": 2, "links": 1, "unitigs": 2, "symbols": 9, "circular": 0, "longest": 2, "palindromes": 1,
                                          "cut_links": 2}


def test_a_hairpin_edge(orc):
    # AACGT -> ACGTT along the palindromic 6-mer AACGTT: ACGTT = rc(AACGT), one class, and the edge is no link
    want, got, b = run(orc, ["AACGTT"], 5)
    assert want["seqs"] == ["AACGT"] and got["count_sums"].tolist() == [2] and got["flags"].tolist() == [0]
    assert got["ends"].tolist() == [16 << 3]  # the real adjacency stays: -> T
    info = b.canonical_unitig_info()
    assert (info["classes"], info["edge_classes"], info["links"], info["unitigs"], info["palindromes"], info["cut_links"]) == (1, 1, 0, 1, 0, 1)


def test_an_edge_by_count_that_lacks_an_end(orc):
    # CATG, k = 2, m = 2: cc(CA) = cc(TG) = 2, cc(AT) = 1 -- AT is a palindrome and counts once -- though cc(CAT) = cc(ATG) = 2
    want, got, b = run(orc, ["CATG"], 2, min_count=2)
    assert want["seqs"] == ["CA"] and got["count_sums"].tolist() == [2] and got["ends"].tolist() == [0]
    assert b.canonical_unitig_info()["edge_classes"] == 0
    want, got, _ = run(orc, ["CATG"], 2)  # at m = 1 AT is a node: CA -> AT -> TG, cut at the palindrome
    assert want["seqs"] == ["AT", "CA"] and got["ends"].tolist() == [1 << 1 | 16 << 2, 16 << 3]


def test_single_reads(orc):
    # a read of exactly k symbols; its canonical word is its reverse complement's here, so what is emitted is not what was loaded
    want, got, _ = run(orc, ["TTACG"], 5)
    assert want["seqs"] == ["CGTAA"] and got["ends"].tolist() == [0] and got["flags"].tolist() == [0] and got["count_sums"].tolist() == [1]
    assert got["offsets"].tolist() == [0, 5] and got["symbols"].tolist() == [2, 3, 5, 1, 1]
    want, got, _ = run(orc, ["ACGTA"], 5)
    assert want["seqs"] == ["ACGTA"]
    # a read on one strand only, longer than k: the emitted orientation is the reverse complement of what was loaded
    want, got, _ = run(orc, ["TTTGGCATC"], 5)
    assert want["seqs"] == ["GATGCCAAA"] and got["count_sums"].tolist() == [5] and got["ends"].tolist() == [0]
    # a branch: TGGCAT -> GGCATC and GGCATG
    want, got, _ = run(orc, ["TGGCATCAAAAAG", "TGGCATG"], 5)
    assert sorted(want["seqs"]) == want["seqs"] and len(want["seqs"]) == 3 and want["info"]["classes"] == 10
    assert "ATGCCA" in want["seqs"]  # rc(TGGCAT): the stem, entered from both branches
    assert got["ends"][want["seqs"].index("ATGCCA")] == (1 << 1 | 1 << 2)  # <- C (CATGC) and G (GATGC); nothing follows
    # the self-loop: A^5 with A^6, and its mirror T^5; one circular unitig of one node
    want, got, b = run(orc, ["AAAAAAAA"], 5)
    assert want["seqs"] == ["AAAAA"] and got["ends"].tolist() == [0x11] and got["flags"].tolist() == [1] and got["count_sums"].tolist() == [4]
    info = b.canonical_unitig_info()
    assert {x: info[x] for x in INFO} == {"classes": 1, "edge_classes": 1, "links": 1, "unitigs": 1, "symbols": 5, "circular": 1, "longest": 1, "palindromes": 0,
                                          "cut_links": 0} and info["rounds"] == 0


def test_a_path_seen_once_per_strand_survives_min_count_2(orc):
    """what the call is for: no k-mer and no edge occurs twice on either strand, every class does"""
    path = "ACGGTCATTGACAGCT"
    reads = [path, rc(path)]
    b = loaded(naive_rle(orc, reads))
    for k in (5, 6):
        assert max(windows(reads, k).values()) == 1
        assert [len(a) for a in b.enumerate_unitigs(k, min_count=2)] == [0, 1, 0, 0, 0]  # the strand-specific call: nothing
        want = canonical_unitigs_of_texts(reads, k, 2)
        got = check_canonical(b, k, want, 2)
        assert want["seqs"] == [min(path, rc(path))] and got[2].tolist() == [2 * (len(path) - k + 1)]
        assert unitigs_of_texts(reads, k, 2)["seqs"] == []


# ---- 2. ragged sets at every k ----

@pytest.mark.parametrize("flipped", [False, True])
@pytest.mark.parametrize("seed", [0, 1, 2, 5, 11])
def test_ragged_sets_at_every_k(orc, seed, flipped):
    reads = ragged_set(seed)
    if seed == 0:
        reads = reads + ["GGACGTCCTAGCATGCTAGG", "GGACGTCCTAGCATGCTAGG"]  # palindromic nodes at every even k up to 8, twice
    if flipped:
        reads = flip_every_second(reads)
    b = loaded(naive_rle(orc, reads))
    longer = palindromes = 0
    for k in KS:
        for min_count, min_edge in ((1, 0), (2, 0), (2, 3)):
            want = canonical_unitigs_of_texts(reads, k, min_count, min_edge)
            check_canonical(b, k, want, min_count, min_edge)
            longer += sum(1 for a, z in zip(want["first"], want["last"]) if a != z)
            palindromes += want["info"]["palindromes"] if k % 2 == 0 else 0
            assert k % 2 == 0 or want["info"]["palindromes"] == 0
    assert longer > 20  # (the sets do yield unitigs of more than one node)
    assert palindromes > 0


def test_strand_symmetry(orc):
    """the index of a read set and the index of its reverse complements give byte-identical outputs"""
    for seed in (1, 5):
        reads = ragged_set(seed)
        a, z = loaded(naive_rle(orc, reads)), loaded(naive_rle(orc, [rc(r) for r in reads]))
        for k in (2, 4, 5, 16, 31):
            for min_count, min_edge in ((1, 0), (2, 3)):
                one = a.enumerate_canonical_unitigs(k, min_count=min_count, min_edge=min_edge or None)
                other = z.enumerate_canonical_unitigs(k, min_count=min_count, min_edge=min_edge or None)
                assert all(x.tobytes() == y.tobytes() for x, y in zip(one, other)), (seed, k, min_count)
                ia, iz = a.canonical_unitig_info(), z.canonical_unitig_info()
                assert {x: ia[x] for x in INFO} == {x: iz[x] for x in INFO}


# ---- 3. rounds and cycles ----

def _genome(n, seed=7):
    return "".join("ACGT"[x] for x in np.random.default_rng(seed).integers(0, 4, size=n))


def _built(reads):
    b = msbwt.RleBWT(device=0)
    b.load_reads(reads, ascii=True)
    return b


def test_one_long_chain_from_both_strands():
    k, g = 15, _genome(20000)
    reads = flip_every_second([g[s:s + 100] for s in range(0, len(g) - 99, 50)])
    want = canonical_unitigs_of_texts(reads, k)
    assert want["info"]["unitigs"] == 1 and want["info"]["longest"] == 19986 == want["info"]["classes"] and want["info"]["circular"] == 0
    b = _built(reads)
    check_canonical(b, k, want)
    info = b.canonical_unitig_info()
    print("k = %d: %d classes in one unitig, %d rounds" % (k, info["classes"], info["rounds"]))
    assert 14 <= info["rounds"] <= math.ceil(math.log2(2 * 19986)) + 2
    assert want["seqs"][0] in (g, rc(g)) and want["seqs"][0][:k] == min(g[:k], rc(g)[:k])


@pytest.mark.parametrize("strands", ["one", "both"])
def test_one_circle(strands):
    k, g = 15, _genome(600, 11)
    text = g + g[:200]
    reads = [text[s:s + 100] for s in range(0, len(text) - 99, 50)]
    if strands == "both":
        reads = flip_every_second(reads)
    want = canonical_unitigs_of_texts(reads, k)
    assert want["info"]["unitigs"] == 1 and want["info"]["longest"] == 600 == want["info"]["classes"] and want["info"]["circular"] == 1
    b = _built(reads)
    symbols, offsets, sums, ends, flags = check_canonical(b, k, want)
    every = windows([text, rc(text)], k)
    first, last = want["seqs"][0][:k], want["seqs"][0][-k:]
    assert first == min(every) and flags.tolist() == [1]  # opened at the smallest word of both strands
    assert ends.tolist() == [1 << "ACGT".index(last[0]) | 16 << "ACGT".index(first[-1])]  # the closing edge last -> first
    info = b.canonical_unitig_info()
    assert info["links"] == 600 and info["rounds"] >= 10


def test_a_cycle_with_a_tail_into_it(orc):
    reads = ["TTCCACGTTGCAGACGTT"]
    for k in (5, 6):
        want, got, _ = run(orc, reads, k)
        assert not got["flags"].any() and want["info"]["circular"] == 0
    want, got, _ = run(orc, flip_every_second(reads + reads), 5, min_count=2)
    assert want["info"]["unitigs"] >= 2


# ---- 4. reads with errors, from both strands ----

_sets = {}


def both_strands(name):
    """(texts, RLE bytes) of read_set(name) with every second read reverse-complemented, built once by the CPU builder"""
    if name not in _sets:
        import synth
        (flat, offsets), _ = read_set(name)
        length = int(offsets[1])
        matrix = flat.reshape(-1, length).copy()
        flip = np.array([0, 5, 3, 2, 4, 1], dtype=np.uint8)  # $ A C G N T -> $ T G C N A
        matrix[1::2] = flip[matrix[1::2, ::-1]]
        rle = synth.rle_encode(synth.build_msbwt_symbols(matrix, 4))
        rle.setflags(write=False)
        texts = texts_of_codes(matrix.reshape(-1), offsets)
        assert texts[1] == rc(texts_of_codes(flat[length:2 * length], offsets[:2])[0]) if "N" not in texts[1] else True
        _sets[name] = (texts, rle, {})
    return _sets[name]


def both_strands_unitigs(name, k, min_count=1, min_edge=0):
    texts, _, cache = both_strands(name)
    if ("windows", k) not in cache:
        cache["windows", k] = (windows(texts, k), windows(texts, k + 1))
    if (k, min_count, min_edge) not in cache:
        cache[k, min_count, min_edge] = canonical_unitigs_of_counters(*cache["windows", k], k, min_count, min_edge)
    return cache[k, min_count, min_edge]


@pytest.mark.parametrize("k", [15, 31])
def test_read_sets_with_errors(k):
    name = "plain_100"
    _, rle, _ = both_strands(name)
    b = loaded(rle)
    for min_count, min_edge in ((1, 0), (2, 0), (2, 3), (10 ** 9, 0)):
        want = both_strands_unitigs(name, k, min_count, min_edge)
        got = check_canonical(b, k, want, min_count, min_edge)
        if min_count == 10 ** 9:
            assert len(got[2]) == 0 and len(got[0]) == 0 and got[1].tolist() == [0]
        print("%s, k = %d, (%d, %d): %s" % (name, k, min_count, min_edge, b.canonical_unitig_info()))
    assert both_strands_unitigs(name, k)["info"]["longest"] > 50 and both_strands_unitigs(name, k)["info"]["unitigs"] > 1000  # (the errors branch the graph)
    for bad in ((3, 2),):
        with pytest.raises(MsbwtError) as err:
            b.enumerate_canonical_unitigs(k, min_count=bad[0], min_edge=bad[1])
        assert err.value.code == _lib.ERR_INVALID_ARG and "min_edge" in str(err.value)


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("k", [17, 21, 31])  # 5, 6 and 8 radix passes: the sorted nodes end in the second pair of buffers (17) and in the first
def test_sort_grid_cap_gives_the_same_unitigs(monkeypatch, k, grid):
    """MSBWT_SORT_GRID caps the grids of the order step's passes (csrc/radix_sort.hip): a workgroup takes several tiles of 4096 slots"""
    name = "plain_100"
    _, rle, _ = both_strands(name)
    want = both_strands_unitigs(name, k)
    slots = 2 * want["info"]["classes"] - want["info"]["palindromes"]
    assert slots > 4 * 4096  # more tiles than workgroups
    b = loaded(rle)
    monkeypatch.delenv("MSBWT_SORT_GRID", raising=False)
    check_canonical(b, k, want)
    unset = b.canonical_unitig_info()
    monkeypatch.setenv("MSBWT_SORT_GRID", str(grid))
    check_canonical(b, k, want)
    assert b.canonical_unitig_info() == unset


# ---- 5. chunks of the walk, and every index form ----

def test_a_frontier_at_its_minimum_gives_the_same_bytes():
    name, k = "plain_100", 31
    _, rle, _ = both_strands(name)
    b = loaded(rle)
    auto = check_canonical(b, k, both_strands_unitigs(name, k, 2), 2)
    b.set_spectrum_frontier(_lib.SPECTRUM_MIN_FRONTIER)
    first = b.enumerate_canonical_unitigs(k, min_count=2)
    assert b.spectrum_info()["chunks"] >= 100
    second = b.enumerate_canonical_unitigs(k, min_count=2)
    for x, y, z in zip(first, second, auto):
        assert np.array_equal(x, z) and np.array_equal(y, z)
    b.set_spectrum_frontier(0)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_every_index_form_gives_the_same_answer(form):
    name = "plain_100"
    _, rle, _ = both_strands(name)
    b = loaded(rle, **FORMS[form])
    assert b.get_block_format() == FORMS[form].get("block_format", "planes")
    for k in (15, 31):
        check_canonical(b, k, both_strands_unitigs(name, k))
        check_canonical(b, k, both_strands_unitigs(name, k, 2, 3), 2, 3)


# ---- 6. capacity, NULL buffers, scratch, guards ----

def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_capacity_and_null_buffers():
    import torch
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    name, k, min_count = "plain_100", 15, 2
    _, rle, _ = both_strands(name)
    want = both_strands_unitigs(name, k, min_count)
    n, U, S = want["info"]["classes"], want["info"]["unitigs"], want["info"]["symbols"]
    assert U > 50 and n > 10000
    b = loaded(rle)
    lib, got_u, got_s = _lib.lib(), C.c_uint64(0), C.c_uint64(0)
    total, free = b.get_total_size(), torch.cuda.mem_get_info(0)[0]
    plan = lambda *a: msbwt.canonical_unitigs_plan(total, free, *a)
    sizes = {"symbols": S, "offsets": U + 1, "count_sums": U, "ends": U, "flags": U}
    staged = {"symbols": 8 * ((S + 7) // 8), "offsets": 0, "count_sums": 8 * U, "ends": 8 * ((U + 7) // 8), "flags": 8 * ((U + 7) // 8)}

    def host(cap_u, cap_s, skip=()):
        bufs = {x: np.full(sizes[x] + 3, 7, dtype=want[x].dtype) for x in NAMES}
        args = [_ptr(bufs[x]) if x not in skip else None for x in NAMES]
        return lib.msbwt_rle_enumerate_canonical_unitigs(b._h, k, min_count, 0, *args, cap_u, cap_s, C.byref(got_u), C.byref(got_s)), bufs

    # the two-call pattern; a capacity too small (each of the two) writes nothing and names U and S
    rc_, bufs = host(0, 0)
    assert rc_ == 0 and (got_u.value, got_s.value) == (U, S) and all((a == 7).all() for a in bufs.values())
    before = b.device_bytes()  # (the packed search keeps its ordering scratch on the handle, as for the canonical dump)
    assert b.spectrum_scratch_bytes() == plan(n) == plan(n, 0, 0)
    for cap_u, cap_s in ((U - 1, S), (U, S - 1), (1, 1), (0, S), (U, 0)):
        got_u.value = got_s.value = 0
        rc_, bufs = host(cap_u, cap_s)
        message = lib.msbwt_rle_last_error(b._h)
        assert rc_ == _lib.ERR_INVALID_ARG and (got_u.value, got_s.value) == (U, S) and str(U).encode() in message and str(S).encode() in message
        assert all((a == 7).all() for a in bufs.values())
    # every output NULL in turn, and all at once; capacities above need
    for skip in ((),) + tuple((x,) for x in NAMES) + (NAMES,):
        rc_, bufs = host(U + 2, S + 2, skip)
        assert rc_ == 0 and (got_u.value, got_s.value) == (U, S), skip
        for x in NAMES:
            assert (bufs[x][sizes[x]:] == 7).all() and (np.array_equal(bufs[x][:sizes[x]], want[x]) if x not in skip else (bufs[x] == 7).all()), (skip, x)
        assert b.spectrum_scratch_bytes() == plan(n, U, S) - sum(staged[x] for x in skip), skip
    rc_, _ = host(U, 0, ("symbols",))  # no symbols wanted: their capacity does not matter
    assert rc_ == 0
    # the device form: the same, into buffers of the caller's; the byte arrays at odd addresses
    assert b.enumerate_canonical_unitigs_device(k, None, None, None, None, None, 0, 0, min_count=min_count, stream=stream) == (U, S)
    assert b.spectrum_scratch_bytes() == plan(n)
    words = ("offsets", "count_sums")
    for skip in ((),) + tuple((x,) for x in NAMES):
        bufs = {x: torch.full((sizes[x] + 9,), 7, dtype=torch.int64 if x in words else torch.uint8, device=dev) for x in NAMES}
        ptrs = [None if x in skip else bufs[x].data_ptr() + (0 if x in words else 1) for x in NAMES]
        for cap_u, cap_s in ((U - 1, S), (U, S - 1)):
            if cap_s < S and "symbols" in skip:
                continue
            with pytest.raises(MsbwtError) as err:
                b.enumerate_canonical_unitigs_device(k, *ptrs, cap_u, cap_s, min_count=min_count, stream=stream)
            assert err.value.code == _lib.ERR_INVALID_ARG and (err.value.n, err.value.symbols) == (U, S) and str(U) in str(err.value) and str(S) in str(err.value)
            assert all(bool((bufs[x] == 7).all()) for x in NAMES)
        assert b.enumerate_canonical_unitigs_device(k, *ptrs, U + 1, S + 1, min_count=min_count, stream=stream) == (U, S)
        b.device_status(stream)
        assert b.spectrum_scratch_bytes() == plan(n, U, S) - sum(staged.values())  # nothing staged
        for x in NAMES:
            got, lead = bufs[x].cpu().numpy(), 0 if x in words else 1
            if x in skip:
                assert (got == 7).all(), (skip, x)
            else:
                assert (got[:lead] == 7).all() and (got[lead + sizes[x]:] == 7).all() and np.array_equal(got[lead:lead + sizes[x]].astype(want[x].dtype), want[x]), (skip, x)
    assert b.device_bytes() == before
    # the guards behind "nothing loaded": k = 32 is refused, as is a min_edge below the node threshold
    for bad_k in (0, 32, 33, 1000):
        assert lib.msbwt_rle_enumerate_canonical_unitigs(b._h, bad_k, 1, 0, None, None, None, None, None, 0, 0, C.byref(got_u), C.byref(got_s)) == _lib.ERR_INVALID_ARG
        assert lib.msbwt_rle_enumerate_canonical_unitigs_device(b._h, bad_k, 1, 0, None, None, None, None, None, 0, 0, C.byref(got_u), C.byref(got_s),
                                                                None) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_enumerate_canonical_unitigs(b._h, k, 3, 2, None, None, None, None, None, 0, 0, C.byref(got_u), C.byref(got_s)) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_enumerate_canonical_unitigs(b._h, k, 1, 0, None, None, None, None, None, 0, 0, None, C.byref(got_s)) == _lib.ERR_INVALID_ARG
    assert lib.msbwt_rle_enumerate_canonical_unitigs(b._h, k, 0, 0, None, None, None, None, None, 0, 0, C.byref(got_u), None) == 0  # min_count 0 is 1; the total is optional
    with pytest.raises(MsbwtError) as err:
        b.enumerate_canonical_unitigs(32)
    assert err.value.code == _lib.ERR_INVALID_ARG and "31" in str(err.value)
    # an empty index
    from test_gpu_merge_many import EMPTY
    empty = loaded(EMPTY)
    for kk in (1, 21, 31):
        got = empty.enumerate_canonical_unitigs(kk)
        assert [len(a) for a in got] == [0, 1, 0, 0, 0] and got[1].tolist() == [0] and not any(empty.canonical_unitig_info().values())
    assert empty.enumerate_canonical_unitigs(5, text=True)[0] == []


# ---- 7. the other calls of the family are unchanged by this one ----

def test_the_other_calls_after_a_canonical_unitig_call():
    name, k = "plain_100", 15
    _, rle, _ = both_strands(name)
    b = loaded(rle)
    for min_count, min_edge in ((1, 0), (2, 3)):
        calls = (lambda: b.enumerate_unitigs(k, min_count=min_count, min_edge=min_edge or None),
                 lambda: b.enumerate_kmer_graph(k, min_count=min_count, min_edge=min_edge or None),
                 lambda: b.enumerate_canonical_kmers(k, min_count=min_count, sorted=True, strands=True))
        before = [call() for call in calls]
        info = b.unitig_info()
        seqs = b.enumerate_canonical_unitigs(k, min_count=min_count, min_edge=min_edge or None, text=True)[0]
        assert seqs == both_strands_unitigs(name, k, min_count, min_edge)["seqs"]
        assert b.unitig_info() == info  # (the plain call's report is its own)
        for call, was in zip(calls, before):
            assert all(np.array_equal(x, y) for x, y in zip(call(), was))
    b.device_status()
