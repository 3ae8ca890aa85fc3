"""A numpy oracle for the k-mer graph, the unitigs and the canonical unitigs of reads given as arrays of symbol codes, k <= 31: what
test_gpu_kmer_graph.graph_of_texts, test_gpu_unitigs.unitigs_of_texts and test_gpu_canonical_unitigs.canonical_unitigs_of_counters
compute over strings, for sets of millions of nodes.  tests/test_graph_oracle.py holds it to those three, column by column, on the CPU.

Everything starts from test_scaled_copies.census_of_codes at k and at k + 1 (a (k+1)-mer fits one word).  A word is looked up with
searchsorted, a node's place in its unitig comes from pointer doubling over the links, a cycle's smallest member from doubling with a
running minimum.  Nothing here calls the library."""
import numpy as np

from test_gpu_kmer_graph import thresholds
from test_scaled_copies import census_of_codes

U64 = np.uint64
CODE_OF = {"$": 0, "A": 1, "C": 2, "G": 3, "N": 4, "T": 5}
SYMBOL = np.array([1, 2, 3, 5], dtype=np.uint8)  # 2-bit value -> symbol code
FLIP = np.array([0, 5, 3, 2, 4, 1], dtype=np.uint8)  # $ A C G N T -> $ T G C N A
NAMES = ("symbols", "offsets", "count_sums", "ends", "flags")
POP = np.array([bin(x).count("1") for x in range(16)], dtype=np.int64)
BIT = np.array([-1, 0, 1, -1, 2, -1, -1, -1, 3], dtype=np.int64)  # a nibble with one bit set -> which


def codes_of_texts(reads):
    return [np.array([CODE_OF[c] for c in r], dtype=np.uint8) for r in reads]


def reverse_complement(read):
    return FLIP[read[::-1]]


def flip_every_second(reads):
    return [reverse_complement(r) if i % 2 else r for i, r in enumerate(reads)]


def rc_words(words, k):
    """the words of the reverse complements of k-mers given as 2-bit words"""
    w = ~np.asarray(words, dtype=U64)
    for shift, mask in ((2, 0x3333333333333333), (4, 0x0F0F0F0F0F0F0F0F), (8, 0x00FF00FF00FF00FF), (16, 0x0000FFFF0000FFFF)):
        w = ((w >> U64(shift)) & U64(mask)) | ((w & U64(mask)) << U64(shift))
    w = (w >> U64(32)) | (w << U64(32))
    return w >> U64(64 - 2 * k)


def slots_of(words, sorted_words):
    """(slot, found) of every word in a sorted array of distinct words"""
    if len(sorted_words) == 0:
        return np.zeros(len(words), dtype=np.int64), np.zeros(len(words), dtype=bool)
    at = np.minimum(np.searchsorted(sorted_words, words), len(sorted_words) - 1)
    return at, sorted_words[at] == words


def counts_of(words, sorted_words, counts):
    at, found = slots_of(words, sorted_words)
    return np.where(found, counts[at], U64(0)).astype(U64) if len(sorted_words) else np.zeros(len(words), dtype=U64)


def census(reads, k):
    """the censuses at k and at k + 1: (words, counts, words1, counts1)"""
    assert 1 <= k <= 31
    return census_of_codes(reads, k) + census_of_codes(reads, k + 1)


def edge_bytes(words, solid, k):
    """one byte per node: bit j = the (k+1)-mer j.q is in `solid`, bit 4 + j = q.j is; both ends of every solid (k+1)-mer are nodes"""
    mask = U64((1 << (2 * k)) - 1)
    edges = np.zeros(len(words), dtype=np.int64)
    for node, sym, shift in ((solid & mask, solid >> U64(2 * k), 0), (solid >> U64(2), solid & U64(3), 4)):
        at, found = slots_of(node, words)
        assert found.all()
        # a (node, symbol) pair occurs once: the weights add up to the OR of the bits, exactly
        edges += np.bincount(at, weights=(1 << (sym.astype(np.int64) + shift)).astype(np.float64), minlength=len(words)).astype(np.int64)
    return edges.astype(np.uint8)


def graph_of_census(cen, k, min_count=1, min_edge=0):
    """(words, counts, edge bytes, number of edges), as enumerate_kmer_graph and kmer_graph_degrees report them"""
    words, counts, words1, counts1 = cen
    m, me = thresholds(min_count, min_edge)
    assert me >= m  # (the library refuses the rest: then a (k+1)-mer that counts has both its ends)
    keep = counts >= U64(m)
    solid = words1[counts1 >= U64(me)]
    return words[keep], counts[keep], edge_bytes(words[keep], solid, k), len(solid)


def graph_of_codes(reads, k, min_count=1, min_edge=0):
    return graph_of_census(census(reads, k), k, min_count, min_edge)


# ---- the links and the walk along them ----

def links_of(words, edges, k, cut=None):
    """up[q] = the slot of the p whose only out-edge is q's only in-edge, -1 where there is none; `cut`(p words, q words) marks the
    links that do not count.  -> (up, the number cut)"""
    n = len(words)
    up = np.full(n, -1, dtype=np.int64)
    q = np.flatnonzero(POP[edges & 15] == 1)
    if q.size == 0:
        return up, 0
    p_words = (BIT[edges[q] & 15].astype(U64) << U64(2 * (k - 1))) | (words[q] >> U64(2))
    p, found = slots_of(p_words, words)
    assert found.all()
    one = POP[edges[p] >> 4] == 1
    q, p = q[one], p[one]
    n_cut = 0
    if cut is not None:
        gone = cut(words[p], words[q])
        n_cut = int(gone.sum())
        q, p = q[~gone], p[~gone]
    up[q] = p
    assert np.unique(p).size == p.size  # no node has two links down
    return up, n_cut


def _double(up, members, head, dist):
    """pointer doubling over `up` for the nodes `members`: head and dist of those that reach a node without a link; -> the others"""
    ptr = head  # (in place: head[i] is i's pointer until it is its head)
    act = members[up[members] >= 0]
    ptr[members] = np.where(up[members] >= 0, up[members], members)
    dist[members] = (up[members] >= 0).astype(np.int64)
    for _ in range(int(len(up)).bit_length() + 1):
        act = act[up[ptr[act]] >= 0]
        if act.size == 0:
            break
        p = ptr[act]
        dist[act] = dist[act] + dist[p]
        ptr[act] = ptr[p]
    return act[up[ptr[act]] >= 0]


def walk(up):
    """(head, dist, circular, up with every cycle opened): per node the slot of the first node of its path and its distance from it;
    what hangs on no head lies on cycles, each opened at its smallest member (circular[that slot] = True)."""
    n = len(up)
    head, dist = np.arange(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    circular = np.zeros(n, dtype=bool)
    on_cycles = _double(up, np.arange(n, dtype=np.int64), head, dist)
    if on_cycles.size:
        least, ptr = np.arange(n, dtype=np.int64), up.copy()
        for _ in range(int(on_cycles.size).bit_length() + 1):
            p = ptr[on_cycles]
            least[on_cycles] = np.minimum(least[on_cycles], least[p])
            ptr[on_cycles] = ptr[p]
        opened = on_cycles[least[on_cycles] == on_cycles]
        circular[opened] = True
        up = up.copy()
        up[opened] = -1
        left = _double(up, on_cycles, head, dist)
        assert left.size == 0
    return head, dist, circular, up


def emit(words, counts, edges, k, head, dist, circular, kept_heads):
    """the five columns of the unitigs whose first nodes are the slots `kept_heads` (ascending), and the slots of their last nodes"""
    n, U = len(words), len(kept_heads)
    out = {"symbols": np.zeros(0, dtype=np.uint8), "offsets": np.zeros(1, dtype=U64), "count_sums": np.zeros(0, dtype=U64),
           "ends": np.zeros(0, dtype=np.uint8), "flags": np.zeros(0, dtype=np.uint8), "first": np.zeros(0, dtype=U64), "last": np.zeros(0, dtype=U64)}
    if U == 0:
        return out, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    rank = np.full(n, -1, dtype=np.int64)
    rank[kept_heads] = np.arange(U)
    members = np.flatnonzero(rank[head] >= 0)
    u = rank[head[members]]
    lengths = np.bincount(u, minlength=U)
    start = np.concatenate([[0], np.cumsum(lengths)])
    place = start[u] + dist[members]
    order = np.full(len(members), -1, dtype=np.int64)
    order[place] = members
    assert (order >= 0).all() and (dist[members] < lengths[u]).all()  # every place of every unitig taken once
    offsets = start + np.arange(U + 1) * (k - 1)
    symbols = np.zeros(int(offsets[-1]), dtype=np.uint8)
    symbols[offsets[u] + (k - 1) + dist[members]] = SYMBOL[(words[members] & U64(3)).astype(np.int64)]
    first = words[kept_heads]
    for j in range(k - 1):
        symbols[offsets[:-1] + j] = SYMBOL[((first >> U64(2 * (k - 1 - j))) & U64(3)).astype(np.int64)]
    last = order[start[1:] - 1]
    out.update(symbols=symbols, offsets=offsets.astype(U64), count_sums=np.add.reduceat(counts[order], start[:-1]).astype(U64),
               ends=((edges[kept_heads] & 15) | (edges[last] & 0xF0)).astype(np.uint8), flags=circular[kept_heads].astype(np.uint8),
               first=first, last=words[last])
    return out, lengths, last


def unitigs_of_census(cen, k, min_count=1, min_edge=0):
    """test_gpu_unitigs.unitigs_of_texts without "seqs"; "first" and "last" are words; "branching" = the nodes with more than one
    predecessor or successor"""
    words, counts, edges, n_edges = graph_of_census(cen, k, min_count, min_edge)
    up, _ = links_of(words, edges, k)
    head, dist, circular, opened = walk(up)
    heads = np.flatnonzero(opened < 0)
    out, lengths, _ = emit(words, counts, edges, k, head, dist, circular, heads)
    out["info"] = {"nodes": len(words), "edges": n_edges, "links": int((up >= 0).sum()), "unitigs": len(heads), "symbols": len(out["symbols"]),
                   "circular": int(circular.sum()), "longest": int(lengths.max()) if len(heads) else 0}
    out["branching"] = int(((POP[edges & 15] > 1) | (POP[edges >> 4] > 1)).sum())
    assert out["info"]["symbols"] == len(words) + len(heads) * (k - 1)
    return out


def unitigs_of_codes(reads, k, min_count=1, min_edge=0):
    return unitigs_of_census(census(reads, k), k, min_count, min_edge)


# ---- the strand-merged graph ----

def class_census(words, counts, k):
    """(words, class counts) of the k-mers of a census and their reverse complements: cc(x) = count(x) + count(rc(x)), a palindrome once"""
    mirror = rc_words(words, k)
    both = np.concatenate([words, mirror])
    order = np.argsort(both, kind="stable")
    both, n = both[order], np.concatenate([counts, np.where(mirror == words, U64(0), counts)])[order]
    if both.size == 0:
        return both, n
    starts = np.flatnonzero(np.concatenate([[True], both[1:] != both[:-1]]))
    return both[starts], np.add.reduceat(n, starts).astype(U64)


def canonical_census(cen, k):
    """the class censuses at k and at k + 1 of census(reads, k)"""
    return class_census(cen[0], cen[1], k) + class_census(cen[2], cen[3], k + 1)


def canonical_graph_of_census(cen, k, min_count=1, min_edge=0, classes=None):
    """(words, class counts, edge bytes, number of edge classes) of the strand-merged graph: both members of every class that counts
    are nodes; an edge needs the class count of its (k+1)-mer and both its ends.  `classes`: canonical_census(cen, k), if at hand."""
    m, me = thresholds(min_count, min_edge)
    words, cc, words1, cc1 = classes if classes is not None else canonical_census(cen, k)
    keep = cc >= U64(m)
    words, cc = words[keep], cc[keep]
    solid = words1[cc1 >= U64(me)]
    solid = solid[slots_of(solid >> U64(2), words)[1] & slots_of(solid & U64((1 << (2 * k)) - 1), words)[1]]
    return words, cc, edge_bytes(words, solid, k), int((solid <= rc_words(solid, k + 1)).sum())


def canonical_unitigs_of_census(cen, k, min_count=1, min_edge=0, classes=None):
    """test_gpu_canonical_unitigs.canonical_unitigs_of_counters without "seqs"; "first" and "last" are words"""
    words, cc, edges, edge_classes = canonical_graph_of_census(cen, k, min_count, min_edge, classes)
    mirror = rc_words(words, k)
    palindromes = int((mirror == words).sum())

    def cut(p, q):  # a palindromic end, or a link along a palindromic (k+1)-mer
        e = (p << U64(2)) | (q & U64(3))
        return (rc_words(q, k) == q) | (rc_words(p, k) == p) | (rc_words(e, k + 1) == e)

    up, n_cut = links_of(words, edges, k, cut)
    head, dist, circular, opened = walk(up)
    heads = np.flatnonzero(opened < 0)
    # of U and rc(U) the one whose first word is smaller: rc(the last node of U) lies in rc(U)
    _, lengths, last = emit(words, cc, edges, k, head, dist, circular, heads)
    mirror_slot, found = slots_of(mirror[last], words)
    assert found.all()
    mirror_head = head[mirror_slot]
    own = mirror_head == heads
    assert np.array_equal(own, (lengths == 1) & (mirror[heads] == words[heads]))  # its own mirror exactly when it is a palindromic node
    kept = heads[heads <= mirror_head]
    out, lengths, _ = emit(words, cc, edges, k, head, dist, circular, kept)
    classes = (len(words) + palindromes) // 2
    n_circular = int(circular[kept].sum())
    out["info"] = {"classes": classes, "edge_classes": edge_classes, "links": classes + n_circular - len(kept), "unitigs": len(kept),
                   "symbols": len(out["symbols"]), "circular": n_circular, "longest": int(lengths.max()) if len(kept) else 0,
                   "palindromes": palindromes, "cut_links": n_cut}
    out["slots"] = len(words)  # 2 classes - palindromes: what the device ranks
    assert int(lengths.sum()) == classes and out["info"]["symbols"] == classes + len(kept) * (k - 1)
    return out


def canonical_unitigs_of_codes(reads, k, min_count=1, min_edge=0):
    return canonical_unitigs_of_census(census(reads, k), k, min_count, min_edge)


def scaled(want, c):
    """the oracle's unitigs of a set with every read c times: the count sums times c, the rest as it is"""
    out = dict(want)
    out["count_sums"] = want["count_sums"] * U64(c)
    return out
