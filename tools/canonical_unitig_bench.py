#!/usr/bin/env python3
"""Canonical unitigs on the read set of a synth.CONFIGS entry (default C4: 12.9 M reads of 150 bp with 0.5 % substitutions, 1.95e9
symbols at scale 1) with every second read reverse-complemented -- the index tools/canonical_bench.py uses --, built and loaded by
load_reads.  For k = 21 and 31 and min_count = 1 and 2, after a warm-up `--repeats` rounds with the calls alternating within a round
(median and spread, wall clock around calls that end in a synchronise):
  canonical  (i) enumerate_canonical_unitigs_device: symbols, offsets, count sums, ends and flags into device buffers
  count      (i) the same call with both capacities 0: U and S only
  plain      (ii) enumerate_unitigs_device on the same index, the strand-specific call: about half of its unitigs are mirrors
  host       (iii) the route a caller had before, timed once: (ii) to host arrays, and the mirrors paired there (first word of one =
             reverse complement of the last word of the other, by binary search in the ascending first words)
Beside the times: classes n, nodes N, U, S, the longest unitig, rounds, palindromic nodes, scratch, and the unitigs of (i) beside half
the unitigs of (ii) -- at min_count = 2 the difference is the fragmentation that thresholds on strand counts cause.
At min_count = 2 (`--check-min-count`) U, S and a fixed sample of 65 536 unitigs are checked against a host restatement in numpy, from
the canonical dumps at k and at k + 1 (classes and edge classes), single-threaded: both members of every class sorted, the edge bytes
with the both-ends clause, links with the two cuts, pointer jumping, min-label opening of cycles, the choice by head slots, numbering,
emission.  A mismatch fails the tool.  One JSON line per (k, min_count) and a closing summary line; no threshold on the times.
A driver that wants each GPU step under its own time limit runs one (k, min_count) per process: --ks 21 --min-counts 2.
`--links` prints the link lines of tools/unitig_bench.py INSTEAD, for the canonical call: enumerate_canonical_unitig_graph_device beside
enumerate_canonical_unitigs_device in the same rounds, and the host route (the unitig call to host arrays, then the numpy join)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import rust_msbwt_amd as msbwt  # noqa: E402
from canonical_bench import COMPLEMENT  # noqa: E402
from kmer_graph_bench import spread, wall  # noqa: E402
from reads_build_bench import read_set  # noqa: E402
from unitig_bench import CODE, LOW, POP, finish_links, link_lines, rank_by_jumping  # noqa: E402

SAMPLE = 1 << 16
U64 = np.uint64
rc2 = msbwt.rle_bwt.reverse_complement_2bit


def slots_of(words, wanted):
    """(slot, present) of every wanted word in the sorted words"""
    at = np.minimum(np.searchsorted(words, wanted), len(words) - 1)
    return at, words[at] == wanted


def host_restatement(class_words, class_counts, edge_words, k):
    """the canonical unitigs from the classes (count >= m) and the edge classes (count >= me) -> (symbols, offsets, sums, ends, flags, N)"""
    mirror = rc2(class_words, k)
    second = mirror != class_words
    words, counts = np.concatenate([class_words, mirror[second]]), np.concatenate([class_counts, class_counts[second]])
    order = np.argsort(words, kind="stable")
    words, counts = words[order], counts[order]
    del order, mirror, second
    n = len(words)
    every = np.unique(np.concatenate([edge_words, rc2(edge_words, k + 1)]))  # the edges of D: both members of every edge class ..
    src, have_src = slots_of(words, every >> U64(2))
    dst, have_dst = slots_of(words, every & U64((1 << (2 * k)) - 1))
    both = have_src & have_dst  # .. whose ends are both nodes
    edges = np.zeros(n, dtype=np.uint8)
    for j in range(4):  # (a node has one edge per symbol and side: no slot twice in one assignment)
        out = both & ((every & U64(3)) == U64(j))
        edges[src[out]] |= np.uint8(16 << j)
        into = both & ((every >> U64(2 * k)) == U64(j))
        edges[dst[into]] |= np.uint8(1 << j)
    del every, src, dst, have_src, have_dst, both
    slots = np.arange(n, dtype=np.int64)
    own_mirror = rc2(words, k) == words
    one = np.flatnonzero(POP[edges & 15] == 1)
    before = (LOW[edges[one] & 15].astype(U64) << U64(2 * (k - 1))) | (words[one] >> U64(2))
    pred = np.searchsorted(words, before)
    linked = POP[edges[pred] >> 4] == 1
    linked &= ~own_mirror[one] & ~own_mirror[pred] & (rc2(words[pred], k) != words[one])  # the two cuts
    up = slots.copy()
    up[one[linked]] = pred[linked]
    circular = np.zeros(n, dtype=bool)
    circular[one[linked][pred[linked] == one[linked]]] = True  # self-loops
    head, dist, cyc, _ = rank_by_jumping(up, np.flatnonzero(up != slots))
    if len(cyc):
        label, ptr = slots.copy(), up.copy()
        for _ in range(max(int(np.ceil(np.log2(len(cyc)))), 1)):
            a = ptr[cyc]
            lower, far = np.minimum(label[cyc], label[a]), ptr[a]
            label[cyc], ptr[cyc] = lower, far
        opening = cyc[label[cyc] == cyc]
        up[opening] = opening
        circular[opening] = True
        h2, d2, left, _ = rank_by_jumping(up, cyc[label[cyc] != cyc])
        assert len(left) == 0
        head[cyc], dist[cyc] = h2[cyc], d2[cyc]
        head[opening], dist[opening] = opening, 0
    is_head = up == slots
    has_down = np.zeros(n, dtype=bool)
    has_down[up[~is_head]] = True
    tails = np.flatnonzero(~has_down)
    partner, present = slots_of(words, rc2(words[tails], k))
    assert present.all()
    kept_head = np.zeros(n, dtype=bool)
    kept_head[head[tails[head[tails] <= head[partner]]]] = True  # the choice
    number = np.cumsum(kept_head) - 1
    emit = kept_head[head]
    unitig = number[head]
    U = int(kept_head.sum())
    nodes = np.bincount(unitig[emit], minlength=U)
    offsets = np.zeros(U + 1, dtype=U64)
    offsets[1:] = np.cumsum(nodes + (k - 1))
    symbols = np.zeros(int(offsets[-1]), dtype=np.uint8)
    at = offsets[:-1].astype(np.int64)
    symbols[at[unitig[emit]] + (k - 1) + dist[emit]] = CODE[(words[emit] & U64(3)).astype(np.int64)]
    first = words[kept_head]
    for j in range(k - 1):
        symbols[at + j] = CODE[((first >> U64(2 * (k - 1 - j))) & U64(3)).astype(np.int64)]
    sums = np.bincount(unitig[emit], weights=counts[emit].astype(np.float64), minlength=U).astype(U64)  # (exact below 2^53)
    kept_tails = tails[kept_head[head[tails]]]
    ends = np.zeros(U, dtype=np.uint8)
    ends[unitig[kept_tails]] = (edges[head[kept_tails]] & 15) | (edges[kept_tails] & 0xF0)
    flags = np.zeros(U, dtype=np.uint8)
    flags[number[np.flatnonzero(circular & kept_head)]] = 1
    return symbols, offsets, sums, ends, flags, n


def word_at(symbols, starts, k):
    two = np.zeros(6, dtype=U64)
    two[[1, 2, 3, 5]] = [0, 1, 2, 3]
    w = np.zeros(len(starts), dtype=U64)
    for j in range(k):
        w = (w << U64(2)) | two[symbols[starts + j]]
    return w


def pair_mirrors(symbols, offsets, k):
    """unitigs of the strand-specific call whose mirror is among them: first word of one = rc(last word of the other)"""
    first = word_at(symbols, offsets[:-1].astype(np.int64), k)
    last = word_at(symbols, offsets[1:].astype(np.int64) - k, k)
    _, present = slots_of(first, rc2(last, k))
    return int(present.sum())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--links", action="store_true", help="the link lines in place of the others: enumerate_canonical_unitig_graph_device beside the unitig call")
    ap.add_argument("--config", default="c4")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--ks", default="21,31")
    ap.add_argument("--min-counts", default="1,2")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--check-min-count", type=int, default=2, help="the host restatement runs at this min_count (0: never)")
    ap.add_argument("--no-host-route", action="store_true", help="skip (iii)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("canonical_unitig_bench needs a GPU")
    if args.repeats < 5:
        sys.exit("a median of at least five calls")
    dev = torch.device("cuda:0")
    reads = np.array(read_set(args.config, args.scale))
    reads[1::2] = COMPLEMENT[reads[1::2, ::-1]]
    n_reads, length = reads.shape
    b = msbwt.RleBWT(device=0)
    (_, load_ms) = wall(lambda: b.load_reads((reads.reshape(-1), np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(length))))
    del reads
    stream = torch.cuda.current_stream(dev).cuda_stream
    if args.links:
        lines, same = link_lines(b, args, True, dev, stream)
        finish_links(args, lines, same, load_ms)
        return
    lines, same = [], True
    for k in [int(x) for x in args.ks.split(",")]:
        for m in [int(x) for x in args.min_counts.split(",")]:
            U, S = b.enumerate_canonical_unitigs_device(k, None, None, None, None, None, 0, 0, min_count=m, stream=stream)
            pU, pS = b.enumerate_unitigs_device(k, None, None, None, None, None, 0, 0, min_count=m, stream=stream)

            def buffers(u, s):
                return {"symbols": torch.empty(s, dtype=torch.uint8, device=dev), "offsets": torch.empty(u + 1, dtype=torch.int64, device=dev),
                        "sums": torch.empty(u, dtype=torch.int64, device=dev), "ends": torch.empty(u, dtype=torch.uint8, device=dev),
                        "flags": torch.empty(u, dtype=torch.uint8, device=dev)}

            out, plain_out = buffers(U, S), buffers(pU, pS)
            ptrs, plain_ptrs = [x.data_ptr() for x in out.values()], [x.data_ptr() for x in plain_out.values()]
            calls = {"canonical": lambda: b.enumerate_canonical_unitigs_device(k, *ptrs, U, S, min_count=m, stream=stream),
                     "count": lambda: b.enumerate_canonical_unitigs_device(k, None, None, None, None, None, 0, 0, min_count=m, stream=stream),
                     "plain": lambda: b.enumerate_unitigs_device(k, *plain_ptrs, pU, pS, min_count=m, stream=stream)}
            for fn in calls.values():  # warm-up
                fn()
            ms = {name: [] for name in calls}
            for _ in range(args.repeats):  # alternating
                for name, fn in calls.items():
                    _, t = wall(fn)
                    ms[name].append(t)
            b.device_status(stream)
            assert calls["canonical"]() == (U, S)
            info, scratch = b.canonical_unitig_info(), b.spectrum_scratch_bytes()
            calls["count"]()
            res = {"k": k, "min_count": m, "symbols": int(b.get_total_size()), "info": info, "nodes": 2 * info["classes"] - info["palindromes"],
                   "scratch_bytes": scratch, "count_scratch_bytes": b.spectrum_scratch_bytes(), "canonical_ms": spread(ms["canonical"]), "count_ms": spread(ms["count"]),
                   "plain_ms": spread(ms["plain"]), "plain_unitigs": pU, "half_plain_unitigs": pU / 2, "plain_symbols": pS}
            res["canonical_over_plain"] = round(res["canonical_ms"]["median"] / res["plain_ms"]["median"], 2)
            del plain_out
            torch.cuda.empty_cache()
            if not args.no_host_route:
                (theirs, dump_ms) = wall(lambda: b.enumerate_unitigs(k, min_count=m))
                (paired, pair_ms) = wall(lambda: pair_mirrors(theirs[0], theirs[1], k))
                res["host_route_ms"] = {"unitigs_to_host": round(dump_ms, 1), "pairing": round(pair_ms, 1), "total": round(dump_ms + pair_ms, 1), "with_a_mirror": paired}
                del theirs
            if m == args.check_min_count:
                (cw, cc), _ = wall(lambda: b.enumerate_canonical_kmers(k, min_count=m))
                (ew, _), _ = wall(lambda: b.enumerate_canonical_kmers(k + 1, min_count=m))
                theirs, host_ms = wall(lambda: host_restatement(cw, cc, ew, k))
                del cw, cc, ew
                res["restatement_ms"] = round(host_ms, 1)
                res["same_totals"] = (len(theirs[2]), len(theirs[0])) == (U, S) and theirs[5] == res["nodes"]
                pick = np.sort(np.random.default_rng(k * 1000 + m).choice(U, size=min(SAMPLE, U), replace=False))
                ours = {name: x.cpu().numpy() for name, x in out.items()}
                ok = res["same_totals"] and np.array_equal(ours["offsets"].astype(U64), theirs[1])
                if ok:
                    for name, their in (("sums", theirs[2]), ("ends", theirs[3]), ("flags", theirs[4])):
                        ok = ok and np.array_equal(ours[name][pick].astype(their.dtype), their[pick])
                    for u in pick:
                        a, z = int(theirs[1][u]), int(theirs[1][u + 1])
                        ok = ok and np.array_equal(ours["symbols"][a:z], theirs[0][a:z])
                res["sample"], res["same_sample"] = int(len(pick)), bool(ok)
                same = same and bool(ok)
                del theirs, ours
            print(json.dumps(res), flush=True)
            lines.append(res)
            del out
            torch.cuda.empty_cache()
    key = lambda r: "%d/%d" % (r["k"], r["min_count"])
    summary = {"config": args.config, "scale": args.scale, "load_reads_ms": round(load_ms, 1), "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
               "canonical_ms": {key(r): r["canonical_ms"]["median"] for r in lines}, "count_ms": {key(r): r["count_ms"]["median"] for r in lines},
               "plain_ms": {key(r): r["plain_ms"]["median"] for r in lines},
               "host_route_ms": {key(r): r["host_route_ms"]["total"] for r in lines if "host_route_ms" in r},
               "unitigs_beside_half_plain": {key(r): [r["info"]["unitigs"], r["half_plain_unitigs"]] for r in lines}, "same": same}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"lines": lines, "summary": summary}, f, indent=1)
    if not same:
        sys.exit("the host restatement and the canonical unitig call disagree")


if __name__ == "__main__":
    main()
