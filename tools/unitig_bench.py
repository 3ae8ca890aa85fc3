#!/usr/bin/env python3
"""Unitigs on the read set of a synth.CONFIGS entry (default C4: 12.9 M reads of 150 bp with 0.5 % substitutions, 1.95e9 symbols at
scale 1), built and loaded by load_reads.  For k = 21 and 31 and min_count = 1 and 2, `--repeats` rounds each, the calls alternating
within a round (median and spread, wall clock around calls that end in a synchronise):
  unitigs    (i) enumerate_unitigs_device: symbols, offsets, count sums, ends and flags into device buffers
  count      (i) the same call with both capacities 0: U and S only
  graph      (ii) enumerate_kmer_graph_device alone: words, counts and edge bytes into device buffers -- the difference to `unitigs` is
             what the compaction adds
  host       (iii) what a caller had before: enumerate_kmer_graph to host arrays (25 bytes a node over the link), then the compaction
             there -- a numpy restatement of the same steps (predecessor by binary search in the sorted words, links, pointer jumping
             over whole arrays, min-label opening of cycles, cumulative sums, scatter of the symbols), single-threaded as numpy is.
             Timed once per window, and only for windows of at most `--host-max-nodes` nodes.
U and S of (i) and (iii) must agree, and so must the sequences, count sums, ends and flags of a fixed sample of unitigs: a mismatch
fails the tool.  One JSON line per (k, min_count) with unitig_info and the scratch bytes, and a closing summary line; no threshold on
the times.
`--links` prints the link lines INSTEAD (tools/canonical_unitig_bench.py --links: the same for the canonical call), per (k, min_count):
  graph      enumerate_unitig_graph_device: the five columns and the link table into device buffers
  unitigs    beside it in the same rounds, enumerate_unitigs_device: what the link table adds is the difference
  host       the route a caller had before, timed once: the unitig call to host arrays, then a numpy join of the end k-mers against the
             first k-mers (the successors of every last word looked up among the first words and the mirrored last words)
The two link tables must be equal, word for word: a mismatch fails the tool."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import rust_msbwt_amd as msbwt  # noqa: E402
from kmer_graph_bench import spread, wall  # noqa: E402
from reads_build_bench import read_set  # noqa: E402

SAMPLE = 1 << 16
U64 = np.uint64
POP = np.array([bin(x).count("1") for x in range(16)], dtype=np.uint8)
LOW = np.array([0, 0, 1, 0, 2, 0, 0, 0, 3] + [0] * 7, dtype=np.uint8)  # the set bit of a nibble that has one
CODE = np.array([1, 2, 3, 5], dtype=np.uint8)


def rank_by_jumping(up, unfinished):
    """(head, distance) of every node from its link up (up[i] == i: a head), by pointer jumping over the `unfinished` nodes; what stays
    unfinished lies on cycles.  Returns head, distance, the nodes still unfinished, rounds."""
    n = len(up)
    head, dist, done = up.copy(), np.zeros(n, dtype=np.int64), np.ones(n, dtype=bool)
    dist[unfinished] = 1
    done[unfinished] = False
    rounds = 0
    while len(unfinished):
        a = head[unfinished]
        step, finished, far = dist[a], done[a], head[a]  # (read whole before anything is written: a round is simultaneous)
        dist[unfinished] += step
        head[unfinished] = far
        done[unfinished] = finished
        rounds += 1
        left = unfinished[~finished]
        if len(left) == len(unfinished):
            break
        unfinished = left
    return head, dist, unfinished, rounds


def host_compaction(words, counts, edges, k):
    """the unitigs from the graph dump's host arrays -> (symbols, offsets, sums, ends, flags, rounds)"""
    n = len(words)
    slots = np.arange(n, dtype=np.int64)
    indeg, outdeg = POP[edges & 15], POP[edges >> 4]
    one = np.flatnonzero(indeg == 1)
    before = (LOW[edges[one] & 15].astype(U64) << U64(2 * (k - 1))) | (words[one] >> U64(2))
    pred = np.searchsorted(words, before)
    linked = outdeg[pred] == 1
    up = slots.copy()
    up[one[linked]] = pred[linked]
    circular = np.zeros(n, dtype=bool)
    circular[one[linked][pred[linked] == one[linked]]] = True  # self-loops
    head, dist, cyc, rounds = rank_by_jumping(up, np.flatnonzero(up != slots))
    if len(cyc):
        label, ptr = slots.copy(), up.copy()
        for _ in range(max(int(np.ceil(np.log2(len(cyc)))), 1)):
            a = ptr[cyc]
            lower, far = np.minimum(label[cyc], label[a]), ptr[a]
            label[cyc], ptr[cyc] = lower, far
            rounds += 1
        opening = cyc[label[cyc] == cyc]
        up[opening] = opening
        circular[opening] = True
        rest = cyc[label[cyc] != cyc]
        h2, d2, left, r2 = rank_by_jumping(up, rest)
        assert len(left) == 0
        head[cyc], dist[cyc] = h2[cyc], d2[cyc]
        head[opening], dist[opening] = opening, 0
        rounds += r2
    is_head = up == slots
    number = np.cumsum(is_head) - 1
    unitig = number[head]
    U = int(is_head.sum())
    nodes = np.bincount(unitig, minlength=U)
    offsets = np.zeros(U + 1, dtype=U64)
    offsets[1:] = np.cumsum(nodes + (k - 1))
    symbols = np.zeros(int(offsets[-1]), dtype=np.uint8)
    at = offsets[:-1].astype(np.int64)
    symbols[at[unitig] + (k - 1) + dist] = CODE[(words & U64(3)).astype(np.int64)]
    first = words[is_head]
    for j in range(k - 1):
        symbols[at + j] = CODE[((first >> U64(2 * (k - 1 - j))) & U64(3)).astype(np.int64)]
    sums = np.bincount(unitig, weights=counts.astype(np.float64), minlength=U).astype(U64)  # (exact below 2^53)
    has_down = np.zeros(n, dtype=bool)
    has_down[up[~is_head]] = True
    tails = np.flatnonzero(~has_down)
    ends = np.zeros(U, dtype=np.uint8)
    ends[unitig[tails]] = (edges[head[tails]] & 15) | (edges[tails] & 0xF0)
    flags = np.zeros(U, dtype=np.uint8)
    flags[number[np.flatnonzero(circular)]] = 1
    return symbols, offsets, sums, ends, flags, rounds


REVERSED = np.array([int("{:04b}".format(x)[::-1], 2) for x in range(16)], dtype=np.uint8)  # a nibble with bit j at 3 - j


def words_at(symbols, starts, k):
    two = np.zeros(6, dtype=U64)
    two[[1, 2, 3, 5]] = [0, 1, 2, 3]
    w = np.zeros(len(starts), dtype=U64)
    for j in range(k):
        w = (w << U64(2)) | two[symbols[starts + j]]
    return w


def host_join(symbols, offsets, ends, k, canonical):
    """the link table from a unitig call's host arrays -> (link_offsets, link_targets): side 2u leaves the last word of u along its
    out-bits, side 2u + 1 the reverse complement of its first word along its in-bits mirrored; the word reached is looked up among the
    first words (2v) and among the reverse complements of the last words (2v + 1)"""
    rc2 = msbwt.rle_bwt.reverse_complement_2bit
    first, last = words_at(symbols, offsets[:-1].astype(np.int64), k), words_at(symbols, offsets[1:].astype(np.int64) - k, k)
    U = len(first)
    mirrored_first, mirrored_last = rc2(first, k), rc2(last, k)
    own_mirror = (first == last) & (mirrored_first == first) if canonical else np.zeros(U, dtype=bool)
    order = np.argsort(mirrored_last, kind="stable")
    mirrored_sorted = mirrored_last[order]
    leaves = np.stack([last, mirrored_first], axis=1).reshape(2 * U)
    bits = np.stack([ends >> 4, np.where(own_mirror, 0, REVERSED[ends & 15])], axis=1).reshape(2 * U)
    present = ((bits[:, None] >> np.arange(4, dtype=np.uint8)[None, :]) & 1).astype(bool)
    side, c = np.nonzero(present)
    reached = (leaves[side] << U64(2)) | c.astype(U64)
    if k < 32:
        reached &= U64((1 << (2 * k)) - 1)
    at_first = np.minimum(np.searchsorted(first, reached), U - 1)
    at_last = order[np.minimum(np.searchsorted(mirrored_sorted, reached), U - 1)]
    to_first = first[at_first] == reached if canonical else side % 2 == 0
    link_offsets = np.zeros(2 * U + 1, dtype=U64)
    np.cumsum(present.sum(axis=1), out=link_offsets[1:])
    return link_offsets, np.where(to_first, 2 * at_first, 2 * at_last + 1).astype(U64)


def link_lines(b, args, canonical, dev, stream):
    """the --links lines of either tool -> (lines, all tables equal)"""
    graph_device = b.enumerate_canonical_unitig_graph_device if canonical else b.enumerate_unitig_graph_device
    unitigs_device = b.enumerate_canonical_unitigs_device if canonical else b.enumerate_unitigs_device
    to_host = b.enumerate_canonical_unitigs if canonical else b.enumerate_unitigs
    lines, same = [], True
    for k in [int(x) for x in args.ks.split(",")]:
        for m in [int(x) for x in args.min_counts.split(",")]:
            U, S, L = graph_device(k, None, None, None, None, None, None, None, 0, 0, 0, min_count=m, stream=stream)
            out = {"symbols": torch.empty(S, dtype=torch.uint8, device=dev), "offsets": torch.empty(U + 1, dtype=torch.int64, device=dev),
                   "sums": torch.empty(U, dtype=torch.int64, device=dev), "ends": torch.empty(U, dtype=torch.uint8, device=dev),
                   "flags": torch.empty(U, dtype=torch.uint8, device=dev), "link_offsets": torch.empty(2 * U + 1, dtype=torch.int64, device=dev),
                   "link_targets": torch.empty(L, dtype=torch.int64, device=dev)}
            ptrs = [x.data_ptr() for x in out.values()]
            calls = {"graph": lambda: graph_device(k, *ptrs, U, S, L, min_count=m, stream=stream),
                     "unitigs": lambda: unitigs_device(k, *ptrs[:5], U, S, min_count=m, stream=stream)}
            for fn in calls.values():  # warm-up
                fn()
            ms = {name: [] for name in calls}
            for _ in range(args.repeats):  # alternating
                for name, fn in calls.items():
                    _, t = wall(fn)
                    ms[name].append(t)
            b.device_status(stream)
            assert calls["graph"]() == (U, S, L)
            scratch = b.spectrum_scratch_bytes()
            info = (b.canonical_unitig_info if canonical else b.unitig_info)()
            res = {"links": True, "canonical": canonical, "k": k, "min_count": m, "symbols": int(b.get_total_size()), "info": info, "link_entries": L,
                   "scratch_bytes": scratch, "graph_ms": spread(ms["graph"]), "unitigs_ms": spread(ms["unitigs"])}
            res["links_add_ms"] = round(res["graph_ms"]["median"] - res["unitigs_ms"]["median"], 3)
            res["ns_per_entry"] = round(1e6 * res["links_add_ms"] / max(L, 1), 2)
            (theirs, dump_ms) = wall(lambda: to_host(k, min_count=m))
            ((link_offsets, link_targets), join_ms) = wall(lambda: host_join(theirs[0], theirs[1], theirs[3], k, canonical))
            res["host_ms"] = {"unitigs_to_host": round(dump_ms, 1), "join": round(join_ms, 1), "total": round(dump_ms + join_ms, 1)}
            res["host_over_graph"] = round(res["host_ms"]["total"] / res["graph_ms"]["median"], 1)
            ok = np.array_equal(out["link_offsets"].cpu().numpy().view(U64), link_offsets) and np.array_equal(out["link_targets"].cpu().numpy().view(U64), link_targets)
            res["same_table"] = bool(ok)
            same = same and bool(ok)
            del theirs, link_offsets, link_targets, out
            torch.cuda.empty_cache()
            print(json.dumps(res), flush=True)
            lines.append(res)
    return lines, same


def finish_links(args, lines, same, load_ms):
    """the closing summary line of a --links run, the file, and the verdict"""
    key = lambda r: "%d/%d" % (r["k"], r["min_count"])
    summary = {"links": True, "config": args.config, "scale": args.scale, "load_reads_ms": round(load_ms, 1), "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
               "graph_ms": {key(r): r["graph_ms"]["median"] for r in lines}, "unitigs_ms": {key(r): r["unitigs_ms"]["median"] for r in lines},
               "host_ms": {key(r): r["host_ms"]["total"] for r in lines}, "link_entries": {key(r): r["link_entries"] for r in lines}, "same": same}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"lines": lines, "summary": summary}, f, indent=1)
    if not same:
        sys.exit("the host join and the device link table disagree")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--links", action="store_true", help="the link lines in place of the others: enumerate_unitig_graph_device beside enumerate_unitigs_device")
    ap.add_argument("--config", default="c4")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--ks", default="21,31")
    ap.add_argument("--min-counts", default="1,2")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-max-nodes", type=float, default=1e8, help="route (iii) runs for windows of at most this many nodes (numpy takes minutes beyond)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("unitig_bench needs a GPU")
    if args.repeats < 5:
        sys.exit("a median of at least five calls")
    dev = torch.device("cuda:0")
    reads = read_set(args.config, args.scale)
    n_reads, length = reads.shape
    b = msbwt.RleBWT(device=0)
    (_, load_ms) = wall(lambda: b.load_reads((reads.reshape(-1), np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(length))))
    del reads
    stream = torch.cuda.current_stream(dev).cuda_stream
    if args.links:
        lines, same = link_lines(b, args, False, dev, stream)
        finish_links(args, lines, same, load_ms)
        return
    lines, same = [], True
    for k in [int(x) for x in args.ks.split(",")]:
        for m in [int(x) for x in args.min_counts.split(",")]:
            U, S = b.enumerate_unitigs_device(k, None, None, None, None, None, 0, 0, min_count=m, stream=stream)
            n = b.unitig_info()["nodes"]
            out = {"symbols": torch.empty(S, dtype=torch.uint8, device=dev), "offsets": torch.empty(U + 1, dtype=torch.int64, device=dev),
                   "sums": torch.empty(U, dtype=torch.int64, device=dev), "ends": torch.empty(U, dtype=torch.uint8, device=dev),
                   "flags": torch.empty(U, dtype=torch.uint8, device=dev)}
            ptrs = [x.data_ptr() for x in out.values()]
            graph = [torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)]
            calls = {"unitigs": lambda: b.enumerate_unitigs_device(k, *ptrs, U, S, min_count=m, stream=stream),
                     "count": lambda: b.enumerate_unitigs_device(k, None, None, None, None, None, 0, 0, min_count=m, stream=stream),
                     "graph": lambda: b.enumerate_kmer_graph_device(k, graph[0].data_ptr(), graph[1].data_ptr(), None, graph[2].data_ptr(), n, min_count=m, stream=stream)}
            for fn in calls.values():  # warm-up
                fn()
            ms = {name: [] for name in calls}
            for _ in range(args.repeats):  # alternating
                for name, fn in calls.items():
                    _, t = wall(fn)
                    ms[name].append(t)
            b.device_status(stream)
            assert calls["unitigs"]() == (U, S)
            info, scratch = b.unitig_info(), b.spectrum_scratch_bytes()
            calls["count"]()
            res = {"k": k, "min_count": m, "symbols": int(b.get_total_size()), "unitig_info": info, "scratch_bytes": scratch, "count_scratch_bytes": b.spectrum_scratch_bytes(),
                   "unitigs_ms": spread(ms["unitigs"]), "count_ms": spread(ms["count"]), "graph_ms": spread(ms["graph"])}
            res["compaction_ms"] = round(res["unitigs_ms"]["median"] - res["graph_ms"]["median"], 3)
            del graph
            torch.cuda.empty_cache()
            if n <= args.host_max_nodes:
                (words, counts, edges), dump_ms = wall(lambda: b.enumerate_kmer_graph(k, min_count=m))
                theirs, host_ms = wall(lambda: host_compaction(words, counts, edges, k))
                res["host_ms"] = {"graph_to_host": round(dump_ms, 1), "compaction": round(host_ms, 1), "total": round(dump_ms + host_ms, 1), "rounds": theirs[5]}
                res["host_over_unitigs"] = round(res["host_ms"]["total"] / res["unitigs_ms"]["median"], 1)
                res["same_totals"] = (len(theirs[2]), len(theirs[0])) == (U, S)
                pick = np.sort(np.random.default_rng(k * 1000 + m).choice(U, size=min(SAMPLE, U), replace=False))
                ours = {name: x.cpu().numpy() for name, x in out.items()}
                ok = res["same_totals"] and np.array_equal(ours["offsets"].astype(U64), theirs[1])
                if ok:
                    for name, their in (("sums", theirs[2]), ("ends", theirs[3]), ("flags", theirs[4])):
                        ok = ok and np.array_equal(ours[name][pick].astype(their.dtype), their[pick])
                    for u in pick[:4096]:
                        a, z = int(theirs[1][u]), int(theirs[1][u + 1])
                        ok = ok and np.array_equal(ours["symbols"][a:z], theirs[0][a:z])
                res["sample"], res["same_sample"] = int(len(pick)), bool(ok)
                same = same and bool(ok)
                del words, counts, edges, theirs, ours
            print(json.dumps(res), flush=True)
            lines.append(res)
            del out
            torch.cuda.empty_cache()
    summary = {"config": args.config, "scale": args.scale, "load_reads_ms": round(load_ms, 1), "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
               "unitigs_ms": {"%d/%d" % (r["k"], r["min_count"]): r["unitigs_ms"]["median"] for r in lines},
               "graph_ms": {"%d/%d" % (r["k"], r["min_count"]): r["graph_ms"]["median"] for r in lines},
               "host_ms": {"%d/%d" % (r["k"], r["min_count"]): r["host_ms"]["total"] for r in lines if "host_ms" in r}, "same": same}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"lines": lines, "summary": summary}, f, indent=1)
    if not same:
        sys.exit("the host compaction and the unitig call disagree")


if __name__ == "__main__":
    main()
