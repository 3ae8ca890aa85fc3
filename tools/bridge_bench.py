#!/usr/bin/env python3
"""Bridges on the read set of a synth.CONFIGS entry (default C4: 12.9 M reads of 150 bp with 0.5 % substitutions; --scale 0.02 is 2 % of
it), built and loaded by load_reads.  The pairs are taken as examples/bridge_kmers.c takes them: every k-mer of every read is counted
with the fused call, and a weak stretch -- a maximal run of k-mers below --min-count with a solid k-mer on both sides -- gives the
pair (the solid k-mer before it, the solid k-mer behind it).  A call takes one window of lengths, so the pairs are grouped by the
stretch's own length D (the k-mers of the stretch + 1) and the `--groups` most frequent groups are run, each with the window
D - D/10 .. D + D/10, max_paths = 4 and max_live = 64, capped at `--max-pairs` pairs taken evenly.  For k = 21 and 31, `--repeats`
rounds each, the two routes alternating within a round (median and spread, wall clock around calls that end in a synchronise):
  bridge     bridge_kmers_device: all seven outputs into device buffers
  host loop  the route a caller has without it, level-synchronous: per round ONE count_kmers_packed_device call on queries built with
             torch ops, the expansion, the numbering of the bridges and the four limits in torch on the device, and the host reading
             the size of the next level: the same rounds, written by a caller
All seven outputs of the two routes must be equal, word for word: a mismatch fails the tool.  One JSON line per setting with
bridge_info, the microseconds a round, and a closing summary line; no threshold on the times."""
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
from kmer_graph_bench import spread, wall  # noqa: E402
from reads_build_bench import read_set  # noqa: E402
from trace_bench import edge_words, next_nodes  # noqa: E402

EXHAUSTED, FULL, MAX_STEPS, TOO_WIDE, NO_SEED, NO_TARGET = range(1, 7)


def host_loop(b, seeds, targets, k, min_steps, max_steps, max_paths, max_live, m, me, stream):
    """the seven outputs by one packed count call a round and torch ops between them (direction right)"""
    dev, n = seeds.device, seeds.numel()
    mask, lo = (1 << (2 * k)) - 1, max(min_steps, 1)
    code = torch.tensor([1, 2, 3, 5], dtype=torch.uint8, device=dev)

    def count(words, kk):
        words = words.contiguous()
        out = torch.empty(words.numel(), dtype=torch.int64, device=dev)
        b.count_kmers_packed_device(words.data_ptr(), kk, words.numel(), out.data_ptr(), stream)
        return out.view(words.shape)

    symbols = torch.zeros((n, max_paths, max_steps), dtype=torch.uint8, device=dev)
    lengths, sums = (torch.zeros((n, max_paths), dtype=torch.int64, device=dev) for _ in range(2))
    found, depths, live = (torch.zeros(n, dtype=torch.int64, device=dev) for _ in range(3))
    s, t = seeds & mask, targets & mask
    both = count(torch.stack([s, t]), k)
    stops = torch.where(both[0] < m, NO_SEED, torch.where(both[1] < m, NO_TARGET, 0)).to(torch.uint8)
    alive = stops == 0
    if max_steps == 0:
        stops[alive], live[alive] = MAX_STEPS, 1
        return symbols, lengths, sums, found, stops, depths, live
    pair = torch.nonzero(alive).flatten()
    node, esum = s[pair], torch.zeros(pair.numel(), dtype=torch.int64, device=dev)
    rows = torch.zeros((pair.numel(), max_steps), dtype=torch.uint8, device=dev)
    fc = count(edge_words(node, k, False), k + 1)
    for r in range(1, max_steps + 1):
        if pair.numel() == 0:  # (the host reads the size of the level: one decision a round)
            break
        solid, nxt = fc >= me, next_nodes(node, k, False)
        bridge = solid & (nxt == t[pair][:, None]) if r >= lo else torch.zeros_like(solid)
        child = solid & ~bridge
        nb = torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, pair, bridge.sum(1))
        nc = torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, pair, child.sum(1))
        at = torch.nonzero(bridge.flatten()).flatten()  # in the order of the level, A < C < G < T within a walk
        if at.numel():
            parent, of = at // 4, pair[at // 4]
            number = found[of] + torch.arange(at.numel(), device=dev) - (torch.cumsum(nb, 0) - nb)[of]
            w = number < max_paths
            parent, of, number, sym = parent[w], of[w], number[w], (at % 4)[w]
            symbols[of, number, :r - 1] = rows[parent, :r - 1]
            symbols[of, number, r - 1] = code[sym]
            lengths[of, number] = r
            sums[of, number] = esum[parent] + fc[parent, sym]
        found += nb
        depths[alive] = r
        stop = torch.where(found >= max_paths, FULL, torch.where(nc == 0, EXHAUSTED, torch.where(nc > max_live, TOO_WIDE, 0)))
        if r == max_steps:
            stop = torch.where((found < max_paths) & (nc > 0), MAX_STEPS, stop)
        done = alive & (stop != 0)
        stops[done], live[done] = stop[done].to(torch.uint8), nc[done]
        alive = alive & ~done
        at = torch.nonzero((child & alive[pair][:, None]).flatten()).flatten()
        parent, sym = at // 4, at % 4
        pair, node, esum, rows = pair[parent], nxt[parent, sym], esum[parent] + fc[parent, sym], rows[parent]
        rows[:, r - 1] = code[sym]
        if at.numel():
            fc = count(edge_words(node, k, False), k + 1)
    return symbols, lengths, sums, found, stops, depths, live


def stretch_pairs(b, d_reads, n_reads, length, k, m, stream):
    """{D: (seeds, targets)} of every weak stretch with solid flanks, by the stretch's own length D, as packed words on the device"""
    dev, W = d_reads.device, length - k + 1
    counts = torch.empty((n_reads, W), dtype=torch.int64, device=dev)
    b.count_read_kmers_device(d_reads.data_ptr(), length, n_reads, k, 0, counts.data_ptr(), None, stream)
    weak = counts < m
    del counts
    start = weak[:, 1:] & ~weak[:, :-1]  # window i + 1 opens a stretch behind the solid window i
    r, i = torch.nonzero(start, as_tuple=True)
    own = torch.where(weak, torch.full((1, 1), W, device=dev), torch.arange(W, device=dev)[None, :])
    nxt = torch.flip(torch.cummin(torch.flip(own, [1]), 1).values, [1])  # the next solid window at or behind each one, W for none
    j = nxt[r, i + 1]
    ok = j < W
    r, i, j = r[ok], i[ok], j[ok]
    two = torch.zeros(6, dtype=torch.int64, device=dev)
    two[torch.tensor([1, 2, 3, 5], device=dev)] = torch.arange(4, device=dev)
    reads = d_reads.view(n_reads, length)

    def words(at):
        w = torch.zeros(at.numel(), dtype=torch.int64, device=dev)
        for x in range(k):
            w = (w << 2) | two[reads[r, at + x].long()]
        return w

    seeds, targets, D = words(i), words(j), j - i
    return {int(d): (seeds[D == d].contiguous(), targets[D == d].contiguous()) for d in torch.unique(D).tolist()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="c4")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--ks", default="21,31")
    ap.add_argument("--groups", type=int, default=2, help="the most frequent stretch lengths that are run")
    ap.add_argument("--max-pairs", type=int, default=10 ** 6)
    ap.add_argument("--min-count", type=int, default=2)
    ap.add_argument("--max-paths", type=int, default=4)
    ap.add_argument("--max-live", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bridge_bench needs a GPU")
    if args.repeats < 5:
        sys.exit("a median of at least five calls")
    dev = torch.device("cuda:0")
    reads = read_set(args.config, args.scale)
    n_reads, length = reads.shape
    b = msbwt.RleBWT(device=0)
    (_, load_ms) = wall(lambda: b.load_reads((reads.reshape(-1), np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(length))))
    d_reads = torch.from_numpy(np.ascontiguousarray(reads).reshape(-1)).to(dev)
    del reads
    stream = torch.cuda.current_stream(dev).cuda_stream
    lines, same = [], True
    for k in [int(x) for x in args.ks.split(",")]:
        groups = stretch_pairs(b, d_reads, n_reads, length, k, args.min_count, stream)
        sizes = {d: int(p[0].numel()) for d, p in groups.items()}
        for D in sorted(groups, key=lambda d: -sizes[d])[:args.groups]:
            seeds, targets = groups[D]
            pick = torch.linspace(0, seeds.numel() - 1, min(seeds.numel(), args.max_pairs), dtype=torch.float64, device=dev).long()
            seeds, targets = seeds[pick].contiguous(), targets[pick].contiguous()
            n, lo, hi = seeds.numel(), D - D // 10, min(D + D // 10, 4096)
            ours = [torch.zeros((n, args.max_paths, hi), dtype=torch.uint8, device=dev)] + [torch.zeros((n, args.max_paths), dtype=torch.int64, device=dev) for _ in range(2)]
            ours += [torch.zeros(n, dtype=dt, device=dev) for dt in (torch.int64, torch.uint8, torch.int64, torch.int64)]
            calls = {"bridge": lambda: b.bridge_kmers_device(seeds.data_ptr(), targets.data_ptr(), k, n, hi, *[x.data_ptr() for x in ours], min_steps=lo,
                                                             max_paths=args.max_paths, max_live=args.max_live, min_count=args.min_count, stream=stream),
                     "host_loop": lambda: host_loop(b, seeds, targets, k, lo, hi, args.max_paths, args.max_live, args.min_count, args.min_count, stream)}
            theirs = calls["host_loop"]()  # warm-up, and the comparison
            calls["bridge"]()
            b.device_status(stream)
            ok = all(torch.equal(x, y) for x, y in zip(ours, theirs))
            del theirs
            ms = {route: [] for route in calls}
            for _ in range(args.repeats):  # alternating
                for route, fn in calls.items():
                    _, t = wall(fn)
                    ms[route].append(t)
            info = b.bridge_info()
            res = {"k": k, "stretch": D, "stretches_by_length": dict(sorted(sizes.items(), key=lambda x: -x[1])[:6]), "n": n, "min_steps": lo, "max_steps": hi,
                   "max_paths": args.max_paths, "max_live": args.max_live, "min_count": args.min_count, "symbols": int(b.get_total_size()), "info": info,
                   "stops": torch.bincount(ours[4], minlength=7).tolist(), "one_bridge_of_own_length": int(((ours[1] == D).sum(1) == 1).sum()),
                   "bridge_ms": spread(ms["bridge"]), "host_loop_ms": spread(ms["host_loop"]), "same": bool(ok)}
            res["host_loop_over_bridge"] = round(res["host_loop_ms"]["median"] / res["bridge_ms"]["median"], 2)
            res["us_per_round"] = round(res["bridge_ms"]["median"] * 1e3 / max(info["rounds"], 1), 1)
            res["queries_per_s"] = round(info["queries"] / (res["bridge_ms"]["median"] * 1e-3), 0)
            same = same and bool(ok)
            print(json.dumps(res), flush=True)
            lines.append(res)
            del ours
            torch.cuda.empty_cache()
    key = lambda r: "%d/%d" % (r["k"], r["stretch"])
    summary = {"config": args.config, "scale": args.scale, "load_reads_ms": round(load_ms, 1), "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
               "bridge_ms": {key(r): r["bridge_ms"]["median"] for r in lines}, "host_loop_ms": {key(r): r["host_loop_ms"]["median"] for r in lines}, "same": same}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"lines": lines, "summary": summary}, f, indent=1)
    if not same:
        sys.exit("the host loop and the bridge call disagree")


if __name__ == "__main__":
    main()
