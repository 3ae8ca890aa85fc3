#!/usr/bin/env python3
"""The k-mer graph on the read set of a synth.CONFIGS entry (default C4: 12.9 M reads of 150 bp with 0.5 % substitutions, 1.95e9
symbols at scale 1), built and loaded by load_reads.  For k = 21 and 31 and min_count = 1 and 2, `--repeats` rounds each, the calls
alternating within a round (median and spread, wall clock around calls that end in a synchronise):
  graph      enumerate_kmer_graph_device: words, counts, l and the edge bytes into device buffers
  degrees    kmer_graph_degrees: the 5 x 5 table, no record leaves the device
  dump       (a) enumerate_kmers_device, sorted, of the same window -- the difference to `graph` is what the edge pass adds
  route      (b) what a caller had before: that dump, the words unpacked to symbol codes (torch), count_kmer_extensions_device for the
             predecessors, and four count_kmers_packed_device batches of q.c ((k+1)-mers) for the successors
On a fixed sample of 2^20 records the edge bytes route (b) implies must equal the call's: a mismatch fails the tool.  One JSON line per
(k, min_count) and a closing summary line; no threshold on the times."""
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
from reads_build_bench import read_set  # noqa: E402

SAMPLE = 1 << 20


def spread(ms):
    t = sorted(ms)
    return {"median": round(float(np.median(t)), 3), "min": round(t[0], 3), "max": round(t[-1], 3)}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def route_b(b, k, n, min_count, bufs, dev, stream):
    """the edge bytes by the calls the library had before; returns (bytes as a uint8 tensor, milliseconds per stage)"""
    words, counts, l = bufs
    ms = {}
    _, ms["dump"] = wall(lambda: b.enumerate_kmers_device(k, words.data_ptr(), counts.data_ptr(), l.data_ptr(), n, min_count=min_count, sorted=True, stream=stream))

    def unpack():
        code = torch.tensor([1, 2, 3, 5], dtype=torch.uint8, device=dev)
        shifts = torch.arange(2 * (k - 1), -2, -2, dtype=torch.int64, device=dev)
        out = torch.empty((n, k), dtype=torch.uint8, device=dev)
        step = 1 << 24  # (pieces: the intermediate of a whole column set is 8 k bytes per record)
        for i in range(0, n, step):
            out[i:i + step] = code[((words[i:i + step, None] >> shifts[None, :]) & 3)]
        return out
    kmers, ms["unpack"] = wall(unpack)
    ext = torch.empty((n, 6), dtype=torch.int64, device=dev)

    def extensions():
        b.count_kmer_extensions_device(kmers.data_ptr(), k, n, ext.data_ptr(), stream)
        b.device_status(stream)
    _, ms["extensions"] = wall(extensions)
    del kmers
    after = torch.empty((4, n), dtype=torch.int64, device=dev)

    def successors():
        for c in range(4):
            q = (words << 2) | c
            if k < 31:
                q &= (1 << (2 * (k + 1))) - 1
            b.count_kmers_packed_device(q.data_ptr(), k + 1, n, after[c].data_ptr(), stream)
            b.device_status(stream)  # (q is released behind it)
    _, ms["successors"] = wall(successors)
    edges = torch.zeros(n, dtype=torch.uint8, device=dev)
    for j, sym in enumerate((1, 2, 3, 5)):
        edges |= (ext[:, sym] >= min_count).to(torch.uint8) << j
        edges |= (after[j] >= min_count).to(torch.uint8) << (4 + j)
    ms["total"] = ms["dump"] + ms["unpack"] + ms["extensions"] + ms["successors"]
    ms["total_without_unpack"] = ms["total"] - ms["unpack"]
    return edges, ms


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="c4")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--ks", default="21,31")
    ap.add_argument("--min-counts", default="1,2")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--route-repeats", type=int, default=1, help="rounds of route (b) that are timed (each takes seconds)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("kmer_graph_bench needs a GPU")
    if args.repeats < 5:
        sys.exit("a median of at least five calls")
    dev = torch.device("cuda:0")
    reads = read_set(args.config, args.scale)
    n_reads, length = reads.shape
    b = msbwt.RleBWT(device=0)
    (_, load_ms) = wall(lambda: b.load_reads((reads.reshape(-1), np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(length))))
    stream = torch.cuda.current_stream(dev).cuda_stream
    lines, same = [], True
    for k in [int(x) for x in args.ks.split(",")]:
        for m in [int(x) for x in args.min_counts.split(",")]:
            n = b.enumerate_kmer_graph_device(k, None, None, None, None, 0, min_count=m, stream=stream)
            bufs = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(3)]
            edges = torch.empty(n, dtype=torch.uint8, device=dev)
            ptrs = [x.data_ptr() for x in bufs]
            calls = {"graph": lambda: b.enumerate_kmer_graph_device(k, *ptrs, edges.data_ptr(), n, min_count=m, stream=stream),
                     "degrees": lambda: b.kmer_graph_degrees(k, min_count=m),
                     "dump": lambda: b.enumerate_kmers_device(k, *ptrs, n, min_count=m, sorted=True, stream=stream)}
            for fn in calls.values():  # warm-up
                fn()
            ms = {name: [] for name in calls}
            for _ in range(args.repeats):  # alternating
                for name, fn in calls.items():
                    out, t = wall(fn)
                    ms[name].append(t)
                    if name == "degrees":
                        table, nodes, n_edges = out
            b.device_status(stream)
            calls["graph"]()
            info = b.spectrum_info()
            graph_words = bufs[0].clone()
            res = {"k": k, "min_count": m, "symbols": int(b.get_total_size()), "nodes": n, "edges": int(n_edges), "table": table.tolist(),
                   "scratch_bytes": b.spectrum_scratch_bytes(), "chunks": info["chunks"], "retries": info["retries"],
                   "graph_ms": spread(ms["graph"]), "degrees_ms": spread(ms["degrees"]), "dump_ms": spread(ms["dump"])}
            res["edge_pass_ms"] = round(res["graph_ms"]["median"] - res["dump_ms"]["median"], 3)
            assert nodes == n == int(table.sum())
            route = []
            for _ in range(max(args.route_repeats, 1)):
                theirs, stages = route_b(b, k, n, m, bufs, dev, stream)
                route.append(stages)
            res["route_b_ms"] = {key: spread([r[key] for r in route]) for key in route[0]}
            res["route_b_over_graph"] = round(res["route_b_ms"]["total_without_unpack"]["median"] / res["graph_ms"]["median"], 2)
            pick = torch.from_numpy(np.random.default_rng(k * 1000 + m).choice(n, size=min(SAMPLE, n), replace=False)).to(dev)
            res["sample"] = int(pick.numel())
            res["same_words"] = bool(torch.equal(graph_words[pick], bufs[0][pick]))
            res["same_edges"] = bool(torch.equal(edges[pick], theirs[pick]))
            res["same_everywhere"] = bool(torch.equal(edges, theirs))
            same = same and res["same_words"] and res["same_edges"]
            print(json.dumps(res), flush=True)
            lines.append(res)
            del bufs, edges, theirs, graph_words
            torch.cuda.empty_cache()
    summary = {"config": args.config, "scale": args.scale, "load_reads_ms": round(load_ms, 1), "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
               "graph_ms": {"%d/%d" % (r["k"], r["min_count"]): r["graph_ms"]["median"] for r in lines},
               "route_b_ms": {"%d/%d" % (r["k"], r["min_count"]): r["route_b_ms"]["total_without_unpack"]["median"] for r in lines}, "same_edges": same}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"lines": lines, "summary": summary}, f, indent=1)
    if not same:
        sys.exit("route (b) and the graph call disagree on the sample")


if __name__ == "__main__":
    main()
