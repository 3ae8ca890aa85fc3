#!/usr/bin/env python3
"""The unitig graph calls by source beside the unitig graph calls, on the read set of a synth.CONFIGS entry (default C4: 12.9 M reads
of 150 bp with 0.5 % substitutions, 1.95e9 symbols at scale 1) cut by read index into `--parts` (4,32) parts, each built on the device,
merged and loaded by load_merged_many(keep_sources=True) -- as tools/source_spectrum_bench.py builds it; the canonical calls run on the
same set with every second read reverse-complemented.  For k in `--ks` (21,31) and min_count in `--min-counts` (1,2), after a warm-up,
`--repeats` rounds in which the two _device calls alternate on the same index (wall clock around calls that synchronise):
  graph       enumerate_[canonical_]unitig_graph_device: the seven columns into device buffers -- the code of before
  by_source   enumerate_[canonical_]unitig_graph_by_source_device: the same and the U x S matrix
  adds        the difference of the two medians: what the matrix costs
  host_route  with --host-route, once per line, where the n x S count matrix is at most --host-bytes: the route a caller had --
              enumerate_kmers_by_source to the host, the graph call to the host, and a numpy join of every unitig's windows against the
              sorted words -- and whether its matrix equals the device's, word for word
One JSON line per (parts, call, k, min_count) and a closing summary line; no threshold."""
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
from canonical_bench import COMPLEMENT  # noqa: E402
from reads_build_bench import read_set  # noqa: E402
from source_count_bench import cut  # noqa: E402
from spectrum_bench import spread, wall  # noqa: E402

U64 = np.uint64
TWO_BITS = np.array([0, 0, 1, 2, 0, 3], dtype=U64)  # symbol code -> 2-bit value


def note(text):
    print(text, file=sys.stderr, flush=True)


def rc_words(words, k):
    w = ~words
    for shift, mask in ((2, 0x3333333333333333), (4, 0x0F0F0F0F0F0F0F0F), (8, 0x00FF00FF00FF00FF), (16, 0x0000FFFF0000FFFF)):
        w = ((w >> U64(shift)) & U64(mask)) | ((w & U64(mask)) << U64(shift))
    w = (w >> U64(32)) | (w << U64(32))
    return w >> U64(64 - 2 * k)


def host_route(b, k, m, canonical):
    """the matrix from the k-mer dump by source and the unitigs' windows, on the host -> (matrix, ms)"""
    t0 = time.perf_counter()
    words, counts = b.enumerate_kmers_by_source(k)  # every k-mer: a member of a class may lie below the threshold
    symbols, offsets, sums = b.enumerate_unitig_graph(k, min_count=m, canonical=canonical)[:3]
    two, offsets = TWO_BITS[symbols], offsets.astype(np.int64)
    nodes = np.diff(offsets) - (k - 1)
    w = np.zeros(len(two) - k + 1, dtype=U64)
    for j in range(k):
        w = (w << U64(2)) | two[j:len(two) - k + 1 + j]
    at = np.arange(len(w))
    w = w[at + k <= offsets[np.searchsorted(offsets, at, side="right")]]
    starts = np.concatenate([[0], np.cumsum(nodes)[:-1]])

    def rows_of(q):
        slot = np.minimum(np.searchsorted(words, q), len(words) - 1)
        return np.where((words[slot] == q)[:, None], counts[slot], U64(0))

    per_node = rows_of(w)
    if canonical:
        mirror = rc_words(w, k)
        per_node = per_node + np.where((mirror != w)[:, None], rows_of(mirror), U64(0))
    matrix = np.add.reduceat(per_node, starts, axis=0)
    assert np.array_equal(matrix.sum(axis=1), sums)
    return matrix, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="c4")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--parts", default="4,32")
    ap.add_argument("--ks", default="21,31")
    ap.add_argument("--min-counts", default="1,2")
    ap.add_argument("--calls", default="plain,canonical")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-route", action="store_true", help="time the route through the k-mer dump by source and a numpy join, and compare the matrices")
    ap.add_argument("--host-bytes", type=float, default=2e9, help="the largest n x S count matrix the host route is run for")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("unitig_source_bench needs a GPU")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    reads = read_set(args.config, args.scale)
    note("read set: %d reads of %d" % reads.shape)
    builder = msbwt.RleBWT(device=0)
    lines = []
    for call in args.calls.split(","):
        canonical = call == "canonical"
        if canonical:
            reads = reads.copy()
            reads[1::2] = COMPLEMENT[reads[1::2, ::-1]]
        for S in [int(x) for x in args.parts.split(",")]:
            rles = cut(reads, S, builder)
            b = msbwt.RleBWT(device=0)
            (_, load_ms) = wall(lambda: b.load_merged_many(rles, keep_sources=True))
            del rles
            note("%s, %d parts merged and loaded in %.0f ms" % (call, S, load_ms))
            graph = b.enumerate_canonical_unitig_graph_device if canonical else b.enumerate_unitig_graph_device
            by_source = b.enumerate_canonical_unitig_graph_by_source_device if canonical else b.enumerate_unitig_graph_by_source_device
            for k in [int(x) for x in args.ks.split(",")]:
                for m in [int(x) for x in args.min_counts.split(",")]:
                    U, sym, L = graph(k, *(None,) * 7, 0, 0, 0, min_count=m, stream=stream)
                    bufs = [torch.empty(max(n, 1), dtype=t, device=dev) for n, t in ((sym, torch.uint8), (U + 1, torch.int64), (U, torch.int64), (U, torch.uint8),
                                                                                      (U, torch.uint8), (2 * U + 1, torch.int64), (L, torch.int64))]
                    matrix = torch.empty((max(U, 1), S), dtype=torch.int64, device=dev)
                    ptrs = [x.data_ptr() for x in bufs]
                    calls = {"graph": lambda: graph(k, *ptrs, U, sym, L, min_count=m, stream=stream),
                             "by_source": lambda: by_source(k, *ptrs, matrix.data_ptr(), U, sym, L, min_count=m, stream=stream)}
                    ms = {name: [] for name in calls}
                    for fn in calls.values():  # the warm-up
                        assert fn() == (U, sym, L)
                    sums = bufs[2][:U].clone()
                    scratch = b.spectrum_scratch_bytes()
                    for _ in range(args.repeats):
                        for name, fn in calls.items():
                            ms[name].append(wall(fn)[1])
                    b.device_status(stream)
                    info = (b.canonical_unitig_info if canonical else b.unitig_info)()
                    nodes = info["classes" if canonical else "nodes"]
                    res = {"call": call, "parts": S, "k": k, "min_count": m, "symbols": int(b.get_total_size()), "nodes": nodes, "unitigs": U, "links": L,
                           "graph_ms": spread(ms["graph"]), "by_source_ms": spread(ms["by_source"]), "scratch_bytes": scratch,
                           "rows_sum_to_count_sums": bool(torch.equal(matrix[:U].sum(dim=1), sums)), "nonzero_cells": int((matrix[:U] != 0).sum())}
                    res["adds_ms"] = round(res["by_source_ms"]["median"] - res["graph_ms"]["median"], 3)
                    kmers = int(b.kmer_spectrum(k, 2)[1])
                    if args.host_route and kmers * S * 8 <= args.host_bytes:
                        host, host_ms = host_route(b, k, m, canonical)
                        res["host_route"] = {"ms": round(host_ms, 1), "matrix_bytes": kmers * S * 8, "same_matrix": bool(np.array_equal(host, matrix[:U].cpu().numpy().view(U64)))}
                    else:
                        res["host_route"] = {"ms": None, "matrix_bytes": kmers * S * 8, "same_matrix": None}
                    note("  %s, %d parts, k = %d, min_count %d: %d unitigs; graph %.1f ms, by source %.1f ms, adds %.1f ms; host route %s"
                         % (call, S, k, m, U, res["graph_ms"]["median"], res["by_source_ms"]["median"], res["adds_ms"], res["host_route"]))
                    print(json.dumps(res), flush=True)
                    lines.append(res)
                    del bufs, matrix, sums
                    torch.cuda.empty_cache()
            del b
            torch.cuda.empty_cache()
    key = lambda r: "%s, %d parts, k = %d, min_count %d" % (r["call"], r["parts"], r["k"], r["min_count"])
    compared = [r["host_route"]["same_matrix"] for r in lines if r["host_route"]["same_matrix"] is not None]
    summary = {"config": args.config, "scale": args.scale, "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "repeats": args.repeats,
               "graph_ms": {key(r): r["graph_ms"]["median"] for r in lines}, "by_source_ms": {key(r): r["by_source_ms"]["median"] for r in lines},
               "adds_ms": {key(r): r["adds_ms"] for r in lines}, "rows_sum_to_count_sums": all(r["rows_sum_to_count_sums"] for r in lines),
               "host_routes_compared": len(compared), "same_matrix": all(compared) if compared else None}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"lines": lines, "summary": summary}, f, indent=1)
    if not summary["rows_sum_to_count_sums"] or summary["same_matrix"] is False:
        sys.exit("the matrix of the device and the host route's, or its rows and the count sums, disagree")


if __name__ == "__main__":
    main()
