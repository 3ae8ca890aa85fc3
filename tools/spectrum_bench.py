#!/usr/bin/env python3
"""The k-mer spectrum and the k-mer dump on the read set of a synth.CONFIGS entry (default C4: 12.9 M reads of 150 bp with 0.5 %
substitutions, 1.95e9 symbols at scale 1), built and loaded by load_reads.  For k = 21 and k = 31, `--repeats` rounds each (median and
spread, wall clock around calls that synchronise):
  spectrum   kmer_spectrum(k)                                              -- the histogram, nothing pruned
  dump_1     enumerate_kmers_device(k, min_count=1), unsorted and sorted   -- every k-mer (the count walk, then the writing walk)
  dump_2     the same with min_count=2                                     -- pruned: the once-only suffixes are dropped at every level
  windows    every window of every read through count_read_kmers_device, duplicates removed on the device with torch (sort by the
             window's 2-bit word, first of each run), then the same histogram -- the route without these calls (it needs the reads)
Per walk: the nodes per level (spectrum_info), the nodes expanded (all but the last level's) and the lines per expanded node the
measured time would mean at the line rate probe_line_rate reports for the array the walk reads (pair blocks, else blocks) -- to be
held against the one to two random lines a node's step really reads (the line of l, and that of h when it lies in another block).
The histograms of `spectrum` and `windows` are compared.  One JSON line per k and a closing summary line; no threshold."""
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

BINS = 256


def spread(ms):
    t = sorted(ms)
    return {"median": round(float(np.median(t)), 3), "min": round(t[0], 3), "max": round(t[-1], 3)}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def walk_figures(b, ms, line_rate):
    info = b.spectrum_info()
    k = info["k"]
    nodes = [int(x) for x in info["nodes"][:k + 1]]
    expanded = sum(nodes[:k])  # (the nodes of the last level are the k-mers themselves: they are not expanded)
    return {"nodes_per_level": {d: n for d, n in enumerate(nodes) if n}, "expanded": expanded, "chunks": info["chunks"], "retries": info["retries"],
            "seed_depth": info["seed_depth"], "walk_ms": round(info["ms"], 3),
            "lines_per_node_by_time": round(ms * 1e-3 * line_rate / max(expanded, 1), 3) if line_rate else None}


def windows_route(b, d_reads, k, dev):
    """histogram by the calls the library had before: count every window, then one count per distinct window"""
    n, length = d_reads.shape
    w = length - k + 1
    stream = torch.cuda.current_stream(dev).cuda_stream
    counts = torch.empty((n, w), dtype=torch.int64, device=dev)
    b.count_read_kmers_device(d_reads.data_ptr(), length, n, k, False, counts.data_ptr(), None, stream)
    b.device_status(stream)
    code = torch.tensor([-1, 0, 1, 2, -1, 3], dtype=torch.int64, device=dev)
    words = torch.zeros((n, w), dtype=torch.int64, device=dev)
    valid = torch.ones((n, w), dtype=torch.bool, device=dev)
    for j in range(k):
        c = code[d_reads[:, j:j + w].long()]
        valid &= c >= 0
        words = (words << 2) | c.clamp(min=0)
    words, counts = words[valid], counts[valid]
    del valid
    words, order = torch.sort(words)
    first = torch.ones_like(words, dtype=torch.bool)
    first[1:] = words[1:] != words[:-1]
    per_kmer = counts[order][first]
    hist = torch.bincount(per_kmer.clamp(max=BINS - 1), minlength=BINS)
    return hist.cpu().numpy().astype(np.uint64), int(first.sum()), int(per_kmer.sum())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="c4")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--ks", default="21,31")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-windows", action="store_true", help="skip the route through count_read_kmers_device")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("spectrum_bench needs a GPU")
    dev = torch.device("cuda:0")
    reads = read_set(args.config, args.scale)
    n, length = reads.shape
    b = msbwt.RleBWT(device=0)
    (_, load_ms) = wall(lambda: b.load_reads((reads.reshape(-1), np.arange(n + 1, dtype=np.uint64) * np.uint64(length))))
    which = "pair_blocks" if b.get_pair_index() else "blocks"
    line_rate = b.probe_line_rate(which)
    stream = torch.cuda.current_stream(dev).cuda_stream
    lines = []
    for k in [int(x) for x in args.ks.split(",")]:
        res = {"k": k, "symbols": int(b.get_total_size()), "pair_index": b.get_pair_index(), "table_depth": b.get_table_depth(), "array": which,
               "line_rate": round(line_rate / 1e9, 3)}
        ms = []
        for _ in range(args.repeats):
            (hist, distinct, occurrences), t = wall(lambda: b.kmer_spectrum(k, BINS))
            ms.append(t)
        res["spectrum"] = dict(ms=spread(ms), distinct=distinct, occurrences=occurrences, once=int(hist[1]), **walk_figures(b, float(np.median(ms)), line_rate))
        for least in (1, 2):
            count, t_count = wall(lambda: b.enumerate_kmers_device(k, None, None, None, 0, min_count=least, stream=stream))
            bufs = [torch.empty(count, dtype=torch.int64, device=dev) for _ in range(3)]
            entry = {"records": count, "count_only_ms": round(t_count, 3)}
            for srt in (False, True):
                ms = []
                for _ in range(args.repeats):
                    _, t = wall(lambda: b.enumerate_kmers_device(k, *[x.data_ptr() for x in bufs], count, min_count=least, sorted=srt, stream=stream))
                    ms.append(t)
                entry["sorted" if srt else "unsorted"] = dict(ms=spread(ms), **walk_figures(b, float(np.median(ms)) / 2, line_rate))  # (two walks per call)
            b.device_status(stream)
            entry["ascending"] = bool((bufs[2][1:] > bufs[2][:-1]).all()) if count > 1 else True
            res["dump_%d" % least] = entry
            del bufs
        if not args.no_windows:
            d_reads = torch.from_numpy(np.ascontiguousarray(reads)).to(dev)
            (whist, wdistinct, woccurrences), t = wall(lambda: windows_route(b, d_reads, k, dev))
            del d_reads
            torch.cuda.empty_cache()
            res["windows"] = {"ms": round(t, 3), "same_histogram": bool(np.array_equal(whist, hist)) and wdistinct == distinct and woccurrences == occurrences}
        print(json.dumps(res), flush=True)
        lines.append(res)
    summary = {"config": args.config, "scale": args.scale, "load_reads_ms": round(load_ms, 1), "device": torch.cuda.get_device_name(0),
               "spectrum_ms": {r["k"]: r["spectrum"]["ms"]["median"] for r in lines},
               "windows_ms": {r["k"]: r["windows"]["ms"] for r in lines if "windows" in r},
               "same_histogram": all(r["windows"]["same_histogram"] for r in lines if "windows" in r)}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"lines": lines, "summary": summary}, f, indent=1)


if __name__ == "__main__":
    main()
