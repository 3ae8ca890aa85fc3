#!/usr/bin/env python3
"""Counts by source against the ways to get them, on the read set of a synth.CONFIGS entry (default C4: 12.9 M reads of 150 bp with
0.5 % substitutions, 1.95e9 symbols at scale 1) cut into `--parts` parts by read index, every part built with build_from_reads and
the parts merged, loaded and coloured by load_merged_many(keep_sources=True).  Device-resident batches of present 31-mers taken from
the reads.  Timed with events, the variants alternating, `--repeats` rounds each (median and spread):
  ranges     kmer_ranges_device on the merged index                      -- phase 1 alone
  by_source  count_kmers_by_source_device on the merged index            -- the new call
  sources    range_sources_device on the precomputed ranges              -- phase 2 alone
  handles    count_kmers_device on one handle per part, one after the other -- the same answer without the call
Once as loaded (k undeclared) and once after set_query_length(31), on the merged handle and on the per-part handles alike.  Then
`by_source` and `sources` once more over the same reads cut into `--many` parts.  Parity of `by_source` against the CPU oracle on
each part, on a sample.  One JSON line per setting and a closing summary line; the bar is by_source <= handles at `--parts` parts.
Kernel times: run it under `rocprofv3 --kernel-trace --stats` with --repeats 2 --no-parity."""
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
from extension_bench import present_kmers, timed  # noqa: E402
from reads_build_bench import read_set  # noqa: E402


def cut(reads, nparts, builder):
    """The BWTs of the read set's parts (by read index)."""
    n, length = reads.shape
    flat, offsets = reads.reshape(-1), np.arange(n + 1, dtype=np.uint64) * np.uint64(length)
    cuts = [n * i // nparts for i in range(nparts + 1)]
    return [builder.build_from_reads((flat, offsets[lo:hi + 1])) for lo, hi in zip(cuts[:-1], cuts[1:])]


def spread(ms):
    t = sorted(ms)
    return {"median": round(float(np.median(t)), 3), "min": round(t[0], 3), "max": round(t[-1], 3)}


def run_setting(merged, handles, q, args, label, oracles):
    dev = q.device
    n, k = q.shape
    ns = merged.source_count()
    stream = torch.cuda.current_stream(dev).cuda_stream
    d_l = torch.empty(n, dtype=torch.int64, device=dev)
    d_h = torch.empty(n, dtype=torch.int64, device=dev)
    by = torch.empty((n, ns), dtype=torch.int64, device=dev)
    again = torch.empty((n, ns), dtype=torch.int64, device=dev)
    variants = {
        "ranges": lambda: merged.kmer_ranges_device(q.data_ptr(), k, n, d_l.data_ptr(), d_h.data_ptr(), stream),
        "by_source": lambda: merged.count_kmers_by_source_device(q.data_ptr(), k, n, by.data_ptr(), stream),
        "sources": lambda: merged.range_sources_device(d_l.data_ptr(), d_h.data_ptr(), n, again.data_ptr(), stream),
    }
    if handles:
        each = torch.empty((len(handles), n), dtype=torch.int64, device=dev)

        def all_handles():
            for i, h in enumerate(handles):
                h.count_kmers_device(q.data_ptr(), k, n, each[i].data_ptr(), stream)
        variants["handles"] = all_handles
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn in variants.values():  # warm-up: every shape once (and the ranges `sources` reads)
        fn()
    merged.device_status(stream)
    ms = {v: [] for v in variants}
    for _ in range(args.repeats):
        for v, fn in variants.items():
            ms[v].append(timed(fn, start, stop))
    merged.device_status(stream)
    res = {"label": label, "parts": ns, "n": n, "k": k, "sparse_depth": merged.get_sparse_table(), "table_depth": merged.get_table_depth(),
           "query_length": merged.get_query_length(), "source_index_bytes": msbwt.source_index_plan(merged.get_total_size(), ns)}
    for v, t in ms.items():
        res[v + "_ms"] = spread(t)
    res["phase2_ms"] = round(res["by_source_ms"]["median"] - res["ranges_ms"]["median"], 3)
    # the library's own invariants on the whole batch, on the device (32 sources make a 25 GB result)
    ok = torch.equal(by, again) and torch.equal(by.sum(dim=1), d_h - d_l)
    if handles:
        res["by_source_over_handles"] = round(res["by_source_ms"]["median"] / res["handles_ms"]["median"], 3)
        res["bar_met"] = res["by_source_ms"]["median"] <= res["handles_ms"]["median"]
        ok = ok and torch.equal(by, each.T)
    res["invariants_ok"] = bool(ok)
    if oracles:
        rng = np.random.default_rng(11)
        ids = torch.from_numpy(np.sort(rng.choice(n, size=min(n, args.parity_sample), replace=False))).to(dev)
        qs = np.ascontiguousarray(q[ids].cpu().numpy())
        got = by[ids].cpu().numpy().astype(np.uint64)
        want = np.stack([ref.count_kmers(qs, nthreads=args.threads) for ref in oracles], axis=1).astype(np.uint64)
        res["parity"] = {"checked": int(len(ids)), "mismatches": int((got != want).any(axis=1).sum())}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="c4")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--parts", type=int, default=4)
    ap.add_argument("--many", type=int, default=32, help="parts of the second, timing-only colouring (0: skip it)")
    ap.add_argument("--queries", type=int, default=100_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--parity-sample", type=int, default=2_000_000)
    ap.add_argument("--threads", type=int, default=16, help="threads of the CPU oracle")
    ap.add_argument("--no-parity", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("source_count_bench needs a GPU")
    dev = torch.device("cuda:0")
    reads = read_set(args.config, args.scale)
    k = 31
    builder = msbwt.RleBWT(device=0)
    q = present_kmers(reads, k, args.queries, 23, dev)
    lines = []
    for nparts in [args.parts] + ([args.many] if args.many else []):
        rles = cut(reads, nparts, builder)
        merged = msbwt.RleBWT(device=0)
        merged.load_merged_many(rles, keep_sources=True)
        first = nparts == args.parts
        handles = []
        for r in rles if first else []:  # the comparison: one handle per part
            handles.append(msbwt.RleBWT(device=0))
            handles[-1].load_vector(r)
        oracles = []
        if not args.no_parity:
            from oracle import oracle as orc
            for r in rles:
                oracles.append(orc.OracleRleBWT(8))
                oracles[-1].load_vector(r)
        for label in ("undeclared", "declared_k31"):
            if label == "declared_k31":
                for h in [merged] + handles:
                    h.set_query_length(31)
            res = run_setting(merged, handles, q, args, label, oracles)
            print(json.dumps(res), flush=True)
            lines.append(res)
        del merged, handles, oracles
    summary = {"config": args.config, "scale": args.scale, "symbols": int(reads.shape[0] * (reads.shape[1] + 1)),
               "bar_met": all(r["bar_met"] for r in lines if "bar_met" in r),
               "by_source_over_handles": [r["by_source_over_handles"] for r in lines if "bar_met" in r],
               "phase2_ms": {"%d parts, %s" % (r["parts"], r["label"]): r["phase2_ms"] for r in lines},
               "mismatches": sum(r["parity"]["mismatches"] for r in lines if "parity" in r), "invariants_ok": all(r["invariants_ok"] for r in lines)}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"lines": lines, "summary": summary}, f, indent=1)


if __name__ == "__main__":
    main()
