#!/usr/bin/env python3
"""Left-extension counts against the ways to get them, on C4 (synth.workload_index("c4"): the real MSBWT of 12.9 M reads with 0.5 %
substitutions, 1.95e9 symbols), device-resident batches of present 31-mers taken from the reads.  Timed with events, the variants
alternating, `--repeats` rounds each (median and spread):
  count      count_kmers_device of the batch
  ranges     kmer_ranges_device
  ext        count_kmer_extensions_device (the two-phase form: ranges into the 48-byte rows, then extend.hip)
  four       count_kmers_device of the 4 n ACGT (k+1)-mers c . q -- what a caller does without the extension call
Once as loaded (k undeclared) and once after set_query_length(31).  Parity of `ranges` and `ext` against the CPU oracle on a sample.
Prints one JSON line per depth setting and a closing summary line.  Kernel times: run it under `rocprofv3 --kernel-trace --stats`
with --repeats 2 --no-parity."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import rust_msbwt_amd as msbwt  # noqa: E402
import synth  # noqa: E402

ACGT = np.array([1, 2, 3, 5], dtype=np.uint8)


def present_kmers(reads, k, n, seed, dev):
    """n windows of the reads (read-derived: present), built on the device in slices"""
    rng = np.random.default_rng(seed)
    d_reads = torch.from_numpy(np.ascontiguousarray(reads)).to(dev)
    nreads, rlen = reads.shape
    out = torch.empty((n, k), dtype=torch.uint8, device=dev)
    cols = torch.arange(k, device=dev)
    step = 10_000_000
    for a in range(0, n, step):
        m = min(step, n - a)
        r = torch.from_numpy(rng.integers(0, nreads, size=m)).to(dev)
        o = torch.from_numpy(rng.integers(0, rlen - k + 1, size=m)).to(dev)
        out[a:a + m] = d_reads[r[:, None], o[:, None] + cols[None, :]]
    del d_reads
    return out


def four_extensions(q):
    """the 4 n rows c . q, c in A C G T (row 4 i + j = ACGT[j] . q_i)"""
    n, k = q.shape
    out = torch.empty((n, 4, k + 1), dtype=torch.uint8, device=q.device)
    for j, c in enumerate(ACGT):
        out[:, j, 0] = int(c)
        out[:, j, 1:] = q
    return out.reshape(4 * n, k + 1)


def timed(fn, start, stop):
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def run_depth(b, q, quad, args, label, ref):
    dev = q.device
    n, k = q.shape
    stream = torch.cuda.current_stream(dev).cuda_stream
    counts = torch.empty(n, dtype=torch.int64, device=dev)
    d_l = torch.empty(n, dtype=torch.int64, device=dev)
    d_h = torch.empty(n, dtype=torch.int64, device=dev)
    ext = torch.empty((n, 6), dtype=torch.int64, device=dev)
    quad_counts = torch.empty(quad.shape[0], dtype=torch.int64, device=dev)
    variants = {
        "count": lambda: b.count_kmers_device(q.data_ptr(), k, n, counts.data_ptr(), stream),
        "ranges": lambda: b.kmer_ranges_device(q.data_ptr(), k, n, d_l.data_ptr(), d_h.data_ptr(), stream),
        "ext": lambda: b.count_kmer_extensions_device(q.data_ptr(), k, n, ext.data_ptr(), stream),
        "four": lambda: b.count_kmers_device(quad.data_ptr(), k + 1, quad.shape[0], quad_counts.data_ptr(), stream),
    }
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn in variants.values():   # warm-up: every shape once
        fn()
    b.device_status(stream)
    ms = {v: [] for v in variants}
    for _ in range(args.repeats):
        for v, fn in variants.items():
            ms[v].append(timed(fn, start, stop))
    b.device_status(stream)
    res = {"label": label, "n": n, "k": k, "sparse_depth": b.get_sparse_table(), "table_depth": b.get_table_depth(),
           "query_length": b.get_query_length()}
    for v, t in ms.items():
        t = sorted(t)
        res[v + "_ms"] = {"median": round(float(np.median(t)), 3), "min": round(t[0], 3), "max": round(t[-1], 3)}
    med = {v: res[v + "_ms"]["median"] for v in variants}
    res["ext_over_count"] = round(med["ext"] / med["count"], 3)
    res["ext_over_four"] = round(med["ext"] / med["four"], 3)
    res["ranges_over_count"] = round(med["ranges"] / med["count"], 3)
    res["bar_met"] = res["ext_over_four"] <= 0.5 and res["ext_over_count"] <= 1.6
    # the library's own invariants on the whole batch
    c = counts.cpu().numpy().astype(np.uint64)
    e = ext.cpu().numpy().astype(np.uint64)
    lo, hi = d_l.cpu().numpy().astype(np.uint64), d_h.cpu().numpy().astype(np.uint64)
    four = quad_counts.cpu().numpy().astype(np.uint64).reshape(n, 4)
    res["invariants_ok"] = bool(np.array_equal(hi - lo, c) and np.array_equal(e.sum(axis=1), c) and np.array_equal(e[:, [1, 2, 3, 5]], four))
    if ref is not None:
        rng = np.random.default_rng(11)
        ids = np.sort(rng.choice(n, size=min(n, args.parity_sample), replace=False))
        qs = np.ascontiguousarray(q[torch.from_numpy(ids).to(dev)].cpu().numpy())
        ol = np.zeros(len(qs), dtype=np.uint64)
        oh = np.full(len(qs), ref.get_total_size(), dtype=np.uint64)
        for t in range(k):
            ol, oh = ref.constrain_ranges(np.ascontiguousarray(qs[:, k - 1 - t]), ol, oh)
        empty = ol == oh
        ol[empty] = 0
        oh[empty] = 0
        oext = np.stack([ref.count_kmers(np.ascontiguousarray(np.hstack([np.full((len(qs), 1), s, dtype=np.uint8), qs]))) for s in range(6)], axis=1)
        bad = (lo[ids] != ol) | (hi[ids] != oh) | (e[ids] != oext.astype(np.uint64)).any(axis=1)
        res["parity"] = {"checked": int(len(ids)), "mismatches": int(bad.sum())}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workload", default="c4")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--queries", type=int, default=100_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--parity-sample", type=int, default=2_000_000)
    ap.add_argument("--no-parity", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("extension_bench needs a GPU")
    dev = torch.device("cuda:0")
    npy, reads = synth.workload_index(args.workload, args.scale)
    k = 31
    b = msbwt.RleBWT()
    b.load_numpy_file(npy)
    ref = None
    if not args.no_parity:
        from oracle import oracle as orc
        ref = orc.OracleRleBWT(8)
        ref.load_numpy_file(npy)
    q = present_kmers(reads, k, args.queries, 23, dev)
    quad = four_extensions(q)
    lines = []
    for label in ("undeclared", "declared_k31"):
        if label == "declared_k31":
            b.set_query_length(31)
        r = run_depth(b, q, quad, args, label, ref)
        print(json.dumps(r), flush=True)
        lines.append(r)
    summary = {"workload": args.workload, "total": b.get_total_size(), "bar_met": all(r["bar_met"] for r in lines),
               "ext_over_count": [r["ext_over_count"] for r in lines], "ext_over_four": [r["ext_over_four"] for r in lines]}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"lines": lines, "summary": summary}, f, indent=1)


if __name__ == "__main__":
    main()
