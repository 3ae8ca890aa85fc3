#!/usr/bin/env python3
"""The merge of BWTs (RleBWT.merge, csrc/merge.hip; RleBWT.merge_many, csrc/merge_many.hip) against building the union from its
reads (RleBWT.build_from_reads) on the same card, on the read set of a synth.CONFIGS entry (default C4: 12.9 M reads of 150 bp with
0.5 % substitutions, 1.95e9 symbols at scale 1) at the given scales.

Per scale and part count (--parts, default 2): the read set is cut into that many parts by read index, each part is built with
build_from_reads, the parts are merged once by the balanced tree of pairwise merge calls (with two parts: one merge) and once by
merge_many in one pass, and both results are compared byte for byte with the build of the whole.  One JSON line: for either way the
wall-clock time and the six stages (host clock around stream synchronisations: copy in, decode, iterate, emit, encode, copy out; the
tree's are summed over its merges), the iterations, milliseconds per iteration, the HBM bytes an iteration moves by the layout's own
arithmetic and the rate that makes (an MI355X's HBM peaks at 8 TB/s), and the build of the whole as the comparison.  Every case
runs in a process of its own under --limit seconds; after one that fails or runs out of time no further case is started."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def iteration_bytes(rows, tile):
    """HBM traffic of one iteration: both passes over the tiles read a symbol per row; the vector is read by the tile counts, the
    histogram, the scatter and twice by the comparison, cleared and written once; a tile's seven counts are written, scanned and read."""
    tiles = -(-rows // tile)
    return rows * 2 + rows * 7 // 8 + tiles * 7 * 8 * 3


def iteration_bytes_many(rows, tile, inputs):
    """HBM traffic of one iteration of the one-pass merge: both passes over the tiles read a symbol per row; the source array, a byte
    per row, is read by the input counts and by the scatter, read once more where the rows go for the comparison, and written once; a
    tile's inputs + 6 counts are written, scanned and read."""
    tiles = -(-rows // tile)
    return rows * 2 + rows * 4 + tiles * (inputs + 6) * 8 * 3


def tree_merge(bwt, parts):
    """The balanced tree of pairwise merges (bwt_util.merge_numpy_files, method="tree"): (merged, iterations, stage ms) summed over
    its merges."""
    level, iterations, stages = list(parts), 0, {}
    while len(level) > 1:
        merged = []
        for i in range(0, len(level) - 1, 2):
            merged.append(bwt.merge(level[i], level[i + 1]))
            info = bwt.merge_info()
            iterations += info.pop("iterations")
            for k, v in info.items():
                stages[k] = stages.get(k, 0.0) + v
        level = merged + ([level[-1]] if len(level) % 2 else [])
    return level[0], iterations, stages


def one(args, scale, nparts):
    import numpy as np
    import torch

    import rust_msbwt_amd as msbwt
    from reads_build_bench import read_set

    bwt = msbwt.RleBWT(device=args.device)
    tiny = bwt.build_from_reads([np.array([1, 2, 3, 5], dtype=np.uint8)])
    bwt.merge(tiny, tiny)  # runtime, stream and code objects are up before anything is timed
    bwt.merge_many([tiny, tiny, tiny])
    reads = read_set(args.config, scale)
    n, length = reads.shape
    total = n * (length + 1)
    cuts = [n * i // nparts for i in range(nparts + 1)]
    sizes = [(hi - lo) * (length + 1) for lo, hi in zip(cuts[:-1], cuts[1:])]
    free, _ = torch.cuda.mem_get_info(args.device)
    need = msbwt.merge_plan(sum(sizes[:(nparts + 1) // 2]), sum(sizes[(nparts + 1) // 2:]))  # the tree's last merge
    need_many = msbwt.merge_many_plan(sizes)
    line = {"config": args.config, "scale": scale, "parts": nparts, "reads": n, "read_length": length, "symbols": total, "plan_bytes": need,
            "one_pass_plan_bytes": need_many, "free_hbm_bytes": free}
    if max(need, need_many, msbwt.build_reads_plan(total, free)[1]) > free:
        line["skipped"] = "the plan needs more HBM than is free"
        return line
    flat, offsets = reads.reshape(-1), np.arange(n + 1, dtype=np.uint64) * np.uint64(length)
    t0 = time.perf_counter()
    whole = bwt.build_from_reads((flat, offsets))
    line["build_whole_seconds"] = round(time.perf_counter() - t0, 4)
    parts = [bwt.build_from_reads((flat, offsets[lo:hi + 1])) for lo, hi in zip(cuts[:-1], cuts[1:])]
    tile = msbwt.merge_tile()

    def report(prefix, seconds, merged, iterations, stages, moved):
        line[prefix + "seconds"] = round(seconds, 4)
        line[prefix.replace("merge_", "") + "iterations"] = iterations
        line[prefix + "stage_ms"] = {k: round(v, 2) for k, v in stages.items()}
        per = stages["iterate"] / max(iterations, 1)
        line[prefix.replace("merge_", "") + "ms_per_iteration"] = round(per, 4)
        line[prefix.replace("merge_", "") + "iteration_bytes"] = moved
        line[prefix.replace("merge_", "") + "iteration_tb_per_s"] = round(moved / (per * 1e-3) / 1e12, 3) if per and moved else None
        line[prefix.replace("merge_", "") + "identical"] = bool(np.array_equal(merged, whole))

    # the tree of pairwise merges (with two parts: one merge; with more its merges are of different sizes: no bytes per iteration)
    t0 = time.perf_counter()
    merged, iterations, stages = tree_merge(bwt, parts)
    report("merge_", time.perf_counter() - t0, merged, iterations, stages, iteration_bytes(total, tile) if nparts == 2 else None)
    line["rle_bytes"] = int(merged.size)
    line["merge_over_build"] = round(line["merge_seconds"] / line["build_whole_seconds"], 2)
    # the same parts in one pass
    t0 = time.perf_counter()
    merged = bwt.merge_many(parts)
    seconds = time.perf_counter() - t0
    info = bwt.merge_info()
    report("one_pass_merge_", seconds, merged, info.pop("iterations"), info, iteration_bytes_many(total, tile, nparts))
    line["one_pass_over_tree"] = round(line["one_pass_merge_seconds"] / line["merge_seconds"], 3)
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="c4")
    ap.add_argument("--scales", default="0.0625,0.25,1")
    ap.add_argument("--parts", default="2", help="how many parts the read set is cut into, by read index (a list: one case per entry)")
    ap.add_argument("--limit", type=float, default=300.0, help="seconds one case may take")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--one", type=float, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one is not None:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        print(json.dumps(one(args, args.one, int(args.parts))), flush=True)
        return 0
    for scale in [float(s) for s in args.scales.split(",")]:
        for nparts in [int(p) for p in args.parts.split(",")]:
            cmd = [sys.executable, os.path.abspath(__file__), "--config", args.config, "--device", str(args.device), "--parts", str(nparts), "--one", repr(scale)]
            case = {"config": args.config, "scale": scale, "parts": nparts}
            try:
                rc = subprocess.run(cmd, timeout=args.limit).returncode
            except subprocess.TimeoutExpired:
                print(json.dumps(dict(case, failed="no result within %g s" % args.limit)), flush=True)
                return 1
            if rc:
                print(json.dumps(dict(case, failed="exit status %d" % rc)), flush=True)
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
