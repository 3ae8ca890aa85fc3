#!/usr/bin/env python3
"""The merge of two BWTs (RleBWT.merge, csrc/merge.hip) against building the union from its reads (RleBWT.build_from_reads) on the
same card, on the read set of a synth.CONFIGS entry (default C4: 12.9 M reads of 150 bp with 0.5 % substitutions, 1.95e9 symbols at
scale 1) at the given scales.

Per scale: the read set is cut in half by read index, each half is built with build_from_reads, the two BWTs are merged, and the
result is compared byte for byte with the build of the whole.  One JSON line: the merge's wall-clock time and its six stages (host
clock around stream synchronisations: copy in, decode, iterate, emit, encode, copy out), the iterations, milliseconds per
iteration, the HBM bytes an iteration moves by the layout's own arithmetic and the rate that makes, and the build of the whole as
the comparison.  Every scale runs in a process of its own under --limit seconds; after one that fails or runs out of time no
further scale is started."""
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


def one(args, scale):
    import numpy as np
    import torch

    import rust_msbwt_amd as msbwt
    from reads_build_bench import read_set

    bwt = msbwt.RleBWT(device=args.device)
    tiny = bwt.build_from_reads([np.array([1, 2, 3, 5], dtype=np.uint8)])
    bwt.merge(tiny, tiny)  # runtime, stream and code objects are up before anything is timed
    reads = read_set(args.config, scale)
    n, length = reads.shape
    total = n * (length + 1)
    half = n // 2
    free, _ = torch.cuda.mem_get_info(args.device)
    need = msbwt.merge_plan(half * (length + 1), (n - half) * (length + 1))
    line = {"config": args.config, "scale": scale, "reads": n, "read_length": length, "symbols": total, "plan_bytes": need, "free_hbm_bytes": free}
    if max(need, msbwt.build_reads_plan(total, free)[1]) > free:
        line["skipped"] = "the plan needs more HBM than is free"
        return line
    flat, offsets = reads.reshape(-1), np.arange(n + 1, dtype=np.uint64) * np.uint64(length)
    t0 = time.perf_counter()
    whole = bwt.build_from_reads((flat, offsets))
    line["build_whole_seconds"] = round(time.perf_counter() - t0, 4)
    first, second = bwt.build_from_reads((flat, offsets[:half + 1])), bwt.build_from_reads((flat, offsets[half:]))
    t0 = time.perf_counter()
    merged = bwt.merge(first, second)
    line["merge_seconds"] = round(time.perf_counter() - t0, 4)
    info = bwt.merge_info()
    line["iterations"] = info.pop("iterations")
    line["merge_stage_ms"] = {k: round(v, 2) for k, v in info.items()}
    line["ms_per_iteration"] = round(info["iterate"] / max(line["iterations"], 1), 4)
    line["iteration_bytes"] = iteration_bytes(total, msbwt.merge_tile())
    line["iteration_tb_per_s"] = round(line["iteration_bytes"] / (line["ms_per_iteration"] * 1e-3) / 1e12, 3) if line["ms_per_iteration"] else None
    line["rle_bytes"] = int(merged.size)
    line["identical"] = bool(np.array_equal(merged, whole))
    line["merge_over_build"] = round(line["merge_seconds"] / line["build_whole_seconds"], 2)
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="c4")
    ap.add_argument("--scales", default="0.0625,0.25,1")
    ap.add_argument("--limit", type=float, default=300.0, help="seconds one scale may take")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--one", type=float, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one is not None:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        print(json.dumps(one(args, args.one)), flush=True)
        return 0
    for scale in [float(s) for s in args.scales.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--config", args.config, "--device", str(args.device), "--one", repr(scale)]
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({"config": args.config, "scale": scale, "failed": "no result within %g s" % args.limit}), flush=True)
            return 1
        if rc:
            print(json.dumps({"config": args.config, "scale": scale, "failed": "exit status %d" % rc}), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
