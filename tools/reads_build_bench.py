#!/usr/bin/env python3
"""The builder from reads (RleBWT.build_from_reads, csrc/reads_build.hip) against the host builder of the tree
(synth.build_msbwt_symbols + synth.rle_encode, 16 threads, the same box), on the read set of a synth.CONFIGS entry (default C4:
12.9 M reads of 150 bp with 0.5 % substitutions, 1.95e9 symbols at scale 1) at the given scales.

Per scale one JSON line: the GPU build's wall-clock time and its stages (host clock around stream synchronisations: copy in, read
order, histogram, collect, sort, emit, encode, copy out), the host builder's wall-clock time, and whether the two outputs are
byte-identical; with --second-piece, the same for a second GPU build under another piece limit.  A scale whose build does not fit the free HBM (msbwt_build_reads_plan, 2 bytes per symbol resident) is reported
as skipped.  Kernel times: run one scale with --no-host under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import rust_msbwt_amd as msbwt  # noqa: E402
import synth  # noqa: E402


def read_set(name, scale):
    cfg = synth.CONFIGS[name]
    g = max(int(cfg["genome"] * scale), 4 * cfg["rlen"])
    n = max(int(cfg["nreads"] * scale), 4)
    genome = synth.repeat_genome(g, cfg["gseed"]) if cfg.get("repeats") else synth.genome(g, cfg["gseed"])
    return synth.reads(genome, n, cfg["rlen"], cfg["rseed"], cfg["err"])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="c4")
    ap.add_argument("--scales", default="0.0625,0.25,1")
    ap.add_argument("--piece", type=int, default=0, help="piece limit in suffixes (0 = automatic)")
    ap.add_argument("--threads", type=int, default=16, help="threads of the host builder")
    ap.add_argument("--no-host", action="store_true", help="GPU build only (no comparison with the host builder)")
    ap.add_argument("--second-piece", type=int, default=0, help="build once more under this piece limit and compare the bytes")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    bwt = msbwt.RleBWT(device=args.device)
    bwt.set_build_piece(args.piece)
    bwt.build_from_reads([np.array([1, 2, 3, 5], dtype=np.uint8)])  # runtime, stream and code objects are up before anything is timed
    for scale in [float(s) for s in args.scales.split(",")]:
        reads = read_set(args.config, scale)
        n, length = reads.shape
        total = n * (length + 1)
        free, _ = torch.cuda.mem_get_info(args.device)
        piece, need = msbwt.build_reads_plan(total, free, args.piece)
        line = {"config": args.config, "scale": scale, "reads": n, "read_length": length, "symbols": total, "piece_limit": args.piece or piece,
                "plan_bytes": need, "free_hbm_bytes": free}
        if need > free:
            line["skipped"] = "the plan needs more HBM than is free"
            print(json.dumps(line), flush=True)
            continue
        pack = (reads.reshape(-1), np.arange(n + 1, dtype=np.uint64) * np.uint64(length))
        t0 = time.perf_counter()
        rle = bwt.build_from_reads(pack)
        line["gpu_seconds"] = round(time.perf_counter() - t0, 4)
        stages = bwt.build_stage_ms()
        line["pieces"] = stages.pop("pieces")
        line["gpu_stage_ms"] = {k: round(v, 2) for k, v in stages.items()}
        line["rle_bytes"] = int(rle.size)
        if not args.no_host:
            t0 = time.perf_counter()
            expected = synth.rle_encode(synth.build_msbwt_symbols(reads, args.threads))
            line["host_seconds"] = round(time.perf_counter() - t0, 4)
            line["host_threads"] = args.threads
            line["identical"] = bool(np.array_equal(rle, expected))
            line["speedup"] = round(line["host_seconds"] / line["gpu_seconds"], 2)
            del expected
        if args.second_piece:
            bwt.set_build_piece(args.second_piece)
            t0 = time.perf_counter()
            again = bwt.build_from_reads(pack)
            line["second"] = {"piece_limit": args.second_piece, "gpu_seconds": round(time.perf_counter() - t0, 4), "pieces": bwt.build_stage_ms()["pieces"],
                              "identical": bool(np.array_equal(rle, again))}
            bwt.set_build_piece(args.piece)
            del again
        print(json.dumps(line), flush=True)
        del rle, reads, pack


if __name__ == "__main__":
    main()
