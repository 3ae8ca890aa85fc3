#!/usr/bin/env python3
"""Left walks on the read set of a synth.CONFIGS entry (default C4: 12.9 M reads of 150 bp with 0.5 % substitutions, 1.95e9 symbols at
scale 1), built and loaded by load_reads:
  locate    walk_rows_device without symbols from 10^6 and 10^7 pseudo-random rows, max_steps = the read length
  walk      walk_rows_device with symbols from 10^6 pseudo-random rows at max_steps = 31 and 150
  extract   extract_reads_device of all reads into n x max_len symbols (one walk)
each beside the route a caller had without these calls, timed in the same rounds (`--repeats` rounds, the two routes alternating,
median and spread of wall clock around calls that end in a synchronise):
  host loop bench.py:walk_kmers's scheme widened to six symbols: per step one constrain_ranges_device call a symbol on the one-row
            ranges [r, r + 1) of the live walks -- the symbol whose range keeps the row is the row's, its l is LF --, the decision in
            torch on the device, the live walks picked out with a boolean mask; extraction turns the rows round with torch ops.
All outputs of the two routes must be equal, word for word: a mismatch fails the tool.  One JSON line per setting with walk_info, the
steps per second, and what msbwt_rle_probe_line_rate says random lines of the same block array are served at in the same session --
one step is one line, so that is the ceiling --, and a closing summary line; no threshold on the times."""
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

DOLLAR, MAX_STEPS = 1, 2


def host_loop(b, rows, max_steps, want_symbols, stream, scratch):
    """(symbols or None, steps, stops, last, reads) by six constrain_ranges_device calls a step and torch ops between them"""
    dev, n = rows.device, rows.numel()
    syms, ol, oh = scratch
    symbols = torch.zeros((n, max_steps), dtype=torch.uint8, device=dev) if want_symbols else None
    steps, last, reads = torch.zeros(n, dtype=torch.int64, device=dev), rows.clone(), torch.full((n,), -1, dtype=torch.int64, device=dev)
    stops = torch.zeros(n, dtype=torch.uint8, device=dev)
    idx, cur = torch.arange(n, device=dev), rows.clone()
    for t in range(max_steps + 1):
        m = idx.numel()  # (the host reads the live count: one decision a step)
        if m == 0:
            break
        h = cur + 1
        sym = torch.full((m,), 255, dtype=torch.uint8, device=dev)
        nxt = torch.zeros(m, dtype=torch.int64, device=dev)
        for s in range(6):
            b.constrain_ranges_device(syms[s].data_ptr(), cur.data_ptr(), h.data_ptr(), m, ol.data_ptr(), oh.data_ptr(), stream)
            hit = (oh[:m] - ol[:m]) == 1
            sym = torch.where(hit, syms[s][:m], sym)
            nxt = torch.where(hit, ol[:m], nxt)
        dollar = sym == 0
        at = idx[dollar]
        stops[at], reads[at], last[at] = DOLLAR, nxt[dollar], cur[dollar]
        keep = ~dollar
        if t == max_steps:
            stops[idx[keep]], last[idx[keep]] = MAX_STEPS, cur[keep]
            break
        idx, cur, sym = idx[keep], nxt[keep].contiguous(), sym[keep]
        if want_symbols:
            symbols[idx, t] = sym
        steps[idx] += 1
        last[idx] = cur
    return symbols, steps, stops, last, reads


def host_extract(b, n_reads, max_len, stream, scratch):
    """(symbols, offsets) in reading order from the host loop's rows"""
    dev = scratch[1].device
    symbols, steps, _, _, _ = host_loop(b, torch.arange(n_reads, dtype=torch.int64, device=dev), max_len, True, stream, scratch)
    offsets = torch.zeros(n_reads + 1, dtype=torch.int64, device=dev)
    torch.cumsum(steps, 0, out=offsets[1:])
    place = torch.arange(max_len, device=dev)[None, :] >= (max_len - steps)[:, None]  # the symbols of a row turned round stand at its end
    return symbols.flip(1)[place], offsets


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="c4")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--locate", default="1000000,10000000", help="rows of the locate settings")
    ap.add_argument("--walk-rows", type=int, default=10 ** 6)
    ap.add_argument("--walk-steps", default="31,150")
    ap.add_argument("--max-reads", type=int, default=0, help="extract this many reads at the most (0 = all)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("left_walk_bench needs a GPU")
    if args.repeats < 5:
        sys.exit("a median of at least five calls")
    dev = torch.device("cuda:0")
    reads = read_set(args.config, args.scale)
    n_reads, length = reads.shape
    b = msbwt.RleBWT(device=0)
    (_, load_ms) = wall(lambda: b.load_reads((reads.reshape(-1), np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(length))))
    del reads
    total = b.get_total_size()
    stream = torch.cuda.current_stream(dev).cuda_stream
    line_rate = b.probe_line_rate("blocks")
    rng = np.random.default_rng(17)
    lines, same = [], True
    biggest = max([int(x) for x in args.locate.split(",")] + [args.walk_rows, min(n_reads, args.max_reads or n_reads)])
    scratch = ([torch.full((biggest,), s, dtype=torch.uint8, device=dev) for s in range(6)], torch.empty(biggest, dtype=torch.int64, device=dev),
               torch.empty(biggest, dtype=torch.int64, device=dev))

    def measure(what, n, max_steps, ours, theirs, compare):
        nonlocal same
        want = theirs()  # warm-up, and the comparison
        got = ours()
        b.device_status(stream)
        ok = compare(got, want)
        del want, got
        ms = {"ours": [], "host_loop": []}
        for _ in range(args.repeats):  # alternating
            for route, fn in (("ours", ours), ("host_loop", theirs)):
                _, t = wall(fn)
                ms[route].append(t)
        ours()
        info = b.walk_info()
        res = {"what": what, "n": n, "max_steps": max_steps, "symbols_in_index": int(total), "block_format": b.get_block_format(), "info": info,
               "ours_ms": spread(ms["ours"]), "host_loop_ms": spread(ms["host_loop"]), "same": bool(ok)}
        lines_fetched = info["steps"] + info["dollar"] + info["max_steps"]  # a step is a line; so is the look that ends a walk
        res["host_loop_over_ours"] = round(res["host_loop_ms"]["median"] / res["ours_ms"]["median"], 2)
        res["steps_per_s"] = round(info["steps"] / (res["ours_ms"]["median"] * 1e-3), 0)
        res["lines_per_s"] = round(lines_fetched / (res["ours_ms"]["median"] * 1e-3), 0)
        res["probed_lines_per_s"] = round(line_rate, 0)
        res["fraction_of_probed_line_rate"] = round(res["lines_per_s"] / line_rate, 3) if line_rate else None
        same = same and bool(ok)
        print(json.dumps(res), flush=True)
        lines.append(res)
        torch.cuda.empty_cache()

    def equal(got, want):
        return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(got, want))

    def walk_setting(what, n, max_steps, want_symbols):
        rows = torch.from_numpy(rng.integers(0, total, size=n, dtype=np.int64)).to(dev)
        outs = [torch.zeros((n, max_steps), dtype=torch.uint8, device=dev) if want_symbols else None] + [torch.zeros(n, dtype=t, device=dev) for t in
                                                                                                          (torch.int64, torch.uint8, torch.int64, torch.int64)]

        def ours():
            b.walk_rows_device(rows.data_ptr(), n, max_steps, *[None if t is None else t.data_ptr() for t in outs], stream=stream)
            return outs
        measure(what, n, max_steps, ours, lambda: host_loop(b, rows, max_steps, want_symbols, stream, scratch), equal)

    for n in [int(x) for x in args.locate.split(",")]:
        walk_setting("locate", n, length, False)
    for max_steps in [int(x) for x in args.walk_steps.split(",")]:
        walk_setting("walk", args.walk_rows, max_steps, True)

    n = min(n_reads, args.max_reads or n_reads)
    symbols, offsets = torch.empty(n * length, dtype=torch.uint8, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev)

    def extract():
        S, truncated = b.extract_reads_device(None, 0, n, length, symbols.data_ptr(), offsets.data_ptr(), n * length, stream=stream)
        assert truncated == 0
        return symbols[:S], offsets
    measure("extract", n, length, extract, lambda: host_extract(b, n, length, stream, scratch), equal)

    summary = {"config": args.config, "scale": args.scale, "load_reads_ms": round(load_ms, 1), "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
               "symbols_in_index": int(total), "probed_lines_per_s": round(line_rate, 0),
               "ours_ms": {"%s/%d/%d" % (r["what"], r["n"], r["max_steps"]): r["ours_ms"]["median"] for r in lines},
               "host_loop_ms": {"%s/%d/%d" % (r["what"], r["n"], r["max_steps"]): r["host_loop_ms"]["median"] for r in lines},
               "fraction_of_probed_line_rate": {"%s/%d/%d" % (r["what"], r["n"], r["max_steps"]): r["fraction_of_probed_line_rate"] for r in lines}, "same": same}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"lines": lines, "summary": summary}, f, indent=1)
    if not same:
        sys.exit("the host loop and the left-walk calls disagree")


if __name__ == "__main__":
    main()
