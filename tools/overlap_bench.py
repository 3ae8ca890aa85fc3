#!/usr/bin/env python3
"""Read overlaps on the read set of a synth.CONFIGS entry (default C4: 12.9 M reads of 150 bp with 0.5 % substitutions, 1.95e9 symbols
at scale 1), built and loaded by load_reads, with the reads themselves as queries (all of them, or `--max-queries` taken evenly).  For
min_overlap 50 and 100, both strands, plane blocks and run blocks, `--repeats` rounds, the routes alternating within a round (median
and spread, wall clock around calls that end in a synchronise):
  count      read_overlaps_device without columns: one search
  fill       read_overlaps_device with columns of exactly R records: two searches
  host loop  the route a caller has without it: per symbol ONE constrain_ranges_device call on the live queries and, from min_overlap
             on, one more with symbol 0 -- [rank('$', l), rank('$', h)) is that call's answer --, the live queries picked out and the
             records compacted with torch ops on the device
All seven outputs of the two routes must be equal, word for word: a mismatch fails the tool.  One JSON line per setting with
overlap_info, the lines fetched per query and the lines per second of the counting call as a fraction of msbwt_rle_probe_line_rate
measured in the same session, and a closing summary line; no threshold on the times."""
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

END, EMPTY = 1, 2


def host_loop(b, queries, m, strand, stream):
    """(offsets, lengths, first, counts, matched, edges, stops) of n queries of one length, by constrain_ranges_device a symbol"""
    dev = queries.device
    n, L = queries.shape
    if strand:
        queries = torch.tensor([0, 5, 3, 2, 4, 1], dtype=torch.uint8, device=dev)[queries.flip(1).long()]
    total = b.get_total_size()

    def constrain(syms, l, h):
        out_l, out_h = torch.empty_like(l), torch.empty_like(h)
        b.constrain_ranges_device(syms.data_ptr(), l.data_ptr(), h.data_ptr(), l.numel(), out_l.data_ptr(), out_h.data_ptr(), stream)
        return out_l, out_h

    live = torch.arange(n, dtype=torch.int64, device=dev)
    l, h = torch.zeros(n, dtype=torch.int64, device=dev), torch.full((n,), total, dtype=torch.int64, device=dev)
    matched, edges = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
    stops = torch.zeros(n, dtype=torch.uint8, device=dev)
    found = []
    for j in range(L + 1):
        if j >= m:
            dl, dh = constrain(torch.zeros(live.numel(), dtype=torch.uint8, device=dev), l, h)
            has = dh > dl
            found.append((live[has], torch.full((int(has.sum()),), j, dtype=torch.int64, device=dev), dl[has], (dh - dl)[has]))
        if j == L:
            stops[live], matched[live] = END, L
            break
        nl, nh = constrain(queries[live, L - 1 - j].contiguous(), l, h)
        empty = nl >= nh
        stops[live[empty]], matched[live[empty]] = EMPTY, j
        live, l, h = live[~empty], nl[~empty], nh[~empty]
        if live.numel() == 0:  # (the host reads the live count: one decision a step)
            break
    query, lengths, first, counts = (torch.cat([f[i] for f in found]) if found else torch.zeros(0, dtype=torch.int64, device=dev) for i in range(4))
    order = torch.argsort(query * (L + 1) + lengths)
    query, lengths, first, counts = query[order], lengths[order], first[order], counts[order]
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(torch.bincount(query, minlength=n), 0)
    edges.index_add_(0, query, counts)
    return offsets, lengths, first, counts, matched, edges, stops


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="c4")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--min-overlaps", default="50,100")
    ap.add_argument("--strands", default="0,1")
    ap.add_argument("--blocks", default="planes,runs")
    ap.add_argument("--max-queries", type=int, default=0, help="queries at the most, taken evenly from the reads (0 = all reads)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("overlap_bench needs a GPU")
    if args.repeats < 5:
        sys.exit("a median of at least five calls")
    dev = torch.device("cuda:0")
    reads = read_set(args.config, args.scale)
    n_reads, length = reads.shape
    pick = np.arange(n_reads) if not args.max_queries or args.max_queries >= n_reads else np.linspace(0, n_reads - 1, args.max_queries).astype(np.int64)
    queries = torch.from_numpy(np.ascontiguousarray(reads[pick])).to(dev)
    n = queries.shape[0]
    q_offsets = torch.arange(n + 1, dtype=torch.int64, device=dev) * length
    stream = torch.cuda.current_stream(dev).cuda_stream
    lines, same = [], True
    for blocks in args.blocks.split(","):
        b = msbwt.RleBWT(device=0)
        b.set_block_format(blocks)
        (_, load_ms) = wall(lambda: b.load_reads((reads.reshape(-1), np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(length))))
        line_rate = b.probe_line_rate("blocks")
        for m in [int(x) for x in args.min_overlaps.split(",")]:
            for strand in [int(x) for x in args.strands.split(",")]:
                theirs = host_loop(b, queries, m, strand, stream)  # warm-up, and the comparison
                ours = b.read_overlaps_device(queries.view(-1), q_offsets, m, strand=strand)
                b.device_status(stream)
                R = int(ours.lengths.numel())
                ok = all(torch.equal(x, y) for x, y in zip((ours.offsets, ours.lengths, ours.first, ours.counts, ours.matched, ours.edges, ours.stops), theirs))
                del theirs
                calls = {"count": lambda: b.read_overlaps_device(queries.view(-1), q_offsets, m, strand=strand, records=False),
                         "fill": lambda: b.read_overlaps_device(queries.view(-1), q_offsets, m, strand=strand, capacity=R),
                         "host_loop": lambda: host_loop(b, queries, m, strand, stream)}
                ms = {route: [] for route in calls}
                for _ in range(args.repeats):  # alternating
                    for route, fn in calls.items():
                        _, t = wall(fn)
                        ms[route].append(t)
                calls["count"]()
                info = b.overlap_info()
                res = {"blocks": blocks, "min_overlap": m, "strand": strand, "n": n, "read_length": int(length), "symbols": int(b.get_total_size()), "load_reads_ms": round(load_ms, 1),
                       "info": info, "records": info["records"], "edges": info["edges"], "lines_per_query": round(info["lines"] / n, 2),
                       "count_ms": spread(ms["count"]), "fill_ms": spread(ms["fill"]), "host_loop_ms": spread(ms["host_loop"]), "same": bool(ok)}
                res["host_loop_over_fill"] = round(res["host_loop_ms"]["median"] / res["fill_ms"]["median"], 2)
                res["host_loop_over_count"] = round(res["host_loop_ms"]["median"] / res["count_ms"]["median"], 2)
                res["lines_per_s"] = round(info["lines"] / (res["count_ms"]["median"] * 1e-3), 0)
                res["probe_lines_per_s"] = round(line_rate, 0)
                res["fraction_of_probe"] = round(res["lines_per_s"] / line_rate, 3) if line_rate else None
                same = same and bool(ok)
                print(json.dumps(res), flush=True)
                lines.append(res)
                del ours
                torch.cuda.empty_cache()
        del b
        torch.cuda.empty_cache()
    key = lambda r: "%s/%d/%d" % (r["blocks"], r["min_overlap"], r["strand"])
    summary = {"config": args.config, "scale": args.scale, "n": n, "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
               "count_ms": {key(r): r["count_ms"]["median"] for r in lines}, "fill_ms": {key(r): r["fill_ms"]["median"] for r in lines},
               "host_loop_ms": {key(r): r["host_loop_ms"]["median"] for r in lines}, "same": same}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"lines": lines, "summary": summary}, f, indent=1)
    if not same:
        sys.exit("the host loop and the read-overlap call disagree")


if __name__ == "__main__":
    main()
