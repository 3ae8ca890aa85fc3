#!/usr/bin/env python3
"""The k-mers by source (one spectrum per input of a merged index, the dump filtered by per-source counts) on the read set of a
synth.CONFIGS entry (default C4: 12.9 M reads of 150 bp with 0.5 % substitutions, 1.95e9 symbols at scale 1) cut by read index into
`--parts` (4,32) parts, each built on the device, merged and loaded by load_merged_many(keep_sources=True).  For k = 21 and k = 31,
`--repeats` rounds each (median and spread, wall clock around calls that synchronise):
  by_source_spectrum   kmer_spectrum_by_source(k)            -- S histograms and the sharing tallies, nothing pruned
  plain_spectrum       kmer_spectrum(k) of the same index    -- the walk alone
  private_count/_dump  ">= 2 in part 0, absent elsewhere": enumerate_kmers_by_source_device with capacity 0, then into buffers (two walks)
  shared_count/_dump   "present in all parts": the same
  composition          what the fused dump replaces, in the same run on the same card: enumerate_kmers_device with ranges (two walks)
                       -> range_sources_device -> a torch predicate and compaction, `--repeats` rounds like the others (its buffers come
                       from torch's caching allocator, warm from the second round on: read the minimum beside the median).  The count
                       matrix n x S x 8 bytes is used whole where it fits in half the free HBM, else row slices of it ("sliced": true).
  reached / passed     the k-mers the last level handed to the sink against those the predicate let through: what per-source pruning
                       at inner levels could save
Expectation, printed beside the measurement: by-source time ~ plain walk time + the sink's source-vector traffic -- per k-mer its 24
staged bytes and the 16-byte chunks of its range (two 128-byte checkpoint lines and up to 2 KB of block prefix for a range wider than
the narrow limit), as if every one were a random line at RANDOM_LINES_PER_S -- an ASSUMED rate, not one measured for this kernel: the
estimate is a ceiling that ignores every cache.  One JSON line per (parts, k) and a closing summary line; no
threshold."""
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
from reads_build_bench import read_set  # noqa: E402
from source_count_bench import cut  # noqa: E402
from spectrum_bench import spread, wall  # noqa: E402

BINS = 256
NO_LIMIT = (1 << 64) - 1
RANDOM_LINES_PER_S = 6.0e9  # assumed, not measured: 128-byte lines a kernel fetches at random on the card; for the expectation only


def note(text):
    print(text, file=sys.stderr, flush=True)


def timed(fn, repeats):
    ms, out = [], None
    for _ in range(repeats):
        out, t = wall(fn)
        ms.append(t)
    return out, spread(ms)


def fused(b, k, lo, hi, dev, stream, repeats):
    """count, then dump: (n, count ms, dump ms, reached, (words, counts))"""
    n, count_ms = timed(lambda: b.enumerate_kmers_by_source_device(k, None, None, None, 0, lo, hi, stream=stream), repeats)
    reached = int(b.spectrum_info()["nodes"][k])
    S = b.source_count()
    words = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    counts = torch.empty((max(n, 1), S), dtype=torch.int64, device=dev)
    _, dump_ms = timed(lambda: b.enumerate_kmers_by_source_device(k, words.data_ptr(), counts.data_ptr(), None, n, lo, hi, stream=stream), repeats)
    b.device_status(stream)
    return n, count_ms, dump_ms, reached, (words[:n], counts[:n])


def composition(b, k, lo, hi, dev, stream):
    """plain dump with ranges -> range_sources -> predicate and compaction on the device: (words, counts, sliced)"""
    S = b.source_count()
    n = b.enumerate_kmers_device(k, None, None, None, 0, stream=stream)
    words, counts, l = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(3))
    b.enumerate_kmers_device(k, words.data_ptr(), counts.data_ptr(), l.data_ptr(), n, stream=stream)
    h = l + counts
    del counts
    free = torch.cuda.mem_get_info(0)[0]
    rows = n if n * S * 8 * 2 < free else max(1, free // (S * 8 * 4))
    lo_t = torch.tensor([int(x) for x in lo], dtype=torch.int64, device=dev)
    hi_t = torch.tensor([(1 << 62) if x is None else int(x) for x in hi], dtype=torch.int64, device=dev)
    kept_words, kept_counts = [], []
    for first in range(0, n, rows):
        m = min(rows, n - first)
        by = torch.empty((m, S), dtype=torch.int64, device=dev)
        b.range_sources_device(l[first:].data_ptr(), h[first:].data_ptr(), m, by.data_ptr(), stream)
        keep = ((by >= lo_t) & (by <= hi_t)).all(dim=1)
        kept_words.append(words[first:first + m][keep])
        kept_counts.append(by[keep])
        del by, keep
    b.device_status(stream)
    return torch.cat(kept_words), torch.cat(kept_counts), rows < n


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="c4")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--parts", default="4,32")
    ap.add_argument("--ks", default="21,31")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-composition", action="store_true", help="skip the route through the plain dump and range_sources")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("source_spectrum_bench needs a GPU")
    dev = torch.device("cuda:0")
    reads = read_set(args.config, args.scale)
    note("read set: %d reads of %d" % reads.shape)
    builder = msbwt.RleBWT(device=0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    narrow = msbwt.source_narrow_rows()
    lines = []
    for S in [int(x) for x in args.parts.split(",")]:
        rles = cut(reads, S, builder)
        b = msbwt.RleBWT(device=0)
        (_, load_ms) = wall(lambda: b.load_merged_many(rles, keep_sources=True))
        del rles
        note("%d parts merged and loaded in %.0f ms" % (S, load_ms))
        predicates = {"private": ([2] + [0] * (S - 1), [None] + [0] * (S - 1)), "shared": ([1] * S, [None] * S)}
        for k in [int(x) for x in args.ks.split(",")]:
            res = {"parts": S, "k": k, "symbols": int(b.get_total_size()), "load_merged_many_ms": round(load_ms, 1)}
            (phist, pdistinct, poccurrences), res["plain_spectrum_ms"] = timed(lambda: b.kmer_spectrum(k, BINS), args.repeats)
            (hist, sharing, distinct, occurrences), res["by_source_spectrum_ms"] = timed(lambda: b.kmer_spectrum_by_source(k, BINS), args.repeats)
            info = b.spectrum_info()
            wide = int(phist[narrow + 1:].sum()) if narrow + 1 < BINS else 0
            # lines the sink touches: per k-mer one of its staged record, one or two of its range's bytes; a wide one two checkpoint lines (four from 17 sources on) and its block prefixes
            sink_lines = pdistinct * 2.2 + wide * (2 * (2 if S > 16 else 1) + 16)
            res.update(kmers=pdistinct, distinct_per_part=[int(x) for x in distinct], sharing=[int(x) for x in sharing], chunks=info["chunks"], retries=info["retries"],
                       wider_than_narrow=wide, sums_agree=int(sharing.sum()) == pdistinct and int(occurrences.sum()) == poccurrences,
                       expected_extra_ms=round(sink_lines / RANDOM_LINES_PER_S * 1e3, 3),
                       extra_ms=round(res["by_source_spectrum_ms"]["median"] - res["plain_spectrum_ms"]["median"], 3))
            note("  k = %d: spectrum %.1f ms, by source %.1f ms" % (k, res["plain_spectrum_ms"]["median"], res["by_source_spectrum_ms"]["median"]))
            for name, (lo, hi) in predicates.items():
                n, count_ms, dump_ms, reached, (words, counts) = fused(b, k, lo, hi, dev, stream, args.repeats)
                res[name] = {"passed": n, "reached": reached, "count_ms": count_ms, "dump_ms": dump_ms}
                note("  k = %d, %s: %d of %d pass, count %.1f ms, dump %.1f ms" % (k, name, n, reached, count_ms["median"], dump_ms["median"]))
                if not args.no_composition:
                    (cwords, ccounts, sliced), t = timed(lambda: composition(b, k, lo, hi, dev, stream), args.repeats)
                    res[name]["composition"] = {"ms": t, "sliced": bool(sliced), "matrix_bytes": pdistinct * S * 8,
                                                "same_records": bool(torch.equal(cwords, words) and torch.equal(ccounts, counts))}
                    note("    composition %.1f ms (%.1f .. %.1f)%s" % (t["median"], t["min"], t["max"], ", sliced" if sliced else ""))
                    del cwords, ccounts
                del words, counts
                torch.cuda.empty_cache()
            print(json.dumps(res), flush=True)
            lines.append(res)
        del b
        torch.cuda.empty_cache()
    key = lambda r: "%d parts, k = %d" % (r["parts"], r["k"])
    summary = {"config": args.config, "scale": args.scale, "device": torch.cuda.get_device_name(0),
               "by_source_spectrum_ms": {key(r): r["by_source_spectrum_ms"]["median"] for r in lines},
               "plain_spectrum_ms": {key(r): r["plain_spectrum_ms"]["median"] for r in lines},
               "private_dump_ms": {key(r): r["private"]["dump_ms"]["median"] for r in lines},
               "shared_dump_ms": {key(r): r["shared"]["dump_ms"]["median"] for r in lines},
               "composition_ms": {key(r): {p: r[p]["composition"]["ms"]["median"] for p in ("private", "shared")} for r in lines if "composition" in r["private"]},
               "reached_over_passed": {key(r): {p: [r[p]["reached"], r[p]["passed"]] for p in ("private", "shared")} for r in lines},
               "same_records": all(r[p]["composition"]["same_records"] for r in lines for p in ("private", "shared") if "composition" in r[p]),
               "sums_agree": all(r["sums_agree"] for r in lines)}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"lines": lines, "summary": summary}, f, indent=1)


if __name__ == "__main__":
    main()
