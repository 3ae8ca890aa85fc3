#!/usr/bin/env python3
"""The canonical k-mer spectrum and dump (a k-mer and its reverse complement as one class) on the read set of a synth.CONFIGS entry
(default C4: 12.9 M reads of 150 bp with 0.5 % substitutions, 1.95e9 symbols at scale 1) with every second read reverse-complemented,
built and loaded by load_reads.  For k = 21 and k = 31, `--repeats` rounds each (median and spread, wall clock around calls that
synchronise):
  canonical_spectrum   canonical_kmer_spectrum(k)                                   -- the histogram over the classes, nothing pruned
  plain_spectrum       kmer_spectrum(k) of the same run                             -- the walk alone
  count_1, count_2     enumerate_canonical_kmers_device(k, capacity 0), min_count 1 and 2 (the walk prunes at ceil(m / 2): not at all)
  dump                 enumerate_canonical_kmers_device(k, min_count=1) into buffers -- two walks, unsorted (there is no sorted form)
  search               count_kmers_packed_device on the reverse complements of the plain dump's words: the k-mers one canonical walk
                       stages, in one batch -- the packed search's rate on this index
  alternative          the route without these calls: enumerate_kmers_device (sorted, two walks), the records to the host,
                       reverse_complement_2bit, np.unique over min(word, rc word) with the counts summed, the histogram
Expectation, printed beside the measurement: canonical time ~ plain walk time + (k-mers staged) / (the search's rate) + the streaming
passes (per staged k-mer: 24 bytes read and 8 written for the reverse complements, 40 read for the classes).  One JSON line per k and a
closing summary line; no threshold."""
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
from spectrum_bench import spread, wall  # noqa: E402

BINS = 256
STREAM_BYTES_PER_KMER = 24 + 8 + 40
HBM_BYTES_PER_S = 4.0e12  # what streaming kernels reach on the card, for the expectation only
COMPLEMENT = np.array([0, 5, 3, 2, 4, 1], dtype=np.uint8)


def timed(fn, repeats):
    ms, out = [], None
    for _ in range(repeats):
        out, t = wall(fn)
        ms.append(t)
    return out, spread(ms)


def alternative_route(b, k, dev, stream):
    """plain device dump, the records to the host, host reverse complement, np.unique join"""
    n = b.enumerate_kmers_device(k, None, None, None, 0, stream=stream)
    bufs = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(2)]
    b.enumerate_kmers_device(k, bufs[0].data_ptr(), bufs[1].data_ptr(), None, n, stream=stream)
    b.device_status(stream)
    words, counts = (x.cpu().numpy().view(np.uint64) for x in bufs)
    canonical = np.minimum(words, msbwt.rle_bwt.reverse_complement_2bit(words, k))
    classes, inverse = np.unique(canonical, return_inverse=True)
    total = np.zeros(len(classes), dtype=np.uint64)
    np.add.at(total, inverse, counts)  # (a palindrome is one plain k-mer: counted once)
    hist = np.bincount(np.minimum(total, np.uint64(BINS - 1)).astype(np.int64), minlength=BINS).astype(np.uint64)
    return hist, len(classes), int(total.sum())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="c4")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--ks", default="21,31")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-alternative", action="store_true", help="skip the route through the plain dump and a host join")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("canonical_bench needs a GPU")
    dev = torch.device("cuda:0")
    reads = np.array(read_set(args.config, args.scale))
    reads[1::2] = COMPLEMENT[reads[1::2, ::-1]]
    n, length = reads.shape
    b = msbwt.RleBWT(device=0)
    (_, load_ms) = wall(lambda: b.load_reads((reads.reshape(-1), np.arange(n + 1, dtype=np.uint64) * np.uint64(length))))
    del reads
    stream = torch.cuda.current_stream(dev).cuda_stream
    lines = []
    for k in [int(x) for x in args.ks.split(",")]:
        res = {"k": k, "symbols": int(b.get_total_size()), "pair_index": b.get_pair_index(), "table_depth": b.get_table_depth(), "sparse_table": b.get_sparse_table()}
        (phist, pdistinct, poccurrences), res["plain_spectrum_ms"] = timed(lambda: b.kmer_spectrum(k, BINS), args.repeats)
        plain_info = b.spectrum_info()
        (hist, classes, occurrences), res["canonical_spectrum_ms"] = timed(lambda: b.canonical_kmer_spectrum(k, BINS), args.repeats)
        info = b.spectrum_info()
        staged = int(info["nodes"][k])
        res.update(classes=classes, occurrences=occurrences, plain_distinct=pdistinct, staged=staged, once=int(hist[1]), twice=int(hist[2]),
                   chunks=info["chunks"], retries=info["retries"], plain_chunks=plain_info["chunks"], plain_retries=plain_info["retries"],
                   same_occurrences=occurrences == poccurrences)
        for least in (1, 2):
            count, res["count_%d_ms" % least] = timed(lambda: b.enumerate_canonical_kmers_device(k, None, None, None, 0, min_count=least, stream=stream), args.repeats)
            res["classes_from_%d" % least] = count
        bufs = [torch.empty(classes, dtype=torch.int64, device=dev) for _ in range(3)]
        _, res["dump_ms"] = timed(lambda: b.enumerate_canonical_kmers_device(k, *[x.data_ptr() for x in bufs], classes, stream=stream), args.repeats)
        b.device_status(stream)
        del bufs
        # the search's rate on what one canonical walk stages: the reverse complements of every plain k-mer, in one batch
        words = torch.empty(pdistinct, dtype=torch.int64, device=dev)
        b.enumerate_kmers_device(k, words.data_ptr(), None, None, pdistinct, sorted=False, stream=stream)
        rc = torch.from_numpy(msbwt.rle_bwt.reverse_complement_2bit(words.cpu().numpy().view(np.uint64), k).view(np.int64)).to(dev)
        counts = torch.empty(pdistinct, dtype=torch.int64, device=dev)
        _, res["search_ms"] = timed(lambda: b.count_kmers_packed_device(rc.data_ptr(), k, pdistinct, counts.data_ptr(), stream), args.repeats)
        b.device_status(stream)
        del words, rc, counts
        torch.cuda.empty_cache()
        stream_ms = staged * STREAM_BYTES_PER_KMER / HBM_BYTES_PER_S * 1e3
        res["expected_ms"] = round(res["plain_spectrum_ms"]["median"] + res["search_ms"]["median"] * staged / max(pdistinct, 1) + stream_ms, 3)
        res["search_rate_per_s"] = round(pdistinct / (res["search_ms"]["median"] * 1e-3)) if res["search_ms"]["median"] else None
        if not args.no_alternative:
            (ahist, aclasses, aoccurrences), t = wall(lambda: alternative_route(b, k, dev, stream))
            res["alternative"] = {"ms": round(t, 3), "same_histogram": bool(np.array_equal(ahist, hist)) and aclasses == classes and aoccurrences == occurrences}
            torch.cuda.empty_cache()
        print(json.dumps(res), flush=True)
        lines.append(res)
    summary = {"config": args.config, "scale": args.scale, "load_reads_ms": round(load_ms, 1), "device": torch.cuda.get_device_name(0),
               "canonical_spectrum_ms": {r["k"]: r["canonical_spectrum_ms"]["median"] for r in lines},
               "expected_ms": {r["k"]: r["expected_ms"] for r in lines},
               "plain_spectrum_ms": {r["k"]: r["plain_spectrum_ms"]["median"] for r in lines},
               "alternative_ms": {r["k"]: r["alternative"]["ms"] for r in lines if "alternative" in r},
               "same_histogram": all(r["alternative"]["same_histogram"] for r in lines if "alternative" in r)}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"lines": lines, "summary": summary}, f, indent=1)


if __name__ == "__main__":
    main()
