#!/usr/bin/env python3
"""Traces on the read set of a synth.CONFIGS entry (default C4: 12.9 M reads of 150 bp with 0.5 % substitutions, 1.95e9 symbols at
scale 1), built and loaded by load_reads.  For k = 21 and 31, the three modes, both directions and max_steps = 100 and 2000, from two
seed sets -- (a) the first k-mers of the unitigs of enumerate_unitigs(k, min_count=2), (b) 10^6 k-mers taken evenly from
enumerate_kmers(k), each capped at `--max-seeds` -- `--repeats` rounds each, the two routes alternating within a round (median and
spread, wall clock around calls that end in a synchronise):
  trace      trace_kmers_device: all six outputs into device buffers
  host loop  the route a caller has without it: per step ONE count_kmers_packed_device call on queries built with torch ops -- the 4
             edges of every live walk's candidate and, in unitig mode, the 4 of its back-fan --, the decision in torch on the device,
             and the live walks picked out with a boolean mask, whose size the host reads: the same rounds, written by a caller
All six outputs of the two routes must be equal, word for word: a mismatch fails the tool.  One JSON line per setting with trace_info
and the queries per second of the search inside the rounds, and a closing summary line; no threshold on the times.

--canonical: the same for trace_canonical_kmers_device, on the read set with every second read reverse-complemented.  The seed sets are
the first k-mers of enumerate_canonical_unitigs(k, min_count=2) and 10^6 k-mers of enumerate_canonical_kmers(k); the host loop searches
every query and its reverse complement -- TWO count_kmers_packed_device calls a step, folded in torch (a third for the far ends where k
is even and min_count >= 2) -- and a third route, `plain`, is trace_kmers_device on the same index and seeds: the strand-specific
walk, which answers another question with half the searches a live walk, for the ratio of the two calls' times."""
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

MODES = {"unique": 0, "unitig": 1, "greedy": 2}
DIRECTIONS = {"right": 0, "left": 1}
DEAD_END, BRANCH, MERGE, RETURNED, TARGET, MAX_STEPS, NOT_A_NODE, MIRROR = range(1, 9)


def edge_words(w, k, left):
    """(m, 4) int64: the four edges out of the nodes w in the walk direction (the header's table; int64 holds the bit pattern)"""
    c = torch.arange(4, dtype=torch.int64, device=w.device)[None, :]
    return (c << (2 * k)) | w[:, None] if left else (w[:, None] << 2) | c


def next_nodes(w, k, left):
    """(m, 4) int64: the nodes at the other end of edge_words"""
    c = torch.arange(4, dtype=torch.int64, device=w.device)[None, :]
    return (c << (2 * (k - 1))) | (w[:, None] >> 2) if left else ((w[:, None] << 2) | c) & ((1 << (2 * k)) - 1)


def reverse_complement(w, length):
    """packed reverse complements of words of `length` symbols (int64 holds the bit pattern: every shift right is masked)"""
    for shift, mask in ((2, 0x3333333333333333), (4, 0x0F0F0F0F0F0F0F0F), (8, 0x00FF00FF00FF00FF), (16, 0x0000FFFF0000FFFF), (32, 0x00000000FFFFFFFF)):
        w = ((w >> shift) & mask) | ((w & mask) << shift)
    w = ~w
    return w if length == 32 else (w >> (64 - 2 * length)) & ((1 << (2 * length)) - 1)


def host_loop(b, seeds, k, max_steps, mode, direction, m, me, stream, canonical=False):
    """the six outputs by one packed count call a step (canonical: two, a word and its reverse complement) and torch ops between them"""
    dev, n = seeds.device, seeds.numel()
    left, unitig, greedy = direction == "left", mode == "unitig", mode == "greedy"
    mask = (1 << (2 * k)) - 1
    code = torch.tensor([1, 2, 3, 5], dtype=torch.uint8, device=dev)
    bit = torch.tensor([1, 2, 4, 8], dtype=torch.int64, device=dev)[None, :]
    symbol = torch.arange(4, dtype=torch.int64, device=dev)[None, :]

    def count(words, kk):
        words = words.contiguous()
        out = torch.empty(words.numel(), dtype=torch.int64, device=dev)
        b.count_kmers_packed_device(words.data_ptr(), kk, words.numel(), out.data_ptr(), stream)
        return out.view(words.shape)

    if canonical:  # the class count: both strands, a palindrome once
        count_one = count

        def count(words, kk):
            other = reverse_complement(words, kk)
            return torch.where(other == words, count_one(words, kk), count_one(words, kk) + count_one(other, kk))

    def missing_far_end(w, lft):
        """(m, 4) bool: the edges of a fan whose far end is a palindrome below the node threshold (even k and m >= 2 only)"""
        far = next_nodes(w, k, lft)
        return (far == reverse_complement(far, k)) & (count_one(far, k) < m)

    node_clause = canonical and k % 2 == 0 and m >= 2
    symbols = torch.zeros((n, max_steps), dtype=torch.uint8, device=dev)
    steps, sums, last = (torch.zeros(n, dtype=torch.int64, device=dev) for _ in range(3))
    stops, fans = (torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(2))

    def finish(idx, stop, r, esum, cur, fanbits):
        steps[idx], stops[idx], sums[idx], last[idx], fans[idx] = r, stop.to(torch.uint8), esum, cur, fanbits.to(torch.uint8)

    seed = seeds & mask
    node = count(seed, k) >= m
    lost = torch.nonzero(~node).flatten()
    finish(lost, torch.full_like(lost, NOT_A_NODE), 0, 0, seed[lost], torch.zeros_like(lost))
    idx = torch.nonzero(node).flatten()
    cur, esum = seed[idx], torch.zeros(idx.numel(), dtype=torch.int64, device=dev)
    fc = count(edge_words(cur, k, left), k + 1)
    lacking = missing_far_end(cur, left) if node_clause else None
    r = 0
    while idx.numel():  # (the host reads the live count: one decision a step)
        solid = fc >= me
        if node_clause:
            solid = solid & ~lacking
        width, fanbits = solid.sum(1), (solid * bit).sum(1)
        stop = torch.zeros_like(idx)
        if r == max_steps:
            stop = torch.full_like(idx, MAX_STEPS)
        stop = torch.where((stop == 0) & (width == 0), torch.full_like(idx, DEAD_END), stop)
        if not greedy:
            stop = torch.where((stop == 0) & (width >= 2), torch.full_like(idx, BRANCH), stop)
        best = torch.where(solid, fc * 4 + (3 - symbol), torch.full_like(fc, -1)).argmax(1)  # the largest count, on a tie the smallest symbol
        bcount = fc.gather(1, best[:, None]).flatten()
        cand = (best << (2 * (k - 1))) | (cur >> 2) if left else ((cur << 2) | best) & mask
        if canonical and unitig:  # a cut of the canonical unitigs' links
            edge = edge_words(cur, k, left).gather(1, best[:, None]).flatten()
            cut = (cur == reverse_complement(cur, k)) | (cand == reverse_complement(cand, k)) | (edge == reverse_complement(edge, k + 1))
            stop = torch.where((stop == 0) & cut, torch.full_like(idx, MIRROR), stop)
        if not unitig:
            stop = torch.where((stop == 0) & (cand == seed[idx]), torch.full_like(idx, RETURNED), stop)
        done = stop != 0
        finish(idx[done], stop[done], r, esum[done], cur[done], fanbits[done])
        keep = ~done
        idx, cur, esum, cand, best, bcount, fanbits = (x[keep] for x in (idx, cur, esum, cand, best, bcount, fanbits))
        if idx.numel() == 0:
            break
        queries = edge_words(cand, k, left)
        if unitig:
            queries = torch.cat([queries, edge_words(cand, k, not left)], dim=1)
        c = count(queries, k + 1)
        if node_clause:
            lacking = missing_far_end(cand, left)
        if unitig:
            back = c[:, 4:] >= me
            if node_clause:
                back = back & ~missing_far_end(cand, not left)
            merge = back.sum(1) >= 2
            done = merge | (cand == seed[idx])
            finish(idx[done], torch.where(merge, torch.full_like(idx, MERGE), torch.full_like(idx, RETURNED))[done], r, esum[done], cur[done], fanbits[done])
            keep = ~done
            idx, esum, cand, best, bcount, c = (x[keep] for x in (idx, esum, cand, best, bcount, c))
            if node_clause:
                lacking = lacking[keep]
        symbols[idx, r] = code[best]
        esum, cur, fc = esum + bcount, cand, c[:, :4]
        r += 1
    return symbols, steps, stops, sums, last, fans


def first_words(symbols, offsets, k):
    two = torch.zeros(6, dtype=torch.int64, device=symbols.device)
    two[torch.tensor([1, 2, 3, 5], device=symbols.device)] = torch.arange(4, device=symbols.device)
    w = torch.zeros(offsets.numel() - 1, dtype=torch.int64, device=symbols.device)
    for j in range(k):
        w = (w << 2) | two[symbols[offsets[:-1] + j].long()]
    return w


def seed_sets(b, k, cap, dev, stream, canonical=False):
    unitigs = b.enumerate_canonical_unitigs_device if canonical else b.enumerate_unitigs_device
    U, S = unitigs(k, None, None, None, None, None, 0, 0, min_count=2, stream=stream)
    symbols, offsets = torch.empty(S, dtype=torch.uint8, device=dev), torch.empty(U + 1, dtype=torch.int64, device=dev)
    unitigs(k, symbols.data_ptr(), offsets.data_ptr(), None, None, None, U, S, min_count=2, stream=stream)
    unitig_firsts = first_words(symbols, offsets, k)
    del symbols, offsets
    if canonical:
        n = b.enumerate_canonical_kmers_device(k, None, None, None, 0, stream=stream)
        words = torch.empty(n, dtype=torch.int64, device=dev)
        b.enumerate_canonical_kmers_device(k, words.data_ptr(), None, None, n, stream=stream)
    else:
        n = b.enumerate_kmers_device(k, None, None, None, 0, stream=stream)
        words = torch.empty(n, dtype=torch.int64, device=dev)
        b.enumerate_kmers_device(k, words.data_ptr(), None, None, n, stream=stream)
    pick = torch.linspace(0, n - 1, min(n, 10 ** 6), dtype=torch.float64, device=dev).long()
    sets = {"unitig_firsts": unitig_firsts, "kmers": words[pick].clone()}
    del words
    torch.cuda.empty_cache()
    return {name: s[torch.linspace(0, s.numel() - 1, min(s.numel(), cap), dtype=torch.float64, device=dev).long()].contiguous() for name, s in sets.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="c4")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--ks", default="21,31")
    ap.add_argument("--modes", default="unique,unitig,greedy")
    ap.add_argument("--directions", default="right,left")
    ap.add_argument("--max-steps", default="100,2000")
    ap.add_argument("--max-seeds", type=int, default=10 ** 6, help="seeds a set at the most, taken evenly (the rows of symbols take n x max_steps bytes)")
    ap.add_argument("--min-count", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--canonical", action="store_true", help="trace_canonical_kmers_device on the read set with every second read reverse-complemented")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("trace_bench needs a GPU")
    if args.repeats < 5:
        sys.exit("a median of at least five calls")
    dev = torch.device("cuda:0")
    reads = read_set(args.config, args.scale)
    n_reads, length = reads.shape
    if args.canonical:  # reads from both strands ($ A C G N T -> $ T G C N A, reversed)
        reads = reads.copy()
        reads[1::2] = np.array([0, 5, 3, 2, 4, 1], dtype=np.uint8)[reads[1::2, ::-1]]
    b = msbwt.RleBWT(device=0)
    (_, load_ms) = wall(lambda: b.load_reads((reads.reshape(-1), np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(length))))
    del reads
    stream = torch.cuda.current_stream(dev).cuda_stream
    lines, same = [], True
    for k in [int(x) for x in args.ks.split(",")]:
        for name, seeds in seed_sets(b, k, args.max_seeds, dev, stream, args.canonical).items():
            n = seeds.numel()
            for max_steps in [int(x) for x in args.max_steps.split(",")]:
                for mode in args.modes.split(","):
                    for direction in args.directions.split(","):
                        ours = [torch.zeros((n, max_steps), dtype=torch.uint8, device=dev)] + [torch.zeros(n, dtype=t, device=dev) for t in
                                                                                              (torch.int64, torch.uint8, torch.int64, torch.int64, torch.uint8)]
                        trace = b.trace_canonical_kmers_device if args.canonical else b.trace_kmers_device
                        calls = {"trace": lambda: trace(seeds.data_ptr(), k, n, max_steps, *[t.data_ptr() for t in ours], mode=MODES[mode], direction=DIRECTIONS[direction],
                                                        min_count=args.min_count, stream=stream),
                                 "host_loop": lambda: host_loop(b, seeds, k, max_steps, mode, direction, args.min_count, args.min_count, stream, args.canonical)}
                        if args.canonical:  # the strand-specific call on the same index and seeds, into buffers of its own
                            plain = [torch.zeros_like(t) for t in ours]
                            calls["plain"] = lambda: b.trace_kmers_device(seeds.data_ptr(), k, n, max_steps, *[t.data_ptr() for t in plain], mode=MODES[mode],
                                                                          direction=DIRECTIONS[direction], min_count=args.min_count, stream=stream)
                        theirs = calls["host_loop"]()  # warm-up, and the comparison
                        calls["trace"]()
                        b.device_status(stream)
                        ok = all(torch.equal(x, y) for x, y in zip(ours, theirs))
                        del theirs
                        ms = {route: [] for route in calls}
                        for _ in range(args.repeats):  # alternating
                            for route, fn in calls.items():
                                _, t = wall(fn)
                                ms[route].append(t)
                        calls["trace"]()
                        info = b.canonical_trace_info() if args.canonical else b.trace_info()
                        res = {"canonical": args.canonical, "k": k, "seeds": name, "n": n, "max_steps": max_steps, "mode": mode, "direction": direction, "min_count": args.min_count,
                               "symbols": int(b.get_total_size()), "info": info, "trace_ms": spread(ms["trace"]), "host_loop_ms": spread(ms["host_loop"]), "same": bool(ok)}
                        res["host_loop_over_trace"] = round(res["host_loop_ms"]["median"] / res["trace_ms"]["median"], 2)
                        res["queries_per_s"] = round(info["queries"] / (res["trace_ms"]["median"] * 1e-3), 0)
                        if args.canonical:
                            calls["plain"]()
                            res.update(plain_ms=spread(ms["plain"]), plain_info=b.trace_info(), stops=torch.bincount(ours[2], minlength=9).tolist())
                            res["trace_over_plain"] = round(res["trace_ms"]["median"] / res["plain_ms"]["median"], 2)
                            del plain
                        same = same and bool(ok)
                        print(json.dumps(res), flush=True)
                        lines.append(res)
                        del ours
                        torch.cuda.empty_cache()
    key = lambda r: "%d/%s/%d/%s/%s" % (r["k"], r["seeds"], r["max_steps"], r["mode"], r["direction"])
    summary = {"canonical": args.canonical, "config": args.config, "scale": args.scale, "load_reads_ms": round(load_ms, 1), "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
               "trace_ms": {key(r): r["trace_ms"]["median"] for r in lines}, "host_loop_ms": {key(r): r["host_loop_ms"]["median"] for r in lines}, "same": same}
    if args.canonical:
        summary["plain_ms"] = {key(r): r["plain_ms"]["median"] for r in lines}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"lines": lines, "summary": summary}, f, indent=1)
    if not same:
        sys.exit("the host loop and the trace call disagree")


if __name__ == "__main__":
    main()
