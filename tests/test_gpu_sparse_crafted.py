"""The sparse suffix table with keys crafted THROUGH its hash (tests/sparse_craft.py; the plans are verified on the CPU by
tests/test_sparse_craft.py): the coincidences random k-mers meet once in 2^24 or 2^32 lookups, or never -- tag 0 and key 0, low tag words
shared inside a bucket of the 40-bit layout, chains that reach the probe limit at both ends of the table, a fill that fails and is repeated
with more buckets, once-only suffixes behind a full chain and a saturated filter in the two-tier form.  Expected values come from the CPU
oracle AND from the multiplicities the plan wished for; the walk of the downloaded table says what the kernels' counters must show.
Needs an MI355X: run with `pytest -m gpu`."""
import numpy as np
import pytest

import rust_msbwt_amd as msbwt
from rust_msbwt_amd import RleBWT
from oracle import oracle as orc
import sparse_craft as sc
from test_gpu_sparse import host_lookup, oracle_ranges, table_key, tier_lookup

pytestmark = pytest.mark.gpu

STRIDE = {"complete16": 96, "complete25": 128, "complete30": 96, "complete31": 128, "tier16": 128, "tier25": 96}
DIRECT = {"packed": {}, "flat": {"MSBWT_TABLE_PACKED": 0}, "none": {"MSBWT_TABLE_DEPTH": 0}}
BIG_ROWS = 2_500_000


class World:
    """one loaded index with everything the tests of a plan share: handle, oracle, the downloaded table, the query rows (every crafted
    suffix behind its prefix, mutations of them) and what the walk of the downloaded table says about each"""


def load(plan, config, blocks="planes", direct="packed", mp=None):
    mp.setenv("MSBWT_SEARCH", "lanes")
    mp.setenv("MSBWT_SPARSE_TABLE", str(plan.depth))
    mp.setenv("MSBWT_SPARSE_TIERS", "1" if plan.tier else "0")
    mp.setenv("MSBWT_PAIR_STRIDE", str(STRIDE[config]))
    mp.setenv("MSBWT_FILTER", "0")             # absent crafted queries must reach the lookup
    mp.setenv("MSBWT_BLOCKS", blocks)
    for name, value in DIRECT[direct].items():
        mp.setenv(name, str(value))
    rle = orc.convert_to_vec(orc.naive_bwt(sc.text_of(plan.reads)))
    ref = orc.OracleRleBWT()
    ref.load_vector(rle)
    b = RleBWT()
    b.load_vector(rle)
    return b, ref


def expected_shape(plan, info, grown=False):
    """entries, filtered and side entries by counting the reads' windows (nothing here comes from the table)"""
    windows = np.lib.stride_tricks.sliding_window_view(plan.reads, plan.depth, axis=1).reshape(-1, plan.depth)
    _, counts = np.unique(windows, axis=0, return_counts=True)
    once = int((counts == 1).sum()) if plan.tier else 0
    nb, probe = plan.grown if grown else (plan.nbuckets, plan.probe)
    want = {"depth": plan.depth, "buckets": nb, "probe": probe, "two_tier": plan.tier, "entries": len(counts) - once, "filtered": once,
            "side_entries": int((counts >= 255).sum()), "bytes": (nb + probe) * 128}
    assert {k: info[k] for k in want} == want
    return want


def walk(w, keys):
    look = tier_lookup if w.plan.tier else host_lookup
    return [look(w.lines, w.side, w.info, int(key), walked=True) for key in keys]


def away_from_home(w):
    """entries of the downloaded table that do not sit in their own bucket: every present suffix is walked to"""
    windows = np.unique(np.lib.stride_tricks.sliding_window_view(w.plan.reads, w.plan.depth, axis=1).reshape(-1, w.plan.depth), axis=0)
    found = walk(w, table_key(windows))
    l, h = oracle_ranges(w.ref, windows)
    away = 0
    for (got, dist), el, eh in zip(found, l, h):
        if w.plan.tier:
            assert got == (("filter",) if eh - el == 1 else ("entry", int(el), int(eh)))
            away += dist > 0 and got != ("filter",)
        else:
            assert got == (int(el), int(eh))     # every entry is found by the walk, with the oracle's range
            away += dist > 0
    return away, found


WORLDS = [(config, kind, "planes", "packed") for config in sc.CONFIGS for kind in ("tags", "chains")]
WORLDS += [("complete16", kind, "runs", "packed") for kind in ("tags", "chains")]        # the sparse kernels with kPair == false
WORLDS += [(config, kind, "planes", direct) for config in ("tier16", "tier25") for kind in ("tags", "chains") for direct in ("flat", "none")]


@pytest.fixture(scope="module", params=WORLDS, ids=lambda p: "-".join(p))
def world(request):
    config, kind, blocks, direct = request.param
    mp = pytest.MonkeyPatch()
    w = World()
    w.config, w.kind, w.blocks, w.direct = request.param
    w.plan = sc.tags_plan(config) if kind == "tags" else sc.chains_plan(config)
    w.b, w.ref = load(w.plan, config, blocks, direct, mp)
    w.info = w.b.sparse_table_info()
    expected_shape(w.plan, w.info)                 # a plan that did not materialise fails here, before anything is asked of it
    w.lines, w.side = w.b.download_sparse_table()
    w.rows, w.names = sc.query_rows(w.plan, seed=7)
    w.keys = table_key(w.rows[:, -w.plan.depth:])
    w.walk = walk(w, w.keys)
    w.displaced = sum(dist for _, dist in w.walk)
    w.fallbacks = sum(got == ("filter",) for got, _ in w.walk)
    w.mult = np.array([c.mult for c in w.plan.crafted], dtype=np.uint64)
    w.ks = sorted({k for k in (w.plan.depth, w.plan.depth + 1, w.plan.depth + 2, 33, 40) if w.plan.depth <= k <= w.plan.read_len})
    w.exp = {k: w.ref.count_kmers(np.ascontiguousarray(w.rows[:, -k:])) for k in w.ks}
    yield w
    mp.undo()


def counted(w, q):
    w.b.set_search_counters(True)
    got = w.b.count_kmers(q)
    cnt = w.b.search_counters(0)
    w.b.set_search_counters(False)
    return got, cnt


def test_the_plan_materialised_and_the_walk_finds_every_entry(world):
    w = world
    plan, info = w.plan, w.info
    assert w.b.get_sparse_table() == plan.depth and w.b.get_sparse_tiers() == plan.tier and w.b.get_pair_index() == (w.blocks == "planes")
    assert w.blocks == "runs" or w.b.get_pair_stride() == STRIDE[w.config]
    if plan.tier:
        assert (w.b.get_table_depth() == 0) == (w.direct == "none") and w.b.get_table_depth() < plan.depth and w.b.get_table_packed() == (w.direct == "packed")
    away, _ = away_from_home(w)
    assert info["displaced"] == away
    by_key = {c.key: c for c in plan.crafted}
    for key, (got, dist), row in zip(w.keys[:len(plan.crafted)], w.walk, w.rows):
        c = by_key[int(key)]
        width = None if got in (None, ("filter",)) else got[-1] - got[-2]
        if c.mult == 0:
            assert got is None or (plan.tier and got == ("filter",)), c
        elif plan.tier and c.mult == 1:
            assert got == ("filter",), c
        else:
            assert width == c.mult, c
    if w.kind == "chains":
        slots, probe = plan.slots, plan.probe
        assert info["displaced"] == 3 * (slots * probe + 1 - slots)
        for name, b0 in sc.chain_buckets(w.config).items():
            dists = sorted(dist for c, (_, dist) in zip(plan.crafted, w.walk) if c.group == "chain_" + name)
            assert dists == sorted([d for d in range(probe) for _ in range(slots)] + [probe])    # one entry exactly `probe` buckets from home
            # an absent suffix homed in B stops at the probe limit; the ones homed behind B see a foreign chain as far as it goes
            assert all(dist == probe for c, (_, dist) in zip(plan.crafted, w.walk) if c.group in ("absent_" + name, "once_" + name))
            assert all(dist == min(probe, b0 + probe - c.bucket) for c, (_, dist) in zip(plan.crafted, w.walk) if c.group == "behind_" + name)
        assert info["bytes"] // 128 - 1 == sc.chain_buckets(w.config)["last"] + probe     # the last chain ends in the last line
    else:
        assert info["side_entries"] >= 1 and info["displaced"] == (6 if plan.depth >= 30 else 0)
        if plan.depth >= 30:
            # the 40-bit layout: the scan takes the candidates of a low word from the lowest slot up, so of m entries of one bucket that share
            # their low word the i-th needs i rounds -- three share it in a bucket of their own, seventeen (two words) in the pushed pair
            def rounds(c, dist):
                line = w.lines[c.bucket + dist]
                raw = line.view(np.uint8)
                his = [int(raw[88 + s]) for s in range(plan.slots) if raw[110 + s] != 0 and int(line[s]) == c.tag & 0xFFFFFFFF]
                return his.index(c.tag >> 32) + 1

            found = {c.key: dist for c, (_, dist) in zip(plan.crafted, w.walk)}
            for name in ("shared_zero", "shared_word"):
                assert sorted(rounds(c, found[c.key]) for c in plan.group(name)) == [1, 2, 3]
            pushed = [rounds(c, found[c.key]) for c in plan.group("pushed_zero") + plan.group("pushed_word")]
            assert len(pushed) == 17 and max(pushed) >= 3 and sum(found[c.key] for c in plan.group("pushed_zero") + plan.group("pushed_word")) == 6
        if plan.tier:   # nearly every absent suffix homed in the saturated bucket is a false positive of its filter
            assert sum(got == ("filter",) for c, (got, _) in zip(plan.crafted, w.walk) if c.group == "saturated_absent") >= 30
            assert all(got == ("filter",) for c, (got, _) in zip(plan.crafted, w.walk) if c.group in ("saturating", "all_a"))


def test_counts_and_ranges_of_every_crafted_query(world):
    w = world
    n = len(w.plan.crafted)
    for k in w.ks:
        q = np.ascontiguousarray(w.rows[:, -k:])
        exp = w.exp[k]
        # the second witness: a crafted suffix occurs as often as wished, with any prefix of its read in front (k > depth), an absent one never
        assert np.array_equal(exp[:n], w.mult), k
        few = np.ascontiguousarray(q[::max(1, len(q) // 60)][:64])
        assert np.array_equal(w.b.count_kmers(few), exp[::max(1, len(q) // 60)][:64]), k
        got, cnt = counted(w, np.ascontiguousarray(np.tile(q, (5, 1))))
        print(w.config, w.kind, w.blocks, w.direct, "k", k, "rows", 5 * len(q), "walk", 5 * w.displaced, 5 * w.fallbacks, cnt)
        assert np.array_equal(got, np.tile(exp, 5)), k
        assert w.b.search_kernel_for(k) == "lanes"
        # every query reaches the lookup (no presence filter, ACGT only); each bucket beyond a query's own is one more step
        assert cnt["table_displaced"] == 5 * w.displaced, (k, cnt)
        assert cnt["tier_fallbacks"] == 5 * w.fallbacks, (k, cnt)
        dlooks = cnt["tier_fallbacks"] if w.plan.tier and w.direct != "none" else 0
        assert cnt["table_steps"] == 5 * len(q) + cnt["table_displaced"] + dlooks, (k, cnt)
        assert cnt["table_steps"] - cnt["table_rides"] > 0, (k, cnt)
        assert cnt["escape_queries"] >= (5 if w.kind == "tags" else 0), (k, cnt)
        assert np.array_equal(w.b.count_kmers_packed(msbwt.rle_bwt.pack_2bit(q), k), exp), k
        l, h = w.b.kmer_ranges(q)
        el, eh = oracle_ranges(w.ref, q)
        hit = eh > el
        assert np.array_equal(l[hit], el[hit]) and np.array_equal(h[hit], eh[hit]) and (l[~hit] == 0).all() and (h[~hit] == 0).all(), k
        assert np.array_equal(h - l, exp), k


def test_tiles_far_outnumber_resident_waves(world):
    """about 2.5e6 rows: most lookups ride along with the search of the tile before theirs -- a chain is then walked across search steps"""
    w = world
    for k in sorted({w.ks[1], w.ks[-1]}):
        q = np.ascontiguousarray(w.rows[:, -k:])
        reps = -(-BIG_ROWS // len(q))
        got, cnt = counted(w, np.ascontiguousarray(np.tile(q, (reps, 1))))
        print(w.config, w.kind, w.blocks, w.direct, "k", k, "rows", reps * len(q), "walk", reps * w.displaced, reps * w.fallbacks, cnt)
        assert np.array_equal(got, np.tile(w.exp[k], reps)), k
        assert cnt["table_rides"] > 0 and cnt["table_steps"] - cnt["table_rides"] > 0, (k, cnt)
        assert cnt["table_displaced"] == reps * w.displaced and cnt["tier_fallbacks"] == reps * w.fallbacks, (k, cnt)
        assert cnt["table_steps"] >= reps * len(q), (k, cnt)


def test_read_windows_of_both_strands_and_the_default_presence_filter(world):
    w = world
    reads = np.unique(w.plan.reads, axis=0)[:300]
    for k in (w.ks[0], w.ks[-2]):
        fwd, rc = w.b.count_read_kmers(reads, k, ascii=False, forward=True, revcomp=True)
        windows = np.lib.stride_tricks.sliding_window_view(reads, k, axis=1).reshape(-1, k)
        assert np.array_equal(fwd, w.ref.count_kmers(windows).reshape(fwd.shape)), k
        rcq = np.array([orc.reverse_complement_i(x) for x in windows], dtype=np.uint8)
        assert np.array_equal(rc, w.ref.count_kmers(rcq).reshape(rc.shape)), k
    if w.blocks == "runs":
        return      # (a rebuilding setter cannot bring the table back there: the plane blocks it was built from are gone)
    assert w.b.get_presence_filter() == 0
    w.b.set_presence_filter(1)
    try:
        info = w.b.sparse_table_info()
        assert {x: info[x] for x in ("buckets", "probe", "entries", "displaced", "filtered")} == {x: w.info[x] for x in ("buckets", "probe", "entries", "displaced", "filtered")}
        for k in w.ks:
            assert np.array_equal(w.b.count_kmers(np.ascontiguousarray(w.rows[:, -k:])), w.exp[k]), k
    finally:
        w.b.set_presence_filter(0)
    assert w.b.get_presence_filter() == 0


@pytest.mark.parametrize("config", sc.REFILL_CONFIGS)
def test_a_fill_that_finds_no_slot_is_repeated_with_a_quarter_more_buckets(config, monkeypatch):
    """slots * (probe + 1) + 1 suffixes homed in one bucket: the first fill must fail, the second (nbuckets + nbuckets / 4) holds them --
    with the entries, filter bits and side entries of ONE fill."""
    w = World()
    w.plan = plan = sc.refill_plan(config)
    w.b, w.ref = load(plan, config, mp=monkeypatch)
    w.info = info = w.b.sparse_table_info()
    nb2, probe2 = plan.grown
    assert info["buckets"] == plan.nbuckets + plan.nbuckets // 4 == nb2 and info["probe"] == probe2
    want = expected_shape(plan, info, grown=True)
    assert want["side_entries"] >= 1
    w.lines, w.side = w.b.download_sparse_table()
    away, _ = away_from_home(w)                    # every entry is found by the walk
    assert info["displaced"] == away > 0
    used = (w.lines.view(np.uint8).reshape(len(w.lines), 128)[:, 108:120] != 0).sum() if plan.depth >= 25 else ((w.lines[:, :plan.slots] >> 24) != 0).sum()
    assert int(used) == info["entries"]            # nothing of the failed fill is left, nothing is there twice
    rows, _ = sc.query_rows(plan, seed=9)
    exp = {}
    for k in (plan.depth, plan.depth + 1, 33, 40):
        q = np.ascontiguousarray(rows[:, -k:])
        exp[k] = w.ref.count_kmers(q)
        assert np.array_equal(exp[k][:len(plan.crafted)], [c.mult for c in plan.crafted])
        assert np.array_equal(w.b.count_kmers(q), exp[k]), k
        l, h = w.b.kmer_ranges(q)
        el, eh = oracle_ranges(w.ref, q)
        hit = eh > el
        assert np.array_equal(l[hit], el[hit]) and np.array_equal(h[hit], eh[hit]) and (h[~hit] == 0).all(), k
    twin = w.b.replicate(w.b.device_ordinal())
    same = ("depth", "buckets", "probe", "bytes", "entries", "filtered", "side_entries", "side_bytes", "displaced", "two_tier")
    tinfo = twin.sparse_table_info()
    assert {x: tinfo[x] for x in same} == {x: info[x] for x in same}
    tl, ts = twin.download_sparse_table()
    assert np.array_equal(tl, w.lines) and np.array_equal(ts, w.side)
    assert np.array_equal(twin.count_kmers(np.ascontiguousarray(rows[:, -33:])), exp[33])
    w.b.set_sparse_table(0)
    assert w.b.get_sparse_table() == 0 and np.array_equal(w.b.count_kmers(np.ascontiguousarray(rows[:, -33:])), exp[33])
    w.b.set_sparse_table(plan.depth)
    again = w.b.sparse_table_info()
    assert {x: again[x] for x in same} == {x: info[x] for x in same}, (again, info)
    assert np.array_equal(w.b.count_kmers(np.ascontiguousarray(rows[:, -plan.depth:])), exp[plan.depth])
