"""tests/sparse_craft.py against the library's own hash and sizing (no device): the restated mix and its inverse, the bucket windows, the
shapes -- and every plan tests/test_gpu_sparse_crafted.py loads, so that what runs on the card is known to be what was wished for:
crafted suffixes in their buckets with their tags, every other window of every read outside the protected zones, chains exactly as
long as intended whatever the insertion order, every planned line inside nbuckets + probe."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

from rust_msbwt_amd import _lib
import sparse_craft as sc


def lib_hash(key, depth, nbuckets):
    b, tag = C.c_uint32(), C.c_uint64()
    assert _lib.lib().msbwt_sparse_hash64(int(key), depth, nbuckets, C.byref(b), C.byref(tag)) == 0
    return b.value, tag.value


def lib_shape(depth, entries):
    nb, probe = C.c_uint64(), C.c_int()
    assert _lib.lib().msbwt_sparse_table_shape(depth, entries, C.byref(nb), C.byref(probe)) == 0
    return nb.value, probe.value


@pytest.mark.parametrize("depth", range(16, 32))
def test_mix_and_its_inverse_against_the_library(depth):
    rng = np.random.default_rng(depth)
    keys = [int(x) & ((1 << (2 * depth)) - 1) for x in rng.integers(0, 1 << 62, size=2000)] + [0, (1 << (2 * depth)) - 1]
    for i, key in enumerate(keys):
        nb = (sc.sparse_min_buckets(depth), 1000, 2 ** 32 - 1, sc.sparse_min_buckets(depth) * 5 // 4)[i % 4]
        mixed = sc.mix(key, depth)
        assert (sc.bucket_of(mixed, depth, nb), sc.tag_of(mixed, depth)) == lib_hash(key, depth, nb)
        assert sc.unmix(mixed, depth) == key and sc.mix(sc.unmix(key, depth), depth) == key


@pytest.mark.parametrize("depth", [16, 20, 24, 25, 29, 30, 31])
def test_bucket_windows_and_shapes(depth):
    nb, probe = lib_shape(depth, 100)
    assert (nb, probe) == (sc.sparse_min_buckets(depth), 7) == sc.shape_of(depth, False)[:2] and sc.probe_limit(depth, nb) == 7
    for nbuckets in (nb, nb + nb // 4, sc.sparse_tier_min_buckets(depth)):
        for bucket in (0, 1, nbuckets // 3, nbuckets - 1):
            lo, hi = sc.window_of(bucket, depth, nbuckets)
            assert lib_hash(sc.unmix(lo, depth), depth, nbuckets)[0] == bucket == lib_hash(sc.unmix(hi - 1, depth), depth, nbuckets)[0]
            assert bucket == 0 or lib_hash(sc.unmix(lo - 1, depth), depth, nbuckets)[0] == bucket - 1
            assert bucket == nbuckets - 1 or lib_hash(sc.unmix(hi, depth), depth, nbuckets)[0] == bucket + 1
        # tags are unambiguous within a probe window: (probe + 1) windows fit the tag space
        p = sc.probe_limit(depth, nbuckets)
        lo, hi = sc.window_of(nbuckets // 3, depth, nbuckets)
        assert p >= 3 and (p + 1) * (hi - lo) <= 1 << sc.tag_bits(depth)
    if depth >= 30:   # a bucket window of the 40-bit layout holds 32 mixed values per low word
        lo, hi = sc.window_of(5, depth, nb)
        assert hi - lo == 32 << 32
    entries = 10 ** 7
    assert lib_shape(depth, entries)[1] == sc.probe_limit(depth, lib_shape(depth, entries)[0])


@pytest.mark.parametrize("depth", [16, 17, 19, 23, 25, 28])
def test_two_tier_shape_against_the_automatic_choice(depth):
    """msbwt_auto_sparse_choice reports the table's bytes: (nbuckets + 15) * 128 without wide entries, which gives the bucket count."""
    def chosen(solid, singles):
        d, w, o = (C.c_uint64 * 32)(), (C.c_uint64 * 32)(), (C.c_uint64 * 32)()
        d[depth], o[depth] = solid + singles, singles
        got, tier, nbytes = C.c_int(), C.c_int(), C.c_uint64()
        assert _lib.lib().msbwt_auto_sparse_choice(d, w, o, 8, 1 << 40, depth, 1, C.byref(got), C.byref(tier), C.byref(nbytes)) == 0
        assert got.value == depth and tier.value == 1
        return nbytes.value // 128 - sc.MAX_PROBE

    least = sc.sparse_tier_min_buckets(depth)
    assert least == 1 << max(0, 2 * depth + 2 - sc.tag_bits(depth))
    cases = [(10 ** 9, 10 ** 8), (10 ** 8, 2 * 10 ** 10), (7 * least, 100), (123456789, 987654321)]
    if least <= 65536:
        cases.append((100, 100))                      # the tags' least bucket count (a toy index keeps it only where it is small)
    for solid, singles in cases:
        assert chosen(solid, singles) == sc.sparse_tier_buckets(depth, solid, singles), (solid, singles)
    assert sc.shape_of(depth, True) == (least, 3, sc.slots_of(depth, True))


# ---- the plans ----
def check_plan(plan):
    """through the library's hash: crafted suffixes where wished; no other window of a read in a protected zone; every suffix as often as
    wished, by counting over the reads; -> the present suffixes that take an entry"""
    d, nb = plan.depth, plan.nbuckets
    assert plan.probe == sc.probe_limit(d, nb) and plan.slots == sc.slots_of(d, plan.tier)
    for c, row in zip(plan.crafted, plan.rows):
        assert lib_hash(c.key, d, nb) == (c.bucket, c.tag)
        assert sc.key_of(row[-d:]) == c.key and np.array_equal(sc.kmer_of(c.key, d), row[-d:]) and len(row) == plan.read_len
        assert set(range(max(0, c.bucket - plan.probe), min(nb, c.bucket + plan.probe + 1))) <= plan.zones
    assert len(plan.zones) <= (16 if len({c.bucket for c in plan.crafted}) == 1 else nb // 8)
    distinct = np.unique(plan.reads, axis=0)
    assert np.isin(distinct, sc.ACGT).all() and plan.reads.shape == (sum(c.mult for c in plan.crafted), plan.read_len)
    for row in distinct:
        for at in range(plan.read_len - d):
            assert lib_hash(sc.key_of(row[at:at + d]), d, nb)[0] not in plan.zones
    text = sc.text_of(plan.reads)
    for c in plan.crafted:
        s = "".join("$ACGNT"[x] for x in sc.kmer_of(c.key, d))
        assert sum(t.count(s, at, at + d) for t in text for at in range(plan.read_len - d + 1)) == c.mult, c
    # the reads' other windows overflow no bucket of their own: whatever is displaced in the table, the plan displaced it
    windows, counts = np.unique(np.lib.stride_tricks.sliding_window_view(plan.reads, d, axis=1).reshape(-1, d), axis=0, return_counts=True)
    takes_entry = [sc.key_of(x) for x, n in zip(windows, counts) if n > (1 if plan.tier else 0)]
    wanted = sc.simulate_fill(takes_entry, nb, plan.probe, plan.slots, depth=d).wanted
    assert all(n <= plan.slots for b, n in wanted.items() if b < nb and b not in plan.zones)
    return plan.present_keys(solid_only=plan.tier)


@pytest.mark.parametrize("config", sc.CONFIGS)
def test_tag_plans(config):
    plan = sc.tags_plan(config)
    depth, tier = sc.CONFIGS[config]
    assert (plan.nbuckets, plan.probe, plan.slots) == {"complete16": (2048, 7, 14), "complete25": (2 ** 21, 7, 12), "complete30": (2 ** 23, 7, 11),
                                                      "complete31": (2 ** 25, 7, 11), "tier16": (1024, 3, 10), "tier25": (2 ** 20, 3, 9)}[config]
    keys = check_plan(plan)
    c = plan.probe + 1
    (all_a,), (all_t,) = plan.group("all_a"), plan.group("all_t")
    assert (all_a.key, all_a.mixed, all_a.bucket, all_a.tag, all_a.mult) == (0, 0, 0, 0, 1) and (sc.kmer_of(0, depth) == 1).all()
    assert all_t.key == 4 ** depth - 1 and (sc.kmer_of(all_t.key, depth) == 5).all()
    assert all(abs(all_t.bucket - o.bucket) > plan.probe for o in plan.crafted if o is not all_t)
    zero = [x for x in plan.crafted if x.tag == 0]
    assert [(x.group, x.bucket, x.mult) for x in zero] == [("all_a", 0, 1), ("tag0", 5 * c, 3), ("tag0", 9 * c, 300), ("tag0_absent_empty", 13 * c, 0),
                                                           ("tag0_absent_partly", 17 * c, 0), ("tag0_absent_full", 21 * c, 0)]
    if tier:   # a tag of 0 hashes to filter word 0 and four times bit 0
        word, mask = C.c_uint32(), C.c_uint32()
        assert _lib.lib().msbwt_sparse_filter_bits(0, C.byref(word), C.byref(mask)) == 0 and (word.value, mask.value) == (0, 1)
    fill = sc.simulate_fill(keys, plan.nbuckets, plan.probe, plan.slots, depth=depth)
    want = {all_t.bucket: 1, 5 * c: 4 if tier else 5, 9 * c: 1, 17 * c: 3, 21 * c: plan.slots}
    if not tier:
        want[0] = 1
    if depth >= 30:
        want.update({25 * c: 6, 29 * c: 11, 29 * c + 1: 6})
        for zero_group, word_group in (("shared_zero", "shared_word"), ("pushed_zero", "pushed_word")):
            for name, low in ((zero_group, 0), (word_group, 0x5EEDBEE5)):
                tags = [x.tag for x in plan.group(name) + plan.group(name + "_absent")]
                assert {t & 0xFFFFFFFF for t in tags} == {low} and len({t >> 32 for t in tags}) == len(tags) and 0 not in tags
                mults = [x.mult for x in plan.group(name)]
                assert len(set(mults)) == len(mults)
        for b, n in ((25 * c, 6), (29 * c, 17)):   # distinct multiplicities: a wrong slot shows in the count
            assert len({x.mult for x in plan.crafted if x.bucket == b and x.mult}) == n
    assert fill.occupancy == want and not fill.can_fail and fill.max_displacement == (1 if depth >= 30 else 0)
    assert fill.wanted[21 * c] == plan.slots        # exactly full: nothing was displaced, a lookup ends here
    if tier:
        sat = plan.group("saturating")
        assert len(sat) == sc.SATURATION and {x.bucket for x in sat + plan.group("saturated_absent")} == {33 * c} and all(x.mult == 1 for x in sat)
        bits = [0] * 8     # the filter of that bucket, as the builder sets it: nearly every absent suffix homed there is a false positive
        word, mask = C.c_uint32(), C.c_uint32()
        for x in sat:
            _lib.lib().msbwt_sparse_filter_bits(x.tag, C.byref(word), C.byref(mask))
            bits[word.value] |= mask.value
        false_pos = 0
        for x in plan.group("saturated_absent"):
            _lib.lib().msbwt_sparse_filter_bits(x.tag, C.byref(word), C.byref(mask))
            false_pos += (bits[word.value] & mask.value) == mask.value
        assert false_pos >= 30, false_pos
    # every line a lookup may touch exists
    assert max(fill.occupancy) < plan.nbuckets + plan.probe


@pytest.mark.parametrize("config", sc.CONFIGS)
def test_chain_plans(config):
    plan = sc.chains_plan(config)
    depth, tier = sc.CONFIGS[config]
    keys = check_plan(plan)
    fill = sc.simulate_fill(keys, plan.nbuckets, plan.probe, plan.slots, depth=depth)
    want = {}
    for name, b in sc.chain_buckets(config).items():
        chain = plan.group("chain_" + name)
        assert len(chain) == plan.slots * plan.probe + 1 and {x.bucket for x in chain} == {b} and all(x.mult >= (2 if tier else 1) for x in chain)
        want.update({b + i: plan.slots for i in range(plan.probe)})
        want[b + plan.probe] = 1
        assert fill.wanted[b] == len(chain) and fill.wanted[b + plan.probe] == 1
        assert {x.bucket for x in plan.group("absent_" + name)} == {b}
        assert {x.bucket for x in plan.group("behind_" + name)} == {b + i for i in range(1, plan.probe + 1) if b + i < plan.nbuckets}
        if tier:
            once = plan.group("once_" + name)
            assert len(once) == 6 and all(x.mult == 1 and x.bucket == b for x in once)
    assert sc.chain_buckets(config)["first"] == 0 and sc.chain_buckets(config)["last"] == plan.nbuckets - 1
    # the same chain whatever the order: B .. B + probe - 1 full, one entry exactly `probe` buckets from home; the last chain ends in the last line
    assert fill.occupancy == want and not fill.can_fail and fill.max_displacement == plan.probe
    assert max(fill.occupancy) == plan.nbuckets + plan.probe - 1


@pytest.mark.parametrize("config", sc.REFILL_CONFIGS)
def test_refill_plans(config):
    plan = sc.refill_plan(config)
    depth, tier = sc.CONFIGS[config]
    keys = check_plan(plan)
    assert len(keys) == len(plan.crafted) == plan.slots * (plan.probe + 1) + 1 and len({x.bucket for x in plan.crafted}) == 1
    # more suffixes than the whole chain holds: the first fill fails whatever the order
    assert sc.simulate_fill(keys, plan.nbuckets, plan.probe, plan.slots, depth=depth).can_fail
    nb2, probe2 = plan.grown
    assert nb2 == plan.nbuckets + plan.nbuckets // 4 and probe2 == sc.probe_limit(depth, nb2) >= plan.probe
    homes = Counter(lib_hash(k, depth, nb2)[0] for k in keys)
    assert homes == Counter(sc.bucket_of(sc.mix(k, depth), depth, nb2) for k in keys) and len(homes) == 2
    fill = sc.simulate_fill(keys, nb2, probe2, plan.slots, depth=depth)
    assert not fill.can_fail and 0 < fill.max_displacement <= probe2 and max(fill.occupancy) < nb2 + probe2
    # and no other window of a read comes near them in the grown table either
    near = {b + i for b in homes for i in range(-probe2, 2 * probe2 + 1)}
    for row in np.unique(plan.reads, axis=0):
        for at in range(plan.read_len - depth):
            assert lib_hash(sc.key_of(row[at:at + depth]), depth, nb2)[0] not in near
