"""Keys crafted THROUGH the hash of the sparse suffix table (test infrastructure; csrc/sparse_table.hpp, csrc/sparse_policy.hpp restated).

sparse_mix is a bijection of 2 d-bit words -- two odd multiplications and two xor-shifts by half the word -- so a test may choose the MIXED
value first (that fixes bucket, tag and filter bits), invert the mix and get the d-mer that lands there.  The planner below turns wishes
("this many suffixes in that bucket, with this tag, occurring so often") into reads whose last `depth` symbols are the crafted suffixes and
whose other windows stay away from the buckets the wishes are about; simulate_fill is the builder's linear probing on the CPU.
Everything here is checked against the library's own hash by tests/test_sparse_craft.py before a GPU test relies on it."""
import functools
from collections import Counter, namedtuple

import numpy as np

MUL1, MUL2 = 0x9E3779B97F4A7C15, 0xD6E8FEB86659FD93
ACGT = np.array([1, 2, 3, 5], dtype=np.uint8)       # symbol codes of the 2-bit codes 0..3
MAX_PROBE = 15
READ_LEN = 40
MAX_TRIES = 1000


# ---- the hash (sparse_table.hpp: sparse_mix, sparse_bucket, sparse_tag) ----
def mix(key, depth):
    n = 2 * depth
    mask = (1 << n) - 1
    x = key & mask
    x = (x * MUL1) & mask
    x ^= x >> (n >> 1)
    x = (x * MUL2) & mask
    x ^= x >> (n >> 1)
    return x


def unmix(mixed, depth):
    """mix backwards: an xor-shift by half the word is its own inverse, an odd multiplier has an inverse modulo 2^n"""
    n = 2 * depth
    mask = (1 << n) - 1
    x = mixed & mask
    x ^= x >> (n >> 1)
    x = (x * pow(MUL2, -1, 1 << n)) & mask
    x ^= x >> (n >> 1)
    x = (x * pow(MUL1, -1, 1 << n)) & mask
    return x


def tag_bits(depth):
    return 40 if depth >= 30 else 32 if depth >= 25 else 24


def bucket_of(mixed, depth, nbuckets):
    return ((mixed >> (2 * depth - 32)) * nbuckets) >> 32


def tag_of(mixed, depth):
    return mixed & ((1 << tag_bits(depth)) - 1)


def window_of(bucket, depth, nbuckets):
    """[lo, hi) of the mixed values whose bucket this is: contiguous, as sparse_bucket documents"""
    lo = -((-bucket << 32) // nbuckets)
    hi = -((-(bucket + 1) << 32) // nbuckets)
    return lo << (2 * depth - 32), hi << (2 * depth - 32)


# ---- shapes (sparse_table.hpp: sparse_slots, sparse_probe_limit, sparse_min_buckets; sparse_policy.hpp: the two-tier form) ----
def slots_of(depth, tier=False):
    if tier:
        return 9 if depth >= 25 else 10
    return 11 if depth >= 30 else 12 if depth >= 25 else 14


def probe_limit(depth, nbuckets):
    per_top = -((-1 << 32) // nbuckets)
    fit = (1 << tag_bits(depth)) // (per_top << (2 * depth - 32))
    return -1 if fit < 2 else min(fit - 1, MAX_PROBE)


def _least_buckets(depth, windows_log2):
    bits, shift = tag_bits(depth), 2 * depth - 32 + windows_log2
    assert shift < bits
    if bits - shift >= 32:
        return 1
    per_top = 1 << (bits - shift)
    return ((1 << 32) + per_top - 1) // per_top


def sparse_min_buckets(depth):
    return _least_buckets(depth, 3)          # a probe limit of 7 at least


def sparse_tier_min_buckets(depth):
    return _least_buckets(depth, 2)          # ... of 3


def sparse_tier_load(depth):
    return 5.0 if depth >= 25 else 5.8


def sparse_tier_buckets(depth, solid, singles):
    return max(int(solid / sparse_tier_load(depth)) + 1, int(singles / 32.0) + 1, sparse_tier_min_buckets(depth))


def shape_of(depth, tier):
    """(nbuckets, probe, slots) of a table at the tags' least bucket count -- what a few hundred reads get"""
    nb = sparse_tier_min_buckets(depth) if tier else sparse_min_buckets(depth)
    return nb, probe_limit(depth, nb), slots_of(depth, tier)


# ---- k-mers: A C G T -> 0..3, step t (the t-th symbol from the END) at bits [2t, 2t+2); symbol codes 1 2 3 5 ----
def kmer_of(key, depth):
    return ACGT[[(key >> (2 * (depth - 1 - i))) & 3 for i in range(depth)]]


def key_of(kmer):
    key = 0
    for c in kmer:
        c = int(c)
        key = (key << 2) | (c - 1 - (c >> 2))
    return key


def text_of(reads):
    return ["".join("$ACGNT"[c] for c in r) for r in reads]


# ---- the builder's linear probing (sparse_table.hip, sparse_insert) ----
Fill = namedtuple("Fill", "can_fail max_displacement occupancy wanted")


def _occupancy(home, slots):
    """slots taken per bucket once every key is in (the same for every insertion order, with unbounded probing), and how many asked"""
    occ, wanted, carry, b = {}, {}, 0, None
    for h in sorted(home):
        if b is not None:
            while carry and b < h:
                wanted[b] = carry
                occ[b] = min(slots, carry)
                carry -= occ[b]
                b += 1
        b = h
        wanted[b] = home[h] + carry
        occ[b] = min(slots, wanted[b])
        carry = wanted[b] - occ[b]
        b += 1
    while carry:
        wanted[b] = carry
        occ[b] = min(slots, carry)
        carry -= occ[b]
        b += 1
    return occ, wanted


def simulate_fill(keys, nbuckets, probe, slots, *, depth):
    """Linear probing over buckets of `slots` entries.  A key's displacement is largest when it is inserted LAST (buckets only fill up), so
    the worst order for a key is every other key first: can_fail = some key then finds buckets home .. home + probe full;
    max_displacement = the farthest any order puts any key.  occupancy / wanted: per bucket, order-independent (wanted = the header)."""
    home = Counter(bucket_of(mix(k, depth), depth, nbuckets) for k in keys)
    can_fail, worst = False, 0
    full, _ = _occupancy(home, slots)
    for h in home:
        if full[h] < slots:     # room in its own bucket whatever came first
            continue
        rest = Counter(home)
        rest[h] -= 1
        occ, _ = _occupancy(+rest, slots)
        d = 0
        while occ.get(h + d, 0) >= slots:
            d += 1
        worst = max(worst, d)
        can_fail |= d > probe
    occ, wanted = _occupancy(home, slots)
    return Fill(can_fail, worst, occ, wanted)


# ---- the planner ----
Crafted = namedtuple("Crafted", "group key mixed bucket tag mult")


def wish(group, bucket=None, n=1, mult=1, tag=None, low=None, key=None):
    """n suffixes in `bucket` (mult: how often each occurs -- a number or n numbers; 0 = absent, a query only).  tag: the whole tag;
    low: its low 32 bits (40-bit layout: different high bytes); key: this very key, wherever it lands."""
    return dict(group=group, bucket=bucket, n=n, mult=mult, tag=tag, low=low, key=key)


class Plan:
    def __init__(self, depth, tier, nbuckets, probe, read_len, seed):
        self.depth, self.tier, self.nbuckets, self.probe, self.read_len, self.seed = depth, tier, nbuckets, probe, read_len, seed
        self.slots = slots_of(depth, tier)
        self.crafted = []          # present and absent (mult 0)
        self.rows = []             # one read_len row per crafted suffix: its read (present) or a query ending in it (absent)
        self.zones = set()
        self.reads = None          # (sum of mult, read_len) symbol codes

    def group(self, name, present=None):
        return [c for c in self.crafted if c.group == name and (present is None or (c.mult > 0) == present)]

    def present_keys(self, solid_only=False):
        return [c.key for c in self.crafted if c.mult > (1 if solid_only else 0)]

    def rows_of(self, name):
        return np.array([r for c, r in zip(self.crafted, self.rows) if c.group == name], dtype=np.uint8)


def _candidates(rng, depth, nbuckets, bucket, w, used, used_low):
    lo, hi = window_of(bucket, depth, nbuckets)
    bits = tag_bits(depth)
    if w["tag"] is not None or w["low"] is not None:
        mod = 1 << (bits if w["tag"] is not None else 32)
        want = w["tag"] if w["tag"] is not None else w["low"]
        first = lo + ((want - lo) % mod)
        cand = list(range(first, hi, mod))
        if w["low"] is not None:
            cand = [v for v in cand if tag_of(v, depth) != 0]
        order = rng.permutation(len(cand))
        for i in order:
            if cand[i] not in used:
                yield cand[i]
        return
    while True:  # any tag but 0, and (40-bit layout) no low word twice: coincidences are wished for, never met
        v = lo + int(rng.integers(0, hi - lo))
        if v in used or tag_of(v, depth) == 0 or (v & 0xFFFFFFFF) == 0 or (depth >= 30 and (bucket, v & 0xFFFFFFFF) in used_low):
            continue
        yield v


def make_plan(depth, tier, nbuckets, probe, wishes, read_len=READ_LEN, seed=1, also=()):
    """also: (nbuckets, buckets) pairs -- the reads' other windows keep out of these buckets of a table of that size as well"""
    assert read_len >= depth
    rng = np.random.default_rng(seed)
    plan = Plan(depth, tier, nbuckets, probe, read_len, seed)
    used, used_low = set(), set()
    for w in wishes:
        mults = w["mult"] if isinstance(w["mult"], (list, tuple)) else [w["mult"]] * w["n"]
        assert len(mults) == w["n"]
        if w["key"] is not None:
            v = mix(w["key"], depth)
            picks, bucket = [v], bucket_of(v, depth, nbuckets)
            assert v not in used
        else:
            bucket = w["bucket"]
            assert 0 <= bucket < nbuckets
            gen = _candidates(rng, depth, nbuckets, bucket, w, used, used_low)
            picks = []
            for _ in range(w["n"]):
                v = next(gen, None)
                if v is None:
                    raise ValueError("bucket %d of depth %d holds no %d values as wished (%s)" % (bucket, depth, w["n"], w["group"]))
                picks.append(v)
                used.add(v)
        for v, m in zip(picks, mults):
            used.add(v)
            used_low.add((bucket, v & 0xFFFFFFFF))
            assert bucket_of(v, depth, nbuckets) == bucket
            plan.crafted.append(Crafted(w["group"], unmix(v, depth), v, bucket, tag_of(v, depth), m))
        plan.zones.update(range(max(0, bucket - probe), min(nbuckets, bucket + probe + 1)))
    assert len({c.key for c in plan.crafted}) == len(plan.crafted)
    # prefixes: seeded rejection sampling -- no other window of a read may be homed in a protected zone (so none is a crafted suffix either)
    mask = (1 << (2 * depth)) - 1
    reads = []
    for c in plan.crafted:
        suffix = kmer_of(c.key, depth)
        for _ in range(MAX_TRIES):
            prefix = rng.integers(0, 4, size=read_len - depth)
            if c.mult == 0:
                break       # a query only: its prefix meets no table
            key, ok = c.key, True
            for code in prefix[::-1]:           # the window one symbol to the left: drop the last symbol, the new one on top
                key = ((key >> 2) | (int(code) << (2 * depth - 2))) & mask
                mixed = mix(key, depth)
                if bucket_of(mixed, depth, nbuckets) in plan.zones or any(bucket_of(mixed, depth, n) in zone for n, zone in also):
                    ok = False
                    break
            if ok:
                break
        else:
            raise RuntimeError("no prefix in %d tries for a suffix of group %s" % (MAX_TRIES, c.group))
        row = np.concatenate([ACGT[prefix], suffix])
        plan.rows.append(row)
        reads += [row] * c.mult
    plan.reads = np.array(reads, dtype=np.uint8)
    return plan


def query_rows(plan, seed, mutations=200):
    """(rows, group of every row): every crafted suffix behind its prefix, and single-symbol mutations of crafted suffixes behind fresh ones"""
    rng = np.random.default_rng(seed)
    rows = [np.array(plan.rows, dtype=np.uint8)]
    names = [c.group for c in plan.crafted]
    pick = rng.integers(0, len(plan.rows), size=mutations)
    mut = rows[0][pick].copy()
    mut[:, :plan.read_len - plan.depth] = ACGT[rng.integers(0, 4, size=(mutations, plan.read_len - plan.depth))]
    pos = rng.integers(plan.read_len - plan.depth, plan.read_len, size=mutations)
    mut[np.arange(mutations), pos] = ACGT[(np.searchsorted(ACGT, mut[np.arange(mutations), pos]) + rng.integers(1, 4, size=mutations)) % 4]
    rows.append(mut)
    names += ["mutated"] * mutations
    return np.ascontiguousarray(np.concatenate(rows)), names


# ---- the plans of tests/test_gpu_sparse_crafted.py (built and verified on the CPU by tests/test_sparse_craft.py) ----
CONFIGS = {"complete16": (16, False), "complete25": (25, False), "complete30": (30, False), "complete31": (31, False),
           "tier16": (16, True), "tier25": (25, True)}
REFILL_CONFIGS = ("complete16", "complete25", "tier16")
SATURATION = 400       # once-only suffixes in one bucket of a two-tier table: 1600 bits asked of the 256 the filter has


@functools.lru_cache(maxsize=None)
def tags_plan(config):
    """Tag 0, key 0, the all-T key, shared low tag words (40-bit layout), a saturated filter (two-tier form).  At the least bucket count a
    tag recurs every probe + 1 buckets exactly, so the buckets that hold a value with tag 0 are the multiples of probe + 1."""
    depth, tier = CONFIGS[config]
    nb, probe, slots = shape_of(depth, tier)
    c = probe + 1
    w = [wish("all_a", key=0, mult=1),
         wish("all_t", key=(1 << (2 * depth)) - 1, mult=2),
         wish("tag0", bucket=5 * c, tag=0, mult=3), wish("beside_tag0", bucket=5 * c, n=4, mult=[1, 2, 2, 4]),
         wish("tag0", bucket=9 * c, tag=0, mult=300),
         wish("tag0_absent_empty", bucket=13 * c, tag=0, mult=0),
         wish("tag0_absent_partly", bucket=17 * c, tag=0, mult=0), wish("filler", bucket=17 * c, n=3, mult=2),
         wish("tag0_absent_full", bucket=21 * c, tag=0, mult=0), wish("filler", bucket=21 * c, n=slots, mult=2)]
    if depth >= 30:
        low = 0x5EEDBEE5
        w += [wish("shared_zero", bucket=25 * c, low=0, n=3, mult=[2, 3, 4]), wish("shared_zero_absent", bucket=25 * c, low=0, mult=0),
              wish("shared_word", bucket=25 * c, low=low, n=3, mult=[5, 6, 7]), wish("shared_word_absent", bucket=25 * c, low=low, mult=0),
              # more of them than a bucket holds: whichever the fill displaces, both buckets keep entries that share their low words
              wish("pushed_zero", bucket=29 * c, low=0, n=9, mult=list(range(2, 11))), wish("pushed_zero_absent", bucket=29 * c, low=0, mult=0),
              wish("pushed_word", bucket=29 * c, low=low, n=8, mult=list(range(11, 19))), wish("pushed_word_absent", bucket=29 * c, low=low, mult=0)]
    if tier:
        w += [wish("saturating", bucket=33 * c, n=SATURATION, mult=1), wish("saturated_absent", bucket=33 * c, n=40, mult=0)]
    return make_plan(depth, tier, nb, probe, w, seed=100 + depth + int(tier))


def chain_buckets(config):
    nb = shape_of(*CONFIGS[config])[0]
    return {"first": 0, "middle": nb // 2 + 3, "last": nb - 1}


@functools.lru_cache(maxsize=None)
def chains_plan(config):
    """slots * probe + 1 suffixes homed in one bucket B and none in B + 1 .. B + probe: B .. B + probe - 1 are full and ONE entry lies exactly
    `probe` buckets from home -- at B = 0, mid-table and B = nbuckets - 1 (the chain then ends in the last line there is).  Two-tier: the
    chain's entries occur twice, and suffixes that occur once are homed in B beside them (filter bits at distance 0, the walk goes on)."""
    depth, tier = CONFIGS[config]
    nb, probe, slots = shape_of(depth, tier)
    w = [wish("all_a_absent", key=0, mult=0), wish("all_t_absent", key=(1 << (2 * depth)) - 1, mult=0)]   # (key 0 is homed in the first chain's bucket)
    for name, b in chain_buckets(config).items():
        n = slots * probe + 1
        w.append(wish("chain_" + name, bucket=b, n=n, mult=2 if tier else [1 + (i % 3 == 0) for i in range(n)]))
        if tier:
            w.append(wish("once_" + name, bucket=b, n=6, mult=1))
        w.append(wish("absent_" + name, bucket=b, n=4, mult=0))
        for d in range(1, probe + 1):
            if b + d < nb:
                w.append(wish("behind_" + name, bucket=b + d, n=2, mult=0))   # sees a foreign chain
    return make_plan(depth, tier, nb, probe, w, seed=200 + depth + int(tier))


@functools.lru_cache(maxsize=None)
def refill_plan(config):
    """One suffix more than a full chain holds, slots * (probe + 1) + 1 in one bucket: the fill fails whatever the order, and the loader's
    answer -- a quarter more buckets -- must hold them.  The grown table's buckets are 4/5 as wide, so the suffixes are spread over the
    two new buckets the old one lies in such that every order succeeds there."""
    depth, tier = CONFIGS[config]
    nb, probe, slots = shape_of(depth, tier)
    nb2 = nb + nb // 4
    probe2 = probe_limit(depth, nb2)
    n = slots * (probe + 1) + 1
    rng = np.random.default_rng(300 + depth + int(tier))
    def smaller_part(b):                        # an old bucket lies in two of the new ones: the size of its smaller part
        lo, hi = window_of(b, depth, nb)
        first, last = bucket_of(lo, depth, nb2), bucket_of(hi - 1, depth, nb2)
        return min(window_of(first, depth, nb2)[1] - lo, hi - window_of(last, depth, nb2)[0]) if last == first + 1 else 0

    b = max(range(nb // 2, nb // 2 + 8), key=smaller_part)
    lo, hi = window_of(b, depth, nb)
    parts = {}
    for _ in range(20 * n):
        v = lo + int(rng.integers(0, hi - lo))
        if tag_of(v, depth) != 0 and (v & 0xFFFFFFFF) != 0:
            parts.setdefault(bucket_of(v, depth, nb2), []).append(unmix(v, depth))
    parts = [list(dict.fromkeys(parts[k])) for k in sorted(parts)]
    assert len(parts) == 2 and min(len(p) for p in parts) >= n
    for a in sorted(range(1, n), key=lambda a: max(a, n - a)):   # the most even split over the two new buckets that no insertion order can make fail
        keys = parts[0][:a] + parts[1][:n - a]
        if not simulate_fill(keys, nb2, probe2, slots, depth=depth).can_fail:
            break
    else:
        raise RuntimeError("no split of %d suffixes survives the grown table" % n)
    wishes = [wish("refill", key=k, mult=300 if i == 0 else 2 if tier else 1 + (i % 2)) for i, k in enumerate(keys)]
    homes = {bucket_of(mix(k, depth), depth, nb2) for k in keys}
    near = {h + i for h in homes for i in range(-probe2, 2 * probe2 + 1)}
    plan = make_plan(depth, tier, nb, probe, wishes, seed=400 + depth + int(tier), also=[(nb2, near)])
    plan.grown = (nb2, probe2)
    return plan
