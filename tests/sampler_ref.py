"""Plain host model of the GPU neighbour sampler (k_sample_reservoir,
nts_hip.hip): the key hash, the path each destination takes, and the exact
sample each path returns, order included.  Pure numpy and Python ints.

Keys.  launch_sampler mixes the caller's seed once on the host,
mseed = fmix64(seed + 0x9e3779b97f4a7c15), and the kernel's key for counter
(d, j) is the low 32 bits of fmix64(mseed ^ (d << 32) ^ j).  hash_u32 takes
the CALLER's seed, like the library's entry points do.

Paths, by the kernel's own conditions (CAP = 1024):
  A  deg <= fanout                      the column, in slot order
  B  fanout < deg <= CAP                the fanout smallest (key, slot)
  C  deg > CAP, fanout <= 64            O(fanout) rejection sampling
  D  deg > CAP, fanout > 64             the fanout smallest (key, slot)
  D' the forced test entry: every destination with deg > fanout selects the
     fanout smallest (key, slot) through the 64-bit bisection
where key = hash_u32(seed, e0 + slot) and B, D, D' differ only in how the
kernel finds the same set.
"""
import numpy as np

CAP = 1024
MAX_FANOUT = 1024
HUB_MAX_FANOUT = 64
HUB_ROUNDS = 100
_M64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15
_C1 = 0xFF51AFD7ED558CCD
_C2 = 0xC4CEB9FE1A85EC53


def _fmix64(z):
    z = ((z ^ (z >> 33)) * _C1) & _M64
    z = ((z ^ (z >> 33)) * _C2) & _M64
    return z ^ (z >> 33)


def mix_seed(seed):
    """sampler_mix_seed: what launch_sampler hands the kernel as its seed."""
    return _fmix64((int(seed) + _GOLDEN) & _M64)


def _hash_int(mseed, j, d=0):
    """k_hash_u32 on Python ints, from the already mixed seed."""
    return _fmix64(mseed ^ ((d & 0xFFFFFFFF) << 32) ^ (j & 0xFFFFFFFF)) \
        & 0xFFFFFFFF


def hash_u32(seed, j, d=0):
    """Bit-exact replica of the sampler's key for the caller's `seed`:
    k_hash_u32(sampler_mix_seed(seed), d, j).  `j` and `d` may be arrays."""
    z = (np.uint64(mix_seed(seed))
         ^ (np.asarray(d).astype(np.uint64) << np.uint64(32))) \
        ^ np.asarray(j).astype(np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(33))) * np.uint64(_C1)
        z = (z ^ (z >> np.uint64(33))) * np.uint64(_C2)
    return ((z ^ (z >> np.uint64(33))) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def hub_sample_rounds(seed, d, deg, fanout):
    """Replica of the kernel's O(fanout) hub rejection sampler (path C):
    slot_p = hash(seed, d, p | attempt << 10) % deg; a pick that equals an
    earlier pick's CURRENT slot re-rolls, round-synchronously, for at most
    HUB_ROUNDS rounds.  Returns (slots, rounds that re-rolled)."""
    ms = mix_seed(seed)
    d, deg = int(d), int(deg)
    slots = [_hash_int(ms, p, d) % deg for p in range(fanout)]
    attempts = [0] * fanout
    rounds = 0
    for _ in range(HUB_ROUNDS):
        seen, dup = set(), []
        for s in slots:             # earlier picks, this round's snapshot
            dup.append(s in seen)
            seen.add(s)
        if not any(dup):
            break
        rounds += 1
        for p in range(fanout):
            if dup[p]:
                attempts[p] += 1
                slots[p] = _hash_int(ms, p | (attempts[p] << 10), d) % deg
    return slots, rounds


def hub_sample_host(seed, d, deg, fanout):
    """The slots of hub_sample_rounds."""
    return hub_sample_rounds(seed, d, deg, fanout)[0]


def column_keys(seed, e0, deg):
    """The 32-bit keys of one column's edge slots e0 .. e0 + deg - 1 (the
    kernel adds e0 + j in 32 bits)."""
    e = (np.uint64(e0) + np.arange(deg, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)
    return hash_u32(seed, e)


def smallest_slots(seed, e0, deg, fanout):
    """Slots of the `fanout` smallest lexicographic (key, slot), smallest
    first: what paths B, D and D' must return."""
    keys = column_keys(seed, e0, deg)
    return np.lexsort((np.arange(deg), keys))[:fanout]


def path_of(deg, fanout, forced=False):
    """Which path the kernel takes: 'A', 'B', 'C', 'D', or "D'" (forced)."""
    if deg <= fanout:
        return "A"
    if forced:
        return "D'"
    if deg > CAP:
        return "C" if fanout <= HUB_MAX_FANOUT else "D"
    return "B"


def expected_slots(column_offset, dst, fanout, seed, forced=False):
    """(slots, path, hub re-roll rounds) of destination `dst`."""
    assert 0 < fanout <= MAX_FANOUT
    e0 = int(column_offset[dst])
    deg = int(column_offset[dst + 1]) - e0
    path = path_of(deg, fanout, forced)
    if path == "A":
        return np.arange(deg, dtype=np.int64), path, 0
    if path == "C":
        slots, rounds = hub_sample_rounds(seed, dst, deg, fanout)
        return np.asarray(slots, dtype=np.int64), path, rounds
    return smallest_slots(seed, e0, deg, fanout).astype(np.int64), path, 0


def expected_sample(column_offset, row_indices, dst, fanout, seed,
                    forced=False, info=None):
    """(src_ids, count) the kernel must write for destination `dst`: the
    first `count` entries of its out_src row, in order.  forced=True models
    nts_sample_reservoir_dbg_fallback.  A dict passed as `info` receives the
    path, the slots and, for path C, the number of re-roll rounds."""
    slots, path, rounds = expected_slots(column_offset, dst, fanout, seed,
                                         forced)
    if info is not None:
        info.update(path=path, slots=slots, rounds=rounds)
    e0 = int(column_offset[dst])
    return np.asarray(row_indices)[e0 + slots].astype(np.uint32), len(slots)


def slot_csc(degs, repeat_mod=None):
    """A CSC whose column d has degs[d] sources that encode the slot:
    row_indices[e0 + j] = j, or j % repeat_mod[d] where that is non-zero
    (a column with repeated sources)."""
    degs = np.asarray(degs, dtype=np.int64)
    coff = np.zeros(len(degs) + 1, dtype=np.int64)
    coff[1:] = np.cumsum(degs)
    rows = np.concatenate([np.arange(n, dtype=np.int64) for n in degs]
                          + [np.zeros(0, dtype=np.int64)])
    if repeat_mod is not None:
        for d, m in enumerate(repeat_mod):
            if m:
                rows[coff[d]:coff[d + 1]] %= m
    return coff.astype(np.uint32), rows.astype(np.uint32)


# ---- the cases of tests/test_gpu_sampler_paths.py, as (deg, fanout) ----
# Shared with the CPU tests, which check that none of these columns holds a
# 32-bit key tie (D and D' agree only through the slot tie-break otherwise).
SEED = 99
A_FANOUTS = (5, 70)
B_CASES = ((2, 1), (64, 63), (65, 1), (65, 64), (130, 65), (1024, 7),
           (1024, 1023))
C_CASES = ((1025, 1), (1025, 64), (4096, 13), (50000, 64))
D_CASES = ((1025, 65), (1025, 1024), (1500, 1024), (1500, 1000), (2048, 256),
           (5000, 65), (5000, 300))
REPEAT_MOD = 7


def case_csc(deg):
    """The three-column CSC one (deg, fanout) case runs on: slot-encoded,
    repeated sources (slot % 7), slot-encoded again at a later e0."""
    return slot_csc([deg, deg, deg], [0, REPEAT_MOD, 0])


# mixed-block launch: kinds cycle A, B, C, D at period 4 (one wave of each
# per 4-wave block); the degrees below keep their kind at fanout 64 and 65
MIXED_DEGS = {"A": (0, 1, 17, 64), "B": (66, 300, 777, 1024),
              "C": (1025, 4096, 1300, 2500), "D": (1026, 3000, 5000, 1700)}


def mixed_case():
    """(column_offset, row_indices, dst_list, kinds) of the mixed launch:
    16 columns, 80 entries, so every destination repeats five times."""
    degs, kinds = [], []
    for r in range(4):
        for kind in "ABCD":
            degs.append(MIXED_DEGS[kind][r])
            kinds.append(kind)
    coff, rows = slot_csc(degs, [REPEAT_MOD if d % 5 == 1 else 0
                                 for d in range(len(degs))])
    dst = np.arange(80, dtype=np.int64) % 16
    # rotate within each kind so a destination meets different neighbours
    dst = (dst + 4 * (np.arange(80) // 16)) % 16
    return coff, rows, dst.astype(np.int32), kinds


def overlap_pairs(seed, ms=(1, 2, 3, 8, 15)):
    """The (other seed, translate mask) pairs the decorrelation condition
    compares with `seed`: seed ^ m against S(seed) and its translate by m,
    and seed + 1 against S(seed) and its translate by seed ^ (seed + 1)."""
    pairs = [(seed ^ m, m) for m in ms]
    pairs.append((seed + 1, seed ^ (seed + 1)))
    return pairs


def check_overlap(base, other, mask, fanout, what):
    """The decorrelation condition on two samples of one destination, given
    as global edge slots e0 + slot: fewer than fanout / 2 shared with the
    other seed's sample and with its translate {e ^ mask}."""
    base, other = {int(e) for e in base}, {int(e) for e in other}
    same = len(base & other)
    shifted = len({e ^ mask for e in base} & other)
    assert 2 * same < fanout, f"{what}: {same} of {fanout} picks repeat"
    assert 2 * shifted < fanout, \
        f"{what}: {shifted} of {fanout} picks are the ^{mask} translate"
