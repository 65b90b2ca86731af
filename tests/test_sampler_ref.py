"""The host model of the GPU neighbour sampler (tests/sampler_ref.py) on
the CPU: the scheme it states is uniform, its hub replica terminates early,
the columns the GPU tests use hold no 32-bit key ties, and samples drawn at
nearby seeds are unrelated."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_ref as S  # noqa: E402

CHI2_15DF_1E6 = 56.49   # upper 1e-6 quantile of chi-square, 15 d.o.f.


def test_hash_matches_its_integer_form_and_the_documented_rule():
    """The numpy and the Python-int restatements agree, arrays included, and
    the seed meets the counter only after the mix: seed 0 is not the
    identity, and d lands in the high word."""
    for seed in (0, 1, 99, 2**63 + 5, 2**64 - 1):
        ms = S.mix_seed(seed)
        j = np.array([0, 1, 63, 1024, 2**31, 2**32 - 1], dtype=np.uint64)
        for d in (0, 3, 2**32 - 1):
            want = [S._hash_int(ms, int(x), d) for x in j]
            assert S.hash_u32(seed, j, d).tolist() == want
            assert int(S.hash_u32(seed, np.uint64(63), d)) == want[2]
    assert S.mix_seed(0) != 0
    z = S.mix_seed(7) ^ (5 << 32) ^ 9
    assert int(S.hash_u32(7, 9, 5)) == S._fmix64(z) & 0xFFFFFFFF


def test_paths_follow_the_kernel_conditions():
    for deg, fanout, want in ((0, 5, "A"), (5, 5, "A"), (6, 5, "B"),
                              (1024, 64, "B"), (1025, 64, "C"),
                              (1025, 65, "D"), (1024, 65, "B"),
                              (1024, 1024, "A"), (1025, 1024, "D")):
        assert S.path_of(deg, fanout) == want
        assert S.path_of(deg, fanout, forced=True) == \
            ("A" if want == "A" else "D'")
    for deg, fanout in S.B_CASES:
        assert S.path_of(deg, fanout) == "B"
    for deg, fanout in S.C_CASES:
        assert S.path_of(deg, fanout) == "C"
    for deg, fanout in S.D_CASES:
        assert S.path_of(deg, fanout) == "D"
    coff, _, dst, kinds = S.mixed_case()
    assert len(dst) >= 64 and [kinds[d] for d in dst[:8]] == list("ABCD") * 2
    for fanout, want in ((64, "ABCC"), (65, "ABDD")):
        for i, d in enumerate(dst):
            deg = int(coff[d + 1]) - int(coff[d])
            assert S.path_of(deg, fanout) == want[i % 4]


def test_expected_sample_orders_by_key_then_slot():
    """Against a direct sort of (key, slot) tuples, on a column of repeated
    sources; path A is the column itself."""
    coff, rows = S.slot_csc([9, 300, 4], [0, 7, 0])
    src, cnt = S.expected_sample(coff, rows, 0, 9, seed=5)
    assert cnt == 9 and src.tolist() == list(range(9))
    info = {}
    src, cnt = S.expected_sample(coff, rows, 1, 40, seed=5, info=info)
    keys = S.hash_u32(5, 9 + np.arange(300, dtype=np.uint64))
    order = [j for _, j in sorted((int(k), j) for j, k in enumerate(keys))][:40]
    assert info["path"] == "B" and cnt == 40
    assert info["slots"].tolist() == order
    assert src.tolist() == [j % 7 for j in order]
    forced, _ = S.expected_sample(coff, rows, 1, 40, seed=5, forced=True)
    assert np.array_equal(forced, src)


def _chi2(counts):
    expect = counts.sum() / counts.size
    return float(((counts - expect) ** 2 / expect).sum())


@pytest.mark.parametrize("seed", [3, 99, 12345])
def test_scheme_is_uniform_over_slots(seed):
    """Chi-square over 16 slot bins (15 degrees of freedom) against the
    1e-6 quantile 56.49, for the k-smallest-keys scheme at a small and a
    large degree and for the hub rejection sampler.  Observed with the
    mixed seed, as (deg 16, deg 2048, hub): seed 3: 6.1, 13.1, 11.5;
    seed 99: 10.2, 6.9, 13.2; seed 12345: 12.8, 13.3, 15.1.  (Before the
    seed mix the same shapes gave 5 to 14.)"""
    got = []
    # 4096 destinations, deg 16, fanout 4, bin = slot
    counts = np.zeros(16)
    for d in range(4096):
        np.add.at(counts, S.smallest_slots(seed, 16 * d, 16, 4), 1)
    got.append(_chi2(counts))
    # 64 destinations, deg 2048, fanout 128, bin = slot // 128
    counts = np.zeros(16)
    for d in range(64):
        np.add.at(counts, S.smallest_slots(seed, 2048 * d, 2048, 128) // 128, 1)
    got.append(_chi2(counts))
    # 512 hub destinations, deg 2048, fanout 16, bin = slot // 128
    counts = np.zeros(16)
    for d in range(512):
        slots = np.asarray(S.hub_sample_host(seed, d, 2048, 16))
        assert S.path_of(2048, 16) == "C" and len(set(slots.tolist())) == 16
        np.add.at(counts, slots // 128, 1)
    got.append(_chi2(counts))
    print(f"seed {seed}: chi2 = " + ", ".join(f"{c:.1f}" for c in got))
    assert max(got) < CHI2_15DF_1E6, got


def test_hub_replica_finishes_in_few_rounds():
    """fanout 64 of deg 1025, the densest hub draw the kernel allows: about
    64^2 / 2 / 1025 = 2 picks collide in the first round and each re-roll
    collides again with probability < 64 / 1025, so needing more than 10
    rounds has probability around 1e-12; the kernel's limit is 100.
    Observed: at most 3."""
    worst = 0
    for d in range(300):
        slots, rounds = S.hub_sample_rounds(S.SEED, d, 1025, 64)
        assert len(slots) == 64 and len(set(slots)) == 64
        assert all(0 <= s < 1025 for s in slots)
        worst = max(worst, rounds)
    print("hub re-roll rounds, worst of 300:", worst)
    assert worst <= 10 < S.HUB_ROUNDS


def _gpu_test_columns():
    """(seed, e0, deg, compared) of every column the GPU sampler tests
    select keys in; `compared` where a test sets D (or B) against D'."""
    cols = []
    compared = {deg for deg, _ in S.B_CASES + S.D_CASES}
    for deg in sorted(compared | {deg for deg, _ in S.C_CASES}):
        coff, _ = S.case_csc(deg)
        cols += [(S.SEED, int(coff[d]), deg, deg in compared)
                 for d in range(3)]
    coff, _, _, _ = S.mixed_case()
    cols += [(S.SEED, int(coff[d]), int(coff[d + 1]) - int(coff[d]), True)
             for d in range(len(coff) - 1)]
    # tests/test_gpu_sampler.py: hubs of 50000, 2000, 1500 back to back,
    # the hub sampler and D' each against the model, never D against D'
    e0 = 0
    for deg in (50000, 2000, 1500):
        cols.append((99, e0, deg, False))
        e0 += deg
    return cols


def test_no_32bit_key_ties_in_the_gpu_test_columns():
    """With all keys of a column distinct, the 32-bit threshold search (D)
    and the 64-bit (key, slot) search (D') must pick the same set without
    leaning on the slot tie-break, so their comparison is meaningful: no
    tie at all in a column where the two are compared (deg <= 5000).  The
    other columns run the hub sampler, which draws no per-slot keys, or D'
    alone; there the CAP + 1 smallest keys, every candidate a threshold
    search could collect, are distinct.  (50000 keys of 32 bits hold
    50000^2 / 2^33 = 0.3 ties on average; the deg 50000 columns hold 1 or 2
    among their large keys.)"""
    for seed, e0, deg, compared in _gpu_test_columns():
        keys = np.sort(S.column_keys(seed, e0, deg))
        if not compared:
            keys = keys[:S.CAP + 1]
        assert (keys[1:] != keys[:-1]).all(), (seed, e0, deg)


BASE_SEEDS = (0, 1, 2, 3, 7, 99, 12345, 1000, 1001, 1002, 1003)
# (path, deg, fanout): independent samples share fanout^2 / deg <= fanout/16
DECORR_SHAPES = (("B", 512, 32), ("D", 2048, 128), ("C", 50000, 10),
                 ("C", 50000, 16))


@pytest.mark.parametrize("path,deg,fanout", DECORR_SHAPES)
def test_nearby_seeds_give_unrelated_samples(path, deg, fanout):
    """Per destination, S(seed ^ m) for m in {1, 2, 3, 8, 15}, and
    S(seed + 1), share fewer than fanout / 2 edge slots with S(seed) and
    with its translate {e ^ m}.  A seed that only XORs into the counter
    gives the full fanout: with the translate on B and D, with S(seed)
    itself on the hub path at fanout 16."""
    assert S.path_of(deg, fanout) == path
    coff, rows = S.slot_csc([deg] * 4)

    def edges(seed, d):
        slots, _, _ = S.expected_slots(coff, d, fanout, seed)
        assert len(set(slots.tolist())) == fanout
        return int(coff[d]) + slots

    for seed in BASE_SEEDS:
        for d in range(4):
            base = edges(seed, d)
            for other, mask in S.overlap_pairs(seed):
                S.check_overlap(base, edges(other, d), mask, fanout,
                                f"{path} deg {deg} dst {d}: seeds {seed}, "
                                f"{other}")
