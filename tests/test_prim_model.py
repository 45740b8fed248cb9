"""CPU checks of tests/prim_model.py, the references and inputs that tests/test_gpu_prims.py holds
the device scans and radix sort against: the references against literal arrays and against a
per-item loop, and every input's claimed property (the edge it is there for)."""
import random

import numpy as np

import prim_model as M

U64 = 0xFFFFFFFFFFFFFFFF


def test_excl_sum_reference_literals():
    assert M.excl_sum_u32([]).tolist() == []
    assert M.excl_sum_u32([9]).tolist() == [0]
    assert M.excl_sum_u32([1, 2, 3, 4]).tolist() == [0, 1, 3, 6]
    # mod 2^32, as the kernel's u32 adds
    assert M.excl_sum_u32([0xFFFFFFFF, 2, 0xFFFFFFFF, 5]).tolist() == [0, 0xFFFFFFFF, 1, 0]
    assert M.excl_sum_u32([0x80000000, 0x80000000, 7]).tolist() == [0, 0x80000000, 0]
    assert M.excl_sum_u32(np.ones(5000, np.uint32)).tolist() == list(range(5000))


SEG_LITERALS = [
    # keys, vals, expected
    ([], [], []),
    ([5], [9], [0]),
    # one run: the running maximum, shifted by one
    ([5, 5, 5, 5], [3, 1, 7, 2], [0, 3, 3, 7]),
    # every item its own run
    ([1, 2, 1, 2], [9, 9, 9, 9], [0, 0, 0, 0]),
    # A, B, A: the returning key starts a new run
    ([7, 7, 8, 7, 7], [10, 4, 99, 1, 2], [0, 10, 0, 0, 1]),
    # keys 0 and 0xFFFFFFFF
    ([0, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0], [5, 6, 7, 1, 9], [0, 5, 0, 7, 0]),
    # a decreasing run: its first value throughout
    ([4, 4, 4, 4], [50, 40, 30, 20], [0, 50, 50, 50]),
    # 2^64 - 1 survives; values that differ in one half only
    ([1, 1, 1], [U64, 0, 5], [0, U64, U64]),
    ([1, 1, 1, 1], [0x100000000, 0x200000000, 0x100000000, 0], [0, 0x100000000, 0x200000000, 0x200000000]),
    ([1, 1, 1, 1], [0x700000001, 0x700000003, 0x700000002, 0], [0, 0x700000001, 0x700000003, 0x700000003]),
    # all-zero values
    ([1, 1, 2, 2], [0, 0, 0, 0], [0, 0, 0, 0]),
]


def test_excl_max_by_key_reference_literals():
    for keys, vals, want in SEG_LITERALS:
        k = np.array(keys, np.uint32)
        v = np.array(vals, np.uint64)
        w = np.array(want, np.uint64)
        assert np.array_equal(M.excl_max_by_key_loop(k, v), w), (keys, vals)
        assert np.array_equal(M.excl_max_by_key(k, v), w), (keys, vals)
        assert np.array_equal(M.excl_max_by_key(k, v, few_runs=0), w), (keys, vals)


def test_excl_max_by_key_forms_equal_the_loop():
    rng = random.Random(20)
    for trial in range(60):
        n = rng.choice([1, 2, 3, 17, 100, 1000])
        nk = rng.choice([1, 2, 3, 50])
        stick = rng.choice([0.0, 0.5, 0.9, 0.99])
        keys, k = [], rng.randrange(nk)
        for _ in range(n):
            if rng.random() >= stick:
                k = rng.choice([0, 0xFFFFFFFF, rng.randrange(nk)])
            keys.append(k)
        vals = [rng.choice([0, U64, rng.getrandbits(64), rng.getrandbits(32), rng.getrandbits(32) << 32, 7])
                for _ in range(n)]
        k = np.array(keys, np.uint32)
        v = np.array(vals, np.uint64)
        want = M.excl_max_by_key_loop(k, v)
        assert np.array_equal(M.excl_max_by_key(k, v), want), trial
        assert np.array_equal(M.excl_max_by_key(k, v, few_runs=0), want), trial
    # the inputs' own patterns, at a size the loop still takes
    for kp in ("one", "alt", "aba", "tile", "tile_s", "chunk", "chunk_s", "edges", "zero_ff", "ff_zero"):
        for vp in ("dec", "inc", "zero", "max", "hi", "lo", "rand"):
            k, v, _ = M.seg_input(4097, kp, vp)
            want = M.excl_max_by_key_loop(k, v)
            assert np.array_equal(M.excl_max_by_key(k, v), want), (kp, vp)
            assert np.array_equal(M.excl_max_by_key(k, v, few_runs=0), want), (kp, vp)
    k, v, _ = M.seg_input(6 * M.TILE + 3, "long", "dec")
    assert np.array_equal(M.excl_max_by_key(k, v), M.excl_max_by_key_loop(k, v))
    assert np.array_equal(M.excl_max_by_key(k, v, few_runs=0), M.excl_max_by_key_loop(k, v))


def test_sort_pairs_reference_literals():
    k, v = M.sort_pairs(np.array([3, 1, 3, 0, 1], np.uint32), np.array([0, 1, 2, 3, 4], np.uint32))
    assert k.tolist() == [0, 1, 1, 3, 3] and v.tolist() == [3, 1, 4, 0, 2]        # equal keys keep their order
    k, v = M.sort_pairs(np.array([U64, 0, 1 << 63, 1 << 32], np.uint64), np.array([9, 8, 7, 6], np.uint32))
    assert k.tolist() == [0, 1 << 32, 1 << 63, U64] and v.tolist() == [8, 6, 7, 9]  # unsigned order
    k, v = M.sort_pairs(np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    assert k.size == 0 and v.size == 0 and k.dtype == np.uint32


def test_case_tables_hold_the_sizes_and_patterns():
    t, s = M.TILE, M.STILE
    scan_sizes = {0, 1, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049, 4097, 256 * t - 1, 256 * t, 256 * t + 1,
                  257 * t + 5, 513 * t + 1, 4096 * t, 4096 * t + 1}
    assert {c[0] for c in M.SUM_CASES} == scan_sizes
    assert {c[0] for c in M.SEG_CASES} == scan_sizes
    assert {c[1] for c in M.SUM_CASES} == {"ones", "zeros", "rand16", "randfull", "tile_edge", "tile_last",
                                           "tile_first"}
    assert {c[1] for c in M.SEG_CASES} == {"one", "alt", "aba", "tile", "tile_s", "chunk", "chunk_s", "edges", "long",
                                           "zero_ff", "ff_zero"}
    assert {c[2] for c in M.SEG_CASES} == {"dec", "inc", "zero", "max", "hi", "lo", "rand"}
    # exactly two cases at the switch of forms per primitive, the rest far below it
    for cases in (M.SUM_CASES, M.SEG_CASES):
        assert sorted(c[0] for c in cases if c[0] >= 4096 * t) == [4096 * t, 4096 * t + 1]
    # very many runs only up to 2^19 + 2^11 items; the carry-trip sizes carry the one-run and long-run patterns
    for n, kp, vp in M.SEG_CASES:
        if kp in ("alt", "aba", "chunk", "chunk_s", "zero_ff", "ff_zero"):
            assert n <= M.RAGGED_MAX, (n, kp)
    for n in (256 * t - 1, 256 * t, 256 * t + 1, 513 * t + 1):
        assert {"one", "long"} <= {c[1] for c in M.SEG_CASES if c[0] == n}
    sort_sizes = {0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8 * s, 9 * s + 1, 17 * s + 1, 33 * s - 1,
                  600 * s + 3}
    for kb, bits in ((4, {1, 8, 9, 12, 16, 17, 24, 25, 32}), (8, {33, 40, 63, 64, 0})):
        mine = [c for c in M.SORT_CASES if c[0] == kb]
        assert {c[1] for c in mine} == sort_sizes
        assert {c[3] for c in mine} == bits
        assert {c[2] for c in mine} == set(M.SORT_PATS) | {"dup"}
        assert {c[4] for c in mine} == {"iota", "randv"}
        assert len([c for c in mine if c[1] == 600 * s + 3]) == 1
        for n in sort_sizes - {0, 600 * s + 3}:
            assert {c[2] for c in mine if c[1] == n} == set(M.SORT_PATS), n
        for kp in ("mod3", "mod257"):
            assert all(c[4] == "iota" for c in mine if c[2] == kp)       # the stability cases
        for b in bits:
            assert {"rand", "extremes"} <= {c[2] for c in mine if c[3] == b}, b
    assert len(set(M.SUM_CASES)) == len(M.SUM_CASES) and len(set(M.SEG_CASES)) == len(M.SEG_CASES)
    assert len(set(M.SORT_CASES)) == len(M.SORT_CASES)


def test_sum_inputs_hold_their_claims():
    seen = set()
    for c in M.SUM_CASES:
        a, claims = M.sum_input(*c)
        assert a.dtype == np.uint32 and a.size == c[0]
        if c[0] < 10000:
            assert np.array_equal(a, M.sum_input(*c)[0])     # seeded: the same again
        for name in claims:
            assert M.claim_holds(name, a=a), (c, name)
        seen |= set(claims)
    assert seen == {"sum_all_ones", "sum_all_zero", "sum_below_2_16", "sum_wraps", "sum_nonzero_only_at_tile_edges",
                    "sum_single_nonzero_at_tile_last", "sum_single_nonzero_at_tile_first"}


def test_seg_inputs_hold_their_claims():
    seen = set()
    for c in M.SEG_CASES:
        k, v, claims = M.seg_input(*c)
        assert k.dtype == np.uint32 and v.dtype == np.uint64 and k.size == v.size == c[0]
        for name in claims:
            assert M.claim_holds(name, keys=k, vals=v), (c, name)
        seen |= set(claims)
    assert seen == {"seg_one_run", "seg_every_item_its_own_run", "seg_key_returns", "seg_runs_of_a_tile",
                    "seg_runs_of_a_tile_shifted", "seg_runs_of_a_chunk", "seg_runs_of_a_chunk_shifted",
                    "seg_boundaries_at_wave_and_tile_edge", "seg_long_run_then_short", "seg_keys_zero_and_ones",
                    "seg_3_whole_tiles_max_is_first", "seg_run_over_a_carry_trip", "seg_decreasing", "seg_increasing",
                    "seg_all_zero", "seg_has_u64_max", "seg_low_halves_equal", "seg_high_halves_equal"}
    # the run that a carry trip cannot hold is there in both forms' sizes
    for n in (513 * M.TILE + 1, 4096 * M.TILE, 4096 * M.TILE + 1):
        assert "seg_run_over_a_carry_trip" in M.seg_input(n, "long", "dec")[2]


def test_sort_inputs_hold_their_claims():
    seen = set()
    for c in M.SORT_CASES:
        kb, n, kp, bits, vp = c
        k, v, claims = M.sort_input(*c)
        assert k.dtype == (np.uint32 if kb == 4 else np.uint64) and v.dtype == np.uint32 and k.size == v.size == n
        if vp == "iota":
            assert np.array_equal(v, np.arange(n, dtype=np.uint32))
        for name in claims:
            assert M.claim_holds(name, keys=k, vals=v, bits=bits), (c, name)
        seen |= set(claims)
    assert seen == {"sort_keys_within_bits", "sort_all_equal", "sort_two_values", "sort_ascending", "sort_descending",
                    "sort_only_top_place_varies", "sort_only_bottom_place_varies", "sort_same_digit_in_every_place",
                    "sort_key_1000_times", "sort_zero_and_max_key", "sort_vals_have_u32_max"}


def test_claims_can_fail():
    """a claim is a check, not a label: each one is false on an input without the property"""
    k, v, _ = M.seg_input(5 * M.TILE, "alt", "inc")
    for name in ("seg_one_run", "seg_runs_of_a_tile", "seg_long_run_then_short", "seg_keys_zero_and_ones",
                 "seg_decreasing", "seg_all_zero", "seg_has_u64_max", "seg_low_halves_equal",
                 "seg_boundaries_at_wave_and_tile_edge", "seg_runs_of_a_chunk_shifted"):
        assert not M.claim_holds(name, keys=k, vals=v), name
    k, v, _ = M.seg_input(5 * M.TILE, "one", "rand")
    for name in ("seg_every_item_its_own_run", "seg_key_returns", "seg_increasing", "seg_high_halves_equal"):
        assert not M.claim_holds(name, keys=k, vals=v), name
    k, v, _ = M.seg_input(8 * M.TILE, "long", "inc")
    assert not M.claim_holds("seg_3_whole_tiles_max_is_first", keys=k, vals=v)
    assert not M.claim_holds("seg_run_over_a_carry_trip", keys=k, vals=v)
    k, v, _ = M.sort_input(4, 5000, "rand", 32, "iota")
    for name in ("sort_all_equal", "sort_two_values", "sort_ascending", "sort_descending", "sort_only_top_place_varies",
                 "sort_only_bottom_place_varies", "sort_same_digit_in_every_place", "sort_key_1000_times",
                 "sort_vals_have_u32_max"):
        assert not M.claim_holds(name, keys=k, vals=v, bits=32), name
    assert not M.claim_holds("sort_keys_within_bits", keys=k, vals=v, bits=9)
    a, _ = M.sum_input(5000, "rand16")
    for name in ("sum_all_ones", "sum_all_zero", "sum_wraps", "sum_nonzero_only_at_tile_edges",
                 "sum_single_nonzero_at_tile_last", "sum_single_nonzero_at_tile_first"):
        assert not M.claim_holds(name, a=a), name
    assert not M.claim_holds("sum_below_2_16", a=M.sum_input(5000, "randfull")[0])
    assert not M.claim_holds("sum_single_nonzero_at_tile_last", a=M.sum_input(4097, "tile_first")[0])
    assert not M.claim_holds("sum_single_nonzero_at_tile_first", a=M.sum_input(4097, "tile_last")[0])
