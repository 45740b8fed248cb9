"""Plain numpy references and named inputs for the device primitives under the dot-set folds, the
Orswot serializer and the GSet state writer (ce_scan.hip: ds_excl_sum_u32, ds_excl_max_by_key;
ce_ser_sort.hip: sort_pairs_u32 / sort_pairs_u64), as reached through ce_ctx_prim_*.

References:
  excl_sum_u32(a)              out[i] = sum of a[0..i) mod 2^32
  excl_max_by_key(keys, vals)  out[i] = max of the vals before i in i's run of adjacent equal keys,
                               0 at a run's first item (excl_max_by_key_loop: the same, one item at
                               a time; tests/test_prim_model.py holds the two against each other and
                               against literal arrays)
  sort_pairs(keys, vals)       both arrays in the order of a stable sort by key

Inputs: sum_input / seg_input / sort_input build one named pattern at one size from a fixed seed
and return the arrays with the names of the properties they claim; claim_holds() evaluates a claim,
and test_prim_model.py asserts every claim of every case in the tables below, so an edit that loses
an edge fails on the CPU.  The tables (SUM_CASES, SEG_CASES, SORT_CASES) are what
tests/test_gpu_prims.py and tests/prim_worker.py run.

The kernels' shapes the sizes are chosen by: the scans work on 2048-item tiles (256 threads x 8
items), 256 tiles per trip of their one-block carry kernels, and switch from the two-launch to the
three-launch form past 4096 tiles; the sort works on 4096-item tiles (4 waves x 1024 items, 64 at
a time), looks back 16 tiles at a time and keeps 8 histogram replicas."""
import zlib

import numpy as np

TILE = 2048           # scan tile
CHUNK = 8             # items per thread of a scan tile
WAVE_ITEMS = 512      # items per wave of a scan tile
TRIP = 256            # tiles per trip of k_scan_tile_sums / k_seg_carry
FORM_TILES = 4096     # the scans' default switch to the three-launch form is past this many tiles
STILE = 4096          # sort tile
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
U32_MAX = np.uint32(0xFFFFFFFF)
RAGGED_MAX = (1 << 19) + (1 << 11)   # the largest size given patterns with very many runs


# ---------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------
def excl_sum_u32(a):
    a = np.ascontiguousarray(a, dtype=np.uint32)
    out = np.zeros(a.size, np.uint32)
    if a.size > 1:
        np.cumsum(a[:-1], dtype=np.uint32, out=out[1:])
    return out


def run_starts(keys):
    """indices at which a run of adjacent equal keys begins"""
    keys = np.asarray(keys)
    if keys.size == 0:
        return np.zeros(0, np.int64)
    return np.flatnonzero(np.concatenate(([True], keys[1:] != keys[:-1])))


def excl_max_by_key(keys, vals, few_runs=4096):
    """few_runs: up to this many runs take the per-run form, more the all-at-once form (the answers
    are the same; the tests force each)"""
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    vals = np.ascontiguousarray(vals, dtype=np.uint64)
    n = keys.size
    assert vals.size == n
    out = np.zeros(n, np.uint64)
    if n == 0:
        return out
    st = run_starts(keys)
    if st.size <= few_runs:
        # few runs: a running maximum per run
        ends = np.append(st[1:], n)
        for s, e in zip(st.tolist(), ends.tolist()):
            if e - s > 1:
                np.maximum.accumulate(vals[s:e - 1], out=out[s + 1:e])
        return out
    # many runs: one running maximum over (run index, rank of the value) -- a later run's items all
    # compare above an earlier run's, so the maximum never crosses a run's start
    uniq, rank = np.unique(vals, return_inverse=True)
    rank = rank.astype(np.int64).reshape(n)
    run = np.zeros(n, np.int64)
    run[st[1:]] = 1
    run = np.cumsum(run)
    inc = np.maximum.accumulate(run * n + rank) - run * n     # inclusive, as ranks
    out[1:] = uniq[inc[:-1]]
    out[st] = 0
    return out


def excl_max_by_key_loop(keys, vals):
    """excl_max_by_key one item at a time, in Python ints"""
    out = []
    prev, cur = None, 0
    for k, v in zip([int(x) for x in keys], [int(x) for x in vals]):
        if prev is None or k != prev:
            prev, cur = k, 0
        out.append(cur)
        cur = max(cur, v)
    return np.array(out, dtype=np.uint64)


def sort_pairs(keys, vals):
    keys = np.asarray(keys)
    vals = np.asarray(vals)
    order = np.argsort(keys, kind="stable")
    return keys[order], vals[order]


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def _rng(*name):
    return np.random.default_rng(zlib.crc32(repr(name).encode()))


def _rand_u64(rng, n):
    return rng.integers(0, 1 << 64, size=n, dtype=np.uint64)


def _rand_u32(rng, n):
    return rng.integers(0, 1 << 32, size=n, dtype=np.uint32)


# ---- exclusive sum ----
def sum_input(n, pat):
    """(a u32[n], claims)"""
    rng = _rng("sum", n, pat)
    if pat == "ones":
        return np.ones(n, np.uint32), ["sum_all_ones"]
    if pat == "zeros":
        return np.zeros(n, np.uint32), ["sum_all_zero"]
    if pat == "rand16":
        return rng.integers(0, 1 << 16, size=n, dtype=np.uint32), ["sum_below_2_16"]
    if pat == "randfull":
        a = _rand_u32(rng, n)
        if n >= 7:
            a[:3] = 0xF0000000      # so the sum wraps whatever the draw
        if n:
            a[-1] = U32_MAX
        return a, (["sum_wraps"] if n >= 7 else [])
    if pat == "tile_edge":
        # nonzero only at a tile's last item and the next tile's first: the first boundary, the
        # boundary at a carry trip's end (tile 255 | 256) and the last one inside n
        a = np.zeros(n, np.uint32)
        for t in sorted({1, TRIP, (n - 1) // TILE}):
            if t >= 1 and t * TILE < n:
                a[t * TILE - 1] = 0x80000001 + t
                a[t * TILE] = 0x7FFFFFF0 + t
        return a, ["sum_nonzero_only_at_tile_edges"]
    if pat in ("tile_last", "tile_first"):
        # a single nonzero in the whole input: the last item of the last whole tile before n's, or
        # the first item of n's own
        a = np.zeros(n, np.uint32)
        t = (n - 1) // TILE
        a[t * TILE - (1 if pat == "tile_last" else 0)] = 0xC0000005
        return a, ["sum_single_nonzero_at_" + pat]
    raise KeyError(pat)


# ---- segmented exclusive max ----
KEY_A, KEY_B, KEY_C, KEY_D = 3, 0x80000008, 11, 0x00FFFF00


def _seg_keys(n, kp, rng):
    i = np.arange(n, dtype=np.int64)
    if kp == "one":
        return np.full(n, KEY_A, np.uint32), ["seg_one_run"]
    if kp == "alt":
        return np.where(i & 1, KEY_B, KEY_A).astype(np.uint32), ["seg_every_item_its_own_run"]
    if kp == "aba":
        # ragged runs of 1..40 items, keys A, B, A, C, ...: a key returns after another key
        ln = rng.integers(1, 41, size=n // 8 + 2)
        run = np.repeat(np.arange(ln.size), ln)[:n]
        return np.array([KEY_A, KEY_B, KEY_A, KEY_C], np.uint32)[run & 3], ["seg_key_returns"]
    if kp in ("tile", "tile_s"):
        run = (i + (TILE - 1 if kp == "tile_s" else 0)) // TILE
        return (run % 3 + 1).astype(np.uint32), ["seg_runs_of_a_tile" + ("_shifted" if kp == "tile_s" else "")]
    if kp in ("chunk", "chunk_s"):
        run = (i + (CHUNK - 1 if kp == "chunk_s" else 0)) // CHUNK
        return (run % 3 + 1).astype(np.uint32), ["seg_runs_of_a_chunk" + ("_shifted" if kp == "chunk_s" else "")]
    if kp == "edges":
        # boundaries exactly at 511 | 512 (wave edge) and 2047 | 2048 (tile edge)
        k = np.full(n, KEY_C, np.uint32)
        k[:WAVE_ITEMS] = KEY_A
        k[WAVE_ITEMS:TILE] = KEY_B
        return k, ["seg_boundaries_at_wave_and_tile_edge"]
    if kp == "long":
        # A | one run B over every whole tile between | a short run of A again | D to the end
        k = np.full(n, KEY_D, np.uint32)
        k[:1000] = KEY_A
        k[1000:n - 300] = KEY_B
        k[n - 300:n - 295] = KEY_A
        return k, ["seg_long_run_then_short"]
    if kp in ("zero_ff", "ff_zero"):
        # keys 0 and 0xFFFFFFFF only, tile by tile, so each is some tile's first item (and item 0's
        # key is 0 or 0xFFFFFFFF); a few switches inside tiles too
        odd = ((i // TILE) & 1) ^ (kp == "ff_zero")
        odd = odd ^ ((i % TILE >= 100) & (i % TILE < 103)) ^ (i % TILE == 1500)
        return np.where(odd, 0xFFFFFFFF, 0).astype(np.uint32), ["seg_keys_zero_and_ones"]
    raise KeyError(kp)


def _seg_vals(n, vp, rng):
    i = np.arange(n, dtype=np.uint64)
    if vp == "dec":
        return (np.uint64((1 << 63) + n) - i), ["seg_decreasing"]
    if vp == "inc":
        return i + np.uint64(1), ["seg_increasing"]
    if vp == "zero":
        return np.zeros(n, np.uint64), ["seg_all_zero"]
    if vp == "max":
        v = _rand_u64(rng, n)
        v[3::997] = U64_MAX
        if n:
            v[0] = U64_MAX
        return v, ["seg_has_u64_max"]
    if vp == "hi":
        return (_rand_u64(rng, n) & np.uint64(0xFFFFFFFF00000000)) | np.uint64(0x89ABCDEF), ["seg_low_halves_equal"]
    if vp == "lo":
        return (_rand_u64(rng, n) & np.uint64(0xFFFFFFFF)) | np.uint64(0x0123456700000000), ["seg_high_halves_equal"]
    if vp == "rand":
        return _rand_u64(rng, n), []
    raise KeyError(vp)


def seg_input(n, kp, vp):
    """(keys u32[n], vals u64[n], claims)"""
    rng = _rng("seg", n, kp, vp)
    keys, ck = _seg_keys(n, kp, rng)
    vals, cv = _seg_vals(n, vp, rng)
    claims = ck + cv
    if kp == "long" and vp == "dec":
        claims.append("seg_3_whole_tiles_max_is_first")
    if kp in ("one", "long") and n > TRIP * TILE + 2 * TILE:
        claims.append("seg_run_over_a_carry_trip")
    if n == 0:
        claims = []
    return keys.astype(np.uint32), vals.astype(np.uint64), claims


# ---- sort ----
def key_mask(bits, kbytes):
    w = 8 * kbytes
    b = w if bits <= 0 or bits > w else bits
    return (1 << b) - 1, b


def _sort_keys(n, kp, bits, kbytes, rng):
    dt = np.uint32 if kbytes == 4 else np.uint64
    mask, b = key_mask(bits, kbytes)
    places = (b + 7) // 8
    i = np.arange(n, dtype=np.uint64)

    def rand_below(width):
        if width >= 64:
            return _rand_u64(rng, n)
        return rng.integers(0, 1 << width, size=n, dtype=np.uint64)

    if kp == "equal":
        k = np.full(n, 0x5A5A5A5A5A5A5A5A & mask, np.uint64)
        claims = ["sort_all_equal"]
    elif kp == "alt2":
        k = np.where(i & np.uint64(1), np.uint64(0xA5A5A5A5A5A5A5A5 & mask), np.uint64(0x5A5A5A5A5A5A5A5A & mask))
        claims = ["sort_two_values"]
    elif kp in ("asc", "desc"):
        if mask >= max(n, 1):
            k = i * np.uint64(mask // max(n, 1))
        else:
            k = (i * np.uint64(mask + 1)) // np.uint64(max(n, 1))
        if kp == "desc":
            k = k[::-1].copy()
        claims = ["sort_ascending" if kp == "asc" else "sort_descending"]
    elif kp == "rand":
        k = rand_below(b)
        claims = []
    elif kp == "dup":
        # 1021 distinct values spread over every digit place, each many times over
        pool = rand_below(b)[:1021]
        k = pool[rng.integers(0, max(pool.size, 1), size=n)] if n else pool
        claims = ["sort_key_1000_times"] if n >= 2000 * 1021 else []
    elif kp == "top":
        shift = 8 * (places - 1)
        k = (rand_below(b - shift) << np.uint64(shift)) | np.uint64(0x3C3C3C3C3C3C3C3C & ((1 << shift) - 1))
        claims = ["sort_only_top_place_varies"]
    elif kp == "bottom":
        k = np.uint64(0xC3C3C3C3C3C3C300 & mask) | rand_below(min(8, b))
        claims = ["sort_only_bottom_place_varies"]
    elif kp == "ff":
        k = np.full(n, mask, np.uint64)
        claims = ["sort_same_digit_in_every_place", "sort_all_equal"]
    elif kp in ("mod3", "mod257"):
        m = 3 if kp == "mod3" else 257
        assert mask >= m - 1
        k = i % np.uint64(m)
        claims = ["sort_key_1000_times"] if n >= 1000 * m else []
    elif kp == "extremes":
        k = rand_below(b)
        if n >= 2:
            k[n // 3] = 0
            k[(2 * n) // 3] = mask
            k[0] = mask
            k[n - 1] = 0
        claims = ["sort_zero_and_max_key"] if n >= 2 else []
    else:
        raise KeyError(kp)
    return k.astype(dt), claims + ["sort_keys_within_bits"]


def sort_input(kbytes, n, kp, bits, vp):
    """(keys u32|u64[n], vals u32[n], claims)"""
    rng = _rng("sort", kbytes, n, kp, bits, vp)
    keys, claims = _sort_keys(n, kp, bits, kbytes, rng)
    if vp == "iota":
        vals = np.arange(n, dtype=np.uint32)
    elif vp == "randv":
        vals = _rand_u32(rng, n)
        vals[::5] = U32_MAX
        claims = claims + (["sort_vals_have_u32_max"] if n else [])
    else:
        raise KeyError(vp)
    if n == 0:
        claims = []
    return keys, vals, claims


# ---------------------------------------------------------------------------------------------
# claims
# ---------------------------------------------------------------------------------------------
def _whole_tile_runs(keys):
    """(start, end) of the runs that cover at least 3 whole tiles"""
    st = run_starts(keys)
    en = np.append(st[1:], keys.size)
    first_tile = (st + TILE - 1) // TILE
    last_tile = en // TILE
    ok = last_tile - first_tile >= 3
    return list(zip(st[ok].tolist(), en[ok].tolist())), (last_tile - first_tile)


def claim_holds(name, keys=None, vals=None, a=None, bits=0):
    """True when the arrays have the named property"""
    if name == "sum_all_ones":
        return bool((a == 1).all()) and np.array_equal(excl_sum_u32(a), np.arange(a.size, dtype=np.uint32))
    if name == "sum_all_zero":
        return not a.any()
    if name == "sum_below_2_16":
        return bool((a < (1 << 16)).all())
    if name == "sum_wraps":
        return int(a.astype(np.uint64).sum()) >= 1 << 32
    if name == "sum_nonzero_only_at_tile_edges":
        nz = np.flatnonzero(a)
        if a.size > TILE and nz.size < 2:
            return False
        return all((p % TILE) in (0, TILE - 1) for p in nz.tolist()) and \
            all((p + 1 in nz) if p % TILE == TILE - 1 else (p - 1 in nz) for p in nz.tolist())
    if name in ("sum_single_nonzero_at_tile_last", "sum_single_nonzero_at_tile_first"):
        nz = np.flatnonzero(a)
        at = TILE - 1 if name.endswith("last") else 0
        return nz.size == 1 and int(nz[0]) % TILE == at and int(nz[0]) >= TILE - 1
    n = keys.size
    st = run_starts(keys)
    en = np.append(st[1:], n)
    if name == "seg_one_run":
        return st.size == 1
    if name == "seg_every_item_its_own_run":
        return st.size == n
    if name == "seg_key_returns":
        rk = keys[st]
        return n < 3 * 40 or bool((rk[2:] == rk[:-2]).any() and (rk[1:] != rk[:-1]).all())
    if name in ("seg_runs_of_a_tile", "seg_runs_of_a_chunk"):
        L = TILE if "tile" in name else CHUNK
        return bool((st % L == 0).all()) and bool(((en - st)[:-1] == L).all())
    if name in ("seg_runs_of_a_tile_shifted", "seg_runs_of_a_chunk_shifted"):
        L = TILE if "tile" in name else CHUNK
        return bool((st[1:] % L == 1).all()) and bool(((en - st)[1:-1] == L).all()) and (n < 2 or st.size >= 2)
    if name == "seg_boundaries_at_wave_and_tile_edge":
        return n > TILE and st.tolist() == [0, WAVE_ITEMS, TILE]
    if name == "seg_long_run_then_short":
        # the longest run is followed by a run of at most 8 items, and other runs surround them
        j = int(np.argmax(en - st))
        return 0 < j < st.size - 2 and en[j + 1] - st[j + 1] <= 8 and keys[st[j + 1]] == keys[st[j - 1]] and \
            (n < 5 * TILE or (en[j] // TILE - (st[j] + TILE - 1) // TILE) >= 3)
    if name == "seg_keys_zero_and_ones":
        firsts = keys[::TILE]
        return set(np.unique(keys).tolist()) <= {0, 0xFFFFFFFF} and int(keys[0]) in (0, 0xFFFFFFFF) and \
            (n <= TILE or (0 in firsts and 0xFFFFFFFF in firsts))
    if name == "seg_3_whole_tiles_max_is_first":
        runs, _ = _whole_tile_runs(keys)
        return n < 5 * TILE or any(int(vals[s]) == int(vals[s:e].max()) for s, e in runs)
    if name == "seg_run_over_a_carry_trip":
        _, whole = _whole_tile_runs(keys)
        return int(whole.max()) > TRIP
    if name == "seg_decreasing":
        return n < 2 or bool((vals[1:] < vals[:-1]).all())
    if name == "seg_increasing":
        return n < 2 or bool((vals[1:] > vals[:-1]).all())
    if name == "seg_all_zero":
        return not vals.any()
    if name == "seg_has_u64_max":
        return bool((vals == U64_MAX).any())
    if name == "seg_low_halves_equal":
        lo, hi = vals & np.uint64(0xFFFFFFFF), vals >> np.uint64(32)
        return np.unique(lo).size == 1 and (n < 8 or np.unique(hi).size > 1)
    if name == "seg_high_halves_equal":
        lo, hi = vals & np.uint64(0xFFFFFFFF), vals >> np.uint64(32)
        return np.unique(hi).size == 1 and (n < 8 or np.unique(lo).size > 1)
    # sort
    mask, b = key_mask(bits, keys.dtype.itemsize)
    k = keys.astype(np.uint64)
    digits = [((k >> np.uint64(8 * p)) & np.uint64(0xFF)) for p in range((b + 7) // 8)]
    if name == "sort_keys_within_bits":
        return bool((k <= np.uint64(mask)).all())
    if name == "sort_all_equal":
        return np.unique(k).size == 1
    if name == "sort_two_values":
        return n < 2 or (np.unique(k).size == 2 and bool((k[1:] != k[:-1]).all()))
    if name == "sort_ascending":
        return n < 2 or bool((k[1:] >= k[:-1]).all() and k[-1] > k[0])
    if name == "sort_descending":
        return n < 2 or bool((k[1:] <= k[:-1]).all() and k[-1] < k[0])
    if name == "sort_only_top_place_varies":
        return all(np.unique(d).size == 1 for d in digits[:-1]) and (n < 64 or np.unique(digits[-1]).size > 1)
    if name == "sort_only_bottom_place_varies":
        return all(np.unique(d).size == 1 for d in digits[1:]) and (n < 64 or np.unique(digits[0]).size > 1)
    if name == "sort_same_digit_in_every_place":
        return all(np.unique(d).size == 1 for d in digits) and all(int(d[0]) == 0xFF for d in digits[:b // 8])
    if name == "sort_key_1000_times":
        return int(np.unique(k, return_counts=True)[1].max()) >= 1000
    if name == "sort_zero_and_max_key":
        return bool((k == 0).any() and (k == np.uint64(mask)).any())
    if name == "sort_vals_have_u32_max":
        return bool((vals == U32_MAX).any())
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------
SCAN_SMALL = [0, 1, 7, 8, 9, 511, 512, 513, 2047, 2048]
SCAN_MID = [2049, 4097]
SCAN_TRIP = [TRIP * TILE - 1, TRIP * TILE, TRIP * TILE + 1]
SCAN_TRIP2 = 257 * TILE + 5
SCAN_TRIP3 = 513 * TILE + 1            # third carry trip; k_seg_apply_direct folds 3 tiles per lane
SCAN_FORM = [FORM_TILES * TILE, FORM_TILES * TILE + 1]   # the last size of the two-launch form, the first of the other
SCAN_WORKER_MAX = SCAN_TRIP3


def _sum_cases():
    out = [(0, "ones")]
    for n in SCAN_SMALL[1:] + SCAN_MID:
        out += [(n, p) for p in ("ones", "zeros", "rand16", "randfull")]
    out += [(n, p) for n in SCAN_MID for p in ("tile_edge", "tile_last", "tile_first")]
    for n in SCAN_TRIP + [SCAN_TRIP2, SCAN_TRIP3]:
        out += [(n, p) for p in ("ones", "rand16", "randfull", "tile_edge", "tile_last", "tile_first")]
    out += [(n, "randfull") for n in SCAN_FORM]
    return out


def _seg_cases():
    out = [(0, "one", "rand")]
    every_val = ("inc", "zero", "max", "hi", "lo")
    for n in SCAN_SMALL[1:]:
        for kp in ("one", "alt", "aba", "chunk", "chunk_s", "zero_ff", "ff_zero"):
            out += [(n, kp, vp) for vp in ("dec", "rand")]
        out += [(n, "one", vp) for vp in every_val]
    for n in SCAN_MID:
        for kp in ("one", "alt", "aba", "tile", "tile_s", "chunk", "chunk_s", "edges", "zero_ff", "ff_zero"):
            out += [(n, kp, vp) for vp in ("dec", "rand")]
        out += [(n, kp, vp) for kp in ("one", "aba") for vp in every_val]
    for n in SCAN_TRIP:
        out += [(n, kp, vp) for kp in ("one", "long") for vp in ("dec", "inc", "rand", "max", "hi", "lo")]
    n = SCAN_TRIP[2]                       # the largest size with very many runs (<= RAGGED_MAX)
    for kp in ("alt", "aba", "tile", "tile_s", "chunk_s", "zero_ff", "ff_zero"):
        out += [(n, kp, vp) for vp in ("dec", "rand")]
    out += [(SCAN_TRIP2, kp, vp) for kp in ("one", "long", "tile_s") for vp in ("dec", "rand")]
    out += [(SCAN_TRIP3, kp, vp) for kp in ("one", "long", "tile", "tile_s") for vp in ("dec", "rand", "hi")]
    out += [(n, "long", "dec") for n in SCAN_FORM]
    return out


SORT_SIZES = [0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8 * STILE, 9 * STILE + 1, 17 * STILE + 1,
              33 * STILE - 1]
SORT_BIG = 600 * STILE + 3
SORT_WORKER_MAX = 33 * STILE - 1
SORT_BITS = {4: [1, 8, 9, 12, 16, 17, 24, 25, 32], 8: [33, 40, 63, 64, 0]}
SORT_PATS = ["equal", "alt2", "asc", "desc", "rand", "top", "bottom", "ff", "mod3", "mod257", "extremes"]
_MIN_BITS = {"mod3": 2, "mod257": 9}
_IOTA_PATS = ("equal", "alt2", "ff", "mod3", "mod257")


def _sort_cases():
    out = []
    for kb in (4, 8):
        blist = SORT_BITS[kb]
        for si, n in enumerate(SORT_SIZES):
            if n == 0:
                out.append((kb, 0, "rand", blist[-1], "iota"))
                continue
            for pi, kp in enumerate(SORT_PATS):
                # every bits value turns up under every pattern across the sizes
                ok = [b for b in blist if b == 0 or b >= _MIN_BITS.get(kp, 1)]
                bits = ok[(si + pi) % len(ok)]
                vp = "iota" if kp in _IOTA_PATS or (si + pi) % 2 else "randv"
                out.append((kb, n, kp, bits, vp))
        for n in (4097, 9 * STILE + 1):
            for bits in blist:
                out.append((kb, n, "rand", bits, "randv"))
                out.append((kb, n, "extremes", bits, "iota"))
        out.append((kb, SORT_BIG, "dup", blist[-1], "iota"))
    # the same case may come up twice (the rotation and the bits sweep)
    return sorted(set(out), key=out.index)


SUM_CASES = _sum_cases()
SEG_CASES = _seg_cases()
SORT_CASES = _sort_cases()


def sum_id(c):
    return "n%d-%s" % c


def seg_id(c):
    return "n%d-%s-%s" % c


def sort_id(c):
    return "u%d-n%d-%s-b%d-%s" % (8 * c[0], c[1], c[2], c[3], c[4])
