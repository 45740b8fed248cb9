"""GPU parity of CE_STATE_LWWREG (crdts 7 LWWReg<u64, u64>) through crdtenc.py and the C ABI,
bit-exact against tests/lwwreg_model.py: return code, per-file statuses, state_bytes() and
lwwreg_read(), and for compactions the decrypted file and its content name.  Files are sealed
with oracle.cryptor_encrypt.  Each test also asserts the path counters, so that none can pass by
sending its files down a slower route.  Without the kind, ce_core_open returns
CE_ERR_INVALID_ARG and every test here fails there."""
import ctypes
import functools
import hashlib
import itertools
import random

import msgpack
import numpy as np
import pytest

import crdtenc
import lwwreg_model as lm
from oracle.crdts import VClock

pytestmark = pytest.mark.gpu
H = bytes.fromhex
APP = H("aadfd5a66e194b24a8024fa27c72f20c")
CORE = crdtenc.CORE_VERSION
LW = crdtenc.STATE_LWWREG
U64 = (1 << 64) - 1
WIDTHS = [1, 2, 3, 5, 9]
# value range of each canonical width
RANGE = {1: (0, 0x80), 2: (0x80, 0x100), 3: (0x100, 0x10000), 5: (0x10000, 1 << 32), 9: (1 << 32, 1 << 64)}
CAPS = [None, 1, 3, 7]
INVALID = 64


@pytest.fixture(scope="module")
def ctx():
    c = crdtenc.Context(0)
    yield c
    c.close()


_OPEN = lm.open_file


@functools.lru_cache(maxsize=4096)
def _open_cached(key, supported, f):
    return _OPEN(key, list(supported), f)


@pytest.fixture(autouse=True)
def _memo_open(monkeypatch):
    """The model opens the same sealed bytes many times in the batch-size tests: memoized."""
    monkeypatch.setattr(lm, "open_file", lambda key, supported, f: _open_cached(key, tuple(supported), f))


def seal(oracle, key, clear, rng):
    st, enc = oracle.cryptor_encrypt(key, rng.randbytes(24), clear)
    assert st == 0
    return CORE + enc


def new_core(ctx, key, **kw):
    c = crdtenc.Core(ctx, kind=LW, supported=[APP], current_data_version=APP, **kw)
    c.set_latest_key(key)
    return c


def of_width(rng, w, span=None):
    lo, hi = RANGE[w]
    return rng.randrange(lo, hi if span is None else min(hi, lo + span))


def hdr(n):
    return bytes([0x90 | n]) if n < 16 else (b"\xdc" + n.to_bytes(2, "big") if n < 65536 else b"\xdd" + n.to_bytes(4, "big"))


def el(val, marker):
    return lm.enc_ops([(val, marker)])[1:]


def check_state(core, model):
    assert core.state_bytes() == model.serialize()
    assert core.lwwreg_read() == model.state.read()


def ingest_and_check(core, model, key, files, actors, fa, vers, want_rc=0):
    rc, st = core.ingest_ops(files, actors, fa, vers)
    orc, ost = model.read_remote_ops(key, [APP], files, [actors[i] for i in fa], vers)
    assert rc == orc == want_rc, (rc, orc, core.ctx.last_error())
    assert st == ost
    check_state(core, model)


def one_writer(oracle, rng, key, bodies, app=APP):
    """bodies as successive versions of one writer"""
    return [seal(oracle, key, app + b, rng) for b in bodies], [0] * len(bodies), list(range(len(bodies)))


def counts(core):
    """(fused, uniform, general, page) files"""
    return tuple(core.path_count("lww_%s_files" % k) for k in ("fused", "uniform", "general", "page"))


def all_uniform_fused(core, n):
    assert core.path_count("open_v3_lww") > 0
    assert counts(core) == (n, n, 0, 0), counts(core)


# ------------------------------------------------------------------ 1. rounds and widths
@pytest.mark.parametrize("wv,wm", list(itertools.product(WIDTHS, WIDTHS)))
def test_rounds_every_width_pair(ctx, oracle, wv, wm):
    """Every (val, marker) width pair at element counts around the lanes' rounds and at the page
    maximum; markers drawn from four values of the width, so ties fall everywhere.  All uniform."""
    rng = random.Random(100 + 10 * wv + wm)
    key, a = rng.randbytes(32), rng.randbytes(16)
    stride = 12 + wv + wm
    page_max = (4096 - 16 - 3) // stride
    assert {30: 135, 14: 291}.get(stride, page_max) == page_max
    ns = [0, 1, 15, 16, 17, 31, 32, 33, 65, page_max]
    bodies = [lm.enc_ops([(of_width(rng, wv), of_width(rng, wm, 4)) for _ in range(n)]) for n in ns]
    assert len(bodies[-1]) == 3 + page_max * stride
    assert len(APP + bodies[-1]) <= 4096 < len(APP + bodies[-1]) + stride  # one more would pass the page
    for order in (list(range(len(ns))), list(reversed(range(len(ns))))):
        files, fa, vers = one_writer(oracle, rng, key, [bodies[i] for i in order])
        core, model = new_core(ctx, key), lm.Core()
        ingest_and_check(core, model, key, files, [a], fa, vers)
        all_uniform_fused(core, len(ns))
        core.close()


# ------------------------------------------------------------------ 2. the winner's place in a file
POSITIONS = [("max_at", (0,)), ("max_at", (15,)), ("max_at", (16,)), ("max_at", (39,)),
             ("tie", (0, 16)), ("tie", (3, 19)), ("tie", (15, 31)), ("tie", (23, 39)),  # the same lane
             ("tie", (17, 32))]                                                         # the later one in a lower lane


@pytest.mark.parametrize("kind,pos", POSITIONS)
def test_winner_position_inside_a_file(ctx, oracle, kind, pos):
    rng = random.Random(200 + sum(pos))
    key, a = rng.randbytes(32), rng.randbytes(16)
    ops = [(1000 + i, 0x200 + rng.randrange(8)) for i in range(40)]
    for p in pos:
        ops[p] = (5000 + p, 0x300)  # equal largest markers, different vals
    files, fa, vers = one_writer(oracle, rng, key, [lm.enc_ops(ops)])
    core, model = new_core(ctx, key), lm.Core()
    ingest_and_check(core, model, key, files, [a], fa, vers)
    assert core.lwwreg_read() == (5000 + pos[0], 0x300)  # the earlier index wins
    all_uniform_fused(core, 1)
    core.close()


# ------------------------------------------------------------------ 3. the winner across files
@pytest.fixture(scope="module")
def tie_files(oracle):
    """Three one-element files: a low marker, and the largest marker with two different vals."""
    rng = random.Random(300)
    key = rng.randbytes(32)
    low, hi_a, hi_b = (seal(oracle, key, APP + lm.enc_ops([op]), rng) for op in ((7, 1), (100, 9), (200, 9)))
    return key, low, hi_a, hi_b


def _sizes(core):
    tile, blocks = core.path_count("lww_reduce_tile"), core.path_count("lww_reduce_max_blocks")
    assert tile >= 2 and blocks >= 2
    return tile, blocks


SIZE_NAMES = ["1", "2", "tile-1", "tile", "tile+1", "tiles*blocks-1", "tiles*blocks+1"]


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("size", SIZE_NAMES)
def test_winner_across_files(ctx, tie_files, monkeypatch, size, cap):
    """Equal largest markers with different vals in files f1 < f2, of one writer and of two, on
    either side of every edge of k_lww_reduce's tile, of a block's grid-stride step and of its final
    stage; the tile and the block bound are the library's own.  f1's val wins every time."""
    key, low, hi_a, hi_b = tie_files
    probe = new_core(ctx, key)
    T, B = _sizes(probe)
    probe.close()
    n = {"1": 1, "2": 2, "tile-1": T - 1, "tile": T, "tile+1": T + 1, "tiles*blocks-1": T * B - 1,
         "tiles*blocks+1": T * B + 1}[size]
    G = min(-(-n // T), B, cap or B)  # the reduce's grid
    if cap:
        monkeypatch.setenv("CE_TEST_GRID_CAP", str(cap))
    edges = {0, 1, 63, 64, T - 1, T, T + 1, 2 * T - 1, 2 * T, T * G - 1, T * G, T * G + 1, n - 2, n - 1}
    edges = sorted(e for e in edges if 0 <= e < n)
    pairs = list(zip(edges, edges[1:])) + [(edges[0], edges[-1])] if len(edges) > 1 else [(0, 0)]
    if n > 4 * T:  # the large batches: the tile's, the stride's and the last edge only
        keep = {(T - 1, T), (T, T + 1), (2 * T - 1, 2 * T), (T * G - 1, T * G), (n - 2, n - 1), (0, n - 1)}
        pairs = [p for p in pairs if p in keep]
    a, b = b"A" * 16, b"B" * 16
    for k, (f1, f2) in enumerate(pairs):
        files = [low] * n
        files[f1] = hi_a
        if f2 != f1:
            files[f2] = hi_b
        if k % 2 == 0 or f2 == f1:  # one writer
            actors, fa, vers = [a], [0] * n, list(range(n))
        else:                       # two: f2 is the second writer's first file
            actors, fa, vers = [a, b], [0] * f2 + [1] * (n - f2), list(range(f2)) + list(range(n - f2))
        core, model = new_core(ctx, key), lm.Core()
        ingest_and_check(core, model, key, files, actors, fa, vers)
        assert core.lwwreg_read() == (100, 9), (f1, f2)
        all_uniform_fused(core, n)
        assert (core.path_count("open_grid_capped") > 0) == bool(cap and -(-n // 4) > cap)
        core.close()


# ------------------------------------------------------------------ 4. the gate
def test_gate(ctx, oracle):
    rng = random.Random(400)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(2))
    mk = lambda v, m: seal(oracle, key, APP + lm.enc_ops([(v, m), (v + 1, m - 1)]), rng)
    core, model = new_core(ctx, key), lm.Core()
    ingest_and_check(core, model, key, [mk(1, 10), mk(2, 20)], actors, [0, 0], [0, 1])
    # a file below the writer's expected version holds the batch's largest marker: ignored
    ingest_and_check(core, model, key, [mk(3, 99), mk(4, 30), mk(5, 25)], actors, [0, 0, 1], [1, 2, 0])
    assert core.lwwreg_read() == (4, 30)
    # a gap: the files before it are folded, a larger marker after it is not
    files = [mk(6, 40), mk(7, 35), mk(8, 77), mk(9, 88)]
    ingest_and_check(core, model, key, files, actors, [0, 1, 1, 0], [3, 1, 3, 4], want_rc=13)
    assert core.lwwreg_read() == (6, 40) and list(core.writer_versions(b"".join(actors))) == [4, 2]
    # a shuffled order goes through the host gate file by file, as the model does
    files = [mk(10 + i, 50 + (i * 7) % 5) for i in range(12)]
    fa = [i % 2 for i in range(12)]
    vers = [model.nov.get(actors[i % 2]) + i // 2 for i in range(12)]
    order = list(range(12))
    rng.shuffle(order)
    ingest_and_check(core, model, key, [files[i] for i in order], actors, [fa[i] for i in order],
                     [vers[i] for i in order], want_rc=model_rc(model, key, files, actors, fa, vers, order))
    assert counts(core)[2:] == (0, 0) and counts(core)[0] == 2 + 3 + 4 + 12
    core.close()


def model_rc(model, key, files, actors, fa, vers, order):
    """what the model answers for this order, on a copy"""
    m = lm.Core()
    m.nov, m.state = VClock(dict(model.nov.dots)), lm.LWWReg(*model.state.read())
    return m.read_remote_ops(key, [APP], [files[i] for i in order], [actors[fa[i]] for i in order],
                             [vers[i] for i in order])[0]


# ------------------------------------------------------------------ 5. against the committed register
def test_against_the_committed_register(ctx, oracle):
    rng = random.Random(500)
    key, a = rng.randbytes(32), rng.randbytes(16)
    core, model = new_core(ctx, key), lm.Core()
    ver = [0]

    def put(ops, want):
        f = [seal(oracle, key, APP + lm.enc_ops(ops), rng)]
        ingest_and_check(core, model, key, f, [a], [0], [ver[0]])
        ver[0] += 1
        assert core.lwwreg_read() == want
        return f
    put([(5, 0), (6, 0)], (0, 0))            # marker-0 ops into a new core
    put([(11, 7)], (11, 7))
    put([(12, 7), (13, 7)], (11, 7))         # an equal marker with another val
    put([(14, 6), (15, 1)], (11, 7))         # lower markers
    put([(16, 8)], (16, 8))                  # a higher one
    f = put([(U64, U64), (1, U64), (0, U64 - 1)], (U64, U64))
    put([(3, U64)], (U64, U64))
    before = core.state_bytes()
    ingest_and_check(core, model, key, f, [a], [0], [5])  # the same batch again (replayed: gated out)
    ingest_and_check(core, model, key, f, [a], [0], [ver[0]])  # and as a new version
    assert core.state_bytes()[-30:] == before[-30:] and core.lwwreg_read() == (U64, U64)  # the same register bytes
    assert counts(core) == (9, 6, 3, 0)  # f, three times, mixes val widths: the general path
    core.close()


# ------------------------------------------------------------------ 6. the general path
def _general_bodies(rng):
    cf = lambda v=None, m=None: el(of_width(rng, 9) if v is None else v, of_width(rng, 9, 16) if m is None else m)
    bodies = []
    for pos in (0, 15, 16, 17, 39):  # a width change at one element
        els = [cf() for _ in range(40)]
        els[pos] = el(of_width(rng, 3), 1 << 63)
        bodies.append(hdr(40) + b"".join(els) + bytes(8))  # (count x the first stride fits: the lanes find it)
    bodies.append(hdr(3) + b"\x92\x07\xcd\x12\x34" + cf() + b"\x92\xcf" + (9).to_bytes(8, "big") + b"\x01")  # 92 v m
    bodies.append(msgpack.packb([{"marker": (1 << 50) + i % 3, "val": i} for i in range(20)]))  # reversed keys
    bodies.append(msgpack.packb([{"val": 1, "x": [1, {"y": b"z"}], "marker": 1 << 51},
                                 {"zz": None, "val": 2, "marker": 1 << 51}], use_bin_type=True))  # unknown keys
    bodies.append(hdr(4) + b"\x82\xa3val\xd0\x7f\xa6marker\xd1\x7f\xff" + b"\x82\xa3val\xd2\x7f\xff\xff\xff\xa6marker\xd3\x7f" +
                  b"\xff" * 7 + cf() + b"\x82\xa3val\xd3" + bytes(8) + b"\xa6marker\xd0\x00")  # d0..d3, >= 0
    bodies.append(hdr(3) + b"\x82\xa3val\xcf" + (7).to_bytes(8, "big") + b"\xa6marker\xcf" + (1 << 52).to_bytes(8, "big") +
                  b"\x82\xa3val\xce\x00\x00\x00\x08\xa6marker\xcd\x00\x09" + cf(3, 1 << 52))  # non-minimal forms
    bodies.append(msgpack.packb([{0: 5, 1: 1 << 53}, {1: 1 << 53, 0: 6}]))  # fields by index
    return bodies


def test_general_path_accepted_forms(ctx, oracle):
    rng = random.Random(600)
    key, a = rng.randbytes(32), rng.randbytes(16)
    bodies = _general_bodies(rng)
    files, fa, vers = one_writer(oracle, rng, key, bodies)
    core, model = new_core(ctx, key), lm.Core()
    ingest_and_check(core, model, key, files, [a], fa, vers)
    assert core.lwwreg_read()[1] == 1 << 63
    assert counts(core) == (len(bodies), 0, len(bodies), 0)
    core.close()
    # each alone in a fresh core, so that each one's own winner is what is read
    for b in bodies:
        files, fa, vers = one_writer(oracle, rng, key, [b])
        core, model = new_core(ctx, key), lm.Core()
        ingest_and_check(core, model, key, files, [a], fa, vers)
        assert counts(core) == (1, 0, 1, 0)
        core.close()


REJECTED = {
    "negative_d3": b"\x91\x82\xa3val\x07\xa6marker\xd3" + b"\xff" * 8,
    "negative_d3_after_good": hdr(2) + el(1, 1 << 40) + b"\x82\xa3val\x07\xa6marker\xd3\x80" + bytes(7),
    "repeated_key": b"\x91\x83\xa3val\x07\xa3val\x08\xa6marker\x09",
    "missing_key": b"\x91\x81\xa3val\x07",
    "count_larger_than_elements": hdr(3) + el(1, 2) + el(3, 4),
    "count_larger_uniform_cf": hdr(17) + el(1 << 40, 1 << 41) * 16,
    "cut_by_the_end": lm.enc_ops([(1 << 40, 1 << 41)] * 5)[:-4],
    "wrong_key_byte": b"\x91\x82\xa3vam\x07\xa6marker\x09",
    "wrong_key_byte_16th": hdr(20) + el(1 << 40, 1 << 41) * 16 + el(1 << 40, 1 << 41).replace(b"marker", b"markes") +
                           el(1 << 40, 1 << 41) * 3,
    "nil_marker": b"\x91\x82\xa3val\x07\xa6marker\xc0",
    "array_of_three": b"\x91\x93\x07\x09\x01",
    "top_level_map": b"\x82\xa3val\x07\xa6marker\x09",
    "empty_body": b"",
}


@pytest.mark.parametrize("name", list(REJECTED))
def test_general_path_rejected_forms(ctx, oracle, name):
    """Each is CE_ERR_DECODE for its file, alone and among good files; the register and
    next_op_versions stay as they were."""
    rng = random.Random(610)
    key, a = rng.randbytes(32), rng.randbytes(16)
    good = [lm.enc_ops([(of_width(rng, 9), of_width(rng, 9)) for _ in range(20)]) for _ in range(4)]
    for bodies in ([REJECTED[name]], good[:2] + [REJECTED[name]] + good[2:]):
        core, model = new_core(ctx, key), lm.Core()
        first, fa, vers = one_writer(oracle, rng, key, [lm.enc_ops([(77, 78)])])
        ingest_and_check(core, model, key, first, [a], fa, vers)
        before = core.state_bytes()
        files, fa, vers = one_writer(oracle, rng, key, bodies)
        ingest_and_check(core, model, key, files, [a], fa, [v + 1 for v in vers], want_rc=12)
        assert core.state_bytes() == before and core.lwwreg_read() == (77, 78)
        assert counts(core)[3] == 0
        core.close()


def test_overstated_count_after_a_full_page(ctx, oracle, monkeypatch):
    """One wave walks every group of four files (CE_TEST_GRID_CAP=1): a full page of cf elements is
    followed, in the same lane group, by a short file whose header overstates its count by one.  The
    LDS bytes past its end are the full page's well-formed elements; they are not its own."""
    rng = random.Random(620)
    key, a = rng.randbytes(32), rng.randbytes(16)
    full = lm.enc_ops([(of_width(rng, 9), of_width(rng, 9)) for _ in range(135)])
    short = b"\xdc\x00\x04" + lm.enc_ops([(of_width(rng, 9), 5 + (1 << 40)) for _ in range(3)])[1:]
    assert len(short) == 93 and full[93:98] == b"\x82\xa3val"
    bodies = [full if i % 8 < 4 else lm.enc_ops([(1, 2)] * 3) for i in range(64)]
    bodies[44] = short
    files, fa, vers = one_writer(oracle, rng, key, bodies)
    monkeypatch.setenv("CE_TEST_GRID_CAP", "1")
    core, model = new_core(ctx, key), lm.Core()
    ingest_and_check(core, model, key, files, [a], fa, vers, want_rc=12)
    assert model.read_remote_ops(key, [APP], files, [a] * 64, vers)[1][44] == 12 and core.lwwreg_read() == (0, 0)
    assert counts(core)[0] == 64 and core.path_count("open_grid_capped") > 0
    core.close()


# ------------------------------------------------------------------ 7. tail lengths
def test_every_tail_length(ctx, oracle):
    """Plaintexts of lengths 17..208 and the last 128 up to one page at 30-byte elements:
    APP || msgpack(Vec<LWWReg>) || trailing random bytes, which from_slice ignores."""
    rng = random.Random(700)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(6))
    lens = list(range(17, 17 + 192)) + list(range(4096 - 127, 4097))
    rng.shuffle(lens)
    per = -(-len(lens) // len(actors))
    files, fa, vers = [], [], []
    for i, L in enumerate(lens):
        k = max(0, min((L - 16 - 3) // 30, 135))
        k = rng.choice([k, k // 2, k])
        body = lm.enc_ops([(of_width(rng, 9), of_width(rng, 9, 64)) for _ in range(k)])
        assert 16 + len(body) <= L
        files.append(seal(oracle, key, APP + body + rng.randbytes(L - 16 - len(body)), rng))
        fa.append(i // per)
        vers.append(i % per)
    core, model = new_core(ctx, key), lm.Core()
    ingest_and_check(core, model, key, files, actors, fa, vers)
    all_uniform_fused(core, len(lens))
    core.close()


# ------------------------------------------------------------------ 8. tamper and key
@pytest.mark.parametrize("where", [0, 7, 15])
@pytest.mark.parametrize("fault", ["tag", "data_version"])
def test_tamper_rejects_the_batch(ctx, oracle, fault, where):
    rng = random.Random(800 + where)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(2))
    core, model = new_core(ctx, key), lm.Core()
    body = lambda: lm.enc_ops([(of_width(rng, 9), of_width(rng, 5)) for _ in range(rng.randrange(1, 60))])
    fa, vers = [0] * 8 + [1] * 8, list(range(8)) * 2
    first = [seal(oracle, key, APP + body(), rng) for _ in range(16)]
    ingest_and_check(core, model, key, first, actors, fa, vers)
    before, nov = core.state_bytes(), list(core.writer_versions(b"".join(actors)))
    good = [seal(oracle, key, APP + body(), rng) for _ in range(15)] + [seal(oracle, key, APP + lm.enc_ops([(1, U64)]), rng)]
    bad = list(good)
    if fault == "tag":
        b = bytearray(bad[where])
        b[-1] ^= 0x40
        bad[where], want = bytes(b), 9
    else:
        bad[where], want = seal(oracle, key, bytes(16) + body(), rng), 11
    vers2 = [v + 8 for v in vers]
    ingest_and_check(core, model, key, bad, actors, fa, vers2, want_rc=want)
    assert core.state_bytes() == before and list(core.writer_versions(b"".join(actors))) == nov
    ingest_and_check(core, model, key, good, actors, fa, vers2)
    assert core.lwwreg_read() == (1, U64) and counts(core)[2:] == (0, 0)
    core.close()


@pytest.mark.parametrize("tamper", [False, True])
def test_multi_key_retry(ctx, oracle, tamper):
    """CE_OPEN_MULTI_KEY: the winner sits in a file sealed under the older key, which opens on the
    retry and is decoded by k_decode_lww; a tampered file fails under every key."""
    from oracle import keys as K
    rng = random.Random(810)
    writer = rng.randbytes(16)
    ks = K.Keys()
    k_old, k_new = rng.randbytes(32), rng.randbytes(32)
    ks.insert_latest_key(writer, rng.randbytes(16), k_old)
    ks.insert_latest_key(writer, rng.randbytes(16), k_new)
    keys = crdtenc.Keys.decode(ks.to_bytes())
    assert keys.latest()[2] == k_new
    bodies = [lm.enc_ops([(of_width(rng, 9), of_width(rng, 5)) for _ in range(rng.randrange(1, 80))]) for _ in range(12)]
    bodies[4] = lm.enc_ops([(4, 1 << 40), (5, 1 << 40)])  # the winner, and a tie behind it in file 7
    bodies[7] = lm.enc_ops([(6, 1 << 40)])
    old = [i % 3 == 1 for i in range(12)]
    files = [seal(oracle, k_old if o else k_new, APP + b, rng) for b, o in zip(bodies, old)]
    assert old[4] and old[7]
    if tamper:
        b = bytearray(files[4])
        b[-2] ^= 1
        files[4] = bytes(b)
    core = crdtenc.Core(ctx, kind=LW, supported=[APP], current_data_version=APP, flags=crdtenc.OPEN_MULTI_KEY)
    core.set_keys(keys)
    empty = core.state_bytes()
    rc, st = core.ingest_ops(files, [writer], [0] * 12, list(range(12)))
    if tamper:
        assert rc == 9 and [i for i, s in enumerate(st) if s] == [4] and core.state_bytes() == empty
    else:
        model = lm.Core()
        same_key = [seal(oracle, k_new, APP + b, rng) for b in bodies]
        assert model.read_remote_ops(k_new, [APP], same_key, [writer] * 12, list(range(12)))[0] == 0
        assert rc == 0 and st == [0] * 12
        check_state(core, model)
        assert core.lwwreg_read() == (4, 1 << 40)
        assert counts(core)[0] == 8 and counts(core)[3] == 4  # the four files of the older key
    core.close()


# ------------------------------------------------------------------ 9. multi-page files
def _paged_body(rng, total, win_at, tie_after=None):
    """hdr || 30-byte elements || trailing bytes, `total` bytes of plaintext with APP; the largest
    marker at element win_at (and again, with another val, at tie_after)"""
    k = (total - 16 - 5) // 30
    ops = [(of_width(rng, 9), (1 << 40) + rng.randrange(1 << 20)) for _ in range(k)]
    ops[win_at % k] = (424242 + (1 << 33), 1 << 41)
    if tie_after is not None:
        ops[tie_after % k] = (1 << 34, 1 << 41)
    body = lm.enc_ops(ops)
    return body + rng.randbytes(total - 16 - len(body)), k


@pytest.mark.parametrize("where", ["first_page", "middle_page", "last_page"])
def test_multi_page_files(ctx, oracle, where):
    """Files of 4097 B, 2 pages, 5 pages and 70 KiB (more than four segments) among single-page
    ones; element 135 of the longer ones straddles the first page edge (16 + 3 + 135 * 30 = 4069 ..
    4099), and in the last file it is the winner."""
    rng = random.Random(900)
    key, a = rng.randbytes(32), rng.randbytes(16)
    bodies, n_big = [], 0
    for total in (4097, 8192, 5 * 4096, 70 * 1024):
        k = (total - 16 - 5) // 30
        at = {"first_page": 3, "middle_page": k // 2, "last_page": k - 1}[where]
        tie = None if at == k - 1 else k - 1
        body, k2 = _paged_body(rng, total, at, tie)
        assert len(APP + body) == total and k2 == k and k >= 135
        bodies.append(body)
        bodies.append(lm.enc_ops([(of_width(rng, 9), of_width(rng, 5)) for _ in range(rng.randrange(50))]))
        n_big += 1
    bodies.append(hdr(136) + el(1 << 40, (1 << 41) + 1) * 135 + el((1 << 33) + 9, U64) + bytes(3))  # the straddler wins
    n_big += 1
    assert len(APP + bodies[-1]) == 4102
    for upto in (len(bodies) - 1, len(bodies)):
        files, fa, vers = one_writer(oracle, rng, key, bodies[:upto])
        core, model = new_core(ctx, key), lm.Core()
        ingest_and_check(core, model, key, files, [a], fa, vers)
        big = n_big - (len(bodies) - upto)
        assert counts(core) == (upto - big, upto, 0, big), counts(core)
        assert core.lwwreg_read() == ((424242 + (1 << 33), 1 << 41) if upto < len(bodies) else ((1 << 33) + 9, U64))
        core.close()


def test_multi_page_general_path_and_truncation(ctx, oracle):
    rng = random.Random(910)
    key, a = rng.randbytes(32), rng.randbytes(16)
    mixed = lm.enc_ops([(of_width(rng, WIDTHS[i % 5]), of_width(rng, WIDTHS[(i // 5) % 5])) for i in range(400)])
    assert len(mixed) > 4096
    files, fa, vers = one_writer(oracle, rng, key, [mixed])
    core, model = new_core(ctx, key), lm.Core()
    ingest_and_check(core, model, key, files, [a], fa, vers)
    assert counts(core) == (0, 0, 1, 1)
    before = core.state_bytes()
    cut = lm.enc_ops([(of_width(rng, 9), of_width(rng, 9)) for _ in range(200)])[:-2]
    files, fa, vers = one_writer(oracle, rng, key, [lm.enc_ops([(3, 3)]), cut])
    ingest_and_check(core, model, key, files, [a], fa, [1, 2], want_rc=12)
    assert core.state_bytes() == before
    core.close()


# ------------------------------------------------------------------ 10. states
def _pack(x):
    return msgpack.packb(x, use_bin_type=True)


@pytest.mark.parametrize("n", [1, 2, 17])
def test_ingest_states(ctx, oracle, n):
    """n state files; two of them share the largest marker with different vals: the first in call
    order wins."""
    rng = random.Random(1000 + n)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(3))
    regs = [(100 + i, 50 + rng.randrange(5)) for i in range(n)]
    if n >= 2:
        regs[(n - 1) // 2], regs[n - 1] = (7, 99), (8, 99)
    sws = [lm.serialize(VClock({actors[i % 3]: i + 1}), lm.LWWReg(*r)) for i, r in enumerate(regs)]
    if n >= 2:
        sws[0] = _pack({"state": [regs[0][0], regs[0][1]], "next_op_versions": {"dots": {actors[0]: 1}}})  # other forms
    sfiles = [seal(oracle, key, APP + sw, rng) for sw in sws]
    core, model = new_core(ctx, key), lm.Core()
    rc, st = core.ingest_states(sfiles)
    assert (rc, st) == model.read_remote_states(key, [APP], sfiles) == (0, [0] * n)
    check_state(core, model)
    if n >= 2:
        assert core.lwwreg_read() == (7, 99)
    # then ops on top, and a rejected state file that leaves everything as it was
    f = [seal(oracle, key, APP + lm.enc_ops([(1, 99), (2, 100)]), rng)]
    ingest_and_check(core, model, key, f, actors, [0], [model.nov.get(actors[0])])
    before = core.state_bytes()
    bad = [sfiles[0], seal(oracle, key, APP + _pack({"next_op_versions": {"dots": {}}, "state": {"val": 1, "marker": -1}}), rng)]
    rc, st = core.ingest_states(bad)
    assert (rc, st) == model.read_remote_states(key, [APP], bad) == (12, [0, 12])
    assert core.state_bytes() == before
    core.close()


@pytest.mark.parametrize("route", ["merge_state", "merge_state_device", "ingest_states_device"])
def test_merge_state_routes(ctx, oracle, route):
    torch = pytest.importorskip("torch")
    rng = random.Random(1010)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(2))
    sws = [lm.serialize(VClock({actors[0]: 2}), lm.LWWReg(1, 9)),
           lm.serialize(VClock({actors[1]: 1, actors[0]: 5}), lm.LWWReg(2, 9)),   # an equal marker: ignored
           lm.serialize(VClock(), lm.LWWReg(3, 1 << 63))]
    core, model = new_core(ctx, key), lm.Core()
    if route == "ingest_states_device":
        sfiles = [seal(oracle, key, APP + sw, rng) for sw in sws]
        blob = b"".join(sfiles)
        offs = np.zeros(len(sfiles) + 1, dtype=np.int64)
        offs[1:] = np.cumsum([len(f) for f in sfiles])
        d_blob = torch.tensor(list(blob) + [0] * 64, dtype=torch.uint8, device="cuda")
        d_offs = torch.tensor(offs, device="cuda")
        torch.cuda.synchronize()
        rc, st = core.ingest_states_device(d_blob.data_ptr(), d_offs.data_ptr(), len(sfiles), len(blob), want_status=True)
        assert rc == 0 and st == [0] * len(sfiles)
        assert model.read_remote_states(key, [APP], sfiles)[0] == 0
        check_state(core, model)
    else:
        for i, sw in enumerate(sws):
            if route == "merge_state":
                assert core.merge_state(sw) == 0
            else:
                d = torch.tensor(list(sw), dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                assert core.merge_state_device(d.data_ptr(), len(sw)) == 0
            model.merge_state(sw)
            check_state(core, model)
            assert core.lwwreg_read() == ((1, 9) if i < 2 else (3, 1 << 63))
    assert core.merge_state(_pack({"next_op_versions": {"dots": {}}, "state": {"val": 1}})) == 12
    check_state(core, model)
    core.close()


def test_golden_states(ctx, oracle):
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lwwreg.json")) as f:
        fx = json.load(f)
    rng = random.Random(1020)
    key = rng.randbytes(32)
    for s in fx["states"]:
        core = new_core(ctx, key)
        rc, st = core.ingest_states([seal(oracle, key, APP + H(s["hex"]), rng)])
        assert rc == 0 and st == [0], s["name"]
        assert core.lwwreg_read() == ((s["val"], s["marker"]) if s["marker"] else (0, 0)), s["name"]
        want = H(s["hex"]) if s["marker"] else lm.serialize(lm.dec_state(H(s["hex"]))[0], lm.LWWReg())
        assert core.state_bytes() == want, s["name"]
        core.close()
    core, model = new_core(ctx, key), lm.Core()
    a = rng.randbytes(16)
    files, fa, vers = one_writer(oracle, rng, key, [H(c["hex"]) for c in fx["ops"]])
    ingest_and_check(core, model, key, files, [a], fa, vers)
    assert counts(core)[0] == len(files) and counts(core)[2] >= 2 and counts(core)[3] == 0  # (array form, reversed keys, mixed widths)
    core.close()


# ------------------------------------------------------------------ 11. compaction and writes
def _to_device(files, fa, vers):
    torch = pytest.importorskip("torch")
    blob = b"".join(files)
    offs = np.zeros(len(files) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(f) for f in files])
    d = (torch.tensor(list(blob) + [0] * 64, dtype=torch.uint8, device="cuda"),
         torch.tensor(offs, device="cuda"),
         torch.tensor(np.array(fa, dtype=np.int32), device="cuda"),
         torch.tensor(np.array(vers, dtype=np.int64), device="cuda"))
    torch.cuda.synchronize()
    return d, len(blob)


@pytest.mark.parametrize("flags", [0, crdtenc.COMPACT_INGEST_FORMAT])
def test_compact_to_buffer(ctx, oracle, flags):
    rng = random.Random(1100 + flags)
    key = rng.randbytes(32)
    nov = VClock()
    for _ in range(3):
        nov.apply(rng.randbytes(16), rng.randrange(1, 1 << 20))
    nonce = bytes(range(24))
    for reg in ((0, 0), (0x7f, 0x80), (0xffff, 0x10000), (U64, (1 << 32) - 1), (1 << 32, U64)):
        want = lm.serialize(nov, lm.LWWReg(*reg))
        core = new_core(ctx, key, flags=flags)
        assert core.merge_state(want) == 0 and core.state_bytes() == want
        f, name = core.compact_to_buffer(nonce=nonce)
        assert name == crdtenc.content_name(f) == oracle.base32_nopad(hashlib.sha3_256(f).digest())
        s, pt = oracle.cryptor_decrypt(key, f[16:])
        assert s == 0
        if flags:
            assert f[:16] == CORE and pt == APP + want
            fresh = new_core(ctx, key)
            rc, sts = fresh.ingest_states([f])
            assert rc == 0 and sts == [0] and fresh.state_bytes() == want
            fresh.close()
        else:
            assert f[:16] == APP and pt == want
        core.close()


@pytest.mark.parametrize("case", ["clean", "tampered", "gap"])
def test_compact_ops_device(ctx, oracle, case):
    """ce_core_compact_ops_device[_into] == ingest_ops_device + compact_to_buffer with the same nonce."""
    rng = random.Random(1110)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(4))
    files, fa, vers = [], [], []
    for a in range(4):
        for v in range(5):
            ops = [(of_width(rng, 9), of_width(rng, 5, 8)) for _ in range(20)]
            files.append(seal(oracle, key, APP + lm.enc_ops(ops), rng))
            fa.append(a)
            vers.append(v)
    if case == "tampered":
        b = bytearray(files[9])
        b[-3] ^= 1
        files[9] = bytes(b)
    if case == "gap":
        keep = [i for i in range(len(files)) if not (fa[i] == 0 and vers[i] == 2)]
        files, fa, vers = [files[i] for i in keep], [fa[i] for i in keep], [vers[i] for i in keep]
    (d_blob, d_offs, d_fa, d_fv), blen = _to_device(files, fa, vers)
    nonce = bytes(range(24))
    args = (d_blob.data_ptr(), d_offs.data_ptr(), len(files), blen, b"".join(actors), d_fa.data_ptr(), d_fv.data_ptr())
    model = lm.Core()
    orc, _ = model.read_remote_ops(key, [APP], files, [actors[i] for i in fa], vers)
    core = new_core(ctx, key)
    before = core.state_bytes()
    rc, f, name = core.compact_ops_device(*args, nonce=nonce)
    assert rc == orc, (rc, orc, ctx.last_error())
    if case == "tampered":
        assert rc == 9 and f is None and core.state_bytes() == before
    elif case == "gap":
        assert rc == 13 and f is None
        check_state(core, model)
    else:
        assert rc == 0
        check_state(core, model)
        s, pt = oracle.cryptor_decrypt(key, f[16:])
        assert s == 0 and f[:16] == APP and pt == model.serialize()
        assert name == crdtenc.content_name(f)
        ref = new_core(ctx, key)
        assert ref.ingest_ops_device(*args) == 0
        assert ref.compact_to_buffer(nonce=nonce) == (f, name)
        buf = np.zeros(1 << 16, np.uint8)
        c3 = new_core(ctx, key)
        rc3, ln, nm3 = c3.compact_ops_device_into(buf, *args, nonce=nonce, name=True)
        assert rc3 == 0 and bytes(buf[:ln]) == f and nm3 == name
        all_uniform_fused(c3, len(files))
        c3.close()
        ref.close()
    core.close()


def test_apply_ops_and_batch(ctx, oracle, tmp_path):
    """apply_ops, and apply_ops_batch of three blobs with ties; a second replica reads the files."""
    rng = random.Random(1120)
    key = rng.randbytes(32)
    remote = str(tmp_path / "remote")
    c1 = new_core(ctx, key, local_path=str(tmp_path / "l1"), remote_path=remote, flags=crdtenc.OPEN_CREATE)
    c2 = new_core(ctx, key, local_path=str(tmp_path / "l2"), remote_path=remote,
                  flags=crdtenc.OPEN_CREATE | crdtenc.COMPACT_INGEST_FORMAT)
    a1 = c1.info_actor()
    model = lm.Core()

    def local(ops):
        for op in ops:
            model.state.apply(op)
        model.nov.apply(a1, model.nov.get(a1) + 1)
        return lm.enc_ops(ops)
    assert c1.apply_ops(b"\x91\x82\xa3val\x01\xa6marker\xc0") == 12
    assert c1.apply_ops(local([(1, 5), (2, 5)])) == 0
    check_state(c1, model)
    assert c1.apply_ops(b"\x92\x92\x03\x05\x92\x04\x06") == 0  # the array form, applied in order
    local([(3, 5), (4, 6)])
    check_state(c1, model)
    rc, written = c1.apply_ops_batch([local([(10, 9), (11, 9)]), local([(12, 9)]), local([(13, 8), (14, 9)])])
    assert rc == 0 and len(written) == 3
    check_state(c1, model)
    assert c1.lwwreg_read() == (10, 9)
    assert c1.apply_ops_batch([lm.enc_ops([(5, 50)]), b"\x91\xc0"])[0] == 12  # nothing sealed or applied
    check_state(c1, model)
    assert c2.read_remote() == 0
    check_state(c2, model)
    rc, name = c2.compact()
    assert rc == 0 and crdtenc.Storage(str(tmp_path / "l2"), remote).list_state_names() == [name]
    c3 = new_core(ctx, key, local_path=str(tmp_path / "l3"), remote_path=remote, flags=crdtenc.OPEN_CREATE)
    assert c3.read_remote() == 0
    check_state(c3, model)
    c1.settle()
    c1.reset()
    assert c1.lwwreg_read() == (0, 0) and c1.state_bytes() == lm.Core().serialize()
    for c in (c1, c2, c3):
        c.close()


# ------------------------------------------------------------------ 12. refusals
def test_refusals(ctx, oracle):
    torch = pytest.importorskip("torch")
    rng = random.Random(1200)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(2))
    L = crdtenc.lib()
    vp = ctypes.c_void_p
    for kind in (crdtenc.STATE_GSET, crdtenc.STATE_GCOUNTER):
        other = crdtenc.Core(ctx, kind=kind, supported=[APP], current_data_version=APP)
        v, m = ctypes.c_uint64(77), ctypes.c_uint64(78)
        assert L.ce_core_lwwreg_read(other.p, ctypes.byref(v), ctypes.byref(m)) == INVALID
        assert (v.value, m.value) == (77, 78)
        other.close()
    core, model = new_core(ctx, key), lm.Core()
    core.register_actors(actors)
    files = [seal(oracle, key, APP + lm.enc_ops([(5, 6)]), rng)]
    ingest_and_check(core, model, key, files, actors, [0], [0])
    before = core.state_bytes()
    n = ctypes.c_uint64(77)
    assert L.ce_core_set_len(core.p, ctypes.byref(n)) == INVALID and n.value == 77
    mag, neg = (ctypes.c_uint64 * 2)(77, 78), ctypes.c_int(5)
    assert L.ce_core_counter_read(core.p, mag, ctypes.byref(neg)) == INVALID and list(mag) == [77, 78] and neg.value == 5
    out = (ctypes.c_uint64 * 2)(77, 78)
    assert L.ce_core_clock_get(core.p, ctypes.c_int(0), b"".join(actors), ctypes.c_uint32(2), out) == INVALID
    assert list(out) == [77, 78]
    b = crdtenc.Buf()
    assert L.ce_core_read_clock(core.p, ctypes.c_int(0), ctypes.byref(b)) == INVALID and not b.data and b.len == 0
    assert L.ce_core_mvreg_read(core.p, ctypes.byref(b)) == INVALID and not b.data and b.len == 0
    q = (ctypes.c_uint64 * 1)(5)
    ans = (ctypes.c_uint8 * 1)(9)
    assert L.ce_core_set_contains(core.p, q, ctypes.c_uint64(1), ans) == INVALID and ans[0] == 9
    cap = core.dense_capacity()
    buf = torch.full((2 * cap,), 7, dtype=torch.int64, device="cuda")
    nov = torch.full((cap,), 7, dtype=torch.int64, device="cuda")
    ready = ctypes.c_int(5)
    assert core.dense_ready() is False and L.ce_core_dense_ready(core.p) == 0
    assert L.ce_core_export_dense(core.p, vp(buf.data_ptr()), vp(nov.data_ptr())) == INVALID
    assert L.ce_core_import_dense(core.p, vp(buf.data_ptr()), vp(nov.data_ptr())) == INVALID
    (d_blob, d_offs, d_fa, d_fv), blen = _to_device([b"x" * 40], [0], [0])
    assert core.ingest_ops_device_sharded(d_blob.data_ptr(), d_offs.data_ptr(), 1, blen, b"".join(actors),
                                          d_fa.data_ptr(), d_fv.data_ptr(), nov.data_ptr()) == INVALID
    st = (ctypes.c_int32 * 1)(55)
    assert L.ce_core_gset_ingest_ops_device_sharded(core.p, vp(d_blob.data_ptr()), vp(d_offs.data_ptr()), ctypes.c_uint32(1),
                                                    ctypes.c_uint64(blen), b"".join(actors), ctypes.c_uint32(2),
                                                    vp(d_fa.data_ptr()), vp(d_fv.data_ptr()), vp(nov.data_ptr()), st) == INVALID
    assert st[0] == 55
    assert L.ce_core_gset_pending_members(core.p, vp(buf.data_ptr()), ctypes.c_uint64(cap), ctypes.byref(n)) == INVALID
    assert L.ce_core_gset_pending_commit(core.p, 1, None, None, ctypes.c_uint32(0)) == INVALID
    assert L.ce_core_pending_export(core.p, vp(buf.data_ptr()), ctypes.c_uint64(2 * cap), ctypes.byref(ready)) == INVALID
    assert L.ce_core_pending_commit(core.p, 1, None, ctypes.c_uint64(0)) == INVALID
    rc, k = core.export_columns_device(buf.data_ptr(), 16 * cap)
    assert rc == INVALID and k == 0
    torch.cuda.synchronize()
    assert ready.value == 5 and n.value == 77 and bool((buf == 7).all()) and bool((nov == 7).all())
    assert core.state_bytes() == before and core.lwwreg_read() == (5, 6)
    # ranks exchange state bytes
    peer, pm = new_core(ctx, key), lm.Core()
    ingest_and_check(peer, pm, key, [seal(oracle, key, APP + lm.enc_ops([(9, 6), (8, 7)]), rng)], actors, [1], [0])
    dev = torch.zeros(1 << 12, dtype=torch.uint8, device="cuda")
    for src, sm, dst, dm in ((core, model, peer, pm), (peer, pm, core, model)):
        rc, k = src.state_bytes_device(dev.data_ptr(), dev.numel())
        assert rc == 0 and bytes(dev[:k].cpu().numpy()) == sm.serialize()
        assert dst.merge_state_device(dev.data_ptr(), k) == 0
        dm.merge_state(sm.serialize())
        check_state(dst, dm)
    assert core.state_bytes() == peer.state_bytes() and core.lwwreg_read() == (8, 7)
    core.close()
    peer.close()
