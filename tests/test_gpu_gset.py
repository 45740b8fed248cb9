"""GPU parity of CE_STATE_GSET (crdts 7 GSet<u64>) through crdtenc.py and the C ABI, bit-exact
against tests/gset_model.py: return code, per-file statuses and state_bytes(), and for
compactions the decrypted file and its content name.  Files are sealed with
oracle.cryptor_encrypt.  Without the kind, ce_core_open returns CE_ERR_INVALID_ARG and every test
here fails there."""
import hashlib
import random

import msgpack
import numpy as np
import pytest

import crdtenc
import gset_model as gm
from oracle.crdts import VClock

pytestmark = pytest.mark.gpu
H = bytes.fromhex
APP = H("aadfd5a66e194b24a8024fa27c72f20c")
CORE = crdtenc.CORE_VERSION
GS = crdtenc.STATE_GSET
U64 = (1 << 64) - 1
# members of each canonical width: fixint, cc, cd, ce, cf
WIDTH_BITS = {"fixint": (0, 7), "cc": (7, 8), "cd": (8, 16), "ce": (16, 32), "cf": (32, 64)}
WIDTH_BYTES = {"fixint": 1, "cc": 2, "cd": 3, "ce": 5, "cf": 9}
SENTINELS = [0, 1, 1 << 63, U64 - 1, U64]
CAPS = [None, 1, 3, 7]


@pytest.fixture(scope="module")
def ctx():
    c = crdtenc.Context(0)
    yield c
    c.close()


def seal(oracle, key, clear, rng):
    st, enc = oracle.cryptor_encrypt(key, rng.randbytes(24), clear)
    assert st == 0
    return CORE + enc


def new_core(ctx, key, **kw):
    c = crdtenc.Core(ctx, kind=GS, supported=[APP], current_data_version=APP, **kw)
    c.set_latest_key(key)
    return c


def member_of(rng, width):
    lo, hi = WIDTH_BITS[width]
    return rng.randrange(1 << lo if lo else 0, 1 << hi)


def hdr(n):
    return bytes([0x90 | n]) if n < 16 else (b"\xdc" + n.to_bytes(2, "big") if n < 65536 else b"\xdd" + n.to_bytes(4, "big"))


def ingest_and_check(core, model, key, files, actors, fa, vers, want_rc=0):
    rc, st = core.ingest_ops(files, actors, fa, vers)
    orc, ost = model.read_remote_ops(key, [APP], files, [actors[i] for i in fa], vers)
    assert rc == orc == want_rc, (rc, orc, core.ctx.last_error())
    assert st == ost
    assert core.state_bytes() == model.serialize()


def one_writer(oracle, rng, key, bodies, app=APP):
    """bodies as successive versions of one writer"""
    return [seal(oracle, key, app + b, rng) for b in bodies], [0] * len(bodies), list(range(len(bodies)))


def paths(core):
    return core.path_count("gset_uniform_files"), core.path_count("gset_general_files")


def fused(core):
    """files decoded inside the fused open (k_open_fold_v3's GSet form), plaintext in LDS"""
    assert core.path_count("open_v3_gset") > 0
    return core.path_count("gset_fused_files")


# ------------------------------------------------------------------ decode rounds and widths
@pytest.mark.parametrize("width", list(WIDTH_BITS))
def test_decode_rounds_every_width(ctx, oracle, width):
    """Every width at counts around the lanes' rounds, and the page maximum for that width; all of
    them take the uniform-width path."""
    rng = random.Random(100 + list(WIDTH_BITS).index(width))
    key, a = rng.randbytes(32), rng.randbytes(16)
    page_max = (4096 - 16 - 3) // WIDTH_BYTES[width]
    assert {"cf": 453, "fixint": 4077}.get(width, page_max) == page_max
    counts = [0, 1, 15, 16, 17, 31, 32, 33, 65, page_max]
    bodies = [gm.enc_ops([member_of(rng, width) for _ in range(n)]) for n in counts]
    assert len(APP + bodies[-1]) <= 4096 < len(APP + bodies[-1]) + WIDTH_BYTES[width]
    files, fa, vers = one_writer(oracle, rng, key, bodies)
    core, model = new_core(ctx, key), gm.Core()
    ingest_and_check(core, model, key, files, [a], fa, vers)
    assert paths(core) == (len(counts), 0) and fused(core) == len(counts)
    core.close()


# ------------------------------------------------------------------ mixed widths
def test_mixed_widths_take_the_general_path(ctx, oracle):
    rng = random.Random(2)
    key, a = rng.randbytes(32), rng.randbytes(16)
    cf = lambda: gm.enc_ops([member_of(rng, "cf")])[1:]
    odd = gm.enc_ops([member_of(rng, "cd")])[1:]
    bodies = []
    for pos in (0, 39, 15, 16, 17):  # one odd element first, last, and around a 16-lane round
        els = [cf() for _ in range(40)]
        els[pos] = odd
        bodies.append(hdr(40) + b"".join(els))
    ws = list(WIDTH_BITS)
    bodies.append(gm.enc_ops([member_of(rng, ws[i % 5]) for i in range(200)]))  # widths alternating
    bodies.append(hdr(5) + b"\xd3" + (1 << 62).to_bytes(8, "big") + cf() + b"\xd0\x7f" + b"\xd1\x00\x05" +
                  b"\xd2\x7f\xff\xff\xff")
    bodies.append(hdr(4) + b"\xcf" + (77).to_bytes(8, "big") + b"\xce\x00\x00\x00\x4d" + b"\xcd\x00\x4d" + b"\xcc\x4d")
    bodies.append(hdr(3) + cf() + b"\xcf" + bytes(8) + b"\x00")  # zero, twice, in two forms
    files, fa, vers = one_writer(oracle, rng, key, bodies)
    core, model = new_core(ctx, key), gm.Core()
    ingest_and_check(core, model, key, files, [a], fa, vers)
    assert paths(core) == (0, len(bodies)) and fused(core) == len(bodies)
    assert {77, 0x7f, 5, 0x7fffffff, 1 << 62, 0} <= model.state.value
    core.close()


# ------------------------------------------------------------------ tail lengths
def test_every_tail_length(ctx, oracle, monkeypatch):
    """Plaintexts of every length mod 64 (and the last 128 lengths up to one page) at cf width:
    APP || msgpack(Vec<u64>) || trailing random bytes, which from_slice ignores.  The table starts
    large enough for the batch's ~60,000 members, so every file is decoded in the fused open."""
    monkeypatch.setenv("CE_GSET_CAP", str(1 << 18))
    rng = random.Random(7)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(6))
    lens = list(range(17, 17 + 192)) + list(range(4096 - 127, 4097))
    rng.shuffle(lens)
    per = -(-len(lens) // len(actors))
    files, fa, vers = [], [], []
    for i, L in enumerate(lens):
        k = max(0, min((L - 16 - 3) // 9, 453))
        k = rng.choice([k, k // 2, k])
        body = gm.enc_ops([member_of(rng, "cf") for _ in range(k)])
        assert 16 + len(body) <= L
        clear = APP + body + rng.randbytes(L - 16 - len(body))
        files.append(seal(oracle, key, clear, rng))
        fa.append(i // per)
        vers.append(i % per)
    core, model = new_core(ctx, key), gm.Core()
    ingest_and_check(core, model, key, files, actors, fa, vers)
    assert paths(core) == (len(lens), 0) and fused(core) == len(lens)
    core.close()


# ------------------------------------------------------------------ sentinel members
@pytest.mark.parametrize("route", ["ops", "state", "apply_ops"])
@pytest.mark.parametrize("when", ["before_growth", "after_growth"])
def test_sentinel_members(ctx, oracle, monkeypatch, route, when):
    """0, 1, 2^63, 2^64 - 2 and 2^64 - 1, alone and together, through each route, present before
    a growth of the table (64 slots, then 600 members) or inserted after it."""
    rng = random.Random(30 + len(route))
    key, a = rng.randbytes(32), rng.randbytes(16)
    monkeypatch.setenv("CE_GSET_CAP", "64")
    core, model = new_core(ctx, key), gm.Core()
    monkeypatch.delenv("CE_GSET_CAP")
    ver = [0]

    def ops_file(members):
        f = [seal(oracle, key, APP + gm.enc_ops(members), rng)]
        ingest_and_check(core, model, key, f, [a], [0], [ver[0]])
        ver[0] += 1

    def grow():
        ops_file([member_of(rng, "cf") for _ in range(600)])
        assert core.path_count("gset_grows") > 0

    def put(members):
        if route == "ops":
            ops_file(members)
        elif route == "state":
            sw = gm.serialize(VClock(), gm.GSet(members))
            rc, st = core.ingest_states([seal(oracle, key, APP + sw, rng)])
            assert rc == 0 and st == [0]
            model.merge_state(sw)
        else:
            assert core.apply_ops(gm.enc_ops(members)) == 0
            model.apply_ops(core.info_actor(), members)
        assert core.state_bytes() == model.serialize()
    if when == "after_growth":
        grow()
    for s in SENTINELS:
        put([s])
    put(SENTINELS)
    if when == "before_growth":
        grow()
    assert set(SENTINELS) <= model.state.value and core.state_bytes() == model.serialize()
    core.close()


# ------------------------------------------------------------------ duplicates and races
def test_duplicates_and_races(ctx, oracle):
    rng = random.Random(4)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(4))
    core, model = new_core(ctx, key), gm.Core()
    x = member_of(rng, "cf")
    # the same member in all four files of a wave's group (files 0..3), then a member repeated
    # inside a file
    bodies = [gm.enc_ops([x + 1, member_of(rng, "cf")]) for _ in range(4)] + [gm.enc_ops([x, 5, x, x, 5])]
    files, fa, vers = one_writer(oracle, rng, key, bodies)
    ingest_and_check(core, model, key, files, actors[:1], fa, vers)
    # the same 32 members in each of 256 files
    same = [member_of(rng, "cf") for _ in range(32)]
    files, fa, vers = [], [], []
    for i in range(256):
        m = list(same)
        rng.shuffle(m)
        files.append(seal(oracle, key, APP + gm.enc_ops(m), rng))
        fa.append(1 + i // 86)
        vers.append(i % 86)
    ingest_and_check(core, model, key, files, actors, fa, vers)
    n = len(model.state.value)
    # the count in the serialized header is the distinct count
    assert n == 3 + 4 + 32 and core.state_bytes().endswith(b"\xa5value\xdc\x00\x27" + gm.enc_ops(sorted(model.state.value))[3:])
    core.close()


# ------------------------------------------------------------------ growth
def test_growth(ctx, oracle, monkeypatch):
    """CE_GSET_CAP=64 (read at ce_core_open): 5,000 distinct members in one batch, then 5,000
    more over three batches; both tables double several times."""
    rng = random.Random(5)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(3))
    monkeypatch.setenv("CE_GSET_CAP", "64")
    core, model = new_core(ctx, key), gm.Core()
    monkeypatch.delenv("CE_GSET_CAP")
    nxt = [0, 0, 0]

    def batch(n_members):
        files, fa, vers = [], [], []
        ms = [member_of(rng, rng.choice(["cf", "cf", "ce"])) for _ in range(n_members)]
        for i in range(0, n_members, 100):
            w = (i // 100) % 3
            files.append(seal(oracle, key, APP + gm.enc_ops(ms[i:i + 100]), rng))
            fa.append(w)
            vers.append(nxt[w])
            nxt[w] += 1
        order = sorted(range(len(files)), key=lambda i: (fa[i], vers[i]))
        ingest_and_check(core, model, key, [files[i] for i in order], actors, [fa[i] for i in order],
                         [vers[i] for i in order])
    batch(5000)
    assert core.path_count("gset_batch_grows") >= 5 and core.path_count("gset_grows") >= 1
    assert core.path_count("gset_refolds") == 1  # the fused open hit the load bound once, then the refold grew the rest
    for n in (2000, 1000, 2000):
        batch(n)
    assert len(model.state.value) > 9900
    core.close()


# ------------------------------------------------------------------ all-or-nothing
@pytest.mark.parametrize("fault", ["tampered_tag", "decode_error_last", "data_version", "too_short"])
def test_all_or_nothing(ctx, oracle, fault):
    rng = random.Random(60 + len(fault))
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(3))
    core, model = new_core(ctx, key), gm.Core()

    def batch(v0, per=4):
        bodies = [[gm.enc_ops([member_of(rng, rng.choice(list(WIDTH_BITS))) for _ in range(rng.randrange(1, 60))])
                   for _ in range(per)] for _ in actors]
        fa = [w for w in range(3) for _ in range(per)]
        vers = [v0 + v for _ in range(3) for v in range(per)]
        return [seal(oracle, key, APP + b, rng) for bs in bodies for b in bs], fa, vers
    files, fa, vers = batch(0)
    ingest_and_check(core, model, key, files, actors, fa, vers)
    state_a, nov_a = core.state_bytes(), list(core.writer_versions(b"".join(actors)))
    assert nov_a == [4, 4, 4]
    good, fa, vers = batch(4)
    bad, want = list(good), None
    if fault == "tampered_tag":
        b = bytearray(bad[5])
        b[-1] ^= 0x40
        bad[5], want = bytes(b), 9
    elif fault == "decode_error_last":
        bad[-1], want = seal(oracle, key, APP + b"\x92\x01\xc0", rng), 12
    elif fault == "data_version":
        bad[3], want = seal(oracle, key, bytes(16) + gm.enc_ops([1]), rng), 11
    else:
        bad[7], want = seal(oracle, key, APP[:9], rng), 10
    ingest_and_check(core, model, key, bad, actors, fa, vers, want_rc=want)
    assert core.state_bytes() == state_a and list(core.writer_versions(b"".join(actors))) == nov_a
    ingest_and_check(core, model, key, good, actors, fa, vers)  # repaired: A u B
    assert core.state_bytes() != state_a
    core.close()


# ------------------------------------------------------------------ version gate
def test_version_gate(ctx, oracle):
    rng = random.Random(8)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(2))
    bodies = [gm.enc_ops([1000 * w + 10 * v + k for k in range(3)]) for w in range(2) for v in range(5)]
    files = [seal(oracle, key, APP + b, rng) for b in bodies]
    fa = [0] * 5 + [1] * 5
    vers = list(range(5)) * 2
    keep = [i for i in range(10) if i != 7]  # writer 1 misses version 2: a gap keeps the files before it
    core, model = new_core(ctx, key), gm.Core()
    ingest_and_check(core, model, key, [files[i] for i in keep], actors, [fa[i] for i in keep], [vers[i] for i in keep],
                     want_rc=13)
    assert model.nov.dots == {actors[0]: 5, actors[1]: 2} and 1020 not in model.state.value
    # replayed files (versions below the expected ones) whose members are absent insert nothing
    replay = [seal(oracle, key, APP + gm.enc_ops([777777 + i]), rng) for i in range(3)]
    before = core.state_bytes()
    ingest_and_check(core, model, key, replay, actors, [0, 0, 1], [1, 4, 0])
    assert core.state_bytes() == before
    core.close()


# ------------------------------------------------------------------ grammar
ACCEPTED = {
    "non_minimal": b"\x94\xcc\x05\xcd\x00\x06\xce\x00\x00\x00\x07\xcf" + bytes(7) + b"\x08",
    "signed_non_negative": b"\x94\xd0\x7f\xd1\x7f\xff\xd2\x7f\xff\xff\xff\xd3\x7f" + b"\xff" * 7,
    "array16_small": b"\xdc\x00\x02\x01\x02",
    "array32_small": b"\xdd\x00\x00\x00\x02\x01\x02",
    "array32_empty": b"\xdd\x00\x00\x00\x00",
    "array16_empty_then_bytes": b"\xdc\x00\x00\xff\xff",
    "trailing_bytes": b"\x92\x01\xcc\xff\xc1\xc1\xff",
    "empty_then_bytes": b"\x90\x05",
}
REJECTED = {
    "negative_fixint": b"\x92\x01\xff",
    "negative_d0": b"\x91\xd0\x80",
    "negative_d3": b"\x91\xd3\x80" + bytes(7),
    "float64": b"\x91\xcb" + bytes(8),
    "float32": b"\x91\xca" + bytes(4),
    "nil": b"\x91\xc0",
    "bool": b"\x91\xc3",
    "str": b"\x91\xa1a",
    "bin": b"\x91\xc4\x01a",
    "nested_array": b"\x91\x91\x01",
    "map": b"\x91\x81\x01\x02",
    "truncated_element": b"\x92\x01\xcf\x00\x00\x00",
    "truncated_uniform": b"\x92\xcf" + bytes(8) + b"\xcf\x00\x00",
    "count_past_the_bytes": b"\x93\x01\x02",
    "count32_past_the_bytes": b"\xdd\xff\xff\xff\xff\x01",
    "truncated_header": b"\xdc\x00",
    "top_level_map": b"\x80",
    "top_level_int": b"\x05",
    "empty_body": b"",
}


@pytest.mark.parametrize("name", list(ACCEPTED))
def test_grammar_accepted_forms(ctx, oracle, name):
    """One file each, as the only file of a batch and as one among good files."""
    rng = random.Random(9)
    key, a = rng.randbytes(32), rng.randbytes(16)
    good = [gm.enc_ops([member_of(rng, "cf") for _ in range(20)]) for _ in range(4)]
    for bodies in ([ACCEPTED[name]], good[:2] + [ACCEPTED[name]] + good[2:]):
        files, fa, vers = one_writer(oracle, rng, key, bodies)
        core, model = new_core(ctx, key), gm.Core()
        ingest_and_check(core, model, key, files, [a], fa, vers)
        core.close()


@pytest.mark.parametrize("name", list(REJECTED))
def test_grammar_rejected_forms(ctx, oracle, name):
    """Each is CE_ERR_DECODE for its file; nothing of its batch is inserted."""
    rng = random.Random(10)
    key, a = rng.randbytes(32), rng.randbytes(16)
    good = [gm.enc_ops([member_of(rng, "cf") for _ in range(20)]) for _ in range(4)]
    for bodies in ([REJECTED[name]], good[:2] + [REJECTED[name]] + good[2:]):
        core, model = new_core(ctx, key), gm.Core()
        first, fa, vers = one_writer(oracle, rng, key, [gm.enc_ops([77, 78])])
        ingest_and_check(core, model, key, first, [a], fa, vers)
        before = core.state_bytes()
        files, fa, vers = one_writer(oracle, rng, key, bodies)
        ingest_and_check(core, model, key, files, [a], fa, [v + 1 for v in vers], want_rc=12)
        assert core.state_bytes() == before
        core.close()


# ------------------------------------------------------------------ stale plaintext
def test_overstated_count_after_a_full_page(ctx, oracle, monkeypatch):
    """One wave walks every group of four files (CE_TEST_GRID_CAP=1) in the fused open: a full-page
    cf file is followed, in the same lane group (four files on), by a short file whose header
    overstates its count by one.  The LDS bytes past its end are the full page's plaintext, well-formed
    cf elements among them; they are not its own: CE_ERR_DECODE."""
    rng = random.Random(11)
    key, a = rng.randbytes(32), rng.randbytes(16)
    full = gm.enc_ops([member_of(rng, "cf") for _ in range(453)])
    # dc 00 04 and three elements: the body ends at offset 30, where the full page before it in the
    # region has an element boundary (3 + 9 k), so the stale bytes there are a well-formed cf element
    short = b"\xdc\x00\x04" + gm.enc_ops([member_of(rng, "cf") for _ in range(3)])[1:]
    assert len(short) == 30 and full[30:31] == b"\xcf"
    bodies = [full if i % 8 < 4 else gm.enc_ops([member_of(rng, "cf") for _ in range(3)]) for i in range(64)]
    bodies[44] = short
    files, fa, vers = one_writer(oracle, rng, key, bodies)
    monkeypatch.setenv("CE_TEST_GRID_CAP", "1")
    core, model = new_core(ctx, key), gm.Core()
    empty = core.state_bytes()
    ingest_and_check(core, model, key, files, [a], fa, vers, want_rc=12)
    assert model.read_remote_ops(key, [APP], files, [a] * 64, vers)[1][44] == 12 and core.state_bytes() == empty
    assert fused(core) == 64 and core.path_count("open_grid_capped") > 0
    core.close()


@pytest.mark.parametrize("cap", CAPS)
def test_mixed_batch_under_the_grid_cap(ctx, oracle, monkeypatch, cap):
    rng = random.Random(12)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(5))
    files, fa, vers = [], [], []
    for w in range(5):
        for v in range(60):
            kind = rng.randrange(4)
            if kind == 0:
                ms = [member_of(rng, "cf") for _ in range(rng.choice([0, 1, 16, 100, 453]))]
            elif kind == 1:
                ms = [member_of(rng, rng.choice(list(WIDTH_BITS))) for _ in range(rng.randrange(70))]
            elif kind == 2:
                ms = [member_of(rng, "fixint") for _ in range(rng.choice([5, 1000, 4077]))]
            else:
                ms = [rng.choice(SENTINELS) for _ in range(rng.randrange(1, 9))]
            body = gm.enc_ops(ms)
            files.append(seal(oracle, key, APP + body + rng.randbytes(rng.randrange(0, min(40, 4080 - len(body)) + 1)), rng))
            fa.append(w)
            vers.append(v)
    if cap:
        monkeypatch.setenv("CE_TEST_GRID_CAP", str(cap))
    monkeypatch.setenv("CE_GSET_CAP", str(1 << 18))  # room for the batch: no refold from HBM
    core, model = new_core(ctx, key), gm.Core()
    ingest_and_check(core, model, key, files, actors, fa, vers)
    assert fused(core) == len(files) and (core.path_count("open_grid_capped") > 0) == bool(cap)
    core.close()


# ------------------------------------------------------------------ multi-page files
@pytest.fixture(scope="module")
def big_bodies():
    rng = random.Random(13)
    five_k = gm.enc_ops([member_of(rng, "cf") for _ in range(570)])
    seventy_k = gm.enc_ops([member_of(rng, "fixint") for _ in range(70000)])
    one_mib = gm.enc_ops([member_of(rng, "cf") for _ in range((1 << 20) // 9)])
    assert 5000 < len(five_k) < 6000 and seventy_k[:1] == b"\xdd" and len(seventy_k) == 70005
    assert (1 << 20) - 16 < len(one_mib) <= (1 << 20) + 16
    return [five_k, seventy_k, one_mib]


@pytest.mark.parametrize("mixed", [False, True])
def test_multi_page_files(ctx, oracle, big_bodies, mixed):
    rng = random.Random(14)
    key, a = rng.randbytes(32), rng.randbytes(16)
    bodies = list(big_bodies)
    if mixed:
        small = [gm.enc_ops([member_of(rng, "cf") for _ in range(rng.randrange(50))]) for _ in range(9)]
        bodies = small[:3] + bodies[:1] + small[3:6] + bodies[1:] + small[6:]
    files, fa, vers = one_writer(oracle, rng, key, bodies)
    core, model = new_core(ctx, key), gm.Core()
    ingest_and_check(core, model, key, files, [a], fa, vers)
    assert paths(core) == (len(bodies), 0) and fused(core) == len(bodies) - 3  # the three multi-page files: k_decode_gset
    core.close()


def test_multi_page_general_path_and_truncation(ctx, oracle):
    """A two-page file of alternating widths, and one whose last element is cut by the file's end."""
    rng = random.Random(15)
    key, a = rng.randbytes(32), rng.randbytes(16)
    ws = list(WIDTH_BITS)
    mixed = gm.enc_ops([member_of(rng, ws[i % 5]) for i in range(1500)])
    assert len(mixed) > 4096
    files, fa, vers = one_writer(oracle, rng, key, [mixed])
    core, model = new_core(ctx, key), gm.Core()
    ingest_and_check(core, model, key, files, [a], fa, vers)
    assert paths(core) == (0, 1)
    before = core.state_bytes()
    cut = gm.enc_ops([member_of(rng, "cf") for _ in range(600)])[:-2]
    files, fa, vers = one_writer(oracle, rng, key, [gm.enc_ops([3]), cut])
    ingest_and_check(core, model, key, files, [a], fa, [1, 2], want_rc=12)
    assert core.state_bytes() == before
    core.close()


@pytest.mark.parametrize("tamper", [False, True])
def test_multi_key_retry(ctx, oracle, big_bodies, tamper):
    """CE_OPEN_MULTI_KEY: files under the older key, a 5 KiB one among them, open on the retry and
    go through the same decode; a tampered file fails under every key and rejects the batch."""
    from oracle import keys as K
    rng = random.Random(16)
    writer = rng.randbytes(16)
    ks = K.Keys()
    k_old, k_new = rng.randbytes(32), rng.randbytes(32)
    ks.insert_latest_key(writer, rng.randbytes(16), k_old)
    ks.insert_latest_key(writer, rng.randbytes(16), k_new)
    keys = crdtenc.Keys.decode(ks.to_bytes())
    assert keys.latest()[2] == k_new
    bodies = [gm.enc_ops([member_of(rng, rng.choice(list(WIDTH_BITS))) for _ in range(rng.randrange(1, 80))]) for _ in range(11)]
    bodies.insert(4, big_bodies[0])
    old = [i % 3 == 1 for i in range(12)]
    files = [seal(oracle, k_old if o else k_new, APP + b, rng) for b, o in zip(bodies, old)]
    if tamper:
        b = bytearray(files[4])
        b[-2] ^= 1
        files[4] = bytes(b)
    core = crdtenc.Core(ctx, kind=GS, supported=[APP], current_data_version=APP, flags=crdtenc.OPEN_MULTI_KEY)
    core.set_keys(keys)
    empty = core.state_bytes()
    rc, st = core.ingest_ops(files, [writer], [0] * 12, list(range(12)))
    if tamper:
        assert rc == 9 and [i for i, s in enumerate(st) if s] == [4] and core.state_bytes() == empty
    else:
        model = gm.Core()
        same_key = [seal(oracle, k_new, APP + b, rng) for b in bodies]
        assert model.read_remote_ops(k_new, [APP], same_key, [writer] * 12, list(range(12)))[0] == 0
        assert rc == 0 and st == [0] * 12 and core.state_bytes() == model.serialize()
    core.close()


# ------------------------------------------------------------------ states
def _pack(x):
    return msgpack.packb(x, use_bin_type=True)


@pytest.mark.parametrize("route", ["ingest_states", "ingest_states_device", "merge_state", "merge_state_device"])
@pytest.mark.parametrize("order", ["states_then_ops", "ops_then_states"])
def test_states(ctx, oracle, route, order):
    """Two overlapping state files (one with an unsorted `value` holding duplicates, one with the
    struct given as an array), before and after ops."""
    torch = pytest.importorskip("torch")
    rng = random.Random(17)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(3))
    shared = [member_of(rng, rng.choice(list(WIDTH_BITS))) for _ in range(40)]
    m1 = shared + [member_of(rng, "cf") for _ in range(30)] + shared[:7] + [0, U64]
    m2 = sorted(shared[10:] + [member_of(rng, "ce") for _ in range(25)])
    rng.shuffle(m1)
    sws = [_pack({"next_op_versions": {"dots": {actors[0]: 2}}, "state": {"value": m1}}),
           _pack({"next_op_versions": {"dots": {actors[1]: 1, actors[0]: 1}}, "state": [m2]})]
    sfiles = [seal(oracle, key, APP + sw, rng) for sw in sws]
    core, model = new_core(ctx, key), gm.Core()

    def states():
        if route == "ingest_states":
            rc, st = core.ingest_states(sfiles)
            assert rc == 0 and st == [0, 0]
        elif route == "ingest_states_device":
            blob = b"".join(sfiles)
            offs = np.zeros(3, dtype=np.int64)
            offs[1:] = np.cumsum([len(f) for f in sfiles])
            d_blob = torch.tensor(list(blob) + [0] * 64, dtype=torch.uint8, device="cuda")
            d_offs = torch.tensor(offs, device="cuda")
            torch.cuda.synchronize()
            rc, st = core.ingest_states_device(d_blob.data_ptr(), d_offs.data_ptr(), 2, len(blob), want_status=True)
            assert rc == 0 and st == [0, 0]
        elif route == "merge_state":
            for sw in sws:
                assert core.merge_state(sw) == 0
        else:
            for sw in sws:
                d = torch.tensor(list(sw), dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                assert core.merge_state_device(d.data_ptr(), len(sw)) == 0
        assert model.read_remote_states(key, [APP], sfiles)[0] == 0
        assert core.state_bytes() == model.serialize()

    def ops():
        bodies = [gm.enc_ops(rng.sample(shared, 10) + [member_of(rng, "cf") for _ in range(10)]) for _ in range(9)]
        files = [seal(oracle, key, APP + b, rng) for b in bodies]
        fa = [w for w in range(3) for _ in range(3)]
        vers = [model.nov.get(actors[w]) + v for w in range(3) for v in range(3)]
        ingest_and_check(core, model, key, files, actors, fa, vers)
    for step in ((states, ops) if order == "states_then_ops" else (ops, states)):
        step()
    # not the `value` form; a rejected state file leaves everything as it was
    before = core.state_bytes()
    assert core.merge_state(_pack({"next_op_versions": {"dots": {}}, "state": {"inner": {"dots": {}}}})) == 12
    bad = [sfiles[0], seal(oracle, key, APP + _pack({"next_op_versions": {"dots": {}}, "state": {"value": [1, -1]}}), rng)]
    rc, st = core.ingest_states(bad)
    assert (rc, st) == model.read_remote_states(key, [APP], bad) == (12, [0, 12])
    assert core.state_bytes() == before
    core.close()


# ------------------------------------------------------------------ serializer
def _members_straddling(rng, n):
    edges = [0, 0x7f, 0x80, 0xff, 0x100, 0xffff, 0x10000, (1 << 32) - 1, 1 << 32, U64]
    ms = set(edges[:n])
    while len(ms) < n:
        ms.add(member_of(rng, rng.choice(list(WIDTH_BITS))))
    return ms


@pytest.mark.parametrize("n", [0, 1, 15, 16, 65535, 65536])
@pytest.mark.parametrize("flags", [0, crdtenc.COMPACT_INGEST_FORMAT])
def test_serializer(ctx, oracle, n, flags, monkeypatch):
    """Member counts across the array headers, widths across every boundary: the writer, the
    CE_HOST_COMPACT=1 writer and the model give the same bytes; the sealed file opens to them and
    is named by its SHA3-256; an ingest-format compaction read by a fresh core gives the state."""
    rng = random.Random(n + flags)
    key = rng.randbytes(32)
    nov = VClock()
    for _ in range(3):
        nov.apply(rng.randbytes(16), rng.randrange(1, 1 << 20))
    want = gm.serialize(nov, gm.GSet(_members_straddling(rng, n)))
    nonce = bytes(range(24))

    def compacted(core):
        assert core.merge_state(want) == 0
        assert core.state_bytes() == want
        f, name = core.compact_to_buffer(nonce=nonce)
        assert name == crdtenc.content_name(f) == oracle.base32_nopad(hashlib.sha3_256(f).digest())
        return f
    core = new_core(ctx, key, flags=flags)
    f = compacted(core)
    s, pt = oracle.cryptor_decrypt(key, f[16:])
    assert s == 0
    if flags:
        assert f[:16] == CORE and pt == APP + want
    else:
        assert f[:16] == APP and pt == want
    monkeypatch.setenv("CE_HOST_COMPACT", "1")
    host = new_core(ctx, key, flags=flags)
    monkeypatch.delenv("CE_HOST_COMPACT")
    assert compacted(host) == f
    # the device writer wrote the first core's state bytes and compaction, the host writer the second's
    assert core.path_count("gset_device_writes") == 2 and host.path_count("gset_device_writes") == 0
    if flags:
        fresh = new_core(ctx, key)
        rc, sts = fresh.ingest_states([f])
        assert rc == 0 and sts == [0] and fresh.state_bytes() == want
        fresh.close()
    core.close()
    host.close()


# ------------------------------------------------------------------ compact_ops_device
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


@pytest.mark.parametrize("case", ["clean", "tampered", "gap"])
def test_compact_ops_device(ctx, oracle, case):
    """ce_core_compact_ops_device == ingest_ops_device + compact_to_buffer with the same nonce."""
    rng = random.Random(18)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(4))
    files, fa, vers = [], [], []
    for a in range(4):
        for v in range(5):
            files.append(seal(oracle, key, APP + gm.enc_ops([member_of(rng, "cf") for _ in range(20)]), rng))
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
    model = gm.Core()
    orc, _ = model.read_remote_ops(key, [APP], files, [actors[i] for i in fa], vers)
    core = new_core(ctx, key)
    before = core.state_bytes()
    rc, f, name = core.compact_ops_device(*args, nonce=nonce)
    assert rc == orc, (rc, orc, ctx.last_error())
    if case == "tampered":
        assert rc == 9 and f is None and core.state_bytes() == before
    elif case == "gap":
        assert rc == 13 and f is None and core.state_bytes() == model.serialize()
    else:
        assert rc == 0 and core.state_bytes() == model.serialize()
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
        c3.close()
        ref.close()
    core.close()


# ------------------------------------------------------------------ storage
def test_storage_two_replicas(ctx, tmp_path, oracle):
    """apply_ops, apply_ops_batch, read_remote, compact, read_remote again: both replicas end
    with the model's bytes."""
    rng = random.Random(19)
    key = rng.randbytes(32)
    remote = str(tmp_path / "remote")
    c1 = new_core(ctx, key, local_path=str(tmp_path / "l1"), remote_path=remote, flags=crdtenc.OPEN_CREATE)
    c2 = new_core(ctx, key, local_path=str(tmp_path / "l2"), remote_path=remote,
                  flags=crdtenc.OPEN_CREATE | crdtenc.COMPACT_INGEST_FORMAT)
    a1, a2 = c1.info_actor(), c2.info_actor()
    model = gm.Core()

    def local(actor, ops):
        model.apply_ops(actor, ops)
        return gm.enc_ops(ops)
    assert c1.apply_ops(b"\x92\x01\xc0") == 12
    for i in range(4):
        assert c1.apply_ops(local(a1, [10 * i + 1, member_of(rng, "cf"), 0])) == 0
    rc, written = c2.apply_ops_batch([local(a2, [1000 + i, U64 - i, 11]) for i in range(3)])
    assert rc == 0 and len(written) == 3
    assert c2.apply_ops_batch([gm.enc_ops([5]), b"\x91\xc0"])[0] == 12  # nothing sealed or applied
    assert c1.read_remote() == 0 and c2.read_remote() == 0
    assert c1.state_bytes() == c2.state_bytes() == model.serialize()
    rc, name = c2.compact()
    assert rc == 0 and crdtenc.Storage(str(tmp_path / "l2"), remote).list_state_names() == [name]
    assert c1.apply_ops(local(a1, [999])) == 0
    assert c1.read_remote() == 0 and c2.read_remote() == 0
    assert c1.state_bytes() == c2.state_bytes() == model.serialize()
    c3 = new_core(ctx, key, local_path=str(tmp_path / "l3"), remote_path=remote, flags=crdtenc.OPEN_CREATE)
    assert c3.read_remote() == 0 and c3.state_bytes() == model.serialize()
    for c in (c1, c2, c3):
        c.close()


def test_reset_and_settle(ctx, oracle):
    rng = random.Random(21)
    key, a = rng.randbytes(32), rng.randbytes(16)
    core, model = new_core(ctx, key), gm.Core()
    empty = core.state_bytes()
    files, fa, vers = one_writer(oracle, rng, key, [gm.enc_ops([0, 5, U64])])
    ingest_and_check(core, model, key, files, [a], fa, vers)
    core.settle()
    core.reset()
    assert core.state_bytes() == empty
    ingest_and_check(core, gm.Core(), key, files, [a], fa, vers)
    core.close()


# ------------------------------------------------------------------ multi-GPU answers
def test_multi_gpu_answers_are_definite(ctx, oracle):
    """No dense exchange for this kind: dense_ready 0 and CE_ERR_INVALID_ARG from the five dense /
    sharded entry points and the column calls, with nothing touched; two cores converge through
    state_bytes_device / merge_state_device."""
    torch = pytest.importorskip("torch")
    import ctypes
    rng = random.Random(20)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(4))
    cores, models = [new_core(ctx, key) for _ in range(2)], [gm.Core() for _ in range(2)]
    for r in range(2):
        cores[r].register_actors(actors)
        bodies = [gm.enc_ops([member_of(rng, rng.choice(list(WIDTH_BITS))) for _ in range(30)]) for _ in range(6)]
        files = [seal(oracle, key, APP + b, rng) for b in bodies]
        ingest_and_check(cores[r], models[r], key, files, actors[2 * r:2 * r + 2], [0, 0, 0, 1, 1, 1], [0, 1, 2] * 2)
    c, L = cores[0], crdtenc.lib()
    before = c.state_bytes()
    cap = c.dense_capacity()
    buf = torch.full((2 * cap,), 7, dtype=torch.int64, device="cuda")
    nov = torch.full((cap,), 7, dtype=torch.int64, device="cuda")
    ready = ctypes.c_int(5)
    vp = ctypes.c_void_p
    assert c.dense_ready() is False and L.ce_core_dense_ready(c.p) == 0
    assert L.ce_core_export_dense(c.p, vp(buf.data_ptr()), vp(nov.data_ptr())) == 64
    assert L.ce_core_import_dense(c.p, vp(buf.data_ptr()), vp(nov.data_ptr())) == 64
    (d_blob, d_offs, d_fa, d_fv), blen = _to_device([b"x" * 40], [0], [0])
    assert c.ingest_ops_device_sharded(d_blob.data_ptr(), d_offs.data_ptr(), 1, blen, b"".join(actors),
                                       d_fa.data_ptr(), d_fv.data_ptr(), nov.data_ptr()) == 64
    assert L.ce_core_pending_export(c.p, vp(buf.data_ptr()), ctypes.c_uint64(2 * cap), ctypes.byref(ready)) == 64
    assert L.ce_core_pending_commit(c.p, 1, None, ctypes.c_uint64(0)) == 64
    rc, n = c.export_columns_device(buf.data_ptr(), 16 * cap)
    assert rc == 64 and n == 0
    torch.cuda.synchronize()
    assert ready.value == 5 and bool((buf == 7).all()) and bool((nov == 7).all())
    assert c.state_bytes() == before
    dev = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    for src, dst in ((0, 1), (1, 0)):
        rc, n = cores[src].state_bytes_device(dev.data_ptr(), dev.numel())
        assert rc == 0 and bytes(dev[:n].cpu().numpy()) == models[src].serialize()
        assert cores[dst].merge_state_device(dev.data_ptr(), n) == 0
        models[dst].merge_state(models[src].serialize())
    assert cores[0].state_bytes() == cores[1].state_bytes() == models[0].serialize() == models[1].serialize()
    for x in cores:
        x.close()
