"""tests/gset_model.py (the checker of the GPU GSet fold) against the fixture packed by Python
msgpack alone, the union laws the fold relies on, and every accepted and rejected wire form.
CPU only."""
import hashlib
import itertools
import json
import os
import random

import msgpack
import pytest

import gset_model as gm
from oracle.crdts import DecodeError, VClock

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gset.json")
H = bytes.fromhex
U64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def fx():
    with open(GOLDEN) as f:
        return json.load(f)


def _pack(x):
    return msgpack.packb(x, use_bin_type=True)


def test_fixture_ops_decode_and_reencode(fx):
    for case in fx["ops"]:
        assert gm.dec_ops(H(case["hex"])) == case["members"], case["name"]
        assert gm.enc_ops(case["members"]) == H(case["hex"]), case["name"]  # the model's writer is canonical


def test_fixture_header_boundaries(fx):
    by = {c["name"]: H(c["hex"]) for c in fx["ops"]}
    assert by["empty"] == b"\x90"
    assert by["fifteen"][0] == 0x9f and by["sixteen"][:3] == b"\xdc\x00\x10"
    for big in fx["ops_big"]:
        n = big["count"]
        body = gm.enc_ops([i & 0x7f for i in range(n)])
        assert body[:5].hex() == big["head"] and len(body) == big["len"]
        assert hashlib.sha256(body).hexdigest() == big["sha256"]
        assert gm.dec_ops(body) == [i & 0x7f for i in range(n)]
    assert H(fx["ops_big"][0]["head"])[:3] == b"\xdc\xff\xff"
    assert H(fx["ops_big"][1]["head"]) == b"\xdd\x00\x01\x00\x00"


def test_element_lengths(fx):
    for k, want in fx["element_lengths"].items():
        assert len(gm.enc_ops([int(k, 16)])) - 1 == want, k


def test_fixture_states_decode_and_reencode(fx):
    for s in fx["states"]:
        nov, st = gm.dec_state(H(s["hex"]))
        assert nov.dots == {H(a): c for a, c in s["next_op_versions"].items()}, s["name"]
        assert st.read() == s["members"], s["name"]
        assert gm.serialize(nov, st) == H(s["hex"]), s["name"]
    edges = H([s for s in fx["states"] if s["name"] == "edges"][0]["hex"])
    assert edges.startswith(b"\x82\xb0next_op_versions\x81\xa4dots\x82")
    assert b"\xa5state\x81\xa5value\x9d\x00\x01\x7f\xcc\x80\xcc\xff\xcd\x01\x00" in edges
    assert edges.endswith(b"\xcf" + b"\xff" * 8)


# ------------------------------------------------------------------ union laws
def _rand_set(rng):
    return gm.GSet(rng.choice([rng.randrange(8), rng.randrange(1 << 64)]) for _ in range(rng.randrange(12)))


def test_merge_is_commutative_associative_idempotent():
    rng = random.Random(1)
    for _ in range(50):
        a, b, c = _rand_set(rng), _rand_set(rng), _rand_set(rng)
        ab, ba = gm.GSet(a.value), gm.GSet(b.value)
        ab.merge(b)
        ba.merge(a)
        assert ab == ba
        l, r = gm.GSet(ab.value), gm.GSet(b.value)
        l.merge(c)
        r.merge(c)
        r.merge(a)
        assert l == r
        again = gm.GSet(ab.value)
        again.merge(ab)
        again.merge(a)
        assert again == ab


def test_op_order_is_irrelevant():
    ops = [5, (1 << 64) - 1, 0, 5, 1 << 33, 0x80]
    want = None
    for perm in itertools.permutations(ops):
        s = gm.GSet()
        for o in perm:
            s.apply(o)
        b = gm.serialize(VClock(), s)
        want = want or b
        assert b == want
    assert want.endswith(b"\xa5value\x95\x00\x05\xcc\x80\xcf\x00\x00\x00\x02\x00\x00\x00\x00" + b"\xcf" + b"\xff" * 8)


# ------------------------------------------------------------------ accepted forms
ACCEPTED = {
    "non_minimal_cc": (b"\x91\xcc\x05", [5]),
    "non_minimal_cd": (b"\x91\xcd\x00\x05", [5]),
    "non_minimal_ce": (b"\x91\xce\x00\x00\x00\x05", [5]),
    "non_minimal_cf": (b"\x91\xcf" + bytes(7) + b"\x05", [5]),
    "d0_non_negative": (b"\x91\xd0\x7f", [0x7f]),
    "d1_non_negative": (b"\x91\xd1\x7f\xff", [0x7fff]),
    "d2_non_negative": (b"\x91\xd2\x7f\xff\xff\xff", [0x7fffffff]),
    "d3_non_negative": (b"\x91\xd3\x7f" + b"\xff" * 7, [(1 << 63) - 1]),
    "array16_small_count": (b"\xdc\x00\x02\x01\x02", [1, 2]),
    "array32_small_count": (b"\xdd\x00\x00\x00\x02\x01\x02", [1, 2]),
    "array32_empty": (b"\xdd\x00\x00\x00\x00", []),
    "trailing_bytes": (b"\x92\x01\xcc\xff\xc1\xc1\xff", [1, 0xff]),
    "trailing_after_empty": (b"\x90\x05", []),
}


@pytest.mark.parametrize("name", list(ACCEPTED))
def test_ops_accepted_forms(name):
    body, want = ACCEPTED[name]
    assert gm.dec_ops(body) == want


# ------------------------------------------------------------------ rejected forms
REJECTED = {
    "negative_fixint": b"\x91\xff",
    "negative_d0": b"\x91\xd0\x80",
    "negative_d1": b"\x91\xd1\x80\x00",
    "negative_d2": b"\x91\xd2\x80\x00\x00\x00",
    "negative_d3": b"\x91\xd3\x80" + bytes(7),
    "float32": b"\x91\xca\x3f\x80\x00\x00",
    "float64": b"\x91\xcb" + bytes(8),
    "nil": b"\x91\xc0",
    "bool": b"\x91\xc3",
    "str": b"\x91\xa1a",
    "bin": b"\x91\xc4\x01a",
    "nested_array": b"\x91\x91\x01",
    "map": b"\x91\x81\x01\x02",
    "truncated_element": b"\x92\x01\xcf\x00\x00\x00",
    "count_past_the_bytes": b"\x93\x01\x02",
    "count16_past_the_bytes": b"\xdc\x00\x03\x01\x02",
    "count32_past_the_bytes": b"\xdd\xff\xff\xff\xff\x01",
    "truncated_header16": b"\xdc\x00",
    "truncated_header32": b"\xdd\x00\x00\x00",
    "top_level_map": b"\x80",
    "top_level_int": b"\x05",
    "top_level_nil": b"\xc0",
    "empty_body": b"",
}


@pytest.mark.parametrize("name", list(REJECTED))
def test_ops_rejected_forms(name):
    with pytest.raises(DecodeError):
        gm.dec_ops(REJECTED[name])


def test_state_accepted_forms():
    a = bytes(range(16))
    nov = {"dots": {a: 4}}
    want = [1, 2, 300, U64]
    forms = [
        _pack({"next_op_versions": nov, "state": {"value": [300, 2, 1, U64]}}),            # unsorted
        _pack({"next_op_versions": nov, "state": {"value": [2, 300, 2, 1, U64, 1, 300]}}),  # duplicates
        _pack({"next_op_versions": nov, "state": [[1, 2, 300, U64]]}),                      # one-element array
        _pack({"next_op_versions": nov, "state": {0: [1, 2, 300, U64]}}),                   # keyed by index
        _pack({"state": {"zzz": None, "value": [1, 2, 300, U64]}, "next_op_versions": nov}),
        _pack([nov, [[1, 2, 300, U64]]]),
        _pack({"next_op_versions": nov, "state": {"value": [1, 2, 300, U64]}}) + b"\xc1tail",
    ]
    for f in forms:
        got_nov, st = gm.dec_state(f)
        assert st.read() == want and got_nov.dots == {a: 4}


@pytest.mark.parametrize("state", [{"value": [1, -1]}, {"value": [1.5]}, {"value": {1: 2}}, {"value": 5}, {"valu": [1]},
                                   [[1], [2]], [], {"value": [[1]]}, {"value": [None]}, {"value": [1], 0: [2]}])
def test_state_rejected_forms(state):
    with pytest.raises(DecodeError):
        gm.dec_state(_pack({"next_op_versions": {"dots": {}}, "state": state}))


# ------------------------------------------------------------------ the Core restatement
def _files(oracle, rng, key, app, bodies):
    out = []
    for b in bodies:
        st, enc = oracle.cryptor_encrypt(key, rng.randbytes(24), app + b)
        assert st == 0
        out.append(bytes.fromhex("e834d789101b463498239de990a9051f") + enc)
    return out


def test_core_gate_and_all_or_nothing(oracle):
    rng = random.Random(3)
    key, app, a, b = rng.randbytes(32), rng.randbytes(16), rng.randbytes(16), rng.randbytes(16)
    c = gm.Core()
    fs = _files(oracle, rng, key, app, [gm.enc_ops([1, 2]), gm.enc_ops([2, 3]), gm.enc_ops([9])])
    assert c.read_remote_ops(key, [app], fs, [a, a, b], [0, 1, 0]) == (0, [0, 0, 0])
    assert c.state.read() == [1, 2, 3, 9] and c.nov.dots == {a: 2, b: 1}
    before = c.serialize()
    # a decode error anywhere rejects the whole batch, whatever the gate would say
    fs = _files(oracle, rng, key, app, [gm.enc_ops([50]), b"\x91\xc0"])
    assert c.read_remote_ops(key, [app], fs, [a, a], [2, 3]) == (12, [0, 12])
    assert c.serialize() == before
    # a replayed version inserts nothing; a gap keeps the files before it
    fs = _files(oracle, rng, key, app, [gm.enc_ops([60]), gm.enc_ops([61]), gm.enc_ops([62]), gm.enc_ops([63])])
    assert c.read_remote_ops(key, [app], fs, [a, a, a, a], [1, 2, 4, 5]) == (13, [0, 0, 13, 0])
    assert c.state.read() == [1, 2, 3, 9, 61] and c.nov.dots == {a: 3, b: 1}
    # states: overlapping sets and version vectors merge
    sw = [_pack({"next_op_versions": {"dots": {a: 7}}, "state": {"value": [3, 1000]}}),
          _pack({"next_op_versions": {"dots": {b: 1}}, "state": {"value": [1000, 0]}})]
    fs = _files(oracle, rng, key, app, sw)
    assert c.read_remote_states(key, [app], fs) == (0, [0, 0])
    assert c.state.read() == [0, 1, 2, 3, 9, 61, 1000] and c.nov.dots == {a: 7, b: 1}
