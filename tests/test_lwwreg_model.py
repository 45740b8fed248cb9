"""tests/lwwreg_model.py (the checker of the GPU LWWReg fold) against the fixture packed by Python
msgpack alone, the tie rules the fold has to reproduce, and every accepted and rejected wire form.
CPU only."""
import json
import os
import random

import msgpack
import pytest

import lwwreg_model as lm
from oracle.crdts import DecodeError, VClock

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lwwreg.json")
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
        ops = [tuple(o) for o in case["ops"]]
        assert lm.dec_ops(H(case["hex"])) == ops, case["name"]
        if case["name"] not in ("array_form", "reversed_keys"):
            assert lm.enc_ops(ops) == H(case["hex"]), case["name"]  # the model's writer is canonical


def test_fixture_header_and_element_layout(fx):
    by = {c["name"]: H(c["hex"]) for c in fx["ops"]}
    assert by["empty"] == b"\x90"
    assert by["fifteen"][0] == 0x9f and by["sixteen"][:3] == b"\xdc\x00\x10"
    assert by["one_val_0"] == b"\x91\x82\xa3val\x00\xa6marker\x01"
    assert by["array_form"][:6] == b"\x92\x92\x07\xcd\x12\x34"
    assert by["reversed_keys"][1:9] == b"\x82\xa6marker"
    for k, want in fx["element_lengths"].items():
        assert len(lm.enc_ops([(int(k, 16), 1)])) - 1 == want, k
        assert len(lm.enc_ops([(1, int(k, 16))])) - 1 == want, k
    # the page bounds the issue names: 135 elements of 30 bytes, 291 of 14
    assert len(lm.enc_ops([(U64, U64)] * 135)) + 16 <= 4096 < len(lm.enc_ops([(U64, U64)] * 136)) + 16
    assert len(lm.enc_ops([(1, 1)] * 291)) + 16 <= 4096 < len(lm.enc_ops([(1, 1)] * 292)) + 16


def test_fixture_states_decode_and_reencode(fx):
    for s in fx["states"]:
        nov, st = lm.dec_state(H(s["hex"]))
        assert nov.dots == {H(a): c for a, c in s["next_op_versions"].items()}, s["name"]
        assert st.read() == (s["val"], s["marker"]), s["name"]
        assert lm.serialize(nov, st) == H(s["hex"]), s["name"]
    d = H([s for s in fx["states"] if s["name"] == "default"][0]["hex"])
    assert d == b"\x82\xb0next_op_versions\x81\xa4dots\x80\xa5state\x82\xa3val\x00\xa6marker\x00"


def test_round_trips_random():
    rng = random.Random(3)
    for _ in range(50):
        ops = [(rng.getrandbits(rng.choice([3, 8, 16, 32, 64])), rng.getrandbits(rng.choice([3, 8, 16, 32, 64])))
               for _ in range(rng.randrange(40))]
        assert lm.dec_ops(lm.enc_ops(ops)) == ops
        assert lm.enc_ops(ops) == _pack([{"val": v, "marker": m} for v, m in ops])
        nov = VClock({rng.randbytes(16): rng.randrange(1, 1 << 20) for _ in range(rng.randrange(4))})
        st = lm.LWWReg(*ops[0]) if ops else lm.LWWReg()
        n2, s2 = lm.dec_state(lm.serialize(nov, st))
        assert n2 == nov and s2 == st


# ------------------------------------------------------------------ the tie rules
def test_strictly_greater_wins_ties_keep_the_incumbent():
    r = lm.LWWReg()
    r.apply((9, 0))
    assert r.read() == (0, 0)            # marker 0 never replaces the default
    r.apply((5, 7))
    r.apply((6, 7))
    assert r.read() == (5, 7)            # an equal marker changes nothing
    r.apply((1, 6))
    assert r.read() == (5, 7)
    r.apply((1, 8))
    assert r.read() == (1, 8)
    r.merge(lm.LWWReg(2, 8))
    assert r.read() == (1, 8)
    r.merge(lm.LWWReg(U64, U64))
    assert r.read() == (U64, U64)


def test_fold_is_argmax_by_marker_then_first_applied():
    rng = random.Random(5)
    for _ in range(200):
        ops = [(rng.randrange(1 << 20), rng.randrange(4)) for _ in range(rng.randrange(1, 30))]
        r = lm.LWWReg()
        for op in ops:
            r.apply(op)
        top = max(m for _, m in ops)
        want = (0, 0) if top == 0 else next(op for op in ops if op[1] == top)
        assert r.read() == want


def _plain_core_ops(core, bodies, actors, versions):
    """read_remote_ops over clear bodies (no cryptor): the gate and the apply order alone"""
    for i, b in enumerate(bodies):
        a, v = actors[i], versions[i]
        e = core.nov.get(a)
        if v < e:
            continue
        if e < v:
            return 13
        for op in lm.dec_ops(b):
            core.state.apply(op)
        core.nov.apply(a, e + 1)
    return 0


def test_batch_order_decides_ties_and_the_gate_hides_files():
    a, b = b"A" * 16, b"B" * 16
    c = lm.Core()
    assert _plain_core_ops(c, [lm.enc_ops([(1, 9)]), lm.enc_ops([(2, 9)])], [a, b], [0, 0]) == 0
    assert c.state.read() == (1, 9)      # the lower file index wins
    c = lm.Core()
    assert _plain_core_ops(c, [lm.enc_ops([(2, 9)]), lm.enc_ops([(1, 9)])], [b, a], [0, 0]) == 0
    assert c.state.read() == (2, 9)
    c = lm.Core()
    c.nov.apply(a, 1)                    # version 0 of a has been read: its file is ignored
    assert _plain_core_ops(c, [lm.enc_ops([(1, 99)]), lm.enc_ops([(2, 9)])], [a, a], [0, 1]) == 0
    assert c.state.read() == (2, 9)
    c = lm.Core()                        # a gap: the files before it are folded, nothing after
    assert _plain_core_ops(c, [lm.enc_ops([(1, 5)]), lm.enc_ops([(2, 99)])], [a, a], [0, 2]) == 13
    assert c.state.read() == (1, 5) and c.nov.get(a) == 1


def test_states_merge_in_call_order():
    a = b"A" * 16
    c = lm.Core()
    c.merge_state(lm.serialize(VClock({a: 2}), lm.LWWReg(1, 9)))
    c.merge_state(lm.serialize(VClock({a: 5}), lm.LWWReg(2, 9)))
    assert c.state.read() == (1, 9) and c.nov.get(a) == 5


# ------------------------------------------------------------------ wire forms
OK_FORMS = [
    (b"\x91\x92\x07\x09", [(7, 9)]),                                       # the struct as an array
    (_pack([{"marker": 9, "val": 7}]), [(7, 9)]),                          # the keys the other way round
    (_pack([{"val": 7, "x": [1, {"y": b"z"}], "marker": 9}]), [(7, 9)]),   # an unknown key, skipped
    (_pack([{0: 7, 1: 9}]), [(7, 9)]),                                     # fields by index
    (b"\x91\x82\xa3val\xd0\x07\xa6marker\xd3" + (9).to_bytes(8, "big"), [(7, 9)]),   # signed forms, >= 0
    (b"\x91\x82\xa3val\xcf" + (7).to_bytes(8, "big") + b"\xa6marker\xcd\x00\x09", [(7, 9)]),  # non-minimal
    (lm.enc_ops([(7, 9)]) + b"\xc1\xff", [(7, 9)]),                        # trailing bytes
]
BAD_FORMS = [
    b"\x91\x82\xa3val\x07\xa6marker\xd3" + (U64).to_bytes(8, "big"),       # a negative d3
    b"\x91\x82\xa3val\xff\xa6marker\x09",                                  # a negative fixint
    b"\x91\x83\xa3val\x07\xa3val\x08\xa6marker\x09",                       # a repeated key
    b"\x91\x81\xa3val\x07",                                                # a missing key
    b"\x92\x82\xa3val\x07\xa6marker\x09",                                  # a count larger than the elements
    lm.enc_ops([(7, 1 << 40)])[:-3],                                       # an element cut by the end
    b"\x91\x82\xa3val\x07\xa6marker\xc0",                                  # nil for a u64
    b"\x91\x93\x07\x09\x01",                                               # an array of 3
    b"\x81\xa3val\x07",                                                    # not a sequence
    b"",
]


def test_accepted_forms():
    for b, want in OK_FORMS:
        assert lm.dec_ops(b) == want, b.hex()
    # a wrong key byte makes the key unknown: the field is then missing
    with pytest.raises(DecodeError):
        lm.dec_ops(b"\x91\x82\xa3vam\x07\xa6marker\x09")


def test_rejected_forms():
    for b in BAD_FORMS:
        with pytest.raises(DecodeError):
            lm.dec_ops(b)
    for b in (b"\x82\xb0next_op_versions\x81\xa4dots\x80\xa5state\x81\xa3val\x00",        # no marker
              b"\x81\xb0next_op_versions\x81\xa4dots\x80"):                              # no state
        with pytest.raises(DecodeError):
            lm.dec_state(b)
