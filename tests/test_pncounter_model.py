"""tests/pncounter_model.py (the checker of the GPU PNCounter fold) against the fixture packed by
Python msgpack alone, and the CRDT laws the fold relies on.  CPU only."""
import itertools
import json
import os
import random

import msgpack
import pytest

import pncounter_model as pm
from oracle.crdts import DecodeError, VClock

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pncounter.json")
H = bytes.fromhex


@pytest.fixture(scope="module")
def fx():
    with open(GOLDEN) as f:
        return json.load(f)


def test_fixture_ops_decode_and_reencode(fx):
    for case in fx["ops"]:
        want = [((H(a), c), d) for a, c, d in case["ops"]]
        assert pm.dec_ops(H(case["hex"])) == want, case["name"]
        assert pm.enc_ops(want) == H(case["hex"]), case["name"]  # the model's writer is canonical


def test_fixture_state_decodes_and_reencodes(fx):
    s = fx["state"]
    nov, st = pm.dec_state(H(s["hex"]))
    assert nov.dots == {H(a): c for a, c in s["next_op_versions"].items()}
    assert st.p.dots == {H(a): c for a, c in s["p"].items()}
    assert st.n.dots == {H(a): c for a, c in s["n"].items()}
    assert pm.serialize(nov, st) == H(s["hex"])
    # the head of the layout, byte for byte: 82 b0"next_op_versions" .. a5"state" 82 a1"p" 81 a5"inner"
    assert H(s["hex"]).startswith(b"\x82\xb0next_op_versions\x81\xa4dots\x82")
    assert b"\xa5state\x82\xa1p\x81\xa5inner\x81\xa4dots\x82" in H(s["hex"])
    assert b"\xa1n\x81\xa5inner\x81\xa4dots\x82" in H(s["hex"])


def test_five_canonical_op_lengths(fx):
    a = bytes(range(16))
    lens = []
    for c in (0x7f, 0xff, 0xffff, 0xffffffff, (1 << 64) - 1):
        for d in pm.DIRS:
            one = pm.enc_ops([((a, c), d)])
            assert one[0] == 0x91 and one[1:6] == b"\x82\xa3dot"
            assert one[-8:] == b"\xa3dir\xa3" + d.encode()
            lens.append(len(one) - 1)
    assert lens[0::2] == lens[1::2] == fx["op_lengths"] == [47, 48, 49, 51, 55]


def test_zero_counter_never_inserts():
    c = pm.PNCounter()
    c.apply(((bytes(16), 0), "Neg"))
    assert c.n.dots == {} and pm.serialize(VClock(), c).endswith(b"\xa1n\x81\xa5inner\x81\xa4dots\x80")


@pytest.mark.parametrize("form", ["dir_first", "array_op", "array_dot", "extra_key", "index_keys", "map_dir",
                                  "map_dir_index"])
def test_noncanonical_forms_decode(form):
    a = bytes(range(16))
    dot = {"actor": a, "counter": 9}
    obj = {"dir_first": {"dir": "Neg", "dot": dot},
           "array_op": [dot, "Neg"],
           "array_dot": {"dot": [a, 9], "dir": "Neg"},
           "extra_key": {"dot": dot, "zzz": [1, {"x": 2}], "dir": "Neg"},
           "index_keys": {1: "Neg", 0: {1: 9, 0: a}},
           "map_dir": {"dot": dot, "dir": {"Neg": None}},
           "map_dir_index": {"dot": dot, "dir": {1: None}}}[form]
    assert pm.dec_ops(msgpack.packb([obj], use_bin_type=True)) == [((a, 9), "Neg")]


@pytest.mark.parametrize("form", ["dir_zero", "dir_bin", "dup_dot", "truncated", "count_too_large", "dir_value",
                                  "missing_dir"])
def test_bad_forms_are_decode_errors(form):
    a = bytes(range(16))
    dot = {"actor": a, "counter": 9}
    good = msgpack.packb({"dot": dot, "dir": "Pos"}, use_bin_type=True)
    b = {"dir_zero": msgpack.packb([{"dot": dot, "dir": "Zero"}], use_bin_type=True),
         "dir_bin": msgpack.packb([{"dot": dot, "dir": b"Pos"}], use_bin_type=True),
         "dup_dot": b"\x91\x83" + b"\xa3dot" + msgpack.packb(dot, use_bin_type=True) + b"\xa3dot" +
                    msgpack.packb(dot, use_bin_type=True) + b"\xa3dir\xa3Pos",
         "truncated": b"\x92" + good + good[:-3],
         "count_too_large": b"\x93" + good + good,
         "dir_value": msgpack.packb([{"dot": dot, "dir": {"Pos": 1}}], use_bin_type=True),
         "missing_dir": msgpack.packb([{"dot": dot}], use_bin_type=True)}[form]
    with pytest.raises(DecodeError):
        pm.dec_ops(b)


def _random_counter(rng, actors):
    c = pm.PNCounter()
    for _ in range(rng.randrange(0, 12)):
        c.apply(((rng.choice(actors), rng.getrandbits(rng.choice([3, 9, 20, 40]))), rng.choice(pm.DIRS)))
    return c


def _clone(c):
    o = pm.PNCounter()
    o.merge(c)
    return o


def test_merge_commutes_and_is_idempotent():
    rng = random.Random(5)
    actors = [rng.randbytes(16) for _ in range(4)]
    for _ in range(50):
        x, y = _random_counter(rng, actors), _random_counter(rng, actors)
        xy, yx = _clone(x), _clone(y)
        xy.merge(y)
        yx.merge(x)
        assert xy == yx
        again = _clone(xy)
        again.merge(xy)
        again.merge(y)
        assert again == xy


def test_any_file_order_of_distinct_writers_gives_the_same_state():
    """read_remote_ops over one file per writer: every order of the files folds to the same
    bytes (the fold is a max-join per plane, so the shards of a batch may land in any order)."""
    rng = random.Random(6)
    actors = sorted(rng.randbytes(16) for _ in range(4))
    key = rng.randbytes(32)
    import oracle
    app = bytes(range(16))
    files = []
    for w in actors:
        ops = [((w if rng.random() < 0.7 else rng.choice(actors), rng.getrandbits(rng.choice([5, 12, 33]))),
                rng.choice(pm.DIRS)) for _ in range(9)]
        st, enc = oracle.cryptor_encrypt(key, rng.randbytes(24), app + pm.enc_ops(ops))
        assert st == 0
        files.append(oracle.crdts.CORE_VERSION + enc)
    want = None
    for order in itertools.permutations(range(4)):
        c = pm.Core()
        rc, st = c.read_remote_ops(key, [app], [files[i] for i in order], [actors[i] for i in order], [0] * 4)
        assert rc == 0 and st == [0] * 4
        want = want or c.serialize()
        assert c.serialize() == want
    assert pm.dec_state(want)[1] == c.state
