"""tests/orswot_write_model.py against oracle/crdts.py's encoder and decoder, the op-length formula
and the one-page rule it relies on."""
import itertools
import random

import pytest

from oracle import crdts as C

import orswot_write_model as wm

ACTOR = bytes(range(0x40, 0x50))
# a counter / member of every encoded width
OF_WIDTH = {1: 0x7f, 2: 0xff, 3: 0xffff, 5: 0xffffffff, 9: wm.U64}


def test_vectors_decode_back_to_the_same_ops():
    """every vector's bytes decode through dec_ops to the ops it was cut into; the ops, in order,
    carry the whole column and counters c0 + 1, c0 + 2, ..."""
    rng = random.Random(1)
    col = [wm.member_of_width(rng, wm.WIDTH_BYTES[i % 5]) for i in range(200)] + list(wm.WIDTH_EDGES)
    for per_op, opf, c0 in ((0, 0, 0), (1, 1, 126), (1, 15, 250), (1, 16, 65530), (1, 58, (1 << 32) - 9),
                            (15, 1, 5), (16, 1, 5), (17, 3, 1 << 40), (446, 1, 0), (5, 7, 3), (3, 0, 0)):
        po, k = wm.shape(per_op, opf)
        vectors = wm.cut(col, per_op, opf, c0, ACTOR)
        ops = [op for v in vectors for op in v]
        assert [m for op in ops for m in op[2]] == col
        assert [op[1] for op in ops] == [(ACTOR, c0 + 1 + j) for j in range(len(ops))]
        assert all(len(op[2]) == po for op in ops[:-1]) and 0 < len(ops[-1][2]) <= po
        assert all(len(v) == k for v in vectors[:-1]) and 0 < len(vectors[-1]) <= k
        for v in vectors:
            clear = wm.clear_text(v)
            assert clear[:16] == wm.APP and C.dec_ops("orswot", clear[16:]) == v
            assert len(clear) == 16 + wm.hdr(len(v)) + sum(wm.op_len(op[1][1], op[2]) for op in v)
            assert len(clear) <= wm.PAGE
    assert wm.cut([], 3, 2, 9, ACTOR) == []


def test_op_length_closed_form():
    """51 + w(counter) + h(count) + sum w(member) over every combination of counter width, member
    width and a count on either side of the members' header change; the issue's table"""
    for wc, wmem, cnt in itertools.product(wm.WIDTH_BYTES, wm.WIDTH_BYTES, (1, 2, 15, 16, 17, 446)):
        op = ("Add", (ACTOR, OF_WIDTH[wc]), [OF_WIDTH[wmem]] * cnt)
        got = len(C.enc_orswot_ops([op])) - 1
        assert got == wm.op_len(op[1][1], op[2]) == 51 + wc + (1 if cnt <= 15 else 3) + wmem * cnt, (wc, wmem, cnt)
    table = {(1, 1, 1): 54, (9, 9, 1): 70, (1, 1, 15): 68, (1, 1, 16): 71, (9, 9, 446): 4077}
    for (wc, wmem, cnt), want in table.items():
        assert wm.op_len(OF_WIDTH[wc], [OF_WIDTH[wmem]] * cnt) == want
    # mixed widths inside one op
    rng = random.Random(2)
    for _ in range(50):
        mem = [wm.member_of_width(rng, rng.choice(wm.WIDTH_BYTES)) for _ in range(rng.randint(1, 40))]
        ctr = wm.member_of_width(rng, rng.choice(wm.WIDTH_BYTES)) or 1
        assert len(C.enc_orswot_ops([("Add", (ACTOR, ctr), mem)])) - 1 == wm.op_len(ctr, mem)


@pytest.mark.parametrize("per_op,opf", [(1, 1), (1, 15), (1, 16), (1, 28), (1, 58), (0, 0), (15, 1), (16, 1), (446, 1),
                                        (5, 7), (16, 0), (3, 0)])
def test_bound_is_met_at_nine_byte_inputs_and_never_passed(per_op, opf):
    po, k = wm.shape(per_op, opf)
    rng = random.Random(per_op * 100 + opf)
    c9 = 1 << 40
    for n in sorted({0, 1, po - 1, po, po + 1, po * k - 1, po * k, po * k + 1, 2 * po * k + 1, 3 * po * k + po + 1} - {-1}):
        top = wm.cut([wm.U64] * n, per_op, opf, c9, ACTOR)
        want = (sum(len(v) for v in top), len(top), sum(16 + wm.sealed_len(len(wm.clear_text(v))) for v in top))
        assert wm.bound(n, per_op, opf) == want, n
        col = [wm.member_of_width(rng, rng.choice(wm.WIDTH_BYTES)) for _ in range(n)]
        for c0 in (0, 120, c9):
            vs = wm.cut(col, per_op, opf, c0, ACTOR)
            got = (sum(len(v) for v in vs), len(vs), sum(16 + wm.sealed_len(len(wm.clear_text(v))) for v in vs))
            assert got[:2] == want[:2] and got[2] <= want[2]


def test_page_rule_corners():
    """28 / 29 ops inside and past the fused region, 58 / 59 inside and past the page at one member
    an op; 446 / 447 members in one op"""
    top = 1 << 63

    def worst(ops, per_op):
        return len(wm.clear_text([("Add", (ACTOR, top), [wm.U64] * per_op)] * ops))
    assert worst(28, 1) == wm.file_bound(28, 1) == 1979 <= wm.FUSE_REGION < wm.file_bound(29, 1) == worst(29, 1)
    assert worst(58, 1) == wm.file_bound(58, 1) == 4079 <= wm.PAGE < wm.file_bound(59, 1) == worst(59, 1)
    assert worst(1, 446) == wm.file_bound(1, 446) == 4094 <= wm.PAGE < wm.file_bound(1, 447) == worst(1, 447)
    assert wm.shape(0, 0) == wm.shape(1, 0) == (1, 28)
    assert wm.shape(1, 58) == (1, 58) and wm.shape(1, 59) is None
    assert wm.shape(446, 1) == (446, 1) and wm.shape(447, 1) is None and wm.shape(447, 0) is None
    assert wm.shape(446, 0) == (446, 1) and wm.shape(446, 2) is None
    # the default at per_op > 1 is the most ops the page holds
    for po in (2, 5, 15, 16, 17, 100, 223, 224):
        _, k = wm.shape(po, 0)
        assert wm.file_bound(k, po) <= wm.PAGE < wm.file_bound(k + 1, po)
    assert wm.bound(10, 1, 59) is None and wm.bound(0, 5, 7) == (0, 0, 0)
