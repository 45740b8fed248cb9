"""The Rm-op writer's CPU model (tests/orswot_rm_model.py) against oracle/crdts.py: the lengths it
states are the lengths enc_orswot_ops writes, dec_ops returns the ops, and applying a call's
vectors removes the queried members and defers nothing."""
import random

import pytest

import orswot_rm_model as rm
from oracle import crdts as C

COUNTERS = (1, 200, 60000, 1 << 31, 1 << 40)     # one of every counter width
MEMBERS = (0, 5, 200, 60000, 1 << 31, 1 << 40, rm.U64)


def clock_of(rng, k):
    return C.VClock({rng.randbytes(16): COUNTERS[i % 5] for i in range(k)})


@pytest.mark.parametrize("k", [0, 1, 15, 16, 17])
def test_op_len_is_the_encoders(k):
    rng = random.Random(k)
    for m in MEMBERS:
        clock = clock_of(rng, k)
        op = ("Rm", clock, [m])
        assert rm.op_len(clock, m) == len(C.enc_orswot_ops([op])) - 1
    for c in COUNTERS:          # every counter width on its own
        clock = C.VClock({rng.randbytes(16): c for _ in range(max(k, 1))})
        assert rm.op_len(clock, 7) == len(C.enc_orswot_ops([("Rm", clock, [7])])) - 1


@pytest.mark.parametrize("n_ops", [1, 15, 16, 17])
def test_file_len_is_the_encoders(n_ops):
    rng = random.Random(100 + n_ops)
    vec = [("Rm", clock_of(rng, i % 4), [MEMBERS[i % len(MEMBERS)]]) for i in range(n_ops)]
    assert rm.file_len(vec) == len(rm.clear_text(vec)) == 16 + len(C.enc_orswot_ops(vec))
    got = C.dec_ops("orswot", C.enc_orswot_ops(vec))
    assert [(o[0], o[1].dots, list(o[2])) for o in got] == [(o[0], o[1].dots, o[2]) for o in vec]


def build_state(rng):
    st = C.Orswot()
    actors = [rng.randbytes(16) for _ in range(17)]
    for i, a in enumerate(actors):
        st.apply(("Add", (a, COUNTERS[i % 5]), [1000] + ([1001] if i < 16 else []) + ([1002] if i < 15 else [])))
    st.apply(("Add", (actors[0], (1 << 40) + 1), [1, 2, 0, rm.U64]))
    st.apply(("Rm", C.VClock(st.entries[2].dots), [2]))                       # added then removed
    st.apply(("Rm", C.VClock({rng.randbytes(16): 9}), [1000, 77]))            # stays deferred
    return st


@pytest.mark.parametrize("flags", [0, rm.LIVE_ONLY])
@pytest.mark.parametrize("opf", [0, 1, 3])
def test_a_calls_vectors_remove_their_members_and_defer_nothing(flags, opf):
    rng = random.Random(7)
    st = build_state(rng)
    deferred = dict(st.deferred)
    clock = dict(st.clock.dots)
    col = [1000, 5, 2, 1001, 1000, 0, rm.U64, 1002, 1, 5, 1001]
    vectors = rm.cut(col, opf, st, flags)
    want_ops = len(col) if not flags else 6          # 1000, 1001, 0, U64, 1002, 1: live, first occurrences
    assert rm.sizes(vectors)[0] == want_ops
    assert all(len(v) == (opf or 16) for v in vectors[:-1]) and 0 < len(vectors[-1]) <= (opf or 16)
    flat = [op for v in vectors for op in v]
    assert [len(op[1].dots) for op in flat if op[2] == [1000]][0] == 17
    if not flags:
        assert flat[4][1].dots == flat[0][1].dots and flat[1][1].dots == {} and flat[2][1].dots == {}
    for v in vectors:
        for op in C.dec_ops("orswot", C.enc_orswot_ops(v)):
            st.apply(op)
    assert st.deferred == deferred and st.clock.dots == clock
    assert all(m not in st.entries for m in col)
