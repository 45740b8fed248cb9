"""The device state reader's run rule, restated sequentially and checked against gset_model: a body
is taken when its elements are unsigned markers whose widths never decrease, each run ending at the
first element (at the run's stride) whose marker is not the run's, or that would pass the file's
end, or at the array's count.  Whatever the rule proves must be what the msgpack reader decodes; and
the shapes the GPU tests expect on the device or on the host fall where they say.

CPU only: this checks the rule and the test expectations, not the kernels (tests/test_gpu_gset_states.py)."""
import random

import pytest

import gset_model as gm

WIDTH = [1, 2, 3, 5, 9]


def runs(body, count):
    """the five phases: (run lengths, end offset); body = the bytes after the array header"""
    s = o = 0
    out = []
    for p, w in enumerate(WIDTH):
        t = 0
        while s + t < count:
            pos = o + w * t
            if pos + w > len(body):
                break
            m = body[pos]
            if not (m <= 0x7f if p == 0 else m == 0xcb + p):
                break
            t += 1
        out.append(t)
        s += t
        o += w * t
    return out, o


def proven(body, count):
    r, _ = runs(body, count)
    return sum(r) == count


def members(body, count):
    r, _ = runs(body, count)
    o, out = 0, []
    for L, w in zip(r, WIDTH):
        for _ in range(L):
            out.append(body[o] if w == 1 else int.from_bytes(body[o + 1:o + w], "big"))
            o += w
    return out


def el(p, v):
    return bytes([v]) if p == 0 else bytes([0xcb + p]) + v.to_bytes(WIDTH[p] - 1, "big")


def hdr(n):
    return gm.enc_ops([0] * n)[:-n] if n else b"\x90"


def test_rule_agrees_with_the_reader_on_random_bodies():
    rng = random.Random(1)
    marker_bytes = [0xcc, 0xcd, 0xce, 0xcf, 0x00, 0x7f, 0xd3, 0xff, 0xc0]
    taken = 0
    for _ in range(3000):
        n = rng.randrange(0, 12)
        ps = [rng.randrange(5) for _ in range(n)]
        if rng.random() < 0.7:
            ps.sort()
        els = []
        for p in ps:
            payload = bytes(rng.choice(marker_bytes) for _ in range(WIDTH[p] - 1))
            els.append(bytes([rng.randrange(128)]) if p == 0 else bytes([0xcb + p]) + payload)
        body = b"".join(els)
        cut = rng.choice([0, 0, 0, 1, 2])
        count = n + rng.choice([0, 0, 0, 1, -1]) if n else 0
        count = max(count, 0)
        body = body[:len(body) - cut] + bytes(rng.choice(marker_bytes) for _ in range(rng.choice([0, 0, 3])))
        if proven(body, count):
            taken += 1
            assert gm.dec_ops(hdr(count) + body) == members(body, count)
    assert taken > 1000


@pytest.mark.parametrize("name,body,count,device", [
    ("all_five", el(0, 1) + el(1, 200) + el(2, 300) + el(3, 70000) + el(4, 1 << 40), 5, True),
    ("non_minimal", el(0, 9) + el(1, 5) + el(2, 6) + el(3, 0) + el(4, 5), 5, True),
    ("ce_of_cd_bytes", el(3, 0xcdcdcdcd) + el(3, 0xcccccccc), 2, True),
    ("cd_run_then_cf_of_marker_bytes", b"".join(el(2, 0xcd00 + i) for i in range(200)) + el(4, int.from_bytes(b"\xcd" * 8, "big")),
     201, True),
    ("descending", el(4, 1 << 40) + el(0, 1), 2, False),
    ("d3", el(3, 70000) + b"\xd3" + bytes(8), 2, False),
    ("negative", b"\x05\xff", 2, False),
    ("count_above", el(4, 1 << 40) * 3, 4, False),
    ("count_below", el(4, 1 << 40) * 3, 2, True),
    ("cut", (el(4, 1 << 40) * 3)[:-1], 3, False),
])
def test_shapes_fall_where_the_gpu_tests_say(name, body, count, device):
    assert proven(body, count) == device
    if device:
        assert gm.dec_ops(hdr(count) + body) == members(body, count)
