"""tests/gset_write_model.py against the msgpack package and the page bound it relies on."""
import random

import msgpack

import gset_model as gm
import gset_write_model as wm


def test_chunks_are_what_msgpack_writes():
    """every chunk's body is msgpack's own encoding of the list (smallest unsigned forms, fixarray
    or array16), at every width, mixed widths, the width edges and around the header change"""
    rng = random.Random(1)
    cols = [[wm.member_of_width(rng, w) for _ in range(40)] for w in wm.WIDTH_BYTES]
    cols.append([wm.member_of_width(rng, wm.WIDTH_BYTES[i % 5]) for i in range(1000)])
    cols.append(list(wm.WIDTH_EDGES) * 3)
    for col in cols:
        for pf in (1, 15, 16, 17, 453, 0):
            chunks = wm.cut(col, pf)
            assert [m for ch in chunks for m in ch] == col
            assert all(len(ch) == wm.per_file_of(pf) for ch in chunks[:-1])
            assert 0 < len(chunks[-1]) <= wm.per_file_of(pf)
            for ch in chunks:
                body = gm.enc_ops(ch)
                assert body == msgpack.packb(ch)
                assert wm.clear_text(ch) == wm.APP + body
                assert len(body) == (1 if len(ch) <= 15 else 3) + sum(wm.width(m) for m in ch)
    assert wm.cut([], 7) == []


def test_every_chunk_fits_one_page():
    """<= 453 members at any width: <= 4096 bytes of clear text; 454 cf members pass it"""
    top = (1 << 64) - 1
    assert len(wm.clear_text([top] * wm.FILE_MEMBERS)) == wm.PAGE
    assert len(wm.clear_text([top] * (wm.FILE_MEMBERS + 1))) > wm.PAGE
    rng = random.Random(2)
    for cnt in (0, 1, 15, 16, 452, 453):
        for w in wm.WIDTH_BYTES:
            assert len(wm.clear_text([wm.member_of_width(rng, w) for _ in range(cnt)])) <= wm.PAGE
        assert len(wm.clear_text([wm.member_of_width(rng, rng.choice(wm.WIDTH_BYTES)) for _ in range(cnt)])) <= wm.PAGE


def test_filter_is_sorted_set_difference():
    assert wm.new_only([5, 3, 5, 0, (1 << 64) - 1, 3], {3, 9}) == [0, 5, (1 << 64) - 1]
    assert wm.new_only([0, (1 << 64) - 1], {0, (1 << 64) - 1}) == []
    assert wm.new_only([], {1}) == []
