"""The two ce_buf layouts of the with_state reads (include/crdtenc.h: ce_core_read_clock and
ce_core_orswot_member_clocks) as crdtenc.py decodes them, on hand-packed buffers, and the 128-bit
p - n words of ce_core_counter_read.  No GPU and no library: the decoders are plain Python."""
import struct

import pytest

import crdtenc

U64 = (1 << 64) - 1


def entry(actor, counter):
    return actor + struct.pack("<Q", counter)


def pack_member_clocks(per):
    """the layout by hand: u32 beg[n + 1], zero padding to 8 bytes, 24-byte entries"""
    beg = [0]
    for e in per:
        beg.append(beg[-1] + len(e))
    head = struct.pack("<%dI" % len(beg), *beg)
    head += bytes(-len(head) % 8)
    return head + b"".join(entry(a, c) for e in per for a, c in e)


def test_clock_entries_round_trip():
    a, b = bytes(range(16)), bytes(range(16, 32))
    assert crdtenc.decode_clock(b"") == []
    assert crdtenc.decode_clock(entry(a, 1) + entry(b, U64)) == [(a, 1), (b, U64)]
    with pytest.raises(ValueError):
        crdtenc.decode_clock(entry(a, 1)[:-1])


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4])
def test_member_clocks_padding_even_and_odd(n):
    """n + 1 offsets: a multiple of 8 bytes for odd n, 4 bytes of padding for even n"""
    acts = [bytes([i]) * 16 for i in range(5)]
    per = [[(acts[j], 100 * i + j + 1) for j in range(i % 3)] for i in range(n)]   # 0, 1, 2, 0 entries
    buf = pack_member_clocks(per)
    head = ((n + 1) * 4 + 7) & ~7
    assert head == (n + 1) * 4 + (4 if n % 2 == 0 else 0)
    assert len(buf) == head + 24 * sum(len(e) for e in per)
    assert crdtenc.decode_member_clocks(buf, n) == per


def test_member_clocks_empty_buffer_and_ranges():
    assert crdtenc.decode_member_clocks(struct.pack("<II", 0, 0), 0) == []           # n = 0: one offset, padded
    a = bytes(16)
    per = [[], [(a, 7)], [], []]                                                       # empty ranges around one
    assert crdtenc.decode_member_clocks(pack_member_clocks(per), 4) == per
    with pytest.raises(ValueError):
        crdtenc.decode_member_clocks(pack_member_clocks(per)[:-1], 4)                 # entries cut short
    with pytest.raises(ValueError):
        crdtenc.decode_member_clocks(b"\0\0\0\0", 1)                                  # offsets cut short


def test_counter_words_on_sums_of_u64_max():
    """p - n over sums of 2^64 - 1 counters: the magnitude's high word, the sign, the tie"""
    for kp, kn in [(1, 0), (3, 0), (3, 1), (1, 3), (2, 2), (0, 0), (0, 1), (1 << 20, 1)]:
        p, n = kp * U64, kn * U64
        lo, hi, neg = crdtenc.pn_words(p, n)
        assert 0 <= lo <= U64 and 0 <= hi <= U64
        assert (hi << 64 | lo) == abs(p - n) and neg == (1 if p < n else 0)
        assert crdtenc.counter_int(lo, hi, neg) == p - n
    assert crdtenc.pn_words(3 * U64, 0) == (U64 - 2, 2, 0)
    assert crdtenc.pn_words(U64, U64) == (0, 0, 0)
    assert crdtenc.counter_int(U64 - 2, 2, 1) == -3 * U64
    with pytest.raises(ValueError):
        crdtenc.pn_words(1 << 128, 0)
