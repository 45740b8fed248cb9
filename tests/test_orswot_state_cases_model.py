"""CPU checks of the Orswot state corpus (tests/orswot_state_cases.py), no GPU.

1. Every case has the facts it claims, computed from its bytes: head offsets against chunk and
   row edges, run positions against 2048 and 256, prefix residues, tail lengths, the candidate
   heads before, inside and after the entries.
2. oracle.crdts.Core("orswot").read_remote_states accepts every file (sealed with the built
   oracle's cryptor).
3. `write_state` restates the device writer (ce_dotset_io.hip k_ser_head_* / k_ser_len_* /
   k_ser_write / k_ser_tail) statement by statement -- sorted pairs, heads, hrank, seg, per-pair
   lengths, per-tile sums and carries, per-256-block [lo, hi) with a 16-byte body and byte ends --
   and reproduces the oracle's bytes on families A-D, at every alignment of the output.
4. `read_state` restates the reader's stages (prefix parse and its longer-prefix loop, the chunked
   head search with the p + 7 <= hi bound, the skip before lo, entry parse, chain check, repeats,
   tail window, emit lookup) and gives the oracle's entries and the stated route on E and F.
5. Sensitivity, of these PYTHON restatements only (never of a kernel): each wrong variant differs
   from the oracle on a named case of its family, so a kernel wrong in that way fails that case.
"""
import random

import pytest

import orswot_state_cases as K
from oracle import crdts as C

CASES = K.all_cases()
APP = bytes.fromhex("aadfd5a66e194b24a8024fa27c72f20c")
M32 = 0xffffffff


def decoded(sw):
    nov, st = C.dec_state("orswot", sw)
    return nov, st


# ------------------------------------------------------------------------------------------ 1. facts
def test_names_and_sizes():
    assert {c.family for c in CASES.values()} == set("ABCDEFGH")
    for c in CASES.values():
        big = c.name in ("B_entries_65535", "B_entries_65536")
        assert sum(map(len, c.files)) < (2.2e6 if big else 1.1e6), c.name
        for f in c.files:
            nov, st = decoded(f)
            if c.canonical:
                assert C.serialize("orswot", nov, st) == f, c.name


def test_family_a_facts():
    _, st = decoded(CASES["A_cross"].files[0])
    assert sorted(st.entries) == K.EDGES
    for m in K.EDGES:
        assert sorted(st.entries[m].dots.values()) == K.EDGES[1:]
    nov, _ = decoded(CASES["A_cross"].files[0])
    assert set(K.EDGES[1:]) <= set(nov.dots.values()) and set(K.EDGES[1:]) <= set(st.clock.dots.values())
    assert sorted(m for f in CASES["A_each_alone"].files for m in decoded(f)[1].entries) == K.EDGES
    sw = CASES["A_wide256"].files[0]
    L = K.layout(sw)
    assert L["n"] == 256 and L["end"] - L["lo"] == 256 * 43 and 43 <= K.SER_MAX_DOT and K.runs_of(sw) == [1] * 256


def test_family_b_facts():
    for n in (1, 15, 16, 17, 65535, 65536):
        sw = CASES["B_entries_%d" % n].files[0]
        L = K.layout(sw)
        assert L["n"] == n and L["lo"] - L["prefix"] == (1 if n < 16 else 3 if n < 65536 else 5)
    assert K.runs_of(CASES["B_dots_per_entry"].files[0]) == [1, 15, 16, 17, 16, 15, 1]
    for name, dfr in (("B_no_entries", 0), ("B_no_entries_deferred", 2)):
        _, st = decoded(CASES[name].files[0])
        assert not st.entries and st.clock.dots and len(st.deferred) == dfr


def test_family_c_facts():
    for c in K.family("C"):
        runs = K.runs_of(c.files[0])
        starts = K.run_starts(runs)
        assert sum(runs) == c.facts["pairs"]
        assert runs[-1] == 1, c.name  # the last pair is a head
        for s, k in c.facts.get("specials", []):
            assert runs[starts.index(s)] == k, (c.name, s, k)
    sp = dict(CASES["C_all_in_middle_tiles"].facts["specials"])
    assert 2044 + sp[2044] == K.TILE and sp[2048] and 4095 < 2 * K.TILE < 4095 + sp[4095]
    assert (2298 // K.BLOCK) != ((2298 + 16) // K.BLOCK) and 6143 % K.TILE == K.TILE - 1
    s, k = CASES["C_run_straddles_tile"].facts["specials"][0]
    assert s == K.TILE - 1 and s + k > K.TILE
    s, k = CASES["C_run17_straddles_block"].facts["specials"][0]
    assert k == 17 and s // K.BLOCK == 0 and (s + k - 1) // K.BLOCK == 1


def test_family_d_facts():
    cs = K.family("D")
    assert sorted(K.layout(c.files[0])["prefix"] % 16 for c in cs) == list(range(16))
    for c in cs:
        assert K.layout(c.files[0])["prefix"] % 16 == c.facts["residue"] and sum(K.runs_of(c.files[0])) == 3001
    assert len({c.files[0][K.layout(c.files[0])["prefix"]:] for c in cs}) == 1  # the same entries under every head


def test_family_e_facts():
    for name, edge in (("E_head_across_chunk_edge", K.CHUNK), ("E_head_across_row_edge", 5 * K.ROW)):
        c = CASES[name]
        assert c.facts["targets"] == list(range(edge - 7, edge + 1)) and edge % K.ROW == 0
        for sw, t in zip(c.files, c.facts["targets"]):
            L = K.layout(sw)
            hp = K.head_positions(sw)
            assert t in hp and L["lo"] < t < L["end"] and K.head_counts(sw) == (2, L["n"], 0)
    sw = CASES["E_head_ends_at_hi"].files[0]
    assert K.head_positions(sw)[-1] == len(sw) - 7 == CASES["E_head_ends_at_hi"].facts["head_at"]
    sw = CASES["E_six_head_bytes_at_hi"].files[0]
    assert sw.endswith(K.HEAD) and len(sw) - 6 not in K.head_positions(sw)
    for n in (300, 1200):
        sw = CASES["E_spurious_in_clock_%d" % n].files[0]
        L = K.layout(sw)
        assert K.head_counts(sw) == (n + 3, L["n"], 0) and n + 3 > 256
    assert K.layout(CASES["E_spurious_in_clock_1200"].files[0])["lo"] > K.HEAD_HINT
    assert K.layout(CASES["E_spurious_in_clock_1200"].facts["primer"])["lo"] < K.HEAD_HINT // 2
    for name in ("E_spurious_in_entry_uuid", "E_spurious_in_counter", "E_spurious_in_member"):
        sw = CASES[name].files[0]
        L = K.layout(sw)
        assert K.head_counts(sw)[1] > L["n"], name
    sw = CASES["E_heads_only_in_deferred"].files[0]
    L = K.layout(sw)
    assert K.head_counts(sw) == (2, L["n"], 40)


def test_family_f_facts():
    for n in (K.TAIL_WIN - 1, K.TAIL_WIN, K.TAIL_WIN + 1):
        L = K.layout(CASES["F_tail_%d" % n].files[0])
        assert L["hi"] - L["end"] == n
    sw = CASES["F_actor_not_in_clock"].files[0]
    _, st = decoded(sw)
    assert any(a not in st.clock.dots for v in st.entries.values() for a in v.dots)
    for name in ("F_repeated_member_small", "F_repeated_member_all_ones"):
        sw = CASES[name].files[0]
        assert K.layout(sw)["n"] == len(decoded(sw)[1].entries) + 1
    assert K.U64 in decoded(CASES["F_repeated_member_all_ones"].files[0])[1].entries
    assert b"\xcd\x00\x05" + K.HEAD in CASES["F_long_member"].files[0]
    assert b"\xcd\x00" in CASES["F_long_counter"].files[0]
    for form, b in (("de", b"\xde\x00\x02"), ("df", b"\xdf\x00\x00\x00\x02")):
        assert K.HEAD + b in CASES["F_entry_header_%s" % form].files[0]


def test_family_g_facts():
    for n in (1, 2, 16, 17, 64, 65):
        c = CASES["G_files_%d" % n]
        sizes = [K.layout(f)["n"] for f in c.files]
        assert len(c.files) == n and sizes == K.g_sizes(n) and sum(map(len, c.files)) < 1.1e6
        if n > 17:
            assert sizes[16] == 1 and sizes[17] == 2049 and sizes[19] == 4097
        assert all(f.endswith(b"\xa8deferred\x80") for f in c.files)
    c = CASES["G_file16_declines"]
    assert c.routes == ["device"] * 16 + ["host"] and K.layout(c.files[16])["n"] == 3 and len(decoded(c.files[16])[1].entries) == 2
    c = CASES["G_middle_has_deferred"]
    assert [len(decoded(f)[1].deferred) for f in c.files] == [0, 2, 0]


def test_family_h_facts():
    for c in K.family("H"):
        sw, stripped = c.files[0], c.facts["stripped"]
        assert sw != stripped
        nov, st = decoded(stripped)
        zeros = [c_ for v in [nov, st.clock] + list(st.entries.values()) + [C.VClock(dict(k)) for k in st.deferred]
                 for c_ in v.dots.values() if c_ == 0]
        assert not zeros
        ref, strip = C.Core("orswot"), C.Core("orswot")
        ref.state.merge(decoded(sw)[1])
        ref.nov.merge(decoded(sw)[0])
        strip.state.merge(st)
        strip.nov.merge(nov)
        assert (ref.serialize() == strip.serialize()) == c.facts["same_as_reference"], c.name


# ------------------------------------------------------------------------------------------ 2. the oracle accepts
def test_oracle_accepts_every_file(oracle):
    rng = random.Random(5)
    key = rng.randbytes(32)
    for c in CASES.values():
        files = []
        for sw in c.files:
            st, enc = oracle.cryptor_encrypt(key, rng.randbytes(24), APP + sw)
            assert st == 0
            files.append(C.CORE_VERSION + enc)
        rc, st = C.Core("orswot").read_remote_states(key, [APP], files)
        assert rc == 0 and st == [0] * len(files), c.name


# ------------------------------------------------------------------------------------------ 3. the writer
RUNGS = {"rung_80": (0x80, 0xff, 0xffff, M32), "rung_100": (0x7f, 0x100, 0xffff, M32),
         "rung_10000": (0x7f, 0xff, 0x10000, M32), "rung_2_32": (0x7f, 0xff, 0xffff, 1 << 32)}


def put_uint(v, bug=None):
    r = RUNGS.get(bug, (0x7f, 0xff, 0xffff, M32))
    if v <= r[0]:
        return bytes([v & 0xff])
    k, mk = (1, 0xcc) if v <= r[1] else (2, 0xcd) if v <= r[2] else (4, 0xce) if v <= r[3] else (8, 0xcf)
    return bytes([mk]) + bytes((v >> (8 * (k - 1 - b))) & 0xff for b in range(k))


def put_map(k, bug=None):
    k &= M32
    fix, m16 = (16, 0xffff) if bug == "map_16" else (15, 0x10000) if bug == "map_65536" else (15, 0xffff)
    if k <= fix:
        return bytes([(0x80 | k) & 0xff])
    if k <= m16:
        return bytes([0xde, (k >> 8) & 0xff, k & 0xff])
    return bytes([0xdf]) + k.to_bytes(4, "big")


def tile_scan(vals, bug=None):
    """exclusive scan in 2048-item tiles: a tile's base is the sum of the tile totals before it"""
    ts = [sum(vals[t:t + K.TILE]) for t in range(0, len(vals), K.TILE)]
    out = []
    for t in range(len(ts)):
        run = sum(ts[:t])
        if bug == "carry" and t >= 2:
            run = ts[t - 1]
        for v in vals[t * K.TILE:(t + 1) * K.TILE]:
            out.append(run)
            run += v
    return out


def write_state(sw, out_align=0, bug=None):
    """the device writer over the state that `sw` decodes to -> the bytes it leaves in a buffer
    pre-filled with a5, cut at the length k_ser_tail reports"""
    nov, st = decoded(sw)
    hw = C.Wr()
    hw.map(2)
    hw.str("next_op_versions")
    hw.vclock(nov)
    hw.str("state")
    hw.map(3)
    hw.str("clock")
    hw.vclock(st.clock)
    hw.str("entries")
    prefix = bytes(hw.b)
    suffix = sw[K.layout(sw)["end"]:]  # ("deferred" and its map: built on the host)
    pairs = sorted((m, a, c) for m, v in st.entries.items() for a, c in v.dots.items())
    member, actor, value = [p[0] for p in pairs], [p[1] for p in pairs], [p[2] for p in pairs]
    n = len(pairs)
    # k_ser_head_tiles / k_ser_head_apply
    head = []
    for i in range(n):
        prev = member[i - 1] if i > 0 else None
        if bug == "tile_first" and i % K.TILE == 0:
            prev = None  # (the previous member not loaded)
        head.append(int(i == 0 or prev is None or member[i] != prev))
    hrank = tile_scan(head, bug)
    seg = [0] * (n + 2)
    for i in range(n):
        e = hrank[i] + head[i] - 1
        if head[i]:
            seg[e] = i
        if i + 1 == n or member[i + 1] != member[i]:
            if not (bug == "seg_tile_last" and i % K.TILE == K.TILE - 1):
                seg[e + 1] = i + 1
    # k_ser_len_tiles / k_ser_len_apply
    ln = []
    for i in range(n):
        l = 18 + len(put_uint(value[i], bug))
        if head[i]:
            e = hrank[i]
            l += len(put_uint(member[i], bug)) + 6 + len(put_map(seg[e + 1] - seg[e], bug))
        ln.append(l)
    pos = tile_scan(ln, bug)
    nm = hrank[n - 1] + head[n - 1] if n else 0
    body = pos[n - 1] + ln[n - 1] if n else 0
    bound = len(prefix) + 5 + K.SER_MAX_DOT * n + len(suffix)
    out = bytearray(b"\xa5" * (bound + 64))
    # k_ser_write
    base = len(prefix) + len(put_map(nm, bug))
    for i0 in range(0, n, K.BLOCK):
        i1 = min(n, i0 + K.BLOCK)
        lo, hi = base + pos[i0], base + pos[i1 - 1] + ln[i1 - 1]
        lo16 = lo & ~15
        buf = bytearray(K.BLOCK * K.SER_MAX_DOT + 32)
        for i in range(i0, i1):
            o = base + pos[i] - lo16
            b = b""
            if head[i]:
                e = hrank[i]
                b = put_uint(member[i], bug) + K.HEAD + put_map(seg[e + 1] - seg[e], bug)
            b += b"\xc4\x10" + actor[i] + put_uint(value[i], bug)
            buf[o:o + len(b)] = b
        a0, a1 = (lo + 15) & ~15, hi & ~15
        if out_align == 0 and a0 < a1:
            for x in range(a0, a1, 16):
                out[x:x + 16] = buf[x - lo16:x - lo16 + 16]
            out[lo:a0] = buf[lo - lo16:a0 - lo16]
            if not (bug == "block_tail" and hi - a1 in (1, 15)):
                out[a1:hi] = buf[a1 - lo16:hi - lo16]
        else:
            out[lo:hi] = buf[lo - lo16:hi - lo16]
    # k_ser_tail
    out[:len(prefix)] = prefix
    s0 = len(prefix) + len(put_map(nm, bug)) + body
    out[s0:s0 + len(suffix)] = suffix
    hdr = put_map(nm, bug)
    out[len(prefix):len(prefix) + len(hdr)] = hdr
    assert s0 + len(suffix) <= bound
    return bytes(out[:s0 + len(suffix)])


@pytest.mark.parametrize("name", [c.name for f in "ABCD" for c in K.family(f)])
def test_writer_restatement(name):
    for sw in CASES[name].files:
        for k in ((0, 5) if len(sw) > 200000 else (0, 1, 15)):
            assert write_state(sw, out_align=k) == sw, (name, k)


WRITER_BUGS = [("rung_80", "A_cross"), ("rung_100", "A_cross"), ("rung_10000", "A_cross"), ("rung_2_32", "A_cross"),
               ("map_16", "B_entries_16"), ("map_16", "B_dots_per_entry"), ("map_65536", "B_entries_65536"),
               ("tile_first", "C_run_straddles_tile"), ("seg_tile_last", "C_pairs_2048"), ("seg_tile_last", "C_pairs_4096"),
               ("carry", "C_pairs_4097"), ("carry", "C_all_in_middle_tiles"), ("block_tail", "D_prefix_mod16_1"), ("block_tail", "D_prefix_mod16_15")]


@pytest.mark.parametrize("bug,name", WRITER_BUGS)
def test_writer_sensitivity(bug, name):
    sw = CASES[name].files[0]
    assert write_state(sw) == sw and write_state(sw, bug=bug) != sw


def test_writer_block_tail_variant_across_family_d():
    """a block's end moves with the prefix residue: of the 12 blocks' ends, one is a byte off a
    16-byte boundary under most of the 16 heads (which ones follows from the entries' lengths)"""
    hit = [c.facts["residue"] for c in K.family("D") if write_state(c.files[0], bug="block_tail") != c.files[0]]
    assert len(hit) >= 8 and {1, 15} <= set(hit), hit


# ------------------------------------------------------------------------------------------ 4. the reader
def rd_uint(s, p, end):
    """canonical msgpack uint at p, bounded by end -> (value, length), length 0 when it is none"""
    if p >= end:
        return 0, 0
    m = s[p]
    if m < 0x80:
        return m, 1
    k = {0xcc: 1, 0xcd: 2, 0xce: 4, 0xcf: 8}.get(m, 0)
    if not k or p + 1 + k > end:
        return 0, 0
    x = int.from_bytes(s[p + 1:p + 1 + k], "big")
    if len(put_uint(x)) != 1 + k:
        return 0, 0
    return x, 1 + k


class Short(Exception):
    pass


def parse_prefix(p, whole):
    """parse_state_prefix over the canonical layout -> (0, nov, clock, body, n) | (1,) | (2,)"""
    i = 0

    def need(k):
        if i + k > len(p):
            raise Short

    def lit(b):
        nonlocal i
        need(len(b))
        if p[i:i + len(b)] != b:
            return False
        i += len(b)
        return True

    def map_hdr():
        nonlocal i
        need(1)
        m = p[i]
        if (m & 0xf0) == 0x80:
            i += 1
            return m & 15
        k = {0xde: 2, 0xdf: 4}.get(m)
        if k is None:
            return None
        need(1 + k)
        i += 1 + k
        return int.from_bytes(p[i - k:i], "big")

    def vclock():
        nonlocal i
        if not lit(K.HEAD):
            return None
        cnt = map_hdr()
        if cnt is None:
            return None
        d = {}
        for _ in range(cnt):
            need(18)
            if p[i:i + 2] != b"\xc4\x10":
                return None
            a = p[i + 2:i + 18]
            need(19)
            k = {0xcc: 1, 0xcd: 2, 0xce: 4, 0xcf: 8}.get(p[i + 18], 0)
            need(19 + k)
            d[a] = int.from_bytes(p[i + 19:i + 19 + k], "big") if k else p[i + 18]
            i += 19 + k
        return d
    try:
        if not lit(b"\x82") or not lit(b"\xb0next_op_versions"):
            return (1,)
        nov = vclock()
        if nov is None or not lit(b"\xa5state") or not lit(b"\x83") or not lit(b"\xa5clock"):
            return (1,)
        clock = vclock()
        if clock is None or not lit(b"\xa7entries"):
            return (1,)
        n = map_hdr()
        if n is None:
            return (1,)
        return (0, nov, clock, i, n)
    except Short:
        return (1,) if whole else (2,)


def find_heads(s, hi, bug=None, after=b"\x80"):
    """stage 0 (k_rdm_count / k_rdm_write) over [0, hi): 4096-position chunks, rows of 256, one
    lane per position; `after` is what memory holds behind the file"""
    mem = s[:hi] + after + bytes(16)
    bound = {"bound6": 6, "bound8": 8}.get(bug, 7)
    cand = []
    for c0 in range(0, hi, K.CHUNK):
        for k in range(K.CHUNK // K.ROW):
            for t in range(K.ROW):
                p = c0 + k * K.ROW + t
                if p + bound > hi or mem[p:p + 6] != K.HEAD:
                    continue
                if bug == "chunk_edge" and p + 7 > c0 + K.CHUNK:
                    continue
                if bug == "row_edge" and p + 7 > c0 + (k + 1) * K.ROW:
                    continue
                m = mem[p + 6]
                if (m & 0xf0) == 0x80 or m in (0xde, 0xdf):
                    cand.append(p)
    return cand


def read_state(sw, hint=1 << 18, bug=None, table=None):
    """-> (route, {member: {actor: counter}} or None, trips of the longer-prefix loop)"""
    hi = len(sw)
    cand = find_heads(sw, hi, bug)
    want = min(hi, hint)
    pr = parse_prefix(sw[:want], want == hi)
    trips = 0
    while pr[0] == 2:
        want = min(hi, want * 4)
        pr = parse_prefix(sw[:want], want == hi)
        trips += 1
    if pr[0] != 0 or pr[4] == 0:
        return "host", None, trips
    _, nov, clock, lo, n = pr
    table = set(clock) if table is None else table | set(clock)
    # k_rdm_skip
    found, cap = len(cand), hi // 7 + 1
    m = min(found, cap)
    k = sum(1 for t in range(min(256, m)) if cand[t] < lo)
    if k == 256 and m > 256 and bug != "skip256":
        l, h = 256, m
        while l < h:
            mid = (l + h) // 2
            if cand[mid] < lo:
                l = mid + 1
            else:
                h = mid
        k = l
    if found - k < n or found > cap:
        return "host", None, trips
    heads = [cand[k + i] - lo for i in range(n)]
    # k_rdm_entry
    end, dots, flags = [], [], 0
    for i in range(n):
        p, ok, d = lo + heads[i] + 6, True, []
        if (sw[p] & 0xf0) == 0x80:
            cnt, p = sw[p] & 15, p + 1
        elif sw[p] == 0xde:
            ok, cnt, p = p + 3 <= hi, int.from_bytes(sw[p + 1:p + 3], "big"), p + 3
        else:
            ok, cnt, p = p + 5 <= hi, int.from_bytes(sw[p + 1:p + 5], "big"), p + 5
        prev = None
        for _ in range(cnt):
            if not ok or p + 18 > hi or sw[p:p + 2] != b"\xc4\x10":
                ok = False
                break
            a = sw[p + 2:p + 18]
            if prev is not None and not a > prev:
                ok = False
                break
            prev = a
            c, ul = rd_uint(sw, p + 18, hi)
            if not ul:
                ok = False
                break
            d.append((a, c))
            p += 18 + ul
        end.append(p - lo if ok else None)
        dots.append(d)
        flags |= 0 if ok else 1
    # k_rdm_chain, k_rdm_dups
    members = []
    for i in range(n):
        start = 0 if i == 0 else end[i - 1]
        mval, ul = rd_uint(sw, lo + start, lo + heads[i]) if start is not None and start <= heads[i] else (0, 0)
        if not ul or start + ul != heads[i] or end[i] is None:
            flags |= 2
        members.append(mval)
    if len(set(members)) != n:
        flags |= 8
    if flags:
        return "host", None, trips
    # k_rdm_tail and the host's choice between the window and a download
    tl = hi - (lo + end[-1])
    copied = tl < K.TAIL_WIN if bug == "tail_lt" else tl <= K.TAIL_WIN
    tail = sw[lo + end[-1]:] if (tl > K.TAIL_WIN or copied) else None
    if tail is None or not tail.startswith(b"\xa8deferred"):
        return "host", None, trips
    # k_rdm_emit
    out = {}
    for mval, d in zip(members, dots):
        for a, c in d:
            if c:
                if a not in table:
                    return "host", None, trips
                out.setdefault(mval, {})[a] = c
    return "device", out, trips


def oracle_entries(sw):
    return {m: dict(v.dots) for m, v in decoded(sw)[1].entries.items() if v.dots}


@pytest.mark.parametrize("name", [c.name for f in "EF" for c in K.family(f)])
def test_reader_restatement(name):
    c = CASES[name]
    for sw, route in zip(c.files, c.routes):
        got, ent, trips = read_state(sw, hint=K.HEAD_HINT if "primer" in c.facts else 1 << 18)
        assert got == route, (name, got)
        if route == "device":
            assert ent == oracle_entries(sw), name
        assert trips == (1 if "primer" in c.facts else 0)


def test_reader_restatement_on_the_writer_families():
    for f in "ABCD":
        for c in K.family(f):
            if sum(map(len, c.files)) > 200000:
                continue
            for sw, route in zip(c.files, c.routes):
                got, ent, _ = read_state(sw)
                assert got == route and (ent is None or ent == oracle_entries(sw)), c.name


READER_BUGS = [("chunk_edge", "E_head_across_chunk_edge", range(1, 7)), ("row_edge", "E_head_across_row_edge", range(1, 7)),
               ("bound8", "E_head_ends_at_hi", [0]), ("bound6", "E_six_head_bytes_at_hi", [0]),
               ("skip256", "E_spurious_in_clock_300", [0]), ("tail_lt", "F_tail_4096", [0])]


@pytest.mark.parametrize("bug,name,which", READER_BUGS)
def test_reader_sensitivity(bug, name, which):
    c = CASES[name]
    for i in which:
        sw = c.files[i]
        if bug.startswith("bound"):  # (the search runs whatever the route: compare its candidates)
            assert find_heads(sw, len(sw)) == K.head_positions(sw) != find_heads(sw, len(sw), bug), (name, i)
            continue
        good, bad = read_state(sw), read_state(sw, bug=bug)
        assert good[0] == c.routes[i] and good[1] == oracle_entries(sw)
        assert bad[:2] != good[:2], (name, i)


def read_many(files, bug=None):
    """launch_orswot_read_multi's descriptor batches: kRdInline files per launch"""
    out = []
    for c0 in range(0, len(files), K.RD_INLINE):
        batch = [files[i if bug == "batch_rereads" else c0 + i] for i in range(min(K.RD_INLINE, len(files) - c0))]
        out += [read_state(sw)[:2] for sw in batch]
    return out


def test_second_descriptor_batch():
    for name in ("G_files_17", "G_file16_declines"):
        c = CASES[name]
        want = [(r, oracle_entries(sw) if r == "device" else None) for sw, r in zip(c.files, c.routes)]
        assert read_many(c.files) == want
        assert read_many(c.files, bug="batch_rereads") != want
