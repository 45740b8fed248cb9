"""StateWrapper<Orswot<u64, Uuid>> files aimed at the edges of the device state writer and reader
(crdt-enc_amd/csrc/ce_dotset_io.hip): msgpack width rungs, map-header counts, 2048-pair scan
tiles, 256-pair output blocks, 16-byte output pieces, 4096-byte head-search chunks and their
256-position rows, the 4096-byte tail window, 16 descriptors per launch, the heads before the
entries.  CPU only and deterministic: tests/test_orswot_state_cases_model.py checks every fact
claimed here from the bytes, tests/test_gpu_orswot_states.py runs the files through the kernels.

Every file is written with oracle.crdts' own primitives (Wr) through one splicing encoder, so a
non-canonical form is the same code with one piece swapped; a case marked `canonical` is asserted
to be what oracle.crdts.serialize gives for its decoded state.

A case's `routes` say, file by file, where the project's rules send it: "device" (read by the
kernels) or "host" (declined to the host parser).  The reasons are in each case's `doc`."""
import functools
import hashlib
import itertools

import msgpack

from oracle import crdts as C

U64 = (1 << 64) - 1
EDGES = [0, 1, 127, 128, 255, 256, 65535, 65536, (1 << 32) - 1, 1 << 32, U64]
HEAD = b"\x81\xa4dots"
TILE, BLOCK, CHUNK, ROW, TAIL_WIN, RD_INLINE, HEAD_HINT, SER_MAX_DOT = 2048, 256, 4096, 256, 4096, 16, 16384, 47


class Case:
    def __init__(self, name, files, routes, doc, canonical=True, **facts):
        self.name, self.family = name, name[0]
        self.files = [files] if isinstance(files, bytes) else list(files)
        self.routes = [routes] * len(self.files) if isinstance(routes, str) else list(routes)
        assert len(self.routes) == len(self.files) and set(self.routes) <= {"device", "host"}
        self.doc, self.canonical, self.facts = doc, canonical, facts

    def __repr__(self):
        return "Case(%s)" % self.name


# ------------------------------------------------------------------------------------------ bytes
def uid(i, tag=b"actor"):
    return hashlib.sha256(tag + b"%d" % i).digest()[:16]


def uint_b(v):
    w = C.Wr()
    w.uint(v)
    return bytes(w.b)


def map_b(n, form=None):
    if form is None:
        w = C.Wr()
        w.map(n)
        return bytes(w.b)
    return {"fix": lambda: bytes([0x80 | n]), "de": lambda: b"\xde" + n.to_bytes(2, "big"),
            "df": lambda: b"\xdf" + n.to_bytes(4, "big")}[form]()


def vc_b(dots, reverse=False, hdr=None, counter_enc=uint_b):
    items = sorted(dict(dots).items(), reverse=reverse)
    return HEAD + map_b(len(items), hdr) + b"".join(b"\xc4\x10" + a + counter_enc(c) for a, c in items)


def entry_b(m, dots, member_enc=uint_b, **kw):
    return member_enc(m) + vc_b(dots, **kw)


def deferred_b(items):
    enc = sorted((vc_b(d), sorted(ms)) for d, ms in items)
    out = map_b(len(enc))
    for kb, ms in enc:
        w = C.Wr()
        w.arr(len(ms))
        for m in ms:
            w.uint(m)
        out += kb + bytes(w.b)
    return out


def state_b(nov, clock, entries, deferred=(), order=("clock", "entries", "deferred"), trailer=b""):
    """entries: (member, dots) pairs or ready bytes, in the order given"""
    ents = [e if isinstance(e, bytes) else entry_b(*e) for e in entries]
    f = {"clock": b"\xa5clock" + vc_b(clock), "entries": b"\xa7entries" + map_b(len(ents)) + b"".join(ents),
         "deferred": b"\xa8deferred" + deferred_b(deferred)}
    return b"\x82\xb0next_op_versions" + vc_b(nov) + b"\xa5state\x83" + b"".join(f[k] for k in order) + trailer


def clock_for(entries, extra=()):
    ck = dict(extra)
    for _, dots in entries:
        for a, c in dict(dots).items():
            ck[a] = max(ck.get(a, 0), c)
    return ck


def canon(entries, nov=None, extra_clock=(), deferred=()):
    entries = sorted(entries, key=lambda e: e[0])
    ck = clock_for(entries, extra_clock)
    return state_b(nov if nov is not None else {a: 1 for a in list(ck)[:2]}, ck, entries, deferred)


def of_width(w, i=0):
    """the i-th distinct value whose smallest encoding takes w bytes"""
    return {1: i, 2: 128 + i, 3: 256 + i, 5: 65536 + i, 9: (1 << 32) + i}[w]


# ------------------------------------------------------------------------------------------ layout facts
def layout(sw):
    """offsets of a file in the canonical field order: prefix (the bytes before the entries' map
    header), lo (the first entry), n (the header's count), end (after the last entry), hi"""
    i = sw.index(b"\xa7entries") + 8
    prefix = i
    m = sw[i]
    if (m & 0xf0) == 0x80:
        n, i = m & 15, i + 1
    elif m == 0xde:
        n, i = int.from_bytes(sw[i + 1:i + 3], "big"), i + 3
    else:
        assert m == 0xdf
        n, i = int.from_bytes(sw[i + 1:i + 5], "big"), i + 5
    u = msgpack.Unpacker(raw=True, strict_map_key=False, max_buffer_size=len(sw) + 1)
    u.feed(sw[i:])
    for _ in range(2 * n):
        u.skip()
    return {"prefix": prefix, "lo": i, "n": n, "end": i + u.tell(), "hi": len(sw)}


def head_positions(sw, lo=0, hi=None):
    """every position where an entry head pattern begins (81 a4 "dots" and a map marker)"""
    hi = len(sw) if hi is None else hi
    out, p = [], sw.find(HEAD, lo)
    while p >= 0 and p + 7 <= hi:
        m = sw[p + 6]
        if (m & 0xf0) == 0x80 or m in (0xde, 0xdf):
            out.append(p)
        p = sw.find(HEAD, p + 1)
    return out


def head_counts(sw):
    """candidate heads before, inside and after the entries"""
    L = layout(sw)
    hp = head_positions(sw)
    return (sum(p < L["lo"] for p in hp), sum(L["lo"] <= p < L["end"] for p in hp), sum(p >= L["end"] for p in hp))


def runs_of(sw):
    """Dots per entry in member order: the writer's runs over its sorted pairs"""
    _, st = C.dec_state("orswot", sw)
    return [len(st.entries[m].dots) for m in sorted(st.entries)]


def run_starts(runs):
    return list(itertools.accumulate([0] + runs[:-1]))


# ------------------------------------------------------------------------------------------ families
ACT = sorted(uid(i) for i in range(24))


def entries_from_runs(runs, member_of=lambda i: 300 + 3 * i, counter_of=lambda i, j: 1 + (i + j) % 200):
    return [(member_of(i), {ACT[j]: counter_of(i, j) for j in range(k)}) for i, k in enumerate(runs)]


def family_a():
    out = []
    ctrs = EDGES[1:]
    ent = [(m, {ACT[j]: c for j, c in enumerate(ctrs)}) for m in EDGES]
    extra = {uid(i, b"clock"): c for i, c in enumerate(ctrs)}
    nov = {uid(i, b"nov"): c for i, c in enumerate(ctrs)}
    out.append(Case("A_cross", canon(ent, nov, extra), "device",
                    "every member width x every counter width; each width in the clock and next_op_versions",
                    members=EDGES, counters=ctrs))
    alone = [canon([(m, {uid(i, b"alone"): c})], {ACT[1]: c}) for i, (m, c) in enumerate(zip(EDGES, ctrs + [77]))]
    out.append(Case("A_each_alone", alone, "device",
                    "one entry per file: each member edge alone, with one counter edge"))
    ent = [((1 << 32) + 5 * i, {ACT[i % 3]: (1 << 32) + i}) for i in range(256)]
    out.append(Case("A_wide256", canon(ent), "device",
                    "256 single-Dot entries, cf member and cf counter: 43 staged bytes per pair", pair_bytes=43, pairs=256))
    return out


def family_b():
    out = []
    for n in (1, 15, 16, 17, 65535, 65536):
        ent = [(2 * i, {ACT[i & 1]: 1 + (i & 63)}) for i in range(n)]
        out.append(Case("B_entries_%d" % n, canon(ent), "device", "entry count at a map-header edge", n=n))
    ent = entries_from_runs([1, 15, 16, 17, 16, 15, 1])
    out.append(Case("B_dots_per_entry", canon(ent), "device", "per-entry map header fixmap 1, 15 and de 16, 17",
                    runs=[1, 15, 16, 17, 16, 15, 1]))
    ck = {ACT[0]: 5, ACT[1]: 1 << 40}
    out.append(Case("B_no_entries", state_b({ACT[0]: 2}, ck, []), "host", "ne == 0: the reader leaves it to the host", n=0))
    dfr = [({ACT[0]: 9}, [1, 2, 300]), ({ACT[2]: 1, ACT[1]: (1 << 40) + 1}, [U64])]
    out.append(Case("B_no_entries_deferred", state_b({ACT[0]: 2}, ck, [], dfr), "host",
                    "ne == 0 with a non-empty deferred map: the writer has n == 0 and a tail", n=0))
    return out


def _runs_to(total, specials):
    """runs summing to `total`: 1, 2, 3 in turn, with each (start, length) of `specials` in place"""
    runs, at, cyc = [], 0, itertools.cycle([1, 2, 3])
    for s, k in sorted(specials) + [(total, 0)]:
        while at < s:
            r = min(next(cyc), s - at)
            runs.append(r)
            at += r
        if k:
            runs.append(k)
            at += k
    assert sum(runs) == total, (sum(runs), total)
    return runs


def family_c():
    out = []
    for p in (255, 256, 257, 2047, 2048, 2049, 4096, 4097):
        runs = _runs_to(p, [(p - 1, 1)])
        out.append(Case("C_pairs_%d" % p, canon(entries_from_runs(runs)), "device", "pair count at a block / tile edge; "
                        "the last pair is a head", pairs=p, last_is_head=True))
    shapes = {
        "C_run_straddles_tile": (2100, [(2047, 3), (2099, 1)], "a run from pair 2047 to 2049"),
        "C_run_ends_at_tile": (2100, [(2044, 4), (2048, 2), (2099, 1)], "a run ends at pair 2047, the next starts at 2048"),
        "C_run17_straddles_block": (300, [(250, 17), (299, 1)], "a run of 17 from pair 250 to 266"),
        "C_all_in_middle_tiles": (3 * 2048 + 5, [(2044, 4), (2048, 2), (2048 + 250, 17), (4095, 3), (6143, 1),
                                                 (3 * 2048 + 4, 1)],
                                  "all of the above in tiles 1 and 2 of four; pair 6143 and the last pair are heads"),
    }
    for name, (p, sp, doc) in shapes.items():
        out.append(Case(name, canon(entries_from_runs(_runs_to(p, sp))), "device", doc, pairs=p, specials=sp))
    return out


def family_d():
    """one state of ~3000 pairs under 16 heads whose length takes every residue mod 16"""
    ent = sorted(entries_from_runs(_runs_to(3001, []), member_of=lambda i: 1 + 37 * i * i))
    found = {}
    for k, w in itertools.product(range(0, 9), (1, 2, 3, 5, 9)):
        extra = {uid(i, b"pad"): of_width(w, 1 + i) for i in range(k)}
        sw = state_b({ACT[0]: 3}, clock_for(ent, extra), ent)
        found.setdefault(layout(sw)["prefix"] % 16, sw)
    assert sorted(found) == list(range(16)), sorted(found)
    return [Case("D_prefix_mod16_%d" % r, found[r], "device", "prefix length = %d mod 16" % r, residue=r, pairs=3001)
            for r in sorted(found)]


def _head_at(target):
    """a state whose last entry's head begins at file offset `target`: cd members, entries of 29
    or 30 bytes (a fixint or a cc counter) before it"""
    def build(rel):
        n, r = divmod(rel - 3, 29)
        assert 16 <= n < 65536 and 0 <= r <= n
        ent = [(256 + i, {ACT[0]: 128 if i < r else 1}) for i in range(n)] + [(256 + n, {ACT[0]: 1, ACT[1]: 2})]
        return state_b({ACT[2]: 1}, {ACT[0]: 128, ACT[1]: 2}, ent)
    lo = layout(build(target))["lo"]  # (the same head and a de header for every count used here)
    return build(target - lo)


def family_e():
    out = []
    for edge, name in ((CHUNK, "chunk"), (5 * ROW, "row")):
        ts = list(range(edge - 7, edge + 1))
        out.append(Case("E_head_across_%s_edge" % name, [_head_at(t) for t in ts], "device",
                        "the last entry's head begins 7 .. 0 bytes before file offset %d: the head search runs over the "
                        "whole file from offset 0, before the host knows where the entries start, so its chunks and "
                        "rows are cut at file offsets" % edge, targets=ts))
    last = entry_b(9, {})
    sw = state_b({ACT[0]: 1}, {ACT[0]: 4}, [entry_b(5, {ACT[0]: 4}), last], order=("clock", "deferred", "entries"))
    assert sw.endswith(HEAD + b"\x80")
    out.append(Case("E_head_ends_at_hi", sw, "host", "the file's last 7 bytes are a head (an entry with an empty Dot map, "
                    "`entries` written last): the canonical field order puts `deferred` after the entries, so a file "
                    "that ends in a head is never in that order and the prefix parse declines it; the head search "
                    "still runs over the whole file before the prefix is known", canonical=False, head_at=len(sw) - 7))
    sw = canon(entries_from_runs([1, 2, 3])) + HEAD
    out.append(Case("E_six_head_bytes_at_hi", sw, "device", "six head bytes end the file (trailing bytes after the value "
                    "are ignored): no head, whatever byte follows the buffer", canonical=False))

    def spur(i, j=0x83):
        return HEAD + bytes([j]) + uid(i, b"spur")[:9]
    ent = entries_from_runs([1, 2, 3, 2, 1])
    for n in (300, 1200):
        extra = {spur(i): 1 + i for i in range(n)}
        out.append(Case("E_spurious_in_clock_%d" % n, canon(ent, {spur(0): 1, ACT[0]: 2}, extra), "device",
                        "%d heads inside clock-only actor UUIDs before the entries%s" %
                        (n, "; after `primer` (a core's first merge fetches 256 KiB, later ones what the last head "
                         "needed, 16 KiB at the least) the head exceeds the hint" if n == 1200 else ""), spurious=n,
                        **({"primer": canon(entries_from_runs([1, 1]))} if n == 1200 else {})))
    a = spur(7, 0xde)
    out.append(Case("E_spurious_in_entry_uuid", canon([(1, {ACT[0]: 1}), (2, {a: 5, ACT[1]: 2}), (3, {ACT[0]: 9})]), "host",
                    "a head inside an entry Dot's UUID: the candidate list is off by one, the chain check fails"))
    c = int.from_bytes(HEAD + b"\x81\x00", "big")
    out.append(Case("E_spurious_in_counter", canon([(1, {ACT[0]: 1}), (2, {ACT[0]: c, ACT[1]: 2}), (3, {ACT[0]: 9})]), "host",
                    "a head inside an entry Dot's cf counter"))
    m = int.from_bytes(HEAD + b"\xdf\x01", "big")
    out.append(Case("E_spurious_in_member", canon([(1, {ACT[0]: 1}), (m, {ACT[0]: 3}), (m + 1, {ACT[0]: 9})]), "host",
                    "a head inside a cf member key"))
    dfr = [({uid(i, b"dfr"): 10 + i, ACT[0]: 100 + i}, [i, 1000 + i]) for i in range(40)]
    out.append(Case("E_heads_only_in_deferred", canon(ent, deferred=dfr), "device",
                    "40 deferred clocks after the entries: the first N heads are the entries", deferred=40))
    return out


def _tail_of(length):
    """a deferred map of one clock whose `deferred` field takes `length` bytes after the entries"""
    base = len(b"\xa8deferred" + deferred_b([({uid(0, b"dfr"): 7}, [])])) + 2  # (array header dc xx xx)
    q, r = divmod(length - base, 9)
    small = {0: [], 1: [1], 2: [2], 3: [3], 4: [2, 2], 5: [5], 6: [3, 3], 7: [5, 2], 8: [5, 3]}[r]
    ms = [of_width(w, 1 + small[:k].count(w)) for k, w in enumerate(small)] + [of_width(9, i) for i in range(q)]
    return [({uid(0, b"dfr"): 7}, ms)]


def family_f():
    out = []
    base = entries_from_runs([2, 1, 3, 1])
    ck = clock_for(base)
    nov = {ACT[0]: 2}
    stranger = uid(1, b"stranger")
    ent = base + [(5000, {stranger: 3})]
    out.append(Case("F_actor_not_in_clock", state_b(nov, ck, ent), "host", "an entry Dot's actor is absent from the clock: "
                    "the emit's table lookup misses (flag 4)"))
    for m, tag in ((base[1][0], "small"), (U64, "all_ones")):
        ent = [e for e in base if e[0] != m] + [(m, {ACT[0]: 1}), (7000, {ACT[1]: 1}), (m, {ACT[1]: 2})]
        out.append(Case("F_repeated_member_%s" % tag, state_b(nov, clock_for(ent), ent), "host",
                        "a member written twice: the later clock wins (HashMap insert)", canonical=False))
    ent = [entry_b(m, d, reverse=True) for m, d in base]
    out.append(Case("F_descending_dots", state_b(nov, ck, ent), "host", "Dots in descending UUID order", canonical=False))
    ent = [entry_b(m, d, counter_enc=lambda c: b"\xcd" + c.to_bytes(2, "big")) for m, d in base]
    out.append(Case("F_long_counter", state_b(nov, ck, ent), "host", "counters as cd 00 xx", canonical=False))
    ent = [entry_b(5, {ACT[0]: 1}, member_enc=lambda m: b"\xcd" + m.to_bytes(2, "big"))] + [entry_b(*e) for e in base]
    out.append(Case("F_long_member", state_b(nov, ck, ent), "host", "a member as cd 00 05: the chain check's canonical "
                    "length does not fill the gap", canonical=False))
    for form in ("de", "df"):
        ent = [entry_b(m, d, hdr=form) for m, d in base]
        out.append(Case("F_entry_header_%s" % form, state_b(nov, ck, ent), "device",
                        "per-entry Dot maps under a %s header with a small count: k_rdm_entry and k_rdm_emit read all "
                        "three header forms, and the chain check needs only the end of each entry" % form, canonical=False))
    for n in (TAIL_WIN - 1, TAIL_WIN, TAIL_WIN + 1):
        sw = state_b(nov, ck, base, _tail_of(n))
        out.append(Case("F_tail_%d" % n, sw, "device", "%d bytes after the last entry, against the %d-byte window" %
                        (n, TAIL_WIN), tail=n))
    return out


def _g_file(i, n):
    a, b = uid(i, b"ga"), uid(i, b"gb")
    return canon([((i * 7919 + j * 13) % 60000, {a: j + 1, b: 2 * j + 1}) for j in range(n)], {a: 1 + i % 3})


def g_sizes(n):
    return [[1, 2049, 3, 4097][i % 4] if i < 4 or 16 <= i < 20 else [2, 130, 7, 600, 5, 33][i % 6] for i in range(n)]


def family_g():
    out = []
    for n in (1, 2, 16, 17, 64, 65):
        files = [_g_file(i, s) for i, s in enumerate(g_sizes(n))]
        out.append(Case("G_files_%d" % n, files, "device", "%d files of unequal sizes, later files of a launch batch larger "
                        "than its first" % n, kway=2 <= n <= 64, early=2 <= n <= RD_INLINE))
    files = [_g_file(i, s) for i, s in enumerate(g_sizes(17))]
    ent = [(5, {ACT[0]: 1}), (6, {ACT[0]: 2}), (5, {ACT[0]: 3})]
    files[16] = state_b({ACT[0]: 1}, clock_for(ent), ent)
    out.append(Case("G_file16_declines", files, ["device"] * 16 + ["host"], "17 files; file 16, alone in the second "
                    "descriptor batch, repeats a member", canonical=False, kway=False, early=False))
    files = [_g_file(i, s) for i, s in enumerate([40, 50, 60])]
    a = uid(1, b"ga")
    files[1] = canon([((7919 + j * 13) % 60000, {a: j + 1}) for j in range(50)], {a: 1},
                     deferred=[({a: 90}, [13, 60001]), ({uid(9, b"gz"): 1}, [5])])
    out.append(Case("G_middle_has_deferred", files, "device", "3 files, the middle one with a deferred map: the early merge "
                    "is queued and must stay idle", kway=False, early=False))
    return out


def strip_zeros(sw):
    """the same file with every zero-counter Dot removed (a clock, an entry's Dots, a deferred key)"""
    nov, st = C.dec_state("orswot", sw)

    def nz(d):
        return {a: c for a, c in dict(d).items() if c}
    dfr = {}
    for k, ms in st.deferred.items():
        dfr.setdefault(tuple(sorted(nz(k).items())), set()).update(ms)
    ent = sorted((m, nz(v.dots)) for m, v in st.entries.items())
    return state_b(nz(nov.dots), nz(st.clock.dots), ent, [(dict(k), ms) for k, ms in dfr.items()])


def family_h():
    out = []
    z = uid(0, b"zero")
    nov, ck = {ACT[0]: 2}, {ACT[0]: 9, ACT[1]: 9, z: 4}
    e_ok = [(10, {ACT[0]: 5}), (30, {ACT[1]: 7})]
    cases = {
        "H_zero_beside_dot": (state_b(nov, ck, sorted(e_ok + [(20, {z: 0, ACT[0]: 5})])), False,
                              "an entry with a zero-counter Dot beside a live one"),
        "H_only_zero_dot": (state_b(nov, ck, sorted(e_ok + [(20, {z: 0})])), True, "an entry whose only Dot is zero"),
        "H_zero_in_clock": (state_b(nov, {**ck, uid(1, b"zero"): 0}, e_ok), True, "a zero Dot in the clock"),
        "H_zero_in_nov": (state_b({**nov, uid(1, b"zero"): 0}, ck, e_ok), True, "a zero Dot in next_op_versions"),
        "H_zero_in_deferred_key": (state_b(nov, ck, e_ok, [({z: 0, ACT[0]: 50}, [10, 11])]), False,
                                   "a zero Dot in a deferred clock"),
    }
    for name, (sw, same, doc) in cases.items():
        out.append(Case(name, sw, "device", doc, canonical=False, stripped=strip_zeros(sw), same_as_reference=same))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    cs = family_a() + family_b() + family_c() + family_d() + family_e() + family_f() + family_g() + family_h()
    names = [c.name for c in cs]
    assert len(set(names)) == len(names)
    return {c.name: c for c in cs}


def family(letter):
    return [c for c in all_cases().values() if c.family == letter]
