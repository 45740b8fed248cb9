"""The Poly1305 edge vectors of tests/poly_edges.py, checked on the CPU (no GPU): every crafted
file is authentic under a big-integer reference that shares no code with the kernels, and under
the C oracle; every reject twin is not; the scenarios' return codes and statuses; the oracle's
own Poly1305 at the extremes of r, s and the message; and that the corpora hold every target
(see the docstring of poly_edges for what each one is for), every delta of k_open_fold_v3 and a
heavy r."""
import random

import pytest

import oracle
import poly_edges as E
import wave_run_corpus as W

H = bytes.fromhex
KINDS = ["gcounter", "pncounter", "orswot"]
CORPORA = {k: (lambda k=k: E.corpus(k)) for k in KINDS}
CORPORA["multi_page"] = E.multi_page_corpus


def n_clean(c):
    return len(c.scenarios["clean"][0][0])


def check_vector(v):
    """v against the reference and the oracle -> its plaintext"""
    assert (len(v.key), len(v.nonce)) == (32, 24)
    _, _, r, s = E.keys(v.key, v.nonce)
    assert (r, s) == (v.r, v.s)
    h = E.poly_h(r, v.ct)
    if v.T is not None:
        assert h == v.T < E.P, v.name
    assert (h + s) % (1 << 128) == v.tag == int.from_bytes(v.sealed()[-16:], "little"), v.name
    st, pt = oracle.xchacha_open(v.key, v.nonce, v.sealed())
    assert st == 0 and pt == v.plaintext(), v.name
    st, enc = oracle.cryptor_encrypt(v.key, v.nonce, pt)  # the same box, byte for byte
    assert st == 0 and enc == v.box(), v.name
    return pt


def check_twin(t):
    assert t.name == "twin%+d" % ((t.tag - t.of.tag + 8) % (1 << 128) - 8) and t.ct == t.of.ct and t.nonce == t.of.nonce
    assert t.tag != E.tag_of(t.r, t.s, t.ct)
    assert oracle.xchacha_open(t.key, t.nonce, t.sealed()) == (9, None), t.of.name
    assert oracle.cryptor_decrypt(t.key, t.box()) == (9, None)


# ------------------------------------------------------------------------------ the reference
def test_reference_rfc8439(kats):
    """The big-integer reference itself: RFC 8439 2.5.2, and the AEAD construction's tags of the
    OpenSSL-generated XChaCha20-Poly1305 vectors"""
    for v in kats["poly1305"]:
        assert E.poly1305(H(v["key"]), H(v["msg"])).hex() == v["tag"]
    for v in kats["xchacha"]:
        _, _, r, s = E.keys(H(v["key"]), H(v["nonce"]))
        ct, tag = v["ct_bytes"][:-16], v["ct_bytes"][-16:]
        assert E.tag_of(r, s, ct).to_bytes(16, "little") == tag, v["len"]


@pytest.mark.parametrize("rb", ["ff" * 16, "00" * 16, "01" + "00" * 15])
@pytest.mark.parametrize("sb", ["ff" * 16, "00" * 16])
def test_oracle_poly1305_against_the_reference(rb, sb):
    """oracle.poly1305 (the checker of every other test) at the extremes: r all ff (clamps to the
    largest r), zero and one; s all ff and zero; messages empty, zero, 2^128 - 5 as a block (h + m
    = p - 4 + ... next to the modulus) and pages of ff with and without a partial last block"""
    key = H(rb) + H(sb)
    for msg in (b"", bytes(64), b"\xfb" + b"\xff" * 15, b"\xff" * 4095, b"\xff" * 4096):
        assert oracle.poly1305(key, msg) == E.poly1305(key, msg), (rb, sb, len(msg))


def test_craft_hits_any_target():
    rng = random.Random(7)
    for _ in range(20):
        r = rng.getrandbits(128) & E.CLAMP
        L = rng.choice([48, 100, 1000, 4097])
        ct = rng.randbytes(L)
        j = rng.randrange(L // 16)
        T = rng.randrange(E.P)
        out, redraws = E.craft(r, ct, j, T, rng, E.free_ranges(L, 0, j))
        assert E.poly_h(r, out) == T and len(out) == L and redraws <= 64
        free = set(range(16 * j, 16 * j + 16)) | {i for lo, hi in E.free_ranges(L, 0, j) for i in range(lo, hi)}
        assert all(out[i] == ct[i] for i in range(L) if i not in free)


# ------------------------------------------------------------------------------ the corpora
@pytest.mark.parametrize("which", list(CORPORA))
def test_crafted_files_against_the_oracle(which):
    c = CORPORA[which]()
    assert CORPORA[which]() is c  # built once, shared
    n = n_clean(c)
    heads = set()
    for i, v in enumerate(c.vectors):
        assert c.files[i] == v.file() and len(v.ct) == c.lens[i]
        if v.of is not None:
            assert i >= n
            check_twin(v)
            continue
        pt = check_vector(v)
        assert pt[:16] == W.APP
        st, pt2 = oracle.cryptor_decrypt(c.key, c.files[i][16:])
        assert st == 0 and pt2 == pt
        heads.add(pt[16:80])
    # every file's op is its own (a wrongly rejected or dropped file changes the state)
    assert len(heads) == sum(1 for v in c.vectors if v.of is None)
    assert max(v.redraws for v in c.vectors) <= 64


@pytest.mark.parametrize("which", list(CORPORA))
def test_scenarios_by_the_oracle(which):
    c = CORPORA[which]()
    n = n_clean(c)
    assert set(c.scenarios) == {"clean", "reject"}
    # load_ops order in every step: writers ascending, each writer's versions consecutive
    for files, fa, vers in c.steps("reject"):
        assert fa == sorted(fa)
    for w in set(c.fa):
        assert [c.vers[i] for i in range(len(c.fa)) if c.fa[i] == w] == list(range(c.fa.count(w)))
    rc, st, state = W.expected(c, "clean")
    assert rc == 0 and st == [0] * n and state != W.new_oracle(c.kind).serialize()
    rc2, st2, state2 = W.expected(c, "reject")
    twins = [i - n for i in range(n, len(c.vectors)) if c.vectors[i].of is not None]
    assert rc2 == 9 and [i for i, s in enumerate(st2) if s] == twins == c.tampered and {st2[i] for i in twins} == {9}
    assert state2 == state
    assert len(twins) == 3 * sum(1 for v in c.vectors[:n] if v.name in E.TWINNED) > 0
    assert 0 not in twins and len(st2) - len(twins) >= 6  # fresh clean files among the twins
    # dropping any one clean file changes the state
    for i in (0, n // 2, n - 1):
        oc = W.new_oracle(c.kind)
        files, fa, vers = c.step([k for k in range(n) if k != i and (c.fa[k] != c.fa[i] or k < i)], {})
        assert oc.read_remote_ops(c.key, [W.APP], files, [c.actors[a] for a in fa], vers)[0] == 0
        assert oc.serialize() != state


@pytest.mark.parametrize("kind", KINDS)
def test_coverage(kind):
    c = E.corpus(kind)
    n = n_clean(c)
    clean = c.vectors[:n]
    assert 100 <= n <= 150
    at = {}
    for v in clean:
        if v.T is not None:
            assert E.target_holds(v.name, v.T, v.s, v.tag), v.name
            at.setdefault(v.name, set()).add(len(v.ct))
    assert set(at) == set(E.TARGETS) and all(len(x) >= 2 for x in at.values())
    fixed = E.fixed_targets()
    want = set(range(6)) | {E.P - d for d in range(1, 7)} | {(1 << 128) + 1, 1 << 129}
    want |= {(1 << k) + d for k in (26, 52, 78, 104) for d in (-5, -1, 0)}
    want |= {(1 << k) + d for k in (32, 64, 96, 128) for d in (-1, 0)}
    assert set(fixed.values()) == want and len(fixed) == 34
    assert {len(v.ct) for v in clean} == set(E.LENS) >= {100, 129, 2047, 2048, 2049, 4033, 4081, 4096}
    assert {W.DS_REGION - 1, W.DS_REGION, W.DS_REGION + 1, 4096} <= set(E.LENS)
    assert {E.delta(len(v.ct)) for v in clean if v.T is not None} == {0, 1, 2, 3}
    # the crafted block: first free, last full and the one before, with full and partial last pieces
    where = {(len(v.ct) // 16 - 1 - v.j, len(v.ct) % 16 != 0) for v in clean if v.T is not None}
    assert {(0, False), (0, True), (1, False), (1, True)} <= where
    assert sum(1 for v in clean if v.T is not None and v.j < 6) >= 30
    hv = [v for v in clean if v.name.startswith("heavy")]
    assert sorted((v.name, len(v.ct)) for v in hv) == [("heavy-00", 4081), ("heavy-00", 4096), ("heavy-ff", 4081), ("heavy-ff", 4096)]
    for v in hv:
        assert all(l & m == m for l, m in zip(E.limbs(v.r), E.HEAVY_MASKS)) and E.is_heavy(v.r)
        free = v.ct[80:]
        assert free == (b"\xff" if v.name == "heavy-ff" else b"\x00") * len(free)
    # the twins: tag - 5, tag + 5, tag + 1 of every file with T in 0..4 or p-5..p-1
    twinned = [v for v in clean if v.T is not None and (v.T < 5 or v.T >= E.P - 5)]
    assert [v.name in E.TWINNED for v in clean] == [v in twinned for v in clean] and len(twinned) == 30
    got = sorted((id(t.of), (t.tag - t.of.tag) % (1 << 128)) for t in c.vectors[n:] if t.of is not None)
    assert got == sorted((id(v), d % (1 << 128)) for v in twinned for d in (-5, 5, 1))


def test_multi_page_and_aead_vectors():
    c = E.multi_page_corpus()
    n = n_clean(c)
    assert {len(v.ct) for v in c.vectors[:n]} - {E.MULTI_SEGMENT} == set(E.MULTI_PAGE) == {4097, 5000, 9000}
    assert sorted(v.name for v in c.vectors[:n] if len(v.ct) == E.MULTI_SEGMENT) == ["0", "p-1", "tag=0"] and E.MULTI_SEGMENT > 2 * 16384
    assert sorted((v.name, len(v.ct)) for v in c.vectors[:n] if v.T is None) == [("heavy-00", 9000), ("heavy-ff", 9000)]
    assert all(E.is_heavy(v.r) for v in c.vectors[:n] if v.T is None)
    assert {len(t.ct) for t in c.vectors[n:] if t.of is not None} == set(E.MULTI_PAGE) | {E.MULTI_SEGMENT}
    key, vs = E.aead_vectors()
    assert E.aead_vectors()[1] is vs
    assert {len(v.ct) for v in vs} == {0, 16, 4096, 16384 - 16, 16384 + 1, 70000, (1 << 20) + 17, (65 << 14) + 4097}
    for v in vs:
        assert v.key == key
        check_vector(v)
        if v.T is not None:
            assert E.target_holds(v.name, v.T, v.s, v.tag)
        for t in v.twins():
            check_twin(t)
    seg = 16384 // 16  # Poly1305 blocks per segment; the length block is one more
    nsegs = {}
    for L in E.AEAD_LONG:
        mine = [v for v in vs if len(v.ct) == L]
        nsegs[L] = -(-((L + 15) // 16 + 1) // seg)
        assert sorted(v.name for v in mine) == sorted(["0", "p-1", "tag=0"] * 2 + ["heavy-ff"])
        # block 1, and the last full block: in the last segment unless that holds only the 1-byte piece
        last = (L // 16 - 1) // seg
        assert sorted(v.j for v in mine if v.T is not None) == [1] * 3 + [L // 16 - 1] * 3
        assert last == nsegs[L] - 1 or L == 16384 + 1
        assert E.is_heavy(next(v for v in mine if v.T is None).r)
    assert nsegs == {16384 - 16: 1, 16384 + 1: 2, 70000: 5, (1 << 20) + 17: 65, (65 << 14) + 4097: 66}
    assert set(E.SEAL_LENS) <= {len(v.ct) for v in vs}
