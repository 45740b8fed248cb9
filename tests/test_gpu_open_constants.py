"""The default fused open (k_open_fold_v3, crdt-enc_amd/csrc/ce_fused.hip) over every value of the
per-file quantities its iteration derives from the plaintext length, and over the edges of the
decode's single-writer template path.

A file's length fixes nblk = ceil(len / 64) (1..64: which lanes own a block, and how many), the
last block's missing Poly1305 pieces delta = 4 nblk - ceil(len / 16) (0..3: lane 0's shifted
pieces and the exponent of r^(6 - delta)) and the last piece's byte count (1..16: the tag bytes
masked off it).  One file per length walks all of them; CE_TEST_GRID_CAP makes one wave (cap 1)
or three take the whole batch, so each length follows another inside a wave's loop.  The template
path (a writer's own increments checked as whole words against Dot 0) is entered, left early and
left late by files built for it: Dot counts around the 16 lanes, every counter width, a foreign
actor in the first and second round, Dots that are canonical in no or another way.

Every comparison is bit-exact against the oracles: return code, per-file statuses and
state_bytes() == serialize(); a rejected batch leaves the state as it was."""
import functools
import random

import msgpack
import pytest

import crdtenc
import oracle
import pncounter_model as pm
import wave_run_corpus as W
from wave_run_worker import run_scenario, set_cap

pytestmark = pytest.mark.gpu

SMALL_MAX = 4096  # kSmallMax (ce_kernels.h): the largest plaintext the fused kernel takes
# counter ranges by msgpack width: Dot lengths 34 (fixint), 35 (cc), 36 (cd), 38 (ce), 42 (cf)
WIDTH = {34: (0, 127), 35: (128, 255), 36: (256, 65535), 38: (65536, (1 << 32) - 1), 42: (1 << 32, (1 << 62) - 1)}


@pytest.fixture(scope="module")
def ctx():
    c = crdtenc.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _no_cap_left_behind():
    yield
    set_cap(None)


def check(ctx, corpus, name, cap, kernel="open_v3_p0e1"):
    where = (name, cap)
    set_cap(cap)
    rc, st, state, before, paths = run_scenario(ctx, corpus, name)
    set_cap(None)
    orc, ost, ostate = W.expected(corpus, name)
    assert rc == orc == corpus.want_rc[name], (where, rc, orc, ctx.last_error())
    assert st == ost, (where, [(i, a, b) for i, (a, b) in enumerate(zip(st, ost)) if a != b][:10])
    assert state == ostate, where
    if corpus.want_rc[name] != 0:
        assert state == before, where
    assert {k for k in W.OPEN_KEYS if paths[k]} == {kernel}, (where, paths)
    assert (paths[W.CAPPED] > 0) == bool(cap), (where, paths)


def in_runs(n, writers):
    """(writer, version) of n files in load_ops order: `writers` runs, none a multiple of 4 long"""
    fa, vers = [], []
    for w, r in enumerate(W.uneven_runs(n, writers)):
        fa += [w] * r
        vers += list(range(r))
    return fa, vers


# ------------------------------------------------------------------ every plaintext length
@functools.lru_cache(maxsize=None)
def every_length_corpus(seed=20241019):
    """One file per plaintext length 17..4096 (16 bytes hold no Vec: bad_files_corpus), shuffled,
    of 7 writers.  Half of the files are a writer's own increments at one counter width (the
    template path), the others mix actors and widths from Dot to Dot."""
    rng = random.Random(seed)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(7))
    lens = list(range(17, SMALL_MAX + 1))
    rng.shuffle(lens)
    fa, vers = in_runs(len(lens), 7)
    files = []
    for L, w in zip(lens, fa):
        own = rng.random() < 0.5
        fixed = WIDTH[rng.choice((35, 36, 38, 42))]

        def draw():
            if own:
                return W._dot(actors[w], rng.randint(*fixed))
            return W._dot(actors[w] if rng.random() < 0.8 else rng.choice(actors), rng.randint(*WIDTH[rng.choice(sorted(WIDTH))]))
        files.append(W.seal(key, W._dots_clear(rng, L, [], draw), rng))
    c = W.Corpus("gcounter", key, actors, files, fa, vers, lens)
    c.scenarios["clean"] = [(list(range(len(files))), {})]
    c.want_rc["clean"] = 0
    return c


def test_every_length_corpus_walks_every_value():
    """(no GPU work) the batch holds every nblk, every delta and every last-piece byte count"""
    lens = every_length_corpus().lens
    assert sorted(lens) == list(range(17, SMALL_MAX + 1))
    assert {(L + 63) // 64 for L in lens} == set(range(1, 65))
    assert {4 * ((L + 63) // 64) - (L + 15) // 16 for L in lens} == {0, 1, 2, 3}
    assert {L - 16 * ((L + 15) // 16 - 1) for L in lens} == set(range(1, 17))


@pytest.mark.parametrize("cap", [None, 1, 3])
def test_every_plaintext_length_in_one_batch(ctx, cap):
    check(ctx, every_length_corpus(), "clean", cap)


# ------------------------------------------------------------------ tampered and bad files
def flip(f, at, bit):
    b = bytearray(f)
    b[at] ^= bit
    return bytes(b)


@functools.lru_cache(maxsize=None)
def bad_files_corpus(seed=20241020):
    """Step one: a clean file of each of 48 lengths (both ends of the range, every delta and
    last-piece count among them).  Step two, the writers' next versions: for each length a clean
    file and three tampered copies (a bit of the first ciphertext byte, of the last one, of the
    tag), then a 16-byte plaintext (no Vec), a wrong outer version, a file sealed under another
    key, an array header that overstates its count and an unsupported data version."""
    rng = random.Random(seed)
    key, other_key = rng.randbytes(32), rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(5))
    lens = [17, 18, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 113, 127, 128, 129, 1000, 1023, 1024, 1025,
            2047, 2048, 2049, 3071, 3072, 3073, 4031, 4032, 4033, 4047, 4048, 4049, 4063, 4064, 4065, 4079, 4080,
            4081, 4085, 4090, 4091, 4092, 4093, 4094, 4095, 4096]
    assert len(lens) == 48

    def clear(L, w):
        return W._dots_clear(rng, L, [], lambda: W._dot(actors[w], rng.randint(*WIDTH[38])))
    per = -(-len(lens) // len(actors))
    first_files, first_fa, first_v = [], [], []
    for i, L in enumerate(lens):
        w = i // per
        first_files.append(W.seal(key, clear(L, w), rng))
        first_fa.append(w)
        first_v.append(i % per)
    nextv = {w: first_fa.count(w) for w in range(len(actors))}
    files, fa, vers, plens = list(first_files), list(first_fa), list(first_v), list(lens)

    def add(w, f, L):
        files.append(f)
        fa.append(w)
        vers.append(nextv[w])
        plens.append(L)
        nextv[w] += 1
    for w in range(len(actors)):  # step two stays in load_ops order: writer by writer
        for i, L in enumerate(lens):
            if i // per != w:
                continue
            add(w, W.seal(key, clear(L, w), rng), L)
            good = W.seal(key, clear(L, w), rng)
            for at, bit in ((-(16 + L), 0x01), (-17, 0x80), (-16 + i % 16, 1 << (i % 8))):
                add(w, flip(good, at, bit), L)
        if w == 1:
            add(w, W.seal(key, W.APP, rng), 16)
        if w == 2:
            add(w, b"\x5a" + W.seal(key, clear(500, w), rng)[1:], 500)
        if w == 3:
            add(w, W.seal(other_key, clear(700, w), rng), 700)
            dots = [W._dot(actors[w], 70000 + j) for j in range(40)]
            add(w, W.seal(key, W.APP + W._arr_header(41) + b"".join(dots), rng), 16 + 3 + 40 * 38)
        if w == 4:
            add(w, W.seal(key, bytes(16) + clear(900, w)[16:], rng), 900)
    c = W.Corpus("gcounter", key, actors, files, fa, vers, plens)
    n1 = len(lens)
    c.scenarios["first"] = [(list(range(n1)), {})]
    c.want_rc["first"] = 0
    c.scenarios["bad"] = [(list(range(n1)), {}), (list(range(n1, len(files))), {})]
    return c


@pytest.mark.parametrize("cap", [None, 1])
def test_tampered_and_bad_files(ctx, cap):
    corpus = bad_files_corpus()
    orc, ost, _ = W.expected(corpus, "bad")
    corpus.want_rc["bad"] = orc
    assert orc != 0
    # the oracle rejects each kind for its own reason: tag, outer version, decode, data version
    assert {9, 2, 12, 11} <= set(ost), sorted(set(ost))
    assert ost.count(9) >= 3 * 48 + 1
    check(ctx, corpus, "first", cap)
    check(ctx, corpus, "bad", cap)


# ------------------------------------------------------------------ template-path edges
@functools.lru_cache(maxsize=None)
def template_edges_corpus(seed=20241021):
    """Single-writer files of 1, 2, 15, 16, 17, 32, 33 and 107 Dots at each Dot length 35, 36, 38
    and 42 (97 Dots at 42: one page); the same with another writer's Dot in place 1, 15, 16, 17
    and last; files whose Dot 0 is not canonical (keys in the other order, a str8 key), whose
    counters are fixints, and whose first Dot alone is a fixint."""
    rng = random.Random(seed)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(4))
    clears = []

    def dots(w, n, L):
        return [W._dot(actors[w], rng.randint(*WIDTH[L])) for _ in range(n)]

    def pack(ds, tail=0):
        return W.APP + W._arr_header(len(ds)) + b"".join(ds) + rng.randbytes(tail)
    for L in (35, 36, 38, 42):
        top = 97 if L == 42 else 107
        for n in (1, 2, 15, 16, 17, 32, 33, top):
            clears.append(pack(dots(0, n, L), tail=n % 3))
        for n in (18, 33, top):
            for at in (1, 15, 16, 17, n - 1):
                ds = dots(1, n, L)
                ds[at] = W._dot(actors[2], rng.randint(*WIDTH[L]))
                clears.append(pack(ds))
    other_order = msgpack.packb({"counter": 70000, "actor": actors[3]}, use_bin_type=True)
    str8_key = b"\x82\xd9\x05actor\xc4\x10" + actors[3] + b"\xa7counter\xce" + (70001).to_bytes(4, "big")
    for first in (other_order, str8_key, W._dot(actors[3], 5)):
        clears.append(pack([first] + dots(3, 40, 38)))
    clears.append(pack(dots(3, 50, 34)))
    clears.append(pack([W._dot(actors[3], 7)] + dots(3, 20, 34) + dots(3, 20, 36)))
    # in load_ops order: by writer (the file's first own Dot names it), versions in turn
    by_writer = sorted(range(len(clears)), key=lambda i: (_writer_of(clears[i], actors), i))
    files, fa, vers, seen = [], [], [], {}
    for i in by_writer:
        w = _writer_of(clears[i], actors)
        files.append(W.seal(key, clears[i], rng))
        fa.append(w)
        vers.append(seen.get(w, 0))
        seen[w] = vers[-1] + 1
    c = W.Corpus("gcounter", key, actors, files, fa, vers, [len(clears[i]) for i in by_writer])
    c.scenarios["clean"] = [(list(range(len(files))), {})]
    c.want_rc["clean"] = 0
    return c


def _writer_of(clear, actors):
    """the writer a template_edges_corpus file belongs to: the actor most of its Dots name"""
    return max(range(len(actors)), key=lambda w: clear.count(actors[w]))


@pytest.mark.parametrize("cap", [None, 1, 3])
def test_template_path_edges(ctx, cap):
    corpus = template_edges_corpus()
    assert max(corpus.lens) <= SMALL_MAX and len(corpus.files) == 4 * (8 + 15) + 5
    check(ctx, corpus, "clean", cap)


# ------------------------------------------------------------------ PNCounter
@functools.lru_cache(maxsize=None)
def pncounter_small_corpus(seed=20241022):
    """24 files of 16 ops (384 ops) of 3 writers, both directions, counters of every width"""
    rng = random.Random(seed)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(3))
    files, fa, vers = [], [], []
    for w in range(3):
        for v in range(8):
            lo, hi = WIDTH[(35, 36, 38, 42)[(w + v) % 4]]
            ops = [((actors[w] if rng.random() < 0.85 else rng.choice(actors), rng.randint(lo, hi)), rng.choice(pm.DIRS))
                   for _ in range(16)]
            files.append(W.seal(key, W.APP + pm.enc_ops(ops), rng))
            fa.append(w)
            vers.append(v)
    c = W.Corpus("pncounter", key, actors, files, fa, vers, [0] * len(files))
    c.scenarios["clean"] = [(list(range(len(files))), {})]
    c.want_rc["clean"] = 0
    return c


@pytest.mark.parametrize("cap", [None, 1])
def test_small_pncounter_batch(ctx, cap):
    check(ctx, pncounter_small_corpus(), "clean", cap, kernel="open_v3_pn")
