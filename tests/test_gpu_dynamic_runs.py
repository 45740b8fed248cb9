"""k_open_fold_v3's dynamic schedule (crdt-enc_amd/csrc/ce_fused.hip): a wave takes a fixed run of
file groups (CE_DYN_STATIC_PCT percent of an even share), then chunks of CE_DYN_CHUNK groups of
four files drawn from a ticket in the ingest's counter block, one chunk ahead.  What a wave
carries from group to group -- the next group's prefetched parameters, the speculated Dot length,
the actor cache, the pending (slot, max), the AuthFails tally -- now crosses chunks that are not
adjacent, the last chunk of a batch is partial, a wave may draw nothing at all, and a second launch
over the same counter block (the fold after actor-table misses) must find the ticket at zero.

C below is a chunk's file count, from the source's default constants; test_wave_stamps checks
them against the schedule the loaded library reports, so a library built with other values
fails there and does not quietly run these cases off its real edges.  The batches are a few hundred
bytes per file with some 4085-byte plaintexts (64 ChaCha20 blocks, every lane's four) placed on
chunk edges.  Every run is at the product's grid and with CE_TEST_GRID_CAP 1, 3 and 7 (read per
ingest), asserts through ce_core_path_count that an open_v3_* kernel ran and whether the cap took
effect, and is compared bit for bit with the oracle: return code, per-file statuses, and the
state bytes -- the serialized StateWrapper, next_op_versions included."""
import functools
import os
import random
import re

import pytest

import crdtenc
import gset_model as gm
import oracle
import pncounter_model as pm
import wave_run_corpus as W
from wave_run_worker import set_cap

pytestmark = pytest.mark.gpu
APP = W.APP
CAPS = [None, 1, 3, 7]
BIG = 4085  # plaintext bytes: nblk = 64
SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "crdt-enc_amd", "csrc", "ce_kernels.h")


def _schedule():
    src = open(SRC).read()
    chunk = int(re.search(r"#define CE_DYN_CHUNK (\d+)u", src).group(1))
    pct = int(re.search(r"#define CE_DYN_STATIC_PCT (\d+)u", src).group(1))
    return chunk, pct


CHUNK_GROUPS, STATIC_PCT = _schedule()
C = 4 * CHUNK_GROUPS
SIZES = sorted({1, 3, 4, 5, C - 1, C, C + 1, 7 * C + 2, 1000})


def run_edges(n, grid):
    """File indexes at which a wave's run starts or ends when n files are opened by `grid` waves:
    the fixed runs' ends, then the chunks' (the kernel's arithmetic)"""
    ngroups = (n + 3) // 4
    grid = min(grid or ngroups, ngroups)
    fixed = (ngroups // grid) * STATIC_PCT // 100
    dyn0 = fixed * grid
    e = {b * fixed for b in range(grid + 1)} | set(range(dyn0, ngroups, CHUNK_GROUPS))
    return sorted(4 * g for g in e if 0 < 4 * g < n)


@pytest.fixture(scope="module")
def ctx():
    c = crdtenc.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _no_cap_left_behind():
    yield
    set_cap(None)


# ---------------------------------------------------------------------------------- batches
class Batch:
    def __init__(self, key, actors, clears, fa, vers, rng):
        self.key, self.actors, self.clears, self.fa, self.vers = key, actors, clears, fa, list(vers)
        self.files = [W.seal(key, c, rng) for c in clears]
        self.n = len(clears)

    def expected(self, files=None, vers=None):
        oc = oracle.Core()
        rc, st = oc.read_remote_ops(self.key, [APP], files or self.files, [self.actors[i] for i in self.fa],
                                    vers or self.vers)
        return rc, list(st), oc.serialize()


def gcounter_batch(seed, runs, big=(), strangers=()):
    """Writer w's run is runs[w] files long.  Its maximum, 2^64 - 1 - w, is the last Dot of its
    run's first file (even w) or last file (odd w): still pending when that file ends, so it is
    folded by a later flush -- the next writer's first Dot or the wave's end.  Files are 120-400
    bytes of plaintext, those at the indexes in `big` 4085; a file at an index in `strangers`
    starts with a Dot of an actor that is not in the table."""
    rng = random.Random(seed)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(len(runs)))
    clears, fa, vers = [], [], []
    for w, r in enumerate(runs):
        for v in range(r):
            i = len(clears)
            ctr = W._counter_draw(rng)

            def draw():
                return W._dot(actors[w] if rng.random() < 0.8 else rng.choice(actors), ctr())
            last = [W._dot(actors[w], (1 << 64) - 1 - w)] if v == (0 if w % 2 == 0 else r - 1) else []
            first = [W._dot(rng.randbytes(16), rng.getrandbits(40))] if i in strangers else []
            clears.append(W._dots_clear(rng, BIG if i in big else rng.randrange(120, 400), first, draw, last))
            fa.append(w)
            vers.append(v)
    return Batch(key, actors, clears, fa, vers, rng)


def split_runs(n, bounds):
    b = [0] + sorted(x for x in set(bounds) if 0 < x < n) + [n]
    return [b[i + 1] - b[i] for i in range(len(b) - 1)]


@functools.lru_cache(maxsize=None)
def sized_batch(n):
    """n files of up to three writers, runs ending off the chunk edges; 4085-byte files on the first
    chunk's edge, on both sides of it, and at both ends of the batch"""
    b = gcounter_batch(1000 + n, split_runs(n, [n // 3 + 1, 2 * n // 3 + 2]), big={0, C - 1, C, n - 1})
    return b, b.expected()


def ingest(ctx, b, cap, files=None, vers=None, kind=crdtenc.STATE_GCOUNTER, key="open_v3_p0e1"):
    """-> (rc, statuses, state bytes, launches of the kernel) of one ingest into a fresh core; asserts
    that the kernel ran, that no other GCounter form did, and whether the grid was capped"""
    core = crdtenc.Core(ctx, kind=kind, supported=[APP], current_data_version=APP)
    core.set_latest_key(b.key)
    set_cap(cap)
    rc, st = core.ingest_ops(files or b.files, b.actors, b.fa, vers or b.vers)
    set_cap(None)
    state = core.state_bytes()
    launches = core.path_count(key)
    assert launches > 0, (key, cap, ctx.last_error())
    assert not any(core.path_count(k) for k in W.OPEN_KEYS if k != key), cap
    assert (core.path_count(W.CAPPED) > 0) == bool(cap and (b.n + 3) // 4 > cap), (cap, b.n)
    core.close()
    return rc, list(st), state, launches


def check(ctx, b, want, cap, **kw):
    rc, st, state, launches = ingest(ctx, b, cap, **kw)
    orc, ost, ostate = want
    where = (b.n, cap)
    assert rc == orc, (where, rc, orc, ctx.last_error())
    assert st == ost, (where, [(i, x, y) for i, (x, y) in enumerate(zip(st, ost)) if x != y][:10])
    assert state == ostate, where
    return launches


# ---------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("cap", CAPS)
def test_batch_sizes(ctx, cap):
    """1, 3, 4, 5, C - 1, C, C + 1, 7 C + 2 and 1,000 files: a batch smaller than one chunk (most
    waves of a capped grid draw an empty chunk at once), a partial last chunk, a last group of
    fewer than four files, more chunks than waves."""
    for n in SIZES:
        b, want = sized_batch(n)
        assert want[0] == 0
        check(ctx, b, want, cap)


# ---------------------------------------------------------------------------------- writer runs
@functools.lru_cache(maxsize=None)
def edge_batch(cap):
    """13 C + 3 files whose writers' runs start and end against the run edges of this grid: on an
    edge, one file before and one after, and in mid-chunk, each followed directly by the next
    writer; two runs span exactly the files between consecutive edges.  4085-byte files sit on
    both sides of three of the edges."""
    n = 13 * C + 3
    e = run_edges(n, cap)
    assert len(e) >= 3, (cap, e)
    pick = [e[i * (len(e) - 1) // 5] for i in range(6)]
    bounds = [pick[0], pick[1] - 1, pick[2] + 1, pick[3], pick[4] + C // 2 if C > 1 else pick[4], pick[5]]
    k = e.index(pick[3])
    bounds += e[k:k + 3]  # runs that are exactly the stretch between two edges
    big = {x + d for x in (pick[0], pick[2], pick[5]) for d in (-1, 0)}
    b = gcounter_batch(2000 + (cap or 0), split_runs(n, bounds), big=big)
    return b, b.expected()


@pytest.mark.parametrize("cap", CAPS)
def test_writer_runs_against_chunk_edges(ctx, cap):
    """A writer's maximum is pending when its run's last (or first) file ends; the wave that holds
    it goes on with a chunk elsewhere in the batch.  The pending (slot, max) must reach the batch
    state whichever chunk follows, and must not be credited to the writer met there."""
    b, want = edge_batch(cap)
    assert want[0] == 0
    check(ctx, b, want, cap)


# ---------------------------------------------------------------------------------- failures
def tampered(f):
    x = bytearray(f)
    x[-3] ^= 0x20  # a tag byte
    return bytes(x)


@functools.lru_cache(maxsize=None)
def failure_cases(cap):
    """[(what, index, files, versions, expected)]: one failing file per case, at the first and at
    the last file of a chunk of this grid and at the batch's last file; then one batch with two
    failures of different kinds, the earlier one in a later chunk's wave"""
    n = 9 * C + 2
    e = run_edges(n, cap)
    first_of, last_of = e[len(e) // 2], e[len(e) // 3] - 1
    b = gcounter_batch(3000 + (cap or 0), split_runs(n, [n // 4 + 1, n // 2 + 3, 3 * n // 4 + 2]))
    other_version = bytes(16 * [0x5a])
    out = []
    for at in (first_of, last_of, n - 1):
        files = list(b.files)
        files[at] = tampered(files[at])
        out.append(("tag", at, files, None, b.expected(files=files)))
        files = list(b.files)
        files[at] = W.seal(b.key, other_version + b.clears[at][16:], random.Random(at))
        out.append(("data version", at, files, None, b.expected(files=files)))
        # the writer's version before this file is missing: this and its later files are one too high
        vers = [v + 1 if b.fa[i] == b.fa[at] and i >= at else v for i, v in enumerate(b.vers)]
        out.append(("gap", at, None, vers, b.expected(vers=vers)))
    files = list(b.files)
    files[last_of] = W.seal(b.key, other_version + b.clears[last_of][16:], random.Random(7))
    files[n - 1] = tampered(files[n - 1])
    files[first_of] = tampered(files[first_of]) if first_of > last_of else files[first_of]
    out.append(("two kinds", last_of, files, None, b.expected(files=files)))
    return b, out


@pytest.mark.parametrize("cap", CAPS)
def test_failures_at_chunk_edges(ctx, cap):
    """A tampered tag (CE_ERR_AUTH), an unsupported data version (CE_ERR_PT_VERSION) and a version
    gap (CE_ERR_OP_VERSION) on a chunk's first file, on a chunk's last file and on the batch's
    last: the per-file statuses, the first failing index and the call's status are the oracle's,
    and a rejected batch leaves the state as it was."""
    b, cases = failure_cases(cap)
    empty = oracle.Core().serialize()
    for what, at, files, vers, want in cases:
        orc, ost, ostate = want
        assert orc == {"tag": 9, "data version": 11, "gap": 13, "two kinds": 11}[what], (what, at, orc)
        rc, st, state, _ = ingest(ctx, b, cap, files=files, vers=vers)
        where = (what, at, cap)
        assert rc == orc, (where, rc, ctx.last_error())
        assert st == ost, (where, [(i, x, y) for i, (x, y) in enumerate(zip(st, ost)) if x != y][:10])
        assert next(i for i, s in enumerate(st) if s) == at and st[at] == orc, where
        if what != "gap":  # (the files before a gap are applied: lib.rs:519-538)
            assert state == empty, where
        assert state == ostate, where


# ---------------------------------------------------------------------------------- refold
def test_refold_after_actor_misses(ctx):
    """Five files name an actor that is not in the table (first and last files of chunks among
    them), at cap 3: the first launch lists the misses, the host inserts the actors and the kernel
    runs again over the marked files with the same counter block.  Its waves must draw their
    chunks from zero: with the ticket where the first launch left it, past the end of the batch,
    they would take their fixed runs only, and the Dots of the missed files in the drawn part of
    the batch (those at chunk edges and the batch's last file) would be lost."""
    n = 11 * C + 1
    e = run_edges(n, 3)
    strangers = {e[1], e[2] - 1, e[len(e) // 2] + 1, n - 1, 2}
    b = gcounter_batch(4000, split_runs(n, [n // 3, 2 * n // 3 + 1]), strangers=strangers, big={e[1]})
    want = b.expected()
    assert want[0] == 0
    assert check(ctx, b, want, 3) >= 2


# ---------------------------------------------------------------------------------- other forms
@functools.lru_cache(maxsize=None)
def pn_batch():
    rng = random.Random(5000)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(3))
    n = 7 * C + 2
    runs = split_runs(n, [n // 3 + 1, 2 * n // 3 - 1])
    files, fa, vers = [], [], []
    for w, r in enumerate(runs):
        for v in range(r):
            k = 78 if len(files) in (0, C - 1, C, n - 1) else rng.randrange(1, 8)  # 78 or 79 ops: the last page
            ops = [((actors[w] if rng.random() < 0.8 else rng.choice(actors), rng.randrange(1 << 16, 1 << 31)),
                    rng.choice(pm.DIRS)) for _ in range(k)]
            if v in (0, r - 1):  # the writer's maxima of both planes at its run's two ends, last in the file
                ops.append(((actors[w], (1 << 32) - 1 - w), pm.DIRS[(w + (v != 0)) % 2]))
            files.append(W.seal(key, APP + pm.enc_ops(ops), rng))
            fa.append(w)
            vers.append(v)
    oc = pm.Core()
    rc, st = oc.read_remote_ops(key, [APP], files, [actors[i] for i in fa], vers)
    return key, actors, files, fa, vers, (rc, list(st), oc.serialize())


@functools.lru_cache(maxsize=None)
def gset_batch():
    rng = random.Random(6000)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(3))
    n = 7 * C + 2
    runs = split_runs(n, [n // 3 + 1, 2 * n // 3 - 1])
    files, fa, vers = [], [], []
    for w, r in enumerate(runs):
        for v in range(r):
            k = 453 if len(files) in (0, C - 1, C, n - 1) else rng.randrange(0, 30)  # 453 cf members: a full page
            ms = [rng.getrandbits(64) | (1 << 63) for _ in range(k)] if k == 453 else \
                 [rng.getrandbits(rng.choice([6, 8, 16, 32, 64])) for _ in range(k)]
            files.append(W.seal(key, APP + gm.enc_ops(ms), rng))
            fa.append(w)
            vers.append(v)
    oc = gm.Core()
    rc, st = oc.read_remote_ops(key, [APP], files, [actors[i] for i in fa], vers)
    return key, actors, files, fa, vers, (rc, list(st), oc.serialize())


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("form", ["pncounter", "gset"])
def test_other_forms(ctx, form, cap):
    """k_open_fold_v3<false, true, true> (PNCounter) and <false, true, false, true> (GSet) share
    the loop: 7 C + 2 files each, full pages on the first chunk's edge and at the batch's ends."""
    key, actors, files, fa, vers, want = pn_batch() if form == "pncounter" else gset_batch()
    kind, path = (crdtenc.STATE_PNCOUNTER, "open_v3_pn") if form == "pncounter" else (crdtenc.STATE_GSET, "open_v3_gset")
    assert want[0] == 0
    core = crdtenc.Core(ctx, kind=kind, supported=[APP], current_data_version=APP)
    core.set_latest_key(key)
    set_cap(cap)
    rc, st = core.ingest_ops(files, actors, fa, vers)
    set_cap(None)
    assert (rc, list(st)) == want[:2], (form, cap, ctx.last_error())
    assert core.state_bytes() == want[2], (form, cap)
    assert core.path_count(path) > 0 and not any(core.path_count(k) for k in W.OPEN_KEYS if k != path)
    assert (core.path_count(W.CAPPED) > 0) == bool(cap)
    core.close()


# ---------------------------------------------------------------------------------- repeatability
def test_same_bytes_every_time(ctx):
    """The 1,000-file batch into five fresh cores at the product's grid: which wave takes which chunk
    differs from run to run, the statuses and the state bytes must not."""
    b, want = sized_batch(1000)
    got = [ingest(ctx, b, None)[:3] for _ in range(5)]
    assert all(g == got[0] for g in got)
    assert got[0] == want


# ---------------------------------------------------------------------------------- stamps
def test_wave_stamps(ctx, monkeypatch):
    """CE_TEST_WAVE_STAMPS=1 (read per ingest) and ce_ctx_wave_stamps: one row per wave of the
    launch, capped or not; every wave left its loop no earlier than it entered it, all within the
    second the ingest took; the hardware id words are not all alike (the waves of an uncapped
    grid sit in different places); the schedule word is this file's C and STATIC_PCT.  The results
    are the oracle's with the stamps on; an ingest that takes another open kernel (CE_FUSED=1), or
    one without the variable, leaves none to read."""
    b, want = sized_batch(1000)
    monkeypatch.setenv("CE_TEST_WAVE_STAMPS", "1")
    for cap, waves in ((None, 250), (7, 7)):
        check(ctx, b, want, cap)
        st = ctx.wave_stamps()
        assert st.shape == (waves, 4), (cap, st.shape)
        t_in, t_out = st[:, 0].astype("int64"), st[:, 1].astype("int64")
        assert (t_in > 0).all() and (t_out >= t_in).all(), cap
        assert int(t_out.max() - t_in.min()) < 100_000_000, cap
        assert (st[:, 2] != 0).all(), cap
        assert (st[:, 3] == (CHUNK_GROUPS | (STATIC_PCT << 32))).all(), (cap, hex(int(st[0, 3])))
        if cap is None:
            assert len(set(st[:, 2].tolist())) > 1
    # an ingest that opens its files with another kernel leaves none to read, not the rows above
    monkeypatch.setenv("CE_FUSED", "1")
    monkeypatch.setenv("CE_FILES_PER_WAVE", "4")
    check(ctx, b, want, None, key="open_small_lpf16")
    assert ctx.wave_stamps().shape == (0, 4)
    monkeypatch.delenv("CE_FUSED")
    monkeypatch.delenv("CE_FILES_PER_WAVE")
    check(ctx, b, want, 7)
    assert ctx.wave_stamps().shape == (7, 4)
    monkeypatch.delenv("CE_TEST_WAVE_STAMPS")
    check(ctx, b, want, None)
    assert ctx.wave_stamps().shape == (0, 4)
