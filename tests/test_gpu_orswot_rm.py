"""GPU parity of ce_core_orswot_rm_members[_device] (include/crdtenc.h) against
tests/orswot_rm_model.py: with fixed nonces the written files, their offsets, the op and file
counts and the bytes are compared byte for byte, state_bytes() with oracle.crdts.Core after the
same ops (which also proves the version bump and the unchanged clock), the sizing call with the
same figures, and a fresh core that ingests the written files reaches the same state on the
device's decoders.  Without the two entry points every test here fails on the missing symbols."""
import ctypes
import itertools
import os
import random

import numpy as np
import pytest
import torch

import crdtenc
import orswot_rm_model as rm
from oracle import crdts as C

pytestmark = pytest.mark.gpu
APP = rm.APP
ORSWOT = crdtenc.STATE_ORSWOT
DEV = "cuda:0"
U64 = rm.U64
LIVE = rm.LIVE_ONLY
INVALID, NO_KEY = 64, 66
GUARD = 64          # bytes / words past every output's bound that must stay as they were
FILL = 0xAB
COUNTERS = (1, 200, 60000, 1 << 31, 1 << 40)        # one of every counter width
WIDE = [0, U64, 5, 200, 60000, 1 << 31, 1 << 40]    # members of every width, and the two sentinels
ABSENT = {1: 90, 2: 201, 3: 50000, 5: 1 << 20, 9: 1 << 50}     # by encoded width; never added
KEYS = ("files", "ops", "entries")


def M(k):
    """the member that k writers added: a clock of k entries"""
    return 1000 + k


@pytest.fixture(scope="module")
def ctx():
    c = crdtenc.Context(0)
    yield c
    c.close()


def new_core(ctx, key, kind=ORSWOT, **kw):
    c = crdtenc.Core(ctx, kind=kind, supported=[APP], current_data_version=APP, **kw)
    if key is not None:
        c.set_latest_key(key)
    return c


def u64_dev(values):
    t = torch.from_numpy(np.asarray(values, np.uint64).view(np.int64).copy()).to(DEV)
    torch.cuda.synchronize()
    return t


def uuid_str(u):
    h = u.hex()
    return "%s-%s-%s-%s-%s" % (h[:8], h[8:12], h[12:16], h[16:20], h[20:])


class Written:
    """a core, its oracle, and every file the local actor wrote so far (versions 0, 1, ...)"""

    def __init__(self, ctx, oracle, key, rng, **kw):
        self.ctx, self.oracle, self.key, self.rng = ctx, oracle, key, rng
        self.core, self.oc = new_core(ctx, key, **kw), C.Core("orswot")
        self.actor = self.core.info_actor()
        self.files = []
        self.before = []            # (files, actors, file_actor, versions) ingested from other writers

    def counts(self):
        return [self.core.path_count("orswot_rm_device_" + k) for k in KEYS]

    def model_apply(self, vectors):
        for vec in vectors:
            for op in vec:
                self.oc.state.apply(op)
            self.oc.nov.apply(self.actor, self.oc.nov.get(self.actor) + 1)

    def seal(self, ops_lists):
        return [crdtenc.CORE_VERSION + e
                for e in self.ctx.encrypt_batch(self.key, [APP + C.enc_orswot_ops(o) for o in ops_lists])]

    def ingest(self, ops_lists, actors, fa, fv):
        files = self.seal(ops_lists)
        rc, st = self.core.ingest_ops(files, actors, fa, fv)
        orc, ost = self.oc.read_remote_ops(self.key, [APP], files, [actors[i] for i in fa], fv)
        assert (rc, st) == (orc, ost) and rc == 0
        assert self.core.state_bytes() == self.oc.serialize()
        self.before.append((files, actors, fa, fv))

    def writers(self, n=17):
        """n writers, writer i adding M(k) for every k > i under a counter of width i % 5: M(k)
        carries k dots.  Random UUIDs: their byte order is neither the order they are inserted in
        nor the order of their stable ids.  Then the members of every width under one more dot,
        2000 added and removed again, and a removal by an unknown writer that stays deferred."""
        actors = [self.rng.randbytes(16) for _ in range(n)]
        assert actors != sorted(actors)
        self.ingest([[("Add", (a, COUNTERS[i % 5]), [M(k) for k in range(i + 1, n + 1)])] for i, a in enumerate(actors)],
                    actors, list(range(n)), [0] * n)
        b, ghost = self.rng.randbytes(16), self.rng.randbytes(16)
        self.ingest([[("Add", (b, 3), WIDE + [2000])], [("Rm", C.VClock({b: 3}), [2000]),
                                                        ("Rm", C.VClock({ghost: 9}), [M(n), 77])]], [b], [0, 0], [0, 1])
        assert 2000 not in self.oc.state.entries and len(self.oc.state.deferred) == 1
        assert [len(self.oc.state.entries[M(k)].dots) for k in range(1, n + 1)] == list(range(1, n + 1))
        return actors

    def remove(self, col, opf=0, flags=0, host=False):
        """one call over col, checked against the model; returns the files it wrote"""
        core = self.core
        vectors = rm.cut(col, opf, self.oc.state, flags)
        n_ops, nf, nbytes = rm.sizes(vectors)
        entries = sum(len(op[1].dots) for v in vectors for op in v)
        nonces = [self.rng.randbytes(24) for _ in range(nf)]
        want = rm.files(self.oracle, self.key, nonces, vectors)
        offs = rm.offsets(want)
        assert offs[-1] == nbytes
        counts, state = self.counts(), core.state_bytes()
        if host:
            rc, got = core.orswot_rm_members(col, opf, flags, nonces)
            assert rc == 0, core.ctx.last_error()
            assert got == want
        else:
            members = u64_dev(col)
            ptr = members.data_ptr() if len(col) else None
            # the sizing call: the same three figures, nothing changed
            assert core.orswot_rm_members_device(ptr, len(col), None, 0, None, opf, flags) == (0, n_ops, nf, nbytes)
            assert core.state_bytes() == state and self.counts() == counts
            d_files = torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device=DEV)
            d_offs = torch.full((nf + 1 + GUARD,), -1, dtype=torch.int64, device=DEV)
            torch.cuda.synchronize()
            got = core.orswot_rm_members_device(ptr, len(col), d_files.data_ptr(), nbytes, d_offs.data_ptr(), opf, flags,
                                                nonces)
            assert got[0] == 0, core.ctx.last_error()
            assert got[1:] == (n_ops, nf, nbytes)
            out, o = d_files.cpu().numpy(), d_offs.cpu().numpy()
            assert [int(x) for x in o[:nf + 1]] == offs
            assert bool((o[nf + 1:] == -1).all())               # no word past the F + 1 offsets
            assert out[:nbytes].tobytes() == b"".join(want)
            assert bool((out[nbytes:] == FILL).all())           # no byte past the files
            assert [int(x) for x in members.cpu().numpy().view(np.uint64)] == list(col)   # the column is read only
        clock = dict(self.oc.state.clock.dots)
        self.model_apply(vectors)
        assert self.oc.state.clock.dots == clock
        assert core.state_bytes() == self.oc.serialize()
        assert [a - b for a, b in zip(self.counts(), counts)] == [nf, n_ops, entries]
        self.files += want
        return want

    def check_readers(self):
        """a fresh core that ingests what this one ingested and then every file it wrote: the same
        state, status 0 for every file, none left to the host op decoder"""
        reader = new_core(self.ctx, self.key)
        for files, actors, fa, fv in self.before:
            assert reader.ingest_ops(files, actors, fa, fv)[0] == 0
        n = len(self.files)
        rc, st = reader.ingest_ops(self.files, [self.actor], [0] * n, list(range(n)))
        assert rc == 0 and st == [0] * n, reader.ctx.last_error()
        assert reader.state_bytes() == self.oc.serialize() == self.core.state_bytes()
        assert reader.path_count("ds_host_decode_files") == 0
        reader.close()

    def close(self):
        self.core.close()


def started(ctx, oracle, seed, **kw):
    rng = random.Random(seed)
    w = Written(ctx, oracle, rng.randbytes(32), rng, **kw)
    w.writers()
    return w


# ------------------------------------------------------------------ clocks, counters, members
@pytest.mark.parametrize("flags", [0, LIVE])
def test_clock_sizes_member_widths_and_states(ctx, oracle, flags):
    """clocks of 0, 1, 2, 15, 16 and 17 entries in one column (the map16 edge) under counters of
    all five widths; members of all five widths, 0 and 2^64 - 1; absent members, one added then
    removed, one repeated next to itself and far apart"""
    w = started(ctx, oracle, 1 + flags)
    col = [ABSENT[1], M(1), M(2), M(15), M(16), M(17), M(17), 2000] + WIDE + list(ABSENT.values()) + [M(9), 0, M(17), M(2)]
    got = w.remove(col, 0, flags)
    assert len(got) == (1 if flags else 2)
    assert all(m not in w.oc.state.entries for m in col) and len(w.oc.state.deferred) == 1
    w.remove(col, 3, flags)                 # everything is gone: empty clocks, or nothing under the flag
    w.check_readers()
    w.close()


@pytest.mark.parametrize("opf", [0, 1, 15, 16, 17])
def test_ops_per_file_headers(ctx, oracle, opf):
    """n = 0, 1, around a file and a short last file; the Vec's fixarray / array16 header at 15 / 16
    ops; all absent under the flag writes nothing"""
    w = started(ctx, oracle, 10 + opf)
    k = opf or 16
    pool = [M(i) for i in range(1, 18)] + WIDE + list(ABSENT.values()) + [2000, 77]
    for n in sorted({0, 1, k - 1, k, k + 1, 2 * k + 1}):
        col = [pool[(7 * i + n) % len(pool)] for i in range(n)]
        assert len(w.remove(col, opf, 0)) == -(-n // k)
    assert w.remove(list(ABSENT.values()) + [2000, 77], opf, LIVE) == []
    assert w.remove([], opf, LIVE) == []
    w.check_readers()
    w.close()


# ------------------------------------------------------------------ file lengths at their edges
def column_of_length(st, target):
    """a column whose one file (every op in it) has exactly `target` bytes of clear text"""
    def length(col):
        return rm.file_len(rm.cut(col, len(col), st)[0])
    if target < 1000:
        for k in range(18):
            for r in range(5):
                for fill in itertools.combinations_with_replacement(sorted(ABSENT), r):
                    col = ([M(k)] if k else []) + [ABSENT[x] for x in fill]
                    if col and length(col) == target:
                        return col
        raise AssertionError(target)
    big = rm.op_len(st.entries[M(17)], M(17))
    nbig = (target - 19 - 900) // big
    rest = target - 19 - nbig * big
    y = rest % 28                           # absent members of one and two bytes: ops of 28 and 29
    x = (rest - 29 * y) // 28
    assert x >= 0 and nbig + x + y > 15
    col = [M(17)] * nbig + [ABSENT[1]] * x + [ABSENT[2]] * y
    assert length(col) == target
    return col


# clear-text lengths on both sides of: the envelope's two bin8 -> bin16 edges, one page, the two
# bin16 -> bin32 edges
EDGES = [(195, 196, 239, 240), (4095, 4096, 4097), (65474, 65475), (65519, 65520)]


@pytest.mark.parametrize("targets", EDGES)
def test_file_lengths_at_the_envelope_and_page_edges(ctx, oracle, targets):
    w = started(ctx, oracle, 20 + len(targets))
    sealed = []
    for t in targets:
        col = column_of_length(w.oc.state, t)
        vec = rm.cut(col, len(col), w.oc.state)
        assert len(vec) == 1 and rm.file_len(vec[0]) == t       # the model lands where the edge needs it
        sealed.append(16 + rm.sealed_len(t) - t)
        # the repeats of M(17) keep their clock: every clock is read before anything changes
        got = w.remove(col, len(col), 0)
        assert len(got) == 1
        # the removed members come back for the next length
        w.ingest([[("Add", (w.before[0][1][i], (1 << 41) + t), [M(k) for k in range(i + 1, 18)])] for i in range(17)],
                 w.before[0][1], list(range(17)), [len(w.before) - 1] * 17)
    assert len(set(sealed)) > 1 or 4096 in targets              # the envelope changed form inside the set
    w.check_readers()
    w.close()


# ------------------------------------------------------------------ grids
@pytest.mark.parametrize("cap", ["1", "7"])
def test_clamped_grids_take_several_trips(ctx, oracle, monkeypatch, cap):
    """a few thousand members over grids clamped to one block and to seven (an uneven last trip)"""
    w = started(ctx, oracle, 30)
    rng = w.rng
    extra = [(1 << 33) + i for i in range(1500)]
    a = [rng.randbytes(16) for _ in range(3)]
    w.ingest([[("Add", (x, 5 + i), extra[i * 300:i * 300 + 900])] for i, x in enumerate(a)], a, [0, 1, 2], [0, 0, 0])
    pool = extra + [M(k) for k in range(1, 18)] + list(ABSENT.values())
    col = [pool[rng.randrange(len(pool))] for _ in range(3000)]
    monkeypatch.setenv("CE_TEST_GRID_CAP", cap)
    assert len(w.remove(col, 0, 0)) == -(-3000 // 16)
    monkeypatch.delenv("CE_TEST_GRID_CAP")
    w.check_readers()
    w.close()


def test_live_only_over_a_long_column(ctx, oracle):
    w = started(ctx, oracle, 31)
    rng = w.rng
    extra = [(1 << 33) + i for i in range(1000)]
    a = rng.randbytes(16)
    w.ingest([[("Add", (a, 1 << 20), extra)]], [a], [0], [0])
    pool = extra + [M(k) for k in range(1, 18)] + list(ABSENT.values()) + [2000]
    col = [pool[rng.randrange(len(pool))] for _ in range(2500)]
    got = w.remove(col, 17, LIVE)
    assert 0 < len(got) < -(-2500 // 17)
    w.check_readers()
    w.close()


# ------------------------------------------------------------------ state preconditions
def test_after_an_ingest_that_grew_the_actor_table_and_after_an_add(ctx, oracle):
    """the rank tables follow the actor table as it stands at the call; the add writer's flags for
    its sort-free fold are not inherited; the deferred removal stays deferred throughout"""
    w = started(ctx, oracle, 40)
    w.remove([M(3), M(17)], 0, 0)
    newer = sorted((w.rng.randbytes(16) for _ in range(40)), reverse=True)
    w.ingest([[("Add", (x, 7 + i), [M(17), 4242])] for i, x in enumerate(newer)], newer, list(range(40)), [0] * 40)
    w.remove([4242, M(17), M(5)], 0, 0)
    # the add writer, then a removal of what it added together with older members
    d_files = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    d_offs = torch.zeros(64, dtype=torch.int64, device=DEV)
    col = [70001, 70002, M(8)]
    c0 = w.oc.state.clock.get(w.actor)
    added = u64_dev(col)
    rc, nf, nb = w.core.orswot_add_members_device(added.data_ptr(), 3, d_files.data_ptr(), 1 << 16, d_offs.data_ptr(),
                                                  1, 0, 0, [bytes(24)])
    assert rc == 0 and nf == 1
    w.files.append(d_files.cpu().numpy()[:nb].tobytes())
    w.model_apply([[("Add", (w.actor, c0 + 1 + j), [m]) for j, m in enumerate(col)]])
    assert w.core.state_bytes() == w.oc.serialize()
    w.remove([70002, M(8), 70001, M(9), 70002], 2, 0)
    assert len(w.oc.state.deferred) == 1
    w.check_readers()
    w.close()


# ------------------------------------------------------------------ twins, storage
def test_same_effect_as_the_batch_route(ctx, oracle, tmp_path):
    """a twin (the same actor: one local directory) reads the clocks with orswot_member_clocks,
    encodes on the host and runs apply_ops_batch with the same nonces: the same files, the same
    state"""
    rng = random.Random(50)
    key = rng.randbytes(32)
    kw = dict(local_path=str(tmp_path / "l"), flags=crdtenc.OPEN_CREATE)
    a = Written(ctx, oracle, key, random.Random(51), remote_path=str(tmp_path / "r1"), **kw)
    b = Written(ctx, oracle, key, random.Random(51), remote_path=str(tmp_path / "r2"), **kw)
    assert a.actor == b.actor
    a.writers()
    b.writers()
    for col, opf in (([M(17), ABSENT[3], M(1), M(17), 0, U64, 2000, M(16)], 3), ([M(k) for k in range(2, 16)], 0)):
        clocks = b.core.orswot_member_clocks(col)
        ops = [("Rm", C.VClock(dict(cl)), [m]) for m, cl in zip(col, clocks)]
        k = opf or 16
        vectors = [ops[i:i + k] for i in range(0, len(ops), k)]
        nonces = [random.Random(52 + i).randbytes(24) for i in range(len(vectors))]
        want = rm.cut(col, opf, a.oc.state)
        assert [[(o[1].dots, o[2]) for o in v] for v in vectors] == [[(o[1].dots, o[2]) for o in v] for v in want]
        rc, fs = b.core.apply_ops_batch([C.enc_orswot_ops(v) for v in vectors], nonces)
        assert rc == 0
        members = u64_dev(col)
        _, n_ops, nf, nbytes = a.core.orswot_rm_members_device(members.data_ptr(), len(col), None, 0, None, opf, 0)
        d_files = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
        d_offs = torch.zeros(nf + 1, dtype=torch.int64, device=DEV)
        got = a.core.orswot_rm_members_device(members.data_ptr(), len(col), d_files.data_ptr(), nbytes, d_offs.data_ptr(), opf,
                                              0, nonces)
        assert got == (0, len(col), len(vectors), sum(len(f) for f in fs))
        assert d_files.cpu().numpy().tobytes() == b"".join(fs)
        assert a.core.state_bytes() == b.core.state_bytes()
        a.model_apply(want)
        assert a.core.state_bytes() == a.oc.serialize()
    a.close()
    b.close()


def test_host_twin_and_storage(ctx, oracle, tmp_path):
    """the host twin returns the device call's bytes; with storage the files sit at
    ops/<actor>/<v0 + i>"""
    rng = random.Random(60)
    remote = str(tmp_path / "remote")
    w = Written(ctx, oracle, rng.randbytes(32), rng, local_path=str(tmp_path / "l1"), remote_path=remote,
                flags=crdtenc.OPEN_CREATE)
    w.writers()
    w.remove([M(17), M(2), ABSENT[5], M(17)], 3, 0)
    w.remove([M(4), M(16), 0, U64, M(4), ABSENT[1], 2000], 2, LIVE, host=True)
    w.remove([M(5), M(6), 77], 0, 0, host=True)
    assert w.remove([], 0, 0, host=True) == []
    d = os.path.join(remote, "ops", uuid_str(w.actor))
    assert sorted(os.listdir(d), key=int) == [str(i) for i in range(len(w.files))] and len(w.files) == 5
    for i, f in enumerate(w.files):
        assert open(os.path.join(d, str(i)), "rb").read() == f
    w.check_readers()
    w.close()


# ------------------------------------------------------------------ refusals
def test_refusals_touch_nothing(ctx, oracle, tmp_path):
    """a wrong kind (GSet, MVReg), an unknown flag, ops_per_file 65,536, n at 2^32, cap one byte
    short, no key: each returns its code and leaves state_bytes(), the storage tree, the path
    counts and every output as they were"""
    rng = random.Random(70)
    key = rng.randbytes(32)
    remote = str(tmp_path / "remote")
    w = Written(ctx, oracle, key, rng, local_path=str(tmp_path / "l1"), remote_path=remote, flags=crdtenc.OPEN_CREATE)
    w.writers()
    gs = new_core(ctx, key, kind=crdtenc.STATE_GSET)
    mv = new_core(ctx, key, kind=crdtenc.STATE_MVREG)
    nokey = new_core(ctx, None, local_path=str(tmp_path / "l2"), remote_path=remote, flags=crdtenc.OPEN_CREATE)
    col = [M(17), M(3), 0, U64, ABSENT[9], M(17)]
    n = len(col)
    members = u64_dev(col)
    n_ops, nf, nbytes = rm.sizes(rm.cut(col, 2, w.oc.state))
    cases = [(gs, n, 2, 0, nbytes, INVALID), (mv, n, 2, 0, nbytes, INVALID), (w.core, n, 2, 2, nbytes, INVALID),
             (w.core, n, 2, 0x80000000, nbytes, INVALID), (w.core, n, 65536, 0, nbytes, INVALID),
             (w.core, 1 << 32, 2, 0, 1 << 62, INVALID), (w.core, n, 2, 0, nbytes - 1, INVALID),
             (nokey, n, 2, 0, nbytes, NO_KEY)]

    def tree():
        return sorted((p, tuple(sorted(fs))) for p, _, fs in os.walk(str(tmp_path)))
    cores = (w.core, gs, mv, nokey)
    before = {c: c.state_bytes() for c in cores}
    disk, counts = tree(), w.counts()
    nonces = ctypes.create_string_buffer(b"\x55" * (24 * nf))
    for core, cnt, opf, flags, cap, code in cases:
        d_files = torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device=DEV)
        d_offs = torch.full((nf + 1 + GUARD,), -1, dtype=torch.int64, device=DEV)
        torch.cuda.synchronize()
        no, nfo, nb = ctypes.c_uint64(0xDEADBEEF), ctypes.c_uint32(0xDEADBEEF), ctypes.c_uint64(0xDEADBEEFDEADBEEF)
        rc = crdtenc.lib().ce_core_orswot_rm_members_device(
            core.p, ctypes.c_void_p(members.data_ptr()), ctypes.c_uint64(cnt), ctypes.c_uint32(opf), ctypes.c_uint32(flags),
            nonces, ctypes.c_void_p(d_files.data_ptr()), ctypes.c_uint64(cap), ctypes.c_void_p(d_offs.data_ptr()),
            ctypes.byref(no), ctypes.byref(nfo), ctypes.byref(nb))
        assert rc == code, (rc, code, cnt, opf, flags, cap)
        assert (no.value, nfo.value, nb.value) == (0xDEADBEEF, 0xDEADBEEF, 0xDEADBEEFDEADBEEF)
        assert bool((d_files == FILL).all()) and bool((d_offs == -1).all())
        assert core.state_bytes() == before[core] and tree() == disk and w.counts() == counts
        if cap >= nbytes and cnt == n:          # the host twin refuses the same arguments (it has no cap)
            assert core.orswot_rm_members(col, opf, flags, [b"\x55" * 24] * nf) == (code, None)
            assert core.state_bytes() == before[core] and tree() == disk
    # the writer still writes its next versions after all of them
    got = w.remove(col, 2, 0)
    assert len(got) == 3 and os.path.exists(os.path.join(remote, "ops", uuid_str(w.actor), "2"))
    for c in (gs, mv, nokey):
        c.close()
    w.close()
