"""GPU parity of ce_core_orswot_add_members[_device] (include/crdtenc.h) against
tests/orswot_write_model.py: with fixed nonces the written files, their offsets, their count and
their bytes are compared byte for byte, state_bytes() with oracle.crdts.Core after the same ops
(which also proves the version bump), and a fresh core that ingests the written files reaches the
same state on the device's decoders.  Without the three entry points every test here fails on the
missing symbols."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import crdtenc
import dotset_gen as G
import orswot_write_model as wm
from oracle import crdts as C

pytestmark = pytest.mark.gpu
APP = wm.APP
ORSWOT = crdtenc.STATE_ORSWOT
DEV = "cuda:0"
U64 = wm.U64
INVALID, NO_KEY = 64, 66
GUARD = 64          # bytes / words past every output's bound that must stay as they were
FILL = 0xAB


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


def mixed(rng, n):
    return [wm.member_of_width(rng, wm.WIDTH_BYTES[i % 5]) for i in range(n)]


class Written:
    """a core, its oracle, and every file the local actor wrote so far (versions 0, 1, ...)"""

    def __init__(self, ctx, oracle, key, rng, **kw):
        self.ctx, self.oracle, self.key, self.rng = ctx, oracle, key, rng
        self.core, self.oc = new_core(ctx, key, **kw), C.Core("orswot")
        self.actor = self.core.info_actor()
        self.files = []
        self.fusable = True         # every own file so far: one-member ops, at most 28 a file
        self.before = []            # (files, actors, file_actor, versions) ingested from other writers

    def c0(self):
        return self.oc.state.clock.get(self.actor)

    def model_apply(self, vectors):
        for vec in vectors:
            for op in vec:
                self.oc.state.apply(op)
            self.oc.nov.apply(self.actor, self.oc.nov.get(self.actor) + 1)

    def local(self, ops):
        """one host apply_ops of `ops` by the core (its file kept for the readers)"""
        rc, fs = self.core.apply_ops_batch([C.enc_orswot_ops(ops)], [self.rng.randbytes(24)])
        assert rc == 0, self.core.ctx.last_error()
        self.model_apply([ops])
        assert self.core.state_bytes() == self.oc.serialize()
        self.files += fs
        self.fusable = self.fusable and all(op[0] == "Add" and len(op[2]) == 1 for op in ops) and len(ops) <= 28

    def ingest(self, files, actors, fa, fv):
        rc, st = self.core.ingest_ops(files, actors, fa, fv)
        orc, ost = self.oc.read_remote_ops(self.key, [APP], files, [actors[i] for i in fa], fv)
        assert (rc, st) == (orc, ost) and rc == 0
        assert self.core.state_bytes() == self.oc.serialize()
        self.before.append((files, actors, fa, fv))

    def add(self, col, per_op=0, opf=0, host=False):
        """one call over col, checked against the model; returns the files it wrote"""
        core = self.core
        vectors = wm.cut(col, per_op, opf, self.c0(), self.actor)
        rc, max_ops, max_files, max_bytes = crdtenc.orswot_add_bound(len(col), per_op, opf)
        assert rc == 0 and (max_ops, max_files, max_bytes) == wm.bound(len(col), per_op, opf)
        nonces = [self.rng.randbytes(24) for _ in range(max_files)]
        want = wm.files(self.oracle, self.key, nonces, vectors)
        offs = wm.offsets(want)
        assert len(want) == max_files and offs[-1] <= max_bytes
        counts = [core.path_count("orswot_add_device_" + k) for k in ("files", "ops", "members")]
        if host:
            rc, got = core.orswot_add_members(col, per_op, opf, 0, nonces)
            assert rc == 0, core.ctx.last_error()
            assert got == want
        else:
            members = u64_dev(col)
            d_files = torch.full((max_bytes + GUARD,), FILL, dtype=torch.uint8, device=DEV)
            d_offs = torch.full((max_files + 1 + GUARD,), -1, dtype=torch.int64, device=DEV)
            torch.cuda.synchronize()
            rc, nf, nb = core.orswot_add_members_device(members.data_ptr() if len(col) else None, len(col),
                                                        d_files.data_ptr(), max_bytes, d_offs.data_ptr(), per_op, opf,
                                                        0, nonces)
            assert rc == 0, core.ctx.last_error()
            assert (nf, nb) == (len(want), offs[-1])
            out, o = d_files.cpu().numpy(), d_offs.cpu().numpy()
            assert [int(x) for x in o[:nf + 1]] == offs
            assert bool((o[nf + 1:] == -1).all())               # no word past the F + 1 offsets
            assert out[:nb].tobytes() == b"".join(want)
            assert bool((out[nb:] == FILL).all())               # no byte past the files
            assert [int(x) for x in members.cpu().numpy().view(np.uint64)] == list(col)   # the column is read only
        self.model_apply(vectors)
        assert core.state_bytes() == self.oc.serialize()
        after = [core.path_count("orswot_add_device_" + k) for k in ("files", "ops", "members")]
        assert [a - b for a, b in zip(after, counts)] == [len(vectors), sum(len(v) for v in vectors), len(col)]
        po, k = wm.shape(per_op, opf)
        if vectors:
            self.fusable = self.fusable and po == 1 and k <= 28
        self.files += want
        return want

    def check_readers(self):
        """a fresh core that ingests what this one ingested and then every file it wrote: the same
        state, no file left to the host parser, and every one-member file of at most 28 ops decoded
        inside the fused open"""
        reader = new_core(self.ctx, self.key)
        for files, actors, fa, fv in self.before:
            assert reader.ingest_ops(files, actors, fa, fv)[0] == 0
        fused0 = reader.path_count("ds_fused_files")
        n = len(self.files)
        rc, st = reader.ingest_ops(self.files, [self.actor], [0] * n, list(range(n)))
        assert rc == 0 and st == [0] * n, reader.ctx.last_error()
        assert reader.state_bytes() == self.oc.serialize() == self.core.state_bytes()
        assert reader.path_count("ds_host_decode_files") == 0
        if self.fusable:
            assert reader.path_count("ds_fused_files") - fused0 == n
        reader.close()

    def close(self):
        self.core.close()


def columns(rng, n):
    """n members of each width, and of all five alternating"""
    return [[wm.member_of_width(rng, w) for _ in range(n)] for w in wm.WIDTH_BYTES] + [mixed(rng, n)]


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize("opf", [1, 15, 16, 17, 28, 58])
def test_ops_per_file_headers(ctx, oracle, opf):
    """one member an op; n around a file (0, 1, a short last file, whole files): the Vec's fixarray /
    array16 header at 15 / 16 ops, every member width"""
    rng = random.Random(opf)
    w = Written(ctx, oracle, rng.randbytes(32), rng)
    for n in sorted({0, 1, opf - 1, opf, opf + 1, 2 * opf + 1}):
        for col in columns(rng, n)[4:] if n > 2 * opf else columns(rng, n):
            assert len(w.add(col, 1, opf)) == -(-n // opf)
    w.check_readers()
    w.close()


@pytest.mark.parametrize("per_op", [1, 15, 16, 17, 446])
def test_members_per_op_headers(ctx, oracle, per_op):
    """one op a file; n around an op (a short last op, whole ops): the members' fixarray / array16
    header at 15 / 16, the lane and the group work unit, the longest op a page holds"""
    rng = random.Random(100 + per_op)
    w = Written(ctx, oracle, rng.randbytes(32), rng)
    for n in sorted({0, 1, per_op - 1, per_op, per_op + 1, 2 * per_op + 1}):
        for col in (columns(rng, n)[4:] if per_op == 446 and n > per_op else columns(rng, n)):
            assert len(w.add(col, per_op, 1)) == -(-n // per_op)
    w.add([U64] * 446, 446, 1)          # the page's last bytes: 4,086 of clear text at a one-byte counter
    w.check_readers()
    w.close()


def test_defaults_and_middle_shapes(ctx, oracle):
    """per_op 5 x 7 ops a file with the last op and the last file both short; the defaults (28
    one-member ops; the most ops of 3, 16 and 100 members a page holds); 19 ops of 16 members"""
    rng = random.Random(3)
    w = Written(ctx, oracle, rng.randbytes(32), rng)
    got = w.add(mixed(rng, 2 * 35 + 3 * 5 + 2), 5, 7)
    assert len(got) == 3
    assert len(w.add(mixed(rng, 57), 0, 0)) == 3 and w.fusable is False
    for per_op in (3, 16, 100):
        _, k = wm.shape(per_op, 0)
        assert len(w.add([U64] * (per_op * k + 1), per_op, 0)) == 2
    assert len(w.add(mixed(rng, 16 * 19 * 2 + 20), 16, 19)) == 3
    w.check_readers()
    w.close()


def test_defaults_are_fused_by_the_readers(ctx, oracle):
    rng = random.Random(31)
    w = Written(ctx, oracle, rng.randbytes(32), rng)
    got = w.add([U64 - i for i in range(57)], 0, 0)      # nine-byte members: the worst case of 28 ops
    assert len(got) == 3 and w.fusable
    w.check_readers()
    w.close()


# ------------------------------------------------------------------ counters
@pytest.mark.parametrize("edge", [127, 255, 65535, (1 << 32) - 1])
def test_counter_widths(ctx, oracle, edge):
    """c0 three below the edge of a counter width (set by a local Add): the call's counters cross
    it inside one file, lane and group work unit"""
    rng = random.Random(edge)
    w = Written(ctx, oracle, rng.randbytes(32), rng)
    w.local([("Add", (w.actor, edge - 3), [7])])
    assert w.c0() == edge - 3
    w.add(mixed(rng, 8), 1, 8)              # counters edge - 2 .. edge + 5 in one file
    w.local([("Add", (w.actor, 2 * edge - 2), [8])])
    w.add(mixed(rng, 20 * 6 + 3), 20, 0)    # 7 ops of the group form in one file
    w.check_readers()
    w.close()


def test_counter_overflow(ctx, oracle):
    """c0 = 2^64 - 1 - 5: five ops are written (the last counter 2^64 - 1), a sixth is refused"""
    rng = random.Random(5)
    w = Written(ctx, oracle, rng.randbytes(32), rng)
    w.local([("Add", (w.actor, U64 - 5), [1])])
    before = w.core.state_bytes()
    for col, per_op in ((mixed(rng, 6), 1), (mixed(rng, 101), 20)):
        rc, _ = w.core.orswot_add_members(col, per_op, 0, 0, [bytes(24)] * 6)
        assert rc == INVALID and w.core.state_bytes() == before
    got = w.add(mixed(rng, 5), 1, 3)
    assert len(got) == 2 and w.c0() == U64
    assert w.core.orswot_add_members([1], 1, 1, 0, [bytes(24)])[0] == INVALID
    assert w.add([], 1, 1) == []
    w.check_readers()
    w.close()


# ------------------------------------------------------------------ members
def test_member_width_edges(ctx, oracle):
    """the smallest and largest member of every width, 0 and 2^64 - 1 among them, in one op, one an
    op, and split unevenly"""
    rng = random.Random(4)
    w = Written(ctx, oracle, rng.randbytes(32), rng)
    for per_op, opf in ((446, 1), (1, 0), (5, 2), (1, 5)):
        w.add(wm.WIDTH_EDGES, per_op, opf)
    assert set(wm.WIDTH_EDGES) == set(w.oc.state.entries)
    w.check_readers()
    w.close()


def members_with_sum(rng, cnt, total):
    """cnt members whose encoded widths sum to total (cnt <= total <= 9 cnt), shuffled"""
    assert cnt <= total <= 9 * cnt
    ws = [1] * cnt
    left = total - cnt
    i = 0
    while left:
        step = max(s for s in (8, 4, 2, 1) if s <= left)    # 1 -> 9, 5, 3, 2
        ws[i] += step
        left -= step
        i += 1
    assert sum(ws) == total and set(ws) <= set(wm.WIDTH_BYTES)
    rng.shuffle(ws)
    return [wm.member_of_width(rng, w) for w in ws]


def column_of_clear_lengths(rng, lens, per_op):
    """one op a file, per_op members an op, counters of one byte: file i's clear text is lens[i] bytes"""
    col = []
    for L in lens:
        col += members_with_sum(rng, per_op, L - 16 - 1 - 51 - 1 - wm.hdr(per_op))
    return col


def test_clear_lengths_sweep(ctx, oracle):
    """files of 64 consecutive clear lengths (every offset of a file's end, and of the next file's
    start, inside a 16-byte chunk and a 64-byte ChaCha20 block), in ascending and shuffled order,
    in the lane and the group form (a fresh core each: 64 one-op files keep the counter one byte)"""
    rng = random.Random(50)
    lens = list(range(100, 164))
    for per_op, order in ((20, lens), (12, rng.sample(lens, len(lens))), (20, rng.sample(lens, len(lens)))):
        w = Written(ctx, oracle, rng.randbytes(32), rng)
        got = w.add(column_of_clear_lengths(rng, order, per_op), per_op, 1)
        assert [len(f) for f in got] == [16 + wm.sealed_len(L) for L in order]
        w.check_readers()
        w.close()


def test_envelope_header_forms(ctx, oracle):
    """clear lengths on both sides of every length at which the envelope's header changes form
    within one page (a bin8 header becoming bin16)"""
    rng = random.Random(6)
    steps = [L for L in range(17, wm.PAGE) if wm.sealed_len(L + 1) - wm.sealed_len(L) != 1]
    assert len(steps) == 2          # the EncBox's length and the ciphertext's length pass 255
    per_op = 30
    lens = sorted({L + d for L in steps for d in (-1, 0, 1, 2)})
    assert 72 + per_op <= lens[0] and lens[-1] <= 72 + 9 * per_op     # 16 + 1 + 51 + 1 + 3 before the members
    w = Written(ctx, oracle, rng.randbytes(32), rng)
    got = w.add(column_of_clear_lengths(rng, lens, per_op), per_op, 1)
    assert [len(f) - 16 - L for f, L in zip(got, lens)] == [wm.sealed_len(L) - L for L in lens]
    assert len({len(f) - 16 - L for f, L in zip(got, lens)}) == 3
    w.check_readers()
    w.close()


# ------------------------------------------------------------------ grids
def test_more_files_than_one_launch_holds_at_once(ctx, oracle, monkeypatch):
    """9,300 files of three one-member ops (more encoder trips than its grid has blocks), and 150
    files of both work units with the grids clamped to two blocks, so every block takes many trips"""
    rng = random.Random(7)
    w = Written(ctx, oracle, rng.randbytes(32), rng)
    assert len(w.add(mixed(rng, 9300 * 3 - 1), 1, 3)) == 9300
    monkeypatch.setenv("CE_TEST_GRID_CAP", "2")
    assert len(w.add(mixed(rng, 150 * 5 - 2), 1, 5)) == 150
    assert len(w.add(mixed(rng, 150 * 2 * 17 - 20), 17, 2)) == 150
    monkeypatch.delenv("CE_TEST_GRID_CAP")
    w.check_readers()
    w.close()


# ------------------------------------------------------------------ fold
def test_duplicate_members(ctx, oracle):
    """members repeated within an op, across ops and across calls: the entry keeps the local
    actor's largest dot, as the oracle does"""
    rng = random.Random(8)
    w = Written(ctx, oracle, rng.randbytes(32), rng)
    base = mixed(rng, 40) + [0, U64]
    w.add(base + base[:10] + [base[0]] * 5, 1, 0)
    w.add(base * 2 + [base[3]] * 20, 7, 3)
    w.add([5] * 100, 20, 0)
    assert all(v.dots == {w.actor: w.c0()} for m, v in w.oc.state.entries.items() if m == 5)
    w.check_readers()
    w.close()


def test_pending_deferred_removal(ctx, oracle):
    """an ingested Rm whose clock names the local actor at c0 + 2 stays deferred; the writer's adds
    then cover it, apply_deferred runs, and the state equals the oracle's"""
    rng = random.Random(9)
    key = rng.randbytes(32)
    w = Written(ctx, oracle, key, rng)
    w.add([1, 2, 3], 1, 0)
    c0 = w.c0()
    other = rng.randbytes(16)
    ops = [("Add", (other, 1), [2, 50]), ("Rm", C.VClock({w.actor: c0 + 2, other: 1}), [1, 2, 60, 61])]
    files = [crdtenc.CORE_VERSION + e for e in ctx.encrypt_batch(key, [APP + C.enc_orswot_ops(ops)])]
    w.ingest(files, [other], [0], [0])
    assert len(w.oc.state.deferred) == 1
    w.add([60, 1], 1, 0)                # counters c0 + 1, c0 + 2: removed again by the deferred clock
    assert w.oc.state.deferred == {} and 1 not in w.oc.state.entries and 60 not in w.oc.state.entries
    w.add([61, 2, 1], 3, 0)             # c0 + 3: past it
    assert {61, 2, 1} <= set(w.oc.state.entries)
    # still deferred while only part of the clock is covered
    ops = [("Rm", C.VClock({w.actor: w.c0() + 5}), [61, 7])]
    files = [crdtenc.CORE_VERSION + e for e in ctx.encrypt_batch(key, [APP + C.enc_orswot_ops(ops)])]
    w.ingest(files, [other], [0], [1])
    w.add([7, 8], 1, 1)
    assert len(w.oc.state.deferred) == 1 and 7 not in w.oc.state.entries
    w.add([7, 9, 10], 1, 2)
    assert w.oc.state.deferred == {} and 7 not in w.oc.state.entries and 10 in w.oc.state.entries
    w.close()


def test_long_ops_meet_a_deferred_removal(ctx, oracle):
    """ops of 16 and more members reach the fold as one add a member under the op's dot: a deferred
    clock at c0 + 2 removes the members of the first two ops it lists and spares the third's, a
    member repeated across the three keeps the last dot"""
    rng = random.Random(91)
    key = rng.randbytes(32)
    w = Written(ctx, oracle, key, rng)
    w.add([900, 901], 1, 0)
    c0 = w.c0()
    other = rng.randbytes(16)
    listed = list(range(100, 160))
    ops = [("Rm", C.VClock({w.actor: c0 + 2}), listed + [900])]
    files = [crdtenc.CORE_VERSION + e for e in ctx.encrypt_batch(key, [APP + C.enc_orswot_ops(ops)])]
    w.ingest(files, [other], [0], [0])
    assert len(w.oc.state.deferred) == 1
    col = list(range(100, 120)) + list(range(120, 139)) + [100] + list(range(140, 150)) + [100, 121]
    w.add(col, 20, 2)       # counters c0 + 1, c0 + 2 (one file), c0 + 3 (the next)
    live = set(w.oc.state.entries)
    assert w.oc.state.deferred == {} and {100, 121} | set(range(140, 150)) <= live
    assert not (set(range(101, 121)) | set(range(122, 139))) & live
    assert w.oc.state.entries[100].dots == {w.actor: c0 + 3}
    w.check_readers()
    w.close()


def test_sorted_fold_path(ctx, oracle, monkeypatch):
    """CE_DS_SORT_ADDS sends the writer's fold down the sorted path (one add an op, the applied
    flags from the counters): the same files and the same state, short and long ops"""
    rng = random.Random(92)
    w = Written(ctx, oracle, rng.randbytes(32), rng)
    monkeypatch.setenv("CE_DS_SORT_ADDS", "1")
    w.add(mixed(rng, 100) + [3, 3], 1, 0)
    w.add(mixed(rng, 90) + [3] * 5, 20, 0)
    w.add(mixed(rng, 33), 5, 7)
    assert w.core.path_count("ds_adds_monotone") == 0 and w.core.path_count("ds_adds_contiguous") == 0
    monkeypatch.delenv("CE_DS_SORT_ADDS")
    w.add(mixed(rng, 90) + [3] * 5, 20, 0)
    assert w.core.path_count("ds_adds_monotone") == 1
    w.check_readers()
    w.close()


def test_after_a_contiguous_ingest(ctx, oracle):
    """a load_ops-ordered ingest of several actors' runs takes the sort-free applied flags; the
    writer's call sets its own for its one run, and a later host apply_ops with interleaved actors
    takes the sort -- equal to the oracle after each step"""
    rng = random.Random(2024)
    key = rng.randbytes(32)
    actors = G.actors_for(rng, 6)
    files, _ = G.well_formed_orswot(rng, actors, 3, 8, 200)
    acts, clears, fa, fv = G.batch(files, "orswot", APP)
    sealed = [crdtenc.CORE_VERSION + e for e in ctx.encrypt_batch(key, clears)]
    w = Written(ctx, oracle, key, rng)
    w.ingest(sealed, acts, fa, fv)
    assert w.core.path_count("ds_adds_monotone") == 1 and w.core.path_count("ds_adds_contiguous") == 0
    w.add(mixed(rng, 300) + [1000, 2000], 1, 0)
    w.add(mixed(rng, 90), 20, 0)
    assert w.core.path_count("ds_adds_monotone") == 3
    a, b = acts[0], acts[1]
    ca, cb = w.oc.state.clock.get(a), w.oc.state.clock.get(b)
    for rnd in range(2):
        ops = [("Add", (a, ca + 1), [1000 + rnd]), ("Add", (b, cb + 1), [2000 + rnd]),
               ("Add", (a, ca + 2), [3000 + rnd]), ("Add", (b, cb + 2), [1000 + rnd])]
        ca, cb = ca + 2, cb + 2
        w.local(ops)
        w.add([1000 + rnd, 4000 + rnd], 1, 0)
    # the local applies took the sort, the writer's calls their own flags
    assert w.core.path_count("ds_adds_monotone") == 5 and w.core.path_count("ds_adds_contiguous") == 0
    w.close()


def test_table_grows_inside_the_call(ctx, oracle):
    """a fresh core's pair table holds 2,048 pairs at its load bound: 3,000 and then 9,000 new
    members rebuild it inside the call"""
    rng = random.Random(10)
    w = Written(ctx, oracle, rng.randbytes(32), rng)
    w.add([1, 2, 3], 1, 0)
    grows = w.core.path_count("ds_table_rebuilds")
    w.add(list(range(10, 3010)), 1, 0)
    w.add([(1 << 40) + i for i in range(9000)], 400, 1)
    assert w.core.path_count("ds_table_rebuilds") >= grows + 2
    w.check_readers()
    w.close()


# ------------------------------------------------------------------ storage
def uuid_str(u):
    h = u.hex()
    return "%s-%s-%s-%s-%s" % (h[:8], h[8:12], h[12:16], h[16:20], h[20:])


def test_storage_round_trip(ctx, oracle, tmp_path):
    """a core with storage writes: the files sit at ops/<actor>/<v0 + i> with the model's bytes; a
    second replica's read_remote and compact reach the model's state"""
    rng = random.Random(11)
    key = rng.randbytes(32)
    remote = str(tmp_path / "remote")
    w = Written(ctx, oracle, key, rng, local_path=str(tmp_path / "l1"), remote_path=remote, flags=crdtenc.OPEN_CREATE)
    w.add(mixed(rng, 100), 1, 0)
    w.add(wm.WIDTH_EDGES, 5, 2, host=True)
    w.add(mixed(rng, 40), 16, 1)
    d = os.path.join(remote, "ops", uuid_str(w.actor))
    assert sorted(os.listdir(d), key=int) == [str(i) for i in range(len(w.files))]
    for i, f in enumerate(w.files):
        assert open(os.path.join(d, str(i)), "rb").read() == f
    c2 = new_core(ctx, key, local_path=str(tmp_path / "l2"), remote_path=remote, flags=crdtenc.OPEN_CREATE)
    assert c2.read_remote() == 0 and c2.state_bytes() == w.oc.serialize()
    rc, name = c2.compact()
    st = crdtenc.Storage(str(tmp_path / "l2"), remote)
    assert rc == 0 and st.list_state_names() == [name]
    f = st.load_state(name)
    s, pt = oracle.cryptor_decrypt(key, f[16:])
    assert s == 0 and f[:16] == APP and pt == w.oc.serialize() and crdtenc.content_name(f) == name
    c2.close()
    w.close()


# ------------------------------------------------------------------ twins
def test_host_twin_writes_the_same_bytes(ctx, oracle, tmp_path):
    """two cores opened over one local directory are the same actor: the device form and the host
    form, given the same columns and nonces, write the same files and reach the same state"""
    rng = random.Random(12)
    key = rng.randbytes(32)
    kw = dict(local_path=str(tmp_path / "l"), flags=crdtenc.OPEN_CREATE)
    a = Written(ctx, oracle, key, random.Random(99), remote_path=str(tmp_path / "r1"), **kw)
    b = Written(ctx, oracle, key, random.Random(99), remote_path=str(tmp_path / "r2"), **kw)    # the same nonces
    assert a.actor == b.actor
    for per_op, opf, n in ((1, 0, 100), (446, 1, 447), (1, 1, 3), (17, 3, 200), (5, 7, 0)):
        col = mixed(rng, n)
        assert a.add(col, per_op, opf) == b.add(col, per_op, opf, host=True)
    assert a.core.state_bytes() == b.core.state_bytes()
    b.check_readers()
    a.close()
    b.close()


def test_same_effect_as_the_batch_route(ctx, oracle):
    """another core runs apply_ops_batch over the model's vectors (its own actor in the dots): the
    same state but for the actor's bytes, and files of the same lengths"""
    rng = random.Random(13)
    key = rng.randbytes(32)
    w = Written(ctx, oracle, key, rng)
    other = new_core(ctx, key)
    me = other.info_actor()
    for per_op, opf, n in ((1, 0, 90), (30, 2, 100), (1, 58, 59)):
        col = mixed(rng, n)
        c0 = w.c0()
        got = w.add(col, per_op, opf)
        vectors = wm.cut(col, per_op, opf, c0, me)
        rc, fs = other.apply_ops_batch([C.enc_orswot_ops(v) for v in vectors])
        assert rc == 0 and [len(f) for f in fs] == [len(f) for f in got]
        assert other.state_bytes().replace(me, w.actor) == w.core.state_bytes()
    other.close()
    w.close()


# ------------------------------------------------------------------ refusals
def test_refusals_touch_nothing(ctx, oracle, tmp_path):
    """a wrong kind (GSet, MVReg), a pair past the page rule, flags, cap below the bound, n at 2^32,
    counter overflow, no key: each returns its code and leaves state_bytes(), the storage tree, the
    next version and every output as they were"""
    rng = random.Random(14)
    key = rng.randbytes(32)
    remote = str(tmp_path / "remote")
    w = Written(ctx, oracle, key, rng, local_path=str(tmp_path / "l1"), remote_path=remote, flags=crdtenc.OPEN_CREATE)
    w.add([1, 2, 3, 1 << 40], 1, 2)
    top = Written(ctx, oracle, key, rng)
    top.local([("Add", (top.actor, U64 - 2), [1])])
    gs = new_core(ctx, key, kind=crdtenc.STATE_GSET)
    mv = new_core(ctx, key, kind=crdtenc.STATE_MVREG)
    nokey = new_core(ctx, None, local_path=str(tmp_path / "l2"), remote_path=remote, flags=crdtenc.OPEN_CREATE)
    col = [7, 8, 9, 1 << 50, 0, U64]
    n = len(col)
    members = u64_dev(col)
    _, _, max_files, max_bytes = crdtenc.orswot_add_bound(n, 1, 2)
    cases = [(gs, n, 1, 2, 0, max_bytes, INVALID), (mv, n, 1, 2, 0, max_bytes, INVALID),
             (w.core, n, 1, 59, 0, 1 << 20, INVALID), (w.core, n, 447, 1, 0, 1 << 20, INVALID),
             (w.core, n, 16, 20, 0, 1 << 20, INVALID),
             (w.core, n, 1, 2, 1, max_bytes, INVALID), (w.core, n, 1, 2, 0, max_bytes - 1, INVALID),
             (w.core, 1 << 32, 1, 2, 0, 1 << 62, INVALID), (w.core, 1 << 32, 446, 1, 0, 1 << 62, INVALID),
             (w.core, (1 << 32) - 1, 1, 58, 0, 1 << 62, INVALID),       # the clear-text bound passes 2^32
             (top.core, n, 1, 2, 0, max_bytes, INVALID),                # counters would pass 2^64 - 1
             (nokey, n, 1, 2, 0, max_bytes, NO_KEY)]

    def tree():
        return sorted((p, tuple(sorted(fs))) for p, _, fs in os.walk(str(tmp_path)))
    cores = (w.core, top.core, gs, mv, nokey)
    before = {c: c.state_bytes() for c in cores}
    disk = tree()
    nonces = ctypes.create_string_buffer(b"\x55" * (24 * max_files))
    for core, cnt, per_op, opf, flags, cap, code in cases:
        d_files = torch.full((max_bytes + GUARD,), FILL, dtype=torch.uint8, device=DEV)
        d_offs = torch.full((max_files + 1 + GUARD,), -1, dtype=torch.int64, device=DEV)
        torch.cuda.synchronize()
        nf, nb = ctypes.c_uint32(0xDEADBEEF), ctypes.c_uint64(0xDEADBEEFDEADBEEF)
        rc = crdtenc.lib().ce_core_orswot_add_members_device(
            core.p, ctypes.c_void_p(members.data_ptr()), ctypes.c_uint64(cnt), ctypes.c_uint32(per_op),
            ctypes.c_uint32(opf), ctypes.c_uint32(flags), nonces, ctypes.c_void_p(d_files.data_ptr()),
            ctypes.c_uint64(cap), ctypes.c_void_p(d_offs.data_ptr()), ctypes.byref(nf), ctypes.byref(nb))
        assert rc == code, (rc, code, cnt, per_op, opf, flags, cap)
        assert (nf.value, nb.value) == (0xDEADBEEF, 0xDEADBEEFDEADBEEF)
        assert bool((d_files == FILL).all()) and bool((d_offs == -1).all())
        assert core.state_bytes() == before[core] and tree() == disk
        if cap >= max_bytes and cnt == n:       # the host twin refuses the same arguments (it has no cap)
            assert core.orswot_add_members(col, per_op, opf, flags, [b"\x55" * 24] * max_files) == (code, None)
            assert core.state_bytes() == before[core] and tree() == disk
    # both writers still write their next version after all of them
    got = w.add(col, 1, 2)
    assert len(got) == 3 and os.path.exists(os.path.join(remote, "ops", uuid_str(w.actor), str(len(w.files) - 1)))
    assert len(top.add([5, 6], 1, 1)) == 2 and top.c0() == U64
    for c in (gs, mv, nokey):
        c.close()
    top.close()
    w.close()
