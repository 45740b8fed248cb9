"""The with_state reads on the GPU (include/crdtenc.h: ce_core_set_contains[_device], ce_core_set_len,
ce_core_set_members_device, ce_core_counter_read, ce_core_clock_get, ce_core_read_clock,
ce_core_orswot_member_clocks, ce_core_mvreg_read).  Every comparison is exact, against the models
read directly: tests/gset_model.py (state.value), oracle/crdts.py (Orswot.entries / .clock,
MVReg.vals, VClock.get), tests/pncounter_model.py and the C oracle's GCounter state.  Without the
nine entry points every test here fails on the missing symbols."""
import ctypes
import random

import msgpack
import numpy as np
import pytest
import torch

import crdtenc
import gset_model as gm
import pncounter_model as pm
from oracle import crdts as C

pytestmark = pytest.mark.gpu
APP = bytes.fromhex("aadfd5a66e194b24a8024fa27c72f20c")
CORE = crdtenc.CORE_VERSION
U64 = (1 << 64) - 1
DEV = "cuda:0"
INVALID = 64
KINDS = {"vclock": crdtenc.STATE_VCLOCK, "gcounter": crdtenc.STATE_GCOUNTER, "orswot": crdtenc.STATE_ORSWOT,
         "mvreg": crdtenc.STATE_MVREG, "pncounter": crdtenc.STATE_PNCOUNTER, "gset": crdtenc.STATE_GSET}


@pytest.fixture(scope="module")
def ctx():
    c = crdtenc.Context(0)
    yield c
    c.close()


def new_core(ctx, kind, key):
    c = crdtenc.Core(ctx, kind=KINDS[kind], supported=[APP], current_data_version=APP)
    c.set_latest_key(key)
    return c


def seal(ctx, key, clears):
    return [CORE + e for e in ctx.encrypt_batch(key, clears)]


def u64_dev(values):
    t = torch.from_numpy(np.asarray(values, np.uint64).view(np.int64).copy()).to(DEV)
    torch.cuda.synchronize()
    return t


def contains_device(core, queries):
    """the device form: numpy u8 answers, 0xAB where the kernel wrote nothing"""
    q = u64_dev(queries)
    out = torch.full((max(len(queries), 1),), 0xAB, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    assert core.contains_device(q.data_ptr() if len(queries) else None, len(queries),
                                out.data_ptr() if len(queries) else None) == 0
    return out.cpu().numpy()[:len(queries)]


def members_device(core):
    rc, n = core.members_device(None, 0)            # the size query: nothing written
    assert rc == 0
    small = torch.full((max(n, 2),), -1, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    if n > 1:
        assert core.members_device(small.data_ptr(), n - 1) == (0, n)     # too small: untouched
        assert bool((small == -1).all())
    assert core.members_device(small.data_ptr(), max(n, 2)) == (0, n)
    return [int(x) for x in small.cpu().numpy().view(np.uint64)[:n]]


def check_set(core, present, queries):
    """contains (both forms), set_len and set_members_device against the model's member set"""
    want = np.array([1 if m in present else 0 for m in queries], np.uint8)
    host = core.contains(queries)
    assert host.tolist() == want.tolist()
    assert contains_device(core, queries).tolist() == want.tolist()
    assert core.set_len() == len(present)
    assert members_device(core) == sorted(present)


# ------------------------------------------------------------------ 1. GSet contains
def gs_hash(k):
    """the Python twin of ce_gset_device.h gs_hash"""
    k = (k * 0x9E3779B97F4A7C15) & U64
    return (k >> 32) ^ (k & 0xFFFFFFFF)


def keys_at(rng, slot, mask, n, avoid=()):
    out = []
    while len(out) < n:
        k = rng.getrandbits(64)
        if k and gs_hash(k) & mask == slot and k not in avoid and k not in out:
            out.append(k)
    return out


def test_gset_contains_min_capacity_and_after_growth(ctx, monkeypatch):
    """A 16-slot table, then the same core after one growth (128 slots).  Present and absent keys,
    duplicates, 0 absent then present, 2^64 - 1, absent keys that hash into occupied runs, and runs
    that wrap past the last slot (three keys whose home is the last slot: the run covers slots
    mask, 0, 1; an absent key with that home walks the whole of it).  Query counts around a wave
    and a block, and one past grid x probes-per-lane under a two-block grid, so the grid-stride
    loop runs three times and the last trip has one query in flight of eight."""
    monkeypatch.setenv("CE_GSET_CAP", "16")
    rng = random.Random(11)
    key = rng.randbytes(32)
    core, model = new_core(ctx, "gset", key), gm.Core()
    me = core.info_actor()
    counts = [0, 1, 63, 64, 65, 257, 2 * 256 * 16 + 1]

    def run(mask):
        present = model.state.value
        homes = sorted({gs_hash(k) & mask for k in present if k})
        absent = keys_at(rng, mask, mask, 3, present)                    # wraps: home = the last slot
        for h in homes[:6]:
            absent += keys_at(rng, h, mask, 2, present)                  # into occupied runs
        absent += [rng.getrandbits(64) | 1 << 63 for _ in range(8)] + [1, U64 - 1]
        absent = [k for k in absent if k not in present]
        pool = sorted(present) + absent + [0, U64]
        for n in counts:
            monkeypatch.setenv("CE_TEST_GRID_CAP", "2" if n > 4096 else "0")
            q = [rng.choice(pool) for _ in range(n)]
            if n >= 63:
                q[:len(pool)] = pool[:n]                                  # every key of the pool, then repeats
            want = [1 if k in present else 0 for k in q]
            assert contains_device(core, q).tolist() == want
            assert core.contains(q).tolist() == want
        monkeypatch.setenv("CE_TEST_GRID_CAP", "0")
        assert core.set_len() == len(present)
        assert members_device(core) == sorted(present)
        assert core.state_bytes() == model.serialize()

    def apply(ops):
        assert core.apply_ops(gm.enc_ops(ops)) == 0
        model.apply_ops(me, ops)

    run(15)                                                               # the empty set
    apply(keys_at(rng, 15, 15, 3) + keys_at(rng, 7, 15, 2) + [U64])      # 6 of the 8 claims allowed
    assert core.path_count("gset_grows") == 0
    run(15)
    apply([0])                                                            # out of band: no claim
    assert core.path_count("gset_grows") == 0
    run(15)
    apply(keys_at(rng, 127, 127, 3) + [rng.getrandbits(64) for _ in range(40)])
    assert core.path_count("gset_grows") == 1
    run(127)
    core.close()


# ------------------------------------------------------------------ 2. GSet pending batch
def test_gset_pending_batch_is_not_read(ctx):
    """After the sharded ingest the batch is pending: its members answer 0 and set_len is
    unchanged; committed (accept = 1) they answer 1; a second batch dropped (accept = 0) answers 0."""
    rng = random.Random(12)
    key, w = rng.randbytes(32), rng.randbytes(16)
    core, model = new_core(ctx, "gset", key), gm.Core()
    base = [rng.getrandbits(64) for _ in range(20)] + [5]
    assert core.apply_ops(gm.enc_ops(base)) == 0
    model.apply_ops(core.info_actor(), base)

    def pending_ingest(version, members):
        files = seal(ctx, key, [APP + gm.enc_ops(members)])
        blob = torch.frombuffer(bytearray(files[0] + bytes(64)), dtype=torch.uint8).to(DEV)
        offs = torch.tensor([0, len(files[0])], dtype=torch.int64, device=DEV)
        fa = torch.zeros(1, dtype=torch.int32, device=DEV)
        fv = torch.tensor([version], dtype=torch.int64, device=DEV)
        st = torch.empty(2 + 3, dtype=torch.int64, device=DEV)
        hi = torch.empty(2, dtype=torch.int64, device=DEV)
        torch.cuda.synchronize()
        core.shard_stats(w, fa.data_ptr(), fv.data_ptr(), 1, 0, 1, st.data_ptr())
        core.shard_window(w, st.data_ptr(), hi.data_ptr())
        assert core.gset_ingest_ops_device_sharded(blob.data_ptr(), offs.data_ptr(), 1, len(files[0]), w,
                                                   fa.data_ptr(), fv.data_ptr(), hi.data_ptr()) == 0
        return files

    first = [rng.getrandbits(64) for _ in range(30)] + [0, base[0]]
    q = first + base + [rng.getrandbits(64) for _ in range(10)]
    files = pending_ingest(0, first)
    check_set(core, model.state.value, q)                     # pending: the committed set alone
    assert core.gset_pending_commit(True) == 0
    assert model.read_remote_ops(key, [APP], files, [w], [0])[0] == 0
    check_set(core, model.state.value, q)
    assert all(core.contains(first))
    second = [rng.getrandbits(64) for _ in range(30)]
    pending_ingest(1, second)
    check_set(core, model.state.value, q + second)
    assert core.gset_pending_commit(False) == 0
    check_set(core, model.state.value, q + second)
    assert not any(core.contains(second))
    assert core.state_bytes() == model.serialize()
    core.close()


# ------------------------------------------------------------------ 3. Orswot contains / len / members
def orswot_files(ctx, key, per_actor):
    """{actor: [ops of version 0, 1, ...]} -> sealed files, writers, file_actor, versions"""
    actors = sorted(per_actor)
    clears, fa, fv = [], [], []
    for i, a in enumerate(actors):
        for v, ops in enumerate(per_actor[a]):
            clears.append(APP + C.enc_orswot_ops(ops))
            fa.append(i)
            fv.append(v)
    return seal(ctx, key, clears), actors, fa, fv


@pytest.mark.parametrize("primary", [None, "32"])
def test_orswot_contains_len_members_through_every_path(ctx, monkeypatch, primary):
    """The reads after each path that changes the tables -- op fold, k-way state merge (with a
    table growth), merge_columns_device, local apply_ops, reset -- each read building the live-flag
    cache the next step has to invalidate.  Members: added; added then removed (the key stays in the
    member table, the answer is 0); removed then added again; under a deferred removal whose clock
    does not cover the member's dot (present, before and after the clock is covered, as the model
    says); ~0 absent, then present.  primary "32": a 32-slot primary member table that is never
    grown, so most members sit in the overflow table."""
    if primary:
        monkeypatch.setenv("CE_DS_PRIMARY_SLOTS", primary)
    rng = random.Random(13)
    key = rng.randbytes(32)
    a0, a1, a2 = sorted(rng.randbytes(16) for _ in range(3))
    core, oc = new_core(ctx, "orswot", key), C.Core("orswot")
    me = core.info_actor()
    X, Y, Z = 500, 501, 502
    touched = {X, Y, Z, U64, 0, 1 << 63}

    def check():
        present = set(oc.state.entries)
        q = sorted(touched) + [rng.getrandbits(64) for _ in range(20)] + [X, U64, X]
        rng.shuffle(q)
        check_set(core, present, q)
        assert core.state_bytes() == oc.serialize()

    check()                                                                # the empty set
    # 1) op fold: adds, X added then removed, Y removed (nothing there) then added
    ops0 = [[("Add", (a0, 1), list(range(1, 101)))], [("Add", (a0, 2), [X, Z])],
            [("Rm", C.VClock({a0: 2}), [X, Y])], [("Add", (a0, 3), [Y])]]
    ops1 = [[("Add", (a1, 1), list(range(90, 201)))]]
    files, acts, fa, fv = orswot_files(ctx, key, {a0: ops0, a1: ops1})
    touched.update(range(1, 201))
    assert core.ingest_ops(files, acts, fa, fv)[0] == 0
    assert oc.read_remote_ops(key, [APP], files, [acts[i] for i in fa], fv)[0] == 0
    assert X not in oc.state.entries and Y in oc.state.entries
    check()
    # 2) k-way state merge of three replicas' states, 3000 members more: the pair table grows
    sws = []
    for r in range(3):
        part = C.Core("orswot")
        b = rng.randbytes(16)
        ms = list(range(10_000 + 1000 * r, 11_000 + 1000 * r)) + [150, Y]
        part.state.apply(("Add", (b, 1), ms))
        part.nov.apply(b, 1)
        touched.update(ms[::37])
        sws.append(part.serialize())
    sf = seal(ctx, key, [APP + sw for sw in sws])
    rebuilds = core.path_count("ds_table_rebuilds")
    assert core.ingest_states(sf)[0] == oc.read_remote_states(key, [APP], sf)[0] == 0
    assert core.path_count("states_kway_merge") == 1
    assert core.path_count("ds_table_rebuilds") > rebuilds
    check()
    # 3) merge_columns_device: another core's column partial, removing 1..10 it saw from a0
    other, om = new_core(ctx, "orswot", key), C.Core("orswot")
    files1, acts1, fa1, fv1 = orswot_files(ctx, key, {a0: ops0[:1]})
    assert other.ingest_ops(files1, acts1, fa1, fv1)[0] == 0
    assert om.read_remote_ops(key, [APP], files1, [acts1[i] for i in fa1], fv1)[0] == 0
    for ops in ([("Rm", C.VClock({a0: 1}), list(range(1, 11)))], [("Add", (other.info_actor(), 1), [7, 700, U64 - 1])]):
        assert other.apply_ops(C.enc_orswot_ops(ops)) == 0
        for op in ops:
            om.state.apply(op)
        om.nov.apply(other.info_actor(), om.nov.get(other.info_actor()) + 1)
    touched.update([700, U64 - 1])
    assert other.state_bytes() == om.serialize()
    rc, n = other.export_columns_device(None, 0)
    assert (rc, n) == (INVALID, 1)
    col = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    rc, n = other.export_columns_device(col.data_ptr(), col.numel())
    assert rc == 0
    assert core.merge_columns_device([col.data_ptr()], [n]) == 0
    oc.state.merge(om.state)
    oc.nov.merge(om.nov)
    assert 3 not in oc.state.entries and 7 in oc.state.entries and 95 in oc.state.entries
    check()
    other.close()
    # 4) local apply_ops: ~0 present, Y removed with its read context, X added again, Z under a
    #    deferred removal that names a counter of a2 nobody has seen and not Z's own dot
    assert U64 not in oc.state.entries

    def local(ops):
        assert core.apply_ops(C.enc_orswot_ops(ops)) == 0
        for op in ops:
            oc.state.apply(op)
        oc.nov.apply(me, oc.nov.get(me) + 1)

    local([("Add", (me, 1), [U64, 42])])
    check()
    local([("Rm", oc.state.entries[Y].clone(), [Y]), ("Add", (me, 2), [X])])
    assert Y not in oc.state.entries and X in oc.state.entries
    check()
    local([("Rm", C.VClock({a0: 1, a2: 7}), [Z, 42])])
    assert oc.state.deferred and Z in oc.state.entries and 42 in oc.state.entries
    check()
    local([("Add", (a2, 7), [42])])                                        # the clock covers the removal now
    assert not oc.state.deferred and Z in oc.state.entries
    check()
    # 5) reset, and a fold into the emptied tables
    core.reset()
    oc = C.Core("orswot")
    check()
    assert core.ingest_ops(files, acts, fa, fv)[0] == 0
    assert oc.read_remote_ops(key, [APP], files, [acts[i] for i in fa], fv)[0] == 0
    check()
    core.close()


# ------------------------------------------------------------------ 4. reads settle
def test_reads_settle_queued_work(ctx):
    """An Orswot op fold and a k-way state merge return without a host wait; a read issued straight
    after them gives the answer that holds after ce_core_settle."""
    rng = random.Random(14)
    key = rng.randbytes(32)
    a0, a1 = sorted(rng.randbytes(16) for _ in range(2))
    files, acts, fa, fv = orswot_files(ctx, key, {a0: [[("Add", (a0, 1), list(range(1, 300)))],
                                                      [("Rm", C.VClock({a0: 1}), list(range(1, 300, 3)))]],
                                                 a1: [[("Add", (a1, 1), [2, 4, 6, 1000])]]})
    sws = []
    for r in range(2):
        part = C.Core("orswot")
        b = rng.randbytes(16)
        part.state.apply(("Add", (b, 1), list(range(2000 + 50 * r, 2100 + 50 * r))))
        part.nov.apply(b, 1)
        sws.append(part.serialize())
    sf = seal(ctx, key, [APP + sw for sw in sws])
    q = list(range(0, 320)) + list(range(1990, 2160)) + [1000, U64]
    got = []
    for settle_first in (False, True):
        core, oc = new_core(ctx, "orswot", key), C.Core("orswot")
        assert core.ingest_ops(files, acts, fa, fv)[0] == 0
        assert oc.read_remote_ops(key, [APP], files, [acts[i] for i in fa], fv)[0] == 0
        if settle_first:
            assert core.settle() == 0
        fold = (core.contains(q).tolist(), core.set_len())
        assert fold == ([1 if m in oc.state.entries else 0 for m in q], len(oc.state.entries))
        assert core.ingest_states(sf)[0] == oc.read_remote_states(key, [APP], sf)[0] == 0
        if settle_first:
            assert core.settle() == 0
        merged = (members_device(core), core.contains(q).tolist())
        assert merged == (sorted(oc.state.entries), [1 if m in oc.state.entries else 0 for m in q])
        got.append((fold, merged))
        assert core.state_bytes() == oc.serialize()
        core.close()
    assert got[0] == got[1]


# ------------------------------------------------------------------ 5. member clocks, the Rm round trip
def test_orswot_member_clocks_and_rm_round_trip(ctx):
    """orswot_member_clocks == entries[m] for present, absent and removed members (entries in UUID
    order, one member holding dots of four actors, a repeated query), then the example app's step:
    an Rm carrying that read context goes through apply_ops and the member is gone."""
    rng = random.Random(15)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(4))
    core, oc = new_core(ctx, "orswot", key), C.Core("orswot")
    me = core.info_actor()
    M, GONE = 77, 78
    per = {a: [[("Add", (a, 1), [M, 1000 + i] + ([GONE] if i == 0 else []))]] for i, a in enumerate(actors)}
    per[actors[0]].append([("Rm", C.VClock({actors[0]: 1}), [GONE])])
    per[actors[1]].append([("Add", (actors[1], 2), list(range(2000, 2400)) + [U64])])
    files, acts, fa, fv = orswot_files(ctx, key, per)
    assert core.ingest_ops(files, acts, fa, fv)[0] == 0
    assert oc.read_remote_ops(key, [APP], files, [acts[i] for i in fa], fv)[0] == 0
    assert len(oc.state.entries[M].dots) == 4 and GONE not in oc.state.entries

    def want(m):
        e = oc.state.entries.get(m)
        return sorted(e.dots.items()) if e else []

    q = [M, 5, GONE, 1000, M, U64, 2399, 1003]
    got = core.orswot_member_clocks(q)
    assert got == [want(m) for m in q]
    assert [a for a, _ in got[0]] == actors and got[1] == got[2] == []
    assert core.orswot_member_clocks([]) == []
    many = list(range(1990, 2410))                                          # more queries than a block
    assert core.orswot_member_clocks(many) == [want(m) for m in many]
    assert core.read_clock() == sorted(oc.state.clock.dots.items())
    # Rm { clock: the member's read context, members: [M] }
    op = ("Rm", C.VClock(dict(got[0])), [M])
    assert core.apply_ops(C.enc_orswot_ops([op])) == 0
    oc.state.apply(op)
    oc.nov.apply(me, oc.nov.get(me) + 1)
    assert M not in oc.state.entries and not oc.state.deferred
    assert core.contains([M, 1000]).tolist() == [0, 1]
    assert core.orswot_member_clocks([M]) == [[]]
    assert core.state_bytes() == oc.serialize()
    core.close()


# ------------------------------------------------------------------ 6. the example app's loop on MVReg
def test_mvreg_read_context_put_loop(ctx):
    """examples/test/src/main.rs:45-54 on an MVReg: read, derive the context, put, apply_ops."""
    rng = random.Random(16)
    key = rng.randbytes(32)
    a, b = sorted(rng.randbytes(16) for _ in range(2))
    core, oc = new_core(ctx, "mvreg", key), C.Core("mvreg")
    me = core.info_actor()
    assert core.mvreg_read() == [] and core.read_clock() == []
    clears = [APP + C.enc_mvreg_ops([("Put", C.VClock({a: 1}), 10)]), APP + C.enc_mvreg_ops([("Put", C.VClock({b: 1}), 20)])]
    files = seal(ctx, key, clears)
    assert core.ingest_ops(files, [a, b], [0, 1], [0, 0])[0] == 0
    assert oc.read_remote_ops(key, [APP], files, [a, b], [0, 0])[0] == 0
    assert core.state_bytes() == oc.serialize()
    vals = core.mvreg_read()
    assert vals == [v for _, v in oc.state.vals] and sorted(vals) == [10, 20]
    join = C.VClock()
    for c, _ in oc.state.vals:
        join.merge(c)
    assert core.read_clock() == sorted(join.dots.items()) == [(a, 1), (b, 1)]
    assert core.clock_get([b, me, a]) == [1, 0, 1]
    clock = C.VClock(dict(core.read_clock()))
    clock.apply(me, core.clock_get([me])[0] + 1)
    op = ("Put", clock, max(vals) + 1)
    assert core.apply_ops(C.enc_mvreg_ops([op])) == 0
    oc.state.apply(op)
    oc.nov.apply(me, oc.nov.get(me) + 1)
    assert core.mvreg_read() == [21] == [v for _, v in oc.state.vals]
    assert core.read_clock() == sorted(clock.dots.items())
    assert core.state_bytes() == oc.serialize()
    core.close()


# ------------------------------------------------------------------ 7. counters
def c_oracle_state(oc):
    """the C oracle's state VClock read directly: {actor: counter}"""
    n = oc.c.state.n
    acts = ctypes.string_at(oc.c.state.actor, 16 * n) if n else b""
    ctrs = (ctypes.c_uint64 * n).from_address(oc.c.state.counter) if n else []
    return {acts[16 * i:16 * i + 16]: int(ctrs[i]) for i in range(n)}


@pytest.mark.parametrize("n_actors", [1, 255, 257, 2100])
def test_gcounter_read_and_clock(ctx, oracle, n_actors):
    """GCounter::read over 1, 255, 257 actors (around a block of the sum) and 2100 (past the 2048
    the actor table holds before it grows), three of them near 2^64 - 1 so the sum needs the high
    word; clock_get for known and unknown actors; read_clock without the zero counters."""
    rng = random.Random(17 + n_actors)
    key, w = rng.randbytes(32), rng.randbytes(16)
    actors = [rng.randbytes(16) for _ in range(n_actors)]
    ctr = {a: rng.getrandbits(rng.choice([6, 20, 40, 63])) + 1 for a in actors}
    for i, a in enumerate(actors[:3]):
        ctr[a] = U64 - i
    zero = rng.randbytes(16)
    dots = [{"actor": a, "counter": c} for a, c in ctr.items()] + [{"actor": zero, "counter": 0}]
    clears = [APP + msgpack.packb(dots[i:i + 80], use_bin_type=True) for i in range(0, len(dots), 80)]
    files = seal(ctx, key, clears)
    core, oc = new_core(ctx, "gcounter", key), oracle.Core(oracle.STATE_GCOUNTER)
    assert core.counter_read() == 0 and core.read_clock() == []
    fv = list(range(len(files)))
    assert core.ingest_ops(files, [w], [0] * len(files), fv)[0] == 0
    assert oc.read_remote_ops(key, [APP], files, [w] * len(files), fv)[0] == 0
    assert core.state_bytes() == oc.serialize()
    state = {a: c for a, c in c_oracle_state(oc).items() if c}
    assert state == ctr
    total = sum(state.values())
    assert core.counter_read() == total and (n_actors < 3 or total >> 64 >= 2)
    assert core.read_clock() == sorted(state.items())
    ask = actors[:5] + [rng.randbytes(16), zero, w] + actors[-3:]
    assert core.clock_get(ask) == [state.get(a, 0) for a in ask]
    assert core.clock_get([]) == []
    core.close()


def test_pncounter_read_and_clocks(ctx):
    """PNCounter::read = p - n: empty, p > n, p == n (magnitude 0, not negative), p < n with the
    difference past 64 bits; clock_get / read_clock of both planes."""
    rng = random.Random(18)
    key = rng.randbytes(32)
    core, model = new_core(ctx, "pncounter", key), pm.Core()
    me = core.info_actor()
    a, b, c = sorted(rng.randbytes(16) for _ in range(3))

    def raw():
        mag = (ctypes.c_uint64 * 2)()
        neg = ctypes.c_int(7)
        assert crdtenc.lib().ce_core_counter_read(core.p, mag, ctypes.byref(neg)) == 0
        return mag[0], mag[1], neg.value

    def apply(ops):
        assert core.apply_ops(pm.enc_ops(ops)) == 0
        for op in ops:
            model.state.apply(op)
        model.nov.apply(me, model.nov.get(me) + 1)

    def check():
        p, n = sum(model.state.p.dots.values()), sum(model.state.n.dots.values())
        assert raw() == crdtenc.pn_words(p, n)
        assert core.counter_read() == model.state.read() == p - n
        for which, v in ((0, model.state.p), (1, model.state.n)):
            live = {x: k for x, k in v.dots.items() if k}
            assert core.read_clock(which) == sorted(live.items())
            ask = [c, a, rng.randbytes(16), b, me]
            assert core.clock_get(ask, which) == [v.get(x) for x in ask]
        assert core.state_bytes() == model.serialize()

    check()
    assert raw() == (0, 0, 0)
    apply([((a, 10), "Pos"), ((b, 3), "Neg")])
    check()
    assert raw() == (7, 0, 0)
    apply([((b, 10), "Neg")])
    check()
    assert raw() == (0, 0, 0)                                              # p == n: magnitude 0, sign clear
    apply([((b, U64), "Neg"), ((c, U64 - 1), "Neg"), ((a, 11), "Pos")])
    check()
    assert raw() == crdtenc.pn_words(11, 2 * U64 - 1) and raw()[1:] == (1, 1)
    apply([((a, U64), "Pos"), ((b, U64), "Pos"), ((c, U64), "Pos")])
    check()
    assert core.counter_read() == 3 * U64 - (2 * U64 - 1)
    core.close()


# ------------------------------------------------------------------ 8. definite refusals
SET_KINDS = {"orswot", "gset"}
COUNTER_KINDS = {"gcounter", "pncounter"}


@pytest.mark.parametrize("kind", list(KINDS))
def test_reads_refuse_other_kinds_definitely(ctx, kind):
    """Every call on every kind it does not serve, and which = 1 on every kind but PNCounter:
    CE_ERR_INVALID_ARG, sentinel-filled outputs untouched, the state bytes unchanged (the
    convention of test_multi_gpu_answers_are_definite)."""
    rng = random.Random(19)
    key = rng.randbytes(32)
    core = new_core(ctx, kind, key)
    a = rng.randbytes(16)
    seed = {"vclock": msgpack.packb([{"actor": a, "counter": 3}], use_bin_type=True),
            "gcounter": msgpack.packb([{"actor": a, "counter": 3}], use_bin_type=True),
            "orswot": C.enc_orswot_ops([("Add", (a, 1), [1, 2, 3])]),
            "mvreg": C.enc_mvreg_ops([("Put", C.VClock({a: 1}), 9)]),
            "pncounter": pm.enc_ops([((a, 3), "Pos"), ((a, 1), "Neg")]),
            "gset": gm.enc_ops([1, 2, 3])}[kind]
    assert core.apply_ops(seed) == 0
    before = core.state_bytes()
    L = crdtenc.lib()
    refused = 0

    def buf():
        b = crdtenc.Buf()
        b.data, b.len = 0xDEAD0, 77
        return b

    def untouched(b):
        return (b.data, b.len) == (0xDEAD0, 77)

    if kind not in SET_KINDS:
        q = u64_dev([1, 2, 3, 4])
        d_out = torch.full((4,), 0xAB, dtype=torch.uint8, device=DEV)
        d_mem = torch.full((8,), -1, dtype=torch.int64, device=DEV)
        torch.cuda.synchronize()
        assert core.contains_device(q.data_ptr(), 4, d_out.data_ptr()) == INVALID
        hq = (ctypes.c_uint64 * 4)(1, 2, 3, 4)
        h_out = (ctypes.c_uint8 * 4)(*[0xAB] * 4)
        assert L.ce_core_set_contains(core.p, hq, ctypes.c_uint64(4), h_out) == INVALID
        n = ctypes.c_uint64(0xAB)
        assert L.ce_core_set_len(core.p, ctypes.byref(n)) == INVALID and n.value == 0xAB
        assert core.members_device(d_mem.data_ptr(), 8)[0] == INVALID
        n2 = ctypes.c_uint64(0xAB)
        assert L.ce_core_set_members_device(core.p, ctypes.c_void_p(d_mem.data_ptr()), ctypes.c_uint64(8),
                                            ctypes.byref(n2)) == INVALID and n2.value == 0xAB
        assert L.ce_core_set_contains_device(core.p, None, ctypes.c_uint64(0), None) == INVALID    # n = 0 too
        torch.cuda.synchronize()
        assert bool((d_out == 0xAB).all()) and bool((d_mem == -1).all()) and list(h_out) == [0xAB] * 4
        refused += 6
    if kind not in COUNTER_KINDS:
        mag = (ctypes.c_uint64 * 2)(0xAB, 0xAB)
        neg = ctypes.c_int(7)
        assert L.ce_core_counter_read(core.p, mag, ctypes.byref(neg)) == INVALID
        assert list(mag) == [0xAB, 0xAB] and neg.value == 7
        refused += 1
    for which in (0, 1):
        if kind != "gset" and (which == 0 or kind == "pncounter"):
            continue
        out = (ctypes.c_uint64 * 2)(0xAB, 0xAB)
        assert L.ce_core_clock_get(core.p, ctypes.c_int(which), a + a, ctypes.c_uint32(2), out) == INVALID
        assert list(out) == [0xAB, 0xAB]
        b = buf()
        assert L.ce_core_read_clock(core.p, ctypes.c_int(which), ctypes.byref(b)) == INVALID and untouched(b)
        refused += 2
    for bad in (2, -1):                                                       # no such clock on any kind
        b = buf()
        assert L.ce_core_read_clock(core.p, ctypes.c_int(bad), ctypes.byref(b)) == INVALID and untouched(b)
    if kind != "orswot":
        hq = (ctypes.c_uint64 * 2)(1, 2)
        b = buf()
        assert L.ce_core_orswot_member_clocks(core.p, hq, ctypes.c_uint32(2), ctypes.byref(b)) == INVALID
        assert untouched(b)
        refused += 1
    if kind != "mvreg":
        b = buf()
        assert L.ce_core_mvreg_read(core.p, ctypes.byref(b)) == INVALID and untouched(b)
        refused += 1
    assert refused >= 3
    assert core.state_bytes() == before
    # and what the kind does serve still answers
    if kind in SET_KINDS:
        assert core.contains([1, 9, 3]).tolist() == [1, 0, 1] and core.set_len() == 3
    if kind in COUNTER_KINDS:
        assert core.counter_read() == (3 if kind == "gcounter" else 2)
    if kind != "gset":
        assert core.clock_get([a]) == [{"orswot": 1, "mvreg": 1}.get(kind, 3)]
    core.close()
