"""The sharded PNCounter ingest on the GPU (ce_core_pn_ingest_ops_device_sharded, ce_core_pn_
pending_export, ce_core_pn_pending_commit, shard.ingest_sharded over a shard.DevicePnShardOps):
every result is compared bit for bit with tests/pncounter_model.py folding the whole batch once in
(shared writer order, version) order.  Scenarios and sealing: tests/test_pn_shard.py.  Without the
three entry points every test here fails on the missing symbols."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest
import torch

import crdtenc
import pncounter_model as pm

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
from test_gset_shard import APP, owners, seal  # noqa: E402
from test_pn_shard import PN_SYMBOLS, SCENARIOS, expected, model_fold, planes_span_ranks, scenario  # noqa: E402
from test_gpu_gset_shard import DEV, WORLD, _find_writers, stats_windows, to_share  # noqa: E402
import kind_shard_gpu as K  # noqa: E402

PN = crdtenc.STATE_PNCOUNTER
SENTINEL = -0x0123456789abcdef


def test_symbols_present():
    for name in PN_SYMBOLS:
        assert hasattr(crdtenc.lib(), name), name


@pytest.fixture(scope="module")
def ctx():
    c = crdtenc.Context(0)
    yield c
    c.close()


def none_pending(core):
    buf = torch.full((2 * core.dense_capacity(),), SENTINEL, dtype=torch.int64, device=DEV)
    for call in (lambda: core.pn_pending_export(buf.data_ptr(), buf.numel()), lambda: core.pn_pending_commit(True),
                 lambda: core.pn_pending_commit(False)):
        with pytest.raises(crdtenc.CeError) as e:
            call()
        assert e.value.code == 64
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())


KIND = K.Kind(PN, pm, "pn_ingest_ops_device_sharded", none_pending)


def export(core):
    """(ready, the exported batch as u64[2 cap]) into a sentinel-filled buffer of exactly 2 cap"""
    cap = core.dense_capacity()
    buf = torch.full((2 * cap + 3,), SENTINEL, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    ready = core.pn_pending_export(buf.data_ptr(), 2 * cap)
    torch.cuda.synchronize()
    assert bool((buf[2 * cap:] == SENTINEL).all())
    if not ready:
        assert bool((buf == SENTINEL).all())        # nothing written
    return ready, K.as_u64(buf[: 2 * cap])


def exchange_commit(cores, rcs, unready=None):
    """The all_reduce(MAX) in numpy: every core commits the elementwise u64 max of the exported
    batches; when a rank is not ready every core commits its own batch and merges the others'
    state bytes.  A failed rank: the healthy ones drop their batch.  unready: the ranks whose export
    must answer ready == 0.  Returns the path."""
    if any(rc not in (0, 13) for rc in rcs):
        for core, rc in zip(cores, rcs):
            if rc in (0, 13):
                core.pn_pending_commit(False)
            none_pending(core)
        return "rejected"
    outs = [export(core) for core in cores]
    if unready is not None:
        assert [r for r, (ready, _) in enumerate(outs) if not ready] == unready
    if all(r for r, _ in outs):
        assert len({b.size for _, b in outs}) == 1          # the same capacity on every rank
        red = torch.from_numpy(np.maximum.reduce([b for _, b in outs]).view(np.int64).copy()).to(DEV)
        torch.cuda.synchronize()
        for core in cores:
            core.pn_pending_commit(True, red.data_ptr(), red.numel())
        return "dense"
    for core in cores:
        core.pn_pending_commit(True)
    states = [core.state_bytes() for core in cores]
    for r, core in enumerate(cores):
        for q, s in enumerate(states):
            if q != r:
                assert core.merge_state(s) == 0
    return "bytes"


@pytest.mark.parametrize("name,want_rc,want_path", SCENARIOS)
def test_three_shares_one_process(ctx, name, want_rc, want_path):
    key, writers, files, fa, fv, pre = scenario(name)
    own = owners(name, writers, fa, fv, WORLD)
    if name == "clean":     # both planes must reduce
        assert planes_span_ranks(key, writers, files, fa, fv, own)
    rcs, cores, shares, starts = K.run_shares(ctx, KIND, key, writers, files, fa, fv, pre, own, name)
    orc, want = expected(pm, name, key, writers, files, fa, fv, pre)
    assert orc == want_rc
    if name == "e0_mismatch":       # refused on every rank, nothing folded, nothing pending
        assert rcs == [69] * WORLD and len(set(starts)) == 2
        for c, s in zip(cores, starts):
            none_pending(c)
            assert c.state_bytes() == s
    elif want_rc in (9, 12):        # one rank holds the bad file: every state bit-identical to its start
        assert sorted(rcs) == [0, 0, want_rc]
        assert exchange_commit(cores, rcs) == "rejected"
        for c, s in zip(cores, starts):
            assert c.state_bytes() == s == want
    else:
        assert rcs == [want_rc] * WORLD
        # the Dot of an unregistered actor sits in (writer 4, version 2): that rank alone is not ready
        unready = [int(own[fa.index(4) + 2])] if name == "unregistered" else []
        assert exchange_commit(cores, rcs, unready) == want_path.split("+")[0]
        for c in cores:
            assert c.state_bytes() == want
            none_pending(c)
    for c in cores:
        c.close()


def _small(rng, key, m, versions, ok):
    """a small clean batch over writers whose owners (world 3) satisfy ok"""
    writers, fa, fv, own = _find_writers(rng, m, versions, ok)
    files = [seal(key, APP + pm.enc_ops([((rng.choice(writers), rng.getrandbits(40)), rng.choice(pm.DIRS))
                                         for _ in range(rng.randint(1, 9))]), rng) for _ in fa]
    return writers, files, fa, fv, own


def test_rank_without_a_file(ctx):
    rng = random.Random(61)
    key = rng.randbytes(32)
    writers, files, fa, fv, own = _small(rng, key, 2, 3, lambda own, fa, fv: set(own) == {0, 1})
    pre = {0: 0, 1: 0}
    rcs, cores, shares, starts = K.run_shares(ctx, KIND, key, writers, files, fa, fv, pre, own)
    assert rcs == [0] * WORLD and shares[2]["n"] == 0
    ready, batch = export(cores[2])
    assert ready and not batch.any()            # an empty pending batch exists
    assert exchange_commit(cores, rcs) == "dense"
    _, model = model_fold(pm, key, writers, files, fa, fv, pre)
    for c in cores:
        assert c.state_bytes() == model.serialize()
        c.close()


def test_export_and_commit_sizes(ctx):
    """cap_words = 2 cap - 1: ready == 0 and nothing written; import_words < 2 cap: refused."""
    rng = random.Random(62)
    key = rng.randbytes(32)
    writers, files, fa, fv, own = _small(rng, key, 2, 4, lambda own, fa, fv: True)
    W = b"".join(writers)
    core = K.new_core(ctx, key, PN, writers)
    d = to_share(files, fa, fv, range(len(files)))
    (hi,) = stats_windows([core], [d], W, 2)
    assert K.ingest(KIND, core, d, W, hi)[0] == 0
    cap = core.dense_capacity()
    buf = torch.full((2 * cap,), SENTINEL, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    assert core.pn_pending_export(buf.data_ptr(), 2 * cap - 1) is False
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
    assert core.pn_pending_export(buf.data_ptr(), 2 * cap) is True
    _, model = model_fold(pm, key, writers, files, fa, fv, {0: 0, 1: 0})
    got = K.as_u64(buf)
    slots = [i for i in range(cap) if got[i] or got[cap + i]]
    assert sorted(int(got[i]) for i in slots if got[i]) == sorted(c for c in model.state.p.dots.values() if c)
    assert sorted(int(got[cap + i]) for i in slots if got[cap + i]) == sorted(c for c in model.state.n.dots.values() if c)
    start = core.state_bytes()
    with pytest.raises(crdtenc.CeError) as e:
        core.pn_pending_commit(True, buf.data_ptr(), 2 * cap - 1)
    assert e.value.code == 64 and core.state_bytes() == start
    core.close()


def test_reject_then_retry(ctx):
    rng = random.Random(63)
    key = rng.randbytes(32)
    writers, files, fa, fv, own = _small(rng, key, 2, 4, lambda own, fa, fv: True)
    W = b"".join(writers)
    core = K.new_core(ctx, key, PN, writers)
    start = core.state_bytes()
    bad = list(files)
    bad[3] = bad[3][:-1] + bytes([bad[3][-1] ^ 1])
    d_bad, d = to_share(bad, fa, fv, range(len(files))), to_share(files, fa, fv, range(len(files)))
    (hi,) = stats_windows([core], [d], W, 2)
    rc, st = K.ingest(KIND, core, d_bad, W, hi)
    assert rc == 9 and st[3] == 9 and sum(st) == 9
    none_pending(core)
    assert core.state_bytes() == start
    assert K.ingest(KIND, core, d, W, hi)[0] == 0
    core.pn_pending_commit(True)
    _, model = model_fold(pm, key, writers, files, fa, fv, {0: 0, 1: 0})
    assert core.state_bytes() == model.serialize()
    none_pending(core)
    core.close()


def test_pending_semantics(ctx):
    rng = random.Random(64)
    key = rng.randbytes(32)
    writers, files, fa, fv, own = _small(rng, key, 2, 3, lambda own, fa, fv: True)
    W = b"".join(writers)
    core, model = K.new_core(ctx, key, PN, writers), pm.Core()
    known = pm.serialize(pm.VClock(), _counter({writers[0]: 5}, {writers[1]: 9}))
    assert core.merge_state(known) == 0
    model.merge_state(known)
    nonce = bytes(range(24))
    before, before_file, before_read = core.state_bytes(), core.compact_to_buffer(nonce=nonce), core.counter_read()
    assert before == model.serialize() and before_read == model.state.read() == -4
    none_pending(core)
    d = to_share(files, fa, fv, range(len(files)))

    def ingest_all(share=d):
        (hi,) = stats_windows([core], [share], W, 2)
        return K.ingest(KIND, core, share, W, hi)[0]
    assert ingest_all() == 0
    # while pending: the committed state only
    assert core.state_bytes() == before and core.compact_to_buffer(nonce=nonce) == before_file
    assert core.counter_read() == before_read
    # dropped, then folded again
    core.pn_pending_commit(False)
    assert core.state_bytes() == before
    none_pending(core)
    assert ingest_all() == 0
    # merge_state while pending goes to the committed state and survives the commit
    more = pm.serialize(pm.VClock(), _counter({writers[1]: 1 << 50}, {}))
    assert core.merge_state(more) == 0
    model.merge_state(more)
    assert core.state_bytes() == model.serialize()
    core.pn_pending_commit(True)
    assert model.read_remote_ops(key, [APP], files, [writers[a] for a in fa], fv)[0] == 0
    assert core.state_bytes() == model.serialize() and core.counter_read() == model.state.read()
    none_pending(core)
    # a plain ingest drops a pending batch: only its own file is folded
    core.reset()
    assert ingest_all() == 0
    rc, _ = core.ingest_ops(files[:1], writers, fa[:1], fv[:1])
    assert rc == 0
    none_pending(core)
    _, one = model_fold(pm, key, writers, files[:1], fa[:1], fv[:1], {0: 0, 1: 0})
    assert core.state_bytes() == one.serialize()
    # a reset drops a pending batch
    assert ingest_all() == 0
    core.reset()
    none_pending(core)
    assert core.state_bytes() == pm.Core().serialize()
    core.close()


def _counter(p, n):
    c = pm.PNCounter()
    c.p, c.n = pm.VClock(p), pm.VClock(n)
    return c


def test_refusals(ctx):
    rng = random.Random(65)
    key = rng.randbytes(32)
    writers = sorted(rng.randbytes(16) for _ in range(2))
    W = b"".join(writers)
    for state in (crdtenc.STATE_VCLOCK, crdtenc.STATE_GCOUNTER, crdtenc.STATE_ORSWOT, crdtenc.STATE_MVREG,
                  crdtenc.STATE_GSET):
        other = K.new_core(ctx, key, state)
        K.new_calls_refuse(other, W)
        other.close()
    # each kind refuses the other's calls, and both still refuse the old ones
    pn, lw = K.new_core(ctx, key, PN, writers), K.new_core(ctx, key, crdtenc.STATE_LWWREG, writers)
    L, vp = crdtenc.lib(), ctypes.c_void_p
    d = to_share([b"x" * 40], [0], [0], [0])
    hi = torch.zeros(3, dtype=torch.int64, device=DEV)
    buf = torch.full((2 * pn.dense_capacity(),), 7, dtype=torch.int64, device=DEV)
    ready, rec = ctypes.c_int(5), (ctypes.c_uint64 * 4)(71, 72, 73, 74)
    assert K.raw_sharded_call(pn, "ce_core_lwwreg_ingest_ops_device_sharded", d, W, hi.data_ptr()) == (64, 55)
    assert L.ce_core_lwwreg_pending_record(pn.p, rec) == 64 and list(rec) == [71, 72, 73, 74]
    assert L.ce_core_lwwreg_pending_commit(pn.p, 1, None, ctypes.c_uint32(0)) == 64
    assert K.raw_sharded_call(lw, "ce_core_pn_ingest_ops_device_sharded", d, W, hi.data_ptr()) == (64, 55)
    assert L.ce_core_pn_pending_export(lw.p, vp(buf.data_ptr()), ctypes.c_uint64(buf.numel()), ctypes.byref(ready)) == 64
    assert L.ce_core_pn_pending_commit(lw.p, 1, None, ctypes.c_uint64(0)) == 64
    torch.cuda.synchronize()
    assert ready.value == 5 and bool((buf == 7).all())
    K.old_calls_still_refuse(pn, W)
    K.old_calls_still_refuse(lw, W)
    pn.close()
    lw.close()


def test_one_rank_rccl_sharded_ingest(tmp_path):
    """World 1 under RCCL: the collectives of shard.ingest_sharded on device tensors, both planes."""
    key, writers, files, fa, fv, pre = scenario("clean")
    orc, want = expected(pm, "clean", key, writers, files, fa, fv, pre)
    ((rc, path, n, state, _start),) = K.rank_worker_results(tmp_path, REPO, "pn", 1, "clean", "nccl")
    assert (rc, path, n) == (0, "dense", len(files)) and state == want
