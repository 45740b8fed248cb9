"""Helpers shared by tests/test_gpu_pn_shard.py and tests/test_gpu_lwwreg_shard.py: three cores on
one device play three ranks of a sharded ingest, exchanged in-process as tests/
test_gpu_gset_shard.py does (whose share upload and window helpers these build on).  `kind` is a
small record of what differs between the two state kinds."""
import ctypes

import numpy as np
import torch

import crdtenc
from test_gset_shard import APP, rank_pre
from test_gpu_gset_shard import DEV, WORLD, exact_windows, stats_windows, to_share

INVALID = 64


class Kind:
    """state: the crdtenc kind; model: the model module; ingest(core, ...): the sharded ingest's
    wrapper name; none_pending(core): asserts that no batch is pending."""

    def __init__(self, state, model, ingest, none_pending):
        self.state, self.model, self.ingest_name, self.none_pending = state, model, ingest, none_pending


def new_core(ctx, key, state, writers=None):
    c = crdtenc.Core(ctx, kind=state, supported=[APP], current_data_version=APP)
    c.set_latest_key(key)
    if writers:
        c.register_actors(writers)
    return c


def ingest(kind, core, d, W, hi):
    """(rc, per-file statuses) of the kind's sharded ingest over one share"""
    return getattr(core, kind.ingest_name)(d["files"].data_ptr(), d["offs"].data_ptr(), d["n"], d["blob_len"], W,
                                           d["fa"].data_ptr(), d["fv"].data_ptr(), hi.data_ptr(), want_status=True)


def file_statuses(kind, key, files, sel):
    """what opening and decoding each file alone gives (the gate has no part in it)"""
    return [kind.model.Core().read_remote_ops(key, [APP], [files[i]], [bytes(16)], [0])[0] for i in sel]


def run_shares(ctx, kind, key, writers, files, fa, fv, pre, own, name="", before=None, order=None):
    """Start state, stats -> max -> windows -> sharded ingest (pending) on WORLD cores.  order: a
    function placing a rank's file indices in the order its share holds them.  Returns (rcs,
    cores, shares, starts); the per-file statuses are checked here."""
    W, m = b"".join(writers), len(writers)
    cores, shares, starts = [], [], []
    for r in range(WORLD):
        core = new_core(ctx, key, kind.state, writers)
        p = rank_pre(name, pre, r)
        first = [i for i in range(len(files)) if fv[i] < p[fa[i]]]
        if first:
            rc, _ = core.ingest_ops([files[i] for i in first], writers, [fa[i] for i in first], [fv[i] for i in first])
            assert rc == 0
        if before:
            before(core)
        cores.append(core)
        starts.append(core.state_bytes())
        sel = [i for i in range(len(files)) if own[i] == r]
        shares.append(to_share(files, fa, fv, order(sel) if order else sel))
    his = stats_windows(cores, shares, W, m)
    got = [ingest(kind, c, d, W, h) for c, d, h in zip(cores, shares, his)]
    if name == "contract":
        # the reduced stats flag the broken contract on every rank: nothing opened, nothing pending
        assert [rc for rc, _ in got] == [69] * WORLD
        for c, s in zip(cores, starts):
            kind.none_pending(c)
            assert c.state_bytes() == s
        his = exact_windows(cores, fa, fv, W)
        got = [ingest(kind, c, d, W, h) for c, d, h in zip(cores, shares, his)]
    for (rc, st), d in zip(got, shares):
        if rc != 69:
            want = file_statuses(kind, key, files, d["sel"])
            assert st == want, (rc, st, want)
            assert rc == next((s for s in want if s), rc)       # the lowest failing file's status
    return [rc for rc, _ in got], cores, shares, starts


def raw_sharded_call(core, symbol, d, W, hi_ptr):
    """(rc, status word) of a sharded-ingest symbol called directly over a one-file share, the
    status preset to 55"""
    st = (ctypes.c_int32 * 1)(55)
    vp = ctypes.c_void_p
    rc = getattr(crdtenc.lib(), symbol)(core.p, vp(d["files"].data_ptr()), vp(d["offs"].data_ptr()),
                                        ctypes.c_uint32(d["n"]), ctypes.c_uint64(d["blob_len"]), W,
                                        ctypes.c_uint32(len(W) // 16), vp(d["fa"].data_ptr()), vp(d["fv"].data_ptr()),
                                        vp(hi_ptr), st)
    return rc, st[0]


def old_calls_still_refuse(core, W):
    """the dense exchange and the generic sharded calls on a PNCounter / LWWReg core: 64, nothing
    touched (pinned by the kinds' own test files too)"""
    L, vp = crdtenc.lib(), ctypes.c_void_p
    cap = core.dense_capacity()
    buf = torch.full((2 * cap,), 7, dtype=torch.int64, device=DEV)
    nov = torch.full((cap,), 7, dtype=torch.int64, device=DEV)
    ready = ctypes.c_int(5)
    before = core.state_bytes()
    assert core.dense_ready() is False and L.ce_core_dense_ready(core.p) == 0
    assert L.ce_core_export_dense(core.p, vp(buf.data_ptr()), vp(nov.data_ptr())) == INVALID
    assert L.ce_core_import_dense(core.p, vp(buf.data_ptr()), vp(nov.data_ptr())) == INVALID
    d = to_share([b"x" * 40], [0], [0], [0])
    assert raw_sharded_call(core, "ce_core_ingest_ops_device_sharded", d, W, nov.data_ptr()) == (INVALID, 55)
    assert raw_sharded_call(core, "ce_core_gset_ingest_ops_device_sharded", d, W, nov.data_ptr()) == (INVALID, 55)
    assert L.ce_core_pending_export(core.p, vp(buf.data_ptr()), ctypes.c_uint64(2 * cap), ctypes.byref(ready)) == INVALID
    assert L.ce_core_pending_commit(core.p, 1, None, ctypes.c_uint64(0)) == INVALID
    torch.cuda.synchronize()
    assert ready.value == 5 and bool((buf == 7).all()) and bool((nov == 7).all())
    assert core.state_bytes() == before


def new_calls_refuse(core, W):
    """each of the six new calls on a core of another kind: 64, no output touched"""
    L, vp = crdtenc.lib(), ctypes.c_void_p
    cap = core.dense_capacity()
    buf = torch.full((2 * max(cap, 1),), 7, dtype=torch.int64, device=DEV)
    hi = torch.zeros(len(W) // 16 + 1, dtype=torch.int64, device=DEV)
    before = core.state_bytes()
    d = to_share([b"x" * 40], [0], [0], [0])
    ready = ctypes.c_int(5)
    rec = (ctypes.c_uint64 * 4)(71, 72, 73, 74)
    assert raw_sharded_call(core, "ce_core_pn_ingest_ops_device_sharded", d, W, hi.data_ptr()) == (INVALID, 55)
    assert raw_sharded_call(core, "ce_core_lwwreg_ingest_ops_device_sharded", d, W, hi.data_ptr()) == (INVALID, 55)
    assert L.ce_core_pn_pending_export(core.p, vp(buf.data_ptr()), ctypes.c_uint64(buf.numel()), ctypes.byref(ready)) == INVALID
    for accept in (0, 1):
        assert L.ce_core_pn_pending_commit(core.p, accept, None, ctypes.c_uint64(0)) == INVALID
        assert L.ce_core_lwwreg_pending_commit(core.p, accept, None, ctypes.c_uint32(0)) == INVALID
    assert L.ce_core_lwwreg_pending_record(core.p, rec) == INVALID
    torch.cuda.synchronize()
    assert ready.value == 5 and list(rec) == [71, 72, 73, 74] and bool((buf == 7).all())
    assert core.state_bytes() == before


def rank_worker_results(tmp_path, repo, kind_name, world, name, backend):
    """tests/kind_rank_worker.py as `world` processes; their [rc, path, files, state, start]"""
    import os
    import socket
    import subprocess
    import sys

    import msgpack
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    out = str(tmp_path / "k")
    env = dict(os.environ, CE_TEST_BACKEND=backend)
    procs = [subprocess.Popen([sys.executable, os.path.join(repo, "tests", "kind_rank_worker.py"), kind_name,
                               str(r), str(world), port, name, out], env=env) for r in range(world)]
    rcs = []
    try:
        for p in procs:
            rcs.append(p.wait(timeout=180))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert rcs == [0] * world       # a failed or signalled child fails the test here
    res = []
    for r in range(world):
        with open("%s.%d" % (out, r), "rb") as f:
            res.append(msgpack.unpackb(f.read(), raw=False))
    return res


def as_u64(t):
    return t.cpu().numpy().view(np.uint64)
