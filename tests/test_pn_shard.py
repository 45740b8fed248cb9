"""PNCounter<Uuid> op files partitioned across ranks by address (shard.ingest_sharded over a
shard.DevicePnShardOps, include/crdtenc.h ce_core_pn_*), on CPU:

  * the entry points are exported by libcrdtenc.so and wrapped in crdtenc.py;
  * gloo runs of shard.ingest_sharded itself at world 2 and 3 over a host twin
    (tests/pn_shard_twin.py: pncounter_model opens and decodes, the product's host twins gate)
    over test_gset_shard.py's scenario list, plus a Dot naming an unregistered actor (the bytes
    path): every rank's state and next_op_versions == pncounter_model's single fold of the whole
    batch in (shared writer order, version) order, bit for bit, every rank returns the same
    (rc, path), and a rank failing locally leaves all ranks unchanged.

The scenarios here are the GPU tests' too (tests/test_gpu_pn_shard.py).
"""
import os
import random
import sys

import msgpack
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "crdt-enc_amd"), REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import crdtenc  # noqa: E402
import pncounter_model as pm  # noqa: E402
import shard  # noqa: E402
from test_gset_shard import APP, _free_port, owners, rank_pre, seal  # noqa: E402,F401

SCENARIOS = [   # (name, rc, path)
    ("clean", 0, "dense"),
    ("old_versions", 0, "dense"),
    ("gap", 13, "dense"),
    ("tamper", 9, "rejected"),
    ("decode", 12, "rejected"),
    ("contract", 0, "dense+exact"),
    ("e0_mismatch", 69, "refused"),
    ("unregistered", 0, "bytes"),
]
PN_SYMBOLS = ("ce_core_pn_ingest_ops_device_sharded", "ce_core_pn_pending_export", "ce_core_pn_pending_commit")


def test_entry_points_are_exported_and_wrapped():
    lib = crdtenc.lib()
    for name in PN_SYMBOLS:
        assert hasattr(lib, name) and name in crdtenc.EXPORTS, name
    for name in ("pn_ingest_ops_device_sharded", "pn_pending_export", "pn_pending_commit"):
        assert callable(getattr(crdtenc.Core, name)), name
    for name in ("compute_stats", "window", "set_window", "metadata", "writer_versions", "ingest", "dense_buffer",
                 "export_pending", "commit"):
        assert callable(getattr(shard.DevicePnShardOps, name)), name


def test_twin_has_the_device_steps():
    import pn_shard_twin
    assert pn_shard_twin.DEVICE is shard.DevicePnShardOps
    for name in ("compute_stats", "window", "set_window", "metadata", "writer_versions", "ingest", "dense_buffer",
                 "export_pending", "commit"):
        assert callable(getattr(pn_shard_twin.HostPnShardOps, name)), name


def scenario(name, seed=19, m=6, versions=9):
    """(key, writers, files, fa, fv, pre): PNCounter op files sealed with the oracle, in (writer,
    version) order, 0-12 ops each naming the writers themselves, Pos and Neg mixed, counters of
    every encoded width; pre = how many leading versions of each writer both the ranks and the
    model fold first (the replicated starting state).  "unregistered": one op names an actor that
    is no writer."""
    rng = random.Random(seed)
    key = rng.randbytes(32)
    writers = sorted(rng.randbytes(16) for _ in range(m))
    stranger = rng.randbytes(16)
    files, fa, fv = [], [], []
    for a in range(m):
        for v in range(versions):
            if name == "gap" and a == 2 and v == 4:
                continue
            ops = [((rng.choice(writers), rng.getrandbits(rng.choice([6, 8, 16, 32, 64]))), rng.choice(pm.DIRS))
                   for _ in range(rng.randint(0, 12))]
            if name == "unregistered" and a == 4 and v == 2:
                ops.append(((stranger, 77), "Neg"))
            body = pm.enc_ops(ops)
            if name == "decode" and a == 3 and v == 5:
                body = pm.enc_ops(ops + [((writers[0], 1 << 40), "Pos")])[:-2]      # the last element cut short
            f = seal(key, APP + body, rng)
            if name == "tamper" and a == 3 and v == 5:
                f = f[:-1] + bytes([f[-1] ^ 1])
            files.append(f)
            fa.append(a)
            fv.append(v)
    pre = {a: (3 if name == "old_versions" and a % 2 == 0 else 0) for a in range(m)}
    return key, writers, files, fa, fv, pre


def model_fold(mod, key, writers, files, fa, fv, pre, cls=None):
    """(rc, model) of the single fold: the start (each writer's first pre versions), then the
    whole batch in (writer, version) order."""
    model = (cls or mod.Core)()
    first = [i for i in range(len(files)) if fv[i] < pre[fa[i]]]
    if first:
        assert model.read_remote_ops(key, [APP], [files[i] for i in first], [writers[fa[i]] for i in first],
                                     [fv[i] for i in first])[0] == 0
    rc, _ = model.read_remote_ops(key, [APP], files, [writers[x] for x in fa], fv)
    return rc, model


def start_core(mod, key, writers, files, fa, fv, pre, cls=None):
    """the model after each writer's first pre versions: a rank's state before the sharded ingest"""
    first = [i for i in range(len(files)) if fv[i] < pre[fa[i]]]
    return model_fold(mod, key, writers, [files[i] for i in first], [fa[i] for i in first], [fv[i] for i in first],
                      {a: 0 for a in pre}, cls)[1]


def expected(mod, name, key, writers, files, fa, fv, pre):
    """(rc, state bytes) every rank must end with; None for the state when it is the rank's own
    start (refused before any fold).  A failing file rejects the batch in the model too."""
    if name == "e0_mismatch":
        return shard.ERR_SHARD, None
    rc, model = model_fold(mod, key, writers, files, fa, fv, pre)
    return rc, model.serialize()


def planes_span_ranks(key, writers, files, fa, fv, own):
    """True when some actor's largest Pos counter and largest Neg counter sit in files of different
    ranks: neither plane's reduce can be skipped."""
    best = {}
    for i, f in enumerate(files):
        one = pm.Core()
        assert one.read_remote_ops(key, [APP], [f], [writers[fa[i]]], [0])[0] == 0
        for d, v in (("p", one.state.p), ("n", one.state.n)):
            for a, c in v.dots.items():
                if c > best.get((a, d), (0, None))[0]:
                    best[(a, d)] = (c, int(own[i]))
    for a in writers:
        p, n = best.get((a, "p")), best.get((a, "n"))
        if p and n and p[1] != n[1]:
            return True
    return False


# ---- gloo runs of shard.ingest_sharded over the host twin -----------------------------------

def _rank_main(rank, world, port, name, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pn_shard_twin import HostPnShardOps, TwinPnCore
        key, writers, files, fa, fv, pre = scenario(name)
        own = owners(name, writers, fa, fv, world)
        pre = rank_pre(name, pre, rank)
        core = start_core(pm, key, writers, files, fa, fv, pre, TwinPnCore)
        start = core.serialize()
        sel = [i for i in range(len(files)) if own[i] == rank]
        ops = HostPnShardOps(core, key, writers, writers, [files[i] for i in sel], [fa[i] for i in sel],
                             [fv[i] for i in sel])
        rc, path = shard.ingest_sharded(ops)
        with open("%s.%d" % (out_path, rank), "wb") as f:
            f.write(msgpack.packb([rc, path, len(sel), sorted(set(fa[i] for i in sel)), core.serialize(), start],
                                  use_bin_type=True))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name,want_rc,want_path", SCENARIOS)
def test_sharded_ingest_equals_single_fold(tmp_path, name, want_rc, want_path, world):
    key, writers, files, fa, fv, pre = scenario(name)
    orc, want = expected(pm, name, key, writers, files, fa, fv, pre)
    assert orc == want_rc
    if name == "clean":
        assert planes_span_ranks(key, writers, files, fa, fv, owners(name, writers, fa, fv, world))
    out = str(tmp_path / "r")
    mp.spawn(_rank_main, args=(world, _free_port(), name, out), nprocs=world, join=True)
    starts = set()
    for r in range(world):
        with open("%s.%d" % (out, r), "rb") as f:
            rc, path, n, split, state, start = msgpack.unpackb(f.read(), raw=False)
        assert (rc, path) == (want_rc, want_path), (r, rc, path)
        assert 0 < n < len(files) and len(split) == len(writers)   # every writer split across ranks
        assert state == (start if want is None else want), r       # (the bytes carry next_op_versions too)
        if want_rc in (9, 12):      # all ranks unchanged, the healthy ones included
            assert state == start
        starts.add(start)
    assert len(starts) == (2 if name == "e0_mismatch" else 1)
