"""LWWReg<u64, u64> op files partitioned across ranks by address (shard.ingest_lwwreg_sharded,
include/crdtenc.h ce_core_lwwreg_*), on CPU:

  * the entry points and the reduce's test hook are exported by libcrdtenc.so and wrapped;
  * the pick rule (shard.lww_pick, the rule of ce_core_lwwreg_pending_commit) against the model's
    fold in (writer, version) order, for every order the ranks' records can arrive in;
  * gloo runs of shard.ingest_lwwreg_sharded itself at world 2 and 3 over a host twin
    (tests/lww_shard_twin.py: lwwreg_model opens and decodes, the product's host twins gate) over
    test_gset_shard.py's scenario list: every rank's state and next_op_versions ==
    lwwreg_model's single fold of the whole batch in (shared writer order, version) order, bit for
    bit -- the markers come from a small pool, so the largest one is tied across files and ranks
    -- every rank returns the same (rc, path), and a rank failing locally leaves all ranks
    unchanged.

The scenarios here are the GPU tests' too (tests/test_gpu_lwwreg_shard.py).
"""
import itertools
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
import lwwreg_model as lm  # noqa: E402
import shard  # noqa: E402
from test_gset_shard import APP, _free_port, owners, rank_pre, seal  # noqa: E402,F401
from test_pn_shard import expected, model_fold, start_core  # noqa: E402,F401

U64 = (1 << 64) - 1
SCENARIOS = [   # (name, rc, path)
    ("clean", 0, "record"),
    ("old_versions", 0, "record"),
    ("gap", 13, "record"),
    ("tamper", 9, "rejected"),
    ("decode", 12, "rejected"),
    ("contract", 0, "record+exact"),
    ("e0_mismatch", 69, "refused"),
]
LWW_SYMBOLS = ("ce_core_lwwreg_ingest_ops_device_sharded", "ce_core_lwwreg_pending_record",
               "ce_core_lwwreg_pending_commit", "ce_ctx_prim_lww_reduce_keyed")


def test_entry_points_are_exported_and_wrapped():
    lib = crdtenc.lib()
    for name in LWW_SYMBOLS:
        assert hasattr(lib, name) and name in crdtenc.EXPORTS, name
    for name in ("lwwreg_ingest_ops_device_sharded", "lwwreg_pending_record", "lwwreg_pending_commit"):
        assert callable(getattr(crdtenc.Core, name)), name
    assert callable(crdtenc.Context.prim_lww_reduce_keyed)
    assert callable(shard.ingest_lwwreg_sharded) and callable(shard.lww_pick)
    for name in ("compute_stats", "window", "set_window", "metadata", "writer_versions", "ingest", "record",
                 "commit"):
        assert callable(getattr(shard.DeviceLwwShardOps, name)), name


def test_pick_rule_equals_the_fold_in_apply_order():
    """Four records at distinct (writer, version) addresses, markers from {0, 5, 9} in all 81
    ways (repeated markers, marker 0, all zero), in all 24 arrival orders: the pick is the
    register a fold in (writer, version) order reaches, and never depends on the arrival order."""
    addrs = [(0, 3), (0, 7), (2, 0), (5, 1)]
    for markers in itertools.product([0, 5, 9], repeat=4):
        recs = [(m, 100 + i, a, v) for i, (m, (a, v)) in enumerate(zip(markers, addrs))]
        reg = lm.LWWReg()
        for m, val, _, _ in sorted(recs, key=lambda r: (r[2], r[3])):
            reg.update(val, m)
        for order in itertools.permutations(recs):
            got = shard.lww_pick(order)
            assert (got[1], got[0]) == reg.read(), (markers, order)
            if reg.marker == 0:
                assert got == shard.LWW_NONE
    # the largest u64s order as unsigned
    assert shard.lww_pick([(U64, 1, 4, 4), (U64 - 1, 2, 0, 0)])[1] == 1
    assert shard.lww_pick([(7, 1, 1, U64), (7, 2, 1, U64 - 1)])[1] == 2


def test_more_than_64_remote_records_raise(monkeypatch):
    """ce_core_lwwreg_pending_commit takes at most 64 remote records: a larger world is refused
    before any collective"""
    monkeypatch.setattr(shard.dist, "get_rank", lambda group=None: 0)
    monkeypatch.setattr(shard.dist, "get_world_size", lambda group=None: 66)
    with pytest.raises(ValueError):
        shard.ingest_lwwreg_sharded(object())


def test_twin_has_the_device_steps():
    import lww_shard_twin
    assert lww_shard_twin.DEVICE is shard.DeviceLwwShardOps
    for name in ("compute_stats", "window", "set_window", "metadata", "writer_versions", "ingest", "record",
                 "commit"):
        assert callable(getattr(lww_shard_twin.HostLwwShardOps, name)), name


def scenario(name, seed=29, m=6, versions=9):
    """(key, writers, files, fa, fv, pre): LWWReg op files sealed with the oracle, in (writer,
    version) order, 0-8 ops each; markers from a pool of 10 values of every encoded width (0 and
    2^64 - 1 among them), so every marker repeats across files with different vals; pre = how many
    leading versions of each writer both the ranks and the model fold first."""
    rng = random.Random(seed)
    key = rng.randbytes(32)
    writers = sorted(rng.randbytes(16) for _ in range(m))
    pool = [0, 1, 0x7f, 0xc8, 0x1234, 0x89abcdef, 1 << 40, U64 - 1, U64, U64]
    files, fa, fv = [], [], []
    for a in range(m):
        for v in range(versions):
            if name == "gap" and a == 2 and v == 4:
                continue
            ops = [(rng.getrandbits(rng.choice([6, 8, 16, 32, 64])), rng.choice(pool))
                   for _ in range(rng.randint(0, 8))]
            body = lm.enc_ops(ops)
            if name == "decode" and a == 3 and v == 5:
                body = lm.enc_ops(ops + [(U64, U64)])[:-2]      # the last element cut short
            f = seal(key, APP + body, rng)
            if name == "tamper" and a == 3 and v == 5:
                f = f[:-1] + bytes([f[-1] ^ 1])
            files.append(f)
            fa.append(a)
            fv.append(v)
    pre = {a: (3 if name == "old_versions" and a % 2 == 0 else 0) for a in range(m)}
    return key, writers, files, fa, fv, pre


# ---- gloo runs of shard.ingest_lwwreg_sharded over the host twin ------------------------------

def _rank_main(rank, world, port, name, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from lww_shard_twin import HostLwwShardOps
        key, writers, files, fa, fv, pre = scenario(name)
        own = owners(name, writers, fa, fv, world)
        pre = rank_pre(name, pre, rank)
        core = start_core(lm, key, writers, files, fa, fv, pre)
        start = core.serialize()
        sel = [i for i in range(len(files)) if own[i] == rank]
        ops = HostLwwShardOps(core, key, writers, [files[i] for i in sel], [fa[i] for i in sel],
                              [fv[i] for i in sel])
        rc, path = shard.ingest_lwwreg_sharded(ops)
        with open("%s.%d" % (out_path, rank), "wb") as f:
            f.write(msgpack.packb([rc, path, len(sel), sorted(set(fa[i] for i in sel)), core.serialize(), start],
                                  use_bin_type=True))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name,want_rc,want_path", SCENARIOS)
def test_sharded_ingest_equals_single_fold(tmp_path, name, want_rc, want_path, world):
    key, writers, files, fa, fv, pre = scenario(name)
    orc, want = expected(lm, name, key, writers, files, fa, fv, pre)
    assert orc == want_rc
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
