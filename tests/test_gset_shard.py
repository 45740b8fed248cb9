"""GSet<u64> op files partitioned across ranks by address (shard.ingest_gset_sharded, include/
crdtenc.h ce_core_gset_*), on CPU:

  * the three entry points are exported by libcrdtenc.so and wrapped in crdtenc.py;
  * gloo runs of shard.ingest_gset_sharded itself at world 2 and 3 over a host twin
    (tests/gset_shard_twin.py: gset_model opens and decodes, the product's host twins gate),
    one writer's run split across the ranks, with a gap, skipped old versions, a tampered file, a
    cut-short element, a partition-contract break (the exact windows) and ranks that start from
    different next_op_versions: every rank's state == gset_model's single fold of the whole batch
    in (shared writer order, version) order, bit for bit, every rank returns the same (rc, path),
    and a rank failing locally leaves all ranks unchanged.

The scenarios here are the GPU tests' too (tests/test_gpu_gset_shard.py).
"""
import os
import random
import socket
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
import gset_model as gm  # noqa: E402
import shard  # noqa: E402

APP = bytes.fromhex("aadfd5a66e194b24a8024fa27c72f20c")
U64 = (1 << 64) - 1
WIDTHS = [(0, 7), (7, 8), (8, 16), (16, 32), (32, 64)]   # fixint, cc, cd, ce, cf
SCENARIOS = [   # (name, rc, path)
    ("clean", 0, "members"),
    ("old_versions", 0, "members"),
    ("gap", 13, "members"),
    ("tamper", 9, "rejected"),
    ("decode", 12, "rejected"),
    ("contract", 0, "members+exact"),
    ("e0_mismatch", 69, "refused"),
]


def test_entry_points_are_exported_and_wrapped():
    lib = crdtenc.lib()
    for name in ("ce_core_gset_ingest_ops_device_sharded", "ce_core_gset_pending_members",
                 "ce_core_gset_pending_commit"):
        assert hasattr(lib, name) and name in crdtenc.EXPORTS, name
    for name in ("gset_ingest_ops_device_sharded", "gset_pending_members", "gset_pending_commit"):
        assert callable(getattr(crdtenc.Core, name)), name
    assert callable(shard.ingest_gset_sharded)
    for name in ("compute_stats", "window", "set_window", "metadata", "writer_versions", "ingest",
                 "pending_count", "export_members", "commit"):
        assert callable(getattr(shard.DeviceGsetShardOps, name)), name


def pool(rng, n=64):
    """~n member ids of every encoded width, 0 and 2^64 - 1 among them"""
    ids = [0, U64]
    for lo, hi in WIDTHS:
        ids += [rng.randrange(1 << lo if lo else 1, 1 << hi) for _ in range((n - 2) // len(WIDTHS))]
    return ids


def seal(key, clear, rng):
    import oracle
    st, enc = oracle.cryptor_encrypt(key, rng.randbytes(24), clear)
    assert st == 0
    return crdtenc.CORE_VERSION + enc


def scenario(name, seed=9, m=6, versions=9):
    """(key, writers, files, fa, fv, pre): GSet op files sealed with the oracle, in (writer,
    version) order, 0-20 members each from a pool of ~64 ids (one width per file for some, mixed
    for the others); pre = how many leading versions of each writer both the ranks and the model
    fold first (the replicated starting state)."""
    rng = random.Random(seed)
    key = rng.randbytes(32)
    writers = sorted(rng.randbytes(16) for _ in range(m))
    ids = pool(rng)
    files, fa, fv = [], [], []
    for a in range(m):
        for v in range(versions):
            if name == "gap" and a == 2 and v == 4:
                continue
            k = rng.randint(0, 20)
            if rng.random() < 0.4:      # one element width: the uniform path
                lo, hi = rng.choice(WIDTHS)
                same = [x for x in ids if (1 << lo if lo else 0) <= x < (1 << hi)]
                ms = [rng.choice(same) for _ in range(k)]
            else:
                ms = [rng.choice(ids) for _ in range(k)]
            body = gm.enc_ops(ms)
            if name == "decode" and a == 3 and v == 5:
                body = gm.enc_ops(ms + [U64])[:-2]      # the last element cut short
            f = seal(key, APP + body, rng)
            if name == "tamper" and a == 3 and v == 5:
                f = f[:-1] + bytes([f[-1] ^ 1])
            files.append(f)
            fa.append(a)
            fv.append(v)
    pre = {a: (3 if name == "old_versions" and a % 2 == 0 else 0) for a in range(m)}
    return key, writers, files, fa, fv, pre


def rank_pre(name, pre, rank):
    """Versions of each writer folded before the sharded ingest on `rank`: the scenario's
    replicated start, except e0_mismatch, where rank 1 alone has also folded writer 1's version 0."""
    if name == "e0_mismatch" and rank == 1:
        return {**pre, 1: 1}
    return pre


def owners(name, writers, fa, fv, world):
    own = crdtenc.shard_owners(writers, fa, fv, world)
    if name == "contract":         # one file handed to the next rank
        own[11] = (own[11] + 1) % world
    return own


def model_fold(key, writers, files, fa, fv, pre):
    """(rc, model) of the single fold: the start (each writer's first pre versions), then the
    whole batch in (writer, version) order."""
    model = gm.Core()
    first = [i for i in range(len(files)) if fv[i] < pre[fa[i]]]
    if first:
        assert model.read_remote_ops(key, [APP], [files[i] for i in first], [writers[fa[i]] for i in first],
                                     [fv[i] for i in first])[0] == 0
    rc, _ = model.read_remote_ops(key, [APP], files, [writers[x] for x in fa], fv)
    return rc, model


def start_core(key, writers, files, fa, fv, pre):
    """the model after each writer's first pre versions: a rank's state before the sharded ingest"""
    first = [i for i in range(len(files)) if fv[i] < pre[fa[i]]]
    return model_fold(key, writers, [files[i] for i in first], [fa[i] for i in first], [fv[i] for i in first],
                      {a: 0 for a in pre})[1]


def expected(name, key, writers, files, fa, fv, pre):
    """(rc, state bytes) every rank must end with; None for the state when it is the rank's own
    start (refused before any fold).  A failing file rejects the batch in the model too
    (read_remote_ops opens and decodes everything first), so its state is the start."""
    if name == "e0_mismatch":
        return shard.ERR_SHARD, None
    rc, model = model_fold(key, writers, files, fa, fv, pre)
    return rc, model.serialize()


# ---- gloo runs of shard.ingest_gset_sharded over the host twin --------------------------------

def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_main(rank, world, port, name, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from gset_shard_twin import HostGsetShardOps
        key, writers, files, fa, fv, pre = scenario(name)
        own = owners(name, writers, fa, fv, world)
        pre = rank_pre(name, pre, rank)
        core = start_core(key, writers, files, fa, fv, pre)
        start = core.serialize()
        sel = [i for i in range(len(files)) if own[i] == rank]
        ops = HostGsetShardOps(core, key, writers, [files[i] for i in sel], [fa[i] for i in sel],
                               [fv[i] for i in sel])
        rc, path = shard.ingest_gset_sharded(ops)
        with open("%s.%d" % (out_path, rank), "wb") as f:
            f.write(msgpack.packb([rc, path, len(sel), sorted(set(fa[i] for i in sel)), core.serialize(), start],
                                  use_bin_type=True))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name,want_rc,want_path", SCENARIOS)
def test_sharded_ingest_equals_single_fold(tmp_path, name, want_rc, want_path, world):
    key, writers, files, fa, fv, pre = scenario(name)
    orc, want = expected(name, key, writers, files, fa, fv, pre)
    assert orc == want_rc
    out = str(tmp_path / "r")
    mp.spawn(_rank_main, args=(world, _free_port(), name, out), nprocs=world, join=True)
    starts, failed_locally = set(), 0
    for r in range(world):
        with open("%s.%d" % (out, r), "rb") as f:
            rc, path, n, split, state, start = msgpack.unpackb(f.read(), raw=False)
        assert (rc, path) == (want_rc, want_path), (r, rc, path)
        assert 0 < n < len(files) and len(split) == len(writers)   # every writer split across ranks
        assert state == (start if want is None else want), r
        if want_rc in (9, 12):      # all ranks unchanged, the healthy ones included
            assert state == start
        starts.add(start)
    assert len(starts) == (2 if name == "e0_mismatch" else 1)
