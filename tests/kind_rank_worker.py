"""One rank of the multi-process sharded PNCounter / LWWReg ingest (tests/test_gpu_pn_shard.py,
tests/test_gpu_lwwreg_shard.py): a real torch.distributed group (gloo, every rank on GPU 0 of the
box; CE_TEST_BACKEND=nccl: RCCL, one rank), this rank's share (by address) of the scenario's op
files resident in HBM, then shard.ingest_sharded over a DevicePnShardOps, or
shard.ingest_lwwreg_sharded, through the C ABI.  Writes [rc, path, files here, state bytes, start
bytes] to <out>.<rank>.

  python tests/kind_rank_worker.py pn|lww RANK WORLD PORT SCENARIO OUT
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "crdt-enc_amd"), REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    kind, rank, world, port, name, out = (sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5],
                                          sys.argv[6])
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    import msgpack
    import numpy as np
    import torch
    import torch.distributed as dist
    import crdtenc
    import shard
    from test_gset_shard import APP, owners, rank_pre
    if kind == "pn":
        from test_pn_shard import scenario
        state = crdtenc.STATE_PNCOUNTER
    else:
        from test_lwwreg_shard import scenario
        state = crdtenc.STATE_LWWREG
    backend = os.environ.get("CE_TEST_BACKEND", "gloo")
    if backend == "nccl":
        torch.cuda.set_device(0)
    dist.init_process_group(backend, rank=rank, world_size=world)
    try:
        key, writers, files, fa, fv, pre = scenario(name)
        pre = rank_pre(name, pre, rank)
        own = owners(name, writers, fa, fv, world)
        ctx = crdtenc.Context(0)
        core = crdtenc.Core(ctx, kind=state, supported=[APP], current_data_version=APP)
        core.set_latest_key(key)
        core.register_actors(writers)
        first = [i for i in range(len(files)) if fv[i] < pre[fa[i]]]
        if first:  # the starting state (replicated, except for e0_mismatch)
            rc, _ = core.ingest_ops([files[i] for i in first], writers, [fa[i] for i in first], [fv[i] for i in first])
            assert rc == 0, rc
        start = core.state_bytes()
        sel = [i for i in range(len(files)) if own[i] == rank]
        blob = b"".join(files[i] for i in sel)
        offs = np.zeros(len(sel) + 1, np.int64)
        offs[1:] = np.cumsum([len(files[i]) for i in sel])
        dev = torch.device("cuda", 0)
        d_files = torch.frombuffer(bytearray(blob + bytes(64)), dtype=torch.uint8).to(dev)
        d_offs = torch.from_numpy(offs).to(dev)
        d_fa = torch.tensor([fa[i] for i in sel], dtype=torch.int32, device=dev)
        d_fv = torch.tensor([fv[i] for i in sel], dtype=torch.int64, device=dev)
        args = (core, b"".join(writers), d_files, d_offs, len(sel), len(blob), d_fa, d_fv)
        if kind == "pn":
            rc, path = shard.ingest_sharded(shard.DevicePnShardOps(*args))
        else:
            rc, path = shard.ingest_lwwreg_sharded(shard.DeviceLwwShardOps(*args))
        with open("%s.%d" % (out, rank), "wb") as f:
            f.write(msgpack.packb([rc, path, len(sel), core.state_bytes(), start], use_bin_type=True))
        core.close()
        ctx.close()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
