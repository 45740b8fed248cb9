#!/usr/bin/env python3
"""The sharded PNCounter and LWWReg ingests at the C2 shape, rank 0 of a world of 8, on one GPU.

The batches are tools/pncounter_bench.py's and tools/lwwreg_bench.py's: 1,048,576 op files of
4 KiB, 4096 writers x 256 versions, from an empty state.  Each is partitioned by op-file address
(crdtenc.shard_owners, world 8).  This process plays rank 0 and times its own share through the
three calls of the sharded path, each complete on return (the commit is followed by a stream wait):

    PNCounter   ce_core_pn_ingest_ops_device_sharded      (the fused open over 1/8 of the files; pending)
                ce_core_pn_pending_export                 (both planes of the pending batch)
                ce_core_pn_pending_commit                 (the reduced batch, both planes)
    LWWReg      ce_core_lwwreg_ingest_ops_device_sharded  (the fused open, the device gate, the keyed reduce)
                ce_core_lwwreg_pending_record             (32 bytes, host)
                ce_core_lwwreg_pending_commit             (the other seven ranks' records)

beside the unsharded ingest of the whole batch (ce_core_ingest_ops_device) in the same process,
the two alternating and the order swapped every iteration.  The other seven shares' batches /
records are produced UNTIMED by a second core on the same GPU; the reduced PNCounter batch is their
elementwise max with rank 0's.  The windows are the whole batch's (every writer's versions 0..255
present: hi = 256, no flags), set directly.  The collectives of shard.ingest_sharded /
shard.ingest_lwwreg_sharded are NOT measured: one GPU has no fabric, so "share_total_ms" is a lower
bound of an N = 8 step and is reported as a projection.

Reported: medians over the timed iterations of each call's wall-clock ms and of the library's
HIP-event ms of the gate, the fused open and the LWW reduce inside them.  The tool reads nothing
outside the repository tree.

    python tools/kind_shard_bench.py --steps 12 --warmup 2 --out profiles/kind_sharded.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import bench  # noqa: E402
from bench import APP, N_ACTORS, crdtenc  # noqa: E402
import lwwreg_bench as lb  # noqa: E402
import pncounter_bench as pb  # noqa: E402
from gset_shard_bench import share_of  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "crdt-enc_amd"))
import shard  # noqa: E402

WORLD = 8
EVENTS = ("gate", "open_fold_small", "lww_reduce")


def check(rc, ctx):
    if rc:
        raise crdtenc.CeError(rc, ctx.last_error())


def median(rows, f):
    return round(statistics.median(r[f] for r in rows), 4)


def timed(ctx, run):
    """run() between a timer reset and a read: (its result, {event: ms})"""
    ctx.synchronize()
    ctx.timing_reset()
    ctx.set_timing_only(None)
    ctx.set_timing(True)
    out = run()
    ctx.synchronize()
    ctx.set_timing(False)
    return out, {e: ctx.timing(e)[0] for e in EVENTS}


def bench_kind(ctx, name, key, actors, args, dev):
    pn = name == "pncounter"
    state = crdtenc.STATE_PNCOUNTER if pn else crdtenc.STATE_LWWREG
    if pn:
        files, offs, n, blen = pb.build_pn_files(ctx, key, actors, args.versions, dev, seed=4321)
        want = pb.expected_pn_state(actors, args.versions)
    else:
        files, offs, n, blen = lb.build_lww_files(ctx, key, actors.shape[0], args.versions, dev, seed=4321)
        want = lb.expected_lww_state(actors, args.versions)
    file_len = blen // n
    W = b"".join(bytes(a) for a in actors)
    writers = [W[i:i + 16] for i in range(0, len(W), 16)]
    fa_h = np.repeat(np.arange(N_ACTORS, dtype=np.uint32), args.versions)
    fv_h = np.tile(np.arange(args.versions, dtype=np.uint64), N_ACTORS)
    own = crdtenc.shard_owners(writers, fa_h, fv_h, WORLD)
    fa = torch.from_numpy(fa_h.astype(np.int32)).to(dev)
    fv = torch.from_numpy(fv_h.astype(np.int64)).to(dev)
    hi = torch.full((N_ACTORS + 1,), args.versions, dtype=torch.int64, device=dev)
    hi[N_ACTORS] = 0
    torch.cuda.synchronize()

    def core_of():
        c = crdtenc.Core(ctx, kind=state, supported=[APP], current_data_version=APP)
        c.set_latest_key(key)
        c.register_actors(writers)
        return c

    def ingest(c, d):
        f = c.pn_ingest_ops_device_sharded if pn else c.lwwreg_ingest_ops_device_sharded
        check(f(d["files"].data_ptr(), d["offs"].data_ptr(), d["n"], d["blob_len"], W, d["fa"].data_ptr(),
                d["fv"].data_ptr(), hi.data_ptr()), ctx)

    res = {"files": n, "world": WORLD, "steps": args.steps, "warmup": args.warmup,
           "share_files": [int(x) for x in np.bincount(own, minlength=WORLD)]}
    core = core_of()
    cap = core.dense_capacity()
    mine = share_of(files, file_len, np.nonzero(own == 0)[0], fa, fv, dev)
    # the other seven ranks' outcome: untimed, a second core, each from an empty state
    other = core_of()
    reduced = torch.zeros(2 * cap, dtype=torch.int64, device=dev) if pn else None
    remote = []
    for r in range(1, WORLD):
        d = share_of(files, file_len, np.nonzero(own == r)[0], fa, fv, dev)
        other.reset()
        ingest(other, d)
        if pn:
            buf = torch.empty(2 * cap, dtype=torch.int64, device=dev)
            if not other.pn_pending_export(buf.data_ptr(), buf.numel()):
                raise SystemExit("a share's batch is not exportable")
            shard.max_u64_(reduced, buf)
        else:
            remote.append(other.lwwreg_pending_record()[1])
        del d
    other.close()
    torch.cuda.empty_cache()
    mybuf = torch.empty(2 * cap, dtype=torch.int64, device=dev) if pn else None
    whole = crdtenc.Core(ctx, kind=state, supported=[APP], current_data_version=APP)
    whole.set_latest_key(key)
    whole.register_actors(writers)
    actor_bytes = W

    def run_share():
        core.reset()
        ctx.synchronize()
        t0 = time.perf_counter()
        ingest(core, mine)
        t1 = time.perf_counter()
        if pn:
            if not core.pn_pending_export(mybuf.data_ptr(), mybuf.numel()):
                raise SystemExit("the share's batch is not exportable")
        else:
            rec = core.lwwreg_pending_record()[1]
        t2 = time.perf_counter()
        if pn:
            # (the all_reduce(MAX) would run here; the reduced batch stands ready)
            core.pn_pending_commit(True, reduced.data_ptr(), reduced.numel())
        else:
            check(core.lwwreg_pending_commit(True, remote), ctx)
        ctx.synchronize()
        t3 = time.perf_counter()
        return {"ingest_ms": (t1 - t0) * 1e3, "exchange_ms": (t2 - t1) * 1e3, "commit_ms": (t3 - t2) * 1e3,
                "share_total_ms": (t3 - t0) * 1e3}

    def run_whole():
        whole.reset()
        ctx.synchronize()
        t0 = time.perf_counter()
        check(whole.ingest_ops_device(files.data_ptr(), offs.data_ptr(), n, blen, actor_bytes, fa.data_ptr(),
                                      fv.data_ptr()), ctx)
        ctx.synchronize()
        return {"ingest_ms": (time.perf_counter() - t0) * 1e3}

    if pn:  # the reduced batch needs rank 0's own share too: one untimed pass
        core.reset()
        ingest(core, mine)
        if not core.pn_pending_export(mybuf.data_ptr(), mybuf.numel()):
            raise SystemExit("the share's batch is not exportable")
        shard.max_u64_(reduced, mybuf)
        core.pn_pending_commit(False)
    torch.cuda.synchronize()    # torch wrote `reduced`; the core reads it on its own stream
    share_rows, whole_rows = [], []
    for i in range(args.warmup + args.steps):
        pair = [("share", run_share), ("whole", run_whole)]
        if i % 2:
            pair.reverse()      # the order swapped each iteration
        for what, run in pair:
            row, ev = timed(ctx, run)
            row.update({e + "_kernel_ms": ev[e] for e in EVENTS})
            if i >= args.warmup:
                (share_rows if what == "share" else whole_rows).append(row)
        if i == 0 and (core.state_bytes() != want or whole.state_bytes() != want):
            raise SystemExit("STATE MISMATCH (%s)" % name)
    fields = ("ingest_ms", "exchange_ms", "commit_ms", "share_total_ms") + tuple(e + "_kernel_ms" for e in EVENTS)
    res["share"] = {f: median(share_rows, f) for f in fields}
    res["unsharded"] = {f: median(whole_rows, f) for f in ("ingest_ms",) + tuple(e + "_kernel_ms" for e in EVENTS)}
    res["share_over_unsharded"] = round(res["share"]["share_total_ms"] / res["unsharded"]["ingest_ms"], 4)
    res["exchange_bytes_per_rank"] = 16 * cap + 16 if pn else 40
    res["projection_n8_step_ms"] = {"value": res["share"]["share_total_ms"],
                                    "note": "projection: rank 0's share only; the collectives are not measured on one GPU"}
    core.close()
    whole.close()
    del mine, files, offs
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12, help="timed iterations (at least 12 for the record)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--versions", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = crdtenc.Context(0)
    key = bytes(np.random.default_rng(7).integers(0, 256, 32, dtype=np.uint8))
    actors = bench.actors_table()
    res = {name: bench_kind(ctx, name, key, actors, args, dev) for name in ("pncounter", "lwwreg")}
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
