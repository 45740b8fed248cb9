#!/usr/bin/env python3
"""The sharded GSet<u64> ingest at the C2 shape, rank 0 of a world of 8, on one GPU.

The batch is tools/gset_bench.py's: 1,048,576 op files of 4 KiB, 451 cf members each from a pool
of 2^20 random 64-bit ids, 4096 writers x 256 versions, from an empty set.  It is partitioned by
op-file address (crdtenc.shard_owners, world 8).  This process plays rank 0 and times its own
share through the three calls of the sharded path:

    ce_core_gset_ingest_ops_device_sharded   (the fused open over 1/8 of the files; pending)
    ce_core_gset_pending_members             (the pending batch as a u64 column)
    ce_core_gset_pending_commit              (local batch + the other seven ranks' columns)

The other seven shares' pending columns are produced UNTIMED by a second core on the same GPU
(each from an empty set, as every rank starts).  The windows are the whole batch's (every writer's
versions 0..255 present: hi = 256, no flags), set directly; the two all-reduces and the column
all-gather of shard.ingest_gset_sharded are NOT measured here -- one GPU has no fabric.

The commit's remote inserts are timed in both forms, interleaved step by step in this process:
one k_gs_insert_parts launch over the seven columns, and seven back-to-back k_gs_insert launches
(CE_GSET_PART_LAUNCHES=1).  Beside them: the unsharded 1M-file ingest (ce_core_ingest_ops_device)
and the unsharded whole step (reset + ce_core_compact_ops_device_into) of the same process.
Last, both ingests against a committed set that already holds the whole pool (known_*): no member
is new, so nothing is claimed; what is left is the probing, which divides by the file count.

Per step after the warm-up steps (which settle the table sizes): wall-clock ms of each call (each
is complete on return) and the library's HIP-event ms of the kernels inside.

    python tools/gset_shard_bench.py --steps 8 --warmup 2 --out profiles/gset_sharded.json
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
import gset_bench as gb  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "tests"))
WORLD = 8
EVENTS = ("gate", "open_setup", "open_fold_small", "segments_open", "finalize_open", "decode_gset", "gset_export",
          "gset_commit", "gset_parts")


def share_of(files, offs_len, sel, fa, fv, dev):
    """the files of `sel` (indices, ascending) gathered into one blob, with their metadata"""
    file_len = offs_len
    idx = torch.from_numpy(sel).to(dev)
    blob = files[: fa.numel() * file_len].view(-1, file_len)[idx].reshape(-1)
    blob = torch.cat([blob, torch.zeros(64, dtype=torch.uint8, device=dev)])
    offs = torch.arange(len(sel) + 1, dtype=torch.int64, device=dev) * file_len
    d = dict(files=blob, offs=offs, n=len(sel), blob_len=len(sel) * file_len, fa=fa[idx].contiguous(),
             fv=fv[idx].contiguous())
    torch.cuda.synchronize()
    return d


def ingest(core, d, W, hi):
    rc = core.gset_ingest_ops_device_sharded(d["files"].data_ptr(), d["offs"].data_ptr(), d["n"], d["blob_len"], W,
                                             d["fa"].data_ptr(), d["fv"].data_ptr(), hi.data_ptr())
    if rc:
        raise crdtenc.CeError(rc, core.ctx.last_error())


def export(core, dev):
    rc, n = core.gset_pending_members(None, 0)
    buf = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    if n:
        rc, n = core.gset_pending_members(buf.data_ptr(), n)
        if rc:
            raise crdtenc.CeError(rc, core.ctx.last_error())
    return buf, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6, help="timed steps (alternating the two insert forms)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--versions", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = crdtenc.Context(0)
    key = bytes(np.random.default_rng(7).integers(0, 256, 32, dtype=np.uint8))
    actors = bench.actors_table()
    n = N_ACTORS * args.versions
    files, offs, blen, pool = gb.build_gset_files(ctx, key, n, dev, seed=4321)
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
        c = crdtenc.Core(ctx, kind=crdtenc.STATE_GSET, supported=[APP], current_data_version=APP)
        c.set_latest_key(key)
        return c
    res = {"files": n, "world": WORLD, "members_per_file": gb.K_MEMBERS, "pool": gb.POOL, "steps": args.steps,
           "warmup": args.warmup, "share_files": [int(x) for x in np.bincount(own, minlength=WORLD)]}
    # the other seven ranks' pending columns: untimed, a second core, each from an empty set
    other = core_of()
    cols = []
    for r in range(1, WORLD):
        d = share_of(files, file_len, np.nonzero(own == r)[0], fa, fv, dev)
        other.reset()
        ingest(other, d, W, hi)
        cols.append(export(other, dev))
        del d
    other.close()
    torch.cuda.empty_cache()
    res["remote_members"] = [k for _, k in cols]
    res["remote_column_bytes"] = [8 * k for _, k in cols]
    parts, counts = [t.data_ptr() for t, _ in cols], [k for _, k in cols]
    # rank 0: its share through the three calls
    mine = share_of(files, file_len, np.nonzero(own == 0)[0], fa, fv, dev)
    core = core_of()
    want = gb.expected_gset_state(actors, args.versions, pool)
    rows = {"parts": [], "launches": []}
    for i in range(args.warmup + args.steps):
        form = "launches" if i % 2 else "parts"
        if form == "launches":
            os.environ["CE_GSET_PART_LAUNCHES"] = "1"
        else:
            os.environ.pop("CE_GSET_PART_LAUNCHES", None)
        core.reset()
        ctx.synchronize()
        ctx.timing_reset()
        ctx.set_timing_only(None)
        ctx.set_timing(True)
        t0 = time.perf_counter()
        ingest(core, mine, W, hi)
        t1 = time.perf_counter()
        buf, k = export(core, dev)
        t2 = time.perf_counter()
        rc = core.gset_pending_commit(True, parts, counts)
        t3 = time.perf_counter()
        ctx.set_timing(False)
        if rc:
            raise crdtenc.CeError(rc, ctx.last_error())
        if i < args.warmup + 2 and core.state_bytes() != want:   # once per form
            raise SystemExit("STATE MISMATCH (sharded, %s)" % form)
        if i < args.warmup:
            continue
        row = {"ingest_ms": (t1 - t0) * 1e3, "export_ms": (t2 - t1) * 1e3, "commit_ms": (t3 - t2) * 1e3,
               "local_members": k}
        row.update({e: ctx.timing(e)[0] for e in EVENTS})
        rows[form].append(row)
    os.environ.pop("CE_GSET_PART_LAUNCHES", None)

    def mean(form, f):
        return round(statistics.mean(r[f] for r in rows[form]), 4)
    both = rows["parts"] + rows["launches"]
    res["local_members"] = both[0]["local_members"]
    res["local_column_bytes"] = 8 * both[0]["local_members"]
    res["sharded_ingest_ms"] = round(statistics.mean(r["ingest_ms"] for r in both), 4)
    res["sharded_kernel_ms"] = {e: round(statistics.mean(r[e] for r in both), 4) for e in EVENTS[:6]}
    res["export_ms"] = round(statistics.mean(r["export_ms"] for r in both), 4)
    res["export_kernel_ms"] = round(statistics.mean(r["gset_export"] for r in both), 4)
    for form in rows:
        res["commit_" + form] = {"commit_ms": mean(form, "commit_ms"), "move_kernel_ms": mean(form, "gset_commit"),
                                 "insert_kernel_ms": mean(form, "gset_parts"),
                                 "insert_kernel_ms_each": [round(r["gset_parts"], 4) for r in rows[form]]}
    res["commit_refolds"] = core.path_count("gset_refolds")
    res["committed_grows"] = core.path_count("gset_grows")
    # the same share against a committed set that already holds the pool (a reset, then the pool
    # merged in as a state: next_op_versions stay 0, so every file is still gated in): every probe
    # is a hit in the committed table, nothing is claimed and nothing is pending
    import gset_model as gm
    from oracle.crdts import VClock
    known = gm.serialize(VClock(), gm.GSet(int(x) for x in np.unique(pool)))

    def steady(c, run):
        out = []
        for i in range(args.warmup + args.steps):
            c.reset()
            if c.merge_state(known):
                raise SystemExit("merge_state failed")
            ctx.synchronize()
            ctx.timing_reset()
            ctx.set_timing_only("open_fold_small")
            ctx.set_timing(True)
            t0 = time.perf_counter()
            run(c)
            ctx.synchronize()
            t1 = time.perf_counter()
            ctx.set_timing(False)
            if i >= args.warmup:
                out.append(((t1 - t0) * 1e3, ctx.timing("open_fold_small")[0]))
        return round(statistics.mean(x for x, _ in out), 4), round(statistics.mean(y for _, y in out), 4)

    def run_sharded(c):
        ingest(c, mine, W, hi)
        if c.gset_pending_members(None, 0) != (0, 0):
            raise SystemExit("members pending against a set that holds the pool")
        c.gset_pending_commit(True, parts, counts)
    res["known_sharded_ingest_ms"], res["known_sharded_fused_ms"] = steady(core, run_sharded)
    core.close()
    del mine
    torch.cuda.empty_cache()
    # the unsharded 1M-file ingest and whole step of the same process
    s = gb.Step(ctx, crdtenc.STATE_GSET, files, offs, n, blen, actors, args.versions, dev, 9 * gb.POOL)
    s.set_key(key)
    ing = []
    for i in range(args.warmup + args.steps):
        s.core.reset()
        ctx.synchronize()
        t0 = time.perf_counter()
        rc = s.core.ingest_ops_device(files.data_ptr(), offs.data_ptr(), n, blen, s.actor_bytes, s.fa.data_ptr(),
                                      s.fv.data_ptr())
        ctx.synchronize()
        if rc:
            raise crdtenc.CeError(rc, ctx.last_error())
        if i >= args.warmup:
            ing.append((time.perf_counter() - t0) * 1e3)

    def run_unsharded(c):
        rc = c.ingest_ops_device(files.data_ptr(), offs.data_ptr(), n, blen, s.actor_bytes, s.fa.data_ptr(),
                                 s.fv.data_ptr())
        if rc:
            raise crdtenc.CeError(rc, ctx.last_error())
    res["known_unsharded_ingest_ms"], res["known_unsharded_fused_ms"] = steady(s.core, run_unsharded)
    ms, step_ms = s.run(args.steps, 1, None, ("open_fold_small",))
    if s.core.state_bytes() != want:
        raise SystemExit("STATE MISMATCH (unsharded)")
    res["unsharded_ingest_ms"] = round(statistics.mean(ing), 4)
    res["unsharded_step_ms"] = round(step_ms, 4)
    res["unsharded_fused_ms"] = round(ms["open_fold_small"], 4)
    s.core.close()
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
