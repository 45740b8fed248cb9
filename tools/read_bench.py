#!/usr/bin/env python3
"""The with_state reads beside the only read the library had before them, ce_core_state_bytes.

Two cores, one process: the GSet of tools/gset_state_bench.py (2^20 random 64-bit members) and an
Orswot of C3's member and actor counts (100k members, 4096 actors, 2-4 dots per member).  Per core:

    contains      ce_core_set_contains_device over 2^20 queries in HBM, half of them present, shuffled
    set_len       ce_core_set_len
    members       ce_core_set_members_device into a buffer in HBM
    member_clocks ce_core_orswot_member_clocks for 1024 present members (Orswot only)
    state_bytes   ce_core_state_bytes: what a client had to call (and then parse) for any of these

The reads and state_bytes alternate, --steps times each after --warmup; call times are a host clock
around calls that end in a wait for the stream (median, least, greatest); kernel times are the
library's HIP event regions (ce_ctx_set_timing), mean per launch, taken in a second pass so the
events do not sit in the timed calls.  An Orswot read after a change of the tables rebuilds the
per-handle live flags first: that first call is timed apart (a one-member local op before it).
probes/s = queries over the contains kernel's time; the bytes it must touch are one 64-byte sector
per probe at best (counted from the shapes, not measured).  One JSON line.

    python tools/read_bench.py --steps 12 --warmup 3 --out profiles/reads.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "crdt-enc_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import crdtenc  # noqa: E402
import gset_model as gm  # noqa: E402
from gset_state_bench import encode_members  # noqa: E402
from oracle import crdts as C  # noqa: E402

APP = bytes.fromhex("aadfd5a66e194b24a8024fa27c72f20c")
N_QUERIES = 1 << 20
N_CLOCKS = 1024


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(ts[len(ts) // 2] * 1e3, 4), "min_ms": round(ts[0] * 1e3, 4),
            "max_ms": round(ts[-1] * 1e3, 4), "n": len(ts)}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def queries_for(rng, members):
    """2^20 queries, half drawn from the members, half random (absent but for chance), shuffled"""
    q = np.concatenate([rng.choice(members, N_QUERIES // 2), rng.integers(0, 1 << 64, N_QUERIES // 2, dtype=np.uint64)])
    rng.shuffle(q)
    return q


def run_core(ctx, core, members, rng, args, dev, kernels, orswot):
    q = queries_for(rng, members)
    want = np.isin(q, members).astype(np.uint8)
    d_q = torch.from_numpy(q.view(np.int64)).to(dev)
    d_out = torch.zeros(N_QUERIES, dtype=torch.uint8, device=dev)
    d_mem = torch.zeros(len(members) + 64, dtype=torch.int64, device=dev)
    clocks_of = [int(x) for x in rng.choice(members, N_CLOCKS, replace=False)]
    torch.cuda.synchronize()

    def contains():
        rc = core.contains_device(d_q.data_ptr(), N_QUERIES, d_out.data_ptr())
        if rc:
            raise crdtenc.CeError(rc, ctx.last_error())

    def members_dev():
        rc, n = core.members_device(d_mem.data_ptr(), d_mem.numel())
        if rc or n != len(members):
            raise crdtenc.CeError(rc, "members: %d of %d" % (n, len(members)))

    calls = {"contains": contains, "set_len": core.set_len, "members": members_dev, "state_bytes": core.state_bytes}
    if orswot:
        calls["member_clocks"] = lambda: core.orswot_member_clocks(clocks_of)
    out = {"members": int(len(members)), "queries": N_QUERIES}
    if orswot:  # the first read after the tables changed: the flag build and the answer
        core.apply_ops(C.enc_orswot_ops([("Add", (core.info_actor(), 1), [int(members[0])])]))
        core.settle()
        out["contains_after_change_ms"] = round(timed(contains) * 1e3, 4)
    contains()
    members_dev()
    torch.cuda.synchronize()
    assert bytes(d_out.cpu().numpy()) == bytes(want), "contains != numpy isin"
    assert (d_mem.cpu().numpy().view(np.uint64)[:len(members)] == np.sort(members)).all(), "members != sorted"
    assert core.set_len() == len(members)
    out["state_bytes_len"] = len(core.state_bytes())
    ts = {k: [] for k in calls}
    for it in range(args.warmup + args.steps):
        for k, fn in calls.items():                       # (the reads and state_bytes in turn)
            t = timed(fn)
            if it >= args.warmup:
                ts[k].append(t)
    out["call"] = {k: stats(v) for k, v in ts.items()}
    # kernel times: a pass of their own
    ctx.set_timing(True)
    ctx.timing_reset()
    reps = max(3, args.steps // 2)
    for _ in range(reps):
        for fn in calls.values():
            fn()
    if orswot:
        core.apply_ops(C.enc_orswot_ops([("Add", (core.info_actor(), 2), [int(members[1])])]))
        contains()
    ctx.synchronize()
    kt = {}
    for k in kernels:
        ms, cnt = ctx.timing(k)
        if cnt:
            kt[k] = {"mean_ms": round(ms / cnt, 4), "launches": cnt}
    ctx.set_timing(False)
    out["kernel"] = kt
    ck = "ds_contains" if orswot else "gs_contains"
    if ck in kt:
        out["contains_probes_per_s"] = round(N_QUERIES / (kt[ck]["mean_ms"] * 1e-3), 1)
        out["contains_sector_bytes_at_best"] = N_QUERIES * 64 + N_QUERIES * 9   # a sector per probe, the query, the answer
    sb = out["call"]["state_bytes"]["median_ms"]
    out["state_bytes_over"] = {k: round(sb / v["median_ms"], 2) for k, v in out["call"].items() if k != "state_bytes"}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.steps < 12:
        ap.error("medians of at least 12")
    if not torch.cuda.is_available():
        raise SystemExit("read_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    key = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    ctx = crdtenc.Context(0)
    res = {"bench": "reads", "steps": args.steps, "warmup": args.warmup,
           "sources": {"call": "host clock around a call that ends in a stream wait",
                       "kernel": "the library's HIP event regions (ce_ctx_set_timing), mean per launch",
                       "contains_sector_bytes_at_best": "counted from the shapes, not measured"}}
    # GSet: 2^20 random members, merged from a StateWrapper in HBM
    members = np.unique(rng.integers(1, 1 << 64, 1 << 20, dtype=np.uint64))
    sw = gm.serialize(C.VClock(), gm.GSet())[:-1] + encode_members(members)
    core = crdtenc.Core(ctx, kind=crdtenc.STATE_GSET, supported=[APP], current_data_version=APP)
    core.set_latest_key(key)
    d_sw = torch.frombuffer(bytearray(sw), dtype=torch.uint8).to(dev)
    torch.cuda.synchronize()
    rc = core.merge_state_device(d_sw.data_ptr(), len(sw))
    if rc:
        raise crdtenc.CeError(rc, ctx.last_error())
    res["gset"] = run_core(ctx, core, members, rng, args, dev, ("gs_contains", "gset_sort", "gset_write"), False)
    core.close()
    # Orswot: 100k members, 4096 actors, 2-4 dots a member
    actors = [bytes(rng.integers(0, 256, 16, dtype=np.uint8)) for _ in range(4096)]
    members = np.unique(rng.integers(1, 1 << 64, 100_000, dtype=np.uint64))
    st = C.Orswot()
    ai = rng.integers(0, 4096, (len(members), 4))
    nd = rng.integers(2, 5, len(members))
    for i, m in enumerate(members):
        st.entries[int(m)] = C.VClock({actors[a]: 1 + (int(m) + j) % 7 for j, a in enumerate(ai[i, :nd[i]])})
    st.clock = C.VClock({a: 8 for a in actors})
    sw = C.serialize("orswot", C.VClock(), st)
    core = crdtenc.Core(ctx, kind=crdtenc.STATE_ORSWOT, supported=[APP], current_data_version=APP)
    core.set_latest_key(key)
    rc = core.merge_state(sw)
    if rc:
        raise crdtenc.CeError(rc, ctx.last_error())
    res["orswot"] = run_core(ctx, core, members, rng, args, dev,
                             ("ds_contains", "ds_member_live", "ds_members", "ds_member_clocks"), True)
    res["orswot"]["dots"] = sum(len(e.dots) for e in st.entries.values())
    core.close()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
