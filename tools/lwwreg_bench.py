#!/usr/bin/env python3
"""LWWReg at the C2 shape, beside the GCounter C2 step of the same process and box.

Both batches: 1,048,576 op files of 4 KiB (4085 B of plaintext), 4096 writers x 256 versions in
load_ops order, resident in HBM, sealed on the GPU; the step is bench.py's single-GPU step
(ce_core_reset + ce_core_compact_ops_device_into).  A GCounter file holds its writer's own 107
Dots at ce width (bench.py variant A); an LWWReg file holds 135 ops of 30 bytes (val and marker
both at cf width) and 16 trailing bytes that from_slice ignores, so both plaintexts -- and the
AEAD work -- are the same length.  Op k of version v has the marker 2^40 + 135 v + k whoever wrote
it, so every writer's last file ends on the batch's largest marker: a 4096-way tie across files,
which the lowest file index (writer 0's) wins.

Prints one JSON line {gcounter_ms, lwwreg_ms, lwwreg_reduce_ms, ratio, ...} (fused-kernel time and
k_lww_reduce's two launches per step from the library's HIP events, and the whole step beside
them) and writes it to --out; --merge FILE puts that file's JSON (the headline's A/B runs) under
"headline_ab" of the same line.

    python tools/lwwreg_bench.py --steps 10 --warmup 2 --out profiles/lwwreg_c2.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import bench  # noqa: E402
from bench import APP, CORE, N_ACTORS, crdtenc  # noqa: E402
from pncounter_bench import Step  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "tests"))

LW_OP = 30                                   # 82 a3"val" cf <8> a6"marker" cf <8>
PT = bench.pt_len("a")                       # 4085
K_OPS = (PT - 19) // LW_OP                   # 135


def build_lww_files(ctx, key, n_actors, versions, dev, seed):
    """bench.build_files for Vec<LWWReg>: writer i // versions, version i % versions; op k of file
    i has val 2^41 + i K + k and marker 2^40 + v K + k."""
    n = n_actors * versions
    file_len = 16 + crdtenc.sealed_len(PT)
    files = torch.empty(n * file_len + 64, dtype=torch.uint8, device=dev)
    offs = torch.arange(n + 1, dtype=torch.int64, device=dev) * file_len

    def t(b):
        return torch.tensor(list(b), dtype=torch.uint8, device=dev)
    head, mid = t(b"\x82\xa3val\xcf"), t(b"\xa6marker\xcf")
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    kk = torch.arange(K_OPS, dtype=torch.int64, device=dev)
    chunk = 1 << 16
    for c0 in range(0, n, chunk):
        m = min(chunk, n - c0)
        idx = torch.arange(c0, c0 + m, dtype=torch.int64, device=dev)
        v = idx % versions
        clear = torch.zeros((m, PT), dtype=torch.uint8, device=dev)
        clear[:, :16] = t(APP)
        clear[:, 16:19] = t(bytes([0xdc, K_OPS >> 8, K_OPS & 255]))
        ops = clear[:, 19:19 + K_OPS * LW_OP].view(m, K_OPS, LW_OP)
        ops[:, :, 0:6] = head
        ops[:, :, 14:22] = mid
        val = (1 << 41) + idx[:, None] * K_OPS + kk[None, :]
        mark = (1 << 40) + v[:, None] * K_OPS + kk[None, :]
        for b in range(8):
            ops[:, :, 6 + b] = ((val >> (8 * (7 - b))) & 255).to(torch.uint8)
            ops[:, :, 22 + b] = ((mark >> (8 * (7 - b))) & 255).to(torch.uint8)
        coffs = torch.arange(m + 1, dtype=torch.int64, device=dev) * PT
        nonces = torch.randint(0, 256, (m, 24), dtype=torch.uint8, device=dev, generator=gen)
        ooffs = (idx * file_len).contiguous()
        torch.cuda.current_stream().synchronize()
        ctx.encrypt_batch_device(key, clear.data_ptr(), coffs.data_ptr(), m, nonces.data_ptr(),
                                 files.data_ptr(), ooffs.data_ptr(), outer_version=CORE)
        ctx.synchronize()
    return files, offs, n, n * file_len


def expected_lww_state(actors, versions):
    """closed form: writer 0's last file holds the first of the ops with the largest marker"""
    import lwwreg_model as lm
    from oracle.crdts import VClock
    last = (versions - 1) * K_OPS + K_OPS - 1
    return lm.serialize(VClock({bytes(a): versions for a in actors}), lm.LWWReg((1 << 41) + last, (1 << 40) + last))


def reduce_ms(s, steps):
    """k_lww_reduce's two launches per step, in a pass of their own"""
    s.ctx.timing_reset()
    s.ctx.set_timing_only("lww_reduce")
    s.ctx.set_timing(True)
    for _ in range(steps):
        s.step()
    torch.cuda.synchronize()
    s.ctx.set_timing(False)
    ms, cnt = s.ctx.timing("lww_reduce")
    return ms / max(cnt, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--versions", type=int, default=256)
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", default=None, help="a JSON file to carry under headline_ab")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = crdtenc.Context(0)
    key = bytes(np.random.default_rng(7).integers(0, 256, 32, dtype=np.uint8))
    actors = bench.actors_table()
    res = {"files": N_ACTORS * args.versions, "plaintext_bytes": PT, "writers": N_ACTORS,
           "gcounter_dots_per_file": bench.K_DOTS["a"], "lwwreg_ops_per_file": K_OPS, "lwwreg_op_bytes": LW_OP,
           "steps": args.steps, "warmup": args.warmup}
    for name, kind in (("gcounter", crdtenc.STATE_GCOUNTER), ("lwwreg", crdtenc.STATE_LWWREG)):
        if kind == crdtenc.STATE_GCOUNTER:
            files, offs, n, blen, _ = bench.build_files(ctx, key, actors, actors, args.versions, dev, seed=1234)
            want = bench.expected_state(actors, args.versions)
        else:
            files, offs, n, blen = build_lww_files(ctx, key, actors.shape[0], args.versions, dev, seed=4321)
            want = expected_lww_state(actors, args.versions)
        s = Step(ctx, kind, files, offs, n, blen, actors, args.versions, dev)
        s.set_key(key)
        fused_ms, step_ms = s.run(args.steps, args.warmup)
        if s.core.state_bytes() != want:
            raise SystemExit("STATE MISMATCH (%s)" % name)
        res[name + "_ms"] = round(fused_ms, 4)
        res[name + "_step_ms"] = round(step_ms, 4)
        if kind == crdtenc.STATE_LWWREG:
            res["lwwreg_reduce_ms"] = round(reduce_ms(s, args.steps), 4)
            res["lwwreg_paths"] = {k: s.core.path_count(k) for k in
                                   ("open_v3_lww", "lww_fused_files", "lww_uniform_files", "lww_general_files",
                                    "lww_page_files")}
        s.core.close()
        del s, files, offs
        torch.cuda.empty_cache()
    res["ratio"] = round(res["lwwreg_ms"] / res["gcounter_ms"], 4)
    res["step_ratio"] = round(res["lwwreg_step_ms"] / res["gcounter_step_ms"], 4)
    if args.merge:
        with open(args.merge) as f:
            res["headline_ab"] = json.load(f)
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
