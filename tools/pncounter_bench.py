#!/usr/bin/env python3
"""PNCounter at the C2 shape, beside the GCounter C2 step of the same process and box.

Both batches: 1,048,576 op files of 4 KiB (4085 B of plaintext), 4096 writers x 256 versions in
load_ops order, resident in HBM, sealed on the GPU; the step is bench.py's single-GPU step
(ce_core_reset + ce_core_compact_ops_device_into).  A GCounter file holds its writer's own 107
Dots at ce width (bench.py variant A); a PNCounter file holds its writer's own 79 Ops at ce width
(51 B each), Pos and Neg alternating, and 37 trailing bytes that from_slice ignores, so both
plaintexts -- and the AEAD work -- are the same length.

Prints one JSON line {gcounter_ms, pncounter_ms, ratio} (fused-kernel time per step from the
library's HIP events, and the whole step beside it) and writes it to --out.

    python tools/pncounter_bench.py --steps 10 --warmup 2 --out profiles/pncounter_c2.json
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
import bench  # noqa: E402
from bench import APP, CORE, N_ACTORS, crdtenc  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "tests"))

PN_OP = 51                                   # 82 a3"dot" <38-byte Dot, ce counter> a3"dir" a3"Pos"|"Neg"
PT = bench.pt_len("a")                       # 4085
K_OPS = (PT - 19) // PN_OP                   # 79


def build_pn_files(ctx, key, actors, versions, dev, seed):
    """bench.build_files for Vec<pncounter::Op>: writer i // versions, version i % versions; op k of
    the file is the writer's own, counter 65536 + v K + k + 1, Pos for even k and Neg for odd."""
    n = actors.shape[0] * versions
    file_len = 16 + crdtenc.sealed_len(PT)
    files = torch.empty(n * file_len + 64, dtype=torch.uint8, device=dev)
    offs = torch.arange(n + 1, dtype=torch.int64, device=dev) * file_len
    act = torch.from_numpy(actors).to(dev)

    def t(b):
        return torch.tensor(list(b), dtype=torch.uint8, device=dev)
    head, pre2 = t(b"\x82\xa3dot\x82\xa5actor\xc4\x10"), t(b"\xa7counter\xce")
    tails = torch.stack([t(b"\xa3dir\xa3Pos"), t(b"\xa3dir\xa3Neg")])
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    kk = torch.arange(K_OPS, dtype=torch.int64, device=dev)
    chunk = 1 << 16
    for c0 in range(0, n, chunk):
        m = min(chunk, n - c0)
        idx = torch.arange(c0, c0 + m, dtype=torch.int64, device=dev)
        a_loc, v = idx // versions, idx % versions
        clear = torch.zeros((m, PT), dtype=torch.uint8, device=dev)
        clear[:, :16] = t(APP)
        clear[:, 16:19] = t(bytes([0xdc, K_OPS >> 8, K_OPS & 255]))
        ops = clear[:, 19:19 + K_OPS * PN_OP].view(m, K_OPS, PN_OP)
        ops[:, :, 0:14] = head
        ops[:, :, 14:30] = act[a_loc][:, None, :]
        ops[:, :, 30:39] = pre2
        cval = 65536 + v[:, None] * K_OPS + kk[None, :] + 1
        for b in range(4):
            ops[:, :, 39 + b] = ((cval >> (8 * (3 - b))) & 255).to(torch.uint8)
        ops[:, :, 43:51] = tails[kk & 1][None, :, :]
        coffs = torch.arange(m + 1, dtype=torch.int64, device=dev) * PT
        nonces = torch.randint(0, 256, (m, 24), dtype=torch.uint8, device=dev, generator=gen)
        ooffs = (idx * file_len).contiguous()
        torch.cuda.current_stream().synchronize()
        ctx.encrypt_batch_device(key, clear.data_ptr(), coffs.data_ptr(), m, nonces.data_ptr(),
                                 files.data_ptr(), ooffs.data_ptr(), outer_version=CORE)
        ctx.synchronize()
    return files, offs, n, n * file_len


def expected_pn_state(actors, versions):
    """closed form: the last file's last even / odd op holds each plane's maximum"""
    import pncounter_model as pm
    from oracle.crdts import VClock
    top = 65536 + (versions - 1) * K_OPS
    last_pos = K_OPS - 1 if (K_OPS - 1) % 2 == 0 else K_OPS - 2
    last_neg = K_OPS - 1 if (K_OPS - 1) % 2 == 1 else K_OPS - 2
    st = pm.PNCounter()
    st.p = VClock({bytes(a): top + last_pos + 1 for a in actors})
    st.n = VClock({bytes(a): top + last_neg + 1 for a in actors})
    return pm.serialize(VClock({bytes(a): versions for a in actors}), st)


class Step:
    def __init__(self, ctx, kind, files, offs, n, blob_len, actors, versions, dev):
        self.ctx, self.files, self.offs, self.n, self.blob_len = ctx, files, offs, n, blob_len
        self.core = crdtenc.Core(ctx, kind=kind, supported=[APP], current_data_version=APP)
        self.actor_bytes = b"".join(bytes(a) for a in actors)
        self.fa = torch.from_numpy(np.repeat(np.arange(actors.shape[0], dtype=np.int32), versions)).to(dev)
        self.fv = torch.from_numpy(np.tile(np.arange(versions, dtype=np.int64), actors.shape[0])).to(dev)
        bound = 16 + crdtenc.sealed_len(128 + 81 * self.core.dense_capacity())
        self.obuf = torch.empty(bound, dtype=torch.uint8, pin_memory=True).numpy()

    def set_key(self, key):
        self.core.set_latest_key(key)
        self.core.register_actors([self.actor_bytes[i:i + 16] for i in range(0, len(self.actor_bytes), 16)])

    def step(self):
        self.core.reset()
        rc, _, _ = self.core.compact_ops_device_into(self.obuf, self.files.data_ptr(), self.offs.data_ptr(), self.n,
                                                     self.blob_len, self.actor_bytes, self.fa.data_ptr(),
                                                     self.fv.data_ptr())
        if rc:
            raise crdtenc.CeError(rc, self.ctx.last_error())

    def run(self, steps, warmup):
        for _ in range(warmup):
            self.step()
        torch.cuda.synchronize()
        self.ctx.timing_reset()
        self.ctx.set_timing_only("open_fold_small")
        self.ctx.set_timing(True)
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step()
        torch.cuda.synchronize()
        step_ms = (time.perf_counter() - t0) * 1e3 / steps
        self.ctx.set_timing(False)
        ms, cnt = self.ctx.timing("open_fold_small")
        return ms / max(cnt, 1), step_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--versions", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = crdtenc.Context(0)
    key = bytes(np.random.default_rng(7).integers(0, 256, 32, dtype=np.uint8))
    actors = bench.actors_table()
    res = {"files": N_ACTORS * args.versions, "plaintext_bytes": PT, "writers": N_ACTORS,
           "gcounter_dots_per_file": bench.K_DOTS["a"], "pncounter_ops_per_file": K_OPS,
           "steps": args.steps, "warmup": args.warmup}
    for name, kind in (("gcounter", crdtenc.STATE_GCOUNTER), ("pncounter", crdtenc.STATE_PNCOUNTER)):
        if kind == crdtenc.STATE_GCOUNTER:
            files, offs, n, blen, _ = bench.build_files(ctx, key, actors, actors, args.versions, dev, seed=1234)
            want = bench.expected_state(actors, args.versions)
        else:
            files, offs, n, blen = build_pn_files(ctx, key, actors, args.versions, dev, seed=4321)
            want = expected_pn_state(actors, args.versions)
        s = Step(ctx, kind, files, offs, n, blen, actors, args.versions, dev)
        s.set_key(key)
        fused_ms, step_ms = s.run(args.steps, args.warmup)
        if s.core.state_bytes() != want:
            raise SystemExit("STATE MISMATCH (%s)" % name)
        res[name + "_ms"] = round(fused_ms, 4)
        res[name + "_step_ms"] = round(step_ms, 4)
        s.core.close()
        del s, files, offs
        torch.cuda.empty_cache()
    res["ratio"] = round(res["pncounter_ms"] / res["gcounter_ms"], 4)
    res["step_ratio"] = round(res["pncounter_step_ms"] / res["gcounter_step_ms"], 4)
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
