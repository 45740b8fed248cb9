#!/usr/bin/env python3
"""GSet<u64> at the C2 shape, beside the GCounter C2 step of the same process and box.

Both batches: 1,048,576 op files of 4 KiB (4085 B of plaintext), 4096 writers x 256 versions in
load_ops order, resident in HBM, sealed on the GPU; the step is bench.py's single-GPU step
(ce_core_reset + ce_core_compact_ops_device_into).  A GCounter file holds its writer's own 107
Dots at ce width (bench.py variant A); a GSet file holds 451 members at cf width (9 B each) drawn
from a pool of 1,048,576 random 64-bit ids, and 7 trailing bytes that from_slice ignores, so both
plaintexts -- and the AEAD work -- are the same length.  Every step starts from an empty set (the
reset), so each one claims the pool's 1,048,576 members once and finds them ~450 times more.

A GSet step is the fused open (open_fold_small: k_open_fold_v3's GSet form decodes each file in
LDS and probes the tables), then the commit (gset_commit), the collect and sort (gset_sort), the
writer (gset_write) and the seal.  The JSON line gives the whole step, each timed region's ms per
step from the library's HIP events (what is left of the step is not attributed), the members
decoded per second of step, and the ratios of the step and of the fused kernel to GCounter's.

    python tools/gset_bench.py --steps 5 --warmup 3 --out profiles/gset_c2.json
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

PT = bench.pt_len("a")                       # 4085
K_MEMBERS = (PT - 19) // 9                   # 451
POOL = 1 << 20
GSET_KERNELS = ("open_setup", "open_fold_small", "segments_open", "finalize_open", "decode_gset", "gset_commit",
                "gset_sort", "gset_write", "seal_setup", "segments_seal", "finalize_seal")


def build_gset_files(ctx, key, n, dev, seed):
    """n files of dc <451> then 451 x (cf <member, big-endian>), members drawn from the pool"""
    file_len = 16 + crdtenc.sealed_len(PT)
    files = torch.empty(n * file_len + 64, dtype=torch.uint8, device=dev)
    offs = torch.arange(n + 1, dtype=torch.int64, device=dev) * file_len
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    hi, lo = (torch.randint(0, 1 << 32, (POOL,), dtype=torch.int64, device=dev, generator=gen) for _ in range(2))
    pool = (hi << 32) | lo  # all 64 bits random (as int64: the byte encoding below masks each shift)

    def t(b):
        return torch.tensor(list(b), dtype=torch.uint8, device=dev)
    chunk = 1 << 15
    for c0 in range(0, n, chunk):
        m = min(chunk, n - c0)
        idx = torch.arange(c0, c0 + m, dtype=torch.int64, device=dev)
        clear = torch.zeros((m, PT), dtype=torch.uint8, device=dev)
        clear[:, :16] = t(APP)
        clear[:, 16:19] = t(bytes([0xdc, K_MEMBERS >> 8, K_MEMBERS & 255]))
        val = pool[torch.randint(0, POOL, (m, K_MEMBERS), dtype=torch.int64, device=dev, generator=gen)]
        els = clear[:, 19:19 + K_MEMBERS * 9].view(m, K_MEMBERS, 9)
        els[:, :, 0] = 0xcf
        for b in range(8):
            els[:, :, 1 + b] = ((val >> (8 * (7 - b))) & 255).to(torch.uint8)
        coffs = torch.arange(m + 1, dtype=torch.int64, device=dev) * PT
        nonces = torch.randint(0, 256, (m, 24), dtype=torch.uint8, device=dev, generator=gen)
        ooffs = (idx * file_len).contiguous()
        torch.cuda.current_stream().synchronize()
        ctx.encrypt_batch_device(key, clear.data_ptr(), coffs.data_ptr(), m, nonces.data_ptr(),
                                 files.data_ptr(), ooffs.data_ptr(), outer_version=CORE)
        ctx.synchronize()
    return files, offs, n * file_len, pool.cpu().numpy().view(np.uint64)


def expected_gset_state(actors, versions, pool):
    """every pool member is drawn (473M draws over 2^20 ids): the set is the pool's distinct ids"""
    import gset_model as gm
    from oracle.crdts import VClock
    return gm.serialize(VClock({bytes(a): versions for a in actors}), gm.GSet(int(x) for x in np.unique(pool)))


class Step:
    def __init__(self, ctx, kind, files, offs, n, blob_len, actors, versions, dev, out_bound):
        self.ctx, self.files, self.offs, self.n, self.blob_len = ctx, files, offs, n, blob_len
        self.core = crdtenc.Core(ctx, kind=kind, supported=[APP], current_data_version=APP)
        self.actor_bytes = b"".join(bytes(a) for a in actors)
        self.fa = torch.from_numpy(np.repeat(np.arange(actors.shape[0], dtype=np.int32), versions)).to(dev)
        self.fv = torch.from_numpy(np.tile(np.arange(versions, dtype=np.int64), actors.shape[0])).to(dev)
        bound = 16 + crdtenc.sealed_len(out_bound + 128 + 81 * self.core.dense_capacity())
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

    def run(self, steps, warmup, only, names):
        for _ in range(warmup):
            self.step()
        torch.cuda.synchronize()
        self.ctx.timing_reset()
        self.ctx.set_timing_only(only)
        self.ctx.set_timing(True)
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step()
        torch.cuda.synchronize()
        step_ms = (time.perf_counter() - t0) * 1e3 / steps
        self.ctx.set_timing(False)
        return {k: self.ctx.timing(k)[0] / steps for k in names}, step_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--versions", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = crdtenc.Context(0)
    key = bytes(np.random.default_rng(7).integers(0, 256, 32, dtype=np.uint8))
    actors = bench.actors_table()
    n = N_ACTORS * args.versions
    res = {"files": n, "plaintext_bytes": PT, "writers": N_ACTORS, "gcounter_dots_per_file": bench.K_DOTS["a"],
           "gset_members_per_file": K_MEMBERS, "gset_pool": POOL, "steps": args.steps, "warmup": args.warmup}
    # GCounter C2: the fused kernel alone, as tools/pncounter_bench.py times it
    files, offs, n_g, blen, _ = bench.build_files(ctx, key, actors, actors, args.versions, dev, seed=1234)
    s = Step(ctx, crdtenc.STATE_GCOUNTER, files, offs, n_g, blen, actors, args.versions, dev, 0)
    s.set_key(key)
    ms, step_ms = s.run(args.steps, args.warmup, "open_fold_small", ["open_fold_small"])
    if s.core.state_bytes() != bench.expected_state(actors, args.versions):
        raise SystemExit("STATE MISMATCH (gcounter)")
    res["gcounter_ms"] = round(ms["open_fold_small"], 4)
    res["gcounter_step_ms"] = round(step_ms, 4)
    s.core.close()
    del s, files, offs
    torch.cuda.empty_cache()
    # GSet at the same shape
    files, offs, blen, pool = build_gset_files(ctx, key, n, dev, seed=4321)
    s = Step(ctx, crdtenc.STATE_GSET, files, offs, n, blen, actors, args.versions, dev, 9 * POOL)
    s.set_key(key)
    ms, step_ms = s.run(args.steps, args.warmup, None, GSET_KERNELS)
    if s.core.state_bytes() != expected_gset_state(actors, args.versions, pool):
        raise SystemExit("STATE MISMATCH (gset)")
    res["gset_step_ms"] = round(step_ms, 4)
    res["gset_kernel_ms"] = {k: round(v, 4) for k, v in ms.items()}
    res["gset_members_per_s"] = round(n * K_MEMBERS / (step_ms * 1e-3))
    res["gset_uniform_files"] = s.core.path_count("gset_uniform_files")
    res["gset_general_files"] = s.core.path_count("gset_general_files")
    res["gset_fused_files"] = s.core.path_count("gset_fused_files")
    res["gset_refolds"] = s.core.path_count("gset_refolds")
    res["step_ratio"] = round(step_ms / res["gcounter_step_ms"], 4)
    res["fused_ratio"] = round(ms["open_fold_small"] / res["gcounter_ms"], 4)
    s.core.close()
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
