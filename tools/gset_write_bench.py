#!/usr/bin/env python3
"""GSet op files written from a member column in HBM, beside the host route.

One process writes 2^16 files of 453 cf members each from one u64 column (29.7 M members, 238 MB)
resident in HBM, with fixed nonces, into one core without storage.  Two routes in turn, their order
swapped from one iteration to the next:

    device   ce_core_gset_apply_members_device: sized, encoded, sealed and inserted on the device
    host     ce_core_apply_ops_batch over the same vectors, their msgpack pre-encoded on the host
             (the encode is timed on its own, outside the call: numpy, one thread)

Both routes insert the same members into the same set (the table grows in the warm-up), seal under
the same nonces and must give the same files; the device route's bytes are compared with the host
route's once, after the clock.  Call times are host clock around calls that end in a wait for the
stream, given as the median of the timed calls with the least and the greatest beside it; kernel
times are the library's HIP event regions, mean per call.  One JSON line.

    python tools/gset_write_bench.py --steps 12 --warmup 2 --out profiles/gset_write.json
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "crdt-enc_amd"))
import crdtenc  # noqa: E402

APP = bytes.fromhex("aadfd5a66e194b24a8024fa27c72f20c")
PER_FILE = crdtenc.GSET_FILE_MEMBERS
KERNELS = ("gset_apply_sizes", "gset_apply_encode", "gset_apply_insert", "seal_setup", "segments_seal", "finalize_seal")


def host_encode(col, files):
    """to_vec_named(Vec<u64>) of every file's vector, back to back: array16 header, cf elements"""
    body = np.empty((files, 3 + 9 * PER_FILE), np.uint8)
    body[:, 0] = 0xdc
    body[:, 1] = PER_FILE >> 8
    body[:, 2] = PER_FILE & 255
    el = body[:, 3:].reshape(files, PER_FILE, 9)
    el[:, :, 0] = 0xcf
    el[:, :, 1:] = col.astype(">u8").view(np.uint8).reshape(files, PER_FILE, 8)
    return body.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--files", type=int, default=1 << 16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    L = crdtenc.lib()
    ctx = crdtenc.Context(0)
    rng = np.random.default_rng(17)
    key = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    F, n = args.files, args.files * PER_FILE
    col = rng.integers(1 << 32, 1 << 64, n, dtype=np.uint64)     # every member 9 bytes wide
    d_col = torch.from_numpy(col.view(np.int64)).to(dev)
    rc, max_files, max_bytes = crdtenc.gset_apply_bound(n, PER_FILE)
    assert rc == 0 and max_files == F
    d_files = torch.zeros(max_bytes + 64, dtype=torch.uint8, device=dev)
    d_offs = torch.zeros(max_files + 1, dtype=torch.int64, device=dev)
    nonces = ctypes.create_string_buffer(bytes(rng.integers(0, 256, 24 * F, dtype=np.uint8)), 24 * F)
    torch.cuda.synchronize()
    core = crdtenc.Core(ctx, kind=crdtenc.STATE_GSET, supported=[APP], current_data_version=APP)
    core.set_latest_key(key)

    enc_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        blob = host_encode(col, F)
        enc_ms.append((time.perf_counter() - t0) * 1e3)
    ops_len = 3 + 9 * PER_FILE
    offs = (np.arange(F + 1, dtype=np.uint64) * np.uint64(ops_len))
    host_files = [None]

    def device():
        nf, nb = ctypes.c_uint32(0), ctypes.c_uint64(0)
        rc = L.ce_core_gset_apply_members_device(
            core.p, ctypes.c_void_p(d_col.data_ptr()), ctypes.c_uint64(n), ctypes.c_uint32(PER_FILE),
            ctypes.c_uint32(0), nonces, ctypes.c_void_p(d_files.data_ptr()), ctypes.c_uint64(max_bytes),
            ctypes.c_void_p(d_offs.data_ptr()), ctypes.byref(nf), ctypes.byref(nb))
        if rc or nf.value != F or nb.value != max_bytes:
            raise crdtenc.CeError(rc, ctx.last_error())

    def host():
        fb, fo = crdtenc.Buf(), crdtenc.Buf()
        rc = L.ce_core_apply_ops_batch(core.p, ctypes.c_void_p(blob.ctypes.data), ctypes.c_void_p(offs.ctypes.data),
                                       ctypes.c_uint32(F), nonces, ctypes.byref(fb), ctypes.byref(fo))
        if rc:
            raise crdtenc.CeError(rc, ctx.last_error())
        if host_files[0] is None:
            host_files[0] = ctypes.string_at(fb.data, fb.len)
        L.ce_buf_free(ctypes.byref(fb))
        L.ce_buf_free(ctypes.byref(fo))

    wall = {"device": [], "host": []}
    kern = {"device": {}, "host": {}}
    routes = {"device": device, "host": host}
    for it in range(args.warmup + args.steps):
        for name in (("device", "host") if it % 2 == 0 else ("host", "device")):
            ctx.synchronize()
            torch.cuda.synchronize()
            ctx.timing_reset()
            ctx.set_timing(it >= args.warmup)
            t0 = time.perf_counter()
            routes[name]()
            ctx.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            ctx.set_timing(False)
            if it >= args.warmup:
                wall[name].append(dt)
                for k in KERNELS:
                    kern[name][k] = kern[name].get(k, 0.0) + ctx.timing(k)[0] / args.steps
    if bytes(d_files[:max_bytes].cpu().numpy()) != host_files[0]:
        raise SystemExit("FILES MISMATCH")
    if core.path_count("gset_apply_device_files") != F * (args.warmup + args.steps):
        raise SystemExit("PATH COUNT MISMATCH")

    def stats(v):
        return {"median_ms": round(float(np.median(v)), 3), "min_max_ms": [round(min(v), 3), round(max(v), 3)]}
    clear_bytes = F * (16 + ops_len)
    enc_k = kern["device"]["gset_apply_encode"]
    res = {"files": F, "per_file": PER_FILE, "members": n, "column_bytes": n * 8, "clear_bytes": clear_bytes,
           "sealed_bytes": max_bytes, "steps": args.steps, "warmup": args.warmup,
           "device_call": stats(wall["device"]), "host_call": stats(wall["host"]),
           "host_encode_ms": round(float(np.median(enc_ms)), 3),
           "device_kernel_ms": {k: round(v, 4) for k, v in kern["device"].items() if v},
           "host_kernel_ms": {k: round(v, 4) for k, v in kern["host"].items() if v},
           "encoder_clear_GBps": round(clear_bytes / (enc_k * 1e-3) / 1e9, 2),
           "encoder_read_plus_write_GBps": round((n * 8 + clear_bytes) / (enc_k * 1e-3) / 1e9, 2),
           "device_over_host": round(float(np.median(wall["device"]) / np.median(wall["host"])), 5),
           "set_len": core.set_len(), "grows": core.path_count("gset_grows")}
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    core.close()
    ctx.close()


if __name__ == "__main__":
    main()
