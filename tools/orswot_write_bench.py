#!/usr/bin/env python3
"""Orswot Add-op files written from a member column in HBM, beside the host route.

One process writes 2^14 files from one u64 column resident in HBM, with fixed nonces, into one core
without storage, in two shapes: 28 one-member ops a file (a dot per member) and one 446-member op a
file (add_all).  Two routes in turn, their order swapped from one iteration to the next:

    device   ce_core_orswot_add_members_device: sized, encoded, sealed and folded on the device
    host     ce_core_apply_ops_batch over the same vectors, their msgpack encoded on the host
             (numpy, one thread; timed on its own, outside the call -- the counters move with
             every call, so the vectors are encoded again before each)

The local actor's counter starts at 2^32 and every member is above 2^32, so every integer is nine
bytes wide and the op length is fixed.  Every call adds the same members again under new dots.
After the clock the core is reset twice and each route writes the same call once more from the
same counter: the two routes' files must be identical.  Call times are host clock around calls
that end in a wait for the stream, given as the median of the timed calls with the least and the
greatest beside it; kernel times are the library's HIP event regions, mean per call.  One JSON
object per shape, in one JSON line.

    python tools/orswot_write_bench.py --steps 12 --warmup 2 --out profiles/orswot_write.json
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
C_START = 1 << 32
KERNELS = ("orswot_add_sizes", "orswot_add_encode", "orswot_add_cols", "seal_setup", "segments_seal", "finalize_seal",
           "ds_applied", "ds_part_fold", "ds_add_pairs", "ds_kill", "ds_finalize")


def arr_hdr(n):
    return bytes([0x90 | n]) if n <= 15 else bytes([0xdc, n >> 8, n & 255])


def host_encode(col, files, opf, per_op, actor, c_first):
    """to_vec_named(Vec<orswot::Op>) of every file's vector, back to back: op j carries the counter
    c_first + j, every counter and member in its cf form"""
    head = (b"\x81\xa3Add\x82\xa3dot\x82\xa5actor\xc4\x10" + actor + b"\xa7counter")
    mid = b"\xa7members" + arr_hdr(per_op)
    vh = arr_hdr(opf)
    op_len = len(head) + 9 + len(mid) + 9 * per_op
    ops = np.empty((files * opf, op_len), np.uint8)
    ops[:, :len(head)] = np.frombuffer(head, np.uint8)
    o = len(head)
    ops[:, o] = 0xcf
    ctr = np.uint64(c_first) + np.arange(files * opf, dtype=np.uint64)
    ops[:, o + 1:o + 9] = ctr.astype(">u8").view(np.uint8).reshape(-1, 8)
    o += 9
    ops[:, o:o + len(mid)] = np.frombuffer(mid, np.uint8)
    o += len(mid)
    el = ops[:, o:].reshape(files * opf, per_op, 9)
    el[:, :, 0] = 0xcf
    el[:, :, 1:] = col.astype(">u8").view(np.uint8).reshape(files * opf, per_op, 8)
    body = np.empty((files, len(vh) + opf * op_len), np.uint8)
    body[:, :len(vh)] = np.frombuffer(vh, np.uint8)
    body[:, len(vh):] = ops.reshape(files, opf * op_len)
    return body.reshape(-1), body.shape[1]


def run_shape(ctx, L, args, opf, per_op):
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(17 + per_op)
    key = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    F = args.files
    n_ops, n = F * opf, F * opf * per_op
    col = rng.integers(1 << 32, 1 << 64, n, dtype=np.uint64)     # every member 9 bytes wide
    d_col = torch.from_numpy(col.view(np.int64)).to(dev)
    rc, max_ops, max_files, max_bytes = crdtenc.orswot_add_bound(n, per_op, opf)
    assert rc == 0 and max_files == F and max_ops == n_ops
    d_files = torch.zeros(max_bytes + 64, dtype=torch.uint8, device=dev)
    d_offs = torch.zeros(max_files + 1, dtype=torch.int64, device=dev)
    nonces = ctypes.create_string_buffer(bytes(rng.integers(0, 256, 24 * F, dtype=np.uint8)), 24 * F)
    torch.cuda.synchronize()
    core = crdtenc.Core(ctx, kind=crdtenc.STATE_ORSWOT, supported=[APP], current_data_version=APP)
    core.set_latest_key(key)
    actor = core.info_actor()
    state = {"c": 0, "blob": None, "ops_len": 0, "host_files": None}

    def start():
        """the local actor's counter at C_START: one host Add"""
        one = b"\x91" + b"\x81\xa3Add\x82\xa3dot\x82\xa5actor\xc4\x10" + actor + b"\xa7counter\xcf" + \
              C_START.to_bytes(8, "big") + b"\xa7members\x91\x01"
        if core.apply_ops(one):
            raise crdtenc.CeError(1, ctx.last_error())
        state["c"] = C_START

    def encode():
        t0 = time.perf_counter()
        state["blob"], state["ops_len"] = host_encode(col, F, opf, per_op, actor, state["c"] + 1)
        return (time.perf_counter() - t0) * 1e3

    def device():
        nf, nb = ctypes.c_uint32(0), ctypes.c_uint64(0)
        rc = L.ce_core_orswot_add_members_device(
            core.p, ctypes.c_void_p(d_col.data_ptr()), ctypes.c_uint64(n), ctypes.c_uint32(per_op),
            ctypes.c_uint32(opf), ctypes.c_uint32(0), nonces, ctypes.c_void_p(d_files.data_ptr()),
            ctypes.c_uint64(max_bytes), ctypes.c_void_p(d_offs.data_ptr()), ctypes.byref(nf), ctypes.byref(nb))
        if rc or nf.value != F or nb.value != max_bytes:
            raise crdtenc.CeError(rc, ctx.last_error())
        state["c"] += n_ops

    def host(keep=False):
        blob = state["blob"]
        offs = np.arange(F + 1, dtype=np.uint64) * np.uint64(state["ops_len"])
        fb, fo = crdtenc.Buf(), crdtenc.Buf()
        rc = L.ce_core_apply_ops_batch(core.p, ctypes.c_void_p(blob.ctypes.data), ctypes.c_void_p(offs.ctypes.data),
                                       ctypes.c_uint32(F), nonces, ctypes.byref(fb), ctypes.byref(fo))
        if rc:
            raise crdtenc.CeError(rc, ctx.last_error())
        if keep:
            state["host_files"] = ctypes.string_at(fb.data, fb.len)
        L.ce_buf_free(ctypes.byref(fb))
        L.ce_buf_free(ctypes.byref(fo))
        state["c"] += n_ops

    start()
    wall = {"device": [], "host": []}
    kern = {"device": {}, "host": {}}
    enc_ms = []
    routes = {"device": device, "host": host}
    for it in range(args.warmup + args.steps):
        for name in (("device", "host") if it % 2 == 0 else ("host", "device")):
            if name == "host":
                enc_ms.append(encode())
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
    if core.path_count("orswot_add_device_files") != F * (args.warmup + args.steps):
        raise SystemExit("PATH COUNT MISMATCH")
    end_state = core.state_bytes()
    # the same call from the same counter by each route: identical files
    core.reset()
    start()
    device()
    dev_files = bytes(d_files[:max_bytes].cpu().numpy())
    dev_state = core.state_bytes()
    core.reset()
    start()
    encode()
    host(keep=True)
    if dev_files != state["host_files"] or dev_state != core.state_bytes():
        raise SystemExit("FILES MISMATCH")

    def stats(v):
        return {"median_ms": round(float(np.median(v)), 3), "min_max_ms": [round(min(v), 3), round(max(v), 3)]}
    clear_bytes = F * (16 + state["ops_len"])
    enc_k = kern["device"]["orswot_add_encode"]
    res = {"files": F, "ops_per_file": opf, "per_op": per_op, "ops": n_ops, "members": n, "column_bytes": n * 8,
           "clear_bytes": clear_bytes, "sealed_bytes": max_bytes, "steps": args.steps, "warmup": args.warmup,
           "device_call": stats(wall["device"]), "host_call": stats(wall["host"]),
           "host_encode_ms": round(float(np.median(enc_ms)), 3),
           "device_kernel_ms": {k: round(v, 4) for k, v in kern["device"].items() if v},
           "host_kernel_ms": {k: round(v, 4) for k, v in kern["host"].items() if v},
           "encoder_clear_GBps": round(clear_bytes / (enc_k * 1e-3) / 1e9, 2),
           "encoder_read_plus_write_GBps": round((n * 8 + clear_bytes) / (enc_k * 1e-3) / 1e9, 2),
           "device_over_host": round(float(np.median(wall["device"]) / np.median(wall["host"])), 5),
           "files_identical": True, "state_bytes": len(end_state),
           "adds_monotone": core.path_count("ds_adds_monotone"), "table_rebuilds": core.path_count("ds_table_rebuilds")}
    core.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--files", type=int, default=1 << 14)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(torch.device("cuda", 0))
    L = crdtenc.lib()
    ctx = crdtenc.Context(0)
    res = {"one_member_ops": run_shape(ctx, L, args, 28, 1), "one_long_op": run_shape(ctx, L, args, 1, 446)}
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
