#!/usr/bin/env python3
"""Orswot Rm-op files written from a member column in HBM, beside the host route.

One process removes a column of live members from an Orswot of C3's shape (100k members, 4096
actors, about 3 dots a member), with fixed nonces, from one core without storage.  Two routes in
turn, their order swapped from one iteration to the next; before every timed call the core is
reset and the same op files are ingested again, so both routes remove live members:

    device   ce_core_orswot_rm_members_device: clocks gathered, ordered, sized, encoded, sealed
             and folded on the device
    host     the members' download, ce_core_orswot_member_clocks, the msgpack of the ops vectors
             encoded on the host (timed on its own), ce_core_apply_ops_batch

Two shapes: 2^16 members at 16 ops a file, and one 1024-member call.  After the clock both routes
write the same call once more from the same state: their files must be identical.  Call times
are host clock around calls that end in a wait for the stream, given as the median of the timed
calls with the least and the greatest beside it; kernel times are the library's HIP event
regions, mean per call.  One JSON object per shape, in one JSON line.

    python tools/orswot_rm_bench.py --steps 12 --warmup 2 --out profiles/orswot_rm.json
"""
import argparse
import ctypes
import json
import os
import struct
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "crdt-enc_amd"))
import crdtenc  # noqa: E402

APP = bytes.fromhex("aadfd5a66e194b24a8024fa27c72f20c")
KERNELS = ("orswot_rm_clocks", "orswot_rm_sizes", "orswot_rm_encode", "orswot_rm_cols", "seal_setup", "segments_seal",
           "finalize_seal", "ds_part_fold", "ds_kill", "ds_finalize", "ds_member_clocks")
N_MEMBERS, N_ACTORS, DOTS = 100_000, 4096, 3


def uint(v):
    if v <= 0x7f:
        return bytes([v])
    if v <= 0xff:
        return b"\xcc" + bytes([v])
    if v <= 0xffff:
        return b"\xcd" + v.to_bytes(2, "big")
    if v <= 0xffffffff:
        return b"\xce" + v.to_bytes(4, "big")
    return b"\xcf" + v.to_bytes(8, "big")


def hdr(n, fix, m16):
    return bytes([fix | n]) if n <= 15 else bytes([m16]) + n.to_bytes(2, "big")


def build_state(rng):
    """op files of N_ACTORS writers: every member under DOTS dots of random writers, a dot an op"""
    actors = [bytes(rng.integers(0, 256, 16, dtype=np.uint8)) for _ in range(N_ACTORS)]
    members = rng.choice(np.arange(1 << 20, 1 << 24, dtype=np.uint64), N_MEMBERS, replace=False)
    who = rng.integers(0, N_ACTORS, (N_MEMBERS, DOTS))
    per = [[] for _ in range(N_ACTORS)]
    for i in range(N_MEMBERS):
        for a in set(int(x) for x in who[i]):
            per[a].append(int(members[i]))
    clears = []
    for a, ms in enumerate(per):
        head = b"\x81\xa3Add\x82\xa3dot\x82\xa5actor\xc4\x10" + actors[a] + b"\xa7counter"
        ops = [head + uint(j + 1) + b"\xa7members\x91" + uint(m) for j, m in enumerate(ms)]
        clears.append(APP + hdr(len(ops), 0x90, 0xdc) + b"".join(ops))
    return actors, members, clears, sum(len(p) for p in per)


def host_encode(col, raw, opf):
    """to_vec_named(Vec<orswot::Op>) of every file's vector from ce_core_orswot_member_clocks'
    answer: u32 beg[n + 1] padded to 8 bytes, then (uuid16, u64 LE counter) entries"""
    n = len(col)
    beg = struct.unpack_from("<%dI" % (n + 1), raw)
    base = ((n + 1) * 4 + 7) & ~7
    head, tail = b"\x81\xa2Rm\x82\xa5clock\x81\xa4dots", b"\xa7members\x91"
    ops = []
    for i in range(n):
        k = beg[i + 1] - beg[i]
        parts = [head, hdr(k, 0x80, 0xde)]
        for e in range(beg[i], beg[i + 1]):
            o = base + 24 * e
            parts += [b"\xc4\x10", raw[o:o + 16], uint(int.from_bytes(raw[o + 16:o + 24], "little"))]
        parts += [tail, uint(int(col[i]))]
        ops.append(b"".join(parts))
    return [hdr(len(ops[i:i + opf]), 0x90, 0xdc) + b"".join(ops[i:i + opf]) for i in range(0, n, opf)]


def run_shape(ctx, L, args, st, n, opf):
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(23 + n)
    key, actors, members, sealed, pairs = st
    F = -(-n // opf)
    col = rng.choice(members, n, replace=False)
    d_col = torch.from_numpy(col.view(np.int64).copy()).to(dev)
    nonces = [bytes(rng.integers(0, 256, 24, dtype=np.uint8)) for _ in range(F)]
    c_nonces = ctypes.create_string_buffer(b"".join(nonces), 24 * F)
    core = crdtenc.Core(ctx, kind=crdtenc.STATE_ORSWOT, supported=[APP], current_data_version=APP)
    core.set_latest_key(key)
    fa, fv = list(range(N_ACTORS)), [0] * N_ACTORS
    state = {"vecs": None, "host_files": None}

    def remerge():
        core.reset()
        rc, _ = core.ingest_ops(sealed, actors, fa, fv, want_status=True)
        if rc:
            raise crdtenc.CeError(rc, ctx.last_error())

    remerge()
    rc, n_ops, nf, nbytes = core.orswot_rm_members_device(d_col.data_ptr(), n, None, 0, None, opf, 0)
    assert rc == 0 and (n_ops, nf) == (n, F), ctx.last_error()
    d_files = torch.zeros(nbytes + 64, dtype=torch.uint8, device=dev)
    d_offs = torch.zeros(F + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    entries0 = core.path_count("orswot_rm_device_entries")

    def device():
        got = core.orswot_rm_members_device(d_col.data_ptr(), n, d_files.data_ptr(), nbytes, d_offs.data_ptr(), opf, 0,
                                            nonces)
        if got != (0, n, F, nbytes):
            raise crdtenc.CeError(got[0], ctx.last_error())

    def host(keep=False):
        t0 = time.perf_counter()
        q = d_col.cpu().numpy().view(np.uint64)
        b = crdtenc.Buf()
        rc = L.ce_core_orswot_member_clocks(core.p, ctypes.c_void_p(q.ctypes.data), ctypes.c_uint32(n), ctypes.byref(b))
        if rc:
            raise crdtenc.CeError(rc, ctx.last_error())
        raw = ctypes.string_at(b.data, b.len)
        L.ce_buf_free(ctypes.byref(b))
        t1 = time.perf_counter()
        vecs = host_encode(q, raw, opf)
        t2 = time.perf_counter()
        rc, fs = core.apply_ops_batch(vecs, nonces)
        if rc:
            raise crdtenc.CeError(rc, ctx.last_error())
        if keep:
            state["host_files"] = b"".join(fs)
        state["clear_bytes"] = sum(16 + len(v) for v in vecs)
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3

    wall = {"device": [], "host": []}
    kern = {"device": {}, "host": {}}
    read_ms, enc_ms = [], []
    for it in range(args.warmup + args.steps):
        for name in (("device", "host") if it % 2 == 0 else ("host", "device")):
            remerge()
            ctx.synchronize()
            torch.cuda.synchronize()
            ctx.timing_reset()
            ctx.set_timing(it >= args.warmup)
            t0 = time.perf_counter()
            parts = device() if name == "device" else host()
            ctx.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            ctx.set_timing(False)
            if it >= args.warmup:
                if parts:
                    read_ms.append(parts[0])
                    enc_ms.append(parts[1])
                    dt -= parts[1]          # the encode is given on its own
                wall[name].append(dt)
                for k in KERNELS:
                    kern[name][k] = kern[name].get(k, 0.0) + ctx.timing(k)[0] / args.steps
    entries = (core.path_count("orswot_rm_device_entries") - entries0) // (args.warmup + args.steps)
    # the same call from the same state by each route: identical files and states
    remerge()
    device()
    dev_files = bytes(d_files[:nbytes].cpu().numpy())
    dev_state = core.state_bytes()
    remerge()
    host(keep=True)
    if dev_files != state["host_files"] or dev_state != core.state_bytes():
        raise SystemExit("FILES MISMATCH")

    def stats(v):
        return {"median_ms": round(float(np.median(v)), 3), "min_max_ms": [round(min(v), 3), round(max(v), 3)]}
    slots = 1
    while slots < 2 * pairs + 1:
        slots *= 2
    table_bytes = slots * 16                # the keys and the values, read by each of the two scans
    enc_k, clk = kern["device"]["orswot_rm_encode"], kern["device"]["orswot_rm_clocks"]
    res = {"members": n, "ops_per_file": opf, "files": F, "entries": int(entries), "clear_bytes": state["clear_bytes"],
           "sealed_bytes": nbytes, "steps": args.steps, "warmup": args.warmup, "state_pairs": pairs,
           "pair_table_bytes": table_bytes,
           "device_call": stats(wall["device"]), "host_call_without_encode": stats(wall["host"]),
           "host_read_clocks_ms": round(float(np.median(read_ms)), 3), "host_encode_ms": round(float(np.median(enc_ms)), 3),
           "device_kernel_ms": {k: round(v, 4) for k, v in kern["device"].items() if v},
           "host_kernel_ms": {k: round(v, 4) for k, v in kern["host"].items() if v},
           "encoder_clear_GBps": round(state["clear_bytes"] / (enc_k * 1e-3) / 1e9, 2),
           # the region also holds the mark, keep, scan, sort and entry kernels: a floor for the scans' rate
           "two_scans_over_clocks_region_GBps": round(2 * table_bytes / (clk * 1e-3) / 1e9, 2),
           "device_over_host": round(float(np.median(wall["device"]) /
                                           (np.median(wall["host"]) + np.median(enc_ms))), 5),
           "files_identical": True}
    core.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(torch.device("cuda", 0))
    L = crdtenc.lib()
    ctx = crdtenc.Context(0)
    rng = np.random.default_rng(5)
    key = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    actors, members, clears, pairs = build_state(rng)
    sealed = [crdtenc.CORE_VERSION + e for e in ctx.encrypt_batch(key, clears)]
    st = (key, actors, members, sealed, pairs)
    res = {"column_65536": run_shape(ctx, L, args, st, 1 << 16, 16), "column_1024": run_shape(ctx, L, args, st, 1024, 16)}
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
