#!/usr/bin/env python3
"""GSet state files: the device reader and the HBM-resident writer beside the host route.

One sealed, ingest-format state file resident in HBM: 2^20 random 64-bit members (all cf but a
handful) under 4096 writers in next_op_versions, ~9.5 MB; and a mixed-width one of the same count
drawn as the serializer tests draw theirs (a fifth of the members in each width, the fixint and cc
ranges exhausted).  Timed in one process after a warm-up, the two routes in turn, their order swapped
from one iteration to the next:

    ingest_empty   ce_core_reset, then ce_core_ingest_states_device (the table keeps its capacity)
    ingest_fresh   ce_core_ingest_states_device into a new core (the table grows from its default)
    ingest_known   ce_core_ingest_states_device into a set that already holds every member
    merge          ce_core_reset, then ce_core_merge_state_device over the clear StateWrapper in HBM
    state_bytes    ce_core_state_bytes_device; the host route is ce_core_state_bytes and an upload

The device route is the default one; the host route is CE_HOST_STATES=1 (every plaintext downloaded,
parsed by one host thread, the members uploaded as a column).  Call times are host clock around
calls that end in a wait for the stream, given as the median of the timed calls with the least and
the greatest beside it; kernel times are the library's HIP event regions, mean per call.  One JSON
line.

    python tools/gset_state_bench.py --steps 11 --warmup 3 --out profiles/gset_states.json
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
sys.path.insert(0, os.path.join(REPO, "tests"))
import crdtenc  # noqa: E402
import gset_model as gm  # noqa: E402
from oracle.crdts import VClock  # noqa: E402

APP = bytes.fromhex("aadfd5a66e194b24a8024fa27c72f20c")
CORE = crdtenc.CORE_VERSION
WRITERS = 4096
KERNELS = ("segments_open", "finalize_open", "gset_state_runs", "gset_state_insert", "gset_sort", "gset_write")
BOUNDS = [(0, 1 << 7, 0), (1 << 7, 1 << 8, 1), (1 << 8, 1 << 16, 2), (1 << 16, 1 << 32, 4), (1 << 32, 1 << 64, 8)]


def encode_members(v):
    """sorted distinct u64 -> the array header and every element in its smallest form"""
    n = len(v)
    out = [bytes([0x90 | n]) if n < 16 else b"\xdc" + n.to_bytes(2, "big") if n < 65536 else b"\xdd" + n.to_bytes(4, "big")]
    be = v.astype(">u8").view(np.uint8).reshape(n, 8)
    for k, (lo, hi, p) in enumerate(BOUNDS):
        sel = (v >= np.uint64(lo)) & (v <= np.uint64(hi - 1))
        rows = be[sel]
        if p == 0:
            out.append(rows[:, 7].tobytes())
            continue
        e = np.empty((len(rows), 1 + p), np.uint8)
        e[:, 0] = 0xcb + k
        e[:, 1:] = rows[:, 8 - p:]
        out.append(e.tobytes())
    return b"".join(out)


def draw(rng, n, mixed):
    if not mixed:
        return np.unique(rng.integers(0, 1 << 64, n, dtype=np.uint64))
    parts = [np.arange(0, 1 << 7, dtype=np.uint64), np.arange(1 << 7, 1 << 8, dtype=np.uint64)]
    per = (n - 256) // 3
    for lo, hi in ((1 << 8, 1 << 16), (1 << 16, 1 << 32), (1 << 32, 1 << 64)):
        parts.append(rng.integers(lo, hi, min(per, (hi - lo) // 2), dtype=np.uint64, endpoint=False))
    return np.unique(np.concatenate(parts))


def state_wrapper(rng, members):
    nov = VClock({bytes(rng.integers(0, 256, 16, dtype=np.uint8)): int(rng.integers(1, 1 << 20)) for _ in range(WRITERS)})
    head = gm.serialize(nov, gm.GSet())
    return head[:-1] + encode_members(members)


def to_dev(b, dev, pad=0):
    t = torch.frombuffer(bytearray(b + bytes(pad)), dtype=torch.uint8).to(dev)
    torch.cuda.synchronize()
    return t


class Case:
    def __init__(self, ctx, key, sw, dev):
        self.ctx, self.key, self.sw, self.dev = ctx, key, sw, dev
        f = CORE + ctx.encrypt(key, APP + sw)
        self.file_len = len(f)
        self.d_file = to_dev(f, dev, pad=64)
        self.d_offs = torch.tensor([0, len(f)], dtype=torch.int64, device=dev)
        self.d_sw = to_dev(sw, dev)
        self.d_out = torch.empty(len(sw) + 4096, dtype=torch.uint8, device=dev)
        self.stage = torch.empty(len(sw) + 4096, dtype=torch.uint8).pin_memory()
        self.core = self.new_core()
        torch.cuda.synchronize()

    def new_core(self):
        c = crdtenc.Core(self.ctx, kind=crdtenc.STATE_GSET, supported=[APP], current_data_version=APP)
        c.set_latest_key(self.key)
        return c

    def ingest(self, core=None):
        core = core or self.core
        rc = core.ingest_states_device(self.d_file.data_ptr(), self.d_offs.data_ptr(), 1, self.file_len)
        if rc:
            raise crdtenc.CeError(rc, self.ctx.last_error())

    def merge(self):
        rc = self.core.merge_state_device(self.d_sw.data_ptr(), len(self.sw))
        if rc:
            raise crdtenc.CeError(rc, self.ctx.last_error())

    def state_bytes(self, host):
        if host:  # the parent's path: serialized to host memory, uploaded into the caller's buffer
            b = self.core.state_bytes()
            ctypes.memmove(self.stage.data_ptr(), b, len(b))  # (one copy into pinned memory, then the upload)
            self.d_out[:len(b)].copy_(self.stage[:len(b)], non_blocking=True)
            torch.cuda.synchronize()
            return len(b)
        rc, n = self.core.state_bytes_device(self.d_out.data_ptr(), self.d_out.numel())
        if rc:
            raise crdtenc.CeError(rc, self.ctx.last_error())
        return n

    def op(self, name, host):
        """(set-up outside the clock, the timed call)"""
        if name == "ingest_empty":
            self.core.reset()
            return self.ingest
        if name == "ingest_fresh":
            c = self.new_core()

            def run():
                self.ingest(c)
                self.fresh = c
            return run
        if name == "ingest_known":
            return self.ingest
        if name == "merge":
            self.core.reset()
            return self.merge
        return lambda: self.state_bytes(host)

    def timed(self, name, steps, warmup):
        """The two routes, their order swapped from one iteration to the next (device host, host
        device, ...), so that each route's calls follow a call of either route equally often: a call
        can leave work for the next one (the host route's 9.5 MB download into pageable memory
        does).  Per route: the calls' median, least and greatest ms, the medians of the calls that
        followed the same route and the other one, and the kernels' mean ms per call."""
        wall = {False: [], True: []}  # (ms, the route of the call before)
        kern = {False: {}, True: {}}
        prev = None
        for it in range(warmup + steps):
            for host in ((False, True) if it % 2 == 0 else (True, False)):
                if host and name != "state_bytes":
                    os.environ["CE_HOST_STATES"] = "1"
                run = self.op(name, host)
                self.ctx.synchronize()
                torch.cuda.synchronize()
                self.ctx.timing_reset()
                self.ctx.set_timing(it >= warmup)
                t0 = time.perf_counter()
                run()
                self.ctx.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                self.ctx.set_timing(False)
                os.environ.pop("CE_HOST_STATES", None)
                if name == "ingest_fresh":
                    self.fresh.close()
                if it >= warmup:
                    wall[host].append((dt, prev))
                    for k in KERNELS:
                        kern[host][k] = kern[host].get(k, 0.0) + self.ctx.timing(k)[0] / steps
                prev = host

        def med(host, after=None):
            v = [dt for dt, p in wall[host] if after is None or p == after]
            return round(float(np.median(v)), 4) if v else None
        dev_k = {k: round(v, 4) for k, v in kern[False].items() if v}
        new_k = sum(v for k, v in kern[False].items() if k.startswith("gset_"))
        all_ms = {h: [dt for dt, _ in wall[h]] for h in wall}
        return {"device_ms": med(False), "host_ms": med(True),
                "device_ms_min_max": [round(min(all_ms[False]), 4), round(max(all_ms[False]), 4)],
                "host_ms_min_max": [round(min(all_ms[True]), 4), round(max(all_ms[True]), 4)],
                "device_ms_after_device": med(False, False), "device_ms_after_host": med(False, True),
                "host_ms_after_host": med(True, True), "host_ms_after_device": med(True, False),
                "device_over_host": round(med(False) / med(True), 4), "device_kernel_ms": dev_k,
                "host_kernel_ms": {k: round(v, 4) for k, v in kern[True].items() if v},
                "gset_kernels_share_of_device_call": round(new_k / med(False), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--members", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = crdtenc.Context(0)
    rng = np.random.default_rng(11)
    key = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    res = {"writers": WRITERS, "steps": args.steps, "warmup": args.warmup}
    for label, mixed in (("random64", False), ("mixed_width", True)):
        members = draw(rng, args.members, mixed)
        sw = state_wrapper(rng, members)
        case = Case(ctx, key, sw, dev)
        r = {"members": int(len(members)), "state_len": len(sw)}
        for name in ("ingest_empty", "ingest_fresh", "ingest_known", "merge", "state_bytes"):
            r[name] = case.timed(name, args.steps, args.warmup)
        # the file is canonical and the core holds exactly it: both routes must give it back
        if case.core.state_bytes() != sw or bytes(case.d_out[:len(sw)].cpu().numpy()) != sw:
            raise SystemExit("STATE MISMATCH (%s)" % label)
        r["device_read_files"] = case.core.path_count("gset_states_device_read")
        r["host_read_files"] = case.core.path_count("gset_states_host_read")
        r["grows"] = case.core.path_count("gset_grows")
        res[label] = r
        case.core.close()
        del case
        torch.cuda.empty_cache()
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
