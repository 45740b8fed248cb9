#!/usr/bin/env python3
"""bench.py -- crdt-enc compaction/ingest hot path on MI355X (BASELINE.json configs[1] = C2).

One step = Core::compact over one batch resident in HBM (crdt-enc/src/lib.rs:332-380 minus
disk I/O): XChaCha20-Poly1305 open of every op file + version gate + Vec<Dot> decode + GCounter
max-fold (read_remote_ops, lib.rs:471-547), StateWrapper serialization, GPU seal of the new
state and its SHA3-256/BASE32 content name.  The core is reset to the empty state before each
step so every step folds all files.

Workload per GPU (weak scaling): 1,048,576 op files from this rank's actor shard.
  Variant A (the headline, SURVEY.md §8d "semantic"): plaintext = APP_VERSION(16) ||
    msgpack(Vec<Dot>) with 107 Dots (4085 B, "4 KiB"); actor a's file v holds its own increments.
  Variant B (§8d "stress", reported as the line's `variant_b` key): 97 Dots per file whose
    actors are uniform over all 4096 actors and whose counters are uniform u64 (4093 B), so
    every Dot takes the actor-table probe and most take an atomicMax.
The global job at N GPUs has 4096 actors x 256*N versions, sharded by actor (all versions of an
actor on one rank, as the version gate needs); the per-rank partial GCounters meet in one RCCL
all_reduce(MAX) over the dense actor-indexed state (shard.exchange_vclock).

`--gpus N` without a launcher starts N rank processes itself (the parent never touches the GPU);
under torch.distributed.run WORLD_SIZE must equal --gpus.  Prints ONE JSON line (rank 0) and
exits non-zero if any size-independent result check fails.

A plain run seals the variant-A batch, warms up, times --steps steps, checks the state against
its closed form and prints the headline line.  `--full` adds everything else to that line: the
per-kernel times and the roofline block, the shader-clock probe, the host-buffer run, the CPU
baselines, variant B, the strong-scaling leg (N > 1) and the other BASELINE configs.
`--dump-outputs DIR` writes what the last timed step returned (dump_outputs).
"""
import argparse
import ctypes
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, "crdt-enc_amd"))
import crdtenc  # noqa: E402
import shard  # noqa: E402

METRIC = ("op files compacted/sec + AEAD-open GB/s, 1M×4KiB ops/4096 actors, 1–8 GPUs")
APP = bytes.fromhex("aadfd5a66e194b24a8024fa27c72f20c")      # examples/test/src/main.rs:7
CORE = crdtenc.CORE_VERSION
N_ACTORS = 4096
K_DOTS = {"a": 107, "b": 97}       # 16 + 3 + 107 * 38 = 4085 B;  16 + 3 + 97 * 42 = 4093 B
DOT_LEN = {"a": 38, "b": 42}       # counter as uint32 (ce) / uint64 (cf)
HBM_PEAK_GBS = 8000.0              # MI355X_MICROARCH.md chip table (spec)
# int32 VALU lane-op peak: 256 CU x 4 SIMD x 32 lanes x 2.4 GHz (a wave64 full-rate VALU
# instruction every 2 cycles per SIMD, MI355X_MICROARCH.md:54,473)
VALU_PEAK_TOPS = 256 * 4 * 32 * 2.4e9 / 1e12
# Measured issue ceilings on one MI355X (tools/ubench_valu.hip, tools/ubench_chacha.hip;
# profiles/r02_ubench_valu.txt, profiles/r02_ubench_chacha.txt, in-kernel clock 2.38-2.40 GHz):
#   v_add/v_xor/v_and/v_bitop3/v_fma_f32: 2 cycles per wave64 instruction (63-69 T lane-ops/s);
#   v_alignbit/v_perm/v_add3/v_xad/v_mul_lo and the SDWA forms: 4 cycles (~37 T);
#   v_mad_u64_u32: 4 cycles (34 T at 8 waves/SIMD);
#   ChaCha20 (add/xor/rotate) keystream: 2.50-2.58 TB/s = ~40 T lane-ops/s of the 992-op blocks.
CHACHA_KS_TBPS = 2.58              # best measured ChaCha20 keystream rate (sdwa rot16, 8 waves/SIMD)
VALU_CHACHA_TOPS = CHACHA_KS_TBPS * 1e12 / 64 * 992 / 1e12   # = 40.0 T: the ARX-mix ceiling
DEFAULT_FUSED = 2                  # ce_core.h `fused` default (CE_FUSED overrides it in both)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def actors_table(seed=0xC0FFEE):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, size=(N_ACTORS, 16), dtype=np.uint8)
    a[:, 6] = (a[:, 6] & 0x0F) | 0x40       # UUIDv4-shaped
    a[:, 8] = (a[:, 8] & 0x3F) | 0x80
    order = sorted(range(N_ACTORS), key=lambda i: a[i].tobytes())
    return a[order]


def pt_len(variant):
    return 16 + 3 + DOT_LEN[variant] * K_DOTS[variant]


def build_files(ctx, key, actors_local, actors_all, versions, dev, seed, variant="a", fa=None, fv=None):
    """Seal n = len(actors_local) * versions op files on the GPU (writer i // versions of
    actors_local, version i % versions), or, with fa / fv (int64 numpy, writer index into
    actors_local and version per file), exactly those files.  Returns (files, offs, n, blob_len,
    smax): smax = the u64 max counter per global actor (variant B; int64 views with the sign
    flipped, shard._FLIP), None for variant A (closed form)."""
    m_act = actors_local.shape[0]
    n = m_act * versions if fa is None else len(fa)
    fa_t = torch.from_numpy(np.ascontiguousarray(fa, np.int64)).to(dev) if fa is not None else None
    fv_t = torch.from_numpy(np.ascontiguousarray(fv, np.int64)).to(dev) if fv is not None else None
    K, L = K_DOTS[variant], DOT_LEN[variant]
    PT = pt_len(variant)
    file_len = 16 + crdtenc.sealed_len(PT)
    files = torch.empty(n * file_len + 64, dtype=torch.uint8, device=dev)
    offs = torch.arange(n + 1, dtype=torch.int64, device=dev) * file_len
    act = torch.from_numpy(actors_local).to(dev)
    act_all = torch.from_numpy(actors_all).to(dev)
    pre1 = torch.tensor(list(b"\x82\xa5actor\xc4\x10"), dtype=torch.uint8, device=dev)
    pre2 = torch.tensor(list(b"\xa7counter"), dtype=torch.uint8, device=dev)
    app = torch.tensor(list(APP), dtype=torch.uint8, device=dev)
    hdr = torch.tensor([0xdc, K >> 8, K & 255], dtype=torch.uint8, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    kk = torch.arange(K, dtype=torch.int64, device=dev)
    smax = torch.full((N_ACTORS,), shard._FLIP, dtype=torch.int64, device=dev) if variant == "b" else None
    chunk = 1 << 16
    for c0 in range(0, n, chunk):
        m = min(chunk, n - c0)
        idx = torch.arange(c0, c0 + m, dtype=torch.int64, device=dev)
        if fa_t is None:
            a_loc, v = idx // versions, idx % versions
        else:
            a_loc, v = fa_t[c0:c0 + m], fv_t[c0:c0 + m]
        clear = torch.empty((m, PT), dtype=torch.uint8, device=dev)
        clear[:, :16] = app
        clear[:, 16:19] = hdr
        dots = clear[:, 19:].view(m, K, L)
        dots[:, :, 0:9] = pre1
        dots[:, :, 25:33] = pre2
        if variant == "a":
            dots[:, :, 9:25] = act[a_loc][:, None, :]
            dots[:, :, 33] = 0xce                                  # uint32, big endian
            cval = 65536 + v[:, None] * K + kk[None, :] + 1        # actor's own increments
            for b in range(4):
                dots[:, :, 34 + b] = ((cval >> (8 * (3 - b))) & 255).to(torch.uint8)
        else:
            da = torch.randint(0, N_ACTORS, (m, K), dtype=torch.int64, device=dev, generator=gen)
            dots[:, :, 9:25] = act_all[da]
            dots[:, :, 33] = 0xcf                                  # uint64, big endian
            cb = torch.randint(0, 256, (m, K, 8), dtype=torch.uint8, device=dev, generator=gen)
            cb[:, :, 0] |= 0x01                                    # >= 2^56: canonical cf form
            dots[:, :, 34:42] = cb
            cw = cb.to(torch.int64)
            ctr = torch.zeros((m, K), dtype=torch.int64, device=dev)
            for b in range(8):
                ctr = (ctr << 8) | cw[:, :, b]
            smax.scatter_reduce_(0, da.reshape(-1), ctr.reshape(-1) ^ shard._FLIP, reduce="amax")
        coffs = torch.arange(m + 1, dtype=torch.int64, device=dev) * PT
        nonces = torch.randint(0, 256, (m, 24), dtype=torch.uint8, device=dev, generator=gen)
        ooffs = (idx * file_len).contiguous()
        torch.cuda.current_stream().synchronize()
        ctx.encrypt_batch_device(key, clear.data_ptr(), coffs.data_ptr(), m, nonces.data_ptr(),
                                 files.data_ptr(), ooffs.data_ptr(), outer_version=CORE)
        ctx.synchronize()
    return files, offs, n, n * file_len, smax


def expected_state(actors_all, versions_global, variant="a", smax=None):
    """Size-independent check: the merged StateWrapper<GCounter> in closed form (variant A) or
    from the generator's per-actor max (variant B)."""
    import msgpack
    nov = {bytes(a): versions_global for a in actors_all}
    if variant == "a":
        top = 65536 + versions_global * K_DOTS["a"]
        st = {bytes(a): top for a in actors_all}
    else:
        mx = (smax ^ shard._FLIP).cpu().numpy().view(np.uint64)
        st = {bytes(actors_all[i]): int(mx[i]) for i in range(N_ACTORS) if mx[i]}
    return msgpack.packb({"next_op_versions": {"dots": nov}, "state": {"inner": {"dots": st}}},
                         use_bin_type=True)


def cgroup_cpus():
    """CPUs the cgroup quota allows (cpu.max 'quota period'), None when unlimited / unknown."""
    for path in ("/sys/fs/cgroup/cpu.max",):
        try:
            with open(path) as f:
                q, p = f.read().split()[:2]
            return None if q == "max" else max(1, int(int(q) // int(p)))
        except (OSError, ValueError):
            pass
    try:
        with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:
            q = int(f.read())
        with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
            p = int(f.read())
        return None if q <= 0 else max(1, q // p)
    except (OSError, ValueError):
        return None


def gpu_node_cpus(dev):
    """CPUs of the NUMA node the GPU hangs off (sysfs), within this process's affinity; empty
    when unknown"""
    try:
        p = torch.cuda.get_device_properties(dev)
        bdf = "%04x:%02x:%02x.0" % (getattr(p, "pci_domain_id", 0), p.pci_bus_id, p.pci_device_id)
        node = int(open("/sys/bus/pci/devices/%s/numa_node" % bdf).read())
        if node < 0:
            return set()
        cpus = set()
        for part in open("/sys/devices/system/node/node%d/cpulist" % node).read().strip().split(","):
            a, _, b = part.partition("-")
            cpus.update(range(int(a), int(b or a) + 1))
        return cpus & os.sched_getaffinity(0)
    except (OSError, ValueError, AttributeError, RuntimeError):
        return set()


def host_cpu():
    """(model, usable CPUs, threads for the best-CPU leg, how the count was chosen).  usable =
    min(affinity, cgroup quota); threads = min(usable, OMP_NUM_THREADS): the job's CPU share --
    on the GPU box the harness sets OMP_NUM_THREADS=16 per one-GPU job, the share we may use."""
    model = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    aff = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    quota = cgroup_cpus()
    usable = min(aff, quota) if quota else aff
    omp = os.environ.get("OMP_NUM_THREADS")
    threads = max(1, min(usable, int(omp) if omp else usable, 256))
    why = {"nproc": os.cpu_count(), "affinity": aff, "cgroup_quota_cpus": quota,
           "OMP_NUM_THREADS": int(omp) if omp else None, "threads": threads,
           "per_gpu_share_of_8_gpu_node": max(1, (os.cpu_count() or 8) // 8),
           "rule": "threads = min(affinity, cgroup quota, OMP_NUM_THREADS): the CPU share this "
                   "one-GPU job is given (the box sets OMP_NUM_THREADS=16)"}
    return model, usable, threads, why


def probe_clock(ctx, step, dev):
    """Shader clock (untimed, after the timed steps): ce_ctx_clock_probe's one-wave blocks,
    one per XCD, on a side stream, sampling every 100 us for 4 ms -- once with the GPU
    otherwise idle, once beside `step` (its main kernel runs ~0.2-3.5 ms into it; the probe's
    waves hold 8 of its wave slots, so that step is slower and is not reported).
    GHz = shader cycles / reference ticks x 0.1 (100 MHz reference clock)."""
    blocks, samples, ticks = 8, 40, 10000
    side = torch.cuda.Stream(device=dev)
    res = {}
    for what in ("idle", "under_step"):
        out = torch.zeros(blocks * samples * 2, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        ctx.clock_probe(out.data_ptr(), blocks, samples, ticks, stream_ptr=side.cuda_stream)
        if what == "under_step":
            step()
        torch.cuda.synchronize()
        v = out.view(blocks, samples, 2).cpu().numpy().astype(np.float64)
        ghz = v[:, :, 0] / np.maximum(v[:, :, 1], 1) * 0.1
        mid = ghz[:, 5:30]   # 0.5-3.0 ms after the probe starts: inside the main kernel
        res[what] = {"median_ghz": round(float(np.median(mid)), 3),
                     "min_ghz": round(float(mid.min()), 3), "max_ghz": round(float(mid.max()), 3)}
    res["method"] = ("ce_ctx_clock_probe: s_memtime over s_memrealtime per 100-us interval, "
                     "8 one-wave blocks, intervals 0.5-3.0 ms after launch")
    return res


def launch_ranks(args):
    """--gpus N without torch.distributed.run: start N rank processes (this parent never
    initialises HIP), forward rank 0's stdout, exit with the worst rank status."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus),
                   LOCAL_WORLD_SIZE=str(args.gpus), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:],
                                      env=env, stdout=subprocess.PIPE if r == 0 else sys.stderr))
    out = procs[0].stdout.read()
    rcs = [p.wait() for p in procs]
    sys.stdout.write(out.decode())
    sys.stdout.flush()
    return max(rcs, key=abs)


class Workload:
    """One variant's sealed batch on this rank, its core and its step function."""

    def __init__(self, ctx, variant, args, world, rank, dev, actors_all, scaling="weak"):
        self.dev = dev
        self.variant = variant
        self.world, self.rank = world, rank
        self.actors_all = actors_all
        self.scaling = scaling
        # weak scaling: 1M files per GPU (the job grows with N); strong: the one 1M-file job split
        # over the N ranks
        self.versions = args.versions * (world if scaling == "weak" else 1)
        self.key = bytes(np.random.default_rng(7).integers(0, 256, 32, dtype=np.uint8))
        # N > 1: files partitioned by address (shard.ingest_sharded), every writer on every rank;
        # --partition actor: the previous writer-sharded layout (shard.exchange_vclock)
        self.partition = args.partition if world > 1 else "single"
        fa_sel = fv_sel = None
        if self.partition == "address":
            fa_all = np.repeat(np.arange(N_ACTORS, dtype=np.uint32), self.versions)
            fv_all = np.tile(np.arange(self.versions, dtype=np.uint64), N_ACTORS)
            own = crdtenc.shard_owners([bytes(a) for a in actors_all], fa_all, fv_all, world)
            keep = own == rank
            fa_sel, fv_sel = fa_all[keep].astype(np.int64), fv_all[keep].astype(np.int64)
            self.actors_local = actors_all
            self.per = N_ACTORS
            del fa_all, fv_all, own, keep
        else:
            lo, hi = shard.actor_range(N_ACTORS, world, rank)
            self.per = hi - lo
            self.actors_local = actors_all[lo:hi]
        t0 = time.time()
        self.files, self.offs, self.n, self.blob_len, smax = build_files(
            ctx, self.key, self.actors_local, actors_all, self.versions, dev,
            seed=1234 + rank + (7919 if variant == "b" else 0), variant=variant, fa=fa_sel, fv=fv_sel)
        if smax is not None and world > 1:
            shard.all_reduce_(smax, dist.ReduceOp.MAX)   # flipped u64 -> signed max
        self.smax = smax
        log("rank %d: variant %s: sealed %d op files (%.2f GB) in %.1f s" % (
            rank, variant, self.n, self.blob_len / 1e9, time.time() - t0))
        self.core = crdtenc.Core(ctx, kind=crdtenc.STATE_GCOUNTER, supported=[APP],
                                 current_data_version=APP)
        self.core.set_latest_key(self.key)
        self.core.register_actors([bytes(a) for a in actors_all])   # same dense slots on every rank
        cap = self.core.dense_capacity()
        # state and next_op_versions side by side: one all_reduce(MAX) per step (latency-bound)
        self.dense = torch.zeros(2 * cap, dtype=torch.int64, device=dev)
        self.local_actor_bytes = b"".join(bytes(a) for a in self.actors_local)
        if fa_sel is not None:
            self.fa, self.fv = fa_sel.astype(np.uint32), fv_sel.astype(np.uint64)
        else:
            self.fa = np.repeat(np.arange(self.per, dtype=np.uint32), self.versions)
            self.fv = np.tile(np.arange(self.versions, dtype=np.uint64), self.per)
        # per-file metadata lives in HBM with the files (what Storage::load_ops hands over)
        self.fa_d = torch.from_numpy(self.fa.astype(np.int32)).to(dev)
        self.fv_d = torch.from_numpy(self.fv.astype(np.int64)).to(dev)
        self.out = {}
        self.paths = set()
        self.sharded = None
        if self.partition == "address":
            self.sharded = shard.DeviceShardOps(self.core, self.local_actor_bytes, self.files, self.offs,
                                                self.n, self.blob_len, self.fa_d, self.fv_d)
        # files of the whole job (the ranks' counts differ slightly under the address partition)
        tot = torch.tensor([self.n], dtype=torch.int64, device=dev)
        if world > 1:
            shard.all_reduce_(tot, dist.ReduceOp.SUM)
        self.total_files = int(tot.item())
        # The SHA3-256 content name of step i's state file (host, ~0.2 MB) is computed on the
        # library's own host thread (ce_content_name_async) while step i+1's kernels run; every
        # name is done before the timed region ends.  (A Python worker thread cost ~35 us per step
        # in interpreter-lock hand-offs with this one: same box, 3.40 vs 3.37 ms.)
        self.names = []
        # the sealed state file is downloaded straight into one of NB pinned buffers (no staging
        # copies); a buffer is reused once its previous step's content name is done
        self.NB = 3
        bound = 16 + crdtenc.sealed_len(69 + 54 * self.core.dense_capacity())
        self.obuf = [torch.empty(bound, dtype=torch.uint8, pin_memory=True).numpy() for _ in range(self.NB)]

    def step(self):
        core = self.core
        core.reset()
        if self.world == 1:
            # Core::compact (lib.rs:332-380): read_remote_ops + the compaction output in one call
            k = len(self.names) % self.NB
            if len(self.names) >= self.NB:
                self.names[-self.NB].result()
            rc, ln, _ = core.compact_ops_device_into(self.obuf[k], self.files.data_ptr(), self.offs.data_ptr(),
                                                     self.n, self.blob_len, self.local_actor_bytes,
                                                     self.fa_d.data_ptr(), self.fv_d.data_ptr())
            if rc:
                raise crdtenc.CeError(rc, core.ctx.last_error())
            self.out["file"] = f = self.obuf[k][:ln]
            self.names.append(crdtenc.content_name_async(f))
            return
        if self.sharded is not None:
            # address partition: cross-rank version gate, pending fold, one all_reduce(MAX) of
            # the dense batch with the failure flags (shard.ingest_sharded)
            rc, path = shard.ingest_sharded(self.sharded)
            if rc:
                raise crdtenc.CeError(rc, core.ctx.last_error())
            self.paths.add(path)
        else:
            rc = core.ingest_ops_device(self.files.data_ptr(), self.offs.data_ptr(), self.n,
                                        self.blob_len, self.local_actor_bytes, self.fa_d.data_ptr(),
                                        self.fv_d.data_ptr())
            if rc:
                raise crdtenc.CeError(rc, core.ctx.last_error())
            self.paths.add(shard.exchange_vclock(core, self.dense))   # all_reduce(MAX) over RCCL
        if self.rank == 0:
            f, _ = core.compact_to_buffer(name=False)
            self.out["file"] = f
            self.names.append(crdtenc.content_name_async(f))

    def close(self):
        self.core.close()

    def drain_names(self):
        for fu in self.names:
            self.out["name"] = fu.result()
        self.names = []

    def run(self, ctx, steps, warmup, all_kernels=True):
        """Warm up, time `steps` steps, check the state.  all_kernels: two more (untimed) steps
        with HIP events around every kernel, for the per-kernel figures (--full)."""
        for _ in range(warmup):
            self.step()
        self.drain_names()
        if self.world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        names = ("open_setup", "gate", "open_fold_small", "segments_open", "finalize_open", "decode",
                 "merge", "seal_setup", "segments_seal", "finalize_seal")
        # the timed steps carry HIP events around the fused kernel only (every timed launch adds
        # two stream markers); the other kernels are timed on two extra steps afterwards
        time_all = bool(os.environ.get("CE_BENCH_TIME_ALL"))
        ctx.timing_reset()
        ctx.set_timing_only(None if time_all else "open_fold_small")
        ctx.set_timing(True)
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step()
        self.drain_names()
        torch.cuda.synchronize()
        if self.world > 1:
            dist.barrier()
        t1 = time.perf_counter()
        ctx.set_timing(False)
        ms = (t1 - t0) * 1e3 / steps
        ms_t = torch.tensor([ms], dtype=torch.float64, device=self.dense.device)
        if self.world > 1:
            shard.all_reduce_(ms_t, dist.ReduceOp.MAX)
        kern = {k: ctx.timing(k) for k in names}
        # what the last timed step handed its caller (rank 0), before any later step reuses the
        # pinned buffer it was downloaded into
        self.last_file = bytes(self.out["file"]) if self.rank == 0 else None
        if all_kernels and not time_all:
            ctx.timing_reset()
            ctx.set_timing_only(None)
            ctx.set_timing(True)
            for _ in range(2):
                self.step()
            self.drain_names()
            ctx.set_timing(False)
            kern.update({k: ctx.timing(k) for k in names if k != "open_fold_small"})
        ok = True
        if self.rank == 0:
            sb = self.core.state_bytes()
            ok = sb == expected_state(self.actors_all if self.world > 1 else self.actors_local,
                                      self.versions, self.variant, self.smax)
            if not ok:
                log("STATE MISMATCH (variant %s)" % self.variant)
        return float(ms_t.item()), kern, ok

    def clock_probe(self, ctx):
        """Shader clock beside one untimed step (probe_clock)."""
        def one():
            self.step()
            self.drain_names()
        return probe_clock(ctx, one, self.dense.device)

    def host_buffer_run(self, ctx, steps=3, warmup=1):
        """Core::compact from per-file host buffers (what Storage::load_ops hands a Rust
        caller, lib.rs:495): ce_core_compact_ops_iov gathers the files into pinned staging chunks
        on host threads and DMAs them while the next chunk fills, then runs the device path.
        Returns the end-to-end files/s and the PCIe rate of the upload (HIP events on the copy
        stream)."""
        n = self.n
        # pageable, like Vec<u8>s, first-touched on the GPU's NUMA node (where a deployment reads
        # its files into; on the other socket the gather reads cross the socket link and the rate
        # depends on which socket the process happened to start on: 43 vs 55 GB/s on two boxes)
        staged = self.files[: self.blob_len].cpu().numpy()
        cpus = gpu_node_cpus(self.dev)
        old_aff = os.sched_getaffinity(0) if cpus else None
        try:
            if cpus:
                os.sched_setaffinity(0, cpus)
            host = np.empty_like(staged)
            host[:] = staged
        finally:
            if old_aff:
                os.sched_setaffinity(0, old_aff)
        del staged
        base = host.ctypes.data
        offs = self.offs[: n + 1].cpu().numpy().astype(np.uint64)
        ptrs = (ctypes.c_void_p * n).from_buffer(np.ascontiguousarray(base + offs[:-1]).astype(np.uint64))
        lens = (ctypes.c_size_t * n).from_buffer(np.ascontiguousarray(offs[1:] - offs[:-1]).astype(np.uint64))
        fa = np.ascontiguousarray(self.fa.astype(np.uint32))
        fv = np.ascontiguousarray(self.fv.astype(np.uint64))
        fa_p, fv_p = fa.ctypes.data_as(ctypes.c_void_p), fv.ctypes.data_as(ctypes.c_void_p)

        def one():
            self.core.reset()
            rc, f, _ = self.core.compact_ops_iov(ptrs, lens, n, self.local_actor_bytes, fa_p, fv_p, name=False)
            if rc:
                raise crdtenc.CeError(rc, ctx.last_error())
            self.names.append(crdtenc.content_name_async(f))

        for _ in range(warmup):
            one()
        self.drain_names()
        torch.cuda.synchronize()
        ctx.timing_reset()
        ctx.set_timing(True)
        t0 = time.perf_counter()
        for _ in range(steps):
            one()
        self.drain_names()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ctx.set_timing(False)
        up_ms, up_n = ctx.timing("upload")
        ms = (t1 - t0) * 1e3 / steps
        ok = self.core.state_bytes() == expected_state(self.actors_local, self.versions, self.variant, self.smax)
        del host
        return {"value": round(n / (ms / 1e3), 1), "ms_per_step": round(ms, 3), "steps": steps,
                "upload_ms": round(up_ms / max(up_n, 1), 3),
                "pcie_GBps": round(self.blob_len / (up_ms / max(up_n, 1) / 1e3) / 1e9, 1) if up_n else None,
                "bytes": self.blob_len, "state_check": "ok" if ok else "MISMATCH",
                "path": "ce_core_compact_ops_iov: 1,048,576 per-file host buffers (pageable) -> "
                        "host-thread gather (threads on the GPU's NUMA node) into a ring of 4 x 32 MiB "
                        "pinned chunks -> DMA on a copy stream -> device compaction (never the line's "
                        "value: inputs are not resident)"}, ok

    def cpu_baseline(self, args):
        """The oracle (C restatement of the reference path) on this host, both modes, over the
        same files; each mode's serialized state must equal the GPU path's on the sample."""
        sys.path.insert(0, REPO)
        import oracle
        model, avail, threads, why = host_cpu()
        n, versions = self.n, self.versions
        s = min(args.cpu_sample, n) if args.cpu_sample > 0 else n
        s -= s % versions
        file_len = self.blob_len // n
        host = self.files[: s * file_len].cpu().numpy()
        h_offs = (np.arange(s + 1, dtype=np.uint64) * file_len)
        h_act = np.ascontiguousarray(self.actors_local[self.fa[:s]])
        h_ver = np.ascontiguousarray(self.fv[:s])
        # the same sample through the GPU path
        self.core.reset()
        rc = self.core.ingest_ops_device(self.files.data_ptr(), self.offs.data_ptr(), s,
                                         s * file_len, b"".join(bytes(a) for a in self.actors_local[: s // versions]),
                                         self.fa_d.data_ptr(), self.fv_d.data_ptr())
        gpu_state = self.core.state_bytes() if rc == 0 else None
        res = {}
        for mode, best, th in (("best", True, threads), ("reference_shaped", False, min(16, threads))):
            t = time.perf_counter()
            err, ser = oracle.compact_ops_baseline(
                oracle.STATE_GCOUNTER, self.key, APP, host.ctypes.data_as(ctypes.c_void_p),
                h_offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                h_act.ctypes.data_as(ctypes.c_void_p),
                h_ver.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), s, th, best=best)
            dt = time.perf_counter() - t
            res[mode] = {"value": round(s / dt, 1), "cores": th, "seconds": round(dt, 3),
                         "same_state_as_gpu": err == 0 and ser == gpu_state}
        b, r = res["best"], res["reference_shaped"]
        return {
            "value": b["value"], "unit": "op files/s", "cores": b["cores"], "kind": "port",
            "sample": "%d files (%d actors x %d versions) of this workload; oracle/ce_oracle.c "
                      "best-CPU mode: AEAD open + decode parallel over files, version gate + "
                      "fold parallel over actors, private states merged, on %d threads; "
                      "serialized state == GPU path: %s" % (s, s // versions, versions, b["cores"],
                                                            b["same_state_as_gpu"]),
            "seconds": b["seconds"], "host_cpu": model, "nproc": os.cpu_count(), "usable_cpus": avail,
            "cores_rule": why,
            "reference_shaped": dict(r, unit="op files/s", mode="%d AEAD threads (buffered(16), "
                                     "lib.rs:497-514), decode + fold on one thread "
                                     "(lib.rs:516-544)" % r["cores"]),
        }, b["same_state_as_gpu"] and r["same_state_as_gpu"]


def ops_8d(pt):
    """ops(file) = 992*ceil(ct/64) + 992 + 960 + 48*(ceil(ct/16) + 1) -- the
    keystream blocks, the Poly1305 key block, HChaCha20 and the Poly1305 pieces + length block"""
    return 992 * -(-pt // 64) + 992 + 960 + 48 * (-(-pt // 16) + 1)


def ops_fused(pt):
    """the part of ops_8d the fused kernel runs: HChaCha20 (960) and the Poly1305 key block (992)
    run in k_open_setup"""
    return ops_8d(pt) - 992 - 960


PROFILE_ROUND = "r06"


def rocprof_avg_ms(name):
    """average duration of the kernel whose name starts with `name` in this round's committed
    rocprofv3 --kernel-trace --stats summary of the bench (profiles/<round>_kernel_stats.csv), or None"""
    import csv
    f = os.path.join(REPO, "profiles", PROFILE_ROUND + "_kernel_stats.csv")
    if not os.path.exists(f):
        return None
    with open(f) as fh:
        for row in csv.DictReader(fh):
            if row["Name"].split("(")[0].replace("void ", "").startswith(name):
                return float(row["AverageNs"]) / 1e6
    return None


def kernel_summary(w, ms, kern):
    seg_ms, seg_n = kern["open_fold_small"]
    avg_s = seg_ms / max(seg_n, 1) / 1e3
    su_ms, su_n = kern.get("open_setup", (0.0, 0))
    setup_s = su_ms / max(su_n, 1) / 1e3
    PT = pt_len(w.variant)
    n = w.n
    ops_per_file = ops_8d(PT)                     # SURVEY.md §8d, the setup's 1,952 ops included
    # the §8d work runs in two launches (k_open_setup, then the fused kernel): timed by both
    valu = n * ops_per_file / (avg_s + setup_s) / 1e12 if avg_s > 0 else 0.0
    valu_fused = n * ops_fused(PT) / avg_s / 1e12 if avg_s > 0 else 0.0
    bytes_per_launch = n * (PT + 16)              # read ct + tag; plaintext stays in LDS
    return {"value": round(w.total_files / (ms / 1e3), 1), "ms_per_step": round(ms, 4),
            "avg_launch_ms": round(avg_s * 1e3, 4), "setup_avg_ms": round(setup_s * 1e3, 4),
            "ops_per_file": ops_per_file, "ops_per_file_fused": ops_fused(PT),
            "valu_tops": round(valu, 2), "valu_frac": round(valu / VALU_PEAK_TOPS, 4),
            "valu_tops_fused_only": round(valu_fused, 2), "valu_frac_fused_only": round(valu_fused / VALU_PEAK_TOPS, 4),
            "hbm_GBps": round(bytes_per_launch / avg_s / 1e9, 1) if avg_s > 0 else None,
            "aead_open_GBps": round(n * PT / avg_s / 1e9, 1) if avg_s > 0 else None,
            "bytes_per_launch": bytes_per_launch,
            "kernels_ms_per_step": {k: round(v[0] / max(v[1], 1), 4) for k, v in kern.items() if v[1]}}


def dump_outputs(d, ctx, w):
    """--dump-outputs: what the last timed step handed its caller, as float32 .npy files (one
    value per byte).  The step returns the compacted state file, APP_VERSION(16) || sealed
    StateWrapper; it is sealed under a fresh random nonce, so two runs agree on the opened
    plaintext, not on the ciphertext:
      state.npy      the StateWrapper bytes the file opens to (the product's own AEAD open)
      file_meta.npy  [file length, the 16 data-version bytes]"""
    f = w.last_file
    st, plain = ctx.decrypt(w.key, f[16:])
    if st:
        raise SystemExit("bench.py: the last step's state file does not open (status %d)" % st)
    os.makedirs(d, exist_ok=True)
    np.save(os.path.join(d, "state.npy"), np.frombuffer(plain, dtype=np.uint8).astype(np.float32))
    np.save(os.path.join(d, "file_meta.npy"),
            np.array([len(f)] + list(f[:16]), dtype=np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one returned as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="beside the headline line: per-kernel and roofline figures, the shader-clock "
                         "probe, the host-buffer run, the CPU baselines, variant B, the strong-scaling "
                         "leg (N > 1) and the other BASELINE configs (the --no-* / --configs options "
                         "below choose among them)")
    ap.add_argument("--versions", type=int, default=256, help="versions per actor per GPU")
    ap.add_argument("--cpu-sample", type=int, default=0,
                    help="files in the CPU baseline sample (0 = the whole per-GPU workload)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-variant-b", action="store_true", help="skip the stress-dot variant")
    ap.add_argument("--no-clock", action="store_true", help="skip the shader-clock probe")
    ap.add_argument("--no-host-buffers", action="store_true",
                    help="skip the end-to-end run from host buffers (H2D over PCIe)")
    ap.add_argument("--configs", default="c3,c3r,c4,c5",
                    help="N=1: also run these BASELINE configs (bench_configs.py runners) and report "
                         "them under the line's `configs` key ('' = none)")
    ap.add_argument("--no-strong", action="store_true", help="N > 1: skip the strong-scaling C2 leg")
    ap.add_argument("--quick", action="store_true",
                    help="tests: the configs at small sizes, 2 timed steps each (never a reported line)")
    ap.add_argument("--partition", choices=("address", "actor"), default="address",
                    help="N > 1: op files by address hash with the cross-rank gate (default), or "
                         "whole writers per rank")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    full = args.full

    if "WORLD_SIZE" not in os.environ:
        if args.gpus > 1:
            sys.exit(launch_ranks(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # CE_BENCH_SHARE_GPU=1: every rank on device 0 (multi-rank rehearsal on a one-GPU box, with
    # CE_DIST_BACKEND=gloo since RCCL refuses two ranks on one device)
    dev_idx = 0 if os.environ.get("CE_BENCH_SHARE_GPU") == "1" else local
    torch.cuda.set_device(dev_idx)
    dev = torch.device("cuda", dev_idx)
    # every host thread (launches, name hashing, host-buffer gathers) on the GPU's NUMA node:
    # the C3 names ran 3.42 -> 2.60 ms/step pinned on the same box (CE_BENCH_NUMA_PIN=0: off)
    if os.environ.get("CE_BENCH_NUMA_PIN", "1") == "1":
        cpus = gpu_node_cpus(dev)
        if cpus:
            os.sched_setaffinity(0, cpus)
    if world > 1:
        backend = os.environ.get("CE_DIST_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    if N_ACTORS % world:
        raise SystemExit("world size must divide 4096")

    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    ctx = crdtenc.Context(dev_idx)
    ctx.set_stream(stream.cuda_stream)
    actors_all = actors_table()

    wa = Workload(ctx, "a", args, world, rank, dev, actors_all)
    ms, kern, ok = wa.run(ctx, args.steps, args.warmup, all_kernels=full)
    sa = kernel_summary(wa, ms, kern)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, ctx, wa)
    # everything from here to the result line is behind --full: a plain run times the C2 steps only
    clock = wa.clock_probe(ctx) if full and world == 1 and not args.no_clock else None
    cpu, cpu_ok = None, True
    hostbuf = None
    if full and world == 1 and not args.no_host_buffers:
        hostbuf, hb_ok = wa.host_buffer_run(ctx)
        ok = ok and hb_ok
    if full and rank == 0 and world == 1 and not args.no_cpu:
        cpu, cpu_ok = wa.cpu_baseline(args)
    paths_a = sorted(wa.paths)
    wa_total = wa.total_files
    wa.close()
    del wa

    vb = None
    if full and not args.no_variant_b:
        wb = Workload(ctx, "b", args, world, rank, dev, actors_all)
        ms_b, kern_b, ok_b = wb.run(ctx, args.steps, args.warmup)
        ok = ok and ok_b
        sb = kernel_summary(wb, ms_b, kern_b)
        vb = dict(sb, workload="C2 variant B (SURVEY.md §8d stress): 1,048,576 x 4093 B op files "
                               "per GPU, 97 Dots each with actors uniform over 4096 and uniform "
                               "u64 counters", dots_per_file=K_DOTS["b"],
                  state_check="StateWrapper bytes == generator's per-actor max: %s" % ("ok" if ok_b else "MISMATCH"))
        wb.close()
        del wb

    # N > 1: the same 1M-file C2 job split over the N ranks (strong scaling), beside the weak line
    strong = None
    if full and world > 1 and not args.no_strong:
        ws = Workload(ctx, "a", args, world, rank, dev, actors_all, scaling="strong")
        ms_s, kern_s, ok_s = ws.run(ctx, args.steps, args.warmup)
        ok = ok and ok_s
        ss = kernel_summary(ws, ms_s, kern_s)
        n_max = torch.tensor([ws.n], dtype=torch.int64, device=dev)
        shard.all_reduce_(n_max, dist.ReduceOp.MAX)
        strong = dict(ss, scaling="strong", files_total=ws.total_files, files_per_gpu_max=int(n_max.item()),
                      workload="C2: the one 1,048,576 x 4 KiB GCounter job (4096 actors x %d versions) "
                               "partitioned by address over %d ranks" % (args.versions, world),
                      exchange_paths=sorted(ws.paths),
                      state_check="closed-form StateWrapper bytes: %s" % ("ok" if ok_s else "MISMATCH"))
        ws.close()
        del ws

    # the other BASELINE configs (C3 Orswot, C4 skewed sizes, C5 key-rotation mix), each timed
    # and checked by bench_configs.py's runner -- reported beside the C2 line, never its value.
    # N = 1: on this GPU; N > 1: strong scaling over the ranks (bench_configs.run_config)
    configs = None
    if full and args.configs:
        import bench_configs
        configs = {}
        for c in [x for x in args.configs.split(",") if x]:
            # C3: 120 steps (~0.4 s) -- every step's 35 MB file is named by a ~48 ms SHA3 on a host
            # thread, so the timed region (which ends when the last name is done) approaches the
            # steady state only over many steps: the last name's latency weighs ~0.4 ms a step here
            steps_c = {"c3": 120, "c3r": 40, "c4": 10, "c5": 10}[c]
            extra = {"c3": ["--versions", "2", "--state-versions", "1"],
                     "c3r": ["--versions", "2", "--state-versions", "1"], "c4": ["--c4-versions", "2"],
                     "c5": ["--c5-versions", "4"]}[c] if args.quick else []
            ns = bench_configs.make_parser().parse_args(
                ["--config", c, "--steps", str(2 if args.quick else steps_c), "--warmup", "1", "--no-clock"] +
                (["--no-cpu"] if args.no_cpu else []) + extra)
            t_c = time.time()
            line_c = bench_configs.run_config(c, ns, ctx, dev, world, rank)
            line_c["wall_s"] = round(time.time() - t_c, 1)
            good = all(bool(v) for v in line_c.get("checks", {}).values()) and (
                line_c.get("cpu_baseline") is None or line_c["cpu_baseline"].get("same_result_as_gpu", True))
            if not good and "skipped" not in line_c:
                log("CONFIG %s CHECK FAILED: %s" % (c, line_c.get("checks")))
                ok = False
            configs[c] = line_c
            torch.cuda.empty_cache()

    if rank == 0:
        line = {
            "metric": METRIC,
            "value": sa["value"],
            "unit": "op files/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": sa["ms_per_step"],
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u32",
            "data": "synthetic (GPU-sealed op files, seeded)",
            "config": {
                "workload": "C2: 1,048,576 x 4 KiB encrypted GCounter op files per GPU "
                            "(4096 actors x %d versions at N=%d%s), decrypt + max-join + compact"
                            % (args.versions * world, world,
                               "" if world == 1 else ", %s-partitioned" % args.partition),
                "files_per_gpu": wa_n(args, world), "files_total": wa_total,
                "plaintext_bytes": pt_len("a"),
                "dots_per_file": K_DOTS["a"], "actors": N_ACTORS,
                "parallelism": (("op files partitioned by address hash (ops/<actor>/<version>), "
                                 "cross-rank version gate (per-writer stats all_reduce MAX), "
                                 "pending batch + failure flags all_reduce(MAX) (%s), exchange "
                                 "path %s" if args.partition == "address" else
                                 "actor-sharded files, all_reduce(MAX) of dense state (%s), "
                                 "exchange path %s") % (os.environ.get("CE_DIST_BACKEND", "nccl"),
                                                        "/".join(paths_a)))
                               if world > 1 else "single GPU",
            },
            "aead_open_GBps": sa["aead_open_GBps"],
            "state_check": "closed-form StateWrapper bytes: %s" % ("ok" if ok else "MISMATCH"),
        }
        if full:
            line.update({
                "roofline": roofline_report(args, world, sa, clock),
                "kernels_ms_per_step": sa["kernels_ms_per_step"],
                "variant_b": vb,
                "strong": strong,
                "host_buffers": hostbuf,
                "cpu_baseline": cpu,
                "configs": configs,
            })
        if not (ok and cpu_ok):
            line.pop("value")
            line["error"] = "result check failed: see state_check / cpu_baseline"
        print(json.dumps(line), flush=True)
    all_ok = torch.tensor([1 if (ok and cpu_ok) else 0], dtype=torch.int64, device=dev)
    if world > 1:
        shard.all_reduce_(all_ok, dist.ReduceOp.MIN)
        dist.barrier()
        dist.destroy_process_group()
    ctx.close()
    if int(all_ok.item()) != 1:
        sys.exit(3)


def roofline_report(args, world, sa, clock):
    """--full: the fused kernel's roofline block, from this run's HIP-event times beside the
    committed profiles of the same kernel and launch size"""
    fused = os.environ.get("CE_FUSED", str(DEFAULT_FUSED))
    lpf = 64 // int(os.environ.get("CE_FILES_PER_WAVE", "4"))
    v3 = fused == "2" and lpf == 16 and not os.environ.get("CE_FUSED_V2")
    v3b = int(os.environ.get("CE_V3", "2"))
    kname = ("k_open_fold_v3<%s, %s> (XChaCha20-Poly1305 open + Vec<Dot> decode + fold, lane-owned "
             "ChaCha20 blocks, Poly1305 as four-product column sums)"
             % ("true" if v3b & 1 else "false", "true" if v3b & 2 else "false") if v3 else
             "k_open_fold_v2<%d> (XChaCha20-Poly1305 open + Vec<Dot> decode + fold, "
             "lane-owned ChaCha20 blocks)" % lpf if fused == "2" and lpf != 64 else
             "k_open_fold_small<%d> (XChaCha20-Poly1305 open + Vec<Dot> decode + fold)" % lpf)
    kshort = kname.split(" (")[0]
    traffic = None
    tf = os.path.join(REPO, "profiles", "traffic_open_fold_small.json")
    if os.path.exists(tf):
        with open(tf) as f:
            rec = json.load(f)
        # only a measurement of the kernel this run used (and of the same 1M-file launch)
        if kname.split(" (")[0].rstrip(">") in rec.get("kernel", "") and \
                rec.get("files_per_launch") == wa_n(args, world):
            traffic = rec.get("bytes_per_launch")
    valu_pmc = None
    vf = os.path.join(REPO, "profiles", "valu_pmc.json")
    if os.path.exists(vf) and sa["avg_launch_ms"] > 0:
        with open(vf) as f:
            rec = json.load(f).get("fused", {})
        ipf = rec.get("valu_instr_per_file_per_lane")
        if ipf and rec.get("kernel", "").replace("void ", "").replace("ce::", "") == kshort:
            t = wa_n(args, world) * ipf / (sa["avg_launch_ms"] / 1e3) / 1e12
            valu_pmc = {"instr_per_file": ipf, "achieved_tops": round(t, 2),
                        "frac_of_peak": round(t / VALU_PEAK_TOPS, 4),
                        "source": "profiles/valu_pmc.json (rocprofv3 SQ_INSTS_VALU x 64 per "
                                  "file, same kernel and workload)"}
    return {
        "kernel": kname,
        "bound": "valu",
        "achieved": sa["valu_tops"], "peak": round(VALU_PEAK_TOPS, 1),
        "unit": "T int32 lane-ops/s", "frac": sa["valu_frac"],
        "ops_per_file": sa["ops_per_file"], "avg_launch_ms": sa["avg_launch_ms"],
        "setup_avg_ms": sa["setup_avg_ms"],
        "traffic": traffic,
        "ops_formula": "992*ceil(ct/64) + 992 + 960 + 48*(ceil(ct/16)+1) per file (SURVEY.md §8d) "
                       "x files per launch / (avg fused launch + avg k_open_setup launch), both "
                       "HIP events on the kernels' stream; the setup runs the HChaCha20 (960) and "
                       "Poly1305-key block (992) ops",
        "fused_only": {"ops_per_file": sa["ops_per_file_fused"], "achieved": sa["valu_tops_fused_only"],
                       "frac": sa["valu_frac_fused_only"],
                       "note": "the fused kernel alone: §8d less the setup's 1,952 ops per file"},
        "rocprof": rocprof_frac(sa, wa_n(args, world), kshort),
        "measured_chacha20_ceiling": {
            "tops": round(VALU_CHACHA_TOPS, 1), "keystream_TBps": CHACHA_KS_TBPS,
            "frac": round(sa["valu_tops"] / VALU_CHACHA_TOPS, 4),
            "source": "profiles/r02_ubench_chacha.txt, profiles/r02_ubench_valu.txt"},
        "hbm": {"achieved": sa["hbm_GBps"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round((sa["hbm_GBps"] or 0) / HBM_PEAK_GBS, 4),
                "bytes_per_launch": sa["bytes_per_launch"]},
        "pmc_valu": valu_pmc,
        # the peak scales with the shader clock: frac against the peak at the clock the
        # probe saw beside the fused kernel (VALU_PEAK_TOPS is quoted at 2.4 GHz)
        "clock": dict(clock, frac_at_measured_clock=round(
            sa["valu_frac"] * 2.4 / clock["under_step"]["median_ghz"], 4)) if clock else None,
    }


def rocprof_frac(sa, n, kshort):
    """the same fraction with the committed rocprofv3 averages of the two kernels (the verdict's
    recomputation uses these) -- only when the profile is of the kernel this run launched, over
    the same files per launch (its .meta.json, written with it), else None"""
    meta = os.path.join(REPO, "profiles", PROFILE_ROUND + "_kernel_stats.meta.json")
    if not os.path.exists(meta):
        return None
    with open(meta) as fh:
        m = json.load(fh)
    if m.get("files_per_launch") != n or m.get("fused_kernel", "").replace("ce::", "") != kshort:
        return None
    f = rocprof_avg_ms("ce::" + kshort)
    s = rocprof_avg_ms("ce::k_open_setup")
    if not f or not s:
        return None
    t = n * sa["ops_per_file"] / ((f + s) / 1e3) / 1e12
    return {"fused_avg_ms": round(f, 4), "setup_avg_ms": round(s, 4), "achieved": round(t, 2),
            "frac": round(t / VALU_PEAK_TOPS, 4), "files_per_launch": m["files_per_launch"],
            "kernel": m["fused_kernel"], "command": m.get("command"),
            "source": "profiles/%s_kernel_stats.csv" % PROFILE_ROUND}


def wa_n(args, world):
    return N_ACTORS // world * args.versions * world


if __name__ == "__main__":
    main()
