"""CPU twin of shard.DeviceLwwShardOps for the gloo tests of shard.ingest_lwwreg_sharded (no GPU
needed): the product's host twins compute the gate (ce_shard_stats_host, ce_shard_window_host,
ce_shard_window_exact -- the same math as the device kernels), and tests/lwwreg_model.py (the
restatement of crdts 7's LWWReg<u64, u64> and of read_remote_ops for it) opens, checks and decodes
each file.  The committed state is a lwwreg_model.Core; the pending batch is the share's winner as
(marker, val, writer index, version), found by the keys themselves like the device's keyed reduce,
and the commit picks with shard.lww_pick, the rule of ce_core_lwwreg_pending_commit."""
import numpy as np
import torch

import crdtenc
import lwwreg_model as lm
import shard

APP = bytes.fromhex("aadfd5a66e194b24a8024fa27c72f20c")
DEVICE = shard.DeviceLwwShardOps     # the class this twin stands in for


class HostLwwShardOps:
    """One rank: files[i] written by writers[fa[i]] at version fv[i] (its partition's share)."""

    def __init__(self, core, key, writers, files, fa, fv):
        self.core, self.key = core, key
        self.writers = list(writers)
        self.files = list(files)
        self.fa = np.asarray(fa, np.uint32)
        self.fv = np.asarray(fv, np.uint64)
        self.pending = None

    def writer_versions(self):
        return np.array([self.core.nov.get(w) for w in self.writers], np.uint64)

    def compute_stats(self, rank, world):
        st = crdtenc.shard_stats_host(self.writers, self.writer_versions(), self.fa, self.fv, rank, world)
        self.stats = torch.from_numpy(st.copy())
        return self.stats

    def window(self):
        self.hi, self.flags = crdtenc.shard_window_host(self.writer_versions(), self.stats.numpy())

    def set_window(self, hi, flags):
        self.hi, self.flags = np.asarray(hi, np.uint64), flags

    def metadata(self):
        return self.fa, self.fv

    def ingest(self):
        self.pending = None
        if self.flags & (shard.SHARD_BAD | shard.SHARD_E0_MISMATCH):
            return shard.ERR_SHARD
        e0 = self.writer_versions()
        recs, first = [], 0
        for i, f in enumerate(self.files):  # every file opens and decodes, applied or not
            one = lm.Core()
            rc, _ = one.read_remote_ops(self.key, [APP], [f], [self.writers[self.fa[i]]], [0])
            if rc:
                first = first or rc
                continue
            a = int(self.fa[i])
            if e0[a] <= self.fv[i] < self.hi[a]:
                val, marker = one.state.read()      # the file's own winner: its first op with its largest marker
                recs.append((marker, val, a, int(self.fv[i])))
        if first:
            return first
        nov = {w: max(int(e0[a]), int(self.hi[a])) for a, w in enumerate(self.writers)}
        self.pending = (shard.lww_pick(recs), nov)
        return shard.ERR_OP_VERSION if self.flags & shard.SHARD_GAP else 0

    def record(self):
        return self.pending[0]

    def commit(self, accept, recs=()):
        (mine, nov), self.pending = self.pending, None
        if not accept:
            return
        marker, val, _, _ = shard.lww_pick([mine] + list(recs))
        if marker:
            self.core.state.update(val, marker)
        for a, c in nov.items():
            if c:
                self.core.nov.apply(a, c)
