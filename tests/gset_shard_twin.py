"""CPU twin of shard.DeviceGsetShardOps for the gloo tests of shard.ingest_gset_sharded (no GPU
needed): the product's host twins compute the gate (ce_shard_stats_host, ce_shard_window_host,
ce_shard_window_exact -- the same math as the device kernels), and tests/gset_model.py (the
restatement of crdts 7's GSet<u64> and of read_remote_ops for it) opens, checks and decodes each
file.  The committed state is a gset_model.Core; the pending batch is the set of gated members
the committed set lacks, exported as an unordered u64 column like the device's."""
import numpy as np
import torch

import crdtenc
import gset_model as gm
import shard

APP = bytes.fromhex("aadfd5a66e194b24a8024fa27c72f20c")


class HostGsetShardOps:
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
        members, first = set(), 0
        for i, f in enumerate(self.files):  # every file opens and decodes, applied or not
            one = gm.Core()
            rc, _ = one.read_remote_ops(self.key, [APP], [f], [self.writers[self.fa[i]]], [0])
            if rc:
                first = first or rc
                continue
            a = int(self.fa[i])
            if e0[a] <= self.fv[i] < self.hi[a]:
                members |= one.state.value - self.core.state.value
        if first:
            return first
        nov = {w: max(int(e0[a]), int(self.hi[a])) for a, w in enumerate(self.writers)}
        self.pending = (members, nov)
        return shard.ERR_OP_VERSION if self.flags & shard.SHARD_GAP else 0

    def pending_count(self):
        return len(self.pending[0])

    def member_buffer(self, n):
        return torch.zeros(n, dtype=torch.int64)

    def export_members(self, t):
        v = np.array(list(self.pending[0]), np.uint64)   # (set order: unordered, like the device's)
        t[: len(v)] = torch.from_numpy(v.view(np.int64))
        return len(v)

    def commit(self, accept, parts=(), counts=()):
        (members, nov), self.pending = self.pending, None
        if not accept:
            return
        self.core.state.value |= members
        for p, c in zip(parts, counts):
            self.core.state.value |= set(int(x) for x in p[:c].numpy().view(np.uint64))
        for a, c in nov.items():
            if c:
                self.core.nov.apply(a, c)
