"""CPU twin of shard.DevicePnShardOps for the gloo tests of shard.ingest_sharded over PNCounter op
files (no GPU needed): the product's host twins compute the gate (ce_shard_stats_host,
ce_shard_window_host, ce_shard_window_exact -- the same math as the device kernels), and
tests/pncounter_model.py (the restatement of crdts 7's PNCounter<Uuid> and of read_remote_ops for
it) opens, checks and decodes each file.  The committed state is a pncounter_model.Core; the
pending batch is a PNCounter of the gated files' ops, exported as both planes of a dense array
over the registered actors (p at [slot], n at [slot + capacity]) like the device's."""
import numpy as np
import torch

import crdtenc
import pncounter_model as pm
import shard

APP = bytes.fromhex("aadfd5a66e194b24a8024fa27c72f20c")
DEVICE = shard.DevicePnShardOps     # the class this twin stands in for


class TwinPnCore(pm.Core):
    """the model with the two calls the bytes exchange makes"""

    def state_bytes(self):
        return self.serialize()

    def merge_state(self, b):
        pm.Core.merge_state(self, b)
        return 0


class HostPnShardOps:
    """One rank: files[i] written by writers[fa[i]] at version fv[i] (its partition's share);
    registered = the actors with dense slots (in order)."""

    def __init__(self, core, key, writers, registered, files, fa, fv):
        self.core, self.key = core, key
        self.writers = list(writers)
        self.reg = list(registered)
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
        batch, first = pm.PNCounter(), 0
        for i, f in enumerate(self.files):  # every file opens and decodes, applied or not
            one = pm.Core()
            rc, _ = one.read_remote_ops(self.key, [APP], [f], [self.writers[self.fa[i]]], [0])
            if rc:
                first = first or rc
                continue
            a = int(self.fa[i])
            if e0[a] <= self.fv[i] < self.hi[a]:
                batch.merge(one.state)
        if first:
            return first
        nov = {w: max(int(e0[a]), int(self.hi[a])) for a, w in enumerate(self.writers)}
        self.pending = (batch, nov)
        return shard.ERR_OP_VERSION if self.flags & shard.SHARD_GAP else 0

    def dense_buffer(self):
        return torch.zeros(2 * len(self.reg) + 2, dtype=torch.int64)

    def export_pending(self, dense):
        batch, cap = self.pending[0], len(self.reg)
        if not all(a in self.reg for v in (batch.p, batch.n) for a, c in v.dots.items() if c):
            return False
        v = np.array([batch.p.get(a) for a in self.reg] + [batch.n.get(a) for a in self.reg], np.uint64)
        dense[: 2 * cap] = torch.from_numpy(v.view(np.int64))
        return True

    def commit(self, accept, reduced=None):
        (batch, nov), self.pending = self.pending, None
        if not accept:
            return
        if reduced is not None:
            v, cap = reduced.numpy().view(np.uint64), len(self.reg)
            for i, a in enumerate(self.reg):
                self.core.state.p.apply(a, int(v[i]))
                self.core.state.n.apply(a, int(v[cap + i]))
        else:
            self.core.state.merge(batch)
        for a, c in nov.items():
            if c:
                self.core.nov.apply(a, c)
