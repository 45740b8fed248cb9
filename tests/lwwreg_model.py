"""Sequential CPU restatement of crdts 7's LWWReg<u64, u64> and of read_remote_ops /
read_remote_states for it: the checker of the GPU fold of CE_STATE_LWWREG.

TEST INFRASTRUCTURE ONLY.  Built on oracle.crdts (VClock, the msgpack reader's struct rules, the
canonical writer), which it imports; the crdts source is not on hand, so the type is restated from
its published definition, unpinned in the same sense as Orswot:

    struct LWWReg<V, M> { val: V, marker: M }          Default: val = 0, marker = 0
    CmRDT::Op = LWWReg<V, M>                           apply(op) = update(op.val, op.marker)
    CvRDT::merge(other) = update(other.val, other.marker)
    update(val, marker): if self.marker < marker { self.val = val; self.marker = marker }

The reference calls no validate_op / validate_merge (crdt-enc/src/lib.rs:460, 534), so an equal
marker keeps the incumbent whatever its val, and the apply order decides ties: read_remote_ops
keeps the batch's order (lib.rs:512-541); read_remote_states merges in completion order
(buffer_unordered, lib.rs:452), which this model and the product define as the call's file order.
"""
from oracle.crdts import DecodeError, VClock, Wr, _seq, _struct, _u64, _unpack, dec_vclock, open_file


class LWWReg:
    def __init__(self, val=0, marker=0):
        self.val = val
        self.marker = marker

    def update(self, val, marker):
        if self.marker < marker:
            self.val = val
            self.marker = marker

    def apply(self, op):
        self.update(op[0], op[1])

    def merge(self, other):
        self.update(other.val, other.marker)

    def read(self):
        return (self.val, self.marker)

    def __eq__(self, other):
        return self.read() == other.read()


def dec_reg(obj):
    val, marker = _struct(obj, ["val", "marker"])
    return (_u64(val), _u64(marker))


def dec_ops(b):
    """Vec<LWWReg<u64, u64>> -> [(val, marker)]"""
    return [dec_reg(o) for o in _seq(_unpack(b))]


def dec_state(b):
    """StateWrapper<LWWReg> -> (next_op_versions, LWWReg)"""
    nov, st = _struct(_unpack(b), ["next_op_versions", "state"])
    return dec_vclock(nov), LWWReg(*dec_reg(st))


def _live(v):
    """a Dot with counter 0 never inserts (VClock::apply): such entries are never written"""
    return VClock({a: c for a, c in v.dots.items() if c})


def _reg(w, val, marker):
    w.map(2)
    w.str("val")
    w.uint(val)
    w.str("marker")
    w.uint(marker)


def serialize(nov, st):
    """Canonical to_vec_named(StateWrapper<LWWReg<u64, u64>>)"""
    w = Wr()
    w.map(2)
    w.str("next_op_versions")
    w.vclock(_live(nov))
    w.str("state")
    _reg(w, st.val, st.marker)
    return bytes(w.b)


def enc_ops(ops):
    """rmp-serde to_vec_named(Vec<LWWReg<u64, u64>>)"""
    w = Wr()
    w.arr(len(ops))
    for val, marker in ops:
        _reg(w, val, marker)
    return bytes(w.b)


class Core:
    """read_remote_ops / read_remote_states (crdt-enc/src/lib.rs:401-547) for S = LWWReg, as
    oracle.crdts.Core states them for the dot-set kinds."""

    def __init__(self):
        self.nov = VClock()
        self.state = LWWReg()

    def serialize(self):
        return serialize(self.nov, self.state)

    def read_remote_ops(self, key, supported, files, actors, versions):
        status, decoded, first = [], [], 0
        for f in files:
            st, pt = open_file(key, supported, f)
            ops = None
            if st == 0:
                try:
                    ops = dec_ops(pt)
                except DecodeError:
                    st = 12
            status.append(st)
            decoded.append(ops)
            if st and not first:
                first = st
        if first:
            return first, status
        for i, ops in enumerate(decoded):
            a, v = actors[i], versions[i]
            expected = self.nov.get(a)
            if v < expected:
                continue
            if expected < v:
                status[i] = 13
                return 13, status
            for op in ops:
                self.state.apply(op)
            self.nov.apply(a, expected + 1)
        return 0, status

    def read_remote_states(self, key, supported, files):
        status, decoded, first = [], [], 0
        for f in files:
            st, pt = open_file(key, supported, f)
            sw = None
            if st == 0:
                try:
                    sw = dec_state(pt)
                except (DecodeError, ValueError, TypeError):
                    st = 12
            status.append(st)
            decoded.append(sw)
            if st and not first:
                first = st
        if first:
            return first, status
        for nov, s in decoded:  # the call's file order
            self.state.merge(s)
            self.nov.merge(nov)
        return 0, status

    def merge_state(self, b):
        nov, s = dec_state(b)
        self.state.merge(s)
        self.nov.merge(nov)
