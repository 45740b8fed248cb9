"""Sequential CPU restatement of crdts 7's GSet<u64> and of read_remote_ops / read_remote_states
for it: the checker of the GPU fold of CE_STATE_GSET.

TEST INFRASTRUCTURE ONLY.  Built on oracle.crdts (VClock, the msgpack reader's struct and u64
rules, the canonical writer), which it imports; the crdts source is not on hand, so the type is
restated from its published definition, unpinned in the same sense as tests/pncounter_model.py:

    struct GSet<T: Ord> { value: BTreeSet<T> }       type Op = T
    apply(op): value.insert(op)      merge(o): value.extend(o.value)      validate_*: never fail

Wire forms (rmp-serde to_vec_named): an op file's body is a Vec<u64>; the state is
{"value": [members ascending]}, every integer in its smallest unsigned form.  from_slice takes any
integer marker whose value lies in [0, 2^64), any array header, and ignores bytes after the value.
"""
from oracle.crdts import (DecodeError, VClock, Wr, _seq, _struct, _u64, _unpack, dec_vclock,
                          open_file)


class GSet:
    def __init__(self, value=()):
        self.value = set(value)

    def apply(self, op):
        self.value.add(op)

    def merge(self, other):
        self.value |= other.value

    def read(self):
        return sorted(self.value)

    def __eq__(self, other):
        return self.value == other.value


def dec_ops(b):
    """Vec<u64> -> [member]"""
    return [_u64(x) for x in _seq(_unpack(b))]


def enc_ops(ops):
    """rmp-serde to_vec_named(Vec<u64>)"""
    w = Wr()
    w.arr(len(ops))
    for m in ops:
        w.uint(m)
    return bytes(w.b)


def dec_state(b):
    """StateWrapper<GSet<u64>> -> (next_op_versions, GSet): `value` in any order, duplicates
    collapse (BTreeSet's visitor inserts one by one)"""
    nov, st = _struct(_unpack(b), ["next_op_versions", "state"])
    (value,) = _struct(st, ["value"])
    return dec_vclock(nov), GSet(_u64(x) for x in _seq(value))


def _live(v):
    """a Dot with counter 0 never inserts (VClock::apply): such entries are never written"""
    return VClock({a: c for a, c in v.dots.items() if c})


def serialize(nov, st):
    """Canonical to_vec_named(StateWrapper<GSet<u64>>)"""
    w = Wr()
    w.map(2)
    w.str("next_op_versions")
    w.vclock(_live(nov))
    w.str("state")
    w.map(1)
    w.str("value")
    w.arr(len(st.value))
    for m in sorted(st.value):
        w.uint(m)
    return bytes(w.b)


class Core:
    """read_remote_ops / read_remote_states (crdt-enc/src/lib.rs:401-547) for S = GSet<u64>, as
    oracle.crdts.Core states them for the dot-set kinds: open and decode everything first, the
    first error rejects the batch, then the version gate."""

    def __init__(self):
        self.nov = VClock()
        self.state = GSet()

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
        for nov, s in decoded:
            self.state.merge(s)
            self.nov.merge(nov)
        return 0, status

    def merge_state(self, b):
        nov, s = dec_state(b)
        self.state.merge(s)
        self.nov.merge(nov)

    def apply_ops(self, actor, ops):
        """Core::apply_ops (lib.rs:666-722) for the local actor"""
        for op in ops:
            self.state.apply(op)
        self.nov.apply(actor, self.nov.get(actor) + 1)
