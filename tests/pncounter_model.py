"""Sequential CPU restatement of crdts 7's PNCounter<Uuid> and of read_remote_ops /
read_remote_states for it: the checker of the GPU fold of CE_STATE_PNCOUNTER.

TEST INFRASTRUCTURE ONLY.  Built on oracle.crdts (VClock, the msgpack reader's struct / enum
rules, the canonical writer), which it imports; the crdts source is not on hand, so the type is
restated from its published definition, unpinned in the same sense as Orswot:

    struct PNCounter<A> { p: GCounter<A>, n: GCounter<A> }     GCounter<A> { inner: VClock<A> }
    enum Dir { Pos, Neg }          struct Op<A> { dot: Dot<A>, dir: Dir }
    apply(op): Pos -> p.apply(op.dot), Neg -> n.apply(op.dot)  (VClock::apply keeps the max)
    merge(o):  p.merge(o.p); n.merge(o.n)

Wire forms (rmp-serde to_vec_named): a unit variant is its name as a str; from_slice also takes
the one-entry map {variant name | index: nil}.
"""
from oracle.crdts import (DecodeError, VClock, Wr, _Map, _seq, _struct, _u64, _unpack, _uuid,
                          dec_vclock, open_file)

DIRS = ["Pos", "Neg"]


class PNCounter:
    def __init__(self):
        self.p = VClock()
        self.n = VClock()

    def apply(self, op):
        (actor, counter), d = op
        (self.p if d == "Pos" else self.n).apply(actor, counter)

    def merge(self, other):
        self.p.merge(other.p)
        self.n.merge(other.n)

    def read(self):
        return sum(self.p.dots.values()) - sum(self.n.dots.values())

    def __eq__(self, other):
        return self.p == other.p and self.n == other.n


def dec_dir(obj):
    if isinstance(obj, str):
        if obj not in DIRS:
            raise DecodeError("variant")
        return obj
    if not isinstance(obj, _Map) or len(obj) != 1:
        raise DecodeError("enum")
    k, body = obj[0]
    if isinstance(k, bytes):
        k = k.decode("latin-1")
    if isinstance(k, int) and not isinstance(k, bool) and 0 <= k < len(DIRS):
        k = DIRS[k]
    if k not in DIRS or body is not None:
        raise DecodeError("variant")
    return k


def dec_op(obj):
    dot, d = _struct(obj, ["dot", "dir"])
    actor, counter = _struct(dot, ["actor", "counter"])
    return ((_uuid(actor), _u64(counter)), dec_dir(d))


def dec_ops(b):
    """Vec<pncounter::Op<Uuid>> -> [((actor, counter), "Pos" | "Neg")]"""
    return [dec_op(o) for o in _seq(_unpack(b))]


def _dec_gcounter(obj):
    (inner,) = _struct(obj, ["inner"])
    return dec_vclock(inner)


def dec_state(b):
    """StateWrapper<PNCounter> -> (next_op_versions, PNCounter)"""
    nov, st = _struct(_unpack(b), ["next_op_versions", "state"])
    p, n = _struct(st, ["p", "n"])
    c = PNCounter()
    c.p, c.n = _dec_gcounter(p), _dec_gcounter(n)
    return dec_vclock(nov), c


def _live(v):
    """a Dot with counter 0 never inserts (VClock::apply): such entries are never written"""
    return VClock({a: c for a, c in v.dots.items() if c})


def serialize(nov, st):
    """Canonical to_vec_named(StateWrapper<PNCounter<Uuid>>)"""
    w = Wr()
    w.map(2)
    w.str("next_op_versions")
    w.vclock(_live(nov))
    w.str("state")
    w.map(2)
    for name, v in (("p", st.p), ("n", st.n)):
        w.str(name)
        w.map(1)
        w.str("inner")
        w.vclock(_live(v))
    return bytes(w.b)


def enc_ops(ops):
    """rmp-serde to_vec_named(Vec<pncounter::Op<Uuid>>)"""
    w = Wr()
    w.arr(len(ops))
    for (actor, counter), d in ops:
        w.map(2)
        w.str("dot")
        w.map(2)
        w.str("actor")
        w.bin(actor)
        w.str("counter")
        w.uint(counter)
        w.str("dir")
        w.str(d)
    return bytes(w.b)


class Core:
    """read_remote_ops / read_remote_states (crdt-enc/src/lib.rs:401-547) for S = PNCounter, as
    oracle.crdts.Core states them for the dot-set kinds."""

    def __init__(self):
        self.nov = VClock()
        self.state = PNCounter()

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
