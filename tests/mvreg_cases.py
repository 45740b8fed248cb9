"""Directed MVReg<u64, Uuid> cases for the survivor rounds of crdt-enc_amd/csrc/ce_dotset.hip
(k_mv_prep, k_mv_argmax, k_mv_final, k_mv_kill, k_mv_clear), the device decode of `Put`
(ce_dotset_codec.h ds_parse_mvreg_ops) and the host driver (ce_dotset_host.cpp mvreg_survivors /
mvreg_commit / mvreg_merge_one), checked on the CPU by tests/test_mvreg_cases_model.py and run on
the GPU by tests/test_gpu_mvreg.py.

TEST INFRASTRUCTURE ONLY: plain Python, no GPU, no torch.  Expected results always come from
oracle/crdts.py (C.Core("mvreg") / C.MVReg), never from the library.

Families (every case names the kernel line it is aimed at in `target`):
  A  the 128-bit clock sum's carry (k_mv_prep `hi += lo < c`, mv_better comparing hi first)
  B  ties and the survivors' order in `vals` (ops: the latest op wins, merges: the earliest value)
  C  winner clocks wider than a block of 256 (k_mv_final's scatter, k_mv_clear, `e += kBlock`)
  D  candidate counts at the block and grid edges (k_mv_final's second trip over the block
     results needs n_blk > 256, k_mv_argmax's grid stride needs more than 1024 * 256 candidates)
  E  the wire grammar of `Put` on the device: accepted forms, rejected files, host-decoder forms
  F  state files whose `vals` is no antichain of non-empty clocks: the survivor rounds do not
     state MVReg::merge for them, the host route (mv_host_merge / mv_host_apply) does

Out of scope: zero counters inside a clock.  The oracle's `lt` (`!=` and `le`) and crdts'
PartialOrd may differ there and the crdts source is not available to settle it, so no case holds
a zero counter and none asserts anything about one.

A case is a list of steps applied to one fresh core, in order:
  ("states", [StateWrapper bytes, ...])            read_remote_states / merge_state of each file
  ("ops", writers, [(clear, file_actor, version)], decoded)
                                                   read_remote_ops; `decoded` = the op tuples per
                                                   file when the builder knows them (family D:
                                                   the oracle's decode is skipped), else None
  ("apply", Vec<Op> bytes)                         Core::apply_ops of the local actor
"""
import functools

from oracle import crdts as C

APP = bytes.fromhex("aadfd5a66e194b24a8024fa27c72f20c")
U = (1 << 64) - 1
K_BLOCK = 256          # ce_dotset.hip kBlock
MAX_BLOCKS = 1024      # mvreg_survivors: n_blk = min(1024, ceil(n / 256))
ME = bytes.fromhex("4d45" * 8)   # stands in for the local actor where a test has no core


def n_blk(n):
    return min(MAX_BLOCKS, (n + K_BLOCK - 1) // K_BLOCK)


def actor(k, tag=0xA0):
    """actor k of a family of up to 65536; ascending k = ascending UUID bytes = clock entry order"""
    return bytes([tag]) + k.to_bytes(2, "big") + bytes([0x11] * 13)


def writer(k):
    return actor(k, 0xF0)


# ------------------------------------------------------------------------------------------
# hand encoder for one Put (rmp-serde from_slice forms, ce_dotset_codec.h)
# ------------------------------------------------------------------------------------------
def uint(x, w="min"):
    """msgpack integer in a chosen width; "min" = the shortest, "neg" = the negative fixint -1"""
    if w == "min":
        w = "fix" if x <= 0x7f else "cc" if x <= 0xff else "cd" if x <= 0xffff else "ce" if x <= 0xffffffff else "cf"
    if w == "fix":
        assert x <= 0x7f
        return bytes([x])
    if w == "neg":
        return b"\xff"
    n = {"cc": 1, "cd": 2, "ce": 4, "cf": 8}[w]
    return bytes([{"cc": 0xcc, "cd": 0xcd, "ce": 0xce, "cf": 0xcf}[w]]) + x.to_bytes(n, "big")


def arr_hdr(n, force16=False):
    if n < 16 and not force16:
        return bytes([0x90 | n])
    if n <= 0xffff:
        return b"\xdc" + n.to_bytes(2, "big")
    return b"\xdd" + n.to_bytes(4, "big")


def map_hdr(n, force16=False):
    return bytes([0x80 | n]) if n < 16 and not force16 else b"\xde" + n.to_bytes(2, "big")


def put(clock, val, cw="min", vw="min", form="map", order="cv", keys="name", variant="name",
        vclock="map", map16=False, extra=False, dup=False, drop_val=False):
    """One mvreg::Op::Put { clock, val }.

    clock    [(actor, counter)] written in this order (the caller sorts, or does not)
    cw, vw   integer width of the counters / of val (see uint)
    form     "map" (struct as a map) or "array" ([clock, val])
    order    "cv" clock first, "vc" val first (map form)
    keys     "name" or "index" (map form)
    variant  "name", "idx0", "idx1", "unknown", or "two" (an enum map of two entries)
    vclock   "map" ({dots: ..}) or "array" ([dots])
    map16    the dots map with a map16 header whatever its size
    extra    an unknown third field (skipped); dup: `clock` twice; drop_val: no `val`
    """
    dots = map_hdr(len(clock), map16) + b"".join(b"\xc4\x10" + a + uint(c, cw) for a, c in clock)
    vc = (b"\x81\xa4dots" if vclock == "map" else b"\x91") + dots
    v = uint(val, vw)
    if form == "array":
        body = b"\x92" + vc + v
    else:
        kc, kv = (b"\xa5clock", b"\xa3val") if keys == "name" else (b"\x00", b"\x01")
        fields = [kc + vc, kv + v]
        if drop_val:
            fields = fields[:1]
        if order == "vc":
            fields.reverse()
        if extra:
            fields.insert(1, b"\xa4note\x92\x07\xa1x")
        if dup:
            fields.append(kc + vc)
        body = map_hdr(len(fields)) + b"".join(fields)
    tag = {"name": b"\xa3Put", "idx0": b"\x00", "idx1": b"\x01", "unknown": b"\xa3Pux", "two": b"\xa3Put"}[variant]
    if variant == "two":
        return b"\x82" + tag + body + b"\xa3Pux" + body
    return b"\x81" + tag + body


def ops_file(puts, count=None, force16=False):
    """clear text of an op file: the data version, then Vec<Op> of already encoded puts"""
    return APP + arr_hdr(len(puts) if count is None else count, force16) + b"".join(puts)


def P(dots, val):
    return ("Put", C.VClock(dots), val)


def enc(op, **kw):
    return put(sorted(op[1].dots.items()), op[2], **kw)


# ------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, purpose, target, steps, facts=None, want=None, host=(0, 0), rc=None,
                 host_decode=0):
        self.name = name
        self.family = name[0]
        self.purpose = purpose
        self.target = target
        self._steps = steps         # a list, or a builder -> (steps, facts) run at first use
        self._facts = facts or {}
        self.want = want            # the final values in `vals` order where the issue states them
        self.host = host            # (mv_host_merge, mv_host_apply) counts the whole case runs up
        self.rc = rc                # return code per step (default: 0 each)
        self.host_decode = host_decode  # files the device decode hands to the host decoder

    def _build(self):
        if callable(self._steps):
            self._steps, self._facts = self._steps()

    @property
    def steps(self):
        self._build()
        return self._steps

    @property
    def facts(self):
        self._build()
        return self._facts

    def __repr__(self):
        return self.name


def ops_step(op_lists, canonical=True, first_version=0, **kw):
    """one file per op list, writers 0.. in load_ops order, version `first_version` each"""
    files, decoded = [], []
    for i, ops in enumerate(op_lists):
        body = C.enc_mvreg_ops(ops) if canonical else arr_hdr(len(ops)) + b"".join(enc(o, **kw) for o in ops)
        files.append((APP + body, i, first_version))
        decoded.append(list(ops))
    return ("ops", [writer(i) for i in range(len(op_lists))], files, decoded)


def raw_step(clears, versions=None):
    """files given as clear texts, one writer each: decoded by the oracle"""
    versions = versions or [0] * len(clears)
    return ("ops", [writer(i) for i in range(len(clears))], [(c, i, versions[i]) for i, c in enumerate(clears)], None)


def state_file(vals, nov=None):
    r = C.MVReg()
    r.vals = [(C.VClock(d), v) for d, v in vals]
    return C.serialize("mvreg", C.VClock(nov or {writer(9): 1}), r)


def split(ops, k):
    """ops in k contiguous runs (empty ones dropped)"""
    q, r = divmod(len(ops), k)
    out, i = [], 0
    for j in range(k):
        n = q + (j < r)
        if n:
            out.append(ops[i:i + n])
        i += n
    return out


def _family_a():
    a, b, c = actor(0), actor(1), actor(2)
    H = 1 << 63
    sets = {
        "A1": ([P({a: H}, 1), P({a: H, b: H}, 2)], [2],
               "sums 2^63 and 2^64: a lost carry makes the dominated put the round's winner"),
        "A2": ([P({c: U}, 1), P({a: U, b: U}, 2), P({a: U, b: U, c: U}, 3)], [3],
               "sum_hi 0, 1, 2: only the clock of hi 2 survives"),
        "A3": ([P({c: 5}, 1), P({a: H, b: H, c: 5}, 2)], [2],
               "equal sum_lo, different sum_hi: a compare that ignored hi lets the other put win"),
        "A5": ([P({**{actor(k): U for k in range(299)}, actor(299): U - 1}, 1), P({actor(k): U for k in range(300)}, 2)],
               [2], "300 entries of 2^64 - 1 (hi 299) against the same clock one lower in one entry"),
    }
    out = []
    for name, (ops, want, purpose) in sets.items():
        for tag, seq in (("first", ops), ("last", ops[::-1])):
            out.append(Case("%s_dominated_%s" % (name, tag), purpose,
                            "k_mv_prep hi += lo < c; mv_better x.hi != y.hi",
                            [ops_step(split(seq, 2))], {"sums": [sum(o[1].dots.values()) for o in seq]}, want))
    ops = [P({a: U, b: 1}, 1), P({a: 1, b: U}, 2)]
    for tag, seq in (("ab", ops), ("ba", ops[::-1])):
        out.append(Case("A4_equal_sums_%s" % tag, "equal 128-bit sums, concurrent: both survive in insertion order",
                        "mv_better prio; k_mv_kill keeps the concurrent one", [ops_step([seq])],
                        {"sums": [1 << 64, 1 << 64]}, [o[2] for o in seq]))
    return out


def _family_b():
    a, b, c = actor(0), actor(1), actor(2)
    out = [Case("B1_op_tie_latest_wins", "equal clocks in one batch go to the latest op, which moves last",
                "k_mv_argmax prio = i (later_wins)", [ops_step([[P({a: 1}, 1), P({b: 1}, 2)], [P({a: 1}, 3)]])],
                want=[2, 3])]
    st = state_file([({a: 1}, 1), ({b: 1}, 2)])
    out.append(Case("B2_state_then_op_ingest", "an op equal to a committed value's clock replaces it at the end",
                    "mvreg_commit prefix K; k_mv_argmax prio", [("states", [st]), ops_step([[P({a: 1}, 3)]])], want=[2, 3]))
    out.append(Case("B2_state_then_op_apply", "the same through apply_ops",
                    "ds_apply_local_ops -> mvreg_commit", [("states", [st]), ("apply", C.enc_mvreg_ops([P({a: 1}, 3)]))],
                    want=[2, 3]))
    out.append(Case("B3_merge_tie_earliest_wins", "equal clocks in a merge keep this core's value and its place",
                    "k_mv_argmax prio = n - 1 - i (merge)",
                    [("states", [st]), ("states", [state_file([({b: 1}, 7), ({a: 1}, 8), ({c: 1}, 9)])])], want=[1, 2, 9]))
    many = [P({actor(k): 1}, 1000 + k) for k in range(300)]
    out.append(Case("B4_300_survivors_then_cover", "300 pairwise concurrent puts survive in insertion order "
                    "(one round and one host wait each); a put covering them all leaves one",
                    "mvreg_survivors round loop; sort of the winners",
                    [ops_step(split(many, 3)), ops_step([[P({actor(k): 1 for k in range(300)}, 7)]], first_version=1)],
                    {"survivors_first_batch": 300}, want=[7]))
    seq = [P({}, 100), P({a: 1}, 1), P({}, 101), P({b: 1}, 2), P({}, 102)]
    out.append(Case("B5_empty_clocks", "puts with an empty clock first, in the middle and last are ignored "
                    "and shift nobody", "k_mv_prep alive = cbeg[i + 1] > cbeg[i]", [ops_step([seq[:2], seq[2:]])], want=[1, 2]))
    return out


def _family_c():
    out = []
    z = actor(9, 0xB0)
    for k, pos in ((256, 255), (257, 256), (513, 512), (513, 255), (513, 256)):
        W = P({actor(j): 10 for j in range(k)}, 1)
        D = P({actor(pos): 10}, 2)
        facts = {"entries": k, "decisive": pos}
        out.append(Case("C1_scatter_k%d_pos%d" % (k, pos), "a put covered only by entry %d of a %d-entry winner dies" % (pos, k),
                        "k_mv_final scatter e += kBlock", [ops_step([[W], [D]])], facts, [1]))
        C3 = P({actor(pos): 3, z: 1}, 3)
        out.append(Case("C2_clear_k%d_pos%d" % (k, pos), "a stale wclock entry %d of the first winner would kill a live "
                        "put in the second winner's round" % pos, "k_mv_clear e += kBlock",
                        [ops_step([[W], [P({z: 5}, 2), C3]])], facts, [1, 2, 3]))
    return out


D_SIZES = (1, 255, 256, 257, 65536 + 257, 262144 + 700)
_D_SPOTS = (0, 255, 256, 65536 + 3, 262144 + 5)


def d_ops(n):
    """put i = the dominated chain {A[i % 7]: 1 + i // 7}, but a one-entry marker from an actor of
    its own at the strategic indices; -> (ops, marker indices)"""
    A = [actor(j) for j in range(7)]
    marks = sorted({i for i in _D_SPOTS + (n - 1,) if 0 <= i < n})
    ops = [P({A[i % 7]: 1 + i // 7}, i) for i in range(n)]
    for j, i in enumerate(marks):
        ops[i] = P({actor(j, 0xC0): 1}, i)
    return ops, marks


def d_case(n, prefix):
    """built at first use: the two largest hold hundreds of thousands of op tuples"""
    total = n + prefix
    return Case("D_n%d%s" % (n, "_after_state" if prefix else ""),
                "%d candidates%s: markers at the block / grid edges survive, the chain leaves its tops"
                % (total, " (3 committed values first)" if prefix else ""),
                "k_mv_argmax grid stride; k_mv_final b += kBlock", lambda: _d_build(n, prefix))


def _d_build(n, prefix):
    ops, marks = d_ops(n)
    nf = 1 if n == 1 else 6 if n < 1000 else 64
    nw = 1 if n == 1 else 3 if n < 1000 else 8
    runs = split(ops, nf)
    per = len(runs) // nw
    files = [(APP + C.enc_mvreg_ops(r), i // per, i % per) for i, r in enumerate(runs)]
    steps = []
    if prefix:
        steps.append(("states", [state_file([({actor(j, 0xD0): 1}, 900 + j) for j in range(prefix)])]))
    steps.append(("ops", [writer(i) for i in range(nw)], files, runs))
    facts = {"n": n, "prefix": prefix, "markers": marks, "n_blk": n_blk(n + prefix),
             "file_bytes": [len(f[0]) for f in files]}
    return steps, facts


def _family_d():
    return [d_case(n, 0) for n in D_SIZES] + [d_case(255, 3), d_case(65536 + 257, 3)]


_BOUNDS = (0x7f, 0x80, 0xff, 0x100, 0xffff, 0x10000, (1 << 32) - 1, 1 << 32, U)


def _e_forms():
    """name -> (list of encoded puts, purpose); every put's clock uses actors of its own so that
    all of them survive and the state shows each decoded counter and value"""
    f = {}
    f["widths"] = ([put([(actor(j), b)], _BOUNDS[-1 - j]) for j, b in enumerate(_BOUNDS)],
                   "counters and val at every integer width boundary and 2^64 - 1")
    f["non_minimal"] = ([put([(actor(0), 5)], 5, cw="cd", vw="cf"), put([(actor(1), 5)], 6, cw="cf", vw="cd"),
                         put([(actor(2), 0x7f)], 0x80, cw="ce", vw="ce")], "integers wider than they need")
    sizes = []
    for n, ctr in ((1, 40), (15, 30), (16, 20), (17, 10)):
        sizes.append(put([(actor(j), ctr) for j in range(n)], n))
    sizes.append(put([(actor(j), 50) for j in range(20, 23)], 3, map16=True))
    f["clock_maps"] = (sizes, "clock maps of 1, 15, 16, 17 entries (fixmap, map16) and a map16 header for 3")
    two = [[(actor(0), 3), (actor(1), 4)], [(actor(2), 5)]]
    f["array_body"] = ([put(c, 10 + i, form="array") for i, c in enumerate(two)], "Put body as [clock, val]")
    f["by_index"] = ([put(c, 20 + i, keys="index") for i, c in enumerate(two)], "fields keyed by index")
    f["val_first"] = ([put(c, 30 + i, order="vc") for i, c in enumerate(two)], "val before clock")
    f["unknown_field"] = ([put(c, 40 + i, extra=True) for i, c in enumerate(two)], "an unknown third field, skipped")
    f["variant_index"] = ([put(c, 50 + i, variant="idx0") for i, c in enumerate(two)], "variant by index 0")
    f["vclock_array"] = ([put(c, 60 + i, vclock="array") for i, c in enumerate(two)], "VClock as an array of one")
    kw = [dict(), dict(form="array"), dict(keys="index", order="vc"), dict(extra=True, variant="idx0"),
          dict(vclock="array", cw="cf"), dict(map16=True, vw="cf"), dict(form="array", vclock="array", variant="idx0")]
    f["mixed"] = ([put([(actor(j), 7 + j), (actor(100 + j), 1)], 70 + j, **k) for j, k in enumerate(kw)],
                  "every form in one file")
    return f


def _e_rejects():
    one = [(actor(0), 3)]
    good = put(one, 1)
    cut = ops_file([good, put([(actor(1), 0x1234), (actor(2), 0x5678)], 2)])
    return {
        "duplicate_field": ops_file([good, put(one, 2, dup=True)]),
        "missing_val": ops_file([good, put(one, 2, drop_val=True)]),
        "variant_index_1": ops_file([good, put(one, 2, variant="idx1")]),
        "variant_unknown": ops_file([good, put(one, 2, variant="unknown")]),
        "enum_two_entries": ops_file([good, put(one, 2, variant="two")]),
        "negative_val": ops_file([good, put(one, 2, vw="neg")]),
        "cut_in_clock_entry": cut[:-(1 + 4 + 3 + 10)],   # inside the last entry's actor
        "count_past_file": ops_file([good, put([(actor(1), 1)], 2)], count=0xffff),
    }


def _family_e():
    out = []
    for name, (puts, purpose) in _e_forms().items():
        out.append(Case("E_accept_" + name, purpose, "ds_parse_mvreg_ops / ds_struct2 / ds_vclock / rd_u64",
                        [raw_step([ops_file(puts)])], {"puts": len(puts)}))
    before = [P({actor(50): 2}, 5)]
    after = [P({actor(51): 2}, 6)]
    for name, clear in _e_rejects().items():
        good0 = APP + C.enc_mvreg_ops([P({actor(60): 1}, 8)])
        good2 = APP + C.enc_mvreg_ops([P({actor(61): 1}, 9)])
        out.append(Case("E_reject_" + name, "a bad file between two good ones: status 12, nothing folded, "
                        "and the next batch still folds", "ds_parse_mvreg_ops kDsErr -> CE_ERR_DECODE",
                        [ops_step([before]), raw_step([good0, clear, good2], versions=[1, 0, 0]),
                         ops_step([after], first_version=1)],
                        {"statuses": [0, 12, 0]}, want=[5, 6], rc=[0, 12, 0]))
    desc = ops_file([put([(actor(3), 4), (actor(1), 9)], 1), put([(actor(1), 2)], 2)])
    rep = ops_file([put([(actor(1), 9), (actor(2), 1), (actor(1), 2)], 1), put([(actor(1), 5)], 2)])
    out.append(Case("E_host_descending_actors", "clock actors descending: the host decoder's file",
                    "ds_vclock cmp <= 0 -> kDsHost", [raw_step([desc])], want=[1], host_decode=1))
    out.append(Case("E_host_repeated_actor", "a repeated actor in a clock: the later value wins ({1: 2, 2: 1}), so the "
                    "second put {1: 5} is concurrent", "ds_vclock cmp <= 0 -> kDsHost", [raw_step([rep])], want=[1, 2],
                    host_decode=1))
    return out


def _family_f():
    a, b = actor(0), actor(1)
    chain = [({a: 1}, 1), ({a: 2}, 2)]
    twins = [({a: 1}, 1), ({a: 1}, 2)]
    merges = [
        ("F1_chain_into_empty", None, chain, [1, 2], 1),
        ("F2_twins_into_empty", None, twins, [1, 2], 1),
        ("F3_chain_into_concurrent", [({b: 1}, 9)], chain, [9, 1, 2], 1),
        ("F4_chain_into_between", [({a: 2}, 9)], [({a: 1}, 1), ({a: 3}, 2)], [1, 2], 1),
        ("F5_empty_clock_into_empty", None, [({}, 2)], [2], 1),
        ("F6_twins_into_concurrent", [({b: 1}, 9)], twins, [9, 1, 2], 1),
        ("F7_empty_clock_twice", [({}, 2)], [({}, 3)], [2], 2),
    ]
    out = []
    for name, mine, other, want, host_merges in merges:
        steps = ([("states", [state_file(mine)])] if mine else []) + [("states", [state_file(other, {writer(8): 2})])]
        out.append(Case(name, "a state file whose vals is no antichain of non-empty clocks merges by "
                        "MVReg::merge exactly", "mvreg_merge_one: mv_regular -> mvreg_host_merge", steps,
                        want=want, host=(host_merges, 0)))
    out.append(Case("F8_ops_on_irregular_state", "ops on vals that hold a dominated value: sequential apply keeps it "
                    "until an op covers it; then the device route again",
                    "mvreg_fold_ops: mv_irregular -> mvreg_host_apply",
                    [("states", [state_file(chain)]), ops_step([[P({b: 1}, 3)]]),
                     ("apply", C.enc_mvreg_ops([P({b: 2}, 4)])),
                     ops_step([[P({a: 9, b: 9}, 5)]], first_version=1), ops_step([[P({actor(2): 1}, 6)]], first_version=2)],
                    {"vals_after_step": [[1, 2], [1, 2, 3], [1, 2, 4], [5], [5, 6]]}, want=[5, 6], host=(1, 3)))
    out.append(Case("F9_regular_file_into_irregular_state", "a regular file merged while this core's vals is irregular "
                    "takes the host route too", "mvreg_merge_one: d->mv_irregular",
                    [("states", [state_file(chain)]), ("states", [state_file([({b: 1}, 7)], {writer(7): 1})])],
                    want=[1, 2, 7], host=(2, 0)))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(_family_a() + _family_b() + _family_c() + _family_d() + _family_e() + _family_f())


def by_name(name):
    return {c.name: c for c in all_cases()}[name]


# ------------------------------------------------------------------------------------------
# the oracle over a case's steps (no sealing: the files' clear texts, decoded as the core would)
# ------------------------------------------------------------------------------------------
def decode_files(step):
    """-> (statuses, ops per file or None)"""
    _, _, files, decoded = step
    st, ops = [], []
    for i, (clear, _, _) in enumerate(files):
        if decoded is not None:
            st.append(0)
            ops.append(decoded[i])
            continue
        try:
            ops.append(C.dec_ops("mvreg", clear[16:]))
            st.append(0)
        except C.DecodeError:
            ops.append(None)
            st.append(12)
    return st, ops


def applied_ops(step, nov):
    """lib.rs:516-544 over decoded files: -> (rc, statuses, [op lists applied, in order]); nov
    advances as read_remote_ops advances it"""
    _, writers, files, _ = step
    st, ops = decode_files(step)
    first = next((s for s in st if s), 0)
    if first:
        return first, st, []
    out = []
    for i, (_, fa, fv) in enumerate(files):
        w = writers[fa]
        expected = nov.get(w)
        if fv < expected:
            continue
        if expected < fv:
            st[i] = 13
            return 13, st, out
        out.append(ops[i])
        nov.apply(w, expected + 1)
    return 0, st, out


def run_steps(case, fold_ops, merge, me=ME):
    """Applies the case's steps to a C.Core("mvreg"); `fold_ops(reg, [op lists])` and
    `merge(reg, other reg)` change core.state.  -> (core, [(rc, statuses, values, state bytes)] per step)"""
    core = C.Core("mvreg")
    trace = []
    for step in case.steps:
        rc, st = 0, None
        if step[0] == "states":
            for sw in step[1]:
                nov, other = C.dec_state("mvreg", sw)
                merge(core.state, other)
                core.nov.merge(nov)
            st = [0] * len(step[1])
        elif step[0] == "ops":
            rc, st, lists = applied_ops(step, core.nov)
            if lists:
                fold_ops(core.state, lists)
        else:
            fold_ops(core.state, [C.dec_ops("mvreg", step[1])])
            core.nov.apply(me, core.nov.get(me) + 1)
        trace.append((rc, st, [v for _, v in core.state.vals], core.serialize()))
    return core, trace


def _oracle_fold(reg, lists):
    for ops in lists:
        for op in ops:
            reg.apply(op)


def run_oracle(case, me=ME):
    """the expected trace: sequential MVReg::apply / MVReg::merge of oracle/crdts.py"""
    return run_steps(case, _oracle_fold, lambda reg, other: reg.merge(other), me)
