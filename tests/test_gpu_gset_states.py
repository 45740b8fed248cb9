"""GPU tests of the device reader and the HBM-resident writer of GSet state files: every case
compares state_bytes() and the per-file statuses with tests/gset_model.py, and the path counts
gset_states_device_read / gset_states_host_read / gset_state_bytes_device say which route ran.

A body is read on the device when its elements are unsigned markers whose widths never decrease
(runs of fixint, cc, cd, ce, cf); every other file goes to the host parser.  The two counts are
added when a call has taken its files: a rejected call leaves them as they were."""
import ctypes
import random

import msgpack
import numpy as np
import pytest

import crdtenc
import gset_model as gm
from oracle.crdts import VClock

pytestmark = pytest.mark.gpu
H = bytes.fromhex
APP = H("aadfd5a66e194b24a8024fa27c72f20c")
CORE = crdtenc.CORE_VERSION
GS = crdtenc.STATE_GSET
U64 = (1 << 64) - 1
WIDTHS = ["fixint", "cc", "cd", "ce", "cf"]
WIDTH_BITS = {"fixint": (0, 7), "cc": (7, 8), "cd": (8, 16), "ce": (16, 32), "cf": (32, 64)}
PAYLOAD = {"cc": 1, "cd": 2, "ce": 4, "cf": 8}
EDGES = [0, 127, 128, 255, 256, 65535, 65536, (1 << 32) - 1, 1 << 32, U64]


@pytest.fixture(scope="module")
def ctx():
    c = crdtenc.Context(0)
    yield c
    c.close()


def seal(oracle, key, clear, rng):
    st, enc = oracle.cryptor_encrypt(key, rng.randbytes(24), clear)
    assert st == 0
    return CORE + enc


def new_core(ctx, key, **kw):
    c = crdtenc.Core(ctx, kind=GS, supported=[APP], current_data_version=APP, **kw)
    c.set_latest_key(key)
    return c


def member_of(rng, width):
    lo, hi = WIDTH_BITS[width]
    return rng.randrange(1 << lo if lo else 0, 1 << hi)


def el(width, v):
    """v in the given marker's form, minimal or not"""
    return bytes([v]) if width == "fixint" else bytes([0xcc + WIDTHS.index(width) - 1]) + v.to_bytes(PAYLOAD[width], "big")


def hdr(n, form=None):
    form = form or ("fix" if n < 16 else "dc" if n < 65536 else "dd")
    return {"fix": lambda: bytes([0x90 | n]), "dc": lambda: b"\xdc" + n.to_bytes(2, "big"),
            "dd": lambda: b"\xdd" + n.to_bytes(4, "big")}[form]()


def nov_of(rng, k=2):
    v = VClock()
    for _ in range(k):
        v.apply(rng.randbytes(16), rng.randrange(1, 1 << 20))
    return v


def sw_raw(nov, body):
    """the writer's head (82 b0"next_op_versions" clock a5"state" 81 a5"value") and a raw array"""
    head = gm.serialize(nov, gm.GSet())
    assert head.endswith(b"\xa5value\x90")
    return head[:-1] + body


def counts(core):
    return core.path_count("gset_states_device_read"), core.path_count("gset_states_host_read")


def to_device(torch, data, pad=0):
    d = torch.tensor(list(data) + [0] * pad, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return d


def ingest_check(ctx, oracle, monkeypatch, rng, key, sws, want_counts, want_rc=0, core=None, model=None):
    """ingest_states of the StateWrappers `sws` into a core and the model: same rc and statuses,
    same state bytes, the path counts as stated; then the same call under CE_HOST_STATES=1 into a
    fresh core gives the same answers.  Returns the statuses."""
    files = [seal(oracle, key, APP + sw, rng) for sw in sws]
    own = core is None
    if own:
        core, model = new_core(ctx, key), gm.Core()
    before, c0 = core.state_bytes(), counts(core)
    rc, st = core.ingest_states(files)
    orc, ost = model.read_remote_states(key, [APP], files)
    assert (rc, st) == (orc, ost) and rc == want_rc, (rc, st, orc, ost, ctx.last_error())
    assert core.state_bytes() == model.serialize()
    got = tuple(a - b for a, b in zip(counts(core), c0))
    assert got == tuple(want_counts), got
    if rc:
        assert core.state_bytes() == before
    if own:
        monkeypatch.setenv("CE_HOST_STATES", "1")
        host = new_core(ctx, key)
        assert host.ingest_states(files) == (rc, st) and host.state_bytes() == core.state_bytes()
        assert counts(host) == (0, 0)
        monkeypatch.delenv("CE_HOST_STATES")
        host.close()
        core.close()
    return st


# ------------------------------------------------------------------ the two that need the feature
def test_canonical_files_are_read_on_the_device(ctx, oracle, monkeypatch):
    rng = random.Random(1)
    key = rng.randbytes(32)
    sws = [gm.serialize(nov_of(rng), gm.GSet(member_of(rng, rng.choice(WIDTHS)) for _ in range(n))) for n in (50, 300)]
    ingest_check(ctx, oracle, monkeypatch, rng, key, sws, (2, 0))


def test_state_bytes_device_counts(ctx, oracle):
    torch = pytest.importorskip("torch")
    rng = random.Random(2)
    key = rng.randbytes(32)
    core = new_core(ctx, key)
    want = gm.serialize(nov_of(rng), gm.GSet(EDGES))
    assert core.merge_state(want) == 0
    dev = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    rc, n = core.state_bytes_device(dev.data_ptr(), dev.numel())
    assert rc == 0 and bytes(dev[:n].cpu().numpy()) == want
    assert core.path_count("gset_state_bytes_device") == 1
    core.close()


# ------------------------------------------------------------------ every route
@pytest.mark.parametrize("route", ["ingest_states", "ingest_states_iov", "ingest_states_device", "merge_state_device",
                                   "read_remote"])
@pytest.mark.parametrize("order", ["states_then_ops", "ops_then_states"])
def test_every_route(ctx, oracle, tmp_path, route, order):
    """Two overlapping canonical state files, before and after ops (the shape of test_states in
    test_gpu_gset.py); both are decoded in HBM on every route."""
    torch = pytest.importorskip("torch")
    rng = random.Random(3)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(3))
    shared = [member_of(rng, rng.choice(WIDTHS)) for _ in range(40)]
    m1 = shared + [member_of(rng, "cf") for _ in range(30)] + [0, U64]
    m2 = shared[10:] + [member_of(rng, "ce") for _ in range(25)]
    n1, n2 = VClock(), VClock()
    n1.apply(actors[0], 2)
    n2.apply(actors[1], 1)
    n2.apply(actors[0], 1)
    sws = [gm.serialize(n1, gm.GSet(m1)), gm.serialize(n2, gm.GSet(m2))]
    sfiles = [seal(oracle, key, APP + sw, rng) for sw in sws]
    kw = {}
    if route == "read_remote":
        remote = str(tmp_path / "remote")
        kw = dict(local_path=str(tmp_path / "l1"), remote_path=remote, flags=crdtenc.OPEN_CREATE)
    core, model = new_core(ctx, key, **kw), gm.Core()

    def states():
        if route == "ingest_states":
            assert core.ingest_states(sfiles) == (0, [0, 0])
        elif route == "ingest_states_iov":
            assert core.ingest_states_iov(sfiles) == (0, [0, 0])
        elif route == "ingest_states_device":
            blob = b"".join(sfiles)
            offs = np.zeros(3, dtype=np.int64)
            offs[1:] = np.cumsum([len(f) for f in sfiles])
            d_blob = to_device(torch, blob, pad=64)
            d_offs = torch.tensor(offs, device="cuda")
            torch.cuda.synchronize()
            assert core.ingest_states_device(d_blob.data_ptr(), d_offs.data_ptr(), 2, len(blob), want_status=True) == (0, [0, 0])
        elif route == "merge_state_device":
            for sw in sws:
                d = to_device(torch, sw)
                assert core.merge_state_device(d.data_ptr(), len(sw)) == 0
        else:
            store = crdtenc.Storage(str(tmp_path / "lw"), remote)
            for f in sfiles:
                store.store_state(f)
            assert core.read_remote() == 0
        assert model.read_remote_states(key, [APP], sfiles)[0] == 0
        assert core.state_bytes() == model.serialize()
        assert counts(core) == (2, 0)

    def ops():
        bodies = [gm.enc_ops(rng.sample(shared, 10) + [member_of(rng, "cf") for _ in range(10)]) for _ in range(9)]
        files = [seal(oracle, key, APP + b, rng) for b in bodies]
        fa = [w for w in range(3) for _ in range(3)]
        vers = [model.nov.get(actors[w]) + v for w in range(3) for v in range(3)]
        rc, st = core.ingest_ops(files, actors, fa, vers)
        assert (rc, st) == model.read_remote_ops(key, [APP], files, [actors[i] for i in fa], vers) == (0, [0] * 9)
        assert core.state_bytes() == model.serialize()
    for step in ((states, ops) if order == "states_then_ops" else (ops, states)):
        step()
    core.close()


# ------------------------------------------------------------------ run structure
@pytest.mark.parametrize("width", WIDTHS)
def test_each_width_alone(ctx, oracle, monkeypatch, width):
    """counts around the four-per-round step, a wave and a block"""
    rng = random.Random(10 + WIDTHS.index(width))
    key = rng.randbytes(32)
    for n in (0, 1, 3, 4, 5, 63, 64, 65, 257):
        body = hdr(n) + b"".join(el(width, member_of(rng, width)) for _ in range(n))
        ingest_check(ctx, oracle, monkeypatch, rng, key, [sw_raw(nov_of(rng), body)], (1, 0))


RUNS = {
    "all_five_of_length_1": ["fixint", "cc", "cd", "ce", "cf"],
    "runs_1_3_9": ["fixint"] * 3 + ["cd"] * 2 + ["cf"] * 4,
    "runs_2_5": ["cc"] * 5 + ["ce"] * 3,
}


@pytest.mark.parametrize("name", list(RUNS))
def test_runs_present_and_missing(ctx, oracle, monkeypatch, name):
    rng = random.Random(20)
    key = rng.randbytes(32)
    ws = RUNS[name]
    body = hdr(len(ws)) + b"".join(el(w, member_of(rng, w)) for w in ws)
    ingest_check(ctx, oracle, monkeypatch, rng, key, [sw_raw(nov_of(rng), body)], (1, 0))


def test_boundary_members(ctx, oracle, monkeypatch):
    rng = random.Random(21)
    key = rng.randbytes(32)
    sw = gm.serialize(nov_of(rng), gm.GSet(EDGES))
    assert sw.endswith(b"\x9a\x00\x7f\xcc\x80\xcc\xff\xcd\x01\x00\xcd\xff\xff\xce\x00\x01\x00\x00\xce\xff\xff\xff\xff"
                       b"\xcf\x00\x00\x00\x01\x00\x00\x00\x00\xcf" + b"\xff" * 8)
    ingest_check(ctx, oracle, monkeypatch, rng, key, [sw] + [gm.serialize(VClock(), gm.GSet([m])) for m in EDGES],
                 (1 + len(EDGES), 0))


@pytest.mark.parametrize("form,n", [("fix", 3), ("dc", 3), ("dd", 3), ("dc", 15), ("dd", 70), ("dc", 300)])
def test_array_headers(ctx, oracle, monkeypatch, form, n):
    rng = random.Random(22)
    key = rng.randbytes(32)
    ms = sorted(member_of(rng, rng.choice(WIDTHS)) for _ in range(n))
    body = hdr(n, form) + gm.enc_ops(ms)[len(hdr(n)):]
    ingest_check(ctx, oracle, monkeypatch, rng, key, [sw_raw(nov_of(rng), body)], (1, 0))


def test_non_minimal_forms_are_taken_on_the_device(ctx, oracle, monkeypatch):
    rng = random.Random(23)
    key = rng.randbytes(32)
    body = hdr(7) + el("fixint", 9) + el("cc", 5) + el("cd", 6) + el("cd", 6) + el("ce", 0) + el("cf", 5) + el("cf", 1 << 40)
    st = ingest_check(ctx, oracle, monkeypatch, rng, key, [sw_raw(nov_of(rng), body), sw_raw(VClock(), hdr(1) + el("cf", 0))],
                      (2, 0))
    assert st == [0, 0]


# ------------------------------------------------------------------ payload bytes that look like markers
def test_payloads_that_look_like_markers(ctx, oracle, monkeypatch):
    """A run ends at the first byte, at the run's stride, that is not its marker: payload bytes
    after that point equal to a marker must not move a boundary."""
    rng = random.Random(24)
    key = rng.randbytes(32)
    cf_like = [int.from_bytes(bytes(p), "big") for p in ([0xcf] * 8, [0xce] * 8, [0xcd] * 8, [0xcd, 0xcf, 0xce, 0xcd] * 2,
                                                         [0xcc] * 8, [0xcf, 0x00] * 4)]
    bodies = [
        hdr(2) + el("ce", 0xcdcdcdcd) + el("ce", 0xcccccccc),
        hdr(len(cf_like)) + b"".join(el("cf", v) for v in cf_like),
        # a long cd run, then directly cf elements made of cd / ce / cf bytes
        hdr(300 + len(cf_like)) + b"".join(el("cd", 0xcd00 + (i & 0xff)) for i in range(300)) +
        b"".join(el("cf", v) for v in cf_like),
        # every run present, every payload of marker bytes
        hdr(9) + b"\x01" + el("cc", 0xcc) + el("cc", 0xcd) + el("cd", 0xcdcd) + el("cd", 0xcecf) + el("ce", 0xcecececf) +
        el("ce", 0xcfcfcfcf) + el("cf", cf_like[0]) + el("cf", cf_like[3]),
    ]
    sws = [sw_raw(nov_of(rng), b) for b in bodies]
    ingest_check(ctx, oracle, monkeypatch, rng, key, sws, (4, 0))
    for sw in sws:  # and each alone
        ingest_check(ctx, oracle, monkeypatch, rng, key, [sw], (1, 0))


# ------------------------------------------------------------------ host fallbacks
def _pack(x):
    return msgpack.packb(x, use_bin_type=True)


def _fallbacks(rng):
    a = rng.randbytes(16)
    shared = [member_of(rng, rng.choice(WIDTHS)) for _ in range(40)]
    m1 = shared + [member_of(rng, "cf") for _ in range(30)] + shared[:7] + [0, U64]
    rng.shuffle(m1)
    cf = [el("cf", member_of(rng, "cf")) for _ in range(6)]
    nov = nov_of(rng)
    # name: (StateWrapper, status, (device, host) counts of a call that holds only this file)
    return {
        "descending_width": (_pack({"next_op_versions": {"dots": {a: 2}}, "state": {"value": m1}}), 0, (0, 1)),
        "d3_non_negative": (sw_raw(nov, hdr(3) + el("ce", 70000) + b"\xd3" + (1 << 40).to_bytes(8, "big") + cf[0]), 0, (0, 1)),
        "negative": (sw_raw(nov, hdr(3) + b"\x05\xff" + cf[0]), 12, (0, 0)),
        "count_one_above": (sw_raw(nov, hdr(7) + b"".join(cf)), 12, (0, 0)),
        "count_one_below": (sw_raw(nov, hdr(5) + b"".join(cf)), 0, (1, 0)),  # (trailing bytes are ignored: device)
        "last_cf_cut": (sw_raw(nov, hdr(6) + b"".join(cf)[:-1]), 12, (0, 0)),
        "struct_as_array": (_pack([{"dots": {a: 1}}, [sorted(shared)]]), 0, (0, 1)),
        "unknown_extra_key": (_pack({"next_op_versions": {"dots": {a: 3}}, "extra": [1, {"x": 2}], "state": {"value": sorted(shared)}}),
                              0, (0, 1)),
    }


@pytest.mark.parametrize("name", ["descending_width", "d3_non_negative", "negative", "count_one_above", "count_one_below",
                                  "last_cf_cut", "struct_as_array", "unknown_extra_key"])
def test_host_fallbacks(ctx, oracle, monkeypatch, name):
    rng = random.Random(25)
    key = rng.randbytes(32)
    sw, status, want = _fallbacks(rng)[name]
    st = ingest_check(ctx, oracle, monkeypatch, rng, key, [sw], want, want_rc=status)
    assert st == [status]


def test_device_files_mixed_with_a_fallback(ctx, oracle, monkeypatch):
    rng = random.Random(26)
    key = rng.randbytes(32)
    fb = _fallbacks(rng)
    good = [gm.serialize(nov_of(rng), gm.GSet(member_of(rng, rng.choice(WIDTHS)) for _ in range(n))) for n in (20, 200)]
    for name in ("descending_width", "struct_as_array", "d3_non_negative"):
        ingest_check(ctx, oracle, monkeypatch, rng, key, [good[0], fb[name][0], good[1]], (2, 1))


# ------------------------------------------------------------------ all or nothing
@pytest.mark.parametrize("fault", ["tag", "undecodable"])
def test_all_or_nothing(ctx, oracle, fault):
    rng = random.Random(27)
    key = rng.randbytes(32)
    core, model = new_core(ctx, key), gm.Core()
    first = gm.serialize(nov_of(rng), gm.GSet(member_of(rng, "cf") for _ in range(30)))
    assert core.merge_state(first) == 0
    model.merge_state(first)
    before, c0 = core.state_bytes(), counts(core)
    sws = [gm.serialize(nov_of(rng), gm.GSet(member_of(rng, rng.choice(WIDTHS)) for _ in range(100))) for _ in range(3)]
    if fault == "undecodable":
        sws[1] = sw_raw(nov_of(rng), hdr(3) + b"\x01\xc0\x02")
    files = [seal(oracle, key, APP + sw, rng) for sw in sws]
    if fault == "tag":
        b = bytearray(files[1])
        b[-1] ^= 0x40
        files[1] = bytes(b)
    rc, st = core.ingest_states(files)
    assert (rc, st) == model.read_remote_states(key, [APP], files) == ({"tag": 9, "undecodable": 12}[fault], [0, rc, 0])
    assert core.state_bytes() == before == model.serialize() and counts(core) == c0
    core.close()


# ------------------------------------------------------------------ neighbouring bytes
@pytest.mark.parametrize("count_off", [0, 1])
def test_neighbouring_bytes_are_not_read(ctx, oracle, count_off):
    """The StateWrapper inside a larger tensor, well-formed cf elements right before and after it:
    only `count` members arrive, and a count one above the elements is CE_ERR_DECODE although the
    bytes behind the buffer would supply the element."""
    torch = pytest.importorskip("torch")
    rng = random.Random(28)
    key = rng.randbytes(32)
    ms = [member_of(rng, "cf") for _ in range(70)]
    sw = sw_raw(nov_of(rng), hdr(70 + count_off) + b"".join(el("cf", m) for m in ms))
    around = [b"".join(el("cf", member_of(rng, "cf")) for _ in range(50)) for _ in range(2)]
    d = to_device(torch, around[0] + sw + around[1])
    core, model = new_core(ctx, key), gm.Core()
    rc = core.merge_state_device(d.data_ptr() + len(around[0]), len(sw))
    if count_off:
        assert rc == 12 and counts(core) == (0, 0)
        with pytest.raises(Exception):
            gm.dec_state(sw)
    else:
        model.merge_state(sw)
        assert rc == 0 and counts(core) == (1, 0) and model.state.value == set(ms)
    assert core.state_bytes() == model.serialize()
    core.close()


# ------------------------------------------------------------------ growth and size
def test_growth_past_the_default_table(ctx, oracle, monkeypatch):
    """40,000 cf members into a default core (65,536 slots, 32,768 claims): several segments, one
    growth; the same file again inserts nothing and grows nothing."""
    rng = random.Random(29)
    key = rng.randbytes(32)
    core, model = new_core(ctx, key), gm.Core()
    sw = gm.serialize(nov_of(rng), gm.GSet(member_of(rng, "cf") for _ in range(40000)))
    ingest_check(ctx, oracle, monkeypatch, rng, key, [sw], (1, 0), core=core, model=model)
    grows = core.path_count("gset_grows")
    assert grows >= 1 and len(model.state.value) == 40000
    before = core.state_bytes()
    ingest_check(ctx, oracle, monkeypatch, rng, key, [sw], (1, 0), core=core, model=model)
    assert core.path_count("gset_grows") == grows and core.state_bytes() == before
    core.close()


def test_tiny_table(ctx, oracle, monkeypatch):
    rng = random.Random(30)
    key = rng.randbytes(32)
    monkeypatch.setenv("CE_GSET_CAP", "16")
    core, model = new_core(ctx, key), gm.Core()
    monkeypatch.delenv("CE_GSET_CAP")
    for n in (1, 7, 8, 9, 40):
        sw = gm.serialize(nov_of(rng, 1), gm.GSet(member_of(rng, rng.choice(WIDTHS)) for _ in range(n)))
        ingest_check(ctx, oracle, monkeypatch, rng, key, [sw], (1, 0), core=core, model=model)
        grows = core.path_count("gset_grows")
        ingest_check(ctx, oracle, monkeypatch, rng, key, [sw], (1, 0), core=core, model=model)
        assert core.path_count("gset_grows") == grows
    assert core.path_count("gset_grows") >= 2
    core.close()


# ------------------------------------------------------------------ a pending sharded batch
def test_pending_batch_stays_pending(ctx, oracle):
    """A sharded ingest leaves a pending batch; a state file that overlaps it goes into the
    committed table: the state bytes before the commit show committed members only."""
    torch = pytest.importorskip("torch")
    rng = random.Random(31)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(2))
    core, model = new_core(ctx, key), gm.Core()
    ops = [[member_of(rng, "cf") for _ in range(20)] for _ in range(4)]
    files = [seal(oracle, key, APP + gm.enc_ops(o), rng) for o in ops]
    fa, vers = [0, 0, 1, 1], [0, 1, 0, 1]
    blob = b"".join(files)
    offs = np.zeros(5, dtype=np.int64)
    offs[1:] = np.cumsum([len(f) for f in files])
    d_blob = to_device(torch, blob, pad=64)
    d_offs = torch.tensor(offs, device="cuda")
    d_fa = torch.tensor(np.array(fa, dtype=np.int32), device="cuda")
    d_fv = torch.tensor(np.array(vers, dtype=np.int64), device="cuda")
    d_hi = torch.tensor(np.array([2, 2, 0], dtype=np.int64), device="cuda")  # the windows' ends, the flags word
    torch.cuda.synchronize()
    empty = core.state_bytes()
    rc = core.gset_ingest_ops_device_sharded(d_blob.data_ptr(), d_offs.data_ptr(), 4, len(blob), b"".join(actors),
                                             d_fa.data_ptr(), d_fv.data_ptr(), d_hi.data_ptr())
    assert rc == 0, ctx.last_error()
    assert core.state_bytes() == empty
    sw = gm.serialize(nov_of(rng), gm.GSet(ops[0][:10] + ops[3][5:] + [member_of(rng, "ce") for _ in range(15)]))
    sfile = seal(oracle, key, APP + sw, rng)
    assert core.ingest_states([sfile]) == (0, [0]) and counts(core) == (1, 0)
    only_state = gm.Core()
    only_state.merge_state(sw)
    assert core.state_bytes() == only_state.serialize()
    assert core.gset_pending_commit(True) == 0
    assert model.read_remote_states(key, [APP], [sfile])[0] == 0
    assert model.read_remote_ops(key, [APP], files, [actors[i] for i in fa], vers)[0] == 0
    assert core.state_bytes() == model.serialize()
    core.close()


# ------------------------------------------------------------------ the writer
def _mixed(rng, n):
    ms = set(EDGES)
    while len(ms) < n:
        ms.add(member_of(rng, rng.choice(WIDTHS)))
    return ms


@pytest.mark.parametrize("case", ["empty", "zero", "one_of_each_width", "mixed_5000"])
def test_writer_bytes(ctx, oracle, monkeypatch, case):
    torch = pytest.importorskip("torch")
    rng = random.Random(32)
    key = rng.randbytes(32)
    ms = {"empty": [], "zero": [0], "one_of_each_width": [member_of(rng, w) for w in WIDTHS]}.get(case) or \
        (_mixed(rng, 5000) if case == "mixed_5000" else [])
    model = gm.Core()
    model.merge_state(gm.serialize(nov_of(rng, 3), gm.GSet(ms)))
    want = model.serialize()
    dev = torch.full((len(want) + 64,), 0xa5, dtype=torch.uint8, device="cuda")
    for host_compact in (False, True):
        if host_compact:
            monkeypatch.setenv("CE_HOST_COMPACT", "1")
        core = new_core(ctx, key)
        monkeypatch.delenv("CE_HOST_COMPACT", raising=False)
        assert core.merge_state(want) == 0
        rc, n = core.state_bytes_device(dev.data_ptr(), dev.numel())
        torch.cuda.synchronize()
        got = bytes(dev.cpu().numpy())
        assert rc == 0 and n == len(want) and got[:n] == want and got[n:] == b"\xa5" * 64
        assert core.path_count("gset_state_bytes_device") == (0 if host_compact else 1)
        assert core.state_bytes() == want
        core.close()


def test_writer_buffer_too_small(ctx, oracle):
    torch = pytest.importorskip("torch")
    rng = random.Random(33)
    key = rng.randbytes(32)
    want = gm.serialize(nov_of(rng), gm.GSet(_mixed(rng, 500)))
    core = new_core(ctx, key)
    assert core.merge_state(want) == 0
    dev = torch.full((len(want),), 0x5a, dtype=torch.uint8, device="cuda")
    for cap in (len(want) - 1, 1, 0):
        rc, n = core.state_bytes_device(dev.data_ptr(), cap)
        torch.cuda.synchronize()
        assert rc == 64 and n == len(want) and bool((dev == 0x5a).all())
    assert core.path_count("gset_state_bytes_device") == 0
    rc, n = core.state_bytes_device(dev.data_ptr(), len(want))
    assert rc == 0 and n == len(want) and bytes(dev.cpu().numpy()) == want
    core.close()


def test_two_cores_converge_in_hbm(ctx, oracle):
    torch = pytest.importorskip("torch")
    rng = random.Random(34)
    key = rng.randbytes(32)
    cores, models = [new_core(ctx, key) for _ in range(2)], [gm.Core() for _ in range(2)]
    for r in range(2):
        sw = gm.serialize(nov_of(rng), gm.GSet(_mixed(rng, 1000 + 500 * r)))
        assert cores[r].merge_state(sw) == 0
        models[r].merge_state(sw)
    dev = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    for src, dst in ((0, 1), (1, 0)):
        rc, n = cores[src].state_bytes_device(dev.data_ptr(), dev.numel())
        assert rc == 0 and n == len(models[src].serialize())
        assert cores[dst].merge_state_device(dev.data_ptr(), n) == 0
        models[dst].merge_state(models[src].serialize())
    assert cores[0].state_bytes() == cores[1].state_bytes() == models[0].serialize() == models[1].serialize()
    for c in cores:
        assert c.path_count("gset_state_bytes_device") == 1 and counts(c) == (1, 0)
        c.close()
