"""GPU parity of CE_STATE_PNCOUNTER (crdts 7 PNCounter<Uuid>) through crdtenc.py and the C ABI,
bit-exact against tests/pncounter_model.py: state_bytes(), per-file statuses, and for
compactions the decrypted file and its content name.  Files are sealed with
oracle.cryptor_encrypt.  Without the kind, ce_core_open returns CE_ERR_INVALID_ARG and every
test here fails there."""
import os
import random

import msgpack
import numpy as np
import pytest

import crdtenc
import pncounter_model as pm
from oracle.crdts import VClock

pytestmark = pytest.mark.gpu
H = bytes.fromhex
APP = H("aadfd5a66e194b24a8024fa27c72f20c")
CORE = crdtenc.CORE_VERSION
PN = crdtenc.STATE_PNCOUNTER
# counters of each canonical width: fixint, cc, cd, ce, cf
WIDTH_BITS = {"fixint": (0, 7), "cc": (7, 8), "cd": (8, 16), "ce": (16, 32), "cf": (32, 64)}


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
    c = crdtenc.Core(ctx, kind=PN, supported=[APP], current_data_version=APP, **kw)
    c.set_latest_key(key)
    return c


def counter_of(rng, width):
    lo, hi = WIDTH_BITS[width]
    return rng.randrange(1 << lo if lo else 0, 1 << hi)


def op(actor, counter, d):
    return ((actor, counter), d)


def ingest_and_check(core, model, key, files, actors, fa, vers, want_rc=0):
    rc, st = core.ingest_ops(files, actors, fa, vers)
    orc, ost = model.read_remote_ops(key, [APP], files, [actors[i] for i in fa], vers)
    assert rc == orc == want_rc, (rc, orc, core.ctx.last_error())
    assert st == ost
    assert core.state_bytes() == model.serialize()


# ------------------------------------------------------------------ plane mix-up
def test_planes_do_not_mix(ctx, oracle):
    """One actor with Pos max 7 and Neg max 300 in the same file, then a file where only Neg
    occurs: each maximum lands in its own plane."""
    rng = random.Random(1)
    key = rng.randbytes(32)
    a, b = sorted(rng.randbytes(16) for _ in range(2))
    f0 = [op(a, 7, "Pos"), op(a, 300, "Neg"), op(a, 3, "Pos"), op(a, 299, "Neg"), op(a, 1, "Neg")]
    f1 = [op(a, 2, "Neg"), op(b, 70000, "Neg"), op(b, 5, "Neg")]
    files = [seal(oracle, key, APP + pm.enc_ops(x), rng) for x in (f0, f1)]
    core, model = new_core(ctx, key), pm.Core()
    ingest_and_check(core, model, key, files, [a], [0, 0], [0, 1])
    assert model.state.p.dots == {a: 7} and model.state.n.dots == {a: 300, b: 70000}
    core.close()


# ------------------------------------------------------------------ round boundaries
@pytest.mark.parametrize("width", list(WIDTH_BITS))
def test_round_boundaries(ctx, oracle, width):
    """Ops per file around the fast path's rounds (two ops per lane, 16 lanes: 32 per round) at
    every counter width; a third of the files name other actors too."""
    rng = random.Random(100 + list(WIDTH_BITS).index(width))
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(3))
    counts = [0, 1, 15, 16, 17, 31, 32, 33, 65]
    files, fa, vers = [], [], []
    for w in range(3):
        for v, cnt in enumerate(counts):
            ops = [op(actors[w] if (v + w) % 3 else rng.choice(actors), counter_of(rng, width), rng.choice(pm.DIRS))
                   for _ in range(cnt)]
            files.append(seal(oracle, key, APP + pm.enc_ops(ops), rng))
            fa.append(w)
            vers.append(v)
    core, model = new_core(ctx, key), pm.Core()
    ingest_and_check(core, model, key, files, actors, fa, vers)
    core.close()


def test_every_tail_length(ctx, oracle):
    """Plaintexts of every length mod 64 (and the last 128 lengths up to one page) at ce width:
    APP || msgpack(Vec<Op>) || trailing bytes, which from_slice ignores."""
    rng = random.Random(7)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(6))
    lens = list(range(17, 17 + 192)) + list(range(4096 - 127, 4097))
    rng.shuffle(lens)
    per = -(-len(lens) // len(actors))
    files, fa, vers = [], [], []
    for i, L in enumerate(lens):
        a = i // per
        k = max(0, min((L - 16 - 3) // 51, 79))
        ops = [op(actors[a] if rng.random() < 0.8 else rng.choice(actors), counter_of(rng, "ce"), rng.choice(pm.DIRS))
               for _ in range(k)]
        body = pm.enc_ops(ops)
        assert 16 + len(body) <= L
        clear = APP + body + rng.randbytes(L - 16 - len(body))
        assert len(clear) == L
        files.append(seal(oracle, key, clear, rng))
        fa.append(a)
        vers.append(i % per)
    core, model = new_core(ctx, key), pm.Core()
    ingest_and_check(core, model, key, files, actors, fa, vers)
    core.close()


# ------------------------------------------------------------------ carry across files
def test_carry_four_files_per_wave(ctx, oracle):
    """A wave's four files of one writer, then a writer change inside the wave's four; the last
    file of the batch holds the maxima of both planes."""
    rng = random.Random(8)
    key = rng.randbytes(32)
    w = sorted(rng.randbytes(16) for _ in range(3))
    plan = [0] * 8 + [1] * 2 + [2] * 2 + [1] * 0 + [2] * 5  # groups of four: 0000 0000 1122 2222 2
    files, fa, vers, nxt = [], [], [], [0, 0, 0]
    for i, a in enumerate(plan):
        last = i == len(plan) - 1
        ops = [op(w[a], (1 << 31) + 5 if last else rng.randrange(1 << 16, 1 << 30), d)
               for d in ("Pos", "Neg") for _ in range(20)]
        rng.shuffle(ops)
        files.append(seal(oracle, key, APP + pm.enc_ops(ops), rng))
        fa.append(a)
        vers.append(nxt[a])
        nxt[a] += 1
    core, model = new_core(ctx, key), pm.Core()
    ingest_and_check(core, model, key, files, w, fa, vers)
    assert model.state.p.dots[w[2]] == model.state.n.dots[w[2]] == (1 << 31) + 5
    core.close()


def test_carry_across_a_waves_run(ctx, oracle):
    """The pending (index, max) is carried from file to file only where a wave takes more than
    one group of four files, i.e. with more groups than resident waves (about 2,000 on the
    MI355X): 16,384 one-op files, the only case here of more than a few hundred.  Writer runs of
    1,024 files, so writers change inside runs; each writer's maxima sit in its run's last files
    and alternate planes."""
    rng = random.Random(9)
    key = rng.randbytes(32)
    w = sorted(rng.randbytes(16) for _ in range(16))
    n_per = 1024
    files, fa, vers = [], [], []
    for a in range(16):
        for v in range(n_per):
            c = (1 << 20) + v if v >= n_per - 2 else rng.randrange(1 << 16, 1 << 20)
            files.append(seal(oracle, key, APP + pm.enc_ops([op(w[a], c, pm.DIRS[v & 1])]), rng))
            fa.append(a)
            vers.append(v)
    core, model = new_core(ctx, key), pm.Core()
    rc, _ = core.ingest_ops(files, w, fa, vers, want_status=False)
    assert rc == 0
    assert model.read_remote_ops(key, [APP], files, [w[i] for i in fa], vers)[0] == 0
    assert core.state_bytes() == model.serialize()
    assert model.state.p.dots[w[5]] == (1 << 20) + n_per - 2 and model.state.n.dots[w[5]] == (1 << 20) + n_per - 1
    core.close()


# ------------------------------------------------------------------ grammar
def _pack(x):
    return msgpack.packb(x, use_bin_type=True)


def _canon(a, c, d):
    return pm.enc_ops([op(a, c, d)])[1:]


def test_grammar_accepted_forms(ctx, oracle):
    """A width change in mid-file, and every non-canonical form the reader accepts, among
    canonical ops (so the fast path hands over and takes back)."""
    rng = random.Random(10)
    key = rng.randbytes(32)
    a, b = sorted(rng.randbytes(16) for _ in range(2))
    dot = {"actor": b, "counter": 40000}
    forms = {
        "dir_first": _pack({"dir": "Neg", "dot": dot}),
        "array_op": _pack([dot, "Neg"]),
        "array_dot": _pack({"dot": [b, 40001], "dir": "Pos"}),
        "extra_key": _pack({"dot": dot, "zzz": [1, {"x": b"yy"}], "dir": "Neg"}),
        "index_keys": _pack({1: "Pos", 0: {1: 40002, 0: b}}),
        "map_dir": _pack({"dot": dot, "dir": {"Neg": None}}),
        "map_dir_index": _pack({"dot": dot, "dir": {0: None}}),
    }
    bodies = []
    # width changes in mid-file: ce ops, then cc, then cf, then fixint, then cd
    mixed = b"".join(_canon(a, counter_of(rng, wd), rng.choice(pm.DIRS))
                     for wd in ["ce"] * 20 + ["cc"] * 3 + ["cf"] * 18 + ["fixint"] * 2 + ["cd"] * 17)
    bodies.append(b"\xdc\x00\x3c" + mixed)
    for name, blob in forms.items():
        pre = [_canon(a, counter_of(rng, "ce"), rng.choice(pm.DIRS)) for _ in range(rng.choice([0, 1, 17, 33]))]
        post = [_canon(a, counter_of(rng, "ce"), rng.choice(pm.DIRS)) for _ in range(rng.choice([0, 2, 31]))]
        n = len(pre) + 1 + len(post)
        bodies.append((bytes([0x90 | n]) if n < 16 else b"\xdc" + n.to_bytes(2, "big")) + b"".join(pre) + blob +
                      b"".join(post))
    bodies.append(b"\x97" + b"".join(forms.values()))  # nothing canonical at all
    files = [seal(oracle, key, APP + x, rng) for x in bodies]
    core, model = new_core(ctx, key), pm.Core()
    ingest_and_check(core, model, key, files, [a], [0] * len(files), list(range(len(files))))
    assert model.state.n.dots[b] == 40000 and model.state.p.dots[b] == 40002
    core.close()


@pytest.mark.parametrize("form", ["dir_zero", "dir_bin", "dup_dot", "truncated", "count_too_large"])
def test_grammar_rejected_forms(ctx, oracle, form):
    """Each is CE_ERR_DECODE for its file, nothing of the batch is folded, the state stays."""
    rng = random.Random(11)
    key = rng.randbytes(32)
    a = rng.randbytes(16)
    dot = {"actor": a, "counter": 9}
    good = [_canon(a, counter_of(rng, "ce"), rng.choice(pm.DIRS)) for _ in range(20)]
    bad = {
        "dir_zero": b"\xdc\x00\x15" + b"".join(good) + _pack({"dot": dot, "dir": "Zero"}),
        "dir_bin": b"\xdc\x00\x15" + b"".join(good) + _pack({"dot": dot, "dir": b"Pos"}),
        "dup_dot": b"\xdc\x00\x15" + b"".join(good) + b"\x83\xa3dot" + _pack(dot) + b"\xa3dot" + _pack(dot) +
                   b"\xa3dir\xa3Pos",
        "truncated": b"\xdc\x00\x14" + b"".join(good)[:-3],
        "count_too_large": b"\xdc\x00\x16" + b"".join(good),
    }[form]
    core, model = new_core(ctx, key), pm.Core()
    first = [seal(oracle, key, APP + pm.enc_ops([op(a, 77, "Pos"), op(a, 78, "Neg")]), rng)]
    ingest_and_check(core, model, key, first, [a], [0], [0])
    before = core.state_bytes()
    files = [seal(oracle, key, APP + x, rng) for x in (b"\xdc\x00\x14" + b"".join(good), bad, b"\x91" + good[0])]
    ingest_and_check(core, model, key, files, [a], [0, 0, 0], [1, 2, 3], want_rc=12)
    assert core.state_bytes() == before
    core.close()


# ------------------------------------------------------------------ batch statuses
def _small_batch(oracle, rng, key, actors, n_vers, app=APP):
    files, fa, vers = [], [], []
    for a in range(len(actors)):
        for v in range(n_vers):
            ops = [op(actors[a] if rng.random() < 0.8 else rng.choice(actors),
                      counter_of(rng, rng.choice(list(WIDTH_BITS))), rng.choice(pm.DIRS)) for _ in range(rng.randrange(1, 40))]
            files.append(seal(oracle, key, app + pm.enc_ops(ops), rng))
            fa.append(a)
            vers.append(v)
    return files, fa, vers


def test_tampered_tag_rejects_the_batch(ctx, oracle):
    rng = random.Random(12)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(4))
    files, fa, vers = _small_batch(oracle, rng, key, actors, 5)
    core, model = new_core(ctx, key), pm.Core()
    empty = core.state_bytes()
    b = bytearray(files[7])
    b[-1] ^= 0x40
    files[7] = bytes(b)
    ingest_and_check(core, model, key, files, actors, fa, vers, want_rc=9)
    assert core.state_bytes() == empty
    core.close()


def test_version_gap_keeps_the_files_before_it(ctx, oracle):
    rng = random.Random(13)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(4))
    files, fa, vers = _small_batch(oracle, rng, key, actors, 5)
    keep = [i for i in range(len(files)) if not (fa[i] == 1 and vers[i] == 2)]
    files, fa, vers = [files[i] for i in keep], [fa[i] for i in keep], [vers[i] for i in keep]
    core, model = new_core(ctx, key), pm.Core()
    ingest_and_check(core, model, key, files, actors, fa, vers, want_rc=13)
    assert model.nov.dots == {actors[0]: 5, actors[1]: 2}
    core.close()


def test_unsupported_data_version(ctx, oracle):
    rng = random.Random(14)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(2))
    files, fa, vers = _small_batch(oracle, rng, key, actors, 3)
    files[4] = seal(oracle, key, bytes(16) + pm.enc_ops([op(actors[1], 1, "Pos")]), rng)
    core, model = new_core(ctx, key), pm.Core()
    empty = core.state_bytes()
    ingest_and_check(core, model, key, files, actors, fa, vers, want_rc=11)
    assert core.state_bytes() == empty
    core.close()


# ------------------------------------------------------------------ table growth
def test_table_growth_moves_both_planes(ctx, oracle):
    """A batch, then one whose Dots name 5,000 actors not yet seen, split between Pos and Neg:
    the rehash (8,192 -> 32,768 slots) carries both planes of the first batch along."""
    rng = random.Random(15)
    key = rng.randbytes(32)
    writers = sorted(rng.randbytes(16) for _ in range(4))
    core, model = new_core(ctx, key), pm.Core()
    files, fa, vers = _small_batch(oracle, rng, key, writers, 4)
    ingest_and_check(core, model, key, files, writers, fa, vers)
    cap0 = core.dense_capacity()
    new = [rng.randbytes(16) for _ in range(5000)]
    files, fa, vers = [], [], []
    for i in range(0, 5000, 70):
        ops = [op(x, counter_of(rng, "ce"), pm.DIRS[j & 1]) for j, x in enumerate(new[i:i + 70])]
        files.append(seal(oracle, key, APP + pm.enc_ops(ops), rng))
        fa.append((i // 70) % 4)
        vers.append(4 + (i // 70) // 4)
    order = sorted(range(len(files)), key=lambda i: (fa[i], vers[i]))
    files, fa, vers = [files[i] for i in order], [fa[i] for i in order], [vers[i] for i in order]
    ingest_and_check(core, model, key, files, writers, fa, vers)
    assert core.dense_capacity() > cap0
    assert len(model.state.p.dots) > 2000 and len(model.state.n.dots) > 2000
    core.close()


# ------------------------------------------------------------------ multi-page files
def test_multi_page_files(ctx, oracle):
    """Op files of about 6, 20 and 70 KiB among small ones: opened to HBM and decoded whole."""
    rng = random.Random(16)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(3))
    files, fa, vers = _small_batch(oracle, rng, key, actors, 4)
    for a, n_ops in ((0, 120), (1, 400), (2, 1400)):
        ops = [op(actors[a] if rng.random() < 0.7 else rng.choice(actors), counter_of(rng, rng.choice(["ce", "cf", "cd"])),
                  rng.choice(pm.DIRS)) for _ in range(n_ops)]
        ops.append(op(actors[a], (1 << 64) - 1 - a, "Neg"))  # the file's last op is the plane's maximum
        clear = APP + pm.enc_ops(ops)
        assert len(clear) > 4096
        files.append(seal(oracle, key, clear, rng))
        fa.append(a)
        vers.append(4)
    order = sorted(range(len(files)), key=lambda i: (fa[i], vers[i]))
    files, fa, vers = [files[i] for i in order], [fa[i] for i in order], [vers[i] for i in order]
    sizes = sorted(len(f) for f in files)[-3:]
    assert 5000 < sizes[0] < 8000 and 18000 < sizes[1] < 24000 and 65000 < sizes[2] < 80000
    core, model = new_core(ctx, key), pm.Core()
    ingest_and_check(core, model, key, files, actors, fa, vers)
    assert model.state.n.dots[actors[2]] == (1 << 64) - 3
    core.close()


# ------------------------------------------------------------------ states
def _random_state(rng, actors):
    nov, st = VClock(), pm.PNCounter()
    for a in rng.sample(actors, 4):
        nov.apply(a, rng.randrange(1, 50))
    for a in rng.sample(actors, 4):
        st.p.apply(a, counter_of(rng, rng.choice(list(WIDTH_BITS))))
    for a in rng.sample(actors, 4):
        st.n.apply(a, counter_of(rng, rng.choice(list(WIDTH_BITS))))
    return nov, st


@pytest.mark.parametrize("route", ["ingest_states", "ingest_states_device", "merge_state", "merge_state_device"])
def test_states_then_ops(ctx, oracle, route):
    """Three states with overlapping p / n actors, then ops."""
    torch = pytest.importorskip("torch")
    rng = random.Random(17)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(6))
    sws = [pm.serialize(*_random_state(rng, actors)) for _ in range(3)]
    sfiles = [seal(oracle, key, APP + sw, rng) for sw in sws]
    core, model = new_core(ctx, key), pm.Core()
    if route == "ingest_states":
        rc, st = core.ingest_states(sfiles)
        assert rc == 0 and st == [0, 0, 0]
    elif route == "ingest_states_device":
        blob = b"".join(sfiles)
        offs = np.zeros(4, dtype=np.int64)
        offs[1:] = np.cumsum([len(f) for f in sfiles])
        d_blob = torch.tensor(list(blob) + [0] * 64, dtype=torch.uint8, device="cuda")
        d_offs = torch.tensor(offs, device="cuda")
        torch.cuda.synchronize()
        rc, st = core.ingest_states_device(d_blob.data_ptr(), d_offs.data_ptr(), 3, len(blob), want_status=True)
        assert rc == 0 and st == [0, 0, 0]
    elif route == "merge_state":
        for sw in sws:
            assert core.merge_state(sw) == 0
    else:
        for sw in sws:
            d = torch.tensor(list(sw), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            assert core.merge_state_device(d.data_ptr(), len(sw)) == 0
    assert model.read_remote_states(key, [APP], sfiles)[0] == 0
    assert core.state_bytes() == model.serialize()
    # ops on top: versions below a state's next_op_versions are skipped by both
    files, fa, vers = _small_batch(oracle, rng, key, actors[:3], 3)
    start = [model.nov.get(a) for a in actors[:3]]
    vers = [start[fa[i]] + vers[i] for i in range(len(files))]
    ingest_and_check(core, model, key, files, actors[:3], fa, vers)
    # a state that is not the p / n form
    assert core.merge_state(_pack({"next_op_versions": {"dots": {}}, "state": {"inner": {"dots": {}}}})) == 12
    core.close()


# ------------------------------------------------------------------ serializer
def _state_with(rng, n_p, n_n, n_nov):
    """actors: some p-only, some n-only, some shared (as far as the counts allow)"""
    total = max(n_p, n_n, n_nov) + min(n_p, n_n) // 2 + 1
    actors = [rng.randbytes(16) for _ in range(total)]
    nov, st = VClock(), pm.PNCounter()
    for a in actors[:n_p]:
        st.p.apply(a, counter_of(rng, rng.choice(list(WIDTH_BITS))) or 1)
    for a in actors[total - n_n:] if n_n else []:
        st.n.apply(a, counter_of(rng, rng.choice(list(WIDTH_BITS))) or 1)
    for a in rng.sample(actors, n_nov):
        nov.apply(a, rng.randrange(1, 1 << 20))
    assert (len(st.p.dots), len(st.n.dots), len(nov.dots)) == (n_p, n_n, n_nov)
    return nov, st


@pytest.mark.parametrize("counts", [(0, 0, 0), (1, 0, 15), (0, 1, 0), (15, 16, 17), (16, 17, 1), (17, 15, 16),
                                    (300, 16, 0), (5000, 300, 17), (17, 5000, 300), (1, 15, 5000)])
@pytest.mark.parametrize("flags", [0, crdtenc.COMPACT_INGEST_FORMAT])
def test_device_serializer(ctx, oracle, counts, flags, monkeypatch):
    """The three maps (next_op_versions, p, n) cross fixmap / map16 independently; the device
    writer, the host writer (CE_HOST_COMPACT=1) and the model give the same bytes; an
    ingest-format compaction read by a fresh core gives the same state."""
    rng = random.Random(sum(counts) + flags)
    key = rng.randbytes(32)
    nov, st = _state_with(rng, *counts)
    want = pm.serialize(nov, st)
    nonce = bytes(range(24))

    def compacted(core):
        assert core.merge_state(want) == 0
        assert core.state_bytes() == want
        f, name = core.compact_to_buffer(nonce=nonce)
        assert name == crdtenc.content_name(f) == oracle.base32_nopad(oracle.sha3_256(f))
        return f
    core = new_core(ctx, key, flags=flags)
    f = compacted(core)
    s, pt = oracle.cryptor_decrypt(key, f[16:])
    assert s == 0
    if flags:
        assert f[:16] == CORE and pt == APP + want
    else:
        assert f[:16] == APP and pt == want
    monkeypatch.setenv("CE_HOST_COMPACT", "1")
    host = new_core(ctx, key, flags=flags)
    monkeypatch.delenv("CE_HOST_COMPACT")
    assert compacted(host) == f
    if flags:
        fresh = new_core(ctx, key)
        rc, sts = fresh.ingest_states([f])
        assert rc == 0 and sts == [0] and fresh.state_bytes() == want
        fresh.close()
    core.close()
    host.close()


# ------------------------------------------------------------------ compact_ops_device
def _to_device(files, fa, vers):
    torch = pytest.importorskip("torch")
    blob = b"".join(files)
    offs = np.zeros(len(files) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(f) for f in files])
    d = (torch.tensor(list(blob) + [0] * 64, dtype=torch.uint8, device="cuda"),
         torch.tensor(offs, device="cuda"),
         torch.tensor(np.array(fa, dtype=np.int32), device="cuda"),
         torch.tensor(np.array(vers, dtype=np.int64), device="cuda"))
    torch.cuda.synchronize()
    return d, len(blob)


@pytest.mark.parametrize("case", ["clean", "foreign_actors", "tampered", "gap"])
def test_compact_ops_device(ctx, oracle, case):
    """ce_core_compact_ops_device == ingest_ops_device + compact_to_buffer with the same nonce, on
    the fast path (the compaction queued behind the device commit of both planes) and off it:
    actors outside the table (both planes folded again), a failing tag, a version gap."""
    rng = random.Random(18)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(6))
    files, fa, vers = [], [], []
    for a in range(6):
        for v in range(5):
            if case == "foreign_actors":
                who = [rng.randbytes(16) for _ in range(7)]
            else:
                who = [actors[a]] * 20
            ops = [op(x, counter_of(rng, "ce"), rng.choice(pm.DIRS)) for x in who]
            files.append(seal(oracle, key, APP + pm.enc_ops(ops), rng))
            fa.append(a)
            vers.append(v)
    if case == "tampered":
        b = bytearray(files[9])
        b[-3] ^= 1
        files[9] = bytes(b)
    if case == "gap":
        keep = [i for i in range(len(files)) if not (fa[i] == 0 and vers[i] == 2)]
        files, fa, vers = [files[i] for i in keep], [fa[i] for i in keep], [vers[i] for i in keep]
    (d_blob, d_offs, d_fa, d_fv), blen = _to_device(files, fa, vers)
    nonce = bytes(range(24))
    args = (d_blob.data_ptr(), d_offs.data_ptr(), len(files), blen, b"".join(actors), d_fa.data_ptr(), d_fv.data_ptr())
    model = pm.Core()
    orc, _ = model.read_remote_ops(key, [APP], files, [actors[i] for i in fa], vers)
    core = new_core(ctx, key)
    before = core.state_bytes()
    rc, f, name = core.compact_ops_device(*args, nonce=nonce)
    assert rc == orc, (rc, orc, ctx.last_error())
    if case == "tampered":
        assert rc == 9 and f is None and core.state_bytes() == before
    elif case == "gap":
        assert rc == 13 and f is None and core.state_bytes() == model.serialize()
    else:
        assert rc == 0 and core.state_bytes() == model.serialize()
        s, pt = oracle.cryptor_decrypt(key, f[16:])
        assert s == 0 and f[:16] == APP and pt == model.serialize()
        assert name == crdtenc.content_name(f)
        ref = new_core(ctx, key)
        assert ref.ingest_ops_device(*args) == 0
        assert ref.compact_to_buffer(nonce=nonce) == (f, name)
        rc2, f2, _ = core.compact_ops_device(*args, nonce=nonce)  # every file below next_op_versions now
        assert rc2 == 0 and f2 == f
        buf = np.zeros(1 << 16, np.uint8)
        c3 = new_core(ctx, key)
        rc3, ln, nm3 = c3.compact_ops_device_into(buf, *args, nonce=nonce, name=True)
        assert rc3 == 0 and bytes(buf[:ln]) == f and nm3 == name
        c3.close()
        ref.close()
    core.close()


# ------------------------------------------------------------------ storage
def test_storage_two_replicas(ctx, tmp_path, oracle):
    """apply_ops, apply_ops_batch, read_remote, compact, read_remote again: both replicas end
    with the model's bytes."""
    rng = random.Random(19)
    key = rng.randbytes(32)
    remote = str(tmp_path / "remote")
    c1 = new_core(ctx, key, local_path=str(tmp_path / "l1"), remote_path=remote, flags=crdtenc.OPEN_CREATE)
    c2 = new_core(ctx, key, local_path=str(tmp_path / "l2"), remote_path=remote,
                  flags=crdtenc.OPEN_CREATE | crdtenc.COMPACT_INGEST_FORMAT)
    a1, a2 = c1.info_actor(), c2.info_actor()
    model = pm.Core()

    def local(actor, ops):
        for o in ops:
            model.state.apply(o)
        model.nov.apply(actor, model.nov.get(actor) + 1)
        return pm.enc_ops(ops)
    assert c1.apply_ops(b"\x91\x82\xa3dot\x82\xa5actor\xc4\x10" + a1 + b"\xa7counter\x01\xa3dir\xa3Zzz") == 12
    for i in range(4):
        assert c1.apply_ops(local(a1, [op(a1, 10 * i + 1, "Pos"), op(a1, i + 1, "Neg")])) == 0
    rc, written = c2.apply_ops_batch([local(a2, [op(a2, 1000 + i, pm.DIRS[i & 1]), op(a1, 3, "Neg")]) for i in range(3)])
    assert rc == 0 and len(written) == 3
    assert c2.apply_ops_batch([pm.enc_ops([op(a2, 5, "Pos")]), b"\x91\xc0"])[0] == 12  # nothing sealed or applied
    assert c1.read_remote() == 0 and c2.read_remote() == 0
    assert c1.state_bytes() == c2.state_bytes() == model.serialize()
    rc, name = c2.compact()
    assert rc == 0 and crdtenc.Storage(str(tmp_path / "l2"), remote).list_state_names() == [name]
    assert c1.apply_ops(local(a1, [op(a1, 999, "Neg")])) == 0
    assert c1.read_remote() == 0 and c2.read_remote() == 0
    assert c1.state_bytes() == c2.state_bytes() == model.serialize()
    c3 = new_core(ctx, key, local_path=str(tmp_path / "l3"), remote_path=remote, flags=crdtenc.OPEN_CREATE)
    assert c3.read_remote() == 0 and c3.state_bytes() == model.serialize()
    for c in (c1, c2, c3):
        c.close()


# ------------------------------------------------------------------ multi-GPU answers
def test_multi_gpu_answers_are_definite(ctx, oracle):
    """No dense exchange for this kind: dense_ready 0 and CE_ERR_INVALID_ARG from the five dense /
    sharded entry points, with nothing touched; two cores converge through state_bytes_device /
    merge_state_device."""
    torch = pytest.importorskip("torch")
    import ctypes
    rng = random.Random(20)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(4))
    cores, models = [new_core(ctx, key) for _ in range(2)], [pm.Core() for _ in range(2)]
    for r in range(2):
        cores[r].register_actors(actors)
        files, fa, vers = _small_batch(oracle, rng, key, actors[2 * r:2 * r + 2], 3)
        ingest_and_check(cores[r], models[r], key, files, actors[2 * r:2 * r + 2], fa, vers)
    c, L = cores[0], crdtenc.lib()
    before = c.state_bytes()
    cap = c.dense_capacity()
    buf = torch.full((2 * cap,), 7, dtype=torch.int64, device="cuda")
    nov = torch.full((cap,), 7, dtype=torch.int64, device="cuda")
    ready = ctypes.c_int(5)
    vp = ctypes.c_void_p
    assert c.dense_ready() is False and L.ce_core_dense_ready(c.p) == 0
    assert L.ce_core_export_dense(c.p, vp(buf.data_ptr()), vp(nov.data_ptr())) == 64
    assert L.ce_core_import_dense(c.p, vp(buf.data_ptr()), vp(nov.data_ptr())) == 64
    (d_blob, d_offs, d_fa, d_fv), blen = _to_device([b"x" * 40], [0], [0])
    assert c.ingest_ops_device_sharded(d_blob.data_ptr(), d_offs.data_ptr(), 1, blen, b"".join(actors),
                                       d_fa.data_ptr(), d_fv.data_ptr(), nov.data_ptr()) == 64
    assert L.ce_core_pending_export(c.p, vp(buf.data_ptr()), ctypes.c_uint64(2 * cap), ctypes.byref(ready)) == 64
    assert L.ce_core_pending_commit(c.p, 1, None, ctypes.c_uint64(0)) == 64
    rc, n = c.export_columns_device(buf.data_ptr(), 16 * cap)
    assert rc == 64 and n == 0
    torch.cuda.synchronize()
    assert ready.value == 5 and bool((buf == 7).all()) and bool((nov == 7).all())
    assert c.state_bytes() == before
    # the exchange this kind has: each rank's state bytes, merged by the other
    dev = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    for src, dst in ((0, 1), (1, 0)):
        rc, n = cores[src].state_bytes_device(dev.data_ptr(), dev.numel())
        assert rc == 0 and bytes(dev[:n].cpu().numpy()) == models[src].serialize()
        assert cores[dst].merge_state_device(dev.data_ptr(), n) == 0
        models[dst].merge_state(models[src].serialize())
    assert cores[0].state_bytes() == cores[1].state_bytes() == models[0].serialize() == models[1].serialize()
    for x in cores:
        x.close()
