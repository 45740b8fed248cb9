"""GPU parity of ce_core_gset_apply_members[_device] (include/crdtenc.h) against
tests/gset_write_model.py: with fixed nonces the written files, their offsets and their count are
compared byte for byte, state_bytes() with gset_model.Core after apply_ops of each chunk (which
also proves the version bump), and a fresh core that ingests the written files reaches the same
state with every file decoded inside the fused open.  Without the three entry points every test
here fails on the missing symbols."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import crdtenc
import gset_model as gm
import gset_write_model as wm

pytestmark = pytest.mark.gpu
APP = wm.APP
GS = crdtenc.STATE_GSET
DEV = "cuda:0"
U64 = (1 << 64) - 1
INVALID, NO_KEY = 64, 66
NEW_ONLY = crdtenc.GSET_APPLY_NEW_ONLY
GUARD = 64          # bytes / words past every output's bound that must stay as they were
FILL = 0xAB


@pytest.fixture(scope="module")
def ctx():
    c = crdtenc.Context(0)
    yield c
    c.close()


def new_core(ctx, key, kind=GS, **kw):
    c = crdtenc.Core(ctx, kind=kind, supported=[APP], current_data_version=APP, **kw)
    if key is not None:
        c.set_latest_key(key)
    return c


def u64_dev(values):
    t = torch.from_numpy(np.asarray(values, np.uint64).view(np.int64).copy()).to(DEV)
    torch.cuda.synchronize()
    return t


class Written:
    """a core, its model, and every file it wrote so far (the local actor's versions 0, 1, ...)"""

    def __init__(self, ctx, oracle, key, rng, **kw):
        self.ctx, self.oracle, self.key, self.rng = ctx, oracle, key, rng
        self.core, self.model = new_core(ctx, key, **kw), gm.Core()
        self.actor = self.core.info_actor()
        self.files = []

    def apply(self, col, per_file, flags=0, host=False):
        """one call over col, checked against the model; returns the files it wrote"""
        core, model = self.core, self.model
        ops = wm.new_only(col, model.state.value) if flags & NEW_ONLY else list(col)
        chunks = wm.cut(ops, per_file)
        rc, max_files, max_bytes = crdtenc.gset_apply_bound(len(col), per_file)
        assert rc == 0 and (max_files, max_bytes) == wm.bound(len(col), per_file)
        nonces = [self.rng.randbytes(24) for _ in range(max_files)]
        want = wm.files(self.oracle, self.key, nonces, chunks)
        offs = wm.offsets(want)
        assert len(want) <= max_files and offs[-1] <= max_bytes
        filtered = core.path_count("gset_apply_filtered")
        if host:
            rc, got = core.gset_apply_members(col, per_file, flags, nonces)
            assert rc == 0, core.ctx.last_error()
            assert got == want
        else:
            members = u64_dev(col)
            d_files = torch.full((max_bytes + GUARD,), FILL, dtype=torch.uint8, device=DEV)
            d_offs = torch.full((max_files + 1 + GUARD,), -1, dtype=torch.int64, device=DEV)
            torch.cuda.synchronize()
            rc, nf, nb = core.gset_apply_members_device(members.data_ptr() if len(col) else None, len(col),
                                                        d_files.data_ptr(), max_bytes, d_offs.data_ptr(), per_file,
                                                        flags, nonces)
            assert rc == 0, core.ctx.last_error()
            assert (nf, nb) == (len(want), offs[-1])
            out, o = d_files.cpu().numpy(), d_offs.cpu().numpy()
            assert [int(x) for x in o[:nf + 1]] == offs
            assert bool((o[nf + 1:] == -1).all())               # no word past the F + 1 offsets
            assert out[:nb].tobytes() == b"".join(want)
            assert bool((out[nb:] == FILL).all())               # no byte past the files
            assert [int(x) for x in members.cpu().numpy().view(np.uint64)] == list(col)   # the column is read only
        for ch in chunks:
            model.apply_ops(self.actor, ch)
        assert core.state_bytes() == model.serialize()
        if flags & NEW_ONLY:
            assert core.path_count("gset_apply_filtered") - filtered == len(col) - len(ops)
        self.files += want
        return want

    def check_readers(self):
        """a fresh core that ingests every written file: the same state, all decoded in the fused open"""
        reader = new_core(self.ctx, self.key)
        n = len(self.files)
        rc, st = reader.ingest_ops(self.files, [self.actor], [0] * n, list(range(n)))
        assert rc == 0 and st == [0] * n, reader.ctx.last_error()
        assert reader.state_bytes() == self.model.serialize() == self.core.state_bytes()
        assert reader.path_count("gset_fused_files") == n
        assert self.core.path_count("gset_apply_device_files") == n
        reader.close()

    def close(self):
        self.core.close()


def columns(rng, n):
    """n members of each width, and of all five alternating"""
    cols = [[wm.member_of_width(rng, w) for _ in range(n)] for w in wm.WIDTH_BYTES]
    cols.append([wm.member_of_width(rng, wm.WIDTH_BYTES[i % 5]) for i in range(n)])
    return cols


def members_with_sum(rng, cnt, total):
    """cnt members whose encoded widths sum to total (cnt <= total <= 9 cnt), shuffled"""
    assert cnt <= total <= 9 * cnt
    ws = [1] * cnt
    left = total - cnt
    i = 0
    while left:
        step = max(s for s in (8, 4, 2, 1) if s <= left)    # 1 -> 9, 5, 3, 2
        ws[i] += step
        left -= step
        i += 1
    assert sum(ws) == total and set(ws) <= set(wm.WIDTH_BYTES)
    rng.shuffle(ws)
    return [wm.member_of_width(rng, w) for w in ws]


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize("per_file", [1, 15, 16, 17, 453])
def test_counts_and_widths(ctx, oracle, per_file):
    """n around the file size (0, 1, a short last file, whole files), each width uniform and all
    five alternating: the fixarray / array16 headers at 15 / 16 members, the 16-lane rounds."""
    rng = random.Random(per_file)
    w = Written(ctx, oracle, rng.randbytes(32), rng)
    ns = sorted({0, 1, per_file - 1, per_file, per_file + 1, 2 * per_file, 2 * per_file + 1})
    for n in ns:
        for col in columns(rng, n):
            got = w.apply(col, per_file)
            assert len(got) == -(-n // per_file)
    assert w.core.path_count("gset_apply_device_members") == 6 * sum(ns)
    w.check_readers()
    w.close()


def test_per_file_zero_means_a_page(ctx, oracle):
    rng = random.Random(3)
    w = Written(ctx, oracle, rng.randbytes(32), rng)
    got = w.apply([wm.member_of_width(rng, 9) for _ in range(454)], 0)
    assert len(got) == 2 and len(got[0]) == 16 + wm.sealed_len(wm.PAGE)
    w.check_readers()
    w.close()


def test_width_edges(ctx, oracle):
    """the smallest and largest member of every width, 0 and 2^64 - 1 among them, in one file, one
    a file, and split unevenly"""
    rng = random.Random(4)
    w = Written(ctx, oracle, rng.randbytes(32), rng)
    for per_file in (453, 1, 5):
        w.apply(wm.WIDTH_EDGES, per_file)
    assert set(wm.WIDTH_EDGES) == w.model.state.value
    w.check_readers()
    w.close()


def test_clear_lengths_sweep(ctx, oracle):
    """files of 64 consecutive clear lengths (every offset of a file's end, and of the next file's
    start, inside a 16-byte chunk and a 64-byte ChaCha20 block), in ascending and shuffled order"""
    rng = random.Random(5)
    w = Written(ctx, oracle, rng.randbytes(32), rng)
    per_file = 20
    lens = list(range(100, 164))
    for order in (lens, rng.sample(lens, len(lens))):
        col = []
        for L in order:
            col += members_with_sum(rng, per_file, L - 16 - 3)
        got = w.apply(col, per_file)
        assert [len(f) for f in got] == [16 + wm.sealed_len(L) for L in order]
    w.check_readers()
    w.close()


def test_envelope_header_forms(ctx, oracle):
    """clear lengths on both sides of every length at which the envelope's header changes form
    within one page (a bin8 header becoming bin16)"""
    rng = random.Random(6)
    steps = [L for L in range(17, wm.PAGE) if wm.sealed_len(L + 1) - wm.sealed_len(L) != 1]
    assert len(steps) == 2          # the EncBox's length and the ciphertext's length pass 255
    per_file = 30
    lens = sorted({L + d for L in steps for d in (-1, 0, 1, 2)})
    assert 16 + 3 + per_file <= lens[0] and lens[-1] <= 16 + 3 + 9 * per_file
    w = Written(ctx, oracle, rng.randbytes(32), rng)
    col = []
    for L in lens:
        col += members_with_sum(rng, per_file, L - 16 - 3)
    got = w.apply(col, per_file)
    assert [len(f) - 16 - L for f, L in zip(got, lens)] == [wm.sealed_len(L) - L for L in lens]
    assert len({len(f) - 16 - L for f, L in zip(got, lens)}) == 3
    w.check_readers()
    w.close()


def test_more_files_than_one_launch_holds_at_once(ctx, oracle, monkeypatch):
    """4,100 files of 17 members (many blocks' worth of groups), and 150 files with the grids
    clamped to two blocks, so that every block of the encoder takes many trips"""
    rng = random.Random(7)
    w = Written(ctx, oracle, rng.randbytes(32), rng)
    col = [wm.member_of_width(rng, wm.WIDTH_BYTES[(i * 7 + i // 17) % 5]) for i in range(4100 * 17)]
    assert len(w.apply(col, 17)) == 4100
    monkeypatch.setenv("CE_TEST_GRID_CAP", "2")
    assert len(w.apply(col[:150 * 17 - 5], 17)) == 150
    monkeypatch.delenv("CE_TEST_GRID_CAP")
    monkeypatch.setenv("CE_GSET_CAP", str(1 << 18))     # the reader's batch table holds the ~72,000 members
    w.check_readers()
    w.close()


def test_table_grows_inside_the_insert(ctx, oracle, monkeypatch):
    rng = random.Random(8)
    monkeypatch.setenv("CE_GSET_CAP", "64")
    w = Written(ctx, oracle, rng.randbytes(32), rng)
    monkeypatch.delenv("CE_GSET_CAP")
    w.apply([wm.member_of_width(rng, 9) for _ in range(600)], 100)
    assert w.core.path_count("gset_grows") > 0
    w.apply(wm.WIDTH_EDGES, 5)
    w.check_readers()
    w.close()


# ------------------------------------------------------------------ CE_GSET_APPLY_NEW_ONLY
def test_new_only(ctx, oracle):
    """duplicates inside the column, members held from an earlier ingest, 0 and 2^64 - 1 new and
    held, and a column the set holds whole: no file, nothing bumped"""
    rng = random.Random(9)
    key = rng.randbytes(32)
    w = Written(ctx, oracle, key, rng)
    other = rng.randbytes(16)
    held = [wm.member_of_width(rng, wm.WIDTH_BYTES[i % 5]) for i in range(300)]
    st, enc = oracle.cryptor_encrypt(key, rng.randbytes(24), APP + gm.enc_ops(held))
    assert st == 0
    rc, sts = w.core.ingest_ops([wm.CORE_VERSION + enc], [other], [0], [0])
    assert rc == 0 and sts == [0]
    w.model.state.value |= set(held)
    w.model.nov.apply(other, 1)
    assert w.core.state_bytes() == w.model.serialize()
    fresh = [wm.member_of_width(rng, wm.WIDTH_BYTES[i % 5]) for i in range(200)]
    col = held[:150] + fresh + fresh[:50] + [0, U64, 0, U64] + held[100:200]       # the sentinels new
    rng.shuffle(col)
    got = w.apply(col, 16, NEW_ONLY)
    assert len(got) == -(-len(set(fresh + [0, U64]) - set(held)) // 16)
    assert {0, U64} <= w.model.state.value
    before, files = w.core.state_bytes(), w.core.path_count("gset_apply_device_files")
    col = [0, U64] * 3 + held[:40] + fresh[:40]                                     # the sentinels held
    assert w.apply(col, 7, NEW_ONLY) == []
    assert w.apply(col, 7, NEW_ONLY, host=True) == []
    assert w.core.state_bytes() == before and w.core.path_count("gset_apply_device_files") == files
    assert w.apply([U64, 5, U64, 1 << 40, 5] + fresh[:3], 2, NEW_ONLY) != []       # the next version is still F
    assert w.apply([], 3, NEW_ONLY) == []
    # the local actor's files alone (a reader without the other writer's file): its members only
    reader = new_core(ctx, key)
    rc, sts = reader.ingest_ops(w.files, [w.actor], [0] * len(w.files), list(range(len(w.files))))
    assert rc == 0 and reader.path_count("gset_fused_files") == len(w.files)
    assert reader.contains(sorted(w.model.state.value - set(held))).all()
    reader.close()
    w.close()


def test_new_only_on_an_empty_set_sorts_and_dedups(ctx, oracle):
    rng = random.Random(10)
    w = Written(ctx, oracle, rng.randbytes(32), rng)
    col = [wm.member_of_width(rng, wm.WIDTH_BYTES[i % 5]) for i in range(5000)]
    col += col[:1000] + [0, U64]
    rng.shuffle(col)
    got = w.apply(col, 453, NEW_ONLY)
    assert len(got) == -(-len(set(col)) // 453)
    w.check_readers()
    w.close()


# ------------------------------------------------------------------ storage
def uuid_str(u):
    h = u.hex()
    return "%s-%s-%s-%s-%s" % (h[:8], h[8:12], h[12:16], h[16:20], h[20:])


def test_storage_round_trip(ctx, oracle, tmp_path):
    """a core with storage writes: the files sit at ops/<actor>/<v0 + i> with the model's bytes; a
    second replica's read_remote and compact reach the model's state, in a file named by its hash"""
    rng = random.Random(11)
    key = rng.randbytes(32)
    remote = str(tmp_path / "remote")
    w = Written(ctx, oracle, key, rng, local_path=str(tmp_path / "l1"), remote_path=remote, flags=crdtenc.OPEN_CREATE)
    w.apply([wm.member_of_width(rng, wm.WIDTH_BYTES[i % 5]) for i in range(100)], 16)
    w.apply(wm.WIDTH_EDGES, 5, host=True)
    w.apply([wm.member_of_width(rng, 9) for _ in range(40)] + wm.WIDTH_EDGES, 9, NEW_ONLY)
    d = os.path.join(remote, "ops", uuid_str(w.actor))
    assert sorted(os.listdir(d), key=int) == [str(i) for i in range(len(w.files))]
    for i, f in enumerate(w.files):
        assert open(os.path.join(d, str(i)), "rb").read() == f
    c2 = new_core(ctx, key, local_path=str(tmp_path / "l2"), remote_path=remote, flags=crdtenc.OPEN_CREATE)
    assert c2.read_remote() == 0 and c2.state_bytes() == w.model.serialize()
    rc, name = c2.compact()
    st = crdtenc.Storage(str(tmp_path / "l2"), remote)
    assert rc == 0 and st.list_state_names() == [name]
    f = st.load_state(name)
    s, pt = oracle.cryptor_decrypt(key, f[16:])
    assert s == 0 and f[:16] == APP and pt == w.model.serialize() and crdtenc.content_name(f) == name
    c2.close()
    w.close()


# ------------------------------------------------------------------ host twin
def test_host_twin_writes_the_same_bytes(ctx, oracle):
    rng = random.Random(12)
    key = rng.randbytes(32)
    a = Written(ctx, oracle, key, random.Random(99))
    b = Written(ctx, oracle, key, random.Random(99))        # the same nonces
    for per_file, n in ((16, 100), (453, 454), (1, 3), (17, 0)):
        col = [wm.member_of_width(rng, wm.WIDTH_BYTES[i % 5]) for i in range(n)]
        assert a.apply(col, per_file) == b.apply(col, per_file, host=True)
    col = list(range(50)) * 2
    assert a.apply(col, 8, NEW_ONLY) == b.apply(col, 8, NEW_ONLY, host=True)
    assert a.core.state_bytes().replace(a.actor, b.actor) == b.core.state_bytes()
    b.check_readers()
    a.close()
    b.close()


# ------------------------------------------------------------------ refusals
def test_refusals_touch_nothing(ctx, oracle, tmp_path):
    """a wrong kind, a bad per_file, unknown flags, cap below the bound, a column whose clear-text
    bound reaches 2^32, no key: each returns its code and leaves state_bytes(), the storage
    directory, the local actor's next version and every output as they were"""
    rng = random.Random(13)
    key = rng.randbytes(32)
    remote = str(tmp_path / "remote")
    w = Written(ctx, oracle, key, rng, local_path=str(tmp_path / "l1"), remote_path=remote, flags=crdtenc.OPEN_CREATE)
    w.apply([1, 2, 3, 1 << 40], 2)
    gc = new_core(ctx, key, kind=crdtenc.STATE_GCOUNTER)
    nokey = new_core(ctx, None, local_path=str(tmp_path / "l2"), remote_path=remote, flags=crdtenc.OPEN_CREATE)
    col = [7, 8, 9, 1 << 50, 0, U64]
    n = len(col)
    members = u64_dev(col)
    _, max_files, max_bytes = crdtenc.gset_apply_bound(n, 2)
    # the smallest column at 453 a file whose bound 19 F + 9 n reaches 2^32 (refused before it is read)
    lo, huge = 0, 1 << 32
    while lo < huge:
        mid = (lo + huge) // 2
        if 19 * -(-mid // 453) + 9 * mid >= 1 << 32:
            huge = mid
        else:
            lo = mid + 1
    assert 19 * -(-(huge - 1) // 453) + 9 * (huge - 1) < 1 << 32 <= 19 * -(-huge // 453) + 9 * huge
    cases = [(gc, n, 2, 0, max_bytes, INVALID), (w.core, n, 454, 0, 1 << 20, INVALID),
             (w.core, n, 2, 2, max_bytes, INVALID), (w.core, n, 2, NEW_ONLY | 4, max_bytes, INVALID),
             (w.core, n, 2, 0, max_bytes - 1, INVALID), (w.core, n, 2, NEW_ONLY, max_bytes - 1, INVALID),
             (w.core, huge, 453, 0, 1 << 62, INVALID), (w.core, huge, 0, NEW_ONLY, 1 << 62, INVALID),
             (nokey, n, 2, 0, max_bytes, NO_KEY)]

    def tree():
        return sorted((p, tuple(sorted(fs))) for p, _, fs in os.walk(str(tmp_path)))
    before = {c: c.state_bytes() for c in (w.core, gc, nokey)}
    disk = tree()
    nonces = ctypes.create_string_buffer(b"\x55" * (24 * max_files))
    for core, cnt, per_file, flags, cap, code in cases:
        d_files = torch.full((max_bytes + GUARD,), FILL, dtype=torch.uint8, device=DEV)
        d_offs = torch.full((max_files + 1 + GUARD,), -1, dtype=torch.int64, device=DEV)
        torch.cuda.synchronize()
        nf, nb = ctypes.c_uint32(0xDEADBEEF), ctypes.c_uint64(0xDEADBEEFDEADBEEF)
        rc = crdtenc.lib().ce_core_gset_apply_members_device(
            core.p, ctypes.c_void_p(members.data_ptr()), ctypes.c_uint64(cnt), ctypes.c_uint32(per_file),
            ctypes.c_uint32(flags), nonces, ctypes.c_void_p(d_files.data_ptr()), ctypes.c_uint64(cap),
            ctypes.c_void_p(d_offs.data_ptr()), ctypes.byref(nf), ctypes.byref(nb))
        assert rc == code, (rc, code, cnt, per_file, flags, cap)
        assert (nf.value, nb.value) == (0xDEADBEEF, 0xDEADBEEFDEADBEEF)
        assert bool((d_files == FILL).all()) and bool((d_offs == -1).all())
        assert core.state_bytes() == before[core] and tree() == disk
        if cap >= max_bytes and cnt == n:       # the host twin refuses the same arguments (it has no cap)
            assert core.gset_apply_members(col, per_file, flags, [b"\x55" * 24] * max_files) == (code, None)
            assert core.state_bytes() == before[core] and tree() == disk
    # the writer still writes its next version after all of them
    got = w.apply(col, 2, NEW_ONLY)
    assert len(got) == 3 and os.path.exists(os.path.join(remote, "ops", uuid_str(w.actor), str(len(w.files) - 1)))
    for c in (gc, nokey):
        c.close()
    w.close()
