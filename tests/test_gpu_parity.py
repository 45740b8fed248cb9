"""GPU parity: the HIP path through the C ABI vs the oracle and the golden fixtures.

Bit-exact everywhere (integer / byte work): plaintexts, ciphertexts, tags, per-file statuses,
serialized StateWrapper bytes and content names.
"""
import os
import random
import struct

import msgpack
import numpy as np
import pytest

import crdtenc
from wave_run_corpus import OPEN_KEYS, _tail_length_batch

pytestmark = pytest.mark.gpu
H = bytes.fromhex
APP = H("aadfd5a66e194b24a8024fa27c72f20c")
CORE = crdtenc.CORE_VERSION


@pytest.fixture(scope="module")
def ctx():
    c = crdtenc.Context(0)
    yield c
    c.close()


def box(nonce, ct):
    return msgpack.packb([H("c7f269be0ff54a7799c37c23c96d5cb4"),
                          msgpack.packb({"nonce": nonce, "enc_data": ct}, use_bin_type=True)],
                         use_bin_type=True)


# ------------------------------------------------------------------ cryptor (EncHandler)
def test_encrypt_matches_oracle_every_length(ctx, oracle, kats):
    for v in kats["xchacha"]:
        key, nonce, pt = H(v["key"]), H(v["nonce"]), v["pt_bytes"]
        enc = ctx.encrypt(key, pt, nonce=nonce)
        st, want = oracle.cryptor_encrypt(key, nonce, pt)
        assert st == 0 and enc == want, v["len"]
        assert enc.endswith(v["ct_bytes"])                 # OpenSSL-generated ct || tag


def test_decrypt_kat_vectors(ctx, kats):
    for v in kats["xchacha"]:
        key, nonce = H(v["key"]), H(v["nonce"])
        st, pt = ctx.decrypt(key, box(nonce, v["ct_bytes"]))
        assert st == 0 and pt == v["pt_bytes"], v["len"]


def test_decrypt_batch_tamper_scrubs(ctx, kats):
    items, want = [], []
    key = H(kats["xchacha"][0]["key"])
    rng = random.Random(5)
    # one key for the whole batch: re-seal every vector's plaintext under `key`
    for i, v in enumerate(kats["xchacha"]):
        nonce = rng.randbytes(24)
        enc = ctx.encrypt(key, v["pt_bytes"], nonce=nonce)
        if i % 3 == 1 and v["len"] > 0:
            b = bytearray(enc)
            b[-1 - rng.randrange(16 + v["len"])] ^= 1 << rng.randrange(8)
            enc = bytes(b)
            want.append((9, None))
        else:
            want.append((0, v["pt_bytes"]))
        items.append(enc)
    rc, st, pts, raw, offs = ctx.decrypt_batch(key, items)
    assert [s for s in st] == [w[0] for w in want]
    assert rc == next(w[0] for w in want if w[0] != 0)
    for i, (s, p) in enumerate(want):
        if s == 0:
            assert pts[i] == p
        else:
            # verify-before-release: the failed file's region holds no plaintext
            n = len(kats["xchacha"][i]["pt_bytes"])
            assert raw[offs[i]:offs[i] + n] == bytes(n)


def test_key_checks_come_first(ctx, repo_fx):
    key = H(repo_fx["key"])
    f = H(repo_fx["files"][0]["file"])[16:]
    assert ctx.decrypt(key, f, key_version=bytes(16))[0] == 3
    assert ctx.decrypt(key[:31], f)[0] == 4
    assert ctx.decrypt(key, b"\xc0")[0] == 5


def test_encrypt_batch_random_nonces_roundtrip(ctx, oracle):
    key = os.urandom(32)
    clears = [os.urandom(n) for n in [0, 5, 4096, 16384 - 16, 16384 + 1, 70000]]
    encs = ctx.encrypt_batch(key, clears)
    for c, e in zip(clears, encs):
        st, pt = oracle.cryptor_decrypt(key, e)
        assert st == 0 and pt == c


# ------------------------------------------------------------------ core ingest
def files_of(repo_fx):
    files = [H(f["file"]) for f in repo_fx["files"]]
    actors = [H(a) for a in repo_fx["actors"]]
    idx = {a: i for i, a in enumerate(actors)}
    fa = [idx[H(f["actor"])] for f in repo_fx["files"]]
    vers = [f["version"] for f in repo_fx["files"]]
    return files, actors, fa, vers


def new_core(ctx, repo_fx, kind, **kw):
    c = crdtenc.Core(ctx, kind=kind, supported=[APP], current_data_version=APP, **kw)
    c.set_latest_key(H(repo_fx["key"]))
    return c


@pytest.mark.parametrize("kind", ["gcounter", "vclock"])
def test_ingest_ops_golden(ctx, repo_fx, kind):
    k = crdtenc.STATE_GCOUNTER if kind == "gcounter" else crdtenc.STATE_VCLOCK
    core = new_core(ctx, repo_fx, k)
    files, actors, fa, vers = files_of(repo_fx)
    rc, st = core.ingest_ops(files, actors, fa, vers)
    assert rc == 0 and st == [0] * len(files)
    assert core.state_bytes().hex() == repo_fx["expected_state"][kind]
    # idempotent re-read: every file is below next_op_versions and skipped
    rc, st = core.ingest_ops(files, actors, fa, vers)
    assert rc == 0 and core.state_bytes().hex() == repo_fx["expected_state"][kind]


@pytest.mark.parametrize("kind", ["gcounter", "vclock"])
def test_ingest_states_then_ops(ctx, repo_fx, kind):
    k = crdtenc.STATE_GCOUNTER if kind == "gcounter" else crdtenc.STATE_VCLOCK
    core = new_core(ctx, repo_fx, k)
    rc, st = core.ingest_states([H(repo_fx["state_files"][kind])])
    assert rc == 0, st
    files, actors, fa, vers = files_of(repo_fx)
    rc, st = core.ingest_ops(files, actors, fa, vers)
    assert rc == 0
    assert core.state_bytes().hex() == repo_fx["expected_after_state_then_ops"][kind]


def test_negative_statuses_match_fixture(ctx, repo_fx, oracle):
    for case in repo_fx["negatives"]:
        core = new_core(ctx, repo_fx, crdtenc.STATE_GCOUNTER)
        empty = core.state_bytes()
        rc, st = core.ingest_ops([H(case["file"])], [bytes(16)], [0], [0])
        assert st[0] == case["status"], (case["name"], st[0], case["status"])
        if case["status"]:
            assert rc == case["status"] and core.state_bytes() == empty
        # and the oracle agrees
        oc = oracle.Core()
        _, ost = oc.read_remote_ops(H(repo_fx["key"]), [APP], [H(case["file"])], [bytes(16)], [0])
        assert ost == st


def test_batch_reject_leaves_state(ctx, repo_fx):
    core = new_core(ctx, repo_fx, crdtenc.STATE_GCOUNTER)
    files, actors, fa, vers = files_of(repo_fx)
    empty = core.state_bytes()
    bad = bytearray(files[7])
    bad[-3] ^= 1
    files[7] = bytes(bad)
    rc, st = core.ingest_ops(files, actors, fa, vers)
    assert rc == 9 and st[7] == 9 and sum(s != 0 for s in st) == 1
    assert core.state_bytes() == empty


def test_version_gate_matches_oracle(ctx, repo_fx, oracle):
    files, actors, fa, vers = files_of(repo_fx)
    keep = [i for i in range(len(files)) if not (fa[i] == 1 and vers[i] == 3)]
    sel = lambda xs: [xs[i] for i in keep]
    core = new_core(ctx, repo_fx, crdtenc.STATE_GCOUNTER)
    rc, st = core.ingest_ops(sel(files), actors, sel(fa), sel(vers))
    oc = oracle.Core()
    orc, ost = oc.read_remote_ops(H(repo_fx["key"]), [APP], sel(files), [actors[i] for i in sel(fa)],
                                  sel(vers))
    assert rc == orc == 13
    assert st == ost
    assert core.state_bytes() == oc.serialize()


def test_compact_to_buffer_matches_fixture(ctx, repo_fx):
    for kind, k in (("gcounter", crdtenc.STATE_GCOUNTER), ("vclock", crdtenc.STATE_VCLOCK)):
        core = new_core(ctx, repo_fx, k)
        files, actors, fa, vers = files_of(repo_fx)
        rc = core.ingest_ops(files, actors, fa, vers)[0]
        assert rc == 0, (kind, rc, ctx.last_error())
        c = repo_fx["compact"][kind]
        f, name = core.compact_to_buffer(nonce=H(c["nonce"]))
        assert f.hex() == c["file"] and name == c["name"]
        # caller-owned buffer: grown from 16 bytes, then reused; the name is over its bytes
        buf = np.zeros(16, np.uint8)
        for _ in range(2):
            buf, n, name2 = core.compact_into(buf, nonce=H(c["nonce"]))
            assert bytes(buf[:n]) == f and name2 == name and buf.nbytes >= n
        assert crdtenc.content_name(buf[:n]) == name == crdtenc.content_name(f)


@pytest.mark.parametrize("n_act", [0, 1, 15, 16, 300, 2500, 5000])
@pytest.mark.parametrize("kind", [crdtenc.STATE_GCOUNTER, crdtenc.STATE_VCLOCK])
@pytest.mark.parametrize("flags", [0, crdtenc.COMPACT_INGEST_FORMAT])
def test_device_compaction_serializer(ctx, oracle, n_act, kind, flags):
    """compact_to_buffer serializes the StateWrapper on the device (k_serialize_vclock): its
    sealed clear text must equal the host serializer's state_bytes(), at every uint width and
    map-header size (fixmap <= 15 < map16), with actors present in only one of the two maps."""
    rng = random.Random(n_act * 7 + kind + 3 * flags)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(n_act))
    widths = [7, 8, 16, 32, 64]

    def val():
        w = rng.choice(widths)
        return rng.randrange(1, 1 << w)

    nov = {a: val() for a in actors if rng.random() < 0.8}
    st = {a: val() for a in actors if rng.random() < 0.8}
    inner = {"dots": dict(sorted(st.items()))}
    sw = {"next_op_versions": {"dots": dict(sorted(nov.items()))},
          "state": {"inner": inner} if kind == crdtenc.STATE_GCOUNTER else inner}
    want = msgpack.packb(sw, use_bin_type=True)
    core = crdtenc.Core(ctx, kind=kind, supported=[APP], current_data_version=APP, flags=flags)
    core.set_latest_key(key)
    core.merge_state(want)
    assert core.state_bytes() == want
    nonce = rng.randbytes(24)
    f, name = core.compact_to_buffer(nonce=nonce)
    ingest = flags == crdtenc.COMPACT_INGEST_FORMAT
    assert f[:16] == (CORE if ingest else APP)
    stt, pt = oracle.cryptor_decrypt(key, f[16:])
    assert stt == 0 and pt == (APP + want if ingest else want)
    assert f[16:] == oracle.cryptor_encrypt(key, nonce, pt)[1]
    assert name == crdtenc.content_name(f)
    core.close()


# ------------------------------------------------------------------ larger random batches
def make_ops_batch(ctx, key, n_actors, n_versions, dots_per_file, seed, stress=False):
    rng = random.Random(seed)
    actors = sorted(rng.randbytes(16) for _ in range(n_actors))
    clears, fa, vers = [], [], []
    for v in range(n_versions):
        for a in range(n_actors):
            dots = []
            for d in range(dots_per_file):
                if stress:
                    dots.append({"actor": rng.choice(actors), "counter": rng.getrandbits(rng.choice([7, 8, 16, 32, 64]))})
                else:
                    dots.append({"actor": actors[a], "counter": v * dots_per_file + d + 1})
            clears.append(APP + msgpack.packb(dots, use_bin_type=True))
            fa.append(a)
            vers.append(v)
    # order files per actor (load_ops order): actor-major
    order = sorted(range(len(clears)), key=lambda i: (fa[i], vers[i]))
    clears = [clears[i] for i in order]
    fa = [fa[i] for i in order]
    vers = [vers[i] for i in order]
    encs = ctx.encrypt_batch(key, clears)
    files = [CORE + e for e in encs]
    return files, actors, fa, vers


@pytest.mark.parametrize("stress", [False, True])
def test_random_batch_matches_oracle(ctx, oracle, stress):
    key = os.urandom(32)
    files, actors, fa, vers = make_ops_batch(ctx, key, 37, 9, 23, seed=11 + stress, stress=stress)
    core = crdtenc.Core(ctx, kind=crdtenc.STATE_GCOUNTER, supported=[APP], current_data_version=APP)
    core.set_latest_key(key)
    rc, st = core.ingest_ops(files, actors, fa, vers)
    assert rc == 0 and set(st) == {0}
    oc = oracle.Core()
    orc, ost = oc.read_remote_ops(key, [APP], files, [actors[i] for i in fa], vers)
    assert orc == 0
    assert core.state_bytes() == oc.serialize()


def test_template_path_cases(ctx, oracle):
    """The fused kernel's template path (every Dot of a file carries Dot 0's 34-byte prefix) and
    its fallbacks, file by file against the oracle: counters of every width (cc/cd/ce/cf, fixint
    first Dots), array16 / fixarray headers, one Dot of another actor, of another width or with
    reordered keys at any position, a lone Dot, a tampered file."""
    key = os.urandom(32)
    rng = random.Random(77)
    actors = sorted(rng.randbytes(16) for _ in range(6))
    ranges = {"cc": (128, 255), "cd": (256, 65535), "ce": (65536, (1 << 32) - 1),
              "cf": (1 << 32, (1 << 64) - 1), "fix": (0, 127)}
    clears, fa = [], []
    for i in range(240):
        w = rng.choice(["cc", "cd", "ce", "cf", "ce", "ce"])
        n = rng.choice([1, 2, 3, 15, 16, 17, 31, 32, 33, 47, 64, 80, 90])
        a = rng.randrange(len(actors))
        dots = [{"actor": actors[a], "counter": rng.randint(*ranges[w])} for _ in range(n)]
        case = rng.choice(["clean", "clean", "other_actor", "other_width", "reordered", "fix_first", "fix_all"])
        k = rng.randrange(n)
        if case == "other_actor":
            dots[k]["actor"] = actors[(a + 1) % len(actors)]
        elif case == "other_width":
            dots[k]["counter"] = rng.randint(*ranges[rng.choice([x for x in ranges if x != w])])
        elif case == "reordered":
            dots[k] = {"counter": dots[k]["counter"], "actor": dots[k]["actor"]}
        elif case == "fix_first":
            dots[0]["counter"] = rng.randint(*ranges["fix"])
        elif case == "fix_all":
            for d in dots:
                d["counter"] = rng.randint(*ranges["fix"])
        clears.append(APP + msgpack.packb(dots, use_bin_type=True))
        fa.append(a)
    order = sorted(range(len(clears)), key=lambda i: (fa[i], i))
    clears = [clears[i] for i in order]
    fa = [fa[i] for i in order]
    vers, cnt = [], {}
    for x in fa:
        vers.append(cnt.get(x, 0))
        cnt[x] = cnt.get(x, 0) + 1
    files = [CORE + e for e in ctx.encrypt_batch(key, clears)]
    for tamper in (False, True):
        fs = list(files)
        if tamper:
            j = rng.randrange(len(fs))
            fs[j] = fs[j][:-1] + bytes([fs[j][-1] ^ 1])
        core = crdtenc.Core(ctx, kind=crdtenc.STATE_GCOUNTER, supported=[APP], current_data_version=APP)
        core.set_latest_key(key)
        rc, st = core.ingest_ops(fs, actors, fa, vers)
        oc = oracle.Core()
        orc, ost = oc.read_remote_ops(key, [APP], fs, [actors[i] for i in fa], vers)
        assert rc == orc and (tamper or set(st) == {0})
        assert core.state_bytes() == oc.serialize()
        core.close()


def test_unknown_dot_actors_grow_table(ctx, oracle):
    """Dots naming actors that are not op writers (table misses -> refold)."""
    key = os.urandom(32)
    rng = random.Random(3)
    writers = [rng.randbytes(16) for _ in range(3)]
    others = [rng.randbytes(16) for _ in range(9000)]   # forces table growth past 8192 slots
    clears = []
    for i in range(30):
        dots = [{"actor": rng.choice(others), "counter": rng.getrandbits(20)} for _ in range(400)]
        clears.append(APP + msgpack.packb(dots, use_bin_type=True))
    files = [CORE + e for e in ctx.encrypt_batch(key, clears)]
    fa = [i % 3 for i in range(30)]
    order = sorted(range(30), key=lambda i: (fa[i], i))
    files = [files[i] for i in order]
    fa = [fa[i] for i in order]
    vers = []
    cnt = {}
    for a in fa:
        vers.append(cnt.get(a, 0))
        cnt[a] = cnt.get(a, 0) + 1
    core = crdtenc.Core(ctx, kind=crdtenc.STATE_VCLOCK, supported=[APP], current_data_version=APP)
    core.set_latest_key(key)
    rc, st = core.ingest_ops(files, writers, fa, vers)
    assert rc == 0
    oc = oracle.Core(oracle.STATE_VCLOCK)
    assert oc.read_remote_ops(key, [APP], files, [writers[i] for i in fa], vers)[0] == 0
    assert core.state_bytes() == oc.serialize()


def test_skewed_sizes_multi_segment(ctx, oracle):
    """Files from 256 B to 1 MiB: multi-wave segments + partial Poly1305 combine."""
    key = os.urandom(32)
    rng = random.Random(9)
    actor = rng.randbytes(16)
    clears, ctr = [], 0
    for i in range(12):
        target = int(256 * (4096 ** (i / 11)))     # 256 B .. 1 MiB, log-spaced
        ndots = max(1, target // 36)
        dots = []
        for _ in range(ndots):
            ctr += rng.choice([1, 300, 70000])
            dots.append({"actor": actor, "counter": ctr})
        clears.append(APP + msgpack.packb(dots, use_bin_type=True))
    files = [CORE + e for e in ctx.encrypt_batch(key, clears)]
    core = crdtenc.Core(ctx, kind=crdtenc.STATE_GCOUNTER, supported=[APP], current_data_version=APP)
    core.set_latest_key(key)
    rc, st = core.ingest_ops(files, [actor], [0] * 12, list(range(12)))
    assert rc == 0
    oc = oracle.Core()
    assert oc.read_remote_ops(key, [APP], files, [actor] * 12, list(range(12)))[0] == 0
    assert core.state_bytes() == oc.serialize()
    # and a tamper in the middle of the biggest file is caught by the segment combine
    bad = bytearray(files[-1])
    bad[len(bad) // 2] ^= 2
    core2 = crdtenc.Core(ctx, kind=crdtenc.STATE_GCOUNTER, supported=[APP], current_data_version=APP)
    core2.set_latest_key(key)
    rc, st = core2.ingest_ops(files[:-1] + [bytes(bad)], [actor], [0] * 12, list(range(12)))
    assert rc == 9 and st[-1] == 9


@pytest.mark.gpu
@pytest.mark.parametrize("n", [255, 256, 257, 769])
def test_setup_block_tails(ctx, oracle, n):
    """k_open_setup stages each 256-file block's FileParams through LDS and stores the rows
    that exist: batches around the block size, a tampered file and a wrong-version file in the
    last (partial) block, state and every status == oracle."""
    key = os.urandom(32)
    rng = random.Random(n)
    actors = [rng.randbytes(16) for _ in range(7)]
    fa = sorted(i % 7 for i in range(n))          # Storage::load_ops order: actor, then version
    ver = [fa[:i].count(fa[i]) for i in range(n)]
    clears = []
    for i in range(n):
        a = actors[fa[i]]
        clears.append(APP + msgpack.packb([{"actor": a, "counter": 1 + i * 3 + k} for k in range(1 + i % 5)],
                                          use_bin_type=True))
    files = [CORE + e for e in ctx.encrypt_batch(key, clears)]
    bad = bytearray(files[n - 1])
    bad[-5] ^= 1                                   # tag of the very last file
    files[n - 1] = bytes(bad)
    files[n - 2] = b"\x00" * 16 + files[n - 2][16:]  # outer version of the one before
    core = crdtenc.Core(ctx, kind=crdtenc.STATE_GCOUNTER, supported=[APP], current_data_version=APP)
    core.set_latest_key(key)
    rc, st = core.ingest_ops(files, actors, fa, ver)
    oc = oracle.Core()
    orc = oc.read_remote_ops(key, [APP], files, [actors[i] for i in fa], ver)
    assert rc == orc[0] and rc != 0
    assert st[n - 1] != 0 and st[n - 2] != 0 and all(x == 0 for x in st[:n - 2])
    assert st == orc[1]
    assert core.state_bytes() == oc.serialize()


@pytest.mark.gpu
@pytest.mark.parametrize("split", [False, True])
def test_split_decode_paths(ctx, oracle, monkeypatch, split):
    """With CE_SPLIT=1, multi-page files of >= 2048 Dots go to k_decode_split (16 waves per file): uniform Dot
    length with one actor folds from the part records; a second registered actor, an
    unregistered actor (miss), a Dot length change in the last part and a non-canonical Dot
    each fall back to the one-wave decode of the whole file.  State == oracle for every file."""
    key = os.urandom(32)
    rng = random.Random(21)
    writer, other, stranger = rng.randbytes(16), rng.randbytes(16), rng.randbytes(16)
    base = 1 << 20                      # uint32 counters: 38-byte Dots throughout

    def dots(n, actor_of=lambda i: writer, ctr_of=lambda i: base + i):
        return [{"actor": actor_of(i), "counter": ctr_of(i)} for i in range(n)]

    bodies = [
        dots(5000),                                                    # fast path
        dots(3000, ctr_of=lambda i: base + 7 * i),                     # fast path, max not last
        dots(4000, actor_of=lambda i: other if i == 3999 else writer),  # second actor, last part
        dots(4000, actor_of=lambda i: stranger if i == 2500 else writer),  # miss
        dots(4000, ctr_of=lambda i: 5 if i == 3998 else base + i),     # shorter Dot near the end
        dots(2047),                                                    # below the split size
    ]
    clears = [APP + msgpack.packb(b, use_bin_type=True) for b in bodies]
    # a non-canonical Dot (keys in the other order) in the middle of a uniform file
    od = msgpack.packb({"counter": base + 1, "actor": writer}, use_bin_type=True)
    canon = [msgpack.packb(d, use_bin_type=True) for d in dots(4000)]
    canon[1700] = od
    clears.append(APP + b"\xdd" + (4000).to_bytes(4, "big") + b"".join(canon))
    n = len(clears)
    files = [CORE + e for e in ctx.encrypt_batch(key, clears)]
    if split:  # opt-in multi-wave decode (read per ingest call by the library)
        monkeypatch.setenv("CE_SPLIT", "1")
    core = crdtenc.Core(ctx, kind=crdtenc.STATE_GCOUNTER, supported=[APP], current_data_version=APP)
    core.set_latest_key(key)
    rc, st = core.ingest_ops(files, [writer, other], [0] * n, list(range(n)))
    oc = oracle.Core()
    orc = oc.read_remote_ops(key, [APP], files, [writer] * n, list(range(n)))[0]
    assert rc == orc == 0, (rc, orc, st)
    assert core.state_bytes() == oc.serialize()


# ------------------------------------------------------------------ storage end to end
def test_storage_apply_read_compact(ctx, tmp_path, oracle):
    """Two replicas share a remote dir (syncthing-style, README.md:3-4)."""
    key = os.urandom(32)
    remote = str(tmp_path / "remote")
    c1 = crdtenc.Core(ctx, kind=crdtenc.STATE_GCOUNTER, supported=[APP], current_data_version=APP,
                      local_path=str(tmp_path / "l1"), remote_path=remote, flags=crdtenc.OPEN_CREATE)
    c2 = crdtenc.Core(ctx, kind=crdtenc.STATE_GCOUNTER, supported=[APP], current_data_version=APP,
                      local_path=str(tmp_path / "l2"), remote_path=remote,
                      flags=crdtenc.OPEN_CREATE | crdtenc.COMPACT_INGEST_FORMAT)
    for c in (c1, c2):
        c.set_latest_key(key)
    a1, a2 = c1.info_actor(), c2.info_actor()
    for i in range(5):
        assert c1.apply_ops(msgpack.packb([{"actor": a1, "counter": i + 1}], use_bin_type=True)) == 0
    for i in range(3):
        assert c2.apply_ops(msgpack.packb([{"actor": a2, "counter": 10 * (i + 1)}], use_bin_type=True)) == 0
    assert c1.read_remote() == 0 and c2.read_remote() == 0
    assert c1.state_bytes() == c2.state_bytes()
    # the state equals the oracle fold of the stored op files
    st = crdtenc.Storage(str(tmp_path / "l1"), remote)
    loaded = st.load_ops([(a1, 0), (a2, 0)])
    oc = oracle.Core()
    assert oc.read_remote_ops(key, [APP], [x[2] for x in loaded], [x[0] for x in loaded],
                              [x[1] for x in loaded])[0] == 0
    assert c1.state_bytes() == oc.serialize()
    # local meta survives a reopen (lib.rs:250-259)
    c1b = crdtenc.Core(ctx, kind=crdtenc.STATE_GCOUNTER, supported=[APP], current_data_version=APP,
                       local_path=str(tmp_path / "l1"), remote_path=remote)
    assert c1b.info_actor() == a1
    # compact (ingest format) on c2: one state file, the last op of each actor removed
    rc, name = c2.compact()
    assert rc == 0 and st.list_state_names() == [name]
    left = st.load_ops([(a1, 0), (a2, 0)])
    assert [(x[0], x[1]) for x in left] == [(a1, v) for v in range(4)] + [(a2, v) for v in range(2)]
    # a fresh replica reads the compacted state + skips the ops it already covers
    c3 = crdtenc.Core(ctx, kind=crdtenc.STATE_GCOUNTER, supported=[APP], current_data_version=APP,
                      local_path=str(tmp_path / "l3"), remote_path=remote, flags=crdtenc.OPEN_CREATE)
    c3.set_latest_key(key)
    assert c3.read_remote() == 0
    assert c3.state_bytes() == c2.state_bytes()


def test_reference_compact_format_is_unreadable_by_read_remote(ctx, tmp_path):
    """Core::compact writes VersionBytes(current_data_version, encrypt(state)),
    which read_remote_states rejects (outer version != CURRENT_VERSION)."""
    key = os.urandom(32)
    remote = str(tmp_path / "remote")
    c1 = crdtenc.Core(ctx, kind=crdtenc.STATE_GCOUNTER, supported=[APP], current_data_version=APP,
                      local_path=str(tmp_path / "l1"), remote_path=remote, flags=crdtenc.OPEN_CREATE)
    c1.set_latest_key(key)
    a1 = c1.info_actor()
    assert c1.apply_ops(msgpack.packb([{"actor": a1, "counter": 7}], use_bin_type=True)) == 0
    rc, name = c1.compact()
    assert rc == 0
    f = crdtenc.Storage(str(tmp_path / "l1"), remote).load_state(name)
    assert f[:16] == APP
    c2 = crdtenc.Core(ctx, kind=crdtenc.STATE_GCOUNTER, supported=[APP], current_data_version=APP,
                      local_path=str(tmp_path / "l2"), remote_path=remote, flags=crdtenc.OPEN_CREATE)
    c2.set_latest_key(key)
    assert c2.read_remote() == 2     # "version check failed" (lib.rs:435)


@pytest.mark.parametrize("fused,fpw", [("1", "1"), ("1", "2"), ("1", "4"), ("2", "2"), ("2", "4")])
def test_fused_geometries_match_oracle(ctx, oracle, fused, fpw, monkeypatch):
    """k_open_fold_small<64|32|16> (CE_FUSED=1 with 1, 2 and 4 files per wavefront),
    k_open_fold_v2<32, 3, false, 3> (CE_FUSED=2 with 2) and the default k_open_fold_v3<false, true>
    (CE_FUSED=2 with 4; k_open_fold_v2<16, ...> is reached only under CE_FUSED_V2, see
    test_gpu_wave_runs.py); mixed single-page sizes.  The path counters say which kernel ran."""
    monkeypatch.setenv("CE_FILES_PER_WAVE", fpw)
    monkeypatch.setenv("CE_FUSED", fused)
    key = os.urandom(32)
    rng = random.Random(int(fpw) + 10 * int(fused))
    actors = sorted(rng.randbytes(16) for _ in range(13))
    clears, fa, vers = [], [], []
    for a in range(13):
        for v in range(11):
            nd = rng.choice([0, 1, 3, 15, 16, 17, 63, 64, 65, 100, 107])
            dots = [{"actor": actors[a] if rng.random() < 0.7 else rng.choice(actors),
                     "counter": rng.getrandbits(rng.choice([5, 7, 8, 16, 32, 63]))} for _ in range(nd)]
            clears.append(APP + msgpack.packb(dots, use_bin_type=True))
            fa.append(a)
            vers.append(v)
    files = [CORE + e for e in ctx.encrypt_batch(key, clears)]
    assert max(len(c) for c in clears) <= 4096
    core = crdtenc.Core(ctx, kind=crdtenc.STATE_GCOUNTER, supported=[APP], current_data_version=APP)
    core.set_latest_key(key)
    rc, st = core.ingest_ops(files, actors, fa, vers)
    oc = oracle.Core()
    orc, ost = oc.read_remote_ops(key, [APP], files, [actors[i] for i in fa], vers)
    assert rc == orc == 0 and st == ost
    assert core.state_bytes() == oc.serialize()
    _only_open_kernel(core, fused, fpw)
    # one tampered file in the middle of a 4-file wave group: whole batch rejected
    bad = bytearray(files[50])
    bad[-20] ^= 8
    files2 = files[:50] + [bytes(bad)] + files[51:]
    core2 = crdtenc.Core(ctx, kind=crdtenc.STATE_GCOUNTER, supported=[APP], current_data_version=APP)
    core2.set_latest_key(key)
    empty = core2.state_bytes()
    rc, st = core2.ingest_ops(files2, actors, fa, vers)
    assert rc == 9 and st[50] == 9 and core2.state_bytes() == empty
    _only_open_kernel(core2, fused, fpw)


FUSED_KERNEL_KEY = {("1", "1"): "open_small_lpf64", ("1", "2"): "open_small_lpf32", ("1", "4"): "open_small_lpf16",
                    ("2", "2"): "open_v2_lpf32", ("2", "4"): "open_v3_p0e1"}


def _only_open_kernel(core, fused, fpw):
    """The open kernel these parameters reach today ran, and no other"""
    key = FUSED_KERNEL_KEY[(fused, fpw)]
    counts = {k: core.path_count(k) for k in OPEN_KEYS}
    assert counts[key] >= 1 and all(v == 0 for k, v in counts.items() if k != key), counts


@pytest.mark.parametrize("fused,fpw", [("1", "4"), ("2", "4"), ("2", "2")])
def test_fused_every_tail_length(ctx, oracle, fused, fpw, monkeypatch):
    """Single-page files of every length class: each ciphertext length mod 64 (0..3 Poly1305
    pieces missing from the last ChaCha20 block, partial last pieces), the shortest envelopes and
    the last 128 lengths up to one page, through k_open_fold_small<16> (CE_FUSED=1),
    k_open_fold_v2<32, 3, false, 3> (CE_FUSED=2 with 2 files per wavefront) and the default
    k_open_fold_v3<false, true> (CE_FUSED=2 with 4), as the path counters confirm; then tampered
    tags and ciphertext bytes at several tail classes (per-file statuses == oracle, batch
    rejected)."""
    monkeypatch.setenv("CE_FILES_PER_WAVE", fpw)
    monkeypatch.setenv("CE_FUSED", fused)
    key = os.urandom(32)
    rng = random.Random(1000 + 10 * int(fused) + int(fpw))
    actors = sorted(rng.randbytes(16) for _ in range(6))
    lens = list(range(17, 17 + 192)) + list(range(4096 - 127, 4097)) + \
        [rng.randrange(17, 4097) for _ in range(160)]
    rng.shuffle(lens)
    clears, fa, vers = _tail_length_batch(rng, actors, lens)
    assert sorted(len(c) for c in clears) == sorted(lens)
    files = [CORE + e for e in ctx.encrypt_batch(key, clears)]
    core = crdtenc.Core(ctx, kind=crdtenc.STATE_GCOUNTER, supported=[APP], current_data_version=APP)
    core.set_latest_key(key)
    rc, st = core.ingest_ops(files, actors, fa, vers)
    oc = oracle.Core()
    orc, ost = oc.read_remote_ops(key, [APP], files, [actors[i] for i in fa], vers)
    assert rc == orc == 0 and st == ost
    assert core.state_bytes() == oc.serialize()
    _only_open_kernel(core, fused, fpw)
    # tamper: the tag of one file per (length mod 64) class in 1..4 pieces-missing shapes, and a
    # ciphertext byte in the partial last piece of another
    bad = list(files)
    picked = {}
    for i, L in enumerate(lens):
        cls = (L % 64 + 15) // 16
        if cls not in picked and L % 16:
            picked[cls] = i
    for cls, i in picked.items():
        b = bytearray(bad[i])
        if cls % 2:
            b[-1] ^= 0x80                 # tag
        else:
            b[-17] ^= 0x01                # last ciphertext byte
        bad[i] = bytes(b)
    core2 = crdtenc.Core(ctx, kind=crdtenc.STATE_GCOUNTER, supported=[APP], current_data_version=APP)
    core2.set_latest_key(key)
    empty = core2.state_bytes()
    rc2, st2 = core2.ingest_ops(bad, actors, fa, vers)
    oc2 = oracle.Core()
    orc2, ost2 = oc2.read_remote_ops(key, [APP], bad, [actors[i] for i in fa], vers)
    assert rc2 == orc2 == 9 and st2 == ost2
    assert all(st2[i] == 9 for i in picked.values())
    assert core2.state_bytes() == empty
    _only_open_kernel(core2, fused, fpw)


def test_unordered_batch_uses_host_gate(ctx, oracle):
    """Files not in load_ops order (actors interleaved, versions shuffled): the device gate
    declines and the host gate reproduces the reference loop exactly."""
    key = os.urandom(32)
    files, actors, fa, vers = make_ops_batch(ctx, key, 5, 6, 4, seed=99)
    rng = random.Random(1)
    order = list(range(len(files)))
    rng.shuffle(order)
    sel = lambda xs: [xs[i] for i in order]
    core = crdtenc.Core(ctx, kind=crdtenc.STATE_GCOUNTER, supported=[APP], current_data_version=APP)
    core.set_latest_key(key)
    rc, st = core.ingest_ops(sel(files), actors, sel(fa), sel(vers))
    oc = oracle.Core()
    orc, ost = oc.read_remote_ops(key, [APP], sel(files), [actors[i] for i in sel(fa)], sel(vers))
    assert rc == orc and st == ost
    assert core.state_bytes() == oc.serialize()
    # interleaved but per-actor ordered (round-robin) -> no gap, everything applies
    rr = sorted(range(len(files)), key=lambda i: (vers[i], fa[i]))
    sel2 = lambda xs: [xs[i] for i in rr]
    core2 = crdtenc.Core(ctx, kind=crdtenc.STATE_GCOUNTER, supported=[APP], current_data_version=APP)
    core2.set_latest_key(key)
    assert core2.ingest_ops(sel2(files), actors, sel2(fa), sel2(vers))[0] == 0
    oc2 = oracle.Core()
    assert oc2.read_remote_ops(key, [APP], files, [actors[i] for i in fa], vers)[0] == 0
    assert core2.state_bytes() == oc2.serialize()


def test_device_metadata_api(ctx, oracle):
    """ce_core_ingest_ops_device with files + per-file metadata in HBM (torch tensors)."""
    torch = pytest.importorskip("torch")
    import numpy as np
    key = os.urandom(32)
    files, actors, fa, vers = make_ops_batch(ctx, key, 9, 7, 30, seed=5)
    blob = b"".join(files)
    offs = np.zeros(len(files) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(f) for f in files])
    d_blob = torch.tensor(list(blob) + [0] * 64, dtype=torch.uint8, device="cuda")
    d_offs = torch.tensor(offs, device="cuda")
    d_fa = torch.tensor(np.array(fa, dtype=np.int32), device="cuda")
    d_fv = torch.tensor(np.array(vers, dtype=np.int64), device="cuda")
    torch.cuda.synchronize()
    core = crdtenc.Core(ctx, kind=crdtenc.STATE_VCLOCK, supported=[APP], current_data_version=APP)
    core.set_latest_key(key)
    rc, st = core.ingest_ops_device(d_blob.data_ptr(), d_offs.data_ptr(), len(files), len(blob),
                                    b"".join(actors), d_fa.data_ptr(), d_fv.data_ptr(),
                                    want_status=True)
    assert rc == 0 and set(st) == {0}
    oc = oracle.Core(oracle.STATE_VCLOCK)
    assert oc.read_remote_ops(key, [APP], files, [actors[i] for i in fa], vers)[0] == 0
    assert core.state_bytes() == oc.serialize()


def test_dense_exchange_two_shards(ctx, oracle):
    """The multi-GPU exchange on one GPU: two cores fold disjoint actor shards (stress dots with
    u64 counters >= 2^63 across shards), export_dense, u64-max combine, import_dense -> the
    single-fold state (shard.py; bench.py runs the same over RCCL)."""
    torch = pytest.importorskip("torch")
    import shard
    key = os.urandom(32)
    files, actors, fa, vers = make_ops_batch(ctx, key, 10, 4, 17, seed=21, stress=True)
    oc = oracle.Core()
    assert oc.read_remote_ops(key, [APP], files, [actors[i] for i in fa], vers)[0] == 0
    cores, dense = [], []
    for r in range(2):
        lo, hi = shard.actor_range(len(actors), 2, r)
        sel = [i for i in range(len(files)) if lo <= fa[i] < hi]
        c = crdtenc.Core(ctx, kind=crdtenc.STATE_GCOUNTER, supported=[APP], current_data_version=APP)
        c.set_latest_key(key)
        c.register_actors(actors)
        rc, _ = c.ingest_ops([files[i] for i in sel], actors[lo:hi], [fa[i] - lo for i in sel],
                             [vers[i] for i in sel])
        assert rc == 0
        cap = c.dense_capacity()
        st = torch.zeros(cap, dtype=torch.int64, device="cuda")
        nv = torch.zeros(cap, dtype=torch.int64, device="cuda")
        c.export_dense(st.data_ptr(), nv.data_ptr())
        cores.append(c)
        dense.append((st, nv))
    assert cores[0].dense_capacity() == cores[1].dense_capacity()
    # device merge through import_dense
    cores[0].import_dense(dense[1][0].data_ptr(), dense[1][1].data_ptr())
    assert cores[0].state_bytes() == oc.serialize()
    # the collective's form: u64 max on int64 views, imported into an empty core
    st, nv = dense[0][0].clone(), dense[0][1].clone()
    shard.max_u64_(st, dense[1][0])
    shard.max_u64_(nv, dense[1][1])
    torch.cuda.synchronize()
    fresh = crdtenc.Core(ctx, kind=crdtenc.STATE_GCOUNTER, supported=[APP], current_data_version=APP)
    fresh.set_latest_key(key)
    fresh.register_actors(actors)
    fresh.import_dense(st.data_ptr(), nv.data_ptr())
    assert fresh.state_bytes() == oc.serialize()


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


@pytest.mark.parametrize("case", ["clean", "stress", "foreign_actors", "tampered", "gap"])
@pytest.mark.parametrize("kind", [crdtenc.STATE_GCOUNTER, crdtenc.STATE_VCLOCK])
def test_compact_ops_device(ctx, oracle, case, kind):
    """ce_core_compact_ops_device (Core::compact, lib.rs:332-380, over a batch in HBM) == the
    two-call path ingest_ops_device + compact_to_buffer with the same nonce, on the fast path
    (compaction queued behind the device commit) and on every slow path: actors outside the
    table (refold), a failing tag (read_remote error, nothing written, state unchanged) and a
    version gap (error)."""
    key = os.urandom(32)
    files, actors, fa, vers = make_ops_batch(ctx, key, 6, 5, 20, seed=11, stress=(case != "clean"))
    if case == "foreign_actors":  # dots of actors no writer list names: device misses + refold
        rng = random.Random(3)
        foreign = sorted(rng.randbytes(16) for _ in range(5))
        clears = [APP + msgpack.packb([{"actor": rng.choice(foreign), "counter": rng.getrandbits(40)}
                                       for _ in range(7)], use_bin_type=True) for _ in files]
        files = [CORE + e for e in ctx.encrypt_batch(key, clears)]
    if case == "tampered":
        b = bytearray(files[9]); b[-3] ^= 1; files[9] = bytes(b)
    if case == "gap":  # drop one version of actor 0: versions after it are not contiguous
        keep = [i for i in range(len(files)) if not (fa[i] == 0 and vers[i] == 2)]
        files, fa, vers = [files[i] for i in keep], [fa[i] for i in keep], [vers[i] for i in keep]
    (d_blob, d_offs, d_fa, d_fv), blen = _to_device(files, fa, vers)
    nonce = bytes(range(24))

    def new():
        c = crdtenc.Core(ctx, kind=kind, supported=[APP], current_data_version=APP)
        c.set_latest_key(key)
        return c
    ref = new()
    rc_ref = ref.ingest_ops_device(d_blob.data_ptr(), d_offs.data_ptr(), len(files), blen,
                                   b"".join(actors), d_fa.data_ptr(), d_fv.data_ptr())
    core = new()
    before = core.state_bytes()
    rc, f, name = core.compact_ops_device(d_blob.data_ptr(), d_offs.data_ptr(), len(files), blen,
                                          b"".join(actors), d_fa.data_ptr(), d_fv.data_ptr(),
                                          nonce=nonce)
    assert rc == rc_ref, (rc, rc_ref, ctx.last_error())
    if case == "tampered":
        assert rc == 9 and f is None and core.state_bytes() == before
    elif case == "gap":
        assert rc == 13 and f is None
        assert core.state_bytes() == ref.state_bytes()   # files before the gap stay folded
    else:
        assert rc == 0
        want, want_name = ref.compact_to_buffer(nonce=nonce)
        assert f == want and name == want_name
        assert core.state_bytes() == ref.state_bytes()
        oc = oracle.Core(oracle.STATE_GCOUNTER if kind == crdtenc.STATE_GCOUNTER else oracle.STATE_VCLOCK)
        assert oc.read_remote_ops(key, [APP], files, [actors[i] for i in fa], vers)[0] == 0
        st, pt = oracle.cryptor_decrypt(key, f[16:])
        assert st == 0 and pt == oc.serialize()
        # a second compaction over the same batch: every file is below next_op_versions now
        rc2, f2, _ = core.compact_ops_device(d_blob.data_ptr(), d_offs.data_ptr(), len(files), blen,
                                             b"".join(actors), d_fa.data_ptr(), d_fv.data_ptr(),
                                             nonce=nonce)
        assert rc2 == 0 and f2 == f
        # the same compaction downloaded straight into a caller's pinned buffer (and into a
        # pageable one, and one too small for the bound)
        import torch
        for pinned in (True, False):
            c3 = new()
            buf = torch.empty(1 << 20, dtype=torch.uint8, pin_memory=pinned).numpy()
            rc3, ln, nm3 = c3.compact_ops_device_into(buf, d_blob.data_ptr(), d_offs.data_ptr(), len(files), blen,
                                                      b"".join(actors), d_fa.data_ptr(), d_fv.data_ptr(),
                                                      nonce=nonce, name=True)
            assert rc3 == 0 and bytes(buf[:ln]) == f and nm3 == name
            assert c3.state_bytes() == ref.state_bytes()
            c3.close()
        c4 = new()
        small = np.zeros(len(f) - 1, np.uint8)
        rc4, ln4, _ = c4.compact_ops_device_into(small, d_blob.data_ptr(), d_offs.data_ptr(), len(files), blen,
                                                 b"".join(actors), d_fa.data_ptr(), d_fv.data_ptr(), nonce=nonce)
        assert rc4 == 64 and ln4 == len(f)   # CE_ERR_INVALID_ARG with the size it needs
        c4.close()
    core.close()
    ref.close()


@pytest.mark.parametrize("n_new", [3, 200])
def test_exotic_envelope_new_actors(ctx, oracle, n_new):
    """Cryptor boxes whose nonce / enc_data are serde_bytes sequences of u8 (not bin): the
    device leaves them to the host parser (kStatusHostParse), which opens the canonical form and
    decodes the plaintext on the GPU.  Their Dots name actors no writer has: those misses go
    through the insert / upload / fold-again loop (200 new actors grow the table, so the ingest
    restarts with the new slots) -- VClock::apply takes any actor (lib.rs:533-535)."""
    rng = random.Random(4242 + n_new)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(8))
    strangers = [rng.randbytes(16) for _ in range(n_new)]
    files, fa, fv, exotic = [], [], [], 0
    for a in range(8):
        for v in range(6):
            dots = [{"actor": actors[a], "counter": 10 * v + d + 1} for d in range(5)]
            ex = (a + v) % 3 == 0
            if ex:
                dots += [{"actor": rng.choice(strangers), "counter": rng.getrandbits(33)}
                         for _ in range(max(1, n_new // 10))]
            clear = APP + msgpack.packb(dots, use_bin_type=True)
            enc = ctx.encrypt(key, clear, nonce=rng.randbytes(24))
            if ex:
                ver, inner = msgpack.unpackb(enc)
                eb = msgpack.unpackb(inner)
                inner = msgpack.packb({"nonce": list(eb["nonce"]), "enc_data": list(eb["enc_data"])},
                                      use_bin_type=True)
                enc = msgpack.packb([ver, inner], use_bin_type=True)
                exotic += 1
            files.append(CORE + enc)
            fa.append(a)
            fv.append(v)
    assert exotic > 0
    oc = oracle.Core()
    orc, ost = oc.read_remote_ops(key, [APP], files, [actors[i] for i in fa], fv)
    assert orc == 0
    core = crdtenc.Core(ctx, kind=crdtenc.STATE_GCOUNTER, supported=[APP], current_data_version=APP)
    core.set_latest_key(key)
    rc, st = core.ingest_ops(files, actors, fa, fv)
    assert (rc, st) == (orc, ost)
    assert core.state_bytes() == oc.serialize()
    core.close()


def test_concurrent_decrypts_one_context(ctx, oracle):
    """include/crdtenc.h: entry points are thread-safe per context.  The reference issues up to
    16 decrypts at once (buffered(16), crdt-enc/src/lib.rs:452,512): 16 threads x 8 calls of
    ce_cryptor_decrypt (ctypes drops the GIL) plus a batch ingest on the same context, every
    result == the oracle's."""
    from concurrent.futures import ThreadPoolExecutor
    rng = random.Random(1616)
    key = rng.randbytes(32)
    items = []
    for i in range(128):
        pt = rng.randbytes(rng.choice([0, 1, 63, 64, 65, 1000, 4096, 20000]))
        enc = ctx.encrypt(key, pt, nonce=rng.randbytes(24))
        if i % 11 == 5:
            b = bytearray(enc)
            b[-1] ^= 0x40
            enc = bytes(b)
        items.append(enc)
    want = [oracle.cryptor_decrypt(key, e) for e in items]
    files, actors, fa, vers = make_ops_batch(ctx, key, 9, 5, 17, seed=16)
    oc = oracle.Core()
    assert oc.read_remote_ops(key, [APP], files, [actors[i] for i in fa], vers)[0] == 0

    def one(i):
        return ctx.decrypt(key, items[i])

    def ingest():
        core = crdtenc.Core(ctx, kind=crdtenc.STATE_GCOUNTER, supported=[APP], current_data_version=APP)
        core.set_latest_key(key)
        rc, _ = core.ingest_ops(files, actors, fa, vers)
        out = (rc, core.state_bytes())
        core.close()
        return out

    with ThreadPoolExecutor(16) as pool:
        futs = [pool.submit(one, i) for i in range(len(items))]
        ing = [pool.submit(ingest) for _ in range(3)]
        got = [f.result() for f in futs]
        ingested = [f.result() for f in ing]
    for (st, pt), (wst, wpt) in zip(got, want):
        assert st == wst
        if st == 0:
            assert pt == wpt
    for rc, sb in ingested:
        assert rc == 0 and sb == oc.serialize()


def test_c1_three_replicas_1k_ops(ctx, tmp_path, oracle):
    """BASELINE C1 at its stated size: 3 replicas (actors) share a remote dir and write ~1k ops
    (Core::apply_ops, lib.rs:666-722: batched with ce_core_apply_ops_batch and single calls
    mixed), whose Dots name ~2,600 distinct actors -- past the 2,048 the initial 8192-slot table
    holds at 1/4 load, so it grows mid-run (asserted) -- and a state file sealed and opened in
    several 16 KiB segments.  Every replica's read_remote folds to the oracle's
    state; compact (ingest format) + a fresh replica reproduce it (lib.rs:332-380, 390-547)."""
    rng = random.Random(1000)
    key = rng.randbytes(32)
    remote = str(tmp_path / "remote")
    pool = [rng.randbytes(16) for _ in range(2600)]
    cores = []
    for r in range(3):
        cores.append(crdtenc.Core(ctx, kind=crdtenc.STATE_GCOUNTER, supported=[APP],
                                  current_data_version=APP, local_path=str(tmp_path / ("l%d" % r)),
                                  remote_path=remote,
                                  flags=crdtenc.OPEN_CREATE | crdtenc.COMPACT_INGEST_FORMAT))
        cores[-1].set_latest_key(key)
    acts = [c.info_actor() for c in cores]
    cap0 = cores[0].dense_capacity()
    written = {a: [] for a in acts}
    for r, c in enumerate(cores):
        total = 0
        while total < 333:
            k = rng.choice([1, 7, 40])
            ops = [msgpack.packb([{"actor": rng.choice(pool + [acts[r]] * 50), "counter": rng.getrandbits(40) + 1}
                                  for _ in range(rng.randint(1, 16))], use_bin_type=True) for _ in range(k)]
            if k == 1:
                assert c.apply_ops(ops[0]) == 0
                written[acts[r]].append(None)
            else:
                rc, files = c.apply_ops_batch(ops, nonces=[rng.randbytes(24) for _ in ops])
                assert rc == 0 and len(files) == k
                written[acts[r]].extend(files)
            total += k
    st = crdtenc.Storage(str(tmp_path / "l0"), remote)
    loaded = st.load_ops([(a, 0) for a in acts])
    assert sum(len(v) for v in written.values()) == len(loaded)
    # what apply_ops_batch returned is what Storage::store_ops wrote
    for a, files in written.items():
        on_disk = [x[2] for x in loaded if x[0] == a]
        assert all(f is None or f == d for f, d in zip(files, on_disk))
    oc = oracle.Core()
    assert oc.read_remote_ops(key, [APP], [x[2] for x in loaded], [x[0] for x in loaded],
                              [x[1] for x in loaded])[0] == 0
    for c in cores:
        assert c.read_remote() == 0
        assert c.state_bytes() == oc.serialize()
    assert len(oc.serialize()) > 20000
    assert cores[0].dense_capacity() > cap0, "the actor table never grew"
    rc, name = cores[1].compact()
    assert rc == 0 and st.list_state_names() == [name]
    fresh = crdtenc.Core(ctx, kind=crdtenc.STATE_GCOUNTER, supported=[APP], current_data_version=APP,
                         local_path=str(tmp_path / "l9"), remote_path=remote, flags=crdtenc.OPEN_CREATE)
    fresh.set_latest_key(key)
    assert fresh.read_remote() == 0
    assert fresh.state_bytes() == oc.serialize()
    for c in cores + [fresh]:
        c.close()


def test_host_iov_ingest_matches_device(ctx, oracle):
    """ce_core_ingest_ops_iov (per-file host buffers, pinned staging ring + copy stream) and
    the contiguous ce_core_ingest_ops == the oracle, here with 8 KiB chunks so files straddle
    chunk boundaries and the two staging buffers are reused many times (a fresh context picks
    CE_UPLOAD_CHUNK up when its uploader is created)."""
    os.environ["CE_UPLOAD_CHUNK"] = "8192"
    try:
        c2 = crdtenc.Context(0)
        key = os.urandom(32)
        files, actors, fa, vers = make_ops_batch(c2, key, 13, 7, 31, seed=77, stress=True)
        oc = oracle.Core()
        orc, ost = oc.read_remote_ops(key, [APP], files, [actors[i] for i in fa], vers)
        for fn in ("ingest_ops_iov", "ingest_ops"):
            core = crdtenc.Core(c2, kind=crdtenc.STATE_GCOUNTER, supported=[APP], current_data_version=APP)
            core.set_latest_key(key)
            rc, st = getattr(core, fn)(files, actors, fa, vers)
            assert (rc, st) == (orc, ost) and rc == 0
            assert core.state_bytes() == oc.serialize()
            core.close()
        c2.close()
    finally:
        del os.environ["CE_UPLOAD_CHUNK"]


@pytest.mark.parametrize("nil_where", ["writer", "dot_only", "absent"])
def test_nil_uuid_actor_lookups(ctx, oracle, nil_where):
    """The device actor lookup reads only the 16-byte key per probe (an empty slot is all zero,
    ce_device.h lookup_slot1); the nil UUID is the one actor whose key looks empty, so with it in
    the table (or looked up) the two-load probe is used.  Stress Dots over a pool that holds the
    nil UUID as a writer, as a Dot actor only (a table miss, inserted and refolded), or not at
    all -- state == oracle in each case."""
    key = os.urandom(32)
    rng = random.Random({"writer": 1, "dot_only": 2, "absent": 3}[nil_where])
    writers = sorted(rng.randbytes(16) for _ in range(12))
    if nil_where == "writer":
        writers[0] = bytes(16)
    pool = writers + ([bytes(16)] if nil_where == "dot_only" else [])
    clears, fa, vers = [], [], []
    for a in range(len(writers)):
        for v in range(6):
            dots = [{"actor": rng.choice(pool), "counter": rng.getrandbits(rng.choice([7, 16, 32, 64]))}
                    for _ in range(60)]
            clears.append(APP + msgpack.packb(dots, use_bin_type=True))
            fa.append(a)
            vers.append(v)
    files = [CORE + e for e in ctx.encrypt_batch(key, clears)]
    core = crdtenc.Core(ctx, kind=crdtenc.STATE_GCOUNTER, supported=[APP], current_data_version=APP)
    core.set_latest_key(key)
    rc, st = core.ingest_ops(files, writers, fa, vers)
    oc = oracle.Core()
    orc, ost = oc.read_remote_ops(key, [APP], files, [writers[i] for i in fa], vers)
    assert (rc, list(st)) == (orc, list(ost)) and rc == 0
    assert core.state_bytes() == oc.serialize()
    core.close()


@pytest.mark.parametrize("kind", [crdtenc.STATE_GCOUNTER, crdtenc.STATE_ORSWOT])
def test_table_growth_inside_one_call(ctx, oracle, kind):
    """More new writers in one ingest (and more actors in one merged state) than the actor table
    holds before it grows: slots handed out before a growth move with it (refresh_slots), so the
    version gate and the merged clock still land on the right actors."""
    key = os.urandom(32)
    if kind == crdtenc.STATE_GCOUNTER:
        files, actors, fa, vers = make_ops_batch(ctx, key, 5000, 1, 3, seed=77)
        core = crdtenc.Core(ctx, kind=kind, supported=[APP], current_data_version=APP)
        core.set_latest_key(key)
        rc, st = core.ingest_ops(files, actors, fa, vers)
        oc = oracle.Core()
        orc, ost = oc.read_remote_ops(key, [APP], files, [actors[i] for i in fa], vers)
        assert (rc, list(st)) == (orc, list(ost)) and rc == 0
        assert core.state_bytes() == oc.serialize()
        core.close()
        return
    # Orswot: a state whose clock names 5000 actors, merged into a fresh core
    rng = random.Random(5)
    actors = sorted(rng.randbytes(16) for _ in range(5000))
    clock = {a: rng.randrange(1, 1 << 20) for a in actors}
    sw = {"next_op_versions": {"dots": dict(sorted((a, 1) for a in actors[:3000]))},
          "state": {"clock": {"dots": dict(sorted(clock.items()))}, "entries": {}, "deferred": {}}}
    want = msgpack.packb(sw, use_bin_type=True)
    core = crdtenc.Core(ctx, kind=kind, supported=[APP], current_data_version=APP)
    core.set_latest_key(key)
    assert core.merge_state(want) == 0
    from oracle import crdts as C
    oc = C.Core("orswot")
    nov, st = C.dec_state("orswot", want)
    oc.state.merge(st)
    oc.nov.merge(nov)
    assert core.state_bytes() == oc.serialize()
    core.close()


@pytest.mark.parametrize("batch", [False, True])
def test_local_writer_survives_table_growth(ctx, tmp_path, oracle, batch):
    """Core::apply_ops (lib.rs:666-722) whose Dots name more new actors than the table holds
    before it grows (2,048 at 1/4 load of 8,192 slots): the apply rehashes the table, so the local
    actor's next_op_versions slot must be looked up again after it.  Every op file survives at
    its own version (none overwritten), the next call writes the next version, and a fresh replica
    reading the remote dir folds to the oracle's state (next_op_versions included)."""
    rng = random.Random(2049 + batch)
    key = rng.randbytes(32)
    remote = str(tmp_path / "remote")
    core = crdtenc.Core(ctx, kind=crdtenc.STATE_GCOUNTER, supported=[APP], current_data_version=APP,
                        local_path=str(tmp_path / "l0"), remote_path=remote, flags=crdtenc.OPEN_CREATE)
    core.set_latest_key(key)
    me = core.info_actor()
    cap0 = core.dense_capacity()
    n_calls = 0
    for round_ in range(3):
        ops = [msgpack.packb([{"actor": rng.randbytes(16), "counter": rng.getrandbits(30) + 1}
                              for _ in range(1500)] + [{"actor": me, "counter": round_ + 1}], use_bin_type=True)
               for _ in range(2)]
        if batch:
            rc, files = core.apply_ops_batch(ops, nonces=[rng.randbytes(24) for _ in ops])
            assert rc == 0 and len(files) == 2
        else:
            for o in ops:
                assert core.apply_ops(o) == 0
        n_calls += 2
    assert core.dense_capacity() > cap0, "the actor table never grew"
    st = crdtenc.Storage(str(tmp_path / "l1"), remote)
    loaded = st.load_ops([(me, 0)])
    assert [x[1] for x in loaded] == list(range(n_calls))
    oc = oracle.Core()
    assert oc.read_remote_ops(key, [APP], [x[2] for x in loaded], [x[0] for x in loaded],
                              [x[1] for x in loaded])[0] == 0
    assert core.state_bytes() == oc.serialize()
    fresh = crdtenc.Core(ctx, kind=crdtenc.STATE_GCOUNTER, supported=[APP], current_data_version=APP,
                         local_path=str(tmp_path / "l2"), remote_path=remote, flags=crdtenc.OPEN_CREATE)
    fresh.set_latest_key(key)
    assert fresh.read_remote() == 0
    assert fresh.state_bytes() == oc.serialize()
    for c in (core, fresh):
        c.close()


@pytest.mark.parametrize("size", [(1 << 20) + 17, (5 << 20) + 1000, 35_000_000])
def test_many_segment_files_seal_and_open(ctx, oracle, size):
    """Files of more than 64 Poly1305 segments (16 KiB each): k_finalize_multi runs one Horner
    chain per lane over segments j = lane, lane + 64, ... in r^(64 S), the last segment apart.
    Seal == the oracle's (OpenSSL ChaCha20 + a reference Poly1305) byte for byte; open returns the
    plaintext, and a flipped ciphertext bit is rejected with the plaintext scrubbed."""
    rng = random.Random(size)
    key, nonce = rng.randbytes(32), rng.randbytes(24)
    pt = rng.randbytes(size)
    enc = ctx.encrypt(key, pt, nonce=nonce)
    st, want = oracle.cryptor_encrypt(key, nonce, pt)
    assert st == 0 and enc == want
    b = bytearray(enc)
    b[len(b) // 2] ^= 0x10
    rc, sts, pts, raw, offs = ctx.decrypt_batch(key, [enc, bytes(b)])
    assert list(sts) == [0, 9] and pts[0] == pt
    assert raw[offs[1]:offs[1] + size] == bytes(size)


def test_clock_probe(ctx):
    """ce_ctx_clock_probe (diagnostics behind bench.py's roofline.clock): every interval spans
    at least the requested reference ticks and reports a plausible shader clock; bad arguments
    are refused before any launch."""
    import torch
    blocks, samples, ticks = 8, 4, 5000
    out = torch.zeros(blocks * samples * 2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.clock_probe(out.data_ptr(), blocks, samples, ticks)
    ctx.synchronize()
    v = out.view(blocks, samples, 2).cpu().numpy()
    assert (v[:, :, 1] >= ticks).all()
    ghz = v[:, :, 0] / v[:, :, 1] * 0.1
    assert ((ghz > 0.3) & (ghz < 4.0)).all(), ghz
    for bad in ((0, 4, 5000), (4097, 4, 5000), (8, 0, 5000), (8, 4, 0), (8, 1000, 10 ** 6)):
        with pytest.raises(crdtenc.CeError):
            ctx.clock_probe(out.data_ptr(), *bad)


@pytest.mark.gpu
def test_diag_env_cannot_select_wrong_variants():
    """CE_V2_OPT=129 (actor lookups skipped, wrong results on purpose) and CE_V2_WAVES=13 once
    selected diagnostics variants of k_open_fold_v2 in a second build of the library.  That build
    is gone and no code reads either variable any more: __graft_entry__.smoke() run with them
    set still folds to the oracle's state."""
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CE_V2_OPT="129", CE_V2_WAVES="13")
    env.pop("CRDTENC_LIB", None)
    r = subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.smoke()"], cwd=repo,
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "smoke ok" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])
