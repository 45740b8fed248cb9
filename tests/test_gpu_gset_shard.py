"""The sharded GSet ingest on the GPU (ce_core_gset_ingest_ops_device_sharded, ce_core_gset_
pending_members, ce_core_gset_pending_commit, shard.ingest_gset_sharded): every result is compared
bit for bit with tests/gset_model.py folding the whole batch once in (shared writer order,
version) order.  Scenarios and sealing: tests/test_gset_shard.py.  Without the three entry points
every test here fails on the missing symbols."""
import os
import random
import socket
import subprocess
import sys

import msgpack
import numpy as np
import pytest
import torch

import crdtenc
import gset_model as gm
from oracle.crdts import VClock

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
from test_gset_shard import (APP, SCENARIOS, U64, expected, model_fold, owners, pool, rank_pre,  # noqa: E402
                             scenario, seal)

GS = crdtenc.STATE_GSET
DEV = "cuda:0"
WORLD = 3


@pytest.fixture(scope="module")
def ctx():
    c = crdtenc.Context(0)
    yield c
    c.close()


def new_core(ctx, key, kind=GS):
    c = crdtenc.Core(ctx, kind=kind, supported=[APP], current_data_version=APP)
    c.set_latest_key(key)
    return c


def to_share(files, fa, fv, sel):
    """one rank's files resident in HBM"""
    blob = b"".join(files[i] for i in sel)
    offs = np.zeros(len(sel) + 1, np.int64)
    offs[1:] = np.cumsum([len(files[i]) for i in sel])
    d = dict(files=torch.frombuffer(bytearray(blob + bytes(64)), dtype=torch.uint8).to(DEV),
             offs=torch.from_numpy(offs).to(DEV), n=len(sel), blob_len=len(blob),
             fa=torch.tensor([fa[i] for i in sel], dtype=torch.int32, device=DEV),
             fv=torch.tensor([fv[i] for i in sel], dtype=torch.int64, device=DEV), sel=list(sel))
    torch.cuda.synchronize()
    return d


def members_of(key, f):
    one = gm.Core()
    assert one.read_remote_ops(key, [APP], [f], [bytes(16)], [0])[0] == 0
    return set(one.state.value)


def stats_windows(cores, shares, W, m):
    """stats -> numpy max (the all_reduce) -> every core's windows"""
    world = len(cores)
    stats = []
    for r, (core, d) in enumerate(zip(cores, shares)):
        st = torch.empty(2 * m + 3, dtype=torch.int64, device=DEV)
        core.shard_stats(W, d["fa"].data_ptr(), d["fv"].data_ptr(), d["n"], r, world, st.data_ptr())
        stats.append(st.cpu().numpy())
    red = torch.from_numpy(np.maximum.reduce(stats)).to(DEV)
    torch.cuda.synchronize()
    his = []
    for core in cores:
        hi = torch.empty(m + 1, dtype=torch.int64, device=DEV)
        core.shard_window(W, red.data_ptr(), hi.data_ptr())
        his.append(hi)
    return his


def exact_windows(cores, fa_all, fv_all, W):
    """the reference loop over everyone's metadata (the fallback of a broken partition contract)"""
    e0 = cores[0].writer_versions(W)
    hi, flags = crdtenc.shard_window_exact(e0, fa_all, fv_all)
    h = torch.from_numpy(np.append(np.asarray(hi, np.uint64), np.uint64(flags)).view(np.int64).copy()).to(DEV)
    torch.cuda.synchronize()
    return [h for _ in cores]


def ingest(core, d, W, hi):
    return core.gset_ingest_ops_device_sharded(d["files"].data_ptr(), d["offs"].data_ptr(), d["n"], d["blob_len"],
                                               W, d["fa"].data_ptr(), d["fv"].data_ptr(), hi.data_ptr())


def export(core):
    """(column tensor, n) through the size query and an exact buffer"""
    rc, n = core.gset_pending_members(None, 0)
    assert rc == (64 if n else 0), (rc, n)
    buf = torch.zeros(max(n, 1), dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    if n:
        assert core.gset_pending_members(buf.data_ptr(), n) == (0, n)
    return buf, n


def exchange_commit(cores, rcs):
    """numpy-free 'all-gather': every core commits the other cores' columns.  A failed rank: the
    healthy ones drop their batch.  Returns the pending counts (None when rejected)."""
    if any(rc not in (0, 13) for rc in rcs):
        for core, rc in zip(cores, rcs):
            if rc in (0, 13):
                assert core.gset_pending_commit(False) == 0
            assert core.gset_pending_members(None, 0) == (64, 0)   # nothing pending on any rank now
        return None
    cols = [export(core) for core in cores]
    for r, core in enumerate(cores):
        others = [q for q in range(len(cores)) if q != r]
        assert core.gset_pending_commit(True, [cols[q][0].data_ptr() if cols[q][1] else None for q in others],
                                        [cols[q][1] for q in others]) == 0
    return [n for _, n in cols]


def want_pending(key, files, fa, fv, sel, e0, hi, have):
    """the members a rank's gated files add to the committed set `have`"""
    new = set()
    for i in sel:
        if e0[fa[i]] <= fv[i] < hi[fa[i]]:
            new |= members_of(key, files[i])
    return new - have


def run_shares(ctx, key, writers, files, fa, fv, pre, own, name="", before=None):
    """Three cores on one GPU play three ranks: start state, stats -> max -> windows -> sharded
    ingest (pending) -> columns -> commit.  Returns (rcs, counts, cores, starts)."""
    W, m = b"".join(writers), len(writers)
    cores, shares, starts = [], [], []
    for r in range(WORLD):
        core = new_core(ctx, key)
        p = rank_pre(name, pre, r)
        first = [i for i in range(len(files)) if fv[i] < p[fa[i]]]
        if first:
            rc, _ = core.ingest_ops([files[i] for i in first], writers, [fa[i] for i in first], [fv[i] for i in first])
            assert rc == 0
        if before:
            before(core)
        cores.append(core)
        starts.append(core.state_bytes())
        shares.append(to_share(files, fa, fv, [i for i in range(len(files)) if own[i] == r]))
    his = stats_windows(cores, shares, W, m)
    rcs = [ingest(c, d, W, h) for c, d, h in zip(cores, shares, his)]
    if name == "contract":
        # the reduced stats flag the broken contract on every rank: nothing folded, nothing pending
        assert rcs == [69] * WORLD
        for c, s in zip(cores, starts):
            assert c.gset_pending_members(None, 0) == (64, 0) and c.state_bytes() == s
        his = exact_windows(cores, fa, fv, W)
        rcs = [ingest(c, d, W, h) for c, d, h in zip(cores, shares, his)]
    return rcs, cores, shares, starts


def check_counts(counts, cores_e0, key, writers, files, fa, fv, shares, have):
    hi, _ = crdtenc.shard_window_exact(cores_e0, fa, fv)
    for r, d in enumerate(shares):
        assert counts[r] == len(want_pending(key, files, fa, fv, d["sel"], cores_e0, hi, have)), r


@pytest.mark.parametrize("name,want_rc,_path", SCENARIOS)
def test_three_shares_one_process(ctx, name, want_rc, _path):
    key, writers, files, fa, fv, pre = scenario(name)
    own = owners(name, writers, fa, fv, WORLD)
    rcs, cores, shares, starts = run_shares(ctx, key, writers, files, fa, fv, pre, own, name)
    orc, want = expected(name, key, writers, files, fa, fv, pre)
    assert orc == want_rc
    if name == "e0_mismatch":       # refused on every rank, nothing folded, nothing pending
        assert rcs == [69] * WORLD
        assert len(set(starts)) == 2
        for c, s in zip(cores, starts):
            assert c.gset_pending_members(None, 0) == (64, 0) and c.state_bytes() == s
    elif want_rc in (9, 12):        # one rank holds the bad file: every state bit-identical to its start
        assert sorted(rcs) == [0, 0, want_rc]
        assert exchange_commit(cores, rcs) is None
        for c, s in zip(cores, starts):
            assert c.state_bytes() == s == want
    else:
        assert rcs == [want_rc] * WORLD
        e0 = np.array([pre[a] for a in range(len(writers))], np.uint64)
        assert list(cores[0].writer_versions(b"".join(writers))) == list(e0)
        have = set(gm.dec_state(starts[0])[1].value)
        counts = exchange_commit(cores, rcs)
        check_counts(counts, e0, key, writers, files, fa, fv, shares, have)   # old versions: nothing pending from them
        for c in cores:
            assert c.state_bytes() == want
    for c in cores:
        c.close()


def _find_writers(rng, m, versions, ok):
    """writers whose files' owners (world 3) satisfy ok(own, fa, fv)"""
    fa = [a for a in range(m) for _ in range(versions)]
    fv = [v for _ in range(m) for v in range(versions)]
    for _ in range(20000):
        writers = sorted(rng.randbytes(16) for _ in range(m))
        own = crdtenc.shard_owners(writers, fa, fv, WORLD)
        if ok(own, fa, fv):
            return writers, fa, fv, own
    raise AssertionError("no writer set with that ownership")


def _exotic(f):
    """the same box with nonce / enc_data as sequences of u8 (serde_bytes takes them): the device
    leaves such an envelope to the host parser"""
    ver, inner = msgpack.unpackb(f[16:])
    eb = msgpack.unpackb(inner)
    inner = msgpack.packb({"nonce": list(eb["nonce"]), "enc_data": list(eb["enc_data"])}, use_bin_type=True)
    return f[:16] + msgpack.packb([ver, inner], use_bin_type=True)


EDGE_CASES = ["zero_remote", "same_on_all", "already_committed", "empty_share", "below_window", "multi_page",
              "host_parse"]


@pytest.mark.parametrize("case", EDGE_CASES)
def test_member_edge_cases(ctx, case):
    rng = random.Random(40 + EDGE_CASES.index(case))
    key = rng.randbytes(32)
    ids = [x for x in pool(rng) if x]      # (0 is placed by the cases that want it)
    m, versions = 2, 6
    pre = {0: 0, 1: 0}
    ok = lambda own, fa, fv: len(set(own)) == WORLD   # noqa: E731
    if case == "empty_share":
        versions = 3
        ok = lambda own, fa, fv: set(own) == {0, 1}   # noqa: E731
    elif case == "below_window":
        pre = {0: 2, 1: 2}
        ok = lambda own, fa, fv: 2 in set(own) and all(v < 2 for o, v in zip(own, fv) if o == 2)   # noqa: E731
    writers, fa, fv, own = _find_writers(rng, m, versions, ok)
    bodies = [[rng.choice(ids) for _ in range(rng.randint(0, 20))] for _ in fa]
    remote = [i for i in range(len(fa)) if own[i] == 1]
    if case == "zero_remote":
        bodies[remote[0]].append(0)
    elif case == "same_on_all":
        for i in range(len(fa)):
            bodies[i] += [0, U64, 0x1234567890ab]
    elif case == "multi_page":
        bodies[remote[0]] = [rng.getrandbits(64) | (1 << 40) for _ in range(570)]
    files = [seal(key, APP + gm.enc_ops(b), rng) for b in bodies]
    if case == "multi_page":
        assert len(files[remote[0]]) > 4096 + 100
    if case == "host_parse":
        files[remote[-1]] = _exotic(files[remote[-1]])
    orc, model = model_fold(key, writers, files, fa, fv, pre)
    assert orc == 0
    everything = gm.serialize(VClock(), gm.GSet(set().union(*map(set, bodies))))
    before = None
    if case == "already_committed":
        def before(core):
            assert core.merge_state(everything) == 0
        model.merge_state(everything)
    rcs, cores, shares, starts = run_shares(ctx, key, writers, files, fa, fv, pre, own, before=before)
    assert rcs == [0] * WORLD
    if case == "empty_share":
        assert shares[2]["n"] == 0
    if case == "multi_page":
        assert cores[1].path_count("gset_fused_files") == shares[1]["n"] - 1    # that file: k_decode_gset
    have = set(gm.dec_state(starts[0])[1].value)
    counts = exchange_commit(cores, rcs)
    e0 = np.array([pre[a] for a in range(m)], np.uint64)
    check_counts(counts, e0, key, writers, files, fa, fv, shares, have)
    if case == "already_committed":
        assert counts == [0] * WORLD and have == model.state.value
    if case in ("empty_share", "below_window"):
        assert counts[2] == 0
    for c in cores:
        assert c.state_bytes() == model.serialize()
        c.close()


def test_growth(ctx, monkeypatch):
    """16-slot tables: the batch table grows inside the sharded ingest, the committed table inside
    the commit, to the bound count + local pending + the remote columns' lengths."""
    rng = random.Random(50)
    key = rng.randbytes(32)
    writers = sorted(rng.randbytes(16) for _ in range(3))
    fa = [a for a in range(3) for _ in range(6)]
    fv = [v for _ in range(3) for v in range(6)]
    files = [seal(key, APP + gm.enc_ops([rng.getrandbits(64) | (1 << 33) for _ in range(12)]), rng) for _ in fa]
    own = owners("", writers, fa, fv, WORLD)
    assert min(np.bincount(own, minlength=WORLD)) >= 2     # >= 24 distinct members on every rank
    monkeypatch.setenv("CE_GSET_CAP", "16")
    rcs, cores, shares, starts = run_shares(ctx, key, writers, files, fa, fv, {a: 0 for a in range(3)}, own)
    monkeypatch.delenv("CE_GSET_CAP")
    assert rcs == [0] * WORLD
    for c in cores:
        assert c.path_count("gset_batch_grows") + c.path_count("gset_refolds") > 0 and c.path_count("gset_grows") == 0
    counts = exchange_commit(cores, rcs)
    assert min(counts) >= 20 and sum(counts) - max(counts) >= 40
    _, model = model_fold(key, writers, files, fa, fv, {a: 0 for a in range(3)})
    for c in cores:
        assert c.path_count("gset_grows") > 0
        assert c.state_bytes() == model.serialize()
        c.close()


def test_pending_semantics(ctx):
    rng = random.Random(51)
    key = rng.randbytes(32)
    writers = sorted(rng.randbytes(16) for _ in range(2))
    W = b"".join(writers)
    ids = pool(rng)
    fa, fv = [0, 0, 0, 1, 1], [0, 1, 2, 0, 1]
    bodies = [[rng.choice(ids) for _ in range(10)] + [0] for _ in fa]
    files = [seal(key, APP + gm.enc_ops(b), rng) for b in bodies]
    core, model = new_core(ctx, key), gm.Core()
    known = [ids[5], ids[20], 77]
    assert core.apply_ops(gm.enc_ops(known)) == 0
    model.apply_ops(core.info_actor(), known)
    nonce = bytes(range(24))
    before, before_file = core.state_bytes(), core.compact_to_buffer(nonce=nonce)
    assert before == model.serialize()
    d = to_share(files, fa, fv, range(5))
    # nothing pending yet: export and commit refuse
    assert core.gset_pending_members(None, 0) == (64, 0) and core.gset_pending_commit(True) == 64

    def ingest_all(share=d):
        (hi,) = stats_windows([core], [share], W, 2)
        return ingest(core, share, W, hi)
    assert ingest_all() == 0
    # while pending: the committed set only
    assert core.state_bytes() == before and core.compact_to_buffer(nonce=nonce) == before_file
    new = sorted(set().union(*map(set, bodies)) - set(known))
    rc, n = core.gset_pending_members(None, 0)
    assert (rc, n) == (64, len(new))
    short = torch.full((n + 3,), -2, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    assert core.gset_pending_members(short.data_ptr(), n - 1) == (64, n)
    assert bool((short == -2).all())
    assert core.gset_pending_members(short.data_ptr(), n) == (0, n)
    got = short.cpu().numpy()
    assert sorted(int(x) for x in got[:n].view(np.uint64)) == new and (got[n:] == -2).all()
    # argument errors leave the batch pending
    one = torch.tensor([5], dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    assert core.gset_pending_commit(True, [one.data_ptr()] * 65, [1] * 65) == 64
    assert core.gset_pending_commit(True, [one.data_ptr(), None], [1, 1]) == 64
    assert core.gset_pending_members(None, 0) == (64, n)
    gc = new_core(ctx, key, kind=crdtenc.STATE_GCOUNTER)
    (hi,) = stats_windows([core], [d], W, 2)
    assert ingest(gc, d, W, hi) == 64 and gc.gset_pending_members(None, 0) == (64, 0)
    assert gc.gset_pending_commit(True) == 64 and gc.gset_pending_commit(False) == 64
    gc.close()
    # dropped, then folded again and committed
    assert core.gset_pending_commit(False) == 0
    assert core.state_bytes() == before and core.gset_pending_members(None, 0) == (64, 0)
    assert ingest_all() == 0
    # a second ingest drops the first pending batch: the share of writer 1 alone
    d1 = to_share(files, fa, fv, [3, 4])
    assert ingest_all(d1) == 0
    only1 = set(bodies[3]) | set(bodies[4])
    assert core.gset_pending_members(None, 0)[1] == len(only1 - set(known))
    assert ingest_all() == 0
    # apply_ops while pending goes to the committed set and survives the commit
    local = [new[0], 0xfeedfacecafe]
    assert core.apply_ops(gm.enc_ops(local)) == 0
    model.apply_ops(core.info_actor(), local)
    assert core.state_bytes() == model.serialize()
    assert core.gset_pending_members(None, 0) == (64, n)
    assert core.gset_pending_commit(True) == 0
    assert model.read_remote_ops(key, [APP], files, [writers[a] for a in fa], fv)[0] == 0
    assert core.state_bytes() == model.serialize()
    assert core.gset_pending_commit(True) == 64     # committed: nothing pending
    # a reset drops a pending batch
    core.reset()
    assert ingest_all() == 0
    core.reset()
    assert core.gset_pending_members(None, 0) == (64, 0) and core.state_bytes() == gm.Core().serialize()
    core.close()


def test_commit_of_64_parts(ctx):
    """k_gs_insert_parts through a direct commit: 64 columns of 0, 1, 63, 64, 65 and 4097 members,
    duplicates within and across them, an empty part between two full ones, the member 0 and
    2^64 - 1 inside; == the model's union."""
    rng = random.Random(52)
    key = rng.randbytes(32)
    core, model = new_core(ctx, key), gm.Core()
    lens = [4097, 0, 4097, 65, 64, 63, 1, 0] + [rng.choice([0, 1, 63, 64, 65, 4097]) for _ in range(56)]
    assert len(lens) == 64
    universe = [0, U64] + [rng.getrandbits(rng.choice([7, 16, 32, 64])) for _ in range(20000)]
    cols = [[rng.choice(universe) for _ in range(k)] for k in lens]
    cols[2][:100] = cols[0][:100]           # across parts
    cols[0][200:300] = cols[0][:100]        # within a part
    cols[6] = [0]
    tens = [torch.from_numpy(np.array(c, np.uint64).view(np.int64).copy()).to(DEV) if c else None for c in cols]
    torch.cuda.synchronize()
    W = rng.randbytes(16)
    hi = torch.zeros(2, dtype=torch.int64, device=DEV)      # one writer, an empty window, no flags
    empty = to_share([], [], [], [])
    assert ingest(core, empty, W, hi) == 0
    assert core.gset_pending_members(None, 0) == (0, 0)
    assert core.gset_pending_commit(True, [t.data_ptr() if t is not None else None for t in tens], lens) == 0
    for c in cols:
        for x in c:
            model.state.apply(x)
    assert core.state_bytes() == model.serialize()
    core.close()


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_ranks(tmp_path, world, name, backend):
    out = str(tmp_path / "g")
    port = str(_port())
    env = dict(os.environ, CE_TEST_BACKEND=backend)
    procs = [subprocess.Popen([sys.executable, os.path.join(REPO, "tests", "gset_rank_worker.py"),
                               str(r), str(world), port, name, out], env=env) for r in range(world)]
    rcs = []
    try:
        for p in procs:
            rcs.append(p.wait(timeout=180))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert rcs == [0] * world       # a failed or signalled child fails the test here
    res = []
    for r in range(world):
        with open("%s.%d" % (out, r), "rb") as f:
            res.append(msgpack.unpackb(f.read(), raw=False))
    return res


@pytest.mark.parametrize("name,want_rc,want_path", [s for s in SCENARIOS if s[0] in ("clean", "gap", "tamper")])
def test_two_process_sharded_ingest(tmp_path, name, want_rc, want_path):
    """shard.ingest_gset_sharded itself, two processes under gloo over one shared GPU."""
    key, writers, files, fa, fv, pre = scenario(name)
    orc, want = expected(name, key, writers, files, fa, fv, pre)
    assert orc == want_rc
    for r, (rc, path, n, state, start) in enumerate(_run_ranks(tmp_path, 2, name, "gloo")):
        assert (rc, path) == (want_rc, want_path), r
        assert 0 < n < len(files)
        assert state == want, r
        if want_rc == 9:
            assert state == start


def test_one_rank_rccl_sharded_ingest(tmp_path):
    """World 1 under RCCL: the collectives of shard.ingest_gset_sharded on device tensors."""
    key, writers, files, fa, fv, pre = scenario("clean")
    orc, want = expected("clean", key, writers, files, fa, fv, pre)
    ((rc, path, n, state, _start),) = _run_ranks(tmp_path, 1, "clean", "nccl")
    assert (rc, path, n) == (0, "members", len(files)) and state == want
