"""The sharded LWWReg ingest on the GPU (ce_core_lwwreg_ingest_ops_device_sharded, ce_core_lwwreg_
pending_record, ce_core_lwwreg_pending_commit, shard.ingest_lwwreg_sharded) and its reduce
(ce_ctx_prim_lww_reduce_keyed): every result is compared bit for bit with tests/lwwreg_model.py
folding the whole batch once in (shared writer order, version) order, or with numpy.  Scenarios and
sealing: tests/test_lwwreg_shard.py.  Without the entry points every test here fails on the
missing symbols."""
import ctypes
import json
import os
import random
import subprocess
import sys

import pytest
import torch

import crdtenc
import lwwreg_model as lm
from oracle.crdts import VClock

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
from test_gset_shard import APP, owners, seal  # noqa: E402
from test_pn_shard import expected, model_fold  # noqa: E402
from test_lwwreg_shard import LWW_SYMBOLS, SCENARIOS, U64, scenario  # noqa: E402
from test_gpu_gset_shard import DEV, WORLD, _find_writers, stats_windows, to_share  # noqa: E402
import kind_shard_gpu as K  # noqa: E402
import lww_keyed_worker as KW  # noqa: E402
import shard  # noqa: E402

LW = crdtenc.STATE_LWWREG
NONE = shard.LWW_NONE
BIG = U64 - 5      # the tie cases' largest marker


def test_symbols_present():
    for name in LWW_SYMBOLS:
        assert hasattr(crdtenc.lib(), name), name


@pytest.fixture(scope="module")
def ctx():
    c = crdtenc.Context(0)
    yield c
    c.close()


def none_pending(core):
    rec = (ctypes.c_uint64 * 4)(71, 72, 73, 74)
    assert crdtenc.lib().ce_core_lwwreg_pending_record(core.p, rec) == 64 and list(rec) == [71, 72, 73, 74]
    assert core.lwwreg_pending_record() == (64, None)
    assert core.lwwreg_pending_commit(True) == 64 and core.lwwreg_pending_commit(False) == 64


KIND = K.Kind(LW, lm, "lwwreg_ingest_ops_device_sharded", none_pending)


def exchange_commit(cores, rcs):
    """The all-gather in-process: every core commits with the other cores' records.  A failed
    rank: the healthy ones drop their batch.  Returns the records (None when rejected)."""
    if any(rc not in (0, 13) for rc in rcs):
        for core, rc in zip(cores, rcs):
            if rc in (0, 13):
                assert core.lwwreg_pending_commit(False) == 0
            none_pending(core)
        return None
    recs = []
    for core in cores:
        rc, rec = core.lwwreg_pending_record()
        assert rc == 0
        recs.append(rec)
    for r, core in enumerate(cores):
        assert core.lwwreg_pending_commit(True, [recs[q] for q in range(len(cores)) if q != r]) == 0
        none_pending(core)
    return recs


def want_records(key, files, fa, fv, shares, e0, hi):
    """each share's winner by the rule itself: over its gated files' own winners"""
    out = []
    for d in shares:
        mine = []
        for i in d["sel"]:
            if e0[fa[i]] <= fv[i] < hi[fa[i]]:
                one = lm.Core()
                assert one.read_remote_ops(key, [APP], [files[i]], [bytes(16)], [0])[0] == 0
                val, marker = one.state.read()
                mine.append((marker, val, fa[i], fv[i]))
        out.append(shard.lww_pick(mine))
    return out


@pytest.mark.parametrize("name,want_rc,_path", SCENARIOS)
def test_three_shares_one_process(ctx, name, want_rc, _path):
    key, writers, files, fa, fv, pre = scenario(name)
    own = owners(name, writers, fa, fv, WORLD)
    rcs, cores, shares, starts = K.run_shares(ctx, KIND, key, writers, files, fa, fv, pre, own, name)
    orc, want = expected(lm, name, key, writers, files, fa, fv, pre)
    assert orc == want_rc
    if name == "e0_mismatch":       # refused on every rank, nothing opened, nothing pending
        assert rcs == [69] * WORLD and len(set(starts)) == 2
        for c, s in zip(cores, starts):
            none_pending(c)
            assert c.state_bytes() == s
    elif want_rc in (9, 12):        # one rank holds the bad file: every state bit-identical to its start
        assert sorted(rcs) == [0, 0, want_rc]
        assert exchange_commit(cores, rcs) is None
        for c, s in zip(cores, starts):
            assert c.state_bytes() == s == want
    else:
        assert rcs == [want_rc] * WORLD
        e0 = [pre[a] for a in range(len(writers))]
        hi, _ = crdtenc.shard_window_exact(e0, fa, fv)
        recs = exchange_commit(cores, rcs)
        assert recs == want_records(key, files, fa, fv, shares, e0, [int(x) for x in hi])
        for c in cores:
            assert c.state_bytes() == want
    for c in cores:
        c.close()


# ---- ties: the files are chosen after the owners are known, so each case really spans ranks ----
TIE_CASES = ["earlier_on_higher_rank", "inside_one_file", "with_the_register", "only_in_skipped_files",
             "only_marker_zero", "rank_without_a_file", "descending_writer_runs"]


def _noise(rng, k):
    return [(rng.getrandbits(40), rng.randrange(1, 1 << 30)) for _ in range(k)]


@pytest.mark.parametrize("case", TIE_CASES)
def test_ties(ctx, case):
    rng = random.Random(70 + TIE_CASES.index(case))
    key = rng.randbytes(32)
    m, versions = 3, 6
    ok = lambda own, fa, fv: len(set(own)) == WORLD   # noqa: E731
    if case == "rank_without_a_file":
        m, versions = 2, 3
        ok = lambda own, fa, fv: set(own) == {0, 1}   # noqa: E731
    writers, fa, fv, own = _find_writers(rng, m, versions, ok)
    n = len(fa)
    bodies = [_noise(rng, rng.randint(0, 6)) for _ in range(n)]
    start = lm.serialize(VClock(), lm.LWWReg())     # merged into every rank (and the model) before the ingest
    order, want_rc = None, 0
    if case in ("earlier_on_higher_rank", "rank_without_a_file"):
        i, j = next((i, j) for i in range(n) for j in range(i + 1, n) if own[i] > own[j])
        bodies[i].append((111, BIG))
        bodies[j].insert(0, (222, BIG))
    elif case == "inside_one_file":
        i = next(i for i in range(n) if own[i] == 2)
        bodies[i] = _noise(rng, 3) + [(111, BIG)] + _noise(rng, 2) + [(222, BIG)]
    elif case == "with_the_register":
        start = lm.serialize(VClock(), lm.LWWReg(999, BIG))
        for i in (next(i for i in range(n) if own[i] == r) for r in range(WORLD)):
            bodies[i].append((100 + i, BIG))
    elif case == "only_in_skipped_files":
        # writer 0 starts at version 2 (its versions 0 and 1 are old); writer 1 lacks version 3
        start = lm.serialize(VClock({writers[0]: 2}), lm.LWWReg())
        bodies[fa.index(0) + 1].append((111, BIG))                  # (writer 0, version 1): old
        bodies[fa.index(1) + 5].append((222, BIG))                  # (writer 1, version 5): beyond the gap
        bodies[fa.index(2) + 0].append((333, BIG))                  # writer 2: after the gap's writer, never folded
        bodies[fa.index(0) + 4].append((444, BIG - 1))              # the winner
        bodies[fa.index(1) + 1].append((555, BIG - 1))
        want_rc = 13
    elif case == "only_marker_zero":
        bodies = [[(rng.getrandbits(40), 0) for _ in range(rng.randint(0, 5))] for _ in range(n)]
    elif case == "descending_writer_runs":
        # the largest marker in two files of one rank, of different writers: in a share laid out by
        # descending writer the later file of the batch comes first
        i, j = next((i, j) for i in range(n) for j in range(i + 1, n) if own[i] == own[j] and fa[i] < fa[j])
        bodies[i].append((111, BIG))
        bodies[j].append((222, BIG))
        order = lambda sel: sorted(sel, key=lambda x: (-fa[x], fv[x]))   # noqa: E731
    keep = [x for x in range(n) if not (case == "only_in_skipped_files" and (fa[x], fv[x]) == (1, 3))]
    files = [seal(key, APP + lm.enc_ops(bodies[x]), rng) for x in keep]
    fa, fv, own = [fa[x] for x in keep], [fv[x] for x in keep], [own[x] for x in keep]
    pre = {a: 0 for a in range(m)}
    model = lm.Core()
    model.merge_state(start)
    assert model.read_remote_ops(key, [APP], files, [writers[a] for a in fa], fv)[0] == want_rc

    def before(core):
        assert core.merge_state(start) == 0
    results = []
    for lay in ([None, order] if order else [None]):
        rcs, cores, shares, starts = K.run_shares(ctx, KIND, key, writers, files, fa, fv, pre, own, before=before,
                                                  order=lay)
        assert rcs == [want_rc] * WORLD
        if case == "rank_without_a_file":
            assert shares[2]["n"] == 0 and cores[2].lwwreg_pending_record() == (0, NONE)
        if case == "descending_writer_runs" and lay:
            assert any(d["sel"] != sorted(d["sel"]) for d in shares)
        recs = exchange_commit(cores, rcs)
        for c in cores:
            assert c.state_bytes() == model.serialize() and c.lwwreg_read() == model.state.read()
            c.close()
        results.append(recs)
    if case == "descending_writer_runs":
        assert results[0] == results[1]
    if case in ("earlier_on_higher_rank", "inside_one_file", "descending_writer_runs", "rank_without_a_file"):
        assert model.state.read() == (111, BIG)
    elif case == "with_the_register":
        assert model.state.read() == (999, BIG)         # the incumbent stays
    elif case == "only_in_skipped_files":
        assert model.state.read() == (444, BIG - 1)
    elif case == "only_marker_zero":
        assert model.state.read() == (0, 0) and results[0] == [NONE] * WORLD


def test_pending_semantics(ctx):
    rng = random.Random(80)
    key = rng.randbytes(32)
    writers = sorted(rng.randbytes(16) for _ in range(2))
    W = b"".join(writers)
    fa, fv = [0, 0, 0, 1, 1], [0, 1, 2, 0, 1]
    bodies = [_noise(rng, 4) for _ in fa]
    bodies[3].append((777, BIG))
    files = [seal(key, APP + lm.enc_ops(b), rng) for b in bodies]
    core, model = K.new_core(ctx, key, LW, writers), lm.Core()
    known = lm.serialize(VClock(), lm.LWWReg(5, 1 << 31))
    assert core.merge_state(known) == 0
    model.merge_state(known)
    nonce = bytes(range(24))
    before, before_file = core.state_bytes(), core.compact_to_buffer(nonce=nonce)
    assert before == model.serialize() and core.lwwreg_read() == (5, 1 << 31)
    none_pending(core)
    d = to_share(files, fa, fv, range(5))

    def ingest_all(share=d):
        (hi,) = stats_windows([core], [share], W, 2)
        return K.ingest(KIND, core, share, W, hi)[0]
    assert ingest_all() == 0
    # while pending: the committed register only
    assert core.state_bytes() == before and core.compact_to_buffer(nonce=nonce) == before_file
    assert core.lwwreg_read() == (5, 1 << 31)
    assert core.lwwreg_pending_record() == (0, (BIG, 777, 1, 0))
    # argument errors leave the batch pending
    assert core.lwwreg_pending_commit(True, [NONE] * 65) == 64
    assert crdtenc.lib().ce_core_lwwreg_pending_commit(core.p, 1, None, ctypes.c_uint32(1)) == 64
    assert core.lwwreg_pending_record() == (0, (BIG, 777, 1, 0))
    # dropped, then folded again
    assert core.lwwreg_pending_commit(False) == 0
    assert core.state_bytes() == before
    none_pending(core)
    assert ingest_all() == 0
    # merge_state while pending goes to the committed register and survives the commit; a remote
    # record with the same marker and an earlier address beats the local winner
    more = lm.serialize(VClock(), lm.LWWReg(6, 1 << 33))
    assert core.merge_state(more) == 0
    model.merge_state(more)
    assert core.state_bytes() == model.serialize()
    assert core.lwwreg_pending_commit(True, [(BIG, 888, 0, 7), (BIG, 999, 1, 1), NONE, (BIG - 1, 1, 0, 0)]) == 0
    assert model.read_remote_ops(key, [APP], files, [writers[a] for a in fa], fv)[0] == 0
    model.state.val = 888           # (writer 0, version 7) comes before (writer 1, version 0)
    assert core.state_bytes() == model.serialize() and core.lwwreg_read() == (888, BIG)
    none_pending(core)
    # a plain ingest drops a pending batch: only its own file is folded
    core.reset()
    assert ingest_all() == 0
    rc, _ = core.ingest_ops(files[:1], writers, fa[:1], fv[:1])
    assert rc == 0
    none_pending(core)
    _, one = model_fold(lm, key, writers, files[:1], fa[:1], fv[:1], {0: 0, 1: 0})
    assert core.state_bytes() == one.serialize()
    # a reset drops a pending batch
    assert ingest_all() == 0
    core.reset()
    none_pending(core)
    assert core.state_bytes() == lm.Core().serialize()
    core.close()


# ---- the keyed reduce against numpy ----
def test_reduce_constants(ctx):
    rng = random.Random(81)
    core = K.new_core(ctx, rng.randbytes(32), LW)
    assert (core.path_count("lww_reduce_tile"), core.path_count("lww_reduce_max_blocks")) == (KW.TILE, KW.MAX_BLOCKS)
    core.close()
    assert ctx.prim_lww_reduce_keyed(0, 0, 0, 0) == NONE


@pytest.mark.parametrize("cap", [None, 1])
@pytest.mark.parametrize("n", KW.SIZES)
def test_keyed_reduce_against_numpy(ctx, monkeypatch, n, cap):
    if cap:
        monkeypatch.setenv("CE_TEST_GRID_CAP", str(cap))
    else:
        monkeypatch.delenv("CE_TEST_GRID_CAP", raising=False)
    for v in KW.run_size(ctx, n):
        assert v["ok"], v


def test_keyed_reduce_under_grid_cap_3():
    """every size and case again in a process of its own with CE_TEST_GRID_CAP=3: blocks that take
    several tiles each, and a final stage over three partials"""
    env = dict(os.environ, CE_TEST_GRID_CAP="3")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "lww_keyed_worker.py")], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    verdicts = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert len(verdicts) == sum(len(KW.cases(n)) for n in KW.SIZES)
    for v in verdicts:
        assert v["ok"], v


def test_one_rank_rccl_sharded_ingest(tmp_path):
    """World 1 under RCCL: the collective of shard.ingest_lwwreg_sharded on device tensors."""
    key, writers, files, fa, fv, pre = scenario("clean")
    orc, want = expected(lm, "clean", key, writers, files, fa, fv, pre)
    ((rc, path, n, state, _start),) = K.rank_worker_results(tmp_path, REPO, "lww", 1, "clean", "nccl")
    assert (rc, path, n) == (0, "record", len(files)) and state == want
