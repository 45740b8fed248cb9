"""The device primitives under every Orswot / MVReg fold, the Orswot serializer and the GSet state
writer, called directly (ce_ctx_prim_*: the product's own functions over 0xFF-filled scratch) and
held to plain numpy references (tests/prim_model.py), exactly, item for item:

  ds_excl_sum_u32      ce_scan.hip      exclusive u32 sum, 2048-item tiles
  ds_excl_max_by_key   ce_scan.hip      exclusive u64 max over runs of equal u32 keys
  sort_pairs_u32/u64   ce_ser_sort.hip  stable LSD radix sort, 8-bit digits, 4096-item tiles

The sizes sit on the kernels' edges: a thread's 8 items, a wave's 512, a tile, the 256 tiles one
trip of the one-block carry kernels takes (past them k_seg_apply_direct folds several tile summaries
per lane and k_sum_apply_direct strides twice), the 4096 tiles at which the scans switch from the
two-launch to the three-launch form; for the sort a wave step of 64, a wave's 1024, a tile, the 8
histogram replicas, the look-back window of 16 tiles and twice that.  Every output is 64 items
longer than n and must keep its sentinel there; the inputs must come back unchanged.

CE_SCAN_3PASS and CE_SORT_TICKET are read once per process: test_prims_under_process_switches
runs the cases again under each in a child process (tests/prim_worker.py)."""
import json
import os
import subprocess
import sys

import pytest

import crdtenc
import prim_model as M
import prim_worker as W

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

# a device error or a child that died: no later test of this file starts anything on the GPU
_STOP = []


@pytest.fixture(scope="module")
def ctx():
    c = crdtenc.Context(0)
    yield c
    c.close()


def check(runner, ctx, case, **kw):
    if _STOP:
        pytest.fail("not run: " + _STOP[0])
    try:
        v = runner(ctx, case, **kw)
    except Exception as e:
        _STOP.append("%s raised %r" % (W.case_id(runner, case), e))
        raise
    assert v["ok"], v
    return v


@pytest.mark.parametrize("case", M.SUM_CASES, ids=M.sum_id)
def test_excl_sum_u32(ctx, case):
    """ds_excl_sum_u32 == the u32 cumulative sum (mod 2^32): all ones (the output is iota), all
    zeros, random below 2^16, random full range (the sum wraps), nonzeros only at a tile's last item
    and the next tile's first, and a single nonzero at either."""
    check(W.run_sum, ctx, case)


@pytest.mark.parametrize("case", M.SEG_CASES, ids=M.seg_id)
def test_excl_max_by_key(ctx, case):
    """ds_excl_max_by_key == the running maximum of the earlier values of each run of adjacent equal
    keys, 0 at a run's start.  Keys: one run, every item its own, returning keys (A, B, A), runs of a
    tile and of a thread's 8 items aligned and shifted by one, boundaries at a wave's and a tile's
    edge, a run over many whole tiles then a short one, keys 0 and 0xFFFFFFFF.  Values: decreasing
    (the maximum is the run's first item, tiles back), increasing, zero, 2^64 - 1, one half constant,
    random."""
    check(W.run_seg, ctx, case)


@pytest.mark.parametrize("case", M.SORT_CASES, ids=M.sort_id)
def test_sort_pairs(ctx, case):
    """sort_pairs_u32 (through ds_sort_pairs_u32) / sort_pairs_u64 == numpy's stable argsort applied
    to keys and values: equal keys keep their input order (what the applied-flags path relies on
    when it sorts adds by actor with their indices as values)."""
    check(W.run_sort, ctx, case)


def test_sorts_back_to_back(ctx):
    """Sorts of different sizes and key types one after another on one context: each starts from
    scratch it has to zero itself, whatever the one before left."""
    seq = [(4, 17 * M.STILE + 1, "mod257", 9, "iota"), (8, 4097, "rand", 40, "randv"),
           (4, 65, "mod3", 32, "iota"), (8, 33 * M.STILE - 1, "mod257", 0, "iota"),
           (4, 17 * M.STILE + 1, "rand", 32, "randv")]
    for case in seq:
        check(W.run_sort, ctx, case)


def test_primitives_reject_what_they_cannot_do(ctx):
    """A look-back word of the sort counts in 30 bits: 2^30 items and more are refused with
    CE_ERR_INVALID_ARG by the size query, before anything is allocated or launched (the pointers
    here are null).  One item fewer passes the query and is refused for its null pointers."""
    if _STOP:
        pytest.fail("not run: " + _STOP[0])
    for f in (ctx.prim_sort_pairs_u32, ctx.prim_sort_pairs_u64):
        for n in (1 << 30, (1 << 30) + 1, 0xFFFFFFFF):
            with pytest.raises(crdtenc.CeError) as e:
                f(0, 0, 0, 0, n, 0)
            assert e.value.code == 64 and "more items than the primitive takes" in str(e.value), str(e.value)
        with pytest.raises(crdtenc.CeError) as e:
            f(0, 0, 0, 0, (1 << 30) - 1, 0)
        assert e.value.code == 64 and "null pointer" in str(e.value), str(e.value)
    with pytest.raises(crdtenc.CeError) as e:
        ctx.prim_excl_sum_u32(0, 0, 5)
    assert e.value.code == 64 and "null pointer" in str(e.value)
    with pytest.raises(crdtenc.CeError) as e:
        ctx.prim_excl_max_by_key(0, 0, 0, 5)
    assert e.value.code == 64 and "null pointer" in str(e.value)
    # and the context still works
    check(W.run_sort, ctx, (4, 65, "mod3", 32, "iota"))


@pytest.mark.parametrize("mode", ["default", "scan_3pass", "sort_ticket"])
def test_prims_under_process_switches(mode):
    """The scans' three-launch form at every scan size up to the third carry trip (CE_SCAN_3PASS=1;
    by default it only runs past 4096 tiles), the sort with its tiles ordered by the dispatch ticket
    at every sort size up to 33 tiles (CE_SORT_TICKET=1; by default only when the tiles do not fit
    the GPU at once), and a few sizes with both unset whatever this process's environment holds.
    One child process each (tests/prim_worker.py), which compares every case itself; every verdict
    is asserted here."""
    if _STOP:
        pytest.fail("not run: " + _STOP[0])
    name, extra = {"default": ("default", {}), "scan_3pass": ("scan", {"CE_SCAN_3PASS": "1"}),
                   "sort_ticket": ("sort", {"CE_SORT_TICKET": "1"})}[mode]
    env = dict(os.environ)
    for k in ("CE_SCAN_3PASS", "CE_SORT_TICKET", "CE_HIPCUB_SCAN"):
        env.pop(k, None)
    env.update(extra)
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "prim_worker.py"), name], env=env,
                           capture_output=True, text=True, timeout=240)
    except subprocess.TimeoutExpired:
        _STOP.append("the %s child did not end in time" % mode)
        raise
    if r.returncode != 0:
        _STOP.append("the %s child exited with %d" % (mode, r.returncode))
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-2000:])
    verdicts = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    want = [W.case_id(f, c) for f, c in W.subset(name)]
    assert len(want) > 50
    assert [v["id"] for v in verdicts] == want
    bad = [v for v in verdicts if not v["ok"]]
    assert not bad, (len(bad), bad[:5])
