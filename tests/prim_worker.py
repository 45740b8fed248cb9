"""The device primitives (ce_ctx_prim_*) run case by case against tests/prim_model.py: the helpers
tests/test_gpu_prims.py calls in its own process, and, run as a script, the child process of its
test_prims_under_process_switches.

CE_SCAN_3PASS and CE_SORT_TICKET are read once per process, so each setting needs a fresh process:

    python prim_worker.py <subset>

runs the named subset of prim_model's cases on cuda:0 under whatever environment it was given,
compares every output itself and prints one JSON line per case: {"id": ..., "ok": true | false,
"detail": ...}.  It exits 0 when every case ran (whatever the verdicts, which the parent asserts one
by one) and stops at the first case that raises."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, "..", "crdt-enc_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import prim_model as M  # noqa: E402

PAD = 64                                   # items past n in every output, which must stay untouched
SENTINEL = {4: 0xDEADBEEF, 8: 0xDEADBEEFCAFEF00D}
_SIGNED = {4: np.int32, 8: np.int64}
_UNSIGNED = {4: np.uint32, 8: np.uint64}


def _up(a):
    """an unsigned numpy array -> a device tensor of the same bits"""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(_SIGNED[a.dtype.itemsize])).to("cuda:0")


def _out(n, itemsize):
    return _up(np.full(n + PAD, SENTINEL[itemsize], _UNSIGNED[itemsize]))


def _down(t):
    a = t.cpu().numpy()
    return a.view(_UNSIGNED[a.dtype.itemsize])


def _ptr(t):
    return t.data_ptr() if t.numel() else 0


def _verdict(cid, outs):
    """outs: (name, device output of n + PAD items, expected first n items).  The whole output must
    equal the reference and the PAD items after it must still hold the sentinel."""
    problems = []
    for name, t, want in outs:
        got = _down(t)
        n = want.size
        if not np.array_equal(got[n:], np.full(PAD, SENTINEL[got.dtype.itemsize], got.dtype)):
            bad = np.flatnonzero(got[n:] != got.dtype.type(SENTINEL[got.dtype.itemsize]))
            problems.append("%s: written past n at n + %d" % (name, int(bad[0])))
        if not np.array_equal(got[:n], want):
            bad = np.flatnonzero(got[:n] != want)
            i = int(bad[0])
            problems.append("%s: %d of %d items differ, first at %d (tile %d + %d): got %#x, want %#x" % (
                name, bad.size, n, i, i // M.TILE, i % M.TILE, int(got[i]), int(want[i])))
    return {"id": cid, "ok": not problems, "detail": "; ".join(problems)}


def _sync():
    import torch
    torch.cuda.synchronize()


def run_sum(ctx, case):
    a, _ = M.sum_input(*case)
    d_in, d_out = _up(a), _out(a.size, 4)
    _sync()
    ctx.prim_excl_sum_u32(_ptr(d_in), d_out.data_ptr(), a.size)
    v = _verdict("sum-" + M.sum_id(case), [("out", d_out, M.excl_sum_u32(a))])
    if not np.array_equal(_down(d_in), a):
        v["ok"], v["detail"] = False, v["detail"] + "; the input was modified"
    return v


def run_seg(ctx, case):
    keys, vals, _ = M.seg_input(*case)
    d_k, d_v, d_out = _up(keys), _up(vals), _out(keys.size, 8)
    _sync()
    ctx.prim_excl_max_by_key(_ptr(d_k), _ptr(d_v), d_out.data_ptr(), keys.size)
    v = _verdict("seg-" + M.seg_id(case), [("out", d_out, M.excl_max_by_key(keys, vals))])
    if not (np.array_equal(_down(d_k), keys) and np.array_equal(_down(d_v), vals)):
        v["ok"], v["detail"] = False, v["detail"] + "; an input was modified"
    return v


def run_sort(ctx, case, inputs=None):
    kb, n, kp, bits, vp = case
    keys, vals, _ = inputs if inputs is not None else M.sort_input(*case)
    d_ki, d_vi, d_ko, d_vo = _up(keys), _up(vals), _out(n, kb), _out(n, 4)
    _sync()
    f = ctx.prim_sort_pairs_u32 if kb == 4 else ctx.prim_sort_pairs_u64
    f(_ptr(d_ki), d_ko.data_ptr(), _ptr(d_vi), d_vo.data_ptr(), n, bits)
    wk, wv = M.sort_pairs(keys, vals)
    v = _verdict("sort-" + M.sort_id(case), [("keys", d_ko, wk), ("vals", d_vo, wv)])
    if not (np.array_equal(_down(d_ki), keys) and np.array_equal(_down(d_vi), vals)):
        v["ok"], v["detail"] = False, v["detail"] + "; an input was modified"
    return v


# the subsets a child process runs: (runner, case) lists
DEFAULT_SCAN_SIZES = (2049, M.TRIP * M.TILE + 1)
DEFAULT_SORT_SIZES = (4097, 17 * M.STILE + 1)


def subset(name):
    if name == "scan":          # under CE_SCAN_3PASS=1: every scan case up to the third carry trip
        return [(run_sum, c) for c in M.SUM_CASES if c[0] <= M.SCAN_WORKER_MAX] + \
               [(run_seg, c) for c in M.SEG_CASES if c[0] <= M.SCAN_WORKER_MAX]
    if name == "sort":          # under CE_SORT_TICKET=1: every sort case up to 33 tiles
        return [(run_sort, c) for c in M.SORT_CASES if c[1] <= M.SORT_WORKER_MAX]
    if name == "default":       # the switches unset whatever the parent's environment holds
        return [(run_sum, c) for c in M.SUM_CASES if c[0] in DEFAULT_SCAN_SIZES] + \
               [(run_seg, c) for c in M.SEG_CASES if c[0] in DEFAULT_SCAN_SIZES] + \
               [(run_sort, c) for c in M.SORT_CASES if c[1] in DEFAULT_SORT_SIZES]
    raise KeyError(name)


def case_id(runner, case):
    if runner is run_sum:
        return "sum-" + M.sum_id(case)
    return ("seg-" + M.seg_id(case)) if runner is run_seg else ("sort-" + M.sort_id(case))


def main():
    import crdtenc
    ctx = crdtenc.Context(0)
    for runner, case in subset(sys.argv[1]):
        print(json.dumps(runner(ctx, case)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
