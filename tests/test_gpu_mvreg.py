"""The MVReg<u64, Uuid> fold on the GPU at its sum-carry, tie, block, grid, grammar and
irregular-state edges: every case of tests/mvreg_cases.py through the C ABI, against the
sequential crdts restatement (oracle/crdts.py).

Per step of a case, bit-exactly: return code, per-file statuses, `state_bytes()`, `mvreg_read()`
(the values in `vals` order) and `read_clock()` (the join of the values' clocks).  State steps
run through ingest_states, ingest_states_device, merge_state and merge_state_device.  Families
A-E must take the device route (the survivor rounds of ce_dotset.hip) and never the host
fallback; family F (state files whose vals is no antichain of non-empty clocks) must take the
host route of ce_dotset_host.cpp (mv_host_merge / mv_host_apply).  What each case is aimed at is
in its `target` and in tests/test_mvreg_cases_model.py, which shows a model wrong in that way
failing it.
"""
import numpy as np
import pytest

import crdtenc
import mvreg_cases as MC
from oracle import crdts as C

pytestmark = pytest.mark.gpu
APP = MC.APP
CORE = crdtenc.CORE_VERSION
KEY = bytes(range(32))
STATE_ROUTES = ("ingest_states", "ingest_states_device", "merge_state", "merge_state_device")
CASES = MC.all_cases()


@pytest.fixture(scope="module")
def ctx():
    c = crdtenc.Context(0)
    yield c
    c.close()


def seal(ctx, clears):
    return [CORE + e for e in ctx.encrypt_batch(KEY, clears)]


def on_device(blobs):
    import torch
    dev = torch.device("cuda", 0)
    offs = np.zeros(len(blobs) + 1, np.int64)
    offs[1:] = np.cumsum([len(x) for x in blobs])
    blob = torch.from_numpy(np.frombuffer(b"".join(blobs) + bytes(64), np.uint8).copy()).to(dev)
    offs_d = torch.from_numpy(offs).to(dev)
    torch.cuda.synchronize()
    return blob, offs_d, int(offs[-1])


def states_step(ctx, core, sws, route):
    """-> (rc, statuses)"""
    if route == "ingest_states":
        return core.ingest_states(seal(ctx, [APP + sw for sw in sws]))
    if route == "ingest_states_device":
        blob, offs, ln = on_device(seal(ctx, [APP + sw for sw in sws]))
        return core.ingest_states_device(blob.data_ptr(), offs.data_ptr(), len(sws), ln, want_status=True)
    rcs = []
    for sw in sws:
        if route == "merge_state":
            rcs.append(core.merge_state(sw))
        else:
            blob, _, ln = on_device([sw])
            rcs.append(core.merge_state_device(blob.data_ptr(), ln))
    return max(rcs), rcs


def run_case(ctx, case, route="ingest_states"):
    core = crdtenc.Core(ctx, kind=crdtenc.STATE_MVREG, supported=[APP], current_data_version=APP)
    core.set_latest_key(KEY)
    me = core.info_actor()
    want = MC.run_oracle(case, me)[1]
    # C.Core itself over the sealed files, where the case leaves the decode to the oracle or is small
    oc = C.Core("mvreg") if case.family != "D" else None
    for step, (wrc, wst, wvals, wbytes) in zip(case.steps, want):
        if step[0] == "states":
            rc, st = states_step(ctx, core, step[1], route)
            if oc:
                assert oc.read_remote_states(KEY, [APP], seal(ctx, [APP + sw for sw in step[1]])) == (wrc, wst)
        elif step[0] == "ops":
            _, writers, files, _ = step
            sealed = seal(ctx, [f[0] for f in files])
            fa, fv = [f[1] for f in files], [f[2] for f in files]
            rc, st = core.ingest_ops(sealed, writers, fa, fv)
            if oc:
                assert oc.read_remote_ops(KEY, [APP], sealed, [writers[i] for i in fa], fv) == (wrc, wst)
        else:
            rc, st = core.apply_ops(step[1]), None
            if oc:
                for op in C.dec_ops("mvreg", step[1]):
                    oc.state.apply(op)
                oc.nov.apply(me, oc.nov.get(me) + 1)
        assert (rc, st) == (wrc, wst), (case, step[0])
        if oc:
            assert oc.serialize() == wbytes
        assert core.state_bytes() == wbytes, (case, step[0], core.mvreg_read(), wvals)
        assert core.mvreg_read() == wvals
        join = C.VClock()
        for c, _ in C.dec_state("mvreg", wbytes)[1].vals:
            join.merge(c)
        assert core.read_clock() == sorted(join.dots.items())
    if case.want is not None:
        assert core.mvreg_read() == case.want
    # the route: the survivor rounds for every case but F's, which the host fallback takes
    assert (core.path_count("mv_host_merge"), core.path_count("mv_host_apply")) == case.host
    if case.family != "F":
        assert core.path_count("mv_device_rounds") >= 1
    assert core.path_count("ds_host_decode_files") == case.host_decode
    core.close()


def has_states(case):
    return case.name.endswith("_after_state") or case.family == "F" or case.name.startswith(("B2", "B3"))


@pytest.mark.parametrize("case", [c for c in CASES if not has_states(c)], ids=repr)
def test_mvreg_ops_case(ctx, case):
    assert not any(s[0] == "states" for s in case.steps)   # (those run below, once per state route)
    run_case(ctx, case)


@pytest.mark.parametrize("route", STATE_ROUTES)
@pytest.mark.parametrize("case", [c for c in CASES if has_states(c)], ids=repr)
def test_mvreg_state_case(ctx, case, route):
    assert any(s[0] == "states" for s in case.steps)
    run_case(ctx, case, route)

