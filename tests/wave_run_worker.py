"""Runs the scenarios of a tests/wave_run_corpus.py corpus on cuda:0 and reports what the product
did.  tests/test_gpu_wave_runs.py imports run_scenario for the variants it can select in-process,
and starts this file as a child process for those the library reads once per process (CE_V3,
CE_FUSED_V2, CE_DS8, CE_DS8_PF, which the parent sets in the child's environment):

    wave_run_worker.py <corpus.json> <caps, comma separated, 0 = none>

For every scenario and cap, in that order, one JSON line: scenario, cap, the return code, a
digest of the statuses, the sha256 of the state bytes, whether a rejected batch left the state as
it was, and the open kernels' path counts."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, "..", "crdt-enc_amd"), os.path.join(HERE, ".."), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import crdtenc  # noqa: E402
import wave_run_corpus as W  # noqa: E402

KIND = {"gcounter": crdtenc.STATE_GCOUNTER, "pncounter": crdtenc.STATE_PNCOUNTER, "orswot": crdtenc.STATE_ORSWOT}


def set_cap(cap):
    """CE_TEST_GRID_CAP for the ingests that follow (None or 0: unset)"""
    if cap:
        os.environ["CE_TEST_GRID_CAP"] = str(cap)
    else:
        os.environ.pop("CE_TEST_GRID_CAP", None)


def run_scenario(ctx, corpus, name):
    """-> (rc, statuses, state bytes, state bytes before the last step, path counts) of the
    scenario's steps into a fresh core"""
    core = crdtenc.Core(ctx, kind=KIND[corpus.kind], supported=[W.APP], current_data_version=W.APP)
    core.set_latest_key(corpus.key)
    rc = st = before = None
    for files, fa, vers in corpus.steps(name):
        before = core.state_bytes()
        rc, st = core.ingest_ops(files, corpus.actors, fa, vers)
    state = core.state_bytes()
    paths = {k: core.path_count(k) for k in W.OPEN_KEYS + (W.CAPPED,)}
    core.close()
    return rc, list(st), state, before, paths


def main():
    corpus = W.Corpus.load(sys.argv[1])
    caps = [int(x) for x in sys.argv[2].split(",")]
    ctx = crdtenc.Context(0)
    for name in corpus.scenarios:
        for cap in caps:
            set_cap(cap)
            rc, st, state, before, paths = run_scenario(ctx, corpus, name)
            print(json.dumps({"scenario": name, "cap": cap, "rc": rc, "statuses": W.status_digest(st),
                              "state": hashlib.sha256(state).hexdigest(), "unchanged": state == before,
                              "paths": paths}), flush=True)
    set_cap(None)
    ctx.close()


if __name__ == "__main__":
    main()
