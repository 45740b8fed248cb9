"""The fused open kernels past one iteration per wave, in every variant the product library can
launch (crdt-enc_amd/csrc/ce_fused.hip: k_open_fold_small<16|32|64>, k_open_fold_v2<16|32, ...>,
k_open_fold_v3<PAIR, EARLY[, PN]>, k_open_ds8<PF> and the 16-lane DS form), and the multi-page
kernels' pull loops.

Each of them is a persistent loop that carries state from one group of files to the next: the
next file's prefetched parameters and ciphertext, PAIR's second keystream, ciphertext registers
and Poly1305 accumulators, the decode's speculated lengths and actor cache, the pending (slot,
max), the AuthFails tally.  The launchers size the grid to the resident blocks, so a wave runs a
second iteration only in batches of many thousands of files.  CE_TEST_GRID_CAP=<blocks> (read per
ingest, host side only) clamps the grid instead: at 1 a single wave walks every group of the
adversarial batches of tests/wave_run_corpus.py, so every length follows every other; at 3 and 7
runs end inside writers' runs, for both the contiguous (v3, ds8) and the strided partitions.

Every comparison is bit-exact against the oracle: return code, per-file statuses and
state_bytes() == serialize().  Every run asserts through ce_core_path_count that the kernel it
claims to test ran, that no alternate did, and whether a grid was capped."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

import crdtenc
import wave_run_corpus as W
from wave_run_worker import run_scenario, set_cap

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CAPS = [None, 1, 3, 7]
# variables the library reads once per process: never inherited by a child, never set in-process
PROCESS_ENV = ("CE_V3", "CE_FUSED_V2", "CE_DS8", "CE_DS8_PF")


@pytest.fixture(scope="module")
def ctx():
    c = crdtenc.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _no_cap_left_behind():
    yield
    set_cap(None)


def check_paths(paths, want, cap, where):
    ran = {k for k in W.OPEN_KEYS if paths[k]}
    assert ran == set(want), (where, paths)
    assert (paths[W.CAPPED] > 0) == bool(cap), (where, paths)


def check_run(ctx, corpus, name, cap, want_paths):
    where = (corpus.kind, name, cap)
    set_cap(cap)
    rc, st, state, before, paths = run_scenario(ctx, corpus, name)
    set_cap(None)
    orc, ost, ostate = W.expected(corpus, name)
    assert rc == orc == corpus.want_rc[name], (where, rc, orc, ctx.last_error())
    assert st == ost, (where, [(i, a, b) for i, (a, b) in enumerate(zip(st, ost)) if a != b][:10])
    assert state == ostate, where
    if name == "reject":
        assert state == before, where
    check_paths(paths, want_paths, cap, where)


# ------------------------------------------------------------------ (a) in-process variants
FUSED_KERNEL = {("1", "1"): "open_small_lpf64", ("1", "2"): "open_small_lpf32", ("1", "4"): "open_small_lpf16",
                ("2", "1"): "open_small_lpf64", ("2", "2"): "open_v2_lpf32", ("2", "4"): "open_v3_p0e1"}


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("fused,fpw", list(FUSED_KERNEL))
def test_gcounter_kernels_under_the_cap(ctx, monkeypatch, fused, fpw, cap):
    """CE_FUSED x CE_FILES_PER_WAVE (read at ce_core_open) reach k_open_fold_small<64|32|16>,
    k_open_fold_v2<32, 3, false, 3> and the default k_open_fold_v3<false, true>; each over the
    GCounter corpus's four scenarios (clean, regate, gap, reject) at the product's grid and
    capped to 1, 3 and 7 blocks."""
    for v in PROCESS_ENV:
        assert v not in os.environ
    monkeypatch.setenv("CE_FUSED", fused)
    monkeypatch.setenv("CE_FILES_PER_WAVE", fpw)
    corpus = W.gcounter_corpus()
    for name in corpus.scenarios:
        check_run(ctx, corpus, name, cap, [FUSED_KERNEL[(fused, fpw)]])


@pytest.mark.parametrize("cap", CAPS)
def test_pncounter_kernel_under_the_cap(ctx, cap):
    """k_open_fold_v3<false, true, true> (the only open a PNCounter core takes) over the PNCounter
    corpus: both planes' maxima in run-first and run-last files, so a pending maximum lost at a
    run's end, or carried into the wrong plane or writer, changes the state."""
    corpus = W.pncounter_corpus()
    for name in corpus.scenarios:
        check_run(ctx, corpus, name, cap, ["open_v3_pn"])


@pytest.mark.parametrize("cap", [None, 1, 3])
def test_dotset_open_only_kernel_under_the_cap(ctx, monkeypatch, cap):
    """CE_DS_FUSED_DECODE=0 (read per ingest): the dot-set kinds' open without the decode,
    k_open_fold_v2<16, 3, false, 1, DEC = false>, plaintext to HBM for the lane-per-file decode."""
    monkeypatch.setenv("CE_DS_FUSED_DECODE", "0")
    corpus = W.orswot_corpus()
    for name in corpus.scenarios:
        check_run(ctx, corpus, name, cap, ["open_only_lpf16"])


# ------------------------------------------------------------------ (b), (c) one child per variant
# one scenario at one cap takes well under a second in (a); a child runs at most 16 of them after
# a few seconds of start-up, so this is a wide margin and not a wait
CHILD_TIMEOUT = 180


def run_child(tmp_path, corpus, env, caps):
    path = str(tmp_path / ("%s.json" % corpus.kind))
    if not os.path.exists(path):
        corpus.dump(path)
    e = {k: v for k, v in os.environ.items() if k not in PROCESS_ENV and k != "CE_TEST_GRID_CAP"}
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(HERE, "wave_run_worker.py"), path,
                        ",".join(str(c or 0) for c in caps)], env=e, capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT)
    assert r.returncode == 0, (env, r.stderr[-3000:])
    return [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]


def check_child(tmp_path, corpus, env, caps, want_paths):
    lines = run_child(tmp_path, corpus, env, caps)
    assert [(x["scenario"], x["cap"]) for x in lines] == [(s, c or 0) for s in corpus.scenarios for c in caps]
    for x in lines:
        where = (env, x["scenario"], x["cap"])
        orc, ost, ostate = W.expected(corpus, x["scenario"])
        assert x["rc"] == orc == corpus.want_rc[x["scenario"]], where
        assert x["statuses"] == W.status_digest(ost), where
        assert x["state"] == hashlib.sha256(ostate).hexdigest(), where
        if x["scenario"] == "reject":
            assert x["unchanged"], where
        check_paths(x["paths"], want_paths, x["cap"], where)


@pytest.mark.parametrize("env,key", [({"CE_V3": "0"}, "open_v3_p0e0"), ({"CE_V3": "1"}, "open_v3_p1e0"),
                                     ({"CE_V3": "3"}, "open_v3_p1e1"), ({"CE_FUSED_V2": "1"}, "open_v2_lpf16")],
                         ids=["v3_plain", "v3_pair", "v3_pair_early", "v2_lpf16"])
def test_gcounter_variants_chosen_per_process(tmp_path, env, key):
    """CE_V3=0|1|3 (k_open_fold_v3<false, false>, <true, false>, <true, true>) and CE_FUSED_V2
    (k_open_fold_v2<16, 2, false, 1>): every scenario at every cap in one child process each."""
    check_child(tmp_path, W.gcounter_corpus(), env, CAPS, [key])


@pytest.mark.parametrize("env,keys", [({}, ["open_ds8_pf", "open_ds16"]),
                                      ({"CE_DS8_PF": "0"}, ["open_ds8_nopf", "open_ds16"]),
                                      ({"CE_DS8": "0"}, ["open_ds16"])],
                         ids=["ds8_pf", "ds8_nopf", "ds16_only"])
def test_orswot_opens(tmp_path, env, keys):
    """The dot-set opens over the Orswot corpus (sizes on both sides of kDsFuseRegion, so the
    default takes k_open_ds8 and then the 16-lane pass over the big files): k_open_ds8<true>,
    k_open_ds8<false> (CE_DS8_PF=0) and the 16-lane DS form for every file (CE_DS8=0)."""
    check_child(tmp_path, W.orswot_corpus(), env, [None, 1, 3], keys)


# ------------------------------------------------------------------ (d) the product's own grid
def test_gcounter_at_the_products_grid(ctx):
    """24,577 files (3 x 8,192 + 1), no cap: the default kernel's grid is its resident blocks, about
    2,048 one-wave blocks on an MI355X (256 CUs x 8; k_open_fold_v3 is bounded to 2 waves per SIMD),
    so each wave takes three groups of four files there -- this rests on the MI355X's residency, as
    test_gpu_pncounter.py::test_carry_across_a_waves_run does.  16 writers in runs of uneven length,
    every eighth file a long one; clean, then four tampered files."""
    for v in PROCESS_ENV + ("CE_FUSED", "CE_FILES_PER_WAVE"):
        assert v not in os.environ
    corpus = W.full_grid_corpus()
    for name in ("clean", "reject"):
        check_run(ctx, corpus, name, None, ["open_v3_p0e1"])


# ------------------------------------------------------------------ multi-page kernels
@pytest.fixture(scope="module")
def segdec_batch():
    """The files of test_gpu_segdec.py::test_segment_decode_cases as one batch, sealed on the CPU,
    and the oracle's result"""
    import random
    import oracle
    from test_gpu_segdec import cases
    writer, other, cs = cases()
    rng = random.Random(78)
    key = rng.randbytes(32)
    files = [W.seal(key, c, rng) for c in cs.values()]
    n = len(files)
    oc = oracle.Core()
    orc, ost = oc.read_remote_ops(key, [W.APP], files, [writer] * n, list(range(n)))
    assert orc == 0
    return key, [writer, other], files, ost, oc.serialize()


@pytest.mark.parametrize("cap", [None, 1, 5])
@pytest.mark.parametrize("mode", ["segdec", "decode_dots", "split"])
def test_multi_page_kernels_under_the_cap(ctx, monkeypatch, segdec_batch, mode, cap):
    """grid_waves_for takes the same cap: the segment pass (with and without the decode inside,
    CE_SEGDEC), the whole-file decode and CE_SPLIT's k_decode_split pull their work items from
    lists, here with one and five waves for about 340 segments of 11 files."""
    key, actors, files, ost, ostate = segdec_batch
    monkeypatch.setenv("CE_SEGDEC", "0" if mode == "decode_dots" else "1")
    if mode == "split":
        monkeypatch.setenv("CE_SPLIT", "1")
    else:
        monkeypatch.delenv("CE_SPLIT", raising=False)
    n = len(files)
    core = crdtenc.Core(ctx, kind=crdtenc.STATE_GCOUNTER, supported=[W.APP], current_data_version=W.APP)
    core.set_latest_key(key)
    set_cap(cap)
    rc, st = core.ingest_ops(files, actors, [0] * n, list(range(n)))
    set_cap(None)
    assert (rc, list(st)) == (0, ost), (mode, cap, ctx.last_error())
    assert core.state_bytes() == ostate
    assert (core.path_count("segdec_records") > 0) == (mode == "segdec")
    core.close()
