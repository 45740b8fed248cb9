"""The Poly1305 edge vectors of tests/poly_edges.py through every open and seal kernel.

The tags of these files are chosen, not random: the fully reduced Horner sum h sits on 0..5 and
p-6..p-1 (the final conditional subtraction of p, where a kernel holds h or h + p), on the limb
and word boundaries (the +5 carry chain and the limb carries rippling, the word carries of h + s),
on bits 128 and 129, and on the tags 0, 1, 2^128 - 1, s, s - 1 and the borrows of tag - s into an
equal word (poly_tag's 128-bit carry, poly_aux's 128-bit borrow); heavy files hold the largest r
limbs and 0xff ciphertext for the stated limb and column bounds.  poly_edges' docstring says what
each target is for; a failure message names the file, and test_poly_edges_model.py::test_coverage
lists them, so a failing vector tells which reduction step broke.

Each family has its own evaluation order and tail over ce_device.h: the segment kernel and
k_finalize_multi (poly_tag), k_open_fold_small<16|32|64> and k_open_fold_v2 (poly_tag),
k_open_fold_v3 in all its forms, k_open_ds8 and the 16-lane DS form (four-product column sums,
unreduced 32-bit lane sums, poly_check against the setup's ts = tag - s).  Every one of them runs
the clean scenario (all accepted, each file's own op in the state) and the reject scenario (the
twins tag - 5, tag + 5, tag + 1 of the files with h in 0..4 and p-5..p-1 among fresh files: rc 9,
status 9 exactly at the twins, state unchanged), bit-exact against the oracle as in
test_gpu_wave_runs.py, with ce_core_path_count showing that the kernel named ran and no other.
Context.decrypt_batch and Context.encrypt have no path counts: their kernels follow from the
lengths alone (one 16 KiB Poly1305 segment: the segment kernel's own tail; 2..65 segments:
k_finalize_multi, a lane per segment; 66: its chained form)."""
import os

import pytest

import crdtenc
import poly_edges as E
import wave_run_corpus as W
from test_gpu_wave_runs import FUSED_KERNEL, PROCESS_ENV, check_child, check_paths
from wave_run_worker import run_scenario, set_cap

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = crdtenc.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _no_cap_left_behind():
    yield
    set_cap(None)


def differing(corpus, name, st, ost):
    """The vectors whose status differs: (target or twin, of which target, length, crafted block,
    got, expected)"""
    idx = corpus.scenarios[name][-1][0]
    vs = [corpus.vectors[i] for i in idx]
    return [(v.name, v.of.name if v.of else None, len(v.ct), (v.of or v).j, a, b)
            for v, a, b in zip(vs, st, ost) if a != b][:12]


def check_named(ctx, corpus, name, cap, want_paths):
    """test_gpu_wave_runs.check_run's comparisons, the statuses first so that a failure names its
    vectors"""
    where = (corpus.kind, name, cap)
    set_cap(cap)
    rc, st, state, before, paths = run_scenario(ctx, corpus, name)
    set_cap(None)
    orc, ost, ostate = W.expected(corpus, name)
    assert st == ost, (where, differing(corpus, name, st, ost))
    assert rc == orc == corpus.want_rc[name], (where, rc, orc, ctx.last_error())
    assert state == ostate, where
    if name == "reject":
        assert state == before, where
        assert [i for i, s in enumerate(st) if s] == corpus.tampered
    return paths


def run_both(ctx, corpus, cap, want_paths):
    for name in ("clean", "reject"):
        check_paths(check_named(ctx, corpus, name, cap, want_paths), want_paths, cap, (corpus.kind, name, cap))


# ------------------------------------------------------------------ GCounter
@pytest.mark.parametrize("fused,fpw", list(FUSED_KERNEL))
def test_gcounter_in_process(ctx, monkeypatch, fused, fpw):
    """k_open_fold_small<64|32|16>, k_open_fold_v2<32, ...> and the default k_open_fold_v3<false,
    true>, by CE_FUSED x CE_FILES_PER_WAVE"""
    for v in PROCESS_ENV:
        assert v not in os.environ
    monkeypatch.setenv("CE_FUSED", fused)
    monkeypatch.setenv("CE_FILES_PER_WAVE", fpw)
    run_both(ctx, E.corpus("gcounter"), None, [FUSED_KERNEL[(fused, fpw)]])


def test_gcounter_default_kernel_one_wave(ctx, monkeypatch):
    """k_open_fold_v3<false, true> capped to one block: one wave's accumulators carry from every
    edge file into the next"""
    monkeypatch.setenv("CE_FUSED", "2")
    monkeypatch.setenv("CE_FILES_PER_WAVE", "4")
    run_both(ctx, E.corpus("gcounter"), 1, ["open_v3_p0e1"])


@pytest.mark.parametrize("env,key", [({"CE_V3": "0"}, "open_v3_p0e0"), ({"CE_V3": "1"}, "open_v3_p1e0"),
                                     ({"CE_V3": "3"}, "open_v3_p1e1"), ({"CE_FUSED_V2": "1"}, "open_v2_lpf16")],
                         ids=["v3_plain", "v3_pair", "v3_pair_early", "v2_lpf16"])
def test_gcounter_variants_chosen_per_process(tmp_path, env, key):
    """k_open_fold_v3<false, false>, <true, false>, <true, true> (PAIR holds two files'
    accumulators) and k_open_fold_v2<16, ...>, one child process each"""
    check_child(tmp_path, E.corpus("gcounter"), env, [None], [key])


# ------------------------------------------------------------------ PNCounter, Orswot
def test_pncounter(ctx):
    """k_open_fold_v3<false, true, true>"""
    run_both(ctx, E.corpus("pncounter"), None, ["open_v3_pn"])


@pytest.mark.parametrize("env,keys", [({}, ["open_ds8_pf", "open_ds16"]),
                                      ({"CE_DS8_PF": "0"}, ["open_ds8_nopf", "open_ds16"]),
                                      ({"CE_DS8": "0"}, ["open_ds16"])],
                         ids=["ds8_pf", "ds8_nopf", "ds16_only"])
def test_orswot_opens(tmp_path, env, keys):
    """k_open_ds8<true>, k_open_ds8<false> and the 16-lane DS form (the files past kDsFuseRegion
    by default, every file with CE_DS8=0), one child process each"""
    check_child(tmp_path, E.corpus("orswot"), env, [None], keys)


def test_orswot_open_only(ctx, monkeypatch):
    """k_open_fold_v2<16, 3, false, 1, DEC = false> (CE_DS_FUSED_DECODE=0)"""
    monkeypatch.setenv("CE_DS_FUSED_DECODE", "0")
    run_both(ctx, E.corpus("orswot"), None, ["open_only_lpf16"])


# ------------------------------------------------------------------ multi-page ingest
@pytest.mark.parametrize("mode", ["segdec", "decode_dots", "split"])
def test_multi_page_ingest(ctx, monkeypatch, mode):
    """Crafted and heavy files of 4097, 5000 and 9000 plaintext bytes (one segment: the segment
    pass's own tag) and of 40000 (three: k_finalize_multi), in the three modes of
    test_multi_page_kernels_under_the_cap"""
    monkeypatch.setenv("CE_SEGDEC", "0" if mode == "decode_dots" else "1")
    if mode == "split":
        monkeypatch.setenv("CE_SPLIT", "1")
    else:
        monkeypatch.delenv("CE_SPLIT", raising=False)
    corpus = E.multi_page_corpus()
    for name in ("clean", "reject"):
        check_named(ctx, corpus, name, None, None)
    # which segment pass ran: the one that decodes counts every file of several segments, folded
    # from its records or handed to the whole-file decode
    core = crdtenc.Core(ctx, kind=crdtenc.STATE_GCOUNTER, supported=[W.APP], current_data_version=W.APP)
    core.set_latest_key(corpus.key)
    files, fa, vers = corpus.steps("clean")[0]
    assert core.ingest_ops(files, corpus.actors, fa, vers)[0] == 0
    assert (core.path_count("segdec_records") + core.path_count("segdec_fallback") > 0) == (mode == "segdec")
    core.close()


# ------------------------------------------------------------------ Context.decrypt_batch, encrypt
SIZE_CLASSES = {"one_segment": (0, 16, 4096, 16384 - 16), "few_segments": (16384 + 1, 70000),
                "many_segments": ((1 << 20) + 17, (65 << 14) + 4097)}


@pytest.mark.parametrize("cls", list(SIZE_CLASSES))
def test_decrypt_batch(ctx, cls):
    """One key; ciphertexts random but for the crafted block: status 0 and ct XOR keystream, first
    alone and then with the twins among them (status 9, the region zeroed, the others still
    released).  The megabyte files' twins are one each (tag - 5, tag + 5, tag + 1 in turn)."""
    key, vs = E.aead_vectors()
    mine = [v for v in vs if len(v.ct) in SIZE_CLASSES[cls]]
    assert {len(v.ct) for v in mine} == set(SIZE_CLASSES[cls])
    rc, st, pts, raw, offs = ctx.decrypt_batch(key, [v.box() for v in mine])
    assert rc == 0 and st == [0] * len(mine), [(v.name, len(v.ct), s) for v, s in zip(mine, st) if s]
    for v, pt in zip(mine, pts):
        assert pt == v.plaintext(), (v.name, len(v.ct), v.j)
    batch, k = [], 0
    for v in mine:
        if v.name in E.TWINNED:
            tw = v.twins()
            if len(v.ct) > 1 << 20:
                tw = [tw[k % 3]]
                k += 1
            batch += tw[:1] + [v] + tw[1:]
        elif v.name == "empty":
            batch += [E.Vector("twin-1", key, v.nonce, v.ct, v.r, v.s, tag=(v.tag - 1) & E.M128, of=v), v]
        else:
            batch.append(v)
    want = [9 if v.of is not None else 0 for v in batch]
    assert want.count(9) >= (6 if cls == "many_segments" else 13)
    rc, st, pts, raw, offs = ctx.decrypt_batch(key, [v.box() for v in batch])
    assert rc == 9 and st == want, [(v.name, len(v.ct), s) for v, s, w in zip(batch, st, want) if s != w]
    for i, v in enumerate(batch):
        if v.of is None:
            assert pts[i] == v.plaintext(), (v.name, len(v.ct))
        else:
            assert raw[offs[i]:offs[i] + len(v.ct)] == bytes(len(v.ct)), (v.name, v.of.name, len(v.ct))


def test_seal(ctx):
    """Context.encrypt of ct XOR keystream under the same (key, nonce) gives the boxed ct || tag
    byte for byte, the tag being the big-integer reference's: the seal's segment kernel (one-page
    segments up to 1 MiB, 16 KiB beyond) and k_finalize_multi<true>"""
    key, vs = E.aead_vectors()
    mine = [v for v in vs if len(v.ct) in E.SEAL_LENS]
    assert {len(v.ct) for v in mine} == set(E.SEAL_LENS)
    for v in mine:
        enc = ctx.encrypt(key, v.plaintext(), nonce=v.nonce)
        assert enc[-16:] == v.tag.to_bytes(16, "little"), (v.name, len(v.ct), v.j)
        assert enc == v.box(), (v.name, len(v.ct))
