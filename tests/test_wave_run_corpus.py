"""The properties of tests/wave_run_corpus.py that tests/test_gpu_wave_runs.py relies on, by the
oracles alone (no GPU): length classes, run shapes, where the maxima and the inactive files sit,
and each scenario's return code and statuses."""
import random

import msgpack
import pytest

import oracle
import pncounter_model as pm
import wave_run_corpus as W


def plain(c, i):
    st, pt = oracle.cryptor_decrypt(c.key, c.files[i][16:])
    assert st == 0 and pt[:16] == W.APP and len(pt) == c.lens[i]
    return pt[16:]


def gcounter_dots(c, i):
    u = msgpack.Unpacker(raw=False)
    u.feed(plain(c, i))
    return [(d["actor"], d["counter"]) for d in u.unpack()]


CORPORA = {"gcounter": W.gcounter_corpus, "pncounter": W.pncounter_corpus, "orswot": W.orswot_corpus}


@pytest.mark.parametrize("kind", list(CORPORA))
def test_shape(kind):
    c = CORPORA[kind]()
    n = len(c.files)
    assert n % 8 == 1 and n == len(c.fa) == len(c.vers) == len(c.lens)
    assert n == {"gcounter": 417, "pncounter": 321, "orswot": 201}[kind]
    assert c.fa == sorted(c.fa)
    for w, lo, hi in c.runs():
        assert c.vers[lo:hi] == list(range(hi - lo))
        if kind != "orswot":
            assert (hi - lo) % 4 != 0
    # writer changes fall inside groups of four, and the last group is ragged
    starts = [lo for _, lo, _ in c.runs()][1:]
    assert sum(1 for s in starts if s % 4) >= len(starts) - 1
    assert CORPORA[kind]() is c  # built once, shared


@pytest.mark.parametrize("kind", ["gcounter", "pncounter"])
def test_length_classes_and_alternation(kind):
    c = CORPORA[kind]()
    have = set(c.lens)
    assert set(range(17, 209)) <= have and set(range(3969, 4097)) <= have
    if kind == "gcounter":
        assert set(W.NBLK_EDGES) <= have and set(W.MULTI_PAGE) <= have
        for k in (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63):
            assert {64 * k - 1, 64 * k, 64 * k + 1} <= have
    for _, lo, hi in c.runs():
        down = sum(1 for i in range(lo, hi - 1) if c.lens[i] >= 2048 and c.lens[i + 1] < 256)
        up = sum(1 for i in range(lo, hi - 1) if c.lens[i] < 256 and c.lens[i + 1] >= 2048)
        assert down >= 8 and up >= 8, (lo, hi, down, up)


def test_gcounter_dots_and_maxima():
    c = W.gcounter_corpus()
    dots = {i: gcounter_dots(c, i) for i in range(len(c.files)) if c.lens[i] <= 4096}
    own = sum(1 for i, ds in dots.items() for a, _ in ds if a == c.actors[c.fa[i]])
    total = sum(len(ds) for ds in dots.values())
    assert 0.7 < own / total < 0.9
    widths = {len(msgpack.packb(ctr)) for ds in dots.values() for _, ctr in ds}
    assert widths == {1, 2, 3, 5, 9}
    assert max(ctr for ds in dots.values() for _, ctr in ds) == (1 << 64) - 1
    for w, lo, hi in c.runs():
        best = max((ctr, i) for i, ds in dots.items() for a, ctr in ds if a == c.actors[w])
        assert best == ((1 << 64) - 1 - w, lo if w % 2 == 0 else hi - 1)
        assert dots[best[1]][-1] == (c.actors[w], best[0])  # the file's last Dot: pending when it ends
    # files of one Dot length (the 16-lane rounds) and files whose Dots change length
    per_file = [{len(msgpack.packb(ctr)) for _, ctr in ds[:-1]} for ds in dots.values() if len(ds) > 4]
    assert sum(1 for x in per_file if len(x) == 1) > len(per_file) // 2
    assert sum(1 for x in per_file if len(x) > 1) > 40


def test_gcounter_inactive_files_inside_runs():
    c = W.gcounter_corpus()
    kinds = sorted(c.notes["special"].values())
    assert kinds == ["multi"] * 3 + ["stranger"] * 3
    inner = {i for _, lo, hi in c.runs() for i in range(lo + 4, hi - 4)}
    for i, k in c.notes["special"].items():
        assert i in inner
        if k == "multi":
            assert c.lens[i] in W.MULTI_PAGE
        else:
            named = {a for a, _ in gcounter_dots(c, i)}
            assert len(named & set(c.notes["strangers"])) == 1 and c.lens[i] <= 4096
    assert not set(c.notes["strangers"]) & set(c.actors)
    assert sorted(c.lens[i] for i, k in c.notes["special"].items() if k == "multi") == list(W.MULTI_PAGE)


def test_pncounter_maxima():
    c = W.pncounter_corpus()
    best = {}
    for i in range(len(c.files)):
        for (a, ctr), d in pm.dec_ops(plain(c, i)):
            best[(a, d)] = max(best.get((a, d), (0, -1)), (ctr, i))
    for w, lo, hi in c.runs():
        first, last = pm.DIRS[w % 2], pm.DIRS[(w + 1) % 2]
        assert best[(c.actors[w], first)] == ((1 << 32) - 1 - w, lo)
        assert best[(c.actors[w], last)] == ((1 << 32) - 1 - w, hi - 1)


def test_orswot_sizes():
    c = W.orswot_corpus()
    assert sum(1 for L in c.lens if L > W.DS_REGION) >= 10
    assert sum(1 for L in c.lens if W.DS_REGION - 64 <= L <= W.DS_REGION) >= 10
    assert min(c.lens) < 100 and max(c.lens) == 4096
    assert W.DS_REGION in c.lens and W.DS_REGION + 1 in c.lens
    assert sum(1 for L in c.lens if 100 <= L < W.DS_REGION - 64) > 150


@pytest.mark.parametrize("kind", list(CORPORA))
def test_scenarios_by_the_oracle(kind):
    c = CORPORA[kind]()
    assert set(c.scenarios) == ({"clean", "reject"} if kind == "orswot" else {"clean", "regate", "gap", "reject"})
    empty = W.new_oracle(kind).serialize()
    for name in c.scenarios:
        rc, st, state = W.expected(c, name)
        assert rc == c.want_rc[name] == {"clean": 0, "regate": 0, "gap": 13, "reject": 9}[name], name
        assert len(st) == len(c.scenarios[name][-1][0])
        if name in ("clean", "regate"):
            assert set(st) == {0} and state == W.expected(c, "clean")[2] != empty
    # reject: five tampered files where the kernels' groups make them interesting, every other
    # status 0, nothing folded
    n = len(c.files)
    rc, st, state = W.expected(c, "reject")
    t = c.tampered
    assert len(t) == 5 and [i for i, s in enumerate(st) if s] == t and {st[i] for i in t} == {9}
    assert state == empty
    assert t[0] < 4 and t[-1] // 4 == (n - 1) // 4
    assert any(c.lens[i] % 16 and c.files[i] != c.scenarios["reject"][0][1][i] and
               c.files[i][-17] != c.scenarios["reject"][0][1][i][-17] for i in t)
    assert any(a // 4 == b // 4 for a, b in zip(t, t[1:]))
    assert all(c.lens[i] <= 4096 for i in t)


@pytest.mark.parametrize("kind", ["gcounter", "pncounter"])
def test_regate_and_gap(kind):
    c = CORPORA[kind]()
    (first, _), (every, _) = c.scenarios["regate"]
    assert every == list(range(len(c.files)))
    oc = W.new_oracle(kind)
    files, fa, vers = c.step(first, {})
    assert oc.read_remote_ops(c.key, [W.APP], files, [c.actors[i] for i in fa], vers)[0] == 0
    for w, lo, hi in c.runs():
        skipped = [i for i in first if lo <= i < hi]
        assert skipped == list(range(lo, lo + (hi - lo + 1) // 2))  # old versions: apply == 0 in mid-run
        assert 1 <= len(skipped) < hi - lo                          # and at least one file applied
    # gap: one file of the third writer's run is missing; what comes before it stays folded
    gone = c.notes["gap"]
    _, lo, hi = c.runs()[2]
    assert lo + 4 < gone < hi - 4
    rc, st, state = W.expected(c, "gap")
    assert st[gone] == 13 and sum(1 for s in st if s) == 1
    before = W.new_oracle(kind)
    files, fa, vers = c.step(list(range(gone)), {})
    assert before.read_remote_ops(c.key, [W.APP], files, [c.actors[i] for i in fa], vers)[0] == 0
    assert state == before.serialize() != W.new_oracle(kind).serialize()


def test_full_grid_corpus():
    c = W.full_grid_corpus()
    n = len(c.files)
    assert n == 24577 == 3 * 8192 + 1 and len(c.actors) == 16 and len(c.runs()) == 16
    assert len({hi - lo for _, lo, hi in c.runs()}) > 4 and all((hi - lo) % 4 for _, lo, hi in c.runs())
    long_ = [i for i in range(n) if c.lens[i] >= 2048]
    assert all(i % 8 == 5 for i in long_) and len(long_) > n // 8 - 40
    assert sum(1 for L in c.lens if L < 200) == n - len(long_)
    assert W.expected(c, "clean")[0] == 0
    rc, st, state = W.expected(c, "reject")
    assert rc == 9 and [i for i, s in enumerate(st) if s] == c.tampered and len(c.tampered) == 4
    assert state == oracle.Core().serialize()


def test_dump_and_load(tmp_path):
    c = W.orswot_corpus()
    c.dump(str(tmp_path / "c.json"))
    d = W.Corpus.load(str(tmp_path / "c.json"))
    assert (d.kind, d.key, d.actors, d.files, d.fa, d.vers, d.lens) == (c.kind, c.key, c.actors, c.files, c.fa, c.vers, c.lens)
    assert d.want_rc == c.want_rc
    for name in c.scenarios:
        assert d.steps(name) == c.steps(name)


def test_tail_length_batch_lengths():
    rng = random.Random(3)
    actors = sorted(rng.randbytes(16) for _ in range(3))
    lens = [17, 18, 59, 60, 64, 1000, 4096]
    clears, fa, vers = W._tail_length_batch(rng, actors, lens)
    assert [len(x) for x in clears] == lens and fa == [0, 0, 0, 1, 1, 1, 2] and vers == [0, 1, 2, 0, 1, 2, 0]
