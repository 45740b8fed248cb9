"""Adversarial batches for the fused open kernels' persistent loops (tests/test_gpu_wave_runs.py,
tests/wave_run_worker.py), checked on the CPU by tests/test_wave_run_corpus.py.

Every fused open kernel carries state from one group of files to the next one of its wave's run:
prefetched parameters and ciphertext, keystream and ciphertext registers, Poly1305 accumulators,
the decode's speculated lengths and actor cache, the pending (slot, max), the AuthFails tally.
The batches here put what disturbs that state next to each other -- long files before short
ones, every tail shape, writer changes inside groups, gated, multi-page and tampered files in
mid-run -- and CE_TEST_GRID_CAP makes a wave walk many groups of them.

Everything is deterministic from a seed and sealed on the CPU (oracle.cryptor_encrypt, rng
nonces); the expected results come from the oracles alone.  A corpus is a base batch in load_ops
order plus scenarios; a scenario is a list of steps (ingest calls) into one fresh core, and the
last step's return code, statuses and state are what is compared."""
import functools
import hashlib
import json
import random

import msgpack

import oracle
import pncounter_model as pm
from oracle import crdts as C

APP = bytes.fromhex("aadfd5a66e194b24a8024fa27c72f20c")
CORE_VERSION = C.CORE_VERSION

# ce_core_path_count keys of the single-page open kernels (one count per launch) and of a grid
# that CE_TEST_GRID_CAP reduced
OPEN_KEYS = ("open_small_lpf16", "open_small_lpf32", "open_small_lpf64", "open_v2_lpf16", "open_v2_lpf32",
             "open_v3_p0e0", "open_v3_p1e0", "open_v3_p0e1", "open_v3_p1e1", "open_v3_pn",
             "open_ds8_pf", "open_ds8_nopf", "open_ds16", "open_only_lpf16")
CAPPED = "open_grid_capped"

# plaintext lengths at which a lane of the 16-lane kernels gains or loses one of its four
# ChaCha20 blocks (nblk = 16 j + 1), and the ends of the one-block and one-page ranges
NBLK_EDGES = sorted({64 * k + d for k in (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63) for d in (-1, 0, 1)} | {4096})
MULTI_PAGE = (4097, 5000, 9000)
DS_REGION = 2048  # kDsFuseRegion (ce_kernels.h)


def seal(key, clear, rng):
    st, enc = oracle.cryptor_encrypt(key, rng.randbytes(24), clear)
    assert st == 0
    return CORE_VERSION + enc


def _tail_length_batch(rng, actors, lens):
    """Plaintexts of exactly the given lengths: APP || msgpack(Vec<Dot>) || trailing bytes
    (rmp_serde::from_slice reads one value; the oracle ignores the tail the same way)."""
    clears, fa, vers = [], [], []
    per = -(-len(lens) // len(actors))
    for i, L in enumerate(lens):
        a, v = i // per, i % per
        dots, body = [], msgpack.packb([])
        while True:
            d = {"actor": actors[a] if rng.random() < 0.8 else rng.choice(actors),
                 "counter": rng.getrandbits(rng.choice([6, 16, 31, 40]))}
            nb = msgpack.packb(dots + [d], use_bin_type=True)
            if 16 + len(nb) > L:
                break
            dots.append(d)
            body = nb
        clears.append(APP + body + rng.randbytes(L - 16 - len(body)))
        fa.append(a)
        vers.append(v)
    return clears, fa, vers


def _canonical_orswot(rng, actors, n_versions, ops_per_file, members, widths=(1, 2, 3, 5, 9), p_rm=0.2):
    """Op files whose ops are all the forms the open's decode proves: one-member Adds of the
    writer's own dots, removals with a one-entry clock {writer: an earlier counter}; counters and
    members drawn from every msgpack uint width (fixint, cc, cd, ce, cf).  ops_per_file: a count,
    or a function of (writer index, version)."""
    lim = {1: (0, 127), 2: (128, 255), 3: (256, 65535), 5: (65536, (1 << 32) - 1), 9: (1 << 32, (1 << 64) - 1)}
    files = {a: [] for a in actors}
    ctr = {a: 0 for a in actors}
    for v in range(n_versions):
        for ai, a in enumerate(actors):
            ops = []
            for _ in range(ops_per_file(ai, v) if callable(ops_per_file) else ops_per_file):
                w = rng.choice(widths)
                lo, hi = lim[w]
                if ctr[a] and rng.random() < p_rm:
                    ops.append(("Rm", C.VClock({a: rng.randint(1, ctr[a])}), [rng.randrange(members)]))
                else:
                    ctr[a] = max(ctr[a] + 1, rng.randint(lo, hi))
                    mem = rng.randrange(members) if rng.random() < 0.5 else rng.randint(*lim[rng.choice(widths)])
                    ops.append(("Add", (a, ctr[a]), [mem]))
            files[a].append(ops)
    return files


class Corpus:
    """kind: "gcounter" | "pncounter" | "orswot"; files / fa / vers: the base batch in load_ops
    order (fa indexes actors); lens: plaintext lengths; scenarios: name -> [(idx, patch)] steps,
    a step's batch being files[i] for i in idx with patch[i] in place of files[i]; want_rc: the
    return code each scenario's last step must have; tampered: the reject scenario's files."""

    def __init__(self, kind, key, actors, files, fa, vers, lens):
        self.kind, self.key, self.actors = kind, key, actors
        self.files, self.fa, self.vers, self.lens = files, fa, vers, lens
        self.scenarios, self.want_rc, self.tampered, self.notes = {}, {}, [], {}

    def step(self, idx, patch):
        return ([patch.get(i, self.files[i]) for i in idx], [self.fa[i] for i in idx], [self.vers[i] for i in idx])

    def steps(self, name):
        return [self.step(idx, patch) for idx, patch in self.scenarios[name]]

    def runs(self):
        """[(writer, first index, one past the last)] of the base batch"""
        out, lo = [], 0
        for i in range(1, len(self.fa) + 1):
            if i == len(self.fa) or self.fa[i] != self.fa[lo]:
                out.append((self.fa[lo], lo, i))
                lo = i
        return out

    def dump(self, path):
        with open(path, "w") as f:
            json.dump({"kind": self.kind, "key": self.key.hex(), "actors": [a.hex() for a in self.actors],
                       "files": [x.hex() for x in self.files], "fa": self.fa, "vers": self.vers, "lens": self.lens,
                       "want_rc": self.want_rc,
                       "scenarios": {k: [[idx, {str(i): b.hex() for i, b in patch.items()}] for idx, patch in v]
                                     for k, v in self.scenarios.items()}}, f)

    @staticmethod
    def load(path):
        with open(path) as f:
            d = json.load(f)
        c = Corpus(d["kind"], bytes.fromhex(d["key"]), [bytes.fromhex(a) for a in d["actors"]],
                   [bytes.fromhex(x) for x in d["files"]], d["fa"], d["vers"], d["lens"])
        c.want_rc = d["want_rc"]
        c.scenarios = {k: [(idx, {int(i): bytes.fromhex(b) for i, b in patch.items()}) for idx, patch in v]
                       for k, v in d["scenarios"].items()}
        return c


def new_oracle(kind):
    if kind == "gcounter":
        return oracle.Core()
    return pm.Core() if kind == "pncounter" else C.Core("orswot")


def status_digest(st):
    return hashlib.sha256(",".join(str(int(s)) for s in st).encode()).hexdigest()


@functools.lru_cache(maxsize=None)
def expected(corpus, name):
    """-> (rc, statuses, state bytes) of the scenario's last step, by the oracle alone"""
    oc = new_oracle(corpus.kind)
    rc = st = None
    for files, fa, vers in corpus.steps(name):
        rc, st = oc.read_remote_ops(corpus.key, [APP], files, [corpus.actors[i] for i in fa], vers)
    return rc, list(st), oc.serialize()


# ---------------------------------------------------------------------------------- ordering
def alternate_long_short(rng, lens):
    """Long and short lengths in turn: the sorted list's two halves, each shuffled"""
    s = sorted(lens)
    short, long_ = s[:len(s) // 2], s[len(s) // 2:]
    rng.shuffle(short)
    rng.shuffle(long_)
    out = []
    for i in range(len(long_)):
        out.append(long_[i])
        if i < len(short):
            out.append(short[i])
    return out


def uneven_runs(n, writers):
    """n files in `writers` runs, none a multiple of 4 long (groups of 4 straddle writer changes)"""
    base = n // writers
    runs = [base + d for d in ([-2, 2, 0, 3, -3, 0] * writers)[:writers]]
    runs[-1] += n - sum(runs)
    for i in range(writers - 1):
        if runs[i] % 4 == 0:
            runs[i] += 1
            runs[-1] -= 1
    if runs[-1] % 4 == 0:
        runs[-1] -= 1
        runs[0] += 1
    assert sum(runs) == n and all(r % 4 and r > 8 for r in runs), runs
    return runs


def _ends_long_enough(order, runs, need, keep=()):
    """Swap a longer file into each run's first and last place (they hold the writer's maxima);
    the places in `keep` stay"""
    lo = 0
    for r in runs:
        for at, scan in ((lo, range(lo + 1, lo + r - 1)), (lo + r - 1, range(lo + r - 2, lo, -1))):
            if order[at] < need:
                j = next(j for j in scan if j not in keep and need <= order[j] <= 4096)
                order[at], order[j] = order[j], order[at]
        lo += r
    return order


def _add_scenarios(c, rng, with_gate):
    n = len(c.files)
    every = list(range(n))
    c.scenarios["clean"] = [(every, {})]
    c.want_rc["clean"] = 0
    if with_gate:
        first = []
        for _, lo, hi in c.runs():
            first += list(range(lo, lo + (hi - lo + 1) // 2))
        c.scenarios["regate"] = [(first, {}), (every, {})]
        c.want_rc["regate"] = 0
        _, lo, hi = c.runs()[2]
        gone = (lo + hi) // 2
        c.scenarios["gap"] = [([i for i in every if i != gone], {})]
        c.want_rc["gap"] = 13
        c.notes["gap"] = gone
    # five tampered single-page files: a tag bit in the batch's first group; the last ciphertext
    # byte of a file whose last Poly1305 piece is partial; two files of one group of four; one in
    # the last (ragged) group
    single = [i for i in every if c.lens[i] <= 4096]
    partial = next(i for i in single if 40 <= i < n - 8 and c.lens[i] % 16 and c.lens[i] > 64)
    pair = next(g for g in range(n // 2 // 4 * 4, n - 8, 4) if g != partial // 4 * 4 and
                g in single and g + 2 in single)
    assert n - 1 in single and 1 in single
    patch = {}
    for i, at, bit in ((1, -1, 0x10), (partial, -17, 0x01), (pair, -3, 0x40), (pair + 2, -20, 0x02),
                       (n - 1, -16, 0x80)):
        b = bytearray(c.files[i])
        b[at] ^= bit
        patch[i] = bytes(b)
    c.tampered = sorted(patch)
    c.scenarios["reject"] = [(every, patch)]
    c.want_rc["reject"] = 9


# ---------------------------------------------------------------------------------- GCounter
def _dot(actor, counter):
    return msgpack.packb({"actor": actor, "counter": counter}, use_bin_type=True)


def _arr_header(n):
    return bytes([0x90 | n]) if n < 16 else (b"\xdc" + n.to_bytes(2, "big") if n < 65536 else b"\xdd" + n.to_bytes(4, "big"))


def _dots_clear(rng, L, first, draw, last=()):
    """APP || Vec<Dot> || trailing bytes of exactly L bytes: the dots in `first`, then draw()'s
    while they fit, then those in `last`"""
    dots = list(first)
    size = sum(map(len, dots)) + sum(map(len, last))
    assert 16 + len(_arr_header(len(dots) + len(last))) + size <= L
    while True:
        d = draw()
        if 16 + len(_arr_header(len(dots) + len(last) + 1)) + size + len(d) > L:
            break
        dots.append(d)
        size += len(d)
    dots += list(last)
    body = _arr_header(len(dots)) + b"".join(dots)
    return APP + body + rng.randbytes(L - 16 - len(body))


# counters of each msgpack width below the writers' maxima: fixint, cc, cd, ce, cf
COUNTER_RANGES = ((0, 127), (128, 255), (256, 65535), (65536, (1 << 32) - 1), (1 << 32, (1 << 62) - 1))


def _counter_draw(rng):
    """A file's counters: seven files in ten keep one width, so every Dot of the file has one
    length (the decode's 16-lane rounds, its speculated length stale from the file before); the
    others change width from Dot to Dot (one Dot per round)."""
    fixed = rng.choice(COUNTER_RANGES) if rng.random() < 0.7 else None
    return lambda: rng.randint(*(fixed or rng.choice(COUNTER_RANGES)))


@functools.lru_cache(maxsize=None)
def gcounter_corpus(seed=20240917):
    """417 files of 6 writers (see the module docstring and tests/test_wave_run_corpus.py for
    the properties): every tail length class, long and short files in turn, runs that are no
    multiple of 4, n = 1 (mod 8); each writer's maximum (2^64 - 1 - w) the last Dot (so it is
    still pending when the file ends) of its run's first file (even w) or last file (odd w);
    three multi-page files and three files naming an actor outside
    the table inside runs."""
    rng = random.Random(seed)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(6))
    strangers = [rng.randbytes(16) for _ in range(3)]
    lens = list(range(17, 209)) + list(range(3969, 4097)) + NBLK_EDGES
    lens += [rng.randrange(209, 3969) for _ in range(411 - len(lens))]
    order = alternate_long_short(rng, lens)
    runs = uneven_runs(417, 6)
    # the inactive files, one per run, away from the run's ends: multi-page in runs 1, 3, 4,
    # foreign-actor files (a mid-sized single page) in runs 0, 2, 5
    special, lo = {}, 0
    for w, r in enumerate(runs):
        at = lo + r // 2 + w
        special[at] = ("multi", MULTI_PAGE[(1, 3, 4).index(w)]) if w in (1, 3, 4) else ("stranger", strangers[(0, 2, 5).index(w)])
        lo += r
    it = iter(order)
    order = [special[i][1] if i in special and special[i][0] == "multi" else
             (700 + 64 * (i % 5) + i % 3 if i in special else next(it)) for i in range(417)]
    order = _ends_long_enough(order, runs, 128, keep=special)
    clears, fa, vers, lo = [], [], [], 0
    for w, r in enumerate(runs):
        for v in range(r):
            i = lo + v
            ctr = _counter_draw(rng)

            def draw():
                return _dot(actors[w] if rng.random() < 0.8 else rng.choice(actors), ctr())
            first, last = [], []
            if v == (0 if w % 2 == 0 else r - 1):
                last.append(_dot(actors[w], (1 << 64) - 1 - w))
            if i in special and special[i][0] == "stranger":
                first.append(_dot(special[i][1], rng.getrandbits(40)))
            clears.append(_dots_clear(rng, order[i], first, draw, last))
            fa.append(w)
            vers.append(v)
        lo += r
    c = Corpus("gcounter", key, actors, [seal(key, x, rng) for x in clears], fa, vers, [len(x) for x in clears])
    c.notes["special"] = {i: k for i, (k, _) in special.items()}
    c.notes["strangers"] = strangers
    _add_scenarios(c, rng, with_gate=True)
    return c


# ---------------------------------------------------------------------------------- PNCounter
@functools.lru_cache(maxsize=None)
def pncounter_corpus(seed=20240918):
    """321 files of 6 writers: every length in 17..208 and 3969..4096 (ce-width ops, trailing
    bytes), long and short in turn, uneven runs; writer w's Pos maximum in its run's first file
    and its Neg maximum in the last (even w), or the other way round (odd w)."""
    rng = random.Random(seed)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(6))
    lens = list(range(17, 209)) + list(range(3969, 4097)) + [1000]
    runs = uneven_runs(len(lens), 6)
    order = _ends_long_enough(alternate_long_short(rng, lens), runs, 19 + 2 * 51)
    files, fa, vers, lo = [], [], [], 0
    for w, r in enumerate(runs):
        for v in range(r):
            L = order[lo + v]
            k = max(0, min((L - 16 - 3) // 51, 79))
            ops = [((actors[w] if rng.random() < 0.8 else rng.choice(actors), rng.randrange(1 << 16, 1 << 31)),
                    rng.choice(pm.DIRS)) for _ in range(k)]
            if v in (0, r - 1):
                d = pm.DIRS[(w + (v != 0)) % 2]
                ops[rng.randrange(k)] = ((actors[w], (1 << 32) - 1 - w), d)
            body = pm.enc_ops(ops)
            assert 16 + len(body) <= L
            files.append(seal(key, APP + body + rng.randbytes(L - 16 - len(body)), rng))
            fa.append(w)
            vers.append(v)
        lo += r
    c = Corpus("pncounter", key, actors, files, fa, vers, list(order))
    _add_scenarios(c, rng, with_gate=True)
    return c


# ---------------------------------------------------------------------------------- Orswot
@functools.lru_cache(maxsize=None)
def orswot_corpus(seed=20240919):
    """201 canonical Orswot op files (p_rm 0.2) of 7 writers, plaintexts from under 100 bytes to
    one page: 12 past kDsFuseRegion (the 16-lane pass), 12 within 64 bytes below it, the rest
    spread over 100..1983; sizes reached with trailing bytes, which from_slice ignores."""
    rng = random.Random(seed)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(7))
    n = 201
    sizes = [DS_REGION + d for d in (1, 2, 15, 16, 17, 64, 500, 1000, 1500, 2000, 2047, 2048)]
    sizes += [DS_REGION - d for d in (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64)]
    sizes += [0] * 6  # a single op, no padding: under 100 bytes
    sizes += [rng.randrange(100, DS_REGION - 64) for _ in range(n - len(sizes))]
    sizes = alternate_long_short(rng, sizes)
    per = [29] * 6 + [27]
    size_of, k = {}, 0
    for ai in range(7):
        for v in range(per[ai]):
            size_of[(ai, v)] = sizes[k]
            k += 1
    hist = _canonical_orswot(rng, actors, 29, lambda ai, v: max(1, size_of.get((ai, v), 0) // 30), 300)
    clears, fa, vers = [], [], []
    for ai, a in enumerate(actors):
        for v in range(per[ai]):
            want, ops = size_of[(ai, v)], hist[a][v]
            if want == 0:
                ops = ops[:1]
            while len(ops) > 1 and 16 + len(C.enc_orswot_ops(ops)) > want:
                ops = ops[:-1]
            body = C.enc_orswot_ops(ops)
            clears.append(APP + body + rng.randbytes(max(0, want - 16 - len(body))))
            fa.append(ai)
            vers.append(v)
    c = Corpus("orswot", key, actors, [seal(key, x, rng) for x in clears], fa, vers, [len(x) for x in clears])
    _add_scenarios(c, rng, with_gate=False)
    return c


# ---------------------------------------------------------------------------------- full grid
@functools.lru_cache(maxsize=None)
def full_grid_corpus(seed=20240920):
    """24,577 GCounter files (3 x 8,192 + 1) of 16 writers in runs of uneven length: 1-3 dots,
    every eighth file one of the long lengths of gcounter_corpus.  Scenarios clean and reject
    (four tampered files)."""
    rng = random.Random(seed)
    key = rng.randbytes(32)
    actors = sorted(rng.randbytes(16) for _ in range(16))
    n = 24577
    runs = uneven_runs(n, 16)
    long_lens = [L for L in gcounter_corpus().lens if 2048 <= L <= 4096]
    files, fa, vers, lens, i = [], [], [], [], 0
    for w, r in enumerate(runs):
        for v in range(r):
            ctr = _counter_draw(rng)

            def draw():
                return _dot(actors[w] if rng.random() < 0.8 else actors[rng.randrange(16)], ctr())
            last = [_dot(actors[w], (1 << 64) - 1 - w)] if v == (0 if w % 2 == 0 else r - 1) else []
            if i % 8 == 5 and not last:
                clear = _dots_clear(rng, long_lens[rng.randrange(len(long_lens))], [], draw)
            else:
                body = [draw() for _ in range(rng.randrange(1, 4) - len(last))] + last
                clear = APP + _arr_header(len(body)) + b"".join(body)
            files.append(seal(key, clear, rng))
            fa.append(w)
            vers.append(v)
            lens.append(len(clear))
            i += 1
    c = Corpus("gcounter", key, actors, files, fa, vers, lens)
    every = list(range(n))
    c.scenarios["clean"] = [(every, {})]
    c.want_rc["clean"] = 0
    patch = {}
    for j, at, bit in ((2, -1, 0x01), (8192 * 4 // 4 + 1, -17, 0x20), (16384 + 7, -2, 0x04), (n - 1, -16, 0x80)):
        b = bytearray(files[j])
        b[at] ^= bit
        patch[j] = bytes(b)
    c.tampered = sorted(patch)
    c.scenarios["reject"] = [(every, patch)]
    c.want_rc["reject"] = 9
    return c
