"""Poly1305 edge vectors for every open and seal kernel (tests/test_poly_edges_model.py on the
CPU, tests/test_gpu_poly_edges.py on the GPU).

Every AEAD tag of the library comes from the radix-2^26 Poly1305 of crdt-enc_amd/csrc/ce_device.h
(mulmod, mac5 / reduce5, carry5, poly_tag, poly_check, poly_aux), under each kernel's own
evaluation order and tail.  Random ciphertexts reach the places where that arithmetic can go wrong
with probability 2^-100 or less, so the vectors here are built to land on them.  For a fixed key
and nonce r and s are known; the MAC input is the ciphertext, which a test may choose (no AAD,
enc_data is opaque), and rmp_serde::from_slice ignores what follows the Vec, so a whole 16-byte
block of an op file's plaintext tail is free: craft() solves for the one block that makes the
fully reduced Horner sum h equal a target T.  The same files are valid op files, so they go
through the accept path of every fused kernel and not only through decrypt.

The reference here is big-integer arithmetic: poly_h is the Horner sum mod p = 2^130 - 5 over the
ciphertext padded to 16 bytes and le64(0) || le64(len), tag = (h + s) mod 2^128.  (subkey, r, s)
come from oracle.hchacha20 and oracle.chacha20_block, both pinned to RFC vectors in
tests/test_oracle.py.  Nothing here calls the oracle's or the product's Poly1305.

What each target is for (T is the fully reduced h; a kernel holds h unreduced until its tail):

  0 .. 5, p-6 .. p-1     the final conditional subtraction of p.  For a true h in [0, 5) a kernel
                         holds h or h + p, and g = h + 5 - 2^130 changes sign between p-6 | p-5
                         and again at 5 (= p + 5 - 2^130 + p): a missed subtraction returns
                         tag - 5, one too many tag + 5.  Files with T in 0..4 and p-5..p-1
                         therefore have reject twins carrying tag - 5, tag + 5 and tag + 1.
  2^k - 5, 2^k - 1, 2^k  k = 26, 52, 78, 104: the limb boundaries.  h + 5 carries out of limb
                         k/26 - 1 exactly from 2^k - 5 on, 2^k - 1 is all-ones limbs below the
                         boundary (the carry5 / poly_check ripple), 2^k the single bit above it.
  2^k - 1, 2^k           k = 32, 64, 96, 128: the 32-bit word boundaries of the limbs-to-words
                         packing and of the (h + s) add in poly_tag; 2^128 - 1 and 2^128 are the
                         128-bit truncation.
  2^128 + 1, 2^129       bits 128 and 129 of h set: they must not reach the tag.
  tag=0, tag=1, tag=max  h mod 2^128 = -s, 1 - s, -1 - s: the (h + s) carry runs out of the top
                         word (poly_tag), and ts = tag - s borrows through every word (poly_aux).
  tag=s, tag=s-1         h mod 2^128 = 0 (h = 3 * 2^128) and 2^128 - 1 (h = 2^129 - 1): ts = 0
                         and ts = all ones.
  borrow1 .. borrow3     tag word i equals s word i while the words below are smaller: the borrow
                         of tag - s runs into an equal word (ts word i = 0xffffffff, borrow on).
  heavy                  an r whose two highest free bits are set in all five limbs (masks
                         0x3000000 four times and 0xc0000; one nonce in 1024), with the whole
                         free tail's ciphertext 0xff, and a second file with an all-zero tail:
                         the largest products, for the stated bounds ("h limbs < 2^28", "up to 64
                         products fit a column", "limbs < 2^31" of the unreduced lane sums).

The crafted block is in turn the first free tail block, the last full block and the one before
it; the kernels deal blocks to lanes from the end, so these land in different lanes and slots.
"""
import functools
import random

import msgpack

import oracle
import pncounter_model as pm
import wave_run_corpus as W
from oracle import crdts as C

P = (1 << 130) - 5
M128 = (1 << 128) - 1
CLAMP = 0x0ffffffc0ffffffc0ffffffc0fffffff
BOX_VERSION = bytes.fromhex("c7f269be0ff54a7799c37c23c96d5cb4")
HEAVY_MASKS = (0x3000000, 0x3000000, 0x3000000, 0x3000000, 0xc0000)

# plaintext lengths of the single-page corpora: k_open_fold_v3's delta = 4 ceil(L / 64) -
# ceil(L / 16) is 1, 3, 0, 0, 3, 3, 2, 0, 0 for them, the last piece full (2048, 4096) or partial;
# 2047 and 2049 are kDsFuseRegion -+ 1 for the dot-set opens
LENS = (100, 129, 2047, 2048, 2049, 4033, 4049, 4081, 4096)
MULTI_PAGE = W.MULTI_PAGE
MULTI_SEGMENT = 40000
# (65 << 14) + 4097 is 66 Poly1305 segments of 16 KiB: k_finalize_multi's lanes chain a second
# segment in r^(64 S) only from 66 on ((1 << 20) + 17 is 65)
AEAD_LONG = (16384 - 16, 16384 + 1, 70000, (1 << 20) + 17, (65 << 14) + 4097)
SEAL_LENS = (16, 4096, 16384 + 1, 70000, (1 << 20) + 17, (65 << 14) + 4097)


def delta(L):
    return 4 * ((L + 63) // 64) - (L + 15) // 16


# ---------------------------------------------------------------------------- the reference
def keys(key, nonce):
    """-> (subkey, 12-byte nonce, r clamped, s) of XChaCha20-Poly1305"""
    subkey = oracle.hchacha20(key, nonce[:16])
    n12 = bytes(4) + nonce[16:]
    b0 = oracle.chacha20_block(subkey, 0, n12)
    return subkey, n12, int.from_bytes(b0[:16], "little") & CLAMP, int.from_bytes(b0[16:32], "little")


def keystream(subkey, n12, n):
    return b"".join(oracle.chacha20_block(subkey, 1 + i, n12) for i in range((n + 63) // 64))[:n]


def xor(a, b):
    assert len(a) == len(b)
    return (int.from_bytes(a, "little") ^ int.from_bytes(b, "little")).to_bytes(len(a), "little")


def mac_blocks(ct):
    """The MAC input's blocks as integers, each with its 2^128 bit: ct padded to 16 bytes, then
    le64(0) || le64(len)"""
    out = [int.from_bytes(ct[i:i + 16], "little") | 1 << 128 for i in range(0, len(ct), 16)]
    out.append(len(ct) << 64 | 1 << 128)
    return out


def horner(r, blocks):
    h = 0
    for m in blocks:
        h = (h + m) * r % P
    return h


def poly_h(r, ct):
    return horner(r, mac_blocks(ct))


def tag_of(r, s, ct):
    return (poly_h(r, ct) + s) & M128


def poly1305(key, msg):
    """Plain Poly1305 (RFC 8439 2.5) of msg under key = r || s, r clamped here: a partial last
    block gets its 1 bit after its last byte and no padding.  -> the 16-byte tag"""
    r, s = int.from_bytes(key[:16], "little") & CLAMP, int.from_bytes(key[16:32], "little")
    blocks = [int.from_bytes(msg[i:i + 16], "little") | 1 << (8 * len(msg[i:i + 16])) for i in range(0, len(msg), 16)]
    return ((horner(r, blocks) + s) & M128).to_bytes(16, "little")


def limbs(x):
    return [(x >> (26 * i)) & 0x3ffffff for i in range(5)]


def is_heavy(r):
    return all(l & m == m for l, m in zip(limbs(r), HEAVY_MASKS))


def craft(r, ct, j, T, rng, others):
    """ct with its full block j replaced so that poly_h(r, ct) == T.  With e the blocks from j to
    the end (the length block included), c = (T - A) r^-e mod p, A the sum with block j's bytes
    zeroed; c fits 128 bits one time in four, otherwise one of `others` (byte ranges (lo, hi),
    each inside one block, free to change) is redrawn.  The sum is linear in every block, so a
    redraw moves A by (new - old) r^e' and no retry walks the file again.
    -> (ct, redraws)"""
    assert 16 * (j + 1) <= len(ct) and all(lo // 16 == (hi - 1) // 16 != j for lo, hi in others)
    b = bytearray(ct)
    b[16 * j:16 * j + 16] = bytes(16)
    n = (len(b) + 15) // 16 + 1
    A = poly_h(r, bytes(b))
    inv = pow(r, -(n - j), P)
    for redraws in range(65):
        c = (T - A) * inv % P
        if c >> 128 == 0:
            b[16 * j:16 * j + 16] = c.to_bytes(16, "little")
            return bytes(b), redraws
        assert others, "no free bytes to redraw"
        lo, hi = others[redraws % len(others)]
        new = rng.randbytes(hi - lo)
        d = int.from_bytes(new, "little") - int.from_bytes(b[lo:hi], "little")
        A = (A + (d << (8 * (lo % 16))) * pow(r, n - lo // 16, P)) % P
        b[lo:hi] = new
    raise AssertionError("no 128-bit block within 64 redraws")


# ---------------------------------------------------------------------------- targets
def fixed_targets():
    t = {}
    for v in range(6):
        t["%d" % v] = v
    for d in range(6, 0, -1):
        t["p-%d" % d] = P - d
    for k in (26, 52, 78, 104):
        t["2^%d-5" % k], t["2^%d-1" % k], t["2^%d" % k] = (1 << k) - 5, (1 << k) - 1, 1 << k
    for k in (32, 64, 96, 128):
        t["2^%d-1" % k], t["2^%d" % k] = (1 << k) - 1, 1 << k
    t["2^128+1"], t["2^129"] = (1 << 128) + 1, 1 << 129
    return t


S_TARGETS = ("tag=0", "tag=1", "tag=max", "tag=s", "tag=s-1", "borrow1", "borrow2", "borrow3")
TARGETS = tuple(fixed_targets()) + S_TARGETS
TWINNED = tuple(str(v) for v in range(5)) + tuple("p-%d" % d for d in range(5, 0, -1))
TWIN_DELTAS = (-5, 5, 1)


def usable(name, s):
    """borrow<i> needs nonzero words of s below word i"""
    return not name.startswith("borrow") or s & ((1 << (32 * int(name[-1]))) - 1) != 0


def target(name, s, rng):
    """-> T for a target name; those chosen from s fix h mod 2^128 (see the module docstring)"""
    fixed = fixed_targets()
    if name in fixed:
        return fixed[name]
    if name == "tag=s":
        return 3 << 128
    if name == "tag=s-1":
        return (1 << 129) - 1
    if name.startswith("borrow"):
        i = int(name[-1])
        low = (1 << (32 * i)) - 1
        tag = (rng.getrandbits(128) & ~((1 << (32 * (i + 1))) - 1) & M128) | (s & (0xffffffff << (32 * i))) \
            | rng.randrange(s & low)
    else:
        tag = {"tag=0": 0, "tag=1": 1, "tag=max": M128}[name]
    return ((tag - s) & M128) + (rng.randrange(3) << 128)


def target_holds(name, T, s, tag):
    """What a vector named `name` must satisfy, from T, s and the tag alone"""
    fixed = fixed_targets()
    if name in fixed:
        return T == fixed[name]
    if name.startswith("borrow"):
        i = int(name[-1])
        low = (1 << (32 * i)) - 1
        return (tag >> (32 * i)) & 0xffffffff == (s >> (32 * i)) & 0xffffffff and tag & low < s & low
    return tag == {"tag=0": 0, "tag=1": 1, "tag=max": M128, "tag=s": s, "tag=s-1": (s - 1) & M128}[name]


# ---------------------------------------------------------------------------- vectors
class Vector:
    """One ciphertext under (key, nonce): name (a target, "heavy-ff", "heavy-00", "plain" or
    "twin<d>"), T (None unless crafted), j (the crafted block), r, s, ct and the reference's tag
    (an integer); twins carry tag + d and keep `of`, the vector they were made from."""

    def __init__(self, name, key, nonce, ct, r, s, T=None, j=None, redraws=0, tag=None, of=None):
        self.name, self.key, self.nonce, self.ct, self.r, self.s = name, key, nonce, ct, r, s
        self.T, self.j, self.redraws, self.of = T, j, redraws, of
        self.tag = tag_of(r, s, ct) if tag is None else tag
        self._pt = None

    def sealed(self):
        """ct || tag"""
        return self.ct + self.tag.to_bytes(16, "little")

    def box(self):
        """The EncHandler's VersionBytes(EncBox{nonce, enc_data})"""
        return msgpack.packb([BOX_VERSION, msgpack.packb({"nonce": self.nonce, "enc_data": self.sealed()},
                                                         use_bin_type=True)], use_bin_type=True)

    def file(self):
        return W.CORE_VERSION + self.box()

    def plaintext(self):
        """ct XOR keystream (computed once)"""
        if self._pt is None:
            subkey, n12, _, _ = keys(self.key, self.nonce)
            self._pt = xor(self.ct, keystream(subkey, n12, len(self.ct)))
        return self._pt

    def twins(self):
        return [Vector("twin%+d" % d, self.key, self.nonce, self.ct, self.r, self.s, tag=(self.tag + d) & M128, of=self)
                for d in TWIN_DELTAS]


def free_ranges(L, free_from, j):
    """The byte ranges craft() may redraw: every full block of the free tail but j, and the
    partial last piece"""
    first = -(-free_from // 16)
    out = [(16 * k, 16 * k + 16) for k in range(first, L // 16) if k != j]
    if L % 16 and max(free_from, L // 16 * 16) < L:
        out.append((max(free_from, L // 16 * 16), L))
    return out[:8] + out[-8:] if len(out) > 16 else out


def crafted(rng, key, name, head, L, where, nonce=None):
    """A ciphertext of L bytes whose plaintext begins with `head`, the rest free, crafted to the
    target `name` in the block `where`: "first" (the first free block), "last" (the last full
    block), "prev" (the one before it; "last" where that is not free) or a block index."""
    first, last = -(-len(head) // 16), L // 16 - 1
    assert first <= last, (len(head), L)
    j = where if isinstance(where, int) else {"first": first, "last": last, "prev": last - 1 if last > first else last}[where]
    assert first <= j <= last
    others = free_ranges(L, len(head), j)
    for _ in range(64 if others else 4096):
        n = nonce or rng.randbytes(24)
        subkey, n12, r, s = keys(key, n)
        if not usable(name, s) or not r:
            assert nonce is None
            continue
        ct = xor(head, keystream(subkey, n12, len(head))) + rng.randbytes(L - len(head))
        T = target(name, s, rng)
        if others:
            ct, redraws = craft(r, ct, j, T, rng, others)
            return Vector(name, key, n, ct, r, s, T, j, redraws)
        # a single free block: nothing to redraw but the nonce
        try:
            ct, _ = craft(r, ct, j, T, rng, others)
            return Vector(name, key, n, ct, r, s, T, j, 0)
        except AssertionError:
            assert nonce is None
    raise AssertionError("no vector for %s at %d" % (name, L))


def plain(rng, key, head, L, name="plain"):
    n = rng.randbytes(24)
    subkey, n12, r, s = keys(key, n)
    return Vector(name, key, n, xor(head, keystream(subkey, n12, len(head))) + rng.randbytes(L - len(head)), r, s)


@functools.lru_cache(maxsize=None)
def heavy_nonce(key, seed=1305):
    """A nonce whose r has the two highest free bits of all five limbs set"""
    rng = random.Random(seed)
    for _ in range(1 << 16):
        n = rng.randbytes(24)
        if is_heavy(keys(key, n)[2]):
            return n
    raise AssertionError("no heavy r in 2^16 nonces")


def heavy(key, head, L, tail):
    """The vector under the heavy nonce whose free tail's ciphertext is the byte `tail` throughout"""
    n = heavy_nonce(key)
    subkey, n12, r, s = keys(key, n)
    return Vector("heavy-" + tail.hex(), key, n, xor(head, keystream(subkey, n12, len(head))) + tail * (L - len(head)), r, s)


# ---------------------------------------------------------------------------- corpora
def _head(kind, rng, actors, w, i, ctr):
    """APP || a Vec of one op whose effect no other file of the corpus has: a Dot of an actor of
    its own (the counters), an Add of a member of its own by the writer's next dot (Orswot)"""
    if kind == "gcounter":
        lo, hi = W.COUNTER_RANGES[i % 5]
        return W.APP + W._arr_header(1) + W._dot(actors[i], rng.randint(max(lo, 1), hi))
    if kind == "pncounter":
        return W.APP + pm.enc_ops([((actors[i], rng.randrange(1 << 16, 1 << 32)), pm.DIRS[i % 2])])
    return W.APP + C.enc_orswot_ops([("Add", (actors[w], ctr), [rng.getrandbits(63) | 1 << 62])])


def _corpus(kind, seed, plan, writers, n_fresh):
    """plan: [(target name | "heavy", L, where)].  The base batch is the crafted files in writer
    order, then (the writers' next versions) the twins with fresh clean files among them."""
    rng = random.Random(seed)
    key = rng.randbytes(32)
    n_twinned = sum(1 for name, _, _ in plan if name in TWINNED)
    n_clean = sum(2 if name == "heavy" else 1 for name, _, _ in plan)
    n_second = 3 * n_twinned + n_fresh
    # the writers' own actors come first; the counters' files each name one further actor
    actors = sorted(rng.randbytes(16) for _ in range(writers))
    if kind != "orswot":
        actors += sorted(rng.randbytes(16) for _ in range(n_clean + n_second))
    vecs, fa, vers = [], [], []
    nxt = [0] * writers

    def place(v, w):
        vecs.append(v)
        fa.append(w)
        vers.append(nxt[w])
        nxt[w] += 1

    def head(w):
        return _head(kind, rng, actors, w, writers + len(vecs), nxt[w] + 1)

    done = 0
    for name, L, where in plan:
        w = done * writers // n_clean
        if name == "heavy":
            for tail in (b"\xff", b"\x00"):
                w = done * writers // n_clean
                place(heavy(key, head(w), L, tail), w)
                done += 1
        else:
            place(crafted(rng, key, name, head(w), L, where), w)
            done += 1
    assert done == n_clean == len(vecs)
    second = [t for v in vecs if v.name in TWINNED for t in v.twins()]
    step = len(second) // n_fresh
    for k in range(n_fresh):  # fresh clean files among the twins, one of them first
        second.insert(k * (step + 1), None)
    lens = [L for name, L, _ in plan for _ in range(2 if name == "heavy" else 1)]
    for k, t in enumerate(second):
        w = k * writers // len(second)
        place(t if t else plain(rng, key, head(w), LENS[k % len(LENS)]), w)
        lens.append(len(vecs[-1].ct))
    c = W.Corpus(kind, key, actors, [v.file() for v in vecs], fa, vers, lens)
    c.vectors = vecs
    every = list(range(len(vecs)))
    c.scenarios["clean"] = [(every[:n_clean], {})]
    c.want_rc["clean"] = 0
    c.scenarios["reject"] = [(every[:n_clean], {}), (every[n_clean:], {})]
    c.want_rc["reject"] = 9
    c.tampered = [i - n_clean for i in every[n_clean:] if vecs[i].of is not None]
    return c


def single_page_plan():
    """Every target at three lengths (nine lengths, three apart) and rotating blocks, and the
    heavy pair at 4096 (the longest single page) and at 4081 (a partial last piece)"""
    plan = []
    for ti, name in enumerate(TARGETS):
        for k in range(3):
            plan.append((name, LENS[(ti + 3 * k) % 9], ("first", "last", "prev")[(ti + k) % 3]))
    plan.insert(len(plan) // 3, ("heavy", 4096, None))
    plan.insert(2 * len(plan) // 3, ("heavy", 4081, None))
    return plan


@functools.lru_cache(maxsize=None)
def corpus(kind):
    """The single-page corpus of "gcounter", "pncounter" or "orswot": 130 crafted and heavy files
    of 6 writers, then 90 twins and 30 fresh files as the writers' next versions"""
    return _corpus(kind, {"gcounter": 1305001, "pncounter": 1305002, "orswot": 1305003}[kind],
                   single_page_plan(), 6, 30)


@functools.lru_cache(maxsize=None)
def multi_page_corpus():
    """Crafted GCounter files of 4097, 5000 and 9000 plaintext bytes (six targets each, the block
    rotating; "prev" and "last" fall in the last page, "first" in the first) and the heavy pair at
    9000: more than a page and one Poly1305 segment, whose tag the segment kernel computes itself.
    Three more of 40000 bytes, three segments, for k_finalize_multi behind an ingest.  Then the
    twins of those with T = 0, 4, p-5, p-1."""
    plan = []
    for ti, name in enumerate(("0", "4", "p-5", "p-1", "tag=0", "2^104-5")):
        for k, L in enumerate(MULTI_PAGE):
            plan.append((name, L, ("first", "last", "prev")[(ti + k) % 3]))
    plan.insert(7, ("heavy", 9000, None))
    for k, name in enumerate(("0", "p-1", "tag=0")):
        plan.insert(5 * k + 2, (name, MULTI_SEGMENT, ("last", "first", "prev")[k]))
    return _corpus("gcounter", 1305004, plan, 3, 6)


@functools.lru_cache(maxsize=None)
def aead_vectors():
    """Ciphertexts for Context.decrypt_batch and Context.encrypt under one key, random but for
    the crafted block: lengths 0 (a bare tag), 16 and 4096, and the long lengths on both sides of
    one 16 KiB Poly1305 segment, of several segments and of 65 and 66 (k_finalize_multi), each
    crafted to 0, p-1 and tag=0 once in the first segment (block 1) and once in the last full
    block (the last segment's, where that has one), with one heavy file.  -> (key, [Vector])"""
    rng = random.Random(1305005)
    key = rng.randbytes(32)
    out = [plain(rng, key, b"", 0, name="empty")]
    for name in ("0", "p-1", "tag=0"):
        out.append(crafted(rng, key, name, b"", 16, 0))
        out.append(crafted(rng, key, name, b"", 4096, "first" if name == "0" else "last"))
    for L in AEAD_LONG:
        for name in ("0", "p-1", "tag=0"):
            out.append(crafted(rng, key, name, b"", L, 1))
            out.append(crafted(rng, key, name, b"", L, "last"))
        out.append(heavy(key, b"", L, b"\xff"))
    return key, out
