"""CPU statement of ce_core_orswot_rm_members[_device] (include/crdtenc.h): a member column turned
into one Rm op a member, each carrying the member's entry clock as the state holds it before the
call, the ops cut into op files, and the expected lengths and file bytes.

TEST INFRASTRUCTURE ONLY.  Built on oracle/crdts.py (VClock, enc_orswot_ops) and the oracle's
Cryptor::encrypt; nothing here is computed by the code under test.
"""
from oracle import crdts as C

from gset_write_model import APP, CORE_VERSION, WIDTH_BYTES, member_of_width, offsets, sealed_len, width  # noqa: F401

LIVE_ONLY = 1
DEFAULT_OPS_PER_FILE = 16
U64 = (1 << 64) - 1


def hdr(cnt):
    """an array header: fixarray up to 15, array16 above"""
    return 1 if cnt <= 15 else 3


def hm(k):
    """a map header: fixmap up to 15 entries, map16 up to 65,535, map32 above"""
    return 1 if k <= 15 else 3 if k <= 65535 else 5


def op_len(clock, member):
    """81 a2 Rm 82 a5 clock 81 a4 dots (17) | map header | k x (c4 10 <16> counter) | a7 members 91
    (9) | member"""
    return 26 + hm(len(clock.dots)) + sum(18 + width(c) for c in clock.dots.values()) + width(member)


def file_len(vec):
    """the clear text of one ops vector: the data version, the Vec's header, the ops"""
    return 16 + hdr(len(vec)) + sum(op_len(op[1], op[2][0]) for op in vec)


def ops(col, state, flags=0):
    """one op a member, every clock read from `state` as it stands (a copy: applying the ops does
    not change the later ones); LIVE_ONLY: only the first occurrence of each member the state holds"""
    out, seen = [], set()
    for m in col:
        e = state.entries.get(m)
        if flags & LIVE_ONLY:
            if e is None or m in seen:
                continue
            seen.add(m)
        out.append(("Rm", C.VClock(e.dots) if e is not None else C.VClock(), [m]))
    return out


def cut(col, opf, state, flags=0):
    """the ops vectors: ops(col, state, flags) in order, opf (0: 16) an ops vector"""
    k = opf or DEFAULT_OPS_PER_FILE
    o = ops(col, state, flags)
    return [o[i:i + k] for i in range(0, len(o), k)]


def clear_text(vec):
    return APP + C.enc_orswot_ops(vec)


def files(oracle, key, nonces, vectors):
    """file i = CURRENT_VERSION || Cryptor::encrypt(APP || to_vec_named(vector_i)) under nonce i"""
    out = []
    for nonce, vec in zip(nonces, vectors):
        st, enc = oracle.cryptor_encrypt(key, nonce, clear_text(vec))
        assert st == 0
        out.append(CORE_VERSION + enc)
    return out


def sizes(vectors):
    """(n_ops, n_files, bytes) of a call that writes `vectors`"""
    return sum(len(v) for v in vectors), len(vectors), sum(16 + sealed_len(file_len(v)) for v in vectors)
