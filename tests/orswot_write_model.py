"""CPU statement of ce_core_orswot_add_members[_device] (include/crdtenc.h): a member column cut
into Add ops by one actor and the ops into op files, the expected file bytes, the one-page rule and
the worst-case bound.

TEST INFRASTRUCTURE ONLY.  Built on oracle/crdts.py (enc_orswot_ops, dec_ops) and the oracle's
Cryptor::encrypt; nothing here is computed by the code under test.
"""
from oracle import crdts as C

from gset_write_model import (APP, CORE_VERSION, PAGE, WIDTH_BYTES, WIDTH_EDGES, member_of_width, offsets,  # noqa: F401
                              sealed_len, width)

FUSE_REGION = 2048      # clear text the readers' fused open decodes in LDS (kDsFuseRegion)
U64 = (1 << 64) - 1


def hdr(cnt):
    """an array header: fixarray up to 15, array16 above"""
    return 1 if cnt <= 15 else 3


def op_len(counter, members):
    """81 a3 Add 82 a3 dot 82 a5 actor c4 10 <16> a7 counter (43) | counter | a7 members (8) |
    header | members"""
    return 51 + width(counter) + hdr(len(members)) + sum(width(m) for m in members)


def op_bound(cnt):
    return 60 + hdr(cnt) + 9 * cnt


def file_bound(ops, per_op):
    """the worst-case clear text of a file of `ops` ops of per_op members"""
    return 16 + hdr(ops) + ops * op_bound(per_op)


def shape(per_op, ops_per_file):
    """the normalised (per_op, ops_per_file), or None when a file may pass one page"""
    po = per_op or 1
    if ops_per_file:
        k = ops_per_file
    elif po == 1:
        k = max(k for k in range(1, 60) if file_bound(k, 1) <= FUSE_REGION)
    else:
        fits = [k for k in range(1, PAGE) if file_bound(k, po) <= PAGE]
        k = max(fits) if fits else 0
    if k == 0 or file_bound(k, po) > PAGE:
        return None
    return po, k


def cut(col, per_op, ops_per_file, c0, actor):
    """the ops vectors: op j = Add { dot: (actor, c0 + 1 + j), members: the j-th per_op members }"""
    po, k = shape(per_op, ops_per_file)
    ops = [("Add", (actor, c0 + 1 + j), list(col[i:i + po])) for j, i in enumerate(range(0, len(col), po))]
    return [ops[i:i + k] for i in range(0, len(ops), k)]


def clear_text(vec):
    return APP + C.enc_orswot_ops(vec)


def bound(n, per_op, ops_per_file):
    """(max_ops, max_files, max_bytes): every counter and member 9 bytes wide; None past the rule"""
    s = shape(per_op, ops_per_file)
    if s is None:
        return None
    po, k = s
    n_ops = -(-n // po)
    nf = -(-n_ops // k)
    if nf == 0:
        return 0, 0, 0
    rem = n % po
    last_ops = n_ops - (nf - 1) * k
    last = 16 + hdr(last_ops) + (last_ops - 1) * op_bound(po) + op_bound(rem or po)
    return n_ops, nf, (nf - 1) * (16 + sealed_len(file_bound(k, po))) + 16 + sealed_len(last)


def files(oracle, key, nonces, vectors):
    """file i = CURRENT_VERSION || Cryptor::encrypt(APP || to_vec_named(vector_i)) under nonce i"""
    out = []
    for nonce, vec in zip(nonces, vectors):
        st, enc = oracle.cryptor_encrypt(key, nonce, clear_text(vec))
        assert st == 0
        out.append(CORE_VERSION + enc)
    return out
