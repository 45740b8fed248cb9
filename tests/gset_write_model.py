"""CPU statement of ce_core_gset_apply_members[_device] (include/crdtenc.h): a member column cut
into op files, the CE_GSET_APPLY_NEW_ONLY filter, the expected file bytes and the worst-case bound.

TEST INFRASTRUCTURE ONLY.  Built on tests/gset_model.py (enc_ops, Core.apply_ops) and the oracle's
Cryptor::encrypt; nothing here is computed by the code under test.
"""
import gset_model as gm

APP = bytes.fromhex("aadfd5a66e194b24a8024fa27c72f20c")
CORE_VERSION = bytes.fromhex("e834d789101b463498239de990a9051f")   # crdt-enc/src/lib.rs:26
FILE_MEMBERS = 453      # (4096 - 16 - 3) // 9: cf members whose clear text still fits one page
PAGE = 4096
NEW_ONLY = 1
WIDTH_BYTES = (1, 2, 3, 5, 9)
# the smallest and largest member of every width, and the sentinels next to them
WIDTH_EDGES = [0, 127, 128, 255, 256, 65535, 65536, (1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 2, (1 << 64) - 1]


def width(m):
    return 1 if m <= 0x7f else 2 if m <= 0xff else 3 if m <= 0xffff else 5 if m <= 0xffffffff else 9


def member_of_width(rng, w):
    lo, hi = {1: (0, 1 << 7), 2: (1 << 7, 1 << 8), 3: (1 << 8, 1 << 16), 5: (1 << 16, 1 << 32),
              9: (1 << 32, 1 << 64)}[w]
    return rng.randrange(lo, hi)


def per_file_of(per_file):
    return FILE_MEMBERS if per_file == 0 else per_file


def cut(col, per_file):
    """the column in order, per_file members a vector, the last may be shorter"""
    pf = per_file_of(per_file)
    return [list(col[i:i + pf]) for i in range(0, len(col), pf)]


def new_only(col, state):
    """with_state(contains) then apply_ops: the distinct members the set does not hold, ascending"""
    return sorted(set(col) - set(state))


def clear_text(chunk):
    return APP + gm.enc_ops(chunk)


def bin_hdr(n):
    return 2 if n <= 0xff else 3 if n <= 0xffff else 5


def sealed_len(clear_len):
    """the canonical envelope of EncHandler::encrypt (xchacha lib.rs:59-67) around clear_len bytes"""
    ct = clear_len + 16
    box = 1 + 6 + 2 + 24 + 9 + bin_hdr(ct) + ct
    return 1 + 2 + 16 + bin_hdr(box) + box


def bound(n, per_file):
    """(max_files, max_bytes): every member 9 bytes wide"""
    pf = per_file_of(per_file)
    full, rem = divmod(n, pf)

    def file_len(cnt):
        return 16 + sealed_len(16 + (1 if cnt <= 15 else 3) + 9 * cnt)
    return full + (1 if rem else 0), full * file_len(pf) + (file_len(rem) if rem else 0)


def files(oracle, key, nonces, chunks):
    """file i = CURRENT_VERSION || Cryptor::encrypt(APP || to_vec_named(chunk_i)) under nonce i"""
    out = []
    for nonce, ch in zip(nonces, chunks):
        st, enc = oracle.cryptor_encrypt(key, nonce, clear_text(ch))
        assert st == 0
        out.append(CORE_VERSION + enc)
    return out


def offsets(fs):
    o = [0]
    for f in fs:
        o.append(o[-1] + len(f))
    return o
