"""ce_ctx_prim_lww_reduce_keyed (k_lww_reduce_keyed and its final stage) case by case against
numpy: the helpers tests/test_gpu_lwwreg_shard.py calls in its own process, and, run as a script,
its child process under another CE_TEST_GRID_CAP:

    python lww_keyed_worker.py

runs every case of every size on cuda:0 under whatever environment it was given and prints one
JSON line per case: {"id": ..., "ok": true | false, "detail": ...}.  It exits 0 when every case ran
(whatever the verdicts, which the parent asserts one by one).

Sizes: the edges of the tile and of kLwwMaxBlocks x tile.  Cases: the records' addresses (fa, fv)
are a random permutation of distinct keys; the largest marker is tied at a tile's first and last
record, across two blocks, and at the records with the globally smallest and largest address; all
markers zero; markers of 2^64 - 1 against ones that differ from it in one 32-bit half only, with
vals that have only their high word set (a half-shuffled 64-bit lane changes the answer)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, "..", "crdt-enc_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

TILE, MAX_BLOCKS = 256, 64          # ce_lww.h kLwwTile / kLwwMaxBlocks (asserted against the library's own)
SIZES = [1, TILE - 1, TILE, TILE + 1, TILE * MAX_BLOCKS - 1, TILE * MAX_BLOCKS, TILE * MAX_BLOCKS + 1,
         2 * TILE * MAX_BLOCKS + 1]
U64 = (1 << 64) - 1
NONE = (0, 0, U64, U64)


def want(markers, vals, fa, fv):
    """largest marker, then lowest fa, fv, index; NONE when every marker is 0"""
    if not markers.any():
        return NONE
    idx = np.flatnonzero(markers == markers.max())
    i = idx[np.lexsort((idx, fv[idx], fa[idx]))[0]]
    return (int(markers[i]), int(vals[i]), int(fa[i]), int(fv[i]))


def addresses(rng, n):
    """n distinct (fa, fv) in random order: a few writers, versions over the whole u64 range"""
    fa = rng.integers(0, 7, n, dtype=np.uint32)
    fv = rng.permutation(n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)     # distinct (odd multiplier)
    fv[rng.integers(0, n)] = np.uint64(U64)
    assert len(set(zip(fa.tolist(), fv.tolist()))) == n
    return fa, fv


def cases(n):
    """(id, markers, vals, fa, fv)"""
    rng = np.random.default_rng(1000 + n)
    fa, fv = addresses(rng, n)
    vals = rng.integers(1, 1 << 32, n, dtype=np.uint64) << np.uint64(32)          # the high word only
    low = rng.integers(1, 1 << 20, n, dtype=np.uint64)                            # the background markers
    order = np.lexsort((fv, fa))                                                  # by address
    first, last = int(order[0]), int(order[-1])
    G = min(-(-n // TILE), MAX_BLOCKS)

    def tied(name, at, top=np.uint64(1 << 40)):
        m = low.copy()
        m[[i for i in at if 0 <= i < n]] = top
        return (name, m, vals, fa, fv)
    out = [("random", rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + np.uint64(1), vals, fa, fv),
           tied("tile-first-last", [0, TILE - 1]),
           tied("last-tile-first-last", [(n - 1) // TILE * TILE, n - 1]),
           tied("two-blocks", [TILE - 1, TILE, TILE * G, TILE * G + 1, n - 1]),
           tied("smallest-largest-address", [first, last]),
           tied("everywhere", range(n)),
           ("all-zero", np.zeros(n, np.uint64), vals, fa, fv)]
    # 2^64 - 1 against markers that share one of its halves
    m = np.where(rng.integers(0, 2, n) == 1, np.uint64(0xFFFFFFFF00000000), np.uint64(0x00000000FFFFFFFF))
    m = m.astype(np.uint64)
    m[[first, last, n // 2]] = np.uint64(U64)
    out.append(("u64-max-halves", m, vals, fa, fv))
    # the same address twice (Storage cannot produce it): the lower index
    if n >= 2:
        fa2, fv2 = fa.copy(), fv.copy()
        fa2[n - 1], fv2[n - 1] = fa2[0], fv2[0]
        out.append(tied("same-address", [0, n - 1])[:3] + (fa2, fv2))
    return out


def run_case(ctx, n, case):
    import torch
    name, markers, vals, fa, fv = case
    rec = np.empty(2 * n, np.uint64)
    rec[0::2], rec[1::2] = markers, vals
    d_rec = torch.from_numpy(rec.view(np.int64)).to("cuda:0")
    d_fa = torch.from_numpy(fa.view(np.int32)).to("cuda:0")
    d_fv = torch.from_numpy(fv.view(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    got = ctx.prim_lww_reduce_keyed(d_rec.data_ptr(), d_fa.data_ptr(), d_fv.data_ptr(), n)
    w = want(markers, vals, fa, fv)
    ok = tuple(got) == w
    return {"id": "%d-%s" % (n, name), "ok": ok, "detail": "" if ok else "got %r, want %r" % (tuple(got), w)}


def run_size(ctx, n):
    return [run_case(ctx, n, c) for c in cases(n)]


def main():
    import crdtenc
    ctx = crdtenc.Context(0)
    for n in SIZES:
        for v in run_size(ctx, n):
            print(json.dumps(v), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
