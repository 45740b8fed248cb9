#!/usr/bin/env python3
"""When the waves of the fused open (k_open_fold_v3) end, on the bench-shaped batch.

Runs bench.py's C2 workload (4096 writers x 256 versions = 1,048,576 op files) for a few untimed
steps, then one step with CE_TEST_WAVE_STAMPS=1: every wave of the fused open records the 100 MHz
reference clock when it enters and leaves its loop over the files and its hardware id
(ce_ctx_wave_stamps).  Prints, relative to the kernel's span (first wave in -> last wave out):

  - the distribution of the waves' end times (how long before the last wave each one ended),
  - the same by XCD,
  - the same by the older and the younger wave of each SIMD (the kernel runs two waves per SIMD;
    the one that entered first is the older, the lower wave slot on a tie),
  - the residency: a wave's mean time in the loop over the span.

    python3 tools/wave_ends.py [--versions 256] [--label TEXT] > profiles/wave_ends.txt

CRDTENC_LIB selects the build, as for bench.py."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "crdt-enc_amd"))

import torch  # noqa: E402

import bench  # noqa: E402
import crdtenc  # noqa: E402


def hw_fields(hw):
    """HW_ID | XCC_ID << 32 -> dict of arrays (gfx9 HW_ID layout: wave 3:0, SIMD 5:4, CU 11:8,
    SH 12, SE 15:13)"""
    lo = hw & 0xffffffff
    return {"wave": lo & 15, "simd": (lo >> 4) & 3, "cu": (lo >> 8) & 15, "sh": (lo >> 12) & 1,
            "se": (lo >> 13) & 7, "xcd": (hw >> 32) & 15}


def pct(x):
    return " ".join("%5.1f" % v for v in np.percentile(x, [0, 1, 10, 25, 50, 75, 90, 99, 100]))


def report(st, label, out=sys.stdout):
    t_in, t_out = st[:, 0].astype(np.int64), st[:, 1].astype(np.int64)
    f = hw_fields(st[:, 2])
    t0, t1 = t_in.min(), t_out.max()
    span = float(t1 - t0)
    early = 100.0 * (t1 - t_out) / span          # ended this many % of the span before the last wave
    res = (t_out - t_in) / span
    w = out.write
    w("# k_open_fold_v3 wave stamps, 100 MHz ticks; %s\n" % label)
    w("waves %d  span %.1f us  waves entering within %.1f us of the first\n" % (
        len(st), span / 100.0, float(np.percentile(t_in - t0, 99)) / 100.0))
    w("residency (mean time in the loop / span): %.3f\n" % res.mean())
    w("ended before the last wave, % of span\n")
    w("  percentile     0     1    10    25    50    75    90    99   100\n")
    w("  all        %s\n" % pct(early))
    w("  waves ending within 2%% of the last: %d of %d; more than 10%% before it: %d; more than 30%%: %d\n" % (
        int((early <= 2).sum()), len(st), int((early > 10).sum()), int((early > 30).sum())))
    w("histogram of end times (% of span before the last wave: waves)\n")
    edges = list(range(0, 55, 5)) + [100]
    h, _ = np.histogram(early, bins=edges)
    w("  " + "  ".join("%d-%d: %d" % (edges[i], edges[i + 1], h[i]) for i in range(len(h))) + "\n")
    w("by XCD: waves, mean / median / max of the same, residency\n")
    for x in sorted(set(f["xcd"].tolist())):
        m = f["xcd"] == x
        w("  xcd %2d  %4d  %5.1f %5.1f %5.1f  %.3f\n" % (x, int(m.sum()), early[m].mean(), np.median(early[m]),
                                                       early[m].max(), res[m].mean()))
    # the two waves of each SIMD: key = (xcd, se, sh, cu, simd)
    key = (((f["xcd"] * 8 + f["se"]) * 2 + f["sh"]) * 16 + f["cu"]) * 4 + f["simd"]
    order = np.lexsort((f["wave"], t_in, key))
    ks = key[order]
    first = np.r_[True, ks[1:] != ks[:-1]]
    counts = np.diff(np.r_[np.flatnonzero(first), len(ks)])
    pair_start = np.flatnonzero(first)[counts == 2]
    older, younger = order[pair_start], order[pair_start + 1]
    w("by age in the SIMD (%d SIMDs with two waves, %d with another count)\n" % (
        len(pair_start), int((counts != 2).sum())))
    for name, idx in (("older", older), ("younger", younger)):
        if len(idx):
            w("  %-8s %4d  %s  residency %.3f\n" % (name, len(idx), pct(early[idx]), res[idx].mean()))
    if len(older):
        gap = (t_out[younger] - t_out[older]) / span * 100.0
        w("  younger's end after the older's, %% of span: %s\n" % pct(gap))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--versions", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    ctx = crdtenc.Context(0)
    ctx.set_stream(stream.cuda_stream)
    args = argparse.Namespace(versions=a.versions, partition="address")
    w = bench.Workload(ctx, "a", args, 1, 0, dev, bench.actors_table())
    for _ in range(a.warmup):
        w.step()
    torch.cuda.synchronize()
    os.environ["CE_TEST_WAVE_STAMPS"] = "1"
    w.step()
    torch.cuda.synchronize()
    del os.environ["CE_TEST_WAVE_STAMPS"]
    st = ctx.wave_stamps()
    w.drain_names()
    w.close()
    if not len(st):
        raise SystemExit("no stamps: the library has no ce_ctx_wave_stamps build, or another kernel ran")
    report(st, "%s%d files" % (a.label + "; " if a.label else "", w.n))


if __name__ == "__main__":
    main()
