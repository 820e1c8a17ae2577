"""What the CC overlap counts of the summary evaluation (lm_kf_pair_counts under the overlay's AccessMath.evaluation.evaluator) cost
on the device, and what the host loop they replace costs on this machine's CPU.

    python tools/evaluation_timing.py [--out profiles/r12_evaluation.json]

Synthetic 1080p keyframes of 2,000 glyph-sized CCs each (a 40 x 50 grid; the second keyframe of a pair is a jittered copy with
other masks), one pair and a batch of 32 pairs.  Timed with HIP events, 2 warm-up rounds, median of 7 with min-max:

  create_1_pair / create_32_pairs     device.CCPairCounts(...): lm_kf_create_from_images of the 4,000 / 128,000 CC masks (upload and
                                      bit packing) plus the Python that flattens the masks
  counts_r0_1_pair / _32_pairs        CCPairCounts.counts at radius 0 (keyframes_overlapping_ccs, match_overlapping_ccs): a query per
                                      pair, rows and counts copied to the host
  counts_r3_1_pair / _32_pairs        the same at radius 3 (keyframes_unique_cc, 49 displacements per row)
  host_r0_1_pair                      the loop of keyframes_overlapping_ccs as it runs without this primitive: every CC of one
                                      keyframe against every CC of the other through the overlay's ConnectedComponent.
                                      getOverlapFMeasure, 4,000,000 calls, wall clock on one core (1 warm-up, 3 repeats)
  host_r3_sample                      check_equivalent_cc as a host loop (49 displacements, getOverlapFMeasure where the boxes
                                      overlap) on the first 150 x 150 CCs of the pair, wall clock; counts_r3_sample is the device on
                                      the same sub-lists

Both routes are asserted equal before anything is timed.  Not measured: how a counts call divides between the two join launches,
the count kernel, the two stream synchronisations and the copies; the host loop at radius 3 on the full 2,000 x 2,000 pairs (the
sample is scaled by nothing: it is reported as it is).  Needs the GPU (--lib PATH runs the same code on another build, e.g. the
emulated one with a small --grid, as a rehearsal that writes no profile)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "lecturemath_amd", "dropin"))

import numpy as np  # noqa: E402

WARMUP, REPEATS = 2, 7


def make_keyframe(rng, rows_n, cols_n, pitch_x, pitch_y, jitter, CC):
    out = []
    for gy in range(rows_n):
        for gx in range(cols_n):
            bw, bh = int(rng.integers(8, pitch_x - 6)), int(rng.integers(8, pitch_y - 5))
            x0, y0 = gx * pitch_x + int(rng.integers(0, jitter + 1)), gy * pitch_y + int(rng.integers(0, jitter + 1))
            img = (rng.random((bh, bw)) < 0.5).astype(np.uint8) * 255
            img[0, 0] = 255
            out.append(CC(len(out), x0, x0 + bw - 1, y0, y0 + bh - 1, int(np.count_nonzero(img)), img))
    return out


def host_overlaps(frame1, frame2, disp):
    """pairs (i, j) with shared ink, found the way keyframes_overlapping_ccs finds them on the host"""
    found = []
    for j, b in enumerate(frame2):
        b.translateBox(disp[1], disp[0])
        for i, a in enumerate(frame1):
            recall, _ = a.getOverlapFMeasure(b, False, False)
            if recall > 0.0:
                found.append((i, j))
        b.translateBox(-disp[1], -disp[0])
    return sorted(found)


def host_window_counts(frame1, frame2, disp, window):
    """{(i, j): {(ey, ex): shared ink}} for the displacements at which the boxes overlap by the strict test of check_equivalent_cc"""
    out = {}
    for j, b in enumerate(frame2):
        for i, a in enumerate(frame1):
            for ey in range(-window, window + 1):
                for ex in range(-window, window + 1):
                    b.translateBox(disp[1] + ex, disp[0] + ey)
                    if b.min_x < a.max_x and a.min_x < b.max_x and b.min_y < a.max_y and a.min_y < b.max_y:
                        recall, _ = b.getOverlapFMeasure(a, False, False)
                        out.setdefault((i, j), {})[(ey, ex)] = int(round(recall * b.size))
                    b.translateBox(-disp[1] - ex, -disp[0] - ey)
    return out


def summary(v, warmup):
    v = v[warmup:]
    return {"median_s": statistics.median(v), "min_s": min(v), "max_s": max(v), "warmup": warmup, "repeats": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="40x50", help="rows x columns of glyph cells per keyframe")
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--sample", type=int, default=150)
    ap.add_argument("--seed", type=int, default=20212)
    ap.add_argument("--lib", default=None, help="another build of the library (rehearsal: nothing is written)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_evaluation.json"))
    args = ap.parse_args()
    rows_n, cols_n = (int(v) for v in args.grid.split("x"))
    if args.lib is None:
        import torch                            # before the library: both must end up on the HIP runtime torch brings along
        if not torch.cuda.is_available():
            raise SystemExit("evaluation_timing: needs a GPU")
    from lecturemath_amd import _lib, device
    from AM_CommonTools.data.connected_component import ConnectedComponent as CC
    lib = _lib.load(args.lib)
    if not lib.is_device_build and args.lib is None:
        raise SystemExit("evaluation_timing: needs the HIP library and a GPU")
    be = device.Backend(lib)
    pitch_x, pitch_y = 38, 27
    width, height = max(cols_n * pitch_x + 20, 64), max(rows_n * pitch_y, 32)
    rng = np.random.default_rng(args.seed)
    frames = []
    for _ in range(args.pairs):
        frames.append(make_keyframe(rng, rows_n, cols_n, pitch_x, pitch_y, 0, CC))
        frames.append(make_keyframe(rng, rows_n, cols_n, pitch_x, pitch_y, 6, CC))
    disp = (2, -3)

    def timed(fn):
        if not lib.is_device_build:
            t0 = time.perf_counter()
            r = fn()
            return r, time.perf_counter() - t0
        e0, e1 = be.torch.cuda.Event(enable_timing=True), be.torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return r, e0.elapsed_time(e1) * 1e-3

    # ---- both routes agree (before any timing)
    one = device.CCPairCounts(frames[:2], width, height, lib=lib)
    q_one = [(one.items(0), one.items(1), disp)]
    rows0, counts0 = one.counts(q_one, 0)
    t0 = time.perf_counter()
    want = host_overlaps(frames[0], frames[1], disp)
    first_host = time.perf_counter() - t0
    got = sorted((int(i), int(j)) for (_, i, j), c in zip(rows0.tolist(), counts0) if c[0, 0] > 0)
    assert got == want, "the device and the host loop disagree on the overlapping pairs"
    ns = min(args.sample, len(frames[0]))
    q_sample = [(one.items(0)[:ns], one.items(1)[:ns], disp)]
    rows_s, counts_s = one.counts(q_sample, 3)
    by_row = {(int(i), int(j)): c for (_, i, j), c in zip(rows_s.tolist(), counts_s)}
    host_s = host_window_counts(frames[0][:ns], frames[1][:ns], disp, 3)
    assert host_s and all(by_row[k][ey + 3, ex + 3] == v for k, d in host_s.items() for (ey, ex), v in d.items()), \
        "the device and the host loop disagree on the window counts"

    t = {k: [] for k in ("create_1_pair", "create_32_pairs", "counts_r0_1_pair", "counts_r0_32_pairs", "counts_r3_1_pair",
                         "counts_r3_32_pairs", "counts_r3_sample", "host_r0_1_pair", "host_r3_sample")}
    t["host_r0_1_pair"].append(first_host)
    batch = device.CCPairCounts(frames, width, height, lib=lib)
    q_batch = [(batch.items(2 * k), batch.items(2 * k + 1), disp) for k in range(args.pairs)]
    n_rows = {}
    for rep in range(WARMUP + REPEATS):         # the routes alternating
        tab, s = timed(lambda: device.CCPairCounts(frames[:2], width, height, lib=lib))
        t["create_1_pair"].append(s)
        tab.close()
        tab, s = timed(lambda: device.CCPairCounts(frames, width, height, lib=lib))
        t["create_32_pairs"].append(s)
        tab.close()
        for r in (0, 3):
            (rw, _), s = timed(lambda: one.counts(q_one, r))
            t["counts_r%d_1_pair" % r].append(s)
            n_rows["r%d_1_pair" % r] = len(rw)
            (rw, _), s = timed(lambda: batch.counts(q_batch, r))
            t["counts_r%d_32_pairs" % r].append(s)
            n_rows["r%d_32_pairs" % r] = len(rw)
        _, s = timed(lambda: one.counts(q_sample, 3))
        t["counts_r3_sample"].append(s)
        if rep < 3:
            t0 = time.perf_counter()
            host_overlaps(frames[0], frames[1], disp)
            t["host_r0_1_pair"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        host_window_counts(frames[0][:ns], frames[1][:ns], disp, 3)
        t["host_r3_sample"].append(time.perf_counter() - t0)
    one.close()
    batch.close()
    timing = {k: summary(v, 1 if k == "host_r0_1_pair" else WARMUP) for k, v in t.items()}
    result = {"width": width, "height": height, "ccs_per_keyframe": rows_n * cols_n, "pairs_in_batch": args.pairs, "sample": ns, "seed": args.seed,
              "displacement": list(disp), "rows": n_rows, "overlapping_pairs_of_one_keyframe_pair": len(want), "timing": timing,
              "clock": {"device": "HIP events around the Python call (every call ends in a stream synchronise)",
                        "host": "time.perf_counter, one core"}}
    host = timing["host_r0_1_pair"]
    result["device_faster_than_host_minus_spread"] = bool(timing["counts_r0_1_pair"]["median_s"] < host["median_s"] - (host["max_s"] - host["min_s"]))
    print(json.dumps(result, indent=1))
    if lib.is_device_build:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    else:
        print("rehearsal on %s: no profile written" % lib.path)


if __name__ == "__main__":
    main()
