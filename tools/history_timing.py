"""What the pixel history costs on the device (lecturemath_amd.device.FrameHistory, csrc/lm_history.hip), on one synthetic lecture.

    python tools/history_timing.py [--frames 1024] [--out profiles/r13_history.json]

The first --frames frames of lecturemath_amd.synth's 1080p bench stream go through steps 02-03 (the drop-in CCStabilityEstimator);
then, timed by HIP events (median of 5 after 1 warm-up) and by the wall clock:

  append    the uint8 frames, already on the device, packed to bit rows (FrameHistory.append)
  images    CCStabilityEstimator.compute_group_images_from_raw_binary for all groups at threshold 127: the events bracket the C call
            lm_hist_masked_images (table upload, allocation of the output, mask pass, two passes over the frames of every job -- maximum,
            then threshold -- and two synchronisations); python_call_ms is FrameHistory.masked_images around it, the wall time the method
  extract   KeyframeExtractor.extract over four equal segments: the events bracket the four FrameHistory.segment_stats calls

Per part: milliseconds and the useful bit-row bytes read per second (append: the uint8 bytes read) against the 8 TB/s HBM peak.  For
`images` the useful bytes are, per job, output words x frames of the range x 4 bytes, once; the kernel reads them twice, and a box that
is not word-aligned reads a second word per output word on top.  The only comparator that exists is the numpy restatement of both
methods (tests/history_checks.py): its time on the first 64 frames of the same work is printed next to the device's time on exactly
that slice.  Needs the GPU: without one it stops (--lib PATH runs the same code on another build of the library, e.g. the emulated
one at a small --size, as a rehearsal that writes no profile)."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--seed", type=int, default=20213)
    ap.add_argument("--slice", type=int, default=64, help="frames of the numpy comparison")
    ap.add_argument("--lib", default=None, help="another build of the library (rehearsal: nothing is written)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_history.json"))
    args = ap.parse_args()
    width, height = (int(v) for v in args.size.split("x"))
    if args.lib is None:
        import torch                            # before the library: both must end up on the HIP runtime torch brings along
        if not torch.cuda.is_available():
            raise SystemExit("history_timing: needs a GPU")
    from lecturemath_amd import _lib, device, synth
    lib = _lib.load(args.lib)
    _lib._default = lib
    if not lib.is_device_build and args.lib is None:
        raise SystemExit("history_timing: needs the HIP library and a GPU")
    sys.path.insert(0, os.path.join(ROOT, "lecturemath_amd", "dropin"))
    from AccessMath.preprocessing.content.cc_stability_estimator import CCStabilityEstimator
    from AccessMath.preprocessing.content.keyframe_extractor import KeyframeExtractor
    import history_checks as hc
    be = device.Backend(lib)
    n = args.frames

    def timed(fn, repeats=5):
        """(median event ms or None, median wall ms, last result): 1 warm-up + repeats"""
        ev, wall, res = [], [], None
        for rep in range(repeats + 1):
            be.synchronize()
            if lib.is_device_build:
                import torch
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            t0 = time.perf_counter()
            res = fn()
            if lib.is_device_build:
                e1.record()
                e1.synchronize()
            be.synchronize()
            if rep:
                wall.append((time.perf_counter() - t0) * 1e3)
                if lib.is_device_build:
                    ev.append(e0.elapsed_time(e1))
        return (statistics.median(ev) if ev else None), statistics.median(wall), res

    t0 = time.perf_counter()
    frames = np.stack(list(synth.binary_stream(n, height, width, seed=args.seed)))
    gen_s = time.perf_counter() - t0
    est = CCStabilityEstimator(width, height, 0.85, 0.85, 85, False)
    d_frames = be.from_host(frames)
    t0 = time.perf_counter()
    for f0 in range(0, n, 64):
        est.add_frames_device(d_frames[f0:f0 + 64])
    with contextlib.redirect_stdout(io.StringIO()):
        est.split_stable_cc_by_gaps(85, 3)
        stable = est.get_stable_cc_idxs(3)
        time_ov, _, _ = est.compute_overlapping_stable_cc(stable, 5)
        groups, _ = est.compute_groups(stable, time_ov, 0.5, None, None)
        ages, _ = est.compute_groups_temporal_information(groups)
    be.synchronize()
    steps_s = time.perf_counter() - t0
    result = {"width": width, "height": height, "n_frames": n, "seed": args.seed, "stream_generation_s": gen_s, "steps_02_03_s": steps_s,
              "n_groups": len(groups), "n_images": sum(len(ages[g]) - 1 for g in range(len(groups)) if len(groups[g])), "hbm_peak_bytes_per_s": HBM_PEAK}

    def part(name, ev_ms, wall_ms, useful_bytes, **more):
        ms = ev_ms if ev_ms is not None else wall_ms
        result[name] = dict(event_ms=ev_ms, wall_ms=wall_ms, useful_bytes=int(useful_bytes), useful_bytes_per_s=useful_bytes / (ms * 1e-3),
                            fraction_of_hbm_peak=useful_bytes / (ms * 1e-3) / HBM_PEAK, **more)

    # append
    hist = device.FrameHistory(width, height, n, lib)

    def append():
        lib.check(lib.lm_hist_truncate(hist.handle, 0))
        hist.append(d_frames)

    ev, wall, _ = timed(append)
    part("append", ev, wall, frames.nbytes, bit_row_bytes=n * height * ((width + 31) // 32) * 4)

    # raw-binary group images of all groups
    calls = []
    plain = hist.masked_images

    def spy(masks, boxes, ranges, lists, thr, item_first=None):
        be.synchronize()
        t0 = time.perf_counter()
        if lib.is_device_build:
            import torch
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        out = plain(masks, boxes, ranges, lists, thr, item_first=item_first)
        ms = None
        if lib.is_device_build:
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
        words = [(b[3] - b[2] + 1) * ((b[1] - b[0] + 32) // 32) for b in boxes]
        calls.append({"ms": ms if ms is not None else (time.perf_counter() - t0) * 1e3, "jobs": len(boxes), "output_words": int(sum(words)),
                      "useful_bytes": int(sum(wd * (r[1] - r[0] + 1) * 4 for wd, r in zip(words, ranges))),
                      "median_box": [int(np.median([b[1] - b[0] + 1 for b in boxes])), int(np.median([b[3] - b[2] + 1 for b in boxes]))] if boxes else None,
                      "median_range_frames": int(np.median([r[1] - r[0] + 1 for r in ranges])) if ranges else 0,
                      "entries": int(sum(len(lst) for lst in lists))})
        return out

    c_call, c_ms = lib.lm_hist_masked_images, []

    def spy_c(*a):
        if not lib.is_device_build:
            return c_call(*a)
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = c_call(*a)
        e1.record()
        e1.synchronize()
        c_ms.append(e0.elapsed_time(e1))
        return out

    hist.masked_images, lib.lm_hist_masked_images = spy, spy_c
    _, wall, (images, _) = timed(lambda: est.compute_group_images_from_raw_binary(groups, ages, hist, 127))
    hist.masked_images, lib.lm_hist_masked_images = plain, c_call
    last = calls[-1]
    part("images", statistics.median(c_ms[1:]) if c_ms else None, wall, last["useful_bytes"], jobs=last["jobs"], output_words=last["output_words"],
         median_box_w_h=last["median_box"], median_range_frames=last["median_range_frames"], timed_call="lm_hist_masked_images",
         python_call_ms=statistics.median(c["ms"] for c in calls[1:]), python_call="FrameHistory.masked_images",
         wall_is="compute_group_images_from_raw_binary", mask_list_entries=last["entries"])

    # extract over four equal segments
    cuts = [round(k * n / 4) for k in range(5)]
    segments = [(cuts[k], cuts[k + 1] - 1) for k in range(4)]
    ev, _, _ = timed(lambda: [hist.segment_stats(s, e) for s, e in segments])
    _, wall, _ = timed(lambda: KeyframeExtractor.extract(hist, segments, 4.5))
    part("extract", ev, wall, n * height * ((width + 31) // 32) * 4, segments=segments, timed_call="4 x FrameHistory.segment_stats", wall_is="KeyframeExtractor.extract")

    # the numpy restatement on the first frames of the same work, against the device on exactly that slice
    m = min(args.slice, n)
    sl_ages = {g: [a for a in ages[g] if a < m] for g in range(len(groups))}
    used = sorted({int(c) for g, group in enumerate(groups) if len(sl_ages[g]) > 1 for c in group})
    cc_boxes, cc_images, cc_life, _ = est._unique_masks(used)
    sl_groups = [list(group) if len(sl_ages[g]) > 1 else [] for g, group in enumerate(groups)]
    t0 = time.perf_counter()
    want, _, _ = hc.numpy_raw_images(cc_boxes, cc_images, cc_life, sl_groups, sl_ages, frames[:m], 127)
    numpy_images_ms = (time.perf_counter() - t0) * 1e3
    sl_hist = device.FrameHistory.from_frames(d_frames[:m], lib)
    _, dev_images_ms, (got, _) = timed(lambda: est.compute_group_images_from_raw_binary(sl_groups, sl_ages, sl_hist, 127))
    assert list(got.keys()) == list(want) and all((got[g][k] == want[g][k]).all() for g in list(want)[::17] for k in range(len(want[g])))
    sl_cuts = [round(k * m / 4) for k in range(5)]
    sl_segments = [(sl_cuts[k], sl_cuts[k + 1] - 1) for k in range(4)]
    t0 = time.perf_counter()
    want_x = hc.numpy_extract(frames[:m], sl_segments, 4.5)
    numpy_extract_ms = (time.perf_counter() - t0) * 1e3
    _, dev_extract_ms, got_x = timed(lambda: KeyframeExtractor.extract(sl_hist, sl_segments, 4.5))
    assert all((a["sum"] == b["sum"]).all() and (a["age"] == b["age"]).all() and (a["filtered"] == b["filtered"]).all() for a, b in zip(got_x, want_x))
    result["slice"] = {"frames": m, "images": sum(len(v) for v in want.values()), "numpy_images_ms": numpy_images_ms, "device_images_wall_ms": dev_images_ms,
                       "numpy_extract_ms": numpy_extract_ms, "device_extract_wall_ms": dev_extract_ms}
    sl_hist.close()
    hist.close()
    print(json.dumps(result, indent=1))
    if lib.is_device_build:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    else:
        print("rehearsal on %s: no profile written" % lib.path)


if __name__ == "__main__":
    main()
