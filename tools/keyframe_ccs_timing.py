"""What the keyframe CC table (device.KeyframeCCs.from_frames, lm_kf_create_from_frames) and the evaluation on it cost on the device,
against the route they replace: host copy of every keyframe, the overlay Labeler per keyframe, then the device.CCPairCounts upload.

    python tools/keyframe_ccs_timing.py [--out profiles/r14_keyframe_ccs.json]
    python tools/keyframe_ccs_timing.py --kernels-only      # the launches alone, for a rocprofv3 --kernel-trace --stats run

Input: 32 frames of the bench stream (synth.binary_stream(256, 1080, 1920, seed=20213), every 8th frame) in the keyframe convention
([32][1080][1920][3] on the device, 0 = ink, 255 = paper) -- the board as it fills up, about a thousand CCs per frame.  (Step 05 of
that stream yields only a handful of keyframes; the stream's own frames have the same content and give the 32 the comparison asks
for.)  Device times: HIP events around the Python call, 2 warm-up rounds, median of 7 with min-max.  Host route: time.perf_counter,
1 warm-up, 2 repeats.  Both routes are asserted equal before anything is timed.

  from_frames_32                 KeyframeCCs.from_frames on the device tensor, max_batch 8
  host_route_32                  per keyframe tensor.cpu() + Labeler.extractSpatioTemporalContent(255 - channel 0, zeros, False), then
                                 CCPairCounts over the 32 lists (lm_kf_create_from_images); its three parts are reported separately
  summary_device / summary_host  Evaluator.compute_summary_metrics end to end on 8 ground-truth keyframes against 8 copies moved by
                                 (2, -3): DeviceKeyframes of one table against host keyframes with the Labeler's CCs (upload route);
                                 making the keyframes is not included (it is the two rows above, for 16 frames)
  pixel_sums_32_stride3 / _stride1   lm_kf_pixel_sums over 32 pairs with masks; bytes = what the kernel must read, share = over the
                                 HBM peak named in the result
Needs the GPU (--lib PATH runs the same code on another build with --small, as a rehearsal that writes no profile)."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "lecturemath_amd", "dropin"))

import numpy as np  # noqa: E402

WARMUP, REPEATS = 2, 7
HBM_PEAK = 8.0e12       # bytes / s, MI355X


def summary(v, warmup):
    v = v[warmup:]
    return {"median_s": statistics.median(v), "min_s": min(v), "max_s": max(v), "warmup": warmup, "repeats": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--small", action="store_true", help="4 frames of 135 x 240 (rehearsal)")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_keyframe_ccs.json"))
    args = ap.parse_args()
    if args.lib is None:
        import torch                            # before the library: both must end up on the HIP runtime torch brings along
        if not torch.cuda.is_available():
            raise SystemExit("keyframe_ccs_timing: needs a GPU")
    from lecturemath_amd import _lib, device, keyframes, synth
    from AccessMath.evaluation.evaluator import Evaluator
    from AccessMath.preprocessing.content.labeler import Labeler
    lib = _lib.load(args.lib)
    _lib._default = lib
    if not lib.is_device_build and args.lib is None:
        raise SystemExit("keyframe_ccs_timing: needs the HIP library and a GPU")
    be = device.Backend(lib)
    h, w, n, every = (135, 240, 4, 8) if args.small else (1080, 1920, 32, 8)
    stream = synth.binary_stream(n * every, h, w, seed=20213)
    planes = np.stack([255 - f for i, f in enumerate(stream) if i % every == every - 1]).astype(np.uint8)
    assert planes.shape == (n, h, w)
    frames = be.from_host(np.repeat(planes[..., None], 3, axis=3))
    rng = np.random.default_rng(14)
    masks = np.zeros((n, h, w), np.uint8)
    for k in range(n):
        masks[k, :h // 3, :w // 4 + k] = 1
    dmasks = be.from_host(masks)

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

    if args.kernels_only:
        for _ in range(3):
            device.KeyframeCCs.from_frames(frames, masks=dmasks, lib=lib).close()
            device.pixel_sums(frames, frames, dmasks, lib=lib)
            device.pixel_sums(be.from_host(planes), be.from_host(planes), dmasks, lib=lib)
        return

    def host_route(parts=None):
        t0 = time.perf_counter()
        host = [np.ascontiguousarray(be.to_host(frames[k])[:, :, 0]) for k in range(n)]
        t1 = time.perf_counter()
        lists = [Labeler.extractSpatioTemporalContent(255 - p, np.zeros((h, w), np.float32), False) for p in host]
        t2 = time.perf_counter()
        table = device.CCPairCounts(lists, w, h, lib=lib)
        be.synchronize()
        t3 = time.perf_counter()
        if parts is not None:
            for name, s in (("host_copy_32", t1 - t0), ("labeler_32", t2 - t1), ("upload_32", t3 - t2), ("host_route_32", t3 - t0)):
                parts.setdefault(name, []).append(s)
        return lists, table

    # ---- both routes agree (before any timing)
    table = device.KeyframeCCs.from_frames(frames, masks=dmasks, lib=lib)
    lists, up = host_route()
    n_cc = [len(lst) for lst in lists]
    assert table.frame_off.tolist() == np.concatenate([[0], np.cumsum(n_cc)]).tolist()
    flat = [cc for lst in lists for cc in lst]
    assert (table.records == np.asarray([[c.cc_id, c.min_x, c.max_x, c.min_y, c.max_y, c.size] for c in flat], np.int32)).all()
    for item in range(0, len(flat), max(1, len(flat) // 200)):
        assert (table.image(item) == flat[item].img).all(), item
    up.close()
    table.close()

    t = {}
    for rep in range(WARMUP + REPEATS):
        tab, s = timed(lambda: device.KeyframeCCs.from_frames(frames, masks=dmasks, lib=lib))
        t.setdefault("from_frames_32", []).append(s)
        tab.close()
        if rep < 3:
            _, up = host_route(t)
            up.close()
    one = be.from_host(planes)
    for rep in range(WARMUP + REPEATS):
        for name, a in (("pixel_sums_32_stride3", frames), ("pixel_sums_32_stride1", one)):
            sums = be.empty((n, 4), np.int64)

            def run():
                for _ in range(20):
                    lib.check(lib.lm_kf_pixel_sums(_lib.ptr(a), 3 if a is frames else 1, _lib.ptr(a), 3 if a is frames else 1, _lib.ptr(dmasks), n, h * w,
                                                   _lib.ptr(sums), be.stream()))
            _, s = timed(run)
            t.setdefault(name, []).append(s / 20)

    # ---- the evaluation end to end: 8 keyframes against 8 moved copies
    m = min(8, n // 2)
    moved = np.full((m, h, w), 255, np.uint8)
    moved[:, 2:, :-3] = planes[:m, :-2, 3:]
    both = be.from_host(np.repeat(np.concatenate([planes[:m], moved])[..., None], 3, axis=3))
    both_masks = np.concatenate([masks[:m], np.zeros((m, h, w), np.uint8)])
    kfs = keyframes.keyframes_from_frames(both, masks=both_masks, lib=lib)
    gt, summ = kfs[:m], kfs[m:]
    hk = []
    for k, kf in enumerate(kfs):
        ns = types.SimpleNamespace(idx=kf.idx, binary_image=kf.binary_image, raw_image=None, object_mask=kf.object_mask.copy(),
                                   binary_cc=Labeler.extractSpatioTemporalContent(255 - kf.binary_image[:, :, 0], np.zeros((h, w), np.float32), False))
        ns.check_cc_overlaps_background = types.MethodType(keyframes.DeviceKeyframe.check_cc_overlaps_background, ns)
        hk.append(ns)

    def evaluate(a, b):
        groups, cc_group, seg_a = keyframes.generate_fake_keyframe_info(a)
        _, _, seg_b = keyframes.generate_fake_keyframe_info(b)
        with contextlib.redirect_stdout(io.StringIO()):
            return Evaluator.compute_summary_metrics(seg_a, a, groups, cc_group, seg_b, b)

    created = device.CCPairCounts.created
    got = evaluate(gt, summ)
    assert device.CCPairCounts.created == created, "the device keyframes were uploaded"
    want = evaluate(hk[:m], hk[m:])
    assert json.dumps(got, default=float, sort_keys=True) == json.dumps(want, default=float, sort_keys=True), "the two routes disagree"
    for rep in range(1 + 2):
        _, s = timed(lambda: evaluate(gt, summ))
        t.setdefault("summary_device", []).append(s)
        t0 = time.perf_counter()
        evaluate(hk[:m], hk[m:])
        t.setdefault("summary_host", []).append(time.perf_counter() - t0)
    kfs[0].set.close()

    timing = {k: summary(v, WARMUP if len(v) == WARMUP + REPEATS else 1) for k, v in t.items()}
    px_bytes = {"pixel_sums_32_stride3": n * h * w * (3 + 3 + 1), "pixel_sums_32_stride1": n * h * w * 3}
    needed = {"pixel_sums_32_stride3": n * h * w * 3, "pixel_sums_32_stride1": n * h * w * 3}
    result = {"width": w, "height": h, "keyframes": n, "ccs_per_keyframe": {"min": min(n_cc), "max": max(n_cc), "total": sum(n_cc)},
              "evaluation": {"keyframes_per_side": m, "displacement": [2, -3]}, "timing": timing, "hbm_peak_bytes_per_s": HBM_PEAK,
              "pixel_sums": {k: {"bytes_needed": needed[k], "bytes_of_the_lines_touched": px_bytes[k],
                                 "needed_bytes_per_s": needed[k] / timing[k]["median_s"],
                                 "share_of_hbm_peak": needed[k] / timing[k]["median_s"] / HBM_PEAK} for k in px_bytes},
              "clock": {"device": "HIP events around the Python call (every call ends in a stream synchronise); pixel sums: 20 launches per event pair",
                        "host": "time.perf_counter"}}
    result["from_frames_faster_than_host_route"] = bool(timing["from_frames_32"]["max_s"] < timing["host_route_32"]["min_s"])
    result["summary_device_faster_than_host"] = bool(timing["summary_device"]["max_s"] < timing["summary_host"]["min_s"])
    print(json.dumps(result, indent=1))
    if lib.is_device_build and not args.small:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    else:
        print("rehearsal: no profile written")


if __name__ == "__main__":
    main()
