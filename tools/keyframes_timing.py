"""What step 05 (keyframes) costs on its two routes, in one process on one synthetic lecture.

    python tools/keyframes_timing.py [--frames 1500] [--out profiles/r08_keyframes.json]

A 1080p lecture from lecturemath_amd.synth.binary_stream (glyphs added every other frame, a third to a half of the board erased
every ~60 frames) goes through LecturePipeline twice, once per route of finish():

  host     finish(keyframes="host"): every group image expanded to host uint8 (lm_group_array(LM_G_GIMG)); step 05 concatenates
           and uploads the alive groups' images per segment (device.image_pairs_overlap) and composes the keyframe with numpy
  device   finish(keyframes="device"): a GroupImages view of the bit rows step 03 left on the device; one lm_kf_overlaps and one
           lm_kf_render call for all segments

Recorded: wall time and peak growth of the host RSS of finish() (sampled from /proc/self/statm while it runs) -- in a fresh child
process per route, twice each, so that neither route inherits the other's heap, and once more in this process; then, on this
process's two finished structures, the wall time of KeyframeExtractor.GenerateFromST3DForIntervals alone -- median of 5 after 1
warm-up, the routes alternating, each run ending in a device synchronise -- and, on the device route, the HIP-event time of the
overlaps and the render call; for the pipeline's own segmentation and for the lecture cut into ten equal parts.  The keyframes of the two routes must be equal.  Needs the GPU: without one it stops (--lib PATH runs the same
code on another build of the library, e.g. the emulated one at a small --size, as a rehearsal that writes no profile)."""
import argparse
import contextlib
import hashlib
import io
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

PAGE = os.sysconf("SC_PAGE_SIZE")


def rss_bytes():
    with open("/proc/self/statm") as f:
        return int(f.read().split()[1]) * PAGE


class RssPeak:
    """peak of the resident set while the block runs, minus what it was at the start"""

    def __enter__(self):
        self.start = self.peak = rss_bytes()
        self._stop = threading.Event()
        self._thread = threading.Thread(target=self._run, daemon=True)
        self._thread.start()
        return self

    def _run(self):
        while not self._stop.wait(0.002):
            self.peak = max(self.peak, rss_bytes())

    def __exit__(self, *exc):
        self._stop.set()
        self._thread.join()
        self.peak = max(self.peak, rss_bytes())
        self.growth = self.peak - self.start


def build_lecture(lib, width, height, n_frames, seed, route):
    from lecturemath_amd import synth
    from lecturemath_amd.pipeline import LecturePipeline
    pipe = LecturePipeline(width, height, lib=lib)
    batch = []
    for frame in synth.binary_stream(n_frames, height, width, seed=seed, erase_every=60):
        batch.append(frame)
        if len(batch) == 50:
            pipe.add_binary_frames(np.stack(batch))
            batch = []
    if batch:
        pipe.add_binary_frames(np.stack(batch))
    pipe.be.synchronize()
    t0 = time.perf_counter()
    with RssPeak() as rss:
        out = pipe.finish(keyframes=route)
        pipe.be.synchronize()
    return pipe, out, {"finish_wall_s": time.perf_counter() - t0, "finish_rss_peak_growth_bytes": rss.growth}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1500)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--seed", type=int, default=20213)
    ap.add_argument("--lib", default=None, help="another build of the library (rehearsal: nothing is written)")
    ap.add_argument("--finish-only", choices=("host", "device"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_keyframes.json"))
    args = ap.parse_args()
    width, height = (int(v) for v in args.size.split("x"))
    if args.lib is None:
        import torch                            # before the library: both must end up on the HIP runtime torch brings along
        if not torch.cuda.is_available():
            raise SystemExit("keyframes_timing: needs a GPU")
    from lecturemath_amd import _lib
    lib = _lib.load(args.lib)
    _lib._default = lib
    if not lib.is_device_build and args.lib is None:
        raise SystemExit("keyframes_timing: needs the HIP library and a GPU")
    sys.path.insert(0, os.path.join(ROOT, "lecturemath_amd", "dropin"))
    from AccessMath.preprocessing.content.keyframe_extractor import KeyframeExtractor

    if args.finish_only:                     # child: one route in a fresh process, so that its RSS figure owes nothing to the other route
        _, out, stats = build_lecture(lib, width, height, args.frames, args.seed, args.finish_only)
        stats["n_keyframes"] = len(out["keyframes"])
        print("FINISH " + json.dumps(stats))
        return
    result = {"width": width, "height": height, "n_frames": args.frames, "seed": args.seed, "routes": {}}
    if args.lib is None:
        import subprocess
        for route in ("device", "host", "device", "host"):      # twice each, alternating: the spread of the figures
            text = subprocess.run([sys.executable, os.path.abspath(__file__), "--frames", str(args.frames), "--size", args.size, "--seed", str(args.seed),
                                   "--finish-only", route], check=True, capture_output=True, text=True).stdout
            line = [ln for ln in text.splitlines() if ln.startswith("FINISH ")][-1]
            result["routes"].setdefault(route, {"fresh_process": []})["fresh_process"].append(json.loads(line[7:]))
    finished = {}
    for route in ("device", "host"):
        pipe, out, stats = build_lecture(lib, width, height, args.frames, args.seed, route)
        finished[route] = (pipe, out)
        result["routes"].setdefault(route, {})["same_process"] = stats
    pipe, out = finished["device"]
    st_dev, st_host = out["st3d"], finished["host"][1]["st3d"]
    intervals = [tuple(int(v) for v in iv) for iv in out["intervals"]]
    assert intervals == [tuple(int(v) for v in iv) for iv in finished["host"][1]["intervals"]]
    view = st_dev._device_images
    grouping = pipe.estimator._cur(pipe.estimator._thr)
    scalars = grouping.array("scalars")
    result.update(n_groups=int(scalars[2]), n_items=len(view), uint8_group_image_bytes=int(scalars[5]),
                  bit_row_bytes=int(sum(int(h) * ((int(w) + 31) // 32) * 4 for h, w in view._shapes)))

    # the two device calls under HIP events
    events = {"overlaps": [], "render": []}

    def with_events(name, fn):
        def call(*a, **kw):
            if not lib.is_device_build:
                return fn(*a, **kw)
            import torch
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*a, **kw)
            e1.record()
            e1.synchronize()
            events[name].append(e0.elapsed_time(e1) * 1e-3)
            return r
        return call

    plain = (view.overlaps, view.render)

    def run(st3d, segments):
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            frames, times = KeyframeExtractor.GenerateFromST3DForIntervals(st3d, segments, False)
        pipe.be.synchronize()
        return time.perf_counter() - t0, frames, times

    def summary(v):
        return {"median_s": statistics.median(v), "min_s": min(v), "max_s": max(v), "warmup": 1, "repeats": len(v)}

    # the pipeline's own segmentation, and the lecture cut into ten equal parts (what "all segments in one call" is about)
    cuts = [round(k * args.frames / 10) for k in range(11)]
    segmentations = {"pipeline": intervals, "ten_equal_parts": [(cuts[k], cuts[k + 1] - 1) for k in range(10)]}
    result["step05"] = {}
    for name, segments in segmentations.items():
        walls = {"host": [], "device": [], "device_with_events": []}
        for ev in events.values():
            del ev[:]
        for rep in range(6):                    # 1 warm-up + 5, the routes alternating
            t_host, f_host, c_host = run(st_host, segments)
            view.overlaps, view.render = plain
            t_dev, f_dev, c_dev = run(st_dev, segments)
            view.overlaps, view.render = with_events("overlaps", plain[0]), with_events("render", plain[1])
            t_ev, _, _ = run(st_dev, segments)
            assert c_host == c_dev and all((a == b).all() for a, b in zip(f_host, f_dev)), "the two routes disagree"
            if rep:
                walls["host"].append(t_host)
                walls["device"].append(t_dev)
                walls["device_with_events"].append(t_ev)
        view.overlaps, view.render = plain
        entry = {"n_segments": len(segments), "wall": {k: summary(v) for k, v in walls.items()},
                 "groups_alive_per_segment": [len(a) for a, _ in KeyframeExtractor._segment_selection(st_dev.cc_group_ages, segments)[2]],
                 "groups_drawn_per_segment": [len(lst) for lst in c_dev],
                 "keyframes_sha256": hashlib.sha256(np.stack(f_dev).tobytes()).hexdigest(),
                 "keyframe_ink_pixels": [int((f[..., 0] == 0).sum()) for f in f_dev]}
        if lib.is_device_build:
            entry["device_calls_hip_events"] = {k: summary(v[1:]) for k, v in events.items()}      # (first = the warm-up round)
        result["step05"][name] = entry
    result["crowded_tiles"] = view.crowded_tiles()
    print(json.dumps(result, indent=1))
    if lib.is_device_build:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    else:
        print("rehearsal on %s: no profile written" % lib.path)


if __name__ == "__main__":
    main()
