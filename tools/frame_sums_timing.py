"""What the frame sums of the reconstructed stream (step 04, method 1; the reference computes them for every method) cost on their
two device routes, in one process on the bench's synthetic stream, and what method 1 costs in LecturePipeline.finish().

    python tools/frame_sums_timing.py [--frames 10000] [--finish-frames 600] [--out profiles/r10_frame_sums.json]

After lm_group_run on the stream (lecturemath_amd.synth.binary_stream, the bench's seed):

  tiles    lm_group_frame_sums for all frames: the render kernel's tile painting, popcounts over the cover counts, no byte frame
  frames   lm_group_render in chunks of --batch frames into one reused buffer + lm_frame_sums of every chunk

The two alternate in this process, --warmup rounds untimed, then --repeats timed; each timed with HIP events around the route's
launches and ended by a synchronise.  The sums of the two routes are compared over all frames.  A route counts as faster only when
its median lies below the other's median minus the other's spread (max - min).  Bytes are counted from shapes: the frames route
writes and reads frames x H x W bytes; the share of the HBM peak is those bytes over its median time over 8 TB/s.

Then finish() with VIDEO_SEGMENTATION_METHOD = 1 against 3 (keyframes on the device, no PNG) on a shorter lecture that is erased
every 60 frames, a fresh pipeline per run, the methods alternating; and, on a finished method-1 pipeline, what the method itself
adds: reconstructed_frame_sums() and the script's sums_intervals (the tree, on the host), median of 5 after 1 warm-up.  Needs the GPU: without one it stops (--lib PATH runs the same
code on another build of the library, e.g. the emulated one at a small --size, as a rehearsal that writes no profile)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HBM_PEAK = 8.0e12


def summary(v):
    return {"median_s": statistics.median(v), "min_s": min(v), "max_s": max(v), "spread_s": max(v) - min(v), "repeats": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10000)
    ap.add_argument("--finish-frames", type=int, default=600)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seed", type=int, default=20213)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--finish-repeats", type=int, default=3)
    ap.add_argument("--lib", default=None, help="another build of the library (rehearsal: nothing is written)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_frame_sums.json"))
    args = ap.parse_args()
    W, H = (int(v) for v in args.size.split("x"))
    F, B = args.frames, args.batch
    torch = None
    if args.lib is None:
        import torch                            # before the library: both must end up on the HIP runtime torch brings along
        if not torch.cuda.is_available():
            raise SystemExit("frame_sums_timing: needs a GPU")
    from lecturemath_amd import _lib, device, synth
    lib = _lib.load(args.lib)
    _lib._default = lib
    if not lib.is_device_build and args.lib is None:
        raise SystemExit("frame_sums_timing: needs the HIP library and a GPU")
    be = device.Backend(lib)

    def sync():
        if torch is not None:
            torch.cuda.synchronize()

    def timed(fn):
        """seconds of fn()'s device work (HIP events; the host clock on the emulated build)"""
        if torch is None:
            t0 = time.perf_counter()
            fn()
            return time.perf_counter() - t0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    result = {"width": W, "height": H, "n_frames": F, "batch": B, "seed": args.seed, "warmup": args.warmup}
    # ---- the stream, steps 02 and 03
    fs = device.FrameStream(W, H, F, 0.85, 0.85, 85, 20, max_batch=B, max_ccs=F * 4096, max_crop_words=F * max(1 << 17, (W * H) // 16), lib=lib)
    buf = []
    for frame in synth.binary_stream(F, H, W, seed=args.seed):
        buf.append(frame)
        if len(buf) == B:
            fs.push(be.from_host(np.stack(buf)))
            buf = []
    if buf:
        fs.push(be.from_host(np.stack(buf)))
    gr = device.Grouping(fs, max_gap=85, min_times=3, t_window=5, min_recall=0.5, img_threshold=0.5, reconstruct=True)
    sync()
    scalars = gr.array("scalars")
    result.update(n_groups=int(scalars[2]), render_items=int(len(gr.array("gpf"))))
    clean = be.empty((B, H, W), np.uint8)
    sums_tiles, sums_frames = be.empty((F,), np.int64), be.empty((F,), np.int64)
    st = be.stream()

    def tiles():
        lib.check(lib.lm_group_frame_sums(gr.handle, 0, F, _lib.ptr(sums_tiles), st))

    def frames():
        for f0 in range(0, F, B):
            n = min(B, F - f0)
            lib.check(lib.lm_group_render(gr.handle, f0, n, _lib.ptr(clean), st))
            lib.check(lib.lm_frame_sums(_lib.ptr(clean), n, H * W, _lib.ptr(sums_frames[f0:f0 + n]), st))

    walls = {"tiles": [], "frames": []}
    for rep in range(args.warmup + args.repeats):
        for name, fn in (("tiles", tiles), ("frames", frames)):
            t = timed(fn)
            sync()
            if rep >= args.warmup:
                walls[name].append(t)
    a, b = be.to_host(sums_tiles), be.to_host(sums_frames)
    assert (a == b).all(), "the two routes disagree at frames %r" % (np.flatnonzero(a != b)[:8],)
    t_tiles, t_frames = summary(walls["tiles"]), summary(walls["frames"])
    frame_bytes = 2 * F * H * W                     # every byte written by the render and read by the sum
    result["sums"] = {
        "equal_over_all_frames": True, "sum_of_sums": int(a.sum()), "frames_with_ink": int((a > 0).sum()),
        "tiles": t_tiles, "frames": dict(t_frames, bytes_moved=frame_bytes, reused_buffer_bytes=B * H * W,
                                         share_of_hbm_peak=frame_bytes / t_frames["median_s"] / HBM_PEAK),
        "tiles_output_bytes": 8 * F,
        "tiles_faster_by_the_rule": bool(t_tiles["median_s"] < t_frames["median_s"] - t_frames["spread_s"]),
        "frames_faster_by_the_rule": bool(t_frames["median_s"] < t_tiles["median_s"] - t_tiles["spread_s"]),
        "ratio_frames_over_tiles": t_frames["median_s"] / t_tiles["median_s"]}
    gr.close()
    fs.close()
    del clean, sums_tiles, sums_frames

    # ---- finish() with method 1 against method 3
    if args.finish_frames > 0:
        from lecturemath_amd.pipeline import LecturePipeline
        n = args.finish_frames
        lecture = np.stack(list(synth.binary_stream(n, H, W, seed=args.seed, erase_every=60)))
        walls, intervals = {"1": [], "3": []}, {}
        for rep in range(1 + args.finish_repeats):
            for method in ("1", "3"):
                pipe = LecturePipeline(W, H, conf={"VIDEO_SEGMENTATION_METHOD": method}, lib=lib)
                pipe.estimator.INITIAL_FRAMES = n           # sized once: no re-allocation of the stream while the frames arrive
                for f0 in range(0, n, 32):
                    pipe.add_binary_frames(lecture[f0:f0 + 32])
                sync()
                t0 = time.perf_counter()
                out = pipe.finish(keyframes="device")
                sync()
                if rep:
                    walls[method].append(time.perf_counter() - t0)
                intervals[method] = [tuple(int(v) for v in iv) for iv in out["intervals"]]
                if method == "1":
                    kept = pipe                             # step 04 alone, below
                del pipe, out
        result["finish"] = {"n_frames": n, "erase_every": 60, "keyframes": "device", "warmup": 1,
                            "method_1": dict(summary(walls["1"]), n_intervals=len(intervals["1"])),
                            "method_3": dict(summary(walls["3"]), n_intervals=len(intervals["3"]))}
        # what method 1 itself adds to finish(): the sums from the device and the tree on the host, on the finished pipeline (the
        # rest of the difference between the two methods is step 05 working on other intervals)
        import contextlib
        import io
        from lecturemath_amd import pipeline
        step04 = pipeline._script("pre_ST3D_v3.0_04_vid_segmentation.py")
        t_sums, t_tree = [], []
        for rep in range(1 + 5):
            sync()
            t0 = time.perf_counter()
            all_sums = [int(v) / 255 for v in kept.estimator.reconstructed_frame_sums()]
            t1 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                again = step04.sums_intervals(kept.process, all_sums)
            t2 = time.perf_counter()
            assert [tuple(int(v) for v in iv) for iv in again] == intervals["1"]
            if rep:
                t_sums.append(t1 - t0)
                t_tree.append(t2 - t1)
        result["finish"]["method_1_step04_alone"] = {"reconstructed_frame_sums": summary(t_sums), "sums_intervals": summary(t_tree)}
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
