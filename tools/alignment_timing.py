"""What the translation alignment of keyframes (Aligner.computeTranslationAlignment, the first stage of the reference's summary
evaluation) costs on the device, and what the reference's loop costs on this machine's CPU.

    python tools/alignment_timing.py [--out profiles/r11_alignment.json]

65 synthetic 1080p keyframes (5 % ink; every image is its predecessor moved by a few pixels, with noise), window 10.  Timed with HIP
events, 2 warm-up rounds, median of 7:

  set_images_host     lm_align_set_images of the 65 images from a numpy array (upload + bit packing)
  set_images_device   the same images already on the device as one uint8 tensor (bit packing alone)
  match_64_pairs      lm_align_run on the 64 pairs of consecutive images (counts copied to the host)
  match_1_pair        lm_align_run on one pair
  numpy_1_pair        the reference's loop over the 441 displacements on ONE pair, stated here in numpy (slices, two comparisons, AND,
                      count) and timed with the wall clock on one core of this machine

The routes must give equal counts.  Not measured: how set_images divides between the upload and the packing kernel on the host
route beyond the difference of the two set_images figures, and how lm_align_run divides between the kernel and the copy of the
counts.  Needs the GPU (--lib PATH runs the same code on another build, e.g. the emulated one at a small --size and --images, as
a rehearsal that writes no profile)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

WARMUP, REPEATS = 2, 7


def make_images(n, h, w, seed):
    rng = np.random.default_rng(seed)
    ink = rng.random((h, w)) < 0.05
    out = np.zeros((n, h, w), np.uint8)
    for k in range(n):
        out[k] = np.where(ink, 0, 255)
        sy, sx = (int(v) for v in rng.integers(-6, 7, 2))
        ink = np.roll(ink, (sy, sx), axis=(0, 1)) ^ (rng.random((h, w)) < 0.002)
    return out


def numpy_pair(first, second, window, lum):
    """match counts of one pair the way the reference obtains them"""
    h, w = first.shape
    out = np.zeros((2 * window + 1, 2 * window + 1), np.int64)
    for dy in range(-window, window + 1):
        for dx in range(-window, window + 1):
            a = first[max(0, dy):h + min(0, dy), max(0, dx):w + min(0, dx)]
            b = second[max(0, -dy):h + min(0, -dy), max(0, -dx):w + min(0, -dx)]
            out[dy + window, dx + window] = np.count_nonzero(np.logical_and(a == b, a == lum))
    return out


def summary(v):
    v = v[WARMUP:]
    return {"median_s": statistics.median(v), "min_s": min(v), "max_s": max(v), "warmup": WARMUP, "repeats": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--images", type=int, default=65)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--seed", type=int, default=20211)
    ap.add_argument("--lib", default=None, help="another build of the library (rehearsal: nothing is written)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_alignment.json"))
    args = ap.parse_args()
    width, height = (int(v) for v in args.size.split("x"))
    if args.lib is None:
        import torch                            # before the library: both must end up on the HIP runtime torch brings along
        if not torch.cuda.is_available():
            raise SystemExit("alignment_timing: needs a GPU")
    from lecturemath_amd import _lib, device
    lib = _lib.load(args.lib)
    if not lib.is_device_build and args.lib is None:
        raise SystemExit("alignment_timing: needs the HIP library and a GPU")
    be = device.Backend(lib)
    n, w = args.images, args.window
    images = make_images(n, height, width, args.seed)
    pairs = [(i, i + 1) for i in range(n - 1)]
    al = device.TranslationAligner(width, height, max_images=n, max_window=w, lib=lib)

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

    dev_images = be.from_host(images)
    be.synchronize()
    t = {"set_images_host": [], "set_images_device": [], "match_64_pairs": [], "match_1_pair": [], "numpy_1_pair": []}
    want_one = None
    for rep in range(WARMUP + REPEATS):         # the routes alternating
        _, s = timed(lambda: al.set_images(images, content_lum=0))
        t["set_images_host"].append(s)
        host_counts, _ = timed(lambda: al.match_counts(pairs, w))
        host_totals = al.totals().copy()
        _, s = timed(lambda: al.set_images(dev_images, content_lum=0, on_device=True))
        t["set_images_device"].append(s)
        counts, s = timed(lambda: al.match_counts(pairs, w))
        t["match_64_pairs"].append(s)
        one, s = timed(lambda: al.match_counts(pairs[:1], w))
        t["match_1_pair"].append(s)
        t0 = time.perf_counter()
        want_one = numpy_pair(images[0], images[1], w, 0)
        t["numpy_1_pair"].append(time.perf_counter() - t0)
        assert (counts == host_counts).all() and (al.totals() == host_totals).all(), "host and device images disagree"
        assert (one[0] == counts[0]).all() and (one[0] == want_one).all(), "the device and the numpy loop disagree"
    best = al.align(pairs, w)
    result = {"width": width, "height": height, "n_images": n, "n_pairs": len(pairs), "window": w, "seed": args.seed,
              "ink_pixels_per_image": {"min": int(host_totals.min()), "max": int(host_totals.max())},
              "displacements_found": sorted({(t_[3], t_[4]) for t_ in best})[:8],
              "timing": {k: summary(v) for k, v in t.items()},
              "clock": {"device": "HIP events around the call (set_images from device memory is asynchronous, the others end in a "
                                  "stream synchronise)", "numpy_1_pair": "time.perf_counter, one core"}}
    tm = result["timing"]
    per_pair = tm["match_64_pairs"]["median_s"] / len(pairs)
    result["per_pair_s"] = {"device_batched": per_pair, "device_single": tm["match_1_pair"]["median_s"], "numpy": tm["numpy_1_pair"]["median_s"]}
    host_spread = tm["numpy_1_pair"]["max_s"] - tm["numpy_1_pair"]["min_s"]
    result["device_faster_than_host_minus_spread"] = bool(tm["match_1_pair"]["median_s"] < tm["numpy_1_pair"]["median_s"] - host_spread)
    al.close()
    print(json.dumps(result, indent=1))
    if lib.is_device_build:
        assert result["device_faster_than_host_minus_spread"], "one pair on the device is not faster than the numpy loop minus its spread"
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    else:
        print("rehearsal on %s: no profile written" % lib.path)


if __name__ == "__main__":
    main()
