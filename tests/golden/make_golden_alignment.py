#!/usr/bin/env python3
"""G21: the reference's Aligner.computeTranslationAlignment (AccessMath/preprocessing/content/aligner.py:27-83) and
Evaluator.keyframes_alignments (AccessMath/evaluation/evaluator.py:149-165), run in THIS container.  Stored in g21_alignment.npz:
inputs and returned tuples only.

(a) about 150 pairs of small images (at most 160 x 48): both content_lum values, both sort_by values, windows 0, 1, 3, 10 and
    min(h, w) (those that fit the image: the reference raises beyond min(h, w)), widths around the 32-bit word boundaries.  Kinds:
      shift   the second image is the first moved by a planted displacement inside the window, with noise;
      sparse  a handful of ink pixels in each image: many displacements tie for the maximum, recall (sort_by = 1) above all;
      gray    a shift case with a share of 128-valued pixels in both images (neither ink nor background);
      empty   one of the two images holds no ink: the reference returns (0.0, 0.0, 0.0, 0, 0).
    Per case: shape, (window, content_lum, sort_by), both images, the returned floats as int64 bit patterns, the displacement, and
    whether the f-score came back as the int 0 (the reference's `f_score = 0` branch) instead of a float.
(b) per golden stream the keyframes of its three G8 segmentations, one after the other, as SimpleNamespace(binary_image=...)
    objects through Evaluator.keyframes_alignments(keyframes, 10, 0.3).  A rejected alignment comes back as (0, 0, 0, 0, 0); when a
    stream yields none, one unrelated image (stored) is appended to its list.

Stand-ins for what the two modules import and never use on this path: cv2 (tests/golden/_ref_shims) and shapely.geometry, which
AccessMath.annotation pulls in for polygon objects."""
import os
import struct
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_env  # noqa: E402

WIDTHS = [5, 31, 32, 33, 64, 65, 70, 129]
WINDOWS = [0, 1, 3, 10, None]          # None: min(h, w)
STREAMS = ("accumulate_erase", "occluder_return", "short_gap_jitter")


def shapely_stand_in():
    if "shapely" not in sys.modules:
        sh, geo = types.ModuleType("shapely"), types.ModuleType("shapely.geometry")
        geo.Polygon = geo.Point = geo.LineString = type("Unused", (), {})
        sh.geometry = geo
        sys.modules["shapely"], sys.modules["shapely.geometry"] = sh, geo


def bits_of(x):
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def case_images(rng, kind, h, w, window, lum):
    """two uint8 images of one case; ink = lum, background = 255 - lum"""
    bg = 255 - lum
    if kind == "sparse":
        out = []
        for _ in range(2):
            img = np.full((h, w), bg, np.uint8)
            n = int(rng.integers(2, 7))
            img[rng.integers(0, h, n), rng.integers(0, w, n)] = lum
            out.append(img)
        return out
    ink = rng.random((h, w)) < rng.choice([0.08, 0.2, 0.4])
    sy, sx = (int(rng.integers(-window, window + 1)) for _ in range(2))
    if window > 0 and sy == 0 and sx == 0:
        sx = window
    moved = np.zeros_like(ink)
    ys, xs = np.nonzero(ink)
    keep = (ys + sy >= 0) & (ys + sy < h) & (xs + sx >= 0) & (xs + sx < w)
    moved[ys[keep] + sy, xs[keep] + sx] = True
    moved ^= rng.random((h, w)) < 0.03
    first, second = (np.where(m, lum, bg).astype(np.uint8) for m in (ink, moved))
    if kind == "gray":
        for img in (first, second):
            img[rng.random((h, w)) < 0.15] = 128
    if kind == "empty":
        (first if rng.random() < 0.5 else second)[:] = rng.choice([bg, 128])
    return [first, second]


def make_cases(Aligner):
    rng = np.random.default_rng(2021)
    shapes, params, first, second, floats, disp, f_is_int, kinds = [], [], [], [], [], [], [], []
    plan = []
    for k, w in enumerate(WIDTHS):              # every width with every window that fits, kinds and switches rotating
        for window in WINDOWS:
            plan.append((w, window, ("shift", "sparse", "gray")[(k + len(plan)) % 3]))
    for w in WIDTHS:                            # sparse and shift again with the other switches
        plan.append((w, 3, "sparse"))
        plan.append((w, 10, "sparse"))
        plan.append((w, 10, "shift"))
        plan.append((w, 1, "sparse"))
        plan.append((w, None, "shift"))
        plan.append((w, 3, "gray"))
        plan.append((w, 10, "empty"))
        plan.append((w, 0, "sparse"))
    for w in (33, 64, 70, 129, 160, 160, 5, 31):
        plan.append((w, 3, "empty"))
        plan.append((w, 10, "gray"))
        plan.append((w, None, "sparse"))
        plan.append((w, 1, "shift"))
        plan.append((w, 3, "shift"))
    plan += [(160, 10, "shift"), (160, None, "shift"), (160, 10, "sparse"), (96, 10, "gray"), (127, 3, "sparse"), (128, 10, "shift")]
    for n, (w, window, kind) in enumerate(plan):
        h = 48 if (w == 160 and n % 2) else int(rng.choice([3, 7, 12, 20, 33, 48]))
        if window is None:
            window = min(h, w)
        window = min(window, min(h, w))
        lum, sort_by = (255, 0)[n % 2], (0, 1)[(n // 2) % 2]
        if kind == "sparse":
            sort_by = (1, 1, 0)[n % 3]
        a, b = case_images(rng, kind, h, w, window, lum)
        got = Aligner.computeTranslationAlignment(a, b, window, lum, sort_by)
        assert len(got) == 5 and all(isinstance(v, float) for v in got[1:3]) and type(got[0]) in (float, int)
        shapes.append((h, w)); params.append((window, lum, sort_by)); kinds.append(kind)
        first.append(a.ravel()); second.append(b.ravel())
        floats.append([bits_of(v) for v in got[:3]]); disp.append((int(got[3]), int(got[4]))); f_is_int.append(type(got[0]) is int)
    off = np.zeros(len(shapes) + 1, np.int64)
    off[1:] = np.cumsum([h * w for h, w in shapes])
    print("cases:", len(shapes), "non-zero displacement:", sum(1 for d in disp if d != (0, 0)), "int f-score:", sum(f_is_int),
          "pixels:", int(off[-1]))
    return {"shapes": np.asarray(shapes, np.int32), "params": np.asarray(params, np.int32), "off": off, "first": np.concatenate(first),
            "second": np.concatenate(second), "floats": np.asarray(floats, np.int64), "disp": np.asarray(disp, np.int32),
            "f_is_int": np.asarray(f_is_int, bool), "kinds": np.frombuffer(",".join(kinds).encode(), np.uint8)}


def unrelated_image(h, w):
    """strokes that share nothing with a synthetic lecture's glyphs"""
    rng = np.random.default_rng(7)
    img = np.full((h, w), 255, np.uint8)
    for _ in range(12):
        y, x = int(rng.integers(0, h - 8)), int(rng.integers(0, w - 40))
        img[y:y + 2, x:x + 40] = 0
    return img


def make_keyframes(Evaluator):
    out = {}
    for name in STREAMS:
        g = np.load(os.path.join(HERE, "g8_step05_%s.npz" % name))
        w = int(g["w"])
        planes = [np.unpackbits(g["keyframes_%d" % k], axis=2)[:, :, :w] * np.uint8(255) for k in range(3)]
        planes = list(np.concatenate(planes))
        extra = np.zeros((0, 0), np.uint8)

        def run():
            frames = [types.SimpleNamespace(binary_image=np.repeat(p[:, :, None], 3, axis=2)) for p in planes]
            return Evaluator.keyframes_alignments(frames, 10, 0.3)

        res = run()
        if not any(r == (0, 0, 0, 0, 0) and type(r[0]) is int for r in res):
            extra = unrelated_image(*planes[0].shape)
            planes.append(extra)
            res = run()
        rejected = [type(r[0]) is int and r == (0, 0, 0, 0, 0) for r in res]
        assert any(rejected), name
        out["kf_extra_" + name] = np.packbits(extra == 255, axis=1) if extra.size else np.zeros((0, 0), np.uint8)
        out["kf_floats_" + name] = np.asarray([[bits_of(v) for v in r[:3]] for r in res], np.int64)
        out["kf_disp_" + name] = np.asarray([(int(r[3]), int(r[4])) for r in res], np.int32)
        out["kf_rejected_" + name] = np.asarray(rejected, bool)
        print(name, len(planes), "keyframes, rejected:", rejected, "displacements:", out["kf_disp_" + name].tolist())
    return out


if __name__ == "__main__":
    assert ref_env.available(), "reference not present: fixtures can only be regenerated in the build container"
    ref_env.enter()
    shapely_stand_in()
    from AccessMath.preprocessing.content.aligner import Aligner  # noqa: E402
    from AccessMath.evaluation.evaluator import Evaluator  # noqa: E402
    data = make_cases(Aligner)
    data.update(make_keyframes(Evaluator))
    path = os.path.join(HERE, "g21_alignment.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")
