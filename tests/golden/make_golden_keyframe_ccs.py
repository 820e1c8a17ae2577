#!/usr/bin/env python3
"""G24: the reference's keyframe CCs and what its evaluation script does with them (lecturenet_eval_keyframe_bin.py:
KeyFrameAnnotation.update_binary_cc, GenerateFakeKeyframeInfo, Evaluator.compute_summary_metrics, compute_pixel_binary_metrics), run
in THIS container with the UNMODIFIED reference.  Stored in g24_keyframe_ccs.npz: inputs and returned values only.

Inputs: two sets of three keyframes of 45 x 70, a "ground truth" and a "binarized" one.  Ground truth: noise at 30 % ink (hundreds of
CCs, many of one pixel), noise at 10 %, a sheet of small strokes with non-binary bytes (17, 128, 254: all ink).  The binarized
keyframe k is the ground truth's moved by a pixel or two with a few percent of its pixels flipped.  Object masks: rectangles that
reach the frame's edges on the ground truth, none on the binarized side.
Recorded: the channel-0 planes and masks; per set the CC records (keyframe offsets, cc_id, box, size, packed img) that
update_binary_cc(False) leaves in binary_cc; GenerateFakeKeyframeInfo's segments, group keys per keyframe and (start_frame, strID)
per group; compute_summary_metrics with its range names and report texts; compute_pixel_binary_metrics of the sets and of a pair
with an empty binarized keyframe.  Values are bit-encoded as in G22 (make_golden_evaluation.encode).

Stand-ins: cv2 (tests/golden/_ref_shims), shapely.geometry (make_golden_alignment.shapely_stand_in).  The keyframes are
SimpleNamespace objects with the reference's own KeyFrameAnnotation methods bound to them."""
import contextlib
import io
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_env  # noqa: E402
from make_golden_alignment import shapely_stand_in  # noqa: E402
from make_golden_evaluation import encode  # noqa: E402

H, W = 45, 70


def make_planes():
    """(gt planes, gt masks, summ planes): uint8 [3][H][W] channel-0 bytes (255 = paper), bool masks"""
    rng = np.random.default_rng(24)
    gt = np.full((3, H, W), 255, np.uint8)
    gt[0][rng.random((H, W)) < 0.30] = 0
    gt[1][rng.random((H, W)) < 0.10] = 0
    for _ in range(40):                                     # strokes, some of them with bytes that are neither 0 nor 255
        y, x = int(rng.integers(0, H - 3)), int(rng.integers(0, W - 6))
        hh, ww = (1, int(rng.integers(2, 7))) if rng.random() < 0.5 else (int(rng.integers(2, 4)), 1)
        gt[2][y:y + hh, x:x + ww] = (0, 17, 128, 254)[int(rng.integers(0, 4))]
    summ = np.full((3, H, W), 255, np.uint8)
    for k, (dy, dx) in enumerate([(1, -2), (0, 1), (-1, 1)]):
        moved = np.full((H, W), 255, np.uint8)
        src = gt[k][max(0, -dy):H - max(0, dy), max(0, -dx):W - max(0, dx)]
        moved[max(0, dy):max(0, dy) + src.shape[0], max(0, dx):max(0, dx) + src.shape[1]] = src
        flip = rng.random((H, W)) < 0.03
        moved[flip] = np.where(moved[flip] == 255, 0, 255)
        summ[k] = moved
    masks = np.zeros((3, H, W), bool)
    for k in range(3):
        masks[k][0:12 + 3 * k, 0:20 + 2 * k] = True
        masks[k][H - 10:H, W - 25 - k:W] = True
        masks[k][20:30, 30:45] = True
    return gt, masks, summ


def keyframes_of(planes, masks, KeyFrameAnnotation):
    out = []
    for k, plane in enumerate(planes):
        kf = types.SimpleNamespace(idx=k, binary_image=np.repeat(plane[:, :, None], 3, axis=2), raw_image=np.zeros((H, W, 3), np.uint8),
                                   object_mask=masks[k].copy(), binary_cc=None)
        kf.check_cc_overlaps_background = types.MethodType(KeyFrameAnnotation.check_cc_overlaps_background, kf)
        KeyFrameAnnotation.update_binary_cc(kf, False)
        out.append(kf)
    return out


def pack_ccs(prefix, keyframes):
    ccs = [cc for kf in keyframes for cc in kf.binary_cc]
    off = np.zeros(len(keyframes) + 1, np.int64)
    off[1:] = np.cumsum([len(kf.binary_cc) for kf in keyframes])
    img_off = np.zeros(len(ccs) + 1, np.int64)
    img_off[1:] = np.cumsum([cc.img.size for cc in ccs])
    for cc in ccs:
        assert cc.img.dtype == np.uint8 and set(np.unique(cc.img).tolist()) <= {0, 255} and cc.start_time == 0.0 and cc.end_time == 0.0
    return {prefix + "_cc_off": off,
            prefix + "_cc_rec": np.asarray([(cc.cc_id, cc.min_x, cc.max_x, cc.min_y, cc.max_y, cc.size) for cc in ccs], np.int32).reshape(-1, 6),
            prefix + "_cc_img_off": img_off,
            prefix + "_cc_bits": np.packbits(np.concatenate([cc.img.ravel() > 0 for cc in ccs]))}


def fake_info(groups, cc_group, segments):
    return {"segments": [list(s) for s in segments], "keys": [list(d.keys()) for d in cc_group],
            "groups": [[g.start_frame, g.cc_refs[0].strID(), len(g.cc_refs)] for g in groups]}


def main():
    assert ref_env.available(), "reference not present: fixtures can only be regenerated in the build container"
    ref_env.enter()
    shapely_stand_in()
    from AccessMath.annotation.keyframe_annotation import KeyFrameAnnotation
    from AccessMath.evaluation.evaluator import Evaluator

    gt_planes, masks, summ_planes = make_planes()
    gt = keyframes_of(gt_planes, masks, KeyFrameAnnotation)
    summ = keyframes_of(summ_planes, np.zeros_like(masks), KeyFrameAnnotation)
    data = {"shape": np.asarray([H, W], np.int32), "gt_planes": gt_planes, "summ_planes": summ_planes, "gt_masks": np.packbits(masks, axis=2)}
    data.update(pack_ccs("gt", gt))
    data.update(pack_ccs("summ", summ))
    print("CCs per keyframe:", [len(kf.binary_cc) for kf in gt], [len(kf.binary_cc) for kf in summ])

    rec = {}
    gt_groups, gt_cc_group, gt_segments = KeyFrameAnnotation.GenerateFakeKeyframeInfo(gt)
    summ_groups, summ_cc_group, summ_segments = KeyFrameAnnotation.GenerateFakeKeyframeInfo(summ)
    rec["fake_gt"], rec["fake_summ"] = fake_info(gt_groups, gt_cc_group, gt_segments), fake_info(summ_groups, summ_cc_group, summ_segments)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        metrics, names = Evaluator.compute_summary_metrics(gt_segments, gt, gt_groups, gt_cc_group, summ_segments, summ)
    rec["metrics"], rec["range_names"] = encode(metrics), names
    prints = {}
    for name in names:
        for fn in ("print_summary_recall_metrics", "print_summary_precision_metrics", "print_compact_CC_metrics"):
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                getattr(Evaluator, fn)(metrics[name], name)
            prints[fn + "|" + name] = buf.getvalue()
    rec["prints"] = prints
    rec["pixel"] = encode(Evaluator.compute_pixel_binary_metrics(gt, summ))
    # degenerate branches: a binarized keyframe without ink (recall + precision = 0 after 0 / 0), and one whose ink all lies on objects
    empty = types.SimpleNamespace(binary_image=np.full((H, W, 3), 255, np.uint8))
    on_objects = np.full((H, W), 255, np.uint8)
    on_objects[2:6, 3:9] = 0                               # inside the first rectangle of mask 0
    covered = types.SimpleNamespace(binary_image=np.repeat(on_objects[:, :, None], 3, axis=2))
    apart = np.full((H, W), 255, np.uint8)                  # ink only where the ground truth has none: recall + precision = 0
    ys, xs = np.nonzero(gt_planes[0] == 255)
    apart[ys[::7], xs[::7]] = 0
    disjoint = types.SimpleNamespace(binary_image=np.repeat(apart[:, :, None], 3, axis=2))
    data["extra_planes"] = np.stack([empty.binary_image[:, :, 0], on_objects, apart])
    with np.errstate(all="ignore"):
        rec["pixel_empty"] = encode(Evaluator.compute_pixel_binary_metrics(gt[:1], [empty]))
    rec["pixel_covered"] = encode(Evaluator.compute_pixel_binary_metrics(gt[:1], [covered]))
    rec["pixel_disjoint"] = encode(Evaluator.compute_pixel_binary_metrics(gt[:1], [disjoint]))
    print("ranges:", names, "pixel:", {k: float(v) for k, v in Evaluator.compute_pixel_binary_metrics(gt, summ).items()})

    data["recorded"] = np.frombuffer(json.dumps(rec).encode(), np.uint8)
    path = os.path.join(HERE, "g24_keyframe_ccs.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
