#!/usr/bin/env python3
"""G22: the reference's summary evaluation (AccessMath/evaluation/evaluator.py) on small synthetic keyframes, run in THIS container
with the UNMODIFIED reference Evaluator.  Stored in g22_evaluation.npz: inputs and returned values only.

Inputs (frames of 100 x 160): a ground-truth set and a summary set of keyframes.  Every keyframe is a grid of cells; a cell holds
one scenario drawn on the ground-truth side and on the summary side (SCENARIOS below: identical blobs, blobs that share too little,
bars that share exactly 10 / 13 / 16 / 19 of 20 pixels, two-against-one, chains of four, one-sided, boxes that touch without
shared ink, one-pixel-wide strokes).  A keyframe shows a subset of the cells, moved as a whole by a few pixels, some cells by one
pixel more; one ground-truth keyframe is empty, one summary keyframe holds unrelated strokes.  The CC lists are the 8-connected
components of the ink; the object masks are rectangles that reach the frame's edges.
Per set: packed ink planes, packed object masks, CC boxes / sizes / packed masks, segments.

Recorded (JSON inside the npz; floats as int64 bit patterns, numpy scalars marked as such):
  equiv     check_equivalent_cc on hand-made pairs (stripes that tie, thin strokes, noisy copies)
  unique    keyframes_alignments + keyframes_unique_cc over the ground-truth set: the alignments, the group of every CC, cc_refs
  pairs     for (gt keyframe, summary keyframe, alignment) cases, some with displacements that move CCs out of the frame:
            keyframes_overlapping_ccs, match_overlapping_ccs at the four default threshold pairs, find_ccs_overlapping_background
  summary   summary_overlapping_ccs, compute_summary_metrics, the stdout of the three print_* functions per range
  pixel     compute_pixel_binary_metrics

Stand-ins: cv2 (tests/golden/_ref_shims), shapely.geometry (make_golden_alignment.shapely_stand_in).  The keyframes are
SimpleNamespace objects; check_cc_overlaps_background is the reference's own KeyFrameAnnotation method bound to them."""
import contextlib
import io
import json
import os
import struct
import sys
import types

import numpy as np
import scipy.ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_env  # noqa: E402
from make_golden_alignment import shapely_stand_in  # noqa: E402

H, W = 100, 160
CELL_W, CELL_H, ORIGIN = 21, 13, 5
COLS, ROWS = 7, 7

# scenario -> (rectangles of the ground-truth side, of the summary side), (y0, y1, x0, x1) inclusive, cell coordinates
SCENARIOS = {
    "exact": ([(2, 6, 3, 9), (7, 8, 3, 4)], [(2, 6, 3, 9), (7, 8, 3, 4)]),
    "exact_noisy": ([(2, 6, 3, 9)], [(2, 6, 4, 10)]),
    "rejected11": ([(1, 4, 1, 6)], [(4, 8, 6, 12)]),
    "two_one_acc": ([(2, 6, 1, 6), (2, 6, 9, 14)], [(2, 6, 2, 13)]),
    "two_one_rej": ([(2, 6, 1, 6), (2, 6, 9, 14)], [(5, 9, 5, 10)]),
    "one_two_acc": ([(2, 6, 2, 13)], [(2, 6, 1, 6), (2, 6, 9, 14)]),
    "one_two_rej": ([(5, 9, 5, 10)], [(2, 6, 1, 6), (2, 6, 9, 14)]),
    "chain_acc": ([(3, 5, 0, 6), (3, 5, 9, 15)], [(3, 5, 1, 10), (3, 5, 12, 17)]),
    "chain_rej": ([(1, 3, 0, 6), (1, 3, 9, 15)], [(3, 6, 5, 10), (3, 6, 14, 18)]),
    "gt_only": ([(2, 5, 2, 8), (6, 7, 2, 3)], []),
    "summ_only": ([], [(3, 7, 4, 9)]),
    "zero_touch": ([(0, 8, 0, 1), (7, 8, 0, 12)], [(1, 3, 6, 10)]),
    "thin_v": ([(1, 9, 4, 4)], [(1, 9, 4, 4)]),
    "thin_h": ([(5, 5, 2, 15)], [(5, 5, 2, 15)]),
}
for _k in (10, 13, 16, 19):             # bars of 20 pixels that share exactly k: recall = precision = k / 20
    _summ = [(3, 3, 2, 11)] + ([(4, 4, 2, 2 + (_k - 10) - 1)] if _k > 10 else []) + [(2, 2, 2, 2 + (20 - _k) - 1)]
    SCENARIOS["share_%d" % _k] = ([(3, 4, 2, 11)], _summ)

LAYOUT = ["exact", "share_10", "two_one_acc", "chain_acc", "gt_only", "zero_touch", "thin_v",
          "share_13", "rejected11", "one_two_acc", "chain_rej", "summ_only", "exact_noisy", "thin_h",
          "two_one_rej", "share_16", "exact", "one_two_rej", "zero_touch", "chain_acc", "share_19",
          "exact_noisy", "chain_rej", "share_10", "two_one_acc", "thin_v", "rejected11", "gt_only",
          "one_two_acc", "zero_touch", "share_13", "exact", "chain_acc", "summ_only", "share_16",
          "thin_h", "two_one_rej", "exact_noisy", "share_19", "one_two_rej", "chain_rej", "exact",
          "share_10", "zero_touch", "rejected11", "two_one_acc", "one_two_acc", "share_13", "chain_acc"]
assert len(LAYOUT) == COLS * ROWS


def bits_of(x):
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def encode(x):
    """JSON form of a returned value that keeps type and bits: float -> {"f": bits}, numpy float -> {"F": bits}, numpy integer ->
    {"I": v}, dict -> {"d": [[key, value], ...]} (order kept), tuple -> {"t": [...]}"""
    if isinstance(x, (bool, np.bool_)):
        return {"b": bool(x)}
    if isinstance(x, np.floating):
        return {"F": bits_of(x)}
    if isinstance(x, float):
        return {"f": bits_of(x)}
    if isinstance(x, np.integer):
        return {"I": int(x)}
    if isinstance(x, (int, str)):
        return x
    if isinstance(x, dict):
        return {"d": [[k, encode(v)] for k, v in x.items()]}
    if isinstance(x, tuple):
        return {"t": [encode(v) for v in x]}
    if isinstance(x, list):
        return [encode(v) for v in x]
    raise TypeError(type(x))


def draw(side, present, shift, jitter):
    """ink plane (bool): the cells of `present`, the whole drawing moved by shift = (dy, dx), cell c by jitter.get(c) more"""
    ink = np.zeros((H, W), bool)
    for c in present:
        cy, cx = ORIGIN + (c // COLS) * CELL_H, ORIGIN + (c % COLS) * CELL_W
        jy, jx = jitter.get(c, (0, 0))
        for y0, y1, x0, x1 in SCENARIOS[LAYOUT[c]][side]:
            ink[cy + y0 + shift[0] + jy:cy + y1 + 1 + shift[0] + jy, cx + x0 + shift[1] + jx:cx + x1 + 1 + shift[1] + jx] = True
    return ink


def unrelated(seed):
    rng = np.random.default_rng(seed)
    ink = np.zeros((H, W), bool)
    for _ in range(9):
        y, x = int(rng.integers(0, H - 3)), int(rng.integers(0, W - 30))
        ink[y:y + 2, x:x + 28] = True
    return ink


def make_sets():
    rng = np.random.default_rng(22)
    cells = list(range(COLS * ROWS))
    # ground truth: cells come and go; cell 0 lives through keyframes 0-3, cell 1 leaves after keyframe 0 and returns in keyframe 3
    gt_shift = [(0, 0), (2, -3), (-1, 2), (3, 4), None, (-2, -2), (1, 3)]
    gt_planes, gt_present = [], []
    for k, shift in enumerate(gt_shift):
        if shift is None:
            gt_planes.append(np.zeros((H, W), bool)); gt_present.append([])
            continue
        present = [c for c in cells if rng.random() < 0.7 or c == 0]
        if k in (1, 2) and 1 in present:
            present.remove(1)
        if k in (0, 3) and 1 not in present:
            present.append(1)
        jitter = {c: (int(rng.integers(-1, 2)), int(rng.integers(-1, 2))) for c in present if rng.random() < 0.3}
        gt_planes.append(draw(0, present, shift, jitter)); gt_present.append(present)
    # summaries: the summary side of the cells the ground-truth keyframe of that time shows (plus / minus a few), displaced
    summ_of = [0, 1, 2, 3, None, 5, 6, 6]
    summ_shift = [(3, -4), (-2, 5), (4, 2), (-5, -3), None, (2, 6), (-3, 1), (5, -6)]
    summ_planes = []
    for k, (g, shift) in enumerate(zip(summ_of, summ_shift)):
        if g is None:
            summ_planes.append(unrelated(5))
            continue
        present = [c for c in gt_present[g] if rng.random() < 0.9] + [c for c in cells if c not in gt_present[g] and rng.random() < 0.15]
        jitter = {c: (int(rng.integers(-1, 2)), int(rng.integers(-1, 2))) for c in present if rng.random() < 0.2}
        total = (gt_shift[g][0] + shift[0], gt_shift[g][1] + shift[1])
        summ_planes.append(draw(1, sorted(present), total, jitter))
    gt_segments = [(0, 100), (100, 200), (200, 300), (300, 400), (400, 500), (500, 600), (600, 700)]
    summ_segments = [(0, 90), (90, 210), (210, 290), (290, 380), (380, 520), (520, 560), (560, 640), (640, 700)]
    masks = []
    for k in range(len(gt_planes)):             # rectangles that reach the left / top and the right / bottom edges
        m = np.zeros((H, W), bool)
        m[0:40 + 3 * k, 0:30 + 2 * k] = True
        m[H - 35:H, W - 50 - k:W] = True
        m[30:60, 70:100] = True
        masks.append(m)
    return (gt_planes, masks, gt_segments), (summ_planes, [np.zeros((H, W), bool)] * len(summ_planes), summ_segments)


def components(ink, CC):
    labels, n = scipy.ndimage.label(ink, structure=np.ones((3, 3), int))
    out = []
    for k, sl in enumerate(scipy.ndimage.find_objects(labels)):
        img = (labels[sl] == k + 1).astype(np.uint8) * 255
        out.append(CC(k, sl[1].start, sl[1].stop - 1, sl[0].start, sl[0].stop - 1, int(np.count_nonzero(img)), img))
    return out


def keyframes_of(planes, masks, CC, KeyFrameAnnotation):
    out = []
    for k, (ink, mask) in enumerate(zip(planes, masks)):
        plane = np.where(ink, 0, 255).astype(np.uint8)
        kf = types.SimpleNamespace(idx=k, binary_image=np.repeat(plane[:, :, None], 3, axis=2), raw_image=np.zeros((H, W, 3), np.uint8),
                                   object_mask=mask.copy(), binary_cc=components(ink, CC))
        kf.check_cc_overlaps_background = types.MethodType(KeyFrameAnnotation.check_cc_overlaps_background, kf)
        out.append(kf)
    return out


def pack_set(prefix, keyframes, segments):
    ccs = [cc for kf in keyframes for cc in kf.binary_cc]
    off = np.zeros(len(keyframes) + 1, np.int64)
    off[1:] = np.cumsum([len(kf.binary_cc) for kf in keyframes])
    img_off = np.zeros(len(ccs) + 1, np.int64)
    img_off[1:] = np.cumsum([cc.img.size for cc in ccs])
    flat = np.concatenate([cc.img.ravel() > 0 for cc in ccs]) if ccs else np.zeros(0, bool)
    return {prefix + "_ink": np.packbits(np.stack([kf.binary_image[:, :, 0] == 0 for kf in keyframes]), axis=2),
            prefix + "_mask": np.packbits(np.stack([kf.object_mask for kf in keyframes]), axis=2),
            prefix + "_cc_off": off,
            prefix + "_cc_box": np.asarray([(cc.min_x, cc.max_x, cc.min_y, cc.max_y) for cc in ccs], np.int32).reshape(-1, 4),
            prefix + "_cc_size": np.asarray([cc.size for cc in ccs], np.int32),
            prefix + "_cc_img_off": img_off, prefix + "_cc_bits": np.packbits(flat),
            prefix + "_segments": np.asarray(segments, np.int64)}


def equiv_cases(CC):
    """(cc1, cc2, (dy, dx), window, min_recall, min_precision)"""
    rng = np.random.default_rng(3)
    cases = []

    def cc(x0, y0, img):
        img = np.asarray(img, np.uint8) * 255
        return CC(0, x0, x0 + img.shape[1] - 1, y0, y0 + img.shape[0] - 1, int(np.count_nonzero(img)), img)

    for n in range(8):                          # few stripes inside many: several displacements contain cc1 entirely
        period = 2 + n % 2
        big = np.zeros((6 + n % 3, 30), bool); big[:, ::period] = True
        small = np.zeros((big.shape[0] - 2 * (n % 2), 3 * period), bool); small[:, ::period] = True
        x0, y0 = 20 + 7 * n, 10 + 5 * n
        d = (int(rng.integers(-4, 5)), int(rng.integers(-4, 5)))
        cases.append((cc(x0 + 9 - d[1], y0 - d[0], small), cc(x0, y0, big), d, 3 if n % 4 else 2, 0.5 + 0.15 * (n % 3), 0.1))
    for n in range(6):                          # one pixel wide / high, identical: the strict box test rejects all displacements
        img = np.ones((1, 9 + n), bool) if n % 2 else np.ones((7 + n, 1), bool)
        d = (n - 2, 3 - n)
        cases.append((cc(40 - d[1], 30 - d[0], img), cc(40, 30, img), d, 3, 0.5, 0.5))
    for n in range(10):                         # noisy copies, some displaced beyond the window
        img = rng.random((8 + n, 12 + 3 * n)) < 0.55
        other = img ^ (rng.random(img.shape) < 0.08 * (n % 4))
        d = (int(rng.integers(-6, 7)), int(rng.integers(-6, 7)))
        off = (int(rng.integers(-2, 3)), int(rng.integers(-2, 3))) if n % 3 else (5, -5)
        cases.append((cc(60 - d[1] + off[1], 40 - d[0] + off[0], other), cc(60, 40, img), d, (1, 3, 3, 8)[n % 4], (0.5, 0.8, 0.95)[n % 3], (0.5, 0.8)[n % 2]))
    # 20 pixels against 20 that share 8 or 10: recall == min_recall is accepted, one step above is not
    cases.append((cc(33, 20, np.ones((4, 5), bool)), cc(30, 20, np.ones((4, 5), bool)), (0, 0), 0, 0.4, 0.4))
    cases.append((cc(35, 20, np.ones((2, 10), bool)), cc(30, 20, np.ones((2, 10), bool)), (0, 0), 0, 0.5, 0.5))
    cases.append((cc(35, 20, np.ones((2, 10), bool)), cc(30, 20, np.ones((2, 10), bool)), (0, 0), 0, 0.5, 0.51))
    return cases


def group_ids(info):
    return [sorted(cc.strID() for cc in info.frame1_ccs_refs), sorted(cc.strID() for cc in info.frame2_ccs_refs)]


def main():
    assert ref_env.available(), "reference not present: fixtures can only be regenerated in the build container"
    ref_env.enter()
    shapely_stand_in()
    from AM_CommonTools.data.connected_component import ConnectedComponent as CC
    from AccessMath.annotation.keyframe_annotation import KeyFrameAnnotation
    from AccessMath.evaluation.eval_parameters import EvalParameters
    from AccessMath.evaluation.evaluator import Evaluator

    (gt_planes, gt_masks, gt_segments), (summ_planes, summ_masks, summ_segments) = make_sets()
    gt = keyframes_of(gt_planes, gt_masks, CC, KeyFrameAnnotation)
    summ = keyframes_of(summ_planes, summ_masks, CC, KeyFrameAnnotation)
    data = {"shape": np.asarray([H, W], np.int32)}
    data.update(pack_set("gt", gt, gt_segments))
    data.update(pack_set("summ", summ, summ_segments))
    rec = {}

    # ---- check_equivalent_cc
    cases = equiv_cases(CC)
    eq_ccs = [cc for c in cases for cc in c[:2]]
    eq_off = np.zeros(len(eq_ccs) + 1, np.int64)
    eq_off[1:] = np.cumsum([cc.img.size for cc in eq_ccs])
    data["eq_box"] = np.asarray([(cc.min_x, cc.max_x, cc.min_y, cc.max_y) for cc in eq_ccs], np.int32)
    data["eq_size"] = np.asarray([cc.size for cc in eq_ccs], np.int32)
    data["eq_img_off"], data["eq_bits"] = eq_off, np.packbits(np.concatenate([cc.img.ravel() > 0 for cc in eq_ccs]))
    data["eq_disp"] = np.asarray([c[2] for c in cases], np.int32)
    data["eq_window"] = np.asarray([c[3] for c in cases], np.int32)
    data["eq_min"] = np.asarray([[bits_of(c[4]), bits_of(c[5])] for c in cases], np.int64)
    rec["equiv"] = [bool(Evaluator.check_equivalent_cc(c[0], c[1], (0.0, 0.0, 0.0, c[2][0], c[2][1]), c[3], c[4], c[5])) for c in cases]
    print("equiv:", len(cases), "true:", sum(rec["equiv"]))

    # ---- unique CCs of the ground truth
    aligns = Evaluator.keyframes_alignments(gt, EvalParameters.UniqueCC_global_tran_window, EvalParameters.UniqueCC_min_translation_fscore)
    groups, cc_group = Evaluator.keyframes_unique_cc(gt, aligns, EvalParameters.UniqueCC_local_trans_window, 0.5, 0.5)
    rec["unique"] = {"alignments": [encode(tuple(a)) for a in aligns],
                     "cc_groups": [[[cc.strID(), cc_group[k][cc.strID()].strID()] for cc in kf.binary_cc] for k, kf in enumerate(gt)],
                     "groups": [[g.start_frame, [cc.strID() for cc in g.cc_refs]] for g in groups]}
    print("unique:", len(groups), "groups, lengths", sorted(set(len(g.cc_refs) for g in groups)), "alignments", [a[3:] for a in aligns])

    # ---- pairs of keyframes under given alignments
    pair_cases = [(0, 0, -3, 4), (1, 1, 2, -5), (2, 2, -4, -2), (3, 3, 5, 3), (5, 5, -2, -6), (6, 6, 3, -1), (6, 7, -5, 6),
                  (0, 1, 0, 0), (3, 2, 1, 1), (4, 0, 0, 0), (2, 4, 3, 3),
                  (0, 0, -40, -70), (1, 1, 45, 80), (2, 2, -20, 5), (3, 3, 6, -60), (5, 5, 30, 60), (6, 6, -90, -150), (6, 7, 95, 155)]
    rec["pairs"] = []
    for g, s, dy, dx in pair_cases:
        align = (0.0, 0.0, 0.0, dy, dx)
        overlap_set = Evaluator.keyframes_overlapping_ccs(gt[g].binary_cc, summ[s].binary_cc, align)
        matches = []
        for min_r, min_p in zip(EvalParameters.UniqueCC_min_recall, EvalParameters.UniqueCC_min_precision):
            exact, partial, un1, un2 = Evaluator.match_overlapping_ccs(overlap_set, align, min_r, min_p)
            matches.append({"exact": [group_ids(i) for i in exact], "partial": [group_ids(i) for i in partial],
                            "un1": sorted(cc.strID() for cc in un1), "un2": sorted(cc.strID() for cc in un2)})
        bg = Evaluator.find_ccs_overlapping_background(gt[g], summ[s], align, False)
        rec["pairs"].append({"g": g, "s": s, "dy": dy, "dx": dx, "groups": [group_ids(i) for i in overlap_set], "match": matches, "bg": bg})
    print("pairs:", len(pair_cases), "groups:", sum(len(p["groups"]) for p in rec["pairs"]), "bg:", sum(len(p["bg"]) for p in rec["pairs"]))

    # ---- the whole summary evaluation
    window, min_align = EvalParameters.UniqueCC_global_tran_window, EvalParameters.UniqueCC_min_align_recall
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        all_overlapping, bg_overlaps = Evaluator.summary_overlapping_ccs(gt_segments, gt, summ_segments, summ, window, min_align, True)
    rec["summary"] = {"all": [[g, s, encode(tuple(a)), [group_ids(i) for i in ov]] for g, s, a, ov in all_overlapping],
                      "bg": [[[k, v] for k, v in d.items()] for d in bg_overlaps], "stdout": buf.getvalue()}
    metrics, names = Evaluator.compute_summary_metrics(gt_segments, gt, groups, cc_group, summ_segments, summ)
    rec["metrics"], rec["range_names"] = encode(metrics), names
    prints = {}
    for name in names:
        for fn in ("print_summary_recall_metrics", "print_summary_precision_metrics", "print_compact_CC_metrics"):
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                getattr(Evaluator, fn)(metrics[name], name)
            prints[fn + "|" + name] = buf.getvalue()
    rec["prints"] = prints
    print("summary pairs:", [(g, s, a[3], a[4]) for g, s, a, _ in all_overlapping], "ranges:", names)
    with np.errstate(all="ignore"):
        rec["pixel"] = encode(Evaluator.compute_pixel_binary_metrics(gt, summ[:len(gt)]))
        rec["pixel_nonempty"] = encode(Evaluator.compute_pixel_binary_metrics(gt[:4], summ[:4]))

    data["recorded"] = np.frombuffer(json.dumps(rec).encode(), np.uint8)
    path = os.path.join(HERE, "g22_evaluation.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
