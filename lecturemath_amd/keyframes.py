"""Keyframe objects over keyframes that stay on the device: what the reference's summary evaluation reads from a
KeyFrameAnnotation (AccessMath/annotation/keyframe_annotation.py: idx, time, objects, raw_image, binary_image, binary_cc, object_mask,
update_binary_cc :139-146, check_cc_overlaps_background :80-100, GenerateFakeKeyframeInfo :550-564), with the connected components
labelled on the device into one bit-row table for the whole set (device.KeyframeCCs).

    kfs = keyframes_from_frames(out["keyframes_device"], masks)     # one table
    groups, cc_group, segments = generate_fake_keyframe_info(kfs)
    Evaluator.compute_summary_metrics(...)                          # counts on the table, nothing is uploaded
    Evaluator.compute_pixel_binary_metrics(gt_kfs, kfs)             # integer sums on the device

Not covered: update_object_mask (cv2.fillPoly), LoadExportedKeyframes and the XML / portion machinery of the annotation package;
CombineKeyframesPerSegment (AND the frames before keyframes_from_frames)."""
import os
import sys

import numpy as np

from . import device

_DROPIN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dropin")


class KeyframeSet:
    """what the keyframes of one keyframes_from_frames call share: the table, the frames and the masks where the library reads them"""

    def __init__(self, table, frames, masks_device, masks_host):
        self.table, self.frames, self.masks_device, self.masks_host = table, frames, masks_device, masks_host
        self.be = table.be

    def close(self):
        self.table.close()


class DeviceKeyframe:
    def __init__(self, kset, k, idx, time, objects=None, raw_image=None):
        self.set, self.k = kset, int(k)
        self.idx, self.time, self.objects, self.raw_image = idx, time, objects, raw_image
        self.object_mask = kset.masks_host[self.k]
        self.binary_cc = kset.table.ccs(self.k)
        self._binary_image = None

    @property
    def table(self):
        return self.set.table

    @property
    def binary_image(self):
        """host copy [H][W][3], made on first access"""
        if self._binary_image is None:
            plane = self.set.be.to_host(self.set.frames[self.k])
            plane = np.asarray(plane)
            if plane.ndim == 2:
                plane = np.repeat(plane[:, :, None], 3, axis=2)
            elif plane.shape[2] != 3:
                plane = np.repeat(plane[:, :, :1], 3, axis=2)
            self._binary_image = np.ascontiguousarray(plane)
        return self._binary_image

    def update_binary_cc(self, verbose=True):
        """the CCs came with the table: nothing to compute, the list stays"""
        if verbose:
            print("Computing CC for frame: " + str(self.idx))
            print("    Found: " + str(len(self.binary_cc)) + " CCs")

    def check_cc_overlaps_background(self, cc):
        mask = self.object_mask
        if cc.max_x < 0 or cc.min_x >= mask.shape[1] or cc.max_y < 0 or cc.min_y >= mask.shape[0]:
            return True         # wholly outside the frame: taken as background
        cut = mask[cc.min_y:cc.max_y + 1, cc.min_x:cc.max_x + 1]      # a numpy slice: a negative start wraps, as in the reference
        y0, x0 = max(0, -cc.min_y), max(0, -cc.min_x)
        own = cc.img[y0:y0 + cut.shape[0], x0:x0 + cut.shape[1]]
        return np.count_nonzero(np.logical_and(own, cut)) > 0


def keyframes_from_frames(frames, masks=None, idxs=None, times=None, min_pixels=1, max_batch=8, lib=None):
    """frames: [n][H][W] or [n][H][W][C] uint8, a numpy array or a torch device tensor (kept where it is); masks: [n][H][W] host array,
    non-zero = object, or None (no objects).  One device.KeyframeCCs for the whole set; returns the list of DeviceKeyframe."""
    if _DROPIN not in sys.path and "AM_CommonTools" not in sys.modules:
        sys.path.insert(0, _DROPIN)
    n, height, width = (int(v) for v in frames.shape[:3])
    if masks is None:
        masks_host = np.zeros((n, height, width), bool)
    else:
        masks_host = np.asarray(masks) != 0
        if masks_host.shape != (n, height, width):
            raise ValueError("keyframes_from_frames: masks of shape %s, expected %s" % (masks_host.shape, (n, height, width)))
    from . import _lib
    be = device.Backend(lib or _lib.load())
    on_device = bool(hasattr(frames, "data_ptr") and frames.is_cuda)
    masks_device = be.from_host(masks_host.astype(np.uint8))        # read by the table (device frames) and by the pixel sums
    table = device.KeyframeCCs.from_frames(frames, masks=masks_device if on_device else masks_host, min_pixels=min_pixels,
                                           max_batch=max_batch, lib=lib)
    dev_frames = frames.contiguous() if on_device else be.from_host(np.ascontiguousarray(np.asarray(frames, np.uint8)))
    kset = KeyframeSet(table, dev_frames, masks_device, masks_host)
    out = []
    for k in range(n):
        kf = DeviceKeyframe(kset, k, idxs[k] if idxs is not None else k, times[k] if times is not None else float(k))
        table.register_mask(k, kf.object_mask)
        out.append(kf)
    return out


def generate_fake_keyframe_info(keyframes):
    """KeyFrameAnnotation.GenerateFakeKeyframeInfo: every CC of every keyframe is a unique CC of its own, keyframe k lives in the
    segment (5 k + 1, 5 k + 4)"""
    if _DROPIN not in sys.path and "AccessMath" not in sys.modules:
        sys.path.insert(0, _DROPIN)
    from AccessMath.evaluation.evaluator import UniqueCCGroup
    groups, cc_group, segments = [], [], []
    for k, keyframe in enumerate(keyframes):
        segments.append((k * 5 + 1, k * 5 + 4))
        cc_group.append({})
        for cc in keyframe.binary_cc:
            group = UniqueCCGroup(cc, k)
            groups.append(group)
            cc_group[k][cc.strID()] = group
    return groups, cc_group, segments


def pixel_sum_pairs(gt_frames, summary_frames):
    """uint64 [n][4] sums (device.pixel_sums) for gt_frames[i] against summary_frames[i], masks = the ground truth's; None when a
    keyframe of either list is not a DeviceKeyframe or the frames differ in size"""
    n = len(gt_frames)
    if n == 0 or len(summary_frames) < n or not all(isinstance(kf, DeviceKeyframe) for kf in list(gt_frames) + list(summary_frames[:n])):
        return None
    if any(tuple(g.set.frames.shape[1:3]) != tuple(s.set.frames.shape[1:3]) for g, s in zip(gt_frames, summary_frames)):
        return None
    lib = gt_frames[0].set.table.lib
    gs, ss = gt_frames[0].set, summary_frames[0].set
    one_run = all(g.set is gs and s.set is ss and g.k == gt_frames[0].k + i and s.k == summary_frames[0].k + i
                  for i, (g, s) in enumerate(zip(gt_frames, summary_frames)))
    if one_run:
        g0, s0 = gt_frames[0].k, summary_frames[0].k
        return device.pixel_sums(gs.frames[g0:g0 + n], ss.frames[s0:s0 + n], gs.masks_device[g0:g0 + n], lib=lib)
    return np.concatenate([device.pixel_sums(g.set.frames[g.k:g.k + 1], s.set.frames[s.k:s.k + 1], g.set.masks_device[g.k:g.k + 1], lib=lib)
                           for g, s in zip(gt_frames, summary_frames)])
