"""VideoSegmenter (AccessMath/preprocessing/content/video_segmenter.py) -- the parts step 04 uses with VIDEO_SEGMENTATION_METHOD = 3
(deletion events, the shipped configuration): compute_binary_sums (:22-28), find_signal_peaks (:133-182), split_video_from_group_deletes
(:499-520); and with method 2 (conflict minimisation): split_video_from_group_conflicts (:186-398), merge_conflict_plot_data (:401-422),
from_group_conflicts (:457-473), from_group_conflicts_with_presegments (:476-496).  Same names, arguments and return values.

compute_binary_sums accepts what the reference accepts (a list of uint8 frames) and, additionally, a device tensor [n, H, W]
as produced by CCStabilityEstimator.frames_from_groups_device -- then the sums are reduced on the GPU (lm_frame_sums).

Method 2 rebuilds, for every node of its recursive split, the per-frame sum of the weights of all conflicting group pairs whose gap
covers the frame.  Here the pairs are flattened once, in the reference's iteration order and with its float64 weight expression, and
the sums come from the device (lecturemath_amd.device.ConflictSignal, lm_conflict_signal), which adds them per frame in that order:
the signal is bit-identical to the reference's, whose peaks are decided by `>` on those sums.  lecturemath_amd is imported when the
first signal is needed, so this module loads on its own.

Method 1 (sums + regression tree): create_regresor_from_sums (:31-40), get_tree_decision_boundaries (:43-55),
identify_descend_intervals (:58-86), video_segments_from_erasing_intervals (:89-99), video_segments_from_sums (:102-130).  The tree is
restated in sum_tree.py beside this file, bit-identical to the reference's sklearn regressor on these inputs; sklearn is not imported."""
import collections.abc

import numpy as np


class _SegmentSignal(collections.abc.Mapping):
    """conflicts_per_frame of one node: reads like the reference's {frame: float} dict of the frames start .. start + len - 1, backed
    by the float64 array the device returned."""

    def __init__(self, start_frame, values):
        self.start_frame, self.values = int(start_frame), values

    def __getitem__(self, frame_idx):
        k = frame_idx - self.start_frame
        if not 0 <= k < len(self.values):
            raise KeyError(frame_idx)
        return float(self.values[k])

    def __iter__(self):
        return iter(range(self.start_frame, self.start_frame + len(self.values)))

    def __len__(self):
        return len(self.values)


class _ConflictPairs:
    """The conflicting pairs of groups of one lecture as the arrays lm_conflict_signal reads, in the order the reference's loops
    visit them (video_segmenter.py:198-216: `for group_idx in group_ages`, `for other_idx in group_conflicts[group_idx]`, pairs with
    group_idx < other_idx whose other group exists), each with the weight the reference computes for it (:235-274).  Built when the
    first node needs a signal (the reference touches nothing for a segment below min_segment_split) and uploaded once.
    A pair whose weight divides by zero is remembered instead: the reference raises for it at the first node where both of its
    groups are alive, and so does signal()."""

    def __init__(self, group_ages, group_conflicts, weight_area, weight_pixels, weight_time, n_frames, area_divisor=None):
        self.args = (group_ages, group_conflicts, weight_area, weight_pixels, weight_time, n_frames, area_divisor)
        self.device_signal = None
        self.failing = []

    @staticmethod
    def flatten(group_ages, group_conflicts, weight_area, weight_pixels, weight_time, n_frames, area_divisor=None):
        """-> (gap_first, gap_last, alive_from, alive_until, weight) and the [(alive_from, alive_until, ZeroDivisionError)] list"""
        VS = VideoSegmenter
        gap_first, gap_last, alive_from, alive_until, weights, failing = [], [], [], [], [], []
        for group_idx in group_ages:
            group_first, group_last = group_ages[group_idx][0], group_ages[group_idx][-1]
            row = group_conflicts[group_idx]
            for other_idx in row:
                if not (group_idx < other_idx and other_idx in group_ages):
                    continue
                other_first, other_last = group_ages[other_idx][0], group_ages[other_idx][-1]
                if group_first < other_first:           # the older group's last frame .. the newer group's first frame - 1
                    conflict_start, conflict_end = group_last, other_first - 1
                else:
                    conflict_start, conflict_end = other_last, group_first - 1
                d = row[other_idx]
                a_from, a_until = max(group_first, other_first), min(group_last, other_last)
                try:
                    if weight_time == VS.ConflictsTimeWeightGap:
                        time_weight = (conflict_end - conflict_start + 1)
                    elif weight_time == VS.ConflictsTimeWeightNormalizedLength:
                        time_weight = ((group_last - group_first + 1) + (other_last - other_first + 1)) / n_frames
                    else:
                        time_weight = 1
                    if weight_pixels == VS.ConflictsPixelsWeightsMatched:
                        pixel_weight = d["matched"]
                    elif weight_pixels == VS.ConflictsPixelsWeightsUnmatched:
                        pixel_weight = d["unmatched"]
                    elif weight_pixels == VS.ConflictsPixelsWeightsIOU:
                        intersection = d["matched"]
                        union = (d["matched"] + d["unmatched"])
                        pixel_weight = 1 - (intersection / union)
                    else:
                        pixel_weight = 1
                    if weight_area == VS.ConflictsAreaWeightsIntersection:
                        area_weight = d["area_intersection"] if area_divisor is None else d["area_intersection"] / area_divisor
                    elif weight_area == VS.ConflictsAreaWeigthsUnion:
                        area_weight = d["area_union"] if area_divisor is None else d["area_union"] / area_divisor
                    elif weight_area == VS.ConflictsAreaWeightsIOU:
                        area_weight = (d["area_intersection"] / d["area_union"])
                    else:
                        area_weight = 1
                    conflict_weight = float(area_weight * pixel_weight * time_weight)
                except ZeroDivisionError as error:
                    failing.append((a_from, a_until, error))
                    continue
                gap_first.append(conflict_start)
                gap_last.append(conflict_end)
                alive_from.append(a_from)
                alive_until.append(a_until)
                weights.append(conflict_weight)
        return (np.asarray(gap_first, np.int32), np.asarray(gap_last, np.int32), np.asarray(alive_from, np.int32),
                np.asarray(alive_until, np.int32), np.asarray(weights, np.float64)), failing

    def signal(self, start_frame, end_frame):
        if self.device_signal is None:
            from lecturemath_amd import device
            pairs, self.failing = self.flatten(*self.args)
            self.device_signal = device.ConflictSignal(pairs)
        for a_from, a_until, error in self.failing:
            if a_from <= end_frame and a_until >= start_frame:
                raise error
        return self.device_signal.signal(start_frame, end_frame)


class VideoSegmenter:
    ConflictsAreaWeightsCount = 0
    ConflictsAreaWeigthsUnion = 3
    ConflictsAreaWeightsIntersection = 4
    ConflictsAreaWeightsIOU = 5

    ConflictsPixelsWeightsNone = 0
    ConflictsPixelsWeightsMatched = 1
    ConflictsPixelsWeightsUnmatched = 2
    ConflictsPixelsWeightsIOU = 3

    ConflictsTimeWeightNone = 0
    ConflictsTimeWeightGap = 1
    ConflictsTimeWeightNormalizedLength = 2

    @staticmethod
    def compute_binary_sums(all_binary):
        if not isinstance(all_binary, (list, tuple)) and hasattr(all_binary, "shape") and len(all_binary.shape) == 3 and \
                not isinstance(all_binary, np.ndarray):
            from lecturemath_amd import device
            return [int(v) / 255 for v in device.frame_sums(all_binary)]
        return [binary.sum() / 255 for binary in all_binary]

    @staticmethod
    def find_signal_peaks(start_frame, end_frame, signal_dict):
        """Peaks of signal[start_frame .. end_frame] as (first frame, frame of the maximum reached while rising, last frame)
        (video_segmenter.py:133-182).  A peak ends where the signal, having fallen, rises again; plateaus keep the direction.
        Formulated on the sign of the first difference: the peaks are delimited by the rising steps that follow a falling
        step, and a peak's top is the last rising step before its first falling one."""
        n = end_frame - start_frame + 1
        if n <= 0:
            return []
        values = np.fromiter((signal_dict[f] for f in range(start_frame, end_frame + 1)), dtype=np.float64, count=n)
        return VideoSegmenter._peaks_of_values(start_frame, end_frame, values)

    @staticmethod
    def _peaks_of_values(start_frame, end_frame, values):
        """find_signal_peaks on the float64 array of the frames start_frame .. end_frame"""
        step = np.sign(np.diff(values)).astype(np.int8)             # step[k]: frame start + k + 1 against the one before
        moves = np.flatnonzero(step)                                 # plateaus carry no information
        rising = step[moves] > 0
        # a new peak starts at every rising step whose previous move was a fall
        starts_new = np.flatnonzero(rising[1:] & ~rising[:-1]) + 1 if len(moves) > 1 else np.zeros(0, np.int64)
        first_move = np.concatenate([[0], starts_new])              # index into `moves` of every peak's first move
        last_move = np.concatenate([starts_new, [len(moves)]])      # one past its last move
        begins = np.concatenate([[start_frame], start_frame + 1 + moves[starts_new]]) if len(moves) else np.array([start_frame])
        ends = np.concatenate([begins[1:] - 1, [end_frame]])
        peaks = []
        for k in range(len(begins)):
            top = int(begins[k])
            seg = rising[first_move[k]:last_move[k]] if len(moves) else rising[:0]
            if len(seg) and seg[0]:                                  # leading run of rises (the very first peak may start falling)
                falls = np.flatnonzero(~seg)
                run = len(seg) if len(falls) == 0 else int(falls[0])
                top = start_frame + 1 + int(moves[first_move[k] + run - 1])
            peaks.append((int(begins[k]), top, int(ends[k])))
        return peaks

    @staticmethod
    def split_video_from_group_deletes(signal, start_frame, end_frame, min_length, threshold):
        """Recursive split at the highest sufficiently prominent peak top that leaves min_length frames on both sides
        (video_segmenter.py:499-520); ties go to the later frame.  Returned intervals are in temporal order.  Worked through
        with an explicit stack (right part pushed first, so leaves come out left to right like the recursion's)."""
        intervals = []
        todo = [(start_frame, end_frame)]
        while todo:
            lo, hi = todo.pop()
            tops = np.array([top for _, top, _ in VideoSegmenter.find_signal_peaks(lo, hi, signal)], dtype=np.int64)
            if len(tops):
                heights = np.array([signal[t] for t in tops], dtype=np.float64)
                keep = (heights > threshold) & (tops >= lo + min_length) & (tops <= hi - min_length)
                tops, heights = tops[keep], heights[keep]
            if len(tops) == 0:
                print(str([(lo, hi)]) + " no good split candidates found")
                intervals.append((lo, hi))
                continue
            best = int(tops[np.lexsort((tops, heights))[-1]])       # highest, then latest
            todo.append((best + 1, hi))
            todo.append((lo, best - 1))
        return intervals

    @staticmethod
    def create_regresor_from_sums(all_sums, leaf_min):
        """The regression tree over (frame number, sum) with leaves of at least leaf_min frames (video_segmenter.py:31-40): an object
        with predict(X), bit-identical to the reference's DecisionTreeRegressor on these inputs (sum_tree, no sklearn)."""
        try:
            from AccessMath.preprocessing.content import sum_tree
        except ImportError:             # this file loaded on its own, by path
            import importlib.util
            import os
            spec = importlib.util.spec_from_file_location("lm_dropin_sum_tree", os.path.join(os.path.dirname(os.path.abspath(__file__)), "sum_tree.py"))
            sum_tree = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(sum_tree)
        return sum_tree.fit(all_sums, leaf_min)

    @staticmethod
    def get_tree_decision_boundaries(regressor_tree, max_x):
        """(first frame, predicted value) of every stretch of frames 0 .. max_x - 1 with one predicted value (:43-55)"""
        predicted = regressor_tree.predict(np.arange(0, max_x, dtype=np.int32).reshape(max_x, 1))
        changes = np.flatnonzero(predicted[1:] != predicted[:-1]) + 1
        interval_idxs = [0] + [int(i) for i in changes]
        return interval_idxs, [predicted[i] for i in interval_idxs]

    @staticmethod
    def identify_descend_intervals(interval_vals, min_pixels_erased):
        """Maximal runs (first, last) of stretches each lower than the one before, kept when the value falls by at least
        min_pixels_erased from the stretch before the run to the run's last (:58-86)."""
        n = len(interval_vals)
        falls = [k for k in range(1, n) if interval_vals[k] < interval_vals[k - 1]]
        runs = []
        for k in falls:
            if runs and runs[-1][1] == k - 1:
                runs[-1][1] = k
            else:
                runs.append([k, k])
        kept = []
        for first, last in runs:
            diff = interval_vals[first - 1] - interval_vals[last]
            ratio = interval_vals[last] / interval_vals[first - 1]         # unused (the ratio test is commented out at :81), but the
            if diff >= min_pixels_erased:                                   # reference divides: a zero before the run warns or raises
                kept.append((first, last))
        return kept

    @staticmethod
    def video_segments_from_erasing_intervals(erasing_intervals, n_images):
        """The stretches between the erasures (:89-99).  An erasure that starts at frame 0 leaves a first segment ending at -1; what
        follows the last erasure counts when it holds more than one frame."""
        segments, current_start = [], 0
        for start_erase, end_erase in erasing_intervals:
            segments.append((current_start, start_erase - 1))
            current_start = end_erase + 1
        if current_start < n_images - 1:
            segments.append((current_start, n_images - 1))
        return segments

    @staticmethod
    def video_segments_from_sums(all_sums, min_points, min_erase):
        """Method 1 (:102-130): fit the tree, take its falling runs that erase at least min_erase of the mean sum, and cut the video
        from each run's first frame to the first frame of the stretch after it (the last frame when there is none)."""
        min_pixels_erased = np.array(all_sums).mean() * min_erase
        regressor = VideoSegmenter.create_regresor_from_sums(all_sums, min_points)
        interval_idxs, interval_vals = VideoSegmenter.get_tree_decision_boundaries(regressor, len(all_sums))
        erasing = []
        for first, last in VideoSegmenter.identify_descend_intervals(interval_vals, min_pixels_erased):
            last_x = interval_idxs[last + 1] if last + 1 < len(interval_idxs) else len(all_sums) - 1
            erasing.append((interval_idxs[first], last_x))
        return VideoSegmenter.video_segments_from_erasing_intervals(erasing, len(all_sums))

    @staticmethod
    def _split_conflicts(pairs, start_frame, end_frame, min_conflicts, min_segment_split, min_segment_len, current_depth, graph_data,
                         split_data):
        """The recursion of split_video_from_group_conflicts on flattened pairs, worked through with an explicit stack (right part
        pushed first: nodes are visited, and graph_data / split_data filled, in the reference's depth-first order and the leaves come
        out left to right)."""
        intervals = []
        todo = [(start_frame, end_frame, current_depth)]
        while todo:
            lo, hi, depth = todo.pop()
            if hi - lo + 1 < min_segment_split:
                print(str([(lo, hi)]) + " cannot split, too small")
                intervals.append((lo, hi))
                continue
            values = pairs.signal(lo, hi)
            graph_data.append((depth, _SegmentSignal(lo, values)))
            tops = np.array([top for _, top, _ in VideoSegmenter._peaks_of_values(lo, hi, values)], dtype=np.int64)
            if len(tops):
                heights = values[tops - lo]
                keep = (heights > min_conflicts) & (tops >= lo + min_segment_len) & (tops <= hi - min_segment_len)
                tops, heights = tops[keep], heights[keep]
            if len(tops) == 0:
                print(str([(lo, hi)]) + " no good split candidates found")
                intervals.append((lo, hi))
                continue
            best = int(tops[np.lexsort((tops, heights))[-1]])       # highest, then latest
            split_data.append((depth, best))
            todo.append((best + 1, hi, depth + 1))
            todo.append((lo, best - 1, depth + 1))
        return intervals

    @staticmethod
    def split_video_from_group_conflicts(start_frame, end_frame, group_ages, group_conflicts, min_conflicts,
                                         min_segment_split, min_segment_len,
                                         method_weight_area, method_weight_pixels, method_weight_time,
                                         current_depth, graph_data, split_data, n_frames):
        """Recursive split of [start_frame, end_frame] at the highest peak of the conflict signal that exceeds min_conflicts and
        leaves min_segment_len frames on both sides (video_segmenter.py:186-398); segments below min_segment_split stay whole.
        graph_data receives (depth, conflicts_per_frame) per examined node -- a read-only mapping frame -> float -- and split_data
        (depth, split frame) per split, both in the reference's order."""
        pairs = _ConflictPairs(group_ages, group_conflicts, method_weight_area, method_weight_pixels, method_weight_time, n_frames)
        return VideoSegmenter._split_conflicts(pairs, start_frame, end_frame, min_conflicts, min_segment_split, min_segment_len,
                                               current_depth, graph_data, split_data)

    @staticmethod
    def merge_conflict_plot_data(graph_data, n_frames):
        """list of (depth, conflicts_per_frame) -> one float32 array [n_frames] per depth (video_segmenter.py:401-422)"""
        max_depth = max([depth for depth, _ in graph_data], default=0)
        final_arrays = [np.zeros(n_frames, dtype=np.float32) for _ in range(max_depth + 1)]
        for depth, data in graph_data:
            for frame_idx in data:
                final_arrays[depth][frame_idx] = data[frame_idx]
        return final_arrays

    @staticmethod
    def from_group_conflicts(n_frames, group_ages, group_conflicts, min_conflicts, min_split, min_len,
                             weight_area, weight_pixels, weight_time, save_prefix=None, area_divisor=None):
        """(video_segmenter.py:457-473)  save_prefix is accepted and ignored: no plots, as for method 3.  area_divisor (not in the
        reference): the step script's normalisation of the areas by the image size (pre_ST3D_v3.0_04_vid_segmentation.py:140-148),
        applied while the pairs are flattened -- the same division on the same doubles -- instead of in place in group_conflicts."""
        return VideoSegmenter.from_group_conflicts_with_presegments(n_frames, [(0, n_frames - 1)], group_ages, group_conflicts,
                                                                    min_conflicts, min_split, min_len, weight_area, weight_pixels,
                                                                    weight_time, save_prefix, area_divisor)

    @staticmethod
    def from_group_conflicts_with_presegments(n_frames, pre_segments, group_ages, group_conflicts, min_conflicts,
                                              min_split, min_len, weight_area, weight_pixels, weight_time,
                                              save_prefix=None, area_divisor=None):
        """(video_segmenter.py:476-496)  The pairs are flattened and uploaded once for all pre-segments."""
        pairs = _ConflictPairs(group_ages, group_conflicts, weight_area, weight_pixels, weight_time, n_frames, area_divisor)
        graph_data, split_data, all_segments = [], [], []
        for seg_start, seg_end in pre_segments:
            all_segments += VideoSegmenter._split_conflicts(pairs, seg_start, seg_end, min_conflicts, min_split, min_len, 0, graph_data,
                                                            split_data)
        return all_segments
