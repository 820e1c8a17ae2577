"""Evaluator: the release's evaluation of a lecture summary against its ground truth (AccessMath/evaluation/evaluator.py), with the
same class, method and argument names and the same return values.

What the release does per pair of connected components in Python -- translate one box, cut both masks to the intersection, AND,
count -- is here one integer primitive on the device (lecturemath_amd.device.CCPairCounts, lm_kf_pair_counts): for a CC of one
list, a CC of another and a displacement, the ink pixels they share, for every extra displacement of a small window at once.  The
CCs of all keyframes involved are packed to bit rows once and every stage asks for all its pairs in one call:
    check_equivalent_cc                 one query of two CCs, radius = window
    keyframes_unique_cc                 one call, a query per pair of consecutive keyframes, radius = local_window
    keyframes_overlapping_ccs           one query, radius 0; a pair overlaps iff its count > 0
    match_overlapping_ccs               counts cached on the CCMatchInfo objects (pair_ink); what is missing comes from one call
    find_ccs_overlapping_background     the ground truth's object mask is one more item; count > 0
    summary_overlapping_ccs             one Aligner.computeTranslationAlignments call for all time-overlapping keyframe pairs
                                        (instead of the release's process pool), then one call for all accepted pairs
The divisions, the order-dependent greedy assignment, the grouping and the report arithmetic stay host Python on those integers,
with the release's expressions, so every returned number is the release's bit for bit.

Precondition of the partial-match branch of match_overlapping_ccs: the CCs of ONE keyframe are pixel-disjoint (every labelling
guarantees it).  The release merges a group's CCs of each frame into one image and counts the shared ink of the two images; for
disjoint CCs that is the sum of the group's pair counts over the summed sizes, which is what is computed here.

Limits: windows up to 8 (lecturemath_amd.device.CC_PAIR_MAX_RADIUS; the release's default is 3); a larger window raises ValueError.
CC boxes lie inside their keyframe (min_x, min_y >= 0), as every labelling produces them."""
import os

import numpy as np

from AccessMath.preprocessing.content.aligner import Aligner

from .cc_match_info import CCMatchInfo
from .eval_parameters import EvalParameters

try:
    from AccessMath.annotation.unique_cc_group import UniqueCCGroup
except ImportError:
    class UniqueCCGroup:
        """Stand-in for AccessMath.annotation.unique_cc_group.UniqueCCGroup where the release's annotation package is not
        importable: a CC that lives through consecutive keyframes, starting at keyframe `start_frame`."""

        def __init__(self, start_cc, start_frame):
            self.cc_refs = [start_cc]
            self.start_frame = start_frame

        def lastFrame(self):
            return self.start_frame + len(self.cc_refs) - 1

        def strID(self):
            return str(self.start_frame) + "-" + self.cc_refs[0].strID()

        def __eq__(self, other):
            return isinstance(other, UniqueCCGroup) and self.cc_refs == other.cc_refs

        __hash__ = None


def _pair_table(cc_lists, extra=(), width=0, height=0):
    """device table of the CCs of `cc_lists` (and `extra` (box, image) items) in a frame that holds them all.  CCs that already are
    items of one live device.KeyframeCCs (lecturemath_amd.keyframes), unmoved, with extras that are masks of that table, are served
    by a view of it: nothing is packed or uploaded.  Anything else -- host CCs, a CC moved by translateBox, two tables -- is uploaded."""
    from lecturemath_amd import device
    view = device.KeyframeCCs.pair_view(cc_lists, extra)
    if view is not None:
        return view
    for lst in cc_lists:
        for cc in lst:
            width, height = max(width, cc.max_x + 1), max(height, cc.max_y + 1)
    for box, _ in extra:
        width, height = max(width, box[1] + 1), max(height, box[3] + 1)
    return device.CCPairCounts(cc_lists, max(int(width), 1), max(int(height), 1), extra=extra)


def _check_window(window):
    from lecturemath_amd import device
    if window != int(window) or window < 0:
        raise ValueError("Evaluator: window = %r is not a window (an integer >= 0)" % (window,))
    if window > device.CC_PAIR_MAX_RADIUS:
        raise ValueError("Evaluator: window = %d exceeds the device limit of %d" % (window, device.CC_PAIR_MAX_RADIUS))
    return int(window)


def _rows_by_query(rows, counts, n_queries):
    """per query a dict (position in A, position in B) -> counts [2r + 1][2r + 1]"""
    out = [{} for _ in range(n_queries)]
    for (q, i, j), c in zip(rows.tolist(), counts):
        out[q][(i, j)] = c
    return out


def _equivalent(moving, fixed, global_align, window, counts, min_recall, min_precision):
    """check_equivalent_cc from the window's integer counts (None: the boxes never touch): `moving` is displaced by the global
    alignment plus every local (y outer, x inner) displacement; a displacement enters the list when the boxes overlap by the
    release's STRICT test; the first one with the best f-score decides."""
    best = None
    for loc_y in range(-window, window + 1):
        dy = global_align[3] + loc_y
        for loc_x in range(-window, window + 1):
            dx = global_align[4] + loc_x
            if not (moving.min_x + dx < fixed.max_x and fixed.min_x < moving.max_x + dx and
                    moving.min_y + dy < fixed.max_y and fixed.min_y < moving.max_y + dy):
                continue
            match = 0 if counts is None else int(counts[loc_y + window][loc_x + window])
            recall, precision = match / float(moving.size), match / float(fixed.size)
            fscore = (2.0 * recall * precision) / (recall + precision) if recall + precision > 0.0 else 0.0
            if best is None or fscore > best[0]:
                best = (fscore, recall, precision)
    if best is None:
        return False
    return best[1] >= min_recall and best[2] >= min_precision


def _is_exact(match):
    return len(match.frame1_ccs_refs) == 1 and len(match.frame2_ccs_refs) == 1


class Evaluator:
    @staticmethod
    def check_equivalent_cc(cc1, cc2, global_align, window, min_recall, min_precision):
        window = _check_window(window)
        table = _pair_table([[cc2], [cc1]])
        try:
            rows, counts = table.counts([(table.items(0), table.items(1), (global_align[3], global_align[4]))], window)
        finally:
            table.close()
        return _equivalent(cc1, cc2, global_align, window, counts[0] if len(rows) else None, min_recall, min_precision)

    @staticmethod
    def _print_percentiles(sizes):
        print("\t-> Percentiles:")
        values = []
        for percent in (25, 50, 75, 100):
            values.append(np.percentile(sizes, percent))
            print("\t\t" + str(percent) + "%\t<\t" + str(values[-1]))
        return values

    @staticmethod
    def keyframes_unique_cc(keyframe_set, alignments, local_window, min_recall, min_precision, verbose=False):
        local_window = _check_window(local_window)
        for keyframe in keyframe_set:
            if keyframe.binary_cc is None:
                keyframe.update_binary_cc()
        h, w, _ = keyframe_set[0].raw_image.shape
        cc_groups = [{cc.strID(): None for cc in keyframe.binary_cc} for keyframe in keyframe_set]
        if verbose:
            print("\tRaw CC count: " + str(sum(len(keyframe.binary_cc) for keyframe in keyframe_set)))
            Evaluator._print_percentiles(np.array([cc.size for keyframe in keyframe_set for cc in keyframe.binary_cc]))

        # the count tables of all consecutive keyframes: query k - 1 = CCs of keyframe k - 1 against the displaced CCs of keyframe k
        n = len(keyframe_set)
        tables = [{} for _ in range(max(n - 1, 0))]
        if n > 1:
            table = _pair_table([keyframe.binary_cc for keyframe in keyframe_set], width=w, height=h)
            try:
                queries = [(table.items(k - 1), table.items(k), (alignments[k - 1][3], alignments[k - 1][4])) for k in range(1, n)]
                rows, counts = table.counts(queries, local_window)
            finally:
                table.close()
            tables = _rows_by_query(rows, counts, n - 1)

        unique_ccs, active = [], []             # active: (group, position of its last CC in the previous keyframe)
        for pos, cc in enumerate(keyframe_set[0].binary_cc):
            group = UniqueCCGroup(cc, 0)
            unique_ccs.append(group)
            cc_groups[0][cc.strID()] = group
            active.append((group, pos))
        for kf_idx in range(1, n):
            pending, active = active, []
            align, found_counts = alignments[kf_idx - 1], tables[kf_idx - 1]
            for pos, kf_cc in enumerate(keyframe_set[kf_idx].binary_cc):
                hit = None
                for slot, (group, prev_pos) in enumerate(pending):      # the first pending group that is equivalent takes the CC
                    if _equivalent(kf_cc, group.cc_refs[-1], align, local_window, found_counts.get((prev_pos, pos)), min_recall,
                                   min_precision):
                        hit = slot
                        break
                if hit is None:
                    group = UniqueCCGroup(kf_cc, kf_idx)
                    unique_ccs.append(group)
                else:
                    group = pending.pop(hit)[0]
                    group.cc_refs.append(kf_cc)
                cc_groups[kf_idx][kf_cc.strID()] = group
                active.append((group, pos))

        if verbose:
            print("\tUnique CC count: " + str(len(unique_ccs)))
            Evaluator._print_percentiles(np.array([group.cc_refs[0].size for group in unique_ccs]))
        return unique_ccs, cc_groups

    @staticmethod
    def keyframes_alignments(keyframes, window, min_fscore):
        planes = [keyframe.binary_image[:, :, 0] for keyframe in keyframes]
        pairs = [(idx, idx + 1) for idx in range(len(keyframes) - 1)]
        alignments = Aligner.computeTranslationAlignments(planes, pairs, window, 0) if pairs else []
        # an alignment below the threshold is dropped: the content changed too much between the two keyframes
        return [(0, 0, 0, 0, 0) if info[0] < min_fscore else info for info in alignments]

    @staticmethod
    def _overlap_groups(frame1_ccs, frame2_ccs, disp, pair_counts, verbose):
        """the groups of keyframes_overlapping_ccs from the radius-0 counts {(i, j): [[count]]} of one query"""
        overlapping = []                        # frame-2 CC outer, frame-1 CC inner: the release's visiting order
        by_j = {}
        for (i, j), c in pair_counts.items():
            if int(c[0][0]) > 0:
                by_j.setdefault(j, []).append(i)
        for j in sorted(by_j):
            for i in sorted(by_j[j]):
                overlapping.append((i, j))
        group1 = {cc.strID(): CCMatchInfo(cc, None) for cc in frame1_ccs}
        group2 = {cc.strID(): CCMatchInfo(None, cc) for cc in frame2_ccs}
        for i, j in overlapping:
            id1, id2 = frame1_ccs[i].strID(), frame2_ccs[j].strID()
            if group1[id1] != group2[id2]:
                merged = CCMatchInfo.Merge(group1[id1], group2[id2])
                for cc in merged.frame1_ccs_refs:
                    group1[cc.strID()] = merged
                for cc in merged.frame2_ccs_refs:
                    group2[cc.strID()] = merged
        overlap_set = list(set(group1.values()) | set(group2.values()))
        # the shared ink of every group, for match_overlapping_ccs
        pos1 = {id(cc): i for i, cc in enumerate(frame1_ccs)}
        pos2 = {id(cc): j for j, cc in enumerate(frame2_ccs)}
        for info in overlap_set:
            total = 0
            for cc1 in info.frame1_ccs_refs:
                for cc2 in info.frame2_ccs_refs:
                    c = pair_counts.get((pos1[id(cc1)], pos2[id(cc2)]))
                    if c is not None:
                        total += int(c[0][0])
            info.pair_ink = (disp[0], disp[1], total)
        if verbose:
            print("\t-> Count of raw pair-wise overlaps: " + str(len(overlapping)))
            print("\t-> total overlapping groups: " + str(len(overlap_set)))
        return overlap_set

    @staticmethod
    def keyframes_overlapping_ccs(frame1_ccs, frame2_ccs, alignment, verbose=False):
        _, _, _, disp_y, disp_x = alignment
        table = _pair_table([frame1_ccs, frame2_ccs])
        try:
            rows, counts = table.counts([(table.items(0), table.items(1), (disp_y, disp_x))], 0)
        finally:
            table.close()
        return Evaluator._overlap_groups(frame1_ccs, frame2_ccs, (disp_y, disp_x), _rows_by_query(rows, counts, 1)[0], verbose)

    @staticmethod
    def _fill_pair_ink(overlap_set, disp):
        """pair_ink of the two-sided groups that do not carry it for this displacement: one call, a query per group"""
        missing = [info for info in overlap_set
                   if info.frame1_ccs_refs and info.frame2_ccs_refs and
                   (getattr(info, "pair_ink", None) is None or tuple(info.pair_ink[:2]) != tuple(disp))]
        if not missing:
            return
        lists = [info.frame1_ccs_refs for info in missing] + [info.frame2_ccs_refs for info in missing]
        table = _pair_table(lists)
        try:
            m = len(missing)
            rows, counts = table.counts([(table.items(k), table.items(m + k), disp) for k in range(m)], 0)
        finally:
            table.close()
        totals = [0] * len(missing)
        for (q, _, _), c in zip(rows.tolist(), counts):
            totals[q] += int(c[0][0])
        for info, total in zip(missing, totals):
            info.pair_ink = (disp[0], disp[1], total)

    @staticmethod
    def match_overlapping_ccs(overlap_set, alignment, min_recall, min_precision, verbose=False):
        _, _, _, disp_y, disp_x = alignment
        Evaluator._fill_pair_ink(overlap_set, (disp_y, disp_x))
        exact_matches, partial_matches, unmatched_frame1, unmatched_frame2 = [], [], [], []
        for info in overlap_set:
            if len(info.frame1_ccs_refs) == 0:
                unmatched_frame2 += info.frame2_ccs_refs
                continue
            if len(info.frame2_ccs_refs) == 0:
                unmatched_frame1 += info.frame1_ccs_refs
                continue
            match = info.pair_ink[2]
            if _is_exact(info):
                accepted = exact_matches
                size1, size2 = info.frame1_ccs_refs[0].size, info.frame2_ccs_refs[0].size
            else:
                # the merged CCs of either frame (see the module's note on pixel-disjoint CCs)
                accepted = partial_matches
                size1 = sum(cc.size for cc in info.frame1_ccs_refs)
                size2 = sum(cc.size for cc in info.frame2_ccs_refs)
            cc_recall, cc_precision = match / float(size1), match / float(size2)
            if cc_recall >= min_recall and cc_precision >= min_precision:
                accepted.append(info)
            else:
                unmatched_frame1 += info.frame1_ccs_refs
                unmatched_frame2 += info.frame2_ccs_refs
        if verbose:
            print("\t-> Total exact matches: " + str(len(exact_matches)))
            print("\t-> Total partial matches groups: " + str(len(partial_matches)))
            print("\t-> Total CC in 1 unmatched: " + str(len(unmatched_frame1)))
            print("\t-> Total CC in 2 unmatched: " + str(len(unmatched_frame2)))
        return exact_matches, partial_matches, unmatched_frame1, unmatched_frame2

    @staticmethod
    def _inside(cc, disp, width, height):
        return (cc.min_x + disp[1] >= 0 and cc.max_x + disp[1] < width and cc.min_y + disp[0] >= 0 and cc.max_y + disp[0] < height)

    @staticmethod
    def _background_ids(gt_keyframe, summ_ccs, disp, mask_counts, inside_pos):
        """ids of the CCs of a summary keyframe that fall on the ground truth's objects: the device count against the mask for a
        CC whose displaced box is wholly inside the frame (mask_counts: position in inside_pos -> count), the keyframe object's
        own check for the others, whose slices wrap negative indices in the release"""
        rank = {pos: k for k, pos in enumerate(inside_pos)}
        ids = []
        for pos, cc in enumerate(summ_ccs):
            cc_id = cc.strID()
            if pos in rank:
                hit = mask_counts.get(rank[pos], 0) > 0
            else:
                cc.translateBox(disp[1], disp[0])
                try:
                    hit = gt_keyframe.check_cc_overlaps_background(cc)
                finally:
                    cc.translateBox(-disp[1], -disp[0])
            if hit:
                ids.append(cc_id)
        return ids

    @staticmethod
    def find_ccs_overlapping_background(gt_keyframe, summ_keyframe, alignment, verbose):
        _, _, _, disp_y, disp_x = alignment
        mask = np.asarray(gt_keyframe.object_mask)
        height, width = mask.shape[:2]
        summ_ccs = summ_keyframe.binary_cc
        inside = [pos for pos, cc in enumerate(summ_ccs) if Evaluator._inside(cc, (disp_y, disp_x), width, height)]
        mask_counts = {}
        if inside:
            table = _pair_table([summ_ccs], extra=[((0, width - 1, 0, height - 1), mask)], width=width, height=height)
            try:
                rows, counts = table.counts([(table.items(-1), table.items(0)[np.asarray(inside, np.int64)], (disp_y, disp_x))], 0)
            finally:
                table.close()
            mask_counts = {j: int(c[0][0]) for (_, _, j), c in zip(rows.tolist(), counts)}
        return Evaluator._background_ids(gt_keyframe, summ_ccs, (disp_y, disp_x), mask_counts, inside)

    @staticmethod
    def parallel_keyframe_align(candidate_data):
        gt_segment_idx, summ_segment_idx, gt_bin, summ_bin, window = candidate_data
        # the alignment with the best recall
        return gt_segment_idx, summ_segment_idx, Aligner.computeTranslationAlignment(gt_bin, summ_bin, window, 0, 1)

    @staticmethod
    def summary_overlapping_ccs(gt_segments, gt_keyframes, summ_segments, summ_keyframes, window, min_align_recall, verbose=False):
        """one keyframe per segment on either side; keyframes whose segments overlap in time are compared"""
        background_overlaps = [{cc.strID(): 0 for cc in keyframe.binary_cc} for keyframe in summ_keyframes]
        if verbose:
            print("Finding alignment candidates")
        candidates = []
        g, s = 0, 0
        while g < len(gt_segments) and s < len(summ_segments):
            if gt_segments[g][0] < summ_segments[s][1] and summ_segments[s][0] < gt_segments[g][1]:
                candidates.append((g, s))
            if summ_segments[s][1] < gt_segments[g][1]:         # the segment that ends first is left behind
                s += 1
            else:
                g += 1
        if verbose:
            print("Starting alignment process")
        # all alignments in one batched call: the ground truth's planes, then the summary's
        used_g, used_s = sorted(set(g for g, _ in candidates)), sorted(set(s for _, s in candidates))
        planes = ([gt_keyframes[g].binary_image[:, :, 0] for g in used_g] + [summ_keyframes[s].binary_image[:, :, 0] for s in used_s])
        slot_g = {g: k for k, g in enumerate(used_g)}
        slot_s = {s: len(used_g) + k for k, s in enumerate(used_s)}
        aligns = Aligner.computeTranslationAlignments(planes, [(slot_g[g], slot_s[s]) for g, s in candidates], window, 0, 1) if candidates else []
        accepted = [k for k, info in enumerate(aligns) if not info[1] < min_align_recall]

        # one table: CC lists of the ground truth's keyframes, of the summary's, and the object masks of the ground truth's
        by_pair = {}
        if accepted:
            acc_g = sorted(set(candidates[k][0] for k in accepted))
            acc_s = sorted(set(candidates[k][1] for k in accepted))
            list_g = {g: k for k, g in enumerate(acc_g)}
            list_s = {s: len(acc_g) + k for k, s in enumerate(acc_s)}
            masks, width, height = [], 0, 0
            for g in acc_g:
                mask = np.asarray(gt_keyframes[g].object_mask)
                masks.append(((0, mask.shape[1] - 1, 0, mask.shape[0] - 1), mask))
                width, height = max(width, mask.shape[1]), max(height, mask.shape[0])
            lists = [gt_keyframes[g].binary_cc for g in acc_g] + [summ_keyframes[s].binary_cc for s in acc_s]
            table = _pair_table(lists, extra=masks, width=width, height=height)
            try:
                queries, inside_of = [], {}
                for k in accepted:
                    g, s = candidates[k]
                    disp = (aligns[k][3], aligns[k][4])
                    mh, mw = np.asarray(gt_keyframes[g].object_mask).shape[:2]
                    inside = [pos for pos, cc in enumerate(summ_keyframes[s].binary_cc) if Evaluator._inside(cc, disp, mw, mh)]
                    inside_of[k] = inside
                    queries.append((table.items(list_g[g]), table.items(list_s[s]), disp))
                    queries.append((table.items(-1)[list_g[g]:list_g[g] + 1], table.items(list_s[s])[np.asarray(inside, np.int64)], disp))
                rows, counts = table.counts(queries, 0)
            finally:
                table.close()
            per_query = _rows_by_query(rows, counts, len(queries))
            for n, k in enumerate(accepted):
                by_pair[k] = (per_query[2 * n], {j: int(c[0][0]) for (_, j), c in per_query[2 * n + 1].items()}, inside_of[k])

        all_overlapping_ccs = []
        for k, (g, s) in enumerate(candidates):
            if verbose:
                print("Computing overlaps GT KF #" + str(g) + " - KF #" + str(s))
            if k not in by_pair:
                if verbose:
                    print("\t-> Recall is to low, skipping ...")
                continue
            pair_counts, mask_counts, inside = by_pair[k]
            disp = (aligns[k][3], aligns[k][4])
            groups = Evaluator._overlap_groups(gt_keyframes[g].binary_cc, summ_keyframes[s].binary_cc, disp, pair_counts, verbose)
            for cc_id in Evaluator._background_ids(gt_keyframes[g], summ_keyframes[s].binary_cc, disp, mask_counts, inside):
                background_overlaps[s][cc_id] += 1
            all_overlapping_ccs.append((g, s, aligns[k], groups))
        return all_overlapping_ccs, background_overlaps

    @staticmethod
    def find_gt_unique_cc_matches(gt_keyframes, gt_groups, gt_cc_group, summ_keyframes, all_overlapping_ccs, min_recall, min_precision,
                                  verbose=False):
        # matches per CC of every summary keyframe, per unique CC (group) of the ground truth, and per CC of every GT keyframe
        summ_matches = [{cc.strID(): [] for cc in keyframe.binary_cc} for keyframe in summ_keyframes]
        gt_matches = {group.strID(): [] for group in gt_groups}
        frame_gt_matches = [{cc.strID(): [] for cc in keyframe.binary_cc} for keyframe in gt_keyframes]
        for gt_idx, summ_idx, align_info, overlapping_ccs in all_overlapping_ccs:
            if verbose:
                print("Computing matches GT KF #" + str(gt_idx) + " - KF #" + str(summ_idx))
            exact, partial, _, _ = Evaluator.match_overlapping_ccs(overlapping_ccs, align_info, min_recall, min_precision, verbose)
            for match in exact + partial:
                for cc in match.frame1_ccs_refs:
                    cc_id = cc.strID()
                    gt_matches[gt_cc_group[gt_idx][cc_id].strID()].append(match)
                    frame_gt_matches[gt_idx][cc_id].append(match)
                for cc in match.frame2_ccs_refs:
                    summ_matches[summ_idx][cc.strID()].append(match)
        return gt_matches, frame_gt_matches, summ_matches

    @staticmethod
    def match_list_type_counts(matches_lists):
        exact = partial = unmatched = 0
        for match_list in matches_lists:
            if len(match_list) == 0:
                unmatched += 1
            elif any(_is_exact(match) for match in match_list):
                exact += 1
            else:
                partial += 1
        return exact, partial, unmatched

    @staticmethod
    def match_list_types(matches_per_cc):
        exact, partial, unmatched = [], [], []
        for cc_id in matches_per_cc:
            match_list = matches_per_cc[cc_id]
            if len(match_list) == 0:
                unmatched.append(cc_id)
            elif any(_is_exact(match) for match in match_list):
                exact.append(cc_id)
            else:
                partial.append(cc_id)
        return exact, partial, unmatched

    @staticmethod
    def compute_unique_cc_summary_metrics(group_matches, per_frame_matches):
        exact, partial, missed = Evaluator.match_list_type_counts([group_matches[group_id] for group_id in group_matches])
        total = len(group_matches)
        if total > 0:
            only_exact_recall, only_partial_recall, recall = exact / total, partial / total, (exact + partial) / total
        else:
            only_exact_recall, only_partial_recall, recall = 0.0, 0.0, 0.0
        # per-keyframe averages; a ground-truth keyframe without CCs does not enter them
        frame_exact, frame_partial, frame_recall = [], [], []
        for frame in per_frame_matches:
            kf_exact, kf_partial, kf_missed = Evaluator.match_list_type_counts([frame[cc_id] for cc_id in frame])
            kf_total = kf_exact + kf_partial + kf_missed
            if kf_total > 0:
                frame_exact.append(kf_exact / kf_total)
                frame_partial.append(kf_partial / kf_total)
                frame_recall.append((kf_exact + kf_partial) / kf_total)
        return {
            "count": total,
            "recall": recall,
            "only_exact_recall": only_exact_recall,
            "only_partial_recall": only_partial_recall,
            "avg_only_exact_recall": np.array(frame_exact).mean(),
            "avg_only_partial_recall": np.array(frame_partial).mean(),
            "avg_recall": np.array(frame_recall).mean(),
            "partial_matches": partial,
            "exact_matches": exact,
            "unmatched": missed,
        }

    @staticmethod
    def compute_per_frame_summary_metrics(per_frame_matches, bg_overlaps):
        total_count = 0
        exact_matches, partial_matches, not_matched, bg_not_matched = [], [], [], []
        all_precision, all_only_exact, all_only_partial, all_bg_share, all_no_bg = [], [], [], [], []
        for kf_idx, frame in enumerate(per_frame_matches):
            kf_exact, kf_partial, kf_missed = Evaluator.match_list_type_counts([frame[cc_id] for cc_id in frame])
            # unmatched CCs that lie on a ground-truth object (the speaker, ...)
            kf_bg_missed = sum(1 for cc_id in frame if len(frame[cc_id]) == 0 and bg_overlaps[kf_idx][cc_id] > 0)
            exact_matches.append(kf_exact)
            partial_matches.append(kf_partial)
            not_matched.append(kf_missed)
            bg_not_matched.append(kf_bg_missed)
            kf_total = kf_exact + kf_partial + kf_missed
            total_count += kf_total
            if kf_total > 0:
                all_only_exact.append(kf_exact / kf_total)
                all_only_partial.append(kf_partial / kf_total)
                all_precision.append((kf_exact + kf_partial) / kf_total)
            else:
                all_only_exact.append(1.0)
                all_only_partial.append(0.0)
                all_precision.append(1.0)
            kf_no_bg_total = kf_total - kf_bg_missed
            all_no_bg.append((kf_exact + kf_partial) / kf_no_bg_total if kf_no_bg_total > 0 else 0.0)
            all_bg_share.append(kf_bg_missed / kf_missed if kf_missed > 0 else 0.0)

        total_exact, total_partial = sum(exact_matches), sum(partial_matches)
        total_missed, total_bg_missed = sum(not_matched), sum(bg_not_matched)
        if total_count > 0:
            only_exact_precision, only_partial_precision = total_exact / total_count, total_partial / total_count
            precision = (total_exact + total_partial) / total_count
        else:
            only_exact_precision, only_partial_precision, precision = 0.0, 0.0, 0.0
        if total_count - total_bg_missed > 0:
            no_bg_precision = (total_exact + total_partial) / (total_count - total_bg_missed)
        else:
            no_bg_precision = 0.0
        global_bg_missed = total_bg_missed / total_missed if total_missed > 0 else 0.0
        return {
            "count": total_count,
            "avg_only_exact_precision": np.array(all_only_exact).mean(),
            "avg_only_partial_precision": np.array(all_only_partial).mean(),
            "avg_precision": np.array(all_precision).mean(),
            "avg_prc_bg_not_matched": np.array(all_bg_share).mean(),
            "avg_no_bg_precision": np.array(all_no_bg).mean(),
            "precision": precision,
            "only_exact_precision": only_exact_precision,
            "only_partial_precision": only_partial_precision,
            "global_bg_unmatched": global_bg_missed,
            "no_bg_precision": no_bg_precision,
            # per keyframe
            "exact_matches": exact_matches,
            "partial_matches": partial_matches,
            "unmatched": not_matched,
            "bg_unmatched": bg_not_matched,
            "all_precision": all_precision,
            "all_only_exact_precision": all_only_exact,
            "all_only_partial_precision": all_only_partial,
            "all_no_bg_precision": all_no_bg,
        }

    @staticmethod
    def filter_matches_per_size(gt_keyframes, gt_groups, gt_matches, frame_gt_matches, summ_keyframes, summ_matches, bound_min, bound_max):
        group_of = {group.strID(): group for group in gt_groups}
        filtered_gt = {group_id: gt_matches[group_id] for group_id in gt_matches
                       if bound_min <= group_of[group_id].cc_refs[0].size < bound_max}

        def per_frame(keyframes, matches):
            out = []
            for kf_idx, keyframe in enumerate(keyframes):
                out.append({})
                for cc in keyframe.binary_cc:
                    if bound_min <= cc.size < bound_max:
                        out[kf_idx][cc.strID()] = matches[kf_idx][cc.strID()]
            return out

        return filtered_gt, per_frame(gt_keyframes, frame_gt_matches), per_frame(summ_keyframes, summ_matches)

    @staticmethod
    def visualize_gt_matches(gt_keyframes, frame_gt_matches, img_prefix):
        import cv2
        from AccessMath.util.visualizer import Visualizer
        for kf_idx, frame in enumerate(frame_gt_matches):
            by_id = gt_keyframes[kf_idx].get_CCs_by_ID()
            exact, partial, unmatched = ([by_id[cc_id] for cc_id in ids] for ids in Evaluator.match_list_types(frame))
            h, w, _ = gt_keyframes[kf_idx].binary_image.shape
            cv2.imwrite("{0:s}_{1:d}.png".format(img_prefix, kf_idx), Visualizer.show_gt_matches(h, w, exact, partial, unmatched))

    @staticmethod
    def compute_summary_metrics(gt_segments, gt_keyframes, gt_groups, gt_cc_group, summ_segments, summ_keyframes, verbose=False,
                                gt_visual_prefix=None):
        all_sizes = np.array([group.cc_refs[0].size for group in gt_groups])
        # size classes of the per-size reports: [0, p10), [p10, p25), ..., [p75, max + 1)
        size_boundaries = [0]
        if EvalParameters.Report_Summary_Show_stats_per_size:
            for percentile in EvalParameters.UniqueCC_size_percentiles:
                size_boundaries.append(int(round(np.percentile(all_sizes, percentile))))
            size_boundaries.append(all_sizes.max() + 1)

        overlapping_ccs, bg_overlaps = Evaluator.summary_overlapping_ccs(
            gt_segments, gt_keyframes, summ_segments, summ_keyframes, EvalParameters.UniqueCC_global_tran_window,
            EvalParameters.UniqueCC_min_align_recall, verbose)

        metrics, sorted_range_names = {}, []
        for min_r, min_p in zip(EvalParameters.UniqueCC_min_recall, EvalParameters.UniqueCC_min_precision):
            gt_matches, frame_gt_matches, summ_matches = Evaluator.find_gt_unique_cc_matches(
                gt_keyframes, gt_groups, gt_cc_group, summ_keyframes, overlapping_ccs, min_r, min_p, False)
            if gt_visual_prefix is not None:
                vis_dir = "{0:s}/{1:.2f}_{2:.2f}".format(gt_visual_prefix, min_r, min_p)
                os.makedirs(vis_dir, exist_ok=True)
                Evaluator.visualize_gt_matches(gt_keyframes, frame_gt_matches, "{0:s}/match_".format(vis_dir))
            for range_idx in range(len(size_boundaries)):
                if range_idx == len(size_boundaries) - 1:
                    name, in_range = "all", (gt_matches, frame_gt_matches, summ_matches)
                else:
                    low, high = size_boundaries[range_idx], size_boundaries[range_idx + 1]
                    name = "[{0}, {1})".format(low, high)
                    in_range = Evaluator.filter_matches_per_size(gt_keyframes, gt_groups, gt_matches, frame_gt_matches, summ_keyframes,
                                                                 summ_matches, low, high)
                if name not in metrics:
                    sorted_range_names.append(name)
                    metrics[name] = []
                metrics[name].append({
                    "min_cc_recall": min_r,
                    "min_cc_precision": min_p,
                    "recall_metrics": Evaluator.compute_unique_cc_summary_metrics(in_range[0], in_range[1]),
                    "precision_metrics": Evaluator.compute_per_frame_summary_metrics(in_range[2], bg_overlaps),
                })
        return metrics, sorted_range_names

    # ---- reports: the release's tab-separated tables, line for line ----------------------------------------------------------------------
    @staticmethod
    def _thresholds(entry):
        return entry["min_cc_recall"] * 100.0, entry["min_cc_precision"] * 100.0

    @staticmethod
    def _summary_totals(metrics):
        exact, partial = sum(metrics["exact_matches"]), sum(metrics["partial_matches"])
        missed, bg_missed = sum(metrics["unmatched"]), sum(metrics["bg_unmatched"])
        return exact + partial, exact, partial, missed, bg_missed, exact + partial + missed

    @staticmethod
    def print_summary_recall_metrics(scope_metrics, scope):
        percent_row = "{0:.2f}\t{1:.2f}\t|\t{2:.2f}\t|\t{3:.2f}\t{4:.2f}"
        percent_head = "Min. R.\tMin. P.\t|\tE + P\t|\tE. Only\tP. Only"
        if EvalParameters.Report_Summary_Show_Counts:
            print("Matching Params\t|\tGround Truth Matches (Count - " + scope + ")")
            print("Min. R.\tMin. P.\t|\tE + P\t|\tE. Only\tP. Only\tMiss\tTotal")
            for entry in scope_metrics:
                m = entry["recall_metrics"]
                print("{0:.2f}\t{1:.2f}\t|\t{2}\t|\t{3}\t{4}\t{5}\t{6}".format(
                    *Evaluator._thresholds(entry), m["exact_matches"] + m["partial_matches"], m["exact_matches"], m["partial_matches"],
                    m["unmatched"], m["count"]))
        if EvalParameters.Report_Summary_Show_AVG_per_frame:
            print("")
            print("Matching Params\t|\tGround Truth Matches (Per Frame Recall - " + scope + ")")
            print(percent_head)
            for entry in scope_metrics:
                m = entry["recall_metrics"]
                print(percent_row.format(*Evaluator._thresholds(entry), m["avg_recall"] * 100.0, m["avg_only_exact_recall"] * 100.0,
                                         m["avg_only_partial_recall"] * 100.0))
        if EvalParameters.Report_Summary_Show_Globals:
            print("")
            print("Matching Params\t|\tGround Truth Matches (Unique CC Recall - " + scope + ")")
            print(percent_head)
            for entry in scope_metrics:
                m = entry["recall_metrics"]
                print(percent_row.format(*Evaluator._thresholds(entry), m["recall"] * 100.0, m["only_exact_recall"] * 100.0,
                                         m["only_partial_recall"] * 100.0))

    @staticmethod
    def print_summary_precision_metrics(scope_metrics, scope):
        percent_row = "{0:.2f}\t{1:.2f}\t|\t{2:.2f}\t|\t{3:.2f}\t{4:.2f}\t{5:.2f}\t{6:.2f}"
        percent_head = "Min. R.\tMin. P.\t|\tE + P\t|\tE. Only\tP. Only\tBG. %\tNo BG P."
        if EvalParameters.Report_Summary_Show_Counts:
            print("")
            print("Matching Params\t|\tSummary Matches (Count - " + scope + ")")
            print("Min. R.\tMin. P.\t|\tE + P\t|\tE. Only\tP. Only\tMiss\tBG. Miss\tTotal")
            for entry in scope_metrics:
                print("{0:.2f}\t{1:.2f}\t|\t{2}\t|\t{3}\t{4}\t{5}\t{6}\t{7}".format(
                    *Evaluator._thresholds(entry), *Evaluator._summary_totals(entry["precision_metrics"])))
        if EvalParameters.Report_Summary_Show_AVG_per_frame:
            print("")
            print("Matching Params\t|\tSummary Matches (AVG Precision per Frame -" + scope + ")")
            print(percent_head)
            for entry in scope_metrics:
                m = entry["precision_metrics"]
                print(percent_row.format(*Evaluator._thresholds(entry), m["avg_precision"] * 100.0, m["avg_only_exact_precision"] * 100.0,
                                         m["avg_only_partial_precision"] * 100.0, m["avg_prc_bg_not_matched"] * 100.0,
                                         m["avg_no_bg_precision"] * 100.0))
        if EvalParameters.Report_Summary_Show_Globals:
            print("")
            print("Matching Params\t|\tSummary Matches (Global Precision -" + scope + ")")
            print(percent_head)
            for entry in scope_metrics:
                m = entry["precision_metrics"]
                print(percent_row.format(*Evaluator._thresholds(entry), m["precision"] * 100.0, m["only_exact_precision"] * 100.0,
                                         m["only_partial_precision"] * 100.0, m["global_bg_unmatched"] * 100.0,
                                         m["no_bg_precision"] * 100.0))

    @staticmethod
    def print_compact_CC_metrics(scope_metrics, scope):
        """one header line and one line per threshold pair: recall columns, then precision columns"""
        headers = "Min_R\tMin_P"
        lines = ["{0:.2f}\t{1:.2f}".format(*Evaluator._thresholds(entry)) for entry in scope_metrics]

        def add(title, row, values):
            nonlocal headers
            headers += title
            for k, entry in enumerate(scope_metrics):
                lines[k] += row.format(*values(entry))

        recall_row = "\t{0:.2f}\t{1:.2f}\t{2:.2f}"
        if EvalParameters.Report_Summary_Show_Counts:
            add("\tR_CT_EP\tR_CT_E\tR_CT_P\tR_CT_M\tR_CT_T", "\t{0:d}\t{1:d}\t{2:d}\t{3:d}\t{4:d}",
                lambda e: (e["recall_metrics"]["exact_matches"] + e["recall_metrics"]["partial_matches"], e["recall_metrics"]["exact_matches"],
                           e["recall_metrics"]["partial_matches"], e["recall_metrics"]["unmatched"], e["recall_metrics"]["count"]))
        if EvalParameters.Report_Summary_Show_AVG_per_frame:
            add("\tR_AVG_EP\tR_AVG_E\tR_AVG_P", recall_row,
                lambda e: (e["recall_metrics"]["avg_recall"] * 100.0, e["recall_metrics"]["avg_only_exact_recall"] * 100.0,
                           e["recall_metrics"]["avg_only_partial_recall"] * 100.0))
        if EvalParameters.Report_Summary_Show_Globals:
            add("\tR_GBL_EP\tR_GBL_E\tR_GBL_P", recall_row,
                lambda e: (e["recall_metrics"]["recall"] * 100.0, e["recall_metrics"]["only_exact_recall"] * 100.0,
                           e["recall_metrics"]["only_partial_recall"] * 100.0))

        precision_row = "\t{0:.2f}\t{1:.2f}\t{2:.2f}\t{3:.2f}\t{4:.2f}"
        if EvalParameters.Report_Summary_Show_Counts:
            add("\tP_CT_EP\tP_CT_E\tP_CT_P\tP_CT_M\tP_CT_BG_M\tP_CT_T", "\t{0:d}\t{1:d}\t{2:d}\t{3:d}\t{4:d}\t{5:d}",
                lambda e: Evaluator._summary_totals(e["precision_metrics"]))
        if EvalParameters.Report_Summary_Show_AVG_per_frame:
            add("\tP_AVG_EP\tP_AVG_E\tP_AVG_P\tP_AVG_BGP\tP_AVG_NBG", precision_row,
                lambda e: (e["precision_metrics"]["avg_precision"] * 100.0, e["precision_metrics"]["avg_only_exact_precision"] * 100.0,
                           e["precision_metrics"]["avg_only_partial_precision"] * 100.0,
                           e["precision_metrics"]["avg_prc_bg_not_matched"] * 100.0, e["precision_metrics"]["avg_no_bg_precision"] * 100.0))
        if EvalParameters.Report_Summary_Show_Globals:
            # the release prints the heading of the long report here as well
            print("")
            print("Matching Params\t|\tSummary Matches (Global Precision -" + scope + ")")
            print("Min. R.\tMin. P.\t|\tE + P\t|\tE. Only\tP. Only\tBG. %\tNo BG P.")
            add("\tP_GBL_EP\tP_GBL_E\tP_GBL_P\tP_GBL_BGP\tP_GBL_NBG", precision_row,
                lambda e: (e["precision_metrics"]["precision"] * 100.0, e["precision_metrics"]["only_exact_precision"] * 100.0,
                           e["precision_metrics"]["only_partial_precision"] * 100.0, e["precision_metrics"]["global_bg_unmatched"] * 100.0,
                           e["precision_metrics"]["no_bg_precision"] * 100.0))
        print(headers)
        for line in lines:
            print(line)

    @staticmethod
    def compute_pixel_binary_metrics(gt_frames, summary_frames):
        """pixel recall / precision / f-measure of the summary's binary keyframes against the ground truth's, keyframe by keyframe,
        averaged; `board` leaves out the summary ink that lies on a ground-truth object.  Keyframes that live on the device
        (lecturemath_amd.keyframes.DeviceKeyframe on both sides) get their four integer sums from one pass on the device
        (lm_kf_pixel_sums); the divisions are the same float64 ones on the same uint64 values."""
        from lecturemath_amd import keyframes as device_keyframes
        device_sums = device_keyframes.pixel_sum_pairs(gt_frames, summary_frames)
        all_recall, all_precision, all_fmeasure, all_board_precision, all_board_fmeasure = [], [], [], [], []
        for idx, gt_frame in enumerate(gt_frames):
            if device_sums is not None:
                total_gt, total_summ, total_correct, total_board = (v / 255 for v in device_sums[idx])
            else:
                gt_ink = 255 - gt_frame.binary_image[:, :, 0]
                summ_ink = 255 - summary_frames[idx].binary_image[:, :, 0]
                total_gt = gt_ink.sum() / 255
                total_summ = summ_ink.sum() / 255
                total_correct = summ_ink[gt_ink > 0].sum() / 255
                on_board = summ_ink.copy()
                on_board[gt_frame.object_mask] = 0.0
                total_board = on_board.sum() / 255

            recall = total_correct / total_gt
            precision = total_correct / total_summ
            board_precision = total_correct / total_board if total_board > 0.0 else 1.0
            fmeasure = (2.0 * recall * precision) / (recall + precision) if recall + precision > 0 else 0.0
            board_fmeasure = (2.0 * recall * board_precision) / (recall + board_precision) if recall + board_precision > 0.0 else 0.0

            all_recall.append(recall)
            all_precision.append(precision)
            all_fmeasure.append(fmeasure)
            all_board_precision.append(board_precision)
            all_board_fmeasure.append(board_fmeasure)
        return {
            "recall": np.array(all_recall).mean(),
            "precision": np.array(all_precision).mean(),
            "fmeasure": np.array(all_fmeasure).mean(),
            "board_precision": np.array(all_board_precision).mean(),
            "board_fmeasure": np.array(all_board_fmeasure).mean(),
        }
