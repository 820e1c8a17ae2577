"""KeyframeExtractor.GenerateFromST3DForIntervals (AccessMath/preprocessing/content/keyframe_extractor.py:13-145): one
keyframe per video segment from the space-time structure.  Same name, arguments and return values (list of H x W x 3 uint8
keyframes, ink = 0; per keyframe the sorted list of (start_time, min_x, max_x, min_y, max_y) of the groups drawn).

What the reference computes per segment, restated:
  1. the groups alive in the segment and, for each, the last of its images that overlaps the segment (:27-47);
  2. the connected components of the "shares an ink pixel" graph over those groups
     (CCStabilityEstimator.compute_overlapping_CC_groups, cc_stability_estimator.py:696-748) -- every pair is tested with
     ConnectedComponent.getOverlapFMeasure there, and AGAIN inside every component (:85-91);
  3. isolated groups are drawn; inside a component the groups are visited from the most recently started to the oldest and a
     group is drawn unless it shares pixels with one drawn before it (:103-118).
Here the pixel question of 2. and 3. is answered ONCE per segment on the device (lecturemath_amd.device.image_pairs_overlap:
box join + bit tests), and the rest works on index arrays.

Order contract.  Only the SET of groups drawn reaches the outputs (the mask is a sum, the times are sorted), and that set
depends on the visiting order of step 3: descending (first frame of the group, position of the group inside its component).
The reference takes the position from `list(set)` of a component that was assembled by `set.union` calls -- CPython's set
iteration order for small ints, which is NOT ascending once values exceed the table size ({5, 300} iterates as 300, 5) and
depends on the sequence of unions.  Groups of one component that start at the same frame and overlap are therefore resolved by
that order; `_component_member_order` reproduces it by performing the same unions on real Python sets, in the sequence the
reference's scan produces (ascending object, ascending partner), and nothing else of it.

Device route (GenerateFromGroupImages).  When the group images already are bit rows on the device
(lecturemath_amd.device.GroupImages) the step is four passes: (1) host: per segment the alive groups and the image chosen for
each; (2) device: ONE overlaps call for all segments; (3) host: the component order and the greedy walk above, unchanged --
it is sequential, order-dependent and a few hundred objects; (4) device: ONE render call for all keyframes.
GenerateFromST3DForIntervals takes that route when the structure carries a live GroupImages (`_device_images`, set by
LecturePipeline.finish(keyframes="device"), never pickled) or when LM_KEYFRAMES=device is set (read at every call, default
"host"): then the images any segment selects are uploaded once (GroupImages.from_host).

KeyframeExtractor.extract (:146-222), the pixel history of the raw binary frames per video segment, runs on the frames as bit rows
on the device (lecturemath_amd.device.FrameHistory): one pass per segment with bit-sliced counters."""
import os

import numpy as np

from AccessMath.data.space_time_struct import SpaceTimeStruct


class KeyframeExtractor:

    @staticmethod
    def _component_member_order(n_objects, pairs):
        """Connected components of the overlap graph.  pairs: (i < j), sorted.  Returns (components with >= 2 members, each as
        the member list in the reference's order; isolated objects), both in ascending order of their smallest member."""
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        # symmetric adjacency in CSR form, partners ascending (the order in which the reference's double loop appends them)
        both = np.concatenate([pairs, pairs[:, ::-1]])
        both = both[np.lexsort((both[:, 1], both[:, 0]))]
        start = np.searchsorted(both[:, 0], np.arange(n_objects + 1))
        owner = list(range(n_objects))                      # representative (= smallest member) of every object's component
        members = {k: {k} for k in range(n_objects)}        # representative -> CPython set of members (the order carrier)
        for obj in range(n_objects):
            mine = owner[obj]
            for other in both[start[obj]:start[obj + 1], 1].tolist():
                theirs = owner[other]
                if theirs == mine:
                    continue
                absorbed = members.pop(theirs)
                members[mine] = members[mine].union(absorbed)
                for k in absorbed:
                    owner[k] = mine
        components = [list(v) for v in members.values() if len(v) > 1]
        isolated = [next(iter(v)) for v in members.values() if len(v) == 1]
        return components, isolated

    @staticmethod
    def _drawn_objects(n, pairs, first_of, ids, seg_no, verbose):
        """Step 3 of the module docstring for one segment: n alive objects, their overlapping pairs (i < j, sorted), the first frame
        of each.  Returns (objects drawn, isolated objects, components)."""
        clash = np.zeros((n, n), dtype=bool)
        if len(pairs):
            pa = np.asarray(pairs, dtype=np.int64)
            clash[pa[:, 0], pa[:, 1]] = clash[pa[:, 1], pa[:, 0]] = True
        components, isolated = KeyframeExtractor._component_member_order(n, pairs)
        drawn = list(isolated)
        for comp in components:
            # most recently started first; equal starts: later position in the component first
            order = sorted(range(len(comp)), key=lambda pos: (first_of[comp[pos]], pos), reverse=True)
            kept = []
            for pos in order:
                if not clash[comp[pos], kept].any():
                    kept.append(comp[pos])
            drawn.extend(kept)
            if verbose:
                print("  segment %d: %d overlapping groups, keeping %s" % (seg_no + 1, len(comp), ",".join(str(ids[o]) for o in kept)))
        return drawn, isolated, components

    @staticmethod
    def _segment_selection(group_ages, video_segments):
        """Pass 1: (group_ids, first frame per group, per segment (alive positions in group_ids, image index k of each))."""
        group_ids = list(group_ages)
        first = np.array([group_ages[g][0] for g in group_ids], dtype=np.int64)
        last = np.array([group_ages[g][-1] for g in group_ids], dtype=np.int64)
        selection = []
        for seg_first, seg_last in video_segments:
            alive = np.flatnonzero((seg_first <= last) & (first <= seg_last))
            ks = []
            for a in alive:
                ages = group_ages[group_ids[a]]
                if len(ages) < 2:
                    raise IndexError("list index out of range")       # no segment image: what cc_group_images[g][0] raises
                # segment image k covers [ages[k], ages[k + 1]]: the last one whose end lies inside the video segment, else the first
                ks.append(max(0, int(np.searchsorted(ages, seg_last, side="right")) - 2))
            selection.append((alive, ks))
        return group_ids, first, selection

    @staticmethod
    def _from_selection(gi, item_of, group_ids, first, selection, group_boundaries, frame_times, video_segments, verbose, device_frames):
        """Passes 2-4 over a GroupImages; item_of(group, k) names the item of a selected image."""
        item_lists = [[item_of(group_ids[a], k) for a, k in zip(alive, ks)] for alive, ks in selection]
        pairs_per_segment = gi.overlaps(item_lists)
        draw_lists, keyframe_times = [], []
        if verbose:
            print("%d CC groups, %d video segments" % (len(group_ids), len(video_segments)))
        for seg_no, ((alive, ks), items, pairs) in enumerate(zip(selection, item_lists, pairs_per_segment)):
            ids = [group_ids[a] for a in alive]
            drawn, isolated, components = KeyframeExtractor._drawn_objects(len(ids), pairs, first[alive], ids, seg_no, verbose)
            times = []
            for o in drawn:
                x0, x1, y0, y1 = (int(v) for v in group_boundaries[ids[o]])
                times.append((frame_times[first[alive[o]]], x0, x1, y0, y1))
            if verbose:
                seg_first, seg_last = video_segments[seg_no]
                print("  segment %d (%d - %d): %d groups, %d isolated, %d in %d overlapping sets" %
                      (seg_no + 1, seg_first, seg_last, len(ids), len(isolated), sum(len(c) for c in components), len(components)))
            draw_lists.append([items[o] for o in drawn])
            keyframe_times.append(sorted(times))
        frames = gi.render(draw_lists, channels=3)
        if device_frames:
            return frames, keyframe_times
        return list(gi.be.to_host(frames)), keyframe_times

    @staticmethod
    def GenerateFromGroupImages(gi, item_first, group_ages, group_boundaries, frame_times, height, width, video_segments, verbose=True,
                                device_frames=False):
        """The keyframes from a lecturemath_amd.device.GroupImages; item_first[g] + k is segment image k of group g.  Returns what
        GenerateFromST3DForIntervals returns; with device_frames the keyframes are ONE device uint8 tensor [n_segments, H, W, 3]."""
        if (int(height), int(width)) != (gi.height, gi.width):
            raise ValueError("GenerateFromGroupImages: frame %d x %d, images placed in %d x %d" % (width, height, gi.width, gi.height))
        group_ids, first, selection = KeyframeExtractor._segment_selection(group_ages, video_segments)
        return KeyframeExtractor._from_selection(gi, lambda g, k: int(item_first[g]) + k, group_ids, first, selection, group_boundaries,
                                                 frame_times, video_segments, verbose, device_frames)

    @staticmethod
    def _generate_uploading(st3D, video_segments, verbose):
        """LM_KEYFRAMES=device on a structure that holds host images: the images any segment selects, uploaded once."""
        from lecturemath_amd import device
        group_ids, first, selection = KeyframeExtractor._segment_selection(st3D.cc_group_ages, video_segments)
        item = {}
        for alive, ks in selection:
            for a, k in zip(alive, ks):
                item.setdefault((group_ids[a], k), len(item))
        boxes = [tuple(int(v) for v in st3D.cc_group_boundaries[g]) for g, _ in item]
        images = [st3D.cc_group_images[g][k] for g, k in item]
        gi = device.GroupImages.from_host(boxes, images, st3D.width, st3D.height)
        try:
            return KeyframeExtractor._from_selection(gi, lambda g, k: item[(g, k)], group_ids, first, selection, st3D.cc_group_boundaries,
                                                     st3D.frame_times, video_segments, verbose, False)
        finally:
            gi.close()

    @staticmethod
    def GenerateFromST3DForIntervals(st3D, video_segments, verbose=True):
        from lecturemath_amd import device
        assert isinstance(st3D, SpaceTimeStruct)
        gi = getattr(st3D, "_device_images", None)
        if gi is not None and getattr(gi, "handle", None):
            frames, times = KeyframeExtractor.GenerateFromGroupImages(gi, gi.item_first, st3D.cc_group_ages, st3D.cc_group_boundaries, st3D.frame_times,
                                                                      st3D.height, st3D.width, video_segments, verbose, device_frames=True)
            st3D._device_keyframes = frames
            return list(gi.be.to_host(frames)), times
        if os.environ.get("LM_KEYFRAMES", "host") == "device":
            return KeyframeExtractor._generate_uploading(st3D, video_segments, verbose)
        group_ids = list(st3D.cc_group_ages)
        first = np.array([st3D.cc_group_ages[g][0] for g in group_ids], dtype=np.int64)
        last = np.array([st3D.cc_group_ages[g][-1] for g in group_ids], dtype=np.int64)
        keyframes, keyframe_times = [], []
        if verbose:
            print("%d CC groups, %d video segments" % (len(group_ids), len(video_segments)))
        for seg_no, (seg_first, seg_last) in enumerate(video_segments):
            alive = np.flatnonzero((seg_first <= last) & (first <= seg_last))
            ids = [group_ids[k] for k in alive]
            boxes, images = [], []
            for g in ids:
                ages = st3D.cc_group_ages[g]
                # segment image k covers [ages[k], ages[k + 1]]: the last one whose end lies inside the video segment, else the first
                k = max(0, int(np.searchsorted(ages, seg_last, side="right")) - 2)
                boxes.append(tuple(int(v) for v in st3D.cc_group_boundaries[g]))
                images.append(st3D.cc_group_images[g][k])
            pairs = device.image_pairs_overlap(boxes, images)
            drawn, isolated, components = KeyframeExtractor._drawn_objects(len(ids), pairs, first[alive], ids, seg_no, verbose)
            n = len(ids)
            mask = np.zeros((st3D.height, st3D.width), dtype=bool)
            times = []
            for o in drawn:
                x0, x1, y0, y1 = boxes[o]
                mask[y0:y1 + 1, x0:x1 + 1] |= images[o] > 0
                times.append((st3D.frame_times[first[alive[o]]], x0, x1, y0, y1))
            frame = np.full((st3D.height, st3D.width, 3), 255, dtype=np.uint8)      # white board, ink = 0 (:131-141)
            frame[mask] = 0
            if verbose:
                print("  segment %d (%d - %d): %d groups, %d isolated, %d in %d overlapping sets" %
                      (seg_no + 1, seg_first, seg_last, n, len(isolated), sum(len(c) for c in components), len(components)))
            keyframes.append(frame)
            keyframe_times.append(sorted(times))
        return keyframes, keyframe_times

    @staticmethod
    def extract(binary_images, video_segments, treshold_length, verbose=False, save_prefix=None):
        """(:146-222) Per video segment (start, end) a dict: "sum" = per pixel the frames of the segment with ink, "age" = the index
        of the first of them (0 where none), both float32; "filtered" = 255 where sum >= treshold_length; "local_max" = the
        segment's frame with most ink (the first of equals: the reference replaces only on a strictly larger count).
        binary_images: a list of uint8 0 / 255 frames, a device uint8 tensor [n, H, W], or a lecturemath_amd.device.FrameHistory
        (used as it is).  local_max is the list's own array when a list was given, a host copy otherwise.  A segment holds at most
        FrameHistory.MAX_RANGE frames; an empty or out-of-range segment raises ValueError.  save_prefix writes
        <prefix>_filt_seg_<i + 1>.png."""
        from lecturemath_amd import device, png
        hist, owned = device.as_frame_history(binary_images)
        out_segments = []
        try:
            for segment_idx, (start_int, end_int) in enumerate(video_segments):
                if verbose:
                    print("Processing segment #" + str(segment_idx))
                start_int, end_int = int(start_int), int(end_int)
                local_sum, local_age = hist.segment_stats(start_int, end_int, host=True)
                best = start_int + int(np.argmax(hist.ink_counts(start_int, end_int - start_int + 1)))
                if isinstance(binary_images, device.FrameHistory):
                    local_max = hist.frame(best)
                elif isinstance(binary_images, (list, tuple, np.ndarray)):
                    local_max = binary_images[best]
                else:
                    local_max = hist.be.to_host(binary_images[best])
                filtered_image = (local_sum >= treshold_length).astype(np.uint8) * 255
                out_segments.append({"start": start_int, "end": end_int, "sum": local_sum, "age": local_age, "filtered": filtered_image,
                                     "local_max": local_max})
                if save_prefix is not None:
                    with open(save_prefix + "_filt_seg_" + str(segment_idx + 1) + ".png", "wb") as f:
                        f.write(png.encode_gray8(filtered_image).tobytes())
        finally:
            if owned:
                hist.close()
        return out_segments
