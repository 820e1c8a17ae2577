"""Step 04 entry point (same name, argv, config keys, inputs and output as the reference's
pre_ST3D_v3.0_04_vid_segmentation.py) for VIDEO_SEGMENTATION_METHOD = 3 (deletion events, :44-99; the shipped configuration):
[(frame_times, frame_indices, compressed_frames), (group_ages, conflicts), SpaceTimeStruct] -> list of (first, last) frame
intervals; and for method 2 (conflict minimisation, :114-159): [(frame_times, frame_indices, compressed_frames), (group_ages,
conflicts)] -> the same; and for method 1 (sums + regression tree, :160-171): (frame_times, frame_indices, compressed_frames) itself -> the
same.  The reference's debug plots (matplotlib, :100-112, :175-218) are not produced, nor, for methods 2 and 3, the decompression + sums
that only feed them (:28-41); pass the parameter `sums=1` to get the binary sums printed.  With LM_PNG_CODEC=device the sums (method 1,
`sums=1`) are taken on the device: the PNG list is decoded 64 files at a time into device memory and summed there (lm_frame_sums)."""
import math
import sys
import time

import numpy as np


def deletion_signal(group_ages, st3D, add_threshold):
    """The signal method 3 segments (:44-99): every group adds its box area (as a fraction of the frame) at the frame it
    appears and at the frame it disappears; the deletions are accumulated over time, restarting from zero at every frame whose
    additions exceed add_threshold.  float64 throughout; np.add.at and np.cumsum add in index order, i.e. in the order the
    reference's loops do, so the sums round identically."""
    n = len(st3D.frame_indices)
    groups = list(group_ages)                      # dict order = group index order
    first = np.fromiter((group_ages[g][0] for g in groups), dtype=np.int64, count=len(groups))
    last = np.fromiter((group_ages[g][-1] for g in groups), dtype=np.int64, count=len(groups))
    boxes = np.array([st3D.cc_group_boundaries[g] for g in groups], dtype=np.int64).reshape(-1, 4)       # min_x, max_x, min_y, max_y
    area = ((boxes[:, 1] - boxes[:, 0] + 1) * (boxes[:, 3] - boxes[:, 2] + 1)) / (st3D.width * st3D.height)
    added, deleted = np.zeros(n), np.zeros(n)
    np.add.at(added, first, area)
    np.add.at(deleted, last, area)
    signal = np.empty(n)
    restarts = np.flatnonzero(added > add_threshold)
    bounds = np.unique(np.concatenate([[0], restarts, [n]]))
    for a, b in zip(bounds[:-1], bounds[1:]):       # a running sum per stretch between restarts
        signal[a:b] = np.cumsum(deleted[a:b])
    return signal


def conflict_intervals(process, n_frames, compressed_frames, group_ages, conflicts, st3D=None):
    """Method 2 (:114-159): the reference's keys, parameter overrides (conf_w, conf_p, conf_t) and defaults.  For the area weights
    "union" and "intersection" the reference divides every conflict's areas by the image size, in place; here the caller's dict is
    left alone and the same division happens where the pairs are flattened (VideoSegmenter.from_group_conflicts, area_divisor).  The
    image size comes from the first reconstructed frame, the only one decoded; a caller that hands over no reconstructed frames but the
    SpaceTimeStruct as a third input (LecturePipeline.finish keeps the frames on the device) gets it from there: the same integer."""
    from AccessMath.preprocessing.content.video_segmenter import VideoSegmenter

    def weight_mode(param, key):
        return int(process.params[param]) if param in process.params else process.configuration.get_int(key, 0)
    weights = weight_mode("conf_w", "VIDEO_SEGMENTATION_CONFLICTS_WEIGHTS")
    weights_pixels = weight_mode("conf_p", "VIDEO_SEGMENTATION_CONFLICTS_WEIGHTS_PIXELS")
    weights_time = weight_mode("conf_t", "VIDEO_SEGMENTATION_CONFLICTS_WEIGHTS_TIME")
    min_conflicts = process.configuration.get("VIDEO_SEGMENTATION_CONFLICTS_MIN_CONFLICTS", 3.0)
    min_split = process.configuration.get_int("VIDEO_SEGMENTATION_CONFLICTS_MIN_SPLIT", 50)
    min_length = process.configuration.get_int("VIDEO_SEGMENTATION_CONFLICTS_MIN_LENGTH", 25)
    print((min_conflicts, min_split, min_length))
    img_size = None
    if weights in [VideoSegmenter.ConflictsAreaWeightsIntersection, VideoSegmenter.ConflictsAreaWeigthsUnion]:
        if len(compressed_frames):
            from AccessMath.preprocessing.content.helper import Helper
            h, w = Helper.decompress_binary_images(compressed_frames[:1])[0].shape
        elif st3D is not None:
            h, w = st3D.height, st3D.width
        else:
            raise ValueError("VIDEO_SEGMENTATION_CONFLICTS_WEIGHTS = %d normalises the areas by the image size, which is read from the "
                             "first reconstructed frame: none was given" % weights)
        img_size = h * w
    return VideoSegmenter.from_group_conflicts(n_frames, group_ages, conflicts, min_conflicts, min_split, min_length, weights,
                                               weights_pixels, weights_time, None, area_divisor=img_size)


def binary_sums(compressed_frames):
    """VideoSegmenter.compute_binary_sums of the decompressed frames (:28-39).  With LM_PNG_CODEC=device the files are decoded a batch
    at a time into device memory and summed there; no frame comes back to the host."""
    from AccessMath.preprocessing.content.video_segmenter import VideoSegmenter
    from lecturemath_amd import png_device
    if png_device.codec() == "device" and len(compressed_frames):
        w, h = png_device.png_size(compressed_frames[0])
        all_sums = []
        for b0 in range(0, len(compressed_frames), png_device.BATCH):
            all_sums.extend(VideoSegmenter.compute_binary_sums(png_device.decode_gray8_device(compressed_frames[b0:b0 + png_device.BATCH], w, h)))
        return all_sums
    from AccessMath.preprocessing.content.helper import Helper
    return VideoSegmenter.compute_binary_sums(Helper.decompress_binary_images(compressed_frames))


def sums_intervals(process, all_sums):
    """Method 1 on the frames' sums (:160-171): the reference's keys, read as it reads them (a missing key is 0 and the tree refuses a minimum leaf of 0,
    as sklearn does there), the minimum leaf of the regression tree in frames, and what it prints."""
    from AccessMath.preprocessing.content.video_segmenter import VideoSegmenter
    sampling_fps = process.configuration.get_float("SAMPLING_FPS")
    sum_min_segment = process.configuration.get_int("VIDEO_SEGMENTATION_SUM_MIN_SEGMENT")
    sum_min_erase_ratio = process.configuration.get_float("VIDEO_SEGMENTATION_SUM_MIN_ERASE_RATIO")
    leaf_min = int(math.ceil(sum_min_segment * sampling_fps))
    intervals = VideoSegmenter.video_segments_from_sums(all_sums, leaf_min, sum_min_erase_ratio)
    print("Erasing Events: ")
    print(intervals)
    print("Total intervals: " + str(len(intervals)))
    return intervals


def process_input(process, input_data):
    from AccessMath.data.space_time_struct import SpaceTimeStruct
    from AccessMath.preprocessing.content.video_segmenter import VideoSegmenter
    segmentation_method = process.configuration.get_int("VIDEO_SEGMENTATION_METHOD", 3)
    if segmentation_method not in (1, 2, 3):
        raise NotImplementedError("VIDEO_SEGMENTATION_METHOD = %d is not built: 3 (deletion events, the shipped configuration), "
                                  "2 (conflict minimisation) and 1 (sums) are" % segmentation_method)
    if segmentation_method == 1:
        frame_times, frame_indices, compressed_frames = input_data
        print("Decompressing input...")
        print("Computing sums...")
        return sums_intervals(process, binary_sums(compressed_frames))
    frame_times, frame_indices, compressed_frames = input_data[0]
    if "sums" in process.params:
        print("Computing sums...")
        print(binary_sums(compressed_frames))
    group_ages, conflicts = input_data[1]
    if segmentation_method == 2:
        intervals = conflict_intervals(process, len(frame_indices), compressed_frames, group_ages, conflicts,
                                       input_data[2] if len(input_data) > 2 else None)
        print("Total intervals: " + str(len(intervals)))
        return intervals
    st3D = input_data[2]
    assert isinstance(st3D, SpaceTimeStruct)
    add_threshold = process.configuration.get_float("VIDEO_SEGMENTATION_DEL_EVENT_ADD_THRESHOLD", 10)
    min_segment_length = process.configuration.get_int("VIDEO_SEGMENTATION_DEL_EVENT_MIN_LENGTH", 15)
    threshold = process.configuration.get_float("VIDEO_SEGMENTATION_DEL_EVENT_THRESHOLD", 0.25)
    cumulative_delete = deletion_signal(group_ages, st3D, add_threshold)
    n = len(cumulative_delete)
    intervals = VideoSegmenter.split_video_from_group_deletes(cumulative_delete, 0, n - 1, min_segment_length, threshold)
    print(intervals)
    print([(st3D.frame_indices[start_f], st3D.frame_indices[end_f]) for start_f, end_f in intervals])
    print("Total intervals: " + str(len(intervals)))
    return intervals


def _inputs_for_method(configuration):
    method = configuration.get_int("VIDEO_SEGMENTATION_METHOD", 2)
    keys = {3: ["CC_RECONSTRUCTED_OUTPUT", "CC_CONFLICTS_OUTPUT", "CC_ST3D_OUTPUT"], 2: ["CC_RECONSTRUCTED_OUTPUT", "CC_CONFLICTS_OUTPUT"]}
    chosen = keys.get(method)
    return [configuration.get(k) for k in chosen] if chosen else configuration.get("CC_RECONSTRUCTED_OUTPUT")


def main():
    import lm_entry
    lm_entry.run_on_inputs(sys.argv, None, "VIDEO_SEGMENTATION_OUTPUT", process_input, choose_inputs=_inputs_for_method)


if __name__ == "__main__":
    main()
