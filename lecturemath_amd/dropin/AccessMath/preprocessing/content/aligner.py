"""Aligner.computeTranslationAlignment (AccessMath/preprocessing/content/aligner.py:27-83): the translation inside a window that
best aligns the ink of two binary images.  Same name, arguments, assertions and return value -- the tuple (f_score, recall,
precision, disp_y, disp_x), bit for bit -- as the reference, whose callers are Evaluator.keyframes_alignments (consecutive keyframes
of a summary) and Evaluator.parallel_keyframe_align (ground truth against summary keyframes), AccessMath/evaluation/evaluator.py.

What the reference computes, restated: for every displacement (dy, dx) of the window, dy then dx ascending, the number of pixels
that are ink (== content_lum) in the first image at (y, x) and in the second at (y - dy, x - dx); recall and precision are that
number over the ink of the first and of the second image, the f-score their harmonic mean; the result is the first displacement
that attains the maximum of field `sort_by` (a stable sort, reversed).  Here the (2w + 1)^2 counts come from the device
(lecturemath_amd.device.TranslationAligner: bit rows, AND, popcount) and the divisions stay host Python on those integers.

computeTranslationAlignments is the batched form, an addition: one set of images (host or device), a list of index pairs, one
launch.  It is the call for in-process use: the evaluator's process pool only hides the cost of the per-pair loop.

Limits: max_window <= MAX_WINDOW (128) and <= min(height, width) -- beyond the latter the reference itself fails with a
broadcasting ValueError; both raise ValueError here."""
import numpy as np


class Aligner:
    # number of frames to test alignment (computeVisualAlignment)
    ALIGNMENT_SAMPLE = 25
    SURF_THRESHOLD = 0.4

    MAX_WINDOW = 128

    _aligners = {}          # (library, height, width) -> lecturemath_amd.device.TranslationAligner, kept between calls

    @staticmethod
    def _check_window(max_window, h, w):
        if max_window != int(max_window) or max_window < 0:
            raise ValueError("Aligner: max_window = %r is not a window (an integer >= 0)" % (max_window,))
        if max_window > Aligner.MAX_WINDOW:
            raise ValueError("Aligner: max_window = %d exceeds the limit of %d" % (max_window, Aligner.MAX_WINDOW))
        if max_window > min(h, w):
            raise ValueError("Aligner: max_window = %d exceeds min(height, width) = %d of the %d x %d images" % (max_window, min(h, w), h, w))
        return int(max_window)

    @staticmethod
    def _aligner(h, w, n_images):
        from lecturemath_amd import _lib, device
        lib = _lib.load()
        key = (id(lib), h, w)
        al = Aligner._aligners.get(key)
        if al is None or al.handle is None or al.lib is not lib or al.max_images < n_images:
            if al is not None:
                al.close()
            if len(Aligner._aligners) >= 4:
                for old in Aligner._aligners.values():
                    old.close()
                Aligner._aligners.clear()
            al = device.TranslationAligner(w, h, max_images=max(n_images, 2), max_window=Aligner.MAX_WINDOW, lib=lib)
            Aligner._aligners[key] = al
        return al

    @staticmethod
    def computeTranslationAlignment(first_content, second_content, max_window, content_lum=255, sort_by=0):
        # assert that both images have the same dimensions
        assert len(first_content.shape) == 2
        assert len(second_content.shape) == 2
        assert first_content.shape == second_content.shape

        h, w = first_content.shape
        max_window = Aligner._check_window(max_window, h, w)
        both = np.stack([np.asarray(first_content), np.asarray(second_content)])
        if both.dtype != np.uint8:
            both, content_lum = (both == content_lum).astype(np.uint8), 1
        al = Aligner._aligner(h, w, 2)
        al.set_images(both, content_lum=content_lum)
        totals = al.totals()
        if totals[0] == 0 or totals[1] == 0:
            # cannot align, at least one of them is empty
            return 0.0, 0.0, 0.0, 0, 0
        return al.align([(0, 1)], max_window, sort_by)[0]

    @staticmethod
    def computeTranslationAlignments(images, pairs, max_window, content_lum=255, sort_by=0):
        """What computeTranslationAlignment(images[i], images[j], ...) returns for every (i, j) of `pairs`, as a list.  images:
        [n][H][W] or [n][H][W][C] (channel 0 is read) uint8 -- a numpy array, a list of equally sized 2-D arrays, or a torch device
        tensor, which is read where it lies."""
        if isinstance(images, (list, tuple)):
            images = np.stack([np.asarray(im) for im in images]) if len(images) else np.zeros((0, 1, 1), np.uint8)
        shape = tuple(int(v) for v in images.shape)
        assert len(shape) in (3, 4)
        pairs = [(int(i), int(j)) for i, j in pairs]
        for i, j in pairs:
            if not (0 <= i < shape[0] and 0 <= j < shape[0]):
                raise IndexError("Aligner: pair (%d, %d) outside the %d images" % (i, j, shape[0]))
        if not pairs:
            return []
        h, w = shape[1:3]
        max_window = Aligner._check_window(max_window, h, w)
        if not hasattr(images, "data_ptr") and images.dtype != np.uint8:
            images, content_lum = (images == content_lum).astype(np.uint8), 1
        al = Aligner._aligner(h, w, shape[0])
        al.set_images(images, content_lum=content_lum)
        return al.align(pairs, max_window, sort_by)

    @staticmethod
    def computeVisualAlignment(m_videos, a_videos, time_offset, motionless, save_frames, extraction_method_id):
        raise NotImplementedError("Aligner.computeVisualAlignment (SURF keypoint matching between two videos) is not part of this "
                                  "overlay; nothing in the release calls it")
