"""GPU: translation alignment on the device (lm_align_*, device.TranslationAligner, the overlay's Aligner) on the MI355X; the checks
are tests/alignment_checks.py, the same ones tests/test_alignment_emulated.py runs on the emulated build, and two that need the
device: a full 1080p pair, and keyframes aligned where lm_kf_render left them."""
import numpy as np
import pytest

import alignment_checks as ac
import keyframe_checks as kc
import lm_checks

pytestmark = pytest.mark.gpu


def test_fixture_is_not_vacuous():
    ac.check_not_vacuous()


def test_g21_through_the_overlay(hip_lib):
    ac.check_g21_overlay(hip_lib)


def test_g21_counts_against_numpy(hip_lib):
    ac.check_counts_g21(hip_lib)


def test_batch_of_pairs_against_numpy(hip_lib):
    ac.check_batch(hip_lib)


def test_pixel_stride_reads_one_channel_in_place(hip_lib):
    ac.check_pixel_stride(hip_lib)


def test_device_input_equals_host_input(hip_lib):
    ac.check_device_input(hip_lib)


def test_all_ink_closed_form(hip_lib):
    ac.check_all_ink(hip_lib, 9, 70, 9)


def test_all_ink_1080p(hip_lib):
    """2,073,600 matches at the centre, 34 row blocks x 21 dy = 714 workgroups of 60-word rows: counter width and grid size"""
    ac.check_all_ink(hip_lib, 1080, 1920, 10)


def test_empty_image_inside_a_batch(hip_lib):
    ac.check_empty_in_batch(hip_lib)


def test_handle_reuse_leaves_no_stale_bits(hip_lib):
    ac.check_reuse(hip_lib)


def test_argument_checks(hip_lib):
    ac.check_argument_errors(hip_lib)


@pytest.mark.parametrize("name", lm_checks.STREAMS)
def test_keyframes_alignments_parity(hip_lib, name):
    ac.check_keyframes_parity(hip_lib, name)


def test_rendered_keyframes_are_aligned_in_place(hip_lib, name="occluder_return"):
    """GroupImages.render leaves the keyframes of a G8 segmentation on the device as [n][H][W][3]; channel 0 of that tensor is
    aligned where it lies, consecutive keyframes, and gives what the host copy of the same keyframes gives -- and what the
    reference recorded for them (G21: the stream's list starts with this segmentation)"""
    from lecturemath_amd import device
    ac.dropin_checks.use_library(hip_lib)
    KE = kc.extractor()
    spec, ages, bounds, images = kc.g4_structure(name)
    g = kc.g8(name)
    times = [1000.0 * i for i in range(int(g["n_frames"]))]
    gi, item_first = kc.from_host(hip_lib, ages, images, bounds, spec["w"], spec["h"])
    try:
        dev, _ = KE.GenerateFromGroupImages(gi, item_first, ages, bounds, times, spec["h"], spec["w"], g["segments"][0], verbose=False, device_frames=True)
    finally:
        gi.close()
    n = int(dev.shape[0])
    assert n >= 3 and tuple(dev.shape) == (n, spec["h"], spec["w"], 3) and dev.is_cuda
    pairs = [(i, i + 1) for i in range(n - 1)]
    al = device.TranslationAligner(spec["w"], spec["h"], max_images=n, max_window=10, lib=hip_lib)
    try:
        in_place = al.set_images(dev, content_lum=0).align(pairs, 10)
        counts = al.match_counts(pairs, 10)
        host = dev.cpu().numpy()
        assert al.set_images(host, content_lum=0).align(pairs, 10) == in_place and (al.match_counts(pairs, 10) == counts).all()
        assert al.set_images(np.ascontiguousarray(host[..., 0]), content_lum=0).align(pairs, 10) == in_place
    finally:
        al.close()
    _, want = ac.g21_keyframes(name)
    for got, rec in zip(in_place, want[:n - 1]):
        assert got[0] < 0.3 if type(rec[0]) is int else ac.same_tuple(got, rec), (got, rec)
