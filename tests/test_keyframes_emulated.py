"""CPU: step 05 on the device (lm_kf_*, device.GroupImages, KeyframeExtractor.GenerateFromGroupImages,
LecturePipeline.finish(keyframes="device")) with the kernels running in the emulated build of the HIP sources; the checks are
tests/keyframe_checks.py, the same ones tests/test_keyframes_gpu.py runs on the GPU."""
import pytest

import keyframe_checks as kc
import lm_checks


def test_fixtures_are_not_vacuous():
    kc.check_not_vacuous()


@pytest.mark.parametrize("name", lm_checks.STREAMS)
def test_g8_through_host_images(emu_lib, name):
    kc.check_g8_host(emu_lib, name)


def test_g8_through_the_device_view(emu_lib):
    """one stream here (a pipeline run takes half a minute on the emulator, as in test_dropin_emulated.py); the GPU file runs all three"""
    kc.check_g8_view(emu_lib, "short_gap_jitter", compare_images=True)


@pytest.mark.parametrize("case", [0, 1])
def test_g8b_ties(emu_lib, case):
    kc.check_ties(emu_lib, case)


def test_g8b_ties_700_groups_take_the_crowded_tile_path(emu_lib):
    """Both: the reference draws up to 32 of the 700 groups on one 256 x 32 tile and the hit list of a tile holds 24 items
    (LM_KT_MAXHIT, chosen with this fixture in mind), and the kernel counts the (tile, keyframe) units that listed more
    (lm_kf_crowded_tiles): the test asserts that the count is not zero."""
    kc.check_ties(emu_lib, 2, want_crowded=True)


def test_overlaps_against_numpy_and_image_pairs_overlap(emu_lib):
    kc.check_overlaps(emu_lib)


def test_overlaps_candidate_region_retry(emu_lib):
    kc.check_overlaps(emu_lib, kc.dense_structure(), list_counts=(1, 3))


@pytest.mark.parametrize("w,h", [(333, 97), (640, 96), (16, 1)])
def test_render_against_numpy(emu_lib, w, h):
    kc.check_render(emu_lib, w, h)


def test_lm_keyframes_switch(emu_lib, monkeypatch):
    kc.check_env_switch(emu_lib, monkeypatch)


def test_argument_checks(emu_lib):
    kc.check_argument_errors(emu_lib)
