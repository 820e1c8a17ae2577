"""GPU: step 05 on the device (lm_kf_*, device.GroupImages, KeyframeExtractor.GenerateFromGroupImages,
LecturePipeline.finish(keyframes="device")) on the MI355X; the checks are
tests/keyframe_checks.py, the same ones tests/test_keyframes_emulated.py runs on the emulated build."""
import pytest

import keyframe_checks as kc
import lm_checks

pytestmark = pytest.mark.gpu


def test_fixtures_are_not_vacuous():
    kc.check_not_vacuous()


@pytest.mark.parametrize("name", lm_checks.STREAMS)
def test_g8_through_host_images(hip_lib, name):
    kc.check_g8_host(hip_lib, name)


@pytest.mark.parametrize("name", lm_checks.STREAMS)
def test_g8_through_the_device_view(hip_lib, name):
    kc.check_g8_view(hip_lib, name, compare_images=(name == "short_gap_jitter"))


@pytest.mark.parametrize("case", [0, 1])
def test_g8b_ties(hip_lib, case):
    kc.check_ties(hip_lib, case)


def test_g8b_ties_700_groups_take_the_crowded_tile_path(hip_lib):
    """Both: the reference draws up to 32 of the 700 groups on one 256 x 32 tile and the hit list of a tile holds 24 items
    (LM_KT_MAXHIT, chosen with this fixture in mind), and the kernel counts the (tile, keyframe) units that listed more
    (lm_kf_crowded_tiles): the test asserts that the count is not zero."""
    kc.check_ties(hip_lib, 2, want_crowded=True)


def test_overlaps_against_numpy_and_image_pairs_overlap(hip_lib):
    kc.check_overlaps(hip_lib)


def test_overlaps_candidate_region_retry(hip_lib):
    kc.check_overlaps(hip_lib, kc.dense_structure(), list_counts=(1, 3))


@pytest.mark.parametrize("w,h", [(333, 97), (640, 96), (16, 1)])
def test_render_against_numpy(hip_lib, w, h):
    kc.check_render(hip_lib, w, h)


def test_lm_keyframes_switch(hip_lib, monkeypatch):
    kc.check_env_switch(hip_lib, monkeypatch)


def test_argument_checks(hip_lib):
    kc.check_argument_errors(hip_lib)
