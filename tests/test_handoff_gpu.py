"""GPU: the stream hand-off ABI on one handle pair in one process (tests/handoff_checks.py) through the real gfx950 library,
including the blocks of more than 1024 frames (lm_k_append_offsets beyond its first chunk of 1024 frames)."""
import pytest

import handoff_checks as hc

pytestmark = pytest.mark.gpu
H, W = 96, 160


def test_block_layout_byte_for_byte(hip_lib):
    hc.check_block_layout(hip_lib, H, W)


def test_assign_layout_byte_for_byte(hip_lib):
    hc.check_assign_layout(hip_lib, H, W)


def test_round_trips_at_cut_lists(hip_lib, oracle_built):
    hc.check_round_trips(hip_lib, H, W)


@pytest.mark.parametrize("n_frames,max_batch", [(2049, 64), (1025, 32), (1024, 64), (1023, 32)])
def test_long_blocks(hip_lib, n_frames, max_batch):
    hc.check_long_block(hip_lib, H, W, n_frames, max_batch, handoff=n_frames == 2049)


def test_matched_handoff(hip_lib):
    hc.check_matched_handoff(hip_lib, H, W)


def test_twin_hash_paths_agree(hip_lib):
    hc.check_twin_hash_paths(hip_lib, H, W)


def test_host_state_continuation(hip_lib):
    hc.check_host_state_continuation(hip_lib, H, W)


def test_rejections_leave_the_stream_usable(hip_lib):
    hc.check_rejections(hip_lib, H, W)
