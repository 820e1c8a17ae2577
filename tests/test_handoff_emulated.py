"""CPU: the stream hand-off ABI on one handle pair in one process (tests/handoff_checks.py), through the emulated build of the
product's HIP sources.  The blocks of more than 1024 frames run on the GPU only (tests/test_handoff_gpu.py): the emulator needs
minutes for each of them."""
import handoff_checks as hc

H, W = 24, 64


def test_block_layout_byte_for_byte(emu_lib):
    hc.check_block_layout(emu_lib, H, W)


def test_assign_layout_byte_for_byte(emu_lib):
    hc.check_assign_layout(emu_lib, H, W)


def test_round_trips_at_cut_lists(emu_lib, oracle_built):
    hc.check_round_trips(emu_lib, H, W)


def test_matched_handoff(emu_lib):
    hc.check_matched_handoff(emu_lib, H, W)


def test_twin_hash_paths_agree(emu_lib):
    hc.check_twin_hash_paths(emu_lib, H, W)


def test_host_state_continuation(emu_lib):
    hc.check_host_state_continuation(emu_lib, H, W)


def test_rejections_leave_the_stream_usable(emu_lib):
    hc.check_rejections(emu_lib, H, W)
