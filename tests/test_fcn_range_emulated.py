"""CPU (emulated build of the HIP sources): f16 range report, device range statistics and the rescale -> f16x3 -> fp32 ladder of the
planar FCN engine.  Bodies shared with the GPU tests: tests/fcn_range_checks.py."""
import numpy as np
import pytest

import fcn_range_checks as rc
from lecturemath_amd import _lib, fcn
from oracle import fcn as ofcn

WIDE = (16, 16, 32, 32, 48, 48, 32, 32, 16, 32, 16, 16, 16, 16, 16, 16, 32, 16)


def test_load_time_weight_check(emu_lib):
    """one BN-folded weight at 1e6: the default guard raises and names the layer; "off" loads; the report lists the layer"""
    sd = {k: v.numpy().copy() for k, v in ofcn.random_state_dict(WIDE, pixel_kernel=7, seed=5).items()}
    w = sd["conv_down_block_3.0.weight"]
    s = sd["conv_down_block_3.1.weight"][4] / np.sqrt(sd["conv_down_block_3.1.running_var"][4] + np.float32(1e-5))
    w[4, 2, 1, 1] = np.float32(1e6) / s
    eng = fcn.FcnEngine(WIDE, 7, 3, 66, 130, emu_lib)
    with pytest.raises(_lib.LecturemathError, match=r"layer 2 \(conv_down_block_3\).*1e\+06"):
        eng.load_state_dict(sd)
    row = eng.range_report[2]
    assert row["name"] == "conv_down_block_3" and row["nonfinite_f16"] == 1 and abs(row["max_abs"] - 1e6) < 1
    eng.close()
    eng = fcn.FcnEngine(WIDE, 7, 3, 66, 130, emu_lib, range_guard="off")
    eng.load_state_dict(sd)
    assert eng.planar and eng.range_report == {}
    eng.close()
    with pytest.raises(_lib.LecturemathError):
        fcn.FcnEngine(WIDE, 7, 3, 66, 130, emu_lib, range_guard="sometimes")


def test_scaled_without_guard_is_wrong(emu_lib):
    rc.check_hole_without_guard(emu_lib)


def test_scaled_rescale(emu_lib):
    rc.check_scaled_rescale(emu_lib)


def test_spread_needs_promotion(emu_lib):
    rc.check_spread(emu_lib)


def test_in_range_network_is_untouched(emu_lib):
    rc.check_identity(emu_lib)


def test_statistics_ignore_an_older_larger_frame(emu_lib):
    """two frame sizes in turn, larger first: the second report counts the smaller frame's interior only and sees none of the first's remains"""
    g, sd, rgb = rc.load("g5_fcn_k7_66x130_wide")
    eng = rc.engine(emu_lib, g)
    eng.load_state_dict(sd)
    big = eng.calibrate([rgb], policy="check")
    small_rgb = np.ascontiguousarray(rgb[:40, :72])
    small = eng.calibrate([small_rgb], policy="check")
    eng.close()
    fresh = fcn.FcnEngine(g["widths"], int(g["pk"]), 3, 40, 72, emu_lib)
    fresh.load_state_dict(sd)
    alone = fresh.calibrate([small_rgb], policy="check")
    fresh.close()
    for a, b, c in zip(small["tensors"], alone["tensors"], big["tensors"]):
        assert a["count"] == b["count"] < c["count"], (a, b, c)
        assert (a["max_abs"], a["subnormal"], a["zero"]) == (b["max_abs"], b["subnormal"], b["zero"]), (a, b)
    assert small["tensors"][1]["count"] == 16 * 40 * 72


def test_all_zero_tensor_settles(emu_lib):
    rc.check_all_zero_tensor_settles(emu_lib)


def test_format_without_instance_rejected_at_load(emu_lib):
    rc.check_no_instance_rejected_at_load(emu_lib)
