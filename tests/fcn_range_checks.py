"""Shared bodies of the f16 range-calibration tests (tests/test_fcn_range_emulated.py on the CPU emulation, tests/test_fcn_range_gpu.py
on the device): the planar FCN engine on the g15 fixtures of tests/golden/make_golden_fcn_range.py, whose activations and BN-folded
weights leave f16's range while the reference's fp32 outputs stay of order one.  The bar is the project's 1e-3 on all three outputs
(BASELINE.json, lm_checks.check_fcn_golden), against the REFERENCE's outputs stored in the fixtures."""
import os

import numpy as np

from lecturemath_amd import _lib, fcn

# the 25 tensors of the planar engine in the order of fcn2.T_* (FcnEngine.TENSOR_NAMES)
TENSORS = (["x0"] + ["down%d_pre" % n for n in range(1, 6)] + ["down%d_pool" % n for n in range(1, 6)] + ["mid"] + ["upsample%d" % n for n in range(5, 0, -1)] +
           ["up%d" % n for n in range(5, 1, -1)] + ["up1", "diff", "p1", "p2"])

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-3


def load(name):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    sd = {k[3:]: g[k] for k in g.files if k.startswith("sd.")}
    return g, sd, g["rgb"]


def engine(lib, g, **kw):
    h, w = g["rgb"].shape[:2]
    return fcn.FcnEngine(g["widths"], int(g["pk"]), 3, h, w, lib, **kw)


def errors(eng, g, rgb):
    """max |engine - reference| of the three outputs (inf when an output is not finite)"""
    res = {}
    for n, v in zip(("out", "text", "rec"), eng.forward(rgb)):
        v = eng.be.to_host(v).reshape(g[n].shape)
        res[n] = float(np.abs(v - g[n]).max()) if np.isfinite(v).all() else float("inf")
    print("max |engine - reference|:", res)
    return res


def check_hole_without_guard(lib):
    """`scaled`, range_guard="off", no calibration: today's path returns non-finite or wrong outputs without an error"""
    g, sd, rgb = load("g15_fcn_range_scaled")
    eng = engine(lib, g, range_guard="off")
    eng.load_state_dict(sd)
    assert eng.planar
    e = errors(eng, g, rgb)
    assert max(e.values()) > TOL
    eng.close()


def check_scaled_rescale(lib):
    g, sd, rgb = load("g15_fcn_range_scaled")
    eng = engine(lib, g, range_guard="rescale")
    eng.load_state_dict(sd)
    rep = eng.calibrate([rgb], policy="rescale")
    assert eng.planar and rep["planar"] and not rep["promoted"]
    assert np.count_nonzero(eng.tensor_exp) > 0 and np.count_nonzero(eng.layer_wexp) > 0
    for t in rep["tensors"] + rep["outputs"]:
        assert t["nonfinite"] == 0 and np.isfinite(t["max_abs"]), t
    assert [t["name"] for t in rep["tensors"]] == TENSORS
    checked = 0
    for t in rep["tensors"]:
        ref = float(g["max." + t["name"]])          # the fixture records all 25: a missing key is an error, not a skip
        if ref > 2.0 ** -10:
            rel = abs(t["max_abs"] - ref) / ref
            print("%-11s max %.6g reference %.6g rel %.2e exp %+d" % (t["name"], t["max_abs"], ref, rel, t["exp"]))
            assert rel <= 2.0 ** -10, (t, ref)
            checked += 1
    assert checked >= 20, checked
    e = errors(eng, g, rgb)
    assert max(e.values()) <= TOL, e
    eng.close()


def check_spread(lib):
    g, sd, rgb = load("g15_fcn_range_spread")
    eng = engine(lib, g, range_guard="rescale")
    eng.load_state_dict(sd)
    try:
        eng.calibrate([rgb], policy="rescale")
        raise AssertionError("policy \"rescale\" accepted a tensor no per-tensor exponent fits")
    except _lib.LecturemathError as e:
        print("rescale:", e)
    eng.close()
    eng = engine(lib, g, range_guard="promote")
    eng.load_state_dict(sd)
    rep = eng.calibrate([rgb])
    print(rep["steps"])
    assert rep["promoted"] and rep["steps"][-1]["rung"] == 3 and not any(s["rung"] == 2 for s in rep["steps"])
    assert rep["engine"] == eng.precision == "fp32" and not eng.planar
    assert all(l["format_after"] == "fp32" for l in rep["layers"]) and len(rep["layers"]) == 20
    e = errors(eng, g, rgb)
    assert max(e.values()) <= TOL, e
    eng.close()


def check_identity(lib):
    """an in-range network: all exponents stay zero and the outputs are bit for bit those of range_guard="off" """
    g, sd, rgb = load("g5_fcn_k7_66x130_wide")
    ref = engine(lib, g, range_guard="off")
    ref.load_state_dict(sd)
    want = [ref.be.to_host(v).copy() for v in ref.forward(rgb)]
    ref.close()
    eng = engine(lib, g)
    assert eng.range_guard == "check"
    eng.load_state_dict(sd)
    rep = eng.calibrate([rgb], policy="rescale")
    assert eng.planar and not rep["steps"]
    assert not eng.tensor_exp.any() and not eng.layer_wexp.any()
    assert all(t["exp"] == 0 for t in rep["tensors"]) and all(l["weight_exp"] == 0 for l in rep["layers"])
    got = [eng.be.to_host(v) for v in eng.forward(rgb)]
    for a, b in zip(want, got):
        assert a.tobytes() == b.tobytes()
    eng.close()


def check_no_instance_rejected_at_load(lib):
    """a format the library holds no kernel instance of fails in load_state_dict, not at the first forward"""
    g, sd, rgb = load("g5_fcn_k7_66x130_wide")
    eng = engine(lib, g, formats={15: "a2"})
    try:
        eng.load_state_dict(sd)
    except _lib.LecturemathError as e:
        assert "no kernel" in str(e), e
    else:
        raise AssertionError("a 3x3 layer on format a2 was accepted at load")
    finally:
        eng.close()


def check_all_zero_tensor_settles(lib):
    """a tensor that is truly zero on the calibration frame (BN weight and bias of mid_block set to zero) costs two steps, not twelve, and is
    named in the report"""
    g, sd, rgb = load("g5_fcn_k7_66x130_wide")
    sd = dict(sd)
    sd["mid_block.1.weight"] = np.zeros_like(sd["mid_block.1.weight"])
    sd["mid_block.1.bias"] = np.zeros_like(sd["mid_block.1.bias"])
    eng = engine(lib, g, range_guard="rescale")
    eng.load_state_dict(sd)
    rep = eng.calibrate([rgb])
    mid = rep["tensors"][11]
    assert mid["name"] == "mid" and mid["all_zero"] and mid["exp"] == -16, mid
    assert rep["passes"] <= 4 and eng.planar, rep["passes"]
    eng.close()
