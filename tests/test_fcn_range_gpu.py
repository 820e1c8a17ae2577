"""GPU: the f16 range calibration of the planar FCN engine on the device (bodies: tests/fcn_range_checks.py), the shipped widths at
1920x1080 with one full-resolution tensor out of f16's range, and the drop-in class under LM_FCN_RANGE."""
import numpy as np
import pytest

import fcn_range_checks as rc

pytestmark = pytest.mark.gpu


def test_scaled_without_guard_is_wrong(hip_lib):
    rc.check_hole_without_guard(hip_lib)


def test_scaled_rescale(hip_lib):
    rc.check_scaled_rescale(hip_lib)


def test_spread_needs_promotion(hip_lib):
    rc.check_spread(hip_lib)


def test_in_range_network_is_untouched(hip_lib):
    rc.check_identity(hip_lib)


def test_all_zero_tensor_settles(hip_lib):
    rc.check_all_zero_tensor_settles(hip_lib)


def test_format_without_instance_rejected_at_load(hip_lib):
    rc.check_no_instance_rejected_at_load(hip_lib)


def test_shipped_config_1080p_scaled_tensor_vs_oracle(hip_lib):
    """shipped widths, 1920x1080: down1_pre (full resolution) carries a compensated 2^18 -- BN weight / bias of conv_down_block_1 times 2^18,
    the weights of conv_down_block_2 and the skip half of conv_up_block_1 times 2^-18 -- against oracle.fcn.forward on the same state dict"""
    import torch
    from lecturemath_amd import fcn, synth
    from oracle import fcn as ofcn
    H, W = 1080, 1920
    widths = ofcn.SHIPPED_WIDTHS
    sd = ofcn.random_state_dict(widths, pixel_kernel=7, seed=0)
    f = 2.0 ** 18
    sd["conv_down_block_1.1.weight"] = sd["conv_down_block_1.1.weight"] * f
    sd["conv_down_block_1.1.bias"] = sd["conv_down_block_1.1.bias"] * f
    sd["conv_down_block_2.0.weight"] = sd["conv_down_block_2.0.weight"] / f
    u1 = widths[14]
    w = sd["conv_up_block_1.0.weight"].clone()
    w[:, u1:] = w[:, u1:] / f
    sd["conv_up_block_1.0.weight"] = w
    rgb, _ = synth.whiteboard_rgb(H, W, 1500, seed=20211)
    with torch.no_grad():
        want = [v.numpy() for v in ofcn.forward(sd, ofcn.prepare_image(rgb))]
    assert all(np.isfinite(v).all() for v in want) and np.abs(want[0]).max() <= 4
    eng = fcn.FcnEngine(widths, 7, 3, H, W, hip_lib, range_guard="rescale")
    eng.load_state_dict(sd)
    rep = eng.calibrate([rgb])
    assert eng.planar and eng.tensor_exp[1] > 0 and eng.tensor_exp[6] == eng.tensor_exp[1]
    for n, a, b in zip(("out", "text", "rec"), want, eng.forward(rgb)):
        err = float(np.abs(eng.be.to_host(b).reshape(a.shape) - a).max())
        print(n, "max |engine - oracle| %.3g" % err, "passes", rep["passes"])
        assert err <= rc.TOL, (n, err)
    eng.close()


def test_dropin_class_calibrates_under_env(hip_lib, monkeypatch):
    """LM_FCN_RANGE=promote: the first binarize() of the drop-in class calibrates on its own frame before answering"""
    import PIL.Image
    from lecturemath_amd.dropin.AccessMath.lecturenet_v1.FCN_lecturenet import FCN_LectureNet
    from oracle import fcn as ofcn
    monkeypatch.setenv("LM_FCN_RANGE", "promote")
    g, sd, rgb = rc.load("g15_fcn_range_scaled")
    w = [int(v) for v in g["widths"]]
    net = FCN_LectureNet(3, *w[:16], 3, w[16], w[17], int(g["pk"]), False)
    net.load_state_dict(sd)
    binary, text_mask, rec_img = net.binarize(PIL.Image.fromarray(rgb), return_others=True, force_binary=True)
    assert net._engine.calibration is not None and np.count_nonzero(net._engine.tensor_exp) > 0
    # the reference's byte images: logits within 1e-3 may cross the threshold on a handful of pixels
    assert (binary != g["binary"]).mean() <= 1e-3 and (text_mask != g["text_mask"]).mean() <= 1e-3
    assert np.abs(rec_img.astype(int) - g["rec_img"].astype(int)).max() <= 1


def test_dropin_video_path_calibrates_both_engines(hip_lib, monkeypatch):
    """LM_FCN_RANGE=rescale: binarize_frames_device (the pipeline's whole-video path: two engines on two streams, frames dealt alternately)
    calibrates on its first frame and gives the second engine the same exponents; forward_logits calibrates alike"""
    import torch
    from lecturemath_amd.dropin.AccessMath.lecturenet_v1.FCN_lecturenet import FCN_LectureNet
    monkeypatch.setenv("LM_FCN_RANGE", "rescale")
    g, sd, rgb = rc.load("g15_fcn_range_scaled")
    w = [int(v) for v in g["widths"]]
    net = FCN_LectureNet(3, *w[:16], 3, w[16], w[17], int(g["pk"]), False)
    net.load_state_dict(sd)
    frames = np.stack([rgb] * 4)
    got = net.binarize_frames_device(frames).cpu().numpy()
    e1, e2 = net._engine, net._engine2
    assert e1.calibration is not None and e2 is not None and e2.calibration is e1.calibration
    assert np.count_nonzero(e1.tensor_exp) > 0 and (e1.tensor_exp == e2.tensor_exp).all() and (e1.layer_wexp == e2.layer_wexp).all()
    want = np.where(g["binary"] == 0, 255, 0).astype(np.uint8)          # the worker's inverted binary: ink = 255
    for i in range(4):                                                  # frames 1 and 3 come from the second engine
        assert (got[i] != want).mean() <= 1e-3, (i, float((got[i] != want).mean()))
    assert (got[1] == got[0]).all() and (got[3] == got[2]).all()
    net2 = FCN_LectureNet(3, *w[:16], 3, w[16], w[17], int(g["pk"]), False)
    net2.load_state_dict(sd)
    out, text, rec = net2.forward_logits(rgb)
    assert net2._engine.calibration is not None
    assert float(np.abs(out.cpu().numpy().reshape(g["out"].shape) - g["out"]).max()) <= rc.TOL
