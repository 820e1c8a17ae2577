#!/usr/bin/env python3
"""G15: FCN-LectureNet golden vectors whose activations and BN-folded weights leave f16's range while the fp32 network stays
well-behaved, produced by the REFERENCE module (container-only; see make_golden.py and make_golden_fcn.py).

Construction (compensated scaling of oracle.fcn.random_state_dict): the BatchNorm weight / bias that produce a tensor are multiplied by
2^a (per tensor, or per channel), and every consumer's convolution weights for those input channels by 2^-a.  GELU is not homogeneous,
so this is a different network from the unscaled one -- not a rescaled copy of it -- but one whose logits stay of order one.
  g15_fcn_range_scaled: one exponent per tensor, spread over +-12, one tensor at +18 and one at -14: per-tensor exponents recover it.
  g15_fcn_range_spread: inside down3_pre half the channels at 2^+18 and half at 2^-18: no per-tensor exponent fits both.
Each file holds what g5_fcn_*.npz holds plus "max.<name>": the oracle's fp32 max |x| of all 25 tensors of the planar engine and of
text / rec ("halfmax.*" for the two channel halves of the spread tensor).  The conditions a fixture must meet are asserted here, on the CPU, before it is written.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
import ref_env  # noqa: E402

assert ref_env.available()
ref_env.enter()
import torch  # noqa: E402
from PIL import Image  # noqa: E402
from AccessMath.lecturenet_v1.FCN_lecturenet import FCN_LectureNet  # noqa: E402
from lecturemath_amd import synth  # noqa: E402
from oracle import fcn as ofcn  # noqa: E402

# Multiples of 16 (the planar engine accepts them), as narrow as that allows: a committed file may not exceed 1 MiB (MAX_BYTES), and the
# full-resolution x_up1 that every g5 file holds is 549 KB at 16 channels already; with g5's wide widths a file comes to 1.37 MB.
WIDTHS = (16, 16, 32, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16)
MAX_BYTES = 1 << 20
PK, H, W, SEED = 7, 66, 130, 15
F16_MAX = 65504.0

# tensor -> (BatchNorm producing it, [(consumer weight, axis of its input channels, first channel or None for all)])
d1, d2, d3, d4, d5, mid, u5, c5, u4, c4, u3, c3, u2, c2, u1, c1, pm1, pm2 = WIDTHS
UPS = {5: u5, 4: u4, 3: u3, 2: u2, 1: u1}
TENSORS = {}
for n in range(1, 6):
    cons = [("conv_up_block_%d.0.weight" % n, 1, UPS[n])]
    cons.append(("conv_down_block_%d.0.weight" % (n + 1), 1, 0) if n < 5 else ("mid_block.0.weight", 1, 0))
    TENSORS["down%d_pre" % n] = ("conv_down_block_%d.1" % n, cons)
TENSORS["mid"] = ("mid_block.1", [("transposed_conv_5.weight", 0, 0)])
for n in range(5, 0, -1):
    TENSORS["upsample%d" % n] = ("upsample_block_%d.0" % n, [("conv_up_block_%d.0.weight" % n, 1, 0)])
    if n > 1:
        TENSORS["up%d" % n] = ("conv_up_block_%d.1" % n, [("transposed_conv_%d.weight" % (n - 1), 0, 0)])
TENSORS["up1"] = ("conv_up_block_1.1", [("conv_text_mask_out.0.weight", 1, 0), ("conv_reconstruct.0.weight", 1, 0), ("conv_pixels_1.0.weight", 1, 3)])
TENSORS["p1"] = ("conv_pixels_1.1", [("conv_pixels_2.0.weight", 1, 3)])
TENSORS["p2"] = ("conv_pixels_2.1", [("conv_out.0.weight", 1, 3)])

SCALED = {"down1_pre": 3, "down2_pre": -7, "down3_pre": 18, "down4_pre": -12, "down5_pre": 9, "mid": -5, "upsample5": 12, "up5": -14,
          "upsample4": 6, "up4": -9, "upsample3": 11, "up3": -3, "upsample2": -11, "up2": 8, "upsample1": -6, "up1": 10, "p1": -8, "p2": 5}
SPREAD_TENSOR, SPREAD_EXP = "down3_pre", 18


def scale_tensor(sd, name, exps):
    """exps: one exponent per channel of tensor `name`"""
    bn, consumers = TENSORS[name]
    f = torch.tensor([2.0 ** int(e) for e in exps], dtype=torch.float32)
    assert len(f) == sd[bn + ".weight"].numel(), (name, len(f))
    sd[bn + ".weight"] = sd[bn + ".weight"] * f
    sd[bn + ".bias"] = sd[bn + ".bias"] * f
    for key, axis, first in consumers:
        w = sd[key].clone()
        shape = [1] * w.ndim
        shape[axis] = -1
        idx = [slice(None)] * w.ndim
        idx[axis] = slice(first, first + len(f))
        w[tuple(idx)] = w[tuple(idx)] / f.reshape(shape)
        sd[key] = w


def build_reference(widths, pk):
    a = list(widths)
    return FCN_LectureNet(3, *a[:16], 3, a[16], a[17], pk, False)


def emit(name, sd, extra_checks):
    net = build_reference(WIDTHS, PK)
    net.load_state_dict(sd, strict=True)
    net.eval()
    rgb, _ = synth.whiteboard_rgb(H, W, n_glyphs=25, seed=SEED)
    pil = Image.fromarray(rgb)
    with torch.no_grad():
        x0 = FCN_LectureNet.prepare_image(pil)
        out, text, rec = net.forward(x0)
        x_up1 = net.encode_decode(x0)
        o2, t2, r2, inter = ofcn.forward(sd, ofcn.prepare_image(rgb), return_intermediates=True)
    binary, text_mask, rec_img = net.binarize(pil, return_others=True, force_binary=True)
    # ---- the conditions the reference alone must satisfy
    for v in (out, text, rec):
        assert torch.isfinite(v).all()
    assert float(out.abs().max()) <= 4 and float(text.abs().max()) <= 4, (float(out.abs().max()), float(text.abs().max()))
    # the oracle agrees with the module as test_oracle_golden.test_g5_fcn asks (x_up1 carries a 2^a: the same bar relative to its maximum)
    assert float((o2 - out).abs().max()) <= 1e-6 and float((t2 - text).abs().max()) <= 1e-6 and float((r2 - rec).abs().max()) <= 1e-6
    assert float((inter["up1"] - x_up1).abs().max()) <= 1e-6 * max(1.0, float(x_up1.abs().max()))
    b, t, r = ofcn.binarize(sd, rgb)
    assert (b == binary).all() and (t == text_mask).all() and (r == rec_img).all()
    o = {"widths": np.asarray(WIDTHS), "pk": np.int64(PK), "rgb": rgb, "out": out.numpy(), "text": text.numpy(), "rec": rec.numpy(),
         "x_up1": x_up1.numpy(), "binary": binary, "text_mask": text_mask, "rec_img": rec_img}
    maxima = {k: float(v.abs().max()) for k, v in inter.items()}
    # what oracle.fcn.forward does not keep: the network input, the pooled copies and the transposed convolutions' outputs
    with torch.no_grad():
        maxima["x0"] = float(x0.abs().max())
        x = inter["mid"]
        for n in range(5, 0, -1):
            maxima["down%d_pool" % n] = float(torch.nn.functional.max_pool2d(inter["down%d_pre" % n], 2).abs().max())
            maxima["upsample%d" % n] = float(ofcn._up(sd, n, x, inter["down%d_pre" % n].shape[2:]).abs().max())
            x = inter["up%d" % n]
    extra_checks(inter, maxima, o)
    for k, v in maxima.items():
        o["max." + k] = np.float64(v)
    for k, v in sd.items():
        o["sd." + k] = v.numpy()
    path = os.path.join(HERE, "g15_fcn_range_%s.npz" % name)
    np.savez_compressed(path, **o)
    assert os.path.getsize(path) <= MAX_BYTES, os.path.getsize(path)
    print(name, "bytes", os.path.getsize(path), "max |out| %.3f std %.3f" % (float(out.abs().max()), float(out.std())),
          "ink frac %.3f" % (binary == 0).mean(), "maxima", {k: "%.3g" % v for k, v in maxima.items()})


def check_scaled(inter, maxima, o):
    planar = [k for k in maxima if k not in ("text", "rec", "diff", "x0")]
    assert max(maxima[k] for k in planar) >= 4 * F16_MAX and min(maxima[k] for k in planar) <= 2.0 ** -10, maxima
    o["exp_names"] = np.asarray(sorted(SCALED))
    o["exp_values"] = np.asarray([SCALED[k] for k in sorted(SCALED)], np.int64)


def check_spread(inter, maxima, o):
    t = inter[SPREAD_TENSOR]
    half = t.shape[1] // 2
    hi, lo = float(t[:, :half].abs().max()), float(t[:, half:].abs().max())
    assert hi >= 4 * F16_MAX and lo <= 2.0 ** -10, (hi, lo)
    o["halfmax." + SPREAD_TENSOR] = np.asarray([hi, lo], np.float64)
    o["spread_tensor"] = np.asarray(SPREAD_TENSOR)


sd = ofcn.random_state_dict(WIDTHS, pixel_kernel=PK, seed=SEED)
for name, e in SCALED.items():
    scale_tensor(sd, name, [e] * sd[TENSORS[name][0] + ".weight"].numel())
emit("scaled", sd, check_scaled)

sd = ofcn.random_state_dict(WIDTHS, pixel_kernel=PK, seed=SEED + 1)
c = sd[TENSORS[SPREAD_TENSOR][0] + ".weight"].numel()
scale_tensor(sd, SPREAD_TENSOR, [SPREAD_EXP] * (c // 2) + [-SPREAD_EXP] * (c - c // 2))
emit("spread", sd, check_spread)
