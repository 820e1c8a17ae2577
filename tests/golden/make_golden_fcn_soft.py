#!/usr/bin/env python3
"""G19: the REFERENCE module's soft outputs for the G5 cases (container-only; see make_golden.py).

binarize(pil, return_others=True, force_binary=False): binary = trunc(sigmoid(logit) * 255) and text_mask likewise, uint8, keyed
"<case name>.binary" / "<case name>.text_mask".  Inputs, state dicts and heads stay in the g5_fcn_*.npz files: the networks are
rebuilt from them here, and the heads this run sees are asserted equal to the recorded ones.
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

CASES = ["k7_70x94", "k3_135x240", "k7_66x130_wide"]

o = {}
for name in CASES:
    g = np.load(os.path.join(HERE, "g5_fcn_%s.npz" % name))
    d1, d2, d3, d4, d5, mid, u5, c5, u4, c4, u3, c3, u2, c2, u1, c1, pm1, pm2 = (int(v) for v in g["widths"])
    net = FCN_LectureNet(3, d1, d2, d3, d4, d5, mid, u5, c5, u4, c4, u3, c3, u2, c2, u1, c1, 3, pm1, pm2, int(g["pk"]), False)
    net.load_state_dict({k[3:]: torch.from_numpy(np.asarray(g[k])) for k in g.files if k.startswith("sd.")}, strict=True)
    net.eval()
    pil = Image.fromarray(g["rgb"])
    with torch.no_grad():
        out, text, _ = net.forward(FCN_LectureNet.prepare_image(pil))
    assert (out.numpy() == g["out"]).all() and (text.numpy() == g["text"]).all(), "the heads of this run are not the recorded ones"
    binary, text_mask, rec_img = net.binarize(pil, return_others=True, force_binary=False)
    assert (rec_img == g["rec_img"]).all()
    o[name + ".binary"], o[name + ".text_mask"] = binary, text_mask
    print(name, binary.shape, "levels", len(np.unique(binary)), len(np.unique(text_mask)))
np.savez_compressed(os.path.join(HERE, "g19_fcn_soft.npz"), **o)
