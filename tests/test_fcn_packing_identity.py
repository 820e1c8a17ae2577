"""CPU: everything FcnEngine hands to the library -- descriptors, packed weights, biases, lo flags, exponents, in call order -- is byte for
byte what tests/golden/g16_fcn_packing.json recorded (tests/golden/make_golden_fcn_packing.py).  The engine is driven through its public
API only (constructor, load_state_dict, calibrate, copy_calibration) with a recording proxy in front of the emulated library, so the same
file checks any revision of the host side against the digests of the one that wrote them."""
import ctypes
import functools
import hashlib
import json
import os

import numpy as np
import pytest

from lecturemath_amd import fcn, synth

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_JSON = os.path.join(GOLD, "g16_fcn_packing.json")
N_TENSORS, N_LAYERS, N_WIDTHS = 25, 21, 18          # array lengths of the C ABI (include/lecturemath_amd.h)
ENV_KEYS = ("LM_FCN2_FUSED_HEADS", "LM_FCN_RANGE", "LM_FCN_FORMATS")


def _bytes(p, nbytes):
    if p is None:
        return b""
    if isinstance(p, ctypes.Array):
        return bytes(p)[:nbytes]
    return ctypes.string_at(p, nbytes)


class RecordingLib:
    """The library with its four weight-taking entry points recorded: per call the scalar arguments and the SHA-256 of the bytes behind
    every pointer argument.  forward=False answers the create / set / destroy calls of both engines here, so that a 1080p configuration
    allocates no arena under emulation (packing sees max_h / max_w only through tile counts)."""

    def __init__(self, lib, forward):
        self._lib, self._forward = lib, forward
        self.calls = []

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def _record(self, fn, scalars, **blobs):
        self.calls.append({"fn": fn, "scalars": [int(v) for v in scalars],
                           "blobs": {k: [len(v), hashlib.sha256(v).hexdigest()] for k, v in sorted(blobs.items())}})

    def lm_fcn_create(self, widths, pk, kk, max_h, max_w):
        self._record("lm_fcn_create", (pk, kk, max_h, max_w), widths=_bytes(widths, 4 * N_WIDTHS))
        return self._lib.lm_fcn_create(widths, pk, kk, max_h, max_w) if self._forward else 1

    def lm_fcn2_create(self, widths, lo, max_h, max_w):
        self._record("lm_fcn2_create", (max_h, max_w), widths=_bytes(widths, 4 * N_WIDTHS), lo=_bytes(lo, 4 * N_TENSORS))
        return self._lib.lm_fcn2_create(widths, lo, max_h, max_w) if self._forward else 2

    def lm_fcn_destroy(self, handle):
        if self._forward:
            self._lib.lm_fcn_destroy(handle)

    def lm_fcn2_destroy(self, handle):
        if self._forward:
            self._lib.lm_fcn2_destroy(handle)

    def lm_fcn_set_layer(self, handle, layer, w, nw, b, nb, cin, cout, k, ck):
        self._record("lm_fcn_set_layer", (layer, nw, nb, cin, cout, k, ck), weights=_bytes(w, 4 * nw), bias=_bytes(b, 4 * nb))
        return self._lib.lm_fcn_set_layer(handle, layer, w, nw, b, nb, cin, cout, k, ck) if self._forward else 0

    def lm_fcn2_set_layer(self, handle, layer, desc, ndesc, w, wbytes, wblocks, bias, nbias):
        self._record("lm_fcn2_set_layer", (layer, ndesc, wbytes, wblocks, nbias), desc=_bytes(desc, 4 * ndesc), weights=_bytes(w, wbytes), bias=_bytes(bias, 4 * nbias))
        return self._lib.lm_fcn2_set_layer(handle, layer, desc, ndesc, w, wbytes, wblocks, bias, nbias) if self._forward else 0

    def lm_fcn2_set_scales(self, handle, texp, wexp):
        self._record("lm_fcn2_set_scales", (), tensor_exp=_bytes(texp, 4 * N_TENSORS), layer_wexp=_bytes(wexp, 4 * N_LAYERS))
        return self._lib.lm_fcn2_set_scales(handle, texp, wexp) if self._forward else 0


def canonical(obj):
    return json.dumps(obj, sort_keys=True, separators=(",", ":"), allow_nan=True)


def digest(obj):
    return hashlib.sha256(canonical(obj).encode()).hexdigest()


def summary(proxy, eng):
    """what the golden file keeps of one case"""
    out = {"calls": len(proxy.calls), "bytes": sum(n for c in proxy.calls for n, _ in c["blobs"].values()), "sha256": digest(proxy.calls),
           "engine": eng.precision, "range_report": digest({str(k): v for k, v in sorted(eng.range_report.items())})}
    if eng.calibration is not None:
        out["calibration"] = digest(eng.calibration)
    return out


def _sd(widths, pk, seed):
    return {k: v.numpy() for k, v in synth.fcn_random_state_dict(widths, pixel_kernel=pk, seed=seed).items()}


def _golden_sd(name):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    return g, {k[3:]: g[k] for k in g.files if k.startswith("sd.")}


SHIPPED = synth.FCN_SHIPPED_WIDTHS
PLANAR_TINY = (16, 32, 16, 16, 16, 32, 32, 16, 16, 16, 16, 16, 16, 48, 16, 32, 32, 16)        # tests/test_kernel_logic_emulated.py
NOT_16 = (8, 16, 16, 8, 8, 8, 8, 8, 8, 8, 16, 16, 8, 8, 8, 8, 16, 8)

# name -> (widths, pixel kernel, max_h, max_w, seed, constructor keywords, environment)
LOAD_CASES = {
    "planar_mixed_1080p": (SHIPPED, 7, 1080, 1920, 11, {"precision": "mixed"}, {}),
    "planar_f16x3_1080p": (SHIPPED, 7, 1080, 1920, 11, {"precision": "planar-f16x3"}, {}),
    "planar_f16_1080p": (SHIPPED, 7, 1080, 1920, 11, {"precision": "planar-f16"}, {}),
    "planar_mixed_formats_1080p": (SHIPPED, 7, 1080, 1920, 11, {"precision": "mixed", "formats": {15: "f16x3", 18: "a2"}}, {}),
    "planar_mixed_fused3_1080p": (SHIPPED, 7, 1080, 1920, 11, {"precision": "mixed"}, {"LM_FCN2_FUSED_HEADS": "3"}),
    "planar_mixed_fused0_1080p": (SHIPPED, 7, 1080, 1920, 11, {"precision": "mixed"}, {"LM_FCN2_FUSED_HEADS": "0"}),
    "planar_mixed_rescale_guard_1080p": (SHIPPED, 7, 1080, 1920, 11, {"precision": "mixed", "range_guard": "rescale"}, {}),
    "planar_mixed_guard_off_1080p": (SHIPPED, 7, 1080, 1920, 11, {"precision": "mixed", "range_guard": "off"}, {}),
    "planar_mixed_tiny_45x61": (PLANAR_TINY, 7, 45, 61, 1, {"precision": "mixed"}, {}),
    "planar_f16x3_tiny_45x61": (PLANAR_TINY, 7, 45, 61, 1, {"precision": "planar-f16x3"}, {}),
    "first_fp32": (SHIPPED, 7, 1080, 1920, 11, {"precision": "fp32"}, {}),
    "first_f16x3": (SHIPPED, 7, 1080, 1920, 11, {"precision": "f16x3"}, {}),
    "first_f16x2": (SHIPPED, 7, 1080, 1920, 11, {"precision": "f16x2"}, {}),
    "first_f16": (SHIPPED, 7, 1080, 1920, 11, {"precision": "f16"}, {}),
    "first_valu_heads_8_k3_f16x3": ((8,) * 18, 3, 64, 96, 3, {"precision": "f16x3"}, {}),
    "first_valu_heads_8_k3_fp32": ((8,) * 18, 3, 64, 96, 3, {"precision": "fp32"}, {}),
    "first_mixed_falls_back": (NOT_16, 7, 64, 96, 2, {"precision": "mixed"}, {}),
    "first_planar_f16_falls_back": (NOT_16, 7, 64, 96, 2, {"precision": "planar-f16"}, {}),
}
LADDER_CASES = ("ladder_scaled_rescale", "ladder_spread_promote", "copy_calibration")
CASES = list(LOAD_CASES) + list(LADDER_CASES)


@functools.lru_cache(maxsize=None)
def _ladder(lib, name, guard):
    """a g15 fixture loaded and calibrated on the emulator (minutes: run once per process, the engine stays open for copy_calibration)"""
    g, sd = _golden_sd(name)
    proxy = RecordingLib(lib, forward=True)
    h, w = g["rgb"].shape[:2]
    eng = fcn.FcnEngine(g["widths"], int(g["pk"]), 3, h, w, proxy, range_guard=guard)
    eng.load_state_dict(sd)
    eng.calibrate([g["rgb"]])
    return g, sd, proxy, eng


def run_case(lib, name):
    saved = {k: os.environ.pop(k, None) for k in ENV_KEYS}
    try:
        if name in LOAD_CASES:
            widths, pk, max_h, max_w, seed, kw, env = LOAD_CASES[name]
            os.environ.update(env)
            proxy = RecordingLib(lib, forward=False)
            eng = fcn.FcnEngine(widths, pk, 3, max_h, max_w, proxy, **kw)
            eng.load_state_dict(_sd(widths, pk, seed))
        elif name == "ladder_scaled_rescale":
            _, _, proxy, eng = _ladder(lib, "g15_fcn_range_scaled", "rescale")
            assert eng.planar and eng.tensor_exp.any() and eng.layer_wexp.any()
        elif name == "ladder_spread_promote":
            _, _, proxy, eng = _ladder(lib, "g15_fcn_range_spread", "promote")
            assert not eng.planar and eng.calibration["promoted"]
        else:
            g, sd, _, first = _ladder(lib, "g15_fcn_range_scaled", "rescale")
            proxy = RecordingLib(lib, forward=True)
            h, w = g["rgb"].shape[:2]
            eng = fcn.FcnEngine(g["widths"], int(g["pk"]), 3, h, w, proxy, range_guard="rescale")
            eng.load_state_dict(sd)
            eng.copy_calibration(first)
            assert (eng.tensor_exp == first.tensor_exp).all() and (eng.layer_wexp == first.layer_wexp).all() and eng.calibration is first.calibration
        return summary(proxy, eng), proxy.calls
    finally:
        for k in ENV_KEYS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def test_cases_cover_the_golden_file():
    assert sorted(json.load(open(GOLDEN_JSON))["cases"]) == sorted(CASES)


@pytest.mark.parametrize("name", CASES)
def test_packing_identity(emu_lib, name):
    want = json.load(open(GOLDEN_JSON))["cases"][name]
    got, calls = run_case(emu_lib, name)
    if got != want:
        for c in calls:
            print(c["fn"], c["scalars"], {k: (v[0], v[1][:12]) for k, v in c["blobs"].items()})
    assert got == want
