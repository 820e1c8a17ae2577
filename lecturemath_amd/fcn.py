"""Host side of the HIP FCN-LectureNet: a class with the reference's inference API (AccessMath/lecturenet_v1/FCN_lecturenet.py:
CreateFromConfig :620-659, load_state_dict, eval, cuda, binarize :430-505) so the step-01 worker and test_FCN_binarizer.py can use it unchanged.
FcnEngine chooses the engine, folds the state dict and hands the layers to the library (where all convolution arithmetic runs):
  fcn2.py       the planar engine (csrc/lm_fcn2.hip, the default): tensor and layer tables, recipes, the network walk planar_layers;
  fcn1.py       the first engine (csrc/lm_fcn.hip): the pack_* functions and the walk first_engine_layers;
  fcn_range.py  the f16 range ladder behind calibrate()."""
import ctypes
import os

import numpy as np

from . import _lib, fcn1, fcn2, fcn_range
from .device import Backend
from .fcn1 import _pad8, pack_mfma, pack_mfma_h, pack_rows_h, pack_small, pack_text_rec_rows_h  # noqa: F401
from .fcn2 import L_DOWN, L_MID, L_OUT, L_PX1, L_PX2, L_REC, L_TEXT, L_UPC, L_UPT  # noqa: F401
from .fcn_range import (LOST_BITS_EXP, LOST_SHARE, MAX_PASSES, OVERFLOW_STEP, RANGE_GUARDS, TENSOR_BAND, TENSOR_TARGET,  # noqa: F401
                        WEIGHT_BAND, WEIGHT_TARGET, ZERO_STEPS)

BN_EPS = 1e-5

WIDTH_KEYS = [  # CreateFromConfig :621-646, with its defaults
    ("FCN_BINARIZER_NET_DOWN_CONV_FILTERS_1", 16), ("FCN_BINARIZER_NET_DOWN_CONV_FILTERS_2", 32),
    ("FCN_BINARIZER_NET_DOWN_CONV_FILTERS_3", 64), ("FCN_BINARIZER_NET_DOWN_CONV_FILTERS_4", 128),
    ("FCN_BINARIZER_NET_DOWN_CONV_FILTERS_5", 256), ("FCN_BINARIZER_NET_MIDDLE_CONV_FILTERS_MIDDLE", 512),
    ("FCN_BINARIZER_NET_UPSAMPLE_FILTERS_5", 256), ("FCN_BINARIZER_NET_UP_CONV_FILTERS_5", 256),
    ("FCN_BINARIZER_NET_UPSAMPLE_FILTERS_4", 128), ("FCN_BINARIZER_NET_UP_CONV_FILTERS_4", 128),
    ("FCN_BINARIZER_NET_UPSAMPLE_FILTERS_3", 64), ("FCN_BINARIZER_NET_UP_CONV_FILTERS_3", 64),
    ("FCN_BINARIZER_NET_UPSAMPLE_FILTERS_2", 32), ("FCN_BINARIZER_NET_UP_CONV_FILTERS_2", 32),
    ("FCN_BINARIZER_NET_UPSAMPLE_FILTERS_1", 16), ("FCN_BINARIZER_NET_UP_CONV_FILTERS_1", 16),
    ("FCN_BINARIZER_NET_PIXEL_FEATURES_1", 32), ("FCN_BINARIZER_NET_PIXEL_FEATURES_2", 16),
]



def _np(v):
    return v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)


def fold_bn(w, b, sd, bn, out_axis):
    """conv (or transposed conv) followed by eval-mode BatchNorm -> one affine conv, in fp32."""
    g, beta = _np(sd[bn + ".weight"]).astype(np.float32), _np(sd[bn + ".bias"]).astype(np.float32)
    mean, var = _np(sd[bn + ".running_mean"]).astype(np.float32), _np(sd[bn + ".running_var"]).astype(np.float32)
    s = (g / np.sqrt(var + np.float32(BN_EPS))).astype(np.float32)
    shape = [1] * w.ndim
    shape[out_axis] = -1
    return (w * s.reshape(shape)).astype(np.float32), ((b - mean) * s + beta).astype(np.float32)


def fold_state_dict(sd):
    """{reference module name: (w, b)} in fp32 with every BatchNorm folded into the convolution (or transposed convolution) before it"""
    def conv(name):
        return _np(sd[name + ".weight"]).astype(np.float32), _np(sd[name + ".bias"]).astype(np.float32)
    blocks = ["conv_down_block_%d" % n for n in range(1, 6)] + ["mid_block"] + ["conv_up_block_%d" % n for n in range(1, 6)]
    folded = {name: fold_bn(*conv(name + ".0"), sd, name + ".1", 0) for name in blocks + ["conv_text_mask_out", "conv_reconstruct", "conv_pixels_1", "conv_pixels_2", "conv_out"]}
    folded.update({"transposed_conv_%d" % n: fold_bn(*conv("transposed_conv_%d" % n), sd, "upsample_block_%d.0" % n, 1) for n in range(1, 6)})      # [Cin][Cout][2][2]
    return folded


def carve_byte_images(be, h, w, want_text=True, want_rec=True):
    """One uint8 device allocation holding binary [h,w], then text [h,w], then rec [h,w,3] (the last two as asked for):
    -> (flat, binary, text | None, rec | None), the images being views of flat.  One copy of flat brings all of them to the host
    (split_byte_images)."""
    n = h * w
    flat = be.empty((n * (1 + (1 if want_text else 0) + (3 if want_rec else 0)),), np.uint8)
    return (flat,) + split_byte_images(flat, h, w, want_text, want_rec)


def split_byte_images(flat, h, w, want_text=True, want_rec=True):
    """the views (binary, text | None, rec | None) of carve_byte_images' allocation, or of its copy on the host"""
    n = h * w
    binary = flat[:n].reshape(h, w)
    text = flat[n:2 * n].reshape(h, w) if want_text else None
    at = 2 * n if want_text else n
    rec = flat[at:at + 3 * n].reshape(h, w, 3) if want_rec else None
    return binary, text, rec


class FcnEngine:
    """Device network built from a reference state_dict."""

    # Operand formats of the "mixed" assignment (fcn2.FORMAT_NAMES).  Below full resolution: plain f16 (all 14 layers together change the
    # logits by 3e-5, profiles/r03_fcn_layer_precision.*).  The six full-resolution layers change them by 0.5-3e-4 EACH on plain f16:
    # round 3 kept all of them on the three-product split (2.6e-5 in all); round 4 measured every assignment by what the path does with
    # the logits -- max |logit - oracle| and BINARY FLIPS against the oracle's binarization, 3 seeds at 1920x1080
    # (profiles/r04_fcn_formats.*) -- and moved conv_up_1, the text / reconstruction heads and conv_pixels_1 to "w2" (weights hi + lo,
    # activations hi: two products, and their input tensors need no lo planes at all): 2.1e-4 (bar 1e-3), flips 392 / 26 / 9 of 2.07 M
    # pixels on random-init logits that crowd the threshold (std 0.06-0.12; all-f16x3: 45 / 2 / 1; all-f16: 1034 / 70 / 47).
    # conv_pixels_2 and conv_out stay on the split: each alone costs 1.5-3e-4 on two products.
    MIXED_FORMATS = {L_DOWN: "f16x3", L_UPC + 4: "w2", L_TEXT: "w2", L_REC: "w2", L_PX1: "w2", L_PX2: "f16x3", L_OUT: "f16x3"}
    DEFAULT_MT, DEFAULT_VARIANTS = fcn2.DEFAULT_MT, fcn2.DEFAULT_VARIANTS        # measured channel tiles / kernel variants per layer
    LAYER_NAMES, TENSOR_NAMES, TENSOR_ORDER, FIXED_TENSORS = fcn2.LAYER_NAMES, fcn2.TENSOR_NAMES, fcn2.TENSOR_ORDER, fcn2.FIXED_TENSORS

    def __init__(self, widths, pixel_kernel, kernel, max_h, max_w, lib=None, precision="mixed", formats=None, range_guard=None):
        """precision:
        "mixed" (default) -- the planar engine (csrc/lm_fcn2.hip): f16 hi + lo split operands (three MFMAs per product, ~22 bits per
            operand) in the full-resolution layers, plain f16 operands below; needs the shipped kernel sizes (7x7 pixel branch, 3x3
            elsewhere) and widths that are multiples of 16, otherwise this falls back to "f16x3";
        "planar-f16x3" / "planar-f16" -- the planar engine with one format everywhere; "planar-f16x3" is the accuracy-first choice
            (hi + lo operands in every layer: 4.25 ms per 1080p frame against 2.13 for "mixed", profiles/r06_fcn_range.json; "mixed" with only
            the six full-resolution layers on f16x3 measures 2.6e-5 max logit error against 2.1e-4, profiles/r04_fcn_formats.json);
        "f16x3" / "f16x2" / "f16" / "fp32" -- the first engine (csrc/lm_fcn.hip): fp32 activations, operands split while staged
            (three, two or one f16 MFMA per product) or exact fp32 MFMA chains."""
        assert precision in ("mixed", "planar-f16x3", "planar-f16", "f16x3", "f16x2", "f16", "fp32")
        # f16 range guard of the planar engine (default: LM_FCN_RANGE, else "check"):
        #   "off"     -- weights are cast to f16 unexamined;
        #   "check"   -- load_state_dict keeps a per-layer weight report (range_report) and raises when a finite weight becomes a non-finite f16;
        #   "rescale" -- load_state_dict also gives a layer whose weights leave f16's comfort band a power-of-two weight exponent, and
        #                calibrate(frames) gives the activation tensors theirs (rung 1);
        #   "promote" -- calibrate() goes on to the fp32 engine (rung 3) where rescaling is not enough.
        range_guard = range_guard or os.environ.get("LM_FCN_RANGE") or "check"
        if range_guard not in RANGE_GUARDS:
            raise _lib.LecturemathError(_lib.LM_ERR_ARG, "range_guard / LM_FCN_RANGE must be one of %s, not %r" % (", ".join(RANGE_GUARDS), range_guard))
        self.range_guard = range_guard
        self.range_report = {}
        self.calibration = None         # the last calibrate() report
        self.tensor_exp = np.zeros(fcn2.N_TENSORS, np.int32)
        self.layer_wexp = np.zeros(fcn2.N_LAYERS, np.int32)
        self._sd = None
        # planar engine only: {layer id: "f16" | "a2" | "w2" | "f16x3"} overriding the precision's assignment (fcn2.FORMAT_NAMES)
        if formats is None and os.environ.get("LM_FCN_FORMATS"):        # experiments: "15=w2,18=a2"
            formats = {int(k): v for k, v in (kv.split("=") for kv in os.environ["LM_FCN_FORMATS"].split(","))}
        self.formats = dict(formats or {})
        # planar engine only: {layer id: (column tiles per wave 1 | 2, loader wave 0 | 1)} -- the kernel variant of a layer (lm_k_g2's NC, LOADER)
        self.variants = dict(self.DEFAULT_VARIANTS)
        self.lib = lib or _lib.load()
        self.be = Backend(self.lib)
        self.widths = [int(v) for v in widths]
        self.pk, self.kk = int(pixel_kernel), int(kernel)
        self.max_h, self.max_w = max_h, max_w
        planar_ok = self.pk == 7 and self.kk == 3 and all(v % 16 == 0 for v in self.widths)
        if precision in ("mixed", "planar-f16x3", "planar-f16") and not planar_ok:
            precision = {"mixed": "f16x3", "planar-f16x3": "f16x3", "planar-f16": "f16"}[precision]
        self.precision = precision
        self.planar = precision in ("mixed", "planar-f16x3", "planar-f16")
        self.handle = self.handle2 = None
        if not self.planar:         # lm_fcn2_create needs the tensors' lo flags: the planar engine is created by load_state_dict
            self._create_first_engine()

    def _create_first_engine(self):
        arr = (ctypes.c_int32 * 18)(*self.widths)
        self.handle = self.lib.lm_fcn_create(arr, self.pk, self.kk, self.max_h, self.max_w)
        if not self.handle:
            raise _lib.LecturemathError(_lib.LM_ERR_ARG, self.lib.last_error())

    def close(self):
        if getattr(self, "handle", None):
            self.lib.lm_fcn_destroy(self.handle)
            self.handle = None
        if getattr(self, "handle2", None):
            self.lib.lm_fcn2_destroy(self.handle2)
            self.handle2 = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def layer_terms(self, layer):
        """operand format of a layer of the planar engine (the TERMS parameter of lm_k_g2, fcn2.FORMAT_NAMES)"""
        if layer in self.formats:
            v = self.formats[layer]
            return fcn2.FORMAT_NAMES[v] if isinstance(v, str) else int(v)
        return {"planar-f16": 1, "planar-f16x3": 3}.get(self.precision) or fcn2.FORMAT_NAMES[self.MIXED_FORMATS.get(layer, "f16")]

    def _load_planar(self, only=None):
        """builds the planar engine's layers (fcn2.planar_layers) from the kept state dict and uploads them.  only: the layers to repack
        into the existing engine (calibrate()); default: all of them, into a new engine"""
        layers = fcn2.planar_layers(fold_state_dict(self._sd), self.widths, self.max_h, self.max_w, self.layer_terms, self.variants, self.DEFAULT_MT,
                                    scale=lambda *a: fcn_range.guarded_weights(self, *a), only=only, fused_heads=int(os.environ.get("LM_FCN2_FUSED_HEADS", "1")))
        if only is None:
            if self.handle2:
                self.lib.lm_fcn2_destroy(self.handle2)
            arr = (ctypes.c_int32 * 18)(*self.widths)
            lo = fcn2.lo_flags(r for r, _ in layers.values())
            self.handle2 = self.lib.lm_fcn2_create(arr, lo.ctypes.data, self.max_h, self.max_w)
            if not self.handle2:
                raise _lib.LecturemathError(_lib.LM_ERR_ARG, self.lib.last_error())
            self.recipes = {}
        for layer, (r, bias) in layers.items():
            desc, bias = r.descriptor(), np.ascontiguousarray(bias, np.float32)
            self.lib.check(self.lib.lm_fcn2_set_layer(self.handle2, layer, desc.ctypes.data, desc.size, r.weights.ctypes.data, r.weights.nbytes, r.wblocks,
                                                      bias.ctypes.data, bias.size))
            self.recipes[layer] = r.summary()
        if self.range_guard != "off":
            self.lib.check(self.lib.lm_fcn2_set_scales(self.handle2, self.tensor_exp.ctypes.data, self.layer_wexp.ctypes.data))

    def executed_gflop(self, h, w):
        """MFMA flops the planar engine EXECUTES for one h x w frame (whole 16 x 16 tiles, whole 32-deep slices, three products per
        operand pair in the split-format layers), as opposed to the network's algorithmic flops"""
        total = 0.0
        for r in self.recipes.values():
            lv = fcn2.TENSORS[r["first_tensor"]].level
            tiles = (((h >> lv) + 15) // 16) * (((w >> lv) + 15) // 16)
            total += 2.0 * tiles * 256 * r["cout"] * r["slices"] * 32 * fcn2.FORMAT_PRODUCTS[r["terms"]] * {fcn2.EPI_TC: 4, fcn2.EPI_TC2: 2}.get(r["epilogue"], 1)
        return total / 1e9

    def load_state_dict(self, sd):
        """sd: the reference's state_dict (torch tensors or numpy arrays).  The engine keeps a reference to it for its lifetime:
        calibrate() repacks layers from it and the fp32 rung reloads it."""
        self._sd = sd
        self.range_report, self.calibration = {}, None
        self.tensor_exp[:] = self.layer_wexp[:] = 0
        if self.planar:
            return self._load_planar()
        for layer, w, b, cin, cout, k, ck in fcn1.first_engine_layers(fold_state_dict(sd), self.widths, self.pk, self.kk, self.precision):
            w, b = np.ascontiguousarray(w, np.float32), np.ascontiguousarray(b, np.float32)
            self.lib.check(self.lib.lm_fcn_set_layer(self.handle, layer, w.ctypes.data, w.size, b.ctypes.data, b.size, cin, cout, k, ck))

    def set_layer_precision(self, layer, precision):
        """Operand format of ONE layer ("f16x3" / "f16x2" / "f16"); the engine must have been loaded with an fp16-split precision."""
        terms = {"f16x3": 3, "f16x2": 2, "f16": 1}[precision]
        if self.planar:
            raise _lib.LecturemathError(_lib.LM_ERR_STATE, "the planar engine's formats are fixed by load_state_dict (precision=...)")
        self.lib.check(self.lib.lm_fcn_set_layer_terms(self.handle, int(layer), terms))

    def calibrate(self, frames, policy=None):
        """Runs `frames` (uint8 [H,W,3] arrays or device tensors, or one of them), reads the range statistics of every activation tensor
        and applies `policy` (default: range_guard; "off" counts as "check"):
          "check"   -- report only; raises when a tensor or an output holds a non-finite value;
          "rescale" -- rung 1: per-tensor / per-layer power-of-two exponents where the measured range leaves the comfort band;
                       raises when that does not bring every tensor into f16's range;
          "promote" -- rung 1; where that is not enough the engine is rebuilt as the first engine with precision="fp32" (rung 3; an
                       f16x3 rung in between is not built: hi + lo adds precision, not range).
        Returns (and keeps as self.calibration) the report: per tensor max |x| in true units, exponent, counts; per layer the format before
        and after; the steps taken; the engine finally in use.  Every step is logged once (logger "lecturemath_amd.fcn").  The ladder: fcn_range.py."""
        policy = policy or self.range_guard
        if policy == "off":
            policy = "check"
        if policy not in RANGE_GUARDS:
            raise _lib.LecturemathError(_lib.LM_ERR_ARG, "calibrate: unknown policy %r" % (policy,))
        if self._sd is None:
            raise _lib.LecturemathError(_lib.LM_ERR_STATE, "FcnEngine.calibrate before load_state_dict")
        if hasattr(frames, "shape") and len(frames.shape) == 3:
            frames = [frames]
        return fcn_range.calibrate(self, list(frames), policy)

    def _rebuild_as_fp32(self):
        """rung 3 of calibrate(): the same network on the first engine with exact fp32 MFMA chains and fp32 activations"""
        self.lib.lm_fcn2_destroy(self.handle2)
        self.handle2 = None
        self.precision, self.planar = "fp32", False
        self._create_first_engine()
        self.load_state_dict(self._sd)

    def copy_calibration(self, other):
        """takes over another engine's calibration (same widths, same state dict loaded): exponents, formats and report.  For the
        second engine of a two-stream pipeline; `other` must still be a planar engine."""
        if not (self.planar and other.planar) or self._sd is None:
            raise _lib.LecturemathError(_lib.LM_ERR_STATE, "copy_calibration: both engines must be loaded planar engines")
        self.tensor_exp[:] = other.tensor_exp
        self.layer_wexp[:] = other.layer_wexp
        self.formats = dict(other.formats)
        self._load_planar()
        self.calibration = other.calibration

    def forward_raw(self, rgb_ptr, h, w, out_ptr, text_ptr=None, rec_ptr=None, stream=None):
        """one forward pass on raw device addresses (uint8 [h,w,3] in; fp32 logit [h,w], text logit [h,w], rec [3,h,w] out, each optional)
        on `stream` (a HIP stream handle; default: the backend's current stream)"""
        fwd, hd = (self.lib.lm_fcn2_forward, self.handle2) if self.planar else (self.lib.lm_fcn_forward, self.handle)
        if not hd:
            raise _lib.LecturemathError(_lib.LM_ERR_STATE, "FcnEngine.forward before load_state_dict")
        self.lib.check(fwd(hd, rgb_ptr, h, w, out_ptr, text_ptr, rec_ptr, self.be.stream() if stream is None else stream))

    def forward(self, rgb):
        """rgb: device (or host numpy) uint8 [H,W,3] -> device fp32 (logit [H,W], text logit [H,W], rec [3,H,W])."""
        if isinstance(rgb, np.ndarray):
            rgb = self.be.from_host(rgb)
        h, w = int(rgb.shape[0]), int(rgb.shape[1])
        out, text, rec = (self.be.empty(shape, np.float32) for shape in ((h, w), (h, w), (3, h, w)))
        self.forward_raw(_lib.ptr(rgb), h, w, _lib.ptr(out), _lib.ptr(text), _lib.ptr(rec))
        return out, text, rec

    def byte_images(self, out, text, rec, threshold=128, soft=False, invert=False, with_buffer=False):
        """The heads of forward() -> the byte images of FCN_LectureNet.binarize (:452-479, :534-555) in one lm_fcn_bytes call:
        device uint8 (binary [H,W], text [H,W], rec [H,W,3] in B G R order), views of ONE allocation (carve_byte_images), so a caller that
        wants them on the host makes one copy.  soft: trunc(sigmoid * 255) instead of {0, 255} by `threshold`; invert: binary is
        255 - value (the step-01 worker's ink = 255).  text / rec may be None: not computed, None returned.  with_buffer: the flat
        allocation comes back as a fourth value."""
        h, w = int(out.shape[0]), int(out.shape[1])
        flat, binary, text_u8, rec_u8 = carve_byte_images(self.be, h, w, text is not None, rec is not None)
        flags = (_lib.LM_FB_SOFT if soft else 0) | (_lib.LM_FB_INVERT if invert else 0)
        self.lib.check(self.lib.lm_fcn_bytes(_lib.ptr(out), _lib.ptr(text), _lib.ptr(rec), h * w, int(threshold), flags, _lib.ptr(binary), _lib.ptr(text_u8),
                                             _lib.ptr(rec_u8), self.be.stream()))
        return (binary, text_u8, rec_u8, flat) if with_buffer else (binary, text_u8, rec_u8)
