"""Host side of the HIP FCN-LectureNet: BatchNorm folding, weight packing into MFMA fragment order, and a class with
the reference's inference API (AccessMath/lecturenet_v1/FCN_lecturenet.py: CreateFromConfig :620-659, load_state_dict,
eval, cuda, binarize :430-505) so the step-01 worker and test_FCN_binarizer.py can use it unchanged.

All convolution arithmetic runs in liblecturemath_hip.so (lm_fcn.hip); numpy here only rearranges weights once.
"""
import ctypes
import logging
import math
import os

import numpy as np

from . import _lib
from .device import Backend

BN_EPS = 1e-5

# layer ids of lm_fcn.hip
L_DOWN, L_MID, L_UPT, L_UPC, L_TEXT, L_REC, L_PX1, L_PX2, L_OUT = 0, 5, 6, 11, 16, 17, 18, 19, 20

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


RANGE_GUARDS = ("off", "check", "rescale", "promote")

# ---- f16 range calibration of the planar engine (FcnEngine.calibrate): the band, the target and the ladder's thresholds, in one place.
# f16 holds |x| <= 65,504 (just under 2^16), is normal down to 2^-14 and carries 11 significant bits.  All figures below are exponents of two.
#   Stored activations (x * 2^-e): a tensor is left alone while floor(log2(max |x|)) lies in [-4, 12).  Above 2^12 fewer than 4 bits of
#   headroom remain for frames the calibration has not seen (overflow is fatal: inf, then NaN downstream).  Below 2^-4 a value 10 bits
#   under the maximum -- still inside the maximum's own 11-bit significand -- is no longer normal (2^-4 * 2^-10 = 2^-14).  A tensor outside
#   the band moves to max in [1, 2): the middle of the normal range on a log scale (15 bits of headroom up, 14 bits down).
#   Packed weights (w * 2^e_in * 2^-k) are known exactly, so they need no headroom: left alone while floor(log2(max |w|)) lies in
#   [-8, 15).  Below 2^-8 the split formats' hi + lo, whose resolution is the subnormal quantum 2^-24, carries fewer than 16 bits of the
#   largest weight and plain f16 loses weights 6 bits under it.  A layer outside the band moves to max in [1/2, 1).
TENSOR_BAND, TENSOR_TARGET = (-4, 12), 0
WEIGHT_BAND, WEIGHT_TARGET = (-8, 15), -1
# An overflowed tensor reads inf: its true scale is unknown, so its exponent rises by a fixed step (half of f16's 16 bits above 1) and the
# frames run again; MAX_PASSES bounds the loop (100 / 8 steps would leave the exponent range lm_fcn2_set_scales accepts).
OVERFLOW_STEP, MAX_PASSES = 8, 16
# A tensor that reads all zero gets the same step downwards at most twice (2^-16 * 2^-24: anything f16 could have flushed from a
# pre-activation of order one is back), then counts as truly zero on the calibration frames and keeps the exponent it has.
ZERO_STEPS = 2
# Rung 2 / 3 trigger, once the exponents are set: the share of a layer's non-zero fp32 weights whose f16 hi part keeps fewer than 6 of its
# 11 bits (|w| < 2^-19, flushed to zero included).  Weights are known exactly, and a scale spread between the channels of one tensor -- which
# no per-tensor exponent can follow -- shows in its consumers' weights, which carry the inverse spread.  The activations' own subnormal and
# zero counts are reported but do not trigger: with the tensor in band a subnormal value is off by at most 2^-25 against a maximum of at
# least 2^-4, and GELU of a large negative number is tiny or zero in fp32 as well.  The weights next to zero are a few percent of any
# smooth distribution; channels go out whole, and the narrowest tensor the planar engine accepts has 16 channels: 1/8 = two of them.
LOST_BITS_EXP = -19
LOST_SHARE = 1.0 / 8.0

_log = logging.getLogger("lecturemath_amd.fcn")


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


def pack_mfma(w_oikk, ck, cin_map, cin_padded):
    """[Cout][Cin][K][K] -> [chunk][tap][kstep][nblock][lane 64][4] for v_mfma_f32_32x32x2_f32:
    element e of lane l = W[co = nblock*32 + (l & 31)][ci = chunk*ck + kstep*8 + 4*(l >> 5) + e][tap].
    cin_map[i] = position of logical input channel i in the padded channel space of the input buffer(s)."""
    cout, cin, k, _ = w_oikk.shape
    nblocks = (cout + 31) // 32
    wp = np.zeros((nblocks * 32, cin_padded, k * k), np.float32)
    wp[:cout][:, np.asarray(cin_map)] = w_oikk.reshape(cout, cin, k * k)
    nchunks, ks = cin_padded // ck, ck // 8
    # wp[co, ci, tap] -> [chunk, ks, half, e, tap, nblock, j]
    a = wp.reshape(nblocks, 32, nchunks, ks, 2, 4, k * k)            # nb, j, chunk, ks, half, e, tap
    a = a.transpose(2, 6, 3, 0, 4, 1, 5)                              # chunk, tap, ks, nb, half, j, e
    return np.ascontiguousarray(a).reshape(-1)


def pack_mfma_h(w_oikk, cin_map, cin_logical):
    """fp16-split packing for lm_k_conv_mfma_h: [chunk][tap][nblock][hi|lo][lane 64][8 halfs], element j of lane l =
    W[co = nblock*32 + (l & 31)][ci = chunk*16 + 8*(l >> 5) + j][tap]; hi = f16(w), lo = f16(w - hi).
    cin_map[i] = position of weight input channel i among the cin_logical concatenated input channels (padded to 16 here).
    Returned as a float32 view (two halfs per float) for lm_fcn_set_layer."""
    cout, cin, kh, kw = w_oikk.shape                                    # square kernels, or the 1 x K rows of pack_rows_h
    taps = kh * kw
    nblocks = (cout + 31) // 32
    cpad = ((cin_logical + 15) // 16) * 16
    wp = np.zeros((nblocks * 32, cpad, taps), np.float32)
    wp[:cout][:, np.asarray(cin_map)] = w_oikk.reshape(cout, cin, taps)
    hi = wp.astype(np.float16)
    lo = (wp - hi.astype(np.float32)).astype(np.float16)
    both = np.stack([hi, lo])                                           # hl, co, ci, tap
    a = both.reshape(2, nblocks, 32, cpad // 16, 2, 8, taps)           # hl, nb, j, chunk, half, e, tap
    a = a.transpose(3, 6, 1, 0, 4, 2, 5)                                # chunk, tap, nb, hl, half, j, e
    return np.ascontiguousarray(a).reshape(-1).view(np.float32)


def pack_rows_h(w_oikk, cin_map, cin_logical):
    """A K x K convolution with NV <= 3 outputs as a 1 x K row convolution with K * NV outputs (lm_rowconv_layer in lm_fcn.hip):
    virtual output kh * NV + co holds kernel row kh of channel co; lm_k_vsum adds the rows up."""
    nv, cin, k, _ = w_oikk.shape
    rows = np.ascontiguousarray(w_oikk.transpose(2, 0, 1, 3)).reshape(k * nv, cin, 1, k)      # [kh][co][ci][kw] -> [kh * NV + co][ci][1][kw]
    return pack_mfma_h(rows, cin_map, cin_logical)


def pack_text_rec_rows_h(w_text, w_rec, cin_map, cin_logical):
    """Text mask (7x7, 1 output) and reconstruction (3x3, 3 outputs) over the same input as ONE 1 x 7 row convolution with 16
    outputs (lm_text_rec_heads): 0..6 = text kernel rows, 7 + kh * 3 + co = reconstruction rows, their taps centred (kw + 2)."""
    cin = w_text.shape[1]
    rows = np.zeros((16, cin, 1, 7), np.float32)
    rows[0:7, :, 0, :] = w_text[0].transpose(1, 0, 2)                   # [ci][kh][kw] -> [kh][ci][kw]
    rows[7:16, :, 0, 2:5] = w_rec.transpose(2, 0, 1, 3).reshape(9, cin, 3)      # [co][ci][kh][kw] -> [kh * 3 + co][ci][kw]
    return pack_mfma_h(rows, cin_map, cin_logical)


def pack_small(w_oikk, cin_map, cin_padded):
    """[Cout<=4][Cin][K][K] -> [chunk of 8 channels][tap][8] for Cout == 1, [chunk][tap][8][4] otherwise (lm_k_conv_small)."""
    cout, cin, k, _ = w_oikk.shape
    lanes = 1 if cout == 1 else 4
    assert cin_padded % 8 == 0
    out = np.zeros((k * k, cin_padded, lanes), np.float32)
    out[:, np.asarray(cin_map), :cout] = w_oikk.reshape(cout, cin, k * k).transpose(2, 1, 0)
    out = out.reshape(k * k, cin_padded // 8, 8, lanes).transpose(1, 0, 2, 3)
    return np.ascontiguousarray(out).reshape(-1)


def _pad8(c):
    return (c + 7) & ~7


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

    # kernel variant per layer, (column tiles per wave, loader wave), measured per layer at 1920x1080 (profiles/r04_variants_*.txt): 16 x 32
    # tiles where the weights are re-fetched per tile at full resolution and the instance keeps two workgroups per CU; the loader wave
    # in the two layers with one workgroup per CU and two channel tiles
    # {layer: channel tiles per workgroup} where fcn2.pick_mt's rule is not the fastest (profiles/r04_mt_{default,a,b}.txt: conv_down_1 on ONE
    # tile = 24,480 small workgroups at 114 VGPRs, 139 -> 124-130 us -- it is a 250 MB store; every other layer is fastest on pick_mt's choice)
    DEFAULT_MT = {L_DOWN: 1}
    DEFAULT_VARIANTS = {L_UPC + 4: (2, 0), L_TEXT: (2, 0), L_PX1: (2, 0), L_PX2: (2, 0), L_MID: (1, 1), L_UPC: (1, 1)}

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
        self.tensor_exp = np.zeros(25, np.int32)
        self.layer_wexp = np.zeros(21, np.int32)
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
        self.handle = None
        self.handle2 = None
        if self.planar:
            return          # lm_fcn2_create needs the tensors' lo flags: created by load_state_dict
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

    def _set(self, layer, w, b, cin, cout, k, ck):
        w = np.ascontiguousarray(w, np.float32)
        b = np.ascontiguousarray(b, np.float32)
        self.lib.check(self.lib.lm_fcn_set_layer(self.handle, layer, w.ctypes.data, w.size, b.ctypes.data, b.size, cin, cout, k, ck))

    def layer_terms(self, layer):
        """operand format of a layer of the planar engine (the TERMS parameter of lm_k_g2, fcn2.FORMAT_NAMES)"""
        from . import fcn2 as f2
        if layer in self.formats:
            v = self.formats[layer]
            return f2.FORMAT_NAMES[v] if isinstance(v, str) else int(v)
        if self.precision == "planar-f16":
            return 1
        if self.precision == "planar-f16x3":
            return 3
        return f2.FORMAT_NAMES[self.MIXED_FORMATS.get(layer, "f16")]

    LAYER_NAMES = {0: "conv_down_block_1", 1: "conv_down_block_2", 2: "conv_down_block_3", 3: "conv_down_block_4", 4: "conv_down_block_5", 5: "mid_block",
                   6: "transposed_conv_5", 7: "transposed_conv_4", 8: "transposed_conv_3", 9: "transposed_conv_2", 10: "transposed_conv_1",
                   11: "conv_up_block_5", 12: "conv_up_block_4", 13: "conv_up_block_3", 14: "conv_up_block_2", 15: "conv_up_block_1",
                   16: "conv_text_mask_out+conv_reconstruct", 18: "conv_pixels_1", 19: "conv_pixels_2", 20: "conv_out"}

    def _range_weights(self, layer, w, inputs, axis=1):
        """The weights of `layer` as they are packed: times 2^e of the tensor feeding each input channel (inputs = [(tensor, channels)] along
        `axis`), times 2^-k of the layer -- k chosen here under "rescale" / "promote" when the weights leave WEIGHT_BAND -- and the layer's
        row of range_report.  All factors are powers of two: with every exponent zero the weights come back unchanged."""
        if self.range_guard == "off":
            return w
        f = np.concatenate([np.full(n, 2.0 ** int(self.tensor_exp[t]), np.float32) for t, n in inputs])
        shape = [1] * w.ndim
        shape[axis] = -1
        w = (w * f.reshape(shape)).astype(np.float32)
        aw = np.abs(w)
        finite = np.isfinite(aw)
        mx = float(aw[finite].max()) if finite.any() else 0.0
        if self.range_guard in ("rescale", "promote"):
            k = int(self.layer_wexp[layer])
            ex = math.floor(math.log2(mx)) - k if mx > 0 else None
            if ex is not None and not (WEIGHT_BAND[0] <= ex < WEIGHT_BAND[1]):
                self.layer_wexp[layer] = k = math.floor(math.log2(mx)) - WEIGHT_TARGET
        k = int(self.layer_wexp[layer])
        w = (w * np.float32(2.0 ** -k)).astype(np.float32)
        aw = np.abs(w)
        with np.errstate(over="ignore"):
            h = np.abs(aw.astype(np.float16))
        bad = finite & ~np.isfinite(h)
        nz = aw > 0
        row = {"layer": layer, "name": self.LAYER_NAMES[layer], "max_abs": float(aw[finite].max()) if finite.any() else 0.0,
               "min_nonzero_abs": float(aw[nz].min()) if nz.any() else 0.0, "nonfinite_f16": int(bad.sum()),
               "subnormal_f16": int((nz & (h < np.float16(2.0 ** -14))).sum()), "lost_f16": int((nz & (aw < 2.0 ** LOST_BITS_EXP)).sum()), "nonzero": int(nz.sum()), "count": int(w.size), "weight_exp": k}
        self.range_report[layer] = row
        if bad.any():
            worst = float(aw[bad].max())
            raise _lib.LecturemathError(_lib.LM_ERR_ARG, "layer %d (%s): BN-folded weight of magnitude %.6g (packed with exponent %d) is finite in fp32 but not in f16 "
                                        "(limit 65,504); use range_guard=\"rescale\" or \"promote\", or precision=\"fp32\"" % (layer, row["name"], worst, k))
        return w

    def _load_planar(self, sd, only=None):
        """recipes of csrc/lm_fcn2.hip (lecturemath_amd/fcn2.py).  only: the layers to repack into the existing engine (calibrate())"""
        from . import fcn2 as f2
        d1, d2, d3, d4, d5, mid, u5, c5, u4, c4, u3, c3, u2, c2, u1, c1, pm1, pm2 = self.widths
        downs = [d1, d2, d3, d4, d5]

        def conv_bn(name):
            w, b = _np(sd[name + ".0.weight"]).astype(np.float32), _np(sd[name + ".0.bias"]).astype(np.float32)
            return fold_bn(w, b, sd, name + ".1", 0)

        def tiles(level):
            return (((self.max_h >> level) + 15) // 16) * (((self.max_w >> level) + 15) // 16)

        T = self.layer_terms

        def V(layer):
            nc, loader = self.variants.get(layer, (1, 0))
            return {"nc": nc, "loader": loader}
        MT = self.DEFAULT_MT.get
        recipes = {}
        R = self._range_weights

        def want(layer):
            return only is None or layer in only
        # every layer aims at fcn2.LDS_TWO_WORKGROUPS of LDS (build's and conv_layer's default): two workgroups per CU
        # encoder: layer 1 reads the input pair plane (3 channels, two horizontal taps per slot)
        if want(L_DOWN):
            w, b = conv_bn("conv_down_block_1")
            w = R(L_DOWN, w, [(f2.T_X0P, 3)])
            pairs = [f2.pairplane_pair(0, dy, dx, 0, 3) for dy in range(3) for dx in (0, 2)]
            recipes[L_DOWN] = (f2.build([w], [{"planes": [(f2.T_X0P, 0)], "pairs": pairs}], 3, 3, T(L_DOWN), MT(L_DOWN) or f2.pick_mt(d1, tiles(0) // V(L_DOWN)["nc"]), f2.EPI_PO, **V(L_DOWN)), b)
        cin = [3] + downs
        for n in range(1, 5):
            if not want(L_DOWN + n):
                continue
            w, b = conv_bn("conv_down_block_%d" % (n + 1))
            w = R(L_DOWN + n, w, [(f2.T_POOL0 + n - 1, cin[n])])
            recipes[L_DOWN + n] = (f2.conv_layer(w, [(f2.T_POOL0 + n - 1, cin[n] // 8)], T(L_DOWN + n), tiles(n), mt=MT(L_DOWN + n), **V(L_DOWN + n)), b)
        if want(L_MID):
            w, b = conv_bn("mid_block")
            w = R(L_MID, w, [(f2.T_POOL0 + 4, d5)])
            recipes[L_MID] = (f2.conv_layer(w, [(f2.T_POOL0 + 4, d5 // 8)], T(L_MID), tiles(5), mt=MT(L_MID), **V(L_MID)), b)
        ups = {5: (mid, u5, c5, d5), 4: (c5, u4, c4, d4), 3: (c4, u3, c3, d3), 2: (c3, u2, c2, d2), 1: (c2, u1, c1, d1)}
        for i, lvl in enumerate((5, 4, 3, 2, 1)):
            tin, u, _, skip = ups[lvl]
            src = f2.T_MID if i == 0 else f2.T_CU0 + i - 1
            if want(L_UPC + i):
                w, b = conv_bn("conv_up_block_%d" % lvl)                                      # input = cat(up, skip_pre)
                w = R(L_UPC + i, w, [(f2.T_UPT0 + i, u), (f2.T_PRE0 + lvl - 1, skip)])
                recipes[L_UPC + i] = (f2.conv_layer(w, [(f2.T_UPT0 + i, u // 8), (f2.T_PRE0 + lvl - 1, skip // 8)], T(L_UPC + i), tiles(lvl - 1), mt=MT(L_UPC + i), **V(L_UPC + i)), b)
            if not want(L_UPT + i):
                continue
            wt = _np(sd["transposed_conv_%d.weight" % lvl]).astype(np.float32)          # [Cin][Cout][2][2]
            bt = _np(sd["transposed_conv_%d.bias" % lvl]).astype(np.float32)
            wt, bt = fold_bn(wt, bt, sd, "upsample_block_%d.0" % lvl, 1)
            wt = R(L_UPT + i, wt, [(src, tin)], axis=0)
            n8 = tin // 8
            co = 8 if n8 % 8 == 0 else (4 if n8 % 4 == 0 else 2)
            chunks = f2.conv_chunks([(src, n8)], 1, 1, co)
            if u % 32 == 0 and not MT(L_UPT + i):
                # both dx of a 32-channel block in one workgroup: per dy a virtual output axis [block][dx][32 channels]
                w2 = []
                for dy in (0, 1):
                    wd = [np.ascontiguousarray(wt[:, :, dy, dx].T) for dx in (0, 1)]             # [u][tin]
                    w2.append(np.concatenate([wd[dx][b * 32:(b + 1) * 32] for b in range(u // 32) for dx in (0, 1)])[:, :, None, None])
                recipes[L_UPT + i] = (f2.build(w2, chunks, 1, 1, T(L_UPT + i), 4, f2.EPI_TC2), bt)
            else:
                w4 = [np.ascontiguousarray(wt[:, :, dy, dx].T)[:, :, None, None] for dy in (0, 1) for dx in (0, 1)]
                recipes[L_UPT + i] = (f2.build(w4, chunks, 1, 1, T(L_UPT + i), MT(L_UPT + i) or f2.pick_mt(u, tiles(lvl)), f2.EPI_TC), bt)
        # heads: the text + reconstruction row convolution is fused with its vertical sums (EPI_V; 56 + 77 -> 93 us: the 133 MB fp32 row buffer
        # is neither written nor read back); the output logit's is not (62 + 20 -> 87 us fused: its tiles of 10 finished rows cost more
        # row-convolution work than its 66 MB of rows; profiles/r04_heads_*.txt).  LM_FCN2_FUSED_HEADS: bit 0 = text / rec, bit 1 = output.
        fused = int(os.environ.get("LM_FCN2_FUSED_HEADS", "1"))
        head_epi, out_epi = (f2.EPI_V if fused & 1 else f2.EPI_T), (f2.EPI_V if fused & 2 else f2.EPI_T)
        if want(L_TEXT):
            wt, bt = conv_bn("conv_text_mask_out")
            wr, br = conv_bn("conv_reconstruct")
            rows = R(L_TEXT, f2.text_rec_rows(wt, wr), [(f2.T_XUP, c1)])
            recipes[L_TEXT] = (f2.build([rows], f2.conv_chunks([(f2.T_XUP, c1 // 8)], 1, 7, c1 // 8), 1, 7, T(L_TEXT), 1, head_epi, **V(L_TEXT)),
                               np.concatenate([np.zeros(16, np.float32), bt, br]))
        # the pixel branch: patch planes single-buffered; feature octets per chunk: two in conv_pixels_1, one in conv_pixels_2, so that
        # the 16 x 32 tile's patch planes of the split format leave room for two workgroups per CU (two octets: 88 KB of LDS, one
        # workgroup, 757 us; one octet: 76 KB, 338 us; 16 x 16 tiles: 364 us)
        if want(L_PX1):
            w, b = conv_bn("conv_pixels_1")
            w = R(L_PX1, w, [(f2.T_DP, 3), (f2.T_XUP, c1)])
            recipes[L_PX1] = (f2.build([w], f2.pixel_chunks(f2.T_XUP, c1 // 8, f2.T_DP, 7, 7, octets=2), 7, 7, T(L_PX1), 2 if pm1 % 32 == 0 else 1, f2.EPI_PO, pdouble=False, **V(L_PX1)), b)
        if want(L_PX2):
            w, b = conv_bn("conv_pixels_2")
            w = R(L_PX2, w, [(f2.T_DP, 3), (f2.T_P1, pm1)])
            recipes[L_PX2] = (f2.build([w], f2.pixel_chunks(f2.T_P1, pm1 // 8, f2.T_DP, 7, 7, octets=1), 7, 7, T(L_PX2), 2 if pm2 % 32 == 0 else 1, f2.EPI_PO, pdouble=False, **V(L_PX2)), b)
        if want(L_OUT):
            w, b = conv_bn("conv_out")
            w = R(L_OUT, w, [(f2.T_DP, 3), (f2.T_P2, pm2)])
            recipes[L_OUT] = (f2.build([f2.out_rows(w)], f2.pixel_chunks(f2.T_P2, pm2 // 8, f2.T_DP, 1, 7), 1, 7, T(L_OUT), 1, out_epi, pdouble=False, **V(L_OUT)),
                              np.concatenate([np.zeros(16, np.float32), b]))
        # a tensor keeps its lo parts when a layer reading it runs the split format
        if only is None:
            lo = np.zeros(f2.N_TENSORS, np.int32)
            for (desc, _, _, _), _ in recipes.values():
                if desc[2] in (2, 3):
                    npl = int(desc[5] * desc[6])
                    lo[desc[13:13 + 2 * npl:2]] = 1
            if self.handle2:
                self.lib.lm_fcn2_destroy(self.handle2)
            arr = (ctypes.c_int32 * 18)(*self.widths)
            self.handle2 = self.lib.lm_fcn2_create(arr, lo.ctypes.data, self.max_h, self.max_w)
            if not self.handle2:
                raise _lib.LecturemathError(_lib.LM_ERR_ARG, self.lib.last_error())
            self.recipes = {}
        for layer, ((desc, wpk, wblocks, need), bias) in recipes.items():
            bias = np.ascontiguousarray(bias, np.float32)
            self.lib.check(self.lib.lm_fcn2_set_layer(self.handle2, layer, desc.ctypes.data, desc.size, wpk.ctypes.data, wpk.nbytes, wblocks,
                                                      bias.ctypes.data, bias.size))
            self.recipes[layer] = {"kh": int(desc[0]), "kw": int(desc[1]), "terms": int(desc[2]), "mt": int(desc[3]), "chunks": int(desc[5]),
                                   "planes_per_chunk": int(desc[6]), "groups": int(desc[7]), "slices": int(desc[8]),
                                   "lds_bytes": int(need), "cout": int(desc[12]), "nc": int(desc[9]) & 15, "loader": (int(desc[9]) >> 8) & 1, "epilogue": int(desc[4]), "first_tensor": int(desc[13]),
                                   "tensors": sorted(set(int(v) for v in desc[13:13 + 2 * int(desc[5] * desc[6]):2]))}
        if self.range_guard != "off":
            self.lib.check(self.lib.lm_fcn2_set_scales(self.handle2, self.tensor_exp.ctypes.data, self.layer_wexp.ctypes.data))

    def executed_gflop(self, h, w):
        """MFMA flops the planar engine EXECUTES for one h x w frame (whole 16 x 16 tiles, whole 32-deep slices, three products per
        operand pair in the split-format layers), as opposed to the network's algorithmic flops"""
        from . import fcn2 as f2
        level_of = {f2.T_X0P: 0, f2.T_MID: 5, f2.T_XUP: 0, f2.T_DP: 0, f2.T_P1: 0, f2.T_P2: 0}
        for n in range(5):
            level_of[f2.T_PRE0 + n] = n
            level_of[f2.T_POOL0 + n] = n + 1
            level_of[f2.T_UPT0 + n] = 4 - n
        for n in range(4):
            level_of[f2.T_CU0 + n] = 4 - n
        total = 0.0
        for r in self.recipes.values():
            lv = level_of[r["first_tensor"]]
            tiles = (((h >> lv) + 15) // 16) * (((w >> lv) + 15) // 16)
            total += 2.0 * tiles * 256 * r["cout"] * r["slices"] * 32 * f2.FORMAT_PRODUCTS[r["terms"]] * (4 if r["epilogue"] == f2.EPI_TC else (2 if r["epilogue"] == f2.EPI_TC2 else 1))
        return total / 1e9

    def load_state_dict(self, sd):
        """sd: the reference's state_dict (torch tensors or numpy arrays).  The engine keeps a reference to it for its lifetime:
        calibrate() repacks layers from it and the fp32 rung reloads it."""
        self._sd = sd
        self.range_report = {}
        self.calibration = None
        self.tensor_exp[:] = 0
        self.layer_wexp[:] = 0
        if self.planar:
            return self._load_planar(sd)
        d1, d2, d3, d4, d5, mid, u5, c5, u4, c4, u3, c3, u2, c2, u1, c1, pm1, pm2 = self.widths
        downs = [d1, d2, d3, d4, d5]

        def conv_bn(name):
            w, b = _np(sd[name + ".0.weight"]).astype(np.float32), _np(sd[name + ".0.bias"]).astype(np.float32)
            return fold_bn(w, b, sd, name + ".1", 0)

        def bias_pad(b):
            out = np.zeros(((len(b) + 31) // 32) * 32, np.float32)
            out[:len(b)] = b
            return out

        def ck_for(*chans):
            return 16 if all(c % 16 == 0 for c in chans) else 8

        h = self.precision != "fp32"
        hck = {"f16x3": 0, "f16x2": -2, "f16": -1}.get(self.precision, 0)       # lm_fcn.hip: products per operand pair

        def mfma(w, cin_map, cin_padded):
            """(packed weights, ck): ck = 0 selects the fp16-split kernel"""
            if h:
                return pack_mfma_h(w, cin_map, sum(cin_padded) if isinstance(cin_padded, tuple) else cin_padded), hck
            ck = ck_for(cin_padded) if not isinstance(cin_padded, tuple) else ck_for(*cin_padded)
            return pack_mfma(w, ck, cin_map, cin_padded if not isinstance(cin_padded, tuple) else sum(cin_padded)), ck

        # encoder + mid (layer 1 sees the 3 RGB channels padded to 8)
        cin = [3] + downs
        for n in range(5):
            w, b = conv_bn("conv_down_block_%d" % (n + 1))
            cpad = 8 if n == 0 else cin[n]
            wpk, ck = mfma(w, range(cin[n]), cpad)
            self._set(L_DOWN + n, wpk, bias_pad(b), cpad, downs[n], self.kk, ck)
        w, b = conv_bn("mid_block")
        wpk, ck = mfma(w, range(d5), d5)
        self._set(L_MID, wpk, bias_pad(b), d5, mid, self.kk, ck)
        # decoder: level 5 .. 1
        ups = {5: (mid, u5, c5, d5), 4: (c5, u4, c4, d4), 3: (c4, u3, c3, d3), 2: (c3, u2, c2, d2), 1: (c2, u1, c1, d1)}
        for i, lvl in enumerate((5, 4, 3, 2, 1)):
            tin, u, c, skip = ups[lvl]
            wt = _np(sd["transposed_conv_%d.weight" % lvl]).astype(np.float32)          # [Cin][Cout][2][2]
            bt = _np(sd["transposed_conv_%d.bias" % lvl]).astype(np.float32)
            wt, bt = fold_bn(wt, bt, sd, "upsample_block_%d.0" % lvl, 1)
            if h:       # one launch: the four (dy, dx) sets are the four "taps" of the packing (lm_k_convT_mfma_h)
                self._set(L_UPT + i, pack_mfma_h(np.ascontiguousarray(wt.transpose(1, 0, 2, 3)), range(tin), tin), bias_pad(bt), tin, u, 1, hck)
            else:
                sets = [mfma(np.ascontiguousarray(wt[:, :, dy, dx].T)[:, :, None, None], range(tin), tin) for dy in (0, 1) for dx in (0, 1)]
                self._set(L_UPT + i, np.concatenate([p for p, _ in sets]), bias_pad(bt), tin, u, 1, sets[0][1])
            w, b = conv_bn("conv_up_block_%d" % lvl)                                      # input = cat(up, skip_pre)
            wpk, ck = mfma(w, range(u + skip), (u, skip))
            self._set(L_UPC + i, wpk, bias_pad(b), u + skip, c, self.kk, ck)
        # heads: inputs are (diff | features | zero pad) buffers
        s0, s1, s2 = _pad8(3 + c1), _pad8(3 + pm1), _pad8(3 + pm2)
        # The fp16-split formats with the shipped kernel sizes (7x7 pixel branch, 3x3 elsewhere) run the heads on the MFMA path
        # (row convolution + vertical sum) and keep x_up1 / diff / pixel features in buffers of their own: a (diff, features)
        # input is the two-input concatenation [d0 d1 d2 0 | features].  Everything else: the round-1 layout, one
        # (diff | features | pad) buffer per stage and VALU kernels for the heads.
        if h and self.pk == 7 and self.kk == 3:
            def head_bias(b):       # [0..31]: zeros for the row convolution's epilogue, [32..]: the bias lm_k_vsum adds
                out = np.zeros(64, np.float32)
                out[32:32 + len(b)] = b
                return out

            def cat_map(nfeat):     # weight input channel -> logical channel of [diff(3) 0 | features]
                return [0, 1, 2] + list(range(4, 4 + nfeat))

            wt, bt = conv_bn("conv_text_mask_out")
            wr, br = conv_bn("conv_reconstruct")
            self._set(L_TEXT, pack_text_rec_rows_h(wt, wr, range(c1), c1), head_bias(np.concatenate([bt, br])), c1, 4, self.pk, hck)
            w, b = conv_bn("conv_pixels_1")
            self._set(L_PX1, pack_mfma_h(w, cat_map(c1), 4 + c1), bias_pad(b), 4 + c1, pm1, self.pk, hck)
            w, b = conv_bn("conv_pixels_2")
            self._set(L_PX2, pack_mfma_h(w, cat_map(pm1), 4 + pm1), bias_pad(b), 4 + pm1, pm2, self.pk, hck)
            w, b = conv_bn("conv_out")
            self._set(L_OUT, pack_rows_h(w, cat_map(pm2), 4 + pm2), head_bias(b), 4 + pm2, 1, self.pk, hck)
            return
        w, b = conv_bn("conv_text_mask_out")
        self._set(L_TEXT, pack_small(w, range(3, 3 + c1), s0), np.pad(b, (0, 4 - len(b))), s0, 1, self.pk, 8)
        w, b = conv_bn("conv_reconstruct")
        self._set(L_REC, pack_small(w, range(3, 3 + c1), s0), np.pad(b, (0, 4 - len(b))), s0, 3, self.kk, 8)
        w, b = conv_bn("conv_pixels_1")
        wpk, ck = (pack_mfma_h(w, range(3 + c1), s0), hck) if h else (pack_mfma(w, 8, range(3 + c1), s0), 8)
        self._set(L_PX1, wpk, bias_pad(b), s0, pm1, self.pk, ck)
        w, b = conv_bn("conv_pixels_2")
        wpk, ck = (pack_mfma_h(w, range(3 + pm1), s1), hck) if h else (pack_mfma(w, 8, range(3 + pm1), s1), 8)
        self._set(L_PX2, wpk, bias_pad(b), s1, pm2, self.pk, ck)
        w, b = conv_bn("conv_out")
        self._set(L_OUT, pack_small(w, range(3 + pm2), s2), np.pad(b, (0, 4 - len(b))), s2, 1, self.pk, 8)

    def set_layer_precision(self, layer, precision):
        """Operand format of ONE layer ("f16x3" / "f16x2" / "f16"); the engine must have been loaded with an fp16-split precision."""
        terms = {"f16x3": 3, "f16x2": 2, "f16": 1}[precision]
        if self.planar:
            raise _lib.LecturemathError(_lib.LM_ERR_STATE, "the planar engine's formats are fixed by load_state_dict (precision=...)")
        self.lib.check(self.lib.lm_fcn_set_layer_terms(self.handle, int(layer), terms))

    # ---- f16 range calibration of the planar engine (constants and their derivation: top of this file)
    TENSOR_NAMES = {0: "x0", 11: "mid", 21: "up1", 22: "diff", 23: "p1", 24: "p2"}
    TENSOR_NAMES.update({1 + n: "down%d_pre" % (n + 1) for n in range(5)})
    TENSOR_NAMES.update({6 + n: "down%d_pool" % (n + 1) for n in range(5)})
    TENSOR_NAMES.update({12 + n: "upsample%d" % (5 - n) for n in range(5)})
    TENSOR_NAMES.update({17 + n: "up%d" % (5 - n) for n in range(4)})
    # tensors in the order the forward pass produces them; a pooled tensor shares the exponent of the tensor it is pooled from
    TENSOR_ORDER = [0, 1, 2, 3, 4, 5, 11, 12, 17, 13, 18, 14, 19, 15, 20, 16, 21, 22, 23, 24]
    FIXED_TENSORS = (0, 22)         # network input and diff: values in [-2, 2] by construction, exponent 0

    def _measure(self, frames):
        """runs the frames and returns the statistics of lm_fcn2_range_stats over all of them: [28][5] float64"""
        tot = None
        for rgb in frames:
            out, text, rec = self.forward(rgb)
            st = np.zeros((28, 5), np.float64)
            self.lib.check(self.lib.lm_fcn2_range_stats(self.handle2, _lib.ptr(out), _lib.ptr(text), _lib.ptr(rec), st.ctypes.data, self.be.stream()))
            if tot is None:
                tot = st
            else:
                with np.errstate(invalid="ignore"):
                    tot[:, 0] = np.where(np.isnan(tot[:, 0]) | np.isnan(st[:, 0]), np.nan, np.maximum(tot[:, 0], st[:, 0]))
                tot[:, 1:] += st[:, 1:]
        return tot

    def _lost(self, st):
        """(tensors holding non-finite values, layers with more than LOST_SHARE of their non-zero weights lost to f16); None when there are none"""
        ts = [t for t in range(25) if st[t, 1] > 0 or not np.isfinite(st[t, 0])]
        ls = [l for l, r in sorted(self.range_report.items()) if r["nonzero"] and r["lost_f16"] / r["nonzero"] > LOST_SHARE]
        if not ts and not ls:
            return None
        return ts, ls

    def _lost_why(self, lost, prefix=""):
        ts, ls = lost
        parts = []
        if ts:
            parts.append("%s hold non-finite values" % ", ".join(self.TENSOR_NAMES[t] for t in ts))
        if ls:
            parts.append("more than 1/8 of the non-zero weights of %s keep fewer than 6 bits in f16" % ", ".join("layer %d (%s)" % (l, self.LAYER_NAMES[l]) for l in ls))
        return prefix + " and ".join(parts)

    def _report(self, st, policy, passes, steps, formats_before):
        from . import fcn2 as f2
        names = {v: k for k, v in f2.FORMAT_NAMES.items()}
        rep = {"policy": policy, "passes": passes, "engine": self.precision, "planar": self.planar, "steps": list(steps),
               "promoted": any(s["rung"] > 1 for s in steps), "tensors": [], "outputs": [], "layers": []}
        if st is not None:
            for t in range(25):
                e = int(self.tensor_exp[t])
                rep["tensors"].append({"tensor": t, "name": self.TENSOR_NAMES[t], "max_abs": float(st[t, 0]) * 2.0 ** e, "stored_max": float(st[t, 0]), "exp": e,
                                       "nonfinite": int(st[t, 1]), "subnormal": int(st[t, 2]), "zero": int(st[t, 3]), "count": int(st[t, 4]),
                                       "all_zero": bool(st[t, 4] > 0 and st[t, 3] == st[t, 4])})
            for i, n in enumerate(("out", "text", "rec")):
                rep["outputs"].append({"name": n, "max_abs": float(st[25 + i, 0]), "nonfinite": int(st[25 + i, 1]), "count": int(st[25 + i, 4])})
        for layer in sorted(formats_before):
            after = names[self.recipes[layer]["terms"]] if self.planar else self.precision
            rep["layers"].append({"layer": layer, "name": self.LAYER_NAMES[layer], "format_before": formats_before[layer], "format_after": after,
                                  "weight_exp": int(self.layer_wexp[layer]) if self.planar else 0})
        self.calibration = rep
        return rep

    def _step(self, steps, rung, what):
        steps.append({"rung": rung, "what": what})
        _log.warning("FCN range calibration, rung %d: %s", rung, what)

    def _rescale(self, frames, steps):
        """rung 1: tensor exponents from the measured maxima, repeated until a pass changes nothing.  Returns (statistics, passes)."""
        zero_steps = {}
        for npass in range(1, MAX_PASSES + 1):
            st = self._measure(frames)
            texp, moved = self.tensor_exp.copy(), []
            for t in self.TENSOR_ORDER:
                m, nonfinite = st[t, 0], st[t, 1] > 0 or not np.isfinite(st[t, 0])
                group = [t, t + 5] if 1 <= t <= 5 else [t]
                if t in self.FIXED_TENSORS:
                    if nonfinite:
                        raise _lib.LecturemathError(_lib.LM_ERR_STATE, "calibrate: tensor %s holds non-finite values and takes no exponent" % self.TENSOR_NAMES[t])
                    continue
                if nonfinite:               # overflowed: true scale unknown, everything after it is unknown too
                    texp[group] += OVERFLOW_STEP
                    moved.append((t, "overflow"))
                    break
                if m == 0:                  # everything reads zero: flushed, or truly zero on these frames.  The same step the other way,
                    if zero_steps.get(t, 0) < ZERO_STEPS:       # a bounded number of times; then the tensor is taken as zero (report: "all_zero")
                        zero_steps[t] = zero_steps.get(t, 0) + 1
                        texp[group] -= OVERFLOW_STEP
                        moved.append((t, "all zero"))
                    continue
                ex = math.floor(math.log2(m))
                if not (TENSOR_BAND[0] <= ex < TENSOR_BAND[1]):
                    texp[group] += ex - TENSOR_TARGET
                    moved.append((t, "max %.3g" % (m * 2.0 ** int(self.tensor_exp[t]))))
            if not moved:
                bad = [n for i, n in enumerate(("out", "text", "rec")) if st[25 + i, 1] > 0]
                if bad:
                    raise _lib.LecturemathError(_lib.LM_ERR_STATE, "calibrate: non-finite values in the fp32 output(s) %s with every tensor finite" % ", ".join(bad))
                return st, npass
            if np.abs(texp).max() > 100:
                raise _lib.LecturemathError(_lib.LM_ERR_STATE, "calibrate: tensor exponents left [-100, 100]")
            changed = [t for t in range(25) if texp[t] != self.tensor_exp[t]]
            self._step(steps, 1, "pass %d: exponents %s" % (npass, ", ".join("%s %+d -> %+d (%s)" % (self.TENSOR_NAMES[t], self.tensor_exp[t], texp[t], why) for t, why in moved)))
            self.tensor_exp[:] = texp
            # repack the layers that read a tensor whose exponent moved (their weights carry its 2^e); producers only need the new scales
            self._load_planar(self._sd, only={l for l, r in self.recipes.items() if set(r["tensors"]) & set(changed)})
        raise _lib.LecturemathError(_lib.LM_ERR_STATE, "calibrate: tensor exponents still moving after %d passes" % MAX_PASSES)

    def calibrate(self, frames, policy=None):
        """Runs `frames` (uint8 [H,W,3] arrays or device tensors, or one of them), reads the range statistics of every activation tensor
        and applies `policy` (default: range_guard; "off" counts as "check"):
          "check"   -- report only; raises when a tensor or an output holds a non-finite value;
          "rescale" -- rung 1: per-tensor / per-layer power-of-two exponents where the measured range leaves the comfort band;
                       raises when that does not bring every tensor into f16's range;
          "promote" -- rung 1; where that is not enough the engine is rebuilt as the first engine with precision="fp32" (rung 3; an
                       f16x3 rung in between is not built: hi + lo adds precision, not range).
        Returns (and keeps as self.calibration) the report: per tensor max |x| in true units, exponent, counts; per layer the format before
        and after; the steps taken; the engine finally in use.  Every step is logged once (logger "lecturemath_amd.fcn")."""
        from . import fcn2 as f2
        policy = policy or self.range_guard
        if policy == "off":
            policy = "check"
        if policy not in RANGE_GUARDS:
            raise _lib.LecturemathError(_lib.LM_ERR_ARG, "calibrate: unknown policy %r" % (policy,))
        if self._sd is None:
            raise _lib.LecturemathError(_lib.LM_ERR_STATE, "FcnEngine.calibrate before load_state_dict")
        if hasattr(frames, "shape") and len(frames.shape) == 3:
            frames = [frames]
        frames = list(frames)
        steps = []
        if not self.planar:             # the first engine keeps fp32 activations: nothing to calibrate
            return self._report(None, policy, 0, steps, {})
        names = {v: k for k, v in f2.FORMAT_NAMES.items()}
        before = {l: names[r["terms"]] for l, r in self.recipes.items()}
        if policy == "check":
            st = self._measure(frames)
            rep = self._report(st, policy, 1, steps, before)
            bad = [r["name"] for r in rep["tensors"] + rep["outputs"] if r["nonfinite"] or not np.isfinite(r["max_abs"])]
            if bad:
                raise _lib.LecturemathError(_lib.LM_ERR_STATE, "calibrate: non-finite values in %s (range_guard=\"rescale\" or \"promote\" can recover them)" % ", ".join(bad))
            return rep
        guard, self.range_guard = self.range_guard, policy      # the weight exponents follow the policy of this call
        try:
            why = None
            try:
                st, passes = self._rescale(frames, steps)
                lost = self._lost(st)
                if lost:
                    why = self._lost_why(lost, "after rescaling, ")
            except _lib.LecturemathError as e:
                if policy == "rescale":
                    raise
                st, passes, why = None, MAX_PASSES, str(e)
            if why is None:
                return self._report(st, policy, passes, steps, before)
            if policy == "rescale":
                self._report(st, policy, passes, steps, before)
                raise _lib.LecturemathError(_lib.LM_ERR_STATE, "calibrate: %s: no per-tensor exponent fits (policy \"promote\" moves on to the fp32 engine)" % why)
            # No f16x3 rung in between: hi + lo of f16x3 adds precision, not range -- the lo part of a value whose hi part is already
            # subnormal or infinite is zero or meaningless -- so no wider planar format can meet the condition that brought us here.
            # rung 3: the first engine on exact fp32 MFMA chains and fp32 activations
            self._step(steps, 3, "%s; rebuilding as the fp32 engine" % why)
            self.lib.lm_fcn2_destroy(self.handle2)
            self.handle2 = None
            self.precision, self.planar = "fp32", False
            self.tensor_exp[:] = 0
            self.layer_wexp[:] = 0
            self._create_first_engine()
            sd = self._sd
            self.load_state_dict(sd)
            for rgb in frames:
                for name, v in zip(("out", "text", "rec"), self.forward(rgb)):
                    if not np.isfinite(self.be.to_host(v)).all():
                        raise _lib.LecturemathError(_lib.LM_ERR_STATE, "calibrate: the fp32 engine's %s holds non-finite values" % name)
            return self._report(None, policy, passes, steps, before)
        finally:
            self.range_guard = guard

    def copy_calibration(self, other):
        """takes over another engine's calibration (same widths, same state dict loaded): exponents, formats and report.  For the
        second engine of a two-stream pipeline; `other` must still be a planar engine."""
        if not (self.planar and other.planar) or self._sd is None:
            raise _lib.LecturemathError(_lib.LM_ERR_STATE, "copy_calibration: both engines must be loaded planar engines")
        self.tensor_exp[:] = other.tensor_exp
        self.layer_wexp[:] = other.layer_wexp
        self.formats = dict(other.formats)
        self._load_planar(self._sd)
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
        out = self.be.empty((h, w), np.float32)
        text = self.be.empty((h, w), np.float32)
        rec = self.be.empty((3, h, w), np.float32)
        self.forward_raw(_lib.ptr(rgb), h, w, _lib.ptr(out), _lib.ptr(text), _lib.ptr(rec))
        return out, text, rec
