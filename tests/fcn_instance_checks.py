"""Shared bodies of the kernel-instance tests of the planar FCN engine (tests/test_fcn_instances_emulated.py on the CPU emulation,
tests/test_fcn_instances_gpu.py on the device).

lm_k_g2 (csrc/lm_fcn2.hip) is a template over (KH, KW, TERMS, MT, EPI, NC, LOADER); lm_g2_launch holds 69 instantiations, each its own
machine code (register budget, LDS layout, counted waits, loader-wave barriers).  The shipped widths reach 28 of them.  configurations()
below is the table of tiny networks -- widths, per-layer formats, kernel variants, channel tiles, fused-heads bits -- that together run
every one; instances() predicts from fcn2.planar_layers which instance each layer of a configuration runs, and the closure test
(test_fcn_instances_emulated.test_table_reaches_every_instance) holds the union of the table against the dispatcher's list, so an
instance added to lm_g2_launch fails that test until a configuration runs it.

How a layer's instance is chosen (all through the engine's existing knobs):
  3x3 EPI_PO (L_DOWN.., L_MID, L_UPC..)  TERMS: formats[layer]; MT: eng.DEFAULT_MT[layer] (cout a multiple of 16 * MT); (NC, LOADER): eng.variants[layer]
  1x1 transposed (L_UPT..)               MT 1-3: DEFAULT_MT; MT 4: no entry and u % 32 == 0 (the merged EPI_TC2 path, template EPI_TC); TERMS 1 / 3
  1x7 heads (L_TEXT, L_OUT)              TERMS 1-4; NC: variants; EPI_V / EPI_T: LM_FCN2_FUSED_HEADS bit 0 / bit 1 (EPI_V: TERMS 3 / 4 only)
  7x7 (L_PX1, L_PX2)                     MT = 2 when widths[16] / widths[17] is a multiple of 32, else 1; TERMS; (NC, LOADER): variants

check_config compares a configuration's three outputs with oracle.fcn.forward under two bounds:
  every layer f16x3   1e-5 per output, the project's bound for planar-f16x3: a dropped lo product (an f16-level error, 15-300 times
                      larger) is visible;
  any other           3 * e16 per output, e16 = max |oracle16 - oracle| where oracle16 is the same torch forward with the weights and the
                      input of every convolution and transposed convolution rounded to f16 (from the oracle alone); the test also holds
                      3 * e16 <= 5 % of the output's standard deviation, two orders of magnitude below an indexing or staging error;
and then bit for bit with its PLAIN TWINS -- the same network with variants = {} and with one channel tile wherever DEFAULT_MT chooses --
wherever the twin walks K alike in every layer (the same planes, chunks and slices: the same fp32 summation order).  That is the sharp check
of the 35 instances with NC = 2, a loader wave or several channel tiles: no tolerance is involved.

What these tests cannot see: for the a2 and w2 BASE instances (plain variant, one channel tile) a lost lo product changes the error by
less than the 3 * e16 bound resolves; their variants are still held bit for bit against those bases.  The 7x7 instances with two channel
tiles have no one-tile twin (the width decides) and are held by the bounds and, for their variants, by the plain two-tile instance.

Measured, worst over the outputs, the configurations run and their twins (seed 0):
                                             all-f16x3 error   kernel error / e16   3 * e16 / std
  emulator, 33x40 (four configurations)      8.3e-7            0.50 - 1.24          1.3 %
  MI355X, 40x56 and 67x131 (all twelve)      1.4e-6            0.58 - 1.67          1.6 %
and every twin comparison was exact (all twelve configurations have twins that walk K alike, at all three sizes).
Mutations tried on the emulator, each failing test_configuration_vs_oracle_and_twins: row_channel's unpaired tile with rows swapped for
mt = 3 (x1-loader: error 6.6e-2 against a bound of 7.9e-4); the hi.lo product dropped from the 7x7 TERMS = 3 instances (x3-wide: 1.0e-4
against 1e-5).
"""
import collections
import contextlib
import functools

import numpy as np

from lecturemath_amd import _lib, fcn, fcn2, synth
from lecturemath_amd.fcn2 import L_DOWN, L_MID, L_OUT, L_PX1, L_PX2, L_TEXT, L_UPC, L_UPT

F16X3_BOUND = 1e-5          # the project's bound for planar-f16x3 (every layer on hi + lo operands)
E16_FACTOR = 3.0            # any other assignment: 3 * e16 (measured kernel error / e16: 0.2-1.6)
E16_OF_STD = 0.05           # ... and 3 * e16 stays below 5 % of the output's standard deviation
SEED, GLYPHS, GLYPH_SEED = 0, 20, 4
OUTPUTS = ("out", "text", "rec")

LAYERS_3X3 = tuple(range(L_DOWN, L_DOWN + 5)) + (L_MID,) + tuple(range(L_UPC, L_UPC + 5))
LAYERS_1X1 = tuple(range(L_UPT, L_UPT + 5))
LAYERS_HEAD = (L_TEXT, L_OUT)
LAYERS_7X7 = (L_PX1, L_PX2)
ALL_LAYERS = LAYERS_3X3 + LAYERS_1X1 + LAYERS_HEAD + LAYERS_7X7

Config = collections.namedtuple("Config", "name widths formats variants mt fused")
"""widths: the 18 of FcnEngine; formats: {layer: fcn2.FORMAT_NAMES key} of EVERY layer; variants: {layer: (nc, loader)} (eng.variants);
mt: {layer: channel tiles} (eng.DEFAULT_MT) of every 3x3 layer and of every transposed convolution but the merged ones; fused: LM_FCN2_FUSED_HEADS"""


def _config(name, widths, base, fused, layers):
    """layers: {layer: "format mt nc loader"} with "-" = the default (base format, one channel tile -- merged for a transposed convolution
    whose width allows it --, plain variant)"""
    formats, variants, mt = {l: base for l in ALL_LAYERS}, {}, {l: 1 for l in LAYERS_3X3 + LAYERS_1X1}
    for l in LAYERS_3X3 + LAYERS_1X1:       # the families without an instance of the base format run plain f16
        if not fcn2.have_instance(*((3, 3) if l in LAYERS_3X3 else (1, 1)), fcn2.FORMAT_NAMES[base], 1, fcn2.EPI_PO if l in LAYERS_3X3 else fcn2.EPI_TC):
            formats[l] = "f16"
    for l in LAYERS_1X1:
        if widths[6 + 2 * (l - L_UPT)] % 32 == 0:
            del mt[l]                       # no entry: the merged path (EPI_TC2, four channel tiles)
    for l, spec in layers.items():
        f, m, nc, loader = spec.split()
        if f != "-":
            formats[l] = f
        if m != "-":
            assert l in LAYERS_3X3 + LAYERS_1X1, (name, l)
            mt[l] = int(m)
        if (nc, loader) != ("-", "-"):
            variants[l] = (int(nc), int(loader))
    return Config(name, tuple(widths), formats, variants, mt, fused)


#          d1  d2  d3  d4  d5  mid u5  c5  u4  c4  u3  c3  u2  c2  u1  c1  pm1 pm2
W_SMALL = (16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 32, 16)
W_TILES = (48, 16, 32, 16, 64, 64, 32, 64, 48, 32, 32, 48, 16, 32, 16, 16, 32, 16)
W_WIDE0 = (32, 16, 32, 16, 64, 64, 32, 64, 48, 32, 32, 48, 16, 32, 16, 16, 32, 16)


def configurations():
    """the table: at most 16 configurations that together run every instance lm_g2_launch holds"""
    D, M, U, C = L_DOWN, L_MID, L_UPT, L_UPC
    LOADER, WIDE = "- - 1 1", "- - 2 0"            # "format mt nc loader"
    tiles = {U + 1: "- 3 - -", U + 2: "- 2 - -"}            # transposed convolutions of W_TILES: 4 (merged), 3, 2, 1, 1 channel tiles
    return [
        # every layer f16x3 (bound 1e-5): the 20 TERMS = 3 instances
        _config("x3-plain", W_TILES, "f16x3", 3, {**tiles, D: "- 3 - -", D + 2: "- 2 - -", D + 4: "- 4 - -", M: "- 2 - -", C + 2: "- 3 - -", L_OUT: WIDE}),
        _config("x3-loader", W_WIDE0, "f16x3", 0, {**tiles, D: "- 2 2 0", D + 2: "- 2 2 0", D + 4: "- 4 - -", L_TEXT: WIDE, L_PX1: LOADER, L_PX2: LOADER}),
        _config("x3-wide", W_SMALL, "f16x3", 1, {D: WIDE, D + 1: WIDE, D + 3: WIDE, L_TEXT: WIDE, L_PX1: WIDE, L_PX2: WIDE}),
        # f16: the 3x3 family's loader wave on 1-4 tiles, 16 x 32 tiles on 1-3
        _config("x1-plain", W_TILES, "f16", 0, {**tiles, D: "- 3 2 0", D + 2: "- 2 2 0", D + 3: WIDE, D + 4: "- 4 1 1", M: "- 4 - -", C: "- 2 1 1", C + 1: "- 2 - -",
                                                C + 2: "- 3 1 1", C + 3: LOADER, L_OUT: WIDE}),
        _config("x1-loader", W_TILES, "f16", 0, {**tiles, D: "- 3 1 1", D + 2: "- 2 1 1", D + 4: "- 2 2 0", M: "- 4 1 1", C + 2: "- 3 - -", C + 4: LOADER, L_TEXT: WIDE,
                                                L_PX1: LOADER, L_PX2: LOADER}),
        _config("x1-wide", W_SMALL, "f16", 0, {D: WIDE, D + 1: LOADER, D + 2: WIDE, L_PX1: WIDE, L_PX2: WIDE}),
        # w2 (weights hi + lo): 3x3 loader wave and 16 x 32 tiles on 1-2 tiles, both fused heads
        _config("x4-plain", W_TILES, "w2", 3, {**tiles, D: "- 3 - -", D + 2: "- 2 2 0", D + 3: WIDE, D + 4: "- 4 - -", M: "- 2 - -", C + 1: "- 2 1 1", C + 3: LOADER,
                                                L_OUT: WIDE}),
        _config("x4-loader", W_SMALL, "w2", 0, {D: LOADER, D + 1: WIDE, L_TEXT: WIDE, L_PX1: LOADER, L_PX2: LOADER}),
        _config("x4-wide", W_SMALL, "w2", 3, {D: WIDE, D + 2: LOADER, L_TEXT: WIDE, L_PX1: WIDE, L_PX2: WIDE}),
        # a2 (activations hi + lo): heads and 7x7 only; everything else f16
        _config("x2-plain", W_SMALL, "a2", 0, {L_OUT: WIDE}),
        _config("x2-loader", W_SMALL, "a2", 0, {L_TEXT: WIDE, L_PX1: LOADER, L_PX2: LOADER}),
        _config("x2-wide", W_SMALL, "a2", 0, {D + 1: "f16x3 - 2 0", L_PX1: WIDE, L_PX2: WIDE}),
    ]


def zero_folded(widths):
    """{module name: (w, b)} of the right shapes for fcn2.planar_layers (the recipes' structure does not depend on the values)"""
    d, mid, c1, pm1, pm2 = widths[0:5], widths[5], widths[15], widths[16], widths[17]

    def wb(cout, cin, k):
        return np.zeros((cout, cin, k, k), np.float32), np.zeros(cout, np.float32)
    folded = {"conv_down_block_%d" % (n + 1): wb(d[n], 3 if n == 0 else d[n - 1], 3) for n in range(5)}
    folded["mid_block"] = wb(mid, d[4], 3)
    for lvl, tin, u, c, skip in fcn2.decoder_levels(widths):
        folded["transposed_conv_%d" % lvl] = (np.zeros((tin, u, 2, 2), np.float32), np.zeros(u, np.float32))
        folded["conv_up_block_%d" % lvl] = wb(c, u + skip, 3)
    folded.update(conv_text_mask_out=wb(1, c1, 7), conv_reconstruct=wb(3, c1, 3), conv_pixels_1=wb(pm1, 3 + c1, 7), conv_pixels_2=wb(pm2, 3 + pm1, 7),
                  conv_out=wb(1, 3 + pm2, 7))
    return folded


@functools.lru_cache(maxsize=None)
def _recipes(cfg_key, h, w):
    widths, formats, variants, mt, fused = cfg_key
    formats = dict(formats)
    return fcn2.planar_layers(zero_folded(widths), list(widths), h, w, lambda l: fcn2.FORMAT_NAMES[formats[l]], dict(variants), dict(mt), fused_heads=fused)


def recipes(cfg, h=40, w=56):
    """{layer: Recipe} as the engine will build them (fcn2.planar_layers; nothing here depends on the weights)"""
    key = (cfg.widths, tuple(sorted(cfg.formats.items())), tuple(sorted(cfg.variants.items())), tuple(sorted(cfg.mt.items())), cfg.fused)
    return {l: r for l, (r, _) in _recipes(key, h, w).items()}


def instance(r):
    """the lm_g2_launch instance of a Recipe or of its FcnEngine.recipes summary; the merged transposed convolution launches EPI_TC"""
    g = r.get if isinstance(r, dict) else (lambda k: getattr(r, {"epilogue": "epi"}.get(k, k)))
    epi = g("epilogue")
    return (g("kh"), g("kw"), g("terms"), g("mt"), fcn2.EPI_TC if epi == fcn2.EPI_TC2 else epi, g("nc"), g("loader"))


def instances(cfg, h=40, w=56):
    return {l: instance(r) for l, r in recipes(cfg, h, w).items()}


def check_requests_honoured(cfg):
    """what the configuration asks for is what planar_layers builds: fcn2.build's silent fall-backs (nc, loader = 1, 0; EPI_V -> EPI_T) and
    pick_mt would otherwise turn a configuration into a repeat of the plain kernel"""
    inst = instances(cfg)
    assert sorted(inst) == sorted(ALL_LAYERS), cfg.name
    for l, (kh, kw, terms, mt, epi, nc, loader) in inst.items():
        assert terms == fcn2.FORMAT_NAMES[cfg.formats[l]] and (nc, loader) == cfg.variants.get(l, (1, 0)), (cfg.name, l, inst[l])
        if l in LAYERS_3X3 + LAYERS_1X1:
            assert mt == cfg.mt.get(l, 4), (cfg.name, l, inst[l])
        if l in LAYERS_HEAD and terms in (3, 4):
            assert (epi == fcn2.EPI_V) == bool(cfg.fused & (1 if l == L_TEXT else 2)), (cfg.name, l, inst[l])


def walk(cfg, h=40, w=56):
    """{layer: the K walk}: planes, chunks and slices -- what fixes the fp32 summation order of every output value"""
    return {l: (tuple(r.planes), r.nchunks, r.nslices) for l, r in recipes(cfg, h, w).items()}


def twins(cfg):
    """[(label, Config)]: the plain twins that differ from cfg -- variants = {}; one channel tile wherever DEFAULT_MT can choose it"""
    out = []
    if cfg.variants:
        out.append(("plain variants", cfg._replace(name=cfg.name + "/plain", variants={})))
    one = {l: 1 for l in LAYERS_3X3 + LAYERS_1X1}
    if cfg.mt != one:
        out.append(("one channel tile", cfg._replace(name=cfg.name + "/mt1", mt=one)))
    return out


def is_variant(inst):
    return (inst[5], inst[6]) != (1, 0) or inst[3] > 1


def all_f16x3(cfg):
    return all(f == "f16x3" for f in cfg.formats.values())


# ------------------------------------------------------------------------------------------------
# the oracle and its f16 twin
# ------------------------------------------------------------------------------------------------
class _F16Operands:
    """torch.nn.functional with the input and the weights of conv2d / conv_transpose2d rounded to f16 (the arithmetic stays fp32)"""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        return getattr(self._real, name)

    @staticmethod
    def _h(t):
        return t.half().float()

    def conv2d(self, x, w, *a, **kw):
        return self._real.conv2d(self._h(x), self._h(w), *a, **kw)

    def conv_transpose2d(self, x, w, *a, **kw):
        return self._real.conv_transpose2d(self._h(x), self._h(w), *a, **kw)


@contextlib.contextmanager
def _f16_oracle():
    from oracle import fcn as ofcn
    real = ofcn.F
    ofcn.F = _F16Operands(real)
    try:
        yield
    finally:
        ofcn.F = real


@functools.lru_cache(maxsize=None)
def frame(h, w):
    return synth.whiteboard_rgb(h, w, n_glyphs=GLYPHS, seed=GLYPH_SEED)[0]


@functools.lru_cache(maxsize=None)
def state_dict(widths):
    from oracle import fcn as ofcn
    return ofcn.random_state_dict(widths, pixel_kernel=7, seed=SEED)


@functools.lru_cache(maxsize=None)
def reference(widths, h, w):
    """(oracle outputs, e16 per output, std per output), computed once per width set and size and left unchanged"""
    import torch
    from oracle import fcn as ofcn
    sd, x0 = state_dict(widths), ofcn.prepare_image(frame(h, w))
    # frames of a few thousand pixels: a handful of threads.  (Other modules of the suite size torch's pool for 1080p oracles by the host's
    # core count; with that many threads on the cores a test run is allowed, these forwards took 26 s each instead of 0.1 s.)
    threads = torch.get_num_threads()
    torch.set_num_threads(min(threads, 4))
    try:
        with torch.no_grad():
            want = [v.numpy()[0].astype(np.float32) for v in ofcn.forward(sd, x0)]
            with _f16_oracle():
                want16 = [v.numpy()[0] for v in ofcn.forward(sd, x0)]
    finally:
        torch.set_num_threads(threads)
    want = [v[0] if v.shape[0] == 1 else v for v in want]
    want16 = [v[0] if v.shape[0] == 1 else v for v in want16]
    for v in want:
        v.setflags(write=False)
    e16 = [float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(want16, want)]
    std = [float(v.astype(np.float64).std()) for v in want]
    return want, e16, std


# ------------------------------------------------------------------------------------------------
# the checks
# ------------------------------------------------------------------------------------------------
def run(lib, cfg, h, w):
    """one forward pass of cfg's engine -> the three outputs on the host; the engine must run exactly the instances the table predicts"""
    eng = fcn.FcnEngine(cfg.widths, 7, 3, h, w, lib, precision="planar-f16", formats=cfg.formats, range_guard="check")
    try:
        eng.variants = dict(cfg.variants)
        eng.DEFAULT_MT = dict(cfg.mt)
        eng.load_state_dict(state_dict(cfg.widths))
        assert eng.planar
        got, want = {l: instance(r) for l, r in eng.recipes.items()}, instances(cfg, h, w)
        assert got == want, (cfg.name, {l: (got.get(l), want.get(l)) for l in set(got) | set(want) if got.get(l) != want.get(l)})
        outs = [eng.be.to_host(v).copy() for v in eng.forward(frame(h, w).copy())]
    finally:
        eng.close()
    return [o.reshape(r.shape) for o, r in zip(outs, reference(cfg.widths, h, w)[0])]


def check_bounds(cfg, outs, h, w):
    want, e16, std = reference(cfg.widths, h, w)
    split = all_f16x3(cfg)
    for n, o, r, e, s in zip(OUTPUTS, outs, want, e16, std):
        assert np.isfinite(o).all(), (cfg.name, n)
        err = float(np.abs(o.astype(np.float64) - r).max())
        print("FIGURE %s %dx%d %s: error %.3g  e16 %.3g  error/e16 %.3g  3*e16/std %.3g%s" % (cfg.name, h, w, n, err, e, err / e, E16_FACTOR * e / s, "  (all f16x3)" if split else ""))
        assert E16_FACTOR * e <= E16_OF_STD * s, (cfg.name, n, e, s)         # from the oracle alone: if a seed breaks it, change the seed
        if split:
            assert err <= F16X3_BOUND, (cfg.name, n, err)
        else:
            assert err <= E16_FACTOR * e, (cfg.name, n, err, e)


def check_config(lib, cfg, h, w, monkeypatch):
    monkeypatch.setenv("LM_FCN2_FUSED_HEADS", str(cfg.fused))
    monkeypatch.delenv("LM_FCN_RANGE", raising=False)
    outs = run(lib, cfg, h, w)
    check_bounds(cfg, outs, h, w)
    mine = walk(cfg, h, w)
    for label, twin in twins(cfg):
        touts = run(lib, twin, h, w)
        check_bounds(twin, touts, h, w)
        other = walk(twin, h, w)
        if other == mine:           # the same fp32 summation order everywhere: no tolerance
            for n, a, b in zip(OUTPUTS, outs, touts):
                diff = a != b
                assert not diff.any(), "%s at %dx%d: %s differs from the twin with %s in %d values, first at %s, max |difference| %.3g" % (
                    cfg.name, h, w, n, label, int(diff.sum()), tuple(int(v) for v in np.argwhere(diff)[0]), float(np.abs(a.astype(np.float64) - b).max()))
        else:
            print("%s: the twin with %s walks K differently in layers %s: bounds only" % (cfg.name, label, sorted(l for l in mine if mine[l] != other[l])))


REFUSALS = (({6: "w2"}, "no kernel for a 1x1 layer: format 4"), ({2: "a2"}, "no kernel for a 3x3 layer: format 2"), ({5: 7}, "operand formats are 1"))


def check_refusals(lib, h=33, w=40):
    """formats without a kernel instance are refused by load_state_dict, by name; a fresh engine with supported formats then loads and runs"""
    sd = state_dict(W_SMALL)
    for formats, message in REFUSALS:
        eng = fcn.FcnEngine(W_SMALL, 7, 3, h, w, lib, precision="planar-f16", formats=formats)
        try:
            eng.load_state_dict(sd)
        except _lib.LecturemathError as e:
            assert message in str(e), (formats, str(e))
        else:
            raise AssertionError("formats=%r were accepted at load" % (formats,))
        finally:
            eng.close()
    eng = fcn.FcnEngine(W_SMALL, 7, 3, h, w, lib, precision="planar-f16", formats={6: "f16x3", 2: "w2"})
    try:
        eng.load_state_dict(sd)
        outs = [eng.be.to_host(v) for v in eng.forward(frame(h, w))]
        assert all(np.isfinite(o).all() for o in outs)
    finally:
        eng.close()
