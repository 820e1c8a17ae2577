"""The f16 range ladder of the planar FCN engine (FcnEngine.calibrate): load-time check of the packed weights, per-tensor / per-layer
power-of-two exponents from measured maxima (rung 1), promotion to the fp32 engine where no exponent fits (rung 3).  range_weights is
pure; the other steps take the engine, read its lm_fcn2_range_stats and have it repack layers (FcnEngine._load_planar)."""
import logging
import math

import numpy as np

from . import _lib
from .fcn2 import FIXED_TENSORS, FORMAT_NAMES, LAYER_NAMES, N_TENSORS, TENSOR_NAMES, TENSOR_ORDER, exponent_group

RANGE_GUARDS = ("off", "check", "rescale", "promote")

# ---- the band, the target and the ladder's thresholds, in one place.
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

OUTPUTS = ("out", "text", "rec")        # rows N_TENSORS .. N_TENSORS + 2 of lm_fcn2_range_stats
FORMAT_OF = {v: k for k, v in FORMAT_NAMES.items()}
_log = logging.getLogger("lecturemath_amd.fcn")


def range_weights(w, input_exponents, wexp, guard, axis=1):
    """The weights of a layer as they are packed: times 2^e of the tensor feeding each input channel (input_exponents: one per channel along
    `axis`), times 2^-k of the layer -- k = wexp, chosen anew under "rescale" / "promote" when the weights leave WEIGHT_BAND.  All factors
    are powers of two: with every exponent zero the weights come back unchanged.  Returns (packed weights, k, the layer's row of
    range_report without its "layer" and "name")."""
    shape = [1] * w.ndim
    shape[axis] = -1
    w = (w * np.ldexp(np.float32(1), np.asarray(input_exponents, np.int32)).reshape(shape)).astype(np.float32)
    aw = np.abs(w)
    finite = np.isfinite(aw)
    mx = float(aw[finite].max()) if finite.any() else 0.0
    k = int(wexp)
    if guard in ("rescale", "promote") and mx > 0 and not (WEIGHT_BAND[0] <= math.floor(math.log2(mx)) - k < WEIGHT_BAND[1]):
        k = math.floor(math.log2(mx)) - WEIGHT_TARGET
    w = (w * np.float32(2.0 ** -k)).astype(np.float32)
    aw = np.abs(w)
    with np.errstate(over="ignore"):
        h = np.abs(aw.astype(np.float16))
    bad = finite & ~np.isfinite(h)
    nz = aw > 0
    row = {"max_abs": float(aw[finite].max()) if finite.any() else 0.0, "min_nonzero_abs": float(aw[nz].min()) if nz.any() else 0.0, "nonfinite_f16": int(bad.sum()),
           "subnormal_f16": int((nz & (h < np.float16(2.0 ** -14))).sum()), "lost_f16": int((nz & (aw < 2.0 ** LOST_BITS_EXP)).sum()), "nonzero": int(nz.sum()), "count": int(w.size),
           "weight_exp": k}
    return w, k, row


def guarded_weights(eng, layer, w, inputs, axis=1):
    """range_weights for `layer` of the engine (inputs = [(tensor, channels)] along `axis`) under its range_guard: keeps the layer's weight
    exponent and its row of range_report, and raises when a weight that is finite in fp32 is not in f16"""
    if eng.range_guard == "off":
        return w
    exps = np.concatenate([np.full(n, eng.tensor_exp[t], np.int32) for t, n in inputs])
    w, eng.layer_wexp[layer], row = range_weights(w, exps, eng.layer_wexp[layer], eng.range_guard, axis)
    eng.range_report[layer] = row = dict(row, layer=layer, name=LAYER_NAMES[layer])
    if row["nonfinite_f16"]:         # the largest finite weight is one of them
        raise _lib.LecturemathError(_lib.LM_ERR_ARG, "layer %d (%s): BN-folded weight of magnitude %.6g (packed with exponent %d) is finite in fp32 but not in f16 "
                                    "(limit 65,504); use range_guard=\"rescale\" or \"promote\", or precision=\"fp32\"" % (layer, row["name"], row["max_abs"], row["weight_exp"]))
    return w


def measure(eng, frames):
    """runs the frames and returns the statistics of lm_fcn2_range_stats over all of them: [N_TENSORS + 3][5] float64"""
    tot = None
    for rgb in frames:
        out, text, rec = eng.forward(rgb)
        st = np.zeros((N_TENSORS + 3, 5), np.float64)
        eng.lib.check(eng.lib.lm_fcn2_range_stats(eng.handle2, _lib.ptr(out), _lib.ptr(text), _lib.ptr(rec), st.ctypes.data, eng.be.stream()))
        if tot is None:
            tot = st
        else:
            with np.errstate(invalid="ignore"):
                tot[:, 0] = np.where(np.isnan(tot[:, 0]) | np.isnan(st[:, 0]), np.nan, np.maximum(tot[:, 0], st[:, 0]))
            tot[:, 1:] += st[:, 1:]
    return tot


def lost(st, range_report):
    """why rescaling was not enough: tensors holding non-finite values, layers with more than LOST_SHARE of their non-zero weights lost to
    f16; None when there are none"""
    ts = [t for t in range(N_TENSORS) if st[t, 1] > 0 or not np.isfinite(st[t, 0])]
    ls = [l for l, r in sorted(range_report.items()) if r["nonzero"] and r["lost_f16"] / r["nonzero"] > LOST_SHARE]
    parts = []
    if ts:
        parts.append("%s hold non-finite values" % ", ".join(TENSOR_NAMES[t] for t in ts))
    if ls:
        parts.append("more than 1/8 of the non-zero weights of %s keep fewer than 6 bits in f16" % ", ".join("layer %d (%s)" % (l, LAYER_NAMES[l]) for l in ls))
    return "after rescaling, " + " and ".join(parts) if parts else None


def report(eng, st, policy, passes, steps, formats_before):
    rep = {"policy": policy, "passes": passes, "engine": eng.precision, "planar": eng.planar, "steps": list(steps),
           "promoted": any(s["rung"] > 1 for s in steps), "tensors": [], "outputs": [], "layers": []}
    if st is not None:
        for t in range(N_TENSORS):
            e = int(eng.tensor_exp[t])
            rep["tensors"].append({"tensor": t, "name": TENSOR_NAMES[t], "max_abs": float(st[t, 0]) * 2.0 ** e, "stored_max": float(st[t, 0]), "exp": e,
                                   "nonfinite": int(st[t, 1]), "subnormal": int(st[t, 2]), "zero": int(st[t, 3]), "count": int(st[t, 4]),
                                   "all_zero": bool(st[t, 4] > 0 and st[t, 3] == st[t, 4])})
        for i, n in enumerate(OUTPUTS):
            rep["outputs"].append({"name": n, "max_abs": float(st[N_TENSORS + i, 0]), "nonfinite": int(st[N_TENSORS + i, 1]), "count": int(st[N_TENSORS + i, 4])})
    for layer in sorted(formats_before):
        after = FORMAT_OF[eng.recipes[layer]["terms"]] if eng.planar else eng.precision
        rep["layers"].append({"layer": layer, "name": LAYER_NAMES[layer], "format_before": formats_before[layer], "format_after": after,
                              "weight_exp": int(eng.layer_wexp[layer]) if eng.planar else 0})
    eng.calibration = rep
    return rep


def _step(steps, rung, what):
    steps.append({"rung": rung, "what": what})
    _log.warning("FCN range calibration, rung %d: %s", rung, what)


def rescale(eng, frames, steps):
    """rung 1: tensor exponents from the measured maxima, repeated until a pass changes nothing.  Returns (statistics, passes)."""
    zero_steps = {}
    for npass in range(1, MAX_PASSES + 1):
        st = measure(eng, frames)
        texp, moved = eng.tensor_exp.copy(), []
        for t in TENSOR_ORDER:
            m, nonfinite = st[t, 0], st[t, 1] > 0 or not np.isfinite(st[t, 0])
            group = exponent_group(t)
            if t in FIXED_TENSORS:
                if nonfinite:
                    raise _lib.LecturemathError(_lib.LM_ERR_STATE, "calibrate: tensor %s holds non-finite values and takes no exponent" % TENSOR_NAMES[t])
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
                moved.append((t, "max %.3g" % (m * 2.0 ** int(eng.tensor_exp[t]))))
        if not moved:
            bad = [n for i, n in enumerate(OUTPUTS) if st[N_TENSORS + i, 1] > 0]
            if bad:
                raise _lib.LecturemathError(_lib.LM_ERR_STATE, "calibrate: non-finite values in the fp32 output(s) %s with every tensor finite" % ", ".join(bad))
            return st, npass
        if np.abs(texp).max() > 100:
            raise _lib.LecturemathError(_lib.LM_ERR_STATE, "calibrate: tensor exponents left [-100, 100]")
        changed = {t for t in range(N_TENSORS) if texp[t] != eng.tensor_exp[t]}
        _step(steps, 1, "pass %d: exponents %s" % (npass, ", ".join("%s %+d -> %+d (%s)" % (TENSOR_NAMES[t], eng.tensor_exp[t], texp[t], why) for t, why in moved)))
        eng.tensor_exp[:] = texp
        # repack the layers that read a tensor whose exponent moved (their weights carry its 2^e); producers only need the new scales
        eng._load_planar(only={l for l, r in eng.recipes.items() if changed & set(r["tensors"])})
    raise _lib.LecturemathError(_lib.LM_ERR_STATE, "calibrate: tensor exponents still moving after %d passes" % MAX_PASSES)


def calibrate(eng, frames, policy):
    """FcnEngine.calibrate on a loaded engine, policy one of "check" / "rescale" / "promote" """
    steps = []
    if not eng.planar:             # the first engine keeps fp32 activations: nothing to calibrate
        return report(eng, None, policy, 0, steps, {})
    before = {l: FORMAT_OF[r["terms"]] for l, r in eng.recipes.items()}
    if policy == "check":
        rep = report(eng, measure(eng, frames), policy, 1, steps, before)
        bad = [r["name"] for r in rep["tensors"] + rep["outputs"] if r["nonfinite"] or not np.isfinite(r["max_abs"])]
        if bad:
            raise _lib.LecturemathError(_lib.LM_ERR_STATE, "calibrate: non-finite values in %s (range_guard=\"rescale\" or \"promote\" can recover them)" % ", ".join(bad))
        return rep
    guard, eng.range_guard = eng.range_guard, policy      # the weight exponents follow the policy of this call
    try:
        try:
            st, passes = rescale(eng, frames, steps)
            why = lost(st, eng.range_report)
        except _lib.LecturemathError as e:
            if policy == "rescale":
                raise
            st, passes, why = None, MAX_PASSES, str(e)
        if why is None:
            return report(eng, st, policy, passes, steps, before)
        if policy == "rescale":
            report(eng, st, policy, passes, steps, before)
            raise _lib.LecturemathError(_lib.LM_ERR_STATE, "calibrate: %s: no per-tensor exponent fits (policy \"promote\" moves on to the fp32 engine)" % why)
        # No f16x3 rung in between: hi + lo of f16x3 adds precision, not range -- the lo part of a value whose hi part is already
        # subnormal or infinite is zero or meaningless -- so no wider planar format can meet the condition that brought us here.
        # rung 3: the first engine on exact fp32 MFMA chains and fp32 activations
        _step(steps, 3, "%s; rebuilding as the fp32 engine" % why)
        eng._rebuild_as_fp32()
        for rgb in frames:
            for name, v in zip(OUTPUTS, eng.forward(rgb)):
                if not np.isfinite(eng.be.to_host(v)).all():
                    raise _lib.LecturemathError(_lib.LM_ERR_STATE, "calibrate: the fp32 engine's %s holds non-finite values" % name)
        return report(eng, None, policy, passes, steps, before)
    finally:
        eng.range_guard = guard
