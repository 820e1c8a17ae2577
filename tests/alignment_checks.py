"""Checks of the translation alignment on the device (lm_align_* / device.TranslationAligner / the overlay's
AccessMath.preprocessing.content.aligner.Aligner) shared by the CPU tests (emulated library) and the GPU tests.  Everything is
compared exactly: returned tuples against what the reference returned (G21, tests/golden/make_golden_alignment.py), integer match
counts against a numpy brute force written here, all-ink images against the closed form (h - |dy|) (w - |dx|).

What the data exercises (check_not_vacuous computes these from the fixture on the CPU, no library involved; the figures are what
it found when the seeds were fixed): 150 cases, 117 with a non-zero best displacement, 48 in which more than one displacement
attains the maximum of the sort field (the first one in dy, dx order must be returned), 27 in which no displacement matches any
pixel (the reference's f-score is then the int 0), 17 with an image that holds no ink, 33 with 128-valued pixels, 47 whose
window is min(h, w)."""
import os
import struct
import sys
import types

import numpy as np

import dropin_checks
import lm_checks

ZERO = (0.0, 0.0, 0.0, 0, 0)


def overlay():
    if dropin_checks.DROPIN not in sys.path:
        sys.path.insert(0, dropin_checks.DROPIN)
    from AccessMath.preprocessing.content.aligner import Aligner
    return Aligner


def value_of(bits):
    return struct.unpack("<d", struct.pack("<q", int(bits)))[0]


def bits_of(x):
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


# ---- fixture (loaded once, never modified) ------------------------------------------------------------------------------------------
_cache = {}


def g21():
    if "g21" not in _cache:
        g = np.load(os.path.join(lm_checks.GOLD, "g21_alignment.npz"))
        cases = []
        kinds = bytes(g["kinds"]).decode().split(",")
        for k, ((h, w), (window, lum, sort_by)) in enumerate(zip(g["shapes"].tolist(), g["params"].tolist())):
            a = g["first"][g["off"][k]:g["off"][k + 1]].reshape(h, w)
            b = g["second"][g["off"][k]:g["off"][k + 1]].reshape(h, w)
            f, r, p = (value_of(v) for v in g["floats"][k])
            want = (0 if g["f_is_int"][k] else f, r, p, int(g["disp"][k][0]), int(g["disp"][k][1]))
            cases.append(dict(a=a, b=b, window=window, lum=lum, sort_by=sort_by, want=want, kind=kinds[k]))
        _cache["g21"] = (g, cases)
    return _cache["g21"]


def g21_keyframes(name):
    """(planes [n][H][W] uint8 with ink = 0: the keyframes of the stream's three G8 segmentations and the appended image, if
    any; the recorded result of Evaluator.keyframes_alignments(keyframes, 10, 0.3))"""
    if ("kf", name) not in _cache:
        g, _ = g21()
        g8 = np.load(os.path.join(lm_checks.GOLD, "g8_step05_%s.npz" % name))
        w = int(g8["w"])
        planes = [np.unpackbits(g8["keyframes_%d" % k], axis=2)[:, :, :w] * np.uint8(255) for k in range(3)]
        extra = g["kf_extra_" + name]
        if extra.size:
            planes.append((np.unpackbits(extra, axis=1)[None, :, :w] * np.uint8(255)))
        want = []
        for fl, d, rejected in zip(g["kf_floats_" + name], g["kf_disp_" + name].tolist(), g["kf_rejected_" + name]):
            want.append((0, 0, 0, 0, 0) if rejected else tuple(value_of(v) for v in fl) + (d[0], d[1]))
        _cache[("kf", name)] = (np.ascontiguousarray(np.concatenate(planes)), want)
    return _cache[("kf", name)]


def same_tuple(got, want):
    """== and the same types; floats bit for bit"""
    if not (isinstance(got, tuple) and len(got) == 5 and got == want):
        return False
    for a, b in zip(got, want):
        if type(a) is not type(b) or (isinstance(a, float) and bits_of(a) != bits_of(b)):
            return False
    return type(got[3]) is int and type(got[4]) is int


# ---- numpy brute force --------------------------------------------------------------------------------------------------------------
def brute_counts(first_ink, second_ink, window):
    """[dy + w][dx + w] = number of (y, x) with first_ink[y, x] and second_ink[y - dy, x - dx], both inside the image"""
    h, w = first_ink.shape
    pad = np.zeros((h + 2 * window, w + 2 * window), bool)
    pad[window:window + h, window:window + w] = second_ink
    out = np.zeros((2 * window + 1, 2 * window + 1), np.int64)
    for dy in range(-window, window + 1):
        for dx in range(-window, window + 1):
            out[dy + window, dx + window] = np.count_nonzero(first_ink & pad[window - dy:window - dy + h, window - dx:window - dx + w])
    return out


def brute_best(counts, total_first, total_second, sort_by):
    """the tuple of the first displacement (dy, dx ascending) that attains the maximum of field sort_by, in plain Python"""
    if total_first == 0 or total_second == 0:
        return ZERO
    window = (counts.shape[0] - 1) // 2
    best = None
    for dy in range(-window, window + 1):
        for dx in range(-window, window + 1):
            m = int(counts[dy + window, dx + window])
            r, p = m / total_first, m / total_second
            t = ((2 * r * p) / (r + p) if r + p > 0 else 0, r, p, dy, dx)
            if best is None or t[sort_by] > best[sort_by]:
                best = t
    return best


def random_images(n, h, w, seed, density=0.2, values=(255, 0, 128)):
    """uint8 images of `values[0]` (density), values[2] (5 %), else values[1]"""
    rng = np.random.default_rng(seed)
    u = rng.random((n, h, w))
    return np.where(u < density, values[0], np.where(u > 0.95, values[2], values[1])).astype(np.uint8)


# ---- 1. G21 through the overlay -------------------------------------------------------------------------------------------------------
def check_g21_overlay(lib):
    dropin_checks.use_library(lib)
    Aligner = overlay()
    _, cases = g21()
    assert len(cases) >= 140
    for k, c in enumerate(cases):
        got = Aligner.computeTranslationAlignment(c["a"], c["b"], c["window"], c["lum"], c["sort_by"])
        assert same_tuple(got, c["want"]), (k, c["kind"], c["a"].shape, c["window"], c["lum"], c["sort_by"], got, c["want"])
    # the batched form on the cases of one shape gives the same tuples
    by_shape = {}
    for c in cases:
        by_shape.setdefault((c["a"].shape, c["window"], c["lum"], c["sort_by"]), []).append(c)
    key, group = max(by_shape.items(), key=lambda kv: len(kv[1]))
    images = [c["a"] for c in group] + [c["b"] for c in group]
    got = Aligner.computeTranslationAlignments(images, [(i, len(group) + i) for i in range(len(group))], key[1], key[2], key[3])
    assert len(group) >= 2 and all(same_tuple(t, c["want"]) for t, c in zip(got, group)), key


# ---- 2. raw counts against numpy ------------------------------------------------------------------------------------------------------
def check_counts_g21(lib):
    from lecturemath_amd import device
    _, cases = g21()
    handles = {}
    try:
        for k, c in enumerate(cases):
            h, w = c["a"].shape
            if (h, w) not in handles:
                handles[(h, w)] = device.TranslationAligner(w, h, max_images=2, max_window=min(h, w, device.ALIGN_MAX_WINDOW), lib=lib)
            al = handles[(h, w)]
            al.set_images(np.stack([c["a"], c["b"]]), content_lum=c["lum"])
            ink_a, ink_b = c["a"] == c["lum"], c["b"] == c["lum"]
            assert al.totals().tolist() == [int(ink_a.sum()), int(ink_b.sum())], k
            got = al.match_counts([(0, 1)], c["window"])
            assert got.dtype == np.int64 and got.shape == (1, 2 * c["window"] + 1, 2 * c["window"] + 1)
            want = brute_counts(ink_a, ink_b, c["window"])
            assert (got[0] == want).all(), (k, c["a"].shape, c["window"])
            assert same_tuple(al.align([(0, 1)], c["window"], c["sort_by"])[0], c["want"]), k
            assert same_tuple(brute_best(want, int(ink_a.sum()), int(ink_b.sum()), c["sort_by"]), c["want"]), k     # (the test's own scoring)
    finally:
        for al in handles.values():
            al.close()


BATCH_PAIRS = [(0, 1), (1, 0), (2, 2), (0, 5), (5, 0), (3, 4), (4, 4), (1, 3), (5, 2)]


def check_batch(lib, h=70, w=97, window=5):
    """six images, taller than a workgroup's row block (32 rows) and wider than two words, nine pairs in one call: (i, i), and
    (i, j) with (j, i), whose tables mirror each other"""
    from lecturemath_amd import device
    images = random_images(6, h, w, seed=31)
    al = device.TranslationAligner(w, h, max_images=6, max_window=window, lib=lib)
    try:
        al.set_images(images)
        ink = images == 255
        assert al.totals().tolist() == ink.sum(axis=(1, 2)).tolist()
        got = al.match_counts(BATCH_PAIRS, window)
        for k, (i, j) in enumerate(BATCH_PAIRS):
            assert (got[k] == brute_counts(ink[i], ink[j], window)).all(), (i, j)
        assert (got[0] == got[1][::-1, ::-1]).all() and got[2][window, window] == ink[2].sum()
        scores = al.align(BATCH_PAIRS, window, 1)
        totals = al.totals()
        assert all(same_tuple(s, brute_best(got[k], int(totals[i]), int(totals[j]), 1)) for k, ((i, j), s) in enumerate(zip(BATCH_PAIRS, scores)))
        assert al.match_counts([], window).shape == (0, 2 * window + 1, 2 * window + 1) and al.align([], window) == []
    finally:
        al.close()


def check_pixel_stride(lib, h=37, w=70, window=3):
    """channel 0 (and, through the channel argument, 2) of an HWC array whose channels hold different data, read in place"""
    from lecturemath_amd import device
    planes = [random_images(3, h, w, seed=40 + c) for c in range(3)]
    hwc = np.ascontiguousarray(np.stack(planes, axis=3))
    assert hwc.shape == (3, h, w, 3) and (planes[0] != planes[1]).any() and (planes[0] != planes[2]).any()
    al = device.TranslationAligner(w, h, max_images=3, max_window=window, lib=lib)
    try:
        for channel, use in ((None, 0), (0, 0), (2, 2), (1, 1)):
            al.set_images(hwc, channel=channel)
            ink = planes[use] == 255
            assert al.totals().tolist() == ink.sum(axis=(1, 2)).tolist(), channel
            got = al.match_counts([(0, 1), (2, 1)], window)
            assert (got[0] == brute_counts(ink[0], ink[1], window)).all() and (got[1] == brute_counts(ink[2], ink[1], window)).all(), channel
    finally:
        al.close()


def check_device_input(lib, h=40, w=65, window=4):
    """images that already lie in device memory give what host images give (on the emulated build device memory is host memory
    and the flag alone selects the route)"""
    from lecturemath_amd import device
    images = random_images(4, h, w, seed=50, values=(0, 255, 128))
    hwc = np.ascontiguousarray(np.repeat(images[..., None], 3, axis=3))
    hwc[..., 1:] ^= 0x55
    pairs = [(0, 1), (1, 2), (2, 3), (3, 0)]
    al = device.TranslationAligner(w, h, max_images=4, max_window=window, lib=lib)
    try:
        host = al.set_images(images, content_lum=0).match_counts(pairs, window)
        host_totals = al.totals().copy()
        for arr in (images, hwc):
            dev = al.be.from_host(arr)
            al.set_images(dev, content_lum=0, on_device=True)
            assert (al.match_counts(pairs, window) == host).all() and (al.totals() == host_totals).all()
        assert (host[0] == brute_counts(images[0] == 0, images[1] == 0, window)).all()
    finally:
        al.close()


def check_all_ink(lib, h, w, window):
    """matches[dy][dx] == (h - |dy|) (w - |dx|); the best alignment is (1.0, 1.0, 1.0, 0, 0)"""
    from lecturemath_amd import device
    al = device.TranslationAligner(w, h, max_images=2, max_window=window, lib=lib)
    try:
        al.set_images(np.full((2, h, w), 255, np.uint8))
        assert al.totals().tolist() == [h * w, h * w]
        d = np.abs(np.arange(-window, window + 1, dtype=np.int64))
        got = al.match_counts([(0, 1)], window)[0]
        assert (got == np.outer(h - d, w - d)).all()
        assert same_tuple(al.align([(0, 1)], window)[0], (1.0, 1.0, 1.0, 0, 0))
    finally:
        al.close()


def check_empty_in_batch(lib, h=33, w=40, window=3):
    from lecturemath_amd import device
    images = random_images(4, h, w, seed=60)
    images[2] = np.where(images[2] == 255, 128, images[2])      # no ink, but not blank
    al = device.TranslationAligner(w, h, max_images=4, max_window=window, lib=lib)
    try:
        al.set_images(images)
        pairs = [(0, 1), (2, 1), (1, 2), (2, 2), (3, 0)]
        got = al.align(pairs, window)
        ink = images == 255
        assert al.totals().tolist()[2] == 0 and ink[2].sum() == 0
        for (i, j), t in zip(pairs, got):
            if 2 in (i, j):
                assert same_tuple(t, ZERO), (i, j, t)
            else:
                assert t[0] > 0 and same_tuple(t, brute_best(brute_counts(ink[i], ink[j], window), int(ink[i].sum()), int(ink[j].sum()), 0)), (i, j)
        counts = al.match_counts(pairs, window)
        assert (counts[1] == 0).all() and (counts[2] == 0).all() and (counts[3] == 0).all() and counts[0].max() > 0
    finally:
        al.close()


def check_reuse(lib, h=35, w=66, window=2):
    """one handle, two set_images calls of different n_images and content_lum: the second answers for its own images only"""
    from lecturemath_amd import _lib, device
    dense = random_images(5, h, w, seed=70, density=0.6)
    sparse = random_images(2, h, w, seed=71, density=0.05, values=(0, 255, 128))
    al = device.TranslationAligner(w, h, max_images=5, max_window=window, lib=lib)
    try:
        al.set_images(dense)
        first = al.match_counts([(0, 4), (3, 3)], window)
        assert (first[0] == brute_counts(dense[0] == 255, dense[4] == 255, window)).all()
        al.set_images(sparse, content_lum=0)
        ink = sparse == 0
        assert al.n_images == 2 and al.totals().tolist() == ink.sum(axis=(1, 2)).tolist()
        second = al.match_counts([(0, 1), (1, 1)], window)
        assert (second[0] == brute_counts(ink[0], ink[1], window)).all() and (second[1] == brute_counts(ink[1], ink[1], window)).all()
        try:                                    # the images of the first call are gone
            al.match_counts([(0, 4)], window)
        except _lib.LecturemathError as e:
            assert e.code == _lib.LM_ERR_ARG
        else:
            raise AssertionError("a pair outside the second set was accepted")
        al.set_images(dense[:3])                # ... and back, the same content_lum as at first
        assert (al.match_counts([(0, 2)], window)[0] == brute_counts(dense[0] == 255, dense[2] == 255, window)).all()
        al.set_images(np.zeros((0, h, w), np.uint8))
        assert al.n_images == 0 and al.totals().tolist() == [] and al.align([], window) == []
    finally:
        al.close()


# ---- 3. keyframes_alignments parity -----------------------------------------------------------------------------------------------------
def consecutive_alignments(Aligner, planes, window, min_fscore):
    """every keyframe against the next one, ink = 0; an f-score below the threshold means the content changed too much: all zeros"""
    out = []
    for a, b in zip(planes[:-1], planes[1:]):
        t = Aligner.computeTranslationAlignment(a, b, window, 0)
        out.append(t if t[0] >= min_fscore else (0, 0, 0, 0, 0))
    return out


def check_keyframes_parity(lib, name):
    dropin_checks.use_library(lib)
    Aligner = overlay()
    planes, want = g21_keyframes(name)
    assert len(want) == len(planes) - 1 and any(t == (0, 0, 0, 0, 0) and type(t[0]) is int for t in want)
    got = consecutive_alignments(Aligner, planes, 10, 0.3)
    assert len(got) == len(want) and all(same_tuple(a, b) for a, b in zip(got, want)), (name, got, want)
    # the batched form on the same images: the same tuples before the threshold
    batched = Aligner.computeTranslationAlignments(planes, [(i, i + 1) for i in range(len(planes) - 1)], 10, 0)
    for t, w in zip(batched, want):
        assert t[0] < 0.3 if type(w[0]) is int else same_tuple(t, w), (name, t, w)


# ---- 4. argument checks -----------------------------------------------------------------------------------------------------------------
def check_argument_errors(lib):
    from lecturemath_amd import _lib, device
    ARG = _lib.LM_ERR_ARG
    be = device.Backend(lib)
    st = be.stream()

    def refused(handle):
        assert not handle and "lm_align_create" in lib.last_error(), (handle, lib.last_error())

    refused(lib.lm_align_create(0, 8, 2, 1, st))
    refused(lib.lm_align_create(8, 0, 2, 1, st))
    refused(lib.lm_align_create(32769, 8, 2, 1, st))
    refused(lib.lm_align_create(8, 8, 0, 1, st))
    refused(lib.lm_align_create(8, 8, 2, -1, st))
    refused(lib.lm_align_create(8, 8, 2, device.ALIGN_MAX_WINDOW + 1, st))
    assert device.ALIGN_MAX_WINDOW >= 64
    lib.lm_align_destroy(None)
    al = lib.lm_align_create(12, 6, 3, 4, st)
    assert al
    try:
        img = np.full((3, 6, 12), 255, np.uint8)
        totals = np.zeros(3, np.int64)
        pairs = np.asarray([[0, 1], [2, 0]], np.int32)
        out = np.full((3, 9, 9), -7, np.int32)

        def set_images(a=al, i=img, dev=0, n=3, ps=1, lum=255):
            return lib.lm_align_set_images(a, i.ctypes.data if i is not None else None, dev, n, ps, lum, st)

        def run(a=al, p=pairs, n=2, w=4, o=out):
            return lib.lm_align_run(a, p.ctypes.data if p is not None else None, n, w, o.ctypes.data if o is not None else None, st)

        # nothing set yet: every pair is out of range, zero pairs are fine
        assert run() == ARG and "lm_align_run" in lib.last_error()
        assert run(n=0) == _lib.LM_OK and lib.lm_align_totals(al, None, st) == _lib.LM_OK
        for kw in (dict(a=None), dict(i=None), dict(n=-1), dict(ps=0), dict(ps=-3)):
            assert set_images(**kw) == ARG and "lm_align_set_images" in lib.last_error(), kw
        assert set_images(n=4) == _lib.LM_ERR_CAPACITY and "lm_align_set_images" in lib.last_error()
        assert set_images() == _lib.LM_OK
        assert lib.lm_align_totals(al, totals.ctypes.data, st) == _lib.LM_OK and totals.tolist() == [72, 72, 72]
        assert lib.lm_align_totals(None, totals.ctypes.data, st) == ARG and lib.lm_align_totals(al, None, st) == ARG
        assert run() == _lib.LM_OK and out[0, 4, 4] == 72 and out[1, 0, 0] == 2 * 8 and (out[2] == -7).all()
        bad = [dict(a=None), dict(p=None), dict(o=None), dict(n=-1), dict(w=-1),
               dict(w=5),                                               # above the handle's capacity
               dict(p=np.asarray([[0, 3], [2, 0]], np.int32)), dict(p=np.asarray([[0, 1], [-1, 0]], np.int32))]
        for kw in bad:
            assert run(**kw) == ARG and "lm_align_run" in lib.last_error(), kw
        assert (out[2] == -7).all()
        # zero pairs / zero images succeed and write nothing
        assert run(n=0, p=None, o=None) == _lib.LM_OK
        assert set_images(n=0, i=None) == _lib.LM_OK and run(n=0) == _lib.LM_OK and run() == ARG
    finally:
        lib.lm_align_destroy(al)
    # a window above min(width, height), where the reference's slices stop matching: refused although the handle would hold it
    al = lib.lm_align_create(40, 3, 2, 10, st)
    try:
        img = np.zeros((2, 3, 40), np.uint8)
        out = np.zeros((1, 21, 21), np.int32)
        pairs = np.asarray([[0, 1]], np.int32)
        assert lib.lm_align_set_images(al, img.ctypes.data, 0, 2, 1, 255, st) == _lib.LM_OK
        assert lib.lm_align_run(al, pairs.ctypes.data, 1, 3, out.ctypes.data, st) == _lib.LM_OK
        assert lib.lm_align_run(al, pairs.ctypes.data, 1, 4, out.ctypes.data, st) == ARG and "min(width, height)" in lib.last_error()
    finally:
        lib.lm_align_destroy(al)
    # the Python layer
    ta = device.TranslationAligner(12, 6, max_images=2, max_window=2, lib=lib)
    for call in (lambda: ta.set_images(np.zeros((2, 6, 11), np.uint8)), lambda: ta.set_images(np.zeros((2, 6, 12), np.int32)),
                 lambda: ta.set_images(np.zeros((2, 6, 12, 3), np.uint8), channel=3), lambda: ta.set_images(np.zeros((3, 6, 12), np.uint8)),
                 lambda: ta.match_counts([(0, 1)], 3), lambda: ta.match_counts([(0, 1)], -1)):
        try:
            call()
        except (ValueError, _lib.LecturemathError):
            pass
        else:
            raise AssertionError("no exception")
    ta.close()
    for call in (lambda: ta.totals(), lambda: ta.match_counts([], 1), lambda: ta.set_images(np.zeros((2, 6, 12), np.uint8))):
        try:
            call()
        except ValueError:
            pass
        else:
            raise AssertionError("no exception")
    # the overlay: the same assertions as the reference, ValueError naming the limit
    dropin_checks.use_library(lib)
    Aligner = overlay()
    a = np.zeros((6, 300), np.uint8)
    for args, word in (((a, a, 7), "min(height, width) = 6"), ((np.zeros((200, 300), np.uint8),) * 2 + (129,), "limit of 128"), ((a, a, -1), "window")):
        try:
            Aligner.computeTranslationAlignment(*args)
        except ValueError as e:
            assert word in str(e), (word, str(e))
        else:
            raise AssertionError("no ValueError")
    try:
        Aligner.computeTranslationAlignments(np.zeros((2, 6, 300), np.uint8), [(0, 1)], 7)
    except ValueError as e:
        assert "min(height, width) = 6" in str(e)
    else:
        raise AssertionError("no ValueError")
    for args in ((a[0], a, 1), (a, a[0], 1), (a, a[:5], 1)):
        try:
            Aligner.computeTranslationAlignment(*args)
        except AssertionError:
            pass
        else:
            raise RuntimeError("no AssertionError")
    try:
        Aligner.computeVisualAlignment(None, None, 0, [], False, 0)
    except NotImplementedError:
        pass
    else:
        raise AssertionError("no NotImplementedError")
    assert Aligner.ALIGNMENT_SAMPLE == 25 and Aligner.SURF_THRESHOLD == 0.4
    assert Aligner.computeTranslationAlignment(a, a, 6) == ZERO          # window == min(h, w) is accepted; no ink


# ---- 5. vacuity guard (CPU, no library) -------------------------------------------------------------------------------------------------
def vacuity_counts():
    _, cases = g21()
    moved = ties = no_match = empty = 0
    for c in cases:
        ink_a, ink_b = c["a"] == c["lum"], c["b"] == c["lum"]
        if not ink_a.any() or not ink_b.any():
            empty += 1
            continue
        moved += (c["want"][3], c["want"][4]) != (0, 0)
        counts = brute_counts(ink_a, ink_b, c["window"])
        # f-score, recall and precision all grow with the match count: the maximum of either sort field sits where the count does
        ties += int((counts == counts.max()).sum() > 1)
        no_match += int(counts.max() == 0)
    kinds = {c["kind"] for c in cases}
    return dict(cases=len(cases), moved=moved, ties=ties, no_match=no_match, empty=empty, kinds=kinds,
                lums={c["lum"] for c in cases}, sorts={c["sort_by"] for c in cases}, windows={c["window"] for c in cases},
                widths={c["a"].shape[1] for c in cases}, gray=sum(1 for c in cases if (c["a"] == 128).any()),
                full_window=sum(1 for c in cases if c["window"] == min(c["a"].shape)))


def check_not_vacuous():
    c = vacuity_counts()
    assert c["cases"] >= 140 and 3 * c["moved"] >= c["cases"] and c["ties"] >= 10 and c["empty"] >= 1 and c["no_match"] >= 1, c
    assert c["lums"] == {0, 255} and c["sorts"] == {0, 1} and {0, 1, 3, 10} <= c["windows"] and c["full_window"] >= 5, c
    assert {5, 31, 32, 33, 64, 65, 70, 129} <= c["widths"] and c["gray"] >= 10 and c["kinds"] == {"shift", "sparse", "gray", "empty"}, c
    for name in lm_checks.STREAMS:
        planes, want = g21_keyframes(name)
        assert any(type(t[0]) is int for t in want) and any(type(t[0]) is float and t[0] >= 0.3 for t in want), name
    return c


# ---- 6. the reference's Evaluator over the overlay's Aligner (CPU, needs the reference tree) ----------------------------------------------
REFERENCE_CHILD = r"""
import importlib.util, os, struct, sys, types
import numpy as np
sys.dont_write_bytecode = True
tests, root, ref_root, lib_path = %(tests)r, %(root)r, %(ref)r, %(lib)r
sys.path[:0] = [tests, root, os.path.join(tests, "golden", "_ref_shims"), ref_root]
from lecturemath_amd import _lib
_lib._default = _lib.load(lib_path)
# stand-in for a module AccessMath.annotation imports for polygon objects, unused here
sh, geo = types.ModuleType("shapely"), types.ModuleType("shapely.geometry")
geo.Polygon = geo.Point = geo.LineString = type("Unused", (), {})
sh.geometry = geo
sys.modules["shapely"], sys.modules["shapely.geometry"] = sh, geo
# the overlay's module under the name the reference imports (what copying the overlay over the release does to the file)
import AccessMath.preprocessing.content as content
assert os.path.realpath(content.__file__).startswith(os.path.realpath(ref_root))
spec = importlib.util.spec_from_file_location("AccessMath.preprocessing.content.aligner",
                                              os.path.join(root, "lecturemath_amd", "dropin", "AccessMath", "preprocessing", "content", "aligner.py"))
mod = importlib.util.module_from_spec(spec)
sys.modules[spec.name] = mod
spec.loader.exec_module(mod)
content.aligner = mod
from AccessMath.evaluation import evaluator
assert os.path.realpath(evaluator.__file__).startswith(os.path.realpath(ref_root))
assert evaluator.Aligner is mod.Aligner and hasattr(mod.Aligner, "computeTranslationAlignments")
import alignment_checks as ac
n = 0
for name in ac.lm_checks.STREAMS:
    planes, want = ac.g21_keyframes(name)
    frames = [types.SimpleNamespace(binary_image=np.repeat(p[:, :, None], 3, axis=2)) for p in planes]
    got = evaluator.Evaluator.keyframes_alignments(frames, 10, 0.3)
    assert len(got) == len(want) and all(ac.same_tuple(a, b) for a, b in zip(got, want)), (name, got, want)
    n += len(got)
_, cases = ac.g21()
m = 0
for c in cases:
    if c["lum"] == 0 and c["sort_by"] == 1:
        got = evaluator.Evaluator.parallel_keyframe_align((3, 5, c["a"], c["b"], c["window"]))
        assert got[:2] == (3, 5) and ac.same_tuple(got[2], c["want"]), (got, c["want"])
        m += 1
assert m >= 10
print("reference evaluator over the overlay aligner ok:", n, "alignments,", m, "pairs")
"""
