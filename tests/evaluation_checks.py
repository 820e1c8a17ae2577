"""Checks of the summary evaluation on the device (lm_kf_pair_counts / device.CCPairCounts / the overlay's
AccessMath.evaluation.evaluator.Evaluator) shared by the CPU tests (emulated library) and the GPU tests.  Everything is compared
exactly: what the overlay returns against what the reference's Evaluator returned (G22, tests/golden/make_golden_evaluation.py),
raw rows and counts against a numpy brute force written here.  The reference's overlap_set order comes from a set of objects and is
arbitrary: group lists are compared as sets of (frozenset of frame-1 ids, frozenset of frame-2 ids), unmatched lists as multisets,
everything else in order.

What the data exercises: fixture_figures() computes it from the fixture on the CPU, no library involved, and check_not_vacuous holds
it against MINIMUMS, which are what the figures were when the seeds were fixed."""
import contextlib
import io
import json
import os
import struct
import sys
import types

import numpy as np

import dropin_checks
import lm_checks

THRESHOLDS = [0.50, 0.65, 0.80, 0.95]


def overlay():
    if dropin_checks.DROPIN not in sys.path:
        sys.path.insert(0, dropin_checks.DROPIN)
    from AccessMath.evaluation.evaluator import Evaluator
    return Evaluator


def cc_class():
    if dropin_checks.DROPIN not in sys.path:
        sys.path.insert(0, dropin_checks.DROPIN)
    from AM_CommonTools.data.connected_component import ConnectedComponent
    return ConnectedComponent


def value_of(bits):
    return struct.unpack("<d", struct.pack("<q", int(bits)))[0]


def bits_of(x):
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


# ---- fixture (loaded once, never modified) ------------------------------------------------------------------------------------------
_cache = {}


def g22():
    if "g" not in _cache:
        g = np.load(os.path.join(lm_checks.GOLD, "g22_evaluation.npz"))
        _cache["g"] = ({k: g[k] for k in g.files}, json.loads(bytes(g["recorded"]).decode()))
    return _cache["g"]


def _ccs_from(box, size, img_off, bits):
    CC = cc_class()
    flat = np.unpackbits(bits)
    out = []
    for k, (b, s) in enumerate(zip(box.tolist(), size.tolist())):
        h, w = b[3] - b[2] + 1, b[1] - b[0] + 1
        img = flat[img_off[k]:img_off[k + 1]].reshape(h, w).astype(np.uint8) * 255
        out.append(CC(k, b[0], b[1], b[2], b[3], s, img))
    return out


def overlaps_background(self, cc):
    """the reference's KeyFrameAnnotation.check_cc_overlaps_background restated: a CC wholly outside the frame counts as background;
    otherwise its mask against the cut of the object mask under its box -- a plain numpy slice, so a negative start wraps around"""
    fh, fw = self.object_mask.shape
    if cc.max_x < 0 or cc.min_x >= fw or cc.max_y < 0 or cc.min_y >= fh:
        return True
    cut = self.object_mask[cc.min_y:cc.max_y + 1, cc.min_x:cc.max_x + 1]
    y0, x0 = max(0, -cc.min_y), max(0, -cc.min_x)
    own = cc.img[y0:y0 + cut.shape[0], x0:x0 + cut.shape[1]]
    return np.count_nonzero(np.logical_and(own, cut)) > 0


def keyframes(prefix):
    """fresh stand-ins of one keyframe set of the fixture: SimpleNamespace(binary_cc, binary_image, object_mask, raw_image, idx)"""
    g, _ = g22()
    h, w = (int(v) for v in g["shape"])
    ccs = _ccs_from(g[prefix + "_cc_box"], g[prefix + "_cc_size"], g[prefix + "_cc_img_off"], g[prefix + "_cc_bits"])
    ink = np.unpackbits(g[prefix + "_ink"], axis=2)[:, :, :w].astype(bool)
    mask = np.unpackbits(g[prefix + "_mask"], axis=2)[:, :, :w].astype(bool)
    out = []
    for k in range(len(ink)):
        plane = np.where(ink[k], 0, 255).astype(np.uint8)
        kf = types.SimpleNamespace(idx=k, binary_image=np.repeat(plane[:, :, None], 3, axis=2), raw_image=np.zeros((h, w, 3), np.uint8),
                                   object_mask=mask[k].copy(), binary_cc=ccs[g[prefix + "_cc_off"][k]:g[prefix + "_cc_off"][k + 1]])
        kf.check_cc_overlaps_background = types.MethodType(overlaps_background, kf)
        out.append(kf)
    return out, [tuple(s) for s in g[prefix + "_segments"].tolist()]


def equiv_cases():
    g, rec = g22()
    ccs = _ccs_from(g["eq_box"], g["eq_size"], g["eq_img_off"], g["eq_bits"])
    out = []
    for k, want in enumerate(rec["equiv"]):
        d = g["eq_disp"][k]
        out.append(dict(cc1=ccs[2 * k], cc2=ccs[2 * k + 1], align=(0.0, 0.0, 0.0, int(d[0]), int(d[1])), window=int(g["eq_window"][k]),
                        min_r=value_of(g["eq_min"][k][0]), min_p=value_of(g["eq_min"][k][1]), want=want))
    return out


def decode(x):
    """the value make_golden_evaluation.encode stored, with its type"""
    if isinstance(x, dict):
        if "b" in x:
            return bool(x["b"])
        if "F" in x:
            return np.float64(value_of(x["F"]))
        if "f" in x:
            return value_of(x["f"])
        if "I" in x:
            return np.int64(x["I"])
        if "t" in x:
            return tuple(decode(v) for v in x["t"])
        return {k: decode(v) for k, v in x["d"]}
    if isinstance(x, list):
        return [decode(v) for v in x]
    return x


def same(got, want, path=""):
    """== and the same kind of type (float / numpy float / int / numpy integer); nan equals nan; dicts in the same key order"""
    if isinstance(want, dict):
        assert isinstance(got, dict) and list(got) == list(want), (path, list(got), list(want))
        for k in want:
            same(got[k], want[k], path + "/" + str(k))
    elif isinstance(want, (list, tuple)):
        assert type(got) is type(want) and len(got) == len(want), (path, got, want)
        for k, (a, b) in enumerate(zip(got, want)):
            same(a, b, path + "[%d]" % k)
    elif isinstance(want, np.floating):
        assert isinstance(got, np.floating) and (got == want or (np.isnan(got) and np.isnan(want))), (path, got, want)
    elif isinstance(want, float):
        assert type(got) is float and (got == want or (got != got and want != want)), (path, got, want)
    elif isinstance(want, np.integer):
        assert isinstance(got, np.integer) and got == want, (path, got, want)
    else:
        assert type(got) is type(want) and got == want, (path, got, want)


def group_key(info_or_ids):
    if isinstance(info_or_ids, list):
        return frozenset(info_or_ids[0]), frozenset(info_or_ids[1])
    return frozenset(cc.strID() for cc in info_or_ids.frame1_ccs_refs), frozenset(cc.strID() for cc in info_or_ids.frame2_ccs_refs)


def same_groups(got, want, what):
    a, b = [group_key(i) for i in got], [group_key(i) for i in want]
    assert len(a) == len(b) and len(set(a)) == len(a) and set(a) == set(b), (what, len(a), len(b))


# ---- numpy brute force --------------------------------------------------------------------------------------------------------------
def box_of(cc):
    return cc.min_x, cc.max_x, cc.min_y, cc.max_y


def brute_pair(a, b, disp, r):
    """(boxes touch for some extra displacement, counts [2r + 1][2r + 1]) of two (box, bool mask) items, B moved by disp: both masks
    on one canvas large enough for every displacement of the window, nothing clipped"""
    (ax0, ax1, ay0, ay1), (bx0, bx1, by0, by1) = a[0], b[0]
    bx0, bx1, by0, by1 = bx0 + disp[1], bx1 + disp[1], by0 + disp[0], by1 + disp[0]
    e = np.arange(-r, r + 1)
    touch = bool(((ax1 >= bx0 + e) & (bx1 + e >= ax0)).any() and ((ay1 >= by0 + e) & (by1 + e >= ay0)).any())
    if not touch:
        return False, None
    ox, oy = min(ax0, bx0 - r) - r, min(ay0, by0 - r) - r            # canvas origin, a margin of r beyond everything
    cw, ch = max(ax1, bx1 + r) + r - ox + 1, max(ay1, by1 + r) + r - oy + 1
    ca, cb = np.zeros((ch, cw), bool), np.zeros((ch + 2 * r, cw + 2 * r), bool)
    ca[ay0 - oy:ay1 - oy + 1, ax0 - ox:ax1 - ox + 1] = a[1]
    cb[by0 - oy + r:by1 - oy + r + 1, bx0 - ox + r:bx1 - ox + r + 1] = b[1]
    out = np.zeros((2 * r + 1, 2 * r + 1), np.int64)
    for ey in range(-r, r + 1):
        for ex in range(-r, r + 1):
            out[ey + r, ex + r] = np.count_nonzero(ca & cb[r - ey:r - ey + ch, r - ex:r - ex + cw])
    return True, out


def brute_query(list_a, list_b, disp, r):
    rows, counts = [], []
    for i, a in enumerate(list_a):
        for j, b in enumerate(list_b):
            touch, c = brute_pair(a, b, disp, r)
            if touch:
                rows.append((i, j))
                counts.append(c)
    return rows, counts


def as_items(ccs):
    return [(box_of(cc), cc.img > 0) for cc in ccs]


def fixture_queries():
    """(A list, B list, (dy, dx)) of (box, mask) items: the consecutive ground-truth keyframes under their recorded alignments, and
    the recorded (gt, summary, alignment) cases"""
    if "queries" not in _cache:
        _, rec = g22()
        gt, _ = keyframes("gt")
        summ, _ = keyframes("summ")
        gi, si = [as_items(k.binary_cc) for k in gt], [as_items(k.binary_cc) for k in summ]
        out = []
        for k, a in enumerate(rec["unique"]["alignments"]):
            a = decode(a)
            out.append((gi[k], gi[k + 1], (int(a[3]), int(a[4]))))
        for p in rec["pairs"]:
            out.append((gi[p["g"]], si[p["s"]], (p["dy"], p["dx"])))
        _cache["queries"] = out
    return _cache["queries"]


def brute_fixture(r):
    if ("brute", r) not in _cache:
        _cache[("brute", r)] = [brute_query(a, b, d, r) for a, b, d in fixture_queries()]
    return _cache[("brute", r)]


# ---- what the fixture exercises -----------------------------------------------------------------------------------------------------
MINIMUMS = {
    "queries": 24, "nonzero_disp_queries": 20, "both_signs": 1, "straddle_32": 85, "straddle_64": 18, "zero_rows": 27,
    "partly_out_top_left": 5, "wholly_out_top_left": 80, "partly_out_bottom_right": 4, "wholly_out_bottom_right": 86, "wrapped_no_overlap": 4,
    "thin_strict_only": 6, "equiv_cases": 27, "equiv_tied": 8, "equiv_true": 12, "equiv_false": 15, "at_threshold": 39,
    "one_one_accepted": 110, "one_one_rejected": 50, "two_one": 32, "one_two": 29, "chain_accepted": 17, "chain_rejected": 12,
    "one_sided_gt": 443, "one_sided_summ": 385, "gt_keyframe_without_ccs": 1, "pair_rejected_by_recall": 1, "lives_3_keyframes": 30,
    "reappears_after_gap": 79,
}


def fixture_figures():
    g, rec = g22()
    gt, _ = keyframes("gt")
    summ, _ = keyframes("summ")
    h, w = (int(v) for v in g["shape"])
    fig = dict.fromkeys(MINIMUMS, 0)
    queries = fixture_queries()
    fig["queries"] = len(queries)
    fig["nonzero_disp_queries"] = sum(1 for _, _, d in queries if d != (0, 0))
    fig["both_signs"] = int(any(d[0] < 0 for _, _, d in queries) and any(d[0] > 0 for _, _, d in queries) and
                            any(d[1] < 0 for _, _, d in queries) and any(d[1] > 0 for _, _, d in queries))
    for kf in gt + summ:
        for cc in kf.binary_cc:
            fig["straddle_32"] += int(cc.min_x // 32 != cc.max_x // 32)
            fig["straddle_64"] += int(cc.min_x // 64 != cc.max_x // 64)
    for rows, counts in brute_fixture(0):
        fig["zero_rows"] += sum(1 for c in counts if not c.any())
    # displaced out of the frame, and the wrapped slice
    for p in rec["pairs"]:
        kf, bg = gt[p["g"]], set(p["bg"])
        for cc in summ[p["s"]].binary_cc:
            x0, x1, y0, y1 = cc.min_x + p["dx"], cc.max_x + p["dx"], cc.min_y + p["dy"], cc.max_y + p["dy"]
            wholly = x1 < 0 or y1 < 0 or x0 >= w or y0 >= h
            if wholly:
                fig["wholly_out_top_left" if (x1 < 0 or y1 < 0) else "wholly_out_bottom_right"] += 1
                continue
            if x0 < 0 or y0 < 0:
                fig["partly_out_top_left"] += 1
                vy, vx = slice(max(y0, 0), min(y1, h - 1) + 1), slice(max(x0, 0), min(x1, w - 1) + 1)
                own = (cc.img > 0)[vy.start - y0:vy.stop - y0, vx.start - x0:vx.stop - x0]
                if np.count_nonzero(own & kf.object_mask[vy, vx]) > 0 and cc.strID() not in bg:
                    fig["wrapped_no_overlap"] += 1
            elif x1 >= w or y1 >= h:
                fig["partly_out_bottom_right"] += 1
    # check_equivalent_cc cases
    cases = equiv_cases()
    fig["equiv_cases"] = len(cases)
    for c in cases:
        fig["equiv_true" if c["want"] else "equiv_false"] += 1
        r, (dy, dx) = c["window"], c["align"][3:]
        touch, counts = brute_pair((box_of(c["cc2"]), c["cc2"].img > 0), (box_of(c["cc1"]), c["cc1"].img > 0), (dy, dx), r)
        scores, strict = [], 0
        for ey in range(-r, r + 1):
            for ex in range(-r, r + 1):
                m, f = c["cc1"], c["cc2"]
                if (m.min_x + dx + ex < f.max_x and f.min_x < m.max_x + dx + ex and m.min_y + dy + ey < f.max_y and f.min_y < m.max_y + dy + ey):
                    strict += 1
                    n = int(counts[ey + r, ex + r])
                    rc, pr = n / m.size, n / f.size
                    scores.append(2 * rc * pr / (rc + pr) if rc + pr > 0 else 0.0)
        if scores and scores.count(max(scores)) > 1 and max(scores) > 0:
            fig["equiv_tied"] += 1
        if touch and strict == 0 and counts.max() > 0 and (c["cc1"].min_x == c["cc1"].max_x or c["cc1"].min_y == c["cc1"].max_y):
            fig["thin_strict_only"] += 1
    # groups and their fate at the first threshold pair; recall or precision equal to a threshold
    sizes = {}
    for kf in gt + summ:
        for cc in kf.binary_cc:
            sizes[cc.strID()] = cc.size
    first = len(rec["unique"]["alignments"])
    for n, p in enumerate(rec["pairs"]):
        rows, counts = brute_fixture(0)[first + n]
        a_ids = [cc.strID() for cc in gt[p["g"]].binary_cc]
        b_ids = [cc.strID() for cc in summ[p["s"]].binary_cc]
        ink = {(a_ids[i], b_ids[j]): int(c[0, 0]) for (i, j), c in zip(rows, counts)}
        accepted = set(group_key(i) for i in p["match"][0]["exact"] + p["match"][0]["partial"])
        for ids in p["groups"]:
            n1, n2 = len(ids[0]), len(ids[1])
            ok = group_key(ids) in accepted
            if n1 == 0:
                fig["one_sided_summ"] += 1
                continue
            if n2 == 0:
                fig["one_sided_gt"] += 1
                continue
            total = sum(ink.get((a, b), 0) for a in ids[0] for b in ids[1])
            rc, pr = total / float(sum(sizes[a] for a in ids[0])), total / float(sum(sizes[b] for b in ids[1]))
            fig["at_threshold"] += int(any(rc == t or pr == t for t in THRESHOLDS))
            if n1 == 1 and n2 == 1:
                fig["one_one_accepted" if ok else "one_one_rejected"] += 1
            elif n1 == 2 and n2 == 1:
                fig["two_one"] += 1
            elif n1 == 1 and n2 == 2:
                fig["one_two"] += 1
            if n1 + n2 >= 4:
                fig["chain_accepted" if ok else "chain_rejected"] += 1
    fig["gt_keyframe_without_ccs"] = sum(1 for kf in gt if not kf.binary_cc)
    fig["pair_rejected_by_recall"] = rec["summary"]["stdout"].count("Recall is to low")
    groups = rec["unique"]["groups"]
    fig["lives_3_keyframes"] = sum(1 for start, ids in groups if len(ids) >= 3)
    masks = {}
    for k, kf in enumerate(gt):
        for cc in kf.binary_cc:
            masks[(k, cc.strID())] = (cc.img.tobytes() + bytes(cc.img.shape), cc.min_x, cc.min_y)
    ended = [(start + len(ids) - 1, masks[(start, ids[0])]) for start, ids in groups]

    def again(start, new):          # the same mask, at most a keyframe's shift away, after at least one keyframe without it
        return any(m[0] == new[0] and abs(m[1] - new[1]) <= 10 and abs(m[2] - new[2]) <= 10 and start > last + 1 for last, m in ended)

    fig["reappears_after_gap"] = sum(1 for start, ids in groups if again(start, masks[(start, ids[0])]))
    return fig


def check_not_vacuous():
    fig = fixture_figures()
    short = {k: (fig[k], MINIMUMS[k]) for k in MINIMUMS if fig[k] < MINIMUMS[k]}
    assert not short, short


# ---- 1. raw rows and counts -----------------------------------------------------------------------------------------------------------
def table_of(lib, lists, w, h, extra=()):
    from lecturemath_amd import device
    return device.CCPairCounts(lists, w, h, extra=extra, lib=lib)


def check_raw_counts(lib):
    """every query of the fixture at radius 0 and 3, one call per radius"""
    g, _ = g22()
    h, w = (int(v) for v in g["shape"])
    queries = fixture_queries()
    lists, index = [], {}
    for a, b, _ in queries:
        for lst in (a, b):
            if id(lst) not in index:
                index[id(lst)] = len(lists)
                lists.append(lst)
    t = table_of(lib, lists, w, h)
    try:
        for r in (0, 3):
            rows, counts = t.counts([(t.items(index[id(a)]), t.items(index[id(b)]), d) for a, b, d in queries], r)
            want = brute_fixture(r)
            want_rows = [(q, i, j) for q, (rw, _) in enumerate(want) for i, j in rw]
            assert [tuple(x) for x in rows.tolist()] == want_rows, (r, len(rows), len(want_rows))
            want_counts = np.asarray([c for _, cs in want for c in cs], np.int64).reshape(-1, 2 * r + 1, 2 * r + 1)
            assert counts.shape == want_counts.shape and (counts == want_counts).all(), (r, np.argwhere(counts != want_counts)[:5])
    finally:
        t.close()


def random_items(rng, n, w, h, max_w=70, max_h=30):
    out = []
    for _ in range(n):
        bw, bh = int(rng.integers(1, max_w + 1)), int(rng.integers(1, max_h + 1))
        x0, y0 = int(rng.integers(0, w - bw + 1)), int(rng.integers(0, h - bh + 1))
        out.append(((x0, x0 + bw - 1, y0, y0 + bh - 1), rng.random((bh, bw)) < 0.5))
    return out


def check_mixed_batch(lib):
    """queries of different list lengths, an empty list on either side, displacements that move everything out of the frame, all
    radii the kernel's slot layout treats differently (1 displacement, 49 < 256, 289 > 256)"""
    rng = np.random.default_rng(8)
    w, h = 200, 90
    lists = [random_items(rng, n, w, h) for n in (7, 1, 12, 3)] + [[((0, w - 1, 0, h - 1), rng.random((h, w)) < 0.3)]]
    t = table_of(lib, lists, w, h)
    plan = [(0, 2, (0, 0)), (1, 0, (4, -9)), (2, None, (1, 1)), (None, 3, (0, 0)), (3, 3, (-2, 2)), (4, 0, (3, -5)), (2, 4, (-30, 60)),
            (0, 1, (-300, 500)), (4, 4, (1, -1))]
    try:
        for r in (0, 1, 3, 8):
            queries = [([] if a is None else t.items(a), [] if b is None else t.items(b), d) for a, b, d in plan]
            rows, counts = t.counts(queries, r)
            want_rows, want_counts = [], []
            for q, (a, b, d) in enumerate(plan):
                rw, cs = brute_query([] if a is None else lists[a], [] if b is None else lists[b], d, r)
                want_rows += [(q, i, j) for i, j in rw]
                want_counts += cs
            assert [tuple(x) for x in rows.tolist()] == want_rows, r
            assert (counts == np.asarray(want_counts, np.int64).reshape(-1, 2 * r + 1, 2 * r + 1)).all(), r
    finally:
        t.close()


# ---- 2. the overlay against the recorded results -----------------------------------------------------------------------------------------
def check_equivalent(lib):
    dropin_checks.use_library(lib)
    Evaluator = overlay()
    for k, c in enumerate(equiv_cases()):
        before = box_of(c["cc1"])
        got = Evaluator.check_equivalent_cc(c["cc1"], c["cc2"], c["align"], c["window"], c["min_r"], c["min_p"])
        assert type(got) is bool and got == c["want"] and box_of(c["cc1"]) == before, (k, got, c["want"])


def check_unique(lib):
    dropin_checks.use_library(lib)
    Evaluator = overlay()
    _, rec = g22()
    gt, _ = keyframes("gt")
    want_align = [decode(a) for a in rec["unique"]["alignments"]]
    aligns = Evaluator.keyframes_alignments(gt, 10, 0.3)
    same(aligns, want_align, "alignments")
    groups, cc_group = Evaluator.keyframes_unique_cc(gt, aligns, 3, 0.5, 0.5)
    assert [[g.start_frame, [cc.strID() for cc in g.cc_refs]] for g in groups] == rec["unique"]["groups"]
    got = [[[cc.strID(), cc_group[k][cc.strID()].strID()] for cc in kf.binary_cc] for k, kf in enumerate(gt)]
    assert got == rec["unique"]["cc_groups"]
    assert [list(d) for d in cc_group] == [[cc.strID() for cc in kf.binary_cc] for kf in gt]
    return groups, cc_group


def check_pairs(lib):
    dropin_checks.use_library(lib)
    from lecturemath_amd import device
    Evaluator = overlay()
    _, rec = g22()
    gt, _ = keyframes("gt")
    summ, _ = keyframes("summ")
    for n, p in enumerate(rec["pairs"]):
        align = (0.0, 0.0, 0.0, p["dy"], p["dx"])
        overlap_set = Evaluator.keyframes_overlapping_ccs(gt[p["g"]].binary_cc, summ[p["s"]].binary_cc, align)
        same_groups(overlap_set, p["groups"], ("groups", n))
        made = []
        real = device.CCPairCounts.__init__

        def counting(self, *a, **kw):
            made.append(self)
            return real(self, *a, **kw)

        device.CCPairCounts.__init__ = counting
        try:
            for k, (min_r, min_p) in enumerate(zip(THRESHOLDS, THRESHOLDS)):
                exact, partial, un1, un2 = Evaluator.match_overlapping_ccs(overlap_set, align, min_r, min_p)
                want = p["match"][k]
                same_groups(exact, want["exact"], ("exact", n, k))
                same_groups(partial, want["partial"], ("partial", n, k))
                assert sorted(cc.strID() for cc in un1) == want["un1"] and sorted(cc.strID() for cc in un2) == want["un2"], (n, k)
        finally:
            device.CCPairCounts.__init__ = real
        assert not made, "match_overlapping_ccs built a device table although the groups carry their counts"
        before = [box_of(cc) for cc in summ[p["s"]].binary_cc]
        assert Evaluator.find_ccs_overlapping_background(gt[p["g"]], summ[p["s"]], align, False) == p["bg"], ("bg", n)
        assert [box_of(cc) for cc in summ[p["s"]].binary_cc] == before
    # groups that carry no counts (built elsewhere): match_overlapping_ccs fetches them in one call, with the same result
    p = rec["pairs"][0]
    align = (0.0, 0.0, 0.0, p["dy"], p["dx"])
    overlap_set = Evaluator.keyframes_overlapping_ccs(gt[p["g"]].binary_cc, summ[p["s"]].binary_cc, align)
    for info in overlap_set:
        info.pair_ink = None
    exact, partial, un1, un2 = Evaluator.match_overlapping_ccs(overlap_set, align, 0.5, 0.5)
    same_groups(exact, p["match"][0]["exact"], "refetched exact")
    same_groups(partial, p["match"][0]["partial"], "refetched partial")


def check_summary(lib):
    dropin_checks.use_library(lib)
    Evaluator = overlay()
    _, rec = g22()
    gt, gt_segments = keyframes("gt")
    summ, summ_segments = keyframes("summ")
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        all_overlapping, bg = Evaluator.summary_overlapping_ccs(gt_segments, gt, summ_segments, summ, 10, 0.05, True)
    want = rec["summary"]
    assert buf.getvalue() == want["stdout"]
    assert [x[:2] for x in all_overlapping] == [tuple(x[:2]) for x in want["all"]]
    for got, w in zip(all_overlapping, want["all"]):
        same(got[2], decode(w[2]), "align")
        same_groups(got[3], w[3], got[:2])
    assert [[[k, v] for k, v in d.items()] for d in bg] == want["bg"]
    # the metrics, from the recorded ground-truth groups rebuilt on these stand-ins
    by_id = [{cc.strID(): cc for cc in kf.binary_cc} for kf in gt]
    from AccessMath.evaluation.evaluator import UniqueCCGroup
    groups, cc_group = [], [dict.fromkeys(d) for d in by_id]
    for start, ids in rec["unique"]["groups"]:
        grp = UniqueCCGroup(by_id[start][ids[0]], start)
        for off, cc_id in enumerate(ids):
            if off:
                grp.cc_refs.append(by_id[start + off][cc_id])
            cc_group[start + off][cc_id] = grp
        groups.append(grp)
    metrics, names = Evaluator.compute_summary_metrics(gt_segments, gt, groups, cc_group, summ_segments, summ)
    assert names == rec["range_names"]
    same(metrics, decode(rec["metrics"]), "metrics")
    for name in names:
        for fn in ("print_summary_recall_metrics", "print_summary_precision_metrics", "print_compact_CC_metrics"):
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                getattr(Evaluator, fn)(metrics[name], name)
            assert buf.getvalue() == rec["prints"][fn + "|" + name], (fn, name)


def check_pixel_metrics():
    Evaluator = overlay()
    _, rec = g22()
    gt, _ = keyframes("gt")
    summ, _ = keyframes("summ")
    with np.errstate(all="ignore"):
        same(Evaluator.compute_pixel_binary_metrics(gt, summ[:len(gt)]), decode(rec["pixel"]), "pixel")
        same(Evaluator.compute_pixel_binary_metrics(gt[:4], summ[:4]), decode(rec["pixel_nonempty"]), "pixel_nonempty")


# ---- 3. the handle ----------------------------------------------------------------------------------------------------------------------
def check_reuse(lib):
    """a large query, a small one, the large one again: equal results, no stale counts in the kept scratch"""
    rng = np.random.default_rng(4)
    w, h = 160, 100
    lists = [random_items(rng, 40, w, h), random_items(rng, 40, w, h), random_items(rng, 2, w, h)]
    t = table_of(lib, lists, w, h)
    try:
        large = [(t.items(0), t.items(1), (2, -3)), (t.items(1), t.items(0), (-1, 1))]
        small = [(t.items(2), t.items(2), (0, 0))]
        r1, c1 = t.counts(large, 3)
        rs, cs = t.counts(small, 3)
        r2, c2 = t.counts(large, 3)
        assert len(r1) > 50 and (r1 == r2).all() and (c1 == c2).all()
        rw, cw = brute_query(lists[2], lists[2], (0, 0), 3)
        assert [tuple(x[1:]) for x in rs.tolist()] == rw and (cs == np.asarray(cw)).all()
        r0, c0 = t.counts(large, 0)         # a smaller count table in the same scratch: the centre of the radius-3 table
        centre = {tuple(row): int(c[3, 3]) for row, c in zip(r1.tolist(), c1)}
        assert 0 < len(r0) <= len(r1) and [int(c[0, 0]) for c in c0] == [centre[tuple(row)] for row in r0.tolist()]
    finally:
        t.close()


def check_argument_errors(lib):
    import pytest
    from lecturemath_amd import _lib
    rng = np.random.default_rng(5)
    w, h = 64, 48
    lists = [random_items(rng, 6, w, h, 20, 20), random_items(rng, 6, w, h, 20, 20)]
    t = table_of(lib, lists, w, h)
    try:
        q = [(t.items(0), t.items(1), (0, 0))]
        with pytest.raises(_lib.LecturemathError, match="radius"):
            t.counts(q, 9)
        with pytest.raises(_lib.LecturemathError, match="radius"):
            t.counts(q, -1)
        with pytest.raises(_lib.LecturemathError, match="item outside"):
            t.counts([([0, 12], [1], (0, 0))], 0)
        with pytest.raises(_lib.LecturemathError, match="item outside"):
            t.counts([([0], [-1], (0, 0))], 0)
        with pytest.raises(_lib.LecturemathError, match="displacement"):
            t.counts([([0], [1], (0, 32769))], 0)
        with pytest.raises(_lib.LecturemathError, match="displacement"):
            t.counts([([0], [1], (-32769, 0))], 0)
        rows, counts = t.counts([([0], [1], (32768, -32768))], 8)      # the limit itself is served: nothing touches
        assert len(rows) == 0 and counts.shape == (0, 17, 17)
        rows, counts = t.counts([], 3)
        assert rows.shape == (0, 3) and counts.shape == (0, 7, 7)
        # too small a cap reports the needed size; CCPairCounts.counts retries once with it
        want_rows, _ = t.counts(q, 3)
        a_off, b_off = np.asarray([0, 6], np.int64), np.asarray([0, 6], np.int64)
        a, b = t.items(0), t.items(1)
        disp, found = np.zeros(2, np.int32), np.zeros(1, np.int64)
        rows1, counts1 = np.zeros((1, 3), np.int32), np.zeros((1, 7, 7), np.int32)
        rc = lib.lm_kf_pair_counts(t.handle, a_off.ctypes.data, a.ctypes.data, b_off.ctypes.data, b.ctypes.data, disp.ctypes.data, 1, 3,
                                   rows1.ctypes.data, counts1.ctypes.data, 1, found.ctypes.data, None)
        assert len(want_rows) > 1 and rc == _lib.LM_ERR_CAPACITY and int(found[0]) == len(want_rows) and "room for 1" in lib.last_error()
        calls = t.calls
        rows2, _ = t.counts(q, 3, cap=1)
        assert t.calls == calls + 2 and (rows2 == want_rows).all()
    finally:
        t.close()
    with pytest.raises(ValueError):
        t.counts([], 0)


# ---- 4. GPU-sized cases (a few seconds each on the device; far too slow for the emulator) ------------------------------------------------
def check_all_ink(lib, h, w, r):
    """an all-ink h x w item against itself: counts[ey][ex] = (h - |ey|) (w - |ex|) -- counter width and the row-block split"""
    t = table_of(lib, [[((0, w - 1, 0, h - 1), np.ones((h, w), bool))]], w, h)
    try:
        rows, counts = t.counts([([0], [0], (0, 0))], r)
    finally:
        t.close()
    e = np.abs(np.arange(-r, r + 1, dtype=np.int64))
    assert rows.tolist() == [[0, 0, 0]] and (counts[0] == np.outer(h - e, w - e)).all()


def check_glyph_grid(lib, rows_n=40, cols_n=50, r=0):
    """rows_n x cols_n glyph-sized items against a jittered copy: the join's grid, the capacity retry, counts against the brute force
    (restricted by a cell test to the pairs that can touch)"""
    rng = np.random.default_rng(6)
    pitch_x, pitch_y = 38, 27
    w, h = cols_n * pitch_x + 48, rows_n * pitch_y + 26      # room for the widest glyph and the jitter in the last cells
    a, b = [], []
    for gy in range(rows_n):
        for gx in range(cols_n):
            for out, jit in ((a, 0), (b, 4)):
                bw, bh = int(rng.integers(8, 45)), int(rng.integers(8, 22))
                x0 = gx * pitch_x + int(rng.integers(0, jit + 1))
                y0 = gy * pitch_y + int(rng.integers(0, jit + 1))
                out.append(((x0, x0 + bw - 1, y0, y0 + bh - 1), rng.random((bh, bw)) < 0.5))
    t = table_of(lib, [a, b], w, h)
    try:
        calls = t.calls
        rows, counts = t.counts([(t.items(0), t.items(1), (1, -2))], r, cap=len(a) // 2)
        retried = t.calls - calls
    finally:
        t.close()
    want_rows, want_counts = [], []
    for i, item in enumerate(a):
        gy, gx = divmod(i, cols_n)
        for ny in range(max(gy - 2, 0), min(gy + 3, rows_n)):
            for nx in range(max(gx - 2, 0), min(gx + 3, cols_n)):
                j = ny * cols_n + nx
                touch, c = brute_pair(item, b[j], (1, -2), r)
                if touch:
                    want_rows.append((0, i, j))
                    want_counts.append(c)
    assert len(want_rows) > len(a) and retried == 2
    assert [tuple(x) for x in rows.tolist()] == want_rows
    assert (counts == np.asarray(want_counts, np.int64)).all()


# ---- 5. keyframes of a G8 stream: the device route against the host loop -------------------------------------------------------------------
def host_equivalent(moving, fixed, align, window, min_recall, min_precision):
    """check_equivalent_cc as a host loop over the overlay's ConnectedComponent.getOverlapFMeasure, pair by pair and displacement by
    displacement: what an evaluation costs without lm_kf_pair_counts"""
    best = None
    for loc_y in range(-window, window + 1):
        for loc_x in range(-window, window + 1):
            dx, dy = align[4] + loc_x, align[3] + loc_y
            moving.translateBox(dx, dy)
            if moving.min_x < fixed.max_x and fixed.min_x < moving.max_x and moving.min_y < fixed.max_y and fixed.min_y < moving.max_y:
                recall, precision = moving.getOverlapFMeasure(fixed, False, False)
                fscore = (2.0 * recall * precision) / (recall + precision) if recall + precision > 0.0 else 0.0
                if best is None or fscore > best[0]:
                    best = (fscore, recall, precision)
            moving.translateBox(-dx, -dy)
    return best is not None and best[1] >= min_recall and best[2] >= min_precision


def host_unique_groups(keyframe_set, alignments, window, min_recall, min_precision):
    """the greedy assignment with host_equivalent: per keyframe the group number of every CC, groups numbered as they appear"""
    n_groups = len(keyframe_set[0].binary_cc)
    member = [list(range(n_groups))]
    active = [(g, cc) for g, cc in enumerate(keyframe_set[0].binary_cc)]
    for k in range(1, len(keyframe_set)):
        pending, active, row = active, [], []
        for cc in keyframe_set[k].binary_cc:
            hit = next((s for s, (_, last) in enumerate(pending)
                        if host_equivalent(cc, last, alignments[k - 1], window, min_recall, min_precision)), None)
            if hit is None:
                g, n_groups = n_groups, n_groups + 1
            else:
                g = pending.pop(hit)[0]
            row.append(g)
            active.append((g, cc))
        member.append(row)
    return member


def check_g8_unique(lib, name="occluder_return"):
    """keyframes rendered by GenerateFromGroupImages on a G8 stream, labelled through the overlay's Labeler: keyframes_unique_cc gives
    the groups of the host loop"""
    import keyframe_checks as kc
    dropin_checks.use_library(lib)
    Evaluator = overlay()
    from AccessMath.preprocessing.content.labeler import Labeler
    KE = kc.extractor()
    spec, ages, bounds, images = kc.g4_structure(name)
    g = kc.g8(name)
    times = [1000.0 * i for i in range(int(g["n_frames"]))]
    gi, item_first = kc.from_host(lib, ages, images, bounds, spec["w"], spec["h"])
    try:
        dev, _ = KE.GenerateFromGroupImages(gi, item_first, ages, bounds, times, spec["h"], spec["w"], g["segments"][0], verbose=False,
                                            device_frames=True)
    finally:
        gi.close()
    planes = dev.cpu().numpy() if hasattr(dev, "cpu") else np.asarray(dev)
    kfs = [types.SimpleNamespace(idx=k, binary_image=p, raw_image=p, binary_cc=Labeler.extractConnectedComponents(255 - p[:, :, 0]))
           for k, p in enumerate(planes)]
    assert len(kfs) >= 3 and sum(len(k.binary_cc) for k in kfs) >= 10
    aligns = Evaluator.keyframes_alignments(kfs, 10, 0.3)
    groups, cc_group = Evaluator.keyframes_unique_cc(kfs, aligns, 3, 0.5, 0.5)
    number = {id(grp): n for n, grp in enumerate(groups)}
    got = [[number[id(cc_group[k][cc.strID()])] for cc in kf.binary_cc] for k, kf in enumerate(kfs)]
    assert got == host_unique_groups(kfs, aligns, 3, 0.5, 0.5)
    assert any(len(grp.cc_refs) >= 2 for grp in groups)
