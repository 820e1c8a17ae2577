"""Steps 02-03 under configuration values other than the shipped ones, against the oracle; shared by the CPU tests (emulated
library) and the GPU tests.  Everything is compared exactly: oracle.cc.Stability for step 02, oracle.grouping.run_step03 for step 03.

The streams are built here with numpy so that every swept parameter decides something in them; check_sweep_stream_not_vacuous,
check_step02_stream_not_vacuous and check_min_pixels_stream_not_vacuous assert that from the oracle's own output (no library
involved), so a stream that stops exercising a parameter fails there.

What sweep_stream holds, for the step-03 parameters:
  * two piles of shapes that share a core block and are drawn one per frame with unequal frequencies, so the members of one group
    have unequal counts inside a segment: the "tie" pile (counts 1, 5, 10, 14 of 30: pixels with v / max == 0.2, 1/3, 0.5 exactly)
    and the "near" pile (2, 7, 18, 12, 14 of 53: pixels strictly between every two adjacent swept thresholds);
  * the member with count 10 of the tie pile has an arm over a box of 2 x 2 tiles of 64 px: three tiles that only its box touches (10 / 30: the 1/3 tie
    again), the group's maximum in the fourth; a blinking square of its own group lies inside that box, so at thresholds <= 0 (boxes filled) the
    reconstructed frames hold wrapped sums;
  * two pairs of overlapping shapes whose lifetimes lie 3 and 5 frames apart (t_window);
  * pairs seen in alternate frames with recall / precision (0.5, 0.2), (0.2, 1/3), (0.2, 0.2), (1.0, 0.4), (0.2, 0.4) (min_recall);
  * squares seen 2, 3, 4 and 8 times with gaps of 2, 3 and 4 frames (max_gap, min_times).

The step-03 stream (sweep_stream) has 62 frames, not the ~40 of the other small streams: a pixel with 1/3 < v / max < 0.34 needs
max >= 53 and one with 0.5 < v / max < 0.51 needs max >= 51, and members of one group that overlap are seen one per frame (two in one
frame would be one component), so max cannot exceed the number of frames of the segment.

Left out because the reference itself is undefined there: min_times = 1.  A unique with a single sighting is then stable, its
group's age list has one entry, compute_group_images makes no image for it and frames_from_groups reads ages[g][1] (IndexError).
img_threshold = NaN and min_recall = NaN are rejected by lm_group_run (check_nan_rejected) and have no oracle run either."""
import copy
import math

import numpy as np

import dropin_checks
import lm_checks
from lecturemath_amd import _lib, device

H, W = 128, 320
N_FRAMES = 62
DEFAULTS = dict(max_gap=85, min_times=3, t_window=5, min_recall=0.5, img_threshold=0.5)

IMG_THRESHOLDS = [-0.5, 0.0, 0.05, 0.2, 0.25, 1 / 3, 0.34, 0.5, 0.51, 0.9, 1.0, 1.5]
TIE_THRESHOLDS = [0.2, 1 / 3, 0.5]
T_WINDOW_GAPS = (3, 5)          # first sighting of the later shape - last sighting of the earlier one, for the two pairs
T_WINDOWS = [0, 2, 3, 4, 5, 6, 1000]
MIN_RECALLS = [0.0, 1 / 3, math.nextafter(1 / 3, 1.0), 0.5, 1.0]
MAX_GAPS = [1, 2, 3, 4, 85]
MIN_TIMES = [2, 3, 6]
MIXED = [dict(min_recall=0.0),                                                   # the 03 script's own default
         dict(min_recall=0.0, img_threshold=0.2, t_window=3, max_gap=2, min_times=2),
         dict(min_recall=1 / 3, img_threshold=1 / 3, t_window=4, max_gap=3, min_times=6),
         dict(min_recall=1.0, img_threshold=0.0, t_window=0, max_gap=1, min_times=2),
         dict(min_recall=math.nextafter(1 / 3, 1.0), img_threshold=0.9, t_window=1000, max_gap=4, min_times=3),
         dict(min_recall=0.0, img_threshold=-0.5, t_window=6, max_gap=85, min_times=6)]

STEP02_THRESHOLDS = [(0.5, 0.9), (0.9, 0.3), (0.3, 0.3), (0.85, 0.85)]
STEP02_GAPS = [0, 1, 3]
MIN_PIXELS = [1, 20, 25, 26]


def params(**kw):
    return dict(DEFAULTS, **kw)


def axis_points():
    """(id, parameter sets) of the one-axis-at-a-time sweep around the shipped defaults and of the mixed points, four runs to a case."""
    out = []
    for name, values in (("img_threshold", IMG_THRESHOLDS), ("t_window", T_WINDOWS), ("min_recall", MIN_RECALLS),
                         ("max_gap", MAX_GAPS), ("min_times", MIN_TIMES), ("mixed", MIXED)):
        points = [params(**v) if name == "mixed" else params(**{name: v}) for v in values]
        for k in range(0, len(points), 4):
            out.append(("%s-%d" % (name, k // 4), points[k:k + 4]))
    return out


# ---- the step-03 stream ------------------------------------------------------------------------------------------------------------
def _spread(counts):
    """Member indices, counts[i] times member i, interleaved evenly (A B B / A B B B B like, with unequal periods)."""
    return [i for _, i in sorted(((j + 0.5) / c, i) for i, c in enumerate(counts) for j in range(c))]


def _pile_members(core, bar_len, membership, arm=None):
    """Masks of the members of a pile: all share a core block (core = (rows, cols)) at the left; region s is a 2-row bar to the
    right of the core at rows 3 s .. 3 s + 1, drawn for the members listed in membership[s].  arm = (member, right, down) lets one
    member's own bar run `right` pixels to the right and then `down` pixels downwards: a box of several 64 x 64 tiles."""
    ch, cw = core
    n = 1 + max(m for mem in membership for m in mem)
    hh = max(ch, 3 * len(membership)) + (arm[2] if arm else 0)
    ww = cw + max(bar_len, arm[1] if arm else 0)
    masks = np.zeros((n, hh, ww), bool)
    masks[:, :ch, :cw] = True
    for s, mem in enumerate(membership):
        for m in mem:
            if arm and arm[0] == m and len(mem) == 1:
                masks[m, 3 * s:3 * s + 2, cw:cw + arm[1]] = True
                masks[m, 3 * s:3 * s + arm[2], cw + arm[1] - 2:cw + arm[1]] = True
            else:
                masks[m, 3 * s:3 * s + 2, cw:cw + bar_len] = True
    return masks


def _pile_schedule(mid_counts):
    """Which member is drawn in which frame.  Member 0 is seen in frames 0 and 1, members 1.. first in frames 2.., and the last
    sightings come in member order at the end; the segment between the last first sighting and the first last sighting then holds
    member i exactly mid_counts[i] times (member 0's last sighting and the last member's first one are inside it)."""
    k = len(mid_counts)
    inner = list(mid_counts)
    inner[0] -= 1
    inner[k - 1] -= 1
    return [0, 0] + list(range(1, k)) + _spread(inner) + list(range(k))


TIE_COUNTS = [1, 5, 10, 14]             # of 30: 6 = 1 + 5 (0.2), 10 (1/3), 15 = 5 + 10 (0.5)
NEAR_COUNTS = [2, 7, 18, 12, 14]        # of 53: 18 (0.3396), 27 = 2 + 7 + 18 (0.5094), 51 = 53 - 2 (0.962), ...
TIE_AT, NEAR_AT = (4, 4), (4, 140)      # (y, x) of the two piles


def _tie_pile():
    # regions: {0, 1}, {1, 2}, {2} = the arm (110 px to the right, 84 px down: a box of 2 x 2 tiles whose tiles other than the first only
    # member 2's box touches; its count there is 10 of 30, the 1/3 tie), {3}
    return _pile_members((12, 12), 24, [[0, 1], [1, 2], [2], [3]], arm=(2, 110, 84)), _pile_schedule(TIE_COUNTS)


def _near_pile():
    return (_pile_members((27, 10), 30, [[0], [1], [2], [3], [4], [0, 1, 2], [1, 3], [2, 3], [1, 2, 3, 4]]),
            _pile_schedule(NEAR_COUNTS))


_cache = {}


def sweep_stream():
    """The step-03 stream: 62 frames of 128 x 320 (the module docstring lists what is in it).  Cached; never modified."""
    if "sweep" in _cache:
        return _cache["sweep"]
    frames = np.zeros((N_FRAMES, H, W), np.uint8)

    def put(f, y, x, mask):
        frames[f, y:y + mask.shape[0], x:x + mask.shape[1]][mask] = 255

    def rect(f, y, x, h, w):
        frames[f, y:y + h, x:x + w] = 255

    for (masks, sched), (y, x) in ((_tie_pile(), TIE_AT), (_near_pile(), NEAR_AT)):
        assert len(sched) <= N_FRAMES
        for f, m in enumerate(sched):
            put(f, y, x, masks[m])
    for f in range(N_FRAMES):
        # a group of its own inside the empty corner of the tie pile's box, alive with it (f % 7: it blinks, so its unique has gaps too)
        if f % 7 != 6:
            rect(f, 50, 30, 10, 10)
        # recall pairs at y = 100, alternating frames: recall / precision of (first, second) = (0.5, 0.2), (0.2, 1/3), (0.2, 0.2), (1.0, 0.4),
        # (0.2, 0.4)
        if f % 2 == 0:
            rect(f, 100, 180, 10, 10)
            rect(f, 100, 100, 4, 10)        # 40 px, 20 shared
            rect(f, 100, 120, 10, 10)       # 100 px, 20 shared
            rect(f, 100, 140, 10, 10)
            rect(f, 100, 160, 4, 10)        # inside its partner
        else:
            rect(f, 102, 100, 10, 10)
            rect(f, 108, 120, 6, 10)        # 60 px
            rect(f, 108, 140, 10, 10)
            rect(f, 100, 160, 10, 10)
            rect(f, 108, 180, 5, 10)        # 50 px, 20 shared
    # temporal-window pairs at y = 100: 12 x 10 shapes, the later one 4 px to the right (80 of 120 px shared), first seen d frames after
    # the earlier one's last sighting
    for x, d in zip((10, 50), T_WINDOW_GAPS):
        for f in range(0, 10):
            rect(f, 100, x, 10, 12)
        for f in range(9 + d, 9 + d + 7):
            rect(f, 100, x + 4, 10, 12)
    # lifetime gaps at y = 118, across the render-tile border at x = 256: 2, 3 and 8 sightings with gaps of 2, 3 and 4 frames, and
    # two whose largest gaps are 3 and 2
    for x, seen in ((244, (3, 5)), (252, (2, 5, 9)), (260, (0, 1, 3, 4, 7, 8, 12, 13)), (268, (0, 1, 4, 5)),
                    (276, (20, 22, 23))):
        for f in seen:
            rect(f, 118, x, 5, 5)
    _cache["sweep"] = frames
    return frames


# ---- oracle runs (cached, never modified) ----------------------------------------------------------------------------------------
def oracle_stream(key, frames, thresholds=(0.85, 0.85), gap2=85, min_pixels=20):
    k = ("state", key, thresholds, gap2, min_pixels)
    if k not in _cache:
        from oracle import cc as occ
        st = occ.Stability(frames[0].shape[1], frames[0].shape[0], thresholds[0], thresholds[1], gap2)
        for f in frames:
            st.add_frame(f, min_pixels)
        _cache[k] = st.result()
    return _cache[k]


def oracle_step03(key, frames, p, reconstruct=True):
    """run_step03 of a fresh copy of the stream's step-02 state; the post-split lists of that copy are added to the dict."""
    k = ("step03", key, tuple(sorted(p.items())), reconstruct)
    if k not in _cache:
        from oracle import grouping as og
        state = copy.deepcopy(oracle_stream(key, frames))
        o = og.run_step03(state, reconstruct=reconstruct, **p)
        o["unique_cc_frames"], o["cc_idx_per_frame"], o["unique_recs"] = state["unique_cc_frames"], state["cc_idx_per_frame"], state["unique_recs"]
        o["unique_crops"] = state["unique_crops"]
        _cache[k] = o
    return _cache[k]


def grouping_equal_oracle(r, o, frame_sums=None):
    """Everything lm_checks.grouping_equal_golden compares, against oracle_step03's dict; exact everywhere.  o["clean_binary"] None:
    the run was made without the frames."""
    assert r["n_split"] == o["n_split"]
    assert r["unique_cc_frames"] == o["unique_cc_frames"]
    assert r["cc_idx_per_frame"] == o["cc_idx_per_frame"]
    assert r["stable_idxs"] == list(o["stable_idxs"])
    assert r["total_intersections"] == o["total_intersections"]

    def tflat(lists):
        return np.asarray([(a, b, np.float64(rc).view(np.int64), np.float64(p).view(np.int64))
                           for a, lst in enumerate(lists) for b, rc, p in lst], np.int64).reshape(-1, 4)
    got, exp = tflat(r["time_overlapping_cc"]), tflat(o["time_overlapping_cc"])
    assert got.shape == exp.shape and (got == exp).all()
    assert len(r["all_overlapping_cc"]) == len(o["all_overlapping_cc"])
    assert [[tuple(int(v) for v in t) for t in lst] for lst in r["all_overlapping_cc"]] == \
           [[tuple(int(v) for v in t) for t in lst] for lst in o["all_overlapping_cc"]]
    assert r["cc_groups"] == o["cc_groups"]
    assert r["group_idx_per_cc"] == o["group_idx_per_cc"]
    ng = len(o["cc_groups"])
    assert sorted(r["group_ages"]) == sorted(o["group_ages"]) == list(range(ng))
    assert [list(r["group_ages"][k]) for k in range(ng)] == [list(o["group_ages"][k]) for k in range(ng)]
    assert [list(fr) for fr in r["groups_per_frame"]] == [list(fr) for fr in o["groups_per_frame"]]

    def cflat(c):
        return sorted((k, other, float(d["matched"]), float(d["unmatched"]), float(d["area_union"]), float(d["area_intersection"]))
                      for k in c for other, d in c[k].items())
    assert sorted(r["conflicts"]) == sorted(o["conflicts"]) and cflat(r["conflicts"]) == cflat(o["conflicts"])
    assert {k: tuple(v) for k, v in r["group_boundaries"].items()} == {k: tuple(v) for k, v in o["group_boundaries"].items()}
    for k in range(ng):
        assert len(r["group_images"][k]) == len(o["group_images"][k]), k
        for a, b in zip(r["group_images"][k], o["group_images"][k]):
            assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all(), k
    if o["clean_binary"] is not None:
        got, exp = np.stack(r["clean_binary"]), np.stack(o["clean_binary"])
        assert got.dtype == exp.dtype and got.shape == exp.shape and (got == exp).all()
        if frame_sums is not None:
            assert frame_sums.dtype == np.int64 and list(frame_sums) == [int(f.astype(np.int64).sum()) for f in exp]
    else:
        assert "clean_binary" not in r


def sweep_frame_stream(lib):
    """The step-03 stream after step 02 on `lib` (checked against the oracle): ONE device.FrameStream per library for all the runs
    of the sweep, which is also how the stream's device arena comes to be re-used by run after run."""
    k = ("fs", id(lib))
    if k not in _cache:
        frames = sweep_stream()
        fs = device.FrameStream(W, H, len(frames), 0.85, 0.85, 85, 20, max_batch=16, lib=lib)
        try:
            fs.push(fs.be.from_host(frames))
            lm_checks.state_equal_oracle(fs.result(), oracle_stream("sweep", frames))
        except BaseException:
            fs.close()
            raise
        _cache[k] = fs
    return _cache[k]


def run_groupings(lib, points, reconstruct=True):
    """One device.Grouping per parameter set on the shared FrameStream, each compared with the oracle in full."""
    frames = sweep_stream()
    fs = sweep_frame_stream(lib)
    for p in points:
        o = oracle_step03("sweep", frames, p, reconstruct)
        gr = device.Grouping(fs, reconstruct=reconstruct, **p)
        try:
            r = gr.result(with_clean=reconstruct)
            sums = gr.frame_sums(0, len(frames)) if reconstruct else None
        finally:
            gr.close()
        try:
            grouping_equal_oracle(r, o, sums)
        except AssertionError as e:
            raise AssertionError("step 03 differs from the oracle at %r" % (p,)) from e


def check_sweep_axis(lib, axis, reconstruct=True):
    points = dict(axis_points())[axis]
    run_groupings(lib, points, reconstruct)


def check_two_runs_alive(lib):
    """Two runs of one stream alive at the same time (the second cannot have the stream's arena) and a third after both closed."""
    frames = sweep_stream()
    pa, pb = params(img_threshold=0.2, t_window=3), params(min_recall=0.0, img_threshold=0.0, min_times=2)
    fs = sweep_frame_stream(lib)
    ga = device.Grouping(fs, **pa)
    try:
        gb = device.Grouping(fs, **pb)
        try:
            rb, ra = gb.result(), ga.result()
            sa, sb = ga.frame_sums(0, len(frames)), gb.frame_sums(0, len(frames))
        finally:
            gb.close()
    finally:
        ga.close()
    grouping_equal_oracle(ra, oracle_step03("sweep", frames, pa), sa)
    grouping_equal_oracle(rb, oracle_step03("sweep", frames, pb), sb)
    gc = device.Grouping(fs, **pb)
    try:
        grouping_equal_oracle(gc.result(), oracle_step03("sweep", frames, pb), gc.frame_sums(0, len(frames)))
    finally:
        gc.close()


# ---- what the step-03 stream exercises, from the oracle alone ----------------------------------------------------------------------
def accumulated(o):
    """[(group, segment, x0, y0, [(member, times)], acc)] -- the member masks of every segment of every group summed with numpy, as
    compute_group_images sums them (oracle.grouping.group_images), from the oracle run's post-split lists."""
    recs, crops, frames = o["unique_recs"], o["unique_crops"], o["unique_cc_frames"]
    out = []
    for g, members in enumerate(o["cc_groups"]):
        x0, x1, y0, y1 = o["group_boundaries"][g]
        ages = o["group_ages"][g]
        for s, (t0, t1) in enumerate(zip(ages[:-1], ages[1:])):
            acc = np.zeros((y1 - y0 + 1, x1 - x0 + 1), np.int64)
            times = []
            for u in members:
                n = sum(1 for f, _ in frames[u] if t0 <= f <= t1)
                if n:
                    c = crops[u]
                    acc[int(recs[u, 2]) - y0:int(recs[u, 2]) - y0 + c.shape[0], int(recs[u, 0]) - x0:int(recs[u, 0]) - x0 + c.shape[1]] += (c // 255) * n
                    times.append((u, n))
            out.append((g, s, x0, y0, times, acc))
    return out


def check_sweep_stream_not_vacuous():
    frames = sweep_stream()
    assert frames.shape == (N_FRAMES, H, W)
    state = oracle_stream("sweep", frames)
    o = oracle_step03("sweep", frames, params())
    acc = accumulated(o)
    # the numpy sums reproduce the oracle's images at the shipped threshold
    for g, s, _, _, _, a in acc:
        assert ((a.astype(np.float64) / a.max() >= 0.5).astype(np.uint8) * 255 == o["group_images"][g][s]).all()
    # -- unequal member counts inside one segment
    assert any(len({n for _, n in times}) >= 3 for _, _, _, _, times, _ in acc)
    pairs = set()
    for _, _, _, _, _, a in acc:
        mx = int(a.max())
        pairs.update((int(v), mx) for v in np.unique(a))
    ratio = sorted({np.float64(v) / np.float64(mx) for v, mx in pairs})
    # -- exact ties: v / max == thr in float64, for a pixel that is neither empty nor the maximum
    for thr in TIE_THRESHOLDS:
        assert any(0 < v < mx and np.float64(v) / np.float64(mx) == thr for v, mx in pairs), thr
    # -- near misses: a pixel strictly between every adjacent pair of swept thresholds (v / max lies in [0, 1]: nothing can lie below 0,
    # and strictly between -0.5 and 0.0 or between 1.0 and 1.5 there is nothing either)
    for lo, hi in zip(IMG_THRESHOLDS[:-1], IMG_THRESHOLDS[1:]):
        if lo >= 0.0 and hi <= 1.0:
            assert any(lo < q < hi for q in ratio), (lo, hi)
            # ... so the oracle's images differ between the two
            a, b = (oracle_step03("sweep", frames, params(img_threshold=t))["group_images"] for t in (lo, hi))
            assert any((x != y).any() for k in a for x, y in zip(a[k], b[k])), (lo, hi)
    # -- a group of several tiles with a tile that only one member's box touches, its maximum in another tile
    recs = o["unique_recs"]
    found = tie = False
    for g, s, x0, y0, times, a in acc:
        hh, ww = a.shape
        if hh <= 64 or ww <= 64 or len(times) < 2:
            continue
        my, mxx = np.unravel_index(int(np.argmax(a)), a.shape)
        assert (a == a.max()).sum() == (a[:64, :64] == a.max()).sum()       # every maximum pixel lies in the first tile
        for ty in range((hh + 63) // 64):
            for tx in range((ww + 63) // 64):
                X0, Y0 = x0 + 64 * tx, y0 + 64 * ty
                touching = [u for u, _ in times if recs[u, 0] <= X0 + 63 and recs[u, 1] >= X0 and recs[u, 2] <= Y0 + 63 and recs[u, 3] >= Y0]
                tile = a[64 * ty:64 * ty + 64, 64 * tx:64 * tx + 64]
                if len(touching) == 1 and (ty, tx) != (my // 64, mxx // 64) and tile.any():
                    n = dict(times)[touching[0]]
                    # the member's count passes some swept thresholds and misses others
                    if any(n / a.max() >= t for t in IMG_THRESHOLDS if t > 0) and any(n / a.max() < t for t in IMG_THRESHOLDS if t <= 1):
                        found = True
                    # ... and sits exactly on one of them
                    tie = tie or np.float64(n) / np.float64(a.max()) in TIE_THRESHOLDS
    assert found and tie
    # -- non-positive thresholds fill the boxes; boxes of groups alive together overlap: sums other than 0 and 255
    for thr in (0.0, -0.5):
        clean = np.stack(oracle_step03("sweep", frames, params(img_threshold=thr))["clean_binary"])
        assert set(np.unique(clean).tolist()) - {0, 255}, thr
    # -- temporal window: each pair joins when t_window reaches its gap
    for d in T_WINDOW_GAPS:
        a, b, c = (oracle_step03("sweep", frames, params(t_window=t)) for t in (d - 1, d, d + 1))
        assert a["total_intersections"] + 1 == b["total_intersections"] == c["total_intersections"], d
        assert a["cc_groups"] != b["cc_groups"] and b["cc_groups"] == c["cc_groups"], d
    assert {d - 1 for d in T_WINDOW_GAPS} | set(T_WINDOW_GAPS) | {d + 1 for d in T_WINDOW_GAPS} <= set(T_WINDOWS)
    # -- recall ties, recall != precision
    tov = [(rc, p) for lst in o["time_overlapping_cc"] for _, rc, p in lst]
    assert any(rc == 0.5 and p not in (0.5, rc) for rc, p in tov) and any(rc == 1 / 3 and p != rc for rc, p in tov)
    assert any(rc == 1.0 and p < 0.5 for rc, p in tov)
    # both orders: the smaller side of a pair first seen earlier (lower unique index) and later
    low_first = [(u, b) for u, lst in enumerate(o["time_overlapping_cc"]) for b, rc, p in lst if u < b and rc > p]
    low_second = [(u, b) for u, lst in enumerate(o["time_overlapping_cc"]) for b, rc, p in lst if u < b and rc < p]
    assert low_first and low_second
    groups = [oracle_step03("sweep", frames, params(min_recall=m))["cc_groups"] for m in MIN_RECALLS]
    assert all(a != b for a, b in zip(groups[:-1], groups[1:]))
    # -- lifetime gaps and sightings
    gaps, seen = set(), set()
    for fl in state["unique_cc_frames"]:
        seen.add(len(fl))
        gaps.update(b[0] - a[0] for a, b in zip(fl[:-1], fl[1:]))
    assert {2, 3, 4} <= gaps and {2, 3} <= seen and any(n >= 6 for n in seen) and any(3 < n < 6 for n in seen)
    by_gap = [oracle_step03("sweep", frames, params(max_gap=m)) for m in MAX_GAPS]
    n_split = [x["n_split"] for x in by_gap]
    assert all(a > b for a, b in zip(n_split[:-1], n_split[1:])), n_split
    assert all(a["stable_idxs"] != b["stable_idxs"] for a, b in zip(by_gap[:-1], by_gap[1:]))
    by_times = [oracle_step03("sweep", frames, params(min_times=m)) for m in MIN_TIMES]
    assert all(len(a["stable_idxs"]) > len(b["stable_idxs"]) for a, b in zip(by_times[:-1], by_times[1:]))
    for a, b in zip(by_times[:-1], by_times[1:]):
        assert a["n_split"] != b["n_split"] or a["cc_groups"] != b["cc_groups"]
    # -- the oracle runs to completion at every point of the sweep (the cache keeps the runs for the comparisons)
    for _, points in axis_points():
        for p in points:
            assert len(oracle_step03("sweep", frames, p)["clean_binary"]) == N_FRAMES


# ---- thresholds the kernels must never see ----------------------------------------------------------------------------------------
def check_huge_img_threshold(lib):
    """img_threshold = +inf and 1e300 (and the sign's other end): lm_group_run maps them on the host; v <= max, so the images are empty
    as the oracle's are (numpy: x >= inf is False)."""
    points = [params(img_threshold=t) for t in (float("inf"), 1e300, 1.0000000000000002, float("-inf"), -1e300)]
    frames = sweep_stream()
    for p in points[:2]:
        o = oracle_step03("sweep", frames, p)
        assert len(o["cc_groups"]) > 5 and not any(im.any() for k in o["group_images"] for im in o["group_images"][k])
    run_groupings(lib, points)


def check_nan_rejected(lib):
    frames = sweep_stream()
    fs = sweep_frame_stream(lib)
    for bad in (dict(img_threshold=float("nan")), dict(min_recall=float("nan")), dict(img_threshold=-float("nan"), min_recall=float("nan"))):
        try:
            device.Grouping(fs, **params(**bad)).close()
        except _lib.LecturemathError as e:
            assert "NaN" in str(e) and "NaN" in lib.last_error(), str(e)
        else:
            raise AssertionError("lm_group_run accepted %r" % (bad,))
    run_groupings(lib, [params()])          # the stream is still good for a run


# ---- step 02 ---------------------------------------------------------------------------------------------------------------------
def step02_stream(n_frames=14, h=64, w=128):
    """Shapes that grow and shrink by fixed fractions, so that (match / size of the new CC, match / size of the unique) is (1, q) or
    (q, 1) with q = 0.4, 0.6, 0.87, 0.95: which of them continue a unique depends on WHICH of the two thresholds is the large
    one.  Blinking shapes (absent for 1, 2 and 4 frames) make max_gap = 0, 1, 3 differ, and a shape that moves by a third of its
    width has recall = precision = 2/3."""
    if "step02" in _cache:
        return _cache["step02"]
    frames = np.zeros((n_frames, h, w), np.uint8)
    for f in range(n_frames):
        for k, q in enumerate((0.4, 0.6, 0.87, 0.95)):
            full, part = 100, int(round(100 * q))
            # 2-row bars of `part` px in even blocks of 3 frames and of `full` px in odd ones; the bar below shrinks where this one grows
            wide = (f // 3) % 2 == 1
            n = full if wide else part
            frames[f, 4 + 12 * k:4 + 12 * k + 2, 4:4 + n // 2] = 255
            n = part if wide else full
            frames[f, 8 + 12 * k:8 + 12 * k + 2, 4:4 + n // 2] = 255
        # blinking 6 x 6 squares: seen, absent for g frames, seen, ...
        for j, g in enumerate((1, 2, 4)):
            if f % (g + 1) == 0:
                frames[f, 54:60, 70 + 10 * j:76 + 10 * j] = 255
        # a 6 x 12 shape hopping 4 px to and fro: 2/3 of it stays
        x = 110 + 4 * ((f // 2) % 2)
        frames[f, 10:16, x:x + 12] = 255
    _cache["step02"] = frames
    return frames


def oracle_step02(thresholds, max_gap):
    k = ("step02", thresholds, max_gap)
    if k not in _cache:
        from oracle import cc as occ
        frames = step02_stream()
        st = occ.Stability(frames.shape[2], frames.shape[1], thresholds[0], thresholds[1], max_gap)
        for f in frames:
            st.add_frame(f)
        _cache[k] = st.result()
    return _cache[k]


def check_step02_stream_not_vacuous():
    # max_gap = 0 retires every unique in the frame after its first (frame 0's in frame 1): no threshold is ever met twice
    lists = [oracle_step02(t, 0)["unique_cc_frames"] for t in STEP02_THRESHOLDS]
    assert all(l == lists[0] for l in lists) and max(len(fl) for fl in lists[0]) == 2
    for gap in STEP02_GAPS[1:]:
        lists = [oracle_step02(t, gap)["unique_cc_frames"] for t in STEP02_THRESHOLDS]
        for i in range(len(lists)):
            for j in range(i + 1, len(lists)):
                assert lists[i] != lists[j], (gap, STEP02_THRESHOLDS[i], STEP02_THRESHOLDS[j])
    # the asymmetric pairs depend on WHICH side is the demanding one: with recall and precision swapped the uniques are others
    for t in STEP02_THRESHOLDS:
        by_gap = [oracle_step02(t, gap)["unique_cc_frames"] for gap in STEP02_GAPS]
        assert by_gap[0] != by_gap[1] and by_gap[1] != by_gap[2], t
    a, b = STEP02_THRESHOLDS[0], STEP02_THRESHOLDS[1]
    from oracle import cc as occ
    frames = step02_stream()
    for t in (a, b):
        st = occ.Stability(frames.shape[2], frames.shape[1], t[1], t[0], 3)
        for f in frames:
            st.add_frame(f)
        assert st.result()["unique_cc_frames"] != oracle_step02(t, 3)["unique_cc_frames"], t


def check_step02(lib, thresholds, max_gap):
    """The batched path (batches of 5 and one push) and records-then-match against the oracle."""
    frames = list(step02_stream())
    r1 = lm_checks.check_stream_oracle(lib, frames, max_gap, max_batch=5, thresholds=thresholds)
    r2 = lm_checks.check_stream_oracle(lib, frames, max_gap, max_batch=5, thresholds=thresholds, records_then_match=True)
    lm_checks.state_equal_oracle(r1, oracle_step02(thresholds, max_gap))
    lm_checks.state_equal_oracle(r2, oracle_step02(thresholds, max_gap))


# ---- min_pixels ------------------------------------------------------------------------------------------------------------------
def min_pixels_stream(n_frames=6, h=48, w=96):
    """5 x 5 squares (25 px), 4 x 5 and 4 x 6 rectangles (20 and 24 px), single pixels and one 6 x 6 square; some of each blink."""
    frames = np.zeros((n_frames, h, w), np.uint8)
    for f in range(n_frames):
        for k in range(4):
            on = (f + k) % 3 != 0
            if on:
                frames[f, 3:8, 3 + 12 * k:8 + 12 * k] = 255            # 25
                frames[f, 12:16, 3 + 12 * k:8 + 12 * k] = 255          # 20
                frames[f, 20:24, 3 + 12 * k:9 + 12 * k] = 255          # 24
            frames[f, 30 + (k % 2) * 2, 5 + 12 * k + f % 2] = 255      # 1
        frames[f, 38:44, 60:66] = 255                                  # 36
        frames[f, 3:8, 70:75] = 255                                    # 25, always on
        frames[f, 3:7, 80:85] = 255                                    # 20, always on
    return frames


def oracle_min_pixels(min_pixels):
    k = ("minpx", min_pixels)
    if k not in _cache:
        _cache[k] = oracle_stream("minpx", min_pixels_stream(), gap2=3, min_pixels=min_pixels)
    return _cache[k]


def check_min_pixels_stream_not_vacuous():
    kept = [sum(len(fr) for fr in oracle_min_pixels(m)["cc_idx_per_frame"]) for m in MIN_PIXELS]
    assert all(a > b for a, b in zip(kept[:-1], kept[1:])) and kept[-1] > 0, kept
    sizes = {int(s) for s in oracle_min_pixels(1)["unique_recs"][:, 4]}
    assert {1, 20, 24, 25} <= sizes


def check_min_pixels(lib, min_pixels, by_setter):
    frames = min_pixels_stream()
    h, w = frames[0].shape
    fs = device.FrameStream(w, h, len(frames), 0.85, 0.85, 3, 20 if by_setter else min_pixels, max_batch=4, lib=lib)
    try:
        if by_setter:
            fs.set_min_pixels(min_pixels)
        fs.push(fs.be.from_host(frames))
        lm_checks.state_equal_oracle(fs.result(), oracle_min_pixels(min_pixels))
    finally:
        fs.close()


# ---- the drop-in's cache of runs -------------------------------------------------------------------------------------------------
P1 = params(t_window=3, min_recall=1 / 3, img_threshold=0.2)
P2 = params(t_window=6, min_recall=1.0, img_threshold=0.9)


def _dropin_step03(est, p, n_frames):
    """The calls of pre_ST3D_v3.0_03_cc_grouping.py process_input, results in the shape of the oracle's dict."""
    stable = est.get_stable_cc_idxs(p["min_times"])
    tov, total, aov = est.compute_overlapping_stable_cc(stable, p["t_window"])
    groups, gid = est.compute_groups(stable, tov, p["min_recall"], None, None)
    ages, gpf = est.compute_groups_temporal_information(groups)
    conflicts = est.compute_conflicting_groups(stable, aov, len(groups), gid)
    images, bounds = est.compute_group_images(groups, ages, p["img_threshold"])
    clean = est._stream.be.to_host(est.frames_from_groups_device(0, n_frames))
    return {"stable_idxs": stable, "time_overlapping_cc": tov, "total_intersections": total, "all_overlapping_cc": aov,
            "cc_groups": groups, "group_idx_per_cc": gid, "group_ages": ages, "groups_per_frame": gpf, "conflicts": conflicts,
            "group_images": images, "group_boundaries": bounds, "clean_binary": list(clean),
            "unique_cc_frames": [[(int(a), int(b)) for a, b in fl] for fl in est.unique_cc_frames],
            "cc_idx_per_frame": [[(int(u), int(c.cc_id)) for u, c in fr] for fr in est.cc_idx_per_frame]}


DROPIN_FRAMES = 30


def check_dropin_parameter_sets(lib):
    """One CCStabilityEstimator asked for step 03 with P1 and then with P2 (its cache of device runs is keyed by the parameters):
    both answers equal the oracle's, the second equals that of an estimator that was never asked anything else (an unpickled copy
    of the first, taken before its first step-03 call), and P1 asked again still gives P1's answer."""
    import pickle
    dropin_checks.use_library(lib)
    from AccessMath.preprocessing.content.cc_stability_estimator import CCStabilityEstimator
    frames = sweep_stream()[:DROPIN_FRAMES]
    key = "sweep%d" % DROPIN_FRAMES
    o1, o2 = oracle_step03(key, frames, P1), oracle_step03(key, frames, P2)
    assert o1["cc_groups"] != o2["cc_groups"] and o1["total_intersections"] != o2["total_intersections"]
    assert any((a != b).any() for a, b in zip(o1["clean_binary"], o2["clean_binary"]))

    def run(est, p, o):
        r = _dropin_step03(est, p, len(frames))
        r["n_split"] = o["n_split"]                 # asked once per estimator, below
        grouping_equal_oracle(r, o, est.reconstructed_frame_sums())

    est = CCStabilityEstimator(W, H, 0.85, 0.85, 85, False)
    for f in frames:
        est.add_frame(f, True)
    est.finish_processing()
    fresh = pickle.loads(pickle.dumps(est))
    try:
        assert est.split_stable_cc_by_gaps(P1["max_gap"], P1["min_times"]) == o1["n_split"]
        run(est, P1, o1)
        run(est, P2, o2)
        assert len(est._groups) >= 2
        assert fresh.split_stable_cc_by_gaps(P2["max_gap"], P2["min_times"]) == o2["n_split"]
        run(fresh, P2, o2)
        run(est, P1, o1)
    finally:
        for e in (est, fresh):
            for g in e._groups.values():
                g.close()
            if e._stream is not None:
                e._stream.close()
