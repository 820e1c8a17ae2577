"""Checks of step 04's SUMS segmentation (VIDEO_SEGMENTATION_METHOD = 1) shared by the CPU tests (emulated library) and the GPU
tests: lm_group_frame_sums against the rendered frames, the drop-in's regression tree / VideoSegmenter / step script / pipeline
against what the reference returned and printed (tests/golden/g20_step04_sums.npz, tests/golden/make_golden_step04_sums.py)."""
import contextlib
import io
import json
import os

import numpy as np

import dropin_checks
import lm_checks
import segment_conflict_checks as scc
from lecturemath_amd import _lib, device

K = "VIDEO_SEGMENTATION_SUM_"
KINDS = 4

_g20 = None


def g20():
    global _g20
    if _g20 is None:
        g = np.load(os.path.join(lm_checks.GOLD, "g20_step04_sums.npz"))
        _g20 = {k: g[k] for k in g.files}
        _g20["params"] = json.loads(bytes(_g20["params"]).decode())
    return _g20


def segmenter():
    return scc.segmenter()


def bits(values):
    return np.asarray(values, np.float64).view(np.int64)


# ---- the random signals --------------------------------------------------------------------------------------------------------
def check_cases_not_vacuous(g):
    n = int(g["n_cases"])
    assert n >= 300 and len(g["kind"]) == n
    assert all(int((g["kind"] == k).sum()) >= 50 for k in range(KINDS))
    assert (np.diff(g["seg_off"]) >= 2).mean() >= 0.5
    assert int(g["short_node"].sum()) >= 20         # a node with leaf_min > m - leaf_min
    assert int(g["backward"].sum()) >= 20           # ... and the left sum of a winning split taken from the far end
    assert int(g["rot_leaf"].sum()) >= 20           # a right child that is a leaf of >= 3 samples with non-integer values
    assert int(g["rot_shows"].sum()) >= 20          # ... whose value is not the frame-order sum / count
    assert g["n"].min() >= 5 and g["n"].max() <= 600 and g["leaf_min"].min() >= 1 and g["leaf_min"].max() <= 40
    assert len(set(g["min_erase"].tolist())) >= 3
    frac = [g["S"][g["y_off"][c]:g["y_off"][c + 1]] % 255 for c in range(n) if g["divisor"][c] == 255]
    assert len(frac) >= 100 and all((f != 0).all() for f in frac)


def case_signal(g, c):
    S = g["S"][g["y_off"][c]:g["y_off"][c + 1]]
    return S / 255 if g["divisor"][c] == 255 else S.astype(np.float64)


def check_cases(which=None):
    """create_regresor_from_sums + get_tree_decision_boundaries and video_segments_from_sums of the drop-in on G20's signals:
    interval_idxs, interval_vals bit for bit, segments."""
    VS = segmenter()
    g = g20()
    for c in (range(int(g["n_cases"])) if which is None else which):
        all_sums = list(case_signal(g, c))
        leaf_min, min_erase = int(g["leaf_min"][c]), float(g["min_erase"][c])
        tree = VS.create_regresor_from_sums(all_sums, leaf_min)
        idxs, vals = VS.get_tree_decision_boundaries(tree, len(all_sums))
        sl = slice(g["idx_off"][c], g["idx_off"][c + 1])
        assert idxs == g["interval_idxs"][sl].tolist(), c
        assert (bits(vals) == g["interval_vals"][sl]).all(), c
        with np.errstate(all="ignore"):
            segments = VS.video_segments_from_sums(all_sums, leaf_min, min_erase)
        assert [tuple(int(v) for v in s) for s in segments] == scc.pairs_of(g["segments"][g["seg_off"][c]:g["seg_off"][c + 1]]), c


def check_tree_vs_sklearn(trials=300, seed=77):
    """fresh random signals of the four kinds: predictions of the restated tree == sklearn's, bit for bit"""
    from sklearn.tree import DecisionTreeRegressor
    VS = segmenter()
    rng = np.random.default_rng(seed)
    for trial in range(trials):
        n, leaf_min = int(rng.integers(1, 400)), int(rng.integers(1, 41))
        level = np.cumsum(rng.integers(0, 400, n))
        for _ in range(int(rng.integers(0, 5))):
            k = int(rng.integers(0, n))
            level[k:] -= int(level[k] * rng.random())
        y = (level.astype(np.float64), np.floor(level / 3.0), (level * 255 + rng.integers(1, 255, n)) / 255,
             np.repeat((level[::20] * 255 + 7) / 255, 20)[:n])[trial % 4]
        X = np.arange(n, dtype=np.int32).reshape(n, 1)
        want = DecisionTreeRegressor(max_depth=None, min_samples_leaf=leaf_min).fit(X, y).predict(X)
        got = VS.create_regresor_from_sums(list(y), leaf_min).predict(X)
        assert got.shape == want.shape and (bits(got) == bits(want)).all(), (trial, n, leaf_min)


# ---- the golden streams --------------------------------------------------------------------------------------------------------
def method1_process(values, params=None):
    return dropin_checks.fake_process(dict({key: str(v) for key, v in values.items()}, VIDEO_SEGMENTATION_METHOD="1"), params)


_runs = {}


def pipeline_run(lib, name, k=1):
    """LecturePipeline with VIDEO_SEGMENTATION_METHOD = 1 (parameter set k of G20) on a golden stream, finished with no
    reconstructed frame asked for; then, from the same estimator, the reconstructed frames as PNG files (what finish(reconstructed_png=
    True) would have returned).  Run once per library and stream: (pipeline, finish()'s result, PNG files, times, indices)."""
    key = (lib.path, name, k)
    if key not in _runs:
        dropin_checks.use_library(lib)
        from lecturemath_amd.pipeline import LecturePipeline
        _, spec, frames = lm_checks.load_stream(name)
        conf = dict(g20()["params"][k], VIDEO_SEGMENTATION_METHOD=1, CC_STABILITY_MAX_GAP=spec["gap2"])
        n = len(frames)
        times, idxs = [1000.0 * i for i in range(n)], list(range(n))
        pipe = LecturePipeline(spec["w"], spec["h"], conf=conf, lib=lib)
        pipe.add_binary_frames(np.stack(frames), times, idxs)
        pipe.configuration.data["CC_STABILITY_MAX_GAP"] = str(spec["gap3"])      # the fixtures ran steps 02 and 03 with different values
        out = pipe.finish()
        assert out["reconstructed_png"] == []
        _runs[key] = (pipe, out, pipe.estimator._frames_png("host"), times, idxs)
    dropin_checks.use_library(lib)
    return _runs[key]


def check_script_stream(lib, name):
    """pre_ST3D 04 with method 1 on the reconstructed PNGs of the drop-in's step 03: the reference's sums, printed text and intervals
    for the parameter sets of G20.  Returns the largest number of intervals."""
    _, _, pngs, times, idxs = pipeline_run(lib, name)
    g = g20()
    s04 = dropin_checks.load_script("pre_ST3D_v3.0_04_vid_segmentation.py")
    assert (bits(s04.binary_sums(pngs)) == g["%s.sums" % name]).all()
    most = 0
    for k, values in enumerate(g["params"]):
        with contextlib.redirect_stdout(io.StringIO()) as text:
            intervals = s04.process_input(method1_process(values), (times, idxs, pngs))
        assert scc.pairs_of(intervals) == scc.pairs_of(g["%s.intervals_%d" % (name, k)]), (name, k)
        assert text.getvalue() == bytes(g["%s.printed_%d" % (name, k)]).decode(), (name, k)
        most = max(most, len(intervals))
    return most


def check_script_sums_parameter(lib, name, n_frames=None):
    """`sums=1` of methods 2 and 3 prints the same sums (of the first n_frames frames, all by default)"""
    pipe, out, pngs, times, idxs = pipeline_run(lib, name)
    s04 = dropin_checks.load_script("pre_ST3D_v3.0_04_vid_segmentation.py")
    n = len(pngs) if n_frames is None else n_frames
    want = [float(v) for v in g20()["%s.sums" % name].view(np.float64)][:n]
    for method in ("2", "3"):
        proc = dropin_checks.fake_process({"VIDEO_SEGMENTATION_METHOD": method}, {"sums": "1"})
        with contextlib.redirect_stdout(io.StringIO()) as text:
            s04.process_input(proc, [(times, idxs, pngs[:n]), (out["group_ages"], out["conflicts"]), out["st3d"]])
        lines = text.getvalue().splitlines()
        assert lines[0] == "Computing sums..." and [float(v) for v in eval(lines[1], {"np": np})] == want, method


def check_pipeline(lib, name, k=1):
    """LecturePipeline with VIDEO_SEGMENTATION_METHOD = 1 (parameter set k of G20), no reconstructed frame asked for, == the step
    script fed the pipeline's own reconstructed PNGs == the reference's intervals."""
    pipe, out, pngs, times, idxs = pipeline_run(lib, name, k)
    g = g20()
    n = len(pngs)
    assert scc.pairs_of(out["intervals"]) == scc.pairs_of(g["%s.intervals_%d" % (name, k)]) and len(out["intervals"]) >= 2
    assert len(out["keyframes"]) == len(out["intervals"])
    sums = pipe.estimator.reconstructed_frame_sums()
    assert sums.dtype == np.int64 and (bits([int(v) / 255 for v in sums]) == g["%s.sums" % name]).all()
    assert (pipe.estimator.reconstructed_frame_sums(3, 5) == sums[3:8]).all() and (pipe.estimator.reconstructed_frame_sums(n - 2) == sums[n - 2:]).all()
    s04 = dropin_checks.load_script("pre_ST3D_v3.0_04_vid_segmentation.py")
    with contextlib.redirect_stdout(io.StringIO()):
        from_script = s04.process_input(method1_process(g["params"][k]), (times, idxs, pngs))
    assert scc.pairs_of(from_script) == scc.pairs_of(out["intervals"])
    from lecturemath_amd.pipeline import DEFAULT_CONF
    assert (DEFAULT_CONF["SAMPLING_FPS"], DEFAULT_CONF[K + "MIN_SEGMENT"], DEFAULT_CONF[K + "MIN_ERASE_RATIO"]) == ("1.0", "10", "0.05")


# ---- the kernel ----------------------------------------------------------------------------------------------------------------
KERNEL_STREAMS = ("blink_overlap", "dot_grid") + tuple(lm_checks.STREAMS)


def kernel_stream(name):
    """(frames, gap2, gap3) of a kernel test stream"""
    if name == "blink_overlap":         # 80 x 300, pixels holding 253 / 254 / 255, items across x = 256 and off the 32-pixel columns
        return np.stack(lm_checks.blink_overlap_stream()), 85, 85
    if name == "dot_grid":              # 72 x 520, more items per tile than the cooperative hit list (LM_RT_MAXHIT) holds
        return np.stack(lm_checks.dot_grid_stream()), 85, 85
    _, spec, frames = lm_checks.load_stream(name)
    return frames, spec["gap2"], spec["gap3"]


@contextlib.contextmanager
def grouping_of(lib, frames, gap2, gap3, reconstruct=True):
    n, h, w = frames.shape
    fs = device.FrameStream(w, h, n, 0.85, 0.85, gap2, 20, max_batch=8, lib=lib, max_ccs=max(n * h * w // 24, 1 << 12),
                            max_crop_words=max(n * h * w // 4, 1 << 14))
    try:
        fs.push(fs.be.from_host(frames))
        gr = device.Grouping(fs, max_gap=gap3, min_times=3, t_window=5, min_recall=0.5, img_threshold=0.5, reconstruct=reconstruct)
        try:
            yield gr
        finally:
            gr.close()
    finally:
        fs.close()


@contextlib.contextmanager
def grouping_for(lib, name):
    """the step-03 run of a kernel test stream: the cached pipeline's for a golden stream, a fresh one otherwise"""
    if name in lm_checks.STREAMS:
        pipe = pipeline_run(lib, name)[0]
        yield pipe.estimator._cur(pipe.estimator._thr)
    else:
        with grouping_of(lib, *kernel_stream(name)) as gr:
            yield gr


def check_kernel_stream(lib, name):
    """lm_group_frame_sums == numpy.sum(dtype=uint64) of lm_group_render's frames (== lm_frame_sums of them on the device), for the
    whole stream and for sub-ranges: first > 0, n = 1 (first, middle and last frame), n = 0.  Returns the set of pixel values."""
    n = len(kernel_stream(name)[0])
    with grouping_for(lib, name) as gr:
        rendered = gr.render(0, n)
        clean = gr.be.to_host(rendered)
        want = clean.reshape(n, -1).sum(axis=1, dtype=np.uint64).astype(np.int64)
        got = gr.frame_sums(0, n)
        assert got.dtype == np.int64 and got.shape == (n,) and (got == want).all(), (name, np.flatnonzero(got != want)[:8])
        assert (device.frame_sums(rendered, lib) == want).all()
        assert want.max() > 0 and len(set(want.tolist())) > 1
        for first, count in ((1, n - 1), (n // 2, 1), (0, 1), (n - 1, 1), (2, n - 3), (0, 0), (n, 0)):
            part = gr.frame_sums(first, count)
            assert part.shape == (count,) and (part == want[first:first + count]).all(), (name, first, count)
        return set(np.unique(clean).tolist())


def check_kernel_arguments(lib):
    frames, gap2, gap3 = kernel_stream("short_gap_jitter")
    frames = frames[:12]
    be = device.Backend(lib)
    out = be.empty((16,), np.int64)
    with grouping_of(lib, frames, gap2, gap3) as gr:
        n, h = len(frames), gr.handle
        for first, count, dst in ((-1, 2, out), (0, n + 1, out), (n - 1, 2, out), (0, -1, out), (n + 1, 0, out), (0, 2, None)):
            assert lib.lm_group_frame_sums(h, first, count, _lib.ptr(dst), be.stream()) == _lib.LM_ERR_ARG, (first, count)
            assert "lm_group_frame_sums" in lib.last_error()
        assert lib.lm_group_frame_sums(None, 0, 1, _lib.ptr(out), be.stream()) == _lib.LM_ERR_ARG
        assert lib.lm_group_frame_sums(h, 0, 0, None, be.stream()) == _lib.LM_OK
        try:
            gr.frame_sums(0, n + 1)
        except _lib.LecturemathError as e:
            assert "lm_group_frame_sums" in str(e)
        else:
            raise AssertionError("frame_sums past the last frame did not raise")
    with grouping_of(lib, frames, gap2, gap3, reconstruct=False) as gr:         # no render tables: refused like lm_group_render
        assert lib.lm_group_frame_sums(gr.handle, 0, 1, _lib.ptr(out), be.stream()) == _lib.LM_ERR_ARG
        assert "reconstruct_tables" in lib.last_error()


def check_script_device_codec(lib, name, n_frames=None, batch=None):
    """LM_PNG_CODEC=device: method 1 and `sums=1` decode the PNG list on the device a batch at a time and sum there.  With n_frames
    (and batch, the files per decode call) only the first frames go through, and method 1 has to return what it returns for them with
    the host codec: the emulated decoder takes most of a second per file."""
    from lecturemath_amd import png_device
    _, _, pngs, times, idxs = pipeline_run(lib, name)
    s04 = dropin_checks.load_script("pre_ST3D_v3.0_04_vid_segmentation.py")
    values = g20()["params"][1]
    host = None
    if n_frames is not None:
        with contextlib.redirect_stdout(io.StringIO()) as host_text:
            host = s04.process_input(method1_process(values), (times[:n_frames], idxs[:n_frames], pngs[:n_frames]))
    old, old_batch = os.environ.get("LM_PNG_CODEC"), png_device.BATCH
    os.environ["LM_PNG_CODEC"] = "device"
    png_device.BATCH = batch or old_batch
    try:
        if n_frames is None:
            most = check_script_stream(lib, name)
        else:
            assert (bits(s04.binary_sums(pngs[:n_frames])) == g20()["%s.sums" % name][:n_frames]).all()
            with contextlib.redirect_stdout(io.StringIO()) as text:
                got = s04.process_input(method1_process(values), (times[:n_frames], idxs[:n_frames], pngs[:n_frames]))
            assert got == host and text.getvalue() == host_text.getvalue()
            most = len(got)
        check_script_sums_parameter(lib, name, n_frames)
    finally:
        png_device.BATCH = old_batch
        if old is None:
            del os.environ["LM_PNG_CODEC"]
        else:
            os.environ["LM_PNG_CODEC"] = old
    return most
