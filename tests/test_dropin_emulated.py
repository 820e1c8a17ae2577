"""CPU: the drop-in layer (reference module paths / script entry points) on the emulated library."""
import io
import os
import pickle

import numpy as np
import pytest

import dropin_checks
import lm_checks


def test_png_roundtrip_and_filters():
    from lecturemath_amd import png
    rng = np.random.default_rng(0)
    img = (rng.random((37, 53)) < 0.3).astype(np.uint8) * 255
    assert (png.decode_gray8(png.encode_gray8(img)) == img).all()
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray((rng.random((40, 61)) * 255).astype(np.uint8)).save(buf, format="PNG", optimize=True)   # adaptive filters
    a = png.decode_gray8(np.frombuffer(buf.getvalue(), np.uint8))
    assert (a == np.array(Image.open(io.BytesIO(buf.getvalue())))).all()


def test_labeler(emu_lib, oracle_built):
    dropin_checks.check_labeler(emu_lib)


def test_steps_02_03_short_gap(emu_lib):
    dropin_checks.check_steps_02_03(emu_lib, "short_gap_jitter")


def test_resize_golden(emu_lib):
    dropin_checks.check_resize_golden(emu_lib)


def test_fcn_class(emu_lib):
    dropin_checks.check_fcn_class(emu_lib, worker=False)       # the worker: test_step01_entry_points below


class _Held:
    """Stand-in for a class of the reference's modules while unpickling: keeps the pickled state as it is."""

    def __setstate__(self, state):
        self.state = state


class _StateUnpickler(pickle.Unpickler):
    def find_class(self, module, name):
        if module.split(".")[0] in ("AccessMath", "AM_CommonTools"):
            return type(name, (_Held,), {"module": module})
        return super().find_class(module, name)


def _same(a, b, path):
    """Equal pickled state: same types, same values (numpy scalars and arrays by dtype and value)."""
    if isinstance(a, _Held) or isinstance(b, _Held):
        assert type(a).__name__ == type(b).__name__ and a.module == b.module, path
        if type(a).__name__ != "IntervalIndex":         # an index of the active list, rebuilt from it by whoever reads it
            _same(a.state, b.state, path + "." + type(a).__name__)
        return
    assert type(a) is type(b), (path, type(a), type(b))
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), (path, sorted(a), sorted(b))
        for k in a:
            _same(a[k], b[k], "%s[%r]" % (path, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for k, (x, y) in enumerate(zip(a, b)):
            _same(x, y, "%s[%d]" % (path, k))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all(), path
    else:
        assert a == b, (path, a, b)


def test_pickle_interop_with_reference(emu_lib):
    """Our step-02 pickle carries the state the REFERENCE's step 02 pickles where the reference's step 03 reads it (same classes,
    attributes, types and values, so that step reads from it what it reads from its own), and the reference's step-02 pickle
    (tests/golden/g13_ref_step02_short_gap_jitter.pkl.gz, tests/golden/make_golden_reference_checks.py) is consumed by our step 03:
    both must reproduce the golden group ages."""
    import gzip
    blob = dropin_checks.check_steps_02_03(emu_lib, "short_gap_jitter")
    with gzip.open(os.path.join(lm_checks.GOLD, "g13_ref_step02_short_gap_jitter.pkl.gz"), "rb") as fh:
        theirs = fh.read()
    ours_state, theirs_state = (_StateUnpickler(io.BytesIO(b)).load() for b in (blob, theirs))
    assert type(ours_state[2]).__name__ == "CCStabilityEstimator" and ours_state[2].module == "AccessMath.preprocessing.content.cc_stability_estimator"
    # what the reference's step 03 reads of the estimator (pre_ST3D_v3.0_03_cc_grouping.py:41-91 and the methods it calls,
    # cc_stability_estimator.py:166-681) -- the rest is add_frame's working state
    step03 = ("width", "height", "unique_cc_objects", "unique_cc_frames", "cc_idx_per_frame", "tempo_count")
    _same(ours_state[:2], theirs_state[:2], "times/indices")
    _same({k: ours_state[2].state[k] for k in step03}, {k: theirs_state[2].state[k] for k in step03}, "estimator")
    g, spec, frames = lm_checks.load_stream("short_gap_jitter")
    # reference's pickle -> our step 03
    dropin_checks.use_library(emu_lib)
    t, i, est = pickle.loads(theirs)
    assert type(est).__module__ == "AccessMath.preprocessing.content.cc_stability_estimator" and hasattr(est, "_imported")
    s03 = dropin_checks.load_script("pre_ST3D_v3.0_03_cc_grouping.py")
    rec, conf, st3d = s03.process_input(dropin_checks.fake_process({"CC_STABILITY_MAX_GAP": str(spec["gap3"])}), (t, i, est))
    ng = len(conf[0])
    assert [[(a,) for a in conf[0][k]] for k in range(ng)] == lm_checks.unrag(g["ages"], g["ages_off"])
    gi = np.concatenate([im.ravel() for k in range(ng) for im in st3d.cc_group_images[k]])
    assert (gi == g["gimg"]).all()


@pytest.mark.parametrize("name", lm_checks.STREAMS)
def test_step_04_on_reference_step03_outputs(name):
    """Step 04 drop-in (host list logic) on the reference's own step-03 outputs: intervals of three parameter sets."""
    dropin_checks.check_step_04_from_golden(name)


def test_frame_sums_kernel(emu_lib):
    from lecturemath_amd import device
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (3, 37, 53), dtype=np.uint8)
    frames[1] = 255
    assert list(device.frame_sums(frames, emu_lib)) == [int(f.astype(np.int64).sum()) for f in frames]


def test_image_pairs_overlap(emu_lib):
    dropin_checks.check_image_pairs(emu_lib)


def test_step_05_short_gap(emu_lib):
    dropin_checks.check_step_05(emu_lib, "short_gap_jitter")


def test_step_05_tie_heavy_structures(emu_lib):
    dropin_checks.check_step_05_ties(emu_lib, cases=(0, 1))


def test_pipeline_short_gap(emu_lib):
    dropin_checks.check_pipeline(emu_lib, "short_gap_jitter")


def test_step01_entry_points(emu_lib, tmp_path):
    """pre_ST3D_v3.0_01_binarize.py get_worker / get_results with a torch.save'd state_dict, and test_FCN_binarizer.py main()."""
    dropin_checks.check_step01_entry_points(emu_lib, tmp_path, n_frames=1, tool=False)     # the one-image tool: GPU suite


def test_rebuilt_binary_images(emu_lib, oracle_built):
    dropin_checks.check_rebuilt_binary_images(emu_lib)


def test_overlap_golden_g2(emu_lib):
    dropin_checks.check_overlap_golden(emu_lib)
