"""GPU: the device PNG codec (csrc/lm_png.hip) on the MI355X, valid inputs only: round trips at 1080p and 4K, host- and
PIL-written files, LecturePipeline.add_png_frames and the LM_PNG_CODEC=device wiring of the drop-in scripts."""
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _frames(n, h, w, seed):
    from lecturemath_amd import synth
    fr = np.stack(list(synth.binary_stream(n, h, w, seed=seed)))
    rng = np.random.default_rng(seed)
    fr[1] = rng.integers(0, 256, (h, w), dtype=np.uint8)                        # any byte values, not just {0, 255}
    fr[2] = ((np.indices((h, w)).sum(0) % 2) * 255).astype(np.uint8)            # the worst case for the encoder
    return fr


@pytest.mark.parametrize("h,w,n", [(1080, 1920, 64), (2160, 3840, 24)])
def test_round_trips(hip_lib, h, w, n):
    import torch
    from lecturemath_amd import png, png_device
    frames = _frames(n, h, w, seed=h)
    files = png_device.encode_gray8_device(torch.from_numpy(frames).cuda(), lib=hip_lib)
    bound = hip_lib.lm_png_encode_bound(w, h)
    assert len(files) == n and max(len(f) for f in files) <= bound
    for i in (0, 1, 2, n - 1):
        assert (png.decode_gray8(files[i]) == frames[i]).all(), i
    dec = png_device.decode_gray8_device(files, w, h, lib=hip_lib)
    assert (dec.cpu().numpy() == frames).all()
    synth_mean = np.mean([len(files[i]) for i in range(3, n)])
    if h == 1080:                                                                # the issue's yardstick (4K blank rows)
        assert synth_mean <= np.mean([len(png.encode_gray8(frames[i])) for i in range(3, n)])


def test_decode_host_and_pil_files(hip_lib):
    from PIL import Image
    from lecturemath_amd import png, png_device
    h, w = 1080, 1920
    frames = _frames(6, h, w, seed=7)
    files, expect = [], []
    for i, f in enumerate(frames):
        for level in (1, 9):
            files.append(png.encode_gray8(f, level))
            expect.append(f)
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, format="PNG", optimize=(i % 2 == 0))
        files.append(buf.getvalue())
        expect.append(f)
    dec = png_device.decode_gray8_device(files, w, h, lib=hip_lib)
    assert (dec.cpu().numpy() == np.stack(expect)).all()


def test_pipeline_add_png_frames(hip_lib):
    """add_png_frames (device decode) against add_binary_frames on the same frames; finish(reconstructed_png="device") against True"""
    import dropin_checks
    from lecturemath_amd import digests, png, synth
    from lecturemath_amd.pipeline import LecturePipeline
    dropin_checks.use_library(hip_lib)
    h, w = 540, 960
    frames = np.stack(list(synth.binary_stream(40, h, w, seed=31, glyphs_per_add=20, erase_every=17)))
    files = [png.encode_gray8(f) for f in frames]
    outs = []
    for feed in ("binary", "png"):
        pipe = LecturePipeline(w, h, lib=hip_lib)
        if feed == "binary":
            pipe.add_binary_frames(frames)
        else:
            pipe.add_png_frames(files)
        out = pipe.finish(reconstructed_png=True if feed == "binary" else "device")
        est = pipe.estimator
        outs.append((digests.from_device(est._stream, est._cur(getattr(est, "_thr", 0.5))), [tuple(iv) for iv in out["intervals"]],
                     np.stack([png.decode_gray8(c) for c in out["reconstructed_png"]])))
    assert outs[0][0] == outs[1][0]
    assert outs[0][1] == outs[1][1]
    assert outs[0][2].shape == (len(frames), h, w) and (outs[0][2] == outs[1][2]).all()


def test_device_codec_wiring(hip_lib, monkeypatch):
    """LM_PNG_CODEC=device: step 02, Helper, the step-01 worker and frames_from_groups give the host path's pixels; step 02's
    products are equal."""
    import dropin_checks
    from lecturemath_amd import png, synth
    dropin_checks.use_library(hip_lib)
    from AccessMath.preprocessing.content.helper import Helper
    from AccessMath.preprocessing.video_worker.FCN_lecturenet_binarizer import FCN_LectureNet_Binarizer
    h, w = 270, 480
    frames = list(synth.binary_stream(30, h, w, seed=41, glyphs_per_add=10, erase_every=11))
    comp = [png.encode_gray8(f) for f in frames]
    times, idxs = [100.0 * i for i in range(len(frames))], list(range(len(frames)))
    s02 = dropin_checks.load_script("pre_ST3D_v3.0_02_cc_analaysis.py")
    s03 = dropin_checks.load_script("pre_ST3D_v3.0_03_cc_grouping.py")
    proc = dropin_checks.fake_process()
    res = {}
    for mode in ("host", "device"):
        monkeypatch.setenv("LM_PNG_CODEC", mode)
        dec = Helper.decompress_binary_images(comp)
        assert all((a == b).all() for a, b in zip(dec, frames)), mode
        t, i, est = s02.process_input(proc, (times, idxs, comp))
        rec, conf, st3d = s03.process_input(proc, (t, i, est))
        res[mode] = (est.tempo_count, est.unique_cc_frames, [[(u, c.cc_id) for u, c in fr] for fr in est.cc_idx_per_frame],
                     list(est.cc_active), [png.decode_gray8(c) for c in rec[2]], conf[0])

        class _Net:                                                  # binarize() stand-in: the frame's own binary, ink = 0
            def __init__(self):
                self.k = 0

            def binarize(self, img, return_others=False, force_binary=False):
                b = 255 - frames[self.k]
                self.k += 1
                return b, np.zeros_like(b), np.zeros((h, w, 3), np.uint8)
        worker = FCN_LectureNet_Binarizer(_Net())
        worker.initialize(w, h)
        for k in range(4):
            worker.handleFrame(np.zeros((h, w, 3), np.uint8), None, 0, float(k), float(k), k)
            assert (worker.last_binary == frames[k]).all()
        assert all((png.decode_gray8(c) == frames[k]).all() for k, c in enumerate(worker.compressed_frames)), mode
        device_made = [bytes(c) != bytes(png.encode_gray8(frames[k])) for k, c in enumerate(worker.compressed_frames)]
        device_made += [bytes(c) != bytes(png.encode_gray8(png.decode_gray8(c))) for c in rec[2][:4]]
        assert all(device_made) if mode == "device" else not any(device_made)
    for a, b in zip(res["host"], res["device"]):
        if isinstance(a, list) and a and isinstance(a[0], np.ndarray):
            assert all((x == y).all() for x, y in zip(a, b)) and len(a) == len(b)
        else:
            assert a == b
