"""GPU parity tests proper: the gfx950 library, through the C ABI, against the reference's golden vectors
(tests/golden, produced by running the reference) and against the oracle on seeded inputs."""
import os

import numpy as np
import pytest

import lm_checks
from lecturemath_amd import device, synth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("i", range(18))
def test_label_stats_golden(hip_lib, oracle_built, i):
    lm_checks.check_g1_frame(hip_lib, i)


def test_threshold_golden(hip_lib):
    g = np.load(os.path.join(lm_checks.GOLD, "g6_threshold.npz"))
    lab = device.FrameLabeler(96, 64, 1, hip_lib)
    out = lab.be.to_host(lab.threshold_invert(lab.be.from_host(g["logits"])))
    far = np.abs(g["logits"] - 0.0078433) > 1e-4
    assert (out[far] == g["expected"][far]).all()
    # pixels within 1e-4 of the decision edge: device expf vs torch CPU sigmoid may round differently
    assert int((out != g["expected"]).sum()) <= 4
    lab.close()


@pytest.mark.parametrize("name", lm_checks.STREAMS)
def test_stream_golden(hip_lib, name):
    lm_checks.check_stream_golden(hip_lib, name, max_batch=16)


def test_label_batch_in_parts(hip_lib, oracle_built):
    """lm_label_batch labels the parts of a batch on two queues; every frame vs the oracle, at a size where the parts overlap."""
    lm_checks.check_label_batch_in_parts(hip_lib)
    lm_checks.check_label_batch_in_parts(hip_lib, n_frames=40, h=270, w=480)


def test_stream_run_logits(hip_lib, oracle_built):
    """The whole steps 01-02 loop in one call: one queue, two queues, and two queues with the gated schedule (labelling kept
    apart from the matching's wide kernels) give the per-batch result and the oracle's."""
    lm_checks.check_stream_run_logits(hip_lib)
    lm_checks.check_stream_run_logits(hip_lib, second_stream=True)
    lm_checks.check_stream_run_logits(hip_lib, n_frames=41, batch=4, schedule=1, second_stream=True)


def test_stream_match_paths_agree(hip_lib, oracle_built):
    lm_checks.check_stream_match_paths(hip_lib, n_frames=150)
    lm_checks.check_stream_match_paths(hip_lib, n_frames=97, max_gap=1, seed=4)


def test_stream_frames_with_thousands_of_ccs(hip_lib, oracle_built):
    """~3.7k kept CCs per frame: more than one LDS pass of the replay kernel (2048 CCs) and several join chunks."""
    frames = lm_checks.dot_grid_stream(n_frames=6, h=200, w=800, seed=8)
    r = lm_checks.check_stream_oracle(hip_lib, frames, max_gap=2, max_batch=4, max_ccs=1 << 16, max_crop_words=1 << 20)
    assert len(r["cc_idx_per_frame"][0]) > 3000


def test_stream_frames_with_seven_thousand_ccs(hip_lib, oracle_built):
    """~7k kept CCs per frame: lm_k_select scans more than 4,096 labels per frame (two passes with a carry), lm_k_emit's workgroups
    search more than 4,096 crop offsets for their first CC and walk many descriptor windows."""
    frames = lm_checks.dot_grid_stream(n_frames=5, h=300, w=1000, seed=5)
    r = lm_checks.check_stream_oracle(hip_lib, frames, max_gap=2, max_batch=5, max_ccs=1 << 16, max_crop_words=1 << 20)
    assert len(r["cc_idx_per_frame"][0]) > 6000


def test_stream_large_components(hip_lib, oracle_built):
    """Large components (crops of 10^3..10^4 words) among glyph-sized ones, as in the later part of a lecture: lm_k_emit by crop
    words, lm_k_mb_twin_cmp, the size prune of lm_k_mb_eval and lm_k_mb_eval_big vs the oracle, both matching paths."""
    lm_checks.check_stream_large_components(hip_lib, n_frames=40, h=400, w=1600)


def test_stream_churn_and_empty_frames(hip_lib, oracle_built):
    """A stream where nearly every CC is a new unique (>16k in-batch sources and >16k active positions in ONE 40-frame
    matching batch: the replay kernel's global-memory fallbacks) and every seventh frame is empty; both matching paths."""
    frames = lm_checks.churn_stream()
    # max_gap = 1: a unique retires as soon as it misses a frame, so almost every CC of the 40-frame batch is a new unique
    r = lm_checks.check_stream_oracle(hip_lib, frames, max_gap=1, max_batch=8, records_then_match=True, max_ccs=1 << 17,
                                      max_crop_words=1 << 21)
    assert len(r["unique_recs"]) > 20000
    lm_checks.check_stream_oracle(hip_lib, frames, max_gap=50, max_batch=8, max_ccs=1 << 17, max_crop_words=1 << 21)


def test_legacy_exports_vs_reference_c(hip_lib, oracle_built):
    """speaker_detection_handle_frame / regionCumulativeDistribution / adapthisteq / combine_results of accessmath_lib.c on
    the device vs what the reference C library returns (tests/golden/g14_legacy_exports.json), bit for bit, up to 1080p."""
    lm_checks.check_legacy_exports(hip_lib, big=True)


def test_stream_vs_oracle_random_noise(hip_lib, oracle_built):
    rng = np.random.default_rng(11)
    base = (rng.random((120, 200)) < 0.5)
    frames = []
    for t in range(12):
        flip = rng.random(base.shape) < 0.002
        base = base ^ flip
        frames.append((base * 255).astype(np.uint8))
    lm_checks.check_stream_oracle(hip_lib, frames, max_gap=3, max_batch=4, max_crop_words=1 << 22, max_ccs=1 << 16)


def test_full_size_1080p_label_vs_oracle(hip_lib, oracle_built):
    """BASELINE.json config-1 style frame at the full 1920x1080: bit-exact labels, counts, stats."""
    frames = np.stack([synth.glyph_mask(1080, 1920, 1500, seed=20211), synth.glyph_mask(1080, 1920, 4000, seed=7)])
    lab = device.FrameLabeler(1920, 1080, 2, hip_lib)
    labels, counts = lab.label(lab.be.from_host(frames))
    labels = lab.be.to_host(labels)
    st = lab.stats(counts)
    for b in range(2):
        l, n = oracle_built.label4(frames[b])
        assert counts[b] == n and (labels[b] == l).all()
        assert (st[b] == np.stack(oracle_built.age_boundaries(l, None, n)[:5])).all()
    lab.close()


def test_full_size_stream_1080p_vs_oracle(hip_lib, oracle_built):
    """The first 96 frames of the bench stream (1920x1080, ~1100 CCs per frame) through 64-frame launches -- one full matching
    batch, one partial -- vs the oracle: records, crops, uniques, assignments, tempo_count."""
    frames = list(synth.binary_stream(256, 1080, 1920, seed=20213))[:96]
    r = lm_checks.check_stream_oracle(hip_lib, frames, max_gap=85, max_batch=64)
    assert len(r["unique_recs"]) > 1000


def test_full_size_properties_4k(hip_lib):
    """3840x2160 (BASELINE.json config 5 size): size-independent properties instead of the oracle:
    relabelling the foreground mask of the labels reproduces them (idempotence), counts sum to the ink."""
    import torch
    f = synth.glyph_mask(2160, 3840, 6000, seed=3)
    lab = device.FrameLabeler(3840, 2160, 1, hip_lib)
    d = lab.be.from_host(f[None])
    labels, counts = lab.label(d)
    st = lab.stats(counts)[0]
    assert int(st[4].sum()) == int((f > 0).sum())
    again, counts2 = lab.label(((labels > 0) * 255).to(torch.uint8))
    assert counts2[0] == counts[0] and bool((again == labels).all())
    lab.close()


def test_4k_stream_and_grouping_vs_oracle(hip_lib, oracle_built):
    """BASELINE configs[4] size (3840x2160, WW = 60 words per row): a 24-frame stream through labelling, statistics, records,
    crops and temporal matching vs the oracle, and step 03 (groups, ages, group images, every reconstructed frame) of its first
    12 frames vs the oracle's grouping."""
    frames = list(synth.binary_stream(24, 2160, 3840, seed=20215, glyphs_per_add=160, erase_every=9, jitter_p=0.2, max_ext=56))
    r = lm_checks.check_stream_oracle(hip_lib, frames, max_gap=85, max_batch=8, max_ccs=1 << 18, max_crop_words=1 << 25)
    assert len(r["unique_recs"]) > 1000
    g = lm_checks.check_grouping_oracle(hip_lib, frames[:12], max_batch=6)
    assert len(g["cc_groups"]) > 100


def test_drop_in_cc_age_boundaries(hip_lib, oracle_built):
    rng = np.random.default_rng(3)
    img = ((rng.random((270, 480)) < 0.4) * 255).astype(np.uint8)
    labels, n = oracle_built.label4(img)
    ages = rng.random(img.shape).astype(np.float32)
    outs = [np.zeros(n, np.int32) for _ in range(5)]
    oa = np.zeros(n, np.float32)
    rc = hip_lib.CC_AgeBoundaries(labels.ctypes.data, ages.ctypes.data, 480, 270, n, *[o.ctypes.data for o in outs], oa.ctypes.data)
    assert rc == 0
    for a, b in zip(outs + [oa], oracle_built.age_boundaries(labels, ages, n)):
        assert (a == b).all()
    # signed ages: the reference's sequential "-1 = nothing yet" rule (accessmath_lib.c:405-407) lets a negative age be
    # overwritten by whatever pixel follows; labels ending on a negative age keep it
    for seed in (4, 5):
        ages = np.random.default_rng(seed).normal(0.2, 1.0, img.shape).astype(np.float32)
        oa = np.zeros(n, np.float32)
        hip_lib.CC_AgeBoundaries(labels.ctypes.data, ages.ctypes.data, img.shape[1], img.shape[0], n, *[o.ctypes.data for o in outs], oa.ctypes.data)
        exp_age = oracle_built.age_boundaries(labels, ages, n)[5]
        assert (exp_age < 0).any() and (exp_age >= 0).any() and (oa == exp_age).all()


def test_label_host(hip_lib, oracle_built):
    img = synth.glyph_mask(270, 480, 200, seed=9)
    out = np.zeros(img.shape, np.int32)
    n = hip_lib.lm_label_host(img.ctypes.data, 480, 270, out.ctypes.data)
    l, m = oracle_built.label4(img)
    assert n == m and (out == l).all()


def test_dense_wide_noise_band_fallback(hip_lib, oracle_built):
    """> 8192 runs inside one 64-row band (LDS forest falls back to L2 atomics) and > 512 labels per stats tile."""
    rng = np.random.default_rng(21)
    img = ((rng.random((70, 1100)) < 0.5) * 255).astype(np.uint8)
    lm_checks.check_label_vs_oracle(hip_lib, img)


@pytest.mark.parametrize("name", lm_checks.STREAMS)
def test_grouping_golden(hip_lib, name):
    """Step 03 (split, stable set, overlaps, groups, ages, conflicts, group images, reconstructed frames) vs the reference."""
    lm_checks.check_grouping_golden(hip_lib, name)


def test_grouping_crowded_tiles_vs_oracle(hip_lib, oracle_built):
    """~800 stable groups on a 72x520 frame: render tiles with more items than the cooperative hit list (96)."""
    r = lm_checks.check_grouping_oracle(hip_lib, lm_checks.dot_grid_stream())
    assert len(r["cc_groups"]) > 500


def test_threshold_comparison_form(hip_lib):
    """x >= x* (the kernel that runs) == the sigmoid formula kernel, ulp by ulp around the edge of eight thresholds."""
    lm_checks.check_threshold_paths(hip_lib)
    lm_checks.check_label_logits_fused(hip_lib, shapes=((3, 37, 68), (2, 9, 1028), (1, 5, 4100), (5, 1080, 1920), (2, 2160, 3840)))


def test_stream_threshold_edges(hip_lib, oracle_built):
    """min recall / precision of exactly 1 (twins only) and above 1 (no twin detection, nothing matches)."""
    lm_checks.check_stream_threshold_edges(hip_lib)


def test_render_overlapping_group_images(hip_lib, oracle_built):
    """Group images added on top of each other (pixels holding 254 and 253) at unaligned columns and across tile borders."""
    lm_checks.check_render_wraparound(hip_lib)


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("name", ["k7_70x94", "k3_135x240", "k7_66x130_wide"])
def test_fcn_golden(hip_lib, name, precision):
    """FCN-LectureNet forward (MFMA conv stack, both operand precisions) vs the reference module: max |logit diff| <= 1e-3
    required by BASELINE.json; 1e-4 demanded here."""
    assert lm_checks.check_fcn_golden(hip_lib, name, precision=precision) < 1e-4


@pytest.mark.parametrize("precision,tol", [("mixed", 5e-4), ("planar-f16x3", 1e-5), ("planar-f16", 1e-3)])
def test_fcn_golden_planar_engine(hip_lib, precision, tol):
    """The DEFAULT engine (csrc/lm_fcn2.hip, the one bench.py times) against the reference module's own outputs: G5's wide case has every
    width a multiple of 16, so the planar engine takes it.  mixed = the shipped per-layer format assignment."""
    assert lm_checks.check_fcn_golden(hip_lib, "k7_66x130_wide", tol=tol, precision=precision, require_planar=True) <= tol


@pytest.mark.parametrize("precision", ["mixed", "planar-f16x3", "f16x3", "fp32"])
def test_fcn_shipped_config_vs_oracle(hip_lib, precision):
    """The shipped network widths (configs/FCN_LectureNet.conf:109-132, 15.8 M parameters, 7x7 pixel convs) on an
    odd-sized 270x478 frame (exercises every output_size padding) against the torch fp32 oracle."""
    import torch
    from lecturemath_amd import fcn
    from oracle import fcn as ofcn
    sd = ofcn.random_state_dict(ofcn.SHIPPED_WIDTHS, pixel_kernel=7, seed=0)
    rgb, _ = synth.whiteboard_rgb(270, 478, n_glyphs=120, seed=4)
    eng = fcn.FcnEngine(ofcn.SHIPPED_WIDTHS, 7, 3, 270, 478, hip_lib, precision=precision)
    eng.load_state_dict(sd)
    out, text, rec = (t.cpu().numpy() for t in eng.forward(rgb))
    with torch.no_grad():
        o, t, r = ofcn.forward(sd, ofcn.prepare_image(rgb))
    assert np.abs(out - o[0, 0].numpy()).max() <= 1e-3
    assert np.abs(text - t[0, 0].numpy()).max() <= 1e-3
    assert np.abs(rec - r[0].numpy()).max() <= 1e-3
    eng.close()


@pytest.fixture(scope="module")
def fcn_1080p_oracle():
    """Shipped widths, one 1920x1080 frame through the torch fp32 oracle (all host cores; once per test module)."""
    import torch
    from oracle import fcn as ofcn
    sd = ofcn.random_state_dict(ofcn.SHIPPED_WIDTHS, pixel_kernel=7, seed=0)
    rgb, _ = synth.whiteboard_rgb(1080, 1920, 1500, seed=20211)
    torch.set_num_threads(os.cpu_count())
    with torch.no_grad():
        o, t, r = ofcn.forward(sd, ofcn.prepare_image(rgb))
    return sd, rgb, o[0, 0].numpy(), t[0, 0].numpy(), r[0].numpy()


@pytest.mark.parametrize("precision,tol", [("mixed", 2.5e-4), ("planar-f16x3", 1e-5), ("planar-f16", 1e-3), ("f16x3", 1e-4), ("fp32", 1e-4), ("f16x2", 1e-3),
                                           ("f16", 1e-3)])
def test_fcn_shipped_config_1080p_vs_oracle(hip_lib, fcn_1080p_oracle, precision, tol):
    """BASELINE configs[1] at its size: the shipped network on one 1920x1080 frame against the oracle.  The bar is 1e-3 on the
    logits (north_star); the default ("mixed": the planar engine with its per-layer operand formats, chosen in round 4 by measured error AND
    binary flips, profiles/r04_fcn_formats.*) is held to 2.5e-4, the all-split formats of both engines and fp32 to 1e-4 or tighter, the
    cheaper operand formats to the bar itself.  For the default the BINARY FLIPS against the oracle's binarization are counted too:
    random-init logits crowd the threshold (std 0.12 here), 392 of 2,073,600 pixels flip in this frame."""
    from lecturemath_amd import fcn
    sd, rgb, o, t, r = fcn_1080p_oracle
    eng = fcn.FcnEngine(synth.FCN_SHIPPED_WIDTHS, 7, 3, 1080, 1920, hip_lib, precision=precision)
    eng.load_state_dict(sd)
    out, text, rec = (x.cpu().numpy() for x in eng.forward(rgb))
    eng.close()
    aux = 2 * tol if precision == "mixed" else tol       # text-mask logit / reconstruction (their head runs on two products: 2.5e-4 / 2.9e-4 measured)
    assert np.abs(out - o).max() <= tol and np.abs(text - t).max() <= aux and np.abs(rec - r).max() <= aux
    if precision == "mixed":
        from oracle import cc as occ
        flips = int((occ.threshold_invert(out) != occ.threshold_invert(o)).sum())
        band = int((np.abs(o - 0.0078433) < tol).sum())           # a pixel can only flip where the oracle's logit is within the engine's error of the edge
        assert flips <= 600 and flips <= band, (flips, band)


def test_fcn_planar_frame_size_change(hip_lib):
    """One planar engine, frames of different sizes one after the other (the zero halos and the tile overhang of its activation
    planes depend on the frame size): every pass within 5e-4 of the oracle (the shipped format assignment; bar 1e-3), and the first size again gives its first result bit for bit."""
    import torch
    from lecturemath_amd import fcn
    from oracle import fcn as ofcn
    sd = ofcn.random_state_dict(ofcn.SHIPPED_WIDTHS, pixel_kernel=7, seed=3)
    eng = fcn.FcnEngine(ofcn.SHIPPED_WIDTHS, 7, 3, 272, 480, hip_lib)
    assert eng.planar
    eng.load_state_dict(sd)
    first = None
    for k, (h, w) in enumerate(((272, 480), (135, 241), (201, 333), (272, 480))):
        rgb, _ = synth.whiteboard_rgb(272, 480, n_glyphs=100, seed=9)
        rgb = np.ascontiguousarray(rgb[:h, :w])
        out, text, rec = (x.cpu().numpy() for x in eng.forward(rgb))
        with torch.no_grad():
            o, t, r = ofcn.forward(sd, ofcn.prepare_image(rgb))
        assert np.abs(out - o[0, 0].numpy()).max() <= 5e-4 and np.abs(text - t[0, 0].numpy()).max() <= 5e-4 and np.abs(rec - r[0].numpy()).max() <= 5e-4, (h, w)
        if k == 0:
            first = out
    assert (first == out).all()
    eng.close()


@pytest.mark.parametrize("precision", ["mixed", "f16x3"])
def test_fcn_two_engines_on_two_streams(hip_lib, fcn_1080p_oracle, precision):
    """Two engines fed from two HIP streams at 1080p, their forward passes really overlapping on the device (nothing in the
    library serialises them), give the single-pass logits -- themselves within 2.5e-4 (mixed) / 1e-4 of the oracle -- bit for bit, pass after
    pass.  Round 1 saw sporadic 1e-3..2e-2 errors in the one-channel heads here (packed-fp32 code)."""
    import torch
    from lecturemath_amd import fcn
    sd, rgb, o, t, r = fcn_1080p_oracle
    h, w = 1080, 1920
    engines = []
    for _ in range(2):
        e = fcn.FcnEngine(synth.FCN_SHIPPED_WIDTHS, 7, 3, h, w, hip_lib, precision=precision)
        e.load_state_dict(sd)
        engines.append(e)
    d = torch.from_numpy(rgb).cuda()
    gold = [x.clone() for x in engines[0].forward(d)]
    tol = 2.5e-4 if precision == "mixed" else 1e-4
    assert float(np.abs(gold[0].cpu().numpy() - o).max()) <= tol and float(np.abs(gold[1].cpu().numpy() - t).max()) <= 2 * tol
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for _ in range(10):
        res = []
        for e, st in zip(engines, streams):
            with torch.cuda.stream(st):
                res.append(e.forward(d))
        torch.cuda.synchronize()
        for rr in res:
            for a, b in zip(gold, rr):
                assert bool((a == b).all())
    for e in engines:
        e.close()


def test_e2e_rgb_binarization_and_cc_sets(hip_lib, oracle_built, fcn_1080p_oracle):
    """The FCN -> CC composition ("report flip counts"): RGB 1080p frames -> HIP network (default engine and format
    assignment) -> fused threshold + labelling in the production loop (lm_stream_run_logits), against oracle/fcn.py -> oracle threshold ->
    oracle labelling (labeler.py:126 / FCN_lecturenet.py:461-467).  Binary pixels may differ only where the oracle's logit is within the
    engine's error bound of the threshold; the flips are counted; and every connected component of the oracle's labelling that no
    flipped pixel touches (4-neighbourhood) must be one connected component of the device's labelling, pixel for pixel."""
    import torch
    from lecturemath_amd import _lib, fcn
    from oracle import fcn as ofcn
    occ = oracle_built
    sd, rgb0, o0, _, _ = fcn_1080p_oracle
    H, W = 1080, 1920
    rgb1, _ = synth.whiteboard_rgb(H, W, 900, seed=7)
    torch.set_num_threads(os.cpu_count())
    with torch.no_grad():
        o1 = ofcn.forward(sd, ofcn.prepare_image(rgb1))[0][0, 0].numpy()
    frames, oracle_logits = [rgb0, rgb1], [o0, o1]
    eng = fcn.FcnEngine(synth.FCN_SHIPPED_WIDTHS, 7, 3, H, W, hip_lib)
    eng.load_state_dict(sd)
    logits = torch.empty((2, H, W), dtype=torch.float32, device="cuda")
    for i, f in enumerate(frames):
        eng.forward_raw(_lib.ptr(torch.from_numpy(f).cuda()), H, W, _lib.ptr(logits[i]), None, None)
    fs = device.FrameStream(W, H, 2, 0.85, 0.85, 85, 20, max_batch=2, max_ccs=2 * 262144, max_crop_words=2 * (1 << 21), lib=hip_lib)
    labels = torch.empty((2, H, W), dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    hip_lib.check(hip_lib.lm_stream_run_logits(fs.handle, _lib.ptr(logits), 2, 2, None, _lib.ptr(labels), 128, 1, 0, st, st))
    torch.cuda.synchronize()
    dl = labels.cpu().numpy()
    total_flips = 0
    for i in range(2):
        ob = occ.threshold_invert(oracle_logits[i])             # ink = 255
        db = np.where(dl[i] > 0, 255, 0).astype(np.uint8)
        flip = ob != db
        band = np.abs(oracle_logits[i] - 0.0078433) < 2.5e-4
        assert not (flip & ~band).any(), "binary pixels differ outside the engine's error band around the threshold"
        nflip = int(flip.sum())
        total_flips += nflip
        ol, n_o = occ.label4(ob)
        assert n_o > 0
        touched = flip.copy()                                   # flipped pixels and their 4-neighbours
        touched[1:] |= flip[:-1]; touched[:-1] |= flip[1:]; touched[:, 1:] |= flip[:, :-1]; touched[:, :-1] |= flip[:, 1:]
        dirty = np.zeros(n_o + 1, bool)
        dirty[np.unique(ol[touched])] = True
        ink = ol > 0
        pairs = np.unique(np.stack([ol[ink], dl[i][ink]], 1), axis=0)      # (oracle CC, device CC) pairs that share a pixel
        clean = pairs[~dirty[pairs[:, 0]]]
        assert (clean[:, 1] > 0).all()                                      # every pixel of a clean oracle CC is ink on the device
        assert len(np.unique(clean[:, 0])) == len(clean), "a clean oracle CC is split on the device"
        size_o, size_d = np.bincount(ol.ravel(), minlength=n_o + 1), np.bincount(dl[i].ravel())
        assert (size_o[clean[:, 0]] == size_d[clean[:, 1]]).all(), "a clean oracle CC is part of a larger device CC"
        print("frame %d: %d CCs, %d flipped pixels, %d CCs touched by a flip, %d compared pixel for pixel" % (i, n_o, nflip, int(dirty[1:].sum()), len(clean)))
    assert total_flips <= 1200, total_flips
    fs.close()
    eng.close()


@pytest.mark.parametrize("fused", ["0", "3"])
def test_fcn_head_variants_vs_oracle(hip_lib, monkeypatch, fused):
    """The heads' other code paths (default: text / rec head fused with its vertical sums, output head as rows + lm_k_vsum): nothing fused
    (row buffer + lm_k_vsum2_text_rec + lm_k_vsum) and both fused, on an odd-sized frame (tiles of 10 finished rows against a height that
    is no multiple of 10 or 16) against the torch oracle."""
    import torch
    from lecturemath_amd import fcn
    from oracle import fcn as ofcn
    monkeypatch.setenv("LM_FCN2_FUSED_HEADS", fused)
    sd = ofcn.random_state_dict(ofcn.SHIPPED_WIDTHS, pixel_kernel=7, seed=2)
    rgb, _ = synth.whiteboard_rgb(203, 331, n_glyphs=80, seed=6)
    eng = fcn.FcnEngine(ofcn.SHIPPED_WIDTHS, 7, 3, 203, 331, hip_lib)
    eng.load_state_dict(sd)
    assert eng.planar and (eng.recipes[16]["epilogue"] == 4) == (fused == "3") and (eng.recipes[20]["epilogue"] == 4) == (fused == "3")
    out, text, rec = (t.cpu().numpy() for t in eng.forward(rgb))
    eng.close()
    with torch.no_grad():
        o, t, r = ofcn.forward(sd, ofcn.prepare_image(rgb))
    assert np.abs(out - o[0, 0].numpy()).max() <= 5e-4 and np.abs(text - t[0, 0].numpy()).max() <= 5e-4 and np.abs(rec - r[0].numpy()).max() <= 5e-4
