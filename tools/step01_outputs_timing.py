"""What step 01's outputs cost: lm_fcn_bytes alone, and binarize() / the worker's handleFrame() against another build of the tree.

    python tools/step01_outputs_timing.py --against PATH_OF_THE_PARENT_COMMITS_TREE [--out profiles/r09_step01_outputs.json]

Workload: the shipped widths at 1920x1080, random-init weights as `bench.py --workload fcn` builds them (synth.fcn_random_state_dict,
seed 0), whiteboard frames from synth.whiteboard_rgb.

  kernel   one child process: lm_fcn_bytes on the heads of one frame, all three pairs, hard and soft -- HIP events over 200 launches
           after 20 warm-up launches; bytes/s against the algorithmic 25 B/px.  In the same run lm_threshold on one plane (the
           comparison kernel lm_k_threshold_cmp, 5 B/px) and the two lm_threshold launches lm_fcn_bytes replaces.
  calls    fresh child processes, this tree and the tree given with --against alternating (so one heap does not serve both), each
           importing lecturemath_amd and the drop-in overlay from ITS tree: binarize(return_others=True, force_binary=True) per call and
           worker.handleFrame per frame under LM_PNG_CODEC=host and =device -- host clock around calls that end in the device-to-host
           copy, 2 warm-ups, then `--repeats` (default 9) calls; and SHA-256 of binary, text_mask and rec_img of three seeded frames.
The change counts as faster only where its median lies below the other tree's median minus that tree's min-max spread.  Every child
runs under a time limit; after a child that fails or runs out of time nothing more is started.  Needs the GPU and both trees built."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1920, 1080
FRAME_SEEDS = (20211, 20212, 20213)


def network(root):
    """(net, synth, lib) of the tree at `root`"""
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "lecturemath_amd", "dropin"))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("step01_outputs_timing: needs a GPU")
    from lecturemath_amd import _lib, fcn, synth
    assert os.path.dirname(os.path.abspath(_lib.__file__)) == os.path.join(os.path.abspath(root), "lecturemath_amd")
    from AM_CommonTools.configuration.configuration import Configuration
    from AccessMath.lecturenet_v1.FCN_lecturenet import FCN_LectureNet
    conf = Configuration({key: str(v) for (key, _), v in zip(fcn.WIDTH_KEYS, synth.FCN_SHIPPED_WIDTHS)})
    conf.set("FCN_BINARIZER_NET_PIXEL_KERNEL_SIZE", "7")
    net = FCN_LectureNet.CreateFromConfig(conf, 3, False)
    net.load_state_dict(synth.fcn_random_state_dict(synth.FCN_SHIPPED_WIDTHS, pixel_kernel=7, seed=0))
    return net.eval().cuda(), synth, _lib.load()


def summary(v, scale=1.0):
    return {"median": statistics.median(v) * scale, "min": min(v) * scale, "max": max(v) * scale, "n": len(v)}


def child_kernel():
    import numpy as np
    import torch
    net, synth, lib = network(ROOT)
    from lecturemath_amd import _lib
    rgb, _ = synth.whiteboard_rgb(H, W, 1500, seed=FRAME_SEEDS[0])
    out, text, rec = net.forward_logits(rgb)
    n = H * W
    dst = torch.empty(5 * n, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    p = _lib.ptr

    def timed(fn, launches=200, warmup=20):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / launches

    def fcn_bytes(flags):
        lib.check(lib.lm_fcn_bytes(p(out), p(text), p(rec), n, 128, flags, p(dst), p(dst) + n, p(dst) + 2 * n, st))

    def threshold(src, off):
        lib.check(lib.lm_threshold(p(src), p(dst) + off, n, 128, 0, st))

    res = {"launches": 200, "warmup": 20, "bytes_per_frame_fcn_bytes": 25 * n, "bytes_per_plane_threshold": 5 * n}
    for name, fn, nbytes in (("fcn_bytes_hard", lambda: fcn_bytes(0), 25 * n), ("fcn_bytes_soft", lambda: fcn_bytes(_lib.LM_FB_SOFT), 25 * n),
                             ("threshold_one_plane", lambda: threshold(out, 0), 5 * n),
                             ("threshold_two_launches", lambda: (threshold(out, 0), threshold(text, n)), 10 * n)):
        reps = [timed(fn) for _ in range(3)]
        res[name] = {"us_per_call": summary(reps, 1e6), "bytes_per_s": nbytes / statistics.median(reps)}
    # the outputs of the timed size against the numpy restatement of the reconstruction and lm_threshold
    fcn_bytes(0)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    v = rec.cpu().numpy().astype(np.float32)
    v *= np.float32(0.5)
    v += np.float32(0.5)
    v *= np.float32(255)
    want_rec = np.clip(v, 0, 255).astype(np.uint8).transpose(1, 2, 0)[:, :, ::-1]
    ref = torch.empty(n, dtype=torch.uint8, device="cuda")
    lib.check(lib.lm_threshold(p(out), p(ref), n, 128, 0, st))
    res["outputs_equal_restatement"] = bool((got[2 * n:].reshape(H, W, 3) == want_rec).all() and (got[:n] == ref.cpu().numpy()).all())
    print("RESULT " + json.dumps(res))


def child_calls(root, repeats):
    import numpy as np
    import PIL.Image
    import torch
    net, synth, lib = network(root)
    from AccessMath.preprocessing.video_worker.FCN_lecturenet_binarizer import FCN_LectureNet_Binarizer
    frames = [synth.whiteboard_rgb(H, W, 1500, seed=s)[0] for s in FRAME_SEEDS]
    res = {"device_route": hasattr(net, "binarize_device"), "repeats": repeats, "warmup": 2, "sha256": []}
    for rgb in frames:
        b, t, r = net.binarize(PIL.Image.fromarray(rgb), return_others=True, force_binary=True)
        res["sha256"].append([hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() for a in (b, t, r)])
    pil = PIL.Image.fromarray(frames[0])
    bgr = np.ascontiguousarray(frames[0][:, :, ::-1])

    def clock(fn):
        v = []
        for k in range(2 + repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            if k >= 2:
                v.append(time.perf_counter() - t0)
        return summary(v, 1e3)

    res["binarize_ms"] = clock(lambda: net.binarize(pil, return_others=True, force_binary=True))
    for codec in ("host", "device"):
        os.environ["LM_PNG_CODEC"] = codec
        worker = FCN_LectureNet_Binarizer(net)
        worker.initialize(W, H)
        res["handle_frame_%s_codec_ms" % codec] = clock(lambda: worker.handleFrame(bgr, None, 0, 0.0, 0.0, 0))
    print("RESULT " + json.dumps(res))


def run_child(args, limit):
    """one child under its time limit -> its RESULT; SystemExit (nothing more is started) when it fails or runs out of time"""
    proc = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit)
    if proc.returncode != 0:
        sys.stderr.write(proc.stdout[-2000:] + proc.stderr[-4000:])
        raise SystemExit("step01_outputs_timing: child %r ended with status %d; stopping" % (args, proc.returncode))
    return json.loads([ln for ln in proc.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--against", default=None, help="a built tree of the commit to compare with")
    ap.add_argument("--against-name", default=None, help="what that tree is, for the record (e.g. the commit)")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=2, help="child processes per tree, the trees alternating")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_step01_outputs.json"))
    ap.add_argument("--child", choices=("kernel", "calls"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child == "kernel":
        return child_kernel()
    if a.child == "calls":
        return child_calls(a.root, a.repeats)
    result = {"width": W, "height": H, "frame_seeds": list(FRAME_SEEDS), "kernel": run_child(["--child", "kernel"], 240)}
    print(json.dumps(result["kernel"], indent=1), flush=True)
    trees = {"this": ROOT}
    if a.against:
        trees["against"] = os.path.abspath(a.against)
    runs = {k: [] for k in trees}
    for _ in range(a.rounds):
        for name, root in trees.items():
            runs[name].append(dict(run_child(["--child", "calls", "--root", root, "--repeats", str(a.repeats)], 300), tree=name))
            print(name, json.dumps(runs[name][-1]), flush=True)
    result["calls"] = runs
    if a.against:
        result["against"] = a.against_name or os.path.basename(os.path.abspath(a.against))
        result["outputs_equal_across_trees"] = all(r["sha256"] == runs["this"][0]["sha256"] for rs in runs.values() for r in rs)
        verdict = {}
        for key in ("binarize_ms", "handle_frame_host_codec_ms", "handle_frame_device_codec_ms"):
            new = statistics.median(r[key]["median"] for r in runs["this"])
            old = statistics.median(r[key]["median"] for r in runs["against"])
            spread = max(r[key]["max"] for r in runs["against"]) - min(r[key]["min"] for r in runs["against"])
            verdict[key] = {"this_median_ms": new, "against_median_ms": old, "against_min_max_spread_ms": spread, "faster": bool(new < old - spread)}
        result["verdict"] = verdict
        print(json.dumps(verdict, indent=1))
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
