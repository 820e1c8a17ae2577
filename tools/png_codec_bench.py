"""Throughput of the device PNG hand-off codec (csrc/lm_png.hip) beside host zlib (lecturemath_amd/png.py) on the same machine.

    python tools/png_codec_bench.py [--sizes 1080p,4k] [--batch 64] [--reps 5] [--host-frames 16] [--out result.json]
    python tools/png_codec_bench.py --kernel-share <rocprofv3 results .db> [--out share.json]

Frames are synth.binary_stream frames (the step-01 worker's inverted binary, ink = 255).  Per size it reports frames/s of
  device encode:  lm_png_encode on a device batch (kernels only, HIP events), and encode_gray8_device end to end (+ pack + D2H)
  device decode:  lm_png_decode of a device-resident batch (kernels only), and decode_gray8_device end to end (H2D + kernels)
  host:           png.encode_gray8 / png.decode_gray8 on one core
plus mean file sizes, and checks every device file against host decode and every device decode against the input.
The second form sums a `rocprofv3 --kernel-trace --stats` run of the first into the share of GPU time per kernel.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

SIZES = {"1080p": (1080, 1920), "4k": (2160, 3840)}


def frames_for(h, w, n):
    from lecturemath_amd import synth
    # one stream of distinct frames (text added every other frame), tiled to n
    base = np.stack(list(synth.binary_stream(min(n, 16), h, w, seed=20213)))
    return np.ascontiguousarray(base[np.arange(n) % len(base)])


def bench_size(name, h, w, batch, reps, host_frames):
    import torch
    from lecturemath_amd import _lib, png, png_device
    lib = _lib.load()
    codec = png_device.PngCodec(w, h, batch, lib)
    frames = frames_for(h, w, batch)
    d_frames = torch.from_numpy(frames).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    # correctness of this batch first
    files = codec.encode(d_frames)
    for i in range(0, batch, max(1, batch // 8)):
        assert (png.decode_gray8(files[i]) == frames[i]).all(), "device file %d does not decode to its frame" % i
    dec = codec.decode(files)
    assert (dec.cpu().numpy() == frames).all(), "device decode mismatch"

    def kernels_ms(fn):
        fn()
        torch.cuda.synchronize()
        ev0.record()
        for _ in range(reps):
            fn()
        ev1.record()
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1) / reps

    enc_ms = kernels_ms(lambda: lib.check(lib.lm_png_encode(codec.h, d_frames.data_ptr(), batch, codec._slots.data_ptr(), codec.bound,
                                                            codec._sizes.data_ptr(), stream)))
    lens = np.asarray([len(f) for f in files], np.int64)
    offs = np.zeros(batch, np.int64)
    np.cumsum(lens[:-1], out=offs[1:])
    d_files = torch.from_numpy(np.concatenate(files)).cuda()
    d_offs, d_lens = torch.from_numpy(offs).cuda(), torch.from_numpy(lens).cuda()
    d_out = torch.empty((batch, h, w), dtype=torch.uint8, device="cuda")
    d_st = torch.empty((batch,), dtype=torch.int32, device="cuda")
    dec_ms = kernels_ms(lambda: lib.check(lib.lm_png_decode(codec.h, d_files.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), batch, d_out.data_ptr(),
                                                            d_st.data_ptr(), stream)))
    assert (d_st.cpu().numpy() == 0).all() and (d_out.cpu().numpy() == frames).all()

    def wall_ms(fn):
        fn()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3 / reps

    enc_e2e_ms = wall_ms(lambda: codec.encode(d_frames))
    dec_e2e_ms = wall_ms(lambda: codec.decode(files))

    k = min(host_frames, batch)
    t = time.perf_counter()
    host_files = [png.encode_gray8(frames[i]) for i in range(k)]
    host_enc_ms = (time.perf_counter() - t) * 1e3 / k
    t = time.perf_counter()
    for f in host_files:
        png.decode_gray8(f)
    host_dec_ms = (time.perf_counter() - t) * 1e3 / k
    codec.close()
    fps = lambda ms_per_batch, nb=batch: round(nb * 1e3 / ms_per_batch, 1)   # noqa: E731
    return {
        "size": name, "height": h, "width": w, "batch": batch, "ink_fraction": round(float((frames > 0).mean()), 4),
        "device_encode_kernels_fps": fps(enc_ms), "device_encode_kernels_ms_per_batch": round(enc_ms, 3),
        "device_encode_e2e_fps": fps(enc_e2e_ms),
        "device_decode_kernels_fps": fps(dec_ms), "device_decode_kernels_ms_per_batch": round(dec_ms, 3),
        "device_decode_e2e_fps": fps(dec_e2e_ms),
        "host_encode_fps_per_core": round(1e3 / host_enc_ms, 1), "host_decode_fps_per_core": round(1e3 / host_dec_ms, 1),
        "device_mean_bytes": round(float(lens.mean()), 1), "host_mean_bytes": round(float(np.mean([len(f) for f in host_files])), 1),
        "device_encode_input_GBps": round(batch * h * w / enc_ms / 1e6, 2),
    }


def kernel_share(db_path):
    import sqlite3
    db = sqlite3.connect(db_path)
    rows = db.execute("select name, count(*), sum(end - start) from kernels group by name order by 3 desc").fetchall()
    tot = sum(r[2] for r in rows) or 1
    png_tot = sum(r[2] for r in rows if "lm_k_png" in r[0])
    return {"kernels": [{"name": r[0].split("(")[0], "calls": r[1], "total_ns": int(r[2]), "percent": round(100.0 * r[2] / tot, 2)} for r in rows],
            "png_kernels_percent_of_gpu_time": round(100.0 * png_tot / tot, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1080p,4k")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-frames", type=int, default=16)
    ap.add_argument("--kernel-share", default=None, help="rocprofv3 results .db of a run of this tool")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.kernel_share:
        res = kernel_share(a.kernel_share)
    else:
        res = {"results": [bench_size(s, *SIZES[s], a.batch, a.reps, a.host_frames) for s in a.sizes.split(",")]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
