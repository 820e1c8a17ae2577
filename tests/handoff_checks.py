"""Single-process edge checks of the stream hand-off ABI (lm_stream_pack_size / lm_stream_pack / lm_stream_append_packed,
lm_stream_assign_bytes / lm_stream_export_assign / lm_stream_import_assign, lm_stream_import / lm_stream_read), shared by the GPU
tests (real HIP library) and the CPU logic tests (emulated build).  The two-process tests (test_sharded_*.py) move one short
stream whose every piece has ink; here one handle pair in one process takes the edges real runs hit: blocks of more than 1024
frames, empty blocks, blocks of blank frames, the bytes on the wire against an independent statement of their layout, and every
refusal with the stream still usable afterwards.  References: the single-process stream (FrameStream.push of all frames) and, for
the short streams, the oracle (oracle.cc.Stability)."""
import ctypes

import numpy as np

import lm_checks
from lecturemath_amd import _lib, device, digests

PACK_MAGIC = 0x4c4d504b31       # "LMPK1"
# one packed record; 32 bytes without holes
REC = np.dtype([("cc_id", "<i4"), ("size", "<i4"), ("min_x", "<i2"), ("max_x", "<i2"), ("min_y", "<i2"), ("max_y", "<i2"),
                ("crop_off", "<u8"), ("frame", "<i4"), ("pad", "<i4")])
assert REC.itemsize == 32
SCALARS = ("n_frames", "n_cc", "n_crop_words", "n_unique", "tempo_count")
GAP = 5


# ------------------------------------------------------------------------------------------------
# input streams
# ------------------------------------------------------------------------------------------------
def square_stream(n_frames, h, w, seed=7, cells=10, mean_gap=3, max_len=12, blanks=(), always=()):
    """5x5 ink squares (25 px >= min_pixels 20), each in a grid cell of its own, that appear and disappear over frame ranges.
    One in three stays identical while it lives (exact twins across frames), one in three carries a tail of 0..2 px that changes
    every frame (versions that differ and still match: 25 of 27 px), one in three blinks every other frame (gaps inside
    max_gap).  The frames listed in `blanks` are cleared."""
    rng = np.random.default_rng(seed)
    gy, gx = (h - 2) // 8, (w - 2) // 8
    frames = np.zeros((n_frames, h, w), np.uint8)
    assert cells + 1 <= gy * gx
    picked = rng.choice(gy * gx, size=cells + 1, replace=False)
    y, x = 1 + 8 * (int(picked[-1]) // gx), 1 + 8 * (int(picked[-1]) % gx)
    for lo, hi in always:                                       # a cell of its own for ink that must be there: frames [lo, hi)
        frames[lo:hi, y:y + 5, x:x + 5] = 255
    for k, c in enumerate(picked[:-1]):
        y, x = 1 + 8 * (int(c) // gx), 1 + 8 * (int(c) % gx)
        t = int(rng.integers(0, mean_gap + 1))
        kind = k
        while t < n_frames:
            ln = int(rng.integers(2, max_len + 1))
            for f in range(t, min(t + ln, n_frames)):
                if kind % 3 == 2 and (f - t) % 2:
                    continue
                frames[f, y:y + 5, x:x + 5] = 255
                if kind % 3 == 1:
                    frames[f, y + 2, x + 5:x + 5 + (f - t) % 3] = 255
            t += ln + int(rng.integers(1, 2 * mean_gap + 1))
            kind += 1
    for b in blanks:
        frames[b] = 0
    return frames


def short_stream(h, w, n_frames=48):
    """The stream of the short checks: blank frames 0, 1, 20..22 (a block of blank frames only), 31 and the last."""
    blanks = (0, 1, 20, 21, 22, 31, n_frames - 1)
    return square_stream(n_frames, h, w, seed=7, blanks=blanks), blanks


def hopping_stream(n_frames, h, w):
    """Exactly one CC in every frame; it moves to another cell every second frame: assign = 0, 0, 1, 1, 2, 2, ..."""
    gx = (w - 2) // 8
    frames = np.zeros((n_frames, h, w), np.uint8)
    for f in range(n_frames):
        c = f // 2
        y, x = 1 + 8 * ((c // gx) % ((h - 2) // 8)), 1 + 8 * (c % gx)
        frames[f, y:y + 5, x:x + 5] = 255
    return frames


def make(lib, h, w, max_frames, max_batch=16, **kw):
    return device.FrameStream(w, h, max_frames, 0.85, 0.85, GAP, 20, max_batch=max_batch, lib=lib, **kw)


def pushed(lib, frames, max_batch=16, records_only=False, **kw):
    n, h, w = frames.shape
    fs = make(lib, h, w, n, max_batch, **kw)
    dev = fs.be.from_host(frames)
    (fs.push_records if records_only else fs.push)(dev)
    return fs


def oracle_result(frames):
    from oracle import cc as occ
    _, h, w = frames.shape
    st = occ.Stability(w, h, 0.85, 0.85, GAP)
    for f in frames:
        st.add_frame(f)
    return st.result()


# ------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------
def same_state(got, ref, active=True, what=""):
    """Two FrameStream.read() results: the counters, every record (with its unique index), the offsets, the crop words and,
    unless the path documents that it stays behind, the active list."""
    for key in SCALARS:
        assert got[key] == ref[key], (what, key, got[key], ref[key])
    for key in ("rec", "frame_off", "crop_off") + (("active",) if active else ()):
        assert got[key].shape == ref[key].shape and (got[key] == ref[key]).all(), (what, key)
    n = ref["n_crop_words"]
    assert (got["crop"][:n] == ref["crop"][:n]).all(), (what, "crop")


def to_backend(be, host_bytes):
    """A uint8 host array in a backend buffer (32-byte aligned, which a plain numpy copy is not)."""
    buf = be.empty((len(host_bytes),), np.uint8)
    if be.device:
        buf.copy_(be.torch.from_numpy(np.ascontiguousarray(host_bytes)))
    else:
        buf[...] = host_bytes
    return buf


def pack_size(lib, fs, first, n):
    nb = ctypes.c_int64(-1)
    rc = lib.lm_stream_pack_size(fs.handle, int(first), int(n), ctypes.addressof(nb), fs.be.stream())
    return rc, int(nb.value)


def expected_block(r, first, n):
    """The packed block of frames [first, first + n) restated in numpy from a FrameStream.read() result."""
    foff = r["frame_off"]
    c0, c1 = int(foff[first]), int(foff[first + n])
    w0 = w1 = 0
    if c1 > c0:
        w0 = int(r["crop_off"][c0])
        w1 = int(r["crop_off"][c1]) if c1 < r["n_cc"] else r["n_crop_words"]
    head = np.array([n, c1 - c0, w1 - w0, PACK_MAGIC], "<i8")
    counts = np.zeros((n + 3) & ~3, "<i8")                      # the padding entries are zero
    counts[:n] = np.diff(foff[first:first + n + 1])
    rec = np.zeros(c1 - c0, REC)
    src = r["rec"][c0:c1]
    rec["cc_id"], rec["size"], rec["frame"] = src[:, 0], src[:, 5], src[:, 6] - first
    rec["min_x"], rec["max_x"], rec["min_y"], rec["max_y"] = src[:, 1], src[:, 2], src[:, 3], src[:, 4]
    rec["crop_off"] = r["crop_off"][c0:c1] - w0
    words = np.asarray(r["crop"][w0:w1], "<u4")
    return np.concatenate([head.view(np.uint8), counts.view(np.uint8), rec.view(np.uint8), words.view(np.uint8)])


def expected_assign(r):
    """The assignment buffer restated from a FrameStream.read() result of a matched stream."""
    a = np.ascontiguousarray(r["rec"][:, 7], "<i4").view(np.uint8)
    pad = np.zeros((-len(a)) % 32, np.uint8)
    tail = np.array([r["n_cc"], r["n_unique"], r["tempo_count"], r["n_frames"]], "<i8").view(np.uint8)
    return np.concatenate([a, pad, tail])


# ------------------------------------------------------------------------------------------------
# 1, 2: the bytes
# ------------------------------------------------------------------------------------------------
def check_block_layout(lib, h, w):
    frames, blanks = short_stream(h, w)
    F = len(frames)
    for records_only in (True, False):                          # the sender of raw records, and the matched stream of the hand-off
        fs = pushed(lib, frames, records_only=records_only)
        try:
            r = fs.read()
            assert r["n_cc"] > F and r["n_crop_words"] > r["n_cc"]
            for first, n in ((0, F), (20, 9), (0, 0), (7, 0), (F, 0), (5, 1), (31, 1), (F - 1, 1), (20, 3), (0, 2), (19, 5), (3, 6)):
                exp = expected_block(r, first, n)
                rc, nb = pack_size(lib, fs, first, n)
                assert rc == _lib.LM_OK and nb == len(exp), (first, n, rc, nb, len(exp))
                got = fs.be.to_host(fs.pack(first, n))
                assert got.dtype == np.uint8 and len(got) == len(exp), (first, n)
                diff = np.flatnonzero(got != exp)
                assert len(diff) == 0, "block (%d, %d): %d bytes differ, the first at %d" % (first, n, len(diff), diff[0])
            assert (np.diff(r["frame_off"])[list(blanks)] == 0).all()
        finally:
            fs.close()


def check_assign_layout(lib, h, w):
    fs = make(lib, h, w, 16, max_batch=16, max_ccs=4096, max_crop_words=1 << 16)
    try:
        for n in (16, 15, 9, 8):                                # the longer stream first: its tail would show behind the shorter one's
            fs.reset()
            fs.push(fs.be.from_host(hopping_stream(16, h, w)[:n]))
            r = fs.read()
            assert r["n_cc"] == n and r["n_unique"] == (n + 1) // 2 and list(r["rec"][:, 7]) == [f // 2 for f in range(n)]
            exp = expected_assign(r)
            nb = ctypes.c_int64(-1)
            assert lib.lm_stream_assign_bytes(fs.handle, ctypes.addressof(nb), fs.be.stream()) == _lib.LM_OK and nb.value == len(exp)
            got = fs.be.to_host(fs.export_assign())
            assert len(got) == len(exp) and len(exp) == ((4 * n + 31) & ~31) + 32
            diff = np.flatnonzero(got != exp)
            assert len(diff) == 0, "assignment of %d CCs: %d bytes differ, the first at %d" % (n, len(diff), diff[0])
    finally:
        fs.close()


# ------------------------------------------------------------------------------------------------
# 3, 4: round trips at cut lists
# ------------------------------------------------------------------------------------------------
def round_trip(src, dst, cuts):
    for a, b in zip(cuts[:-1], cuts[1:]):
        dst.append_packed(src.pack(a, b - a))
        dst.match(b - a)


def short_cut_lists(F, blanks):
    mid = [b for b in blanks if 1 < b < F - 1]
    run0, run1 = mid[0], mid[0]
    while run1 + 1 in mid:
        run1 += 1
    lone = [b for b in mid if b - 1 not in mid and b + 1 not in mid][0]
    return {
        "empty blocks first, middle and last": (0, 0, 7, 7, F, F),
        "single frames": tuple(range(F + 1)),
        "a block of blank frames only": (0, run0, run1 + 1, F),
        "cuts before and after a blank frame": (0, lone, lone + 1, F),
        "cuts inside the leading and trailing blanks": (0, 1, 2, F - 1, F),
        "even 16s": tuple(range(0, F, 16)) + (F,),
    }


def check_round_trips(lib, h, w, with_oracle=True):
    frames, blanks = short_stream(h, w)
    F = len(frames)
    single, src = pushed(lib, frames), pushed(lib, frames, records_only=True)
    try:
        ref = single.read()
        assert 3 < ref["n_unique"] < ref["n_cc"] and 0 < len(ref["active"]) < ref["n_unique"]
        orc = oracle_result(frames) if with_oracle else None
        if orc is not None:
            lm_checks.state_equal_oracle(single.result(), orc)
        dst = make(lib, h, w, F)
        try:
            for name, cuts in short_cut_lists(F, blanks).items():
                assert cuts[0] == 0 and cuts[-1] == F and all(a <= b for a, b in zip(cuts[:-1], cuts[1:]))
                dst.reset()
                round_trip(src, dst, cuts)
                same_state(dst.read(), ref, what=name)
                if orc is not None:
                    lm_checks.state_equal_oracle(dst.result(), orc)
        finally:
            dst.close()
    finally:
        single.close()
        src.close()


def long_stream(n_frames, h, w):
    """Mostly blank frames (the frame count is what the long blocks test): three cells, long pauses; the first dozen blank; ink
    in the frames on both sides of every 1024th frame and in the last frame."""
    always = [(k - 2, min(k + 2, n_frames)) for k in range(1024, n_frames, 1024)] + [(n_frames - 1, n_frames)]
    return square_stream(n_frames, h, w, seed=11, cells=3, mean_gap=12, max_len=6, blanks=tuple(range(12)), always=always)


LONG_CASES = {2049: (0, 1025, 1025, 2049), 1025: (0, 1, 1025), 1024: (0, 1024), 1023: (0, 1023)}


def check_long_block(lib, h, w, F, max_batch=64, handoff=False):
    """Blocks of more than 1024 frames: lm_k_append_offsets scans the per-frame counts in chunks of 1024 with a carry."""
    frames = long_stream(F, h, w)
    kw = dict(max_ccs=8 * F + 64, max_crop_words=64 * F + 4096)     # at most 4 CCs of 5 or 10 words per frame: far from the capacities
    single, src = pushed(lib, frames, max_batch, **kw), pushed(lib, frames, max_batch, records_only=True, **kw)
    try:
        ref = single.read()
        per_frame = np.diff(ref["frame_off"])
        assert ref["n_cc"] > F // 8 and (per_frame[:12] == 0).all() and (per_frame == 0).sum() > F // 4
        if F > 1024:
            assert per_frame[1023] > 0 and per_frame[1024] > 0 and per_frame[F - 1] > 0    # CCs on both sides of the scan's chunk border
        dst = make(lib, h, w, F, max_batch, **kw)
        try:
            round_trip(src, dst, LONG_CASES[F])
            same_state(dst.read(), ref, what="cuts %r" % (LONG_CASES[F],))
            if handoff:
                dst.reset()
                dst.append_packed(single.pack(0, F))
                dst.import_assign(single.export_assign())
                same_state(dst.read(), ref, active=False, what="matched hand-off of %d frames" % F)
        finally:
            dst.close()
    finally:
        single.close()
        src.close()


# ------------------------------------------------------------------------------------------------
# 5: matched hand-off
# ------------------------------------------------------------------------------------------------
def check_matched_handoff(lib, h, w):
    frames, _ = short_stream(h, w)
    F = len(frames)
    single = pushed(lib, frames)
    g = make(lib, h, w, F)
    try:
        ref = single.read()
        for rep in range(2):                                    # twice on the same receiver
            g.reset()
            g.append_packed(single.pack(0, F))
            g.import_assign(single.export_assign())
            same_state(g.read(), ref, active=False, what="matched hand-off %d" % rep)
        ga, gb = device.Grouping(g, max_gap=GAP), device.Grouping(single, max_gap=GAP)
        try:
            da, db = digests.from_device(g, ga), digests.from_device(single, gb)
            assert da == db
            assert len(gb.array("grp_off")) > 2                 # there are groups to compare
            ra, rb = g.be.to_host(ga.render(0, F)), single.be.to_host(gb.render(0, F))
            assert (ra == rb).all() and rb.any()
        finally:
            ga.close()
            gb.close()
    finally:
        g.close()
        single.close()


# ------------------------------------------------------------------------------------------------
# 6: the twin hash of lm_k_emit and of lm_k_crop_hash
# ------------------------------------------------------------------------------------------------
def match_stats(lib, fs):
    out = np.zeros(5, np.int64)
    lib.check(lib.lm_stream_match_stats(fs.handle, out.ctypes.data, fs.be.stream()))
    return [int(v) for v in out]


def check_twin_hash_paths(lib, h, w, B=16):
    """Records that came through lm_k_emit and records that came through lm_stream_append_packed (hashed by lm_k_crop_hash) find
    the same exact twins: the last matching batch has the same sources, tiles and pairs.  A disagreement would not change any
    result (twins are verified word for word), only feed the matcher more sources."""
    frames, _ = short_stream(h, w)
    F = len(frames)
    assert F % B == 0
    single, src = pushed(lib, frames, B), pushed(lib, frames, B, records_only=True)
    g, mixed = make(lib, h, w, F, B), make(lib, h, w, F, B)
    try:
        ref, ref_stats = single.read(), match_stats(lib, single)
        assert ref_stats[4] == B and ref_stats[0] > 0 and ref_stats[1] > 0
        n_last = int(ref["frame_off"][F] - ref["frame_off"][F - B])
        assert ref_stats[0] < n_last                            # some CCs of the batch are twins (or surely matched): no source
        round_trip(src, g, tuple(range(0, F + 1, B)))
        assert match_stats(lib, g) == ref_stats
        same_state(g.read(), ref, what="appended batches")
        # the last batch holds records of both origins: its first half labelled here, its second half appended
        dev = mixed.be.from_host(frames)
        mixed.push(dev[:F - B])
        mixed.push_records(dev[F - B:F - B // 2])
        mixed.append_packed(src.pack(F - B // 2, B // 2))
        mixed.match(B)
        assert match_stats(lib, mixed) == ref_stats
        same_state(mixed.read(), ref, what="mixed batch")
    finally:
        for fs in (single, src, g, mixed):
            fs.close()
    return ref_stats


# ------------------------------------------------------------------------------------------------
# 7: continuation through the host state
# ------------------------------------------------------------------------------------------------
def check_host_state_continuation(lib, h, w):
    frames, blanks = short_stream(h, w)
    F = len(frames)
    single, raw = pushed(lib, frames), pushed(lib, frames, records_only=True)
    a, b = make(lib, h, w, F), make(lib, h, w, F)
    try:
        ref = single.read()
        lone = [x for x in blanks if 1 < x < F - 1 and x - 1 not in blanks and x + 1 not in blanks][0]
        for cut in (1, lone, lone + 1, F // 2 + 3):
            a.reset()
            dev = a.be.from_host(frames)
            a.push(dev[:cut])
            st = a.export_state()
            b.import_state(st)                                  # resets b first
            b.push(dev[cut:])
            same_state(b.read(), ref, what="continued at %d" % cut)
        # raw records (gathered, nothing matched): no uniques, no active list, n_matched = 0; then one matching call
        r = raw.read()
        st = {"rec": r["rec"], "frame_off": r["frame_off"], "crop_off": r["crop_off"], "crop": r["crop"][:r["n_crop_words"]],
              "n_unique": 0, "tempo_count": 0, "active": np.zeros(0, np.int32), "active_cc": np.zeros(0, np.int32),
              "active_last": np.zeros(0, np.int32), "n_matched": 0}
        b.import_state(st)
        b.match(F)
        same_state(b.read(), ref, what="raw records imported, then matched")
    finally:
        for fs in (single, raw, a, b):
            fs.close()


# ------------------------------------------------------------------------------------------------
# 8: refusals
# ------------------------------------------------------------------------------------------------
def check_rejections(lib, h, w):
    """Every refusal happens on the host before a kernel is launched: the return code, the counters unchanged, and the same handle
    then completes a valid append + match (or append + import_assign) with the right result."""
    frames, _ = short_stream(h, w)
    F = len(frames)
    half = F // 2
    single, src = pushed(lib, frames), pushed(lib, frames, records_only=True)
    single_half = pushed(lib, frames[:half])
    other = pushed(lib, frames[:half + 5])                      # another stream's assignment: other n_cc, other n_frames
    g, small = make(lib, h, w, F), make(lib, h, w, half)
    try:
        ref, ref_half = single.read(), single_half.read()
        be, st = g.be, g.be.stream()
        block = src.pack(0, F)
        nbytes = int(block.shape[0])
        rc, nb = pack_size(lib, src, 0, F)
        assert rc == _lib.LM_OK and nb == nbytes
        host = be.to_host(block).copy()
        bad_magic = host.copy()
        bad_magic[24] ^= 0x01
        bad_magic = to_backend(be, bad_magic)
        shifted = to_backend(be, np.concatenate([np.zeros(4, np.uint8), host]))    # the block itself at an address that is 4 mod 32
        assert _lib.ptr(bad_magic) % 32 == 0 and _lib.ptr(block) % 32 == 0 and _lib.ptr(shifted) % 32 == 0

        def then_valid(dst, what):
            dst.append_packed(block)
            dst.match(F)
            same_state(dst.read(), ref, what="after " + what)
            dst.reset()

        def refused(dst, what, code, call):
            before = dst.counters()
            rc = call()
            assert rc == code, (what, rc, code, lib.last_error())
            assert dst.counters() == before, what

        refused(g, "truncated block", _lib.LM_ERR_ARG, lambda: lib.lm_stream_append_packed(g.handle, _lib.ptr(block), nbytes - 4, st))
        then_valid(g, "truncated block")
        refused(g, "wrong magic", _lib.LM_ERR_ARG, lambda: lib.lm_stream_append_packed(g.handle, _lib.ptr(bad_magic), nbytes, st))
        then_valid(g, "wrong magic")
        refused(g, "misaligned block", _lib.LM_ERR_ARG, lambda: lib.lm_stream_append_packed(g.handle, _lib.ptr(shifted) + 4, nbytes, st))
        then_valid(g, "misaligned block")
        # a receiver that is too small, with frames in it already
        small.append_packed(src.pack(0, 3))
        refused(small, "too-small receiver", _lib.LM_ERR_CAPACITY, lambda: lib.lm_stream_append_packed(small.handle, _lib.ptr(block), nbytes, st))
        small.append_packed(src.pack(3, half - 3))
        small.match(half)
        same_state(small.read(), ref_half, what="after too-small receiver")
        # pack / pack_size beyond the pushed frames
        scratch = be.empty((nbytes,), np.uint8)
        for first, n in ((0, F + 1), (F, 1), (F + 1, 0), (-1, 2), (3, -1)):
            refused(src, "pack_size(%d, %d)" % (first, n), _lib.LM_ERR_ARG, lambda: pack_size(lib, src, first, n)[0])
            refused(src, "pack(%d, %d)" % (first, n), _lib.LM_ERR_ARG,
                    lambda: lib.lm_stream_pack(src.handle, first, n, _lib.ptr(scratch), nbytes, st))
        refused(src, "pack into a misaligned buffer", _lib.LM_ERR_ARG,
                lambda: lib.lm_stream_pack(src.handle, 0, 2, _lib.ptr(shifted) + 4, nbytes, st))
        assert (be.to_host(src.pack(0, F)) == host).all()
        # export_assign of an unmatched stream
        out = be.empty((((4 * ref["n_cc"] + 31) & ~31) + 32,), np.uint8)
        refused(src, "export_assign of an unmatched stream", _lib.LM_ERR_STATE,
                lambda: lib.lm_stream_export_assign(src.handle, _lib.ptr(out), int(out.shape[0]), st))
        refused(single, "export_assign into a misaligned buffer", _lib.LM_ERR_ARG,
                lambda: lib.lm_stream_export_assign(single.handle, _lib.ptr(shifted) + 4, int(out.shape[0]), st))
        # import_assign of another stream's assignment, of a misaligned one, and into a stream that is matched already
        assign, foreign = single.export_assign(), other.export_assign()
        assert int(foreign.shape[0]) != int(assign.shape[0])
        g.append_packed(block)
        refused(g, "foreign assignment", _lib.LM_ERR_ARG,
                lambda: lib.lm_stream_import_assign(g.handle, _lib.ptr(foreign), int(foreign.shape[0]), st))
        moved = to_backend(be, np.concatenate([np.zeros(4, np.uint8), be.to_host(assign)]))
        refused(g, "misaligned assignment", _lib.LM_ERR_ARG,
                lambda: lib.lm_stream_import_assign(g.handle, _lib.ptr(moved) + 4, int(assign.shape[0]), st))
        g.import_assign(assign)
        same_state(g.read(), ref, active=False, what="after foreign assignment")
        refused(g, "assignment into a matched stream", _lib.LM_ERR_ARG,
                lambda: lib.lm_stream_import_assign(g.handle, _lib.ptr(assign), int(assign.shape[0]), st))
        same_state(g.read(), ref, active=False, what="after a second import")
    finally:
        for fs in (single, src, single_half, other, g, small):
            fs.close()
