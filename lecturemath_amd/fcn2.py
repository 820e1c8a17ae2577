"""Recipes of the second FCN engine (csrc/lm_fcn2.hip): for every layer of FCN-LectureNet (AccessMath/lecturenet_v1/FCN_lecturenet.py
:260-323, :364-403) the K walk of the gather-GEMM kernel -- which (plane, tap) pair feeds each of the four k-groups of every
32-deep slice -- and the weights packed as that kernel's A fragments.  numpy only rearranges weights once; all arithmetic of a
forward pass runs in liblecturemath_hip.so.

Vocabulary (see the header of lm_fcn2.hip): a TENSOR is C/8 planes of 16-byte slots (8 channels of a pixel as f16, hi parts, then
optionally the lo parts); a layer stages its input a CHUNK of planes at a time into LDS; a PAIR is (plane of the chunk, tap dy, dx):
the 8 k-values one lane group reads with one ds_read_b128; a SLICE is four pairs = one 16x16x32 MFMA step; consecutive slices are
fetched as weight GROUPS.  A pair plane (network input, diff) holds {c0 c1 c2 0 | the same of pixel x + 1} per slot.
"""
import collections

import numpy as np

EPI_PO, EPI_T, EPI_TC, EPI_TC2, EPI_V = 0, 1, 2, 3, 4      # EPI_V: a head's row convolution fused with its vertical sum
LDS_TWO_WORKGROUPS = 80 * 1024        # a workgroup's LDS for two of them to share a CU's 160 KB

# layer ids (both engines: lm_fcn.hip, lm_fcn2.hip); L_DOWN, L_UPT and L_UPC are the first of five.  The planar engine runs L_REC inside L_TEXT.
L_DOWN, L_MID, L_UPT, L_UPC, L_TEXT, L_REC, L_PX1, L_PX2, L_OUT, N_LAYERS = 0, 5, 6, 11, 16, 17, 18, 19, 20, 21
LAYER_NAMES = {L_MID: "mid_block", L_TEXT: "conv_text_mask_out+conv_reconstruct", L_PX1: "conv_pixels_1", L_PX2: "conv_pixels_2", L_OUT: "conv_out"}
for _n in range(5):
    LAYER_NAMES.update({L_DOWN + _n: "conv_down_block_%d" % (_n + 1), L_UPT + _n: "transposed_conv_%d" % (5 - _n), L_UPC + _n: "conv_up_block_%d" % (5 - _n)})

# The activation tensors of the planar engine (the LM_F2_* enum and the def(id, channels, level) calls of lm_fcn2_create): id, name, pyramid
# level (0 = full resolution) and which of the 18 widths is its channel count (None: a pair plane of 8 channels, values in [-2, 2] by construction)
Tensor = collections.namedtuple("Tensor", "id name level width")
T_X0P, T_PRE0, T_POOL0, T_MID, T_UPT0, T_CU0, T_XUP, T_DP, T_P1, T_P2 = 0, 1, 6, 11, 12, 17, 21, 22, 23, 24
TENSORS = sorted([Tensor(T_X0P, "x0", 0, None), Tensor(T_MID, "mid", 5, 5), Tensor(T_XUP, "up1", 0, 15), Tensor(T_DP, "diff", 0, None), Tensor(T_P1, "p1", 0, 16), Tensor(T_P2, "p2", 0, 17)] +
                 [Tensor(T_PRE0 + n, "down%d_pre" % (n + 1), n, n) for n in range(5)] + [Tensor(T_POOL0 + n, "down%d_pool" % (n + 1), n + 1, n) for n in range(5)] +
                 [Tensor(T_UPT0 + n, "upsample%d" % (5 - n), 4 - n, 6 + 2 * n) for n in range(5)] + [Tensor(T_CU0 + n, "up%d" % (5 - n), 4 - n, 7 + 2 * n) for n in range(4)])
N_TENSORS = len(TENSORS)
TENSOR_NAMES = {t.id: t.name for t in TENSORS}
FIXED_TENSORS = tuple(t.id for t in TENSORS if t.width is None)        # network input and diff take no exponent
# tensors in the order the forward pass produces them; a pooled tensor shares the exponent of the tensor it is pooled from (exponent_group)
TENSOR_ORDER = ([T_X0P] + [T_PRE0 + n for n in range(5)] + [T_MID] + [t for n in range(5) for t in (T_UPT0 + n, T_CU0 + n if n < 4 else T_XUP)] + [T_DP, T_P1, T_P2])


def exponent_group(t):
    return [t, t - T_PRE0 + T_POOL0] if T_PRE0 <= t < T_POOL0 else [t]


def geom(kh, kw, terms, nc=1):
    pw, ph = 16 * nc + kw - 1, 16 + kh - 1
    pls = (ph * pw * 16 + 255) & ~255
    return pw, ph, pls, (2 if terms in (2, 3) else 1)


# operand formats (the TERMS parameter of lm_k_g2): MFMA products per operand pair
FORMAT_PRODUCTS = {1: 1, 2: 2, 3: 3, 4: 2}
FORMAT_NAMES = {"f16": 1, "a2": 2, "f16x3": 3, "w2": 4}     # a2: activations hi + lo; w2: weights hi + lo


def octet_pair(plane, dy, dx, cbase):
    """k-values of an ordinary plane at tap (dy, dx): channels cbase .. cbase + 7 of the weights' input axis"""
    return {"plane": plane, "dy": dy, "dx": dx, "kmap": [(cbase + j, dy, dx) for j in range(8)]}


def pairplane_pair(plane, dy, dx, cbase, kw_total):
    """k-values of a pair plane read at tap (dy, dx): three channels of that tap, a zero, three channels of tap dx + 1, a zero"""
    km = [(cbase + j, dy, dx) for j in range(3)] + [None]
    km += [((cbase + j, dy, dx + 1) if dx + 1 < kw_total else None) for j in range(3)] + [None]
    return {"plane": plane, "dy": dy, "dx": dx, "kmap": km}


def row_channel(mt, m, r, epi):
    """channel (relative to the workgroup's first) held by row r of channel tile m -- lm_k_g2's epilogues"""
    if epi not in (EPI_T, EPI_V) and m < 2 * (mt // 2):
        return 32 * (m // 2) + 8 * (r >> 2) + 4 * (m & 1) + (r & 3)
    return 16 * m + r


def have_instance(kh, kw, terms, mt, epi, nc=1, loader=0):
    """the kernel instances csrc/lm_fcn2.hip compiles (lm_g2_launch)"""
    v = (nc, loader)
    if (kh, kw) == (3, 3) and epi == EPI_PO:
        if v == (1, 0):
            return terms in (1, 3, 4) and 1 <= mt <= 4
        if v == (1, 1):
            return (terms == 1 and 1 <= mt <= 4) or (terms == 4 and mt in (1, 2))
        return v == (2, 0) and terms in (1, 3, 4) and 1 <= mt <= (3 if terms == 1 else 2)
    if (kh, kw) == (1, 1) and epi in (EPI_TC, EPI_TC2):
        return v == (1, 0) and terms in (1, 3) and 1 <= mt <= 4
    if (kh, kw) == (1, 7) and epi == EPI_T:
        return v in ((1, 0), (2, 0)) and 1 <= terms <= 4 and mt == 1
    if (kh, kw) == (1, 7) and epi == EPI_V:
        return v in ((1, 0), (2, 0)) and terms in (3, 4) and mt == 1
    if (kh, kw) == (7, 7) and epi == EPI_PO:
        return v in ((1, 0), (1, 1), (2, 0)) and 1 <= terms <= 4 and mt in (1, 2)
    return False


def table_bytes(nslices):
    """LDS bytes of the slice table: 16 bytes per slice (the four k-groups' patch offsets) + two entries of look-ahead"""
    return ((nslices + 2) * 16 + 255) & ~255


def lds_bytes(kh, kw, terms, npc, nslices, pdouble, wbuf, ngroups, nc=1):
    _, _, pls, nhl = geom(kh, kw, terms, nc)
    return table_bytes(nslices) + (2 if pdouble else 1) * npc * nhl * pls + (2 if ngroups > 1 else 1) * wbuf


class Recipe(collections.namedtuple("Recipe", "kh kw terms mt epi nchunks npc ngroups nslices nc loader lds_target pdouble wbuf cout planes groups slices weights wblocks lds_bytes")):
    """One layer as lm_k_g2 runs it.  planes: [(tensor, octet)] of all chunks, npc per chunk; groups: [first slice, slices, chunk]; slices: the
    four LDS offsets of each; weights: the packed A fragments [parity][block][slice][tile][hi|lo][lane][8] f16; lds_bytes: what a workgroup needs."""
    __slots__ = ()

    def descriptor(self):
        """the int32 array of lm_fcn2_set_layer (read back by lm_fcn2_set_layer in lm_fcn2.hip: the one place that knows its order).
        flags: bits 0-3 column tiles, bit 8 loader wave, bits 16.. the LDS target in KB (the run-time weight ring stays inside it)"""
        flags = self.nc | (self.loader << 8) | ((self.lds_target // 1024) << 16)
        head = [self.kh, self.kw, self.terms, self.mt, self.epi, self.nchunks, self.npc, self.ngroups, self.nslices, flags, int(self.pdouble), self.wbuf, self.cout]
        return np.asarray(head + [v for rows in (self.planes, self.groups, self.slices) for row in rows for v in row], np.int32)

    @property
    def tensors(self):
        return sorted(set(t for t, _ in self.planes))

    def summary(self):
        """FcnEngine.recipes[layer]"""
        return {"kh": self.kh, "kw": self.kw, "terms": self.terms, "mt": self.mt, "chunks": self.nchunks, "planes_per_chunk": self.npc, "groups": self.ngroups,
                "slices": self.nslices, "lds_bytes": self.lds_bytes, "cout": self.cout, "nc": self.nc, "loader": self.loader, "epilogue": self.epi,
                "first_tensor": self.planes[0][0], "tensors": self.tensors}


def lo_flags(recipes):
    """[N_TENSORS] int32 for lm_fcn2_create: a tensor keeps its lo parts when a layer reading it splits its activations (a2, f16x3)"""
    lo = np.zeros(N_TENSORS, np.int32)
    lo[[t for r in recipes if r.terms in (2, 3) for t in r.tensors]] = 1
    return lo


def build(w_list, chunks, kh, kw, terms, mt, epi, gsize=None, pdouble=None, lds_target=LDS_TWO_WORKGROUPS, nc=1, loader=0):
    """w_list: one [cout][cin][KH][KW] float32 array (or four, one per (dy, dx) of a transposed convolution).
    chunks: [{"planes": [(tensor, octet), ...], "pairs": [pair, ...]}], every chunk with the same number of planes.
    Returns the layer's Recipe."""
    if epi == EPI_V and not have_instance(kh, kw, terms, mt, epi, nc, loader):       # no fused instance for this format: rows + vertical-sum kernel
        epi = EPI_T
    if not have_instance(kh, kw, terms, mt, epi, nc, loader):       # a variant the library does not hold: the plain one
        nc, loader = 1, 0
    pw, ph, pls, nhl = geom(kh, kw, terms, nc)
    nwl = 2 if terms >= 3 else 1
    cout = w_list[0].shape[0]
    assert cout % (16 * mt) == 0, (cout, mt)
    npc = len(chunks[0]["planes"])
    slices, kidx = [], []                        # slices: (four LDS offsets, chunk)
    wshape = w_list[0].shape
    for ci, ch in enumerate(chunks):
        assert len(ch["planes"]) == npc
        prs = ch["pairs"]
        for s0 in range(0, len(prs), 4):
            four = list(prs[s0:s0 + 4])
            while len(four) < 4:                 # unused k-groups: zero weights over data that is certainly finite (the slice's first pair)
                four.append({"plane": four[0]["plane"], "dy": four[0]["dy"], "dx": four[0]["dx"], "kmap": [None] * 8})
            offs = [p["plane"] * nhl * pls + (p["dy"] * pw + p["dx"]) * 16 for p in four]
            assert all(0 <= p["dy"] < kh and 0 <= p["dx"] < kw and 0 <= p["plane"] < npc for p in four)
            slices.append((offs, ci))
            idx = np.full(32, -1, np.int64)
            for g, p in enumerate(four):
                for j, km in enumerate(p["kmap"]):
                    if km is not None:
                        idx[g * 8 + j] = (km[0] * wshape[2] + km[1]) * wshape[3] + km[2]
            kidx.append(idx)
    nslices = len(slices)
    kidx = np.stack(kidx)                                           # [nslices][32]
    # weight groups: consecutive slices of one chunk
    per_slice = mt * nwl * 1024
    if pdouble is None:
        pdouble = len(chunks) > 1
    if gsize is None:
        gsize = 1
        for cand in range(2, 17):
            # two weight buffers within the target for the layers that share a CU's LDS between two workgroups (the run-time ring takes a
            # third when it fits 80 KB); three where a workgroup has the CU to itself
            if lds_bytes(kh, kw, terms, npc, nslices, pdouble, cand * per_slice * (3 if lds_target > LDS_TWO_WORKGROUPS else 2) // 2, 2, nc) <= lds_target:
                gsize = cand
    groups = []
    s = 0
    while s < nslices:                       # per chunk: as few groups as gsize allows, sizes as even as possible
        n = 1
        while s + n < nslices and slices[s + n][1] == slices[s][1]:
            n += 1
        k = (n + gsize - 1) // gsize
        for i in range(k):
            cnt = n // k + (1 if i < n % k else 0)
            groups.append([s, cnt, slices[s][1]])
            s += cnt
    wbuf = max(g[1] for g in groups) * per_slice
    # weights: [parity][block][slice][tile][hi|lo][lane = kgroup * 16 + row][8]
    nblocks = cout // (16 * mt)
    rows = np.array([[[b * 16 * mt + row_channel(mt, m, r, epi) for r in range(16)] for m in range(mt)] for b in range(nblocks)])     # [b][m][r]
    packed = []
    for w in w_list:
        assert w.shape == wshape
        w2 = np.concatenate([w.reshape(cout, -1).astype(np.float32), np.zeros((cout, 1), np.float32)], axis=1)
        ws = w2[:, kidx]                                            # [cout][nslices][32]   (index -1 = the zero column)
        a = ws[rows]                                                # [b][m][r][nslices][32]
        a = a.reshape(nblocks, mt, 16, nslices, 4, 8).transpose(0, 3, 1, 4, 2, 5)       # b, slice, m, kgroup, r, j
        hi = a.astype(np.float16)
        parts = [hi]
        if nwl == 2:
            parts.append((a - hi.astype(np.float32)).astype(np.float16))
        packed.append(np.stack(parts, axis=3).reshape(nblocks, nslices, mt, nwl, 64, 8))
    wpk = np.ascontiguousarray(np.stack(packed))                    # [parity][block]...
    return Recipe(kh, kw, terms, mt, epi, len(chunks), npc, len(groups), nslices, nc, loader, lds_target, bool(pdouble), wbuf, cout,
                  [pl for ch in chunks for pl in ch["planes"]], groups, [offs for offs, _ in slices], wpk, len(w_list) * nblocks,
                  lds_bytes(kh, kw, terms, npc, nslices, pdouble, wbuf, len(groups), nc))


def conv_chunks(inputs, kh, kw, co):
    """ordinary planes: inputs = [(tensor, octets)] concatenated along the weights' input axis; chunks of `co` planes, pairs in
    (tap, plane) order"""
    planes, cbase = [], 0
    for t, n in inputs:
        for o in range(n):
            planes.append((t, o, cbase))
            cbase += 8
    assert len(planes) % co == 0
    chunks = []
    for c0 in range(0, len(planes), co):
        pl = planes[c0:c0 + co]
        pairs = [octet_pair(i, dy, dx, p[2]) for dy in range(kh) for dx in range(kw) for i, p in enumerate(pl)]
        chunks.append({"planes": [(p[0], p[1]) for p in pl], "pairs": pairs})
    return chunks


def pick_mt(cout, tiles, prefer=(4, 3, 2)):
    """channel tiles per workgroup: the largest that divides cout / 16 and still leaves the grid >= 1.5 workgroups per CU"""
    nt = cout // 16
    ok = [m for m in prefer if nt % m == 0] or [1]
    for m in ok:
        if tiles * (nt // m) >= 384:
            return m
    return ok[-1]


def conv_layer(w, inputs, terms, tiles, mt=None, nc=1, loader=0, lds_target=LDS_TWO_WORKGROUPS, gsize=None):
    """tiles: 16 x 16 pixel tiles of the layer's grid (a 16 x 32 tile counts as two)"""
    cout, _, kh, kw = w.shape
    if not have_instance(kh, kw, terms, mt or pick_mt(cout, tiles // nc), EPI_PO, nc, loader):
        nc, loader = 1, 0
    mt = mt or pick_mt(cout, tiles // nc)
    total = sum(n for _, n in inputs)
    best = None
    for co in (4, 3, 2, 1):
        if total % co:
            continue
        chunks = conv_chunks(inputs, kh, kw, co)
        pd = len(chunks) > 1
        r = build([w], chunks, kh, kw, terms, mt, EPI_PO, pdouble=pd, nc=nc, loader=loader, lds_target=lds_target, gsize=gsize)
        key = (r.lds_bytes > lds_target, r.nslices)      # room for two workgroups per CU first, then the fewest slices
        if best is None or key < best[0]:
            best = (key, r)
    return best[1]


def pixel_chunks(feat_tensor, nf, dp_tensor, kh_total, kw_total, octets=2):
    """(diff, features) input of the 7x7 pixel branch / the output row convolution: chunks of two feature octets + the diff pair plane;
    the pair plane's taps (kernel columns 0, 2, 4, 6: a slot covers two) are spread over the chunks' last slices.
    Weight input axis: 0..2 diff, 3.. features (cat((diff, features)), FCN_lecturenet.py:383-395).
    octets = 1: chunks of ONE feature octet + the pair plane (half the patch bytes in LDS: a 16 x 32 tile of a split format fits)."""
    if octets == 1:
        return pixel_chunks_1(feat_tensor, nf, dp_tensor, kh_total, kw_total)
    assert nf % 2 == 0
    nch = nf // 2
    dp_taps = list(range(0, kw_total, 2))
    share = [dp_taps[i * len(dp_taps) // nch:(i + 1) * len(dp_taps) // nch] for i in range(nch)]
    chunks = []
    for c in range(nch):
        pairs = []
        for dy in range(kh_total):
            row = []
            for dx in range(0, kw_total - 1, 2):
                row += [octet_pair(0, dy, dx, 3 + 16 * c), octet_pair(1, dy, dx, 3 + 16 * c + 8),
                        octet_pair(0, dy, dx + 1, 3 + 16 * c), octet_pair(1, dy, dx + 1, 3 + 16 * c + 8)]
            if kw_total & 1:
                row += [octet_pair(0, dy, kw_total - 1, 3 + 16 * c), octet_pair(1, dy, kw_total - 1, 3 + 16 * c + 8)]
            row += [pairplane_pair(2, dy, dx, 0, kw_total) for dx in share[c]]
            pairs += row
        chunks.append({"planes": [(feat_tensor, 2 * c), (feat_tensor, 2 * c + 1), (dp_tensor, 0)], "pairs": pairs})
    return chunks


def pixel_chunks_1(feat_tensor, nf, dp_tensor, kh_total, kw_total):
    """one feature octet per chunk: per kernel row its kw taps, then the chunk's share of the pair plane's taps"""
    dp_taps = list(range(0, kw_total, 2))
    share = [dp_taps[i * len(dp_taps) // nf:(i + 1) * len(dp_taps) // nf] for i in range(nf)]
    chunks = []
    for c in range(nf):
        pairs = []
        for dy in range(kh_total):
            pairs += [octet_pair(0, dy, dx, 3 + 8 * c) for dx in range(kw_total)]
            pairs += [pairplane_pair(1, dy, dx, 0, kw_total) for dx in share[c]]
        chunks.append({"planes": [(feat_tensor, c), (dp_tensor, 0)], "pairs": pairs})
    return chunks


def text_rec_rows(w_text, w_rec):
    """text mask (7x7, 1 output) + reconstruction (3x3, 3 outputs) as one 1x7 row convolution with 16 outputs: 0..6 text kernel rows,
    7 + kh * 3 + co reconstruction rows with their three taps centred (lm_k_vsum2_text_rec adds the rows up)"""
    cin = w_text.shape[1]
    rows = np.zeros((16, cin, 1, 7), np.float32)
    rows[0:7, :, 0, :] = w_text[0].transpose(1, 0, 2)
    rows[7:16, :, 0, 2:5] = w_rec.transpose(2, 0, 1, 3).reshape(9, cin, 3)
    return rows


def out_rows(w_out):
    """7x7 convolution with one output as a 1x7 row convolution with 7 (of 16) outputs: row kh = kernel row kh"""
    _, cin, k, _ = w_out.shape
    rows = np.zeros((16, cin, 1, k), np.float32)
    rows[0:k, :, 0, :] = w_out[0].transpose(1, 0, 2)
    return rows


# {layer: channel tiles per workgroup} where pick_mt's rule is not the fastest (profiles/r04_mt_{default,a,b}.txt: conv_down_1 on ONE
# tile = 24,480 small workgroups at 114 VGPRs, 139 -> 124-130 us -- it is a 250 MB store; every other layer is fastest on pick_mt's choice)
DEFAULT_MT = {L_DOWN: 1}
# kernel variant per layer, (column tiles per wave, loader wave), measured per layer at 1920x1080 (profiles/r04_variants_*.txt): 16 x 32
# tiles where the weights are re-fetched per tile at full resolution and the instance keeps two workgroups per CU; the loader wave
# in the two layers with one workgroup per CU and two channel tiles
DEFAULT_VARIANTS = {L_UPC + 4: (2, 0), L_TEXT: (2, 0), L_PX1: (2, 0), L_PX2: (2, 0), L_MID: (1, 1), L_UPC: (1, 1)}


def decoder_levels(widths):
    """[(level, channels in, upsampled, out, skip)] of the five decoder stages, level 5 first"""
    d, mid, up = widths[0:5], widths[5], widths[6:16]
    return [(lvl, (mid if lvl == 5 else up[2 * (5 - lvl) - 1]), up[2 * (5 - lvl)], up[2 * (5 - lvl) + 1], d[lvl - 1]) for lvl in (5, 4, 3, 2, 1)]


def planar_layers(folded, widths, max_h, max_w, terms_of, variants=DEFAULT_VARIANTS, mt_of=DEFAULT_MT, scale=None, only=None, fused_heads=1):
    """The network walk of the planar engine: {layer: (Recipe, bias)} of the layers in `only` (default: all), in upload order.
    folded: {reference module name: (w, b)} with BatchNorm folded in; terms_of(layer): its operand format; variants, mt_of: {layer: (nc,
    loader)}, {layer: channel tiles}; scale(layer, w, [(tensor, channels)], axis) -> w as packed (the tensors' and the layer's power-of-two
    exponents: fcn_range.range_weights); fused_heads: bit 0 = text / rec, bit 1 = output.
    Every layer aims at LDS_TWO_WORKGROUPS of LDS (build's and conv_layer's default): two workgroups per CU."""
    d1, pm1, pm2, c1 = widths[0], widths[16], widths[17], widths[15]
    out, want = {}, (range(N_LAYERS) if only is None else only).__contains__

    def tiles(level):
        return (((max_h >> level) + 15) // 16) * (((max_w >> level) + 15) // 16)

    def V(layer):
        nc, loader = variants.get(layer, (1, 0))
        return {"nc": nc, "loader": loader}

    def weights(layer, name, inputs, axis=1):
        w, b = folded[name]
        return scaled(layer, w, inputs, axis), b

    def scaled(layer, w, inputs, axis=1):
        return scale(layer, w, inputs, axis) if scale else w

    def conv(layer, name, inputs, level):
        if want(layer):
            w, b = weights(layer, name, inputs)
            out[layer] = (conv_layer(w, [(t, n // 8) for t, n in inputs], terms_of(layer), tiles(level), mt=mt_of.get(layer), **V(layer)), b)

    def tconv(layer, lvl, src, tin, u):
        if not want(layer):
            return
        wt, bt = weights(layer, "transposed_conv_%d" % lvl, [(src, tin)], axis=0)          # [Cin][Cout][2][2]
        n8 = tin // 8
        chunks = conv_chunks([(src, n8)], 1, 1, 8 if n8 % 8 == 0 else (4 if n8 % 4 == 0 else 2))
        quad = {(dy, dx): np.ascontiguousarray(wt[:, :, dy, dx].T) for dy in (0, 1) for dx in (0, 1)}         # [u][tin]
        if u % 32 == 0 and not mt_of.get(layer):
            # both dx of a 32-channel block in one workgroup: per dy a virtual output axis [block][dx][32 channels]
            w2 = [np.concatenate([quad[dy, dx][b * 32:(b + 1) * 32] for b in range(u // 32) for dx in (0, 1)])[:, :, None, None] for dy in (0, 1)]
            out[layer] = (build(w2, chunks, 1, 1, terms_of(layer), 4, EPI_TC2), bt)
        else:
            w4 = [quad[dy, dx][:, :, None, None] for dy in (0, 1) for dx in (0, 1)]
            out[layer] = (build(w4, chunks, 1, 1, terms_of(layer), mt_of.get(layer) or pick_mt(u, tiles(lvl)), EPI_TC), bt)

    # encoder: layer 1 reads the input pair plane (3 channels, two horizontal taps per slot)
    if want(L_DOWN):
        w, b = weights(L_DOWN, "conv_down_block_1", [(T_X0P, 3)])
        pairs = [pairplane_pair(0, dy, dx, 0, 3) for dy in range(3) for dx in (0, 2)]
        out[L_DOWN] = (build([w], [{"planes": [(T_X0P, 0)], "pairs": pairs}], 3, 3, terms_of(L_DOWN), mt_of.get(L_DOWN) or pick_mt(d1, tiles(0) // V(L_DOWN)["nc"]), EPI_PO, **V(L_DOWN)), b)
    for n in range(1, 5):
        conv(L_DOWN + n, "conv_down_block_%d" % (n + 1), [(T_POOL0 + n - 1, widths[n - 1])], n)
    conv(L_MID, "mid_block", [(T_POOL0 + 4, widths[4])], 5)
    for i, (lvl, tin, u, _, skip) in enumerate(decoder_levels(widths)):
        conv(L_UPC + i, "conv_up_block_%d" % lvl, [(T_UPT0 + i, u), (T_PRE0 + lvl - 1, skip)], lvl - 1)         # input = cat(up, skip_pre)
        tconv(L_UPT + i, lvl, T_MID if i == 0 else T_CU0 + i - 1, tin, u)
    # heads: the text + reconstruction row convolution is fused with its vertical sums (EPI_V; 56 + 77 -> 93 us: the 133 MB fp32 row buffer
    # is neither written nor read back); the output logit's is not (62 + 20 -> 87 us fused: its tiles of 10 finished rows cost more
    # row-convolution work than its 66 MB of rows; profiles/r04_heads_*.txt).
    head_epi, out_epi = (EPI_V if fused_heads & 1 else EPI_T), (EPI_V if fused_heads & 2 else EPI_T)
    if want(L_TEXT):
        (wt, bt), (wr, br) = folded["conv_text_mask_out"], folded["conv_reconstruct"]
        rows = scaled(L_TEXT, text_rec_rows(wt, wr), [(T_XUP, c1)])
        out[L_TEXT] = (build([rows], conv_chunks([(T_XUP, c1 // 8)], 1, 7, c1 // 8), 1, 7, terms_of(L_TEXT), 1, head_epi, **V(L_TEXT)), np.concatenate([np.zeros(16, np.float32), bt, br]))
    # the pixel branch: patch planes single-buffered; feature octets per chunk: two in conv_pixels_1, one in conv_pixels_2, so that
    # the 16 x 32 tile's patch planes of the split format leave room for two workgroups per CU (two octets: 88 KB of LDS, one
    # workgroup, 757 us; one octet: 76 KB, 338 us; 16 x 16 tiles: 364 us)
    for layer, name, feat, nf, cout, octets in ((L_PX1, "conv_pixels_1", T_XUP, c1, pm1, 2), (L_PX2, "conv_pixels_2", T_P1, pm1, pm2, 1)):
        if want(layer):
            w, b = weights(layer, name, [(T_DP, 3), (feat, nf)])
            out[layer] = (build([w], pixel_chunks(feat, nf // 8, T_DP, 7, 7, octets=octets), 7, 7, terms_of(layer), 2 if cout % 32 == 0 else 1, EPI_PO, pdouble=False, **V(layer)), b)
    if want(L_OUT):
        w, b = weights(L_OUT, "conv_out", [(T_DP, 3), (T_P2, pm2)])
        out[L_OUT] = (build([out_rows(w)], pixel_chunks(T_P2, pm2 // 8, T_DP, 1, 7), 1, 7, terms_of(L_OUT), 1, out_epi, pdouble=False, **V(L_OUT)), np.concatenate([np.zeros(16, np.float32), b]))
    return out
