"""The first FCN engine (csrc/lm_fcn.hip: fp32 activations, operands split into f16 hi + lo while staged, or exact fp32 MFMA chains): its
weights packed into MFMA fragment order, and the walk over the network that packs every layer.  numpy only rearranges weights once."""
import numpy as np

from .fcn2 import L_DOWN, L_MID, L_OUT, L_PX1, L_PX2, L_REC, L_TEXT, L_UPC, L_UPT, decoder_levels, text_rec_rows


def pack_mfma(w_oikk, ck, cin_map, cin_padded):
    """[Cout][Cin][K][K] -> [chunk][tap][kstep][nblock][lane 64][4] for v_mfma_f32_32x32x2_f32:
    element e of lane l = W[co = nblock*32 + (l & 31)][ci = chunk*ck + kstep*8 + 4*(l >> 5) + e][tap].
    cin_map[i] = position of logical input channel i in the padded channel space of the input buffer(s)."""
    cout, cin, k, _ = w_oikk.shape
    nblocks = (cout + 31) // 32
    wp = np.zeros((nblocks * 32, cin_padded, k * k), np.float32)
    wp[:cout][:, np.asarray(cin_map)] = w_oikk.reshape(cout, cin, k * k)
    nchunks, ks = cin_padded // ck, ck // 8
    # wp[co, ci, tap] -> [chunk, ks, half, e, tap, nblock, j]
    a = wp.reshape(nblocks, 32, nchunks, ks, 2, 4, k * k)            # nb, j, chunk, ks, half, e, tap
    a = a.transpose(2, 6, 3, 0, 4, 1, 5)                              # chunk, tap, ks, nb, half, j, e
    return np.ascontiguousarray(a).reshape(-1)


def pack_mfma_h(w_oikk, cin_map, cin_logical):
    """fp16-split packing for lm_k_conv_mfma_h: [chunk][tap][nblock][hi|lo][lane 64][8 halfs], element j of lane l =
    W[co = nblock*32 + (l & 31)][ci = chunk*16 + 8*(l >> 5) + j][tap]; hi = f16(w), lo = f16(w - hi).
    cin_map[i] = position of weight input channel i among the cin_logical concatenated input channels (padded to 16 here).
    Returned as a float32 view (two halfs per float) for lm_fcn_set_layer."""
    cout, cin, kh, kw = w_oikk.shape                                    # square kernels, or the 1 x K rows of pack_rows_h
    taps = kh * kw
    nblocks = (cout + 31) // 32
    cpad = ((cin_logical + 15) // 16) * 16
    wp = np.zeros((nblocks * 32, cpad, taps), np.float32)
    wp[:cout][:, np.asarray(cin_map)] = w_oikk.reshape(cout, cin, taps)
    hi = wp.astype(np.float16)
    lo = (wp - hi.astype(np.float32)).astype(np.float16)
    both = np.stack([hi, lo])                                           # hl, co, ci, tap
    a = both.reshape(2, nblocks, 32, cpad // 16, 2, 8, taps)           # hl, nb, j, chunk, half, e, tap
    a = a.transpose(3, 6, 1, 0, 4, 2, 5)                                # chunk, tap, nb, hl, half, j, e
    return np.ascontiguousarray(a).reshape(-1).view(np.float32)


def pack_rows_h(w_oikk, cin_map, cin_logical):
    """A K x K convolution with NV <= 3 outputs as a 1 x K row convolution with K * NV outputs (lm_rowconv_layer in lm_fcn.hip):
    virtual output kh * NV + co holds kernel row kh of channel co; lm_k_vsum adds the rows up."""
    nv, cin, k, _ = w_oikk.shape
    rows = np.ascontiguousarray(w_oikk.transpose(2, 0, 1, 3)).reshape(k * nv, cin, 1, k)      # [kh][co][ci][kw] -> [kh * NV + co][ci][1][kw]
    return pack_mfma_h(rows, cin_map, cin_logical)


def pack_text_rec_rows_h(w_text, w_rec, cin_map, cin_logical):
    """Text mask and reconstruction over the same input as ONE 1 x 7 row convolution with 16 outputs (fcn2.text_rec_rows; lm_text_rec_heads)"""
    return pack_mfma_h(text_rec_rows(w_text, w_rec), cin_map, cin_logical)


def pack_small(w_oikk, cin_map, cin_padded):
    """[Cout<=4][Cin][K][K] -> [chunk of 8 channels][tap][8] for Cout == 1, [chunk][tap][8][4] otherwise (lm_k_conv_small)."""
    cout, cin, k, _ = w_oikk.shape
    lanes = 1 if cout == 1 else 4
    assert cin_padded % 8 == 0
    out = np.zeros((k * k, cin_padded, lanes), np.float32)
    out[:, np.asarray(cin_map), :cout] = w_oikk.reshape(cout, cin, k * k).transpose(2, 1, 0)
    out = out.reshape(k * k, cin_padded // 8, 8, lanes).transpose(1, 0, 2, 3)
    return np.ascontiguousarray(out).reshape(-1)


def _pad8(c):
    return (c + 7) & ~7


def _bias_pad(b, n=None, at=0):
    """b at offset `at` of n zeros (default: len(b) rounded up to 32)"""
    out = np.zeros(n or ((len(b) + 31) // 32) * 32, np.float32)
    out[at:at + len(b)] = b
    return out


def first_engine_layers(folded, widths, pk, kk, precision):
    """The arguments of lm_fcn_set_layer after the handle, per layer in upload order: (layer, weights, bias, cin, cout, k, ck).
    folded: {reference module name: (w, b)} with BatchNorm folded in; precision: "fp32" | "f16x3" | "f16x2" | "f16"."""
    d1, d2, d3, d4, d5, mid = widths[:6]
    c1, pm1, pm2 = widths[15:]
    h = precision != "fp32"
    hck = {"f16x3": 0, "f16x2": -2, "f16": -1}.get(precision, 0)       # lm_fcn.hip: ck <= 0 selects the fp16-split kernel and its products per operand pair

    def mfma(w, cin_map, *cin_padded):
        """(packed weights, ck) of a layer whose input buffers hold cin_padded channels"""
        if h:
            return pack_mfma_h(w, cin_map, sum(cin_padded)), hck
        ck = 16 if all(c % 16 == 0 for c in cin_padded) else 8
        return pack_mfma(w, ck, cin_map, sum(cin_padded)), ck

    # encoder + mid (layer 1 sees the 3 RGB channels padded to 8)
    cin = [3, d1, d2, d3, d4, d5]
    for n in range(6):
        w, b = folded["conv_down_block_%d" % (n + 1) if n < 5 else "mid_block"]
        cpad = 8 if n == 0 else cin[n]
        wpk, ck = mfma(w, range(cin[n]), cpad)
        yield L_DOWN + n, wpk, _bias_pad(b), cpad, w.shape[0], kk, ck
    for i, (lvl, tin, u, c, skip) in enumerate(decoder_levels(widths)):
        wt, bt = folded["transposed_conv_%d" % lvl]                                     # [Cin][Cout][2][2]
        if h:       # one launch: the four (dy, dx) sets are the four "taps" of the packing (lm_k_convT_mfma_h)
            yield L_UPT + i, pack_mfma_h(np.ascontiguousarray(wt.transpose(1, 0, 2, 3)), range(tin), tin), _bias_pad(bt), tin, u, 1, hck
        else:
            sets = [mfma(np.ascontiguousarray(wt[:, :, dy, dx].T)[:, :, None, None], range(tin), tin) for dy in (0, 1) for dx in (0, 1)]
            yield L_UPT + i, np.concatenate([p for p, _ in sets]), _bias_pad(bt), tin, u, 1, sets[0][1]
        w, b = folded["conv_up_block_%d" % lvl]                                        # input = cat(up, skip_pre)
        wpk, ck = mfma(w, range(u + skip), u, skip)
        yield L_UPC + i, wpk, _bias_pad(b), u + skip, c, kk, ck
    (wt, bt), (wr, br), (w1, b1), (w2, b2), (wo, bo) = (folded[n] for n in ("conv_text_mask_out", "conv_reconstruct", "conv_pixels_1", "conv_pixels_2", "conv_out"))
    # The fp16-split formats with the shipped kernel sizes (7x7 pixel branch, 3x3 elsewhere) run the heads on the MFMA path
    # (row convolution + vertical sum) and keep x_up1 / diff / pixel features in buffers of their own: a (diff, features)
    # input is the two-input concatenation [d0 d1 d2 0 | features].  Head biases: [0..31] zeros for the row convolution's epilogue,
    # [32..] the bias lm_k_vsum adds.
    if h and pk == 7 and kk == 3:
        def cat_map(nfeat):     # weight input channel -> logical channel of [diff(3) 0 | features]
            return [0, 1, 2] + list(range(4, 4 + nfeat))

        yield L_TEXT, pack_text_rec_rows_h(wt, wr, range(c1), c1), _bias_pad(np.concatenate([bt, br]), 64, 32), c1, 4, pk, hck
        yield L_PX1, pack_mfma_h(w1, cat_map(c1), 4 + c1), _bias_pad(b1), 4 + c1, pm1, pk, hck
        yield L_PX2, pack_mfma_h(w2, cat_map(pm1), 4 + pm1), _bias_pad(b2), 4 + pm1, pm2, pk, hck
        yield L_OUT, pack_rows_h(wo, cat_map(pm2), 4 + pm2), _bias_pad(bo, 64, 32), 4 + pm2, 1, pk, hck
        return
    # Everything else: the round-1 layout, one (diff | features | zero pad) buffer per stage and VALU kernels for the heads.
    s0, s1, s2 = _pad8(3 + c1), _pad8(3 + pm1), _pad8(3 + pm2)
    yield L_TEXT, pack_small(wt, range(3, 3 + c1), s0), _bias_pad(bt, 4), s0, 1, pk, 8
    yield L_REC, pack_small(wr, range(3, 3 + c1), s0), _bias_pad(br, 4), s0, 3, kk, 8
    for layer, (w, b), feat, s, cout in ((L_PX1, (w1, b1), c1, s0, pm1), (L_PX2, (w2, b2), pm1, s1, pm2)):
        wpk, ck = (pack_mfma_h(w, range(3 + feat), s), hck) if h else (pack_mfma(w, 8, range(3 + feat), s), 8)
        yield layer, wpk, _bias_pad(b), s, cout, pk, ck
    yield L_OUT, pack_small(wo, range(3 + pm2), s2), _bias_pad(bo, 4), s2, 1, pk, 8
