// lm_ctx.hip -- the labelling context and its entry points: lm_ctx_*, lm_threshold*, lm_fcn_bytes, lm_label_*, lm_cc_stats_* (batched
// scipy.ndimage.label of labeler.py:126 and the CC_AgeBoundaries arrays of accessmath_lib.c:357-413).  Included by lm_api.hip after
// lm_cc_kernels.hip and lm_fcn_bytes.hip, whose kernels it launches.

// LM_DEBUG_BAND_PHASES=2 makes lm_k_band leave every band's unions to lm_k_band_union_global (results unchanged); default 3
static int lm_debug_band_phases()
{
    static int v = -1;
    if (v < 0) { const char* e = getenv("LM_DEBUG_BAND_PHASES"); v = e ? atoi(e) : 3; if (v < 2 || v > 3) v = 3; }
    return v;
}

// LM_DEBUG_BAND_STAMPS=<file>: lm_k_band leaves wall-clock stamps per phase and workgroup (8 x u64 each); the last launch's are
// written to <file> by lm_label_counts (tools/band_phases.py reads them).  Tuning aid only.
static unsigned long long* g_band_stamps = nullptr;
static size_t g_band_stamps_n = 0;
static unsigned long long* lm_debug_band_stamps(int nbands, int n_frames)
{
    static const char* path = getenv("LM_DEBUG_BAND_STAMPS");
    if (!path) return nullptr;
    const size_t need = (size_t)nbands * n_frames * 8;
    if (need > g_band_stamps_n) {
        if (g_band_stamps) (void)hipFree(g_band_stamps);
        g_band_stamps = nullptr;
        if (hipMalloc((void**)&g_band_stamps, need * sizeof(unsigned long long)) != hipSuccess) return nullptr;
        g_band_stamps_n = need;
    }
    return g_band_stamps;
}

// ------------------------------------------------------------------------------------------------
// live profiling (event pairs around the labelling launch sequence)
// ------------------------------------------------------------------------------------------------
#include <mutex>
#include <vector>
struct LmProfile {
    std::vector<hipEvent_t> ev;     // pairs: start, stop
    std::vector<int> frames;
    size_t used = 0;                // pairs in use since the last read
};

static void lm_profile_free(LmCtx* c)
{
    LmProfile* p = (LmProfile*)c->prof;
    if (!p) return;
    for (hipEvent_t e : p->ev) (void)hipEventDestroy(e);
    delete p;
    c->prof = nullptr;
}

extern "C" int lm_ctx_set_profiling(LmCtx* c, int enable)
{
    if (!c) { lm_set_error("lm_ctx_set_profiling: null ctx"); return LM_ERR_ARG; }
    c->profiling = enable ? 1 : 0;
    if (enable && !c->prof) c->prof = new LmProfile();
    return LM_OK;
}

extern "C" int lm_ctx_profile_read(LmCtx* c, double* total_ms, int64_t* calls, int64_t* frames)
{
    if (!c || !total_ms || !calls || !frames) { lm_set_error("lm_ctx_profile_read: bad arguments"); return LM_ERR_ARG; }
    *total_ms = 0.0; *calls = 0; *frames = 0;
    LmProfile* p = (LmProfile*)c->prof;
    if (!p) return LM_OK;
    for (size_t i = 0; i < p->used; i++) {
        float ms = 0.f;
        LM_HIP(hipEventSynchronize(p->ev[2 * i + 1]));
        LM_HIP(hipEventElapsedTime(&ms, p->ev[2 * i], p->ev[2 * i + 1]));
        *total_ms += ms;
        *frames += p->frames[i];
    }
    *calls = (int64_t)p->used;
    p->used = 0;
    return LM_OK;
}

static int lm_profile_mark(LmCtx* c, hipStream_t st, bool start, int n_frames)
{
    LmProfile* p = (LmProfile*)c->prof;
    if (!c->profiling || !p) return LM_OK;
    if (start) {
        if (p->ev.size() < 2 * (p->used + 1)) {
            hipEvent_t a, b;
            LM_HIP(hipEventCreate(&a));
            LM_HIP(hipEventCreate(&b));
            p->ev.push_back(a);
            p->ev.push_back(b);
            p->frames.push_back(0);
        }
        p->frames[p->used] = n_frames;
        LM_HIP(hipEventRecord(p->ev[2 * p->used], st));
    } else {
        LM_HIP(hipEventRecord(p->ev[2 * p->used + 1], st));
        p->used++;
    }
    return LM_OK;
}

// ------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------
extern "C" void lm_ctx_destroy(LmCtx* c)
{
    if (!c) return;
    lm_profile_free(c);
    void* ptrs[] = {c->bits, c->starts, c->prefix, c->rowoff, c->rowcnt, c->band_runs, c->band_base, c->band_roots, c->band_fallback, c->parent, c->final_label,
                    c->n_labels, c->rootbits, c->wordprefix, c->st_min_y, c->st_max_y, c->st_min_x, c->st_max_x, c->st_count, c->kept_label,
                    c->kept_cropoff, c->frame_kept, c->frame_cropwords, c->stage_u8, c->stage_i32, c->stage_f32};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (c->aux_stream) { (void)hipStreamDestroy((hipStream_t)c->aux_stream); (void)hipEventDestroy((hipEvent_t)c->ev_fork); (void)hipEventDestroy((hipEvent_t)c->ev_join); }
    delete c;
}

extern "C" LmCtx* lm_ctx_create(int width, int height, int max_batch)
{
    if (width <= 0 || height <= 0 || max_batch <= 0 || max_batch > 1024 || width > 32767 || height > 32767) {
        lm_set_error("lm_ctx_create: bad arguments (width=%d height=%d max_batch=%d; batch <= 1024, sides <= 32767)",
                     width, height, max_batch);
        return nullptr;
    }
    LmCtx* c = new LmCtx();
    memset(c, 0, sizeof(*c));
    c->g.W = width;
    c->g.H = height;
    c->g.WW = (width + 63) / 64;
    c->band_rows = (c->g.WW > 32) ? 16 : LM_BAND_ROWS_MAX;
    c->nbands = (height + c->band_rows - 1) / c->band_rows;
    c->slot = ((c->band_rows * ((width + 1) / 2)) + 63) & ~63;       // worst-case runs of one band, multiple of 64
    c->g.cap = c->nbands * c->slot;
    c->max_batch = max_batch;
    (void)hipGetDevice(&c->device);
    const size_t R = (size_t)max_batch * height, RW = R * c->g.WW, BC = (size_t)max_batch * c->g.cap;
    int rc = LM_OK;
    rc |= lm_alloc(&c->bits, RW);
    rc |= lm_alloc(&c->starts, RW);
    rc |= lm_alloc(&c->prefix, RW);
    rc |= lm_alloc(&c->rowoff, R);
    rc |= lm_alloc(&c->rowcnt, R);
    rc |= lm_alloc(&c->band_runs, (size_t)max_batch * c->nbands);
    rc |= lm_alloc(&c->band_base, (size_t)max_batch * c->nbands);
    rc |= lm_alloc(&c->band_roots, (size_t)max_batch * c->nbands);
    rc |= lm_alloc(&c->band_fallback, (size_t)max_batch * c->nbands);
    rc |= lm_alloc(&c->parent, BC);
    rc |= lm_alloc(&c->final_label, BC);     // lm_k_stats' lm_load4 may read up to 12 bytes past B * cap: inside lm_alloc's 64 bytes of slack
    rc |= lm_alloc(&c->n_labels, (size_t)max_batch);
    rc |= lm_alloc(&c->rootbits, (size_t)max_batch * (c->g.cap / 64));
    rc |= lm_alloc(&c->wordprefix, (size_t)max_batch * (c->g.cap / 64));
    rc |= lm_alloc(&c->st_min_y, BC);
    rc |= lm_alloc(&c->st_max_y, BC);
    rc |= lm_alloc(&c->st_min_x, BC);
    rc |= lm_alloc(&c->st_max_x, BC);
    rc |= lm_alloc(&c->st_count, BC);
    rc |= lm_alloc(&c->kept_label, BC);
    rc |= lm_alloc(&c->kept_cropoff, BC);
    rc |= lm_alloc(&c->frame_kept, (size_t)max_batch);
    rc |= lm_alloc(&c->frame_cropwords, (size_t)max_batch);
    if (rc != LM_OK) {
        lm_ctx_destroy(c);
        return nullptr;
    }
    return c;
}

// ------------------------------------------------------------------------------------------------
// threshold
// ------------------------------------------------------------------------------------------------
// x* of lm_k_thr_edge per threshold value, found once per process (0: not yet, 1: usable, 2: keep the formula kernel)
static float g_thr_edge[256];
static int g_thr_state[256];
static std::mutex g_thr_mutex;

static int lm_threshold_edge(int thr, hipStream_t st, float* edge, int* state)
{
    std::lock_guard<std::mutex> lock(g_thr_mutex);
    if (!g_thr_state[thr]) {
        float* d = nullptr;
        float h[2] = {0.0f, 0.0f};
        LM_HIP(hipMalloc(&d, 2 * sizeof(float)));
        hipLaunchKernelGGL(lm_k_thr_edge, dim3(1), dim3(64), 0, st, thr, d);
        const hipError_t e = hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, st);
        const hipError_t e2 = hipStreamSynchronize(st);
        (void)hipFree(d);
        LM_HIP(e);
        LM_HIP(e2);
        g_thr_edge[thr] = h[0];
        g_thr_state[thr] = h[1] == 1.0f ? 1 : 2;
    }
    *edge = g_thr_edge[thr];
    *state = g_thr_state[thr];
    return LM_OK;
}

// Which form a thresholding call takes: the comparison x >= *edge (*cmp = 1) needs buffers that qualify for the caller's vector kernel, a
// threshold the sigmoid can straddle and a verified x* (lm_threshold_edge; its first use per threshold value synchronises the stream
// once); everything else, and LM_THRESHOLD_FORMULA, keeps the per-pixel formula lm_thr_px (*cmp = 0).  lm_threshold, lm_fcn_bytes and
// lm_label_batch_logits all decide here.
static int lm_threshold_form(bool buffers_ok, int thr, hipStream_t st, float* edge, int* cmp)
{
    *edge = 0.0f;
    *cmp = 0;
    if (buffers_ok && thr >= 1 && thr <= 255 && !getenv("LM_THRESHOLD_FORMULA")) {
        int state = 0;
        const int rc = lm_threshold_edge(thr, st, edge, &state);
        if (rc) return rc;
        *cmp = state == 1;
    }
    return LM_OK;
}

extern "C" int lm_threshold(const float* d_logits, uint8_t* d_out, int64_t n, int thr, int invert, void* stream)
{
    if (!d_logits || !d_out || n < 0) { lm_set_error("lm_threshold: bad arguments"); return LM_ERR_ARG; }
    if (n == 0) return LM_OK;
    const bool aligned = ((((uintptr_t)d_logits) & 15) == 0) && ((((uintptr_t)d_out) & 15) == 0);
    float edge = 0.0f;
    int cmp = 0;
    const int rc = lm_threshold_form(aligned, thr, (hipStream_t)stream, &edge, &cmp);
    if (rc) return rc;
    if (cmp) {
        hipLaunchKernelGGL(lm_k_threshold_cmp, dim3(lm_blocks((n + 4095) / 4096, 1, 1 << 20)), dim3(256), 0, (hipStream_t)stream, d_logits, d_out,
                           (long long)n, edge, invert ? 0xffu : 0u);
        LM_HIP(hipGetLastError());
        return LM_OK;
    }
    hipLaunchKernelGGL(lm_k_threshold_invert, dim3(lm_blocks((n + 3) / 4, 256)), dim3(256), 0, (hipStream_t)stream,
                       d_logits, d_out, (long long)n, thr, invert ? 0xffu : 0u);
    LM_HIP(hipGetLastError());
    return LM_OK;
}

extern "C" int lm_threshold_invert(const float* d_logits, uint8_t* d_out, int64_t n, int thr, void* stream)
{
    return lm_threshold(d_logits, d_out, n, thr, 1, stream);
}

// the vector kernel of lm_fcn_bytes for the pairs present (have: bit 0 logit, bit 1 text, bit 2 rec; never 0)
template <int MODE>
static void lm_fcn_bytes_launch(int have, dim3 grid, hipStream_t st, const float* d_logit, const float* d_text, const float* d_rec, long long n, float edge, int thr,
                                unsigned flip, uint8_t* d_binary, uint8_t* d_text_u8, uint8_t* d_rec_bgr)
{
#define LM_FB_CASE(H) \
    case H: hipLaunchKernelGGL((lm_k_fcn_bytes<MODE, H>), grid, dim3(256), 0, st, d_logit, d_text, d_rec, n, edge, thr, flip, d_binary, d_text_u8, d_rec_bgr); break
    switch (have) { LM_FB_CASE(1); LM_FB_CASE(2); LM_FB_CASE(3); LM_FB_CASE(4); LM_FB_CASE(5); LM_FB_CASE(6); LM_FB_CASE(7); }
#undef LM_FB_CASE
}

// The byte images of FCN_LectureNet.binarize from the three heads in one pass (kernels: lm_fcn_bytes.hip).  The vector kernel needs every
// present source and destination 16-byte aligned and, for the planes of d_rec at d_rec + n_px and d_rec + 2 n_px, n_px % 4 == 0; any
// other call takes the scalar kernel as a whole.  Hard bytes are lm_threshold's: the same form decision, the same x*.
extern "C" int lm_fcn_bytes(const float* d_logit, const float* d_text, const float* d_rec, int64_t n_px, int thr, int flags, uint8_t* d_binary,
                            uint8_t* d_text_u8, uint8_t* d_rec_bgr, void* stream)
{
    if ((!d_logit != !d_binary) || (!d_text != !d_text_u8) || (!d_rec != !d_rec_bgr) || (!d_logit && !d_text && !d_rec) || n_px < 0 ||
        (flags & ~(LM_FB_SOFT | LM_FB_INVERT))) {
        lm_set_error("lm_fcn_bytes: bad arguments (every source needs its destination and the reverse, at least one pair, n_px >= 0, flags in %d)",
                     LM_FB_SOFT | LM_FB_INVERT);
        return LM_ERR_ARG;
    }
    if (n_px == 0) return LM_OK;
    const uintptr_t bits = (uintptr_t)d_logit | (uintptr_t)d_text | (uintptr_t)d_rec | (uintptr_t)d_binary | (uintptr_t)d_text_u8 | (uintptr_t)d_rec_bgr;
    const bool vec = (bits & 15) == 0 && (!d_rec || (n_px & 3) == 0);
    const hipStream_t st = (hipStream_t)stream;
    const unsigned flip = (flags & LM_FB_INVERT) ? 0xffu : 0u;
    const long long n = (long long)n_px;
    float edge = 0.0f;
    int cmp = 0;
    if (!(flags & LM_FB_SOFT)) {
        const int rc = lm_threshold_form(vec, thr, st, &edge, &cmp);
        if (rc) return rc;
    }
    const int mode = (flags & LM_FB_SOFT) ? LM_FB_SOFT_BYTES : (cmp ? LM_FB_HARD_CMP : LM_FB_HARD_FORMULA);
    if (vec) {
        const dim3 grid(lm_blocks((n / 16 + 255) / 256, 1, 1 << 20));
        const int have = (d_logit ? 1 : 0) | (d_text ? 2 : 0) | (d_rec ? 4 : 0);
        if (mode == LM_FB_HARD_CMP) lm_fcn_bytes_launch<LM_FB_HARD_CMP>(have, grid, st, d_logit, d_text, d_rec, n, edge, thr, flip, d_binary, d_text_u8, d_rec_bgr);
        else if (mode == LM_FB_HARD_FORMULA) lm_fcn_bytes_launch<LM_FB_HARD_FORMULA>(have, grid, st, d_logit, d_text, d_rec, n, edge, thr, flip, d_binary, d_text_u8, d_rec_bgr);
        else lm_fcn_bytes_launch<LM_FB_SOFT_BYTES>(have, grid, st, d_logit, d_text, d_rec, n, edge, thr, flip, d_binary, d_text_u8, d_rec_bgr);
    } else {
        const dim3 grid(lm_blocks(n, 256));
        if (mode == LM_FB_SOFT_BYTES)
            hipLaunchKernelGGL(lm_k_fcn_bytes_scalar<LM_FB_SOFT_BYTES>, grid, dim3(256), 0, st, d_logit, d_text, d_rec, n, thr, flip, d_binary, d_text_u8, d_rec_bgr);
        else
            hipLaunchKernelGGL(lm_k_fcn_bytes_scalar<LM_FB_HARD_FORMULA>, grid, dim3(256), 0, st, d_logit, d_text, d_rec, n, thr, flip, d_binary, d_text_u8, d_rec_bgr);
    }
    LM_HIP(hipGetLastError());
    return LM_OK;
}

// ------------------------------------------------------------------------------------------------
// labelling
// ------------------------------------------------------------------------------------------------
// The launch sequence of frames [f0, f0 + n) of a batch on stream `st`.  All the per-frame tables of the context are indexed by
// the frame's position in the batch and hold frame-relative ids, so a part of a batch is the same launches on shifted pointers.
// The frames come as {0, non-zero} bytes (d_binary) or -- logits != null -- as fp32 logits thresholded on the fly ((x >= edge ? 255 : 0) ^
// flip; d_binary, when given as well, receives that frame).
struct LmLabelSrc {
    const uint8_t* d_binary;
    const float* logits; float edge; unsigned flip; uint8_t* d_binary_out;
};

// dynamic LDS of lm_k_band: the band's bit rows, run starts and prefixes (18 B per 64-px word), a forest of LM_BAND_LDS runs,
// row offsets and run counts
static inline size_t lm_band_smem(const LmCtx* c) { return (size_t)c->band_rows * c->g.WW * 18 + (size_t)LM_BAND_LDS * 4 + (65 + 64) * 4 + 64; }

static int lm_label_launch(LmCtx* c, const LmLabelSrc& src, int f0, int n, int32_t* d_labels, hipStream_t st)
{
    const uint8_t* d_binary = src.d_binary;
    const LmGeom g = c->g;
    const int nbands = c->nbands, slot = c->slot;
    const int capw = g.cap / 64;
    const unsigned long long magic_ww = ((1ull << 40) / (unsigned)g.WW) + 1;
    const long long R = (long long)n * g.H;
    const size_t px = (size_t)g.W * g.H, r0 = (size_t)f0 * g.H, w0 = r0 * g.WW, b0 = (size_t)f0 * nbands, c0 = (size_t)f0 * g.cap, cw0 = (size_t)f0 * capw;
    if (src.logits)
        hipLaunchKernelGGL(lm_k_pack_rows_logits, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, st, src.logits + f0 * px, src.edge, src.flip,
                           src.d_binary_out ? src.d_binary_out + f0 * px : nullptr, c->bits + w0, c->starts + w0, c->prefix + w0, c->rowcnt + r0, g.W, g.WW, R);
    else
        hipLaunchKernelGGL(lm_k_pack_rows, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, st, d_binary + f0 * px, c->bits + w0, c->starts + w0, c->prefix + w0,
                           c->rowcnt + r0, g.W, g.WW, R);
    hipLaunchKernelGGL(lm_k_band, dim3(nbands, n), dim3(512), lm_band_smem(c), st, c->bits + w0, c->starts + w0, c->prefix + w0, c->rowcnt + r0,
                       c->rowoff + r0, c->band_runs + b0, c->parent + c0, c->band_fallback + b0, g.H, g.WW, slot, g.cap, lm_debug_band_phases(), magic_ww,
                       c->band_rows, f0 == 0 ? lm_debug_band_stamps(nbands, n) : nullptr, LM_BAND_LDS);
    const LmStatInit si = {c->st_min_y + c0, c->st_max_y + c0, c->st_min_x + c0, c->st_max_x + c0, c->st_count + c0, g.W, g.H};
    hipLaunchKernelGGL(lm_k_seam_union, dim3(nbands, n), dim3(256), 0, st, c->bits + w0, c->starts + w0, c->prefix + w0, c->rowoff + r0,
                       c->band_fallback + b0, c->parent + c0, g.WW, g.H, g.cap, c->band_rows);
    hipLaunchKernelGGL(lm_k_flatten_flag, dim3(nbands, n), dim3(256), 0, st, c->parent + c0, c->band_runs + b0, c->rootbits + cw0, c->wordprefix + cw0,
                       c->band_roots + b0, slot, g.cap, capw);
    hipLaunchKernelGGL(lm_k_apply_labels, dim3(nbands, n), dim3(256), 0, st, c->parent + c0, c->band_runs + b0, c->rootbits + cw0, c->wordprefix + cw0,
                       c->band_roots + b0, c->band_base + b0, c->n_labels + f0, c->final_label + c0, slot, g.cap, capw, si);
    if (d_labels) {
        const unsigned Q = (unsigned)(g.W + 3) / 4;
        const unsigned long long magic_q = ((1ull << 40) / Q) + 1;       // lm_fastdiv: exact for H * Q < 2^24
        const long long quads = (long long)g.H * Q;
        // one chunk of 64 * LM_WL_Q quads per wave (measured: work distribution moves this kernel by < 5 %, it runs at the
        // mixed read/write bandwidth of the device)
        const unsigned gx = (unsigned)((quads + 256 * LM_WL_Q - 1) / (256 * LM_WL_Q));
        hipLaunchKernelGGL(lm_k_write_labels, dim3(gx, n), dim3(256), 0, st, c->bits + w0, c->starts + w0, c->prefix + w0, c->rowoff + r0,
                           c->final_label + c0, d_labels + f0 * px, g.W, g.H, g.WW, g.cap, magic_q, 0);
    }
    LM_HIP(hipGetLastError());
    return LM_OK;
}

// Parts of a batch are labelled side by side: the middle of the sequence (band forests, seams, numbering) is a chain of
// latency-bound kernels on ~1/8 of the bytes, its two ends (row packing, the label image) stream at HBM rate -- with the parts on
// two queues the ends of one part run under the middle of the other.  The second queue belongs to the context and is joined back
// into the caller's stream before the call returns, so the caller's ordering is that of a single launch sequence.
static int lm_label_batch_src(LmCtx* c, const LmLabelSrc& src, int n_frames, int32_t* d_labels, void* stream)
{
    if (!c || (!src.d_binary && !src.logits) || n_frames <= 0 || n_frames > c->max_batch) {
        lm_set_error("lm_label_batch: bad arguments (n_frames=%d, max_batch=%d)", n_frames, c ? c->max_batch : -1);
        return LM_ERR_ARG;
    }
    const LmGeom g = c->g;
    hipStream_t st = (hipStream_t)stream;
    if ((long long)g.H * ((g.W + 3) / 4) >= (1ll << 24) && d_labels) { lm_set_error("lm_label_batch: frame too large for the label writer (H*W/4 must be < 2^24)"); return LM_ERR_ARG; }
#if !LM_HIP_EMULATED
    {
        // per call: the attribute belongs to the (function, device) pair and the call is cheap; a process-wide "already configured"
        // flag would skip it on a second device or race between caller threads
        LM_HIP(hipFuncSetAttribute((const void*)lm_k_band, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lm_band_smem(c)));
    }
#endif
    if (lm_profile_mark(c, st, true, n_frames)) return LM_ERR_HIP;
    static const int want_parts = [] { const char* e = getenv("LM_LABEL_PARTS"); const int v = e ? atoi(e) : LM_LABEL_PARTS; return (v >= 1 && v <= 8) ? v : LM_LABEL_PARTS; }();
    int parts = want_parts;
    while (parts > 1 && n_frames / parts < LM_LABEL_PART_MIN) parts--;
    if (parts > 1 && !c->aux_stream) {
        LM_HIP(hipStreamCreateWithFlags((hipStream_t*)&c->aux_stream, hipStreamNonBlocking));
        LM_HIP(hipEventCreateWithFlags((hipEvent_t*)&c->ev_fork, hipEventDisableTiming));
        LM_HIP(hipEventCreateWithFlags((hipEvent_t*)&c->ev_join, hipEventDisableTiming));
    }
    if (parts <= 1) {
        const int rc = lm_label_launch(c, src, 0, n_frames, d_labels, st);
        if (rc) return rc;
    } else {
        hipStream_t aux = (hipStream_t)c->aux_stream;
        LM_HIP(hipEventRecord((hipEvent_t)c->ev_fork, st));
        LM_HIP(hipStreamWaitEvent(aux, (hipEvent_t)c->ev_fork, 0));
        // from here on the second queue holds work: whatever fails below, it is joined back into the caller's stream before the
        // call returns (both queues touch the context's tables and d_binary)
        int rc = LM_OK;
        for (int k = 0, f0 = 0; k < parts && rc == LM_OK; k++) {
            const int n = n_frames / parts + (k < n_frames % parts ? 1 : 0);
            rc = lm_label_launch(c, src, f0, n, d_labels, (k & 1) ? aux : st);
            f0 += n;
        }
        const hipError_t e1 = hipEventRecord((hipEvent_t)c->ev_join, aux);
        const hipError_t e2 = (e1 == hipSuccess) ? hipStreamWaitEvent(st, (hipEvent_t)c->ev_join, 0) : e1;
        if (e2 != hipSuccess) {
            (void)hipStreamSynchronize(aux);        // could not order the queues with an event: drain the second one instead
            if (rc == LM_OK) { lm_set_error("lm_label_batch: joining the second queue failed: %s", hipGetErrorString(e2)); rc = LM_ERR_HIP; }
        }
        if (rc) return rc;
    }
    if (lm_profile_mark(c, st, false, n_frames)) return LM_ERR_HIP;
    c->last_batch = n_frames;
    c->last_fused = src.logits ? 1 : 0;
    c->stats_fresh = 1;
    return LM_OK;
}

extern "C" int lm_label_batch(LmCtx* c, const uint8_t* d_binary, int n_frames, int32_t* d_labels, void* stream)
{
    LmLabelSrc src = {d_binary, nullptr, 0.0f, 0u, nullptr};
    return lm_label_batch_src(c, src, n_frames, d_labels, stream);
}

// Labelling straight from fp32 logits: binary = ((uint8)(sigmoid(x) * 255) >= thr ? 255 : 0), inverted when `invert` (the step-01 worker's
// 255 - binary), 4-connected labels of its non-zero pixels -- lm_threshold + lm_label_batch in one pass over the logits (4 B/px read
// instead of 4 B/px read + 1 B/px written + 1 B/px read).  d_binary may be null; when given it receives the {0, 255} frames.
// Falls back to the two calls (d_binary required then) when the row width is not a multiple of 4 pixels, the buffers are not 16-byte
// aligned or the threshold has no comparison form (lm_threshold_edge).
extern "C" int lm_label_batch_logits(LmCtx* c, const float* d_logits, int n_frames, int thr, int invert, uint8_t* d_binary, int32_t* d_labels, void* stream)
{
    if (!c || !d_logits || n_frames <= 0 || n_frames > c->max_batch) {
        lm_set_error("lm_label_batch_logits: bad arguments (n_frames=%d, max_batch=%d)", n_frames, c ? c->max_batch : -1);
        return LM_ERR_ARG;
    }
    const LmGeom g = c->g;
    float edge = 0.0f;
    int cmp = 0;
    const bool shape_ok = (g.W & 3) == 0 && ((((uintptr_t)d_logits) & 15) == 0) && (!d_binary || ((((uintptr_t)d_binary) & 3) == 0));
    {
        const int rc = lm_threshold_form(shape_ok && !getenv("LM_LABEL_UNFUSED"), thr, (hipStream_t)stream, &edge, &cmp);
        if (rc) return rc;
    }
    if (cmp) {
        LmLabelSrc src = {nullptr, d_logits, edge, invert ? 0xffu : 0u, d_binary};
        return lm_label_batch_src(c, src, n_frames, d_labels, stream);
    }
    if (!d_binary) { lm_set_error("lm_label_batch_logits: this frame shape / threshold needs the two-pass path, which needs d_binary"); return LM_ERR_ARG; }
    const int rc = lm_threshold(d_logits, d_binary, (int64_t)n_frames * g.W * g.H, thr, invert, stream);
    if (rc) return rc;
    return lm_label_batch(c, d_binary, n_frames, d_labels, stream);
}

extern "C" int lm_label_was_fused(LmCtx* c) { return c ? c->last_fused : 0; }

extern "C" int lm_label_counts(LmCtx* c, int32_t* h_counts, void* stream)
{
    if (!c || !h_counts || c->last_batch <= 0) { lm_set_error("lm_label_counts: no labelled batch"); return LM_ERR_STATE; }
    LM_HIP(hipMemcpyAsync(h_counts, c->n_labels, (size_t)c->last_batch * sizeof(int32_t), hipMemcpyDeviceToHost,
                          (hipStream_t)stream));
    LM_HIP(hipStreamSynchronize((hipStream_t)stream));
    if (g_band_stamps && getenv("LM_DEBUG_BAND_STAMPS")) {
        const size_t n = (size_t)c->nbands * c->last_batch * 8;
        unsigned long long* h = (unsigned long long*)malloc(n * sizeof(unsigned long long));
        if (h && hipMemcpy(h, g_band_stamps, n * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess) {
            FILE* f = fopen(getenv("LM_DEBUG_BAND_STAMPS"), "wb");
            if (f) { fwrite(h, sizeof(unsigned long long), n, f); fclose(f); }
        }
        free(h);
    }
    return LM_OK;
}

extern "C" int lm_cc_stats_batch(LmCtx* c, void* stream)
{
    if (!c || c->last_batch <= 0) { lm_set_error("lm_cc_stats_batch: no labelled batch"); return LM_ERR_STATE; }
    const LmGeom g = c->g;
    hipStream_t st = (hipStream_t)stream;
    const int B = c->last_batch;
    // the labelling launch leaves the arrays initialised (lm_k_apply_labels); a second call for the same batch starts over
    if (!c->stats_fresh)
        hipLaunchKernelGGL(lm_k_stats_init, dim3(32, B), dim3(256), 0, st, c->st_min_y, c->st_max_y, c->st_min_x, c->st_max_x,
                           c->st_count, c->n_labels, g.W, g.H, g.cap);
    c->stats_fresh = 0;
    hipLaunchKernelGGL(lm_k_stats, dim3((g.WW + LM_ST_WORDS - 1) / LM_ST_WORDS, (g.H + LM_ST_ROWS - 1) / LM_ST_ROWS, B), dim3(256), 0,
                       st, c->bits, c->starts, c->prefix, c->rowoff, c->final_label, c->st_min_y, c->st_max_y, c->st_min_x,
                       c->st_max_x, c->st_count, g.WW, g.H, g.cap);
    LM_HIP(hipGetLastError());
    return LM_OK;
}

extern "C" int lm_cc_stats_read(LmCtx* c, int frame, int n, int32_t* h_mins_y, int32_t* h_maxs_y, int32_t* h_mins_x,
                                int32_t* h_maxs_x, int32_t* h_counts, void* stream)
{
    if (!c || frame < 0 || frame >= c->last_batch || n < 0 || n > c->g.cap) {
        lm_set_error("lm_cc_stats_read: bad arguments");
        return LM_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t off = (size_t)frame * c->g.cap, nb = (size_t)n * sizeof(int32_t);
    if (n > 0) {
        if (h_mins_y) LM_HIP(hipMemcpyAsync(h_mins_y, c->st_min_y + off, nb, hipMemcpyDeviceToHost, st));
        if (h_maxs_y) LM_HIP(hipMemcpyAsync(h_maxs_y, c->st_max_y + off, nb, hipMemcpyDeviceToHost, st));
        if (h_mins_x) LM_HIP(hipMemcpyAsync(h_mins_x, c->st_min_x + off, nb, hipMemcpyDeviceToHost, st));
        if (h_maxs_x) LM_HIP(hipMemcpyAsync(h_maxs_x, c->st_max_x + off, nb, hipMemcpyDeviceToHost, st));
        if (h_counts) LM_HIP(hipMemcpyAsync(h_counts, c->st_count + off, nb, hipMemcpyDeviceToHost, st));
    }
    LM_HIP(hipStreamSynchronize(st));
    return LM_OK;
}
