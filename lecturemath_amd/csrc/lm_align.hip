// lm_align.hip -- translation alignment of binary images (Aligner.computeTranslationAlignment, AccessMath/preprocessing/content/
// aligner.py:27-83; called by Evaluator.keyframes_alignments and Evaluator.parallel_keyframe_align) as bit-row work on the device.
// Included by lm_api.hip.
//
// LmAlign holds up to max_images images of one W x H frame size as bit rows: bit (x & 31) of word [image][y][x >> 5] is set where the
// pixel equals content_lum, bits past W are zero.  Two things are asked of it:
//   lm_align_set_images   packs uint8 images (host or device, any pixel stride: channel 0 of an HWC keyframe is read in place) and
//                         counts every image's ink (lm_k_align_pack)
//   lm_align_run          for a list of image pairs (i, j) and a window w the (2w + 1)^2 numbers
//                             matches[dy + w][dx + w] = #{(y, x) : image i has ink at (y, x) and image j at (y - dy, x - dx)}
//                         = sum over y of popcount(A[y] & shift(B[y - dy], dx))           (lm_k_align_match)
// Everything is integer, so the counts do not depend on the order of the additions; the f-score, recall and precision the reference
// derives from them are three divisions per displacement on the host (lecturemath_amd/device/align.py: TranslationAligner).
//
// Limits (checked): W, H <= 32768 (the frame limit of lm_kf_*), hence H * W <= 2^30 and every count fits the int32 table;
// window <= LM_ALIGN_MAX_WINDOW and <= min(W, H) (beyond that the reference's slices turn empty or misshapen and it raises).
#define LM_ALIGN_MAX_WINDOW 128
#define LM_AL_ROWS 32                       // rows of a workgroup's block ...
#define LM_AL_LDS_BYTES (48 * 1024)         // ... fewer when the two staged row blocks would not fit this much LDS

// A wave per 64 consecutive pixels of a row: the ballot of (pixel == lum) is two words of the row.  grid.y strides over the images,
// grid.x over the (row, 64-pixel chunk) units of an image; a wave adds its ink to the image's total once.
__global__ void __launch_bounds__(256) lm_k_align_pack(const uint8_t* __restrict__ src, long long pixel_stride, int n_images, int W, int H, int nw,
                                                       int lum, uint32_t* __restrict__ bits, unsigned long long* __restrict__ totals)
{
    const int lane = lm_lane();
    const int chunks = (W + 63) >> 6;
    const long long units = (long long)H * chunks;
    const long long wave0 = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * (blockDim.x >> 6);
    for (int img = blockIdx.y; img < n_images; img += gridDim.y) {
        const uint8_t* s = src + (long long)img * H * W * pixel_stride;
        uint32_t* out = bits + (long long)img * H * nw;
        unsigned long long ink = 0;
        for (long long u = wave0; u < units; u += nwaves) {                // the same trips for every lane of a wave
            const int y = (int)(u / chunks), c = (int)(u - (long long)y * chunks);
            const int x = 64 * c + lane;
            const bool on = x < W && (int)s[((long long)y * W + x) * pixel_stride] == lum;
            const unsigned long long m = __ballot(on);
            uint32_t* row = out + (long long)y * nw;
            if (lane == 0) row[2 * c] = (uint32_t)m;
            if (lane == 32 && 2 * c + 1 < nw) row[2 * c + 1] = (uint32_t)(m >> 32);
            ink += (unsigned long long)__popcll(m);
        }
        if (lane == 0 && ink) atomicAdd(&totals[img], ink);
    }
}

// Workgroup per (pair, dy, block of R rows).  LDS: the block's rows of A, the rows y - dy of B with hw zero words on either side
// (rows outside the image are zero), ndx counters.  Thread slot = (dx, row group): the slots of a wave read a handful of LDS
// addresses (the A word is shared by all dx of a row group, the B words of neighbouring dx are the same or adjacent).
// counts [n_pairs][ndx][ndx] is zeroed by the caller; a workgroup adds once per displacement.
__global__ void __launch_bounds__(256) lm_k_align_match(const uint32_t* __restrict__ bits, const int2* __restrict__ pairs, int n_pairs, int H, int nw,
                                                        int window, int R, unsigned* __restrict__ counts)
{
    LM_DYN_SMEM(smem);
    const int ndx = 2 * window + 1;
    const int hw = ((window + 31) >> 5) + 1;            // zero words beside a row of B: 32 * hw >= window + 32
    const int bw = nw + 2 * hw;
    const int as = nw | 1, bs = bw | 1;                 // odd row strides: the rows of the row groups of a wave start on different banks
    unsigned* sA = (unsigned*)smem;                     // [R][as]
    unsigned* sB = sA + (size_t)R * as;                 // [R][bs]
    unsigned* sC = sB + (size_t)R * bs;                 // [ndx]
    const int nrb = (H + R - 1) / R;
    const long long img_words = (long long)H * nw;
    const long long units = (long long)n_pairs * ndx * nrb;
    const int T = (int)blockDim.x;
    const int G = ndx < T ? T / ndx : 1;                // row groups
    for (long long unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const int rb = (int)(unit % nrb);
        const int dyi = (int)((unit / nrb) % ndx);
        const int p = (int)(unit / ((long long)nrb * ndx));
        const int dy = dyi - window, y0 = rb * R;
        const int rows = (H - y0 < R) ? H - y0 : R;
        const int2 pr = pairs[p];
        const uint32_t* A = bits + (long long)pr.x * img_words;
        const uint32_t* B = bits + (long long)pr.y * img_words;
        __syncthreads();                                // the unit before has read sA / sB / sC
        for (int i = threadIdx.x; i < rows * nw; i += T) {
            const int r = i / nw;
            sA[r * as + (i - r * nw)] = A[(long long)y0 * nw + i];
        }
        for (int i = threadIdx.x; i < rows * bw; i += T) {
            const int r = i / bw, j = i - r * bw - hw;
            const int yb = y0 + r - dy;
            sB[r * bs + j + hw] = (yb >= 0 && yb < H && j >= 0 && j < nw) ? B[(long long)yb * nw + j] : 0u;
        }
        for (int i = threadIdx.x; i < ndx; i += T) sC[i] = 0;
        __syncthreads();
        for (int slot = threadIdx.x; slot < ndx * G; slot += T) {
            const int g = slot / ndx, dxi = slot - g * ndx;
            // word j of B shifted right by dx starts at bit 32 * j - dx of the row = bit s0 + 32 * j of the padded row; s0 >= 32
            const int s0 = 32 * hw - (dxi - window);
            const int sw = s0 >> 5, sh = s0 & 31;       // sw + nw <= bw - 1: the pair of words read last exists
            unsigned cnt = 0;
            for (int r = g; r < rows; r += G) {
                const unsigned* a = sA + r * as;
                const unsigned* b = sB + r * bs + sw;
                unsigned lo = b[0];
                for (int j = 0; j < nw; j++) {
                    const unsigned hi = b[j + 1];
                    const unsigned v = (unsigned)(((((unsigned long long)hi) << 32) | lo) >> sh);
                    cnt += (unsigned)__popc(a[j] & v);
                    lo = hi;
                }
            }
            if (cnt) atomicAdd(&sC[dxi], cnt);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < ndx; i += T)
            if (sC[i]) atomicAdd(&counts[((long long)p * ndx + dyi) * ndx + i], sC[i]);
    }
}

// ================================================================================================
// host side
// ================================================================================================
struct LmAlign {
    int W = 0, H = 0, nw = 0;
    int max_images = 0, max_window = 0;
    int n_images = 0;                           // of the last lm_align_set_images
    void* ws[4] = {nullptr, nullptr, nullptr, nullptr};     // grow-only scratch: bit rows, totals, upload staging, pairs + counts
    size_t ws_cap[4] = {0, 0, 0, 0};
    std::vector<char> stage;                    // host side of the pair upload (alive until the next call)
};

static void* lm_al_scratch(LmAlign* al, int slot, size_t bytes, const char* who)
{
    if (al->ws[slot] && bytes <= al->ws_cap[slot]) return al->ws[slot];
    if (al->ws[slot]) (void)hipFree(al->ws[slot]);
    al->ws[slot] = nullptr; al->ws_cap[slot] = 0;
    const size_t want = bytes + 256;
    if (hipMalloc(&al->ws[slot], want) != hipSuccess) { lm_set_error("%s: hipMalloc(%zu) failed", who, want); return nullptr; }
    al->ws_cap[slot] = want;
    return al->ws[slot];
}

static size_t lm_al_up(size_t v) { return (v + 255) & ~(size_t)255; }

extern "C" LmAlign* lm_align_create(int width, int height, int max_images, int max_window, void* stream)
{
    (void)stream;
    if (width <= 0 || height <= 0 || width > 32768 || height > 32768 || max_images < 1 || max_window < 0 || max_window > LM_ALIGN_MAX_WINDOW) {
        lm_set_error("lm_align_create: bad arguments (frame %d x %d, limit 32768 x 32768; max_images=%d; max_window=%d, limit %d)", width, height,
                     max_images, max_window, LM_ALIGN_MAX_WINDOW);
        return nullptr;
    }
    LmAlign* al = new LmAlign();
    al->W = width; al->H = height; al->nw = (width + 31) >> 5;
    al->max_images = max_images; al->max_window = max_window;
    return al;
}

extern "C" void lm_align_destroy(LmAlign* al)
{
    if (!al) return;
    for (void* p : al->ws)
        if (p) (void)hipFree(p);
    delete al;
}

extern "C" int lm_align_set_images(LmAlign* al, const uint8_t* images, int on_device, int n_images, int64_t pixel_stride, int content_lum, void* stream)
{
    if (!al || n_images < 0 || pixel_stride < 1 || (n_images > 0 && !images)) {
        lm_set_error("lm_align_set_images: bad arguments (null pointer, n_images=%d, pixel_stride=%lld)", n_images, (long long)pixel_stride);
        return LM_ERR_ARG;
    }
    if (n_images > al->max_images) {
        lm_set_error("lm_align_set_images: %d images, the handle was created for %d", n_images, al->max_images);
        return LM_ERR_CAPACITY;
    }
    al->n_images = 0;
    if (n_images == 0) return LM_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t img_words = (size_t)al->H * al->nw, img_px = (size_t)al->H * al->W;
    uint32_t* d_bits = (uint32_t*)lm_al_scratch(al, 0, (size_t)n_images * img_words * sizeof(uint32_t), "lm_align_set_images");
    unsigned long long* d_tot = (unsigned long long*)lm_al_scratch(al, 1, (size_t)al->max_images * sizeof(unsigned long long), "lm_align_set_images");
    if (!d_bits || !d_tot) return LM_ERR_HIP;
    LM_HIP(hipMemsetAsync(d_tot, 0, (size_t)n_images * sizeof(unsigned long long), st));
    const long long units = (long long)al->H * ((al->W + 63) >> 6);
    const unsigned gx = (unsigned)std::min<long long>((units + 3) / 4, LM_HIP_EMULATED ? 1 : 64);
    if (on_device) {
        hipLaunchKernelGGL(lm_k_align_pack, dim3(gx, (unsigned)std::min(n_images, LM_HIP_EMULATED ? 1 : 4096)), dim3(256), 0, st, images,
                           (long long)pixel_stride, n_images, al->W, al->H, al->nw, content_lum, d_bits, d_tot);
        LM_HIP(hipGetLastError());
    } else {
        // host images go through a staging buffer of at most ~64 MB, a few images at a time; the last pixel read of a chunk is its
        // last byte copied (the caller's pointer may be offset to another channel)
        const size_t per_img = img_px * (size_t)pixel_stride;
        const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_images, ((size_t)64 << 20) / per_img));
        uint8_t* d_src = (uint8_t*)lm_al_scratch(al, 2, (size_t)chunk * per_img, "lm_align_set_images");
        if (!d_src) return LM_ERR_HIP;
        for (int first = 0; first < n_images; first += chunk) {
            const int cnt = std::min(chunk, n_images - first);
            const size_t bytes = ((size_t)cnt * img_px - 1) * (size_t)pixel_stride + 1;
            LM_HIP(hipMemcpyAsync(d_src, images + (size_t)first * per_img, bytes, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(lm_k_align_pack, dim3(gx, (unsigned)std::min(cnt, LM_HIP_EMULATED ? 1 : 4096)), dim3(256), 0, st, (const uint8_t*)d_src,
                               (long long)pixel_stride, cnt, al->W, al->H, al->nw, content_lum, d_bits + (size_t)first * img_words, d_tot + first);
            LM_HIP(hipGetLastError());
        }
        LM_HIP(hipStreamSynchronize(st));       // the caller's host memory has been read when the call returns
    }
    al->n_images = n_images;
    return LM_OK;
}

extern "C" int lm_align_totals(LmAlign* al, int64_t* h_totals, void* stream)
{
    if (!al || (al->n_images > 0 && !h_totals)) { lm_set_error("lm_align_totals: bad arguments (null pointer)"); return LM_ERR_ARG; }
    if (al->n_images == 0) return LM_OK;
    LM_HIP(hipMemcpyAsync(h_totals, al->ws[1], (size_t)al->n_images * sizeof(int64_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
    LM_HIP(hipStreamSynchronize((hipStream_t)stream));
    return LM_OK;
}

extern "C" int lm_align_run(LmAlign* al, const int32_t* h_pairs, int n_pairs, int max_window, int32_t* h_matches, void* stream)
{
    if (!al || n_pairs < 0 || (n_pairs > 0 && (!h_pairs || !h_matches))) {
        lm_set_error("lm_align_run: bad arguments (null pointer, n_pairs=%d)", n_pairs);
        return LM_ERR_ARG;
    }
    if (max_window < 0 || max_window > al->max_window || max_window > LM_ALIGN_MAX_WINDOW || max_window > std::min(al->W, al->H)) {
        lm_set_error("lm_align_run: max_window=%d outside 0 .. %d (the handle's capacity %d, the library's limit %d, min(width, height) = %d)",
                     max_window, std::min(std::min(al->max_window, LM_ALIGN_MAX_WINDOW), std::min(al->W, al->H)), al->max_window, LM_ALIGN_MAX_WINDOW,
                     std::min(al->W, al->H));
        return LM_ERR_ARG;
    }
    for (int k = 0; k < 2 * n_pairs; k++)
        if (h_pairs[k] < 0 || h_pairs[k] >= al->n_images) {
            lm_set_error("lm_align_run: pair %d names image %d, the handle holds %d", k / 2, h_pairs[k], al->n_images);
            return LM_ERR_ARG;
        }
    if (n_pairs == 0) return LM_OK;
    hipStream_t st = (hipStream_t)stream;
    const int ndx = 2 * max_window + 1, hw = ((max_window + 31) >> 5) + 1;
    const size_t row_bytes = (size_t)((al->nw | 1) + ((al->nw + 2 * hw) | 1)) * sizeof(unsigned);      // the kernel's two odd row strides
    const int R = (int)std::max<size_t>(1, std::min<size_t>(LM_AL_ROWS, LM_AL_LDS_BYTES / row_bytes));
    const size_t lds = (size_t)R * row_bytes + (size_t)ndx * sizeof(unsigned);      // <= 48 KB + 1 KB (R >= 5 for the widest frame)
    const size_t o_cnt = lm_al_up((size_t)n_pairs * sizeof(int2)), cnt_bytes = (size_t)n_pairs * ndx * ndx * sizeof(unsigned);
    char* ws = (char*)lm_al_scratch(al, 3, o_cnt + cnt_bytes, "lm_align_run");
    if (!ws) return LM_ERR_HIP;
    al->stage.assign((const char*)h_pairs, (const char*)h_pairs + (size_t)n_pairs * sizeof(int2));
    LM_HIP(hipMemcpyAsync(ws, al->stage.data(), al->stage.size(), hipMemcpyHostToDevice, st));
    LM_HIP(hipMemsetAsync(ws + o_cnt, 0, cnt_bytes, st));
    const long long units = (long long)n_pairs * ndx * ((al->H + R - 1) / R);
    hipLaunchKernelGGL(lm_k_align_match, dim3((unsigned)std::min<long long>(units, LM_HIP_EMULATED ? 2 : (1 << 20))), dim3(256), lds, st,
                       (const uint32_t*)al->ws[0], (const int2*)ws, n_pairs, al->H, al->nw, max_window, R, (unsigned*)(ws + o_cnt));
    LM_HIP(hipGetLastError());
    LM_HIP(hipMemcpyAsync(h_matches, ws + o_cnt, cnt_bytes, hipMemcpyDeviceToHost, st));
    LM_HIP(hipStreamSynchronize(st));
    return LM_OK;
}
