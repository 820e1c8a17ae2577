// lm_history.hip -- the pixel history of a binary stream on the device: for every pixel, in how many frames of a frame range was it
// ink, and when first?  Serves CCStabilityEstimator.compute_group_images_from_raw_binary (cc_stability_estimator.py:502-573) and
// KeyframeExtractor.extract (keyframe_extractor.py:146-222).  Included by lm_api.hip.
//
// LmHistory holds the frames of one stream as bit rows: 32-bit words, wpr = ceil(W / 32) per row, frame after frame, bit = ink --
// the LmBitImage convention (lm_group.hip), a frame being an item at x0 = y0 = 0.  1080p: 259 KB per frame.
//   lm_k_hist_pack       uint8 {0, 255} frames -> bit rows, per-frame ink count (popcount), flag for any other byte
//   lm_k_hist_stats      per pixel of the whole frame: ink count over [t0, t1] and first frame with ink, as float32
//   lm_k_hist_masks      per job (box, frame range, list of mask items) the OR of its mask items, into the output table's bit rows
//   lm_k_hist_job<PASS>  per job the ink count under that mask; pass 0 leaves the job's maximum (atomicMax), pass 1 recomputes the
//                        counts and writes `count >= cut` over the mask
// One thread owns one word of 32 pixels and walks the frames with the counts kept bit-sliced in registers: plane p holds bit p of 32
// counters, adding a word is a ripple of AND / XOR.  16 planes, fully unrolled: a range holds at most 65,535 frames (LM_HIST_MAX_RANGE).
// The four low planes ripple on every frame; the carry out of them (once in 16 inked frames of a pixel) takes the twelve high ones.
#define LM_HIST_PLANES 16
#define LM_HIST_MAX_RANGE 65535
#define LM_HIST_UNROLL 16                   // frame words in flight per thread: whole frames (segments are long) ...
#define LM_HIST_JOB_UNROLL 8                // ... and jobs (an age segment of a group is a few frames)

LM_DEV void lm_hist_add(unsigned (&pl)[LM_HIST_PLANES], unsigned v)
{
    unsigned c = v;
#pragma unroll
    for (int p = 0; p < 4; p++) { const unsigned t = pl[p] & c; pl[p] ^= c; c = t; }
    if (c) {
#pragma unroll
        for (int p = 4; p < LM_HIST_PLANES; p++) { const unsigned t = pl[p] & c; pl[p] ^= c; c = t; }
    }
}

// counter of pixel b
LM_DEV unsigned lm_hist_get(const unsigned (&pl)[LM_HIST_PLANES], int b)
{
    unsigned v = 0;
#pragma unroll
    for (int p = 0; p < LM_HIST_PLANES; p++) v |= ((pl[p] >> b) & 1u) << p;
    return v;
}

// the largest of the 32 counters, read off the planes from the top
LM_DEV unsigned lm_hist_max(const unsigned (&pl)[LM_HIST_PLANES])
{
    unsigned m = 0, cand = 0xffffffffu;
#pragma unroll
    for (int p = LM_HIST_PLANES - 1; p >= 0; p--) {
        const unsigned t = cand & pl[p];
        if (t) { m |= 1u << p; cand = t; }
    }
    return m;
}

// bit b set <=> counter b >= cut (cut < 2^16)
LM_DEV unsigned lm_hist_ge(const unsigned (&pl)[LM_HIST_PLANES], unsigned cut)
{
    unsigned gt = 0, eq = 0xffffffffu;
#pragma unroll
    for (int p = LM_HIST_PLANES - 1; p >= 0; p--) {
        const unsigned cb = ((cut >> p) & 1u) ? 0xffffffffu : 0u;
        gt |= eq & pl[p] & ~cb;
        eq &= ~(pl[p] ^ cb);
    }
    return gt | eq;
}

// ink bits of four {0, 255} bytes (bit 0 of each, gathered by one multiplication whose partial products meet in no bit); any
// byte that is neither 0 nor 255 sets `bad`
LM_DEV unsigned lm_hist_pack4(unsigned q, unsigned& bad)
{
    const unsigned ones = q & 0x01010101u;
    bad |= q ^ (ones * 255u);
    return ((ones * 0x01020408u) >> 24) & 15u;
}

// Grid: x = chunks of a frame's words, y = frames (both strided).  src [n][H][W]; bits / ink point at the first appended frame.
__global__ void __launch_bounds__(256) lm_k_hist_pack(const uint8_t* __restrict__ src, int n, int W, int H, int wpr, uint32_t* __restrict__ bits,
                                                      unsigned* __restrict__ ink, unsigned* __restrict__ flag)
{
    const int fw = H * wpr;
    const bool vec = ((W & 15) == 0) && ((((uintptr_t)src) & 15) == 0);
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        const uint8_t* fsrc = src + (long long)f * H * W;
        unsigned count = 0, bad = 0;
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < fw; i += gridDim.x * blockDim.x) {
            const int y = i / wpr, k = i - y * wpr;
            const uint8_t* p = fsrc + (long long)y * W + k * 32;
            const int lim = (W - k * 32 < 32) ? W - k * 32 : 32;
            unsigned word = 0;
#pragma unroll
            for (int c = 0; c < 2; c++) {
                if (vec && 16 * (c + 1) <= lim) {
                    const uint4 v = *(const uint4*)(p + 16 * c);
                    word |= (lm_hist_pack4(v.x, bad) | (lm_hist_pack4(v.y, bad) << 4) | (lm_hist_pack4(v.z, bad) << 8) | (lm_hist_pack4(v.w, bad) << 12))
                            << (16 * c);
                } else {
                    for (int b = 16 * c; b < lim && b < 16 * (c + 1); b++) {
                        const unsigned v = p[b], one = v & 1u;
                        bad |= v ^ (one * 255u);
                        word |= one << b;
                    }
                }
            }
            bits[(long long)f * fw + i] = word;
            count += (unsigned)__popc(word);
        }
        count = lm_wave_sum(count);
        if (lm_lane() == 0 && count) atomicAdd(&ink[f], count);
        if (bad) atomicOr(flag, 1u);
    }
}

// Thread per word of the frame (fw = H * wpr words).  sum / age [H][W] float32; age = first frame of [t0, t1] with ink, 0 where none.
__global__ void __launch_bounds__(256) lm_k_hist_stats(const uint32_t* __restrict__ bits, int W, int wpr, int fw, int t0, int t1,
                                                       float* __restrict__ sum, float* __restrict__ age)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < fw; i += gridDim.x * blockDim.x) {
        unsigned cnt[LM_HIST_PLANES], first[LM_HIST_PLANES], seen = 0;
#pragma unroll
        for (int p = 0; p < LM_HIST_PLANES; p++) { cnt[p] = 0; first[p] = 0; }
        const uint32_t* src = bits + i;
        int t = t0;
        while (t <= t1) {
            unsigned w[LM_HIST_UNROLL];
#pragma unroll
            for (int u = 0; u < LM_HIST_UNROLL; u++) w[u] = (t + u <= t1) ? src[(long long)(t + u) * fw] : 0u;
#pragma unroll
            for (int u = 0; u < LM_HIST_UNROLL; u++) {
                lm_hist_add(cnt, w[u]);
                const unsigned fresh = w[u] & ~seen;
                if (fresh) {
                    const unsigned rel = (unsigned)(t + u - t0);
#pragma unroll
                    for (int p = 0; p < LM_HIST_PLANES; p++) first[p] |= ((rel >> p) & 1u) ? fresh : 0u;
                    seen |= fresh;
                }
            }
            t += LM_HIST_UNROLL;
        }
        const int y = i / wpr, k = i - y * wpr;
        const int lim = (W - k * 32 < 32) ? W - k * 32 : 32;
        float* so = sum + (long long)y * W + k * 32;
        float* ao = age + (long long)y * W + k * 32;
        for (int b = 0; b < lim; b++) {
            so[b] = (float)lm_hist_get(cnt, b);
            ao[b] = ((seen >> b) & 1u) ? (float)(t0 + (int)lm_hist_get(first, b)) : 0.0f;
        }
    }
}

// A job: the box (x0, y0, w, h) of the output item, the frame range, its mask items (mask_off .. + mask_n in the call's item list),
// word_off = output words of the jobs before it, bits_off = its bit rows in the output table, cut = the count a pixel needs (pass 1).
struct LmHistJob { int32_t x0, y0, w, h, t0, t1, mask_n; uint32_t cut; long long mask_off, word_off, bits_off; };

// The union masks of all jobs, written into the output table's own bit rows (zeroed before): a wave per list entry, a lane per word of
// its mask item, shifted from the item's 32-pixel grid to the job's and clipped to the job's box.  The job kernels read the mask word
// they own from there and pass 1 overwrites it with the result, so no thread scans its job's list and no scratch grows with the area.
__global__ void __launch_bounds__(256) lm_k_hist_masks(const LmHistJob* __restrict__ jobs, const LmBitImage* __restrict__ mitems,
                                                       const int32_t* __restrict__ entry_job, long long n_entries,
                                                       const uint32_t* __restrict__ mbits, uint32_t* __restrict__ out)
{
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long e = wave; e < n_entries; e += n_waves) {
        const LmBitImage it = mitems[e];
        const LmHistJob jb = jobs[entry_job[e]];
        const int ibw = (it.w + 31) >> 5, jbw = (jb.w + 31) >> 5;
        for (int i = lm_lane(); i < it.h * ibw; i += 64) {
            const int yy = i / ibw, k = i - yy * ibw;
            const int Y = it.y0 + yy, col = it.x0 + 32 * k;             // frame row, frame column of the word's bit 0
            if (Y < jb.y0 || Y >= jb.y0 + jb.h) continue;
            unsigned v = mbits[it.bits_off + i];
            const int below = jb.x0 - col, above = col + 32 - (jb.x0 + jb.w);       // columns of the word outside the box
            if (below > 0) v &= below >= 32 ? 0u : 0xffffffffu << below;
            if (above > 0) v &= above >= 32 ? 0u : 0xffffffffu >> above;
            if (!v) continue;
            const int d = col - jb.x0;                                  // job column under bit 0 (> -32 here)
            const int j = d >> 5, sh = d & 31;                          // floor
            uint32_t* row = out + jb.bits_off + (long long)(Y - jb.y0) * jbw;
            if (j >= 0 && (v << sh)) atomicOr(&row[j], v << sh);
            if (sh && j + 1 < jbw && (v >> (32 - sh))) atomicOr(&row[j + 1], v >> (32 - sh));
        }
    }
}

// Thread per output word; `total` words over all jobs; out holds the union masks (lm_k_hist_masks).  PASS 0: job_max[j] = max count.
// PASS 1: out bits = count >= cut, clipped to the box.  A job whose cut is 0 (every pixel) or above its maximum (none) is written
// without a walk over the frames.
template <int PASS>
__global__ void __launch_bounds__(256) lm_k_hist_job(const LmHistJob* __restrict__ jobs, int n_jobs, long long total, const uint32_t* __restrict__ bits,
                                                     int wpr, int fw, unsigned* job_max, uint32_t* __restrict__ out)
{
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long long)gridDim.x * blockDim.x) {
        int a = 0, b = n_jobs;                          // largest j with jobs[j].word_off <= g
        while (b - a > 1) {
            const int mid = (a + b) >> 1;
            if (jobs[mid].word_off <= g) a = mid; else b = mid;
        }
        const LmHistJob jb = jobs[a];
        const int bw = (jb.w + 31) >> 5;
        const int idx = (int)(g - jb.word_off), y = idx / bw, k = idx - y * bw;
        const int Y = jb.y0 + y, col = jb.x0 + 32 * k;
        const unsigned clip = (jb.w - 32 * k < 32) ? (0xffffffffu >> (32 - (jb.w - 32 * k))) : 0xffffffffu;
        if (PASS == 1) {
            const unsigned m = job_max[a];
            if (jb.cut == 0 || jb.cut > m) { out[jb.bits_off + idx] = jb.cut == 0 ? clip : 0u; continue; }
        }
        const unsigned mask = out[jb.bits_off + idx];     // (inside the box already)
        unsigned cnt[LM_HIST_PLANES];
#pragma unroll
        for (int p = 0; p < LM_HIST_PLANES; p++) cnt[p] = 0;
        if (mask) {
            // frame words funnel-shifted to the item's grid; the box lies inside the frame, so word sw exists and sw + 1 is read only where
            // the row has it (a box that touches the right edge: the bits beyond it are cut by `clip`)
            const int sw = col >> 5, sh = col & 31;
            const int hi_off = (sh && sw + 1 < wpr) ? 1 : 0;
            const unsigned hi_keep = hi_off ? 0xffffffffu : 0u;
            const uint32_t* src = bits + (long long)Y * wpr + sw;
            int t = jb.t0;
            while (t <= jb.t1) {
                unsigned lo[LM_HIST_JOB_UNROLL], hi[LM_HIST_JOB_UNROLL];
#pragma unroll
                for (int u = 0; u < LM_HIST_JOB_UNROLL; u++) {
                    const bool in = t + u <= jb.t1;
                    const uint32_t* p = src + (long long)(in ? t + u : jb.t1) * fw;
                    lo[u] = in ? p[0] : 0u;
                    hi[u] = in ? p[hi_off] & hi_keep : 0u;
                }
#pragma unroll
                for (int u = 0; u < LM_HIST_JOB_UNROLL; u++)
                    lm_hist_add(cnt, (unsigned)(((((unsigned long long)hi[u]) << 32) | lo[u]) >> sh) & mask);
                t += LM_HIST_JOB_UNROLL;
            }
        }
        if (PASS == 0) {
            // most words of a large job lie below the maximum its first words left: look before the atomic (a stale value costs one
            // atomic more, never a wrong maximum) -- without the look the 10^4 .. 10^6 atomics of one box on one address are the kernel
            const unsigned m = lm_hist_max(cnt);
            if (m > *(volatile unsigned*)&job_max[a]) atomicMax(&job_max[a], m);
        } else {
            out[jb.bits_off + idx] = lm_hist_ge(cnt, jb.cut) & clip;
        }
    }
}

// ================================================================================================
// host side
// ================================================================================================
struct LmHistory {
    int W = 0, H = 0, wpr = 0, max_frames = 0, n = 0;
    uint32_t* d_bits = nullptr;                 // [max_frames][H][wpr]
    unsigned* d_ink = nullptr;                  // [max_frames] ink pixels per frame, [max_frames]: the bad-byte flag
    std::vector<int64_t> ink;                   // host copy of the committed frames' counts
    void* ws = nullptr;                         // grow-only scratch of lm_hist_masked_images (job table, mask items, maxima)
    size_t ws_cap = 0;
    std::vector<char> stage;                    // host side of its upload (alive until the next call)
};

extern "C" void lm_hist_destroy(LmHistory* h)
{
    if (!h) return;
    if (h->d_bits) (void)hipFree(h->d_bits);
    if (h->d_ink) (void)hipFree(h->d_ink);
    if (h->ws) (void)hipFree(h->ws);
    delete h;
}

extern "C" LmHistory* lm_hist_create(int width, int height, int max_frames)
{
    if (width <= 0 || height <= 0 || width > 32768 || height > 32768 || max_frames <= 0 ||
        (long long)height * ((width + 31) >> 5) > 0x7fffffffLL / 4) {
        lm_set_error("lm_hist_create: bad arguments (frame %d x %d, %d frames)", width, height, max_frames);
        return nullptr;
    }
    LmHistory* h = new LmHistory();
    h->W = width; h->H = height; h->wpr = (width + 31) >> 5; h->max_frames = max_frames;
    const size_t words = (size_t)max_frames * height * h->wpr;
    if (hipMalloc((void**)&h->d_bits, words * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc((void**)&h->d_ink, ((size_t)max_frames + 1) * sizeof(unsigned)) != hipSuccess) {
        lm_set_error("lm_hist_create: hipMalloc failed (%zu bytes of bit rows)", words * sizeof(uint32_t));
        lm_hist_destroy(h);
        return nullptr;
    }
    return h;
}

extern "C" int lm_hist_count(const LmHistory* h) { return h ? h->n : -1; }

extern "C" int lm_hist_truncate(LmHistory* h, int n_frames)
{
    if (!h || n_frames < 0 || n_frames > h->n) { lm_set_error("lm_hist_truncate: bad arguments (null handle, or not 0 <= n_frames <= count)"); return LM_ERR_ARG; }
    h->n = n_frames;
    h->ink.resize((size_t)n_frames);
    return LM_OK;
}

extern "C" int lm_hist_append(LmHistory* h, const uint8_t* d_frames, int n, void* stream)
{
    if (!h || n < 0 || (n > 0 && !d_frames)) { lm_set_error("lm_hist_append: bad arguments"); return LM_ERR_ARG; }
    if (n == 0) return LM_OK;
    if ((long long)h->n + n > h->max_frames) {
        lm_set_error("lm_hist_append: %d + %d frames, room for %d", h->n, n, h->max_frames);
        return LM_ERR_CAPACITY;
    }
    hipStream_t st = (hipStream_t)stream;
    const int fw = h->H * h->wpr;
    unsigned* d_flag = h->d_ink + h->max_frames;
    LM_HIP(hipMemsetAsync(h->d_ink + h->n, 0, (size_t)n * sizeof(unsigned), st));
    LM_HIP(hipMemsetAsync(d_flag, 0, sizeof(unsigned), st));
    const dim3 grid(LM_HIP_EMULATED ? 1 : lm_blocks(fw, 256, 64), (unsigned)std::min(n, LM_HIP_EMULATED ? 2 : 1024));
    hipLaunchKernelGGL(lm_k_hist_pack, grid, dim3(256), 0, st, d_frames, n, h->W, h->H, h->wpr, h->d_bits + (size_t)h->n * fw, h->d_ink + h->n, d_flag);
    LM_HIP(hipGetLastError());
    std::vector<unsigned> got((size_t)n);
    unsigned flag = 0;
    LM_HIP(hipMemcpyAsync(got.data(), h->d_ink + h->n, (size_t)n * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    LM_HIP(hipMemcpyAsync(&flag, d_flag, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    LM_HIP(hipStreamSynchronize(st));
    if (flag) {
        lm_set_error("lm_hist_append: a frame holds a byte that is neither 0 nor 255");
        return LM_ERR_ARG;
    }
    for (unsigned v : got) h->ink.push_back((int64_t)v);
    h->n += n;
    return LM_OK;
}

extern "C" int lm_hist_ink_counts(const LmHistory* h, int first, int n, int64_t* h_counts)
{
    if (!h || first < 0 || n < 0 || (long long)first + n > h->n || (n > 0 && !h_counts)) {
        lm_set_error("lm_hist_ink_counts: bad arguments (null pointer, or frames outside the history)");
        return LM_ERR_ARG;
    }
    for (int i = 0; i < n; i++) h_counts[i] = h->ink[(size_t)first + i];
    return LM_OK;
}

extern "C" int lm_hist_read_bits(const LmHistory* h, int first, int n, uint32_t* h_words, void* stream)
{
    if (!h || first < 0 || n < 0 || (long long)first + n > h->n || (n > 0 && !h_words)) {
        lm_set_error("lm_hist_read_bits: bad arguments (null pointer, or frames outside the history)");
        return LM_ERR_ARG;
    }
    if (n == 0) return LM_OK;
    const size_t fw = (size_t)h->H * h->wpr;
    LM_HIP(hipMemcpyAsync(h_words, h->d_bits + (size_t)first * fw, (size_t)n * fw * sizeof(uint32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
    LM_HIP(hipStreamSynchronize((hipStream_t)stream));
    return LM_OK;
}

static bool lm_hist_range_ok(const LmHistory* h, int t0, int t1, const char* who)
{
    if (t0 < 0 || t1 < t0 || t1 >= h->n) {
        lm_set_error("%s: frame range [%d, %d] outside the %d frames held (or empty)", who, t0, t1, h->n);
        return false;
    }
    if ((long long)t1 - t0 + 1 > LM_HIST_MAX_RANGE) {
        lm_set_error("%s: frame range [%d, %d] is longer than %d frames", who, t0, t1, LM_HIST_MAX_RANGE);
        return false;
    }
    return true;
}

extern "C" int lm_hist_segment_stats(LmHistory* h, int t0, int t1, float* d_sum, float* d_age, void* stream)
{
    if (!h || !d_sum || !d_age) { lm_set_error("lm_hist_segment_stats: bad arguments"); return LM_ERR_ARG; }
    if (!lm_hist_range_ok(h, t0, t1, "lm_hist_segment_stats")) return LM_ERR_ARG;
    const int fw = h->H * h->wpr;
    hipLaunchKernelGGL(lm_k_hist_stats, dim3(LM_HIP_EMULATED ? 2 : lm_blocks(fw, 256)), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)h->d_bits, h->W,
                       h->wpr, fw, t0, t1, d_sum, d_age);
    LM_HIP(hipGetLastError());
    return LM_OK;
}

// the count a pixel needs: ((c * 255) // m) > threshold  <=>  c * 255 >= k * m with k = floor(threshold) + 1 (m > 0); numpy's
// int32 // 0 yields 0, so m == 0 keeps nothing for threshold >= 0 and everything below
static uint32_t lm_hist_cut(double threshold, unsigned m)
{
    if (threshold < 0.0) return 0;
    if (threshold >= 255.0) return LM_HIST_MAX_RANGE + 1;           // c * 255 // m <= 255
    const long long k = (long long)floor(threshold) + 1;
    if (m == 0) return 1;
    return (uint32_t)((k * (long long)m + 254) / 255);
}

extern "C" LmKeyframes* lm_hist_masked_images(LmHistory* h, LmKeyframes* masks, const int32_t* h_boxes, const int32_t* h_ranges, const int64_t* h_list_off,
                                              const int32_t* h_list_items, int n_jobs, double threshold, int64_t* h_max_out, void* stream)
{
    if (!h || !masks || n_jobs < 0 || (n_jobs > 0 && (!h_boxes || !h_ranges)) || !(threshold == threshold) ||
        !lm_kf_lists_ok(masks, h_list_off, h_list_items, n_jobs)) {
        lm_set_error("lm_hist_masked_images: bad arguments (null pointer, NaN threshold, offsets that descend or do not start at 0, or a mask item "
                     "outside the table)");
        return nullptr;
    }
    if (masks->W != h->W || masks->H != h->H) {
        lm_set_error("lm_hist_masked_images: masks placed in %d x %d, frames are %d x %d", masks->W, masks->H, h->W, h->H);
        return nullptr;
    }
    const int64_t E = h_list_off[n_jobs];
    const size_t o_items = lm_kf_up((size_t)std::max(n_jobs, 1) * sizeof(LmHistJob));
    const size_t o_ejob = o_items + lm_kf_up((size_t)std::max<int64_t>(E, 1) * sizeof(LmBitImage));
    const size_t o_max = o_ejob + lm_kf_up((size_t)std::max<int64_t>(E, 1) * sizeof(int32_t));
    const size_t bytes = o_max + (size_t)std::max(n_jobs, 1) * sizeof(unsigned);
    std::vector<char>& up = h->stage;
    up.assign(bytes, 0);
    LmHistJob* jobs = (LmHistJob*)up.data();
    std::vector<LmBitImage> items((size_t)n_jobs);
    long long words = 0, src = 0;
    for (int j = 0; j < n_jobs; j++) {
        const int32_t* bx = h_boxes + (size_t)j * 4;
        if (bx[0] < 0 || bx[2] < 0 || bx[1] < bx[0] || bx[3] < bx[2] || bx[1] >= h->W || bx[3] >= h->H) {
            lm_set_error("lm_hist_masked_images: job %d: box (%d, %d, %d, %d) outside the %d x %d frame", j, bx[0], bx[1], bx[2], bx[3], h->W, h->H);
            return nullptr;
        }
        if (!lm_hist_range_ok(h, h_ranges[2 * j], h_ranges[2 * j + 1], "lm_hist_masked_images")) return nullptr;
        LmHistJob& jb = jobs[j];
        jb.x0 = bx[0]; jb.y0 = bx[2]; jb.w = bx[1] - bx[0] + 1; jb.h = bx[3] - bx[2] + 1;
        jb.t0 = h_ranges[2 * j]; jb.t1 = h_ranges[2 * j + 1];
        jb.mask_off = h_list_off[j]; jb.mask_n = (int32_t)(h_list_off[j + 1] - h_list_off[j]);
        jb.word_off = jb.bits_off = words; jb.cut = 0;
        LmBitImage& im = items[(size_t)j];
        im.x0 = jb.x0; im.y0 = jb.y0; im.w = jb.w; im.h = jb.h; im.src_off = src; im.bits_off = words;
        words += (long long)jb.h * ((jb.w + 31) >> 5);
        src += (long long)jb.w * jb.h;
    }
    for (int64_t e = 0; e < E; e++) ((LmBitImage*)(up.data() + o_items))[e] = masks->items[(size_t)h_list_items[e]];
    for (int j = 0; j < n_jobs; j++)
        for (int64_t e = h_list_off[j]; e < h_list_off[j + 1]; e++) ((int32_t*)(up.data() + o_ejob))[e] = j;
    LmKeyframes* kf = lm_kf_new(h->W, h->H, "lm_hist_masked_images");
    if (!kf) return nullptr;
    kf->items.swap(items);
    if (n_jobs == 0) return kf;
    hipStream_t st = (hipStream_t)stream;
    if (bytes > h->ws_cap) {
        if (h->ws) (void)hipFree(h->ws);
        h->ws = nullptr; h->ws_cap = 0;
        const size_t want = bytes + bytes / 4 + 256;
        if (hipMalloc(&h->ws, want) == hipSuccess) h->ws_cap = want;
    }
    bool ok = h->ws != nullptr && hipMalloc((void**)&kf->d_owned, (size_t)words * sizeof(uint32_t)) == hipSuccess;
    std::vector<unsigned> maxima((size_t)n_jobs);
    if (ok) {
        char* ws = (char*)h->ws;
        const LmHistJob* d_jobs = (const LmHistJob*)ws;
        const LmBitImage* d_items = (const LmBitImage*)(ws + o_items);
        unsigned* d_max = (unsigned*)(ws + o_max);
        const int fw = h->H * h->wpr;
        const dim3 grid(LM_HIP_EMULATED ? 2 : lm_blocks(words, 256, 1 << 16));
        ok = hipMemcpyAsync(ws, up.data(), bytes, hipMemcpyHostToDevice, st) == hipSuccess &&        // (the maxima start at 0)
             hipMemsetAsync(kf->d_owned, 0, (size_t)words * sizeof(uint32_t), st) == hipSuccess;
        if (ok) {
            if (E > 0)
                hipLaunchKernelGGL(lm_k_hist_masks, dim3(LM_HIP_EMULATED ? 2 : lm_blocks(E, 4, 1 << 16)), dim3(256), 0, st, d_jobs, d_items,
                                   (const int32_t*)(ws + o_ejob), (long long)E, masks->d_bits, kf->d_owned);
            hipLaunchKernelGGL((lm_k_hist_job<0>), grid, dim3(256), 0, st, d_jobs, n_jobs, words, (const uint32_t*)h->d_bits, h->wpr, fw, d_max,
                               kf->d_owned);
            ok = hipGetLastError() == hipSuccess &&
                 hipMemcpyAsync(maxima.data(), d_max, (size_t)n_jobs * sizeof(unsigned), hipMemcpyDeviceToHost, st) == hipSuccess &&
                 hipStreamSynchronize(st) == hipSuccess;
        }
        if (ok) {
            for (int j = 0; j < n_jobs; j++) jobs[j].cut = lm_hist_cut(threshold, maxima[(size_t)j]);
            ok = hipMemcpyAsync(ws, up.data(), (size_t)n_jobs * sizeof(LmHistJob), hipMemcpyHostToDevice, st) == hipSuccess;
        }
        if (ok) {
            hipLaunchKernelGGL((lm_k_hist_job<1>), grid, dim3(256), 0, st, d_jobs, n_jobs, words, (const uint32_t*)h->d_bits, h->wpr, fw, d_max,
                               kf->d_owned);
            ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
        }
    }
    if (!ok) {
        lm_set_error("lm_hist_masked_images: HIP error (%d jobs, %lld output words)", n_jobs, words);
        lm_kf_destroy(kf);
        return nullptr;
    }
    kf->d_bits = kf->d_owned;
    if (h_max_out)
        for (int j = 0; j < n_jobs; j++) h_max_out[j] = (int64_t)maxima[(size_t)j];
    return kf;
}
