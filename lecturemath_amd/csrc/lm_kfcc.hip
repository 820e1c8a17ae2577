// lm_kfcc.hip -- keyframes on the device -> a bit-row table of their connected components (KeyFrameAnnotation.update_binary_cc,
// AccessMath/annotation/keyframe_annotation.py:139-146: Labeler.extractSpatioTemporalContent(255 - binary_image[:, :, 0], zeros,
// False)), and the pixel sums of Evaluator.compute_pixel_binary_metrics (AccessMath/evaluation/evaluator.py).  Included by
// lm_api.hip after lm_ccmatch.hip.
//
// lm_kf_create_from_frames labels the keyframes in batches of the context's max_batch with the labeller's own launch sequence
// (lm_label_batch, lm_cc_stats_batch, lm_k_select, lm_k_batch_offsets, lm_k_emit -- what lm_stream_push_records runs, on
// buffers sized for the batch instead of a stream's capacity).  What that leaves are 32-byte records and crops aligned to
// ABSOLUTE 32-pixel columns of the frame (words min_x >> 5 .. max_x >> 5 per row).  An LmKeyframes item is aligned to its own x0
// (ceil(w / 32) words per row), so one kernel moves every crop of the batch to the item layout:
//   lm_k_kfcc_ink       keyframe bytes at a pixel stride -> the {0, 255} plane the labeller reads (ink iff channel 0 != 255)
//   lm_k_kfcc_convert   a thread per OUTPUT word: two crop words funnel-shifted by min_x & 31, the tail beyond w cleared
//   lm_k_kfcc_sums      per keyframe pair four exact byte sums in one pass over channel 0 of both frames
// Only the records (32 bytes per CC) and two counts per frame cross to the host; it builds the item table from them.
struct LmKfccItem {
    long long src_off;      // first crop word of the CC (relative to the batch's crop array)
    long long dst_off;      // first item word (relative to the batch's bit array); ascending over the batch's items
    int32_t sh;             // min_x & 31
    int32_t src_nw;         // crop words per row
    int32_t w, h;
};

// out[i] = 255 where the byte of pixel i (at in[i * stride]) is not 255.  A thread per four pixels.
__global__ void __launch_bounds__(256) lm_k_kfcc_ink(const uint8_t* __restrict__ in, long long stride, long long n_px, uint8_t* __restrict__ out)
{
    const long long nq = (n_px + 3) >> 2;
    const bool vec_out = ((((uintptr_t)out) & 3) == 0);
    const bool vec_in = stride == 1 && ((((uintptr_t)in) & 3) == 0);
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (long long)gridDim.x * blockDim.x) {
        const long long p0 = q << 2;
        const int m = (n_px - p0 < 4) ? (int)(n_px - p0) : 4;
        unsigned o = 0;
        if (vec_in && m == 4) {
            const unsigned v = *(const unsigned*)(in + p0);
#pragma unroll
            for (int t = 0; t < 4; t++) o |= (((v >> (8 * t)) & 0xffu) != 0xffu ? 0xffu : 0u) << (8 * t);
        } else {
            for (int t = 0; t < m; t++) o |= (in[(p0 + t) * stride] != 0xffu ? 0xffu : 0u) << (8 * t);
        }
        if (vec_out && m == 4) {
            *(unsigned*)(out + p0) = o;
        } else {
            for (int t = 0; t < m; t++) out[p0 + t] = (uint8_t)(o >> (8 * t));
        }
    }
}

// A thread per output word g in [0, n_words): its item is the last one whose dst_off <= g (binary search; the items of a CC-sized
// neighbourhood share cache lines of the table).  Output word k of row y holds box columns 32 k .. 32 k + 31 = crop bits
// sh + 32 k ..: crop words k and k + 1 of the row, funnel-shifted.  Bits at or beyond w are cleared (lm_kf_pair_counts relies on it).
__global__ void __launch_bounds__(256) lm_k_kfcc_convert(const LmKfccItem* __restrict__ items, int n_items, const uint32_t* __restrict__ crop,
                                                         long long n_words, uint32_t* __restrict__ bits)
{
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n_words; g += (long long)gridDim.x * blockDim.x) {
        int a = 0, b = n_items;
        while (b - a > 1) {
            const int mid = (a + b) >> 1;
            if (items[mid].dst_off <= g) a = mid; else b = mid;
        }
        const LmKfccItem it = items[a];
        const int bw = (it.w + 31) >> 5;
        const long long idx = g - it.dst_off;
        const int y = (int)(idx / bw), k = (int)(idx - (long long)y * bw);
        const uint32_t* r = crop + it.src_off + (long long)y * it.src_nw;
        const unsigned lo = r[k];                                       // k < bw <= src_nw
        const unsigned hi = (it.sh && k + 1 < it.src_nw) ? r[k + 1] : 0u;
        unsigned v = it.sh ? ((lo >> it.sh) | (hi << (32 - it.sh))) : lo;
        const int left = it.w - 32 * k;                                 // columns of the box from this word on (>= 1)
        if (left < 32) v &= 0xffffffffu >> (32 - left);
        bits[g] = v;
    }
}

// 64-bit sum over the wave (three 32-bit wave sums of 24-bit slices, as lm_k_frame_sums does)
LM_DEV unsigned long long lm_kfcc_wave_sum64(unsigned long long acc)
{
    const unsigned lo = lm_wave_sum((unsigned)(acc & 0xffffffu)), mid = lm_wave_sum((unsigned)((acc >> 24) & 0xffffffu));
    const unsigned hi = lm_wave_sum((unsigned)(acc >> 48));
    return (unsigned long long)lo + ((unsigned long long)mid << 24) + ((unsigned long long)hi << 48);
}

LM_DEV void lm_kfcc_acc(unsigned g, unsigned s, unsigned m, unsigned long long (&acc)[4])
{
    const unsigned gi = 255u - g, si = 255u - s;
    acc[0] += gi; acc[1] += si;
    if (g != 255u) acc[2] += si;
    if (m == 0u) acc[3] += si;
}

// grid (x, pair).  sums[pair][4] = sum(255 - gt), sum(255 - summ), sum(255 - summ where gt != 255), sum(255 - summ where mask == 0);
// gt / summ read at their pixel strides, the mask ([pixels] bytes per pair, null = all zero) at stride 1.  Both strides 1 and all
// three rows 16-byte aligned: 16-byte loads.
__global__ void __launch_bounds__(256) lm_k_kfcc_sums(const uint8_t* __restrict__ gt, long long stride_gt, const uint8_t* __restrict__ summ,
                                                      long long stride_summ, const uint8_t* __restrict__ mask, long long px,
                                                      unsigned long long* __restrict__ sums)
{
    __shared__ unsigned long long s_acc[4];
    const long long pair = blockIdx.y;
    const uint8_t* g = gt + pair * px * stride_gt;
    const uint8_t* s = summ + pair * px * stride_summ;
    const uint8_t* m = mask ? mask + pair * px : nullptr;
    const bool vec = stride_gt == 1 && stride_summ == 1 && ((((uintptr_t)g) | ((uintptr_t)s) | ((uintptr_t)m)) & 15) == 0;
    unsigned long long acc[4] = {0, 0, 0, 0};
    const long long n16 = vec ? (px >> 4) : 0;
    const long long t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x, nt = (long long)gridDim.x * blockDim.x;
    for (long long i = t0; i < n16; i += nt) {
        const uint4 vg = *(const uint4*)(g + (i << 4)), vs = *(const uint4*)(s + (i << 4));
        const uint4 vm = m ? *(const uint4*)(m + (i << 4)) : make_uint4(0u, 0u, 0u, 0u);
        const unsigned wg[4] = {vg.x, vg.y, vg.z, vg.w}, wsu[4] = {vs.x, vs.y, vs.z, vs.w}, wm[4] = {vm.x, vm.y, vm.z, vm.w};
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
            for (int t = 0; t < 4; t++) lm_kfcc_acc((wg[k] >> (8 * t)) & 0xffu, (wsu[k] >> (8 * t)) & 0xffu, (wm[k] >> (8 * t)) & 0xffu, acc);
    }
    for (long long i = (n16 << 4) + t0; i < px; i += nt) lm_kfcc_acc(g[i * stride_gt], s[i * stride_summ], m ? m[i] : 0u, acc);
    if (threadIdx.x < 4) s_acc[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const unsigned long long w = lm_kfcc_wave_sum64(acc[k]);
        if (lm_lane() == 0 && w) atomicAdd(&s_acc[k], w);
    }
    __syncthreads();
    if (threadIdx.x < 4 && s_acc[threadIdx.x]) atomicAdd(&sums[pair * 4 + threadIdx.x], s_acc[threadIdx.x]);
}

// ================================================================================================
// host side
// ================================================================================================
extern "C" int lm_kf_pixel_sums(const uint8_t* d_gt, int64_t stride_gt, const uint8_t* d_summ, int64_t stride_summ, const uint8_t* d_mask, int n,
                                int64_t pixels, uint64_t* d_sums, void* stream)
{
    if (n < 0 || pixels <= 0 || stride_gt < 1 || stride_summ < 1 || (n > 0 && (!d_gt || !d_summ || !d_sums))) {
        lm_set_error("lm_kf_pixel_sums: bad arguments (n=%d, pixels=%lld, strides %lld / %lld, or a null pointer)", n, (long long)pixels,
                     (long long)stride_gt, (long long)stride_summ);
        return LM_ERR_ARG;
    }
    if (n == 0) return LM_OK;
    hipStream_t st = (hipStream_t)stream;
    LM_HIP(hipMemsetAsync(d_sums, 0, (size_t)n * 4 * sizeof(uint64_t), st));
    long long bx = (pixels / 16 + 255) / 256;
    bx = bx > 256 ? 256 : bx < 1 ? 1 : bx;
    for (int p0 = 0; p0 < n; p0 += 32768) {         // (the grid's y extent ends at 65,535)
        const int m = n - p0 < 32768 ? n - p0 : 32768;
        hipLaunchKernelGGL(lm_k_kfcc_sums, dim3((unsigned)(LM_HIP_EMULATED ? 2 : bx), (unsigned)m), dim3(256), 0, st, d_gt + (size_t)p0 * pixels * stride_gt,
                           (long long)stride_gt, d_summ + (size_t)p0 * pixels * stride_summ, (long long)stride_summ,
                           d_mask ? d_mask + (size_t)p0 * pixels : nullptr, (long long)pixels, (unsigned long long*)d_sums + (size_t)p0 * 4);
    }
    LM_HIP(hipGetLastError());
    return LM_OK;
}

namespace {
// device buffers of one lm_kf_create_from_frames call; whatever is left in it is freed when the call returns
struct LmKfccWork {
    std::vector<void*> owned;
    std::vector<std::pair<uint32_t*, long long>> chunks;    // box-relative bits of every batch (device, words)
    ~LmKfccWork()
    {
        for (void* p : owned)
            if (p) (void)hipFree(p);
        for (auto& c : chunks)
            if (c.first) (void)hipFree(c.first);
    }
    template <class T> bool alloc(T** p, size_t count)
    {
        void* q = nullptr;
        if (hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T) + 64) != hipSuccess) return false;
        owned.push_back(q);
        *p = (T*)q;
        return true;
    }
    void release(void* p)
    {
        for (void*& q : owned)
            if (q == p && p) { (void)hipFree(p); q = nullptr; }
    }
};
}  // namespace

extern "C" LmKeyframes* lm_kf_create_from_frames(LmCtx* c, const uint8_t* frames, int on_device, int n_frames, int64_t pixel_stride,
                                                 const uint8_t* masks, int n_masks, int min_pixels, void* stream)
{
    if (!c || n_frames < 0 || pixel_stride < 1 || min_pixels < 0 || (n_frames > 0 && !frames) || (n_masks != 0 && n_masks != n_frames) ||
        (n_masks > 0 && !masks)) {
        lm_set_error("lm_kf_create_from_frames: bad arguments (n_frames=%d, pixel_stride=%lld, n_masks=%d (0 or n_frames), min_pixels=%d, or a "
                     "null pointer)", n_frames, (long long)pixel_stride, n_masks, min_pixels);
        return nullptr;
    }
    const LmGeom g = c->g;
    const size_t px = (size_t)g.W * g.H;
    const int bwf = (g.W + 31) >> 5;
    if ((long long)c->max_batch * g.cap > 0x7fffffffll) {
        lm_set_error("lm_kf_create_from_frames: a batch of %d frames of %d labels each exceeds 2^31 records", c->max_batch, g.cap);
        return nullptr;
    }
    hipStream_t st = (hipStream_t)stream;
    LmKfccWork wk;
    std::vector<LmBitImage> items;
    std::vector<int32_t> recs;
    std::vector<int64_t> frame_off((size_t)n_frames + 1, 0);
    long long words = 0;                            // of the whole table
#define LM_KC(x, what) do { if (!(x)) { lm_set_error("lm_kf_create_from_frames: %s failed (%d frames of %d x %d)", what, n_frames, g.W, g.H); return nullptr; } } while (0)
#define LM_KH(x) LM_KC((x) == hipSuccess, #x)
    // ---- frames and masks where the kernels can read them
    const uint8_t* d_frames = frames;
    const uint8_t* d_masks = masks;
    if (!on_device) {
        uint8_t* up = nullptr;
        if (n_frames > 0) {
            LM_KC(wk.alloc(&up, (size_t)n_frames * px * (size_t)pixel_stride), "hipMalloc");
            LM_KH(hipMemcpyAsync(up, frames, (size_t)n_frames * px * (size_t)pixel_stride, hipMemcpyHostToDevice, st));
            d_frames = up;
        }
        if (n_masks > 0) {
            LM_KC(wk.alloc(&up, (size_t)n_masks * px), "hipMalloc");
            LM_KH(hipMemcpyAsync(up, masks, (size_t)n_masks * px, hipMemcpyHostToDevice, st));
            d_masks = up;
        }
    }
    // ---- per batch: ink plane -> labels -> statistics -> kept CCs -> records + crops -> item bits
    const int MB = c->max_batch;
    uint8_t* d_plane = nullptr;
    LmCounters* d_cnt = nullptr;
    long long* d_fcc = nullptr;
    long long* d_ccbase = nullptr;
    unsigned long long* d_wbase = nullptr;
    if (n_frames > 0) {
        LM_KC(wk.alloc(&d_plane, (size_t)MB * px) && wk.alloc(&d_cnt, 1) && wk.alloc(&d_fcc, (size_t)MB + 1) && wk.alloc(&d_ccbase, (size_t)MB) &&
              wk.alloc(&d_wbase, (size_t)MB), "hipMalloc");
    }
    std::vector<int32_t> kept((size_t)MB);
    std::vector<uint32_t> cwords((size_t)MB);
    std::vector<LmCcRec> hrec;
    std::vector<LmKfccItem> tab;
    for (int f0 = 0; f0 < n_frames; f0 += MB) {
        const int B = n_frames - f0 < MB ? n_frames - f0 : MB;
        const long long bpx = (long long)B * (long long)px;
        hipLaunchKernelGGL(lm_k_kfcc_ink, dim3(lm_blocks((bpx + 3) / 4, 256, LM_HIP_EMULATED ? 2 : 8192)), dim3(256), 0, st,
                           d_frames + (size_t)f0 * px * (size_t)pixel_stride, (long long)pixel_stride, bpx, d_plane);
        if (lm_label_batch(c, d_plane, B, nullptr, stream) != LM_OK) return nullptr;
        if (lm_cc_stats_batch(c, stream) != LM_OK) return nullptr;
        hipLaunchKernelGGL(lm_k_select, dim3(B), dim3(1024), 0, st, c->st_min_y, c->st_max_y, c->st_min_x, c->st_max_x, c->st_count, c->n_labels,
                           c->kept_label, c->kept_cropoff, c->frame_kept, c->frame_cropwords, g.cap, min_pixels);
        LM_KH(hipGetLastError());
        LM_KH(hipMemcpyAsync(kept.data(), c->frame_kept, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        LM_KH(hipMemcpyAsync(cwords.data(), c->frame_cropwords, (size_t)B * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        LM_KH(hipStreamSynchronize(st));
        long long ncc = 0, ncw = 0;
        for (int b = 0; b < B; b++) {
            frame_off[(size_t)(f0 + b)] = (int64_t)items.size() + ncc;
            ncc += kept[(size_t)b]; ncw += cwords[(size_t)b];
        }
        if ((long long)items.size() + ncc + n_masks > 0x7fffffffll) {
            lm_set_error("lm_kf_create_from_frames: more than 2^31 - 1 items (%lld connected components up to frame %d)", (long long)items.size() + ncc, f0 + B);
            return nullptr;
        }
        if (ncc == 0) continue;
        LmCcRec* d_rec = nullptr;
        uint32_t* d_crop = nullptr;
        uint32_t* d_hash = nullptr;
        LM_KC(wk.alloc(&d_rec, (size_t)ncc) && wk.alloc(&d_crop, (size_t)ncw) && wk.alloc(&d_hash, (size_t)ncc), "hipMalloc");
        LM_KH(hipMemsetAsync(d_cnt, 0, sizeof(LmCounters), st));
        LM_KH(hipMemsetAsync(d_hash, 0, (size_t)ncc * sizeof(uint32_t), st));       // lm_k_emit adds into it
        hipLaunchKernelGGL(lm_k_batch_offsets, dim3(1), dim3(1024), 0, st, c->frame_kept, c->frame_cropwords, B, d_cnt, d_fcc, d_ccbase, d_wbase, ncc,
                           (unsigned long long)ncw, B);
        hipLaunchKernelGGL(lm_k_emit, dim3(LM_HIP_EMULATED ? 2 : LM_EMIT_GRID, B), dim3(256), 0, st, c->bits, c->starts, c->prefix, c->rowoff, c->final_label,
                           c->st_min_y, c->st_max_y, c->st_min_x, c->st_max_x, c->st_count, c->kept_label, c->kept_cropoff, c->frame_kept,
                           c->frame_cropwords, d_ccbase, d_wbase, d_rec, d_crop, d_hash, f0, g.WW, g.H, g.cap);
        LM_KH(hipGetLastError());
        hrec.resize((size_t)ncc);
        LM_KH(hipMemcpyAsync(hrec.data(), d_rec, (size_t)ncc * sizeof(LmCcRec), hipMemcpyDeviceToHost, st));
        LM_KH(hipStreamSynchronize(st));
        // the item table of the batch, from the records
        tab.resize((size_t)ncc);
        long long bwords = 0;
        for (long long k = 0; k < ncc; k++) {
            const LmCcRec& r = hrec[(size_t)k];
            const int w = r.max_x - r.min_x + 1, h = r.max_y - r.min_y + 1, snw = (r.max_x >> 5) - (r.min_x >> 5) + 1;
            if (r.min_x < 0 || r.min_y < 0 || w < 1 || h < 1 || r.max_x >= g.W || r.max_y >= g.H || r.crop_off + (unsigned long long)snw * h > (unsigned long long)ncw) {
                lm_set_error("lm_kf_create_from_frames: record %lld of the batch at frame %d is inconsistent (box %d..%d x %d..%d, crop at %llu of %lld)", k, f0,
                             r.min_x, r.max_x, r.min_y, r.max_y, r.crop_off, ncw);
                return nullptr;
            }
            LmKfccItem& t = tab[(size_t)k];
            t.src_off = (long long)r.crop_off; t.dst_off = bwords; t.sh = r.min_x & 31; t.src_nw = snw; t.w = w; t.h = h;
            LmBitImage im;
            im.x0 = r.min_x; im.y0 = r.min_y; im.w = w; im.h = h; im.src_off = 0; im.bits_off = words + bwords;
            items.push_back(im);
            const int32_t six[6] = {r.cc_id, r.min_x, r.max_x, r.min_y, r.max_y, r.size};
            recs.insert(recs.end(), six, six + 6);
            bwords += (long long)h * ((w + 31) >> 5);
        }
        LmKfccItem* d_tab = nullptr;
        uint32_t* d_bits = nullptr;
        LM_KC(wk.alloc(&d_tab, (size_t)ncc), "hipMalloc");
        LM_KH(hipMalloc((void**)&d_bits, (size_t)bwords * sizeof(uint32_t)));
        wk.chunks.push_back(std::make_pair(d_bits, bwords));
        LM_KH(hipMemcpyAsync(d_tab, tab.data(), (size_t)ncc * sizeof(LmKfccItem), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(lm_k_kfcc_convert, dim3(lm_blocks(bwords, 256, LM_HIP_EMULATED ? 2 : 8192)), dim3(256), 0, st, (const LmKfccItem*)d_tab, (int)ncc,
                           (const uint32_t*)d_crop, bwords, d_bits);
        LM_KH(hipGetLastError());
        LM_KH(hipStreamSynchronize(st));            // tab (host) and the batch's buffers are reused / released below
        wk.release(d_rec); wk.release(d_crop); wk.release(d_hash); wk.release(d_tab);
        words += bwords;
    }
    frame_off[(size_t)n_frames] = (int64_t)items.size();
    // ---- one full-frame item per mask, then the table that owns all bits
    const long long cc_words = words;
    const size_t n_cc = items.size();
    for (int k = 0; k < n_masks; k++) {
        LmBitImage im;
        im.x0 = 0; im.y0 = 0; im.w = g.W; im.h = g.H; im.src_off = (long long)k * (long long)px; im.bits_off = words;
        items.push_back(im);
        words += (long long)g.H * bwf;
    }
    LmKeyframes* kf = lm_kf_new(g.W, g.H, "lm_kf_create_from_frames");
    if (!kf) return nullptr;
    bool ok = hipMalloc((void**)&kf->d_owned, (size_t)std::max<long long>(words, 1) * sizeof(uint32_t)) == hipSuccess;
    long long at = 0;
    for (size_t k = 0; ok && k < wk.chunks.size(); k++) {
        ok = hipMemcpyAsync(kf->d_owned + at, wk.chunks[k].first, (size_t)wk.chunks[k].second * sizeof(uint32_t), hipMemcpyDeviceToDevice, st) == hipSuccess;
        at += wk.chunks[k].second;
    }
    if (ok && at != cc_words) ok = false;
    if (ok && n_masks > 0) {
        LmBitImage* d_mi = nullptr;
        ok = wk.alloc(&d_mi, (size_t)n_masks) &&
             hipMemcpyAsync(d_mi, items.data() + n_cc, (size_t)n_masks * sizeof(LmBitImage), hipMemcpyHostToDevice, st) == hipSuccess;
        if (ok) {
            hipLaunchKernelGGL(lm_k_img_pack, dim3(LM_HIP_EMULATED ? 1 : 64, (unsigned)std::min(n_masks, LM_HIP_EMULATED ? 2 : 4096)), dim3(256), 0, st,
                               (const LmBitImage*)d_mi, n_masks, d_masks, kf->d_owned);
            ok = hipGetLastError() == hipSuccess;
        }
    }
    if (ok) ok = hipStreamSynchronize(st) == hipSuccess;
    if (!ok) {
        lm_set_error("lm_kf_create_from_frames: HIP error while assembling the table (%zu items, %lld words)", items.size(), words);
        lm_kf_destroy(kf);
        return nullptr;
    }
#undef LM_KH
#undef LM_KC
    kf->d_bits = kf->d_owned;
    kf->items.swap(items);
    kf->from_frames = 1;
    kf->cc_rec.swap(recs);
    kf->cc_frame_off.swap(frame_off);
    return kf;
}

extern "C" int lm_kf_cc_records(const LmKeyframes* kf, int64_t* h_frame_off, int32_t* h_rec)
{
    if (!kf) { lm_set_error("lm_kf_cc_records: null table"); return LM_ERR_ARG; }
    if (!kf->from_frames) { lm_set_error("lm_kf_cc_records: the table was not made by lm_kf_create_from_frames"); return LM_ERR_STATE; }
    if (h_frame_off) memcpy(h_frame_off, kf->cc_frame_off.data(), kf->cc_frame_off.size() * sizeof(int64_t));
    if (h_rec && !kf->cc_rec.empty()) memcpy(h_rec, kf->cc_rec.data(), kf->cc_rec.size() * sizeof(int32_t));
    return LM_OK;
}
