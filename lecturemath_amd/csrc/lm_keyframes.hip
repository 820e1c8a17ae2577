// lm_keyframes.hip -- step 05 (KeyframeExtractor.GenerateFromST3DForIntervals, AccessMath/preprocessing/content/
// keyframe_extractor.py:13-145) on images that already are bit rows on the device.  Included by lm_api.hip after lm_group.hip.
//
// LmKeyframes is a table of bit-row images placed in a W x H frame (LmBitImage: x0, y0, w, h, bits_off; ceil(w / 32) words per
// row relative to the item's own x0 -- the layout of LmGroups::d_gbits and of lm_k_img_pack alike).  Two things are asked of it:
//   lm_kf_overlaps   for every video segment, which of the images selected for it share an ink pixel: a box join per segment
//                    (lm_k_selfjoin, launched on the segment's slice of the box array, so no pair crosses segments), one
//                    compaction of the per-segment candidate regions, one bit test over all candidates (lm_k_bitimg_pair_any)
//   lm_kf_render     the keyframes: OR of the drawn images into an LDS bit tile per (tile, keyframe), expanded to 0 / 255 bytes
// The item table lives on the host: both calls gather the few items they name into a per-call device list, so a view of a
// lecture's group images (lm_kf_create_from_group) costs no device memory and copies no pixel.
#define LM_KT_COLS 256                      // tile: 256 x 32 pixels = 8 x 32 LDS words
#define LM_KT_ROWS 32
#define LM_KT_WPR (LM_KT_COLS / 32)
// Items of a tile that the whole workgroup composes from one flat word list; what a tile lists beyond them is composed by the thread
// that found it (crowded-tile path).  A lecture's keyframe puts a handful of group boxes on a 256 x 32 tile; 24 also makes the
// densest fixture (700 groups in 640 x 96, up to 32 drawn items on a tile) run the crowded path, which lm_kf_crowded_tiles counts.
#define LM_KT_MAXHIT 24

struct LmKfClip { int xa, xb, ya, yb, jlo, nw; };      // item x tile intersection [xa, xb) x [ya, yb), its tile words jlo .. jlo + nw - 1

LM_DEV LmKfClip lm_kf_clip(const LmBitImage& it, int X0, int Y0)
{
    LmKfClip c;
    c.xa = it.x0 > X0 ? it.x0 : X0;
    c.xb = (it.x0 + it.w < X0 + LM_KT_COLS) ? it.x0 + it.w : X0 + LM_KT_COLS;
    c.ya = it.y0 > Y0 ? it.y0 : Y0;
    c.yb = (it.y0 + it.h < Y0 + LM_KT_ROWS) ? it.y0 + it.h : Y0 + LM_KT_ROWS;
    c.jlo = (c.xa - X0) >> 5;
    c.nw = ((c.xb - 1 - X0) >> 5) - c.jlo + 1;
    if (c.xb <= c.xa || c.yb <= c.ya) c.nw = 0;
    return c;
}

// ORs the item's ink under tile word (row c.ya + yy, word c.jlo + j) into the LDS tile: two image words funnel-shifted to the
// tile's 32-pixel grid, clipped to the intersection
LM_DEV void lm_kf_or_word(const LmBitImage& it, const LmKfClip& c, const uint32_t* __restrict__ bits, int X0, int Y0, int yy, int j, unsigned* s_tile)
{
    const int bw = (it.w + 31) >> 5;
    const int col = X0 + 32 * (c.jlo + j);              // frame column of the tile word's bit 0
    const int d = col - it.x0;                          // ... and the image column under it (> -32)
    const int sw = d >> 5, sh = d & 31;                 // floor
    const uint32_t* r = bits + it.bits_off + (long long)(c.ya - it.y0 + yy) * bw;
    const unsigned lo = (sw >= 0 && sw < bw) ? r[sw] : 0u;
    const unsigned hi = (sh && sw + 1 < bw) ? r[sw + 1] : 0u;
    unsigned v = sh ? ((lo >> sh) | (hi << (32 - sh))) : lo;
    if (col < c.xa) v &= 0xffffffffu << (c.xa - col);
    if (col + 32 > c.xb) v &= 0xffffffffu >> (col + 32 - c.xb);
    if (v) atomicOr(&s_tile[(c.ya - Y0 + yy) * LM_KT_WPR + c.jlo + j], v);
}

// 16 output bytes starting at byte `byte0` of the tile's row (CH bytes per pixel): 0 where the pixel has ink, 255 elsewhere
template <int CH> LM_DEV void lm_kf_expand16(const unsigned* s_row, int byte0, unsigned (&o)[4])
{
#pragma unroll
    for (int q = 0; q < 4; q++) {
        o[q] = 0;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int px = (byte0 + 4 * q + t) / CH;
            const unsigned ink = px < LM_KT_COLS ? (s_row[px >> 5] >> (px & 31)) & 1u : 0u;
            o[q] |= (ink ? 0u : 0xffu) << (8 * t);
        }
    }
}

// Workgroup per (tile, keyframe).  draw_off [n_seg + 1] delimits the keyframes' lists in `draw`.  Every byte of `out`
// ([n_seg][H][W][CH]) is written exactly once: the tiles partition the frame and the 16-byte chunks partition a tile's rows.
template <int CH>
__global__ void __launch_bounds__(256) lm_k_kf_render(const long long* __restrict__ draw_off, const LmBitImage* __restrict__ draw,
                                                      const uint32_t* __restrict__ bits, int W, int H, int n_seg, int tiles_x, int tiles_y,
                                                      uint8_t* __restrict__ out, unsigned long long* __restrict__ crowded)
{
    __shared__ unsigned s_tile[LM_KT_ROWS * LM_KT_WPR];
    __shared__ LmBitImage s_hit[LM_KT_MAXHIT];
    __shared__ unsigned s_pre[LM_KT_MAXHIT + 1];
    __shared__ int s_nhit;
    const long long per_frame = (long long)tiles_x * tiles_y, n_units = per_frame * n_seg;
    const long long row_bytes = (long long)W * CH;
    const bool vec = ((row_bytes & 15) == 0) && ((((uintptr_t)out) & 15) == 0);
    for (long long unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
        const int seg = (int)(unit / per_frame), t = (int)(unit - (long long)seg * per_frame);
        const int X0 = (t % tiles_x) * LM_KT_COLS, Y0 = (t / tiles_x) * LM_KT_ROWS;
        __syncthreads();                                // the stores of the unit before read s_tile
        for (int i = threadIdx.x; i < LM_KT_ROWS * LM_KT_WPR; i += blockDim.x) s_tile[i] = 0;
        if (threadIdx.x == 0) s_nhit = 0;
        __syncthreads();
        // screen the keyframe's draw list (an item per thread and trip), collect what touches the tile
        const long long i0 = draw_off[seg], i1 = draw_off[seg + 1];
        for (long long ib = i0 + threadIdx.x; ib < i1; ib += blockDim.x) {
            const LmBitImage mine = draw[ib];
            const LmKfClip c = lm_kf_clip(mine, X0, Y0);
            if (c.nw <= 0) continue;
            const int slot = atomicAdd(&s_nhit, 1);
            if (slot < LM_KT_MAXHIT) {
                s_hit[slot] = mine;
            } else {                                    // crowded tile: the finder composes its item alone
                for (int k = 0; k < c.nw * (c.yb - c.ya); k++) lm_kf_or_word(mine, c, bits, X0, Y0, k / c.nw, k % c.nw, s_tile);
            }
        }
        __syncthreads();
        const int nhit = s_nhit < LM_KT_MAXHIT ? s_nhit : LM_KT_MAXHIT;
        if (threadIdx.x == 0 && s_nhit > LM_KT_MAXHIT) atomicAdd(crowded, 1ull);
        // the tile words of all listed items as one flat list dealt to the threads; s_pre[h] = tile words of the items before h
        if (threadIdx.x < 64) {
            const int lane = lm_lane();
            unsigned words = 0;
            if (lane < nhit) {
                const LmKfClip c = lm_kf_clip(s_hit[lane], X0, Y0);
                words = (unsigned)(c.nw * (c.yb - c.ya));
            }
            const unsigned incl = lm_wave_incl_scan(words);
            if (lane < nhit) s_pre[lane] = incl - words;
            if (lane == 63) s_pre[nhit] = incl;
        }
        __syncthreads();
        const unsigned total = s_pre[nhit];
        for (unsigned g = threadIdx.x; g < total; g += blockDim.x) {
            int a = 0, b = nhit;                        // largest h with s_pre[h] <= g
            while (b - a > 1) {
                const int mid = (a + b) >> 1;
                if (s_pre[mid] <= g) a = mid; else b = mid;
            }
            const LmBitImage it = s_hit[a];
            const LmKfClip c = lm_kf_clip(it, X0, Y0);
            const int idx = (int)(g - s_pre[a]);
            lm_kf_or_word(it, c, bits, X0, Y0, idx / c.nw, idx % c.nw, s_tile);
        }
        __syncthreads();
        // expand and store: a lane per 16-byte chunk of a tile row, consecutive lanes consecutive chunks
        const long long b0 = (long long)X0 * CH;
        const long long b1 = (long long)((X0 + LM_KT_COLS < W) ? X0 + LM_KT_COLS : W) * CH;
        const int nchunk = (int)((b1 - b0 + 15) >> 4);
        const int rows = (Y0 + LM_KT_ROWS < H) ? LM_KT_ROWS : H - Y0;
        for (int i = threadIdx.x; i < rows * nchunk; i += blockDim.x) {
            const int yy = i / nchunk, ch = i - yy * nchunk;
            unsigned o[4];
            lm_kf_expand16<CH>(s_tile + yy * LM_KT_WPR, ch * 16, o);
            uint8_t* d = out + ((long long)seg * H + (Y0 + yy)) * row_bytes + b0 + (long long)ch * 16;
            if (vec) {
                *(uint4*)d = make_uint4(o[0], o[1], o[2], o[3]);
            } else {                                    // byte-exact path: rows of W * CH bytes that are no multiple of 16
                const long long left = b1 - (b0 + (long long)ch * 16);
                for (int k = 0; k < 16 && k < left; k++) d[k] = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
            }
        }
    }
}

// candidate pairs of all segments, gathered from the per-segment regions the joins filled (local list positions) into one list of
// entry indices: q in [cnt_off[s], cnt_off[s + 1]) <- region[reg_off[s] + q - cnt_off[s]] + seg_off[s]
__global__ void __launch_bounds__(256) lm_k_kf_compact(const int2* __restrict__ region, const long long* __restrict__ reg_off,
                                                       const long long* __restrict__ cnt_off, const long long* __restrict__ seg_off, int n_seg,
                                                       int2* __restrict__ pairs)
{
    const long long np = cnt_off[n_seg];
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < np; q += (long long)gridDim.x * blockDim.x) {
        int a = 0, b = n_seg;                           // largest s with cnt_off[s] <= q
        while (b - a > 1) {
            const int mid = (a + b) >> 1;
            if (cnt_off[mid] <= q) a = mid; else b = mid;
        }
        const int2 p = region[reg_off[a] + (q - cnt_off[a])];
        const int base = (int)seg_off[a];
        pairs[q] = make_int2(p.x + base, p.y + base);
    }
}

// ================================================================================================
// host side
// ================================================================================================
struct LmKeyframes {
    int W = 0, H = 0;
    std::vector<LmBitImage> items;              // src_off: byte offset of the item in the lecture's uint8 image array (views) / upload
    const uint32_t* d_bits = nullptr;           // the group's d_gbits (view) or d_owned
    uint32_t* d_owned = nullptr;
    unsigned long long* d_crowded = nullptr;    // tiles that took the crowded-tile path, since creation
    void* ws[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // grow-only scratch: join, bit tests, render, image,
    size_t ws_cap[6] = {0, 0, 0, 0, 0, 0};                                  // and the two of lm_kf_pair_counts (lm_ccmatch.hip)
    std::vector<char> stage[6];                 // host side of the uploads (alive until the next call)
    // lm_kf_create_from_frames (lm_kfcc.hip): the CC items of frame f are cc_frame_off[f] .. cc_frame_off[f + 1], the masks follow
    int from_frames = 0;
    std::vector<int64_t> cc_frame_off;          // [n_frames + 1]
    std::vector<int32_t> cc_rec;                // [n_cc][6] = cc_id, min_x, max_x, min_y, max_y, size
};

static void* lm_kf_scratch(LmKeyframes* kf, int slot, size_t bytes, const char* who)
{
    if (kf->ws[slot] && bytes <= kf->ws_cap[slot]) return kf->ws[slot];
    if (kf->ws[slot]) (void)hipFree(kf->ws[slot]);
    kf->ws[slot] = nullptr; kf->ws_cap[slot] = 0;
    const size_t want = bytes + bytes / 4 + 256;
    if (hipMalloc(&kf->ws[slot], want) != hipSuccess) { lm_set_error("%s: hipMalloc(%zu) failed", who, want); return nullptr; }
    kf->ws_cap[slot] = want;
    return kf->ws[slot];
}

static size_t lm_kf_up(size_t v) { return (v + 255) & ~(size_t)255; }

static unsigned long long lm_kf_pack_box(const LmBitImage& im)
{
    return (unsigned long long)(unsigned short)im.x0 | ((unsigned long long)(unsigned short)(im.x0 + im.w - 1) << 16) |
           ((unsigned long long)(unsigned short)im.y0 << 32) | ((unsigned long long)(unsigned short)(im.y0 + im.h - 1) << 48);
}

static LmKeyframes* lm_kf_new(int W, int H, const char* who)
{
    LmKeyframes* kf = new LmKeyframes();
    kf->W = W; kf->H = H;
    if (hipMalloc((void**)&kf->d_crowded, sizeof(unsigned long long)) != hipSuccess || hipMemset(kf->d_crowded, 0, sizeof(unsigned long long)) != hipSuccess) {
        lm_set_error("%s: hipMalloc failed", who);
        delete kf;
        return nullptr;
    }
    return kf;
}

extern "C" void lm_kf_destroy(LmKeyframes* kf)
{
    if (!kf) return;
    for (void* p : kf->ws)
        if (p) (void)hipFree(p);
    if (kf->d_owned) (void)hipFree(kf->d_owned);
    if (kf->d_crowded) (void)hipFree(kf->d_crowded);
    delete kf;
}

extern "C" int lm_kf_count(const LmKeyframes* kf) { return kf ? (int)kf->items.size() : -1; }

extern "C" LmKeyframes* lm_kf_create_from_group(LmGroups* g)
{
    if (!g) { lm_set_error("lm_kf_create_from_group: null group"); return nullptr; }
    if (g->n_items <= 0 || !g->d_gbits) { lm_set_error("lm_kf_create_from_group: the group holds no images"); return nullptr; }
    const LmGeom gm = g->s->ctx->g;
    LmKeyframes* kf = lm_kf_new(gm.W, gm.H, "lm_kf_create_from_group");
    if (!kf) return nullptr;
    kf->d_bits = g->d_gbits;
    kf->items.resize((size_t)g->n_items);
    const size_t ng = g->gimg_item_off.size() - 1;
    for (size_t gi = 0; gi < ng; gi++) {
        const int32_t* b = &g->bounds[gi * 4];
        for (int64_t it = g->gimg_item_off[gi]; it < g->gimg_item_off[gi + 1]; it++) {
            LmBitImage& im = kf->items[(size_t)it];
            im.x0 = b[0]; im.y0 = b[2]; im.w = b[1] - b[0] + 1; im.h = b[3] - b[2] + 1;
            im.src_off = g->gimg_off[(size_t)it];
            im.bits_off = g->gbits_off[(size_t)it];
        }
    }
    return kf;
}

extern "C" LmKeyframes* lm_kf_create_from_images(const int32_t* h_boxes, const uint8_t* h_images, const int64_t* h_img_off, int n, int W, int H,
                                                 void* stream)
{
    if (n < 0 || W <= 0 || H <= 0 || W > 32768 || H > 32768 || (n > 0 && (!h_boxes || !h_images || !h_img_off))) {
        lm_set_error("lm_kf_create_from_images: bad arguments (n=%d, frame %d x %d)", n, W, H);
        return nullptr;
    }
    std::vector<LmBitImage> items((size_t)n);
    long long words = 0;
    for (int k = 0; k < n; k++) {
        const int32_t* bx = h_boxes + (size_t)k * 4;
        LmBitImage& im = items[(size_t)k];
        if (bx[0] < 0 || bx[2] < 0 || bx[1] < bx[0] || bx[3] < bx[2] || bx[1] >= W || bx[3] >= H) {
            lm_set_error("lm_kf_create_from_images: image %d: box (%d, %d, %d, %d) outside the %d x %d frame", k, bx[0], bx[1], bx[2], bx[3], W, H);
            return nullptr;
        }
        im.x0 = bx[0]; im.y0 = bx[2]; im.w = bx[1] - bx[0] + 1; im.h = bx[3] - bx[2] + 1;
        if (h_img_off[k] < 0 || h_img_off[k + 1] - h_img_off[k] != (int64_t)im.w * im.h) {
            lm_set_error("lm_kf_create_from_images: image %d: box / size mismatch", k);
            return nullptr;
        }
        im.src_off = h_img_off[k];
        im.bits_off = words;
        words += (long long)im.h * ((im.w + 31) >> 5);
    }
    LmKeyframes* kf = lm_kf_new(W, H, "lm_kf_create_from_images");
    if (!kf) return nullptr;
    kf->items.swap(items);
    if (n == 0) return kf;
    hipStream_t st = (hipStream_t)stream;
    const size_t img_bytes = (size_t)h_img_off[n], tab_bytes = (size_t)n * sizeof(LmBitImage);
    char* d_tmp = nullptr;                      // [item table][uint8 images]: gone after the packing
    bool ok = hipMalloc((void**)&kf->d_owned, (size_t)std::max<long long>(words, 1) * sizeof(uint32_t)) == hipSuccess &&
              hipMalloc((void**)&d_tmp, lm_kf_up(tab_bytes) + std::max<size_t>(img_bytes, 1)) == hipSuccess;
    if (ok) {
        uint8_t* d_src = (uint8_t*)(d_tmp + lm_kf_up(tab_bytes));
        ok = hipMemcpyAsync(d_tmp, kf->items.data(), tab_bytes, hipMemcpyHostToDevice, st) == hipSuccess &&
             hipMemcpyAsync(d_src, h_images, img_bytes, hipMemcpyHostToDevice, st) == hipSuccess;
        if (ok) {
            hipLaunchKernelGGL(lm_k_img_pack, dim3(LM_HIP_EMULATED ? 1 : 4, (unsigned)std::min(n, LM_HIP_EMULATED ? 2 : 4096)), dim3(256), 0, st,
                               (const LmBitImage*)d_tmp, n, d_src, kf->d_owned);
            ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
        }
    }
    if (d_tmp) (void)hipFree(d_tmp);
    if (!ok) {
        lm_set_error("lm_kf_create_from_images: HIP error (%d images, %zu bytes)", n, img_bytes);
        lm_kf_destroy(kf);
        return nullptr;
    }
    kf->d_bits = kf->d_owned;
    return kf;
}

// offsets [n + 1] start at 0 and do not descend; every listed item exists
static bool lm_kf_lists_ok(const LmKeyframes* kf, const int64_t* off, const int32_t* list, int n)
{
    if (!off || off[0] != 0) return false;
    for (int s = 0; s < n; s++)
        if (off[s + 1] < off[s]) return false;
    if (off[n] > 0x7fffffff || (off[n] > 0 && !list)) return false;
    for (int64_t e = 0; e < off[n]; e++)
        if (list[e] < 0 || (size_t)list[e] >= kf->items.size()) return false;
    return true;
}

extern "C" int lm_kf_overlaps(LmKeyframes* kf, const int64_t* h_seg_off, const int32_t* h_items, int n_seg, int32_t* h_triples, int64_t cap,
                              int64_t* n_found, void* stream)
{
    if (!kf || !n_found || n_seg < 0 || cap < 0 || (cap > 0 && !h_triples) || !lm_kf_lists_ok(kf, h_seg_off, h_items, n_seg)) {
        lm_set_error("lm_kf_overlaps: bad arguments (null pointer, offsets that descend or do not start at 0, or an item outside the table)");
        return LM_ERR_ARG;
    }
    *n_found = 0;
    const int64_t E = h_seg_off[n_seg];
    if (n_seg == 0 || E < 2) return LM_OK;
    hipStream_t st = (hipStream_t)stream;
#define LM_KO(x) do { if ((x) != hipSuccess) { lm_set_error("lm_kf_overlaps: HIP error at %s", #x); return LM_ERR_HIP; } } while (0)
    // candidate regions: room for every pair of a small segment, a guess for a large one (the join counts past its room)
    std::vector<long long> reg_cap((size_t)n_seg), off3((size_t)(n_seg + 1) * 3);
    long long* reg_off = off3.data();
    long long* cnt_off = reg_off + (n_seg + 1);
    long long* seg_off = cnt_off + (n_seg + 1);
    for (int s = 0; s < n_seg; s++) {
        const long long ns = h_seg_off[s + 1] - h_seg_off[s];
        reg_cap[(size_t)s] = std::min(ns * (ns - 1) / 2, 8 * ns + 64);
        seg_off[s] = h_seg_off[s];
    }
    seg_off[n_seg] = E;
    std::vector<int> cnt((size_t)n_seg);
    const size_t o_box = lm_kf_up((size_t)E * sizeof(LmBitImage)), o_cnt = o_box + lm_kf_up((size_t)E * sizeof(unsigned long long));
    const size_t o_reg = o_cnt + lm_kf_up((size_t)n_seg * sizeof(int));
    std::vector<char>& up = kf->stage[0];
    up.assign(o_cnt, 0);
    for (int64_t e = 0; e < E; e++) {
        const LmBitImage& im = kf->items[(size_t)h_items[e]];
        ((LmBitImage*)up.data())[e] = im;
        ((unsigned long long*)(up.data() + o_box))[e] = lm_kf_pack_box(im);
    }
    char* wsA = nullptr;
    long long np = 0;
    for (;;) {
        reg_off[0] = 0;
        for (int s = 0; s < n_seg; s++) reg_off[s + 1] = reg_off[s] + reg_cap[(size_t)s];
        wsA = (char*)lm_kf_scratch(kf, 0, o_reg + (size_t)std::max<long long>(reg_off[n_seg], 1) * sizeof(int2), "lm_kf_overlaps");
        if (!wsA) return LM_ERR_HIP;
        LM_KO(hipMemcpyAsync(wsA, up.data(), o_cnt, hipMemcpyHostToDevice, st));
        LM_KO(hipMemsetAsync(wsA + o_cnt, 0, (size_t)n_seg * sizeof(int), st));
        for (int s = 0; s < n_seg; s++) {
            const int ns = (int)(h_seg_off[s + 1] - h_seg_off[s]);
            if (ns < 2) continue;
            const int gb = std::min((ns + LM_SJ_TILE - 1) / LM_SJ_TILE, LM_HIP_EMULATED ? 2 : 64);
            hipLaunchKernelGGL(lm_k_selfjoin, dim3(gb, gb), dim3(256), 0, st, (const unsigned long long*)(wsA + o_box) + h_seg_off[s], ns,
                               (int*)(wsA + o_cnt) + s, (int2*)(wsA + o_reg) + reg_off[s], (int)std::min<long long>(reg_cap[(size_t)s], 0x7fffffff));
        }
        LM_KO(hipGetLastError());
        LM_KO(hipMemcpyAsync(cnt.data(), wsA + o_cnt, (size_t)n_seg * sizeof(int), hipMemcpyDeviceToHost, st));
        LM_KO(hipStreamSynchronize(st));
        bool fits = true;
        np = 0;
        for (int s = 0; s < n_seg; s++) {
            if (cnt[(size_t)s] > reg_cap[(size_t)s]) { fits = false; reg_cap[(size_t)s] = cnt[(size_t)s]; }     // the retry gets the exact room
            np += cnt[(size_t)s];
        }
        if (fits) break;
    }
    if (np == 0) return LM_OK;
    if (np > 0x7fffffff) { lm_set_error("lm_kf_overlaps: %lld candidate pairs (limit 2^31)", np); return LM_ERR_CAPACITY; }
    cnt_off[0] = 0;
    for (int s = 0; s < n_seg; s++) cnt_off[s + 1] = cnt_off[s] + cnt[(size_t)s];
    const size_t off_bytes = off3.size() * sizeof(long long);
    const size_t o_pairs = lm_kf_up(off_bytes), o_hit = o_pairs + lm_kf_up((size_t)np * sizeof(int2));
    char* wsB = (char*)lm_kf_scratch(kf, 1, o_hit + (size_t)np * sizeof(int32_t), "lm_kf_overlaps");
    if (!wsB) return LM_ERR_HIP;
    kf->stage[1].assign((const char*)off3.data(), (const char*)off3.data() + off_bytes);
    LM_KO(hipMemcpyAsync(wsB, kf->stage[1].data(), off_bytes, hipMemcpyHostToDevice, st));
    const long long* d_off = (const long long*)wsB;
    int2* d_pairs = (int2*)(wsB + o_pairs);
    int32_t* d_hit = (int32_t*)(wsB + o_hit);
    hipLaunchKernelGGL(lm_k_kf_compact, dim3((unsigned)std::min<long long>((np + 255) / 256, LM_HIP_EMULATED ? 2 : 1024)), dim3(256), 0, st,
                       (const int2*)(wsA + o_reg), d_off, d_off + (n_seg + 1), d_off + 2 * (n_seg + 1), n_seg, d_pairs);
    hipLaunchKernelGGL(lm_k_bitimg_pair_any, dim3(LM_HIP_EMULATED ? 2 : 1024), dim3(256), 0, st, (const LmBitImage*)wsA, kf->d_bits, d_pairs, (int)np,
                       d_hit);
    LM_KO(hipGetLastError());
    std::vector<int2> hp((size_t)np);
    std::vector<int32_t> hh((size_t)np);
    LM_KO(hipMemcpyAsync(hp.data(), d_pairs, (size_t)np * sizeof(int2), hipMemcpyDeviceToHost, st));
    LM_KO(hipMemcpyAsync(hh.data(), d_hit, (size_t)np * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    LM_KO(hipStreamSynchronize(st));
#undef LM_KO
    struct Triple { int32_t s, i, j; };
    std::vector<Triple> found;
    for (int s = 0; s < n_seg; s++)
        for (long long q = cnt_off[s]; q < cnt_off[s + 1]; q++)
            if (hh[(size_t)q]) found.push_back({s, (int32_t)(hp[(size_t)q].x - seg_off[s]), (int32_t)(hp[(size_t)q].y - seg_off[s])});
    std::sort(found.begin(), found.end(), [](const Triple& a, const Triple& b) { return a.s != b.s ? a.s < b.s : a.i != b.i ? a.i < b.i : a.j < b.j; });
    *n_found = (int64_t)found.size();
    if ((int64_t)found.size() > cap) {
        lm_set_error("lm_kf_overlaps: %zu overlapping pairs, room for %lld", found.size(), (long long)cap);
        return LM_ERR_CAPACITY;
    }
    for (size_t k = 0; k < found.size(); k++) { h_triples[k * 3] = found[k].s; h_triples[k * 3 + 1] = found[k].i; h_triples[k * 3 + 2] = found[k].j; }
    return LM_OK;
}

extern "C" int lm_kf_render(LmKeyframes* kf, const int64_t* h_draw_off, const int32_t* h_draw_items, int n_seg, int channels, uint8_t* d_out,
                            void* stream)
{
    if (!kf || !d_out || n_seg < 0 || (channels != 1 && channels != 3) || !lm_kf_lists_ok(kf, h_draw_off, h_draw_items, n_seg)) {
        lm_set_error("lm_kf_render: bad arguments (null pointer, channels not 1 or 3, offsets that descend or do not start at 0, or an item outside "
                     "the table)");
        return LM_ERR_ARG;
    }
    if (n_seg == 0) return LM_OK;
    hipStream_t st = (hipStream_t)stream;
    const int64_t E = h_draw_off[n_seg];
    const size_t o_items = lm_kf_up((size_t)(n_seg + 1) * sizeof(long long));
    const size_t bytes = o_items + (size_t)std::max<int64_t>(E, 1) * sizeof(LmBitImage);
    std::vector<char>& up = kf->stage[2];
    up.assign(bytes, 0);
    for (int s = 0; s <= n_seg; s++) ((long long*)up.data())[s] = h_draw_off[s];
    for (int64_t e = 0; e < E; e++) ((LmBitImage*)(up.data() + o_items))[e] = kf->items[(size_t)h_draw_items[e]];
    char* ws = (char*)lm_kf_scratch(kf, 2, bytes, "lm_kf_render");
    if (!ws) return LM_ERR_HIP;
    LM_HIP(hipMemcpyAsync(ws, up.data(), bytes, hipMemcpyHostToDevice, st));
    const int tx = (kf->W + LM_KT_COLS - 1) / LM_KT_COLS, ty = (kf->H + LM_KT_ROWS - 1) / LM_KT_ROWS;
    const long long units = (long long)tx * ty * n_seg;
    const dim3 grid((unsigned)std::min<long long>(units, LM_HIP_EMULATED ? 2 : (1 << 20)));
    if (channels == 1)
        hipLaunchKernelGGL((lm_k_kf_render<1>), grid, dim3(256), 0, st, (const long long*)ws, (const LmBitImage*)(ws + o_items), kf->d_bits, kf->W, kf->H,
                           n_seg, tx, ty, d_out, kf->d_crowded);
    else
        hipLaunchKernelGGL((lm_k_kf_render<3>), grid, dim3(256), 0, st, (const long long*)ws, (const LmBitImage*)(ws + o_items), kf->d_bits, kf->W, kf->H,
                           n_seg, tx, ty, d_out, kf->d_crowded);
    LM_HIP(hipGetLastError());
    return LM_OK;
}

extern "C" int lm_kf_image(LmKeyframes* kf, int item, uint8_t* h_out, int64_t bytes, void* stream)
{
    if (!kf || !h_out || item < 0 || (size_t)item >= kf->items.size() || bytes != (int64_t)kf->items[(size_t)item].w * kf->items[(size_t)item].h) {
        lm_set_error("lm_kf_image: bad arguments (null pointer, item outside the table, or bytes != h * w of the item)");
        return LM_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    const LmBitImage& im = kf->items[(size_t)item];
    LmGimgItem one;
    one.x0 = im.x0; one.y0 = im.y0; one.w = im.w; one.h = im.h; one.img_off = 0; one.bits_off = im.bits_off;
    kf->stage[3].assign((const char*)&one, (const char*)&one + sizeof(one));
    const size_t o_img = lm_kf_up(sizeof(one));
    char* ws = (char*)lm_kf_scratch(kf, 3, o_img + (size_t)bytes, "lm_kf_image");
    if (!ws) return LM_ERR_HIP;
    LM_HIP(hipMemcpyAsync(ws, kf->stage[3].data(), sizeof(one), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(lm_k_gimg_expand, dim3(LM_HIP_EMULATED ? 1 : 8, 1), dim3(256), 0, st, (const LmGimgItem*)ws, 1, kf->d_bits, (uint8_t*)(ws + o_img));
    LM_HIP(hipGetLastError());
    LM_HIP(hipMemcpyAsync(h_out, ws + o_img, (size_t)bytes, hipMemcpyDeviceToHost, st));
    LM_HIP(hipStreamSynchronize(st));
    return LM_OK;
}

extern "C" int lm_kf_crowded_tiles(LmKeyframes* kf, int64_t* h_count, void* stream)
{
    if (!kf || !h_count) { lm_set_error("lm_kf_crowded_tiles: bad arguments"); return LM_ERR_ARG; }
    unsigned long long v = 0;
    LM_HIP(hipMemcpyAsync(&v, kf->d_crowded, sizeof(v), hipMemcpyDeviceToHost, (hipStream_t)stream));
    LM_HIP(hipStreamSynchronize((hipStream_t)stream));
    *h_count = (int64_t)v;
    return LM_OK;
}
