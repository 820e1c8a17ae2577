// lm_fcn_bytes.hip -- the three FCN heads -> the byte images of FCN_LectureNet.binarize in one pass (lm_fcn_bytes).
//
// Replaces, per frame, for heads that already lie in HBM:
//   sigmoid -> *255 -> astype(uint8) [-> >= thr -> {0, 255}]   lecturenet_v1/FCN_lecturenet.py:452-476, for res AND text_mask
//   from_img_space_to_cv2 (transpose, *0.5, +0.5, BGR, *255, clip, uint8)   FCN_lecturenet.py:478-479, 534-555
//   255 - binary                                               video_worker/FCN_lecturenet_binarizer.py:54
// 20 B/px read (logit, text logit, three reconstruction planes, fp32), 5 B/px written (binary, text mask, B G R).
// Included after lm_cc_kernels.hip: lm_sigmoid_u8 / lm_thr_px (the per-pixel formula), lm_ld_stream, lm_cmp4.
#include "lm_common.h"

#define LM_FB_HARD_CMP 0        // {0, 255} by x >= x* (lm_threshold_edge's x*, as lm_k_threshold_cmp)
#define LM_FB_HARD_FORMULA 1    // {0, 255} by the per-pixel formula (as lm_k_threshold_invert)
#define LM_FB_SOFT_BYTES 2      // trunc(sigmoid(x) * 255)

typedef unsigned lm_u32x4 __attribute__((ext_vector_type(4)));

template <int MODE> LM_DEV unsigned lm_fb_px(float x, float edge, int thr, unsigned flip)
{
    if (MODE == LM_FB_HARD_CMP) return ((x >= edge) ? 255u : 0u) ^ flip;
    if (MODE == LM_FB_HARD_FORMULA) return lm_thr_px(x, thr, flip);
    return lm_sigmoid_u8(x) ^ flip;             // 255 - v == v ^ 0xff for a byte
}

template <int MODE> LM_DEV unsigned lm_fb_px4(float4 v, float edge, int thr, unsigned flip)
{
    if (MODE == LM_FB_HARD_CMP) return lm_cmp4(v, edge, 255u ^ flip, flip);
    return lm_fb_px<MODE>(v.x, edge, thr, flip) | (lm_fb_px<MODE>(v.y, edge, thr, flip) << 8) | (lm_fb_px<MODE>(v.z, edge, thr, flip) << 16) |
           (lm_fb_px<MODE>(v.w, edge, thr, flip) << 24);
}

// from_img_space_to_cv2 per value, in the reference's fp32 steps: x *= 0.5 (exact), x += 0.5, x *= 255 -- each rounds on its own --
// clip to [0, 255], truncate
LM_DEV unsigned lm_rec_u8(float x)
{
#pragma clang fp contract(off)
    float v = x * 0.5f;
    v = v + 0.5f;
    v = v * 255.0f;
    v = (v > 255.0f) ? 255.0f : v;
    v = (v < 0.0f) ? 0.0f : v;
    return (unsigned)v;
}

// one pixel, byte stores: the tail of the vector kernel and the whole of the scalar one
template <int MODE> LM_DEV void lm_fb_one(long long i, const float* logit, const float* text, const float* rec, long long n, float edge, int thr, unsigned flip,
                                          uint8_t* binary, uint8_t* text_u8, uint8_t* rec_bgr)
{
    if (logit) binary[i] = (uint8_t)lm_fb_px<MODE>(logit[i], edge, thr, flip);
    if (text) text_u8[i] = (uint8_t)lm_fb_px<MODE>(text[i], edge, thr, 0u);
    if (rec) {
        rec_bgr[3 * i + 0] = (uint8_t)lm_rec_u8(rec[2 * n + i]);
        rec_bgr[3 * i + 1] = (uint8_t)lm_rec_u8(rec[n + i]);
        rec_bgr[3 * i + 2] = (uint8_t)lm_rec_u8(rec[i]);
    }
}

// Vector form: every present source and destination 16-byte aligned, n % 4 == 0 (the planes of rec start at rec + n, rec + 2n).
// A thread takes the 16 consecutive pixels of group g per trip: up to twenty 16-byte streaming loads issued before the first use,
// then one 16-byte store per byte image and three for the 48 bytes of B G R.  The workgroup's 256 groups are consecutive, so the byte
// images' stores of a wave are 1 KB contiguous; its loads (64 B per thread and plane) and the B G R stores (48 B per thread) cover
// whole 128-byte lines between the thread's back-to-back instructions.  The n % 16 pixels behind the last group: workgroup 0, one each.
// HAVE: bit 0 logit, bit 1 text, bit 2 rec -- a template parameter, because a run-time test of the pointers puts every group of loads
// into a basic block of its own and the compiler then waits for each before it issues the next.
template <int MODE, int HAVE>
__global__ void __launch_bounds__(256) lm_k_fcn_bytes(const float* __restrict__ logit, const float* __restrict__ text, const float* __restrict__ rec, long long n,
                                                      float edge, int thr, unsigned flip, uint8_t* __restrict__ binary, uint8_t* __restrict__ text_u8,
                                                      uint8_t* __restrict__ rec_bgr)
{
    constexpr bool has_logit = HAVE & 1, has_text = HAVE & 2, has_rec = HAVE & 4;
    const long long n16 = n >> 4;
    const float4* s_logit = (const float4*)logit;
    const float4* s_text = (const float4*)text;
    const float4* s_r = (const float4*)rec;
    const float4* s_g = (const float4*)(has_rec ? rec + n : nullptr);
    const float4* s_b = (const float4*)(has_rec ? rec + 2 * n : nullptr);
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < n16; g += (long long)gridDim.x * 256) {
        float4 a[4], t[4], r[4], gr[4], b[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            a[k] = has_logit ? lm_ld_stream(s_logit + g * 4 + k) : z;
            t[k] = has_text ? lm_ld_stream(s_text + g * 4 + k) : z;
            r[k] = has_rec ? lm_ld_stream(s_r + g * 4 + k) : z;
            gr[k] = has_rec ? lm_ld_stream(s_g + g * 4 + k) : z;
            b[k] = has_rec ? lm_ld_stream(s_b + g * 4 + k) : z;
        }
        LM_SCHED_BARRIER();         // every load of the trip is issued before its first use
        if (has_logit) {
            lm_u32x4 o;
#pragma unroll
            for (int k = 0; k < 4; k++) o[k] = lm_fb_px4<MODE>(a[k], edge, thr, flip);
            __builtin_nontemporal_store(o, (lm_u32x4*)binary + g);
        }
        if (has_text) {
            lm_u32x4 o;
#pragma unroll
            for (int k = 0; k < 4; k++) o[k] = lm_fb_px4<MODE>(t[k], edge, thr, 0u);
            __builtin_nontemporal_store(o, (lm_u32x4*)text_u8 + g);
        }
        if (has_rec) {
            unsigned w[12];
#pragma unroll
            for (int k = 0; k < 4; k++) {       // pixels 4k .. 4k + 3 -> bytes 12k .. 12k + 11: B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
                const unsigned b0 = lm_rec_u8(b[k].x), g0 = lm_rec_u8(gr[k].x), r0 = lm_rec_u8(r[k].x);
                const unsigned b1 = lm_rec_u8(b[k].y), g1 = lm_rec_u8(gr[k].y), r1 = lm_rec_u8(r[k].y);
                const unsigned b2 = lm_rec_u8(b[k].z), g2 = lm_rec_u8(gr[k].z), r2 = lm_rec_u8(r[k].z);
                const unsigned b3 = lm_rec_u8(b[k].w), g3 = lm_rec_u8(gr[k].w), r3 = lm_rec_u8(r[k].w);
                w[3 * k + 0] = b0 | (g0 << 8) | (r0 << 16) | (b1 << 24);
                w[3 * k + 1] = g1 | (r1 << 8) | (b2 << 16) | (g2 << 24);
                w[3 * k + 2] = r2 | (b3 << 8) | (g3 << 16) | (r3 << 24);
            }
            lm_u32x4* dst = (lm_u32x4*)rec_bgr + g * 3;
#pragma unroll
            for (int j = 0; j < 3; j++) {
                lm_u32x4 o;
#pragma unroll
                for (int c = 0; c < 4; c++) o[c] = w[4 * j + c];
                __builtin_nontemporal_store(o, dst + j);
            }
        }
    }
    const long long tail = n16 * 16 + threadIdx.x;
    if (blockIdx.x == 0 && tail < n) lm_fb_one<MODE>(tail, logit, text, rec, n, edge, thr, flip, binary, text_u8, rec_bgr);
}

// Scalar form, byte for byte the same images: any alignment, any n (odd frame sizes, slices of [n,H,W,3] tensors at odd H*W)
template <int MODE>
__global__ void __launch_bounds__(256) lm_k_fcn_bytes_scalar(const float* __restrict__ logit, const float* __restrict__ text, const float* __restrict__ rec,
                                                             long long n, int thr, unsigned flip, uint8_t* __restrict__ binary, uint8_t* __restrict__ text_u8,
                                                             uint8_t* __restrict__ rec_bgr)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        lm_fb_one<MODE>(i, logit, text, rec, n, 0.0f, thr, flip, binary, text_u8, rec_bgr);
}
