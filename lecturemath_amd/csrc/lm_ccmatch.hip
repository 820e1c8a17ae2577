// lm_ccmatch.hip -- the integer primitive under the reference's summary evaluation (AccessMath/evaluation/evaluator.py:
// check_equivalent_cc, keyframes_overlapping_ccs, match_overlapping_ccs, find_ccs_overlapping_background), on the bit rows of an
// LmKeyframes table.  Included by lm_api.hip after lm_keyframes.hip.
//
// A query names two lists of items, A and B, and a displacement (dy, dx) applied to every item of B.  lm_kf_pair_counts returns,
// for every pair (i of A, j of B) whose boxes touch for at least one extra displacement (ey, ex) in [-r, r]^2, the (2r + 1)^2 numbers
//     counts[ey + r][ex + r] = #{(y, x) : A_i has ink at (y, x) and B_j at (y - dy - ey, x - dx - ex)}
// in frame coordinates that are NOT clipped to the frame (the reference translates boxes freely; ConnectedComponent.
// getOverlapFMeasure, AM_CommonTools/data/connected_component.py:202-250, counts on the intersection of the two boxes, which is
// the same number).  Everything is integer, so the order of the additions does not matter.
//
// Three kernels:
//   lm_k_ccm_join<false>   a wave per entry of A: the entries of B of the same query whose box, grown by r, touches (the inclusive
//                          test of connected_component.py:204-205); counts rows and work units per entry of A
//   (host)                 exclusive scans of the two counts: the rows come out sorted by (query, i, j) whatever the schedule
//   lm_k_ccm_join<true>    the same walk, writing rows and units at their exact offsets (ballot rank / wave scan)
//   lm_k_ccm_count         a workgroup per unit = (row, block of LM_CCM_ROWS rows, block of LM_CCM_XW words of A) of the
//                          intersection of A's box with B's grown box.  A's words and B's rows (grown by r, with the words that
//                          the shifts reach, zero outside the image) are staged in LDS; thread slot = (displacement, group), the
//                          group strides over the block's (row, word) pairs: B operand = two adjacent LDS words shifted, AND,
//                          popcount.  One LDS atomic per thread, one global atomic per (unit, displacement) with a non-zero count.
// A 20-pixel glyph is one unit; a 1080p full-frame item (the object mask) against a ruled line is a unit per 32 rows.
//
// Limits (checked): radius <= LM_CCM_MAX_RADIUS; |dy|, |dx| <= 32768; frames <= 32768 x 32768 (the table's own limit), so a count
// is at most 2^30 and fits the int32 table; rows and units < 2^31 per call.
#define LM_CCM_MAX_RADIUS 8
#define LM_CCM_MAX_DISP 32768
#define LM_CCM_ROWS 32
#define LM_CCM_XW 64                                        // words of A per unit (2048 pixels)
#define LM_CCM_BS (LM_CCM_XW + 3)                           // row stride of the staged B rows: XW + 2 words are read, odd stride
#define LM_CCM_MAX_NE ((2 * LM_CCM_MAX_RADIUS + 1) * (2 * LM_CCM_MAX_RADIUS + 1))

// the part of A's box that B's box, grown by r on every side, covers; as rows [ya, yb] and words [ka, kb] of A.  Empty (nk <= 0)
// when the boxes do not touch for any extra displacement.
struct LmCcmClip { int ya, yb, ka, kb, nrb, nxb; };

LM_DEV LmCcmClip lm_ccm_clip(const LmBitImage& a, const LmBitImage& b, int r)
{
    LmCcmClip c;
    const int x0 = a.x0 > b.x0 - r ? a.x0 : b.x0 - r;
    const int x1 = (a.x0 + a.w - 1 < b.x0 + b.w - 1 + r) ? a.x0 + a.w - 1 : b.x0 + b.w - 1 + r;
    c.ya = a.y0 > b.y0 - r ? a.y0 : b.y0 - r;
    c.yb = (a.y0 + a.h - 1 < b.y0 + b.h - 1 + r) ? a.y0 + a.h - 1 : b.y0 + b.h - 1 + r;
    if (x1 < x0 || c.yb < c.ya) { c.ka = 0; c.kb = -1; c.nrb = 0; c.nxb = 0; return c; }
    c.ka = (x0 - a.x0) >> 5;
    c.kb = (x1 - a.x0) >> 5;
    c.nrb = (c.yb - c.ya + LM_CCM_ROWS) / LM_CCM_ROWS;
    c.nxb = (c.kb - c.ka + LM_CCM_XW) / LM_CCM_XW;
    return c;
}

// Wave per entry of A (grid-stride).  a_q [EA] = query of the entry, a_off / b_off [n_q + 1] delimit the queries' lists in entA /
// entB (B's boxes already carry the query's displacement).  FILL false: cnt[a] = (rows, units) of the entry.  FILL true: row_off /
// unit_off [EA] are the exclusive scans of those; rows [.][3] = (query, position in A, position in B), units [.] = (row, block).
template <bool FILL>
__global__ void __launch_bounds__(256) lm_k_ccm_join(const LmBitImage* __restrict__ entA, const LmBitImage* __restrict__ entB,
                                                     const int32_t* __restrict__ a_q, const int32_t* __restrict__ a_off,
                                                     const int32_t* __restrict__ b_off, int EA, int radius, int2* __restrict__ cnt,
                                                     const long long* __restrict__ row_off, const long long* __restrict__ unit_off,
                                                     int32_t* __restrict__ rows, int2* __restrict__ units)
{
    const int lane = lm_lane();
    const int wave0 = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)), nwaves = (int)(gridDim.x * (blockDim.x >> 6));
    for (int a = wave0; a < EA; a += nwaves) {                  // the same trips for every lane of a wave
        const LmBitImage A = entA[a];
        const int q = a_q[a];
        const int b0 = b_off[q], nb = b_off[q + 1] - b0;
        long long n_rows = 0, n_units = 0;
        for (int base = 0; base < nb; base += 64) {
            const int j = base + lane;
            int blocks = 0;
            if (j < nb) {
                const LmCcmClip c = lm_ccm_clip(A, entB[b0 + j], radius);
                blocks = c.nrb * c.nxb;
            }
            const unsigned long long hit = __ballot(blocks > 0);
            const int incl = lm_wave_incl_scan(blocks);
            const int total = __shfl(incl, 63);
            if (FILL) {
                if (blocks > 0) {
                    const long long row = row_off[a] + n_rows + __popcll(hit & lm_lowmask_excl(lane));
                    rows[row * 3] = q; rows[row * 3 + 1] = a - a_off[q]; rows[row * 3 + 2] = j;
                    int2* u = units + unit_off[a] + n_units + (incl - blocks);
                    for (int k = 0; k < blocks; k++) u[k] = make_int2((int)row, k);
                }
            }
            n_rows += __popcll(hit);
            n_units += total;
        }
        if (!FILL && lane == 0) cnt[a] = make_int2((int)n_rows, (int)(n_units > 0x7fffffff ? 0x7fffffff : n_units));
    }
}

// Workgroup per unit (grid-stride).  counts [n_rows][ne] is zeroed by the caller on the same stream.
__global__ void __launch_bounds__(256) lm_k_ccm_count(const LmBitImage* __restrict__ entA, const LmBitImage* __restrict__ entB,
                                                      const int32_t* __restrict__ a_off, const int32_t* __restrict__ b_off,
                                                      const uint32_t* __restrict__ bits, const int32_t* __restrict__ rows,
                                                      const int2* __restrict__ units, long long n_units, int radius,
                                                      unsigned* __restrict__ counts)
{
    __shared__ unsigned sA[LM_CCM_ROWS * LM_CCM_XW];
    __shared__ unsigned sB[(LM_CCM_ROWS + 2 * LM_CCM_MAX_RADIUS) * LM_CCM_BS];
    __shared__ unsigned sC[LM_CCM_MAX_NE];
    const int T = (int)blockDim.x;
    const int nd = 2 * radius + 1, ne = nd * nd;
    const int G = ne < T ? T / ne : 1;                          // groups of one displacement
    for (long long unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
        const int2 un = units[unit];
        const int32_t* rw = rows + (long long)un.x * 3;
        const LmBitImage A = entA[a_off[rw[0]] + rw[1]], B = entB[b_off[rw[0]] + rw[2]];
        const LmCcmClip c = lm_ccm_clip(A, B, radius);
        const int rb = un.y / c.nxb, xb = un.y - rb * c.nxb;
        const int ya = c.ya + rb * LM_CCM_ROWS;
        const int nrow = (c.yb - ya + 1 < LM_CCM_ROWS) ? c.yb - ya + 1 : LM_CCM_ROWS;
        const int k0 = c.ka + xb * LM_CCM_XW;
        const int nk = (c.kb - k0 + 1 < LM_CCM_XW) ? c.kb - k0 + 1 : LM_CCM_XW;
        const int abw = (A.w + 31) >> 5, bbw = (B.w + 31) >> 5;
        // column of B (its own coordinates) under bit 0 of A's word k0 for ex = +r, the smallest one read; floor to B's word grid
        const int umin = A.x0 + 32 * k0 - B.x0 - radius;
        const int sb0 = umin >> 5;                              // arithmetic shift: floor for negative columns
        const int nsb = nk + 2;                                 // words umin .. umin + 32 (nk - 1) + 2 r + 63
        const int nbr = nrow + 2 * radius;                      // staged row t = row ya + t - r - B.y0 of B
        __syncthreads();                                        // the unit before has read sA / sB / sC
        for (int i = threadIdx.x; i < nrow * nk; i += T) {
            const int r = i / nk, j = i - r * nk;
            sA[r * LM_CCM_XW + j] = bits[A.bits_off + (long long)(ya - A.y0 + r) * abw + k0 + j];
        }
        for (int i = threadIdx.x; i < nbr * nsb; i += T) {
            const int t = i / nsb, s = i - t * nsb;
            const int v = ya + t - radius - B.y0, kw = sb0 + s;
            sB[t * LM_CCM_BS + s] = (v >= 0 && v < B.h && kw >= 0 && kw < bbw) ? bits[B.bits_off + (long long)v * bbw + kw] : 0u;
        }
        for (int i = threadIdx.x; i < ne; i += T) sC[i] = 0;
        __syncthreads();
        for (int slot = threadIdx.x; slot < ne * G; slot += T) {
            const int g = slot / ne, e = slot - g * ne;
            const int eyi = e / nd, ex = e - eyi * nd - radius;
            // B column under bit 0 of A's word k0 + j: umin + radius - ex + 32 j, relative to the staged words
            const int rel = umin + radius - ex - 32 * sb0;      // 0 .. 31 + 2 r
            const int sw = rel >> 5, sh = rel & 31;
            unsigned n = 0;
            for (int idx = g; idx < nrow * nk; idx += G) {
                const int r = idx / nk, j = idx - r * nk;
                const unsigned* b = sB + (r - (eyi - radius) + radius) * LM_CCM_BS + sw + j;
                const unsigned v = (unsigned)(((((unsigned long long)b[1]) << 32) | b[0]) >> sh);
                n += (unsigned)__popc(sA[r * LM_CCM_XW + j] & v);
            }
            if (n) atomicAdd(&sC[e], n);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < ne; i += T)
            if (sC[i]) atomicAdd(&counts[(long long)un.x * ne + i], sC[i]);
    }
}

// ================================================================================================
// host side
// ================================================================================================
extern "C" int lm_kf_pair_counts(LmKeyframes* kf, const int64_t* h_a_off, const int32_t* h_a_items, const int64_t* h_b_off,
                                 const int32_t* h_b_items, const int32_t* h_disp, int n_q, int radius, int32_t* h_rows, int32_t* h_counts,
                                 int64_t cap, int64_t* n_found, void* stream)
{
    if (!kf || !n_found || n_q < 0 || cap < 0 || (cap > 0 && (!h_rows || !h_counts)) || (n_q > 0 && !h_disp)) {
        lm_set_error("lm_kf_pair_counts: bad arguments (null pointer, n_q=%d, cap=%lld)", n_q, (long long)cap);
        return LM_ERR_ARG;
    }
    *n_found = 0;
    if (radius < 0 || radius > LM_CCM_MAX_RADIUS) {
        lm_set_error("lm_kf_pair_counts: radius=%d outside 0 .. %d", radius, LM_CCM_MAX_RADIUS);
        return LM_ERR_ARG;
    }
    if (!lm_kf_lists_ok(kf, h_a_off, h_a_items, n_q) || !lm_kf_lists_ok(kf, h_b_off, h_b_items, n_q)) {
        lm_set_error("lm_kf_pair_counts: bad lists (offsets that descend or do not start at 0, or an item outside the table of %zu)",
                     kf->items.size());
        return LM_ERR_ARG;
    }
    for (int q = 0; q < n_q; q++)
        for (int k = 0; k < 2; k++)
            if (h_disp[2 * q + k] < -LM_CCM_MAX_DISP || h_disp[2 * q + k] > LM_CCM_MAX_DISP) {
                lm_set_error("lm_kf_pair_counts: query %d: displacement (%d, %d) beyond +-%d", q, h_disp[2 * q], h_disp[2 * q + 1], LM_CCM_MAX_DISP);
                return LM_ERR_ARG;
            }
    const int64_t EA = n_q ? h_a_off[n_q] : 0, EB = n_q ? h_b_off[n_q] : 0;
    if (EA == 0 || EB == 0) return LM_OK;
    hipStream_t st = (hipStream_t)stream;
    const int ne = (2 * radius + 1) * (2 * radius + 1);
    // ---- the entries of both sides, B translated, and the lists' offsets
    const size_t o_b = lm_kf_up((size_t)EA * sizeof(LmBitImage)), o_aq = o_b + lm_kf_up((size_t)EB * sizeof(LmBitImage));
    const size_t o_aoff = o_aq + lm_kf_up((size_t)EA * sizeof(int32_t)), o_boff = o_aoff + lm_kf_up((size_t)(n_q + 1) * sizeof(int32_t));
    const size_t o_cnt = o_boff + lm_kf_up((size_t)(n_q + 1) * sizeof(int32_t));
    std::vector<char>& up = kf->stage[4];
    up.assign(o_cnt, 0);
    LmBitImage* hA = (LmBitImage*)up.data();
    LmBitImage* hB = (LmBitImage*)(up.data() + o_b);
    int32_t* h_aq = (int32_t*)(up.data() + o_aq);
    int32_t* h_ao = (int32_t*)(up.data() + o_aoff);
    int32_t* h_bo = (int32_t*)(up.data() + o_boff);
    for (int q = 0; q < n_q; q++) {
        h_ao[q] = (int32_t)h_a_off[q]; h_bo[q] = (int32_t)h_b_off[q];
        for (int64_t e = h_a_off[q]; e < h_a_off[q + 1]; e++) { hA[e] = kf->items[(size_t)h_a_items[e]]; h_aq[e] = q; }
        for (int64_t e = h_b_off[q]; e < h_b_off[q + 1]; e++) {
            hB[e] = kf->items[(size_t)h_b_items[e]];
            hB[e].y0 += h_disp[2 * q]; hB[e].x0 += h_disp[2 * q + 1];
        }
    }
    h_ao[n_q] = (int32_t)EA; h_bo[n_q] = (int32_t)EB;
    char* wsA = (char*)lm_kf_scratch(kf, 4, o_cnt + (size_t)EA * sizeof(int2), "lm_kf_pair_counts");
    if (!wsA) return LM_ERR_HIP;
    LM_HIP(hipMemcpyAsync(wsA, up.data(), o_cnt, hipMemcpyHostToDevice, st));
    const LmBitImage* dA = (const LmBitImage*)wsA;
    const LmBitImage* dB = (const LmBitImage*)(wsA + o_b);
    const int32_t* d_aq = (const int32_t*)(wsA + o_aq);
    const int32_t* d_ao = (const int32_t*)(wsA + o_aoff);
    const int32_t* d_bo = (const int32_t*)(wsA + o_boff);
    int2* d_cnt = (int2*)(wsA + o_cnt);
    const dim3 jgrid((unsigned)std::min<int64_t>((EA + 3) / 4, LM_HIP_EMULATED ? 2 : 4096));
    hipLaunchKernelGGL((lm_k_ccm_join<false>), jgrid, dim3(256), 0, st, dA, dB, d_aq, d_ao, d_bo, (int)EA, radius, d_cnt, (const long long*)nullptr,
                       (const long long*)nullptr, (int32_t*)nullptr, (int2*)nullptr);
    LM_HIP(hipGetLastError());
    std::vector<int2> cnt((size_t)EA);
    LM_HIP(hipMemcpyAsync(cnt.data(), d_cnt, (size_t)EA * sizeof(int2), hipMemcpyDeviceToHost, st));
    LM_HIP(hipStreamSynchronize(st));
    // ---- exclusive scans: where every entry of A writes its rows and units
    std::vector<char>& up2 = kf->stage[5];
    up2.assign((size_t)EA * 2 * sizeof(long long), 0);
    long long* h_ro = (long long*)up2.data();
    long long* h_uo = h_ro + EA;
    long long n_rows = 0, n_units = 0;
    for (int64_t a = 0; a < EA; a++) {
        h_ro[a] = n_rows; h_uo[a] = n_units;
        n_rows += cnt[(size_t)a].x; n_units += cnt[(size_t)a].y;
    }
    *n_found = (int64_t)n_rows;
    if (n_rows > 0x7fffffff / ne || n_units >= 0x7fffffff) {       // an entry's block count saturates at 2^31 - 1
        lm_set_error("lm_kf_pair_counts: %lld rows of %d counts in %lld blocks (limit 2^31)", n_rows, ne, n_units);
        return LM_ERR_CAPACITY;
    }
    if (n_rows > cap) {
        lm_set_error("lm_kf_pair_counts: %lld rows, room for %lld", n_rows, (long long)cap);
        return LM_ERR_CAPACITY;
    }
    if (n_rows == 0) return LM_OK;
    const size_t o_uo = lm_kf_up((size_t)EA * sizeof(long long)), o_rows = o_uo + lm_kf_up((size_t)EA * sizeof(long long));
    const size_t o_units = o_rows + lm_kf_up((size_t)n_rows * 3 * sizeof(int32_t)), o_counts = o_units + lm_kf_up((size_t)n_units * sizeof(int2));
    const size_t cnt_bytes = (size_t)n_rows * ne * sizeof(int32_t);
    char* wsB = (char*)lm_kf_scratch(kf, 5, o_counts + cnt_bytes, "lm_kf_pair_counts");
    if (!wsB) return LM_ERR_HIP;
    LM_HIP(hipMemcpyAsync(wsB, h_ro, (size_t)EA * sizeof(long long), hipMemcpyHostToDevice, st));
    LM_HIP(hipMemcpyAsync(wsB + o_uo, h_uo, (size_t)EA * sizeof(long long), hipMemcpyHostToDevice, st));
    LM_HIP(hipMemsetAsync(wsB + o_counts, 0, cnt_bytes, st));
    int32_t* d_rows = (int32_t*)(wsB + o_rows);
    int2* d_units = (int2*)(wsB + o_units);
    hipLaunchKernelGGL((lm_k_ccm_join<true>), jgrid, dim3(256), 0, st, dA, dB, d_aq, d_ao, d_bo, (int)EA, radius, (int2*)nullptr, (const long long*)wsB,
                       (const long long*)(wsB + o_uo), d_rows, d_units);
    hipLaunchKernelGGL(lm_k_ccm_count, dim3((unsigned)std::min<long long>(n_units, LM_HIP_EMULATED ? 2 : (1 << 20))), dim3(256), 0, st, dA, dB, d_ao, d_bo,
                       kf->d_bits, (const int32_t*)d_rows, (const int2*)d_units, n_units, radius, (unsigned*)(wsB + o_counts));
    LM_HIP(hipGetLastError());
    LM_HIP(hipMemcpyAsync(h_rows, d_rows, (size_t)n_rows * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    LM_HIP(hipMemcpyAsync(h_counts, wsB + o_counts, cnt_bytes, hipMemcpyDeviceToHost, st));
    LM_HIP(hipStreamSynchronize(st));
    return LM_OK;
}
