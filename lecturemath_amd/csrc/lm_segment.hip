// lm_segment.hip -- step 04, conflict-minimisation segmentation (VIDEO_SEGMENTATION_METHOD = 2): the per-frame conflict signal of
// one segment (AccessMath/preprocessing/content/video_segmenter.py:206-278).  Included by lm_api.hip.
//
// The reference adds, for every conflicting pair of groups alive in the segment and in the iteration order of its dicts, one float64
// weight to every frame of the gap between the two groups.  What a frame ends up with is a sequential float64 sum whose ORDER is
// part of the result (the weighted modes are not exact sums), so the parallel axis here is the frame: one thread per frame walks the
// pair list in list order and does the same `+=` the reference does.  Nothing is reduced across threads and nothing is reordered.
// The pair index, the alive test and the pair's fields are the same in every lane, so they live in scalar registers and pairs that
// are not alive in the segment cost scalar loads and a branch.
#define LM_CS_BLOCK 8
__global__ void __launch_bounds__(64) lm_k_conflict_signal(const int32_t* __restrict__ gap_first, const int32_t* __restrict__ gap_last,
                                                            const int32_t* __restrict__ alive_from, const int32_t* __restrict__ alive_until,
                                                            const double* __restrict__ weight, long long n_pairs, int start_frame, int end_frame,
                                                            double* __restrict__ signal)
{
    const long long f = (long long)start_frame + (long long)blockIdx.x * 64 + threadIdx.x;
    double acc = 0.0;
    long long p = 0;
    // LM_CS_BLOCK pairs at a time, still in list order: the alive fields of a block are fetched together (one wide scalar load per array
    // instead of a load-and-wait per pair) and a block with no pair alive in the segment is skipped after those two loads
    for (; p + LM_CS_BLOCK <= n_pairs; p += LM_CS_BLOCK) {
        unsigned alive = 0;
#pragma unroll
        for (int k = 0; k < LM_CS_BLOCK; k++) alive |= (alive_from[p + k] <= end_frame && alive_until[p + k] >= start_frame) ? (1u << k) : 0u;
        if (!alive) continue;
        int a[LM_CS_BLOCK], b[LM_CS_BLOCK];
        double w[LM_CS_BLOCK];
#pragma unroll
        for (int k = 0; k < LM_CS_BLOCK; k++) { a[k] = gap_first[p + k]; b[k] = gap_last[p + k]; w[k] = weight[p + k]; }
#pragma unroll
        for (int k = 0; k < LM_CS_BLOCK; k++)
            acc = (((alive >> k) & 1u) && f >= a[k] && f <= b[k]) ? acc + w[k] : acc;       // the only arithmetic: the reference's `+=`
    }
    for (; p < n_pairs; p++) {
        if (alive_from[p] > end_frame || alive_until[p] < start_frame) continue;        // one of the two groups is not in the segment
        const int a = gap_first[p], b = gap_last[p];
        const double w = weight[p];
        acc = (f >= a && f <= b) ? acc + w : acc;
    }
    if (f <= end_frame) signal[f - start_frame] = acc;
}

extern "C" int lm_conflict_signal(const int32_t* d_gap_first, const int32_t* d_gap_last, const int32_t* d_alive_from, const int32_t* d_alive_until,
                                  const double* d_weight, int64_t n_pairs, int start_frame, int end_frame, double* d_signal, void* stream)
{
    if (n_pairs < 0 || end_frame < start_frame || !d_signal ||
        (n_pairs > 0 && (!d_gap_first || !d_gap_last || !d_alive_from || !d_alive_until || !d_weight))) {
        lm_set_error("lm_conflict_signal: bad arguments (n_pairs=%lld, frames %d..%d; all arrays are needed when n_pairs > 0)", (long long)n_pairs,
                     start_frame, end_frame);
        return LM_ERR_ARG;
    }
    const long long n = (long long)end_frame - start_frame + 1;
    hipLaunchKernelGGL(lm_k_conflict_signal, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, d_gap_first, d_gap_last, d_alive_from,
                       d_alive_until, d_weight, (long long)n_pairs, start_frame, end_frame, d_signal);
    LM_HIP(hipGetLastError());
    return LM_OK;
}
