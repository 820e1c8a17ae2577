// lm_handoff.hip -- the hand-off ABI of the sharded path: a frame range of a stream as one packed block (lm_stream_pack*,
// lm_stream_append_packed) and what the temporal matching added to it (lm_stream_*_assign; cc_idx_per_frame,
// cc_stability_estimator.py:102,117).  Included by lm_api.hip after lm_stream.hip.
//
// ------------------------------------------------------------------------------------------------
// Frame-range sharding: the CC records + crops of whole frames as ONE flat device buffer, so that the gather to
// the rank that replays the temporal matching is one send / recv per rank over RCCL (no pickling, no host copy).
// Layout (bytes, little endian): [0,32) header int64 {n_frames, n_cc, n_words, magic}; int64 kept-CC counts per frame, padded
// to a multiple of four entries -- the padding entries are zero; the 32-byte LmCcRec records {int32 cc_id, size; int16 min_x,
// max_x, min_y, max_y; uint64 crop_off; int32 frame, pad} (frame numbers relative to the block's first frame, crop offsets
// relative to its first crop word); the uint32 crop words.  lm_stream_pack writes every byte of the block: equal frame ranges of
// equal streams give equal bytes.
// ------------------------------------------------------------------------------------------------
#define LM_PACK_MAGIC 0x4c4d504b31ll   /* "LMPK1" */

static inline size_t lm_pack_rec_off(long long n_frames) { return 32 + (size_t)((n_frames + 3) & ~3ll) * 8; }
static inline size_t lm_pack_bytes(long long n_frames, long long n_cc, long long n_words)
{
    return lm_pack_rec_off(n_frames) + (size_t)n_cc * sizeof(LmCcRec) + (size_t)n_words * 4;
}

__global__ void __launch_bounds__(256) lm_k_pack_block(const LmCcRec* __restrict__ cc, const uint32_t* __restrict__ crop,
                                                       const long long* __restrict__ frame_cc_off, int first, int n_frames, long long c0,
                                                       long long n_cc, unsigned long long w0, long long nw, long long* __restrict__ head,
                                                       LmCcRec* __restrict__ orec, uint32_t* __restrict__ ocrop)
{
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long long)gridDim.x * blockDim.x;
    if (tid == 0) { head[0] = n_frames; head[1] = n_cc; head[2] = nw; head[3] = LM_PACK_MAGIC; }
    const long long n_counts = ((long long)n_frames + 3) & ~3ll;        // the padding entries are written too (zero): every byte of a block is defined
    for (long long i = tid; i < n_counts; i += nth) head[4 + i] = (i < n_frames) ? frame_cc_off[first + i + 1] - frame_cc_off[first + i] : 0ll;
    for (long long i = tid; i < n_cc; i += nth) {
        LmCcRec r = cc[c0 + i];
        r.frame -= first;
        r.crop_off -= w0;
        orec[i] = r;
    }
    for (long long i = tid; i < nw; i += nth) ocrop[i] = crop[w0 + i];
}

__global__ void __launch_bounds__(256) lm_k_append_block(const LmCcRec* __restrict__ irec, const uint32_t* __restrict__ icrop, long long n_cc,
                                                         long long nw, LmCcRec* __restrict__ cc, uint32_t* __restrict__ crop,
                                                         const LmCounters* __restrict__ cnt)
{
    const long long c0 = cnt->n_cc;
    const unsigned long long w0 = cnt->n_words;
    const int f0 = cnt->n_frames;
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long long)gridDim.x * blockDim.x;
    for (long long i = tid; i < n_cc; i += nth) {
        LmCcRec r = irec[i];
        r.frame += f0;
        r.crop_off += w0;
        cc[c0 + i] = r;
    }
    for (long long i = tid; i < nw; i += nth) crop[w0 + i] = icrop[i];
}

// one workgroup, after lm_k_append_block: exclusive scan of the block's per-frame counts -> frame_cc_off, then the counters
__global__ void __launch_bounds__(1024) lm_k_append_offsets(const long long* __restrict__ head, long long* __restrict__ frame_cc_off,
                                                            LmCounters* __restrict__ cnt)
{
    const int n_frames = (int)head[0];
    const long long c0 = cnt->n_cc;
    const int f0 = cnt->n_frames;
    unsigned long long carry = 0;
    for (int base = 0; base < n_frames; base += 1024) {
        const int i = base + (int)threadIdx.x;
        const unsigned k = (i < n_frames) ? (unsigned)head[4 + i] : 0u;
        unsigned tot;
        const unsigned ex = lm_block_excl_scan<1024>(k, &tot);
        if (i < n_frames) frame_cc_off[f0 + i] = c0 + (long long)(carry + ex);
        carry += tot;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        frame_cc_off[f0 + n_frames] = c0 + head[1];
        cnt->n_cc = c0 + head[1];
        cnt->n_words += (unsigned long long)head[2];
        cnt->n_frames = f0 + n_frames;
    }
}

// record range [c0, c0 + n_cc) and crop-word range [w0, w0 + nw) of frames [first, first + n); synchronises the stream
static int lm_pack_query(LmStream* s, int first, int n, long long* c0, long long* n_cc, unsigned long long* w0, long long* nw, hipStream_t st)
{
    LmCounters h;
    long long c01[2] = {0, 0};
    LM_HIP(hipMemcpyAsync(&h, s->counters, sizeof(h), hipMemcpyDeviceToHost, st));
    LM_HIP(hipMemcpyAsync(&c01[0], s->frame_cc_off + first, sizeof(long long), hipMemcpyDeviceToHost, st));
    LM_HIP(hipMemcpyAsync(&c01[1], s->frame_cc_off + first + n, sizeof(long long), hipMemcpyDeviceToHost, st));
    LM_HIP(hipStreamSynchronize(st));
    if (h.error) { lm_set_error("lm_stream_pack: stream capacity exceeded on device"); return h.error; }
    *c0 = c01[0];
    *n_cc = c01[1] - c01[0];
    *w0 = 0;
    *nw = 0;
    if (*n_cc > 0) {
        // records are emitted in (frame, label) order and their crops appended in the same order: the block's words are contiguous
        LmCcRec r0, r1;
        unsigned long long w1 = h.n_words;
        LM_HIP(hipMemcpyAsync(&r0, s->cc + c01[0], sizeof(LmCcRec), hipMemcpyDeviceToHost, st));
        if (c01[1] < h.n_cc) LM_HIP(hipMemcpyAsync(&r1, s->cc + c01[1], sizeof(LmCcRec), hipMemcpyDeviceToHost, st));
        LM_HIP(hipStreamSynchronize(st));
        if (c01[1] < h.n_cc) w1 = r1.crop_off;
        *w0 = r0.crop_off;
        *nw = (long long)(w1 - r0.crop_off);
    }
    return LM_OK;
}

extern "C" int lm_stream_pack_size(LmStream* s, int first_frame, int n_frames, int64_t* h_bytes, void* stream)
{
    if (!s || !h_bytes || first_frame < 0 || n_frames < 0 || first_frame + n_frames > s->frames_pushed) {
        lm_set_error("lm_stream_pack_size: bad arguments (frames [%d, %d) of %d pushed)", first_frame, first_frame + n_frames, s ? s->frames_pushed : 0);
        return LM_ERR_ARG;
    }
    long long c0, n_cc, nw;
    unsigned long long w0;
    const int rc = lm_pack_query(s, first_frame, n_frames, &c0, &n_cc, &w0, &nw, (hipStream_t)stream);
    if (rc) return rc;
    *h_bytes = (int64_t)lm_pack_bytes(n_frames, n_cc, nw);
    return LM_OK;
}

extern "C" int lm_stream_pack(LmStream* s, int first_frame, int n_frames, void* d_buf, int64_t bytes, void* stream)
{
    if (!s || !d_buf || first_frame < 0 || n_frames < 0 || first_frame + n_frames > s->frames_pushed || (((uintptr_t)d_buf) & 31)) {
        lm_set_error("lm_stream_pack: bad arguments (32-byte aligned device buffer, frames [%d, %d) of %d pushed)", first_frame,
                     first_frame + n_frames, s ? s->frames_pushed : 0);
        return LM_ERR_ARG;
    }
    long long c0, n_cc, nw;
    unsigned long long w0;
    const int rc = lm_pack_query(s, first_frame, n_frames, &c0, &n_cc, &w0, &nw, (hipStream_t)stream);
    if (rc) return rc;
    const size_t need = lm_pack_bytes(n_frames, n_cc, nw);
    if ((size_t)bytes < need) { lm_set_error("lm_stream_pack: buffer of %lld bytes, %lld needed", (long long)bytes, (long long)need); return LM_ERR_CAPACITY; }
    char* b = (char*)d_buf;
    const size_t rec_off = lm_pack_rec_off(n_frames);
    hipLaunchKernelGGL(lm_k_pack_block, dim3(lm_blocks(n_cc + nw / 4 + n_frames, 256, 4096)), dim3(256), 0, (hipStream_t)stream, s->cc, s->crop,
                       s->frame_cc_off, first_frame, n_frames, c0, n_cc, w0, nw, (long long*)b, (LmCcRec*)(b + rec_off),
                       (uint32_t*)(b + rec_off + (size_t)n_cc * sizeof(LmCcRec)));
    LM_HIP(hipGetLastError());
    return LM_OK;
}

extern "C" int lm_stream_append_packed(LmStream* s, const void* d_buf, int64_t bytes, void* stream)
{
    if (!s || !d_buf || bytes < 32 || (((uintptr_t)d_buf) & 31)) { lm_set_error("lm_stream_append_packed: bad arguments"); return LM_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    long long head[4];
    LM_HIP(hipMemcpyAsync(head, d_buf, sizeof(head), hipMemcpyDeviceToHost, st));
    LmCounters h;
    LM_HIP(hipMemcpyAsync(&h, s->counters, sizeof(h), hipMemcpyDeviceToHost, st));
    LM_HIP(hipStreamSynchronize(st));
    if (head[3] != LM_PACK_MAGIC || head[0] < 0 || head[1] < 0 || head[2] < 0 || (size_t)bytes < lm_pack_bytes(head[0], head[1], head[2])) {
        lm_set_error("lm_stream_append_packed: not a packed block (or truncated: %lld bytes)", (long long)bytes);
        return LM_ERR_ARG;
    }
    if (h.error) { lm_set_error("lm_stream_append_packed: stream capacity exceeded on device"); return h.error; }
    if (s->frames_pushed + head[0] > s->cap_frames || h.n_cc + head[1] > s->cap_cc || h.n_words + (unsigned long long)head[2] > s->cap_words) {
        lm_set_error("lm_stream_append_packed: stream too small (frames %lld/%d, ccs %lld/%lld, crop words %llu/%llu)", s->frames_pushed + head[0],
                     s->cap_frames, h.n_cc + head[1], s->cap_cc, h.n_words + (unsigned long long)head[2], s->cap_words);
        return LM_ERR_CAPACITY;
    }
    const char* b = (const char*)d_buf;
    const size_t rec_off = lm_pack_rec_off(head[0]);
    hipLaunchKernelGGL(lm_k_append_block, dim3(lm_blocks(head[1] + head[2] / 4 + 1, 256, 4096)), dim3(256), 0, st, (const LmCcRec*)(b + rec_off),
                       (const uint32_t*)(b + rec_off + (size_t)head[1] * sizeof(LmCcRec)), head[1], head[2], s->cc, s->crop, s->counters);
    if (head[1] > 0)
        hipLaunchKernelGGL(lm_k_crop_hash, dim3(lm_blocks(head[2] / 64 + 1, 4, 2048)), dim3(256), 0, st, s->cc, s->crop, (long long)h.n_cc, head[1],
                           h.n_words + (unsigned long long)head[2], s->chash);
    hipLaunchKernelGGL(lm_k_append_offsets, dim3(1), dim3(1024), 0, st, (const long long*)b, s->frame_cc_off, s->counters);
    LM_HIP(hipGetLastError());
    s->frames_pushed += (int)head[0];
    return LM_OK;
}

// Hand-off of a MATCHED stream to another rank (step 03 on a rank of its own): the packed block carries records and crops, this
// carries what the temporal matching added -- the unique index of every kept CC (cc_idx_per_frame, cc_stability_estimator.py:102,117)
// and the counters.  Layout of d_out (bytes, little endian): int32 assign[n_cc]; zero bytes up to the next multiple of 32; 4 x int64
// {n_cc, n_unique, tempo_count, n_frames}.  `bytes` must be what lm_stream_assign_bytes returned; every byte is written.
__global__ void __launch_bounds__(256) lm_k_assign_tail(const LmCounters* __restrict__ cnt, long long* __restrict__ tail)
{
    if (threadIdx.x == 0) { tail[0] = cnt->n_cc; tail[1] = cnt->n_uniq; tail[2] = (long long)cnt->tempo_count; tail[3] = cnt->n_matched; }
}

__global__ void __launch_bounds__(256) lm_k_assign_apply(const long long* __restrict__ tail, LmCounters* __restrict__ cnt)
{
    if (threadIdx.x == 0) { cnt->n_uniq = (int)tail[1]; cnt->tempo_count = (unsigned long long)tail[2]; cnt->n_matched = (int)tail[3]; }
}

static inline size_t lm_assign_bytes(long long n_cc) { return (((size_t)n_cc * 4 + 31) & ~(size_t)31) + 32; }

extern "C" int lm_stream_assign_bytes(LmStream* s, int64_t* bytes, void* stream)
{
    if (!s || !bytes) { lm_set_error("lm_stream_assign_bytes: bad arguments"); return LM_ERR_ARG; }
    LmCounters h;
    LM_HIP(hipMemcpyAsync(&h, s->counters, sizeof(h), hipMemcpyDeviceToHost, (hipStream_t)stream));
    LM_HIP(hipStreamSynchronize((hipStream_t)stream));
    if (h.error) { lm_set_error("lm_stream_assign_bytes: stream capacity exceeded on device"); return h.error; }
    *bytes = (int64_t)lm_assign_bytes(h.n_cc);
    return LM_OK;
}

extern "C" int lm_stream_export_assign(LmStream* s, void* d_out, int64_t bytes, void* stream)
{
    if (!s || !d_out || bytes < 32 || (((uintptr_t)d_out) & 31)) { lm_set_error("lm_stream_export_assign: bad arguments"); return LM_ERR_ARG; }
    if (s->frames_matched != s->frames_pushed) { lm_set_error("lm_stream_export_assign: %d frames are unmatched", s->frames_pushed - s->frames_matched); return LM_ERR_STATE; }
    hipStream_t st = (hipStream_t)stream;
    LmCounters h;
    LM_HIP(hipMemcpyAsync(&h, s->counters, sizeof(h), hipMemcpyDeviceToHost, st));
    LM_HIP(hipStreamSynchronize(st));
    if (h.error) { lm_set_error("lm_stream_export_assign: stream capacity exceeded on device"); return h.error; }
    if ((size_t)bytes != lm_assign_bytes(h.n_cc)) {             // the caller sizes the buffer with lm_stream_assign_bytes
        lm_set_error("lm_stream_export_assign: buffer of %lld bytes, the stream's %lld CCs need %lld", (long long)bytes, h.n_cc, (long long)lm_assign_bytes(h.n_cc));
        return LM_ERR_ARG;
    }
    // exactly the stream's n_cc entries: what lies behind them in assign[] belongs to an earlier stream of this handle (or to nobody)
    const size_t used = (size_t)h.n_cc * 4, pad = (size_t)bytes - 32 - used;
    if (used) LM_HIP(hipMemcpyAsync(d_out, s->assign, used, hipMemcpyDeviceToDevice, st));
    if (pad) LM_HIP(hipMemsetAsync((char*)d_out + used, 0, pad, st));
    hipLaunchKernelGGL(lm_k_assign_tail, dim3(1), dim3(64), 0, st, s->counters, (long long*)((char*)d_out + bytes - 32));
    LM_HIP(hipGetLastError());
    return LM_OK;
}

// the stream must hold exactly the frames the assignment belongs to (appended with lm_stream_append_packed), all of them unmatched
extern "C" int lm_stream_import_assign(LmStream* s, const void* d_in, int64_t bytes, void* stream)
{
    if (!s || !d_in || bytes < 32 || (((uintptr_t)d_in) & 31)) { lm_set_error("lm_stream_import_assign: bad arguments"); return LM_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    long long tail[4];
    LmCounters h;
    LM_HIP(hipMemcpyAsync(tail, (const char*)d_in + bytes - 32, 32, hipMemcpyDeviceToHost, st));
    LM_HIP(hipMemcpyAsync(&h, s->counters, sizeof(h), hipMemcpyDeviceToHost, st));
    LM_HIP(hipStreamSynchronize(st));
    if (tail[0] != h.n_cc || tail[3] != s->frames_pushed || (size_t)bytes != lm_assign_bytes(tail[0]) || s->frames_matched != 0 || tail[1] > s->cap_uniq) {
        lm_set_error("lm_stream_import_assign: the assignment (%lld CCs, %lld frames) does not belong to this stream (%lld CCs, %d frames, %d matched)",
                     tail[0], tail[3], h.n_cc, s->frames_pushed, s->frames_matched);
        return LM_ERR_ARG;
    }
    LM_HIP(hipMemcpyAsync(s->assign, d_in, (size_t)h.n_cc * 4, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(lm_k_assign_apply, dim3(1), dim3(64), 0, st, (const long long*)((const char*)d_in + bytes - 32), s->counters);
    LM_HIP(hipGetLastError());
    s->frames_matched = s->frames_pushed;
    return LM_OK;
}
