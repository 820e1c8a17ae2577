// lm_stream.hip -- the frame stream (LmStream of lm_stream.h): lm_stream_* for its lifecycle, pushing frames, temporal matching and the
// host copies of its state (CCStabilityEstimator.add_frame, cc_stability_estimator.py:11-155).  Included by lm_api.hip after lm_ctx.hip,
// lm_match_kernels.hip and lm_match_batch.hip.

extern "C" void lm_stream_destroy(LmStream* s)
{
    if (!s) return;
    void* ptrs[] = {s->cc, s->assign, s->frame_cc_off, s->crop, s->chash, s->active_cc, s->active_box, s->active_last, s->active, s->counters, s->best,
                    s->batch_cc_base, s->batch_word_base};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (s->mb) {
        LmMatchBatch* m = s->mb;
        void* mp[] = {m->nt_cnt, m->nt_src, m->tlast, m->tcur[0], m->tcur[1], m->ftile_all, m->nt_foff, m->nt_list, m->cls, m->troot, m->rootpos, m->ftile, m->s_prefix, m->tcount[0], m->tcount[1], m->toff[0], m->toff[1], m->pairs[0], m->pairs[1], m->pair_u[0],
                      m->pair_u[1], m->sidx, m->s_list, m->s_box, m->newpos, m->n_src, m->ttab, m->tkey, m->twin, m->big[0], m->big[1], m->n_big};
        for (void* p : mp)
            if (p) (void)hipFree(p);
        delete m;
    }
    for (int i = 0; i < s->n_run_events; i++) (void)hipEventDestroy(s->run_events[i]);
    free(s->run_events);
    if (s->rd_scratch) (void)hipFree(s->rd_scratch);
    if (s->garena) (void)hipFree(s->garena);
    if (s->gpin) (void)hipHostFree(s->gpin);
    delete s;
}

extern "C" int lm_stream_set_min_pixels(LmStream* s, int min_pixels)
{
    if (!s || min_pixels < 0) { lm_set_error("lm_stream_set_min_pixels: bad arguments"); return LM_ERR_ARG; }
    s->min_pixels = min_pixels;
    return LM_OK;
}

extern "C" int lm_stream_reset(LmStream* s, void* stream)
{
    if (!s) { lm_set_error("lm_stream_reset: null stream"); return LM_ERR_ARG; }
    LM_HIP(hipMemsetAsync(s->counters, 0, sizeof(LmCounters), (hipStream_t)stream));
    LM_HIP(hipMemsetAsync(s->best, 0xff, (size_t)s->ctx->g.cap * sizeof(unsigned long long), (hipStream_t)stream));
    LM_HIP(hipMemsetAsync(s->frame_cc_off, 0, sizeof(long long), (hipStream_t)stream));
    LM_HIP(hipMemsetAsync(s->chash, 0, (size_t)s->cap_cc * sizeof(uint32_t), (hipStream_t)stream));     // lm_k_emit adds into it
    // the twin table is empty between batches (lm_k_mb_twin_final clears what its batch inserted); a batch cut short by an error leaves entries behind
    if (s->mb) LM_HIP(hipMemsetAsync(s->mb->ttab, 0xff, (size_t)LM_MB_TTAB * sizeof(unsigned long long), (hipStream_t)stream));
    s->frames_pushed = 0;
    s->frames_matched = 0;
    s->tempo_B = 0;
    return LM_OK;
}

extern "C" LmStream* lm_stream_create(LmCtx* ctx, int max_frames, int64_t max_ccs, int64_t max_crop_words, int max_uniques,
                                      double min_recall, double min_precision, int max_gap, int min_pixels)
{
    if (!ctx || max_frames <= 0 || max_ccs <= 0 || max_crop_words <= 0 || max_uniques <= 0) {
        lm_set_error("lm_stream_create: bad arguments");
        return nullptr;
    }
    LmStream* s = new LmStream();
    memset(s, 0, sizeof(*s));
    s->ctx = ctx;
    s->cap_frames = max_frames;
    s->cap_cc = max_ccs;
    s->cap_words = (unsigned long long)max_crop_words;
    s->cap_uniq = max_uniques;
    s->min_recall = min_recall;
    s->min_precision = min_precision;
    s->max_gap = max_gap;
    s->min_pixels = min_pixels;
    int rc = LM_OK;
    rc |= lm_alloc(&s->cc, (size_t)max_ccs);
    rc |= lm_alloc(&s->assign, (size_t)max_ccs);
    rc |= lm_alloc(&s->frame_cc_off, (size_t)max_frames + 1);
    rc |= lm_alloc(&s->crop, (size_t)max_crop_words);
    rc |= lm_alloc(&s->chash, (size_t)max_ccs);
    rc |= lm_alloc(&s->active_cc, (size_t)max_uniques);
    rc |= lm_alloc(&s->active_box, (size_t)max_uniques);
    rc |= lm_alloc(&s->active_last, (size_t)max_uniques);
    rc |= lm_alloc(&s->active, (size_t)max_uniques);
    rc |= lm_alloc(&s->best, (size_t)ctx->g.cap);
    rc |= lm_alloc(&s->counters, (size_t)1);
    rc |= lm_alloc(&s->batch_cc_base, (size_t)ctx->max_batch);
    rc |= lm_alloc(&s->batch_word_base, (size_t)ctx->max_batch);
    {
        LmMatchBatch* m = new LmMatchBatch();
        memset(m, 0, sizeof(*m));
        s->mb = m;
        m->cap_tiles = (int)(max_ccs / LM_MB_TILE) + max_frames + 2;
        long long cp = 16 * (long long)max_ccs;
        if (cp < (1 << 16)) cp = 1 << 16;
        if (cp > (1 << 23)) cp = 1 << 23;
        m->cap_pairs = (uint32_t)cp;
        rc |= lm_alloc(&m->ftile, (size_t)max_frames + 2);
        rc |= lm_alloc(&m->s_prefix, (size_t)max_frames + 2);
        rc |= lm_alloc(&m->ftile_all, (size_t)max_frames + 2);
        rc |= lm_alloc(&m->nt_foff, (size_t)max_frames + 2);
        rc |= lm_alloc(&m->nt_list, (size_t)max_ccs);
        rc |= lm_alloc(&m->cls, (size_t)max_ccs);
        rc |= lm_alloc(&m->troot, (size_t)max_ccs);
        rc |= lm_alloc(&m->rootpos, (size_t)max_ccs);
        rc |= lm_alloc(&m->nt_cnt, (size_t)LM_MB_MAX_FRAMES);
        rc |= lm_alloc(&m->nt_src, (size_t)max_ccs);
        rc |= lm_alloc(&m->tlast, (size_t)max_ccs);
        for (int k = 0; k < 2; k++) {
            rc |= lm_alloc(&m->tcount[k], (size_t)m->cap_tiles + 1);
            rc |= lm_alloc(&m->toff[k], (size_t)m->cap_tiles + 1);
            rc |= lm_alloc(&m->tcur[k], ((size_t)m->cap_tiles + 1) * LM_MB_JY);
            rc |= lm_alloc(&m->pairs[k], (size_t)m->cap_pairs);
            rc |= lm_alloc(&m->pair_u[k], (size_t)m->cap_pairs);
        }
        rc |= lm_alloc(&m->sidx, (size_t)max_ccs);
        rc |= lm_alloc(&m->s_list, (size_t)max_ccs);
        rc |= lm_alloc(&m->s_box, (size_t)max_ccs);
        rc |= lm_alloc(&m->newpos, (size_t)max_ccs);
        rc |= lm_alloc(&m->n_src, (size_t)1);
        rc |= lm_alloc(&m->ttab, (size_t)LM_MB_TTAB);
        rc |= lm_alloc(&m->tkey, (size_t)max_ccs);
        rc |= lm_alloc(&m->twin, (size_t)max_ccs);
        m->cap_big = 1u << 16;
        rc |= lm_alloc(&m->big[0], (size_t)m->cap_big);
        rc |= lm_alloc(&m->big[1], (size_t)m->cap_big);
        rc |= lm_alloc(&m->n_big, (size_t)2);
#if !LM_HIP_EMULATED
        if (rc == LM_OK &&
            hipFuncSetAttribute((const void*)lm_k_mb_resolve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LM_MB_RESOLVE_SMEM) != hipSuccess)
            rc = LM_ERR_HIP;
#endif
        const char* e = getenv("LM_MATCH_PER_FRAME");
        s->match_per_frame = (e && atoi(e) == 1) ? 1 : 0;
    }
    if (rc == LM_OK && hipMemset(s->mb->twin, 0, (size_t)max_ccs) != hipSuccess) rc = LM_ERR_HIP;   // stays 0 when twin detection is off
    if (rc == LM_OK) rc = lm_stream_reset(s, nullptr);
    if (rc == LM_OK && hipStreamSynchronize(nullptr) != hipSuccess) rc = LM_ERR_HIP;
    if (rc != LM_OK) {
        lm_stream_destroy(s);
        return nullptr;
    }
    return s;
}

static void lm_launch_match(LmStream* s, int f, hipStream_t st)
{
    hipLaunchKernelGGL(lm_k_match, LM_HIP_EMULATED ? dim3(2, 2) : dim3(16, 64), dim3(256), 0, st, s->cc, s->crop, s->frame_cc_off, f,
                       s->active_box, s->active_last, s->active_cc, s->counters, s->best, s->min_recall, s->min_precision, s->max_gap);
    // compact the active list every 16 frames (purely an optimisation: retirement is evaluated lazily)
    hipLaunchKernelGGL(lm_k_update, dim3(1), dim3(1024), 0, st, s->cc, s->frame_cc_off, f, s->active, s->active_cc, s->active_box,
                       s->active_last, s->counters, s->assign, s->best, s->max_gap, s->cap_uniq, (f & 15) == 15 ? 1 : 0);
}

// Matches frames [f0, f0 + n) (all emitted already) in chunks of at most LM_MB_MAX_FRAMES frames.
// ev_pre (optional): recorded on `st` in front of the last chunk's replay kernel, i.e. when the wide kernels of the matching
// (twin detection, joins, pair evaluation) have been issued and only the single-workgroup replay, finish and tempo_count remain
// defer_tempo: the tempo_count kernel of the LAST chunk (a wide launch that only adds to a counter) is not launched here but in front
// of the next call's kernels, or by lm_flush_tempo: in the gated schedule it would run beside the next batch's labelling launches,
// deferred it runs beside that batch's record emission instead.  It reads the active list as the replay left it and the tile
// table of its batch: both are untouched until the next batch's lm_k_mb_nt, which the same queue runs after it.
static void lm_flush_tempo(LmStream* s, hipStream_t st)
{
    if (s->tempo_B <= 0) return;
    const LmMatchBatch mb = *s->mb;
    hipLaunchKernelGGL(lm_k_mb_tempo, dim3(LM_HIP_EMULATED ? 2 : 1024), dim3(256), 0, st, s->cc, s->frame_cc_off, s->tempo_f0, s->tempo_B, s->active_box,
                       s->active_cc, s->active_last, s->counters, mb, s->max_gap, s->active, s->assign);
    s->tempo_B = 0;
}

static void lm_launch_match_frames(LmStream* s, int f0, int n, hipStream_t st, hipEvent_t ev_pre = nullptr, bool defer_tempo = false)
{
    if (!s->match_per_frame) lm_flush_tempo(s, st);
    if (s->match_per_frame) {
        for (int i = 0; i < n; i++) lm_launch_match(s, f0 + i, st);
        return;
    }
    const LmMatchBatch mb = *s->mb;
    const dim3 gj(LM_HIP_EMULATED ? 2 : 128, LM_HIP_EMULATED ? 2 : LM_MB_JY), gt(LM_HIP_EMULATED ? 2 : 1024), ge(LM_HIP_EMULATED ? 2 : 2048), gb(LM_HIP_EMULATED ? 2 : 1024);
    for (int done = 0; done < n;) {
        const int B = (n - done < LM_MB_MAX_FRAMES) ? n - done : LM_MB_MAX_FRAMES;
        const int f = f0 + done;
        s->last_match_frames = B;
        const int twins = (s->min_recall <= 1.0 && s->min_precision <= 1.0) ? 1 : 0;     // the twin rule needs "identical crops are accepted"; otherwise twin[] stays 0
        if (twins) {
            const dim3 gc(LM_HIP_EMULATED ? 2 : 256);
            hipLaunchKernelGGL(lm_k_mb_twin_insert, gc, dim3(256), 0, st, s->cc, s->chash, s->frame_cc_off, f, B, s->counters, mb);
            hipLaunchKernelGGL(lm_k_mb_twin_probe, gc, dim3(256), 0, st, s->cc, s->frame_cc_off, f, B, s->counters, mb, s->max_gap);
            hipLaunchKernelGGL(lm_k_mb_twin_cmp, ge, dim3(256), 0, st, s->cc, s->crop, s->frame_cc_off, f, B, s->counters, mb);
            hipLaunchKernelGGL(lm_k_mb_twin_final, gc, dim3(256), 0, st, s->cc, s->frame_cc_off, f, B, s->counters, mb);
        }
        hipLaunchKernelGGL(lm_k_mb_nt, dim3(B + 1), dim3(1024), 0, st, s->frame_cc_off, f, B, s->active, s->active_cc, s->active_box, s->active_last,
                           s->counters, mb, s->max_gap, twins);
        hipLaunchKernelGGL((lm_k_mb_join<0, 0>), gj, dim3(256), 0, st, s->cc, s->frame_cc_off, f, B, s->active_box, s->active_cc, s->counters, mb);
        hipLaunchKernelGGL((lm_k_mb_join<0, 1>), gj, dim3(256), 0, st, s->cc, s->frame_cc_off, f, B, s->active_box, s->active_cc, s->counters, mb);
        hipLaunchKernelGGL((lm_k_mb_eval<0>), ge, dim3(256), 0, st, s->cc, s->crop, s->frame_cc_off, f, B, s->active_last, s->counters, mb,
                           s->min_recall, s->min_precision, s->max_gap);
        hipLaunchKernelGGL((lm_k_mb_eval_big<0>), gb, dim3(256), 0, st, s->cc, s->crop, s->active_last, s->counters, mb, s->min_recall, s->min_precision,
                           s->max_gap);
        hipLaunchKernelGGL(lm_k_mb_sources, dim3(1), dim3(1024), 0, st, s->cc, s->frame_cc_off, f, B, s->counters, mb);
        hipLaunchKernelGGL((lm_k_mb_join<1, 0>), gj, dim3(256), 0, st, s->cc, s->frame_cc_off, f, B, s->active_box, s->active_cc, s->counters, mb);
        hipLaunchKernelGGL((lm_k_mb_join<1, 1>), gj, dim3(256), 0, st, s->cc, s->frame_cc_off, f, B, s->active_box, s->active_cc, s->counters, mb);
        hipLaunchKernelGGL((lm_k_mb_eval<1>), ge, dim3(256), 0, st, s->cc, s->crop, s->frame_cc_off, f, B, s->active_last, s->counters, mb,
                           s->min_recall, s->min_precision, s->max_gap);
        hipLaunchKernelGGL((lm_k_mb_eval_big<1>), gb, dim3(256), 0, st, s->cc, s->crop, s->active_last, s->counters, mb, s->min_recall, s->min_precision,
                           s->max_gap);
        if (ev_pre && done + B >= n) (void)hipEventRecord(ev_pre, st);
        hipLaunchKernelGGL(lm_k_mb_resolve, dim3(1), dim3(LM_MB_RT), LM_MB_RESOLVE_SMEM, st, s->cc, s->frame_cc_off, f, B, s->active, s->active_cc,
                           s->active_box, s->active_last, s->counters, s->assign, mb, s->max_gap, s->cap_uniq);
        if (defer_tempo && done + B >= n) { s->tempo_f0 = f; s->tempo_B = B; }
        else
            hipLaunchKernelGGL(lm_k_mb_tempo, gt, dim3(256), 0, st, s->cc, s->frame_cc_off, f, B, s->active_box, s->active_cc, s->active_last,
                               s->counters, mb, s->max_gap, s->active, s->assign);
        done += B;
    }
}

// statistics, kept-CC selection, record + crop emission for the B frames last labelled in the stream's context
static int lm_stream_emit_batch(LmStream* s, int B, void* stream)
{
    LmCtx* c = s->ctx;
    const LmGeom g = c->g;
    hipStream_t st = (hipStream_t)stream;
    int rc = lm_cc_stats_batch(c, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(lm_k_select, dim3(B), dim3(1024), 0, st, c->st_min_y, c->st_max_y, c->st_min_x, c->st_max_x,
                       c->st_count, c->n_labels, c->kept_label, c->kept_cropoff, c->frame_kept, c->frame_cropwords, g.cap,
                       s->min_pixels);
    hipLaunchKernelGGL(lm_k_batch_offsets, dim3(1), dim3(1024), 0, st, c->frame_kept, c->frame_cropwords, B, s->counters,
                       s->frame_cc_off, s->batch_cc_base, s->batch_word_base, s->cap_cc, s->cap_words, s->cap_frames);
    hipLaunchKernelGGL(lm_k_emit, dim3(LM_HIP_EMULATED ? 2 : LM_EMIT_GRID, B), dim3(256), 0, st, c->bits, c->starts, c->prefix, c->rowoff, c->final_label,
                       c->st_min_y, c->st_max_y, c->st_min_x, c->st_max_x, c->st_count, c->kept_label, c->kept_cropoff,
                       c->frame_kept, c->frame_cropwords, s->batch_cc_base, s->batch_word_base, s->cc, s->crop, s->chash, s->frames_pushed, g.WW,
                       g.H, g.cap);
    LM_HIP(hipGetLastError());
    return LM_OK;
}

// The second half of lm_stream_push_records for callers that label a batch themselves (lm_label_batch on the stream's context)
// and want to schedule the two halves separately.
extern "C" int lm_stream_push_labelled(LmStream* s, int n_frames, void* stream)
{
    if (!s || n_frames <= 0 || n_frames != s->ctx->last_batch) {
        lm_set_error("lm_stream_push_labelled: %d frames, the context's last labelled batch has %d", n_frames, s ? s->ctx->last_batch : 0);
        return LM_ERR_ARG;
    }
    if (s->frames_pushed + n_frames > s->cap_frames) {
        lm_set_error("lm_stream_push_labelled: stream holds %d frames, capacity %d", s->frames_pushed, s->cap_frames);
        return LM_ERR_CAPACITY;
    }
    const int rc = lm_stream_emit_batch(s, n_frames, stream);
    if (rc) return rc;
    s->frames_pushed += n_frames;
    return LM_OK;
}

static int lm_stream_push_impl(LmStream* s, const uint8_t* d_binary, int n_frames, int32_t* d_labels, int do_match, void* stream)
{
    if (!s || !d_binary || n_frames <= 0) { lm_set_error("lm_stream_push: bad arguments"); return LM_ERR_ARG; }
    LmCtx* c = s->ctx;
    const LmGeom g = c->g;
    hipStream_t st = (hipStream_t)stream;
    if (s->frames_pushed + n_frames > s->cap_frames) {
        lm_set_error("lm_stream_push: stream holds %d frames, capacity %d", s->frames_pushed, s->cap_frames);
        return LM_ERR_CAPACITY;
    }
    if (do_match && s->frames_matched != s->frames_pushed) {
        lm_set_error("lm_stream_push: %d frames pushed without matching; call lm_stream_match first", s->frames_pushed - s->frames_matched);
        return LM_ERR_STATE;
    }
    const size_t px = (size_t)g.W * g.H;
    for (int done = 0; done < n_frames;) {
        const int B = (n_frames - done < c->max_batch) ? n_frames - done : c->max_batch;
        int rc = lm_label_batch(c, d_binary + (size_t)done * px, B, d_labels ? d_labels + (size_t)done * px : nullptr, stream);
        if (rc) return rc;
        rc = lm_stream_emit_batch(s, B, stream);
        if (rc) return rc;
        if (do_match) {
            lm_launch_match_frames(s, s->frames_pushed, B, st);
            s->frames_matched += B;
        }
        LM_HIP(hipGetLastError());
        s->frames_pushed += B;
        done += B;
    }
    return LM_OK;
}

extern "C" int lm_stream_push(LmStream* s, const uint8_t* d_binary, int n_frames, int32_t* d_labels, void* stream)
{
    return lm_stream_push_impl(s, d_binary, n_frames, d_labels, 1, stream);
}

extern "C" int lm_stream_push_records(LmStream* s, const uint8_t* d_binary, int n_frames, int32_t* d_labels, void* stream)
{
    return lm_stream_push_impl(s, d_binary, n_frames, d_labels, 0, stream);
}

// Steps 01-02 of a whole resident stream in one call: per batch threshold+invert -> label -> records on `stream_wide`, temporal
// matching on `stream_match` behind an event per batch (the two must be different streams for the phases to overlap).  The
// launch loop runs here instead of in the caller's interpreter: a 10,000-frame stream is ~5,000 kernel launches, and a Python
// loop around them (plus a second Python thread driving step 03 of the previous stream) was the bottleneck of the pipeline.
// d_binary: scratch for `batch` frames; d_labels: label image of one batch, or NULL.  Asynchronous: when the call returns
// everything is enqueued; the work of the stream is complete when `stream_match` has drained.
static int lm_run_events(LmStream* s, int want)
{
    if (want <= s->n_run_events) return LM_OK;
    want += 192;
    hipEvent_t* ev = (hipEvent_t*)realloc(s->run_events, (size_t)want * sizeof(hipEvent_t));
    if (!ev) { lm_set_error("lm_stream_run_logits: out of memory"); return LM_ERR_HIP; }
    s->run_events = ev;
    for (; s->n_run_events < want; s->n_run_events++) LM_HIP(hipEventCreateWithFlags(&s->run_events[s->n_run_events], hipEventDisableTiming));
    return LM_OK;
}

extern "C" int lm_stream_run_logits(LmStream* s, const float* d_logits, int n_frames, int batch, uint8_t* d_binary, int32_t* d_labels, int thr,
                                    int do_match, int schedule, void* stream_wide, void* stream_match)
{
    if (!s || !d_logits || n_frames < 0 || batch <= 0 || batch > s->ctx->max_batch || schedule < 0 || schedule > 1) {
        lm_set_error("lm_stream_run_logits: bad arguments (batch %d, context batch %d, schedule %d)", batch, s ? s->ctx->max_batch : 0, schedule);
        return LM_ERR_ARG;
    }
    if (do_match && s->frames_matched != s->frames_pushed) {
        lm_set_error("lm_stream_run_logits: %d frames pushed without matching; call lm_stream_match first", s->frames_pushed - s->frames_matched);
        return LM_ERR_STATE;
    }
    hipStream_t sw = (hipStream_t)stream_wide, sm = (hipStream_t)stream_match;
    const bool two = do_match && sm != sw;
    const bool gated = two && schedule == 1 && batch <= LM_MB_MAX_FRAMES && !s->match_per_frame;
    const size_t px = (size_t)s->ctx->g.W * s->ctx->g.H;
    const int nb = (n_frames + batch - 1) / batch;
    if (two) { const int rc = lm_run_events(s, 3 * nb); if (rc) return rc; }
    // events of batch k: 3k = labelled, 3k + 1 = records appended, 3k + 2 = its matching has reached the replay kernel
    hipEvent_t* ev = s->run_events;
    int prev_n = 0;
    for (int k = 0, f0 = 0; f0 < n_frames; f0 += batch, k++) {
        const int n = (n_frames - f0 < batch) ? n_frames - f0 : batch;
        if (gated && k >= 2) LM_HIP(hipStreamWaitEvent(sw, ev[3 * (k - 2) + 2], 0));       // the wide kernels of matching k-2 are through
        int rc = lm_label_batch_logits(s->ctx, d_logits + (size_t)f0 * px, n, thr, 1, d_binary, d_labels, stream_wide);
        if (rc) return rc;
        if (gated) LM_HIP(hipEventRecord(ev[3 * k], sw));
        rc = lm_stream_push_labelled(s, n, stream_wide);
        if (rc) return rc;
        if (!do_match) continue;
        if (!two) {
            rc = lm_stream_match(s, n, stream_wide);
            if (rc) return rc;
        } else if (!gated) {
            LM_HIP(hipEventRecord(ev[3 * k + 1], sw));
            LM_HIP(hipStreamWaitEvent(sm, ev[3 * k + 1], 0));
            rc = lm_stream_match(s, n, stream_match);
            if (rc) return rc;
        } else {
            LM_HIP(hipEventRecord(ev[3 * k + 1], sw));
            if (k >= 1) {               // matching of batch k-1 starts when batch k has been labelled (which implies its records are in)
                LM_HIP(hipStreamWaitEvent(sm, ev[3 * k], 0));
                lm_launch_match_frames(s, s->frames_matched, prev_n, sm, ev[3 * (k - 1) + 2], true);
                s->frames_matched += prev_n;
            }
        }
        prev_n = n;
    }
    if (gated && nb > 0) {
        LM_HIP(hipStreamWaitEvent(sm, ev[3 * (nb - 1) + 1], 0));
        lm_launch_match_frames(s, s->frames_matched, prev_n, sm, ev[3 * (nb - 1) + 2]);
        s->frames_matched += prev_n;
    }
    lm_flush_tempo(s, sm);
    LM_HIP(hipGetLastError());
    return LM_OK;
}

extern "C" int lm_stream_match(LmStream* s, int n_frames, void* stream)
{
    if (!s || n_frames < 0 || s->frames_matched + n_frames > s->frames_pushed) {
        lm_set_error("lm_stream_match: %d frames requested, %d pushed, %d matched", n_frames, s ? s->frames_pushed : 0, s ? s->frames_matched : 0);
        return LM_ERR_ARG;
    }
    lm_launch_match_frames(s, s->frames_matched, n_frames, (hipStream_t)stream);
    s->frames_matched += n_frames;
    LM_HIP(hipGetLastError());
    return LM_OK;
}

// Diagnostic: sizes of the LAST matching batch {sources, tiles, pairs vs earlier uniques, pairs vs in-batch sources, frames}.
extern "C" int lm_stream_match_stats(LmStream* s, int64_t* out5, void* stream)
{
    if (!s || !out5 || !s->mb) { lm_set_error("lm_stream_match_stats: bad arguments"); return LM_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    const LmMatchBatch* m = s->mb;
    const int B = s->last_match_frames;
    int32_t nsrc = 0, nt = 0;
    uint32_t ta = 0, tb = 0;
    if (B > 0) {
        LM_HIP(hipMemcpyAsync(&nsrc, m->n_src, 4, hipMemcpyDeviceToHost, st));
        LM_HIP(hipMemcpyAsync(&nt, m->ftile + B, 4, hipMemcpyDeviceToHost, st));
        LM_HIP(hipStreamSynchronize(st));
        if (nt > 0) {
            LM_HIP(hipMemcpyAsync(&ta, m->toff[0] + nt, 4, hipMemcpyDeviceToHost, st));
            LM_HIP(hipMemcpyAsync(&tb, m->toff[1] + nt, 4, hipMemcpyDeviceToHost, st));
            LM_HIP(hipStreamSynchronize(st));
        }
    }
    out5[0] = nsrc; out5[1] = nt; out5[2] = ta; out5[3] = tb; out5[4] = B;
    return LM_OK;
}

// drops retired entries from the active list so that it equals the reference's cc_active after the last frame
__global__ void __launch_bounds__(1024) lm_k_compact_active(int32_t* __restrict__ active, int32_t* __restrict__ active_cc,
                                                            unsigned long long* __restrict__ active_box, int32_t* __restrict__ active_last,
                                                            LmCounters* __restrict__ cnt, int max_gap)
{
    if (cnt->error) return;
    const int f = cnt->n_matched;       // index of the next frame
    const int nA = cnt->n_active;
    if (f <= 1) return;
    unsigned kept = 0;
    for (int base = 0; base < nA; base += 1024) {
        int i = base + (int)threadIdx.x;
        int32_t u = 0, uc = 0, ul = 0;
        unsigned long long ub = 0;
        unsigned keep = 0;
        if (i < nA) {
            u = active[i]; uc = active_cc[i]; ub = active_box[i]; ul = active_last[i];
            keep = ((f - 1) - ul < max_gap) ? 1u : 0u;
        }
        unsigned tot;
        unsigned ex = lm_block_excl_scan<1024>(keep, &tot);
        if (keep) { active[kept + ex] = u; active_cc[kept + ex] = uc; active_box[kept + ex] = ub; active_last[kept + ex] = ul; }
        kept += tot;
    }
    if (threadIdx.x == 0) cnt->n_active = (int)kept;
}

extern "C" int lm_stream_counters(LmStream* s, int64_t* out, void* stream)
{
    if (!s || !out) { lm_set_error("lm_stream_counters: bad arguments"); return LM_ERR_ARG; }
    hipLaunchKernelGGL(lm_k_compact_active, dim3(1), dim3(1024), 0, (hipStream_t)stream, s->active, s->active_cc, s->active_box,
                       s->active_last, s->counters, s->max_gap);
    LmCounters h;
    LM_HIP(hipMemcpyAsync(&h, s->counters, sizeof(h), hipMemcpyDeviceToHost, (hipStream_t)stream));
    LM_HIP(hipStreamSynchronize((hipStream_t)stream));
    out[0] = h.n_frames; out[1] = h.n_cc; out[2] = (int64_t)h.n_words; out[3] = h.n_uniq; out[4] = h.n_active;
    out[5] = (int64_t)h.tempo_count; out[6] = h.error;
    if (h.error) {
        lm_set_error("stream capacity exceeded on device (max_ccs=%lld max_crop_words=%llu max_uniques=%d max_frames=%d)",
                     s->cap_cc, s->cap_words, s->cap_uniq, s->cap_frames);
        return h.error;
    }
    return LM_OK;
}

// unpack host records into the device layout (inverse of lm_k_pack_records)
__global__ void __launch_bounds__(256) lm_k_unpack_records(const int32_t* __restrict__ in8, const long long* __restrict__ crop_off,
                                                           long long n, LmCcRec* __restrict__ cc, int32_t* __restrict__ assign)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int32_t* o = in8 + i * 8;
        LmCcRec r;
        r.cc_id = o[0]; r.min_x = (int16_t)o[1]; r.max_x = (int16_t)o[2]; r.min_y = (int16_t)o[3]; r.max_y = (int16_t)o[4];
        r.size = o[5]; r.frame = o[6]; r.pad = 0; r.crop_off = (unsigned long long)crop_off[i];
        cc[i] = r;
        assign[i] = o[7];
    }
}

__global__ void __launch_bounds__(256) lm_k_import_active(const LmCcRec* __restrict__ cc, const int32_t* __restrict__ active_cc, int n,
                                                          unsigned long long* __restrict__ active_box)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) active_box[i] = lm_pack_box(cc[active_cc[i]]);
}

// Rebuilds a stream on the device from host arrays in lm_stream_read's format (the step-02 -> step-03 hand-off through a
// pickle, console_ui_process.py:150-186).  With the active list (unique index, its first-seen CC, last frame matched; may be
// NULL / 0) the stream can also keep receiving frames.
extern "C" int lm_stream_import(LmStream* s, const int32_t* h_rec, const int64_t* h_frame_off, const int64_t* h_crop_off,
                                const uint32_t* h_crop, int n_frames, int64_t n_cc, int64_t n_crop_words, int n_unique,
                                int64_t tempo_count, const int32_t* h_active, const int32_t* h_active_cc,
                                const int32_t* h_active_last, int n_active, int n_matched, void* stream)
{
    if (!s || n_frames < 0 || n_cc < 0 || n_crop_words < 0 || (n_cc > 0 && (!h_rec || !h_crop_off || !h_crop)) || !h_frame_off ||
        n_matched < 0 || n_matched > n_frames) {
        lm_set_error("lm_stream_import: bad arguments");
        return LM_ERR_ARG;
    }
    if (n_frames > s->cap_frames || n_cc > s->cap_cc || (unsigned long long)n_crop_words > s->cap_words || n_unique > s->cap_uniq) {
        lm_set_error("lm_stream_import: stream too small (frames %d/%d, ccs %lld/%lld, crop words %lld/%llu, uniques %d/%d)", n_frames,
                     s->cap_frames, (long long)n_cc, s->cap_cc, (long long)n_crop_words, s->cap_words, n_unique, s->cap_uniq);
        return LM_ERR_CAPACITY;
    }
    hipStream_t st = (hipStream_t)stream;
    int rc = lm_stream_reset(s, stream);
    if (rc) return rc;
    if (n_cc > 0) {
        int32_t* d_rec = nullptr;
        long long* d_off = nullptr;
        LM_HIP(hipMalloc((void**)&d_rec, (size_t)n_cc * 8 * sizeof(int32_t)));
        if (hipMalloc((void**)&d_off, (size_t)n_cc * sizeof(long long)) != hipSuccess) { (void)hipFree(d_rec); lm_set_error("lm_stream_import: hipMalloc failed"); return LM_ERR_HIP; }
        hipError_t e = hipMemcpyAsync(d_rec, h_rec, (size_t)n_cc * 8 * sizeof(int32_t), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d_off, h_crop_off, (size_t)n_cc * sizeof(long long), hipMemcpyHostToDevice, st);
        if (e == hipSuccess && n_crop_words > 0) e = hipMemcpyAsync(s->crop, h_crop, (size_t)n_crop_words * sizeof(uint32_t), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(lm_k_unpack_records, dim3(lm_blocks(n_cc, 256)), dim3(256), 0, st, d_rec, d_off, (long long)n_cc, s->cc, s->assign);
            hipLaunchKernelGGL(lm_k_crop_hash, dim3(lm_blocks(n_crop_words / 64 + 1, 4, 2048)), dim3(256), 0, st, s->cc, s->crop, 0ll, (long long)n_cc,
                               (unsigned long long)n_crop_words, s->chash);
            e = hipStreamSynchronize(st);
        }
        (void)hipFree(d_rec);
        (void)hipFree(d_off);
        if (e != hipSuccess) { lm_set_error("lm_stream_import: copy failed"); return LM_ERR_HIP; }
    }
    LM_HIP(hipMemcpyAsync(s->frame_cc_off, h_frame_off, (size_t)(n_frames + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
    LmCounters h;
    memset(&h, 0, sizeof(h));
    h.n_cc = n_cc; h.n_words = (unsigned long long)n_crop_words; h.tempo_count = (unsigned long long)tempo_count;
    h.n_frames = n_frames; h.n_matched = n_matched; h.n_uniq = n_unique; h.n_active = 0;
    if (n_active > 0 && h_active && h_active_cc && h_active_last) {
        if (n_active > s->cap_uniq) { lm_set_error("lm_stream_import: active list larger than max_uniques"); return LM_ERR_CAPACITY; }
        LM_HIP(hipMemcpyAsync(s->active, h_active, (size_t)n_active * sizeof(int32_t), hipMemcpyHostToDevice, st));
        LM_HIP(hipMemcpyAsync(s->active_cc, h_active_cc, (size_t)n_active * sizeof(int32_t), hipMemcpyHostToDevice, st));
        LM_HIP(hipMemcpyAsync(s->active_last, h_active_last, (size_t)n_active * sizeof(int32_t), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(lm_k_import_active, dim3(lm_blocks(n_active, 256)), dim3(256), 0, st, s->cc, s->active_cc, n_active, s->active_box);
        h.n_active = n_active;
    }
    LM_HIP(hipMemcpyAsync(s->counters, &h, sizeof(h), hipMemcpyHostToDevice, st));
    LM_HIP(hipStreamSynchronize(st));
    s->frames_pushed = n_frames;
    s->frames_matched = n_matched;
    return LM_OK;
}

// pack records for the host: 8 x int32 per CC
__global__ void __launch_bounds__(256) lm_k_pack_records(const LmCcRec* __restrict__ cc, const int32_t* __restrict__ assign,
                                                         long long n, int32_t* __restrict__ out8, long long* __restrict__ crop_off)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const LmCcRec r = cc[i];
        int32_t* o = out8 + i * 8;
        o[0] = r.cc_id; o[1] = r.min_x; o[2] = r.max_x; o[3] = r.min_y; o[4] = r.max_y; o[5] = r.size; o[6] = r.frame;
        o[7] = assign[i];
        if (crop_off) crop_off[i] = (long long)r.crop_off;
    }
}

extern "C" int lm_stream_read(LmStream* s, int32_t* h_rec, int64_t* h_frame_off, int64_t* h_crop_off, uint32_t* h_crop,
                              int32_t* h_active, void* stream)
{
    if (!s) { lm_set_error("lm_stream_read: null stream"); return LM_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    int64_t k[7];
    int rc = lm_stream_counters(s, k, stream);
    if (rc) return rc;
    const long long n_cc = k[1];
    if ((h_rec || h_crop_off) && n_cc > 0) {
        const size_t need = (size_t)n_cc * (8 * sizeof(int32_t) + sizeof(long long));
        if (s->rd_scratch_bytes < need) {
            if (s->rd_scratch) (void)hipFree(s->rd_scratch);
            s->rd_scratch = nullptr; s->rd_scratch_bytes = 0;
            LM_HIP(hipMalloc(&s->rd_scratch, need + need / 4));
            s->rd_scratch_bytes = need + need / 4;
        }
        long long* d_off = (long long*)s->rd_scratch;                       // 8-byte aligned part first
        int32_t* d_rec = (int32_t*)(d_off + n_cc);
        hipLaunchKernelGGL(lm_k_pack_records, dim3(lm_blocks(n_cc, 256)), dim3(256), 0, st, s->cc, s->assign, n_cc, d_rec, d_off);
        if (h_rec) LM_HIP(hipMemcpyAsync(h_rec, d_rec, (size_t)n_cc * 8 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (h_crop_off) LM_HIP(hipMemcpyAsync(h_crop_off, d_off, (size_t)n_cc * sizeof(long long), hipMemcpyDeviceToHost, st));
        LM_HIP(hipStreamSynchronize(st));
    }
    if (h_frame_off) LM_HIP(hipMemcpyAsync(h_frame_off, s->frame_cc_off, (size_t)(k[0] + 1) * sizeof(long long), hipMemcpyDeviceToHost, st));
    if (h_crop && k[2] > 0) LM_HIP(hipMemcpyAsync(h_crop, s->crop, (size_t)k[2] * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (h_active && k[4] > 0) LM_HIP(hipMemcpyAsync(h_active, s->active, (size_t)k[4] * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    LM_HIP(hipStreamSynchronize(st));
    return LM_OK;
}
