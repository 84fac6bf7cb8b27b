// if_fir_rsynth_shim.cpp — the C ABI of the real-output polyphase synthesis bank (include/if_fir.h, if_fir_rsynth_*; docs/SPEC.md
// §18).  Its own opaque context beside the other streaming families.  Same conventions: 1/0 status, a message per context, no
// CPU fallback.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <vector>

#include "if_fir.h"
#ifdef IF_FIR_DEVELOPMENT
#include "if_fir_debug.h"
#endif
#include "if_fir_rsynth.h"
#include "if_fir_stream_ctx.h"

#define IF_FIR_API extern "C" __attribute__((visibility("default")))

// the streaming state: what a call advances (and a failed if_fir_rsynth_process puts back)
struct rsynth_state
{
    int hist_cur;
    uint64_t position;        // input frames since init/reset
};

struct if_fir_rsynth : if_fir::StreamCtx
{
    int M, T, J, L, first_bin, bins;
    int out_i16;
    float *d_taps;            // the table of synth_build_taps
    float2 *d_twiddle;        // the M/2-point transform's
    uint16_t *d_place;        // rsynth_slot_place
    float2 *d_pretangle;      // rsynth_build_twiddles
    if_fir::StreamHistory hist; // the last J - 1 input frames of the span, float32
    float *d_work;            // work_frames x M floats: transformed frames
    uint64_t work_frames;
    rsynth_state st;
    void *d_stage_in;         // if_fir_rsynth_process: staging, allocated by its first call (device-pointer users never pay for it)
    void *d_stage_out;
    int grid_limit;           // development hook
};

using if_fir::set_err;
static thread_local char g_rsynth_init_err[256] = "";

static void free_ctx(if_fir_rsynth *c)
{
    if (!c)
        return;
    if_fir::stream_ctx_close(c, {c->d_taps, c->d_twiddle, c->d_place, c->d_pretangle, c->hist.buf[0], c->hist.buf[1], c->d_work, c->d_stage_in,
                                 c->d_stage_out});
    delete c;
}

// rows of a workspace of `bytes` for this context: no more than its largest call needs
static uint64_t work_rows(const if_fir_rsynth *c, uint64_t bytes)
{
    const uint64_t rows = if_fir::rsynth_workspace_frames(bytes, (uint32_t)c->M, (uint32_t)c->J), most = c->max_samples + (uint64_t)c->J - 1;
    return rows < most ? rows : most;
}

IF_FIR_API uint8_t if_fir_rsynth_init(if_fir_rsynth_t **ppCtx, const if_fir_rsynth_config_t *pCfg, const float *pfTaps, uint32_t ulTaps,
                                      uint64_t ullMaxFrames, int32_t lDevice)
{
    if (!if_fir::stream_ctx_init_begin(g_rsynth_init_err, "if_fir_rsynth_init", ppCtx))
        return 0;
    if (!pCfg)
    {
        set_err(g_rsynth_init_err, "if_fir_rsynth_init: pCfg is NULL");
        return 0;
    }
    const uint32_t M = pCfg->ulChannels, L = pCfg->ulHop;
    if (!if_fir::rsynth_size_ok(M))
    {
        set_err(g_rsynth_init_err, "if_fir_rsynth_init: channels must be 128, 256, 512, 1024, 2048, 4096 or 8192 (got %u)", M);
        return 0;
    }
    if (!pfTaps || ulTaps < 1 || ulTaps > (uint32_t)if_fir::RSYNTH_MAX_ROWS * M)
    {
        set_err(g_rsynth_init_err, "if_fir_rsynth_init: taps must be 1..%u = 16 x channels (got %u)%s", (uint32_t)if_fir::RSYNTH_MAX_ROWS * M,
                ulTaps, pfTaps ? "" : ", pfTaps is NULL");
        return 0;
    }
    if (L < 1 || L > M)
    {
        set_err(g_rsynth_init_err, "if_fir_rsynth_init: hop must be 1..%u (got %u)", M, L);
        return 0;
    }
    if (if_fir::synth_terms(ulTaps, L) > (uint32_t)if_fir::RSYNTH_MAX_TERMS)
    {
        set_err(g_rsynth_init_err, "if_fir_rsynth_init: ceil(taps / hop) must be at most %d (got %u taps at hop %u: %u)",
                if_fir::RSYNTH_MAX_TERMS, ulTaps, L, if_fir::synth_terms(ulTaps, L));
        return 0;
    }
    if (!if_fir::rsynth_span_ok(pCfg->ulFirstBin, pCfg->ulBins, M))
    {
        set_err(g_rsynth_init_err, "if_fir_rsynth_init: the span needs 1 <= ulBins and ulFirstBin + ulBins <= %u = channels / 2 + 1 (got %u, %u)",
                M / 2 + 1, pCfg->ulFirstBin, pCfg->ulBins);
        return 0;
    }
    if (ullMaxFrames == 0 || ullMaxFrames > if_fir::RSYNTH_MAX_CALL)
    {
        set_err(g_rsynth_init_err, "if_fir_rsynth_init: ullMaxFrames must be 1..2^32 (got %llu)", (unsigned long long)ullMaxFrames);
        return 0;
    }
    const uint32_t T = ulTaps, J = if_fir::synth_terms(T, L), H = M / 2;
    std::vector<float> table((size_t)J * L);
    if_fir::synth_build_taps(pfTaps, T, L, table.data());
    const std::vector<float> twiddle = if_fir::stream_ctx_twiddles(H);
    std::vector<uint16_t> place(H);
    for (uint32_t t = 0; t < H; t++)
        place[t] = (uint16_t)if_fir::rsynth_slot_place(t, M);
    std::vector<float> pretangle(2 * (size_t)if_fir::rsynth_pair_items(M));
    if_fir::rsynth_build_twiddles(M, pretangle.data());

    if_fir_rsynth *c = if_fir::stream_ctx_new<if_fir_rsynth>(g_rsynth_init_err, "if_fir_rsynth_init", lDevice);
    if (!c)
        return 0;
    c->M = (int)M;
    c->T = (int)T;
    c->J = (int)J;
    c->L = (int)L;
    c->first_bin = (int)pCfg->ulFirstBin;
    c->bins = (int)pCfg->ulBins;
    hipError_t e = if_fir::stream_ctx_open(c, lDevice, ullMaxFrames);
    c->work_frames = work_rows(c, if_fir::RSYNTH_WORKSPACE_DEFAULT);
    if_fir::stream_ctx_alloc_upload(e, &c->d_taps, table.data(), table.size() * sizeof(float));
    if_fir::stream_ctx_alloc_upload(e, &c->d_twiddle, twiddle.data(), twiddle.size() * sizeof(float));
    if_fir::stream_ctx_alloc_upload(e, &c->d_place, place.data(), place.size() * sizeof(uint16_t));
    if_fir::stream_ctx_alloc_upload(e, &c->d_pretangle, pretangle.data(), pretangle.size() * sizeof(float));
    if_fir::stream_history_alloc(e, &c->hist, (size_t)(c->J - 1) * (size_t)c->bins * sizeof(float2), sizeof(float2));
    if (e == hipSuccess)
        e = hipMalloc(&c->d_work, (size_t)c->work_frames * M * sizeof(float));
    return if_fir::stream_ctx_init_end(g_rsynth_init_err, "if_fir_rsynth_init", e, c, ppCtx, free_ctx);
}

IF_FIR_API void if_fir_rsynth_destroy(if_fir_rsynth_t *pCtx)
{
    free_ctx(pCtx);
}

IF_FIR_API const char *if_fir_rsynth_last_error(const if_fir_rsynth_t *pCtx)
{
    return pCtx ? pCtx->err : g_rsynth_init_err;
}

IF_FIR_API uint8_t if_fir_rsynth_reset(if_fir_rsynth_t *pCtx)
{
    if (!pCtx || !if_fir::stream_history_zero(pCtx, pCtx->hist))
        return 0;
    pCtx->st.position = 0;
    return 1;
}

IF_FIR_API uint8_t if_fir_rsynth_set_input_format(if_fir_rsynth_t *pCtx, uint32_t ulFormat)
{
    return if_fir::stream_ctx_set_input_format(pCtx, "if_fir_rsynth_set_input_format", ulFormat);
}

IF_FIR_API uint8_t if_fir_rsynth_set_output_format(if_fir_rsynth_t *pCtx, uint32_t ulFormat)
{
    if (!pCtx)
        return 0;
    if (ulFormat > IF_FIR_OUTPUT_I16)
    {
        set_err(pCtx->err, "if_fir_rsynth_set_output_format: unknown format %u", ulFormat);
        return 0;
    }
    pCtx->out_i16 = (int)ulFormat;
    return 1;
}

IF_FIR_API uint8_t if_fir_rsynth_set_stream(if_fir_rsynth_t *pCtx, void *pStream)
{
    return if_fir::stream_ctx_set_stream(pCtx, pStream);
}

IF_FIR_API uint8_t if_fir_rsynth_synchronize(if_fir_rsynth_t *pCtx)
{
    return if_fir::stream_ctx_synchronize(pCtx);
}

IF_FIR_API uint64_t if_fir_rsynth_sample_count(const if_fir_rsynth_t *pCtx, uint64_t ullFrames)
{
    if_fir::SynthCall call;
    if (!pCtx || !if_fir::synth_call(pCtx->st.position, ullFrames, (uint32_t)pCtx->M, (uint32_t)pCtx->L, (uint32_t)pCtx->T, &call))
        return 0;
    return call.outputs;
}

// the checks of a call that need no device: the frame count against init's and the stream position against 2^64
static bool plan_call(if_fir_rsynth *c, const char *who, uint64_t frames, if_fir::SynthCall *call)
{
    if (frames > c->max_samples)
    {
        set_err(c->err, "%s: %llu frames exceed ullMaxFrames %llu of init", who, (unsigned long long)frames, (unsigned long long)c->max_samples);
        return false;
    }
    if (!if_fir::synth_call(c->st.position, frames, (uint32_t)c->M, (uint32_t)c->L, (uint32_t)c->T, call))
    {
        set_err(c->err, "%s: frame count too large: the output position would pass 2^64", who);
        return false;
    }
    return true;
}

static uint8_t run_device(if_fir_rsynth *c, const void *in, void *out, uint64_t frames, uint64_t *psamples, const char *who)
{
    if_fir::SynthCall call;
    if (!plan_call(c, who, frames, &call))
        return 0;
    if (!if_fir::stream_ctx_aligned(c, who, "element", in, c->in_i16 ? 3 : 7, out, c->out_i16 ? 1 : 3) ||
        !if_fir::stream_ctx_device_ptrs(c, who, frames, in, frames, out))
        return 0;
    if (if_fir::stream_ctx_capturing(c, who))
        return 0;
    if (psamples)
        *psamples = 0;
    if (frames == 0)
        return 1;
    HIP_TRY(c, hipSetDevice(c->device));
    if_fir::RsynthArgs a{};
    a.in = in;
    a.hist = c->hist.at<float2>(c->st.hist_cur);
    a.hist_out = c->hist.at<float2>(c->st.hist_cur ^ 1);
    a.taps = c->d_taps;
    a.twiddle = c->d_twiddle;
    a.place = c->d_place;
    a.pretangle = c->d_pretangle;
    a.work = c->d_work;
    a.out = out;
    a.M = c->M;
    a.T = c->T;
    a.J = c->J;
    a.L = c->L;
    a.first_bin = c->first_bin;
    a.bins = c->bins;
    a.in_i16 = c->in_i16;
    a.out_i16 = c->out_i16;
    a.frames = (int64_t)frames;
    a.work_frames = c->work_frames;
    a.call = call;
    a.grid_limit = c->grid_limit;
    a.device = c->device;
    a.stream = c->stream;
    HIP_TRY(c, if_fir::launch_rsynth(a));
    c->st.position += frames;
    if (c->J > 1)
        c->st.hist_cur ^= 1;
    if (psamples)
        *psamples = call.outputs;
    return 1;
}

IF_FIR_API uint8_t if_fir_rsynth_process_device(if_fir_rsynth_t *pCtx, const void *pDevIn, void *pDevOut, uint64_t ullFrames,
                                                uint64_t *pullSamples)
{
    if (!pCtx)
        return 0;
    return run_device(pCtx, pDevIn, pDevOut, ullFrames, pullSamples, "if_fir_rsynth_process_device");
}

IF_FIR_API uint8_t if_fir_rsynth_process(if_fir_rsynth_t *pCtx, const void *pFramesIn, void *pOut, uint64_t ullFrames, uint64_t *pullSamples)
{
    if (!pCtx)
        return 0;
    if_fir::SynthCall call;
    if (!plan_call(pCtx, "if_fir_rsynth_process", ullFrames, &call))
        return 0;
    if (!if_fir::stream_ctx_host_ptrs(pCtx, "if_fir_rsynth_process", ullFrames, pFramesIn, ullFrames, pOut))
        return 0;
    if (pullSamples)
        *pullSamples = 0;
    if (ullFrames == 0)
        return 1;
    // the output staging holds float32: the format may change between calls
    if (!pCtx->d_stage_in &&
        !if_fir::stream_ctx_alloc_staging(pCtx, "if_fir_rsynth_process",
                                          {{&pCtx->d_stage_out, (size_t)pCtx->max_samples * (size_t)pCtx->L * sizeof(float)},
                                           {&pCtx->d_stage_in, (size_t)pCtx->max_samples * (size_t)pCtx->bins * 8}}))
        return 0;
    uint64_t m = 0;
    const size_t out_bytes = pCtx->out_i16 ? 2 : 4;
    if (!if_fir::stream_ctx_staged_bytes(
            pCtx, "if_fir_rsynth_process", "outputs", pCtx->d_stage_in, pFramesIn,
            (size_t)ullFrames * (size_t)pCtx->bins * (pCtx->in_i16 ? 4 : 8), &pCtx->st,
            [&] { return run_device(pCtx, pCtx->d_stage_in, pCtx->d_stage_out, ullFrames, &m, "if_fir_rsynth_process"); },
            [&] { return hipMemcpyAsync(pOut, pCtx->d_stage_out, (size_t)m * out_bytes, hipMemcpyDeviceToHost, pCtx->stream); }))
        return 0;
    if (pullSamples)
        *pullSamples = m;
    return 1;
}

#ifdef IF_FIR_DEVELOPMENT
IF_FIR_API uint8_t if_fir_debug_rsynth_config(if_fir_rsynth_t *pCtx, uint32_t ulGridLimit, uint64_t ullPosition)
{
    if (!pCtx)
        return 0;
    if (ullPosition != UINT64_MAX)
    {
        if (!if_fir::stream_history_zero(pCtx, pCtx->hist))
            return 0;
        pCtx->st.position = ullPosition;
    }
    pCtx->grid_limit = if_fir::stream_ctx_grid_limit(ulGridLimit);
    return 1;
}

IF_FIR_API uint8_t if_fir_debug_rsynth_workspace(if_fir_rsynth_t *pCtx, uint64_t ullBytes, uint64_t *pullFrames)
{
    if (!pCtx)
        return 0;
    if (ullBytes)
    {
        const uint64_t rows = work_rows(pCtx, ullBytes);
        HIP_TRY(pCtx, hipSetDevice(pCtx->device));
        HIP_TRY(pCtx, hipStreamSynchronize(pCtx->stream));
        float *work = nullptr;
        HIP_TRY(pCtx, hipMalloc(&work, (size_t)rows * (size_t)pCtx->M * sizeof(float)));
        (void)hipFree(pCtx->d_work);
        pCtx->d_work = work;
        pCtx->work_frames = rows;
    }
    if (pullFrames)
        *pullFrames = if_fir::synth_chunk_frames(pCtx->work_frames, (uint32_t)pCtx->J);
    return 1;
}
#endif
