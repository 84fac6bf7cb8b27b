// if_fir_rpfb_shim.cpp — the C ABI of the real-input polyphase filter bank (include/if_fir.h, if_fir_rpfb_*; docs/SPEC.md §17).  Its own
// opaque context beside the other streaming families.  Same conventions: 1/0 status, a message per context, no CPU fallback.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <vector>

#include "if_fir.h"
#ifdef IF_FIR_DEVELOPMENT
#include "if_fir_debug.h"
#endif
#include "if_fir_rpfb.h"
#include "if_fir_stream_ctx.h"

#define IF_FIR_API extern "C" __attribute__((visibility("default")))

// the streaming state: what a call advances (and a failed if_fir_rpfb_process puts back)
struct rpfb_state
{
    int hist_cur;
    uint64_t position;        // input samples since init/reset
};

struct if_fir_rpfb : if_fir::StreamCtx
{
    int M, T, K, D, first_bin, bins;
    float *d_taps;            // the table of rpfb_build_taps
    float2 *d_twiddle;        // the M/2-point transform's
    uint32_t *d_places;       // rpfb_build_places
    float2 *d_untangle;       // rpfb_build_twiddles
    if_fir::StreamHistory hist; // the last T - 1 REAL input samples, float32
    int hist_len;
    rpfb_state st;
    void *d_stage_in;         // if_fir_rpfb_process: staging, allocated by its first call (device-pointer users never pay for it)
    float2 *d_stage_out;
    int grid_limit;           // development hook
};

using if_fir::set_err;
static thread_local char g_rpfb_init_err[256] = "";

static void free_ctx(if_fir_rpfb *c)
{
    if (!c)
        return;
    if_fir::stream_ctx_close(c, {c->d_taps, c->d_twiddle, c->d_places, c->d_untangle, c->hist.buf[0], c->hist.buf[1], c->d_stage_in, c->d_stage_out});
    delete c;
}

IF_FIR_API uint8_t if_fir_rpfb_init(if_fir_rpfb_t **ppCtx, const if_fir_rpfb_config_t *pCfg, const float *pfTaps, uint32_t ulTaps,
                                   uint64_t ullMaxSamples, int32_t lDevice)
{
    if (!if_fir::stream_ctx_init_begin(g_rpfb_init_err, "if_fir_rpfb_init", ppCtx))
        return 0;
    if (!pCfg)
    {
        set_err(g_rpfb_init_err, "if_fir_rpfb_init: pCfg is NULL");
        return 0;
    }
    const uint32_t M = pCfg->ulChannels;
    if (!if_fir::rpfb_size_ok(M))
    {
        set_err(g_rpfb_init_err, "if_fir_rpfb_init: channels must be 128, 256, 512, 1024, 2048, 4096 or 8192 (got %u)", M);
        return 0;
    }
    if (!pfTaps || ulTaps < 1 || ulTaps > (uint32_t)if_fir::RPFB_MAX_ROWS * M)
    {
        set_err(g_rpfb_init_err, "if_fir_rpfb_init: taps must be 1..%u = 16 x channels (got %u)%s", (uint32_t)if_fir::RPFB_MAX_ROWS * M, ulTaps,
                pfTaps ? "" : ", pfTaps is NULL");
        return 0;
    }
    if (pCfg->ulHop < 1 || pCfg->ulHop > M)
    {
        set_err(g_rpfb_init_err, "if_fir_rpfb_init: hop must be 1..%u (got %u)", M, pCfg->ulHop);
        return 0;
    }
    if (!if_fir::rpfb_span_ok(pCfg->ulFirstBin, pCfg->ulBins, M))
    {
        set_err(g_rpfb_init_err, "if_fir_rpfb_init: the span needs 1 <= ulBins and ulFirstBin + ulBins <= %u = channels / 2 + 1 (got %u, %u)",
                M / 2 + 1, pCfg->ulFirstBin, pCfg->ulBins);
        return 0;
    }
    if (ullMaxSamples == 0 || ullMaxSamples > if_fir::RPFB_MAX_CALL)
    {
        set_err(g_rpfb_init_err, "if_fir_rpfb_init: ullMaxSamples must be 1..2^40 (got %llu)", (unsigned long long)ullMaxSamples);
        return 0;
    }
    const uint32_t T = ulTaps, K = if_fir::rpfb_rows(T, M), bins = pCfg->ulBins;
    std::vector<float> table((size_t)K * M);
    if_fir::rpfb_build_taps(pfTaps, T, M, table.data());
    const std::vector<float> twiddle = if_fir::stream_ctx_twiddles(M / 2);
    std::vector<uint32_t> places(M / 2);
    if_fir::rpfb_build_places(M, places.data());
    std::vector<float> untangle(2 * ((size_t)M / 2 + 1));
    if_fir::rpfb_build_twiddles(M, untangle.data());

    if_fir_rpfb *c = if_fir::stream_ctx_new<if_fir_rpfb>(g_rpfb_init_err, "if_fir_rpfb_init", lDevice);
    if (!c)
        return 0;
    c->M = (int)M;
    c->T = (int)T;
    c->K = (int)K;
    c->D = (int)pCfg->ulHop;
    c->first_bin = (int)pCfg->ulFirstBin;
    c->bins = (int)bins;
    c->hist_len = (int)T - 1;
    hipError_t e = if_fir::stream_ctx_open(c, lDevice, ullMaxSamples);
    if_fir::stream_ctx_alloc_upload(e, &c->d_taps, table.data(), table.size() * sizeof(float));
    if_fir::stream_ctx_alloc_upload(e, &c->d_twiddle, twiddle.data(), twiddle.size() * sizeof(float));
    if_fir::stream_ctx_alloc_upload(e, &c->d_places, places.data(), places.size() * sizeof(uint32_t));
    if_fir::stream_ctx_alloc_upload(e, &c->d_untangle, untangle.data(), untangle.size() * sizeof(float));
    if_fir::stream_history_alloc(e, &c->hist, (size_t)c->hist_len * sizeof(float), sizeof(float));
    return if_fir::stream_ctx_init_end(g_rpfb_init_err, "if_fir_rpfb_init", e, c, ppCtx, free_ctx);
}

IF_FIR_API void if_fir_rpfb_destroy(if_fir_rpfb_t *pCtx)
{
    free_ctx(pCtx);
}

IF_FIR_API const char *if_fir_rpfb_last_error(const if_fir_rpfb_t *pCtx)
{
    return pCtx ? pCtx->err : g_rpfb_init_err;
}

IF_FIR_API uint8_t if_fir_rpfb_reset(if_fir_rpfb_t *pCtx)
{
    if (!pCtx || !if_fir::stream_history_zero(pCtx, pCtx->hist))
        return 0;
    pCtx->st.position = 0;
    return 1;
}

IF_FIR_API uint8_t if_fir_rpfb_set_input_format(if_fir_rpfb_t *pCtx, uint32_t ulFormat)
{
    return if_fir::stream_ctx_set_input_format(pCtx, "if_fir_rpfb_set_input_format", ulFormat);
}

IF_FIR_API uint8_t if_fir_rpfb_set_stream(if_fir_rpfb_t *pCtx, void *pStream)
{
    return if_fir::stream_ctx_set_stream(pCtx, pStream);
}

IF_FIR_API uint8_t if_fir_rpfb_synchronize(if_fir_rpfb_t *pCtx)
{
    return if_fir::stream_ctx_synchronize(pCtx);
}

IF_FIR_API uint64_t if_fir_rpfb_frame_count(const if_fir_rpfb_t *pCtx, uint64_t ullSamples)
{
    if_fir::RpfbCall call;
    if (!pCtx || !if_fir::rpfb_call(pCtx->st.position, ullSamples, (uint32_t)pCtx->M, (uint32_t)pCtx->D, (uint32_t)pCtx->T, &call))
        return 0;
    return call.frames;
}

static uint8_t run_device(if_fir_rpfb *c, const void *in, void *out, uint64_t n, uint64_t *pframes, const char *who)
{
    if_fir::RpfbCall call;
    if (!if_fir::stream_ctx_fits(c, who, n))
        return 0;
    if (!if_fir::rpfb_call(c->st.position, n, (uint32_t)c->M, (uint32_t)c->D, (uint32_t)c->T, &call))
    {
        set_err(c->err, "%s: sample count too large: the stream position would pass 2^64", who);
        return 0;
    }
    if (!if_fir::stream_ctx_aligned(c, who, "sample", in, c->in_i16 ? 1 : 3, out, 7) ||
        !if_fir::stream_ctx_device_ptrs(c, who, n, in, call.frames, out))
        return 0;
    if (if_fir::stream_ctx_capturing(c, who))
        return 0;
    if (pframes)
        *pframes = 0;
    if (n == 0)
        return 1;
    HIP_TRY(c, hipSetDevice(c->device));
    if_fir::RpfbArgs a{};
    a.in = in;
    a.hist = c->hist.at<float>(c->st.hist_cur);
    a.hist_out = c->hist.at<float>(c->st.hist_cur ^ 1);
    a.taps = c->d_taps;
    a.twiddle = c->d_twiddle;
    a.places = c->d_places;
    a.untangle = c->d_untangle;
    a.out = static_cast<float2 *>(out);
    a.M = c->M;
    a.T = c->T;
    a.K = c->K;
    a.D = c->D;
    a.first_bin = c->first_bin;
    a.bins = c->bins;
    a.in_i16 = c->in_i16;
    a.hist_len = c->hist_len;
    a.n = (int64_t)n;
    a.call = call;
    a.grid_limit = c->grid_limit;
    a.device = c->device;
    a.stream = c->stream;
    HIP_TRY(c, if_fir::launch_rpfb(a));
    c->st.position += n;
    if (c->hist_len > 0)
        c->st.hist_cur ^= 1;
    if (pframes)
        *pframes = call.frames;
    return 1;
}

IF_FIR_API uint8_t if_fir_rpfb_process_device(if_fir_rpfb_t *pCtx, const void *pDevIn, void *pDevOut, uint64_t ullSamples, uint64_t *pullFrames)
{
    if (!pCtx)
        return 0;
    return run_device(pCtx, pDevIn, pDevOut, ullSamples, pullFrames, "if_fir_rpfb_process_device");
}

IF_FIR_API uint8_t if_fir_rpfb_process(if_fir_rpfb_t *pCtx, const void *pIn, float *pfIQOut, uint64_t ullSamples, uint64_t *pullFrames)
{
    if (!pCtx)
        return 0;
    if (!if_fir::stream_ctx_fits(pCtx, "if_fir_rpfb_process", ullSamples))
        return 0;
    if_fir::RpfbCall call;
    if (!if_fir::rpfb_call(pCtx->st.position, ullSamples, (uint32_t)pCtx->M, (uint32_t)pCtx->D, (uint32_t)pCtx->T, &call))
    {
        set_err(pCtx->err, "if_fir_rpfb_process: sample count too large: the stream position would pass 2^64");
        return 0;
    }
    if (!if_fir::stream_ctx_host_ptrs(pCtx, "if_fir_rpfb_process", ullSamples, pIn, call.frames, pfIQOut))
        return 0;
    if (pullFrames)
        *pullFrames = 0;
    if (ullSamples == 0)
        return 1;
    // the most frames of a call of ullMaxSamples samples, whatever the position
    const size_t frames = (size_t)((pCtx->max_samples + (uint64_t)pCtx->D - 1) / (uint64_t)pCtx->D);
    if (!pCtx->d_stage_in &&
        !if_fir::stream_ctx_alloc_staging(pCtx, "if_fir_rpfb_process",
                                          {{(void **)&pCtx->d_stage_out, frames * (size_t)pCtx->bins * sizeof(float2)},
                                           {&pCtx->d_stage_in, (size_t)pCtx->max_samples * 4}}))
        return 0;
    uint64_t m = 0;
    if (!if_fir::stream_ctx_staged_bytes(
            pCtx, "if_fir_rpfb_process", "frames", pCtx->d_stage_in, pIn, (size_t)ullSamples * (pCtx->in_i16 ? 2 : 4), &pCtx->st,
            [&] { return run_device(pCtx, pCtx->d_stage_in, pCtx->d_stage_out, ullSamples, &m, "if_fir_rpfb_process"); },
            [&] {
                return m ? hipMemcpyAsync(pfIQOut, pCtx->d_stage_out, (size_t)m * (size_t)pCtx->bins * sizeof(float2), hipMemcpyDeviceToHost,
                                          pCtx->stream)
                         : hipSuccess;
            }))
        return 0;
    if (pullFrames)
        *pullFrames = m;
    return 1;
}

#ifdef IF_FIR_DEVELOPMENT
IF_FIR_API uint8_t if_fir_debug_rpfb_config(if_fir_rpfb_t *pCtx, uint32_t ulGridLimit, uint32_t *pulGroupFrames, uint64_t ullPosition)
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
    if (pulGroupFrames)
        *pulGroupFrames = if_fir::rpfb_group_frames((uint32_t)pCtx->M);
    return 1;
}
#endif
