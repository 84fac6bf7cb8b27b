// if_fir_resamp_shim.cpp — the C ABI of the rational resampler (include/if_fir.h, if_fir_resamp_*; docs/SPEC.md §7).  Its own
// opaque context beside if_fir_ctx_t and if_fir_interp_t.  Same conventions: 1/0 status, a message per context, no CPU fallback.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <vector>

#include "if_fir.h"
#ifdef IF_FIR_DEVELOPMENT
#include "if_fir_debug.h"
#endif
#include "if_fir_resamp.h"
#include "if_fir_stream_ctx.h"

#define IF_FIR_API extern "C" __attribute__((visibility("default")))

// the streaming state: what a call advances (and a failed if_fir_resamp_process puts back)
struct resamp_state
{
    int hist_cur;
    uint64_t consumed;        // input samples since init/reset
};

struct if_fir_resamp : if_fir::StreamCtx
{
    int T, L, M;
    int ctaps;
    float *d_taps;            // the phase-major table (resamp_build_taps)
    if_fir::StreamHistory hist; // the last resamp_hist_len input samples, float32
    resamp_state st;
    void *d_stage_in, *d_stage_out; // if_fir_resamp_process
    int grid_limit;           // development hook
};

using if_fir::set_err;
static thread_local char g_resamp_init_err[256] = "";

static void free_ctx(if_fir_resamp *c)
{
    if (!c)
        return;
    if_fir::stream_ctx_close(c, {c->d_taps, c->hist.buf[0], c->hist.buf[1], c->d_stage_in, c->d_stage_out});
    delete c;
}

// the most outputs a call of n inputs can emit, whatever the stream position
static uint64_t max_out(uint64_t n, uint64_t L, uint64_t M)
{
    return (n * L + M - 1) / M + 1;
}

static uint8_t resamp_init(if_fir_resamp_t **ppCtx, const float *pfTaps, uint32_t ulTaps, uint32_t ulL, uint32_t ulM, uint64_t ullMax,
                           int32_t lDevice, int ctaps)
{
    if (!if_fir::stream_ctx_init_begin(g_resamp_init_err, "if_fir_resamp_init", ppCtx))
        return 0;
    if (!pfTaps || ulTaps == 0 || ulTaps > IF_FIR_MAX_TAPS)
    {
        set_err(g_resamp_init_err, "if_fir_resamp_init: taps must be 1..%u (got %u)%s", IF_FIR_MAX_TAPS, ulTaps, pfTaps ? "" : ", pfTaps is NULL");
        return 0;
    }
    if (ulL < 1 || ulL > IF_FIR_MAX_INTERPOLATION)
    {
        set_err(g_resamp_init_err, "if_fir_resamp_init: interpolation must be 1..%u (got %u)", IF_FIR_MAX_INTERPOLATION, ulL);
        return 0;
    }
    if (ulM < 1 || ulM > IF_FIR_MAX_DECIMATION)
    {
        set_err(g_resamp_init_err, "if_fir_resamp_init: decimation must be 1..%u (got %u)", IF_FIR_MAX_DECIMATION, ulM);
        return 0;
    }
    if (ullMax == 0 || ullMax > ((uint64_t)1 << 40) / ulL)
    {
        set_err(g_resamp_init_err, "if_fir_resamp_init: ullMaxSamples must be 1..2^40/L (got %llu)", (unsigned long long)ullMax);
        return 0;
    }
    if_fir_resamp *c = if_fir::stream_ctx_new<if_fir_resamp>(g_resamp_init_err, "if_fir_resamp_init", lDevice);
    if (!c)
        return 0;
    c->T = (int)ulTaps;
    c->L = (int)ulL;
    c->M = (int)ulM;
    c->ctaps = ctaps;
    const if_fir::ResampShape shape = if_fir::resamp_shape(c->T, c->L, c->M);
    std::vector<float> table((size_t)shape.tap_entries * (ctaps ? 2 : 1));
    if_fir::resamp_build_taps(pfTaps, c->T, ctaps, c->L, table.data());
    hipError_t e = if_fir::stream_ctx_open(c, lDevice, ullMax);
    if_fir::stream_ctx_alloc_upload(e, &c->d_taps, table.data(), table.size() * sizeof(float));
    if_fir::stream_history_alloc(e, &c->hist, (size_t)if_fir::resamp_hist_len(c->T, c->L) * sizeof(float2), sizeof(float2));
    if (e == hipSuccess)
        e = hipMalloc(&c->d_stage_in, (size_t)ullMax * 8);
    if (e == hipSuccess)
        e = hipMalloc(&c->d_stage_out, (size_t)max_out(ullMax, ulL, ulM) * 8);
    return if_fir::stream_ctx_init_end(g_resamp_init_err, "if_fir_resamp_init", e, c, ppCtx, free_ctx);
}

IF_FIR_API uint8_t if_fir_resamp_init(if_fir_resamp_t **ppCtx, const float *pfTaps, uint32_t ulTaps, uint32_t ulInterpolation,
                                      uint32_t ulDecimation, uint64_t ullMaxSamples, int32_t lDevice)
{
    return resamp_init(ppCtx, pfTaps, ulTaps, ulInterpolation, ulDecimation, ullMaxSamples, lDevice, 0);
}

IF_FIR_API uint8_t if_fir_resamp_init_complex(if_fir_resamp_t **ppCtx, const float *pfTapsIQ, uint32_t ulTaps, uint32_t ulInterpolation,
                                              uint32_t ulDecimation, uint64_t ullMaxSamples, int32_t lDevice)
{
    return resamp_init(ppCtx, pfTapsIQ, ulTaps, ulInterpolation, ulDecimation, ullMaxSamples, lDevice, 1);
}

IF_FIR_API void if_fir_resamp_destroy(if_fir_resamp_t *pCtx)
{
    free_ctx(pCtx);
}

IF_FIR_API const char *if_fir_resamp_last_error(const if_fir_resamp_t *pCtx)
{
    return pCtx ? pCtx->err : g_resamp_init_err;
}

IF_FIR_API uint8_t if_fir_resamp_reset(if_fir_resamp_t *pCtx)
{
    if (!pCtx || !if_fir::stream_history_zero(pCtx, pCtx->hist))
        return 0;
    pCtx->st.consumed = 0;
    return 1;
}

IF_FIR_API uint8_t if_fir_resamp_set_input_format(if_fir_resamp_t *pCtx, uint32_t ulFormat)
{
    return if_fir::stream_ctx_set_input_format(pCtx, "if_fir_resamp_set_input_format", ulFormat);
}

IF_FIR_API uint8_t if_fir_resamp_set_stream(if_fir_resamp_t *pCtx, void *pStream)
{
    return if_fir::stream_ctx_set_stream(pCtx, pStream);
}

IF_FIR_API uint8_t if_fir_resamp_synchronize(if_fir_resamp_t *pCtx)
{
    return if_fir::stream_ctx_synchronize(pCtx);
}

IF_FIR_API uint64_t if_fir_resamp_out_count(const if_fir_resamp_t *pCtx, uint64_t ullSamples)
{
    if_fir::ResampCall call;
    if (!pCtx || !if_fir::resamp_call(pCtx->st.consumed, ullSamples, pCtx->L, pCtx->M, &call))
        return 0;
    return call.count;
}

static uint8_t run_device(if_fir_resamp *c, const void *in, void *out, uint64_t n, uint64_t *pout, const char *who)
{
    if_fir::ResampCall call;
    if (n > ((uint64_t)1 << 40) / (uint64_t)c->L || !if_fir::resamp_call(c->st.consumed, n, c->L, c->M, &call))
    {
        set_err(c->err, "%s: sample count too large", who);
        return 0;
    }
    if (!if_fir::stream_ctx_aligned(c, who, "sample", in, c->in_i16 ? 3 : 7, out, 7) ||
        !if_fir::stream_ctx_device_ptrs(c, who, n, in, call.count, out))
        return 0;
    if (if_fir::stream_ctx_capturing(c, who))
        return 0;
    if (n == 0)
    {
        if (pout)
            *pout = 0;
        return 1;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    if_fir::ResampArgs a{};
    a.in = in;
    a.out = out;
    a.hist = c->hist.at<float2>(c->st.hist_cur);
    a.hist_out = c->hist.at<float2>(c->st.hist_cur ^ 1);
    a.taps = c->d_taps;
    a.T = c->T;
    a.L = c->L;
    a.M = c->M;
    a.ctaps = c->ctaps;
    a.in_i16 = c->in_i16;
    a.N = (int64_t)n;
    a.count = (int64_t)call.count;
    a.t0 = (int)call.t0;
    a.grid_limit = c->grid_limit;
    a.device = c->device;
    a.stream = c->stream;
    HIP_TRY(c, if_fir::launch_resamp(a));
    c->st.consumed += n;
    c->st.hist_cur ^= 1;
    if (pout)
        *pout = call.count;
    return 1;
}

IF_FIR_API uint8_t if_fir_resamp_process_device(if_fir_resamp_t *pCtx, const void *pDevIn, void *pDevOut, uint64_t ullSamples,
                                                uint64_t *pullOutSamples)
{
    if (!pCtx)
        return 0;
    return run_device(pCtx, pDevIn, pDevOut, ullSamples, pullOutSamples, "if_fir_resamp_process_device");
}

IF_FIR_API uint8_t if_fir_resamp_process(if_fir_resamp_t *pCtx, const void *pIQIn, float *pfIQOut, uint64_t ullSamples,
                                         uint64_t *pullOutSamples)
{
    if (!pCtx)
        return 0;
    if (!if_fir::stream_ctx_fits(pCtx, "if_fir_resamp_process", ullSamples))
        return 0;
    const uint64_t want = if_fir_resamp_out_count(pCtx, ullSamples);
    if (!if_fir::stream_ctx_host_ptrs(pCtx, "if_fir_resamp_process", ullSamples, pIQIn, want, pfIQOut))
        return 0;
    if (pullOutSamples)
        *pullOutSamples = 0;
    if (ullSamples == 0)
        return 1;
    uint64_t m = 0;
    if (!if_fir::stream_ctx_staged(
            pCtx, "if_fir_resamp_process", "outputs", pCtx->d_stage_in, pIQIn, ullSamples, &pCtx->st,
            [&] { return run_device(pCtx, pCtx->d_stage_in, pCtx->d_stage_out, ullSamples, &m, "if_fir_resamp_process"); },
            [&] { return m ? hipMemcpyAsync(pfIQOut, pCtx->d_stage_out, (size_t)m * 8, hipMemcpyDeviceToHost, pCtx->stream) : hipSuccess; }))
        return 0;
    if (pullOutSamples)
        *pullOutSamples = m;
    return 1;
}

#ifdef IF_FIR_DEVELOPMENT
IF_FIR_API uint8_t if_fir_debug_resamp_config(if_fir_resamp_t *pCtx, uint32_t ulGridLimit, uint32_t *pulTileOutputs)
{
    if (!pCtx)
        return 0;
    pCtx->grid_limit = if_fir::stream_ctx_grid_limit(ulGridLimit);
    if (pulTileOutputs)
        *pulTileOutputs = (uint32_t)if_fir::resamp_shape(pCtx->T, pCtx->L, pCtx->M).tile_out;
    return 1;
}
#endif
