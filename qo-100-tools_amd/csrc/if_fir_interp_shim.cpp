// if_fir_interp_shim.cpp — the C ABI of the interpolator (include/if_fir.h, if_fir_interp_*; docs/SPEC.md §6).  Its own
// opaque context: nothing of if_fir_ctx_t changes.  Same conventions: 1/0 status, a message per context, no CPU fallback.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <vector>

#include "if_fir.h"
#ifdef IF_FIR_DEVELOPMENT
#include "if_fir_debug.h"
#endif
#include "if_fir_interp.h"
#include "if_fir_stream_ctx.h"

#define IF_FIR_API extern "C" __attribute__((visibility("default")))

// the streaming state: what a call advances (and a failed if_fir_interp_process puts back)
struct interp_state
{
    int hist_cur;
    uint64_t consumed;        // input samples since init/reset (the next call's first output has index consumed * L)
};

struct if_fir_interp : if_fir::StreamCtx
{
    int T, L;
    int ctaps;
    uint32_t backend_req, backend;
    float *d_taps;            // generic kernel: T floats or T (re, im) pairs
    float2 *d_H, *d_tw;       // overlap-save: the multiply table and the twiddles (nullptr outside its range)
    if_fir::StreamHistory hist; // the last hist_len input samples, float32
    int hist_len;
    interp_state st;
    void *d_stage_in, *d_stage_out; // if_fir_interp_process
    uint32_t nco_word;
    int force_full, grid_limit; // development hooks
};

using if_fir::set_err;
static thread_local char g_interp_init_err[256] = "";

static uint32_t resolve_backend(const if_fir_interp *c, uint32_t req)
{
    if (req == IF_FIR_BACKEND_AUTO)
        return if_fir::interp_fft_supported(c->T, c->L) ? IF_FIR_BACKEND_HIP_FFT : IF_FIR_BACKEND_HIP_GENERIC;
    return req;
}

static void free_ctx(if_fir_interp *c)
{
    if (!c)
        return;
    if_fir::stream_ctx_close(c, {c->d_taps, c->d_H, c->d_tw, c->hist.buf[0], c->hist.buf[1], c->d_stage_in, c->d_stage_out});
    delete c;
}

static uint8_t interp_init(if_fir_interp_t **ppCtx, const float *pfTaps, uint32_t ulTaps, uint32_t ulL, uint64_t ullMax,
                           int32_t lDevice, int ctaps)
{
    if (!if_fir::stream_ctx_init_begin(g_interp_init_err, "if_fir_interp_init", ppCtx))
        return 0;
    if (!pfTaps || ulTaps == 0 || ulTaps > IF_FIR_MAX_TAPS)
    {
        set_err(g_interp_init_err, "if_fir_interp_init: taps must be 1..%u (got %u)%s", IF_FIR_MAX_TAPS, ulTaps, pfTaps ? "" : ", pfTaps is NULL");
        return 0;
    }
    if (ulL < 1 || ulL > IF_FIR_MAX_INTERPOLATION)
    {
        set_err(g_interp_init_err, "if_fir_interp_init: interpolation must be 1..%u (got %u)", IF_FIR_MAX_INTERPOLATION, ulL);
        return 0;
    }
    if (ullMax == 0 || ullMax > ((uint64_t)1 << 40) / ulL)
    {
        set_err(g_interp_init_err, "if_fir_interp_init: ullMaxSamples must be 1..2^40/L (got %llu)", (unsigned long long)ullMax);
        return 0;
    }
    if_fir_interp *c = if_fir::stream_ctx_new<if_fir_interp>(g_interp_init_err, "if_fir_interp_init", lDevice);
    if (!c)
        return 0;
    c->T = (int)ulTaps;
    c->L = (int)ulL;
    c->ctaps = ctaps;
    c->backend_req = IF_FIR_BACKEND_AUTO;
    c->backend = resolve_backend(c, IF_FIR_BACKEND_AUTO);
    c->hist_len = if_fir::interp_hist_len(c->T, c->L);
    const size_t tap_floats = (size_t)ulTaps * (ctaps ? 2 : 1);
    hipError_t e = if_fir::stream_ctx_open(c, lDevice, ullMax);
    if_fir::stream_ctx_alloc_upload(e, &c->d_taps, pfTaps, tap_floats * sizeof(float));
    if_fir::stream_history_alloc(e, &c->hist, (size_t)c->hist_len * sizeof(float2), 0);
    if (e == hipSuccess && if_fir::interp_fft_supported(c->T, c->L))
    {
        std::vector<float2> H(if_fir::INTERP_N), tw(if_fir::INTERP_N);
        if_fir::interp_build_tables(pfTaps, c->T, ctaps, H.data(), tw.data());
        if_fir::stream_ctx_alloc_upload(e, &c->d_H, H.data(), H.size() * sizeof(float2));
        if_fir::stream_ctx_alloc_upload(e, &c->d_tw, tw.data(), tw.size() * sizeof(float2));
    }
    if (e == hipSuccess)
        e = hipMalloc(&c->d_stage_in, (size_t)ullMax * 8);
    if (e == hipSuccess)
        e = hipMalloc(&c->d_stage_out, (size_t)ullMax * ulL * 8);
    return if_fir::stream_ctx_init_end(g_interp_init_err, "if_fir_interp_init", e, c, ppCtx, free_ctx);
}

IF_FIR_API uint8_t if_fir_interp_init(if_fir_interp_t **ppCtx, const float *pfTaps, uint32_t ulTaps, uint32_t ulInterpolation,
                                      uint64_t ullMaxSamples, int32_t lDevice)
{
    return interp_init(ppCtx, pfTaps, ulTaps, ulInterpolation, ullMaxSamples, lDevice, 0);
}

IF_FIR_API uint8_t if_fir_interp_init_complex(if_fir_interp_t **ppCtx, const float *pfTapsIQ, uint32_t ulTaps,
                                              uint32_t ulInterpolation, uint64_t ullMaxSamples, int32_t lDevice)
{
    return interp_init(ppCtx, pfTapsIQ, ulTaps, ulInterpolation, ullMaxSamples, lDevice, 1);
}

IF_FIR_API void if_fir_interp_destroy(if_fir_interp_t *pCtx)
{
    free_ctx(pCtx);
}

IF_FIR_API const char *if_fir_interp_last_error(const if_fir_interp_t *pCtx)
{
    return pCtx ? pCtx->err : g_interp_init_err;
}

IF_FIR_API uint8_t if_fir_interp_reset(if_fir_interp_t *pCtx)
{
    if (!pCtx || !if_fir::stream_history_zero(pCtx, pCtx->hist))
        return 0;
    pCtx->st.consumed = 0;
    return 1;
}

IF_FIR_API uint8_t if_fir_interp_set_backend(if_fir_interp_t *pCtx, uint32_t ulBackend)
{
    if (!pCtx)
        return 0;
    if (ulBackend != IF_FIR_BACKEND_AUTO && ulBackend != IF_FIR_BACKEND_HIP_FFT && ulBackend != IF_FIR_BACKEND_HIP_GENERIC)
    {
        set_err(pCtx->err, "if_fir_interp_set_backend: backend %u does not interpolate (AUTO, HIP_FFT or HIP_GENERIC)", ulBackend);
        return 0;
    }
    if (ulBackend == IF_FIR_BACKEND_HIP_FFT && !if_fir::interp_fft_supported(pCtx->T, pCtx->L))
    {
        set_err(pCtx->err, "if_fir_interp_set_backend: the overlap-save backend takes L in {1, 2, 4, ..., 64} and <= %d taps "
                      "(L = %d, %d taps)", if_fir::INTERP_FFT_MAX_TAPS, pCtx->L, pCtx->T);
        return 0;
    }
    pCtx->backend_req = ulBackend;
    pCtx->backend = resolve_backend(pCtx, ulBackend);
    return 1;
}

IF_FIR_API uint32_t if_fir_interp_get_backend(const if_fir_interp_t *pCtx)
{
    return pCtx ? pCtx->backend : 0u;
}

IF_FIR_API uint8_t if_fir_interp_set_input_format(if_fir_interp_t *pCtx, uint32_t ulFormat)
{
    return if_fir::stream_ctx_set_input_format(pCtx, "if_fir_interp_set_input_format", ulFormat);
}

IF_FIR_API uint8_t if_fir_interp_set_nco(if_fir_interp_t *pCtx, double dFreq)
{
    if (!pCtx)
        return 0;
    return if_fir::stream_ctx_nco_word(pCtx, "if_fir_interp_set_nco", dFreq, &pCtx->nco_word);
}

IF_FIR_API uint8_t if_fir_interp_get_nco(const if_fir_interp_t *pCtx, double *pdFreq)
{
    if (!pCtx || !pdFreq)
        return 0;
    *pdFreq = if_fir::nco_freq_of(pCtx->nco_word);
    return 1;
}

IF_FIR_API uint8_t if_fir_interp_set_stream(if_fir_interp_t *pCtx, void *pStream)
{
    return if_fir::stream_ctx_set_stream(pCtx, pStream);
}

IF_FIR_API uint8_t if_fir_interp_synchronize(if_fir_interp_t *pCtx)
{
    return if_fir::stream_ctx_synchronize(pCtx);
}

IF_FIR_API uint64_t if_fir_interp_out_count(const if_fir_interp_t *pCtx, uint64_t ullSamples)
{
    return pCtx ? ullSamples * (uint64_t)pCtx->L : 0;
}

static uint8_t run_device(if_fir_interp *c, const void *in, void *out, uint64_t n, uint64_t *pout, const char *who)
{
    if (n > ((uint64_t)1 << 40) / (uint64_t)c->L)
    {
        set_err(c->err, "%s: sample count too large", who);
        return 0;
    }
    const bool fft = c->backend == IF_FIR_BACKEND_HIP_FFT;
    const uintptr_t in_mask = fft ? (c->in_i16 ? 3 : 7) : 15, out_mask = fft ? 7 : 15;
    if (((uintptr_t)in & in_mask) || ((uintptr_t)out & out_mask))
    {
        set_err(c->err, "%s: device pointers must be %u-byte (input) and %u-byte (output) aligned for this backend", who,
                (unsigned)in_mask + 1, (unsigned)out_mask + 1);
        return 0;
    }
    if (!if_fir::stream_ctx_device_ptrs(c, who, n, in, n, out))
        return 0;
    const uint64_t m = n * (uint64_t)c->L;
    if (pout)
        *pout = m;
    if (n == 0)
        return 1;
    if (if_fir::stream_ctx_capturing(c, who))
        return 0;
    HIP_TRY(c, hipSetDevice(c->device));
    if_fir::InterpArgs a{};
    a.in = in;
    a.out = out;
    a.hist = c->hist.at<float2>(c->st.hist_cur);
    a.hist_out = c->hist.at<float2>(c->st.hist_cur ^ 1);
    a.hist_len = c->hist_len;
    a.H = c->d_H;
    a.tw = c->d_tw;
    a.taps = c->d_taps;
    a.T = c->T;
    a.L = c->L;
    a.ctaps = c->ctaps;
    a.in_i16 = c->in_i16;
    a.N = (int64_t)n;
    a.M = (int64_t)m;
    a.nco_word = c->nco_word;
    a.nco_phi0 = c->nco_word * (uint32_t)(c->st.consumed * (uint64_t)c->L);
    a.full = c->force_full;
    a.grid_limit = c->grid_limit;
    a.device = c->device;
    a.stream = c->stream;
    HIP_TRY(c, fft ? if_fir::launch_interp_fft(a) : if_fir::launch_interp_generic(a));
    c->st.consumed += n;
    c->st.hist_cur ^= 1;
    return 1;
}

IF_FIR_API uint8_t if_fir_interp_process_device(if_fir_interp_t *pCtx, const void *pDevIn, void *pDevOut, uint64_t ullSamples,
                                                uint64_t *pullOutSamples)
{
    if (!pCtx)
        return 0;
    return run_device(pCtx, pDevIn, pDevOut, ullSamples, pullOutSamples, "if_fir_interp_process_device");
}

IF_FIR_API uint8_t if_fir_interp_process(if_fir_interp_t *pCtx, const void *pIQIn, float *pfIQOut, uint64_t ullSamples,
                                         uint64_t *pullOutSamples)
{
    if (!pCtx)
        return 0;
    if (!if_fir::stream_ctx_fits(pCtx, "if_fir_interp_process", ullSamples))
        return 0;
    if (!if_fir::stream_ctx_host_ptrs(pCtx, "if_fir_interp_process", ullSamples, pIQIn, ullSamples, pfIQOut))
        return 0;
    if (pullOutSamples)
        *pullOutSamples = 0;
    if (ullSamples == 0)
        return 1;
    uint64_t m = 0;
    if (!if_fir::stream_ctx_staged(
            pCtx, "if_fir_interp_process", "outputs", pCtx->d_stage_in, pIQIn, ullSamples, &pCtx->st,
            [&] { return run_device(pCtx, pCtx->d_stage_in, pCtx->d_stage_out, ullSamples, &m, "if_fir_interp_process"); },
            [&] { return hipMemcpyAsync(pfIQOut, pCtx->d_stage_out, (size_t)m * 8, hipMemcpyDeviceToHost, pCtx->stream); }))
        return 0;
    if (pullOutSamples)
        *pullOutSamples = m;
    return 1;
}

#ifdef IF_FIR_DEVELOPMENT
IF_FIR_API uint8_t if_fir_debug_interp_config(if_fir_interp_t *pCtx, uint32_t bForceFull, uint32_t ulGridLimit)
{
    if (!pCtx)
        return 0;
    pCtx->force_full = bForceFull ? 1 : 0;
    pCtx->grid_limit = if_fir::stream_ctx_grid_limit(ulGridLimit);
    return 1;
}

IF_FIR_API uint8_t if_fir_debug_interp_seek(if_fir_interp_t *pCtx, uint64_t ullSamples)
{
    if (!pCtx)
        return 0;
    pCtx->st.consumed = ullSamples;
    return 1;
}

IF_FIR_API uint32_t if_fir_debug_interp_tables(const float *pfTaps, uint32_t ulTaps, uint32_t bComplexTaps, float *pfOut,
                                               uint32_t ulOutFloats)
{
    if (!pfTaps || !pfOut || ulOutFloats < 2u * if_fir::INTERP_N || !if_fir::interp_fft_supported((int)ulTaps, 1))
        return 0;
    std::vector<float2> H(if_fir::INTERP_N), tw(if_fir::INTERP_N);
    if_fir::interp_build_tables(pfTaps, (int)ulTaps, bComplexTaps ? 1 : 0, H.data(), tw.data());
    memcpy(pfOut, H.data(), H.size() * sizeof(float2));
    return 2u * if_fir::INTERP_N;
}

IF_FIR_API uint8_t if_fir_debug_interp_plan(uint32_t ulTaps, uint32_t ulInterpolation, uint32_t *pulRows, uint32_t *pulHistLen,
                                            uint32_t *pbFftOk)
{
    if (!pulRows || !pulHistLen || !pbFftOk || ulTaps == 0 || ulTaps > IF_FIR_MAX_TAPS || ulInterpolation < 1 ||
        ulInterpolation > IF_FIR_MAX_INTERPOLATION)
        return 0;
    *pulRows = (uint32_t)if_fir::interp_overlap_rows((int)ulTaps);
    *pulHistLen = (uint32_t)if_fir::interp_hist_len((int)ulTaps, (int)ulInterpolation);
    *pbFftOk = if_fir::interp_fft_supported((int)ulTaps, (int)ulInterpolation) ? 1u : 0u;
    return 1;
}
#endif
