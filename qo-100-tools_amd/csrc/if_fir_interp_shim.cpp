// if_fir_interp_shim.cpp — the C ABI of the interpolator (include/if_fir.h, if_fir_interp_*; docs/SPEC.md §6).  Its own
// opaque context: nothing of if_fir_ctx_t changes.  Same conventions: 1/0 status, a message per context, no CPU fallback.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "if_fir.h"
#ifdef IF_FIR_DEVELOPMENT
#include "if_fir_debug.h"
#endif
#include "if_fir_interp.h"

#define IF_FIR_API extern "C" __attribute__((visibility("default")))

struct if_fir_interp
{
    int device;
    hipStream_t own_stream;
    hipStream_t stream;
    int T, L;
    int ctaps;
    int in_i16;
    uint32_t backend_req, backend;
    float *d_taps;            // generic kernel: T floats or T (re, im) pairs
    float2 *d_H, *d_tw;       // overlap-save: the multiply table and the twiddles (nullptr outside its range)
    float2 *d_hist[2];        // the last hist_len input samples, float32, ping-pong
    int hist_len;
    int hist_cur;
    uint64_t consumed;        // input samples since init/reset (the next call's first output has index consumed * L)
    uint64_t max_samples;
    void *d_stage_in, *d_stage_out; // if_fir_interp_process
    uint32_t nco_word;
    int force_full, grid_limit; // development hooks
    mutable char err[256];
};

static thread_local char g_interp_init_err[256] = "";

static void set_err(const if_fir_interp *ctx, const char *fmt, ...)
{
    char *dst = ctx ? ctx->err : g_interp_init_err;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(dst, 256, fmt, ap);
    va_end(ap);
}

#define HIP_TRY(ctx, call)                                                                                \
    do                                                                                                    \
    {                                                                                                     \
        hipError_t e_ = (call);                                                                           \
        if (e_ != hipSuccess)                                                                             \
        {                                                                                                 \
            set_err(ctx, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__);      \
            return 0;                                                                                     \
        }                                                                                                 \
    } while (0)

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
    (void)hipSetDevice(c->device);
    if (c->stream && c->stream != c->own_stream && hipStreamSynchronize(c->stream) != hipSuccess)
        (void)hipGetLastError();
    if (c->own_stream)
    {
        (void)hipStreamSynchronize(c->own_stream);
        (void)hipStreamDestroy(c->own_stream);
    }
    void *bufs[] = {c->d_taps, c->d_H, c->d_tw, c->d_hist[0], c->d_hist[1], c->d_stage_in, c->d_stage_out};
    for (void *b : bufs)
        if (b)
            (void)hipFree(b);
    delete c;
}

static uint8_t interp_init(if_fir_interp_t **ppCtx, const float *pfTaps, uint32_t ulTaps, uint32_t ulL, uint64_t ullMax,
                           int32_t lDevice, int ctaps)
{
    if (!ppCtx)
    {
        set_err(nullptr, "if_fir_interp_init: ppCtx is NULL");
        return 0;
    }
    *ppCtx = nullptr;
    if (!pfTaps || ulTaps == 0 || ulTaps > IF_FIR_MAX_TAPS)
    {
        set_err(nullptr, "if_fir_interp_init: taps must be 1..%u (got %u)%s", IF_FIR_MAX_TAPS, ulTaps, pfTaps ? "" : ", pfTaps is NULL");
        return 0;
    }
    if (ulL < 1 || ulL > IF_FIR_MAX_INTERPOLATION)
    {
        set_err(nullptr, "if_fir_interp_init: interpolation must be 1..%u (got %u)", IF_FIR_MAX_INTERPOLATION, ulL);
        return 0;
    }
    if (ullMax == 0 || ullMax > ((uint64_t)1 << 40) / ulL)
    {
        set_err(nullptr, "if_fir_interp_init: ullMaxSamples must be 1..2^40/L (got %llu)", (unsigned long long)ullMax);
        return 0;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    {
        (void)hipGetLastError();
        set_err(nullptr, "if_fir_interp_init: no HIP device");
        return 0;
    }
    if (lDevice < 0 || lDevice >= ndev)
    {
        set_err(nullptr, "if_fir_interp_init: device %d does not exist (%d visible)", lDevice, ndev);
        return 0;
    }
    if_fir_interp *c = new (std::nothrow) if_fir_interp();
    if (!c)
    {
        set_err(nullptr, "if_fir_interp_init: out of host memory");
        return 0;
    }
    c->device = lDevice;
    c->T = (int)ulTaps;
    c->L = (int)ulL;
    c->ctaps = ctaps;
    c->max_samples = ullMax;
    c->backend_req = IF_FIR_BACKEND_AUTO;
    c->backend = resolve_backend(c, IF_FIR_BACKEND_AUTO);
    c->hist_len = if_fir::interp_hist_len(c->T, c->L);
    const size_t tap_floats = (size_t)ulTaps * (ctaps ? 2 : 1);
    hipError_t e = hipSetDevice(lDevice);
    if (e == hipSuccess)
        e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    c->stream = c->own_stream;
    if (e == hipSuccess)
        e = hipMalloc(&c->d_taps, tap_floats * sizeof(float));
    if (e == hipSuccess)
        e = hipMemcpy(c->d_taps, pfTaps, tap_floats * sizeof(float), hipMemcpyHostToDevice);
    for (int i = 0; i < 2 && e == hipSuccess; i++)
    {
        e = hipMalloc(&c->d_hist[i], (size_t)c->hist_len * sizeof(float2));
        if (e == hipSuccess)
            e = hipMemset(c->d_hist[i], 0, (size_t)c->hist_len * sizeof(float2));
    }
    if (e == hipSuccess && if_fir::interp_fft_supported(c->T, c->L))
    {
        std::vector<float2> H(if_fir::INTERP_N), tw(if_fir::INTERP_N);
        if_fir::interp_build_tables(pfTaps, c->T, ctaps, H.data(), tw.data());
        e = hipMalloc(&c->d_H, H.size() * sizeof(float2));
        if (e == hipSuccess)
            e = hipMalloc(&c->d_tw, tw.size() * sizeof(float2));
        if (e == hipSuccess)
            e = hipMemcpy(c->d_H, H.data(), H.size() * sizeof(float2), hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = hipMemcpy(c->d_tw, tw.data(), tw.size() * sizeof(float2), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess)
        e = hipMalloc(&c->d_stage_in, (size_t)ullMax * 8);
    if (e == hipSuccess)
        e = hipMalloc(&c->d_stage_out, (size_t)ullMax * ulL * 8);
    if (e != hipSuccess)
    {
        set_err(nullptr, "if_fir_interp_init: %s", hipGetErrorString(e));
        (void)hipGetLastError();
        free_ctx(c);
        return 0;
    }
    *ppCtx = c;
    return 1;
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
    if (!pCtx)
        return 0;
    HIP_TRY(pCtx, hipSetDevice(pCtx->device));
    for (int i = 0; i < 2; i++)
        HIP_TRY(pCtx, hipMemsetAsync(pCtx->d_hist[i], 0, (size_t)pCtx->hist_len * sizeof(float2), pCtx->stream));
    HIP_TRY(pCtx, hipStreamSynchronize(pCtx->stream));
    pCtx->consumed = 0;
    return 1;
}

IF_FIR_API uint8_t if_fir_interp_set_backend(if_fir_interp_t *pCtx, uint32_t ulBackend)
{
    if (!pCtx)
        return 0;
    if (ulBackend != IF_FIR_BACKEND_AUTO && ulBackend != IF_FIR_BACKEND_HIP_FFT && ulBackend != IF_FIR_BACKEND_HIP_GENERIC)
    {
        set_err(pCtx, "if_fir_interp_set_backend: backend %u does not interpolate (AUTO, HIP_FFT or HIP_GENERIC)", ulBackend);
        return 0;
    }
    if (ulBackend == IF_FIR_BACKEND_HIP_FFT && !if_fir::interp_fft_supported(pCtx->T, pCtx->L))
    {
        set_err(pCtx, "if_fir_interp_set_backend: the overlap-save backend takes L in {1, 2, 4, ..., 64} and <= %d taps "
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
    if (!pCtx)
        return 0;
    if (ulFormat > IF_FIR_INPUT_I16)
    {
        set_err(pCtx, "if_fir_interp_set_input_format: unknown format %u", ulFormat);
        return 0;
    }
    pCtx->in_i16 = (int)ulFormat; // (the history is kept as float32: a change of format keeps the stream)
    return 1;
}

IF_FIR_API uint8_t if_fir_interp_set_nco(if_fir_interp_t *pCtx, double dFreq)
{
    if (!pCtx)
        return 0;
    if (!std::isfinite(dFreq) || std::fabs(dFreq) > 0.5)
    {
        set_err(pCtx, "if_fir_interp_set_nco: frequency must be within +-0.5 cycles/sample (got %g)", dFreq);
        return 0;
    }
    pCtx->nco_word = (uint32_t)(int64_t)std::llround(dFreq * 4294967296.0); // mod 2^32, as if_fir_set_nco
    return 1;
}

IF_FIR_API uint8_t if_fir_interp_get_nco(const if_fir_interp_t *pCtx, double *pdFreq)
{
    if (!pCtx || !pdFreq)
        return 0;
    *pdFreq = (double)(int32_t)pCtx->nco_word / 4294967296.0;
    return 1;
}

IF_FIR_API uint8_t if_fir_interp_set_stream(if_fir_interp_t *pCtx, void *pStream)
{
    if (!pCtx)
        return 0;
    pCtx->stream = pStream ? static_cast<hipStream_t>(pStream) : pCtx->own_stream;
    return 1;
}

IF_FIR_API uint8_t if_fir_interp_synchronize(if_fir_interp_t *pCtx)
{
    if (!pCtx)
        return 0;
    HIP_TRY(pCtx, hipSetDevice(pCtx->device));
    HIP_TRY(pCtx, hipStreamSynchronize(pCtx->stream));
    return 1;
}

IF_FIR_API uint64_t if_fir_interp_out_count(const if_fir_interp_t *pCtx, uint64_t ullSamples)
{
    return pCtx ? ullSamples * (uint64_t)pCtx->L : 0;
}

static uint8_t run_device(if_fir_interp *c, const void *in, void *out, uint64_t n, uint64_t *pout, const char *who)
{
    if (n > ((uint64_t)1 << 40) / (uint64_t)c->L)
    {
        set_err(c, "%s: sample count too large", who);
        return 0;
    }
    const bool fft = c->backend == IF_FIR_BACKEND_HIP_FFT;
    const uintptr_t in_mask = fft ? (c->in_i16 ? 3 : 7) : 15, out_mask = fft ? 7 : 15;
    if (((uintptr_t)in & in_mask) || ((uintptr_t)out & out_mask))
    {
        set_err(c, "%s: device pointers must be %u-byte (input) and %u-byte (output) aligned for this backend", who,
                (unsigned)in_mask + 1, (unsigned)out_mask + 1);
        return 0;
    }
    if (n && (!in || !out))
    {
        set_err(c, "%s: NULL device pointer", who);
        return 0;
    }
    const uint64_t m = n * (uint64_t)c->L;
    if (pout)
        *pout = m;
    if (n == 0)
        return 1;
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(c->stream, &capture) == hipSuccess && capture != hipStreamCaptureStatusNone)
    {
        set_err(c, "%s: the context's stream is being captured into a hipGraph; calls carry host-side streaming state and "
                   "cannot be replayed", who);
        return 0;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    if_fir::InterpArgs a{};
    a.in = in;
    a.out = out;
    a.hist = c->d_hist[c->hist_cur];
    a.hist_out = c->d_hist[c->hist_cur ^ 1];
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
    a.nco_phi0 = c->nco_word * (uint32_t)(c->consumed * (uint64_t)c->L);
    a.full = c->force_full;
    a.grid_limit = c->grid_limit;
    a.device = c->device;
    a.stream = c->stream;
    HIP_TRY(c, fft ? if_fir::launch_interp_fft(a) : if_fir::launch_interp_generic(a));
    c->consumed += n;
    c->hist_cur ^= 1;
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
    if (ullSamples > pCtx->max_samples)
    {
        set_err(pCtx, "if_fir_interp_process: %llu samples exceed ullMaxSamples %llu of init", (unsigned long long)ullSamples,
                (unsigned long long)pCtx->max_samples);
        return 0;
    }
    if (ullSamples && (!pIQIn || !pfIQOut))
    {
        set_err(pCtx, "if_fir_interp_process: NULL buffer");
        return 0;
    }
    if (pullOutSamples)
        *pullOutSamples = 0;
    if (ullSamples == 0)
        return 1;
    HIP_TRY(pCtx, hipSetDevice(pCtx->device));
    const size_t in_bytes = (size_t)ullSamples * (pCtx->in_i16 ? 4 : 8);
    const size_t out_bytes = (size_t)ullSamples * pCtx->L * 8;
    HIP_TRY(pCtx, hipMemcpyAsync(pCtx->d_stage_in, pIQIn, in_bytes, hipMemcpyHostToDevice, pCtx->stream));
    uint64_t m = 0;
    if (!run_device(pCtx, pCtx->d_stage_in, pCtx->d_stage_out, ullSamples, &m, "if_fir_interp_process"))
    {
        (void)hipStreamSynchronize(pCtx->stream);
        return 0;
    }
    HIP_TRY(pCtx, hipMemcpyAsync(pfIQOut, pCtx->d_stage_out, out_bytes, hipMemcpyDeviceToHost, pCtx->stream));
    HIP_TRY(pCtx, hipStreamSynchronize(pCtx->stream));
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
    pCtx->grid_limit = (int)(ulGridLimit > 65536u ? 65536u : ulGridLimit);
    return 1;
}

IF_FIR_API uint8_t if_fir_debug_interp_seek(if_fir_interp_t *pCtx, uint64_t ullSamples)
{
    if (!pCtx)
        return 0;
    pCtx->consumed = ullSamples;
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
