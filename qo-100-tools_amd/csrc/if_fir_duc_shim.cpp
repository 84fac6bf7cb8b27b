// if_fir_duc_shim.cpp — the C ABI of the real-output up-converter (include/if_fir.h, if_fir_duc_*; docs/SPEC.md §11).  Its own
// opaque context beside the other streaming families.  Same conventions: 1/0 status, a message per context, no CPU fallback.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "if_fir.h"
#ifdef IF_FIR_DEVELOPMENT
#include "if_fir_debug.h"
#endif
#include "if_fir_duc.h"
#include "if_fir_stream_ctx.h"

#define IF_FIR_API extern "C" __attribute__((visibility("default")))

// the streaming state: what a call advances (and a failed if_fir_duc_process puts back)
struct duc_state
{
    int hist_cur;
    uint64_t consumed;        // input samples since init/reset
};

struct if_fir_duc : if_fir::StreamCtx
{
    int T, L;
    int ctaps;
    int out_i16;
    std::vector<float> h_taps; // as given to init
    uint32_t nco_word;        // SPEC §11 phase word (0 = no mixing)
    float *d_taps;            // the table of duc_build_table for nco_word
    float2 *d_hist[2];        // the last K - 1 input samples, unrotated float32 I/Q, ping-pong
    int hist_len;
    duc_state st;
    void *d_stage_in, *d_stage_out; // if_fir_duc_process
    int grid_limit;           // development hook
};

using if_fir::set_err;
static thread_local char g_duc_init_err[256] = "";

static void free_ctx(if_fir_duc *c)
{
    if (!c)
        return;
    if_fir::stream_ctx_close(c, {c->d_taps, c->d_hist[0], c->d_hist[1], c->d_stage_in, c->d_stage_out});
    delete c;
}

// the kernel's table for a phase word: g = h e^{+j theta k} in float64, rounded once, in the order the kernel reads it
static std::vector<float> build_table(const if_fir_duc *c, uint32_t word)
{
    std::vector<float> g(2 * (size_t)c->T), table(2 * (size_t)if_fir::duc_shape(c->T, c->L).tap_entries);
    if_fir::duc_mix_taps(c->h_taps.data(), c->T, c->ctaps, word, g.data());
    if_fir::duc_build_table(g.data(), c->T, c->L, table.data());
    return table;
}

static uint8_t duc_init(if_fir_duc_t **ppCtx, const float *pfTaps, uint32_t ulTaps, uint32_t ulL, uint64_t ullMax, int32_t lDevice,
                        int ctaps)
{
    if (!ppCtx)
    {
        set_err(g_duc_init_err, "if_fir_duc_init: ppCtx is NULL");
        return 0;
    }
    *ppCtx = nullptr;
    if (!pfTaps || ulTaps == 0 || ulTaps > IF_FIR_MAX_TAPS)
    {
        set_err(g_duc_init_err, "if_fir_duc_init: taps must be 1..%u (got %u)%s", IF_FIR_MAX_TAPS, ulTaps, pfTaps ? "" : ", pfTaps is NULL");
        return 0;
    }
    if (ulL < 1 || ulL > IF_FIR_MAX_INTERPOLATION)
    {
        set_err(g_duc_init_err, "if_fir_duc_init: interpolation must be 1..%u (got %u)", IF_FIR_MAX_INTERPOLATION, ulL);
        return 0;
    }
    for (size_t i = 0; i < (size_t)ulTaps * (ctaps ? 2 : 1); i++)
        if (!std::isfinite(pfTaps[i]))
        {
            set_err(g_duc_init_err, "if_fir_duc_init: tap %zu is not finite", i / (ctaps ? 2 : 1));
            return 0;
        }
    if (ullMax == 0 || ullMax > ((uint64_t)1 << 40))
    {
        set_err(g_duc_init_err, "if_fir_duc_init: ullMaxSamples must be 1..2^40 (got %llu)", (unsigned long long)ullMax);
        return 0;
    }
    if (!if_fir::stream_ctx_device_ok(g_duc_init_err, "if_fir_duc_init", lDevice))
        return 0;
    if_fir_duc *c = new (std::nothrow) if_fir_duc();
    if (!c)
    {
        set_err(g_duc_init_err, "if_fir_duc_init: out of host memory");
        return 0;
    }
    c->T = (int)ulTaps;
    c->L = (int)ulL;
    c->ctaps = ctaps;
    c->h_taps.assign(pfTaps, pfTaps + (size_t)ulTaps * (ctaps ? 2 : 1));
    c->hist_len = if_fir::duc_phase_taps(c->T, c->L) - 1;
    const std::vector<float> table = build_table(c, 0);
    const size_t hist_bytes = (size_t)(c->hist_len > 0 ? c->hist_len : 1) * sizeof(float2);
    hipError_t e = if_fir::stream_ctx_open(c, lDevice, ullMax);
    if_fir::stream_ctx_alloc_upload(e, &c->d_taps, table.data(), table.size() * sizeof(float));
    for (int i = 0; i < 2; i++)
        if_fir::stream_ctx_alloc_zeroed(e, &c->d_hist[i], hist_bytes);
    if (e == hipSuccess)
        e = hipMalloc(&c->d_stage_in, (size_t)ullMax * 8);
    if (e == hipSuccess)
        e = hipMalloc(&c->d_stage_out, (size_t)ullMax * ulL * 4);
    if (e != hipSuccess)
    {
        set_err(g_duc_init_err, "if_fir_duc_init: %s", hipGetErrorString(e));
        (void)hipGetLastError();
        free_ctx(c);
        return 0;
    }
    *ppCtx = c;
    return 1;
}

IF_FIR_API uint8_t if_fir_duc_init(if_fir_duc_t **ppCtx, const float *pfTaps, uint32_t ulTaps, uint32_t ulInterpolation,
                                   uint64_t ullMaxSamples, int32_t lDevice)
{
    return duc_init(ppCtx, pfTaps, ulTaps, ulInterpolation, ullMaxSamples, lDevice, 0);
}

IF_FIR_API uint8_t if_fir_duc_init_complex(if_fir_duc_t **ppCtx, const float *pfTapsIQ, uint32_t ulTaps, uint32_t ulInterpolation,
                                           uint64_t ullMaxSamples, int32_t lDevice)
{
    return duc_init(ppCtx, pfTapsIQ, ulTaps, ulInterpolation, ullMaxSamples, lDevice, 1);
}

IF_FIR_API void if_fir_duc_destroy(if_fir_duc_t *pCtx)
{
    free_ctx(pCtx);
}

IF_FIR_API const char *if_fir_duc_last_error(const if_fir_duc_t *pCtx)
{
    return pCtx ? pCtx->err : g_duc_init_err;
}

// zero both history buffers on the context's stream and wait
static uint8_t zero_history(if_fir_duc *c)
{
    HIP_TRY(c, hipSetDevice(c->device));
    for (int i = 0; i < 2 && c->hist_len > 0; i++)
        HIP_TRY(c, hipMemsetAsync(c->d_hist[i], 0, (size_t)c->hist_len * sizeof(float2), c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return 1;
}

IF_FIR_API uint8_t if_fir_duc_reset(if_fir_duc_t *pCtx)
{
    if (!pCtx || !zero_history(pCtx))
        return 0;
    pCtx->st.consumed = 0;
    return 1;
}

IF_FIR_API uint8_t if_fir_duc_set_input_format(if_fir_duc_t *pCtx, uint32_t ulFormat)
{
    return if_fir::stream_ctx_set_input_format(pCtx, "if_fir_duc_set_input_format", ulFormat);
}

// (the result is float32 whatever the format, and the streaming state holds inputs only: a change keeps the stream)
IF_FIR_API uint8_t if_fir_duc_set_output_format(if_fir_duc_t *pCtx, uint32_t ulFormat)
{
    if (!pCtx)
        return 0;
    if (ulFormat > IF_FIR_OUTPUT_I16)
    {
        set_err(pCtx->err, "if_fir_duc_set_output_format: unknown format %u", ulFormat);
        return 0;
    }
    pCtx->out_i16 = (int)ulFormat;
    return 1;
}

// SPEC §11: the new frequency holds from the next call as if set since the last reset.  Waits for the context's stream: kernels
// in flight still read the old table.
IF_FIR_API uint8_t if_fir_duc_set_nco(if_fir_duc_t *pCtx, double dFreq)
{
    if (!pCtx)
        return 0;
    if (!std::isfinite(dFreq) || std::fabs(dFreq) > 0.5)
    {
        set_err(pCtx->err, "if_fir_duc_set_nco: frequency must be within +-0.5 cycles/sample (got %g)", dFreq);
        return 0;
    }
    const uint32_t word = (uint32_t)(int64_t)std::llround(dFreq * 4294967296.0); // mod 2^32, as if_fir_set_nco
    if (word == pCtx->nco_word)
        return 1;
    const std::vector<float> table = build_table(pCtx, word);
    HIP_TRY(pCtx, hipSetDevice(pCtx->device));
    HIP_TRY(pCtx, hipStreamSynchronize(pCtx->stream));
    HIP_TRY(pCtx, hipMemcpy(pCtx->d_taps, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice));
    pCtx->nco_word = word;
    return 1;
}

IF_FIR_API uint8_t if_fir_duc_get_nco(const if_fir_duc_t *pCtx, double *pdFreq)
{
    if (!pCtx || !pdFreq)
        return 0;
    *pdFreq = (double)(int32_t)pCtx->nco_word / 4294967296.0; // the quantised frequency actually applied
    return 1;
}

IF_FIR_API uint8_t if_fir_duc_set_stream(if_fir_duc_t *pCtx, void *pStream)
{
    return if_fir::stream_ctx_set_stream(pCtx, pStream);
}

IF_FIR_API uint8_t if_fir_duc_synchronize(if_fir_duc_t *pCtx)
{
    return if_fir::stream_ctx_synchronize(pCtx);
}

IF_FIR_API uint64_t if_fir_duc_out_count(const if_fir_duc_t *pCtx, uint64_t ullSamples)
{
    uint64_t count;
    if (!pCtx || !if_fir::duc_call(pCtx->st.consumed, ullSamples, pCtx->L, &count))
        return 0;
    return count;
}

static uint8_t run_device(if_fir_duc *c, const void *in, void *out, uint64_t n, uint64_t *pout, const char *who)
{
    uint64_t count;
    if (n > ((uint64_t)1 << 40))
    {
        set_err(c->err, "%s: sample count too large", who);
        return 0;
    }
    if (!if_fir::duc_call(c->st.consumed, n, c->L, &count))
    {
        set_err(c->err, "%s: the stream position would pass 2^64 outputs", who);
        return 0;
    }
    const uintptr_t in_mask = c->in_i16 ? 3 : 7, out_mask = c->out_i16 ? 1 : 3;
    if (((uintptr_t)in & in_mask) || ((uintptr_t)out & out_mask))
    {
        set_err(c->err, "%s: device pointers must be aligned to one element: %u-byte (input) and %u-byte (output)", who,
                (unsigned)in_mask + 1, (unsigned)out_mask + 1);
        return 0;
    }
    if (n && (!in || !out))
    {
        set_err(c->err, "%s: NULL device pointer", who);
        return 0;
    }
    if (if_fir::stream_ctx_capturing(c, who))
        return 0;
    if (n == 0)
    {
        if (pout)
            *pout = 0;
        return 1;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    if_fir::DucArgs a{};
    a.in = in;
    a.out = out;
    a.hist = c->d_hist[c->st.hist_cur];
    a.hist_out = c->d_hist[c->st.hist_cur ^ 1];
    a.taps = c->d_taps;
    a.T = c->T;
    a.L = c->L;
    a.in_i16 = c->in_i16;
    a.out_i16 = c->out_i16;
    a.N = (int64_t)n;
    a.nco_word = c->nco_word;
    a.nco_abs0 = (uint32_t)c->st.consumed;
    a.grid_limit = c->grid_limit;
    a.device = c->device;
    a.stream = c->stream;
    HIP_TRY(c, if_fir::launch_duc(a));
    c->st.consumed += n;
    c->st.hist_cur ^= 1;
    if (pout)
        *pout = count;
    return 1;
}

IF_FIR_API uint8_t if_fir_duc_process_device(if_fir_duc_t *pCtx, const void *pDevIn, void *pDevOut, uint64_t ullSamples,
                                             uint64_t *pullOutSamples)
{
    if (!pCtx)
        return 0;
    return run_device(pCtx, pDevIn, pDevOut, ullSamples, pullOutSamples, "if_fir_duc_process_device");
}

IF_FIR_API uint8_t if_fir_duc_process(if_fir_duc_t *pCtx, const void *pIQIn, void *pOut, uint64_t ullSamples, uint64_t *pullOutSamples)
{
    if (!pCtx)
        return 0;
    if (!if_fir::stream_ctx_fits(pCtx, "if_fir_duc_process", ullSamples))
        return 0;
    if (ullSamples && (!pIQIn || !pOut))
    {
        set_err(pCtx->err, "if_fir_duc_process: NULL buffer");
        return 0;
    }
    if (pullOutSamples)
        *pullOutSamples = 0;
    if (ullSamples == 0)
        return 1;
    uint64_t m = 0;
    const size_t out_bytes = pCtx->out_i16 ? 2 : 4;
    if (!if_fir::stream_ctx_staged(
            pCtx, "if_fir_duc_process", "outputs", pCtx->d_stage_in, pIQIn, ullSamples, &pCtx->st,
            [&] { return run_device(pCtx, pCtx->d_stage_in, pCtx->d_stage_out, ullSamples, &m, "if_fir_duc_process"); },
            [&] { return m ? hipMemcpyAsync(pOut, pCtx->d_stage_out, (size_t)m * out_bytes, hipMemcpyDeviceToHost, pCtx->stream) : hipSuccess; }))
        return 0;
    if (pullOutSamples)
        *pullOutSamples = m;
    return 1;
}

#ifdef IF_FIR_DEVELOPMENT
IF_FIR_API uint8_t if_fir_debug_duc_config(if_fir_duc_t *pCtx, uint32_t ulGridLimit, uint32_t *pulTileInputs, uint64_t ullPosition)
{
    if (!pCtx)
        return 0;
    if (ullPosition != UINT64_MAX)
    {
        if (!zero_history(pCtx))
            return 0;
        pCtx->st.consumed = ullPosition;
    }
    pCtx->grid_limit = (int)(ulGridLimit > 65536u ? 65536u : ulGridLimit);
    if (pulTileInputs)
        *pulTileInputs = (uint32_t)if_fir::duc_shape(pCtx->T, pCtx->L).Q;
    return 1;
}
#endif
