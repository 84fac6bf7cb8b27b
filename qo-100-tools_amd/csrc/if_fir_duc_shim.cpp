// if_fir_duc_shim.cpp — the C ABI of the real-output up-converter (include/if_fir.h, if_fir_duc_*; docs/SPEC.md §11).  Its own
// opaque context beside the other streaming families.  Same conventions: 1/0 status, a message per context, no CPU fallback.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
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
    if_fir::StreamHistory hist; // the last K - 1 input samples, unrotated float32 I/Q
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
    if_fir::stream_ctx_close(c, {c->d_taps, c->hist.buf[0], c->hist.buf[1], c->d_stage_in, c->d_stage_out});
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
    if (!if_fir::stream_ctx_init_begin(g_duc_init_err, "if_fir_duc_init", ppCtx))
        return 0;
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
    if_fir_duc *c = if_fir::stream_ctx_new<if_fir_duc>(g_duc_init_err, "if_fir_duc_init", lDevice);
    if (!c)
        return 0;
    c->T = (int)ulTaps;
    c->L = (int)ulL;
    c->ctaps = ctaps;
    c->h_taps.assign(pfTaps, pfTaps + (size_t)ulTaps * (ctaps ? 2 : 1));
    const std::vector<float> table = build_table(c, 0);
    hipError_t e = if_fir::stream_ctx_open(c, lDevice, ullMax);
    if_fir::stream_ctx_alloc_upload(e, &c->d_taps, table.data(), table.size() * sizeof(float));
    if_fir::stream_history_alloc(e, &c->hist, (size_t)(if_fir::duc_phase_taps(c->T, c->L) - 1) * sizeof(float2), sizeof(float2));
    if (e == hipSuccess)
        e = hipMalloc(&c->d_stage_in, (size_t)ullMax * 8);
    if (e == hipSuccess)
        e = hipMalloc(&c->d_stage_out, (size_t)ullMax * ulL * 4);
    return if_fir::stream_ctx_init_end(g_duc_init_err, "if_fir_duc_init", e, c, ppCtx, free_ctx);
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

IF_FIR_API uint8_t if_fir_duc_reset(if_fir_duc_t *pCtx)
{
    if (!pCtx || !if_fir::stream_history_zero(pCtx, pCtx->hist))
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
    uint32_t word;
    if (!if_fir::stream_ctx_nco_word(pCtx, "if_fir_duc_set_nco", dFreq, &word))
        return 0;
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
    *pdFreq = if_fir::nco_freq_of(pCtx->nco_word); // the quantised frequency actually applied
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
    if (!if_fir::stream_ctx_aligned(c, who, "element", in, c->in_i16 ? 3 : 7, out, c->out_i16 ? 1 : 3) ||
        !if_fir::stream_ctx_device_ptrs(c, who, n, in, n, out))
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
    if_fir::DucArgs a{};
    a.in = in;
    a.out = out;
    a.hist = c->hist.at<float2>(c->st.hist_cur);
    a.hist_out = c->hist.at<float2>(c->st.hist_cur ^ 1);
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
    if (!if_fir::stream_ctx_host_ptrs(pCtx, "if_fir_duc_process", ullSamples, pIQIn, ullSamples, pOut))
        return 0;
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
        if (!if_fir::stream_history_zero(pCtx, pCtx->hist))
            return 0;
        pCtx->st.consumed = ullPosition;
    }
    pCtx->grid_limit = if_fir::stream_ctx_grid_limit(ulGridLimit);
    if (pulTileInputs)
        *pulTileInputs = (uint32_t)if_fir::duc_shape(pCtx->T, pCtx->L).Q;
    return 1;
}
#endif
