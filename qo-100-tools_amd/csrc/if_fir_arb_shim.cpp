// if_fir_arb_shim.cpp — the C ABI of the arbitrary-ratio resampler (include/if_fir.h, if_fir_arb_*; docs/SPEC.md §12).  Its own
// opaque context beside the other streaming families'.  Same conventions: 1/0 status, a message per context, no CPU fallback.
// This file is the only place that holds the stream position c and the output time tau; the kernel gets their difference.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <vector>

#include "if_fir.h"
#ifdef IF_FIR_DEVELOPMENT
#include "if_fir_debug.h"
#endif
#include "if_fir_arb.h"
#include "if_fir_stream_ctx.h"

#define IF_FIR_API extern "C" __attribute__((visibility("default")))

// the streaming state: what a call advances (and a failed if_fir_arb_process puts back)
struct arb_state
{
    int hist_cur;
    uint64_t consumed;        // c: absolute index of the next input
    if_fir::arb_u128 tau;     // time of the next output in 2^-32 input samples (96 bits used)
};

struct if_fir_arb : if_fir::StreamCtx
{
    int T, bits;
    uint64_t step;            // R; set_step changes nothing else
    float *d_taps;            // the pair table (arb_build_taps)
    if_fir::StreamHistory hist; // the last K - 1 input samples, float32
    arb_state st;
    void *d_stage_in, *d_stage_out; // if_fir_arb_process
    uint64_t stage_out_cap;   // samples d_stage_out holds: sized for the step of init, grown when a smaller step needs more
    int grid_limit;           // development hook
};

using if_fir::set_err;
static thread_local char g_arb_init_err[256] = "";

static void free_ctx(if_fir_arb *c)
{
    if (!c)
        return;
    if_fir::stream_ctx_close(c, {c->d_taps, c->hist.buf[0], c->hist.buf[1], c->d_stage_in, c->d_stage_out});
    delete c;
}

// the most outputs a call of n inputs can emit at this step, whatever the stream position
static uint64_t max_out(uint64_t n, uint64_t step)
{
    return (uint64_t)((((if_fir::arb_u128)n << 32) + step - 1) / step) + 1;
}

static bool step_ok(uint64_t step)
{
    return step >= if_fir::ARB_MIN_STEP && step <= if_fir::ARB_MAX_STEP;
}

IF_FIR_API uint64_t if_fir_arb_step_from_rates(double dRateIn, double dRateOut)
{
    return if_fir::arb_step_from_rates(dRateIn, dRateOut);
}

IF_FIR_API uint8_t if_fir_arb_init(if_fir_arb_t **ppCtx, const float *pfTaps, uint32_t ulTaps, uint32_t ulPhaseBits, uint64_t ullStep,
                                   uint64_t ullMaxSamples, int32_t lDevice)
{
    if (!if_fir::stream_ctx_init_begin(g_arb_init_err, "if_fir_arb_init", ppCtx))
        return 0;
    if (!pfTaps || ulTaps == 0 || ulTaps > IF_FIR_ARB_MAX_TAPS)
    {
        set_err(g_arb_init_err, "if_fir_arb_init: taps must be 1..%u (got %u)%s", IF_FIR_ARB_MAX_TAPS, ulTaps, pfTaps ? "" : ", pfTaps is NULL");
        return 0;
    }
    if (ulPhaseBits < IF_FIR_ARB_MIN_PHASE_BITS || ulPhaseBits > IF_FIR_ARB_MAX_PHASE_BITS)
    {
        set_err(g_arb_init_err, "if_fir_arb_init: phase bits must be %u..%u (got %u)", IF_FIR_ARB_MIN_PHASE_BITS, IF_FIR_ARB_MAX_PHASE_BITS,
                ulPhaseBits);
        return 0;
    }
    if (!step_ok(ullStep))
    {
        set_err(g_arb_init_err, "if_fir_arb_init: step must be 2^26..2^34 (got %llu)", (unsigned long long)ullStep);
        return 0;
    }
    if (ullMaxSamples == 0 || ullMaxSamples > ((uint64_t)1 << 30))
    {
        set_err(g_arb_init_err, "if_fir_arb_init: ullMaxSamples must be 1..2^30 (got %llu)", (unsigned long long)ullMaxSamples);
        return 0;
    }
    if_fir_arb *c = if_fir::stream_ctx_new<if_fir_arb>(g_arb_init_err, "if_fir_arb_init", lDevice);
    if (!c)
        return 0;
    c->T = (int)ulTaps;
    c->bits = (int)ulPhaseBits;
    c->step = ullStep;
    const if_fir::ArbShape shape = if_fir::arb_shape(c->T, c->bits, c->step);
    std::vector<float> table((size_t)shape.tap_entries * 2);
    if_fir::arb_build_taps(pfTaps, c->T, c->bits, table.data());
    hipError_t e = if_fir::stream_ctx_open(c, lDevice, ullMaxSamples);
    if_fir::stream_ctx_alloc_upload(e, &c->d_taps, table.data(), table.size() * sizeof(float));
    if_fir::stream_history_alloc(e, &c->hist, (size_t)(shape.K - 1) * sizeof(float2), sizeof(float2));
    if (e == hipSuccess)
        e = hipMalloc(&c->d_stage_in, (size_t)ullMaxSamples * 8);
    c->stage_out_cap = max_out(ullMaxSamples, ullStep);
    if (e == hipSuccess)
        e = hipMalloc(&c->d_stage_out, (size_t)c->stage_out_cap * 8);
    return if_fir::stream_ctx_init_end(g_arb_init_err, "if_fir_arb_init", e, c, ppCtx, free_ctx);
}

IF_FIR_API void if_fir_arb_destroy(if_fir_arb_t *pCtx)
{
    free_ctx(pCtx);
}

IF_FIR_API const char *if_fir_arb_last_error(const if_fir_arb_t *pCtx)
{
    return pCtx ? pCtx->err : g_arb_init_err;
}

IF_FIR_API uint8_t if_fir_arb_reset(if_fir_arb_t *pCtx)
{
    if (!pCtx || !if_fir::stream_history_zero(pCtx, pCtx->hist))
        return 0;
    pCtx->st.consumed = 0;
    pCtx->st.tau = 0;
    return 1;
}

IF_FIR_API uint8_t if_fir_arb_set_step(if_fir_arb_t *pCtx, uint64_t ullStep)
{
    if (!pCtx)
        return 0;
    if (!step_ok(ullStep))
    {
        set_err(pCtx->err, "if_fir_arb_set_step: step must be 2^26..2^34 (got %llu)", (unsigned long long)ullStep);
        return 0;
    }
    pCtx->step = ullStep; // c, tau and the history stay: the next output is where it was, the one after it ullStep later
    return 1;
}

IF_FIR_API uint8_t if_fir_arb_set_input_format(if_fir_arb_t *pCtx, uint32_t ulFormat)
{
    return if_fir::stream_ctx_set_input_format(pCtx, "if_fir_arb_set_input_format", ulFormat);
}

IF_FIR_API uint8_t if_fir_arb_set_stream(if_fir_arb_t *pCtx, void *pStream)
{
    return if_fir::stream_ctx_set_stream(pCtx, pStream);
}

IF_FIR_API uint8_t if_fir_arb_synchronize(if_fir_arb_t *pCtx)
{
    return if_fir::stream_ctx_synchronize(pCtx);
}

IF_FIR_API uint64_t if_fir_arb_out_count(const if_fir_arb_t *pCtx, uint64_t ullSamples)
{
    uint64_t count = 0;
    if (!pCtx || !if_fir::arb_out_count(pCtx->st.consumed, pCtx->st.tau, ullSamples, pCtx->step, &count))
        return 0;
    return count;
}

static uint8_t run_device(if_fir_arb *c, const void *in, void *out, uint64_t n, uint64_t *pout, const char *who)
{
    uint64_t count = 0;
    if (n > if_fir::ARB_MAX_SAMPLES || !if_fir::arb_out_count(c->st.consumed, c->st.tau, n, c->step, &count))
    {
        set_err(c->err, "%s: sample count too large", who);
        return 0;
    }
    if (!if_fir::stream_ctx_aligned(c, who, "sample", in, c->in_i16 ? 3 : 7, out, 7) ||
        !if_fir::stream_ctx_device_ptrs(c, who, n, in, count, out))
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
    if_fir::ArbArgs a{};
    a.in = in;
    a.out = out;
    a.hist = c->hist.at<float2>(c->st.hist_cur);
    a.hist_out = c->hist.at<float2>(c->st.hist_cur ^ 1);
    a.taps = c->d_taps;
    a.T = c->T;
    a.bits = c->bits;
    a.in_i16 = c->in_i16;
    a.step = c->step;
    a.tau_rel = (uint64_t)(c->st.tau - ((if_fir::arb_u128)c->st.consumed << 32)); // < 2^34 (arb_state_ok)
    a.N = (int64_t)n;
    a.count = (int64_t)count;
    a.grid_limit = c->grid_limit;
    a.device = c->device;
    a.stream = c->stream;
    HIP_TRY(c, if_fir::launch_arb(a));
    c->st.consumed += n;
    c->st.tau += (if_fir::arb_u128)count * c->step;
    c->st.hist_cur ^= 1;
    if (pout)
        *pout = count;
    return 1;
}

IF_FIR_API uint8_t if_fir_arb_process_device(if_fir_arb_t *pCtx, const void *pDevIn, void *pDevOut, uint64_t ullSamples,
                                             uint64_t *pullOutSamples)
{
    if (!pCtx)
        return 0;
    return run_device(pCtx, pDevIn, pDevOut, ullSamples, pullOutSamples, "if_fir_arb_process_device");
}

IF_FIR_API uint8_t if_fir_arb_process(if_fir_arb_t *pCtx, const void *pIQIn, float *pfIQOut, uint64_t ullSamples, uint64_t *pullOutSamples)
{
    if (!pCtx)
        return 0;
    if (!if_fir::stream_ctx_fits(pCtx, "if_fir_arb_process", ullSamples))
        return 0;
    const uint64_t want = if_fir_arb_out_count(pCtx, ullSamples);
    if (!if_fir::stream_ctx_host_ptrs(pCtx, "if_fir_arb_process", ullSamples, pIQIn, want, pfIQOut))
        return 0;
    if (pullOutSamples)
        *pullOutSamples = 0;
    if (ullSamples == 0)
        return 1;
    if (want > pCtx->stage_out_cap)
    {
        // a retune to a smaller step since init: the staging buffer grows to what ullMaxSamples can emit at this step
        const uint64_t cap = max_out(pCtx->max_samples, pCtx->step);
        void *grown = nullptr;
        HIP_TRY(pCtx, hipSetDevice(pCtx->device));
        HIP_TRY(pCtx, hipStreamSynchronize(pCtx->stream));
        HIP_TRY(pCtx, hipMalloc(&grown, (size_t)cap * 8));
        (void)hipFree(pCtx->d_stage_out);
        pCtx->d_stage_out = grown;
        pCtx->stage_out_cap = cap;
    }
    uint64_t m = 0;
    if (!if_fir::stream_ctx_staged(
            pCtx, "if_fir_arb_process", "outputs", pCtx->d_stage_in, pIQIn, ullSamples, &pCtx->st,
            [&] { return run_device(pCtx, pCtx->d_stage_in, pCtx->d_stage_out, ullSamples, &m, "if_fir_arb_process"); },
            [&] { return m ? hipMemcpyAsync(pfIQOut, pCtx->d_stage_out, (size_t)m * 8, hipMemcpyDeviceToHost, pCtx->stream) : hipSuccess; }))
        return 0;
    if (pullOutSamples)
        *pullOutSamples = m;
    return 1;
}

#ifdef IF_FIR_DEVELOPMENT
IF_FIR_API uint8_t if_fir_debug_arb_config(if_fir_arb_t *pCtx, uint32_t ulGridLimit, uint32_t *pulTileOutputs, uint64_t ullPosition,
                                           uint64_t ullTimeOffset)
{
    if (!pCtx)
        return 0;
    if (ullTimeOffset >= ((uint64_t)1 << 34))
    {
        set_err(pCtx->err, "if_fir_debug_arb_config: ullTimeOffset must be below 2^34 (got %llu)", (unsigned long long)ullTimeOffset);
        return 0;
    }
    pCtx->grid_limit = if_fir::stream_ctx_grid_limit(ulGridLimit);
    if (pulTileOutputs)
        *pulTileOutputs = (uint32_t)if_fir::arb_shape(pCtx->T, pCtx->bits, pCtx->step).tile_out;
    if (ullPosition != UINT64_MAX)
    {
        pCtx->st.consumed = ullPosition;
        pCtx->st.tau = ((if_fir::arb_u128)ullPosition << 32) + ullTimeOffset;
    }
    return 1;
}
#endif
