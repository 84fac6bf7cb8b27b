// if_fir_fpow_shim.cpp — the C ABI of the frame power stage (include/if_fir.h, if_fir_fpow_*; docs/SPEC.md §19).  Its own opaque
// context beside the other streaming families.  Same conventions: 1/0 status, a message per context, no CPU fallback.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>

#include "if_fir.h"
#ifdef IF_FIR_DEVELOPMENT
#include "if_fir_debug.h"
#endif
#include "if_fir_fpow.h"
#include "if_fir_stream_ctx.h"

#define IF_FIR_API extern "C" __attribute__((visibility("default")))

// the streaming state: what a call advances (and a failed if_fir_fpow_process puts back)
struct fpow_state
{
    int cur;                  // which of d_state the next call reads
    uint64_t position;        // input frames since init/reset
};

struct if_fir_fpow : if_fir::StreamCtx
{
    int B, first, G, Bo, K;
    float scale;              // 1 / (K G fNorm), rounded once
    double ref_power;
    float *d_state[2];        // 2 Bo each: the open frame's accumulator, the open chunk's partial sum; ping-pong
    float *d_work;            // chunk sums of one call
    fpow_state st;
    void *d_stage_in;         // if_fir_fpow_process: staging, allocated by its first call (device-pointer users never pay for it)
    uint16_t *d_stage_codes;
    float *d_stage_power;
    int grid_limit;           // development hook
};

using if_fir::set_err;
static thread_local char g_fpow_init_err[256] = "";

static void free_ctx(if_fir_fpow *c)
{
    if (!c)
        return;
    if_fir::stream_ctx_close(c, {c->d_state[0], c->d_state[1], c->d_work, c->d_stage_in, c->d_stage_codes, c->d_stage_power});
    delete c;
}

IF_FIR_API uint8_t if_fir_fpow_init(if_fir_fpow_t **ppCtx, const if_fir_fpow_config_t *pCfg, uint64_t ullMaxFrames, int32_t lDevice)
{
    if (!if_fir::stream_ctx_init_begin(g_fpow_init_err, "if_fir_fpow_init", ppCtx))
        return 0;
    if (!pCfg)
    {
        set_err(g_fpow_init_err, "if_fir_fpow_init: pCfg is NULL");
        return 0;
    }
    char why[256];
    if (!if_fir::fpow_config_ok(pCfg->ulBins, pCfg->ulFirst, pCfg->ulGroup, pCfg->ulOutBins, pCfg->ulFrames,
                                pCfg->fNorm > 0.0f && std::isfinite(pCfg->fNorm), pCfg->fRefPower > 0.0f && std::isfinite(pCfg->fRefPower),
                                pCfg->ulInputFormat, ullMaxFrames, why))
    {
        set_err(g_fpow_init_err, "if_fir_fpow_init: %s", why);
        return 0;
    }
    if_fir_fpow *c = if_fir::stream_ctx_new<if_fir_fpow>(g_fpow_init_err, "if_fir_fpow_init", lDevice);
    if (!c)
        return 0;
    c->B = (int)pCfg->ulBins;
    c->first = (int)pCfg->ulFirst;
    c->G = (int)pCfg->ulGroup;
    c->Bo = (int)pCfg->ulOutBins;
    c->K = (int)pCfg->ulFrames;
    c->in_i16 = (int)pCfg->ulInputFormat;
    c->ref_power = (double)pCfg->fRefPower;
    c->scale = if_fir::fpow_scale(pCfg->ulFrames, pCfg->ulGroup, pCfg->fNorm);
    hipError_t e = if_fir::stream_ctx_open(c, lDevice, ullMaxFrames);
    for (int i = 0; i < 2; i++)
        if_fir::stream_ctx_alloc_zeroed(e, &c->d_state[i], 2 * (size_t)c->Bo * sizeof(float));
    if (e == hipSuccess)
        e = hipMalloc(&c->d_work, (size_t)if_fir::fpow_max_chunks(ullMaxFrames, pCfg->ulFrames) * (size_t)c->Bo * sizeof(float));
    return if_fir::stream_ctx_init_end(g_fpow_init_err, "if_fir_fpow_init", e, c, ppCtx, free_ctx);
}

IF_FIR_API void if_fir_fpow_destroy(if_fir_fpow_t *pCtx)
{
    free_ctx(pCtx);
}

IF_FIR_API const char *if_fir_fpow_last_error(const if_fir_fpow_t *pCtx)
{
    return pCtx ? pCtx->err : g_fpow_init_err;
}

IF_FIR_API uint8_t if_fir_fpow_reset(if_fir_fpow_t *pCtx)
{
    if (!pCtx)
        return 0;
    HIP_TRY(pCtx, hipSetDevice(pCtx->device));
    HIP_TRY(pCtx, hipStreamSynchronize(pCtx->stream));
    // (no buffer needs zeroing: nothing is read of the accumulator or the partial sum beyond what the position says is there)
    pCtx->st.position = 0;
    return 1;
}

IF_FIR_API uint8_t if_fir_fpow_set_input_format(if_fir_fpow_t *pCtx, uint32_t ulFormat)
{
    return if_fir::stream_ctx_set_input_format(pCtx, "if_fir_fpow_set_input_format", ulFormat);
}

IF_FIR_API uint8_t if_fir_fpow_set_stream(if_fir_fpow_t *pCtx, void *pStream)
{
    return if_fir::stream_ctx_set_stream(pCtx, pStream);
}

IF_FIR_API uint8_t if_fir_fpow_synchronize(if_fir_fpow_t *pCtx)
{
    return if_fir::stream_ctx_synchronize(pCtx);
}

IF_FIR_API uint64_t if_fir_fpow_frame_count(const if_fir_fpow_t *pCtx, uint64_t ullFrames)
{
    if_fir::FpowPlan plan;
    if (!pCtx || !if_fir::fpow_plan(pCtx->st.position, ullFrames, (uint32_t)pCtx->K, &plan))
        return 0;
    return plan.frames;
}

// the checks of a call that need no device: the frame count against init's and the stream position against 2^64
static bool plan_call(if_fir_fpow *c, const char *who, uint64_t frames, if_fir::FpowPlan *plan)
{
    if (frames > c->max_samples)
    {
        set_err(c->err, "%s: %llu frames exceed ullMaxFrames %llu of init", who, (unsigned long long)frames, (unsigned long long)c->max_samples);
        return false;
    }
    if (!if_fir::fpow_plan(c->st.position, frames, (uint32_t)c->K, plan))
    {
        set_err(c->err, "%s: frame count too large: the stream position would pass 2^64", who);
        return false;
    }
    return true;
}

static uint8_t run_device(if_fir_fpow *c, const void *in, uint16_t *codes, float *power, uint64_t frames, uint32_t *pframes, const char *who)
{
    if_fir::FpowPlan plan;
    if (!plan_call(c, who, frames, &plan))
        return 0;
    const uintptr_t in_mask = c->in_i16 ? 3 : 7;
    if (((uintptr_t)in & in_mask) || ((uintptr_t)codes & 1) || ((uintptr_t)power & 3))
    {
        set_err(c->err, "%s: device pointers must be aligned to one element: %u-byte (input), 2-byte (codes), 4-byte (power)", who,
                (unsigned)in_mask + 1);
        return 0;
    }
    if (!if_fir::stream_ctx_device_ptrs(c, who, frames, in, plan.frames, codes))
        return 0;
    if (if_fir::stream_ctx_capturing(c, who))
        return 0;
    if (pframes)
        *pframes = 0;
    if (frames == 0)
        return 1;
    HIP_TRY(c, hipSetDevice(c->device));
    if_fir::FpowArgs a{};
    a.in = in;
    a.work = c->d_work;
    a.state = c->d_state[c->st.cur];
    a.state_out = c->d_state[c->st.cur ^ 1];
    a.codes = codes;
    a.power = power;
    a.B = c->B;
    a.first = c->first;
    a.G = c->G;
    a.Bo = c->Bo;
    a.K = c->K;
    a.in_i16 = c->in_i16;
    a.F = (int64_t)frames;
    a.plan = plan;
    a.scale = c->scale;
    a.ref_power = c->ref_power;
    a.grid_limit = c->grid_limit;
    a.device = c->device;
    a.stream = c->stream;
    HIP_TRY(c, if_fir::launch_fpow(a));
    c->st.position += frames;
    c->st.cur ^= 1;
    if (pframes)
        *pframes = (uint32_t)plan.frames;
    return 1;
}

IF_FIR_API uint8_t if_fir_fpow_process_device(if_fir_fpow_t *pCtx, const void *pDevIn, uint64_t ullFrames, uint16_t *pusDevBins,
                                              float *pfDevPower, uint32_t *pulOutFrames)
{
    if (!pCtx)
        return 0;
    return run_device(pCtx, pDevIn, pusDevBins, pfDevPower, ullFrames, pulOutFrames, "if_fir_fpow_process_device");
}

IF_FIR_API uint8_t if_fir_fpow_process(if_fir_fpow_t *pCtx, const void *pFramesIn, uint64_t ullFrames, uint16_t *pusBins, float *pfPower,
                                       uint32_t *pulOutFrames)
{
    if (!pCtx)
        return 0;
    if_fir::FpowPlan plan;
    if (!plan_call(pCtx, "if_fir_fpow_process", ullFrames, &plan))
        return 0;
    if (!if_fir::stream_ctx_host_ptrs(pCtx, "if_fir_fpow_process", ullFrames, pFramesIn, plan.frames, pusBins))
        return 0;
    if (pulOutFrames)
        *pulOutFrames = 0;
    if (ullFrames == 0)
        return 1;
    // the most output frames of a call of ullMaxFrames frames, whatever the position
    const size_t values = (size_t)(pCtx->max_samples / (uint64_t)pCtx->K + 1) * (size_t)pCtx->Bo;
    if (!pCtx->d_stage_in &&
        !if_fir::stream_ctx_alloc_staging(pCtx, "if_fir_fpow_process",
                                          {{(void **)&pCtx->d_stage_codes, values * sizeof(uint16_t)},
                                           {(void **)&pCtx->d_stage_power, values * sizeof(float)},
                                           {&pCtx->d_stage_in, (size_t)pCtx->max_samples * (size_t)pCtx->B * 8}}))
        return 0;
    uint32_t m = 0;
    if (!if_fir::stream_ctx_staged_bytes(
            pCtx, "if_fir_fpow_process", "frames", pCtx->d_stage_in, pFramesIn, (size_t)ullFrames * (size_t)pCtx->B * (pCtx->in_i16 ? 4 : 8),
            &pCtx->st,
            [&] {
                return run_device(pCtx, pCtx->d_stage_in, pCtx->d_stage_codes, pfPower ? pCtx->d_stage_power : nullptr, ullFrames, &m,
                                  "if_fir_fpow_process");
            },
            [&] {
                const size_t got = (size_t)m * (size_t)pCtx->Bo;
                hipError_t e = m ? hipMemcpyAsync(pusBins, pCtx->d_stage_codes, got * sizeof(uint16_t), hipMemcpyDeviceToHost, pCtx->stream) : hipSuccess;
                if (e == hipSuccess && m && pfPower)
                    e = hipMemcpyAsync(pfPower, pCtx->d_stage_power, got * sizeof(float), hipMemcpyDeviceToHost, pCtx->stream);
                return e;
            }))
        return 0;
    if (pulOutFrames)
        *pulOutFrames = m;
    return 1;
}

#ifdef IF_FIR_DEVELOPMENT
IF_FIR_API uint8_t if_fir_debug_fpow_config(if_fir_fpow_t *pCtx, uint32_t ulGridLimit, uint64_t ullPosition)
{
    if (!pCtx)
        return 0;
    if (ullPosition != UINT64_MAX)
    {
        // the carried accumulator and partial sum start from +0 at the new position
        HIP_TRY(pCtx, hipSetDevice(pCtx->device));
        for (int i = 0; i < 2; i++)
            HIP_TRY(pCtx, hipMemsetAsync(pCtx->d_state[i], 0, 2 * (size_t)pCtx->Bo * sizeof(float), pCtx->stream));
        HIP_TRY(pCtx, hipStreamSynchronize(pCtx->stream));
        pCtx->st.position = ullPosition;
    }
    pCtx->grid_limit = if_fir::stream_ctx_grid_limit(ulGridLimit);
    return 1;
}
#endif
