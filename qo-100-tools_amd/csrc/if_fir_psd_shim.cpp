// if_fir_psd_shim.cpp — the C ABI of the streaming power-spectrum estimator (include/if_fir.h, if_fir_psd_*; docs/SPEC.md §8).  Its
// own opaque context beside if_fir_ctx_t, if_fir_interp_t and if_fir_resamp_t.  Same conventions: 1/0 status, a message per
// context, no CPU fallback.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "if_fir.h"
#ifdef IF_FIR_DEVELOPMENT
#include "if_fir_debug.h"
#endif
#include "if_fir_psd.h"
#include "if_fir_stream_ctx.h"

#define IF_FIR_API extern "C" __attribute__((visibility("default")))

// the streaming state: what a call advances (and a failed if_fir_psd_process puts back)
struct psd_state
{
    int carry_cur, acc_cur;   // which of d_carry / d_acc the next call reads
    uint64_t position;        // samples since init/reset
    uint64_t carried;         // samples in d_carry[carry_cur]
};

struct if_fir_psd : if_fir::StreamCtx
{
    int N, H, K, bins;
    float scale;              // 1 / (K sum w^2), rounded once
    double ref_power;
    float *d_window;
    float2 *d_twiddle;
    uint16_t *d_bin_pos;
    float2 *d_carry[2];       // the samples of the open chunk, float32, ping-pong
    float *d_acc[2];          // the open frame's accumulator, ping-pong
    float *d_work;            // chunk sums of one call
    uint64_t work_chunks;
    psd_state st;
    void *d_stage_in;         // if_fir_psd_process: staging, allocated by its first call (device-pointer users never pay for it)
    uint16_t *d_stage_codes;
    float *d_stage_power;
    int grid_limit;           // development hook
};

using if_fir::set_err;
static thread_local char g_psd_init_err[256] = "";

static void free_ctx(if_fir_psd *c)
{
    if (!c)
        return;
    if_fir::stream_ctx_close(c, {c->d_window, c->d_twiddle, c->d_bin_pos, c->d_carry[0], c->d_carry[1], c->d_acc[0], c->d_acc[1], c->d_work,
                                 c->d_stage_in, c->d_stage_codes, c->d_stage_power});
    delete c;
}

IF_FIR_API uint8_t if_fir_psd_init(if_fir_psd_t **ppCtx, const if_fir_psd_config_t *pCfg, const float *pfWindow, uint64_t ullMaxSamples,
                                   int32_t lDevice)
{
    if (!if_fir::stream_ctx_init_begin(g_psd_init_err, "if_fir_psd_init", ppCtx))
        return 0;
    if (!pCfg)
    {
        set_err(g_psd_init_err, "if_fir_psd_init: pCfg is NULL");
        return 0;
    }
    const uint32_t N = pCfg->ulSize;
    if (!if_fir::psd_size_ok(N))
    {
        set_err(g_psd_init_err, "if_fir_psd_init: transform size must be 256, 512, 1024, 2048 or 4096 (got %u)", N);
        return 0;
    }
    if (pCfg->ulHop < 1 || pCfg->ulHop > N)
    {
        set_err(g_psd_init_err, "if_fir_psd_init: hop must be 1..%u (got %u)", N, pCfg->ulHop);
        return 0;
    }
    if (pCfg->ulSegments < 1 || pCfg->ulSegments > if_fir::PSD_MAX_SEGMENTS)
    {
        set_err(g_psd_init_err, "if_fir_psd_init: segments per frame must be 1..%u (got %u)", if_fir::PSD_MAX_SEGMENTS, pCfg->ulSegments);
        return 0;
    }
    const int64_t half = (int64_t)N / 2, first = pCfg->lFirstBin;
    if (pCfg->ulBins < 1 || pCfg->ulBins > N || first < -half || first + (int64_t)pCfg->ulBins > half)
    {
        set_err(g_psd_init_err, "if_fir_psd_init: bins [%d, %lld) are outside [-%lld, %lld) (ulBins 1..%u)", pCfg->lFirstBin,
                (long long)(first + (int64_t)pCfg->ulBins), (long long)half, (long long)half, N);
        return 0;
    }
    if (!(pCfg->fRefPower > 0.0f) || !std::isfinite(pCfg->fRefPower))
    {
        set_err(g_psd_init_err, "if_fir_psd_init: fRefPower must be a finite value > 0");
        return 0;
    }
    if (pCfg->ulInputFormat > IF_FIR_INPUT_I16)
    {
        set_err(g_psd_init_err, "if_fir_psd_init: unknown input format %u", pCfg->ulInputFormat);
        return 0;
    }
    if (ullMaxSamples == 0 || ullMaxSamples > ((uint64_t)1 << 40))
    {
        set_err(g_psd_init_err, "if_fir_psd_init: ullMaxSamples must be 1..2^40 (got %llu)", (unsigned long long)ullMaxSamples);
        return 0;
    }
    const uint32_t H = pCfg->ulHop, K = pCfg->ulSegments, bins = pCfg->ulBins;
    const uint64_t work_chunks = if_fir::psd_max_chunks(ullMaxSamples, H, K);
    if (if_fir::psd_max_segments(ullMaxSamples, H) >= if_fir::PSD_MAX_CALL_SEGMENTS)
    {
        set_err(g_psd_init_err, "if_fir_psd_init: a call of ullMaxSamples = %llu samples at hop %u could sum 2^31 segments or more: lower "
                         "ullMaxSamples", (unsigned long long)ullMaxSamples, H);
        return 0;
    }
    if (work_chunks * bins > ((uint64_t)1 << 29))
    {
        set_err(g_psd_init_err, "if_fir_psd_init: a call of ullMaxSamples = %llu samples at hop %u would need %llu chunk sums of %u bins; "
                         "the work buffer is limited to 2^29 values: lower ullMaxSamples",
                (unsigned long long)ullMaxSamples, H, (unsigned long long)work_chunks, bins);
        return 0;
    }
    // the window as given, or the periodic Hann window computed in float64 and rounded once; sum w^2 over the ROUNDED values
    std::vector<float> window(N);
    double energy = 0.0;
    for (uint32_t i = 0; i < N; i++)
    {
        window[i] = pfWindow ? pfWindow[i] : (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)i / (double)N));
        if (!std::isfinite(window[i]))
        {
            set_err(g_psd_init_err, "if_fir_psd_init: window value %u is not finite", i);
            return 0;
        }
        energy += (double)window[i] * (double)window[i];
    }
    if (!(energy > 0.0))
    {
        set_err(g_psd_init_err, "if_fir_psd_init: the window is all zero");
        return 0;
    }
    const std::vector<float> twiddle = if_fir::stream_ctx_twiddles(N);
    std::vector<uint16_t> where(bins);
    for (uint32_t j = 0; j < bins; j++)
        where[j] = (uint16_t)if_fir::psd_bin_position((uint32_t)((first + (int64_t)j + (int64_t)N) % (int64_t)N), N);

    if_fir_psd *c = if_fir::stream_ctx_new<if_fir_psd>(g_psd_init_err, "if_fir_psd_init", lDevice);
    if (!c)
        return 0;
    c->N = (int)N;
    c->H = (int)H;
    c->K = (int)K;
    c->bins = (int)bins;
    c->in_i16 = (int)pCfg->ulInputFormat;
    c->ref_power = (double)pCfg->fRefPower;
    c->scale = (float)(1.0 / ((double)K * energy));
    c->work_chunks = work_chunks;
    const size_t carry_bytes = ((size_t)(if_fir::PSD_CHUNK - 1) * H + N) * sizeof(float2);
    hipError_t e = if_fir::stream_ctx_open(c, lDevice, ullMaxSamples);
    if_fir::stream_ctx_alloc_upload(e, &c->d_window, window.data(), N * sizeof(float));
    if_fir::stream_ctx_alloc_upload(e, &c->d_twiddle, twiddle.data(), N * sizeof(float2));
    if_fir::stream_ctx_alloc_upload(e, &c->d_bin_pos, where.data(), bins * sizeof(uint16_t));
    for (int i = 0; i < 2; i++)
    {
        if_fir::stream_ctx_alloc_zeroed(e, &c->d_carry[i], carry_bytes);
        if_fir::stream_ctx_alloc_zeroed(e, &c->d_acc[i], bins * sizeof(float));
    }
    if (e == hipSuccess)
        e = hipMalloc(&c->d_work, (size_t)work_chunks * bins * sizeof(float));
    return if_fir::stream_ctx_init_end(g_psd_init_err, "if_fir_psd_init", e, c, ppCtx, free_ctx);
}

IF_FIR_API void if_fir_psd_destroy(if_fir_psd_t *pCtx)
{
    free_ctx(pCtx);
}

IF_FIR_API const char *if_fir_psd_last_error(const if_fir_psd_t *pCtx)
{
    return pCtx ? pCtx->err : g_psd_init_err;
}

IF_FIR_API uint8_t if_fir_psd_reset(if_fir_psd_t *pCtx)
{
    if (!pCtx)
        return 0;
    HIP_TRY(pCtx, hipSetDevice(pCtx->device));
    HIP_TRY(pCtx, hipStreamSynchronize(pCtx->stream));
    // (no buffer needs zeroing: nothing is read of the carried samples or the accumulator beyond what the position says is there)
    pCtx->st.position = 0;
    pCtx->st.carried = 0;
    return 1;
}

IF_FIR_API uint8_t if_fir_psd_set_input_format(if_fir_psd_t *pCtx, uint32_t ulFormat)
{
    return if_fir::stream_ctx_set_input_format(pCtx, "if_fir_psd_set_input_format", ulFormat);
}

IF_FIR_API uint8_t if_fir_psd_set_stream(if_fir_psd_t *pCtx, void *pStream)
{
    return if_fir::stream_ctx_set_stream(pCtx, pStream);
}

IF_FIR_API uint8_t if_fir_psd_synchronize(if_fir_psd_t *pCtx)
{
    return if_fir::stream_ctx_synchronize(pCtx);
}

IF_FIR_API uint64_t if_fir_psd_frame_count(const if_fir_psd_t *pCtx, uint64_t ullSamples)
{
    if_fir::PsdPlan plan;
    if (!pCtx || !if_fir::psd_plan(pCtx->st.position, pCtx->st.carried, ullSamples, (uint32_t)pCtx->N, (uint32_t)pCtx->H, (uint32_t)pCtx->K, &plan))
        return 0;
    return plan.frames;
}

static uint8_t run_device(if_fir_psd *c, const void *in, uint16_t *codes, float *power, uint64_t n, uint32_t *pframes, const char *who)
{
    if_fir::PsdPlan plan;
    if (!if_fir::stream_ctx_fits(c, who, n))
        return 0;
    if (!if_fir::psd_plan(c->st.position, c->st.carried, n, (uint32_t)c->N, (uint32_t)c->H, (uint32_t)c->K, &plan) ||
        plan.chunks > c->work_chunks || plan.frames > 0xffffffffull)
    {
        set_err(c->err, "%s: sample count too large", who);
        return 0;
    }
    const uintptr_t in_mask = c->in_i16 ? 3 : 7;
    if (((uintptr_t)in & in_mask) || ((uintptr_t)codes & 1) || ((uintptr_t)power & 3))
    {
        set_err(c->err, "%s: device pointers must be aligned to one element: %u-byte (input), 2-byte (codes), 4-byte (power)", who,
                (unsigned)in_mask + 1);
        return 0;
    }
    if (!if_fir::stream_ctx_device_ptrs(c, who, n, in, plan.frames, codes))
        return 0;
    if (if_fir::stream_ctx_capturing(c, who))
        return 0;
    if (pframes)
        *pframes = 0;
    if (n == 0)
        return 1;
    HIP_TRY(c, hipSetDevice(c->device));
    if_fir::PsdArgs a{};
    a.in = in;
    a.carry = c->d_carry[c->st.carry_cur];
    a.carry_out = c->d_carry[c->st.carry_cur ^ 1];
    a.window = c->d_window;
    a.twiddle = c->d_twiddle;
    a.bin_pos = c->d_bin_pos;
    a.work = c->d_work;
    a.acc = c->d_acc[c->st.acc_cur];
    a.acc_out = c->d_acc[c->st.acc_cur ^ 1];
    a.codes = codes;
    a.power = power;
    a.N = c->N;
    a.H = c->H;
    a.K = c->K;
    a.bins = c->bins;
    a.in_i16 = c->in_i16;
    a.n = (int64_t)n;
    a.carried = (int64_t)c->st.carried;
    a.plan = plan;
    a.scale = c->scale;
    a.ref_power = c->ref_power;
    a.grid_limit = c->grid_limit;
    a.device = c->device;
    a.stream = c->stream;
    HIP_TRY(c, if_fir::launch_psd(a));
    c->st.position += n;
    c->st.carried = plan.carry;
    if (plan.carry > 0)
        c->st.carry_cur ^= 1;
    if (plan.chunks > 0)
        c->st.acc_cur ^= 1;
    if (pframes)
        *pframes = (uint32_t)plan.frames;
    return 1;
}

IF_FIR_API uint8_t if_fir_psd_process_device(if_fir_psd_t *pCtx, const void *pDevIn, uint64_t ullSamples, uint16_t *pusDevBins,
                                             float *pfDevPower, uint32_t *pulFrames)
{
    if (!pCtx)
        return 0;
    return run_device(pCtx, pDevIn, pusDevBins, pfDevPower, ullSamples, pulFrames, "if_fir_psd_process_device");
}

IF_FIR_API uint8_t if_fir_psd_process(if_fir_psd_t *pCtx, const void *pIQIn, uint64_t ullSamples, uint16_t *pusBins, float *pfPower,
                                      uint32_t *pulFrames)
{
    if (!pCtx)
        return 0;
    if (!if_fir::stream_ctx_fits(pCtx, "if_fir_psd_process", ullSamples))
        return 0;
    const uint64_t want = if_fir_psd_frame_count(pCtx, ullSamples);
    if (!if_fir::stream_ctx_host_ptrs(pCtx, "if_fir_psd_process", ullSamples, pIQIn, want, pusBins))
        return 0;
    if (pulFrames)
        *pulFrames = 0;
    if (ullSamples == 0)
        return 1;
    const size_t values = (size_t)if_fir::psd_max_frames(pCtx->max_samples, (uint32_t)pCtx->H, (uint32_t)pCtx->K) * (size_t)pCtx->bins;
    if (!pCtx->d_stage_in &&
        !if_fir::stream_ctx_alloc_staging(pCtx, "if_fir_psd_process",
                                          {{(void **)&pCtx->d_stage_codes, values * sizeof(uint16_t)},
                                           {(void **)&pCtx->d_stage_power, values * sizeof(float)},
                                           {&pCtx->d_stage_in, (size_t)pCtx->max_samples * 8}}))
        return 0;
    uint32_t m = 0;
    if (!if_fir::stream_ctx_staged(
            pCtx, "if_fir_psd_process", "frames", pCtx->d_stage_in, pIQIn, ullSamples, &pCtx->st,
            [&] {
                return run_device(pCtx, pCtx->d_stage_in, pCtx->d_stage_codes, pfPower ? pCtx->d_stage_power : nullptr, ullSamples, &m,
                                  "if_fir_psd_process");
            },
            [&] {
                const size_t values = (size_t)m * (size_t)pCtx->bins;
                hipError_t e = m ? hipMemcpyAsync(pusBins, pCtx->d_stage_codes, values * sizeof(uint16_t), hipMemcpyDeviceToHost, pCtx->stream) : hipSuccess;
                if (e == hipSuccess && m && pfPower)
                    e = hipMemcpyAsync(pfPower, pCtx->d_stage_power, values * sizeof(float), hipMemcpyDeviceToHost, pCtx->stream);
                return e;
            }))
        return 0;
    if (pulFrames)
        *pulFrames = m;
    return 1;
}

#ifdef IF_FIR_DEVELOPMENT
IF_FIR_API uint8_t if_fir_debug_psd_plan(const if_fir_psd_t *pCtx, uint64_t ullSamples, uint64_t *pullPlan)
{
    if_fir::PsdPlan plan;
    if (!pCtx || !pullPlan ||
        !if_fir::psd_plan(pCtx->st.position, pCtx->st.carried, ullSamples, (uint32_t)pCtx->N, (uint32_t)pCtx->H, (uint32_t)pCtx->K, &plan))
        return 0;
    pullPlan[0] = plan.segments;
    pullPlan[1] = plan.chunks;
    pullPlan[2] = plan.frames;
    pullPlan[3] = plan.carry;
    return 1;
}

IF_FIR_API uint8_t if_fir_debug_psd_config(if_fir_psd_t *pCtx, uint32_t ulGridLimit, uint64_t ullPosition)
{
    if (!pCtx)
        return 0;
    if (ullPosition != UINT64_MAX)
    {
        // only where psd_plan accepts (position, carried = 0): on a segment's first sample, and that segment the first of a chunk
        const uint64_t H = (uint64_t)pCtx->H, K = (uint64_t)pCtx->K;
        if (ullPosition % H || ((ullPosition / H) % K) % if_fir::PSD_CHUNK)
        {
            set_err(pCtx->err, "if_fir_debug_psd_config: position %llu is not the first sample of a chunk (hop %llu, %llu segments per frame)",
                    (unsigned long long)ullPosition, (unsigned long long)H, (unsigned long long)K);
            return 0;
        }
        // the open frame's accumulator starts from +0 at the new position, whichever buffer the next call reads
        HIP_TRY(pCtx, hipSetDevice(pCtx->device));
        for (int i = 0; i < 2; i++)
            HIP_TRY(pCtx, hipMemsetAsync(pCtx->d_acc[i], 0, (size_t)pCtx->bins * sizeof(float), pCtx->stream));
        HIP_TRY(pCtx, hipStreamSynchronize(pCtx->stream));
        pCtx->st.position = ullPosition;
        pCtx->st.carried = 0;
    }
    pCtx->grid_limit = if_fir::stream_ctx_grid_limit(ulGridLimit);
    return 1;
}
#endif
