// if_fir_subup_shim.cpp — the C ABI of the per-bin interpolating FIR stage over frames (include/if_fir.h, if_fir_subup_*;
// docs/SPEC.md §16).  Its own opaque context beside the other streaming families.  Same conventions: 1/0 status, a message per
// context, no CPU fallback.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <vector>

#include "if_fir.h"
#ifdef IF_FIR_DEVELOPMENT
#include "if_fir_debug.h"
#endif
#include "if_fir_stream_ctx.h"
#include "if_fir_subup.h"

#define IF_FIR_API extern "C" __attribute__((visibility("default")))

// the streaming state: what a call advances (and a failed if_fir_subup_process puts back)
struct subup_state
{
    int hist_cur;
    uint64_t position;        // input frames since init/reset
};

struct if_fir_subup : if_fir::StreamCtx
{
    int B, T, rows, R, J;
    std::vector<uint32_t> words;     // phase word per bin (0 = no mixing)
    float *d_taps;                   // the table of subup_build_table
    uint32_t *d_words;
    if_fir::StreamHistory hist;      // the last J - 1 input frames, float32
    subup_state st;
    void *d_stage_in;                // if_fir_subup_process: staging, allocated by its first call
    float2 *d_stage_out;
    int grid_limit;                  // development hook
};

using if_fir::set_err;
static thread_local char g_subup_init_err[256] = "";

static void free_ctx(if_fir_subup *c)
{
    if (!c)
        return;
    if_fir::stream_ctx_close(c, {c->d_taps, c->d_words, c->hist.buf[0], c->hist.buf[1], c->d_stage_in, c->d_stage_out});
    delete c;
}

IF_FIR_API uint8_t if_fir_subup_init(if_fir_subup_t **ppCtx, const if_fir_subup_config_t *pCfg, const float *pfTaps, uint64_t ullMaxFrames,
                                     int32_t lDevice)
{
    if (!if_fir::stream_ctx_init_begin(g_subup_init_err, "if_fir_subup_init", ppCtx))
        return 0;
    if (!pCfg)
    {
        set_err(g_subup_init_err, "if_fir_subup_init: pCfg is NULL");
        return 0;
    }
    char why[256];
    if (!if_fir::subup_config_ok(pCfg->ulBins, pCfg->ulTaps, pCfg->ulTapRows, pCfg->ulInterpolation, ullMaxFrames, pfTaps != nullptr, why))
    {
        set_err(g_subup_init_err, "if_fir_subup_init: %s", why);
        return 0;
    }
    if_fir_subup *c = if_fir::stream_ctx_new<if_fir_subup>(g_subup_init_err, "if_fir_subup_init", lDevice);
    if (!c)
        return 0;
    c->B = (int)pCfg->ulBins;
    c->T = (int)pCfg->ulTaps;
    c->rows = (int)pCfg->ulTapRows;
    c->R = (int)pCfg->ulInterpolation;
    c->J = (int)if_fir::subup_j(pCfg->ulTaps, pCfg->ulInterpolation);
    c->words.assign((size_t)c->B, 0u);
    std::vector<float> table(if_fir::subup_table_floats(pCfg->ulTaps, pCfg->ulTapRows, pCfg->ulInterpolation));
    if_fir::subup_build_table(pfTaps, pCfg->ulTaps, pCfg->ulTapRows, pCfg->ulInterpolation, table.data());
    hipError_t e = if_fir::stream_ctx_open(c, lDevice, ullMaxFrames);
    if_fir::stream_ctx_alloc_upload(e, &c->d_taps, table.data(), table.size() * sizeof(float));
    if_fir::stream_ctx_alloc_upload(e, &c->d_words, c->words.data(), c->words.size() * sizeof(uint32_t));
    if_fir::stream_history_alloc(e, &c->hist, (size_t)(c->J - 1) * c->B * sizeof(float2), sizeof(float2));
    return if_fir::stream_ctx_init_end(g_subup_init_err, "if_fir_subup_init", e, c, ppCtx, free_ctx);
}

IF_FIR_API void if_fir_subup_destroy(if_fir_subup_t *pCtx)
{
    free_ctx(pCtx);
}

IF_FIR_API const char *if_fir_subup_last_error(const if_fir_subup_t *pCtx)
{
    return pCtx ? pCtx->err : g_subup_init_err;
}

IF_FIR_API uint8_t if_fir_subup_reset(if_fir_subup_t *pCtx)
{
    if (!pCtx || !if_fir::stream_history_zero(pCtx, pCtx->hist))
        return 0;
    pCtx->st.position = 0;
    return 1;
}

IF_FIR_API uint8_t if_fir_subup_set_input_format(if_fir_subup_t *pCtx, uint32_t ulFormat)
{
    return if_fir::stream_ctx_set_input_format(pCtx, "if_fir_subup_set_input_format", ulFormat);
}

// SPEC §16: the words in force at a call rotate that call's outputs by their absolute index (the history holds unmixed
// frames and the taps are not mixed: only the words change).  Every frequency is checked before anything changes.  Waits for
// the context's stream: kernels in flight still read the old words.
IF_FIR_API uint8_t if_fir_subup_set_nco(if_fir_subup_t *pCtx, const double *pdFreq)
{
    if (!pCtx)
        return 0;
    std::vector<uint32_t> words((size_t)pCtx->B, 0u);
    for (int j = 0; pdFreq && j < pCtx->B; j++)
        if (!if_fir::stream_ctx_nco_word(pCtx, "if_fir_subup_set_nco", pdFreq[j], &words[(size_t)j]))
            return 0;
    if (words == pCtx->words)
        return 1;
    HIP_TRY(pCtx, hipSetDevice(pCtx->device));
    HIP_TRY(pCtx, hipStreamSynchronize(pCtx->stream));
    HIP_TRY(pCtx, hipMemcpy(pCtx->d_words, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    pCtx->words = words;
    return 1;
}

IF_FIR_API uint8_t if_fir_subup_get_nco(const if_fir_subup_t *pCtx, double *pdFreq)
{
    if (!pCtx || !pdFreq)
        return 0;
    for (int j = 0; j < pCtx->B; j++)
        pdFreq[j] = if_fir::nco_freq_of(pCtx->words[(size_t)j]); // the quantised frequencies actually applied
    return 1;
}

IF_FIR_API uint8_t if_fir_subup_set_stream(if_fir_subup_t *pCtx, void *pStream)
{
    return if_fir::stream_ctx_set_stream(pCtx, pStream);
}

IF_FIR_API uint8_t if_fir_subup_synchronize(if_fir_subup_t *pCtx)
{
    return if_fir::stream_ctx_synchronize(pCtx);
}

IF_FIR_API uint64_t if_fir_subup_frame_count(const if_fir_subup_t *pCtx, uint64_t ullFrames)
{
    if_fir::SubUpCall call;
    if (!pCtx || !if_fir::subup_call(pCtx->st.position, ullFrames, (uint32_t)pCtx->R, &call))
        return 0;
    return call.count;
}

// the checks of a call that need no device: the frame count against init's and the output position against 2^64
static bool plan_call(if_fir_subup *c, const char *who, uint64_t frames, if_fir::SubUpCall *call)
{
    if (frames > c->max_samples)
    {
        set_err(c->err, "%s: %llu frames exceed ullMaxFrames %llu of init", who, (unsigned long long)frames, (unsigned long long)c->max_samples);
        return false;
    }
    if (!if_fir::subup_call(c->st.position, frames, (uint32_t)c->R, call))
    {
        set_err(c->err, "%s: frame count too large: the stream position would pass 2^64", who);
        return false;
    }
    return true;
}

static uint8_t run_device(if_fir_subup *c, const void *in, void *out, uint64_t frames, uint64_t *pframes, const char *who)
{
    if_fir::SubUpCall call;
    if (!plan_call(c, who, frames, &call))
        return 0;
    if (!if_fir::stream_ctx_aligned(c, who, "element", in, c->in_i16 ? 3 : 7, out, 7) ||
        !if_fir::stream_ctx_device_ptrs(c, who, frames, in, call.count, out))
        return 0;
    if (if_fir::stream_ctx_capturing(c, who))
        return 0;
    if (pframes)
        *pframes = 0;
    if (frames == 0)
        return 1;
    HIP_TRY(c, hipSetDevice(c->device));
    if_fir::SubUpArgs a{};
    a.in = in;
    a.out = static_cast<float2 *>(out);
    a.hist = c->hist.at<float2>(c->st.hist_cur);
    a.hist_out = c->hist.at<float2>(c->st.hist_cur ^ 1);
    a.taps = c->d_taps;
    a.words = c->d_words;
    a.B = c->B;
    a.T = c->T;
    a.rows = c->rows;
    a.R = c->R;
    a.in_i16 = c->in_i16;
    a.F = (int64_t)frames;
    a.call = call;
    a.grid_limit = c->grid_limit;
    a.device = c->device;
    a.stream = c->stream;
    HIP_TRY(c, if_fir::launch_subup(a));
    c->st.position += frames;
    if (c->J > 1)
        c->st.hist_cur ^= 1;
    if (pframes)
        *pframes = call.count;
    return 1;
}

IF_FIR_API uint8_t if_fir_subup_process_device(if_fir_subup_t *pCtx, const void *pDevIn, void *pDevOut, uint64_t ullFrames,
                                               uint64_t *pullOutFrames)
{
    if (!pCtx)
        return 0;
    return run_device(pCtx, pDevIn, pDevOut, ullFrames, pullOutFrames, "if_fir_subup_process_device");
}

IF_FIR_API uint8_t if_fir_subup_process(if_fir_subup_t *pCtx, const void *pFramesIn, float *pfFramesOut, uint64_t ullFrames,
                                        uint64_t *pullOutFrames)
{
    if (!pCtx)
        return 0;
    if_fir::SubUpCall call;
    if (!plan_call(pCtx, "if_fir_subup_process", ullFrames, &call))
        return 0;
    if (!if_fir::stream_ctx_host_ptrs(pCtx, "if_fir_subup_process", ullFrames, pFramesIn, call.count, pfFramesOut))
        return 0;
    if (pullOutFrames)
        *pullOutFrames = 0;
    if (ullFrames == 0)
        return 1;
    const size_t B = (size_t)pCtx->B;
    if (!pCtx->d_stage_in &&
        !if_fir::stream_ctx_alloc_staging(pCtx, "if_fir_subup_process",
                                          {{(void **)&pCtx->d_stage_out, (size_t)pCtx->max_samples * (size_t)pCtx->R * B * sizeof(float2)},
                                           {&pCtx->d_stage_in, (size_t)pCtx->max_samples * B * 8}}))
        return 0;
    uint64_t m = 0;
    if (!if_fir::stream_ctx_staged_bytes(
            pCtx, "if_fir_subup_process", "frames", pCtx->d_stage_in, pFramesIn, (size_t)ullFrames * B * (pCtx->in_i16 ? 4 : 8), &pCtx->st,
            [&] { return run_device(pCtx, pCtx->d_stage_in, pCtx->d_stage_out, ullFrames, &m, "if_fir_subup_process"); },
            [&] {
                return m ? hipMemcpyAsync(pfFramesOut, pCtx->d_stage_out, (size_t)m * B * sizeof(float2), hipMemcpyDeviceToHost, pCtx->stream)
                         : hipSuccess;
            }))
        return 0;
    if (pullOutFrames)
        *pullOutFrames = m;
    return 1;
}

#ifdef IF_FIR_DEVELOPMENT
IF_FIR_API uint8_t if_fir_debug_subup_config(if_fir_subup_t *pCtx, uint32_t ulGridLimit, uint32_t *pulTileOutputs, uint64_t ullPosition)
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
    if (pulTileOutputs)
        *pulTileOutputs = (uint32_t)if_fir::SUBUP_THREADS * (uint32_t)if_fir::SUBUP_Q; // (output, bin) values of one tile
    return 1;
}
#endif
