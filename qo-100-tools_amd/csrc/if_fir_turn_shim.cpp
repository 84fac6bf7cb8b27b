// if_fir_turn_shim.cpp — the C ABI of the corner turn (include/if_fir.h, if_fir_turn_*; docs/SPEC.md §20).  Its own opaque context
// beside the other streaming families.  Same conventions: 1/0 status, a message per context, no CPU fallback.  The stage carries
// no streaming state: no history, no position, no reset.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <vector>

#include "if_fir.h"
#ifdef IF_FIR_DEVELOPMENT
#include "if_fir_debug.h"
#endif
#include "if_fir_stream_ctx.h"
#include "if_fir_turn.h"

#define IF_FIR_API extern "C" __attribute__((visibility("default")))

struct if_fir_turn : if_fir::StreamCtx
{
    int direction, B, C, out_i16;
    uint16_t *d_map;          // sel[c] (TO_STREAMS) or inv[i] (TO_FRAMES)
    void *d_stage_frames;     // if_fir_turn_process: staging, allocated by its first call (device-pointer users never pay for it):
    void *d_stage_rows;       // max frames x B elements, and C rows of pitch max frames
    int grid_limit;           // development hook
};

using if_fir::set_err;
static thread_local char g_turn_init_err[256] = "";

static void free_ctx(if_fir_turn *c)
{
    if (!c)
        return;
    if_fir::stream_ctx_close(c, {c->d_map, c->d_stage_frames, c->d_stage_rows});
    delete c;
}

IF_FIR_API uint8_t if_fir_turn_init(if_fir_turn_t **ppCtx, const if_fir_turn_config_t *pCfg, const uint32_t *pulSel, uint64_t ullMaxFrames,
                                    int32_t lDevice)
{
    if (!if_fir::stream_ctx_init_begin(g_turn_init_err, "if_fir_turn_init", ppCtx))
        return 0;
    if (!pCfg)
    {
        set_err(g_turn_init_err, "if_fir_turn_init: pCfg is NULL");
        return 0;
    }
    char why[256];
    if (!if_fir::turn_config_ok(pCfg->ulDirection, pCfg->ulBins, pCfg->ulChannels, pCfg->ulFirst, pCfg->ulInputFormat, pCfg->ulOutputFormat,
                                pulSel, ullMaxFrames, why))
    {
        set_err(g_turn_init_err, "if_fir_turn_init: %s", why);
        return 0;
    }
    if_fir_turn *c = if_fir::stream_ctx_new<if_fir_turn>(g_turn_init_err, "if_fir_turn_init", lDevice);
    if (!c)
        return 0;
    c->direction = (int)pCfg->ulDirection;
    c->B = (int)pCfg->ulBins;
    c->C = (int)pCfg->ulChannels;
    c->in_i16 = (int)pCfg->ulInputFormat;
    c->out_i16 = (int)pCfg->ulOutputFormat;
    std::vector<uint16_t> sel(pCfg->ulChannels), inv(pCfg->ulBins);
    if_fir::turn_maps(pCfg->ulBins, pCfg->ulChannels, pCfg->ulFirst, pulSel, sel.data(), inv.data());
    const std::vector<uint16_t> &map = c->direction == (int)if_fir::TURN_TO_FRAMES ? inv : sel;
    hipError_t e = if_fir::stream_ctx_open(c, lDevice, ullMaxFrames);
    if_fir::stream_ctx_alloc_upload(e, &c->d_map, map.data(), map.size() * sizeof(uint16_t));
    return if_fir::stream_ctx_init_end(g_turn_init_err, "if_fir_turn_init", e, c, ppCtx, free_ctx);
}

IF_FIR_API void if_fir_turn_destroy(if_fir_turn_t *pCtx)
{
    free_ctx(pCtx);
}

IF_FIR_API const char *if_fir_turn_last_error(const if_fir_turn_t *pCtx)
{
    return pCtx ? pCtx->err : g_turn_init_err;
}

IF_FIR_API uint8_t if_fir_turn_set_input_format(if_fir_turn_t *pCtx, uint32_t ulFormat)
{
    return if_fir::stream_ctx_set_input_format(pCtx, "if_fir_turn_set_input_format", ulFormat);
}

IF_FIR_API uint8_t if_fir_turn_set_output_format(if_fir_turn_t *pCtx, uint32_t ulFormat)
{
    if (!pCtx)
        return 0;
    if (ulFormat > IF_FIR_OUTPUT_I16)
    {
        set_err(pCtx->err, "if_fir_turn_set_output_format: unknown format %u", ulFormat);
        return 0;
    }
    pCtx->out_i16 = (int)ulFormat;
    return 1;
}

IF_FIR_API uint8_t if_fir_turn_set_stream(if_fir_turn_t *pCtx, void *pStream)
{
    return if_fir::stream_ctx_set_stream(pCtx, pStream);
}

IF_FIR_API uint8_t if_fir_turn_synchronize(if_fir_turn_t *pCtx)
{
    return if_fir::stream_ctx_synchronize(pCtx);
}

// the checks of a call that need no device: the pitch against the frame count, the frame count against init's
static bool plan_call(if_fir_turn *c, const char *who, uint64_t frames, uint64_t pitch)
{
    char why[256];
    if (if_fir::turn_call_ok(frames, pitch, c->max_samples, why))
        return true;
    set_err(c->err, "%s: %s", who, why);
    return false;
}

static uint8_t run_device(if_fir_turn *c, const void *in, void *out, uint64_t frames, uint64_t pitch, const char *who)
{
    if (!plan_call(c, who, frames, pitch))
        return 0;
    if (!if_fir::stream_ctx_aligned(c, who, "element", in, c->in_i16 ? 3 : 7, out, c->out_i16 ? 3 : 7))
        return 0;
    if (!if_fir::stream_ctx_device_ptrs(c, who, frames, in, frames, out))
        return 0;
    if (if_fir::stream_ctx_capturing(c, who))
        return 0;
    if (frames == 0)
        return 1;
    HIP_TRY(c, hipSetDevice(c->device));
    if_fir::TurnArgs a{};
    a.in = in;
    a.out = out;
    a.map = c->d_map;
    a.direction = c->direction;
    a.B = c->B;
    a.C = c->C;
    a.in_i16 = c->in_i16;
    a.out_i16 = c->out_i16;
    a.F = (int64_t)frames;
    a.P = (int64_t)pitch;
    a.grid_limit = c->grid_limit;
    a.device = c->device;
    a.stream = c->stream;
    HIP_TRY(c, if_fir::launch_turn(a));
    return 1;
}

IF_FIR_API uint8_t if_fir_turn_process_device(if_fir_turn_t *pCtx, const void *pDevIn, void *pDevOut, uint64_t ullFrames, uint64_t ullPitch)
{
    if (!pCtx)
        return 0;
    return run_device(pCtx, pDevIn, pDevOut, ullFrames, ullPitch, "if_fir_turn_process_device");
}

// host pointers: the frame side goes as one piece, the row side as C rows of the caller's pitch against the staging's pitch of
// ullFrames, so the tails of the caller's rows are neither read nor written
IF_FIR_API uint8_t if_fir_turn_process(if_fir_turn_t *pCtx, const void *pIn, void *pOut, uint64_t ullFrames, uint64_t ullPitch)
{
    const char *who = "if_fir_turn_process";
    if_fir_turn *c = pCtx;
    if (!c)
        return 0;
    if (!plan_call(c, who, ullFrames, ullPitch))
        return 0;
    if (!if_fir::stream_ctx_host_ptrs(c, who, ullFrames, pIn, ullFrames, pOut))
        return 0;
    if (ullFrames == 0)
        return 1;
    if (!c->d_stage_frames && !if_fir::stream_ctx_alloc_staging(c, who,
                                                                {{&c->d_stage_frames, (size_t)c->max_samples * (size_t)c->B * 8},
                                                                 {&c->d_stage_rows, (size_t)c->max_samples * (size_t)c->C * 8}}))
        return 0;
    const bool to_frames = c->direction == (int)if_fir::TURN_TO_FRAMES;
    const size_t ein = c->in_i16 ? 4 : 8, eout = c->out_i16 ? 4 : 8, F = (size_t)ullFrames, P = (size_t)ullPitch;
    void *d_in = to_frames ? c->d_stage_rows : c->d_stage_frames, *d_out = to_frames ? c->d_stage_frames : c->d_stage_rows;
    HIP_TRY(c, hipSetDevice(c->device));
    if (to_frames)
        HIP_TRY(c, hipMemcpy2DAsync(d_in, F * ein, pIn, P * ein, F * ein, (size_t)c->C, hipMemcpyHostToDevice, c->stream));
    else
        HIP_TRY(c, hipMemcpyAsync(d_in, pIn, F * (size_t)c->B * ein, hipMemcpyHostToDevice, c->stream));
    if (!run_device(c, d_in, d_out, ullFrames, ullFrames, who))
    {
        (void)hipStreamSynchronize(c->stream);
        return 0;
    }
    hipError_t e = to_frames ? hipMemcpyAsync(pOut, d_out, F * (size_t)c->B * eout, hipMemcpyDeviceToHost, c->stream)
                             : hipMemcpy2DAsync(pOut, P * eout, d_out, F * eout, F * eout, (size_t)c->C, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess)
        e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess)
    {
        set_err(c->err, "%s: copying the result back failed: %s", who, hipGetErrorString(e));
        (void)hipGetLastError();
        return 0;
    }
    return 1;
}

#ifdef IF_FIR_DEVELOPMENT
IF_FIR_API uint8_t if_fir_debug_turn_config(if_fir_turn_t *pCtx, uint32_t ulGridLimit)
{
    if (!pCtx)
        return 0;
    pCtx->grid_limit = if_fir::stream_ctx_grid_limit(ulGridLimit);
    return 1;
}
#endif
