// if_fir_stream_ctx.h — what the C-ABI shims of the streaming contexts (if_fir_interp_t, if_fir_resamp_t, if_fir_psd_t, if_fir_ddc_t, if_fir_duc_t, if_fir_arb_t, if_fir_pfb_t, if_fir_synth_t) share: the base
// of the context struct, the message writer, opening and closing, and the host-pointer ("staged") call.  Host code only.
//
// The rule for what belongs here: code in this header never branches on which family calls it.  Where the families differ --
// argument validation and its order, run_device and the order of its checks, alignment masks, lazily allocated buffers, what
// counts as streaming state -- the code stays in the family's shim and calls these helpers.  Everything is static: a shim
// exports its IF_FIR_API entry points and nothing of this.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "if_fir.h"

namespace if_fir
{

struct StreamCtx
{
    int device;
    hipStream_t own_stream;
    hipStream_t stream;       // own_stream, or the caller's (set_stream)
    int in_i16;
    uint64_t max_samples;     // of the host-pointer call
    mutable char err[256];
};

// dst: a context's err, or the family's thread-local buffer for init (if_fir_X_last_error(NULL) is per family and per thread)
static inline void set_err(char *dst, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(dst, 256, fmt, ap);
    va_end(ap);
}

#define HIP_TRY(ctx, call)                                                                                     \
    do                                                                                                         \
    {                                                                                                          \
        hipError_t e_ = (call);                                                                                \
        if (e_ != hipSuccess)                                                                                  \
        {                                                                                                      \
            if_fir::set_err((ctx)->err, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return 0;                                                                                          \
        }                                                                                                      \
    } while (0)

// init, after the family's own argument checks: is lDevice one of the visible devices?  who = "if_fir_X_init"
static inline bool stream_ctx_device_ok(char *err, const char *who, int32_t lDevice)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    {
        (void)hipGetLastError();
        set_err(err, "%s: no HIP device", who);
        return false;
    }
    if (lDevice < 0 || lDevice >= ndev)
    {
        set_err(err, "%s: device %d does not exist (%d visible)", who, lDevice, ndev);
        return false;
    }
    return true;
}

// init: select the device and create the context's own non-blocking stream.  The result starts the chain of the allocation
// helpers below: each does nothing once e is an error, so an init is a straight list of calls and one check at its end.
static inline hipError_t stream_ctx_open(StreamCtx *c, int32_t lDevice, uint64_t ullMaxSamples)
{
    c->device = lDevice;
    c->max_samples = ullMaxSamples;
    hipError_t e = hipSetDevice(lDevice);
    if (e == hipSuccess)
        e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    c->stream = c->own_stream;
    return e;
}

template <typename T>
static inline void stream_ctx_alloc_upload(hipError_t &e, T **p, const void *src, size_t bytes)
{
    if (e == hipSuccess)
        e = hipMalloc(p, bytes);
    if (e == hipSuccess)
        e = hipMemcpy(*p, src, bytes, hipMemcpyHostToDevice);
}

template <typename T>
static inline void stream_ctx_alloc_zeroed(hipError_t &e, T **p, size_t bytes)
{
    if (e == hipSuccess)
        e = hipMalloc(p, bytes);
    if (e == hipSuccess)
        e = hipMemset(*p, 0, bytes);
}

// destroy, and init after a failure: wait for the work in flight, destroy the own stream, free the family's buffers (nulls are
// skipped).  A caller-owned stream may be gone already: its error is swallowed.
static inline void stream_ctx_close(StreamCtx *c, std::initializer_list<void *> bufs)
{
    (void)hipSetDevice(c->device);
    if (c->stream && c->stream != c->own_stream && hipStreamSynchronize(c->stream) != hipSuccess)
        (void)hipGetLastError();
    if (c->own_stream)
    {
        (void)hipStreamSynchronize(c->own_stream);
        (void)hipStreamDestroy(c->own_stream);
    }
    for (void *b : bufs)
        if (b)
            (void)hipFree(b);
}

// who = "if_fir_X_set_input_format".  (The families keep their streaming state as float32: a change of format keeps the stream.)
static inline uint8_t stream_ctx_set_input_format(StreamCtx *c, const char *who, uint32_t ulFormat)
{
    if (!c)
        return 0;
    if (ulFormat > IF_FIR_INPUT_I16)
    {
        set_err(c->err, "%s: unknown format %u", who, ulFormat);
        return 0;
    }
    c->in_i16 = (int)ulFormat;
    return 1;
}

// (unlike if_fir_set_stream, this does not drain the old stream first: work on the two streams may overlap on the context's buffers)
static inline uint8_t stream_ctx_set_stream(StreamCtx *c, void *pStream)
{
    if (!c)
        return 0;
    c->stream = pStream ? static_cast<hipStream_t>(pStream) : c->own_stream;
    return 1;
}

static inline uint8_t stream_ctx_synchronize(StreamCtx *c)
{
    if (!c)
        return 0;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return 1;
}

// true, with the message set, when the context's stream is being captured: a family's run_device then refuses the call
static inline bool stream_ctx_capturing(StreamCtx *c, const char *who)
{
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(c->stream, &capture) != hipSuccess || capture == hipStreamCaptureStatusNone)
        return false;
    set_err(c->err, "%s: the context's stream is being captured into a hipGraph; calls carry host-side streaming state and "
                    "cannot be replayed", who);
    return true;
}

static inline bool stream_ctx_fits(StreamCtx *c, const char *who, uint64_t n)
{
    if (n <= c->max_samples)
        return true;
    set_err(c->err, "%s: %llu samples exceed ullMaxSamples %llu of init", who, (unsigned long long)n, (unsigned long long)c->max_samples);
    return false;
}

// The host-pointer call of a family, after its own checks (n > 0 samples at host_in): copy them to d_stage_in on the context's
// stream, run() the family's run_device on its staging buffers, copy_back() what that produced (a hipError_t: the asynchronous
// copies, hipSuccess if there is nothing to copy), synchronize.  *state is the family's streaming state, the fields run_device
// advances; what = "outputs" / "frames", for the message.
// (stream_ctx_staged_bytes: the same for a family whose samples are not IQ pairs; it gives the bytes of its input itself)
template <typename State, typename Run, typename CopyBack>
static inline uint8_t stream_ctx_staged_bytes(StreamCtx *c, const char *who, const char *what, void *d_stage_in, const void *host_in,
                                              size_t bytes, State *state, Run run, CopyBack copy_back)
{
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(d_stage_in, host_in, bytes, hipMemcpyHostToDevice, c->stream));
    const State before = *state;
    if (!run())
    {
        (void)hipStreamSynchronize(c->stream);
        return 0;
    }
    hipError_t e = copy_back();
    if (e == hipSuccess)
        e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess)
    {
        // the results did not reach the caller: the call failed, so the stream goes back to where it was (the state of before
        // the call is still in the ping-pong buffers the kernels read)
        *state = before;
        set_err(c->err, "%s: copying the %s back failed: %s", who, what, hipGetErrorString(e));
        (void)hipGetLastError();
        return 0;
    }
    return 1;
}

template <typename State, typename Run, typename CopyBack>
static inline uint8_t stream_ctx_staged(StreamCtx *c, const char *who, const char *what, void *d_stage_in, const void *host_in,
                                        uint64_t n, State *state, Run run, CopyBack copy_back)
{
    return stream_ctx_staged_bytes(c, who, what, d_stage_in, host_in, (size_t)n * (c->in_i16 ? 4 : 8), state, run, copy_back);
}

} // namespace if_fir
