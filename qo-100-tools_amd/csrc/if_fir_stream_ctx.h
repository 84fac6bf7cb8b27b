// if_fir_stream_ctx.h — what the C-ABI shims of the streaming contexts (STREAM_FAMILIES in the Makefile: one if_fir_X_t and one
// if_fir_X_shim.cpp each) share: the base of the context struct, the message writer, opening and closing, the frame of an init,
// the ping-pong history, the pointer checks of a call, the host-pointer ("staged") call and its lazily allocated buffers, and
// the small conversions several families repeat (NCO word, grid limit, transform twiddles).  Host code only.
//
// The rule for what belongs here: code in this header never branches on which family calls it.  Where the families differ --
// argument validation and its order, run_device and the order of its checks, alignment masks, element types and sizes, what
// counts as streaming state -- the code stays in the family's shim and calls these helpers with the difference as an argument.
// A piece that would fit a family only through a flag stays a copy in that family.  Everything is static: a shim exports its
// IF_FIR_API entry points and nothing of this.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <new>
#include <utility>
#include <vector>

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

// The frame of an init.  Head: stream_ctx_init_begin first of all, the family's own argument checks in its own order, then
// stream_ctx_new (device check, nothrow allocation).  Tail, after the allocation chain: stream_ctx_init_end.  err is the family's
// thread-local init message, who = "if_fir_X_init".
template <typename Ctx>
static inline bool stream_ctx_init_begin(char *err, const char *who, Ctx **ppCtx)
{
    if (!ppCtx)
    {
        set_err(err, "%s: ppCtx is NULL", who);
        return false;
    }
    *ppCtx = nullptr;
    return true;
}

template <typename Ctx>
static inline Ctx *stream_ctx_new(char *err, const char *who, int32_t lDevice)
{
    if (!stream_ctx_device_ok(err, who, lDevice))
        return nullptr;
    Ctx *c = new (std::nothrow) Ctx();
    if (!c)
        set_err(err, "%s: out of host memory", who);
    return c;
}

// e: the result of the allocation chain; free_ctx: the family's teardown (stream_ctx_close with its buffers, delete)
template <typename Ctx, typename Free>
static inline uint8_t stream_ctx_init_end(char *err, const char *who, hipError_t e, Ctx *c, Ctx **ppCtx, Free free_ctx)
{
    if (e != hipSuccess)
    {
        set_err(err, "%s: %s", who, hipGetErrorString(e));
        (void)hipGetLastError();
        free_ctx(c);
        return 0;
    }
    *ppCtx = c;
    return 1;
}

// The ping-pong history of a family: a call reads at(hist_cur) and writes at(hist_cur ^ 1).  What the elements are is the
// family's business; which buffer is current stays in the family's streaming state (stream_ctx_staged rolls that back).
// Both buffers go into the family's stream_ctx_close list.
struct StreamHistory
{
    void *buf[2];
    size_t bytes;             // of the history proper (0: the family keeps none at this shape)

    template <typename T>
    T *at(int cur) const
    {
        return static_cast<T *>(buf[cur]);
    }
};

// init: both buffers, zeroed, in the allocation chain.  min_bytes: the least to allocate (one element where a family never
// hands its kernels a null history, 0 otherwise)
static inline void stream_history_alloc(hipError_t &e, StreamHistory *h, size_t bytes, size_t min_bytes)
{
    h->bytes = bytes;
    for (int i = 0; i < 2; i++)
        stream_ctx_alloc_zeroed(e, &h->buf[i], bytes > min_bytes ? bytes : min_bytes);
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

// reset, and a development hook that moves the stream position: zero both history buffers on the context's stream and wait
static inline uint8_t stream_history_zero(StreamCtx *c, const StreamHistory &h)
{
    HIP_TRY(c, hipSetDevice(c->device));
    for (int i = 0; i < 2 && h.bytes > 0; i++)
        HIP_TRY(c, hipMemsetAsync(h.buf[i], 0, h.bytes, c->stream));
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

// The pointer checks of a call; each family makes them where its order of checks has them.  The masks are the family's (they may
// depend on its formats); noun = "sample" / "element", for the message.
static inline bool stream_ctx_aligned(StreamCtx *c, const char *who, const char *noun, const void *in, uintptr_t in_mask, const void *out,
                                      uintptr_t out_mask)
{
    if (!((uintptr_t)in & in_mask) && !((uintptr_t)out & out_mask))
        return true;
    set_err(c->err, "%s: device pointers must be aligned to one %s: %u-byte (input) and %u-byte (output)", who, noun, (unsigned)in_mask + 1,
            (unsigned)out_mask + 1);
    return false;
}

// n inputs are read from in, count outputs written to out: a pointer may be NULL only where nothing goes through it.
// stream_ctx_device_ptrs for the device call, stream_ctx_host_ptrs for the host-pointer call.
static inline bool stream_ctx_device_ptrs(StreamCtx *c, const char *who, uint64_t n, const void *in, uint64_t count, const void *out)
{
    if (!(n && !in) && !(count && !out))
        return true;
    set_err(c->err, "%s: NULL device pointer", who);
    return false;
}

static inline bool stream_ctx_host_ptrs(StreamCtx *c, const char *who, uint64_t n, const void *in, uint64_t count, const void *out)
{
    if (!(n && !in) && !(count && !out))
        return true;
    set_err(c->err, "%s: NULL buffer", who);
    return false;
}

// The staging buffers of a family that allocates them on its first host-pointer call (device-pointer users never pay for them):
// every (pointer, bytes) of the list in order; on a failure what was allocated is freed, the pointers are null again and the
// message is set.
static inline uint8_t stream_ctx_alloc_staging(StreamCtx *c, const char *who, std::initializer_list<std::pair<void **, size_t>> bufs)
{
    HIP_TRY(c, hipSetDevice(c->device));
    hipError_t e = hipSuccess;
    for (const auto &b : bufs)
        if (e == hipSuccess)
            e = hipMalloc(b.first, b.second);
    if (e == hipSuccess)
        return 1;
    (void)hipGetLastError();
    for (const auto &b : bufs)
    {
        if (*b.first)
            (void)hipFree(*b.first);
        *b.first = nullptr;
    }
    set_err(c->err, "%s: staging buffers: %s", who, hipGetErrorString(e));
    return 0;
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

// The NCO phase word of a frequency in cycles/sample (SPEC §3.2), mod 2^32 as if_fir_set_nco, and the quantised frequency a
// word stands for.  stream_ctx_nco_word: the same with the range check of a set_nco; who = "if_fir_X_set_nco".
static inline uint32_t nco_word_of(double f)
{
    return (uint32_t)(int64_t)std::llround(f * 4294967296.0);
}

static inline double nco_freq_of(uint32_t word)
{
    return (double)(int32_t)word / 4294967296.0;
}

static inline bool stream_ctx_nco_word(StreamCtx *c, const char *who, double f, uint32_t *word)
{
    if (!std::isfinite(f) || std::fabs(f) > 0.5)
    {
        set_err(c->err, "%s: frequency must be within +-0.5 cycles/sample (got %g)", who, f);
        return false;
    }
    *word = nco_word_of(f);
    return true;
}

// the development hooks' ulGridLimit as the launchers take it
static inline int stream_ctx_grid_limit(uint32_t ulGridLimit)
{
    return (int)(ulGridLimit > 65536u ? 65536u : ulGridLimit);
}

// the transform's table e^{-2 pi j t / M}, t = 0 .. M - 1, as (re, im) pairs: float64 cos and sin, rounded once
static inline std::vector<float> stream_ctx_twiddles(uint32_t M)
{
    std::vector<float> twiddle(2 * (size_t)M);
    for (uint32_t t = 0; t < M; t++)
    {
        const double ang = -2.0 * M_PI * (double)t / (double)M;
        twiddle[2 * t] = (float)cos(ang);
        twiddle[2 * t + 1] = (float)sin(ang);
    }
    return twiddle;
}

} // namespace if_fir
