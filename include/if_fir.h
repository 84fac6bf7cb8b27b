/*
 * if_fir.h — C ABI of libif_fir.so: MI355X-native IF-chain FIR filter / decimator for complex IQ streams.
 *
 * Plain C99, no HIP types.  Host code stays C and reaches the CDNA4 kernels through these entry points.
 *
 * WHAT THIS REPLACES IN THE REFERENCE: nothing that exists.  vankxr/qo-100-tools has no filter entry
 * point to bind: `util/if-bandpass-filter/` is an analog LC design
 * (/root/reference/util/if-bandpass-filter/schematic.svg:174-222) and `software/opi-rf-manager/package.json:6-15`
 * lists no DSP dependency.  The surface below is BUILD-DEFINED; only the reference's *conventions* are kept:
 *   - snake_case `module_verb_noun` names and Hungarian argument prefixes
 *     (/root/reference/software/upconverter/src/main.c:572,585  — `ulSamples`, `pfPData`, `fAttenuation`);
 *   - `uint8_t` status, 1 = success, 0 = failure
 *     (/root/reference/software/upconverter/src/f1958.c:12-27, .../src/include/adf4351.h:93-100);
 *   - small enums for modes (/root/reference/software/gpsdo/src/include/ocxo.h:15-19).
 *
 * Semantics: docs/SPEC.md.   y[n] = Σ_k h[k]·x[n-k],  y_D[m] = y[mD],  interleaved float32 I/Q, real float32 taps,
 * T-1 samples of history and the decimation phase carried across calls.
 *
 * Error model: every function that can fail returns 0 and records a message retrievable with
 * if_fir_last_error(); nothing aborts or throws across the boundary; a context stays usable after a failed call.
 * There is NO CPU fallback: without a usable HIP device if_fir_init() fails.
 *
 * Threading: one context = one HIP stream, not re-entrant; distinct contexts may be used from distinct threads.
 */
#ifndef IF_FIR_H
#define IF_FIR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IF_FIR_VERSION_MAJOR 0
#define IF_FIR_VERSION_MINOR 1

#define IF_FIR_MAX_TAPS 4096u
#define IF_FIR_MAX_DECIMATION 64u

typedef struct if_fir_ctx if_fir_ctx_t; /* opaque: device buffers, history, phase, stream, last error */

/* kernel families.  AUTO picks per (T, D). */
enum
{
    IF_FIR_BACKEND_AUTO = 0,
    IF_FIR_BACKEND_HIP_DIRECT = 1,  /* register-blocked sample-stationary direct form, taps in SGPRs            */
    IF_FIR_BACKEND_HIP_TAPSPLIT = 2,/* any T, D: taps staged in LDS, split over 4 lanes, partial sums DPP-reduced */
    IF_FIR_BACKEND_HIP_GENERIC = 3, /* any T, D: one output per thread (simple cross-check kernel)                */
    IF_FIR_BACKEND_HIP_FFT = 4      /* overlap-save, wave-private 4096-point FFT (any T ≤ 4096, any D ≤ 64); AUTO's pick */
};

/* input sample formats (if_fir_set_input_format) */
enum
{
    IF_FIR_INPUT_F32 = 0, /* interleaved float32 I,Q (8 bytes per sample), the default                         */
    IF_FIR_INPUT_I16 = 1  /* interleaved int16 I,Q (4 bytes per sample), value = int16 * 2^-15  */
};

/* output sample formats of the real-output up-converter (if_fir_duc_set_output_format) */
enum
{
    IF_FIR_OUTPUT_F32 = 0, /* one float32 per real sample (4 bytes), the default                                         */
    IF_FIR_OUTPUT_I16 = 1  /* one int16 per real sample (2 bytes): the float32 result * 2^15, to nearest even, saturated */
};

/* window ids for if_bpf_design */
enum
{
    IF_BPF_WINDOW_RECT = 0,
    IF_BPF_WINDOW_HAMMING = 1,
    IF_BPF_WINDOW_HANN = 2,
    IF_BPF_WINDOW_BLACKMAN = 3
};

/* ---- tap generator (host, once; SPEC §4) ------------------------------------------------------ */
/* Windowed-sinc band-pass, odd ulTaps, band [dLow,dHigh] in cycles/sample (0 ≤ dLow < dHigh ≤ 0.5),
 * unity gain at the band centre.  Defaults used by the benchmarks: 0.15–0.25, Blackman. */
uint8_t if_bpf_design(float *pfTaps, uint32_t ulTaps, double dLow, double dHigh, uint32_t ulWindow);

/* Complex taps for channel selection (one-sided band-pass): low-pass prototype of two-sided bandwidth dBandwidth
 * shifted to dCentre (both in cycles/sample, |dCentre| ≤ 0.5); pfTapsIQ receives ulTaps interleaved (re, im) pairs. */
uint8_t if_bpf_design_complex(float *pfTapsIQ, uint32_t ulTaps, double dCentre, double dBandwidth, uint32_t ulWindow);

/* ---- context -------------------------------------------------------------------------------------------------- */
/* Copies the taps to the device, allocates history (and, for if_fir_process, staging buffers sized for
 * ullMaxSamples input samples per call).  lDevice = HIP device ordinal. */
uint8_t if_fir_init(if_fir_ctx_t **ppCtx, const float *pfTaps, uint32_t ulTaps, uint32_t ulDecimation,
                    uint64_t ullMaxSamples, int32_t lDevice);
/* Same with COMPLEX taps (ulTaps interleaved re,im pairs): y[n] = Σ g[k]·x[n-k].  Served by the overlap-save backend at
 * the speed of real taps (its transfer function is complex anyway) and by the generic kernel; the unrolled direct and
 * tap-split kernels take real taps only. */
uint8_t if_fir_init_complex(if_fir_ctx_t **ppCtx, const float *pfTapsIQ, uint32_t ulTaps, uint32_t ulDecimation,
                            uint64_t ullMaxSamples, int32_t lDevice);
void if_fir_destroy(if_fir_ctx_t *pCtx);
/* zero the history and the decimation phase */
uint8_t if_fir_reset(if_fir_ctx_t *pCtx);
uint8_t if_fir_set_backend(if_fir_ctx_t *pCtx, uint32_t ulBackend);
uint32_t if_fir_get_backend(const if_fir_ctx_t *pCtx); /* the resolved (non-AUTO) backend */
/* Input sample format: IF_FIR_INPUT_F32 (default) or IF_FIR_INPUT_I16 (pfIQIn / pDevIn then point at int16 pairs; the
 * conversion is fused into the kernels' loads; overlap-save and generic backends).  Outputs stay float32. */
uint8_t if_fir_set_input_format(if_fir_ctx_t *pCtx, uint32_t ulFormat);
/* NCO fused into the filter (docs/SPEC.md §3.2): the input is mixed with exp(-j*2*pi*f*a), a = absolute
 * sample index since init/reset, f quantised to a 32-bit phase word (if_fir_get_nco returns the value applied).
 * dFreq in cycles/sample, |dFreq| <= 0.5; 0 switches the NCO off.  Takes effect from the next call, as if it had been
 * set since the last reset (the phase is a function of the absolute index).  Overlap-save and generic kernels only. */
uint8_t if_fir_set_nco(if_fir_ctx_t *pCtx, double dFreq);
uint8_t if_fir_get_nco(const if_fir_ctx_t *pCtx, double *pdFreq);
/* expert knob: pick a schedule variant of the direct-form kernels (0 = default, 1..6: workgroup kernel v1 in
 * three tile shapes, the wave kernel with 8- or 16-byte LDS reads and 2 / 4 / 8 tiles per run).  Variants change
 * speed only.  Everything else (diagnostic launches, grid limits, test hooks) lives in the development library, see
 * if_fir_debug.h.
 * Environment: IF_FIR_RCCL_LIBRARY = path of the library providing the nccl* entry points of the multi-channel front
 * (default: librccl.so.1 by name); IF_FIR_MC_TIMEOUT_S = seconds a rank waits for its peers' transfers (default 300). */
uint8_t if_fir_set_tuning(if_fir_ctx_t *pCtx, uint32_t ulVariant);
/* (calls on a stream that is being captured into a hipGraph are refused: the streaming state advances on the host) */
/* run on a caller-owned HIP stream (pass a hipStream_t as void*; NULL = the context's own stream) */
uint8_t if_fir_set_stream(if_fir_ctx_t *pCtx, void *pStream);
/* waits for the context's stream; also fails (0 + message) if the overlap-save kernel's block queue reported an expired
 * bounded wait since the last check -- outputs would then be incomplete; it never should */
uint8_t if_fir_synchronize(if_fir_ctx_t *pCtx);
/* last error message of this context (or of the failed if_fir_init when pCtx is NULL); never NULL */
const char *if_fir_last_error(const if_fir_ctx_t *pCtx);

/* number of output samples a call with ullSamples inputs will produce in the current phase */
uint64_t if_fir_out_count(const if_fir_ctx_t *pCtx, uint64_t ullSamples);

/* ---- filtering ------------------------------------------------------------------------------------------------ */
/* Host pointers: H2D copy + kernel + D2H copy, synchronous.  ullSamples ≤ ullMaxSamples of init. */
uint8_t if_fir_process(if_fir_ctx_t *pCtx, const float *pfIQIn, float *pfIQOut, uint64_t ullSamples,
                       uint64_t *pullOutSamples);
/* Device pointers, 16-byte aligned (the overlap-save backend, AUTO's pick, also takes pointers aligned to one sample:
 * 8 bytes, 4 for int16 input), asynchronous on the context's stream; what the benchmark times.
 * pDevOut must hold if_fir_out_count() samples. */
uint8_t if_fir_process_device(if_fir_ctx_t *pCtx, const void *pDevIn, void *pDevOut, uint64_t ullSamples,
                              uint64_t *pullOutSamples);

/* ---- device-side utilities used by benchmarks and tests ------------------------------------------------------ */
/* Fill pDevIQ with the SPEC §5 synthetic stream of channel ulChannel, samples [ullFirst, ullFirst+ullSamples). */
uint8_t if_fir_synth_device(if_fir_ctx_t *pCtx, void *pDevIQ, uint64_t ullFirst, uint64_t ullSamples,
                            uint32_t ulChannel);
/* Device memory helpers so that a pure-C host needs no HIP headers. */
/* mean(|y|^2) of a device IQ buffer (float32 I,Q), accumulated in float64; synchronous.  The measurement side of a
 * level-control loop; writing the attenuator register stays with the rack controller's daemon. */
uint8_t if_fir_power_device(if_fir_ctx_t *pCtx, const void *pDevIQ, uint64_t ullSamples, double *pdMeanPower);
/* page-locked host memory (hipHostMalloc) for the buffers of if_fir_process: the copies then run at PCIe speed and
 * overlap the kernels; ordinary (pageable) buffers work too, more slowly */
uint8_t if_fir_host_alloc(if_fir_ctx_t *pCtx, void **ppHost, uint64_t ullBytes);
uint8_t if_fir_host_free(if_fir_ctx_t *pCtx, void *pHost);
uint8_t if_fir_dev_alloc(if_fir_ctx_t *pCtx, void **ppDev, uint64_t ullBytes);
uint8_t if_fir_dev_free(if_fir_ctx_t *pCtx, void *pDev);
uint8_t if_fir_dev_upload(if_fir_ctx_t *pCtx, void *pDev, const void *pHost, uint64_t ullBytes);
uint8_t if_fir_dev_download(if_fir_ctx_t *pCtx, void *pHost, const void *pDev, uint64_t ullBytes);
/* "gfx950", CU count, etc.: writes a short description of the context's device */
uint8_t if_fir_device_info(const if_fir_ctx_t *pCtx, char *pszOut, uint32_t ulOutBytes);

/* ---- uniform filter bank (BUILD-DEFINED) -----------------------------------------------------------
 * Channel c = mix-down by pulSlots[c]/16 cycles/sample, the context's prototype taps (real or complex), decimation by the
 * context's decimation: the result of ulChannels contexts with if_fir_set_nco(slot/16.0), computed in ONE pass over the input.
 * The context must have <= 3073 taps, float32 or int16 input, run on the overlap-save backend and have decimation 4 (fs/16
 * channels 4x oversampled; no NCO), 8 (2x oversampled) or 16 (the channel rate: all 16 slots come out of one
 * forward transform; the wanted ones are stored); every other multiple of 4 up to 64 is served through the per-channel forms
 * of if_fir_channelizer_process_device_freq (slot s = centre s/16).  At decimation 8 and 16 the context may carry an NCO: it shifts the WHOLE
 * slot grid (channel c is centred at pulSlots[c]/16 + f_nco: a common fine offset).
 * The context's streaming state (history, decimation phase, sample index) is shared
 * by all channels.  ulChannels 1..16, slots 0..15: any subset, repeats allowed (decimation 16: each slot at most once);
 * ppDevOut[c]: 16-byte aligned device buffers of if_fir_out_count() samples each.  Asynchronous on the context's stream
 * like if_fir_process_device.  (Decimation 8, no NCO on the context: four or more channels on even -- or on odd -- slots, no
 * slot listed twice, are computed together from one pair of 8-point transforms per group, whatever their number; a call is then
 * up to two kernel launches on the context's stream.  Results do not depend on the route beyond float32 rounding.) */
uint8_t if_fir_channelizer_process_device(if_fir_ctx_t *pCtx, uint32_t ulChannels, const uint32_t *pulSlots,
                                          const void *pDevIn, void *const *ppDevOut, uint64_t ullSamples,
                                          uint64_t *pullOutSamples);
/* Channels at ARBITRARY centre frequencies from one pass over the input (round 4; decimation 4, 8, 12, ..., 64 -- any multiple of 4 --,
 * context without NCO, real or complex prototype taps, float32 or int16 input).  Channel c = the prototype centred at pdCentre[c] cycles/sample
 * (|pdCentre[c]| <= 0.5), mixed down and decimated by the context's decimation:
 *     y_c[m] = exp(-j 2 pi f_c a) * sum_k h[k] exp(+j 2 pi g_c k) x[a - k],   a = absolute index of the output's input sample,
 * with g_c = the multiple of 1/4096 nearest to f_c (the overlap-save kernel moves the prototype's response by whole bins of its
 * 4096-point transform) and f_c quantised to a 32-bit phase word like if_fir_set_nco.  For centres on the 1/4096 grid this is
 * exactly what ulChannels contexts with if_fir_set_nco(f_c) compute; off the grid the filter sits at most 1/8192 cycles/sample
 * (0.4 % of a slot) beside the centre the output is mixed to.  Everything else as if_fir_channelizer_process_device
 * (slot s of that call = centre s/16 here). */
uint8_t if_fir_channelizer_process_device_freq(if_fir_ctx_t *pCtx, uint32_t ulChannels, const double *pdCentre,
                                               const void *pDevIn, void *const *ppDevOut, uint64_t ullSamples,
                                               uint64_t *pullOutSamples);

/* ---- multi-channel front (BUILD-DEFINED, the reference has no filter surface) -------------------
 * One process per GPU.  Channel c is filtered by rank if_fir_mc_owner(c, world) = c mod world with its own taps and
 * its own streaming state.  The channel inputs and outputs live on rank 0's GPU; if_fir_mc_process_device() is called
 * by EVERY rank with the same ullSamples and moves them itself in chunks of ~2^24 samples: grouped RCCL sends root ->
 * owners on a transfer stream, the filters of a chunk on a second stream once it has landed, its outputs owners -> root
 * behind the next chunk's scatter; a status word per owner tells the root about a remote filter failure (nobody is left
 * waiting).  With ulWorld == 1 nothing is moved and librccl is never loaded.
 * Bootstrap: rank 0 calls if_fir_mc_unique_id(), the host program hands the 128 bytes to the other ranks by whatever
 * means it has (MPI, a socket, torch.distributed, a file), every rank passes them to if_fir_mc_init().
 * Errors: 0 + if_fir_mc_last_error(); the context stays valid.  Not re-entrant per context. */
typedef struct if_fir_mc_ctx if_fir_mc_ctx_t;
#define IF_FIR_MC_ID_BYTES 128u

uint32_t if_fir_mc_owner(uint32_t ulChannel, uint32_t ulWorld);
uint8_t if_fir_mc_unique_id(uint8_t *pubId /* IF_FIR_MC_ID_BYTES */);
/* pfTaps: ulChannels rows of ulTaps real float32 taps.  ullMaxSamples > 0: per-call limit.  Ranks other than 0 stage two
 * chunks per owned channel (not the whole call).  pubId may be NULL when ulWorld == 1. */
uint8_t if_fir_mc_init(if_fir_mc_ctx_t **ppCtx, uint32_t ulChannels, const float *pfTaps, uint32_t ulTaps,
                       uint32_t ulDecimation, uint64_t ullMaxSamples, int32_t lDevice, uint32_t ulRank,
                       uint32_t ulWorld, const uint8_t *pubId);
void if_fir_mc_destroy(if_fir_mc_ctx_t *pCtx);
uint8_t if_fir_mc_reset(if_fir_mc_ctx_t *pCtx);
/* all channels take IF_FIR_INPUT_F32 or IF_FIR_INPUT_I16 samples (every rank must make the same call) */
uint8_t if_fir_mc_set_input_format(if_fir_mc_ctx_t *pCtx, uint32_t ulFormat);
/* rank 0: ppDevIn[c] / ppDevOut[c] = device pointers on rank 0's GPU for every channel; other ranks may pass NULL.
 * Synchronous: returns when this rank's part (transfers and filters) has finished.  *pullOutSamples: per channel.
 * A failing filter on any rank (or an expired wait of its block queue) makes the call fail on that rank AND on rank 0 (the other ranks complete normally; the
 * transfer protocol is always run to its end, nobody is left waiting); the channel streams are then out of step:
 * call if_fir_mc_reset() on every rank before the next call.  After an RCCL failure the communicator is aborted and the
 * context refuses further calls (destroy it and create a new one); the peers notice through the communicator's
 * asynchronous error state, which their waits poll, or at the latest after IF_FIR_MC_TIMEOUT_S seconds (best effort:
 * the failure paths have run against a stand-in transport only; the protocol itself also over the real librccl in
 * loopback, one process playing all ranks -- no multi-GPU node was available to the build). */
uint8_t if_fir_mc_process_device(if_fir_mc_ctx_t *pCtx, const void *const *ppDevIn, void *const *ppDevOut,
                                 uint64_t ullSamples, uint64_t *pullOutSamples);
/* chunk length of the following calls: 0 = default (about 2^24 samples; with one rank: never split), UINT64_MAX = never split,
 * otherwise a request in samples.  The library rounds the request to the nearest multiple of the context's UNIT = lcm(block
 * advance of the filter's overlap-save kernel -- 3840, 3584, 3072, 2048 or 1024 samples --, twice the decimation) and,
 * where the kernel's block grid follows the decimation phase (every even decimation), makes the first chunk of an off-phase call
 * that many samples longer: the blocks of a chunked call are then the blocks of an unchunked one and the results are
 * bit-identical whatever the chunk and whatever the phase.  Calls are split on the overlap-save backend (AUTO's pick) only: with a
 * channel switched to another backend a call that would be split is refused.  Every rank must make the same call.
 * if_fir_mc_get_chunk_samples reports the chunk in effect (0 = not split) and the unit. */
uint8_t if_fir_mc_set_chunk_samples(if_fir_mc_ctx_t *pCtx, uint64_t ullChunk);
uint8_t if_fir_mc_get_chunk_samples(const if_fir_mc_ctx_t *pCtx, uint64_t *pullChunk, uint64_t *pullUnit);
/* the single-channel context behind a channel this rank owns (NULL otherwise), e.g. for if_fir_set_backend() */
if_fir_ctx_t *if_fir_mc_channel_ctx(if_fir_mc_ctx_t *pCtx, uint32_t ulChannel);
const char *if_fir_mc_last_error(const if_fir_mc_ctx_t *pCtx);

/* ---- interpolator (docs/SPEC.md §6; BUILD-DEFINED) ---------------------------------------------------------------------
 * The transmit direction: upsample by L (1..64), filter, and optionally mix UP:
 *     u[n] = x[n/L] if n mod L == 0, else 0;   y[n] = sum_k h[k] u[n-k];   y'[n] = exp(+j*2*pi*P*n/2^32) y[n]
 * n = absolute OUTPUT index since init/reset.  A call with N input samples emits exactly N*L outputs (no phase is carried:
 * process(a||b) == process(a); process(b)).  Taps are used as given: image-rejection taps need a gain of L.  Real or complex
 * taps, T <= 4096; float32 or int16 input (if_fir_interp_set_input_format); float32 I/Q output.
 * Backends: IF_FIR_BACKEND_HIP_FFT (AUTO's pick for L in {1, 2, 4, ..., 64} and T <= 3073: overlap-save) and
 * IF_FIR_BACKEND_HIP_GENERIC (any L and T: one output per thread); others are refused.  Errors: 0 + if_fir_interp_last_error();
 * the context stays usable.  Calls on a stream that is being captured into a hipGraph are refused. */
typedef struct if_fir_interp if_fir_interp_t;
#define IF_FIR_MAX_INTERPOLATION 64u

uint8_t if_fir_interp_init(if_fir_interp_t **ppCtx, const float *pfTaps, uint32_t ulTaps, uint32_t ulInterpolation,
                           uint64_t ullMaxSamples, int32_t lDevice);
/* complex taps: ulTaps interleaved (re, im) pairs */
uint8_t if_fir_interp_init_complex(if_fir_interp_t **ppCtx, const float *pfTapsIQ, uint32_t ulTaps, uint32_t ulInterpolation,
                                   uint64_t ullMaxSamples, int32_t lDevice);
void if_fir_interp_destroy(if_fir_interp_t *pCtx);
/* zero the history and the output index */
uint8_t if_fir_interp_reset(if_fir_interp_t *pCtx);
uint8_t if_fir_interp_set_backend(if_fir_interp_t *pCtx, uint32_t ulBackend);
uint32_t if_fir_interp_get_backend(const if_fir_interp_t *pCtx); /* the resolved (non-AUTO) backend */
uint8_t if_fir_interp_set_input_format(if_fir_interp_t *pCtx, uint32_t ulFormat);
/* NCO as an UP-mix of the output: y'[n] = exp(+j*2*pi*f*n) y[n], n = absolute output index (mod 2^32), f quantised to a 32-bit
 * phase word as in if_fir_set_nco.  Note the sign: if_fir_set_nco mixes the decimator's INPUT DOWN with exp(-j*2*pi*f*a).
 * |dFreq| <= 0.5; 0 switches it off; takes effect from the next call as if set since the last reset. */
uint8_t if_fir_interp_set_nco(if_fir_interp_t *pCtx, double dFreq);
uint8_t if_fir_interp_get_nco(const if_fir_interp_t *pCtx, double *pdFreq);
uint8_t if_fir_interp_set_stream(if_fir_interp_t *pCtx, void *pStream);
uint8_t if_fir_interp_synchronize(if_fir_interp_t *pCtx);
const char *if_fir_interp_last_error(const if_fir_interp_t *pCtx);
/* = ullSamples * L */
uint64_t if_fir_interp_out_count(const if_fir_interp_t *pCtx, uint64_t ullSamples);
/* host pointers, synchronous; ullSamples <= ullMaxSamples of init; pfIQOut holds ullSamples * L samples */
uint8_t if_fir_interp_process(if_fir_interp_t *pCtx, const void *pIQIn, float *pfIQOut, uint64_t ullSamples,
                              uint64_t *pullOutSamples);
/* device pointers, asynchronous on the context's stream.  Overlap-save backend: aligned to one sample (input 8 bytes, 4 for
 * int16; output 8 bytes); generic backend: 16 bytes.  pDevOut holds ullSamples * L samples. */
uint8_t if_fir_interp_process_device(if_fir_interp_t *pCtx, const void *pDevIn, void *pDevOut, uint64_t ullSamples,
                                     uint64_t *pullOutSamples);

/* ---- channel combiner (docs/SPEC.md §9; BUILD-DEFINED) --------------------------------------------------------------------
 * The transmit counterpart of the channelizer: C baseband streams (1..64), each interpolated by L (1..64) with ONE prototype
 * filter and mixed UP to its own centre, summed into one stream in one pass:
 *     u_c[n] = x_c[n/L] if n mod L == 0, else 0;   y[n] = sum_c exp(+j*2*pi*P_c*n/2^32) sum_k h[k] u_c[n-k]
 * n = absolute OUTPUT index since init/reset (mod 2^32 in the rotation), P_c = centre c quantised to a 32-bit phase word as the
 * interpolator's NCO: what C interpolator contexts with their NCOs at the centres compute, added.  A call brings N samples for
 * EVERY channel and emits exactly N*L outputs; process(a||b) == process(a); process(b) within the SPEC tolerance wherever the
 * stream is cut.  Taps are used as given (image rejection needs a gain of L); real or complex, T <= 4096; float32 or int16 input,
 * the same for all channels; float32 I/Q output.  Two channels may share a centre; a centre of 0 means no rotation.
 * Backends: IF_FIR_BACKEND_HIP_FFT (AUTO's pick for L in {4, 8, 16, 32, 64} and T <= 3073: overlap-save, one inverse transform
 * and one store for all channels) and IF_FIR_BACKEND_HIP_GENERIC (any L, T and C: one output per thread); others are refused.
 * Errors: 0 + if_fir_combiner_last_error(); a failed call leaves the context usable and its stream position unchanged.  Calls on
 * a stream that is being captured into a hipGraph are refused. */
typedef struct if_fir_combiner if_fir_combiner_t;
#define IF_FIR_COMBINER_MAX_CHANNELS 64u

/* pdCentre: ulChannels centres in cycles per OUTPUT sample, |f| <= 0.5 */
uint8_t if_fir_combiner_init(if_fir_combiner_t **ppCtx, const float *pfTaps, uint32_t ulTaps, uint32_t ulInterpolation,
                             uint32_t ulChannels, const double *pdCentre, uint64_t ullMaxSamples, int32_t lDevice);
/* complex taps: ulTaps interleaved (re, im) pairs */
uint8_t if_fir_combiner_init_complex(if_fir_combiner_t **ppCtx, const float *pfTapsIQ, uint32_t ulTaps, uint32_t ulInterpolation,
                                     uint32_t ulChannels, const double *pdCentre, uint64_t ullMaxSamples, int32_t lDevice);
void if_fir_combiner_destroy(if_fir_combiner_t *pCtx);
/* zero every channel's history and the output index */
uint8_t if_fir_combiner_reset(if_fir_combiner_t *pCtx);
uint8_t if_fir_combiner_set_backend(if_fir_combiner_t *pCtx, uint32_t ulBackend);
uint32_t if_fir_combiner_get_backend(const if_fir_combiner_t *pCtx); /* the resolved (non-AUTO) backend */
/* IF_FIR_INPUT_F32 or IF_FIR_INPUT_I16 (value = int16 * 2^-15); the histories are float32, so a change keeps the stream */
uint8_t if_fir_combiner_set_input_format(if_fir_combiner_t *pCtx, uint32_t ulFormat);
/* all centres at once; takes effect from the next call as if set since the last reset (phase-continuous in n).  Waits for the
 * context's stream (the multiply tables are rebuilt and uploaded). */
uint8_t if_fir_combiner_set_centres(if_fir_combiner_t *pCtx, const double *pdCentre);
/* the quantised centres, ulChannels values */
uint8_t if_fir_combiner_get_centres(const if_fir_combiner_t *pCtx, double *pdCentre);
uint8_t if_fir_combiner_set_stream(if_fir_combiner_t *pCtx, void *pStream);
uint8_t if_fir_combiner_synchronize(if_fir_combiner_t *pCtx);
const char *if_fir_combiner_last_error(const if_fir_combiner_t *pCtx);
/* = ullSamples * L */
uint64_t if_fir_combiner_out_count(const if_fir_combiner_t *pCtx, uint64_t ullSamples);
/* host pointers, synchronous: ppIQIn[c] = ullSamples samples of channel c; ullSamples <= ullMaxSamples of init; pfIQOut holds
 * ullSamples * L samples */
uint8_t if_fir_combiner_process(if_fir_combiner_t *pCtx, const void *const *ppIQIn, float *pfIQOut, uint64_t ullSamples,
                                uint64_t *pullOutSamples);
/* ppDevIn: a HOST array of ulChannels device pointers (handed to the kernel by value: the call makes no allocation, copy or
 * synchronise of its own); asynchronous on the context's stream.  Alignment as the interpolator's: overlap-save backend one
 * sample (input 8 bytes, 4 for int16; output 8 bytes), generic backend 16 bytes.  pDevOut holds ullSamples * L samples. */
uint8_t if_fir_combiner_process_device(if_fir_combiner_t *pCtx, const void *const *ppDevIn, void *pDevOut, uint64_t ullSamples,
                                       uint64_t *pullOutSamples);

/* ---- rational resampler (docs/SPEC.md §7; BUILD-DEFINED) -----------------------------------------------------------------
 * Changes a stream's rate by L/M (L, M in 1..64, used as given: a common factor is legal) in ONE polyphase pass:
 *     u[n] = x[n/L] if n mod L == 0, else 0;   v[n] = sum_k h[k] u[n-k];   y[m] = v[m*M]
 * n = index at the L-times rate, m = absolute OUTPUT index, both since init/reset.  A call whose first input has absolute index
 * c and which brings N inputs emits exactly the outputs m with c*L <= m*M < (c+N)*L: ceil((c+N)*L/M) - ceil(c*L/M) of them,
 * possibly none when L < M.  process(a||b) == process(a); process(b), bit for bit, wherever the stream is cut.  Taps are used as
 * given (an image-rejection low-pass needs a gain of L); real or complex, T <= 4096; float32 or int16 input; float32 I/Q output.
 * No NCO.  Errors: 0 + if_fir_resamp_last_error(); a failed call leaves the context usable and its stream position unchanged.
 * Calls on a stream that is being captured into a hipGraph are refused. */
typedef struct if_fir_resamp if_fir_resamp_t;

uint8_t if_fir_resamp_init(if_fir_resamp_t **ppCtx, const float *pfTaps, uint32_t ulTaps, uint32_t ulInterpolation,
                           uint32_t ulDecimation, uint64_t ullMaxSamples, int32_t lDevice);
/* complex taps: ulTaps interleaved (re, im) pairs */
uint8_t if_fir_resamp_init_complex(if_fir_resamp_t **ppCtx, const float *pfTapsIQ, uint32_t ulTaps, uint32_t ulInterpolation,
                                   uint32_t ulDecimation, uint64_t ullMaxSamples, int32_t lDevice);
void if_fir_resamp_destroy(if_fir_resamp_t *pCtx);
/* zero the history and the stream position */
uint8_t if_fir_resamp_reset(if_fir_resamp_t *pCtx);
/* IF_FIR_INPUT_F32 or IF_FIR_INPUT_I16 (value = int16 * 2^-15); the history is float32, so a change keeps the stream */
uint8_t if_fir_resamp_set_input_format(if_fir_resamp_t *pCtx, uint32_t ulFormat);
uint8_t if_fir_resamp_set_stream(if_fir_resamp_t *pCtx, void *pStream);
uint8_t if_fir_resamp_synchronize(if_fir_resamp_t *pCtx);
const char *if_fir_resamp_last_error(const if_fir_resamp_t *pCtx);
/* outputs of a call with ullSamples inputs at the current stream position */
uint64_t if_fir_resamp_out_count(const if_fir_resamp_t *pCtx, uint64_t ullSamples);
/* host pointers, synchronous; ullSamples <= ullMaxSamples of init; pfIQOut holds if_fir_resamp_out_count() samples */
uint8_t if_fir_resamp_process(if_fir_resamp_t *pCtx, const void *pIQIn, float *pfIQOut, uint64_t ullSamples,
                              uint64_t *pullOutSamples);
/* device pointers aligned to one sample (input 8 bytes, 4 for int16; output 8 bytes), asynchronous on the context's stream;
 * pDevOut holds if_fir_resamp_out_count() samples */
uint8_t if_fir_resamp_process_device(if_fir_resamp_t *pCtx, const void *pDevIn, void *pDevOut, uint64_t ullSamples,
                                     uint64_t *pullOutSamples);

/* ---- streaming power-spectrum estimator (docs/SPEC.md §8; BUILD-DEFINED) ---------------------------------------------------
 * Averaged periodogram (Welch) of a complex IQ stream with the WB detector's dB-to-code scale: IQ in, frames of uint16 spectrum
 * bins out, in the layout wb_detect_frames_device() reads.  Segment s covers stream samples [s*H, s*H + N); frame f is made of
 * segments f*K .. f*K + K - 1:
 *     S_s[k] = |sum_n w[n] x[s*H + n] e^(-2 pi i k n / N)|^2,   P[k] = (sum_s S_s[k]) / (K * sum_n w[n]^2)
 *     code   = clamp(rint((10 log10(P / fRefPower) + 3.35) / ((16.7 + 3.35) / 65535)), 0, 65535);   P = 0 gives code 0
 * Output bin j is FFT bin (lFirstBin + j) mod N, -N/2 <= lFirstBin, lFirstBin + ulBins <= N/2.  A frame's segments are summed in
 * float32 in chunks of 8 (SPEC §8), so process(a||b) == process(a); process(b), bit for bit in both outputs, wherever the stream
 * is cut.  A call emits the frames whose last segment it completes.  Errors: 0 + if_fir_psd_last_error(); a failed call leaves
 * the context usable and its stream position unchanged.  Calls on a stream that is being captured into a hipGraph are refused. */
typedef struct if_fir_psd if_fir_psd_t;

typedef struct
{
    uint32_t ulSize;        /* N: 256, 512, 1024, 2048 or 4096 */
    uint32_t ulHop;         /* H: 1..N */
    uint32_t ulSegments;    /* K: segments averaged per frame, 1..65535 */
    int32_t lFirstBin;      /* first output bin, relative to DC */
    uint32_t ulBins;        /* output bins, 1..N */
    float fRefPower;        /* > 0 */
    uint32_t ulInputFormat; /* IF_FIR_INPUT_F32 or IF_FIR_INPUT_I16 (value = int16 * 2^-15) */
} if_fir_psd_config_t;

/* pfWindow: N float32 values, or NULL = the periodic Hann window 0.5 - 0.5 cos(2 pi n / N), computed in float64 and rounded once.
 * ullMaxSamples: the most samples of one call; it sizes the context's work buffer (one float32 per bin and chunk of a call) */
uint8_t if_fir_psd_init(if_fir_psd_t **ppCtx, const if_fir_psd_config_t *pCfg, const float *pfWindow, uint64_t ullMaxSamples,
                        int32_t lDevice);
void if_fir_psd_destroy(if_fir_psd_t *pCtx);
/* back to stream position 0: no samples and no accumulator carried */
uint8_t if_fir_psd_reset(if_fir_psd_t *pCtx);
/* the carried samples are float32, so a change keeps the stream */
uint8_t if_fir_psd_set_input_format(if_fir_psd_t *pCtx, uint32_t ulFormat);
uint8_t if_fir_psd_set_stream(if_fir_psd_t *pCtx, void *pStream);
uint8_t if_fir_psd_synchronize(if_fir_psd_t *pCtx);
const char *if_fir_psd_last_error(const if_fir_psd_t *pCtx);
/* frames a call with ullSamples samples would emit at the current stream position */
uint64_t if_fir_psd_frame_count(const if_fir_psd_t *pCtx, uint64_t ullSamples);
/* host pointers, synchronous; ullSamples <= ullMaxSamples of init.  pusBins holds if_fir_psd_frame_count() x ulBins codes, pfPower
 * (may be NULL) as many float32 P; *pulFrames (may be NULL) receives the frames emitted */
uint8_t if_fir_psd_process(if_fir_psd_t *pCtx, const void *pIQIn, uint64_t ullSamples, uint16_t *pusBins, float *pfPower,
                           uint32_t *pulFrames);
/* device pointers aligned to one element (input 8 bytes, 4 for int16), asynchronous on the context's stream */
uint8_t if_fir_psd_process_device(if_fir_psd_t *pCtx, const void *pDevIn, uint64_t ullSamples, uint16_t *pusDevBins, float *pfDevPower,
                                  uint32_t *pulFrames);

/* ---- real-input down-converter (docs/SPEC.md §10; BUILD-DEFINED) -----------------------------------------------------------
 * Real IF samples r[a] (one float32, or one int16 = value * 2^15, per sample) to decimated complex baseband in ONE pass:
 *     x'[a] = r[a] exp(-j 2 pi ((P a) mod 2^32) / 2^32);   y[n] = sum_k h[k] x'[n-k];   y_D[m] = y[m*D]
 * a, n = absolute index since init/reset, P = round(f * 2^32) mod 2^32 (if_fir_ddc_set_nco; P = 0: no mixing): by definition the
 * decimator with if_fir_set_nco fed (r, 0).  D in 1..64, T <= 4096, taps real or complex.  A call whose first sample has absolute
 * index c and which brings N samples emits the outputs with n in [c, c+N), n mod D == 0 (possibly none).
 * process(a||b) == process(a); process(b), bit for bit, wherever the stream is cut.  Output float32 I/Q.
 * Errors: 0 + if_fir_ddc_last_error(); a failed call leaves the context usable and its stream position unchanged.
 * Calls on a stream that is being captured into a hipGraph are refused. */
typedef struct if_fir_ddc if_fir_ddc_t;

uint8_t if_fir_ddc_init(if_fir_ddc_t **ppCtx, const float *pfTaps, uint32_t ulTaps, uint32_t ulDecimation, uint64_t ullMaxSamples,
                        int32_t lDevice);
/* complex taps: ulTaps interleaved (re, im) pairs */
uint8_t if_fir_ddc_init_complex(if_fir_ddc_t **ppCtx, const float *pfTapsIQ, uint32_t ulTaps, uint32_t ulDecimation,
                                uint64_t ullMaxSamples, int32_t lDevice);
void if_fir_ddc_destroy(if_fir_ddc_t *pCtx);
/* zero the history and the stream position (the NCO frequency stays) */
uint8_t if_fir_ddc_reset(if_fir_ddc_t *pCtx);
/* IF_FIR_INPUT_F32 (4 bytes per sample) or IF_FIR_INPUT_I16 (2 bytes, value = int16 * 2^-15); the history is float32, so a
 * change keeps the stream */
uint8_t if_fir_ddc_set_input_format(if_fir_ddc_t *pCtx, uint32_t ulFormat);
/* dFreq in cycles/sample, |dFreq| <= 0.5; holds from the next call as if set since the last reset (the phase is a function of
 * the absolute index only).  Waits for the context's stream. */
uint8_t if_fir_ddc_set_nco(if_fir_ddc_t *pCtx, double dFreq);
/* the quantised frequency P / 2^32, P read as a signed word */
uint8_t if_fir_ddc_get_nco(const if_fir_ddc_t *pCtx, double *pdFreq);
uint8_t if_fir_ddc_set_stream(if_fir_ddc_t *pCtx, void *pStream);
uint8_t if_fir_ddc_synchronize(if_fir_ddc_t *pCtx);
const char *if_fir_ddc_last_error(const if_fir_ddc_t *pCtx);
/* outputs of a call with ullSamples inputs at the current stream position */
uint64_t if_fir_ddc_out_count(const if_fir_ddc_t *pCtx, uint64_t ullSamples);
/* host pointers, synchronous; ullSamples <= ullMaxSamples of init; pfIQOut holds if_fir_ddc_out_count() samples */
uint8_t if_fir_ddc_process(if_fir_ddc_t *pCtx, const void *pIn, float *pfIQOut, uint64_t ullSamples, uint64_t *pullOutSamples);
/* device pointers aligned to one sample (input 4 bytes, 2 for int16; output 8 bytes), asynchronous on the context's stream;
 * pDevOut holds if_fir_ddc_out_count() samples */
uint8_t if_fir_ddc_process_device(if_fir_ddc_t *pCtx, const void *pDevIn, void *pDevOut, uint64_t ullSamples,
                                  uint64_t *pullOutSamples);

/* ---- real-output up-converter (docs/SPEC.md §11; BUILD-DEFINED) --------------------------------------------------------------
 * Complex baseband x[n] to a REAL IF stream at L times the rate in ONE pass, the stage in front of a DAC:
 *     u[m] = x[m/L] if m mod L == 0 else 0;   v[m] = sum_k h[k] u[m-k];   y[m] = Re{ exp(+j 2 pi ((P m) mod 2^32) / 2^32) v[m] }
 * m = absolute OUTPUT index since init/reset, P = round(f * 2^32) mod 2^32 (if_fir_duc_set_nco; P = 0: no mixing): by definition
 * the interpolator with if_fir_interp_set_nco followed by the real part.  L in 1..64, T <= 4096, taps real or complex.  A call
 * with N inputs emits exactly N*L outputs.  process(a||b) == process(a); process(b), bit for bit, wherever the stream is cut.
 * Errors: 0 + if_fir_duc_last_error(); a failed call leaves the context usable and its stream position unchanged.
 * Calls on a stream that is being captured into a hipGraph are refused. */
typedef struct if_fir_duc if_fir_duc_t;

uint8_t if_fir_duc_init(if_fir_duc_t **ppCtx, const float *pfTaps, uint32_t ulTaps, uint32_t ulInterpolation, uint64_t ullMaxSamples,
                        int32_t lDevice);
/* complex taps: ulTaps interleaved (re, im) pairs */
uint8_t if_fir_duc_init_complex(if_fir_duc_t **ppCtx, const float *pfTapsIQ, uint32_t ulTaps, uint32_t ulInterpolation,
                                uint64_t ullMaxSamples, int32_t lDevice);
void if_fir_duc_destroy(if_fir_duc_t *pCtx);
/* zero the history and the stream position (the NCO frequency and the formats stay) */
uint8_t if_fir_duc_reset(if_fir_duc_t *pCtx);
/* IF_FIR_INPUT_F32 (8 bytes per sample) or IF_FIR_INPUT_I16 (4 bytes, value = int16 * 2^-15); the history is float32, so a
 * change keeps the stream */
uint8_t if_fir_duc_set_input_format(if_fir_duc_t *pCtx, uint32_t ulFormat);
/* IF_FIR_OUTPUT_F32 (4 bytes per sample, the default) or IF_FIR_OUTPUT_I16 (2 bytes: the same float32 result * 2^15, rounded
 * to nearest even, saturated to -32768..32767); a change keeps the stream */
uint8_t if_fir_duc_set_output_format(if_fir_duc_t *pCtx, uint32_t ulFormat);
/* dFreq in cycles per OUTPUT sample, |dFreq| <= 0.5; holds from the next call as if set since the last reset (the phase is a
 * function of the absolute index only).  Waits for the context's stream. */
uint8_t if_fir_duc_set_nco(if_fir_duc_t *pCtx, double dFreq);
/* the quantised frequency P / 2^32, P read as a signed word */
uint8_t if_fir_duc_get_nco(const if_fir_duc_t *pCtx, double *pdFreq);
uint8_t if_fir_duc_set_stream(if_fir_duc_t *pCtx, void *pStream);
uint8_t if_fir_duc_synchronize(if_fir_duc_t *pCtx);
const char *if_fir_duc_last_error(const if_fir_duc_t *pCtx);
/* outputs of a call with ullSamples inputs: ullSamples * L (0 where the stream position would pass 2^64 outputs) */
uint64_t if_fir_duc_out_count(const if_fir_duc_t *pCtx, uint64_t ullSamples);
/* host pointers, synchronous; ullSamples <= ullMaxSamples of init; pOut holds if_fir_duc_out_count() float32 or int16 */
uint8_t if_fir_duc_process(if_fir_duc_t *pCtx, const void *pIQIn, void *pOut, uint64_t ullSamples, uint64_t *pullOutSamples);
/* device pointers aligned to one element (input 8 bytes, 4 for int16; output 4 bytes, 2 for int16), asynchronous on the
 * context's stream; pDevOut holds if_fir_duc_out_count() elements */
uint8_t if_fir_duc_process_device(if_fir_duc_t *pCtx, const void *pDevIn, void *pDevOut, uint64_t ullSamples,
                                  uint64_t *pullOutSamples);

/* ---- arbitrary-ratio resampler with a retunable step (docs/SPEC.md §12; BUILD-DEFINED) ---------------------------------------
 * Changes a stream's rate by ANY ratio in the range below, and lets the ratio be nudged between calls without restarting the
 * stream.  The prototype h[0..T-1] (real float32, T <= 8192) is designed at P = 2^ulPhaseBits times the input rate (4 <=
 * ulPhaseBits <= 10) and is used as given: unity pass-band gain needs sum h = P.  K = ceil(T/P) taps per phase.  The step
 * ullStep = R is input samples per output sample times 2^32, 2^26 <= R <= 2^34 (ratios 1/64 .. 4).  The context keeps c, the
 * absolute index of the next input (64 bits), and tau, the time of the next output in units of 2^-32 input samples (96 bits);
 * both are 0 after init and reset.  One output:
 *     q = floor(tau / 2^32), f = tau mod 2^32, p = the top ulPhaseBits bits of f, mu = (the other bits of f) / 2^(32-ulPhaseBits)
 *     y = sum_{j<K} [(1-mu) h[p + j*P] + mu h[p+1 + j*P]] x[q-j]      (h[k] = 0 for k >= T, x[i] = 0 for i < 0);   tau += R
 * A call that brings the inputs [c, c+N) emits, in order, every output with floor(tau / 2^32) < c+N:
 * max(0, ceil(((c+N)*2^32 - tau) / R)) of them, possibly none; then c += N.  All of this is integer arithmetic, so
 * process(a||b) == process(a); process(b), bit for bit, wherever the stream is cut.  Float32 or int16 input; float32 I/Q output.
 * No NCO, real taps only.  Errors: 0 + if_fir_arb_last_error(); a failed call leaves the context usable and c, tau unchanged.
 * Calls on a stream that is being captured into a hipGraph are refused. */
#define IF_FIR_ARB_MAX_TAPS 8192u
#define IF_FIR_ARB_MIN_PHASE_BITS 4u
#define IF_FIR_ARB_MAX_PHASE_BITS 10u
typedef struct if_fir_arb if_fir_arb_t;

/* ullMaxSamples: 1..2^30, the most inputs of one if_fir_arb_process() call */
uint8_t if_fir_arb_init(if_fir_arb_t **ppCtx, const float *pfTaps, uint32_t ulTaps, uint32_t ulPhaseBits, uint64_t ullStep,
                        uint64_t ullMaxSamples, int32_t lDevice);
void if_fir_arb_destroy(if_fir_arb_t *pCtx);
/* zero the history, c and tau; the step stays */
uint8_t if_fir_arb_reset(if_fir_arb_t *pCtx);
/* retune between calls: c, tau and the history stay, so the next output is where it was and the one after it ullStep later.
 * Setting the current value changes no bit. */
uint8_t if_fir_arb_set_step(if_fir_arb_t *pCtx, uint64_t ullStep);
/* IF_FIR_INPUT_F32 or IF_FIR_INPUT_I16 (value = int16 * 2^-15); the history is float32, so a change keeps the stream */
uint8_t if_fir_arb_set_input_format(if_fir_arb_t *pCtx, uint32_t ulFormat);
uint8_t if_fir_arb_set_stream(if_fir_arb_t *pCtx, void *pStream);
uint8_t if_fir_arb_synchronize(if_fir_arb_t *pCtx);
const char *if_fir_arb_last_error(const if_fir_arb_t *pCtx);
/* outputs of a call with ullSamples inputs at the current position and step */
uint64_t if_fir_arb_out_count(const if_fir_arb_t *pCtx, uint64_t ullSamples);
/* host pointers, synchronous; ullSamples <= ullMaxSamples of init; pfIQOut holds if_fir_arb_out_count() samples */
uint8_t if_fir_arb_process(if_fir_arb_t *pCtx, const void *pIQIn, float *pfIQOut, uint64_t ullSamples, uint64_t *pullOutSamples);
/* device pointers aligned to one sample (input 8 bytes, 4 for int16; output 8 bytes), asynchronous on the context's stream;
 * ullSamples <= 2^36; pDevOut holds if_fir_arb_out_count() samples */
uint8_t if_fir_arb_process_device(if_fir_arb_t *pCtx, const void *pDevIn, void *pDevOut, uint64_t ullSamples,
                                  uint64_t *pullOutSamples);
/* the step for a pair of rates: rint(dRateIn / dRateOut * 2^32), or 0 when that is outside 2^26 .. 2^34 or a rate is not a
 * positive finite number.  Touches no context and no GPU. */
uint64_t if_fir_arb_step_from_rates(double dRateIn, double dRateOut);

/* ---- polyphase filter bank (docs/SPEC.md §13; BUILD-DEFINED) ------------------------------------------------------------------
 * ALL M channels of a uniform grid out of one complex IQ stream in ONE pass (the analysis bank also known as PFB or weighted
 * overlap-add), M = 64 .. 4096.  Channel k is the decimator of SPEC §3.2 with phase word k * 2^32 / M, the real prototype
 * h[0..T-1] (T <= 16 M) and decimation D = ulHop (1 <= D <= M, any integer):
 *     y_k[m] = sum_{t<T} h[t] x[a-t] exp(-j 2 pi k (a-t) / M),   a = m*D = absolute index since init/reset,   x[i<0] = 0
 * Output is complex64 (float32 I, Q), frame-major: out[m*ulBins + j] = channel (lFirstBin + j) mod M of frame m.  A call whose
 * first sample has absolute index c and which brings N samples emits the frames with m*D in [c, c+N) (possibly none).
 * process(a||b) == process(a); process(b), bit for bit, wherever the stream is cut.  Float32 or int16 input.
 * The filter bank of if_fir_channelizer_process_device stays the route for up to 16 channels.
 * Errors: 0 + if_fir_pfb_last_error(); a failed call leaves the context usable and its stream position unchanged.
 * Calls on a stream that is being captured into a hipGraph are refused. */
typedef struct if_fir_pfb if_fir_pfb_t;

typedef struct
{
    uint32_t ulChannels; /* M: 64, 128, 256, 512, 1024, 2048 or 4096 */
    uint32_t ulHop;      /* D: input samples per frame, 1..M */
    int32_t lFirstBin;   /* first output channel, -M/2 <= lFirstBin < M (negative: counted down from M) */
    uint32_t ulBins;     /* output channels per frame, 1..M; the span wraps at M */
} if_fir_pfb_config_t;

/* pfTaps: ulTaps real float32 taps, 1 <= ulTaps <= 16 M, used as given.  ullMaxSamples: 1..2^40, the most samples of one call */
uint8_t if_fir_pfb_init(if_fir_pfb_t **ppCtx, const if_fir_pfb_config_t *pCfg, const float *pfTaps, uint32_t ulTaps,
                        uint64_t ullMaxSamples, int32_t lDevice);
void if_fir_pfb_destroy(if_fir_pfb_t *pCtx);
/* zero the history and the stream position */
uint8_t if_fir_pfb_reset(if_fir_pfb_t *pCtx);
/* IF_FIR_INPUT_F32 or IF_FIR_INPUT_I16 (value = int16 * 2^-15); the history is float32, so a change keeps the stream */
uint8_t if_fir_pfb_set_input_format(if_fir_pfb_t *pCtx, uint32_t ulFormat);
uint8_t if_fir_pfb_set_stream(if_fir_pfb_t *pCtx, void *pStream);
uint8_t if_fir_pfb_synchronize(if_fir_pfb_t *pCtx);
const char *if_fir_pfb_last_error(const if_fir_pfb_t *pCtx);
/* frames a call with ullSamples samples would emit at the current stream position */
uint64_t if_fir_pfb_frame_count(const if_fir_pfb_t *pCtx, uint64_t ullSamples);
/* host pointers, synchronous; ullSamples <= ullMaxSamples of init; pfIQOut holds if_fir_pfb_frame_count() x ulBins samples;
 * *pullFrames (may be NULL) receives the frames emitted */
uint8_t if_fir_pfb_process(if_fir_pfb_t *pCtx, const void *pIQIn, float *pfIQOut, uint64_t ullSamples, uint64_t *pullFrames);
/* device pointers aligned to one sample (input 8 bytes, 4 for int16; output 8 bytes), asynchronous on the context's stream;
 * pDevOut holds if_fir_pfb_frame_count() x ulBins samples */
uint8_t if_fir_pfb_process_device(if_fir_pfb_t *pCtx, const void *pDevIn, void *pDevOut, uint64_t ullSamples, uint64_t *pullFrames);

/* ---- polyphase synthesis bank (docs/SPEC.md §14; BUILD-DEFINED) ---------------------------------------------------------------
 * M channel streams on a uniform grid to ONE complex IQ stream in ONE pass (the weighted overlap-add synthesis bank, the
 * counterpart of if_fir_pfb_t), M = 64 .. 4096.  By definition the sum of M interpolators of SPEC §6 with factor L = ulHop
 * (1 <= L <= M, any integer), the real prototype h[0..T-1] (T <= 16 M, ceil(T / L) <= 32) and phase word k * 2^32 / M:
 *     y[n] = sum_k exp(+j 2 pi k n / M) sum_m h[n - m*L] X_k[m],   n = absolute output index since init/reset,   X_k[m<0] = 0
 * Input is frame-major, the output layout of if_fir_pfb_t: in[m*ulBins + j] = channel (lFirstBin + j) mod M of frame m, complex64
 * or int16 pairs; channels outside the span are 0.  F frames in give exactly F*L float32 I/Q samples out.
 * process(a||b) == process(a); process(b), bit for bit, wherever the frames are cut.
 * The channel combiner (if_fir_combiner_t) stays the route for up to 64 channels at arbitrary centres.
 * Errors: 0 + if_fir_synth_last_error(); a failed call leaves the context usable and its stream position unchanged.
 * Calls on a stream that is being captured into a hipGraph are refused. */
typedef struct if_fir_synth if_fir_synth_t;

typedef struct
{
    uint32_t ulChannels; /* M: 64, 128, 256, 512, 1024, 2048 or 4096 */
    uint32_t ulHop;      /* L: output samples per frame, 1..M */
    int32_t lFirstBin;   /* first input channel, -M/2 <= lFirstBin < M (negative: counted down from M) */
    uint32_t ulBins;     /* input channels per frame, 1..M; the span wraps at M */
} if_fir_synth_config_t;

/* pfTaps: ulTaps real float32 taps, 1 <= ulTaps <= 16 M and ceil(ulTaps / L) <= 32, used as given (no 1/M, no gain of L).
 * ullMaxFrames: 1..2^32, the most frames of one call */
uint8_t if_fir_synth_init(if_fir_synth_t **ppCtx, const if_fir_synth_config_t *pCfg, const float *pfTaps, uint32_t ulTaps,
                          uint64_t ullMaxFrames, int32_t lDevice);
void if_fir_synth_destroy(if_fir_synth_t *pCtx);
/* zero the history and the stream position */
uint8_t if_fir_synth_reset(if_fir_synth_t *pCtx);
/* IF_FIR_INPUT_F32 or IF_FIR_INPUT_I16 (value = int16 * 2^-15); the history is float32, so a change keeps the stream */
uint8_t if_fir_synth_set_input_format(if_fir_synth_t *pCtx, uint32_t ulFormat);
uint8_t if_fir_synth_set_stream(if_fir_synth_t *pCtx, void *pStream);
uint8_t if_fir_synth_synchronize(if_fir_synth_t *pCtx);
const char *if_fir_synth_last_error(const if_fir_synth_t *pCtx);
/* samples a call with ullFrames frames would emit at the current stream position: ullFrames * L (0 when the call would be refused
 * because its last output index would pass 2^64) */
uint64_t if_fir_synth_sample_count(const if_fir_synth_t *pCtx, uint64_t ullFrames);
/* host pointers, synchronous; ullFrames <= ullMaxFrames of init; pFramesIn holds ullFrames x ulBins elements, pfIQOut
 * if_fir_synth_sample_count() samples; *pullSamples (may be NULL) receives the samples emitted */
uint8_t if_fir_synth_process(if_fir_synth_t *pCtx, const void *pFramesIn, float *pfIQOut, uint64_t ullFrames, uint64_t *pullSamples);
/* device pointers aligned to one element (input 8 bytes, 4 for int16; output 8 bytes), asynchronous on the context's stream */
uint8_t if_fir_synth_process_device(if_fir_synth_t *pCtx, const void *pDevIn, void *pDevOut, uint64_t ullFrames, uint64_t *pullSamples);

/* ---- per-channel FIR stage over filter-bank frames (docs/SPEC.md §15; BUILD-DEFINED) -------------------------------------------
 * The second stage of a two-stage channelizer in ONE pass: frames in the banks' layout in (in[a*ulBins + j], what if_fir_pfb_t
 * emits and if_fir_synth_t takes), frames in the same layout out at 1/R of the frame rate, every bin filtered by its own real
 * FIR row, decimated, and mixed by its own NCO.  Bin j is, by definition, the decimator of SPEC §2/§3.2 on the strided stream
 * x_j[a] = in[a*B + j], a = absolute FRAME index since init/reset, x_j[a<0] = 0:
 *     x'_j[a] = x_j[a] exp(-j 2 pi ((P_j a) mod 2^32) / 2^32),   y_j[n] = sum_{k<T} h_r[k] x'_j[n*R - k],   r = j or 0
 *     out[n'*B + j] = y_j[n] for the n with c <= n*R < c + F, in order (c = frames before the call; possibly none)
 * B = ulBins is any integer 1..4096 and is not tied to a bank's M.  Input complex64 or int16 pairs, output complex64.
 * process(a||b) == process(a); process(b), bit for bit, wherever the frames are cut.
 * Errors: 0 + if_fir_sub_last_error(); a failed call leaves the context usable and its position, history and NCO words unchanged.
 * Calls on a stream that is being captured into a hipGraph are refused. */
typedef struct if_fir_sub if_fir_sub_t;

typedef struct
{
    uint32_t ulBins;       /* B: elements per frame, 1..4096 */
    uint32_t ulTaps;       /* T: taps per row, 1..128 */
    uint32_t ulTapRows;    /* 1: one row for all bins; B: a row per bin */
    uint32_t ulDecimation; /* R: input frames per output frame, 1..64 */
} if_fir_sub_config_t;

/* pfTaps: ulTapRows x ulTaps real float32 taps, row-major, used as given.  ullMaxFrames: 1..2^32, the most frames of one call
 * (host or device pointers).  After init every NCO word is 0 */
uint8_t if_fir_sub_init(if_fir_sub_t **ppCtx, const if_fir_sub_config_t *pCfg, const float *pfTaps, uint64_t ullMaxFrames, int32_t lDevice);
void if_fir_sub_destroy(if_fir_sub_t *pCtx);
/* zero the history and the stream position; the NCO words stay */
uint8_t if_fir_sub_reset(if_fir_sub_t *pCtx);
/* IF_FIR_INPUT_F32 or IF_FIR_INPUT_I16 (value = int16 * 2^-15); the history is float32, so a change keeps the stream */
uint8_t if_fir_sub_set_input_format(if_fir_sub_t *pCtx, uint32_t ulFormat);
/* pdFreq: B frequencies in cycles per INPUT FRAME, |f| <= 0.5, quantised to P_j = round(f_j 2^32) mod 2^32; NULL sets every word
 * to 0.  The words of a call apply to every frame its outputs weigh, the carried history included (it holds unmixed frames): a
 * retune is the phase step of if_fir_set_nco.  Setting the values in force changes nothing.  Waits for the context's stream */
uint8_t if_fir_sub_set_nco(if_fir_sub_t *pCtx, const double *pdFreq);
/* pdFreq receives the B quantised frequencies in force */
uint8_t if_fir_sub_get_nco(const if_fir_sub_t *pCtx, double *pdFreq);
uint8_t if_fir_sub_set_stream(if_fir_sub_t *pCtx, void *pStream);
uint8_t if_fir_sub_synchronize(if_fir_sub_t *pCtx);
const char *if_fir_sub_last_error(const if_fir_sub_t *pCtx);
/* output frames a call with ullFrames frames would emit at the current stream position (0 when the call would be refused because
 * the position would pass 2^64) */
uint64_t if_fir_sub_frame_count(const if_fir_sub_t *pCtx, uint64_t ullFrames);
/* host pointers, synchronous; ullFrames <= ullMaxFrames of init; pFramesIn holds ullFrames x ulBins elements, pfFramesOut
 * if_fir_sub_frame_count() x ulBins complex64; *pullOutFrames (may be NULL) receives the frames emitted */
uint8_t if_fir_sub_process(if_fir_sub_t *pCtx, const void *pFramesIn, float *pfFramesOut, uint64_t ullFrames, uint64_t *pullOutFrames);
/* device pointers aligned to one element (input 8 bytes, 4 for int16; output 8 bytes), asynchronous on the context's stream */
uint8_t if_fir_sub_process_device(if_fir_sub_t *pCtx, const void *pDevIn, void *pDevOut, uint64_t ullFrames, uint64_t *pullOutFrames);

/* ---- per-bin interpolating FIR stage over frames, the transmit mirror of the stage above (docs/SPEC.md §16; BUILD-DEFINED) ------
 * Frames in the banks' layout in (in[m*ulBins + j]), frames in the same layout out at R times the frame rate: every bin
 * interpolated by R through its own real FIR row and mixed up by its own NCO, in ONE pass.  Bin j is, by definition, the
 * interpolator of SPEC §6 with factor R and if_fir_interp_set_nco(f_j) on the strided stream x_j[m] = in[m*B + j], m = absolute
 * INPUT frame index since init/reset, x_j[m<0] = 0; n = absolute OUTPUT frame index:
 *     u_j[n] = x_j[n/R] if R divides n, else 0;   v_j[n] = sum_{k<T} h_r[k] u_j[n - k],   r = j or 0
 *     y_j[n] = exp(+j 2 pi ((P_j n) mod 2^32) / 2^32) v_j[n];   out[(n - c*R)*B + j] = y_j[n] for c*R <= n < (c + F)*R
 * (c = input frames before the call).  F frames in give exactly F*R frames out.  The taps are used as given (no gain of R).
 * B = ulBins is any integer 1..4096 and is not tied to a bank's M.  Input complex64 or int16 pairs, output complex64.
 * process(a||b) == process(a); process(b), bit for bit, wherever the frames are cut.
 * Errors: 0 + if_fir_subup_last_error(); a failed call leaves the context usable and its position, history and NCO words unchanged.
 * Calls on a stream that is being captured into a hipGraph are refused. */
typedef struct if_fir_subup if_fir_subup_t;

typedef struct
{
    uint32_t ulBins;          /* B: elements per frame, 1..4096 */
    uint32_t ulTaps;          /* T: taps per row, 1..2048, with ceil(T / R) <= 32 */
    uint32_t ulTapRows;       /* 1: one row for all bins; B: a row per bin */
    uint32_t ulInterpolation; /* R: output frames per input frame, 1..64 */
} if_fir_subup_config_t;

/* pfTaps: ulTapRows x ulTaps real float32 taps, row-major, used as given.  ullMaxFrames: 1..2^32, the most INPUT frames of one
 * call (host or device pointers).  After init every NCO word is 0 */
uint8_t if_fir_subup_init(if_fir_subup_t **ppCtx, const if_fir_subup_config_t *pCfg, const float *pfTaps, uint64_t ullMaxFrames, int32_t lDevice);
void if_fir_subup_destroy(if_fir_subup_t *pCtx);
/* zero the history and the stream position; the NCO words stay */
uint8_t if_fir_subup_reset(if_fir_subup_t *pCtx);
/* IF_FIR_INPUT_F32 or IF_FIR_INPUT_I16 (value = int16 * 2^-15); the history is float32, so a change keeps the stream */
uint8_t if_fir_subup_set_input_format(if_fir_subup_t *pCtx, uint32_t ulFormat);
/* pdFreq: B frequencies in cycles per OUTPUT FRAME, |f| <= 0.5, quantised to P_j = round(f_j 2^32) mod 2^32; NULL sets every
 * word to 0.  The words in force at a call rotate that call's outputs by their absolute index (the history holds unmixed
 * frames): a retune is the phase step of if_fir_interp_set_nco.  Setting the values in force changes nothing.  Waits for the
 * context's stream */
uint8_t if_fir_subup_set_nco(if_fir_subup_t *pCtx, const double *pdFreq);
/* pdFreq receives the B quantised frequencies in force */
uint8_t if_fir_subup_get_nco(const if_fir_subup_t *pCtx, double *pdFreq);
uint8_t if_fir_subup_set_stream(if_fir_subup_t *pCtx, void *pStream);
uint8_t if_fir_subup_synchronize(if_fir_subup_t *pCtx);
const char *if_fir_subup_last_error(const if_fir_subup_t *pCtx);
/* output frames a call with ullFrames frames would emit: ullFrames * R (0 when the call would be refused because its last
 * output index would pass 2^64 - 1) */
uint64_t if_fir_subup_frame_count(const if_fir_subup_t *pCtx, uint64_t ullFrames);
/* host pointers, synchronous; ullFrames <= ullMaxFrames of init; pFramesIn holds ullFrames x ulBins elements, pfFramesOut
 * if_fir_subup_frame_count() x ulBins complex64; *pullOutFrames (may be NULL) receives the frames emitted */
uint8_t if_fir_subup_process(if_fir_subup_t *pCtx, const void *pFramesIn, float *pfFramesOut, uint64_t ullFrames, uint64_t *pullOutFrames);
/* device pointers aligned to one element (input 8 bytes, 4 for int16; output 8 bytes), asynchronous on the context's stream */
uint8_t if_fir_subup_process_device(if_fir_subup_t *pCtx, const void *pDevIn, void *pDevOut, uint64_t ullFrames, uint64_t *pullOutFrames);

/* ---- real-input polyphase filter bank (docs/SPEC.md §17; BUILD-DEFINED) --------------------------------------------------------
 * The M/2 + 1 distinct channels of a uniform grid out of one REAL sample stream in ONE pass, M = 128 .. 8192: the bank of
 * if_fir_pfb_t fed (r, 0), without widening the stream, folding zeros or transforming M points.  Channel k is the down-converter
 * of SPEC §10 (if_fir_ddc_t) with phase word k * 2^32 / M, the real prototype h[0..T-1] (T <= 16 M) and decimation D = ulHop
 * (1 <= D <= M, any integer):
 *     y_k[m] = sum_{t<T} h[t] r[a-t] exp(-j 2 pi k (a-t) / M),   a = m*D = absolute index since init/reset,   r[i<0] = 0,   k = 0 .. M/2
 * The channels above M/2 are the complex conjugates y_{M-k} = conj y_k and are not offered; channels 0 and M/2 are real (their
 * imaginary part is exactly zero).  Input is one float32 or one int16 (value = int16 * 2^-15) per sample.  Output is complex64
 * (float32 I, Q), frame-major, the layout of if_fir_pfb_t: out[m*ulBins + j] = channel ulFirstBin + j of frame m.  A call whose
 * first sample has absolute index c and which brings N samples emits the frames with m*D in [c, c+N) (possibly none).
 * process(a||b) == process(a); process(b), bit for bit, wherever the stream is cut.
 * Errors: 0 + if_fir_rpfb_last_error(); a failed call leaves the context usable and its stream position unchanged.
 * Calls on a stream that is being captured into a hipGraph are refused. */
typedef struct if_fir_rpfb if_fir_rpfb_t;

typedef struct
{
    uint32_t ulChannels; /* M: 128, 256, 512, 1024, 2048, 4096 or 8192 */
    uint32_t ulHop;      /* D: input samples per frame, 1..M */
    uint32_t ulFirstBin; /* first output channel, 0 <= ulFirstBin */
    uint32_t ulBins;     /* output channels per frame, >= 1; ulFirstBin + ulBins <= M/2 + 1: the span does not wrap */
} if_fir_rpfb_config_t;

/* pfTaps: ulTaps real float32 taps, 1 <= ulTaps <= 16 M, used as given.  ullMaxSamples: 1..2^40, the most samples of one call */
uint8_t if_fir_rpfb_init(if_fir_rpfb_t **ppCtx, const if_fir_rpfb_config_t *pCfg, const float *pfTaps, uint32_t ulTaps,
                         uint64_t ullMaxSamples, int32_t lDevice);
void if_fir_rpfb_destroy(if_fir_rpfb_t *pCtx);
/* zero the history and the stream position */
uint8_t if_fir_rpfb_reset(if_fir_rpfb_t *pCtx);
/* IF_FIR_INPUT_F32 or IF_FIR_INPUT_I16 (value = int16 * 2^-15); the history is float32, so a change keeps the stream */
uint8_t if_fir_rpfb_set_input_format(if_fir_rpfb_t *pCtx, uint32_t ulFormat);
uint8_t if_fir_rpfb_set_stream(if_fir_rpfb_t *pCtx, void *pStream);
uint8_t if_fir_rpfb_synchronize(if_fir_rpfb_t *pCtx);
const char *if_fir_rpfb_last_error(const if_fir_rpfb_t *pCtx);
/* frames a call with ullSamples samples would emit at the current stream position */
uint64_t if_fir_rpfb_frame_count(const if_fir_rpfb_t *pCtx, uint64_t ullSamples);
/* host pointers, synchronous; ullSamples <= ullMaxSamples of init; pIn holds ullSamples real samples, pfIQOut
 * if_fir_rpfb_frame_count() x ulBins complex64; *pullFrames (may be NULL) receives the frames emitted */
uint8_t if_fir_rpfb_process(if_fir_rpfb_t *pCtx, const void *pIn, float *pfIQOut, uint64_t ullSamples, uint64_t *pullFrames);
/* device pointers aligned to one sample (input 4 bytes, 2 for int16; output 8 bytes), asynchronous on the context's stream;
 * pDevOut holds if_fir_rpfb_frame_count() x ulBins samples */
uint8_t if_fir_rpfb_process_device(if_fir_rpfb_t *pCtx, const void *pDevIn, void *pDevOut, uint64_t ullSamples, uint64_t *pullFrames);

/* ---- real-output polyphase synthesis bank (docs/SPEC.md §18; BUILD-DEFINED) ----------------------------------------------------
 * The M/2 + 1 distinct channels of a uniform grid to ONE REAL sample stream in ONE pass, M = 128 .. 8192: the real part of the
 * bank of if_fir_synth_t fed the Hermitian extension of each frame (channel M - k = conj of channel k), without writing the
 * extension, transforming M points or emitting a complex stream.  By definition the sum of the up-converters of SPEC §11
 * (if_fir_duc_t) with phase word k * 2^32 / M, the real prototype h[0..T-1] (T <= 16 M, ceil(T / L) <= 32) and factor L = ulHop
 * (1 <= L <= M, any integer), channels 0 and M/2 once and every channel between them twice:
 *     y[n] = sum_m h[n - m*L] ( Re X_0[m] + (-1)^n Re X_{M/2}[m] + 2 sum_{0<k<M/2} Re( X_k[m] exp(+j 2 pi k n / M) ) ),
 *     n = absolute output index since init/reset,   X_k[m<0] = 0
 * The imaginary parts of channels 0 and M/2 are ignored.  Input is frame-major, the output layout of if_fir_rpfb_t:
 * in[m*ulBins + j] = channel ulFirstBin + j of frame m, complex64 or int16 pairs; channels outside the span are 0.  F frames in
 * give exactly F*L real samples out, float32 or (if_fir_rsynth_set_output_format) int16.
 * process(a||b) == process(a); process(b), bit for bit, wherever the frames are cut.
 * Errors: 0 + if_fir_rsynth_last_error(); a failed call leaves the context usable and its stream position unchanged.
 * Calls on a stream that is being captured into a hipGraph are refused. */
typedef struct if_fir_rsynth if_fir_rsynth_t;

typedef struct
{
    uint32_t ulChannels; /* M: 128, 256, 512, 1024, 2048, 4096 or 8192 */
    uint32_t ulHop;      /* L: output samples per frame, 1..M */
    uint32_t ulFirstBin; /* first input channel, 0 <= ulFirstBin */
    uint32_t ulBins;     /* input channels per frame, >= 1; ulFirstBin + ulBins <= M/2 + 1: the span does not wrap */
} if_fir_rsynth_config_t;

/* pfTaps: ulTaps real float32 taps, 1 <= ulTaps <= 16 M and ceil(ulTaps / L) <= 32, used as given (no 1/M, no gain of L).
 * ullMaxFrames: 1..2^32, the most frames of one call */
uint8_t if_fir_rsynth_init(if_fir_rsynth_t **ppCtx, const if_fir_rsynth_config_t *pCfg, const float *pfTaps, uint32_t ulTaps,
                           uint64_t ullMaxFrames, int32_t lDevice);
void if_fir_rsynth_destroy(if_fir_rsynth_t *pCtx);
/* zero the history and the stream position */
uint8_t if_fir_rsynth_reset(if_fir_rsynth_t *pCtx);
/* IF_FIR_INPUT_F32 or IF_FIR_INPUT_I16 (value = int16 * 2^-15); the history is float32, so a change keeps the stream */
uint8_t if_fir_rsynth_set_input_format(if_fir_rsynth_t *pCtx, uint32_t ulFormat);
/* IF_FIR_OUTPUT_F32 (4 bytes per sample, the default) or IF_FIR_OUTPUT_I16 (2 bytes: the same float32 result * 2^15, rounded
 * to nearest even, saturated at -32768 / 32767); a change keeps the stream */
uint8_t if_fir_rsynth_set_output_format(if_fir_rsynth_t *pCtx, uint32_t ulFormat);
uint8_t if_fir_rsynth_set_stream(if_fir_rsynth_t *pCtx, void *pStream);
uint8_t if_fir_rsynth_synchronize(if_fir_rsynth_t *pCtx);
const char *if_fir_rsynth_last_error(const if_fir_rsynth_t *pCtx);
/* samples a call with ullFrames frames would emit at the current stream position: ullFrames * L (0 when the call would be refused
 * because its last output index would pass 2^64) */
uint64_t if_fir_rsynth_sample_count(const if_fir_rsynth_t *pCtx, uint64_t ullFrames);
/* host pointers, synchronous; ullFrames <= ullMaxFrames of init; pFramesIn holds ullFrames x ulBins elements, pOut
 * if_fir_rsynth_sample_count() real samples in the output format; *pullSamples (may be NULL) receives the samples emitted */
uint8_t if_fir_rsynth_process(if_fir_rsynth_t *pCtx, const void *pFramesIn, void *pOut, uint64_t ullFrames, uint64_t *pullSamples);
/* device pointers aligned to one element (input 8 bytes, 4 for int16; output 4 bytes, 2 for int16), asynchronous on the
 * context's stream */
uint8_t if_fir_rsynth_process_device(if_fir_rsynth_t *pCtx, const void *pDevIn, void *pDevOut, uint64_t ullFrames, uint64_t *pullSamples);

/* ---- frame power stage: filter-bank frames to detector spectrum codes (docs/SPEC.md §19; BUILD-DEFINED) ------------------------
 * Frames in the banks' layout in (in[a*ulBins + i], what if_fir_pfb_t, if_fir_rpfb_t and if_fir_sub_t emit), K-frame averages of
 * |.|^2 per output bin out, as the uint16 spectrum codes wb_detect_frames_device() reads (the mapping of if_fir_psd_t) and,
 * optionally, as float32 powers: the polyphase spectrometer of a stream whose bank is already running, without a second pass
 * over the samples and without a transform.  Output bin j sums the G adjacent elements ulFirst + j*G .. ulFirst + j*G + G - 1;
 * output frame f averages the input frames f*K .. f*K + K - 1 (a = absolute frame index since init/reset):
 *     P[f][j] = ( sum_{a in frame f} sum_{g<G} |in[a*B + ulFirst + j*G + g]|^2 ) / (K * G * fNorm)
 * in float32, in the order SPEC §19 fixes; the code of P is that of SPEC §8 with fRefPower.  A call with F frames at position c
 * emits floor((c+F)/K) - floor(c/K) output frames (possibly none); what it leaves open is carried as sums, not as samples.
 * Input complex64 or int16 pairs (value = int16 * 2^-15).
 * process(a||b) == process(a); process(b), bit for bit in both outputs, wherever the frames are cut.
 * Errors: 0 + if_fir_fpow_last_error(); a failed call leaves the context usable and its stream position unchanged.
 * Calls on a stream that is being captured into a hipGraph are refused. */
typedef struct if_fir_fpow if_fir_fpow_t;

typedef struct
{
    uint32_t ulBins;        /* B: elements per input frame, 1..8192 (if_fir_rpfb_t at M = 8192 emits 4097) */
    uint32_t ulFirst;       /* first element of a frame that is used */
    uint32_t ulGroup;       /* G: adjacent elements summed into one output bin, 1..64 */
    uint32_t ulOutBins;     /* Bo >= 1, ulFirst + G*Bo <= B */
    uint32_t ulFrames;      /* K: input frames averaged per output frame, 1..65535 */
    float fNorm;            /* > 0, finite: sum h^2 of the bank's prototype makes white noise of variance s^2 read s^2 */
    float fRefPower;        /* > 0, finite: as if_fir_psd_config_t */
    uint32_t ulInputFormat; /* IF_FIR_INPUT_F32 (complex64) or IF_FIR_INPUT_I16 (int16 pairs * 2^-15) */
} if_fir_fpow_config_t;

/* ullMaxFrames: 1..2^32, the most input frames of one call (host or device pointers); refused where the chunk sums of such a
 * call would pass 2^29 float32 values */
uint8_t if_fir_fpow_init(if_fir_fpow_t **ppCtx, const if_fir_fpow_config_t *pCfg, uint64_t ullMaxFrames, int32_t lDevice);
void if_fir_fpow_destroy(if_fir_fpow_t *pCtx);
/* zero the stream position (and with it what is carried) */
uint8_t if_fir_fpow_reset(if_fir_fpow_t *pCtx);
/* IF_FIR_INPUT_F32 or IF_FIR_INPUT_I16; what is carried is float32 sums, so a change keeps the stream */
uint8_t if_fir_fpow_set_input_format(if_fir_fpow_t *pCtx, uint32_t ulFormat);
uint8_t if_fir_fpow_set_stream(if_fir_fpow_t *pCtx, void *pStream);
uint8_t if_fir_fpow_synchronize(if_fir_fpow_t *pCtx);
const char *if_fir_fpow_last_error(const if_fir_fpow_t *pCtx);
/* output frames a call with ullFrames frames would emit at the current stream position (0 when the call would be refused because
 * the position would pass 2^64) */
uint64_t if_fir_fpow_frame_count(const if_fir_fpow_t *pCtx, uint64_t ullFrames);
/* host pointers, synchronous; ullFrames <= ullMaxFrames of init; pFramesIn holds ullFrames x ulBins elements, pusBins
 * if_fir_fpow_frame_count() x ulOutBins codes, pfPower (may be NULL) as many float32 powers; *pulOutFrames (may be NULL) receives
 * the frames emitted */
uint8_t if_fir_fpow_process(if_fir_fpow_t *pCtx, const void *pFramesIn, uint64_t ullFrames, uint16_t *pusBins, float *pfPower,
                            uint32_t *pulOutFrames);
/* device pointers aligned to one element (input 8 bytes, 4 for int16; codes 2; powers 4), asynchronous on the context's stream */
uint8_t if_fir_fpow_process_device(if_fir_fpow_t *pCtx, const void *pDevIn, uint64_t ullFrames, uint16_t *pusDevBins, float *pfDevPower,
                                   uint32_t *pulOutFrames);

/* ---- corner turn: bank frames to channel streams and back (docs/SPEC.md §20; BUILD-DEFINED) ------------------------------------
 * The frame families (if_fir_pfb_t, if_fir_rpfb_t, if_fir_sub_t, if_fir_subup_t, if_fir_synth_t, if_fir_rsynth_t, if_fir_fpow_t)
 * read or write frames, in[a*ulBins + i]; the stream families read or write one contiguous stream per context.  This stage
 * moves a list of bins between the two layouts on the device, with the format conversion fused, one kernel pass per direction:
 *     IF_FIR_TURN_TO_STREAMS:  out[c*P + a] = conv(in[a*B + sel[c]])            0 <= a < F, 0 <= c < C; row tails untouched
 *     IF_FIR_TURN_TO_FRAMES:   out[a*B + i] = conv(in[c*P + a]) if i == sel[c], +0 (all bits zero) otherwise; every element written
 * F = frames of the call, P = row pitch in elements (a call argument, P >= F, at most 2^40: a caller appends into per-channel
 * buffers).  conv: float32 to float32 and int16 to int16 copy the bits; int16 to float32 is the exact int16 * 2^-15; float32
 * to int16 is times 2^15, to nearest even, saturated (+-inf saturate), NaN gives 0.  No arithmetic otherwise: bit for bit.
 * The stage carries no state (no history, no position, no reset): process(a||b) == process(a); process(b) with the pointers
 * advanced by hand.  Errors: 0 + if_fir_turn_last_error(); a failed call leaves the context usable.
 * Calls on a stream that is being captured into a hipGraph are refused. */
typedef struct if_fir_turn if_fir_turn_t;

enum
{
    IF_FIR_TURN_TO_STREAMS = 0, /* frames in, C rows of pitch P out */
    IF_FIR_TURN_TO_FRAMES = 1   /* C rows of pitch P in, whole frames out (unlisted bins zero) */
};

typedef struct
{
    uint32_t ulDirection;    /* IF_FIR_TURN_TO_STREAMS or IF_FIR_TURN_TO_FRAMES */
    uint32_t ulBins;         /* B: elements per frame, 1..8192 */
    uint32_t ulChannels;     /* C: channel rows, 1..B */
    uint32_t ulFirst;        /* first bin of the span sel[c] = ulFirst + c (list pointer NULL), ulFirst + C <= B; 0 beside a list */
    uint32_t ulInputFormat;  /* IF_FIR_INPUT_F32 (complex64) or IF_FIR_INPUT_I16 (int16 pairs * 2^-15) */
    uint32_t ulOutputFormat; /* IF_FIR_OUTPUT_F32 (complex64) or IF_FIR_OUTPUT_I16 (int16 pairs) */
} if_fir_turn_config_t;

/* pulSel: NULL for the span, or ulChannels bin indices, each < ulBins, pairwise distinct, in any order (copied).  ullMaxFrames:
 * 1..2^32, the most frames of one call (host or device pointers) */
uint8_t if_fir_turn_init(if_fir_turn_t **ppCtx, const if_fir_turn_config_t *pCfg, const uint32_t *pulSel, uint64_t ullMaxFrames,
                         int32_t lDevice);
void if_fir_turn_destroy(if_fir_turn_t *pCtx);
/* from the next call on */
uint8_t if_fir_turn_set_input_format(if_fir_turn_t *pCtx, uint32_t ulFormat);
uint8_t if_fir_turn_set_output_format(if_fir_turn_t *pCtx, uint32_t ulFormat);
uint8_t if_fir_turn_set_stream(if_fir_turn_t *pCtx, void *pStream);
uint8_t if_fir_turn_synchronize(if_fir_turn_t *pCtx);
const char *if_fir_turn_last_error(const if_fir_turn_t *pCtx);
/* host pointers, synchronous; ullFrames <= ullMaxFrames of init (0 is legal and writes nothing); the frame side holds
 * ullFrames x ulBins elements, the row side ulChannels rows of ullPitch elements of which the first ullFrames are used */
uint8_t if_fir_turn_process(if_fir_turn_t *pCtx, const void *pIn, void *pOut, uint64_t ullFrames, uint64_t ullPitch);
/* device pointers aligned to one element (8 bytes, 4 for int16 pairs), asynchronous on the context's stream */
uint8_t if_fir_turn_process_device(if_fir_turn_t *pCtx, const void *pDevIn, void *pDevOut, uint64_t ullFrames, uint64_t ullPitch);

#ifdef __cplusplus
}
#endif
#endif /* IF_FIR_H */
