/*
 * if_fir_debug.h — development hooks of the IF-chain FIR library.  NOT part of the product ABI: these entry points and
 * the tuning variants listed below exist only in libif_fir_dev.so (the same sources built with -DIF_FIR_DEVELOPMENT),
 * which the test-suite and the tools under tools/ load; libif_fir.so exports none of them (tests/test_host.py checks).
 *
 * Development tuning variants of if_fir_set_tuning() (dev library only; the diagnostic ones additionally need
 * IF_FIR_DEBUG=1 in the environment because their results are WRONG by construction):
 *   2000 + k       at most k workgroups for the overlap-save kernel: same results; lets small inputs run through every
 *                  stage of the block queue (tests/test_gpu_parity.py)
 *   1000 + bits    diagnostic launches of the overlap-save kernel (IF_FIR_DEBUG=1): 1 skip the global loads, 2 skip the
 *                  stores
 *   1000000 + bits the same with room for more bits; 256 no tail phase in short launches; 512 the waves of workgroup 0 count a
 *                  queue fault and leave as if their bounded wait had expired: blocks stay unwritten and if_fir_synchronize must
 *                  report it (the fault path's test); 4096 (round 4) the filter bank at decimation 8 without the all-slots form:
 *                  every channel through the per-channel form (same results to tolerance; A/B timing and tests); 8192 (round 4)
 *                  both slot parities of such a call as two launches instead of one; 262144 (round 5) no single-round launches: a
 *                  call of at most one block per wave of the chip fills eight waves per workgroup instead of one block per wave
 *                  dealt over all CUs (same results, A/B timing; 131072 is the launcher's own bit).  Any other bit belonged to a
 *                  closed experiment and is refused.
 *   3000           decimation 2, 6, 10, ..., 62 through the full-rate kernel + selecting store instead of the decimate-by-2 tail (same results to
 *                  tolerance; A/B timing)
 *   4000           the next call fails before anything is launched (IF_FIR_DEBUG=1): lets tests reach callers' error paths
 * Environment (dev library only): IF_FIR_DEBUG=1 IF_FIR_VARIANT=n preselects a variant at if_fir_init.
 * IF_FIR_MC_LOOPBACK=N (dev library only, read by if_fir_mc_init with one rank and >= 2 channels; N = 2..16 virtual ranks, 1 = 2):
 * this process plays all ranks of an N-rank world over a one-rank communicator of the real librccl (every send matched by its
 * receive in the same group, peer = itself): the multi-channel front's whole transfer protocol on a one-GPU box
 * (tools/mc_selfcheck.py).
 */
#ifndef IF_FIR_DEBUG_H
#define IF_FIR_DEBUG_H

#include "if_fir.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Time ulReps back-to-back if_fir_process_device() calls with HIP events on the context's stream, after
 * ulWarmup untimed ones; *pfMsPerCall receives the mean.  History/phase are restored afterwards. */
uint8_t if_fir_time_device(if_fir_ctx_t *pCtx, const void *pDevIn, void *pDevOut, uint64_t ullSamples,
                           uint32_t ulWarmup, uint32_t ulReps, float *pfMsPerCall);
/* first call with pullOut = NULL arms per-wave start/end time stamps for the persistent kernels; later calls copy the
 * last launch's stamps (4 x uint64 per wave) and return the number of words written. */
uint32_t if_fir_debug_stamps(if_fir_ctx_t *pCtx, uint64_t *pullOut, uint32_t ulWords);
/* host-only: the overlap-save kernel's table image (float32, ulOutFloats >= IF_FIR_DEBUG_TABLE_FLOATS) for these taps;
 * returns the number of floats written, 0 if the (taps, decimation) pair is not served by that kernel. */
#define IF_FIR_DEBUG_TABLE_FLOATS 21632u
uint32_t if_fir_debug_fft_tables(const float *pfTaps, uint32_t ulTaps, uint32_t bComplexTaps, uint32_t ulDecimation,
                                 uint32_t ulNcoDelta, float *pfOut, uint32_t ulOutFloats);
/* host-only: a filter bank's table image (ulBank 8 or 16; bank 8: ulParity 0 = the per-channel forms' image, also the all-slots
 * form's for the even slots, 1 = the all-slots form's for the odd slots), IF_FIR_DEBUG_TABLE_FLOATS floats */
uint32_t if_fir_debug_fft_tables_bank(const float *pfTaps, uint32_t ulTaps, uint32_t bComplexTaps, uint32_t ulBank, uint32_t ulParity,
                                      float *pfOut, uint32_t ulOutFloats);
/* host-only: the filter bank's tail for a decimation (4, 8 or 16; bOwnCentres: channels at their own centres, every multiple of 4 up
 * to 64 -- the tail then keeps every (decimation / tail)-th output); 0 = not served */
uint32_t if_fir_debug_bank_tail(uint32_t ulDecimation, uint32_t bOwnCentres);
/* host-only: routing of a decimation-8 filter-bank call on the slot grid: pulOut[0], pulOut[1] = slot masks of the all-slots
 * launches (even / odd slots; 0 = none), pulOut[2] = bit c set: channel c goes through the per-channel form */
uint8_t if_fir_debug_bank_plan(const uint32_t *pulSlots, uint32_t ulChannels, uint32_t *pulOut);
/* host-only: the table image of the odd-decimation kernel (decimation 3, 9, 15, ...: 2 * (3 * 1024 + 2176) = 10496 floats) */
#define IF_FIR_DEBUG_ODD_TABLE_FLOATS 10496u
uint32_t if_fir_debug_fft_tables_odd(const float *pfTaps, uint32_t ulTaps, uint32_t bComplexTaps, uint32_t ulDecimation,
                                     uint32_t ulNcoDelta, float *pfOut, uint32_t ulOutFloats);
/* host-only: the plan of an overlap-save launch of ullBlocks blocks on at most ulWorkgroups workgroups, as the launcher makes it
 * (bSingleOk = 0: with the single-round form switched off, like 262144 above): pllOut[4] = workgroups launched, blocks handed out
 * in groups (nblocks_main; the rest is the queue's tail phase), 1 = single-round launch (wave w of workgroup b takes block
 * w * workgroups + b), upper bound of the global ticket counter */
uint8_t if_fir_debug_fft_schedule(uint64_t ullBlocks, uint32_t ulWorkgroups, uint32_t bSingleOk, int64_t *pllOut);
/* bounded waits of the overlap-save kernel's block queue that expired since if_fir_init (a word of the context's
 * queue block; 0 in a healthy run: a wave that gives up leaves its blocks unwritten instead of hanging the device) */
uint8_t if_fir_debug_queue_faults(if_fir_ctx_t *pCtx, uint32_t *pulFaults);
/* host-only: the transfer plan of one rank of the multi-channel front for one call, 8 uint64 per operation {kind 0 send /
 * 1 recv, phase 0 scatter / 1 gather / 2 status, group, peer, channel, chunk, byte offset in rank 0's channel buffer,
 * bytes}; returns the operation count */
uint32_t if_fir_mc_debug_plan(uint32_t ulWorld, uint32_t ulChannels, uint32_t ulRank, uint64_t ullSamples,
                              uint32_t ulInBytes, uint32_t ulTaps, uint32_t ulDecimation, uint64_t ullConsumed,
                              uint64_t ullChunk, uint64_t *pullOut, uint32_t ulMaxOps);

/* interpolator (if_fir_interp_t): bForceFull = 1 runs the overlap-save kernel's full form (4096-point forward transform of the
 * zero-stuffed block) for every L instead of the small form (L >= 4); ulGridLimit = at most this many workgroups (0 = the
 * launcher's choice; same results: small inputs then take several rounds of the persistent workgroups) */
uint8_t if_fir_debug_interp_config(if_fir_interp_t *pCtx, uint32_t bForceFull, uint32_t ulGridLimit);
/* interpolator: set the count of input samples consumed since reset (the output index of the next call is ullSamples * L; the
 * history is kept): lets a test reach output indices past 2^32 without streaming them */
uint8_t if_fir_debug_interp_seek(if_fir_interp_t *pCtx, uint64_t ullSamples);
/* host-only: the interpolator's multiply table H[k] = FFT_4096(taps)[k] / 4096 as 4096 (re, im) pairs (ulOutFloats >= 8192);
 * returns the floats written, 0 when the taps are not served by the overlap-save kernel */
uint32_t if_fir_debug_interp_tables(const float *pfTaps, uint32_t ulTaps, uint32_t bComplexTaps, float *pfOut, uint32_t ulOutFloats);
/* host-only: what the interpolator decides for (taps, interpolation): *pulRows = the overlap-save kernel's overlap in rows of 64
 * outputs (the unit launched; 48 beyond its range), *pulHistLen = input samples of history kept between calls, *pbFftOk = 1 when
 * the overlap-save backend serves the pair; 0 = taps or interpolation outside if_fir_interp_init's range */
uint8_t if_fir_debug_interp_plan(uint32_t ulTaps, uint32_t ulInterpolation, uint32_t *pulRows, uint32_t *pulHistLen,
                                 uint32_t *pbFftOk);
/* channel combiner (if_fir_combiner_t): ulGridLimit = at most this many workgroups (0 = the launcher's choice; same results: one
 * workgroup then walks several blocks at test size) */
uint8_t if_fir_debug_combiner_config(if_fir_combiner_t *pCtx, uint32_t ulGridLimit);
/* channel combiner: set the count of input samples per channel consumed since reset (the output index of the next call is
 * ullSamples * L; the histories are kept), as the interpolator's seek */
uint8_t if_fir_debug_combiner_seek(if_fir_combiner_t *pCtx, uint64_t ullSamples);
/* host-only: the split of a centre's phase word P = G 2^20 + r (*pulGrid = G in 0..4095, *plResidual = r in -2^19..2^19-1) and the
 * combiner's multiply table for it, FFT_4096(h[k] exp(j 2 pi r k / 2^32)) / 4096, as 4096 (re, im) pairs (ulOutFloats >= 8192);
 * returns the floats written, 0 when the taps are not served by the overlap-save kernel or |dCentre| > 0.5 */
uint32_t if_fir_debug_combiner_tables(const float *pfTaps, uint32_t ulTaps, uint32_t bComplexTaps, double dCentre, uint32_t *pulGrid,
                                      int32_t *plResidual, float *pfOut, uint32_t ulOutFloats);
/* resampler (if_fir_resamp_t): ulGridLimit = at most this many workgroups (0 = the launcher's choice; same results: one
 * workgroup then walks many tiles at test size); *pulTileOutputs (may be NULL) receives the outputs of one tile of this context */
uint8_t if_fir_debug_resamp_config(if_fir_resamp_t *pCtx, uint32_t ulGridLimit, uint32_t *pulTileOutputs);
/* down-converter (if_fir_ddc_t): ulGridLimit and *pulTileOutputs as if_fir_debug_resamp_config; an ullPosition other than
 * UINT64_MAX sets the context's absolute sample index (the index of the next call's first sample) and zeroes its history */
uint8_t if_fir_debug_ddc_config(if_fir_ddc_t *pCtx, uint32_t ulGridLimit, uint32_t *pulTileOutputs, uint64_t ullPosition);
/* up-converter (if_fir_duc_t): ulGridLimit as if_fir_debug_resamp_config; *pulTileInputs (may be NULL) receives the INPUT samples
 * of one tile of this context (a tile emits L times as many outputs); an ullPosition other than UINT64_MAX sets the count of
 * input samples consumed since reset (the index of the next call's first input) and zeroes the history */
uint8_t if_fir_debug_duc_config(if_fir_duc_t *pCtx, uint32_t ulGridLimit, uint32_t *pulTileInputs, uint64_t ullPosition);
/* power-spectrum estimator (if_fir_psd_t): the plan of the next call of ullSamples samples at the current stream position:
 * pullPlan[0..3] = segments summed, chunks summed, frames emitted, samples carried after the call (nothing runs) */
uint8_t if_fir_debug_psd_plan(const if_fir_psd_t *pCtx, uint64_t ullSamples, uint64_t *pullPlan);
/* power-spectrum estimator: ulGridLimit as if_fir_debug_resamp_config, for the chunk kernel (one workgroup then sums several
 * chunks; the frame and carry kernels have no stride loop); an ullPosition other than UINT64_MAX sets the stream position (the
 * index of the next call's first sample) with nothing carried and the open frame's accumulator at +0.  It must be the first
 * sample of a chunk: ullPosition mod H == 0 and ((ullPosition / H) mod K) mod 8 == 0; any other is refused with a message and
 * the context is unchanged */
uint8_t if_fir_debug_psd_config(if_fir_psd_t *pCtx, uint32_t ulGridLimit, uint64_t ullPosition);
/* arbitrary-ratio resampler (if_fir_arb_t): ulGridLimit and *pulTileOutputs as if_fir_debug_resamp_config; an ullPosition other
 * than UINT64_MAX, on a freshly reset context, sets c = ullPosition and tau = c * 2^32 + ullTimeOffset (ullTimeOffset < 2^34) */
uint8_t if_fir_debug_arb_config(if_fir_arb_t *pCtx, uint32_t ulGridLimit, uint32_t *pulTileOutputs, uint64_t ullPosition,
                                uint64_t ullTimeOffset);
/* polyphase filter bank (if_fir_pfb_t): ulGridLimit as if_fir_debug_resamp_config; *pulGroupFrames (may be NULL) receives the
 * consecutive frames one workgroup owns; an ullPosition other than UINT64_MAX sets the context's absolute sample index (the
 * index of the next call's first sample) and zeroes its history */
uint8_t if_fir_debug_pfb_config(if_fir_pfb_t *pCtx, uint32_t ulGridLimit, uint32_t *pulGroupFrames, uint64_t ullPosition);
/* polyphase synthesis bank (if_fir_synth_t): ulGridLimit as if_fir_debug_resamp_config, for every kernel of a call; ulRoute
 * forces a route from the next call on (0 = the plan's choice, 1 = workspace, 2 = the one-kernel LDS ring, refused where two
 * workgroups of it do not fit a CU's LDS); *pulRoute (may be NULL) receives the route in use; an ullPosition other than
 * UINT64_MAX sets the context's absolute FRAME index (the index of the next call's first frame) and zeroes its history */
uint8_t if_fir_debug_synth_config(if_fir_synth_t *pCtx, uint32_t ulGridLimit, uint32_t ulRoute, uint32_t *pulRoute, uint64_t ullPosition);
/* ullBytes > 0 replaces the workspace of transformed frames by one of that budget (at least ceil(T / L) frames, at most 2^30
 * bytes; the default is 128 MB); *pullFrames (may be NULL) receives the frames of a call one chunk then emits the outputs of */
uint8_t if_fir_debug_synth_workspace(if_fir_synth_t *pCtx, uint64_t ullBytes, uint64_t *pullFrames);
/* per-channel FIR stage (if_fir_sub_t): ulGridLimit as if_fir_debug_resamp_config, for both kernels of a call; *pulTileOutputs
 * (may be NULL) receives the (output, bin) values one tile holds; an ullPosition other than UINT64_MAX sets the context's absolute
 * FRAME index (the index of the next call's first frame) and zeroes its history */
uint8_t if_fir_debug_sub_config(if_fir_sub_t *pCtx, uint32_t ulGridLimit, uint32_t *pulTileOutputs, uint64_t ullPosition);
/* per-bin interpolating FIR stage (if_fir_subup_t): ulGridLimit as if_fir_debug_resamp_config, for both kernels of a call;
 * *pulTileOutputs (may be NULL) receives the (output, bin) values one tile holds; an ullPosition other than UINT64_MAX sets the
 * context's absolute INPUT FRAME index (the index of the next call's first frame) and zeroes its history */
uint8_t if_fir_debug_subup_config(if_fir_subup_t *pCtx, uint32_t ulGridLimit, uint32_t *pulTileOutputs, uint64_t ullPosition);
/* real-input polyphase filter bank (if_fir_rpfb_t): the three arguments as if_fir_debug_pfb_config */
uint8_t if_fir_debug_rpfb_config(if_fir_rpfb_t *pCtx, uint32_t ulGridLimit, uint32_t *pulGroupFrames, uint64_t ullPosition);
/* real-output polyphase synthesis bank (if_fir_rsynth_t): ulGridLimit as if_fir_debug_resamp_config, for every kernel of a
 * call; an ullPosition other than UINT64_MAX sets the context's absolute FRAME index (the index of the next call's first frame)
 * and zeroes its history */
uint8_t if_fir_debug_rsynth_config(if_fir_rsynth_t *pCtx, uint32_t ulGridLimit, uint64_t ullPosition);
/* as if_fir_debug_synth_workspace; a transformed frame takes 4 M bytes here */
uint8_t if_fir_debug_rsynth_workspace(if_fir_rsynth_t *pCtx, uint64_t ullBytes, uint64_t *pullFrames);
/* frame power stage (if_fir_fpow_t): ulGridLimit as if_fir_debug_resamp_config, for both kernels of a call; an ullPosition other
 * than UINT64_MAX sets the context's absolute input FRAME index (the index of the next call's first frame) and clears what is
 * carried: the open frame's accumulator and the open chunk's partial sum start from +0 there */
uint8_t if_fir_debug_fpow_config(if_fir_fpow_t *pCtx, uint32_t ulGridLimit, uint64_t ullPosition);

/* corner turn (if_fir_turn_t): ulGridLimit as if_fir_debug_resamp_config (at most that many workgroups, 0 = the launcher's choice):
 * a small call then walks the grid-stride loop over its tiles */
uint8_t if_fir_debug_turn_config(if_fir_turn_t *pCtx, uint32_t ulGridLimit);

#ifdef __cplusplus
}
#endif
#endif /* IF_FIR_DEBUG_H */
