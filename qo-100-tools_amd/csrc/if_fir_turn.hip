// if_fir_turn.hip — corner turn for gfx950: frames in the polyphase banks' layout to one contiguous row per listed bin and back,
// with the format conversion fused, one kernel pass per direction (docs/SPEC.md §20).
//
//   TO_STREAMS:  out[c P + a] = conv(in[a B + sel[c]])
//   TO_FRAMES:   out[a B + i] = conv(in[inv[i] P + a]), all bits zero where no channel lists bin i
//
// turn_kernel<DIR, I16, O16>: a workgroup takes tiles of X columns by 4096 / X frames (if_fir_turn_plan.h: the tile map, which
// the plan checker plays on the host) in a grid-stride loop and exchanges each through LDS.  The FRAME side of a tile is moved
// with lanes along a frame's columns, the ROW side with lanes along a row's frames, so a wave's global access is one
// contiguous run of 64 elements wherever the selection is contiguous; what a lane moves is one element (8 or 4 bytes), which
// is all the alignment a pointer has.  The tile holds elements already converted, 8 bytes (float32 out) or 4 (int16 out), as
// tile[f][j] with an odd row pitch: the column accesses of the row-side phase fall on distinct banks.  A thread issues the 16
// loads of a phase before it stores the first.  TO_FRAMES: a tile none of whose bins is listed writes zeros and touches no LDS.
// Bounds are predicates: every lane reaches every barrier.  No arithmetic but conv; float32 to float32 moves the bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "if_fir_kernels.h"
#include "if_fir_stream_dev.h"
#include "if_fir_turn.h"

namespace if_fir
{

typedef uint32_t turn_v2u __attribute__((ext_vector_type(2)));

// one component, float32 to int16 (SPEC §11's rule and §20's own for a NaN): times 2^15, to nearest even, saturated; NaN: 0
__device__ __forceinline__ uint32_t turn_to_i16(float v)
{
    const float s = fminf(fmaxf(rintf(__fmul_rn(v, 32768.0f)), -32768.0f), 32767.0f);
    return (uint32_t)(v == v ? __float2int_rn(s) : 0) & 0xffffu;
}

template <bool O16>
struct turn_elem
{
    typedef turn_v2u type;
};
template <>
struct turn_elem<true>
{
    typedef uint32_t type;
};

// element e of the input in the output's format
template <bool I16, bool O16>
__device__ __forceinline__ typename turn_elem<O16>::type turn_load(const void *__restrict__ in, uint64_t e)
{
    if constexpr (I16)
    {
        const uint32_t w = static_cast<const uint32_t *>(in)[e];
        if constexpr (O16)
            return w;
        else
        {
            const float re = __fmul_rn((float)(short)(w & 0xffffu), 1.0f / 32768.0f), im = __fmul_rn((float)((int)w >> 16), 1.0f / 32768.0f);
            return turn_v2u{__float_as_uint(re), __float_as_uint(im)};
        }
    }
    else
    {
        const turn_v2u v = static_cast<const turn_v2u *>(in)[e];
        if constexpr (O16)
            return turn_to_i16(__uint_as_float(v.x)) | (turn_to_i16(__uint_as_float(v.y)) << 16);
        else
            return v;
    }
}

template <bool O16>
__device__ __forceinline__ typename turn_elem<O16>::type turn_zero()
{
    if constexpr (O16)
        return 0u;
    else
        return turn_v2u{0u, 0u};
}

template <int DIR, bool I16, bool O16>
__global__ __launch_bounds__(TURN_THREADS) void turn_kernel(const void *__restrict__ in, void *__restrict__ out, const uint16_t *__restrict__ map,
                                                            uint32_t B, uint32_t C, uint64_t F, uint64_t P, int xs, int64_t tiles_x, int64_t tiles)
{
    typedef typename turn_elem<O16>::type E;
    extern __shared__ __attribute__((aligned(8))) unsigned char turn_lds[];
    E *tile = reinterpret_cast<E *>(turn_lds);
    E *dst = static_cast<E *>(out);
    const int tid = threadIdx.x;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x)
    {
        uint32_t x0;
        uint64_t a0;
        turn_tile_origin(t, tiles_x, xs, &x0, &a0);
        E v[TURN_ITEMS];
        if constexpr (DIR == (int)TURN_TO_STREAMS)
        {
            // the frame side in: lanes along the listed bins of a frame
            int j, f;
            turn_item_along_frame(0, tid, xs, &j, &f);
            const uint32_t c = x0 + (uint32_t)j;
            const uint32_t bin = c < C ? map[c] : 0u;
#pragma unroll
            for (int k = 0; k < TURN_ITEMS; k++)
            {
                turn_item_along_frame(k, tid, xs, &j, &f);
                const uint64_t a = a0 + (uint64_t)f;
                v[k] = turn_zero<O16>();
                if (c < C && a < F)
                    v[k] = turn_load<I16, O16>(in, turn_frame_offset(a, B, bin));
            }
#pragma unroll
            for (int k = 0; k < TURN_ITEMS; k++)
            {
                turn_item_along_frame(k, tid, xs, &j, &f);
                tile[turn_lds_index(j, f, xs)] = v[k];
            }
            __syncthreads();
            // the row side out: lanes along the frames of a row
#pragma unroll
            for (int k = 0; k < TURN_ITEMS; k++)
            {
                turn_item_along_row(k, tid, xs, &j, &f);
                v[k] = tile[turn_lds_index(j, f, xs)];
            }
#pragma unroll
            for (int k = 0; k < TURN_ITEMS; k++)
            {
                turn_item_along_row(k, tid, xs, &j, &f);
                const uint32_t cr = x0 + (uint32_t)j;
                const uint64_t a = a0 + (uint64_t)f;
                if (cr < C && a < F)
                    dst[turn_row_offset(cr, P, a)] = v[k];
            }
            __syncthreads(); // the next tile overwrites what the slowest wave may still be reading
        }
        else
        {
            int j, f;
            turn_item_along_frame(0, tid, xs, &j, &f);
            const uint32_t bin = x0 + (uint32_t)j;
            const uint32_t mine = bin < B ? map[bin] : (uint32_t)TURN_NONE;
            // (the thread's column is every column of the tile as tid runs: X <= 64 <= TURN_THREADS)
            const int any = __syncthreads_or(mine != (uint32_t)TURN_NONE);
            if (any)
            {
                // the row side in: lanes along the frames of a row; a wave has one bin, so its test is uniform
#pragma unroll
                for (int k = 0; k < TURN_ITEMS; k++)
                {
                    turn_item_along_row(k, tid, xs, &j, &f);
                    const uint32_t i = x0 + (uint32_t)j;
                    const uint32_t cr = i < B ? map[i] : (uint32_t)TURN_NONE;
                    const uint64_t a = a0 + (uint64_t)f;
                    v[k] = turn_zero<O16>();
                    if (cr != (uint32_t)TURN_NONE && a < F)
                        v[k] = turn_load<I16, O16>(in, turn_row_offset(cr, P, a));
                }
#pragma unroll
                for (int k = 0; k < TURN_ITEMS; k++)
                {
                    turn_item_along_row(k, tid, xs, &j, &f);
                    tile[turn_lds_index(j, f, xs)] = v[k];
                }
            }
            __syncthreads();
            // the frame side out: lanes along the bins of a frame, every bin of every frame written
#pragma unroll
            for (int k = 0; k < TURN_ITEMS; k++)
            {
                turn_item_along_frame(k, tid, xs, &j, &f);
                v[k] = turn_zero<O16>();
                if (any)
                    v[k] = tile[turn_lds_index(j, f, xs)];
            }
#pragma unroll
            for (int k = 0; k < TURN_ITEMS; k++)
            {
                turn_item_along_frame(k, tid, xs, &j, &f);
                const uint64_t a = a0 + (uint64_t)f;
                if (bin < B && a < F)
                    dst[turn_frame_offset(a, B, bin)] = v[k];
            }
            __syncthreads();
        }
    }
}

template <int DIR, bool I16, bool O16>
static hipError_t launch_t(const TurnArgs &a)
{
    const uint32_t cols = DIR == (int)TURN_TO_STREAMS ? (uint32_t)a.C : (uint32_t)a.B;
    const int xs = turn_tile_shift(cols);
    const size_t lds = (size_t)turn_lds_elements(xs) * (O16 ? 4 : 8);
    int cus = 0;
    const hipError_t e = stream_kernel_setup<&turn_kernel<DIR, I16, O16>>(a.device, TURN_TILE / 2 * 3 * 8, &cus);
    if (e != hipSuccess)
        return e;
    int64_t tiles_x;
    const int64_t tiles = turn_tiles(cols, (uint64_t)a.F, xs, &tiles_x);
    const unsigned groups = stream_persistent_groups(cus, stream_groups_per_cu(lds), tiles, a.grid_limit);
    hipLaunchKernelGGL((turn_kernel<DIR, I16, O16>), dim3(groups), dim3(TURN_THREADS), lds, a.stream, a.in, a.out, a.map, (uint32_t)a.B,
                       (uint32_t)a.C, (uint64_t)a.F, (uint64_t)a.P, xs, tiles_x, tiles);
    return hipGetLastError();
}

template <int DIR>
static hipError_t launch_d(const TurnArgs &a)
{
    if (a.in_i16)
        return a.out_i16 ? launch_t<DIR, true, true>(a) : launch_t<DIR, true, false>(a);
    return a.out_i16 ? launch_t<DIR, false, true>(a) : launch_t<DIR, false, false>(a);
}

hipError_t launch_turn(const TurnArgs &a)
{
    if (a.B < 1 || a.B > (int)TURN_MAX_BINS || a.C < 1 || a.C > a.B || a.F < 1 || (uint64_t)a.F > TURN_MAX_CALL_FRAMES || a.P < a.F ||
        (uint64_t)a.P > TURN_MAX_PITCH || !a.in || !a.out || !a.map)
        return hipErrorInvalidValue;
    return a.direction == (int)TURN_TO_FRAMES ? launch_d<(int)TURN_TO_FRAMES>(a) : launch_d<(int)TURN_TO_STREAMS>(a);
}

} // namespace if_fir
