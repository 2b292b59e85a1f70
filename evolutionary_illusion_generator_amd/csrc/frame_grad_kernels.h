// frame_grad_kernels.h -- HIP kernels of the frame gradient d loss / d frames of PredNet training and of the gradient refinement of
// stills (prednet_train.hip, DESIGN.md section 13, "Frame gradients"): the element-wise kernel that joins the two halves of the
// frame gradient on every backward step, a per-image max |g| and the normalised ascent step on the bytes.  Like train_kernels.h:
// fixed partitions, fixed orders, no float atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "train_kernels.h"

namespace eigt {

// g_s = d loss / d x_s of one backward step s, for sample b at out + b * out_bstride as [C][H][W] (per_b = C H W floats).
//   input path (has_input: step s read its frame): dA = (E0[first half] > 0 ? dE0 : 0) - (E0[second half] > 0 ? dE0 : 0), the
//     expression of terr_bwd_kernel<0>, whose negation that kernel stores as dP; dE and E are [B][2C][H][W] of step s.
//   target path (has_target: frame s is the target of term s - 1 and its scale is not zero): minus the seed tpact_bwd_kernel<OBJ> adds
//     to dP0_{s-1}, from Pprev = P0_{s-1} [B][C][H][W] and the bytes of frame s (sample b at x + b * xbstride), d = p - x / 255.0f:
//     OBJ 0: -(scale * d); OBJ 1: -scale * sign(d), sign(0) = 0.
// accumulate = 0: a plain store; 1: out += g_s (the tied mode: one image per sample, launches of one stream in step order).
template <int OBJ>
__global__ void __launch_bounds__(EW_T) tframe_grad_kernel(const float* __restrict__ dE, const float* __restrict__ E, const float* __restrict__ Pprev,
                                                           const uint8_t* __restrict__ x, long long xbstride, float scale, int has_input, int has_target,
                                                           long long per_b, long long n, float* __restrict__ out, long long out_bstride, int accumulate)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const long long b = i / per_b, r = i - b * per_b;
    float g = 0.f;
    if (has_input) {
        const long long e0 = b * 2 * per_b + r, e1 = e0 + per_b;
        g = (E[e0] > 0.f ? dE[e0] : 0.f) - (E[e1] > 0.f ? dE[e1] : 0.f);
    }
    if (has_target) {
        const float d = Pprev[i] - (float)x[b * xbstride + r] / 255.0f;
        if constexpr (OBJ == 0) {
            g -= scale * d;
        } else {
            if (d > 0.f) g -= scale;
            else if (d < 0.f) g += scale;
        }
    }
    float* o = out + b * out_bstride + r;
    *o = accumulate ? *o + g : g;
}

// m[b] = max |g| over the elements of image b whose mask byte is not 0 (mask [H][W] shared by the channels, or nullptr: all); one
// block per image, a fixed strided slice per thread and a fixed LDS tree.  A maximum does not depend on the order anyway.
__global__ void __launch_bounds__(EW_T) tstill_absmax_kernel(const float* __restrict__ g, long long g_bstride, const uint8_t* __restrict__ mask, int HW,
                                                             long long per_b, float* __restrict__ m)
{
    __shared__ float red[EW_T];
    const float* gb = g + (long long)blockIdx.x * g_bstride;
    float v = 0.f;
    for (long long r = threadIdx.x; r < per_b; r += EW_T) {
        if (mask && mask[r % HW] == 0) continue;
        v = fmaxf(v, fabsf(gb[r]));
    }
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = EW_T / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) m[blockIdx.x] = red[0];
}

// One normalised ascent step on the bytes of stills [B][C][H][W], in place: x = byte / 255, x' = clamp(x + k * (g / m_b), 0, 1),
// byte' = (uint8_t)(int)(x' * 255 + 0.5).  A pixel whose mask byte is 0 keeps its byte, and so does every pixel of an image with
// m_b == 0.  Every operation is one float32 operation (the build's -ffp-contract=off): tests restate it in numpy.
__global__ void __launch_bounds__(EW_T) tstill_step_kernel(uint8_t* __restrict__ img, const float* __restrict__ g, long long g_bstride,
                                                           const uint8_t* __restrict__ mask, const float* __restrict__ m, float k, int HW, long long per_b,
                                                           long long n)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const long long b = i / per_b, r = i - b * per_b;
    if (mask && mask[r % HW] == 0) return;
    const float mb = m[b];
    if (!(mb > 0.f)) return;
    const float x = (float)img[i] / 255.0f;
    const float xn = fminf(fmaxf(x + k * (g[b * g_bstride + r] / mb), 0.f), 1.f);
    img[i] = (uint8_t)(int)(xn * 255.0f + 0.5f);
}

}  // namespace eigt
