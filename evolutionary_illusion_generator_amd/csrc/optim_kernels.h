// optim_kernels.h -- HIP kernels of the optimiser controls (prednet_train.hip, DESIGN.md section 13, "Optimiser controls"): the
// norm of the gradient table, per tensor and global, in double; the accumulator's axpy; and Adam with gradient clipping and weight
// decay.  The tables are float32, every reduction is float64 with a fixed partition and a fixed order: no atomics, so norms,
// clipped steps and accumulated gradients are bit-identical from run to run.  The unit is compiled with -ffp-contract=off: every
// product and every sum below is rounded once, as written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "train_kernels.h"

namespace eigt {

constexpr int NORM_SLICES = 16;   // blocks per tensor of the sum of squares
constexpr int NORM_FINAL_T = 256; // threads of the one block that finishes it

// Sum of squares of every tensor of the flat gradient table, one launch: block (slice, k) sums (double)g_i * (double)g_i (exact: a
// float's square fits a double) over tensor k = tab[k] = (offset, count), a fixed strided slice per thread, then a fixed LDS tree;
// part[k][slice].  A thread with nothing to read adds +0.0, so a tensor shorter than a block or than the grid comes out exact.
__global__ void __launch_bounds__(EW_T) tgrad_sumsq_kernel(const float* __restrict__ g, const long long* __restrict__ tab, double* __restrict__ part)
{
    __shared__ double red[EW_T];
    const int k = blockIdx.y;
    const long long off = tab[2 * k], n = tab[2 * k + 1];
    const float* gk = g + off;
    double s = 0.0;
    for (long long i = (long long)blockIdx.x * EW_T + threadIdx.x; i < n; i += (long long)gridDim.x * EW_T) {
        const double v = (double)gk[i];
        s += v * v;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = EW_T / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[(long long)k * gridDim.x + blockIdx.x] = red[0];
}

// sumsq[k] = part[k][0] + part[k][1] + ... in slice order, one thread per tensor; then thread 0 adds the sumsq in tensor order and
// writes norm[0] = sqrt of that.  One block.
__global__ void __launch_bounds__(NORM_FINAL_T) tgrad_norm_final_kernel(const double* __restrict__ part, int slices, int n_tensors, double* __restrict__ sumsq,
                                                                        double* __restrict__ norm)
{
    for (int k = threadIdx.x; k < n_tensors; k += NORM_FINAL_T) {
        double s = 0.0;
        for (int j = 0; j < slices; ++j) s += part[(long long)k * slices + j];
        sumsq[k] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int k = 0; k < n_tensors; ++k) s += sumsq[k];
    norm[0] = sqrt(s);
}

// acc[i] = acc[i] + s * g[i]: one rounded product, one rounded sum
__global__ void __launch_bounds__(EW_T) tgrad_axpy_kernel(float* __restrict__ acc, const float* __restrict__ g, float s, long long n)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const float sg = s * g[i];
    acc[i] = acc[i] + sg;
}

// tadam_kernel with gradient clipping and weight decay, chainer's GradientClipping hook followed by its AdamRule with
// weight_decay_rate and eta = 1.  norm[0] is the global norm tgrad_norm_final_kernel left on the device: rate = clip / norm (the
// division in double) where clip > 0 and norm > clip, else 1 (a norm of 0, or one that is not a number, divides nothing);
// g' = rate g; m += (1 - b1) (g' - m); v += (1 - b2) (g'^2 - v); p -= lr_t m / (sqrt(v) + eps) + wd p, the two terms added first.
// g itself is read only.
__global__ void __launch_bounds__(EW_T) tadam_ex_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, const float* __restrict__ g,
                                                        long long n, float lr_t, float omb1, float omb2, float eps, float wd, double clip,
                                                        const double* __restrict__ norm)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const double nrm = norm[0];
    const float rate = (clip > 0.0 && nrm > clip) ? (float)(clip / nrm) : 1.0f;
    const float gi = rate * g[i];
    const float mi = m[i] + omb1 * (gi - m[i]);
    const float vi = v[i] + omb2 * (gi * gi - v[i]);
    m[i] = mi;
    v[i] = vi;
    const float pi = p[i];
    const float adam = lr_t * mi / (sqrtf(vi) + eps);
    p[i] = pi - (wd != 0.f ? adam + wd * pi : adam);  // wd = 0: tadam_kernel's bits, signed zeros and non-finite weights included
}

}  // namespace eigt
