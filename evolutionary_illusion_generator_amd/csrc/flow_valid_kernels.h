// flow_valid_kernels.h -- per-sample validity planes under the flow objective's target field (prednet_train.hip, DESIGN.md section 13,
// "The joint objective and the valid pixels"): a pixel counts where the shared mask M counts it and the validity plane V_b of its own
// sample is not zero, and every sample's squared endpoint error is averaged over its own counted pixels.  Float64, one IEEE operation per
// operation written, like flow_target_kernels.h, which is left as it is; tests/flow_joint_support.py restates both kernels in numpy.
//
//   c_b = #{p : M(p) != 0 and V_b(p) != 0}                      an integer, summed without atomics
//   r_b = c_b > 0 ? (double)N_m / (double)c_b : 0.0             N_m: the count of M (H W without one)
//   ex = ux - tx, ey = uy - ty, v = ex ex + ey ey
//   mv = counted ? v r_b : 0, g = counted ? ((2 ex) r_b, (2 ey) r_b) : 0
//
// so that the unchanged tail (tflow_sum_kernel, the division by B N_m, kappa, tflow_struct_q_kernel, iter_backward) yields the mean over
// the samples of each sample's mean over its own counted pixels.  A sample that counts no pixel gives exact zeros; all-ones planes give
// r_b = 1.0 exactly, and v 1.0 and (2 ex) 1.0 are v and 2 ex, the bytes of tflow_target_kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "train_common.h"

namespace eigt {

// One block per sample: the count of its counted pixels, then r_b.  The validity byte of sample b, pixel p is valid[b * v_bstride + p];
// the mask as in tflow_target_kernel (nullptr: all).  Integer sums are exact in any order: the block's tree is as good as any.
__global__ void __launch_bounds__(EW_T) tflow_valid_count_kernel(const uint8_t* __restrict__ valid, long long v_bstride, const uint8_t* __restrict__ mask,
                                                                 long long mask_bstride, long long HW, long long n_mask, double* __restrict__ r)
{
    __shared__ int red[EW_T];
    const long long b = blockIdx.x;
    int c = 0;
    for (long long p = threadIdx.x; p < HW; p += EW_T) c += ((!mask || mask[b * mask_bstride + p] != 0) && valid[b * v_bstride + p] != 0) ? 1 : 0;
    red[threadIdx.x] = c;
    __syncthreads();
    for (int w = EW_T / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) r[b] = red[0] > 0 ? (double)n_mask / (double)red[0] : 0.0;
}

// tflow_target_kernel under the planes: the same arguments plus valid, its stride and r [B] from tflow_valid_count_kernel.  One kernel
// serves both solves, at the two places tflow_target_kernel is launched.
__global__ void __launch_bounds__(EW_T) tflow_target_valid_kernel(const double* __restrict__ u, const double* __restrict__ tg, long long t_bstride,
                                                                  const uint8_t* __restrict__ mask, long long mask_bstride, const uint8_t* __restrict__ valid,
                                                                  long long v_bstride, const double* __restrict__ r, long long HW, long long n,
                                                                  double* __restrict__ mv, double* __restrict__ g)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const long long b = i / HW, p = i - b * HW;
    const double ex = u[2 * b * HW + p] - tg[b * t_bstride + p], ey = u[2 * b * HW + HW + p] - tg[b * t_bstride + HW + p];
    const bool counted = (!mask || mask[b * mask_bstride + p] != 0) && valid[b * v_bstride + p] != 0;
    const double rb = r[b];
    mv[i] = counted ? (ex * ex + ey * ey) * rb : 0.0;
    g[2 * b * HW + p] = counted ? (2.0 * ex) * rb : 0.0;
    g[2 * b * HW + HW + p] = counted ? (2.0 * ey) * rb : 0.0;
}

}  // namespace eigt
