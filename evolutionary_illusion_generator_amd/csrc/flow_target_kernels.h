// flow_target_kernels.h -- the flow objective's third displacement mode (prednet_train.hip, DESIGN.md section 13, "The target field"):
// the squared endpoint error of the solved field against a per-call target field.  Float64, one IEEE operation per operation written,
// like flow_obj_kernels.h; tests/flow_target_support.py restates it in numpy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "train_common.h"

namespace eigt {

// On the solved field u [B][2][H W] and the target tg (sample b at tg + b * t_bstride doubles, [2][H W]):
//   ex = ux - tx, ey = uy - ty, v = ex ex + ey ey, g = (2 ex, 2 ey)
// mv [n] = v and g [B][2][H W] where the mask counts the pixel (mask nullptr: all), else 0.  n = B H W.  One kernel serves both solves:
// after the single step it replaces the mv tflow_solve_kernel wrote and tflow_struct_q_kernel forms q from g; after the iterated solve
// g is what iter_backward takes, as from tfiter_value_kernel.  The target is not inspected: a non-finite element propagates.
__global__ void __launch_bounds__(EW_T) tflow_target_kernel(const double* __restrict__ u, const double* __restrict__ tg, long long t_bstride,
                                                            const uint8_t* __restrict__ mask, long long mask_bstride, long long HW, long long n,
                                                            double* __restrict__ mv, double* __restrict__ g)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const long long b = i / HW, p = i - b * HW;
    const double ex = u[2 * b * HW + p] - tg[b * t_bstride + p], ey = u[2 * b * HW + HW + p] - tg[b * t_bstride + HW + p];
    const bool counted = !mask || mask[b * mask_bstride + p] != 0;
    mv[i] = counted ? ex * ex + ey * ey : 0.0;
    g[2 * b * HW + p] = counted ? 2.0 * ex : 0.0;
    g[2 * b * HW + HW + p] = counted ? 2.0 * ey : 0.0;
}

}  // namespace eigt
