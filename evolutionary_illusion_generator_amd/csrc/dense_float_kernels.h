// dense_float_kernels.h -- HIP kernels of the dense motion fitness on float frames (EIGEN_DENSE_FLOAT_FRAMES, eigen_dense_score_float,
// DESIGN.md section 14, "Float frames"): the stage starts from the two float64 gray planes I0, I1 [B][H W] of its pair in place of two
// byte batches, so that the roll-out can leave the gray of a float prediction P0 behind the ConvP0 launch that wrote it and nothing of
// the image itself has to be kept.
//   tdense_gray_of_kernel    the gray plane of one batch of planar images, float or byte: tflow_gray of every pixel
//   tdense_prep_gray_kernel  Ix, Iy, It from the two gray planes: tdense_prep_kernel / tflow_pair_prep_kernel with the nine neighbours read
//                            from I0 in place of re-formed; the gray is a pure function of the pixel, so the planes are their bytes
// Everything behind the planes (tdense_solve_kernel, tdense_pyrdown_kernel, tdense_iter_kernel, the score passes, the members) is launched
// as it is.  Float64, one IEEE operation per operation written (the build's -ffp-contract=off), fixed orders.  Both are one-pass,
// HBM-bound: one thread per pixel, consecutive lanes on consecutive elements.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flow_obj_kernels.h"

namespace eigt {

// I [n], n = B H W: the gray of image b at img + b * stride (elements), planar [C][H][W]
template <typename T>
__global__ void __launch_bounds__(EW_T) tdense_gray_of_kernel(const T* __restrict__ img, long long stride, int C, long long HW, long long n, double* __restrict__ I)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const long long b = i / HW, p = i - b * HW;
    I[i] = tflow_gray(img + b * stride, C, HW, p);
}

// planes [3][n], n = B H W: Ix, Iy (normalised Scharr of I0, indices clamped to the image) and It = I1 - I0
__global__ void __launch_bounds__(EW_T) tdense_prep_gray_kernel(const double* __restrict__ I0, const double* __restrict__ I1, int H, int W, long long n,
                                                                double* __restrict__ planes)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const long long HW = (long long)H * W;
    const long long b = i / HW, p = i - b * HW;
    const int y = (int)(p / W), x = (int)(p - (long long)y * W);
    const double* rb = I0 + b * HW;
    const int ym = y > 0 ? y - 1 : 0, yp = y < H - 1 ? y + 1 : H - 1, xm = x > 0 ? x - 1 : 0, xp = x < W - 1 ? x + 1 : W - 1;
    const double a_mm = rb[(long long)ym * W + xm], a_m0 = rb[(long long)ym * W + x], a_mp = rb[(long long)ym * W + xp], a_0m = rb[(long long)y * W + xm], a_00 = rb[p],
                 a_0p = rb[(long long)y * W + xp], a_pm = rb[(long long)yp * W + xm], a_p0 = rb[(long long)yp * W + x], a_pp = rb[(long long)yp * W + xp];
    planes[i] = ((3.0 * (a_mp - a_mm) + 10.0 * (a_0p - a_0m)) + 3.0 * (a_pp - a_pm)) / 32.0;
    planes[n + i] = ((3.0 * (a_pm - a_mm) + 10.0 * (a_p0 - a_m0)) + 3.0 * (a_pp - a_mp)) / 32.0;
    planes[2 * n + i] = I1[i] - a_00;
}

}  // namespace eigt
