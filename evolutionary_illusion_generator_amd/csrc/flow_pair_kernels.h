// flow_pair_kernels.h -- the HIP kernel of the flow objective's prediction pairing (prednet_train.hip, DESIGN.md section 13, "The
// prediction pairing"): term s runs from the previous PREDICTION P0_{s-1}, a float image that is itself part of the graph, to P0_s, as
// the population fitness pairs its two images.  Everything downstream of the three planes is shared with the frame pairing: the tiled
// solve, the value and the seed of flow_obj_kernels.h, and the reference gradient of flow_ref_kernels.h, which a training call adds to
// dP0_{s-1} after layer 0's terr_bwd of step s has written it.  So the pairing needs one kernel of its own: the planes from two float
// images.  Float64, one IEEE operation per operation written (the build's -ffp-contract=off); tests/flow_pair_support.py restates it in
// numpy and the fields are compared bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flow_obj_kernels.h"

namespace eigt {

// tflow_prep_kernel with a float reference: planes [3][n], n = B H W: Ix, Iy (normalised Scharr of the reference's gray I0, the floats
// widened, indices clamped to the image) and It = I1 - I0 with I1 the gray of the prediction.  Sample b: prediction at
// pred + b * pred_bstride, reference at ref + b * ref_bstride (floats both).  One thread per pixel; consecutive lanes read consecutive
// floats of each of the three rows the stencil touches and write consecutive doubles of each plane.
__global__ void __launch_bounds__(EW_T) tflow_pair_prep_kernel(const float* __restrict__ pred, long long pred_bstride, const float* __restrict__ ref,
                                                               long long ref_bstride, int C, int H, int W, long long n, double* __restrict__ planes)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const long long HW = (long long)H * W;
    const long long b = i / HW, p = i - b * HW;
    const int y = (int)(p / W), x = (int)(p - (long long)y * W);
    const float* rb = ref + b * ref_bstride;
    const int ym = y > 0 ? y - 1 : 0, yp = y < H - 1 ? y + 1 : H - 1, xm = x > 0 ? x - 1 : 0, xp = x < W - 1 ? x + 1 : W - 1;
    const double a_mm = tflow_gray(rb, C, HW, (long long)ym * W + xm), a_m0 = tflow_gray(rb, C, HW, (long long)ym * W + x),
                 a_mp = tflow_gray(rb, C, HW, (long long)ym * W + xp), a_0m = tflow_gray(rb, C, HW, (long long)y * W + xm),
                 a_00 = tflow_gray(rb, C, HW, p), a_0p = tflow_gray(rb, C, HW, (long long)y * W + xp),
                 a_pm = tflow_gray(rb, C, HW, (long long)yp * W + xm), a_p0 = tflow_gray(rb, C, HW, (long long)yp * W + x),
                 a_pp = tflow_gray(rb, C, HW, (long long)yp * W + xp);
    planes[i] = ((3.0 * (a_mp - a_mm) + 10.0 * (a_0p - a_0m)) + 3.0 * (a_pp - a_pm)) / 32.0;
    planes[n + i] = ((3.0 * (a_pm - a_mm) + 10.0 * (a_p0 - a_m0)) + 3.0 * (a_pp - a_mp)) / 32.0;
    planes[2 * n + i] = tflow_gray(pred + b * pred_bstride, C, HW, p) - a_00;
}

}  // namespace eigt
