// cppn_valid_kernel.h -- the validity planes of moving CPPN textures ("The joint objective and the valid pixels"):
// whether the exact flow cppn_motion_kernel states at a pixel of frame t can be recovered from frames t and t + 1 at all.  It depends on
// the affines alone: no CPPN is evaluated, no LDS is used, and cppn_motion_kernel is left as it is.
//
//   px = col - (W - 1) / 2, py = row - (H - 1) / 2                              (exact)
//   (u, v), vis                      as cppn_motion_kernel forms them from A[b][t][.] (layer 1 where u1 u1 + v1 v1 < 1.0)
//   qx = (i0 u + i1 v) + i2, qy = (i3 u + i4 v) + i5                            Ainv[b][t + 1][vis]: where the surface is in frame t + 1
//   inb = qx >= -(W - 1) / 2 && qx <= (W - 1) / 2 && qy >= -(H - 1) / 2 && qy <= (H - 1) / 2
//   occ = L == 2 && vis == 0 && u1' u1' + v1' v1' < 1.0                         (u1', v1') = A[b][t + 1][1] at (qx, qy): layer 1 covers it there
//   valid = inb && !occ                                                         uint8 0 / 1; a NaN compares false -> 0
//
// Every product and sum is one float64 rounding in the order written (the unit is compiled with -ffp-contract=off), so qx and qy are
// the bits cppn_motion_kernel adds px and py to.  One thread is one pixel of one sample (blockIdx.y) and loops over its T - 1 frame
// pairs; the affines are the packed records of eigen_render_moving_cppn, uniform over the block.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cppn_kernel.h"

namespace eig {

struct CppnValidArgs {
    const double* affine;  // [n][T][L][12]: a0 .. a5 (pixel -> texture), then i0 .. i5 (texture -> pixel)
    int W, H, N;           // N = H*W
    int T, L;
    uint8_t* valid;        // [n][T-1][N]
};

__global__ void __launch_bounds__(CPPN_THREADS) cppn_valid_kernel(const CppnValidArgs a)
{
    const int b = blockIdx.y;
    const int p = blockIdx.x * CPPN_THREADS + threadIdx.x;
    if (p >= a.N) return;
    const int row = p / a.W, col = p - row * a.W;
    const double hx = (double)(a.W - 1) / 2.0, hy = (double)(a.H - 1) / 2.0;
    const double px = (double)col - hx;
    const double py = (double)row - hy;
    uint8_t* out = a.valid + (size_t)b * (a.T - 1) * a.N + p;
    const double* A = a.affine + (size_t)b * a.T * a.L * 12;   // uniform over the block

    for (int t = 0; t < a.T - 1; ++t, A += a.L * 12, out += a.N) {
        double u = (A[0] * px + A[1] * py) + A[2];
        double v = (A[3] * px + A[4] * py) + A[5];
        int vis = 0;
        if (a.L == 2) {
            const double u1 = (A[12] * px + A[13] * py) + A[14];
            const double v1 = (A[15] * px + A[16] * py) + A[17];
            if (u1 * u1 + v1 * v1 < 1.0) { vis = 1; u = u1; v = v1; }
        }
        const double* N1 = A + a.L * 12;          // the records of frame t + 1
        const double* I = N1 + vis * 12 + 6;      // the visible layer's inverse
        const double qx = (I[0] * u + I[1] * v) + I[2];
        const double qy = (I[3] * u + I[4] * v) + I[5];
        const bool inb = qx >= -hx && qx <= hx && qy >= -hy && qy <= hy;
        bool occ = false;
        if (a.L == 2 && vis == 0) {
            const double u1 = (N1[12] * qx + N1[13] * qy) + N1[14];
            const double v1 = (N1[15] * qx + N1[16] * qy) + N1[17];
            occ = u1 * u1 + v1 * v1 < 1.0;
        }
        *out = (uint8_t)(inb && !occ);
    }
}

}  // namespace eig
