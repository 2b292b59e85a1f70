// flow_ref_kernels.h -- HIP kernels of the flow objective's "moving reference" mode (prednet_train.hip, DESIGN.md section 13, "The moving
// reference"): the exact gradient of one flow term by its REFERENCE frame, which flow_obj_kernels.h treats as a constant.  They run after
// the flow stage of the same term and read what it left: the planes Ix, Iy, It, the masked q and the flow u.  All arithmetic is float64,
// one IEEE operation per operation written (the build's -ffp-contract=off); tests/flow_ref_support.py restates it in numpy and the result
// is compared bit for bit.  Fixed partitions, fixed orders, no float atomics.
//
// With Q = the window sums of q and the three sums M of the products of q and u below, the term moves with the reference's gray I0 by
//   d f / d I0 = e + S^T(rx, ry),   e = (Ix Qx + Iy Qy) kappa                         (the path through It = I1 - I0)
//   rx = -(((Qx It + Mxx Ix) + Mxy Iy) kappa),  ry = -(((Qy It + Mxy Ix) + Myy Iy) kappa)   (d f / d Ix, d f / d Iy)
// and S^T is the adjoint of the normalised Scharr pair with its indices clamped to the image.
//
// The order of additions of S^T, fixed here and restated in numpy.  Take r as zero outside the image and let (Y, X) run over the padded
// positions -1 .. H, -1 .. W.  With RX(j, i) = rx(Y + j, X + i), RY alike:
//   gx = ((3 (RX(-1,-1) - RX(-1,+1)) + 10 (RX(0,-1) - RX(0,+1))) + 3 (RX(+1,-1) - RX(+1,+1))) / 32
//   gy = ((3 (RY(-1,-1) - RY(+1,-1)) + 10 (RY(-1,0) - RY(+1,0))) + 3 (RY(-1,+1) - RY(+1,+1))) / 32
//   G(Y, X) = gx + gy
// A pixel (y, x) collects the padded positions the forward pass clamps onto it: Y = y, and -1 where y = 0, and H where y = H - 1; X alike.
// Per Y, ascending, the G of its X, ascending, are added, the sum started from its first term; those row sums are added over Y,
// ascending, the same way.  d f / d I0 = e + that sum.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flow_obj_kernels.h"

namespace eigt {

// The five window sums (the order of tflow_solve_kernel: rows first, then columns, offsets ascending, each sum started from its first
// term) of qx, qy, 2 (qx ux), qx uy + qy ux, 2 (qy uy) of every pixel of one tile (blockIdx: tile x, tile y, sample), then rx, ry and e
// into r [3][n].  planes [3][n], q [2][n] as the flow stage left them; u [B][2][H][W].
__global__ void __launch_bounds__(FLOW_T) tflow_ref_sums_kernel(const double* __restrict__ planes, const double* __restrict__ q, const double* __restrict__ u,
                                                                long long n, int H, int W, int r, double kappa, double* __restrict__ out)
{
    __shared__ double rs[5][FLOW_ROWS][FLOW_TILE];
    const int tx = threadIdx.x & (FLOW_TILE - 1), ty = threadIdx.x / FLOW_TILE;
    const int x0 = blockIdx.x * FLOW_TILE, y0 = blockIdx.y * FLOW_TILE;
    const long long HW = (long long)H * W, base = (long long)blockIdx.z * HW;
    const double *qx = q + base, *qy = q + n + base, *ux = u + 2 * base, *uy = u + 2 * base + HW;
    const int rows = FLOW_TILE + 2 * r;
    for (int item = threadIdx.x; item < rows * FLOW_TILE; item += FLOW_T) {
        const int ry = item / FLOW_TILE, cx = item & (FLOW_TILE - 1);
        const int y = y0 - r + ry, x = x0 + cx;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
        if (y >= 0 && y < H && x < W) {
            const int lo = x - r > 0 ? x - r : 0, hi = x + r < W - 1 ? x + r : W - 1;
            const long long row = (long long)y * W;
            {
                const double a = qx[row + lo], b = qy[row + lo], c = ux[row + lo], d = uy[row + lo];
                s0 = a; s1 = b; s2 = 2.0 * (a * c); s3 = a * d + b * c; s4 = 2.0 * (b * d);
            }
            for (int xx = lo + 1; xx <= hi; ++xx) {
                const double a = qx[row + xx], b = qy[row + xx], c = ux[row + xx], d = uy[row + xx];
                s0 += a; s1 += b; s2 += 2.0 * (a * c); s3 += a * d + b * c; s4 += 2.0 * (b * d);
            }
        }
        rs[0][ry][cx] = s0; rs[1][ry][cx] = s1; rs[2][ry][cx] = s2; rs[3][ry][cx] = s3; rs[4][ry][cx] = s4;
    }
    __syncthreads();
    const int x = x0 + tx, y = y0 + ty;
    if (x >= W || y >= H) return;
    const int lo = y - r > 0 ? y - r : 0, hi = y + r < H - 1 ? y + r : H - 1;
    int k = lo - (y0 - r);
    double Qx = rs[0][k][tx], Qy = rs[1][k][tx], Mxx = rs[2][k][tx], Mxy = rs[3][k][tx], Myy = rs[4][k][tx];
    for (int yy = lo + 1; yy <= hi; ++yy) {
        ++k;
        Qx += rs[0][k][tx]; Qy += rs[1][k][tx]; Mxx += rs[2][k][tx]; Mxy += rs[3][k][tx]; Myy += rs[4][k][tx];
    }
    const long long p = base + (long long)y * W + x;
    const double Ix = planes[p], Iy = planes[n + p], It = planes[2 * n + p];
    out[p] = -(((Qx * It + Mxx * Ix) + Mxy * Iy) * kappa);
    out[n + p] = -(((Qy * It + Mxy * Ix) + Myy * Iy) * kappa);
    out[2 * n + p] = (Ix * Qx + Iy * Qy) * kappa;
}

// v (y, x) of one [H][W] plane, zero outside the image
__device__ __forceinline__ double tflow_ref_at(const double* __restrict__ v, int H, int W, int y, int x)
{
    return (y >= 0 && y < H && x >= 0 && x < W) ? v[(long long)y * W + x] : 0.0;
}

// G of the padded position (Y, X), the header's formula
__device__ __forceinline__ double tflow_ref_gather(const double* __restrict__ rx, const double* __restrict__ ry, int H, int W, int Y, int X)
{
    const double gx = ((3.0 * (tflow_ref_at(rx, H, W, Y - 1, X - 1) - tflow_ref_at(rx, H, W, Y - 1, X + 1)) +
                        10.0 * (tflow_ref_at(rx, H, W, Y, X - 1) - tflow_ref_at(rx, H, W, Y, X + 1))) +
                       3.0 * (tflow_ref_at(rx, H, W, Y + 1, X - 1) - tflow_ref_at(rx, H, W, Y + 1, X + 1))) / 32.0;
    const double gy = ((3.0 * (tflow_ref_at(ry, H, W, Y - 1, X - 1) - tflow_ref_at(ry, H, W, Y + 1, X - 1)) +
                        10.0 * (tflow_ref_at(ry, H, W, Y - 1, X) - tflow_ref_at(ry, H, W, Y + 1, X))) +
                       3.0 * (tflow_ref_at(ry, H, W, Y - 1, X + 1) - tflow_ref_at(ry, H, W, Y + 1, X + 1))) / 32.0;
    return gx + gy;
}

// d = e + S^T(rx, ry) of every pixel i < n = B H W (the header's order), then (float)(k_c d) of every channel, k = (0.299, 0.587, 0.114)
// or (1): scale * d value / d reference, by x = (float)byte / 255.0f.  Sample b at out + b * out_bstride as [C][H][W]; accumulate = 1:
// out += that (a float addition), 0: a plain store.
__global__ void __launch_bounds__(EW_T) tflow_ref_fold_kernel(const double* __restrict__ r, long long n, int H, int W, int C, float* __restrict__ out,
                                                              long long out_bstride, int accumulate)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const long long HW = (long long)H * W;
    const long long b = i / HW, p = i - b * HW;
    const int y = (int)(p / W), x = (int)(p - (long long)y * W);
    const double *rx = r + b * HW, *ry = r + n + b * HW;
    const int Y0 = y == 0 ? -1 : y, Y1 = y == H - 1 ? H : y, X0 = x == 0 ? -1 : x, X1 = x == W - 1 ? W : x;
    double tot = 0.0;
    for (int Y = Y0; Y <= Y1; ++Y) {
        double row = tflow_ref_gather(rx, ry, H, W, Y, X0);
        for (int X = X0 + 1; X <= X1; ++X) row += tflow_ref_gather(rx, ry, H, W, Y, X);
        tot = Y == Y0 ? row : tot + row;
    }
    const double d = r[2 * n + i] + tot;
    float* o = out + b * out_bstride + p;
    if (C == 1) {
        const float g = (float)d;
        o[0] = accumulate ? o[0] + g : g;
    } else {
        const float g0 = (float)(0.299 * d), g1 = (float)(0.587 * d), g2 = (float)(0.114 * d);
        o[0] = accumulate ? o[0] + g0 : g0;
        o[HW] = accumulate ? o[HW] + g1 : g1;
        o[2 * HW] = accumulate ? o[2 * HW] + g2 : g2;
    }
}

}  // namespace eigt
