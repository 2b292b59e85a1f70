// flow_obj_kernels.h -- HIP kernels of the differentiable motion objective of PredNet training (prednet_train.hip, DESIGN.md section 13,
// "The flow objective"): a dense, regularised Lucas-Kanade solve from a reference frame (bytes, a constant of the graph) to a float
// prediction, reduced to the mean squared displacement or to the mean displacement along a direction field, and the exact gradient of
// that value by the prediction.  All arithmetic is float64, one IEEE operation per operation written (the build's -ffp-contract=off);
// tests/flow_obj_support.py restates it in numpy and the fields are compared bit for bit.  Like train_kernels.h: fixed partitions, fixed
// orders, no float atomics.
//
// Tiles: FLOW_TILE x FLOW_TILE = 16 x 16 pixels per block of 256 threads (four waves).  A window sum of radius r <= FLOW_MAX_R is
// separable: the block first forms the row sums of its 16 columns over the 16 + 2 r rows the tile's windows reach (read from the float64
// planes, which sit in L2), keeps them in LDS ([fields][48][16] doubles: 30 KB for the five fields of the solve, 12 KB for the two of
// the seed), then every thread adds the row sums of its column.  Windows are truncated at the image border, never padded: a sum runs
// over the in-image offsets in ascending order and starts from its first term.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "train_common.h"

namespace eigt {

constexpr int FLOW_TILE = 16;
constexpr int FLOW_MAX_R = 16;
constexpr int FLOW_ROWS = FLOW_TILE + 2 * FLOW_MAX_R;  // rows of row sums one tile can need
constexpr int FLOW_T = FLOW_TILE * FLOW_TILE;          // threads per block of the tiled kernels

// gray value of pixel p of one image [C][H][W], C = 1 or 3, from bytes (v = (float)byte / 255.0f, widened) or from floats
__device__ __forceinline__ double tflow_gray(const uint8_t* __restrict__ x, int C, long long HW, long long p)
{
    const double v0 = (double)((float)x[p] / 255.0f);
    if (C == 1) return v0;
    const double v1 = (double)((float)x[HW + p] / 255.0f), v2 = (double)((float)x[2 * HW + p] / 255.0f);
    return (0.299 * v0 + 0.587 * v1) + 0.114 * v2;
}

__device__ __forceinline__ double tflow_gray(const float* __restrict__ x, int C, long long HW, long long p)
{
    const double v0 = (double)x[p];
    if (C == 1) return v0;
    const double v1 = (double)x[HW + p], v2 = (double)x[2 * HW + p];
    return (0.299 * v0 + 0.587 * v1) + 0.114 * v2;
}

// planes [3][n], n = B H W: Ix, Iy (normalised Scharr of the reference's gray I0, indices clamped to the image) and It = I1 - I0 with I1
// the gray of the prediction.  Sample b: prediction at pred + b * pred_bstride (floats), reference at ref + b * ref_bstride (bytes).
__global__ void __launch_bounds__(EW_T) tflow_prep_kernel(const float* __restrict__ pred, long long pred_bstride, const uint8_t* __restrict__ ref,
                                                          long long ref_bstride, int C, int H, int W, long long n, double* __restrict__ planes)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const long long HW = (long long)H * W;
    const long long b = i / HW, p = i - b * HW;
    const int y = (int)(p / W), x = (int)(p - (long long)y * W);
    const uint8_t* rb = ref + b * ref_bstride;
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

// The five window sums, the solve, the value and q of every pixel of one tile (blockIdx: tile x, tile y, sample).
//   Gxx = sum Ix Ix, Gxy = sum Ix Iy, Gyy = sum Iy Iy, bx = sum Ix It, by = sum Iy It over the truncated window
//   a = Gxx + eps, c = Gyy + eps, b = Gxy, det = a c - b b, ux = -((c bx - b by) / det), uy = -((a by - b bx) / det)
//   value v = ux ux + uy uy (dir == nullptr) or dx ux + dy uy (dir float [2][H][W]); mv = v where the mask byte is not 0 (mask nullptr: all), else 0
//   g = (2 ux, 2 uy) or d; q = ((c gx - b gy) / det, (a gy - b gx) / det) where the mask counts, else 0
// q [2][n], mv [n]; flow (may be null) [B][2][H][W].  The mask byte of sample b, pixel p is mask[b * mask_bstride + p]: stride 0 is one plane
// shared by the batch.
__global__ void __launch_bounds__(FLOW_T) tflow_solve_kernel(const double* __restrict__ planes, long long n, int H, int W, int r, double eps,
                                                             const float* __restrict__ dir, const uint8_t* __restrict__ mask, long long mask_bstride, double* __restrict__ q,
                                                             double* __restrict__ mv, double* __restrict__ flow)
{
    __shared__ double rs[5][FLOW_ROWS][FLOW_TILE];
    const int tx = threadIdx.x & (FLOW_TILE - 1), ty = threadIdx.x / FLOW_TILE;
    const int x0 = blockIdx.x * FLOW_TILE, y0 = blockIdx.y * FLOW_TILE;
    const long long HW = (long long)H * W, base = (long long)blockIdx.z * HW;
    const double *Ix = planes + base, *Iy = planes + n + base, *It = planes + 2 * n + base;
    const int rows = FLOW_TILE + 2 * r;
    for (int item = threadIdx.x; item < rows * FLOW_TILE; item += FLOW_T) {
        const int ry = item / FLOW_TILE, cx = item & (FLOW_TILE - 1);
        const int y = y0 - r + ry, x = x0 + cx;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
        if (y >= 0 && y < H && x < W) {
            const int lo = x - r > 0 ? x - r : 0, hi = x + r < W - 1 ? x + r : W - 1;
            const long long row = (long long)y * W;
            {
                const double ix = Ix[row + lo], iy = Iy[row + lo], it = It[row + lo];
                s0 = ix * ix; s1 = ix * iy; s2 = iy * iy; s3 = ix * it; s4 = iy * it;
            }
            for (int xx = lo + 1; xx <= hi; ++xx) {
                const double ix = Ix[row + xx], iy = Iy[row + xx], it = It[row + xx];
                s0 += ix * ix; s1 += ix * iy; s2 += iy * iy; s3 += ix * it; s4 += iy * it;
            }
        }
        rs[0][ry][cx] = s0; rs[1][ry][cx] = s1; rs[2][ry][cx] = s2; rs[3][ry][cx] = s3; rs[4][ry][cx] = s4;
    }
    __syncthreads();
    const int x = x0 + tx, y = y0 + ty;
    if (x >= W || y >= H) return;
    const int lo = y - r > 0 ? y - r : 0, hi = y + r < H - 1 ? y + r : H - 1;
    int k = lo - (y0 - r);
    double Gxx = rs[0][k][tx], Gxy = rs[1][k][tx], Gyy = rs[2][k][tx], bx = rs[3][k][tx], by = rs[4][k][tx];
    for (int yy = lo + 1; yy <= hi; ++yy) {
        ++k;
        Gxx += rs[0][k][tx]; Gxy += rs[1][k][tx]; Gyy += rs[2][k][tx]; bx += rs[3][k][tx]; by += rs[4][k][tx];
    }
    const double a = Gxx + eps, c = Gyy + eps, b = Gxy;
    const double det = a * c - b * b;
    const double ux = -((c * bx - b * by) / det), uy = -((a * by - b * bx) / det);
    const long long p = (long long)y * W + x;
    double v, gx, gy;
    if (dir) {
        gx = (double)dir[p]; gy = (double)dir[HW + p];
        v = gx * ux + gy * uy;
    } else {
        gx = 2.0 * ux; gy = 2.0 * uy;
        v = ux * ux + uy * uy;
    }
    const bool counted = !mask || mask[(long long)blockIdx.z * mask_bstride + p] != 0;
    mv[base + p] = counted ? v : 0.0;
    q[base + p] = counted ? (c * gx - b * gy) / det : 0.0;
    q[n + base + p] = counted ? (a * gy - b * gx) / det : 0.0;
    if (flow) {
        flow[2 * base + p] = ux;
        flow[2 * base + HW + p] = uy;
    }
}

// Q = the window sums of q (the same order: rows first, then columns; window membership is symmetric), t = Ix Qx + Iy Qy,
// s = -(t kappa), and the seed (float)(k_c s) of every channel, k = (0.299, 0.587, 0.114) or (1): d value / d prediction.  Sample b at
// out + b * out_bstride as [C][H][W]; accumulate = 1: out += seed (a float addition), 0: a plain store.
__global__ void __launch_bounds__(FLOW_T) tflow_seed_kernel(const double* __restrict__ planes, const double* __restrict__ q, long long n, int H, int W, int C,
                                                            int r, double kappa, float* __restrict__ out, long long out_bstride, int accumulate)
{
    __shared__ double rs[2][FLOW_ROWS][FLOW_TILE];
    const int tx = threadIdx.x & (FLOW_TILE - 1), ty = threadIdx.x / FLOW_TILE;
    const int x0 = blockIdx.x * FLOW_TILE, y0 = blockIdx.y * FLOW_TILE;
    const long long HW = (long long)H * W, base = (long long)blockIdx.z * HW;
    const double *qx = q + base, *qy = q + n + base;
    const int rows = FLOW_TILE + 2 * r;
    for (int item = threadIdx.x; item < rows * FLOW_TILE; item += FLOW_T) {
        const int ry = item / FLOW_TILE, cx = item & (FLOW_TILE - 1);
        const int y = y0 - r + ry, x = x0 + cx;
        double s0 = 0.0, s1 = 0.0;
        if (y >= 0 && y < H && x < W) {
            const int lo = x - r > 0 ? x - r : 0, hi = x + r < W - 1 ? x + r : W - 1;
            const long long row = (long long)y * W;
            s0 = qx[row + lo]; s1 = qy[row + lo];
            for (int xx = lo + 1; xx <= hi; ++xx) { s0 += qx[row + xx]; s1 += qy[row + xx]; }
        }
        rs[0][ry][cx] = s0; rs[1][ry][cx] = s1;
    }
    __syncthreads();
    const int x = x0 + tx, y = y0 + ty;
    if (x >= W || y >= H) return;
    const int lo = y - r > 0 ? y - r : 0, hi = y + r < H - 1 ? y + r : H - 1;
    int k = lo - (y0 - r);
    double Qx = rs[0][k][tx], Qy = rs[1][k][tx];
    for (int yy = lo + 1; yy <= hi; ++yy) {
        ++k;
        Qx += rs[0][k][tx]; Qy += rs[1][k][tx];
    }
    const long long p = (long long)y * W + x;
    const double t = planes[base + p] * Qx + planes[n + base + p] * Qy;
    const double s = -(t * kappa);
    float* o = out + (long long)blockIdx.z * out_bstride + p;
    if (C == 1) {
        const float g = (float)s;
        o[0] = accumulate ? o[0] + g : g;
    } else {
        const float g0 = (float)(0.299 * s), g1 = (float)(0.587 * s), g2 = (float)(0.114 * s);
        o[0] = accumulate ? o[0] + g0 : g0;
        o[HW] = accumulate ? o[HW] + g1 : g1;
        o[2 * HW] = accumulate ? o[2 * HW] + g2 : g2;
    }
}

// part[k] = the sum of block k's fixed strided slice of v [n] in double, then a fixed LDS tree (the pattern of tloss_step_partial_kernel);
// tloss_step_final_kernel adds the partials in order and divides
__global__ void __launch_bounds__(EW_T) tflow_sum_kernel(const double* __restrict__ v, long long n, double* __restrict__ part)
{
    __shared__ double red[EW_T];
    double s = 0.0;
    for (long long i = (long long)blockIdx.x * EW_T + threadIdx.x; i < n; i += (long long)gridDim.x * EW_T) s += v[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = EW_T / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

}  // namespace eigt
