// dense_fitness_kernels.h -- HIP kernels of the dense motion fitness of the population path (eigen_dense_score):
// the flow objective's score (flow_obj_kernels.h, flow_score_kernels.h, flow_struct_kernels.h) as the fitness of a genome, formed from
// the two uint8 frames the fitness compares.  Only the value is wanted, so these are the score-only forms of three kernels of those
// headers; every sum keeps the header's order and the results are the trainer's stage bit for bit (tests/test_gpu_dense_fitness.py):
//   tdense_prep_kernel      tflow_pair_prep_kernel with both images read as bytes, (float)byte / 255.0f widened: no float copy exists
//   tdense_solve_kernel     tflow_solve_kernel without value, q, direction and mask: the field u alone
//   tdense_free_pair_kernel tflow_free_pair_kernel without the sign sums of the gradient: L alone, half the work per pair
// The moment and final kernels of the two score headers are launched as they are.  Float64, one IEEE operation per operation written
// (the build's -ffp-contract=off), fixed partitions, fixed orders, no float atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flow_obj_kernels.h"
#include "flow_struct_kernels.h"

namespace eigt {

// planes [3][n], n = B H W: Ix, Iy (normalised Scharr of the gray I0 of img0, indices clamped to the image) and It = I1 - I0 with I1
// the gray of img1.  Image b of either batch at its pointer + b * its stride (bytes), planar [C][H][W].
__global__ void __launch_bounds__(EW_T) tdense_prep_kernel(const uint8_t* __restrict__ img0, long long stride0, const uint8_t* __restrict__ img1, long long stride1, int C,
                                                           int H, int W, long long n, double* __restrict__ planes)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const long long HW = (long long)H * W;
    const long long b = i / HW, p = i - b * HW;
    const int y = (int)(p / W), x = (int)(p - (long long)y * W);
    const uint8_t* rb = img0 + b * stride0;
    const int ym = y > 0 ? y - 1 : 0, yp = y < H - 1 ? y + 1 : H - 1, xm = x > 0 ? x - 1 : 0, xp = x < W - 1 ? x + 1 : W - 1;
    const double a_mm = tflow_gray(rb, C, HW, (long long)ym * W + xm), a_m0 = tflow_gray(rb, C, HW, (long long)ym * W + x),
                 a_mp = tflow_gray(rb, C, HW, (long long)ym * W + xp), a_0m = tflow_gray(rb, C, HW, (long long)y * W + xm),
                 a_00 = tflow_gray(rb, C, HW, p), a_0p = tflow_gray(rb, C, HW, (long long)y * W + xp),
                 a_pm = tflow_gray(rb, C, HW, (long long)yp * W + xm), a_p0 = tflow_gray(rb, C, HW, (long long)yp * W + x),
                 a_pp = tflow_gray(rb, C, HW, (long long)yp * W + xp);
    planes[i] = ((3.0 * (a_mp - a_mm) + 10.0 * (a_0p - a_0m)) + 3.0 * (a_pp - a_pm)) / 32.0;
    planes[n + i] = ((3.0 * (a_pm - a_mm) + 10.0 * (a_p0 - a_m0)) + 3.0 * (a_pp - a_mp)) / 32.0;
    planes[2 * n + i] = tflow_gray(img1 + b * stride1, C, HW, p) - a_00;
}

// The five window sums and the solve of every pixel of one tile (blockIdx: tile x, tile y, sample), in tflow_solve_kernel's order: rows
// first, then columns, offsets ascending, each sum started from its first term.  flow [B][2][H][W].
__global__ void __launch_bounds__(FLOW_T) tdense_solve_kernel(const double* __restrict__ planes, long long n, int H, int W, int r, double eps, double* __restrict__ flow)
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
    const long long p = (long long)y * W + x;
    flow[2 * base + p] = -((c * bx - b * by) / det);
    flow[2 * base + HW + p] = -((a * by - b * bx) / det);
}

// The pair pass of the Free structure for the value alone (blockIdx: block of PAIR_T pixels, sample): L_k of tflow_free_pair_kernel, the
// members m walked in ascending pixel order in tiles of PAIR_T staged in LDS, every lane reading the same LDS word.
__global__ void __launch_bounds__(PAIR_T) tdense_free_pair_kernel(const double* __restrict__ theta, const uint8_t* __restrict__ flag, int H, int W, double DD,
                                                                  double* __restrict__ L)
{
    __shared__ double sth[PAIR_T];
    __shared__ int sfl[PAIR_T];
    const int HW = H * W;
    const long long base = (long long)blockIdx.y * HW;
    const int k = blockIdx.x * PAIR_T + threadIdx.x;
    const bool own = k < HW && flag[base + k] != 0;
    const double th_k = own ? theta[base + k] : 0.0;
    const int yk = k / W, xk = k - yk * W;
    double Lk = 0.0;
    for (int p0 = 0; p0 < HW; p0 += PAIR_T) {
        const int p = p0 + threadIdx.x;
        sth[threadIdx.x] = p < HW ? theta[base + p] : 0.0;
        sfl[threadIdx.x] = p < HW ? (int)flag[base + p] : 0;
        __syncthreads();
        if (own) {
            const int cnt = HW - p0 < PAIR_T ? HW - p0 : PAIR_T;
            int ym = p0 / W, xm = p0 - ym * W;
            for (int j = 0; j < cnt; ++j) {
                if (sfl[j]) {
                    const double ddx = (double)(xm - xk), ddy = (double)(ym - yk);
                    double f = (ddx * ddx + ddy * ddy) / DD;
                    f = f > 1.0 ? 1.0 : f;
                    if (f < 1.0) {
                        double o = th_k + f * STRUCT_PI;
                        o = (o - 2.0 * floor(o * 0.5)) * STRUCT_PI;
                        Lk += fabs(sth[j] - o);
                    }
                }
                if (++xm == W) { xm = 0; ++ym; }
            }
        }
        __syncthreads();
    }
    if (k < HW) L[base + k] = Lk;
}

}  // namespace eigt
