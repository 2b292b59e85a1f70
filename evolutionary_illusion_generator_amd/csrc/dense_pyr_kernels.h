// dense_pyr_kernels.h -- HIP kernels of the dense motion fitness's opt-in solve (eigen_dense_solve, DESIGN.md section 14, "The
// pyramidal, iterated solve"): Lucas-Kanade over `levels` pyramid levels with `iters` iterations per level, in the per-pixel window form:
// the whole window of pixel p is sampled at q + u(p), OpenCV's iteration applied at every pixel.  Score only: the field of level 0 goes
// into the unchanged moment, prepare, pair and final kernels.
//   tdense_gray_kernel     the two float64 gray planes of level 0 from the bytes: what tdense_prep_kernel reads
//   tdense_pyrdown_kernel  both images of one level reduced: 5 taps (1, 4, 6, 4, 1) / 16 about source index 2 i, reflect-101, x then y
//   tdense_iter_kernel     one level: Scharr pair and window sums G of I0, then every iteration of every pixel of a 16 x 16 tile
// Float64, one IEEE operation per operation written (the build's -ffp-contract=off), fixed orders, every sum started from its first term:
// tests/dense_pyr_support.py restates them in numpy bit for bit, and levels = 1, iters = 1 is tdense_solve_kernel's field bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flow_obj_kernels.h"

namespace eigt {

constexpr int PYR_MARGIN = 4;  // pixels the staged I1 patch reaches beyond the tile's windows; taps further out are read from global memory

// edges of the staged squares of one tile at radius r, and the doubles of dynamic LDS of tdense_iter_kernel
__host__ __device__ constexpr int pyr_edge_i0(int r) { return FLOW_TILE + 2 * (r + 1); }           // I0: the Scharr taps of the windows
__host__ __device__ constexpr int pyr_edge_g(int r) { return FLOW_TILE + 2 * r; }                  // Ix, Iy: the windows
__host__ __device__ constexpr int pyr_edge_i1(int r) { return FLOW_TILE + 2 * (r + PYR_MARGIN); }  // the I1 patch
__host__ __device__ constexpr int pyr_lds_doubles(int r)
{
    return pyr_edge_i0(r) * pyr_edge_i0(r) + 2 * pyr_edge_g(r) * pyr_edge_g(r) + 3 * pyr_edge_g(r) * FLOW_TILE + pyr_edge_i1(r) * pyr_edge_i1(r);
}
static_assert(pyr_lds_doubles(FLOW_MAX_R) * 8 <= 160 * 1024, "the tile of the largest radius fits the 160 KiB of LDS");

// I0, I1 [n], n = B H W: the gray planes of the two byte batches (image b of either at its pointer + b * its stride, planar [C][H][W])
__global__ void __launch_bounds__(EW_T) tdense_gray_kernel(const uint8_t* __restrict__ img0, long long stride0, const uint8_t* __restrict__ img1, long long stride1, int C,
                                                           int H, int W, long long n, double* __restrict__ I0, double* __restrict__ I1)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const long long HW = (long long)H * W;
    const long long b = i / HW, p = i - b * HW;
    I0[i] = tflow_gray(img0 + b * stride0, C, HW, p);
    I1[i] = tflow_gray(img1 + b * stride1, C, HW, p);
}

__device__ __forceinline__ int pyr_reflect(int i, int n)
{
    i = i < 0 ? -i : i;
    return i >= n ? 2 * (n - 1) - i : i;
}

__device__ __forceinline__ double pyr_taps(double a, double b, double c, double d, double e) { return (((a + e) + 4.0 * (b + d)) + 6.0 * c) / 16.0; }

// one reduced pixel (y, x) of one image [H][W]: the five source rows reduced along x, then those five along y
__device__ __forceinline__ double pyr_reduce(const double* __restrict__ s, int H, int W, int y, int x)
{
    const int c0 = pyr_reflect(2 * x - 2, W), c1 = pyr_reflect(2 * x - 1, W), c2 = 2 * x, c3 = pyr_reflect(2 * x + 1, W), c4 = pyr_reflect(2 * x + 2, W);
    double h[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const double* row = s + (long long)pyr_reflect(2 * y + k - 2, H) * W;
        h[k] = pyr_taps(row[c0], row[c1], row[c2], row[c3], row[c4]);
    }
    return pyr_taps(h[0], h[1], h[2], h[3], h[4]);
}

// level l + 1 [B][Hn][Wn], Hn = (H + 1) / 2, Wn = (W + 1) / 2, of both images of level l [B][H][W]; n = B Hn Wn
__global__ void __launch_bounds__(EW_T) tdense_pyrdown_kernel(const double* __restrict__ s0, const double* __restrict__ s1, int H, int W, int Hn, int Wn, long long n,
                                                              double* __restrict__ d0, double* __restrict__ d1)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const long long HWn = (long long)Hn * Wn;
    const long long b = i / HWn, p = i - b * HWn;
    const int y = (int)(p / Wn), x = (int)(p - (long long)y * Wn);
    const long long src = b * H * W;
    d0[i] = pyr_reduce(s0 + src, H, W, y, x);
    d1[i] = pyr_reduce(s1 + src, H, W, y, x);
}

// The sampler S of I1 [H][W] at (x, y): coordinates clamped to the image (a NaN goes to 0), bilinear with x1 = min(x0 + 1, W - 1).  A tap
// inside the staged patch (origin (px0, py0), edge P) is read from LDS, any other from global memory: the same doubles either way.
__device__ __forceinline__ double pyr_sample(const double* __restrict__ s1, int P, int px0, int py0, const double* __restrict__ I1, int H, int W, double x, double y)
{
    x = x > 0.0 ? x : 0.0;
    x = x < (double)(W - 1) ? x : (double)(W - 1);
    y = y > 0.0 ? y : 0.0;
    y = y < (double)(H - 1) ? y : (double)(H - 1);
    const double xf = floor(x), yf = floor(y);
    const int x0 = (int)xf, y0 = (int)yf;
    const int x1 = x0 + 1 < W - 1 ? x0 + 1 : W - 1, y1 = y0 + 1 < H - 1 ? y0 + 1 : H - 1;
    const double fx = x - xf, fy = y - yf;
    const int lx0 = x0 - px0, lx1 = x1 - px0, ly0 = y0 - py0, ly1 = y1 - py0;
    double v00, v01, v10, v11;
    if (lx0 >= 0 && lx1 < P && ly0 >= 0 && ly1 < P) {
        v00 = s1[ly0 * P + lx0]; v01 = s1[ly0 * P + lx1]; v10 = s1[ly1 * P + lx0]; v11 = s1[ly1 * P + lx1];
    } else {
        v00 = I1[(long long)y0 * W + x0]; v01 = I1[(long long)y0 * W + x1]; v10 = I1[(long long)y1 * W + x0]; v11 = I1[(long long)y1 * W + x1];
    }
    const double top = v00 + fx * (v01 - v00), bot = v10 + fx * (v11 - v10);
    return top + fy * (bot - top);
}

// One level of the solve for one tile (blockIdx: tile x, tile y, sample; FLOW_T threads, pyr_lds_doubles(r) doubles of dynamic LDS).
//   staged: I0 with halo r + 1 (indices clamped to the image, which is the Scharr pair's own border rule), Ix and Iy with halo r formed
//   from it, the row sums of Ix Ix, Ix Iy, Iy Iy in tdense_solve_kernel's order, and the I1 patch with halo r + PYR_MARGIN
//   per pixel: G, a, c, b, det once; u = 2.0 * coarse(y >> 1, x >> 1) (coarse null: the zero field, held as -0.0 so that the first step
//   added to it is the step itself, bit for bit); then `iters` times, u in registers: d(q) = S(I1, qx + ux, qy + uy) - I0(q) over the
//   truncated window, bx = sum Ix d, by = sum Iy d (per row ascending in x from its first term, then the rows ascending in y from the
//   first row), ux += -((c bx - b by) / det), uy += -((a by - b bx) / det)
// I0, I1 [B][H][W]; coarse [B][2][Hc][Wc] or null; flow [B][2][H][W].
// flow_iter_kernels.h holds this kernel's twin, tfiter_fwd_kernel (the same staging and loop, statement for statement, plus the stores of
// every iterate for the trainer's backward pass): a change here is a change there, and tests/test_gpu_flow_iter.py compares the two fields
// bit for bit.
__global__ void __launch_bounds__(FLOW_T) tdense_iter_kernel(const double* __restrict__ I0, const double* __restrict__ I1, int H, int W, int r, double eps, int iters,
                                                             const double* __restrict__ coarse, int Hc, int Wc, double* __restrict__ flow)
{
    extern __shared__ double pyr_lds[];
    const int E0 = pyr_edge_i0(r), E = pyr_edge_g(r), P = pyr_edge_i1(r);
    double* s0 = pyr_lds;
    double* sx = s0 + E0 * E0;
    double* sy = sx + E * E;
    double* rs = sy + E * E;  // [3][E][FLOW_TILE]
    double* s1 = rs + 3 * E * FLOW_TILE;
    const int tx = threadIdx.x & (FLOW_TILE - 1), ty = threadIdx.x / FLOW_TILE;
    const int x0 = blockIdx.x * FLOW_TILE, y0 = blockIdx.y * FLOW_TILE;
    const long long HW = (long long)H * W, base = (long long)blockIdx.z * HW;
    const double *g0 = I0 + base, *g1 = I1 + base;
    const int ox0 = x0 - r - 1, oy0 = y0 - r - 1, px0 = x0 - r - PYR_MARGIN, py0 = y0 - r - PYR_MARGIN;
    for (int item = threadIdx.x; item < E0 * E0; item += FLOW_T) {
        const int ly = item / E0, lx = item - ly * E0;
        int y = oy0 + ly, x = ox0 + lx;
        y = y < 0 ? 0 : (y > H - 1 ? H - 1 : y);
        x = x < 0 ? 0 : (x > W - 1 ? W - 1 : x);
        s0[item] = g0[(long long)y * W + x];
    }
    for (int item = threadIdx.x; item < P * P; item += FLOW_T) {
        const int ly = item / P, lx = item - ly * P;
        const int y = py0 + ly, x = px0 + lx;
        s1[item] = (y >= 0 && y < H && x >= 0 && x < W) ? g1[(long long)y * W + x] : 0.0;
    }
    __syncthreads();
    for (int item = threadIdx.x; item < E * E; item += FLOW_T) {
        const int ly = item / E, lx = item - ly * E;
        const double* c = s0 + (ly + 1) * E0 + (lx + 1);
        const double a_mm = c[-E0 - 1], a_m0 = c[-E0], a_mp = c[-E0 + 1], a_0m = c[-1], a_0p = c[1], a_pm = c[E0 - 1], a_p0 = c[E0], a_pp = c[E0 + 1];
        sx[item] = ((3.0 * (a_mp - a_mm) + 10.0 * (a_0p - a_0m)) + 3.0 * (a_pp - a_pm)) / 32.0;
        sy[item] = ((3.0 * (a_pm - a_mm) + 10.0 * (a_p0 - a_m0)) + 3.0 * (a_pp - a_mp)) / 32.0;
    }
    __syncthreads();
    for (int item = threadIdx.x; item < E * FLOW_TILE; item += FLOW_T) {
        const int ry = item / FLOW_TILE, cx = item & (FLOW_TILE - 1);
        const int y = y0 - r + ry, x = x0 + cx;
        double q0 = 0.0, q1 = 0.0, q2 = 0.0;
        if (y >= 0 && y < H && x < W) {
            const int lo = x - r > 0 ? x - r : 0, hi = x + r < W - 1 ? x + r : W - 1;
            const double *px = sx + ry * E - (x0 - r), *py = sy + ry * E - (x0 - r);
            {
                const double ix = px[lo], iy = py[lo];
                q0 = ix * ix; q1 = ix * iy; q2 = iy * iy;
            }
            for (int xx = lo + 1; xx <= hi; ++xx) {
                const double ix = px[xx], iy = py[xx];
                q0 += ix * ix; q1 += ix * iy; q2 += iy * iy;
            }
        }
        rs[item] = q0; rs[E * FLOW_TILE + item] = q1; rs[2 * E * FLOW_TILE + item] = q2;
    }
    __syncthreads();
    const int x = x0 + tx, y = y0 + ty;
    if (x >= W || y >= H) return;  // no barrier follows
    const int ylo = y - r > 0 ? y - r : 0, yhi = y + r < H - 1 ? y + r : H - 1;
    const int xlo = x - r > 0 ? x - r : 0, xhi = x + r < W - 1 ? x + r : W - 1;
    int k = (ylo - (y0 - r)) * FLOW_TILE + tx;
    double Gxx = rs[k], Gxy = rs[E * FLOW_TILE + k], Gyy = rs[2 * E * FLOW_TILE + k];
    for (int yy = ylo + 1; yy <= yhi; ++yy) {
        k += FLOW_TILE;
        Gxx += rs[k]; Gxy += rs[E * FLOW_TILE + k]; Gyy += rs[2 * E * FLOW_TILE + k];
    }
    const double a = Gxx + eps, c = Gyy + eps, b = Gxy;
    const double det = a * c - b * b;
    double ux = -0.0, uy = -0.0;
    if (coarse) {
        const long long HWc = (long long)Hc * Wc, pc = (long long)(y >> 1) * Wc + (x >> 1);
        ux = 2.0 * coarse[2 * blockIdx.z * HWc + pc];
        uy = 2.0 * coarse[(2 * blockIdx.z + 1) * HWc + pc];
    }
    for (int it = 0; it < iters; ++it) {
        double bx = 0.0, by = 0.0;
        for (int qy = ylo; qy <= yhi; ++qy) {
            const double sy_ = (double)qy + uy;
            const double* r0 = s0 + (qy - oy0) * E0 - ox0;
            const double *rx = sx + (qy - (y0 - r)) * E - (x0 - r), *ry = sy + (qy - (y0 - r)) * E - (x0 - r);
            double d = pyr_sample(s1, P, px0, py0, g1, H, W, (double)xlo + ux, sy_) - r0[xlo];
            double rbx = rx[xlo] * d, rby = ry[xlo] * d;
            for (int qx = xlo + 1; qx <= xhi; ++qx) {
                d = pyr_sample(s1, P, px0, py0, g1, H, W, (double)qx + ux, sy_) - r0[qx];
                rbx += rx[qx] * d; rby += ry[qx] * d;
            }
            if (qy == ylo) { bx = rbx; by = rby; }
            else { bx += rbx; by += rby; }
        }
        ux += -((c * bx - b * by) / det);
        uy += -((a * by - b * bx) / det);
    }
    const long long p = (long long)y * W + x;
    flow[2 * base + p] = ux;
    flow[2 * base + HW + p] = uy;
}

}  // namespace eigt
