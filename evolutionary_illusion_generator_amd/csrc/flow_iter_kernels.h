// flow_iter_kernels.h -- HIP kernels of the flow objective's iterated solve (prednet_train.hip, DESIGN.md section 13, "The iterated
// solve's gradient"): the pyramidal, iterated Lucas-Kanade solve of dense_pyr_kernels.h (eigen_dense_solve) run on the trainer's float
// images with every iterate kept, and the exact gradient of a flow term through it, by the prediction (I1) and by the reference (I0).
// Float64, one IEEE operation per operation written (the build's -ffp-contract=off), fixed partitions, fixed orders, no atomics.
//
// Forward: tfiter_gray_kernel forms the gray planes tflow_prep_kernel / tflow_pair_prep_kernel read, tdense_pyrdown_kernel reduces them,
// and tfiter_fwd_kernel is tdense_iter_kernel operation for operation (the field is that kernel's bit for bit) which also stores u_k, the
// field every iteration k samples at (the tape, [iters][B][2][H W] per level), and the level's Scharr pair [B][2][H W].
//
// Backward, per level from the finest to the coarsest, with ub the gradient arriving at the level's final field (level 0: g = d value /
// d u; below: twice the sum of the in-image children (2Y, 2X) .. (2Y + 1, 2X + 1) of the finer level's ub_0, in row-major order).  The
// derivative is that of the written formulas with floor, x1 = min(x0 + 1, W - 1) and the sampler's two clamps held constant: a clamped
// coordinate passes no gradient, at an integer coordinate the slope is the forward difference.
//   tfiter_adj_kernel    one pixel p per thread, the forward's staging; k = iters - 1 .. 0 with ub and Mb in registers:
//                        beta_k = -(M ub), M = [[c, -b], [-b, a]] / det; over the window in the forward's order (per row ascending in x
//                        from its first term, rows ascending in y from the first row) bx, by as the forward forms them and
//                        gx = sum w dS/dx, gy = sum w dS/dy with w = beta_k,x Ix(q) + beta_k,y Iy(q); Mb -= ub (bx, by)^T; ub += (gx, gy).
//                        Then Ab = -(M (Mb M)), ab = Ab00, cb = Ab11, bb = Ab01 + Ab10.  Stores beta_k, (ab, bb, cb) and ub_0.
//   tfiter_umax_kernel   max |u_k| of the level's tape per sample: the reach of the gather below comes from what the call stored.
//   tfiter_i1_kernel     I1b of one pixel z per thread, a gather: the pixels p within radius + 2 + floor(max |u|) of z in row-major order,
//                        per p the iterations ascending, per iteration the window positions q of p whose bilinear taps can land on z
//                        (two per axis away from the clamps, every clamped q on a border row or column) in row-major order;
//                        the sum starts at +0.0 and adds (w wx) wy, wx and wy the weights the sampler gives tap z along x and y.
//   tfiter_q_kernel      one pixel q per thread: over the p of the truncated window of q in row-major order, per p the iterations
//                        ascending, d_k(p, q) = S(I1, q + u_k(p)) - I0(q) sampled again; Ixb = sum beta_k,x d + (2 (Ix W[ab]) + Iy W[bb]),
//                        Iyb = sum beta_k,y d + (2 (Iy W[cb]) + Ix W[bb]), and I0b's direct term -(Ix sum beta_k,x + Iy sum beta_k,y);
//                        every sum starts at +0.0.
//   tfiter_i0_kernel     I0b = the direct term + S^T(Ixb, Iyb): flow_ref_kernels.h's Scharr adjoint in its order, at the level's size.
//   tfiter_down_kernel   hands ub_0 to the next coarser level (the coarsest level's is dropped).
// After all levels, from the coarsest to the finest, tfiter_pyr_adj_kernel adds the adjoint of the 5-tap reduction of level l + 1 to
// I0b_l and I1b_l: per fine pixel the reduced rows Y then columns X that reach it (through reflect-101 too), ascending, each with the
// product of its two tap weights, the sum started at +0.0 and added to the level's own value once.  tfiter_store_kernel scales level 0 by
// kappa, applies the gray weights, casts to float once and stores or adds.
//
// A sample's planes depend on that sample alone: every grid is (tiles or pixels) x samples, and the reach is per sample.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dense_pyr_kernels.h"
#include "flow_ref_kernels.h"
#include "flow_score_kernels.h"

namespace eigt {

// I0 = gray of the reference (bytes or floats), I1 = gray of the prediction, [n], n = B H W: the values the single step's planes are made of
template <typename REF>
__global__ void __launch_bounds__(EW_T) tfiter_gray_kernel(const float* __restrict__ pred, long long pred_bstride, const REF* __restrict__ ref, long long ref_bstride, int C,
                                                           int H, int W, long long n, double* __restrict__ I0, double* __restrict__ I1)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const long long HW = (long long)H * W;
    const long long b = i / HW, p = i - b * HW;
    I0[i] = tflow_gray(ref + b * ref_bstride, C, HW, p);
    I1[i] = tflow_gray(pred + b * pred_bstride, C, HW, p);
}

// what one tile of tdense_iter_kernel stages, and where
struct TFIterTile {
    double *s0, *sx, *sy, *rs, *s1;
    int E0, E, P, ox0, oy0, px0, py0;
};

// tdense_iter_kernel's staging, statement for statement: I0 with halo r + 1, the Scharr pair with halo r, the row sums of its products
// and the I1 patch with halo r + PYR_MARGIN.  Every thread of the block calls it (three barriers).
__device__ __forceinline__ void tfiter_stage(TFIterTile& t, double* __restrict__ lds, const double* __restrict__ g0, const double* __restrict__ g1, int H, int W, int r, int x0,
                                             int y0)
{
    const int E0 = pyr_edge_i0(r), E = pyr_edge_g(r), P = pyr_edge_i1(r);
    double* s0 = lds;
    double* sx = s0 + E0 * E0;
    double* sy = sx + E * E;
    double* rs = sy + E * E;  // [3][E][FLOW_TILE]
    double* s1 = rs + 3 * E * FLOW_TILE;
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
    t.s0 = s0; t.sx = sx; t.sy = sy; t.rs = rs; t.s1 = s1;
    t.E0 = E0; t.E = E; t.P = P; t.ox0 = ox0; t.oy0 = oy0; t.px0 = px0; t.py0 = py0;
}

// a, b, c and det of the pixel in column tx of its tile whose window covers the rows ylo .. yhi: tdense_iter_kernel's sums
__device__ __forceinline__ void tfiter_system(const TFIterTile& t, int tx, int y0, int r, int ylo, int yhi, double eps, double& a, double& b, double& c, double& det)
{
    const int E = t.E;
    int k = (ylo - (y0 - r)) * FLOW_TILE + tx;
    double Gxx = t.rs[k], Gxy = t.rs[E * FLOW_TILE + k], Gyy = t.rs[2 * E * FLOW_TILE + k];
    for (int yy = ylo + 1; yy <= yhi; ++yy) {
        k += FLOW_TILE;
        Gxx += t.rs[k]; Gxy += t.rs[E * FLOW_TILE + k]; Gyy += t.rs[2 * E * FLOW_TILE + k];
    }
    a = Gxx + eps; c = Gyy + eps; b = Gxy;
    det = a * c - b * b;
}

// tdense_iter_kernel with the tape: the same grid, block and dynamic LDS, the same operations on the field.  tape [iters][B][2][H W]
// receives u_k, the field iteration k samples at; gxy [B][2][H W] the level's Ix, Iy; flow [B][2][H W] the field after the last iteration.
__global__ void __launch_bounds__(FLOW_T) tfiter_fwd_kernel(const double* __restrict__ I0, const double* __restrict__ I1, int H, int W, int r, double eps, int iters,
                                                            const double* __restrict__ coarse, int Hc, int Wc, double* __restrict__ flow, double* __restrict__ tape,
                                                            double* __restrict__ gxy)
{
    extern __shared__ double pyr_lds[];
    const int tx = threadIdx.x & (FLOW_TILE - 1), ty = threadIdx.x / FLOW_TILE;
    const int x0 = blockIdx.x * FLOW_TILE, y0 = blockIdx.y * FLOW_TILE;
    const long long HW = (long long)H * W, base = (long long)blockIdx.z * HW;
    const double *g0 = I0 + base, *g1 = I1 + base;
    TFIterTile t;
    tfiter_stage(t, pyr_lds, g0, g1, H, W, r, x0, y0);
    const double *s0 = t.s0, *sx = t.sx, *sy = t.sy, *s1 = t.s1;
    const int E0 = t.E0, E = t.E, P = t.P, ox0 = t.ox0, oy0 = t.oy0, px0 = t.px0, py0 = t.py0;
    const int x = x0 + tx, y = y0 + ty;
    if (x >= W || y >= H) return;  // no barrier follows
    const int ylo = y - r > 0 ? y - r : 0, yhi = y + r < H - 1 ? y + r : H - 1;
    const int xlo = x - r > 0 ? x - r : 0, xhi = x + r < W - 1 ? x + r : W - 1;
    double a, b, c, det;
    tfiter_system(t, tx, y0, r, ylo, yhi, eps, a, b, c, det);
    const long long p = (long long)y * W + x;
    gxy[2 * base + p] = sx[(ty + r) * E + (tx + r)];
    gxy[2 * base + HW + p] = sy[(ty + r) * E + (tx + r)];
    double ux = -0.0, uy = -0.0;
    if (coarse) {
        const long long HWc = (long long)Hc * Wc, pc = (long long)(y >> 1) * Wc + (x >> 1);
        ux = 2.0 * coarse[2 * blockIdx.z * HWc + pc];
        uy = 2.0 * coarse[(2 * blockIdx.z + 1) * HWc + pc];
    }
    for (int it = 0; it < iters; ++it) {
        double* tp = tape + ((long long)it * gridDim.z + blockIdx.z) * 2 * HW + p;
        tp[0] = ux; tp[HW] = uy;
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
    flow[2 * base + p] = ux;
    flow[2 * base + HW + p] = uy;
}

// The sampler S of pyr_sample with its derivative by the coordinates: S is pyr_sample's value bit for bit; a coordinate one of the two
// clamps replaced passes no gradient (a NaN counts as clamped); floor and x1 = min(x0 + 1, W - 1) are constants
struct TFIterSample {
    double S, Sx, Sy;
};

__device__ __forceinline__ TFIterSample tfiter_sample(const double* __restrict__ s1, int P, int px0, int py0, const double* __restrict__ I1, int H, int W, double x, double y)
{
    const bool free_x = x > 0.0 && x < (double)(W - 1), free_y = y > 0.0 && y < (double)(H - 1);
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
    const double dt = v01 - v00, db = v11 - v10;
    const double top = v00 + fx * dt, bot = v10 + fx * db;
    TFIterSample o;
    o.S = top + fy * (bot - top);
    o.Sx = free_x ? dt + fy * (db - dt) : 0.0;
    o.Sy = free_y ? bot - top : 0.0;
    return o;
}

// The adjoint of one level's iterations at every pixel of one tile (the header): ubK [B][2][H W] arrives, beta [iters][B][2][H W],
// abc [B][3][H W] (ab, bb, cb) and ub0 [B][2][H W] leave.  Grid, block and dynamic LDS are the forward's.
__global__ void __launch_bounds__(FLOW_T) tfiter_adj_kernel(const double* __restrict__ I0, const double* __restrict__ I1, int H, int W, int r, double eps, int iters,
                                                            const double* __restrict__ tape, const double* __restrict__ ubK, double* __restrict__ beta,
                                                            double* __restrict__ abc, double* __restrict__ ub0)
{
    extern __shared__ double pyr_lds[];
    const int tx = threadIdx.x & (FLOW_TILE - 1), ty = threadIdx.x / FLOW_TILE;
    const int x0 = blockIdx.x * FLOW_TILE, y0 = blockIdx.y * FLOW_TILE;
    const long long HW = (long long)H * W, base = (long long)blockIdx.z * HW;
    const double *g0 = I0 + base, *g1 = I1 + base;
    TFIterTile t;
    tfiter_stage(t, pyr_lds, g0, g1, H, W, r, x0, y0);
    const double *s0 = t.s0, *sx = t.sx, *sy = t.sy, *s1 = t.s1;
    const int E0 = t.E0, E = t.E, P = t.P, ox0 = t.ox0, oy0 = t.oy0, px0 = t.px0, py0 = t.py0;
    const int x = x0 + tx, y = y0 + ty;
    if (x >= W || y >= H) return;  // no barrier follows
    const int ylo = y - r > 0 ? y - r : 0, yhi = y + r < H - 1 ? y + r : H - 1;
    const int xlo = x - r > 0 ? x - r : 0, xhi = x + r < W - 1 ? x + r : W - 1;
    double a, b, c, det;
    tfiter_system(t, tx, y0, r, ylo, yhi, eps, a, b, c, det);
    const long long p = (long long)y * W + x;
    double ubx = ubK[2 * base + p], uby = ubK[2 * base + HW + p];
    double m00 = 0.0, m01 = 0.0, m10 = 0.0, m11 = 0.0;
    for (int it = iters - 1; it >= 0; --it) {
        const long long at = ((long long)it * gridDim.z + blockIdx.z) * 2 * HW + p;
        const double ux = tape[at], uy = tape[at + HW];
        const double bex = -((c * ubx - b * uby) / det), bey = -((a * uby - b * ubx) / det);
        beta[at] = bex; beta[at + HW] = bey;
        double bx = 0.0, by = 0.0, gx = 0.0, gy = 0.0;
        for (int qy = ylo; qy <= yhi; ++qy) {
            const double sy_ = (double)qy + uy;
            const double* r0 = s0 + (qy - oy0) * E0 - ox0;
            const double *rx = sx + (qy - (y0 - r)) * E - (x0 - r), *ry = sy + (qy - (y0 - r)) * E - (x0 - r);
            TFIterSample o = tfiter_sample(s1, P, px0, py0, g1, H, W, (double)xlo + ux, sy_);
            double d = o.S - r0[xlo];
            double w = bex * rx[xlo] + bey * ry[xlo];
            double rbx = rx[xlo] * d, rby = ry[xlo] * d, rgx = w * o.Sx, rgy = w * o.Sy;
            for (int qx = xlo + 1; qx <= xhi; ++qx) {
                o = tfiter_sample(s1, P, px0, py0, g1, H, W, (double)qx + ux, sy_);
                d = o.S - r0[qx];
                w = bex * rx[qx] + bey * ry[qx];
                rbx += rx[qx] * d; rby += ry[qx] * d; rgx += w * o.Sx; rgy += w * o.Sy;
            }
            if (qy == ylo) { bx = rbx; by = rby; gx = rgx; gy = rgy; }
            else { bx += rbx; by += rby; gx += rgx; gy += rgy; }
        }
        m00 -= ubx * bx; m01 -= ubx * by; m10 -= uby * bx; m11 -= uby * by;
        ubx += gx; uby += gy;
    }
    const double M00 = c / det, M01 = -(b / det), M11 = a / det;
    const double t00 = m00 * M00 + m01 * M01, t01 = m00 * M01 + m01 * M11, t10 = m10 * M00 + m11 * M01, t11 = m10 * M01 + m11 * M11;
    const double A00 = -(M00 * t00 + M01 * t10), A01 = -(M00 * t01 + M01 * t11), A10 = -(M01 * t00 + M11 * t10), A11 = -(M01 * t01 + M11 * t11);
    abc[3 * base + p] = A00;
    abc[3 * base + HW + p] = A01 + A10;
    abc[3 * base + 2 * HW + p] = A11;
    ub0[2 * base + p] = ubx;
    ub0[2 * base + HW + p] = uby;
}

// umax [B]: the largest |u_k| of sample blockIdx.x over the level's tape [iters][B][2][H W] (a NaN is passed over).  One block per sample:
// a maximum does not depend on the order it is taken in.
__global__ void __launch_bounds__(EW_T) tfiter_umax_kernel(const double* __restrict__ tape, int iters, long long HW, double* __restrict__ umax)
{
    __shared__ double red[EW_T];
    double m = 0.0;
    for (int it = 0; it < iters; ++it) {
        const double* v = tape + ((long long)it * gridDim.x + blockIdx.x) * 2 * HW;
        for (long long i = threadIdx.x; i < 2 * HW; i += EW_T) {
            const double s = fabs(v[i]);
            m = s > m ? s : m;
        }
    }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int w = EW_T / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] = red[threadIdx.x + w] > red[threadIdx.x] ? red[threadIdx.x + w] : red[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x == 0) umax[blockIdx.x] = red[0];
}

// the weight the sampler gives the tap at index z along an axis of n pixels for the coordinate x: (x0 == z) (1 - f) + (x1 == z) f
__device__ __forceinline__ double tfiter_tap_weight(double x, int n, int z)
{
    x = x > 0.0 ? x : 0.0;
    x = x < (double)(n - 1) ? x : (double)(n - 1);
    const double xf = floor(x);
    const int x0 = (int)xf;
    const int x1 = x0 + 1 < n - 1 ? x0 + 1 : n - 1;
    const double f = x - xf;
    return (x0 == z ? 1.0 - f : 0.0) + (x1 == z ? f : 0.0);
}

// a double as an int, out-of-range values (and a NaN) held at +-2^30: only ever compared against window bounds
__device__ __forceinline__ int tfiter_int(double v)
{
    v = v < 1073741824.0 ? v : 1073741824.0;
    v = v > -1073741824.0 ? v : -1073741824.0;
    return (int)v;
}

// the window positions lo .. hi (of lo0 .. hi0) along an axis of n pixels whose coordinate q + u can put a tap on index z: away from the
// clamps q + u in (z - 1, z + 1), taken one wider on both sides (a position that does not reach z has weight 0); z = 0 also collects
// every position clamped from below, z = n - 1 every position clamped from above
__device__ __forceinline__ void tfiter_tap_range(double u, int n, int z, int lo0, int hi0, int& lo, int& hi)
{
    const double t = (double)z - u;
    lo = z == 0 ? lo0 : tfiter_int(floor(t - 1.0));
    hi = z == n - 1 ? hi0 : tfiter_int(floor(t + 2.0));
    lo = lo > lo0 ? lo : lo0;
    hi = hi < hi0 ? hi : hi0;
}

// I1b [n] of one level, n = B H W, the header's gather.  tape, beta [iters][B][2][H W]; gxy [B][2][H W]; umax [B].
__global__ void __launch_bounds__(EW_T) tfiter_i1_kernel(const double* __restrict__ tape, const double* __restrict__ beta, const double* __restrict__ gxy,
                                                         const double* __restrict__ umax, int B, int H, int W, int r, int iters, long long n, double* __restrict__ I1b)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const long long HW = (long long)H * W;
    const long long b = i / HW, z = i - b * HW;
    const int zy = (int)(z / W), zx = (int)(z - (long long)zy * W);
    const int span = H > W ? H : W;
    int reach = r + 2 + tfiter_int(floor(umax[b]));  // floor + 1 is at least the ceiling
    reach = reach < span ? reach : span;
    const int py0 = zy - reach > 0 ? zy - reach : 0, py1 = zy + reach < H - 1 ? zy + reach : H - 1;
    const int px0 = zx - reach > 0 ? zx - reach : 0, px1 = zx + reach < W - 1 ? zx + reach : W - 1;
    const double *Ix = gxy + 2 * b * HW, *Iy = Ix + HW;
    double acc = 0.0;
    for (int py = py0; py <= py1; ++py) {
        const int ylo = py - r > 0 ? py - r : 0, yhi = py + r < H - 1 ? py + r : H - 1;
        for (int px = px0; px <= px1; ++px) {
            const int xlo = px - r > 0 ? px - r : 0, xhi = px + r < W - 1 ? px + r : W - 1;
            const long long p = (long long)py * W + px;
            for (int it = 0; it < iters; ++it) {
                const long long at = ((long long)it * B + b) * 2 * HW + p;
                const double ux = tape[at], uy = tape[at + HW];
                int qx0, qx1, qy0, qy1;
                tfiter_tap_range(ux, W, zx, xlo, xhi, qx0, qx1);
                tfiter_tap_range(uy, H, zy, ylo, yhi, qy0, qy1);
                if (qx0 > qx1 || qy0 > qy1) continue;
                const double bex = beta[at], bey = beta[at + HW];
                for (int qy = qy0; qy <= qy1; ++qy) {
                    const double wy = tfiter_tap_weight((double)qy + uy, H, zy);
                    for (int qx = qx0; qx <= qx1; ++qx) {
                        const double wx = tfiter_tap_weight((double)qx + ux, W, zx);
                        const long long q = (long long)qy * W + qx;
                        const double w = bex * Ix[q] + bey * Iy[q];
                        acc += (w * wx) * wy;
                    }
                }
            }
        }
    }
    I1b[i] = acc;
}

// pyr_sample with every tap read from global memory: the same operations on the same doubles
__device__ __forceinline__ double tfiter_sample_global(const double* __restrict__ I1, int H, int W, double x, double y)
{
    x = x > 0.0 ? x : 0.0;
    x = x < (double)(W - 1) ? x : (double)(W - 1);
    y = y > 0.0 ? y : 0.0;
    y = y < (double)(H - 1) ? y : (double)(H - 1);
    const double xf = floor(x), yf = floor(y);
    const int x0 = (int)xf, y0 = (int)yf;
    const int x1 = x0 + 1 < W - 1 ? x0 + 1 : W - 1, y1 = y0 + 1 < H - 1 ? y0 + 1 : H - 1;
    const double fx = x - xf, fy = y - yf;
    const double v00 = I1[(long long)y0 * W + x0], v01 = I1[(long long)y0 * W + x1], v10 = I1[(long long)y1 * W + x0], v11 = I1[(long long)y1 * W + x1];
    const double top = v00 + fx * (v01 - v00), bot = v10 + fx * (v11 - v10);
    return top + fy * (bot - top);
}

// Ixb, Iyb into rxy [B][2][H W] and I0b's direct term into dir [n] of one level, n = B H W, the header's sums.  I0, I1 [B][H W];
// tape, beta [iters][B][2][H W]; abc [B][3][H W]; gxy [B][2][H W].
__global__ void __launch_bounds__(EW_T) tfiter_q_kernel(const double* __restrict__ I0, const double* __restrict__ I1, const double* __restrict__ tape,
                                                        const double* __restrict__ beta, const double* __restrict__ abc, const double* __restrict__ gxy, int B, int H, int W,
                                                        int r, int iters, long long n, double* __restrict__ rxy, double* __restrict__ dir)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const long long HW = (long long)H * W;
    const long long b = i / HW, q = i - b * HW;
    const int qy = (int)(q / W), qx = (int)(q - (long long)qy * W);
    const int ylo = qy - r > 0 ? qy - r : 0, yhi = qy + r < H - 1 ? qy + r : H - 1;
    const int xlo = qx - r > 0 ? qx - r : 0, xhi = qx + r < W - 1 ? qx + r : W - 1;
    const double* g1 = I1 + b * HW;
    const double i0 = I0[i], ix = gxy[2 * b * HW + q], iy = gxy[2 * b * HW + HW + q];
    const double* A = abc + 3 * b * HW;
    double sbx = 0.0, sby = 0.0, Bx = 0.0, By = 0.0, Wa = 0.0, Wb = 0.0, Wc = 0.0;
    for (int py = ylo; py <= yhi; ++py)
        for (int px = xlo; px <= xhi; ++px) {
            const long long p = (long long)py * W + px;
            Wa += A[p]; Wb += A[HW + p]; Wc += A[2 * HW + p];
            for (int it = 0; it < iters; ++it) {
                const long long at = ((long long)it * B + b) * 2 * HW + p;
                const double d = tfiter_sample_global(g1, H, W, (double)qx + tape[at], (double)qy + tape[at + HW]) - i0;
                const double bex = beta[at], bey = beta[at + HW];
                sbx += bex * d; sby += bey * d; Bx += bex; By += bey;
            }
        }
    rxy[2 * b * HW + q] = sbx + (2.0 * (ix * Wa) + iy * Wb);
    rxy[2 * b * HW + HW + q] = sby + (2.0 * (iy * Wc) + ix * Wb);
    dir[i] = -(Bx * ix + By * iy);
}

// I0b [n] = dir + S^T(Ixb, Iyb) of one level, n = B H W: tflow_ref_fold_kernel's collection of the padded positions, in its order
__global__ void __launch_bounds__(EW_T) tfiter_i0_kernel(const double* __restrict__ rxy, const double* __restrict__ dir, int H, int W, long long n, double* __restrict__ I0b)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const long long HW = (long long)H * W;
    const long long b = i / HW, p = i - b * HW;
    const int y = (int)(p / W), x = (int)(p - (long long)y * W);
    const double *rx = rxy + 2 * b * HW, *ry = rx + HW;
    const int Y0 = y == 0 ? -1 : y, Y1 = y == H - 1 ? H : y, X0 = x == 0 ? -1 : x, X1 = x == W - 1 ? W : x;
    double tot = 0.0;
    for (int Y = Y0; Y <= Y1; ++Y) {
        double row = tflow_ref_gather(rx, ry, H, W, Y, X0);
        for (int X = X0 + 1; X <= X1; ++X) row += tflow_ref_gather(rx, ry, H, W, Y, X);
        tot = Y == Y0 ? row : tot + row;
    }
    I0b[i] = dir[i] + tot;
}

// ubK [B][2][Hc Wc] of the coarser level from ub0 [B][2][H W]: twice the sum of the in-image children, row-major, from the first; n = B Hc Wc
__global__ void __launch_bounds__(EW_T) tfiter_down_kernel(const double* __restrict__ ub0, int H, int W, int Hc, int Wc, long long n, double* __restrict__ ubK)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const long long HWc = (long long)Hc * Wc, HW = (long long)H * W;
    const long long b = i / HWc, pc = i - b * HWc;
    const int Y = (int)(pc / Wc), X = (int)(pc - (long long)Y * Wc);
    const bool right = 2 * X + 1 < W, below = 2 * Y + 1 < H;
    for (int comp = 0; comp < 2; ++comp) {
        const double* v = ub0 + (2 * b + comp) * HW + (long long)(2 * Y) * W + 2 * X;
        double s = v[0];
        if (right) s += v[1];
        if (below) {
            s += v[W];
            if (right) s += v[W + 1];
        }
        ubK[(2 * b + comp) * HWc + pc] = 2.0 * s;
    }
}

// the weight of source index y in the reduced index Y along an axis of n pixels: the taps (1, 4, 6, 4, 1) / 16 about 2 Y that reflect-101
// puts on y, added in tap order
__device__ __forceinline__ double tfiter_pyr_weight(int Y, int y, int n)
{
    double w = 0.0;
    if (pyr_reflect(2 * Y - 2, n) == y) w += 1.0;
    if (pyr_reflect(2 * Y - 1, n) == y) w += 4.0;
    if (2 * Y == y) w += 6.0;
    if (pyr_reflect(2 * Y + 1, n) == y) w += 4.0;
    if (pyr_reflect(2 * Y + 2, n) == y) w += 1.0;
    return w / 16.0;
}

// f0, f1 [B][H W] += the adjoint of tdense_pyrdown_kernel applied to c0, c1 [B][Hn Wn] (the header's order); n = B H W
__global__ void __launch_bounds__(EW_T) tfiter_pyr_adj_kernel(const double* __restrict__ c0, const double* __restrict__ c1, int H, int W, int Hn, int Wn, long long n,
                                                              double* __restrict__ f0, double* __restrict__ f1)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const long long HW = (long long)H * W, HWn = (long long)Hn * Wn;
    const long long b = i / HW, p = i - b * HW;
    const int y = (int)(p / W), x = (int)(p - (long long)y * W);
    const int Ylo = (y >> 1) - 2 > 0 ? (y >> 1) - 2 : 0, Yhi = (y >> 1) + 2 < Hn - 1 ? (y >> 1) + 2 : Hn - 1;
    const int Xlo = (x >> 1) - 2 > 0 ? (x >> 1) - 2 : 0, Xhi = (x >> 1) + 2 < Wn - 1 ? (x >> 1) + 2 : Wn - 1;
    double s0 = 0.0, s1 = 0.0;
    for (int Y = Ylo; Y <= Yhi; ++Y) {
        const double wy = tfiter_pyr_weight(Y, y, H);
        if (wy == 0.0) continue;
        for (int X = Xlo; X <= Xhi; ++X) {
            const double wx = tfiter_pyr_weight(X, x, W);
            if (wx == 0.0) continue;
            const double w = wy * wx;
            s0 += w * c0[b * HWn + (long long)Y * Wn + X];
            s1 += w * c1[b * HWn + (long long)Y * Wn + X];
        }
    }
    f0[i] = f0[i] + s0;
    f1[i] = f1[i] + s1;
}

// (float)(k_c (g kappa)) of every channel from the gray adjoint g [n] of level 0, k = (0.299, 0.587, 0.114) or (1), n = B H W.  Sample b at
// out + b * out_bstride as [C][H][W]; accumulate = 1: out += that (a float addition), 0: a plain store.
__global__ void __launch_bounds__(EW_T) tfiter_store_kernel(const double* __restrict__ g, double kappa, int C, long long HW, long long n, float* __restrict__ out,
                                                            long long out_bstride, int accumulate)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const long long b = i / HW, p = i - b * HW;
    const double s = g[i] * kappa;
    float* o = out + b * out_bstride + p;
    if (C == 1) {
        const float v = (float)s;
        o[0] = accumulate ? o[0] + v : v;
    } else {
        const float v0 = (float)(0.299 * s), v1 = (float)(0.587 * s), v2 = (float)(0.114 * s);
        o[0] = accumulate ? o[0] + v0 : v0;
        o[HW] = accumulate ? o[HW] + v1 : v1;
        o[2 * HW] = accumulate ? o[2 * HW] + v2 : v2;
    }
}

// The displacement modes on the solved field u [B][2][H W]: tflow_solve_kernel's value and g.  v = ux ux + uy uy, g = (2 ux, 2 uy), or with a
// direction field v = dx ux + dy uy, g = d; mv [n] = v and g [B][2][H W] where the mask counts the pixel, else 0.  n = B H W.
__global__ void __launch_bounds__(EW_T) tfiter_value_kernel(const double* __restrict__ u, const float* __restrict__ dirf, const uint8_t* __restrict__ mask,
                                                            long long mask_bstride, long long HW, long long n, double* __restrict__ mv, double* __restrict__ g)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const long long b = i / HW, p = i - b * HW;
    const double ux = u[2 * b * HW + p], uy = u[2 * b * HW + HW + p];
    double v, gx, gy;
    if (dirf) {
        gx = (double)dirf[p]; gy = (double)dirf[HW + p];
        v = gx * ux + gy * uy;
    } else {
        gx = 2.0 * ux; gy = 2.0 * uy;
        v = ux * ux + uy * uy;
    }
    const bool counted = !mask || mask[b * mask_bstride + p] != 0;
    mv[i] = counted ? v : 0.0;
    g[2 * b * HW + p] = counted ? gx : 0.0;
    g[2 * b * HW + HW + p] = counted ? gy : 0.0;
}

// The score mode's g [B][2][H W] = d S_b / d u from u and the samples' records: what tflow_score_q_kernel folds into q, left as it is
__global__ void __launch_bounds__(EW_T) tfiter_score_g_kernel(const double* __restrict__ u, int H, int W, long long n, const uint8_t* __restrict__ mask, long long mask_bstride,
                                                              TFlowScore s, const double* __restrict__ rec, double* __restrict__ g)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const long long HW = (long long)H * W;
    const long long b = i / HW, p = i - b * HW;
    const int y = (int)(p / W), x = (int)(p - (long long)y * W);
    const double ux = u[2 * b * HW + p], uy = u[2 * b * HW + HW + p];
    const double* R = rec + b * SCORE_REC;
    const TScorePoint o = tflow_score_point(ux, uy, x, y, H, W, !mask || mask[b * mask_bstride + p] != 0, s);
    double gx = 0.0, gy = 0.0;
    if (o.member && !(R[0] < (double)s.min_count)) tflow_score_g(ux, o, R, s, gx, gy);
    g[2 * b * HW + p] = gx;
    g[2 * b * HW + HW + p] = gy;
}

}  // namespace eigt
