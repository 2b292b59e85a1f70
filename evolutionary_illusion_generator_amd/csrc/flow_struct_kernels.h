// flow_struct_kernels.h -- HIP kernels of the flow objective's structure scores (prednet_train.hip, DESIGN.md section 13, "The structure
// scores"): the value of a term is the population fitness's own score of the Bands structure (horizontal_symmetry_score, quirk Q10 kept)
// or of the Free structure (swarm_score, quirk Q11 kept, with strength_number and the count term), evaluated on the dense field u the
// tiled solve of flow_obj_kernels.h left, and q is formed from the exact gradient of that value by u.  Everything downstream of q (the
// seed, the reference gradient, the prediction pairing) is the kernels of flow_obj_kernels.h and flow_ref_kernels.h unchanged.  Float64,
// one IEEE operation per operation written (the build's -ffp-contract=off); tests/flow_struct_support.py restates it in numpy.  Fixed
// partitions, fixed orders, no float atomics.
//
// Common to both: nrm = sqrt(ux ux + uy uy); member: the mask counts the pixel, the structure's geometric rule holds, nrm > 0 and
// min_norm <= nrm <= max_norm (a constant of the graph); nx = ux / nrm, ny = uy / nrm.  N < min_count: S_b = 0 and g = 0; N = 0: no
// quotient is formed, every moment is 0.  f = (sum_b S_b) / B, b ascending.
//
// Bands.  Rule: lim_lo <= y <= lim_hi; middle = (int)(lim_hi / 2).  y < middle: mx = nx, my = nx (the quirk); else mx = -nx, my = ny.
//   Pass 1: N, m_x = sum mx / N, m_y = sum my / N.  Pass 2: V = sum (mx - m_x)^2 / N.  S_b = ((1 - V) + |m_x| + (1 - |m_y|)) / 3.
//   c_x = (-(2 (mx - m_x)) + sign(m_x)) / (3 N), c_y = -sign(m_y) / (3 N), sign(0) = 0
//   y < middle: a_x = c_x + c_y, a_y = 0; else a_x = -c_x, a_y = c_y
//   gx = (a_x (ny ny) - a_y (nx ny)) / nrm, gy = (a_y (nx nx) - a_x (nx ny)) / nrm
//
// Free.  No rule beyond the mask.  theta = acos(nx).  For members i, j (i = j included), DD = D D:
//   d2 = (x_j - x_i)^2 + (y_j - y_i)^2, f = min(d2 / DD, 1), close iff f < 1, opt_ij = fmod(theta_i + f pi, 2) pi,
//   L_i = sum_j close_ij |theta_j - opt_ij|, j ascending in pixel order, from 0.  fmod(x, 2) is formed as x - 2 floor(x / 2), which is
//   exact for finite x >= 0, as fmod is.  rowS_i = sum_j close_ij sign(theta_j - opt_ij), colS_j = sum_i close_ij sign(theta_j - opt_ij):
//   integers, exact in any order.
//   Pass 1: N, m_a = sum |ux| / N, m_n = sum nrm / N.  Pass 2: V_n = sum (nrm - m_n)^2 / N, swarm = (sum_i (pi - L_i / N) / pi) / N.
//   A = m_a / max_norm, F = 1 - min(V_n, 1), S_b = (w0 swarm + w1 (A F)) + w2 (min(N, 15) / 15).
//   c_th = -((w0 (colS - pi rowS)) / (pi (N N))); gx = (c_th (-|ny|)) / nrm, gy = (c_th (sign(ny) nx)) / nrm
//   gx = gx + ((w1 F) sign(ux)) / (N max_norm); c_n = -(((w1 A) (2 (nrm - m_n))) / N) where V_n < 1, else 0; gx += c_n nx, gy += c_n ny
//
// q = ((c gx - b gy) / det, (a gy - b gx) / det) with the solve's a, b, c, det; g is 0 off the members, and so is q.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flow_obj_kernels.h"

namespace eigt {

constexpr int STRUCT_BANDS = 0, STRUCT_FREE = 2;  // the engine's numbering of the structures (eigen_score)
constexpr int STRUCT_SLICES = 16;  // blocks per sample of the moment reductions
constexpr int STRUCT_REC = 10;     // doubles of one sample's record.  Bands: N, m_x, m_y, V, 0 x 4, S_b, 0.  Free: N, m_a, m_n, V_n, swarm, A F, 0 x 2, S_b, 0
constexpr int STRUCT_K = 3;        // partial sums per slice: pass 1 fills three, pass 2 one (Bands) or two (Free)
constexpr int PAIR_T = 256;        // threads of a pair block, and the pixels of one LDS tile
constexpr double STRUCT_PI = 3.141592653589793;

// what the passes and the gradient need of one pixel
struct TStructPoint {
    double nrm, nx, ny;
    bool member;
};

template <int STRUCT>
__device__ __forceinline__ TStructPoint tflow_struct_point(double ux, double uy, int y, bool counted, const TFlowStruct& s)
{
    TStructPoint o;
    o.nrm = sqrt(ux * ux + uy * uy);
    const bool rule = STRUCT == STRUCT_BANDS ? (s.lim_lo <= (double)y && (double)y <= s.lim_hi) : true;
    o.member = counted && rule && o.nrm > 0.0 && s.min_norm <= o.nrm && o.nrm <= s.max_norm;
    o.nx = o.ny = 0.0;
    if (o.member) {
        o.nx = ux / o.nrm;
        o.ny = uy / o.nrm;
    }
    return o;
}

__device__ __forceinline__ double tflow_sign(double v) { return v > 0.0 ? 1.0 : v < 0.0 ? -1.0 : 0.0; }

// theta and the member flag of every pixel of the Free structure; n = B H W, u [B][2][H][W]
__global__ void __launch_bounds__(EW_T) tflow_free_prepare_kernel(const double* __restrict__ u, long long n, int H, int W, const uint8_t* __restrict__ mask, long long mask_bstride, TFlowStruct s,
                                                                  double* __restrict__ theta, uint8_t* __restrict__ flag)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const long long HW = (long long)H * W, b = i / HW, p = i - b * HW;
    const TStructPoint o = tflow_struct_point<STRUCT_FREE>(u[2 * b * HW + p], u[2 * b * HW + HW + p], 0, !mask || mask[b * mask_bstride + p] != 0, s);
    theta[i] = o.member ? acos(o.nx) : 0.0;
    flag[i] = o.member ? 1 : 0;
}

// part[b][slice][k]: the sums of one fixed strided slice of sample b's pixels (blockIdx: slice, sample), every thread its pixels in
// ascending order, then a fixed LDS tree (the pattern of tflow_score_moment_kernel).  Bands pass 1: N, mx, my; pass 2: (mx - m_x)^2.
// Free pass 1: N, |ux|, nrm; pass 2: (nrm - m_n)^2, (pi - L / N) / pi with L [B][H W] of the pair kernel.
template <int STRUCT, int PASS>
__global__ void __launch_bounds__(EW_T) tflow_struct_moment_kernel(const double* __restrict__ u, int H, int W, const uint8_t* __restrict__ mask, long long mask_bstride, TFlowStruct s,
                                                                   const double* __restrict__ rec, const double* __restrict__ L, double* __restrict__ part)
{
    constexpr int K = PASS == 1 ? 3 : STRUCT == STRUCT_BANDS ? 1 : 2;
    __shared__ double red[K][EW_T];
    const long long HW = (long long)H * W;
    const int b = blockIdx.y;
    const double *ux = u + 2 * b * HW, *uy = ux + HW;
    double N = 0.0, mean = 0.0;
    if (PASS == 2) { N = rec[b * STRUCT_REC]; mean = rec[b * STRUCT_REC + (STRUCT == STRUCT_BANDS ? 1 : 2)]; }
    double acc[K];
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    for (long long p = (long long)blockIdx.x * EW_T + threadIdx.x; p < HW; p += (long long)STRUCT_SLICES * EW_T) {
        const int y = (int)(p / W);
        const double vx = ux[p], vy = uy[p];
        const TStructPoint o = tflow_struct_point<STRUCT>(vx, vy, y, !mask || mask[b * mask_bstride + p] != 0, s);
        if (!o.member) continue;
        if constexpr (STRUCT == STRUCT_BANDS) {
            const bool upper = y < s.middle;
            const double mx = upper ? o.nx : -o.nx, my = upper ? o.nx : o.ny;
            if constexpr (PASS == 1) {
                acc[0] += 1.0; acc[1] += mx; acc[2] += my;
            } else {
                const double d = mx - mean;
                acc[0] += d * d;
            }
        } else if constexpr (PASS == 1) {
            acc[0] += 1.0; acc[1] += fabs(vx); acc[2] += o.nrm;
        } else {
            const double d = o.nrm - mean;
            acc[0] += d * d;
            acc[1] += (STRUCT_PI - L[b * HW + p] / N) / STRUCT_PI;
        }
    }
    for (int k = 0; k < K; ++k) red[k][threadIdx.x] = acc[k];
    __syncthreads();
    for (int w = EW_T / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w)
            for (int k = 0; k < K; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x < K) part[((long long)b * STRUCT_SLICES + blockIdx.x) * STRUCT_K + threadIdx.x] = red[threadIdx.x][0];
}

// sum over the slices, ascending, of partial k of sample b
__device__ __forceinline__ double tflow_struct_slices(const double* __restrict__ part, int b, int k)
{
    double t = part[(long long)b * STRUCT_SLICES * STRUCT_K + k];
    for (int i = 1; i < STRUCT_SLICES; ++i) t += part[((long long)b * STRUCT_SLICES + i) * STRUCT_K + k];
    return t;
}

// S_b of a record whose moments are complete; Free also leaves A F in r5
template <int STRUCT>
__device__ __forceinline__ double tflow_struct_value(double N, double r1, double r2, double r3, double r4, double* r5, const TFlowStruct& s)
{
    if (N < (double)s.min_count) return 0.0;
    if (STRUCT == STRUCT_BANDS) return ((1.0 - r3) + fabs(r1) + (1.0 - fabs(r2))) / 3.0;
    const double A = r1 / s.max_norm;
    const double F = 1.0 - (r3 < 1.0 ? r3 : 1.0);
    const double AF = A * F;
    if (r5) *r5 = AF;
    const double num = (N < 15.0 ? N : 15.0) / 15.0;
    return (s.w0 * r4 + s.w1 * AF) + s.w2 * num;
}

// One block per sample, its first thread: the partials added in slice order into the sample's record.  PASS 1: N and the two means (and
// zeros in the rest of the record); PASS 2: the variance, for Free the swarm term, and S_b; block 0 then forms f = (sum_b S_b) / B over
// all B samples, b ascending, each S_b from the same partials by the same operations (value may be null).
template <int STRUCT, int PASS>
__global__ void __launch_bounds__(64) tflow_struct_final_kernel(const double* __restrict__ part, int B, TFlowStruct s, double* __restrict__ rec, double* __restrict__ value)
{
    if (threadIdx.x != 0) return;
    const int b = blockIdx.x;
    double* r = rec + b * STRUCT_REC;
    if (PASS == 1) {
        const double N = tflow_struct_slices(part, b, 0);
        r[0] = N;
        for (int k = 1; k < 3; ++k) r[k] = N > 0.0 ? tflow_struct_slices(part, b, k) / N : 0.0;
        for (int k = 3; k < STRUCT_REC; ++k) r[k] = 0.0;
    } else {
        double total = 0.0;
        for (int bb = b; bb < (b == 0 && value ? B : b + 1); ++bb) {
            const double N = rec[bb * STRUCT_REC], r1 = rec[bb * STRUCT_REC + 1], r2 = rec[bb * STRUCT_REC + 2];
            const double V = N > 0.0 ? tflow_struct_slices(part, bb, 0) / N : 0.0;
            const double sw = STRUCT == STRUCT_FREE && N > 0.0 ? tflow_struct_slices(part, bb, 1) / N : 0.0;
            double AF = 0.0;
            const double S = tflow_struct_value<STRUCT>(N, r1, r2, V, sw, &AF, s);
            if (bb == b) { r[3] = V; r[4] = sw; r[5] = AF; r[8] = S; }
            total = bb == 0 ? S : total + S;
        }
        if (b == 0 && value) *value = total / (double)B;
    }
}

// The pair pass of the Free structure (blockIdx: block of PAIR_T pixels, sample).  One thread owns pixel k and walks all pixels m of its
// sample in ascending order, in tiles of PAIR_T staged in LDS (theta and the flag; the position follows from the index): every lane
// reads the same LDS word, a broadcast.  In that one walk: L_k (k as the row i), rowS_k, and colS_k (k as the column j); f is the same
// either way.  A pixel that is no member, of the tile or of the thread, is skipped; the order among the members does not depend on it.
__global__ void __launch_bounds__(PAIR_T) tflow_free_pair_kernel(const double* __restrict__ theta, const uint8_t* __restrict__ flag, int H, int W, double DD,
                                                                 double* __restrict__ L, int* __restrict__ rowS, int* __restrict__ colS)
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
    int rs = 0, cs = 0;
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
                        const double th_m = sth[j], fp = f * STRUCT_PI;
                        double o = th_k + fp;                                   // row k, column m
                        o = (o - 2.0 * floor(o * 0.5)) * STRUCT_PI;
                        const double d1 = th_m - o;
                        Lk += fabs(d1);
                        rs += d1 > 0.0 ? 1 : d1 < 0.0 ? -1 : 0;
                        o = th_m + fp;                                          // row m, column k
                        o = (o - 2.0 * floor(o * 0.5)) * STRUCT_PI;
                        const double d2 = th_k - o;
                        cs += d2 > 0.0 ? 1 : d2 < 0.0 ? -1 : 0;
                    }
                }
                if (++xm == W) { xm = 0; ++ym; }
            }
        }
        __syncthreads();
    }
    if (k < HW) { L[base + k] = Lk; rowS[base + k] = rs; colS[base + k] = cs; }
}

// g = d S_b / d u of every pixel, [B][2][H][W]; n = B H W; 0 off the members and in a sample below min_count.  rowS, colS: Free only.
template <int STRUCT>
__global__ void __launch_bounds__(EW_T) tflow_struct_grad_kernel(const double* __restrict__ u, long long n, int H, int W, const uint8_t* __restrict__ mask, long long mask_bstride, TFlowStruct s,
                                                                 const double* __restrict__ rec, const int* __restrict__ rowS, const int* __restrict__ colS,
                                                                 double* __restrict__ g)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const long long HW = (long long)H * W, b = i / HW, p = i - b * HW;
    const int y = (int)(p / W);
    const double ux = u[2 * b * HW + p], uy = u[2 * b * HW + HW + p];
    const TStructPoint o = tflow_struct_point<STRUCT>(ux, uy, y, !mask || mask[b * mask_bstride + p] != 0, s);
    const double* R = rec + b * STRUCT_REC;
    const double N = R[0];
    double gx = 0.0, gy = 0.0;
    if (o.member && !(N < (double)s.min_count)) {
        if (STRUCT == STRUCT_BANDS) {
            const double m_x = R[1], m_y = R[2];
            const bool upper = y < s.middle;
            const double mx = upper ? o.nx : -o.nx;
            const double c_x = (-(2.0 * (mx - m_x)) + tflow_sign(m_x)) / (3.0 * N);
            const double c_y = -tflow_sign(m_y) / (3.0 * N);
            const double a_x = upper ? c_x + c_y : -c_x, a_y = upper ? 0.0 : c_y;
            const double xy = o.nx * o.ny;
            gx = (a_x * (o.ny * o.ny) - a_y * xy) / o.nrm;
            gy = (a_y * (o.nx * o.nx) - a_x * xy) / o.nrm;
        } else {
            const double m_a = R[1], m_n = R[2], Vn = R[3];
            const double c_th = -((s.w0 * ((double)colS[i] - STRUCT_PI * (double)rowS[i])) / (STRUCT_PI * (N * N)));
            gx = (c_th * -fabs(o.ny)) / o.nrm;
            gy = (c_th * (tflow_sign(o.ny) * o.nx)) / o.nrm;
            const double A = m_a / s.max_norm;
            const double F = 1.0 - (Vn < 1.0 ? Vn : 1.0);
            gx = gx + ((s.w1 * F) * tflow_sign(ux)) / (N * s.max_norm);
            const double c_n = Vn < 1.0 ? -(((s.w1 * A) * (2.0 * (o.nrm - m_n))) / N) : 0.0;
            gx = gx + c_n * o.nx;
            gy = gy + c_n * o.ny;
        }
    }
    g[2 * b * HW + p] = gx;
    g[2 * b * HW + HW + p] = gy;
}

// q of every pixel of one tile (blockIdx: tile x, tile y, sample) from g [B][2][H][W].  Gxx, Gxy, Gyy are formed again in
// tflow_solve_kernel's order (rows first, offsets ascending, each sum started from its first term), as tflow_score_q_kernel does, so
// a, b, c and det are the solve's bits.  q [2][n] replaces what the solve wrote there.
__global__ void __launch_bounds__(FLOW_T) tflow_struct_q_kernel(const double* __restrict__ planes, const double* __restrict__ g, long long n, int H, int W, int r, double eps,
                                                                double* __restrict__ q)
{
    __shared__ double rs[3][FLOW_ROWS][FLOW_TILE];
    const int tx = threadIdx.x & (FLOW_TILE - 1), ty = threadIdx.x / FLOW_TILE;
    const int x0 = blockIdx.x * FLOW_TILE, y0 = blockIdx.y * FLOW_TILE;
    const long long HW = (long long)H * W, base = (long long)blockIdx.z * HW;
    const double *Ix = planes + base, *Iy = planes + n + base;
    const int rows = FLOW_TILE + 2 * r;
    for (int item = threadIdx.x; item < rows * FLOW_TILE; item += FLOW_T) {
        const int ry = item / FLOW_TILE, cx = item & (FLOW_TILE - 1);
        const int y = y0 - r + ry, x = x0 + cx;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        if (y >= 0 && y < H && x < W) {
            const int lo = x - r > 0 ? x - r : 0, hi = x + r < W - 1 ? x + r : W - 1;
            const long long row = (long long)y * W;
            {
                const double ix = Ix[row + lo], iy = Iy[row + lo];
                s0 = ix * ix; s1 = ix * iy; s2 = iy * iy;
            }
            for (int xx = lo + 1; xx <= hi; ++xx) {
                const double ix = Ix[row + xx], iy = Iy[row + xx];
                s0 += ix * ix; s1 += ix * iy; s2 += iy * iy;
            }
        }
        rs[0][ry][cx] = s0; rs[1][ry][cx] = s1; rs[2][ry][cx] = s2;
    }
    __syncthreads();
    const int x = x0 + tx, y = y0 + ty;
    if (x >= W || y >= H) return;
    const int lo = y - r > 0 ? y - r : 0, hi = y + r < H - 1 ? y + r : H - 1;
    int k = lo - (y0 - r);
    double Gxx = rs[0][k][tx], Gxy = rs[1][k][tx], Gyy = rs[2][k][tx];
    for (int yy = lo + 1; yy <= hi; ++yy) {
        ++k;
        Gxx += rs[0][k][tx]; Gxy += rs[1][k][tx]; Gyy += rs[2][k][tx];
    }
    const double a = Gxx + eps, c = Gyy + eps, b = Gxy;
    const double det = a * c - b * b;
    const long long p = (long long)y * W + x;
    const double gx = g[2 * base + p], gy = g[2 * base + HW + p];
    q[base + p] = (c * gx - b * gy) / det;
    q[n + base + p] = (a * gy - b * gx) / det;
}

}  // namespace eigt
