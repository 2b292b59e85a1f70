// flow_score_kernels.h -- HIP kernels of the flow objective's score mode (prednet_train.hip, DESIGN.md section 13, "The score mode"): the
// value of a term is the Circles score of the population fitness, 0.7 rotation_symmetry_score + 0.3 strength_number with the reference's
// own constants as defaults, evaluated on the dense field u the tiled solve of flow_obj_kernels.h left, and q is formed from the exact
// gradient of that value by u.  Everything downstream of q (the seed, the reference gradient, the prediction pairing) is the kernels of
// flow_obj_kernels.h and flow_ref_kernels.h unchanged: they read only the planes, q and u.  Float64, one IEEE operation per operation
// written (the build's -ffp-contract=off); tests/flow_score_support.py restates it in numpy, and what follows the per-sample record is
// compared bit for bit.  Fixed partitions, fixed orders, no float atomics.
//
// Per sample b and pixel (x, y), u = (ux, uy):
//   px = x - W / 2.0, py = y - H / 2.0, dist = sqrt(px px + py py), nrm = sqrt(ux ux + uy uy)
//   member: the mask counts the pixel, dist != 0, r_min <= dist <= r_max, nrm > 0, min_norm <= nrm <= max_norm (a constant of the graph)
//   nx = ux / nrm, ny = uy / nrm, x1 = px + nx, y1 = py + ny, rho = (x1 px + y1 py) / dist - dist, tau = (-x1 py + y1 px) / dist
// Pass 1 over the members: N, m_rho = sum rho / N, m_tau, m_a = sum |ux| / N, m_n = sum nrm / N.  Pass 2: V_rho = sum (rho - m_rho)^2 / N,
// V_tau, V_n = sum (nrm - m_n)^2 / N.  N = 0: every moment is 0.
//   R = ((1 - V_rho) (1 - V_rho) + (1 - V_tau) (1 - V_tau)) / 2, A = m_a / max_norm, F = 1 - min(V_n, 1)
//   S_b = w_direction R + w_strength (A F); N < min_count: S_b = 0 and g = 0.  f = (sum_b S_b) / B, b ascending.
//
// g = d S_b / d u at a member, 0 elsewhere.  The order of the operations, fixed here and restated in numpy:
//   c_rho = -(((w_direction (1 - V_rho)) (2 (rho - m_rho))) / N), c_tau alike
//   gamma_x = (c_rho px) / dist - (c_tau py) / dist, gamma_y = (c_rho py) / dist + (c_tau px) / dist
//   d = gamma_x nx + gamma_y ny, gx = (gamma_x - d nx) / nrm, gy = (gamma_y - d ny) / nrm
//   gx = gx + ((w_strength F) sign(ux)) / (N max_norm), sign(0) = 0
//   c_n = -(((w_strength A) (2 (nrm - m_n))) / N) where V_n < 1, else 0; gx = gx + c_n nx, gy = gy + c_n ny
//   q = ((c gx - b gy) / det, (a gy - b gx) / det) with the solve's a, b, c, det; 0 where the pixel is no member
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flow_obj_kernels.h"

namespace eigt {

constexpr int SCORE_SLICES = 16;  // blocks per sample of the moment reductions
constexpr int SCORE_REC = 10;     // doubles of one sample's record: N, m_rho, m_tau, m_a, m_n, V_rho, V_tau, V_n, S_b, spare
constexpr int SCORE_K = 5;        // partial sums per slice: pass 1 fills five, pass 2 the first three

// what the passes and the gradient need of one pixel
struct TScorePoint {
    double px, py, dist, nrm, nx, ny, rho, tau;
    bool member;
};

__device__ __forceinline__ TScorePoint tflow_score_point(double ux, double uy, int x, int y, int H, int W, bool counted, const TFlowScore& s)
{
    TScorePoint o;
    o.px = (double)x - (double)W / 2.0;
    o.py = (double)y - (double)H / 2.0;
    o.dist = sqrt(o.px * o.px + o.py * o.py);
    o.nrm = sqrt(ux * ux + uy * uy);
    o.member = counted && o.dist != 0.0 && s.r_min <= o.dist && o.dist <= s.r_max && o.nrm > 0.0 && s.min_norm <= o.nrm && o.nrm <= s.max_norm;
    o.nx = o.ny = o.rho = o.tau = 0.0;
    if (o.member) {
        o.nx = ux / o.nrm;
        o.ny = uy / o.nrm;
        const double x1 = o.px + o.nx, y1 = o.py + o.ny;
        o.rho = (x1 * o.px + y1 * o.py) / o.dist - o.dist;
        o.tau = (-x1 * o.py + y1 * o.px) / o.dist;
    }
    return o;
}

// part[b][slice][k]: the sums of one fixed strided slice of sample b's pixels (blockIdx: slice, sample), every thread its pixels in
// ascending order, then a fixed LDS tree (the pattern of tloss_step_partial_kernel).  PASS 1: N, rho, tau, |ux|, nrm; PASS 2, with the
// means of rec: (rho - m_rho)^2, (tau - m_tau)^2, (nrm - m_n)^2.  u [B][2][H][W]; consecutive lanes read consecutive doubles.
template <int PASS>
__global__ void __launch_bounds__(EW_T) tflow_score_moment_kernel(const double* __restrict__ u, int H, int W, const uint8_t* __restrict__ mask, long long mask_bstride, TFlowScore s,
                                                                  const double* __restrict__ rec, double* __restrict__ part)
{
    constexpr int K = PASS == 1 ? 5 : 3;
    __shared__ double red[K][EW_T];
    const long long HW = (long long)H * W;
    const int b = blockIdx.y;
    const double *ux = u + 2 * b * HW, *uy = ux + HW;
    double m_rho = 0.0, m_tau = 0.0, m_n = 0.0;
    if (PASS == 2) { m_rho = rec[b * SCORE_REC + 1]; m_tau = rec[b * SCORE_REC + 2]; m_n = rec[b * SCORE_REC + 4]; }
    double acc[K];
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    for (long long p = (long long)blockIdx.x * EW_T + threadIdx.x; p < HW; p += (long long)SCORE_SLICES * EW_T) {
        const int y = (int)(p / W), x = (int)(p - (long long)y * W);
        const double vx = ux[p], vy = uy[p];
        const TScorePoint o = tflow_score_point(vx, vy, x, y, H, W, !mask || mask[b * mask_bstride + p] != 0, s);
        if (!o.member) continue;
        if (PASS == 1) {
            acc[0] += 1.0; acc[1] += o.rho; acc[2] += o.tau; acc[3] += fabs(vx); acc[4] += o.nrm;
        } else {
            const double dr = o.rho - m_rho, dt = o.tau - m_tau, dn = o.nrm - m_n;
            acc[0] += dr * dr; acc[1] += dt * dt; acc[2] += dn * dn;
        }
    }
    for (int k = 0; k < K; ++k) red[k][threadIdx.x] = acc[k];
    __syncthreads();
    for (int w = EW_T / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w)
            for (int k = 0; k < K; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x < K) part[((long long)b * SCORE_SLICES + blockIdx.x) * SCORE_K + threadIdx.x] = red[threadIdx.x][0];
}

// sum over the slices, ascending, of partial k of sample b
__device__ __forceinline__ double tflow_score_slices(const double* __restrict__ part, int b, int k)
{
    double t = part[(long long)b * SCORE_SLICES * SCORE_K + k];
    for (int i = 1; i < SCORE_SLICES; ++i) t += part[((long long)b * SCORE_SLICES + i) * SCORE_K + k];
    return t;
}

// S_b from the record's first-pass entries and the three variances
__device__ __forceinline__ double tflow_score_value(double N, double m_a, double Vr, double Vt, double Vn, const TFlowScore& s)
{
    if (N < (double)s.min_count) return 0.0;
    const double R = ((1.0 - Vr) * (1.0 - Vr) + (1.0 - Vt) * (1.0 - Vt)) / 2.0;
    const double A = m_a / s.max_norm;
    const double F = 1.0 - (Vn < 1.0 ? Vn : 1.0);
    return s.w_direction * R + s.w_strength * (A * F);
}

// One block per sample, its first thread: the partials added in slice order into the sample's record.  PASS 1: N and the four means
// (and zeros in the rest of the record); PASS 2: the three variances and S_b, and block 0 then forms f = (sum_b S_b) / B over all B
// samples, b ascending, each S_b from the same partials by the same operations (value may be null).
template <int PASS>
__global__ void __launch_bounds__(64) tflow_score_final_kernel(const double* __restrict__ part, int B, TFlowScore s, double* __restrict__ rec,
                                                               double* __restrict__ value)
{
    if (threadIdx.x != 0) return;
    const int b = blockIdx.x;
    double* r = rec + b * SCORE_REC;
    if (PASS == 1) {
        const double N = tflow_score_slices(part, b, 0);
        r[0] = N;
        for (int k = 1; k < 5; ++k) r[k] = N > 0.0 ? tflow_score_slices(part, b, k) / N : 0.0;
        for (int k = 5; k < SCORE_REC; ++k) r[k] = 0.0;
    } else {
        double total = 0.0;
        for (int bb = b; bb < (b == 0 && value ? B : b + 1); ++bb) {
            const double N = rec[bb * SCORE_REC], m_a = rec[bb * SCORE_REC + 3];
            double V[3];
            for (int k = 0; k < 3; ++k) V[k] = N > 0.0 ? tflow_score_slices(part, bb, k) / N : 0.0;
            const double S = tflow_score_value(N, m_a, V[0], V[1], V[2], s);
            if (bb == b) { r[5] = V[0]; r[6] = V[1]; r[7] = V[2]; r[8] = S; }
            total = bb == 0 ? S : total + S;
        }
        if (b == 0 && value) *value = total / (double)B;
    }
}

// g = d S_b / d u at a member o of a sample whose record R holds at least min_count members: the header's gradient.  tflow_score_q_kernel
// folds it into q; the iterated solve's gradient (flow_iter_kernels.h) takes g itself.
__device__ __forceinline__ void tflow_score_g(double ux, const TScorePoint& o, const double* __restrict__ R, const TFlowScore& s, double& gx, double& gy)
{
    const double N = R[0], m_rho = R[1], m_tau = R[2], m_a = R[3], m_n = R[4], Vr = R[5], Vt = R[6], Vn = R[7];
    const double c_rho = -(((s.w_direction * (1.0 - Vr)) * (2.0 * (o.rho - m_rho))) / N);
    const double c_tau = -(((s.w_direction * (1.0 - Vt)) * (2.0 * (o.tau - m_tau))) / N);
    const double gmx = (c_rho * o.px) / o.dist - (c_tau * o.py) / o.dist;
    const double gmy = (c_rho * o.py) / o.dist + (c_tau * o.px) / o.dist;
    const double d = gmx * o.nx + gmy * o.ny;
    gx = (gmx - d * o.nx) / o.nrm;
    gy = (gmy - d * o.ny) / o.nrm;
    const double A = m_a / s.max_norm;
    const double F = 1.0 - (Vn < 1.0 ? Vn : 1.0);
    const double sg = ux > 0.0 ? 1.0 : ux < 0.0 ? -1.0 : 0.0;
    gx = gx + ((s.w_strength * F) * sg) / (N * s.max_norm);
    const double c_n = Vn < 1.0 ? -(((s.w_strength * A) * (2.0 * (o.nrm - m_n))) / N) : 0.0;
    gx = gx + c_n * o.nx;
    gy = gy + c_n * o.ny;
}

// q of every pixel of one tile (blockIdx: tile x, tile y, sample).  Gxx, Gxy, Gyy are formed again in tflow_solve_kernel's order (rows
// first, offsets ascending, each sum started from its first term), so a, b, c and det are the solve's bits; g is the header's gradient
// from u and the sample's record.  q [2][n] replaces what the solve wrote there.
__global__ void __launch_bounds__(FLOW_T) tflow_score_q_kernel(const double* __restrict__ planes, const double* __restrict__ u, long long n, int H, int W, int r,
                                                               double eps, const uint8_t* __restrict__ mask, long long mask_bstride, TFlowScore s, const double* __restrict__ rec,
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
    const double ux = u[2 * base + p], uy = u[2 * base + HW + p];
    const double* R = rec + (long long)blockIdx.z * SCORE_REC;
    const double N = R[0];
    const TScorePoint o = tflow_score_point(ux, uy, x, y, H, W, !mask || mask[(long long)blockIdx.z * mask_bstride + p] != 0, s);
    double qx = 0.0, qy = 0.0;
    if (o.member && !(N < (double)s.min_count)) {
        double gx, gy;
        tflow_score_g(ux, o, R, s, gx, gy);
        qx = (c * gx - b * gy) / det;
        qy = (a * gy - b * gx) / det;
    }
    q[base + p] = qx;
    q[n + base + p] = qy;
}

}  // namespace eigt
