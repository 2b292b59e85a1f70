// train_kernels.h -- HIP kernels of PredNet training (prednet_train.hip): a direct 3x3 implicit-GEMM
// convolution on v_mfma_f32_16x16x4_f32 that serves the training forward and dgrad, a split-K wgrad GEMM on the same
// instruction with a fixed-order slab reducer, and the element-wise forward / backward kernels of the error units, ConvLSTM,
// ConvP activations, max-pool, loss and Adam.  Every reduction has a fixed partition and a fixed order: no float atomics,
// so gradients and weights are bit-identical from run to run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "train_common.h"  // WAVE, EW_T

namespace eigt {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// One source of a 3x3 'same' convolution.  Source sample n lives at p + n * nstride as [cin][Hs][Ws]; up = 1 reads it as the
// nearest 2x upsample of a half-resolution map (Hs = H / 2).  Weight modes:
//   wmode 0 (forward): w is OIHW [cout][cin][3][3]
//   wmode 1 (dgrad):   w is the OIHW weight of the forward convolution this one differentiates, [cin][cout][3][3]
//                      (its Cout is this source, its Cin this output), read transposed and spatially flipped.
struct TSrc {
    const float* p;
    const float* w;
    long long nstride;
    int cin, up, wmode, pad_;
};

struct TConvArgs {
    TSrc s[3];
    int nsrc;
    float* out;            // [n][cout][H][W] at out + n * out_nstride
    long long out_nstride;
    const float* bias;     // [cout] or nullptr
    int cout, H, W, N;     // output channels, size, samples
    int accumulate;        // 1: out += result (every element has one writer: no atomics)
};

// Implicit GEMM D[co][pixel] = sum_k A[co][k] * B[k][pixel], k = (source, ci, tap).  One wave per block computes a
// (16 * MT) x (16 * NT) tile: MT output-channel blocks by NT blocks of 16 consecutive pixels (row-major over n, y, x).
// Operands are read per lane straight from L1 / L2 (A[l & 15][k = l >> 4], B[k = l >> 4][l & 15]); C/D: row (l >> 4) * 4 + r,
// column l & 15.
template <int MT, int NT>
__global__ void __launch_bounds__(WAVE) tconv3x3_kernel(const TConvArgs a)
{
    const int lane = threadIdx.x;
    const int HW = a.H * a.W;
    const long long P = (long long)a.N * HW;
    const long long pbase = (long long)blockIdx.x * (16 * NT);
    const int co0 = blockIdx.y * (16 * MT);
    const int kq = lane >> 4, jl = lane & 15;

    int pn[NT], py[NT], px[NT];
    bool pv[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const long long p = pbase + n * 16 + jl;
        pv[n] = p < P;
        const long long pc = pv[n] ? p : 0;
        pn[n] = (int)(pc / HW);
        const int rem = (int)(pc - (long long)pn[n] * HW);
        py[n] = rem / a.W;
        px[n] = rem - py[n] * a.W;
    }
    f32x4 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int si = 0; si < a.nsrc; ++si) {
        const TSrc s = a.s[si];
        const int K = s.cin * 9;
        const int Hs = s.up ? a.H >> 1 : a.H, Ws = s.up ? a.W >> 1 : a.W;
        const int HWs = Hs * Ws;
        for (int k0 = 0; k0 < K; k0 += 4) {
            const int kk = k0 + kq;
            const bool kv = kk < K;
            const int ci = kk / 9, tap = kk - ci * 9;
            const int ky = tap / 3, kx = tap - ky * 3;
            float av[MT], bv[NT];
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const int co = co0 + m * 16 + jl;
                const long long wi = s.wmode ? ((long long)ci * a.cout + co) * 9 + (8 - tap) : (long long)co * K + kk;
                av[m] = (kv && co < a.cout) ? s.w[wi] : 0.f;
            }
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const int yy = py[n] + ky - 1, xx = px[n] + kx - 1;
                const bool in = kv && pv[n] && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
                const int ys = s.up ? yy >> 1 : yy, xs = s.up ? xx >> 1 : xx;
                bv[n] = in ? s.p[pn[n] * s.nstride + (long long)ci * HWs + ys * Ws + xs] : 0.f;
            }
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int n = 0; n < NT; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], bv[n], acc[m][n], 0, 0, 0);
        }
    }
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        if (!pv[n]) continue;
        float* o = a.out + pn[n] * a.out_nstride + py[n] * a.W + px[n];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = co0 + m * 16 + kq * 4 + r;
                if (co >= a.cout) continue;
                float v = acc[m][n][r];
                if (a.bias) v += a.bias[co];
                if (a.accumulate) v += o[(long long)co * HW];
                o[(long long)co * HW] = v;
            }
    }
}

struct TWgradArgs {
    const float* dy;       // [n][cout][H][W] at dy + n * dy_nstride: the output gradient
    long long dy_nstride;
    TSrc x;                // the forward source (its w / wmode unused)
    float* slab;           // [nsplit][cout][cin * 9]
    int cout, H, W, N;
    int nsplit;
    long long chunk;       // pixels per split (a multiple of 4)
};

// dW[co][kk] = sum over pixels p of dy[co][p] * im2col(x)[kk][p]: M = cout, N = cin * 9, K = N * H * W pixels, split into
// nsplit fixed contiguous pixel ranges; block z writes its partial sums to slab z (plain stores), tsum_slabs_kernel adds the
// slabs in order.  A[co = l & 15][pixel = l >> 4], B[pixel = l >> 4][kk = l & 15].
template <int MT, int NT>
__global__ void __launch_bounds__(WAVE) twgrad_kernel(const TWgradArgs a)
{
    const int lane = threadIdx.x;
    const int HW = a.H * a.W;
    const long long P = (long long)a.N * HW;
    const int K = a.x.cin * 9;
    const int kk0 = blockIdx.x * (16 * NT), co0 = blockIdx.y * (16 * MT);
    const int kq = lane >> 4, jl = lane & 15;
    const long long p_begin = (long long)blockIdx.z * a.chunk;
    const long long p_end = p_begin + a.chunk < P ? p_begin + a.chunk : P;
    const int Hs = a.x.up ? a.H >> 1 : a.H, Ws = a.x.up ? a.W >> 1 : a.W;
    const int HWs = Hs * Ws;

    int bci[NT], bky[NT], bkx[NT];
    bool bkv[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int kk = kk0 + n * 16 + jl;
        bkv[n] = kk < K;
        bci[n] = kk / 9;
        const int tap = kk - bci[n] * 9;
        bky[n] = tap / 3 - 1;
        bkx[n] = tap - (tap / 3) * 3 - 1;
    }
    f32x4 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

    // this lane's pixel p = p0 + kq, decoded once and advanced by 4 per step
    long long p = p_begin + kq;
    int pn = (int)(p / HW);
    int rem = (int)(p - (long long)pn * HW);
    int y = rem / a.W, x = rem - y * a.W;
    for (long long p0 = p_begin; p0 < p_end; p0 += 4) {
        const bool ok = p < p_end;
        float av[MT], bv[NT];
        const float* dyp = a.dy + pn * a.dy_nstride + y * a.W + x;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int co = co0 + m * 16 + jl;
            av[m] = (ok && co < a.cout) ? dyp[(long long)co * HW] : 0.f;
        }
        const float* xp = a.x.p + pn * a.x.nstride;
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int yy = y + bky[n], xx = x + bkx[n];
            const bool in = ok && bkv[n] && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
            const int ys = a.x.up ? yy >> 1 : yy, xs = a.x.up ? xx >> 1 : xx;
            bv[n] = in ? xp[(long long)bci[n] * HWs + ys * Ws + xs] : 0.f;
        }
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], bv[n], acc[m][n], 0, 0, 0);
        p += 4;
        x += 4;
        while (x >= a.W) {
            x -= a.W;
            if (++y == a.H) { y = 0; ++pn; }
        }
    }
    float* slab = a.slab + (long long)blockIdx.z * a.cout * K;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int kk = kk0 + n * 16 + jl;
        if (kk >= K) continue;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = co0 + m * 16 + kq * 4 + r;
                if (co < a.cout) slab[(long long)co * K + kk] = acc[m][n][r];
            }
    }
}

// out[i] = slab[0][i] + slab[1][i] + ... in split order
__global__ void __launch_bounds__(EW_T) tsum_slabs_kernel(const float* __restrict__ slab, int nsplit, long long n, float* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    float s = slab[i];
    for (int k = 1; k < nsplit; ++k) s += slab[(long long)k * n + i];
    out[i] = s;
}

// bias gradient partials: block (c, k) sums dy[n][c][.] over the k-th of gridDim.y fixed slices of the (sample, pixel) range, a
// fixed strided partition per thread, then a fixed LDS tree; part[k][c] (tsum_slabs_kernel adds the slices in order)
__global__ void __launch_bounds__(EW_T) tbias_grad_kernel(const float* __restrict__ dy, int C, int HW, int N, float* __restrict__ part)
{
    __shared__ float red[EW_T];
    const int c = blockIdx.x;
    const long long n_el = (long long)N * HW;
    const long long per = (n_el + gridDim.y - 1) / gridDim.y;
    const long long e0 = (long long)blockIdx.y * per, e1 = e0 + per < n_el ? e0 + per : n_el;
    float s = 0.f;
    for (long long i = e0 + threadIdx.x; i < e1; i += EW_T) {
        const long long n = i / HW, j = i - n * HW;
        s += dy[(n * C + c) * HW + j];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = EW_T / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[(long long)blockIdx.y * C + c] = red[0];
}

// E = [relu(A - P), relu(P - A)] of one layer at one step.  Layer 0: A = frame byte / 255 (frame b at x + b * xbstride);
// layer l > 0: A = maxpool2(relu(ZA)) with ZA [B][C][2H][2W] the ConvA output.
__global__ void __launch_bounds__(EW_T) terr_fwd_kernel(const uint8_t* __restrict__ x, long long xbstride, const float* __restrict__ za,
                                                        const float* __restrict__ P, float* __restrict__ E, int C, int H, int W, int B)
{
    const int HW = H * W;
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= (long long)B * C * HW) return;
    const int b = (int)(i / ((long long)C * HW));
    const int r = (int)(i - (long long)b * C * HW);
    const int c = r / HW, j = r - c * HW;
    float A;
    if (x) {
        A = (float)x[b * xbstride + r] / 255.0f;
    } else {
        const int y = j / W, xx = j - y * W;
        const float* z = za + ((long long)b * C + c) * 4 * HW + (2 * y) * (2 * W) + 2 * xx;
        A = fmaxf(fmaxf(fmaxf(z[0], z[1]), fmaxf(z[2 * W], z[2 * W + 1])), 0.f);
    }
    const float p = P[i];
    float* e = E + (long long)b * 2 * C * HW + (long long)c * HW + j;
    e[0] = fmaxf(A - p, 0.f);
    e[(long long)C * HW] = fmaxf(p - A, 0.f);
}

// Image-layer error unit of a self-fed step: the input is the previous prediction P0 itself (requant = 0: E is exactly zero)
// or the byte the inference engine would emit for it, over 255 (requant = 1; the statement of EPI_CONVP and e0_resume_kernel in
// conv_mfma.h).  The fed-back value is a constant of the graph; terr_bwd_kernel sends dE into dP under the mask E > 0.
__global__ void __launch_bounds__(EW_T) terr_fed_fwd_kernel(const float* __restrict__ P, float* __restrict__ E, int requant, long long per_b, long long n)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const long long b = i / per_b;
    const float v = P[i];
    const float A = requant ? (float)(uint8_t)(int)(v * 255.0f) / 255.0f : v;
    float* e = E + b * 2 * per_b + (i - b * per_b);
    e[0] = fmaxf(A - v, 0.f);
    e[per_b] = fmaxf(v - A, 0.f);
}

// Backward of E = [relu(A - P), relu(P - A)] (relu'(0) = 0: a unit that is zero passes nothing): dP_prev = -dA.  For l > 0 the
// max-pool / ReLU backward follows: dA goes to the first maximum of the 2x2 window of relu(ZA) in row-major order, where ZA > 0;
// ZA is overwritten with dZA (each thread owns its window).  SEED = 1 (the error-unit objective, layers l > 0): `seed`, the
// derivative of the loss by every element of this E, is added to dE ahead of the mask; SEED = 0 is the arithmetic without it.
template <int SEED>
__global__ void __launch_bounds__(EW_T) terr_bwd_kernel(const float* __restrict__ dE, const float* __restrict__ E, float* __restrict__ dP,
                                                        float* za, int C, int H, int W, int B, float seed)
{
    const int HW = H * W;
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= (long long)B * C * HW) return;
    const int b = (int)(i / ((long long)C * HW));
    const int r = (int)(i - (long long)b * C * HW);
    const int c = r / HW, j = r - c * HW;
    const long long e0 = (long long)b * 2 * C * HW + (long long)c * HW + j, e1 = e0 + (long long)C * HW;
    float d0 = dE[e0], d1 = dE[e1];
    if constexpr (SEED) { d0 += seed; d1 += seed; }
    const float dA = (E[e0] > 0.f ? d0 : 0.f) - (E[e1] > 0.f ? d1 : 0.f);
    dP[i] = -dA;
    if (za) {
        const int y = j / W, xx = j - y * W;
        float* z = za + ((long long)b * C + c) * 4 * HW + (2 * y) * (2 * W) + 2 * xx;
        const float v[4] = {fmaxf(z[0], 0.f), fmaxf(z[1], 0.f), fmaxf(z[2 * W], 0.f), fmaxf(z[2 * W + 1], 0.f)};
        const bool pos[4] = {z[0] > 0.f, z[1] > 0.f, z[2 * W] > 0.f, z[2 * W + 1] > 0.f};
        int am = 0;
        for (int k = 1; k < 4; ++k) if (v[k] > v[am]) am = k;
        float g[4] = {0.f, 0.f, 0.f, 0.f};
        if (pos[am]) g[am] = dA;
        z[0] = g[0]; z[1] = g[1]; z[2 * W] = g[2]; z[2 * W + 1] = g[3];
    }
}

__device__ __forceinline__ float tsigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// ConvLSTM forward, gates stacked i, f, c, o along the channels.  zg [B][4C][H][W] holds the summed convolutions plus bias on
// entry and the activations i, f, g = tanh(zc), o on exit (the tape).  Peepholes (per pixel, [C][H][W]) see the old c.
__global__ void __launch_bounds__(EW_T) tlstm_fwd_kernel(float* zg, const float* __restrict__ c_old, float* __restrict__ c_new,
                                                         float* __restrict__ h_new, const float* __restrict__ wci, const float* __restrict__ wcf,
                                                         const float* __restrict__ wco, int C, int HW, int B)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= (long long)B * C * HW) return;
    const int b = (int)(i / ((long long)C * HW));
    const int r = (int)(i - (long long)b * C * HW);
    const long long CHW = (long long)C * HW;
    float* z = zg + (long long)b * 4 * CHW + r;
    const float co = c_old[i];
    const float ig = tsigmoid(z[0] + wci[r] * co);
    const float fg = tsigmoid(z[CHW] + wcf[r] * co);
    const float gg = tanhf(z[2 * CHW]);
    const float og = tsigmoid(z[3 * CHW] + wco[r] * co);
    const float cn = gg * ig + fg * co;
    z[0] = ig; z[CHW] = fg; z[2 * CHW] = gg; z[3 * CHW] = og;
    c_new[i] = cn;
    h_new[i] = og * tanhf(cn);
}

// ConvLSTM backward of one step.  dh = dh_p (ConvP dgrad) + dh_carry (the h source of the next step, may be null) + the 2x2 sum of
// dh_up (the upsampled source of the layer below, [B][C][2H][2W], may be null).  dc (in: from the next step, out: to the previous)
// gains the peephole paths.  The gate activations in zg are overwritten with dZ (the tape wgrad reads).
__global__ void __launch_bounds__(EW_T) tlstm_bwd_kernel(float* zg, const float* __restrict__ c_old, const float* __restrict__ c_new,
                                                         const float* __restrict__ dh_p, const float* __restrict__ dh_carry,
                                                         const float* __restrict__ dh_up, float* __restrict__ dc,
                                                         const float* __restrict__ wci, const float* __restrict__ wcf,
                                                         const float* __restrict__ wco, int C, int H, int W, int B)
{
    const int HW = H * W;
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= (long long)B * C * HW) return;
    const int b = (int)(i / ((long long)C * HW));
    const int r = (int)(i - (long long)b * C * HW);
    const long long CHW = (long long)C * HW;
    float* z = zg + (long long)b * 4 * CHW + r;
    float dh = dh_p[i];
    if (dh_carry) dh += dh_carry[i];
    if (dh_up) {
        const int c = r / HW, j = r - c * HW;
        const int y = j / W, x = j - y * W;
        const float* u = dh_up + ((long long)b * C + c) * 4 * HW + (2 * y) * (2 * W) + 2 * x;
        dh += (u[0] + u[1]) + (u[2 * W] + u[2 * W + 1]);
    }
    const float ig = z[0], fg = z[CHW], gg = z[2 * CHW], og = z[3 * CHW];
    const float co = c_old[i], tc = tanhf(c_new[i]);
    const float dcv = dc[i] + dh * og * (1.f - tc * tc);
    const float dzi = dcv * gg * ig * (1.f - ig);
    const float dzf = dcv * co * fg * (1.f - fg);
    const float dzc = dcv * ig * (1.f - gg * gg);
    const float dzo = dh * tc * og * (1.f - og);
    z[0] = dzi; z[CHW] = dzf; z[2 * CHW] = dzc; z[3 * CHW] = dzo;
    dc[i] = dcv * fg + dzi * wci[r] + dzf * wcf[r] + dzo * wco[r];
}

// peephole gradients dW[g][c][y][x] = sum over samples n of dZ_g[n] * c_old[n], g = i, f, o (a fixed loop over n per element)
__global__ void __launch_bounds__(EW_T) tpeep_grad_kernel(const float* __restrict__ dz, const float* __restrict__ c_old, int C, int HW, int N,
                                                          float* __restrict__ dwi, float* __restrict__ dwf, float* __restrict__ dwo)
{
    const long long CHW = (long long)C * HW;
    const long long r = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (r >= CHW) return;
    float si = 0.f, sf = 0.f, so = 0.f;
    for (int n = 0; n < N; ++n) {
        const float co = c_old[n * CHW + r];
        const float* z = dz + n * 4 * CHW + r;
        si += z[0] * co;
        sf += z[CHW] * co;
        so += z[3 * CHW] * co;
    }
    dwi[r] = si; dwf[r] = sf; dwo[r] = so;
}

// ConvP activation in place: clamp(v, 0, 1) on layer 0, relu above; pred (layer 0, optional) gets P0 of this step for sample b at
// pred + b * pred_bstride
__global__ void __launch_bounds__(EW_T) tpact_fwd_kernel(float* P, long long n, int clamp01, float* __restrict__ pred, long long per_b, long long pred_bstride)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const float v = P[i];
    const float p = clamp01 ? fminf(fmaxf(v, 0.f), 1.f) : fmaxf(v, 0.f);
    P[i] = p;
    if (pred) {
        const long long b = i / per_b;
        pred[b * pred_bstride + (i - b * per_b)] = p;
    }
}

// dV = (dP + dloss) * act'(V).  The activation's derivative is read off P: clamp passes where 0 < v < 1 (0 < P < 1), relu where
// v > 0 (P > 0).  dloss (layer 0, steps 0..T-2) = loss_scale (P0_t - x_{t+1}) with frame t + 1 of sample b at x + b * xbstride;
// loss_scale is per launch, i.e. per step: 2 / n_terms without step weights, 2 w_t / (sum w * numel) with them.  OBJ = 1 (the
// error-unit objective): dloss = loss_scale sign(P0_t - x_{t+1}), sign(0) = 0, the derivative of the image layer's error units
// against the true frame; loss_scale = w_t lambda_0 / (sum w * 2 numel).
template <int OBJ>
__global__ void __launch_bounds__(EW_T) tpact_bwd_kernel(const float* __restrict__ P, const float* __restrict__ dP, const uint8_t* __restrict__ x,
                                                         long long xbstride, long long per_b, float loss_scale, int clamp01, long long n,
                                                         float* __restrict__ dV)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const float p = P[i];
    float g = dP[i];
    if (x) {
        const long long b = i / per_b;
        const float d = p - (float)x[b * xbstride + (i - b * per_b)] / 255.0f;
        if constexpr (OBJ == 0) {
            g += loss_scale * d;
        } else {
            if (d > 0.f) g += loss_scale;
            else if (d < 0.f) g -= loss_scale;
        }
    }
    const bool pass = clamp01 ? (p > 0.f && p < 1.f) : p > 0.f;
    dV[i] = pass ? g : 0.f;
}

// loss partials: block k sums (P0_t - x_{t+1})^2 over its fixed slice of the (t, b, element) terms in double; tloss_final_kernel
// adds the partials in order
__global__ void __launch_bounds__(EW_T) tloss_partial_kernel(const float* __restrict__ P0, const uint8_t* __restrict__ x, long long xbstride,
                                                             int T1, int B, long long per_b, double* __restrict__ part)
{
    __shared__ double red[EW_T];
    const long long n = (long long)T1 * B * per_b;
    double s = 0.0;
    for (long long i = (long long)blockIdx.x * EW_T + threadIdx.x; i < n; i += (long long)gridDim.x * EW_T) {
        const long long tb = i / per_b, e = i - tb * per_b;
        const int t = (int)(tb / B), b = (int)(tb - (long long)t * B);
        // P0 slot t + 1 (the prediction after frame t) against frame t + 1
        const double d = (double)P0[((long long)(t + 1) * B + b) * per_b + e] - (double)((float)x[b * xbstride + (long long)(t + 1) * per_b + e] / 255.0f);
        s += d * d;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = EW_T / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

__global__ void __launch_bounds__(64) tloss_final_kernel(const double* __restrict__ part, int n, double scale, double* __restrict__ out)
{
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int k = 0; k < n; ++k) s += part[k];
    out[0] = s * scale;
}

// per-step loss partials: block (k, t) sums (P0_t - x_{t+1})^2 over its fixed strided slice of the (b, element) terms of step t
// in double, then a fixed LDS tree; part[t][k].  P0 points at the prediction of the first step, x at the frame it is compared
// with; step t is P0 + t * B * per_b against x + t * per_b.
// TERM_ABS sums the image layer's error units against that frame instead, relu(x - P0) + relu(P0 - x), each formed in float as
// terr_fwd_kernel forms them.  TERM_SUM sums the floats themselves (x unused): P0 is then one layer's E tape, [B][2C][H][W] per
// step, per_b = 2 C H W.
enum { TERM_SQ = 0, TERM_ABS = 1, TERM_SUM = 2 };
template <int TERM>
__global__ void __launch_bounds__(EW_T) tloss_step_partial_kernel(const float* __restrict__ P0, const uint8_t* __restrict__ x, long long xbstride,
                                                                  int B, long long per_b, double* __restrict__ part)
{
    __shared__ double red[EW_T];
    const int t = blockIdx.y;
    const long long n = (long long)B * per_b;
    const float* p = P0 + (long long)t * n;
    const uint8_t* xt = x + (long long)t * per_b;
    double s = 0.0;
    for (long long i = (long long)blockIdx.x * EW_T + threadIdx.x; i < n; i += (long long)gridDim.x * EW_T) {
        if constexpr (TERM == TERM_SUM) {
            s += (double)p[i];
        } else {
            const long long b = i / per_b;
            const float xv = (float)xt[b * xbstride + (i - b * per_b)] / 255.0f;
            if constexpr (TERM == TERM_SQ) {
                const double d = (double)p[i] - (double)xv;
                s += d * d;
            } else {
                s += (double)fmaxf(xv - p[i], 0.f) + (double)fmaxf(p[i] - xv, 0.f);
            }
        }
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = EW_T / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[(long long)t * gridDim.x + blockIdx.x] = red[0];
}

// step_loss[t * stride] = (part[t][0] + part[t][1] + ... in order) / numel, one thread per step (stride > 1: one column of the
// [step][layer] table of error-unit means)
__global__ void __launch_bounds__(64) tloss_step_final_kernel(const double* __restrict__ part, int nblk, int n_steps, double numel, double* __restrict__ step_loss,
                                                              int stride)
{
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n_steps) return;
    double s = 0.0;
    for (int k = 0; k < nblk; ++k) s += part[(long long)t * nblk + k];
    step_loss[(long long)t * stride] = s / numel;
}

// Adam as chainer defines it: m += (1 - b1) (g - m); v += (1 - b2) (g^2 - v); p -= lr_t m / (sqrt(v) + eps).  omb1 = 1 - b1 and
// omb2 = 1 - b2 come from the host in double (1 - 0.999f in float is off by 1.3e-5)
__global__ void __launch_bounds__(EW_T) tadam_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, const float* __restrict__ g,
                                                     long long n, float lr_t, float omb1, float omb2, float eps)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const float gi = g[i];
    const float mi = m[i] + omb1 * (gi - m[i]);
    const float vi = v[i] + omb2 * (gi * gi - v[i]);
    m[i] = mi;
    v[i] = vi;
    p[i] -= lr_t * mi / (sqrtf(vi) + eps);
}

}  // namespace eigt
