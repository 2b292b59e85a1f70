// cppn_grad_kernel.h -- the backward pass through the batched CPPN render (cppn_kernel.h): d loss / d (bias, response, weight) of
// every genome of a batch from d loss / d image ("CPPN parameter gradients").
//
// cppn_grad_kernel: grid (pixel blocks, genome) as cppn_render_kernel, one thread per pixel, ONE wave per block.  The forward is the
// render's, operation by operation (cppn_act, separate product and sum in connection order, pre = resp * sum, act(pre + bias), under
// the unit's -ffp-contract=off), so the node values and with them the quantisation mask are the bits the render produced.  Values and
// adjoints live in LDS as [node][thread] columns.  The seed passes straight through the uint8 quantisation where the byte follows the
// node (not background, 0 <= trunc(255 v) <= 255) and is zero elsewhere.  The reverse pass runs in float64; per parameter the 64
// lanes are added by a fixed butterfly (every lane ends with the same sum) and lane 0 writes it into the block's float64 slab.
// cppn_grad_sum_kernel adds the slabs in block order.  No atomics: the same call gives the same bits, and the bits of a genome do not
// depend on the batch it is in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cppn_kernel.h"

namespace eig {

constexpr int CPPN_GRAD_THREADS = 64;   // one wave: the in-block tree is six lane exchanges; half the columns of the render's 128

struct CppnGradArgs {
    CppnArgs c;               // the render's arguments (out, out_f64, mode unused); c.max_nodes: LDS columns of values AND of adjoints
    const float* image_grad;  // d loss / d (byte / 255): image g at image_grad + g * g_bstride as [c_dim][N]
    long long g_bstride;      // floats
    int total_nodes, total_edges;
    double* slabs;            // [pixel blocks][2 * total_nodes + total_edges]: bias | resp | w, each in the batch's own layout
};

// the sum over the wave's 64 lanes by a fixed butterfly: lane l adds the value of lane l ^ 32, ^ 16, ... ^ 1 (a + b is commutative,
// so every lane holds the same bits at every level)
__device__ __forceinline__ double cppn_wave_sum(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

// d act / d z from the pre-activation z and the value y = act(z) the forward kept
__device__ __forceinline__ double cppn_act_grad(int act, double z, double y)
{
    switch (act) {
        case 0: return (5.0 * y) * (1.0 - y);
        case 1: return 2.5 * (1.0 - y * y);
        case 2: return z > 0.0 ? 1.0 : (z < 0.0 ? -1.0 : 0.0);
        case 3: return (-10.0 * z) * y;
        case 4: return 1.0;
        case 5: return cos(z);
        default: return z > 0.0 ? 1.0 : 0.0;
    }
}

__global__ void __launch_bounds__(CPPN_GRAD_THREADS) cppn_grad_kernel(const CppnGradArgs ga)
{
    constexpr int T = CPPN_GRAD_THREADS;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const CppnArgs& a = ga.c;
    const int g = blockIdx.y;
    const int n0 = a.node_off[g], n1 = a.node_off[g + 1];
    const int nn = n1 - n0;
    const int e0 = a.edge_off[n0], e1 = a.edge_off[n1];
    const int ne = e1 - e0;
    // LDS carve: values [max_nodes][T] f64 | adjoints [max_nodes][T] f64 | bias[nn] | resp[nn] | ew[ne] f64 | eoff[nn+1] i32 | esrc[ne] i32 | act[nn] u8
    double* vals = reinterpret_cast<double*>(smem);
    double* adj = vals + (size_t)a.max_nodes * T;
    double* s_bias = adj + (size_t)a.max_nodes * T;
    double* s_resp = s_bias + nn;
    double* s_ew = s_resp + nn;
    int32_t* s_eoff = reinterpret_cast<int32_t*>(s_ew + ne);
    int32_t* s_esrc = s_eoff + nn + 1;
    uint8_t* s_act = reinterpret_cast<uint8_t*>(s_esrc + ne);
    const int tid = threadIdx.x;
    for (int i = tid; i < nn; i += T) {
        s_bias[i] = a.node_bias[n0 + i];
        s_resp[i] = a.node_resp[n0 + i];
        s_act[i] = a.node_act[n0 + i];
    }
    for (int i = tid; i <= nn; i += T) s_eoff[i] = a.edge_off[n0 + i] - e0;
    for (int i = tid; i < ne; i += T) {
        s_ew[i] = a.edge_w[e0 + i];
        s_esrc[i] = a.edge_src[e0 + i];
    }
    __syncthreads();

    // a lane past the last pixel runs along on zeros (the butterfly needs all 64) and contributes exact zeros
    const int p = blockIdx.x * T + tid;
    const bool live = p < a.N;
    double leaf[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) leaf[i] = (live && i < a.n_planes) ? a.planes[(size_t)i * a.N + p] : 0.0;
    const bool seeded = live && !(leaf[0] == -1.0);

    // ---- forward: cppn_render_kernel's loop
    for (int n = 0; n < nn; ++n) {
        const int b = s_eoff[n], e = s_eoff[n + 1];
        double sum = 0.0;
        for (int k = b; k < e; ++k) {
            const int src = s_esrc[k];
            double x;
            if (src >= 0) x = vals[(size_t)src * T + tid];
            else {
                const int li = -src - 1;
                x = (li >= a.n_planes) ? 1.0 : (li == 0 ? leaf[0] : li == 1 ? leaf[1] : li == 2 ? leaf[2] : leaf[3]);
            }
            const double term = s_ew[k] * x;
            sum = (k == b) ? term : sum + term;
        }
        const double pre = s_resp[n] * sum;
        vals[(size_t)n * T + tid] = cppn_act(s_act[n], pre + s_bias[n]);
        adj[(size_t)n * T + tid] = 0.0;
    }

    // ---- seed: straight through uint8(v * 255) where the byte follows the node
    if (seeded) {
        for (int c = 0; c < a.c_dim; ++c) {
            const int o = a.out_node[g * a.c_out + c];
            const double t = trunc(vals[(size_t)o * T + tid] * 255.0);
            if (t >= 0.0 && t <= 255.0)
                adj[(size_t)o * T + tid] += (double)ga.image_grad[(size_t)g * ga.g_bstride + (size_t)c * a.N + p];
        }
    }

    // ---- reverse, last node first
    double* slab = ga.slabs + (size_t)blockIdx.x * (2 * (size_t)ga.total_nodes + ga.total_edges);
    double* g_bias = slab + n0;
    double* g_resp = slab + ga.total_nodes + n0;
    double* g_w = slab + 2 * (size_t)ga.total_nodes + e0;
    for (int n = nn - 1; n >= 0; --n) {
        const int b = s_eoff[n], e = s_eoff[n + 1];
        double sum = 0.0;
        for (int k = b; k < e; ++k) {
            const int src = s_esrc[k];
            double x;
            if (src >= 0) x = vals[(size_t)src * T + tid];
            else {
                const int li = -src - 1;
                x = (li >= a.n_planes) ? 1.0 : (li == 0 ? leaf[0] : li == 1 ? leaf[1] : li == 2 ? leaf[2] : leaf[3]);
            }
            const double term = s_ew[k] * x;
            sum = (k == b) ? term : sum + term;
        }
        const double resp = s_resp[n];
        const double pre = resp * sum;
        const double z = pre + s_bias[n];
        const double an = adj[(size_t)n * T + tid];
        const double d = live ? an * cppn_act_grad(s_act[n], z, vals[(size_t)n * T + tid]) : 0.0;
        const double rb = cppn_wave_sum(d);
        const double rr = cppn_wave_sum(d * sum);
        if (tid == 0) { g_bias[n] = rb; g_resp[n] = rr; }
        const double ds = d * resp;
        for (int k = b; k < e; ++k) {
            const int src = s_esrc[k];
            double x;
            if (src >= 0) {
                x = vals[(size_t)src * T + tid];
                adj[(size_t)src * T + tid] += ds * s_ew[k];
            } else {
                const int li = -src - 1;
                x = (li >= a.n_planes) ? 1.0 : (li == 0 ? leaf[0] : li == 1 ? leaf[1] : li == 2 ? leaf[2] : leaf[3]);
            }
            const double rw = cppn_wave_sum(ds * x);
            if (tid == 0) g_w[k] = rw;
        }
    }
}

// out[i] = the sum over the pixel blocks, in block order, of slabs[block][i]; one thread per parameter
__global__ void __launch_bounds__(256) cppn_grad_sum_kernel(const double* __restrict__ slabs, double* __restrict__ out, int n_params, int n_blocks)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_params) return;
    double s = 0.0;
    for (int b = 0; b < n_blocks; ++b) s = s + slabs[(size_t)b * n_params + i];
    out[i] = s;
}

}  // namespace eig
