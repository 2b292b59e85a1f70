// cppn_motion_kernel.h -- moving CPPN textures: the arithmetic of cppn_render_kernel on per-sample, per-frame, per-layer affine
// coordinates, with the exact flow of every pixel and the visible-layer map ("Moving textures").
//
// One block is CPPN_THREADS pixels of one sample (blockIdx.y) and loops over its T frames: the one or two node programs of the sample
// are staged in LDS once, the [node][thread] float64 value columns (the render's conflict-free layout) are reused from frame to frame
// and from layer to layer.  The affines of a frame are uniform over the block; the host packs each beside its inverse, so one pointer
// walks the frames.  (They arrive through uniform-address vector loads: as a __restrict__ parameter of its own the pointer gives
// scalar loads and two SGPR spills beside the sixty SGPRs of the activations' hoisted constants; DESIGN.md has the figures.)
//
//   px = col - (W - 1) / 2, py = row - (H - 1) / 2                              (exact)
//   u = (a0 px + a1 py) + a2, v = (a3 px + a4 py) + a5                          A[b][t][l]: pixel -> texture; leaves x = u, y = v
//   layer 0 covers every pixel, layer 1 where u1 u1 + v1 v1 < 1.0; a pixel shows the topmost layer that covers it
//   byte = quant_u8(255 value_c) of the visible layer's output node c           (no background fill, no rounding mode)
//   flow = ((i0 u + i1 v) + i2 - px, (i3 u + i4 v) + i5 - py)                   Ainv[b][t + 1][visible layer]: texture -> pixel
//
// Every product and sum is one float64 rounding in the order written (the unit is compiled with -ffp-contract=off).  A thread
// evaluates the program of its visible layer only: a wave runs both only where the disc's edge crosses it, and the bytes do not
// depend on that.  cppn_render_kernel is left as it is; the node loop is restated here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cppn_kernel.h"

namespace eig {

struct CppnMotionArgs {
    const int32_t* node_off;  // [n*L + 1]; genome b*L + l is layer l of sample b
    const int32_t* edge_off;
    const uint8_t* node_act;
    const double* node_bias;
    const double* node_resp;
    const int32_t* edge_src;
    const double* edge_w;
    const int32_t* out_node;   // [n*L*c_out]
    const double* affine;      // [n][T][L][12]: a0 .. a5 (pixel -> texture), then i0 .. i5 (texture -> pixel; read only with flow)
    int W, H, N;               // N = H*W
    int T, L;
    int c_out, c_dim;
    uint8_t* frames;           // sample b at frames + b*f_bstride: [T][c_dim][N]
    long long f_bstride;
    double* flow;              // [n][T-1][2][N] or null
    uint8_t* layer;            // [n][T][N] or null
};

// bytes of one staged program: out[4] nn ne - - i32 | bias[nn] resp[nn] ew[ne] f64 | eoff[nn+1] esrc[ne] i32 | act[nn] u8, rounded up so that the next one is 8-aligned
__host__ __device__ inline size_t cppn_program_bytes(int nn, int ne)
{
    const size_t b = 32 + (size_t)nn * 16 + (size_t)ne * 8 + (size_t)(nn + 1) * 4 + (size_t)ne * 4 + (size_t)nn;
    return (b + 7) & ~(size_t)7;
}

__global__ void __launch_bounds__(CPPN_THREADS) cppn_motion_kernel(const CppnMotionArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int b = blockIdx.y;
    const int tid = threadIdx.x;
    double* vals = reinterpret_cast<double*>(smem);
    const int g0 = b * a.L;
    const int nA = a.node_off[g0], nB = a.node_off[g0 + 1], nC = a.node_off[g0 + a.L];
    const int eA = a.edge_off[nA], eB = a.edge_off[nB], eC = a.edge_off[nC];
    const int nn0 = nB - nA, ne0 = eB - eA, nn1 = nC - nB, ne1 = eC - eB;   // (L == 1: nC == nB, the second program is empty)
    // LDS carve: values [max(nn0, nn1)][T] f64 | program 0 | program 1
    unsigned char* prog0 = smem + (size_t)(nn0 > nn1 ? nn0 : nn1) * CPPN_THREADS * sizeof(double);
    unsigned char* prog1 = prog0 + cppn_program_bytes(nn0, ne0);
    for (int l = 0; l < a.L; ++l) {
        const int n0 = l ? nB : nA, e0 = l ? eB : eA, nn = l ? nn1 : nn0, ne = l ? ne1 : ne0;
        int32_t* s_out = reinterpret_cast<int32_t*>(l ? prog1 : prog0);   // the output nodes: c_dim <= 3 of them
        double* s_bias = reinterpret_cast<double*>(s_out + 8);
        double* s_resp = s_bias + nn;
        double* s_ew = s_resp + nn;
        int32_t* s_eoff = reinterpret_cast<int32_t*>(s_ew + ne);
        int32_t* s_esrc = s_eoff + nn + 1;
        uint8_t* s_act = reinterpret_cast<uint8_t*>(s_esrc + ne);
        for (int i = tid; i < nn; i += CPPN_THREADS) {
            s_bias[i] = a.node_bias[n0 + i];
            s_resp[i] = a.node_resp[n0 + i];
            s_act[i] = a.node_act[n0 + i];
        }
        for (int i = tid; i <= nn; i += CPPN_THREADS) s_eoff[i] = a.edge_off[n0 + i] - e0;
        if (tid < a.c_dim) s_out[tid] = a.out_node[(size_t)(g0 + l) * a.c_out + tid];
        if (tid == 0) { s_out[4] = nn; s_out[5] = ne; }   // the frame loop reads its counts from here: fewer scalars live across it
        for (int i = tid; i < ne; i += CPPN_THREADS) {
            s_ew[i] = a.edge_w[e0 + i];
            s_esrc[i] = a.edge_src[e0 + i];
        }
    }
    __syncthreads();

    const int p = blockIdx.x * CPPN_THREADS + tid;
    if (p >= a.N) return;   // (no barrier follows)
    const int row = p / a.W, col = p - row * a.W;
    const double px = (double)col - (double)(a.W - 1) / 2.0;
    const double py = (double)row - (double)(a.H - 1) / 2.0;
    // per-lane cursors, advanced by one frame per turn of the loop
    uint8_t* out = a.frames + (size_t)b * a.f_bstride + p;
    uint8_t* lay = a.layer ? a.layer + (size_t)b * a.T * a.N + p : nullptr;
    double* flo = a.flow ? a.flow + (size_t)b * (a.T - 1) * 2 * a.N + p : nullptr;
    const double* A = a.affine + (size_t)b * a.T * a.L * 12;   // uniform over the block

    for (int t = 0; t < a.T; ++t, A += a.L * 12) {
        double u = (A[0] * px + A[1] * py) + A[2];
        double v = (A[3] * px + A[4] * py) + A[5];
        int vis = 0;
        if (a.L == 2) {
            const double u1 = (A[12] * px + A[13] * py) + A[14];
            const double v1 = (A[15] * px + A[16] * py) + A[17];
            if (u1 * u1 + v1 * v1 < 1.0) { vis = 1; u = u1; v = v1; }
        }
        for (int l = 0; l < a.L; ++l) {
            if (l != vis) continue;
            const int32_t* s_out = reinterpret_cast<const int32_t*>(l ? prog1 : prog0);
            const int nn = __builtin_amdgcn_readfirstlane(s_out[4]), ne = __builtin_amdgcn_readfirstlane(s_out[5]);
            const double* s_bias = reinterpret_cast<const double*>(s_out + 8);
            const double* s_resp = s_bias + nn;
            const double* s_ew = s_resp + nn;
            const int32_t* s_eoff = reinterpret_cast<const int32_t*>(s_ew + ne);
            const int32_t* s_esrc = s_eoff + nn + 1;
            const uint8_t* s_act = reinterpret_cast<const uint8_t*>(s_esrc + ne);
            for (int n = 0; n < nn; ++n) {
                const int kb = s_eoff[n], ke = s_eoff[n + 1];
                double sum = 0.0;
                for (int k = kb; k < ke; ++k) {
                    const int src = s_esrc[k];
                    const double x = (src >= 0) ? vals[(size_t)src * CPPN_THREADS + tid] : (src == -1 ? u : src == -2 ? v : 1.0);
                    const double term = s_ew[k] * x;
                    sum = (k == kb) ? term : sum + term;   // as cppn_render_kernel: Python's sum() but for the sign of a zero
                }
                const double pre = s_resp[n] * sum;
                vals[(size_t)n * CPPN_THREADS + tid] = cppn_act(s_act[n], pre + s_bias[n]);
            }
            for (int c = 0; c < a.c_dim; ++c, out += a.N) *out = quant_u8(vals[(size_t)s_out[c] * CPPN_THREADS + tid] * 255.0);
        }
        if (lay) { *lay = (uint8_t)vis; lay += a.N; }
        if (flo && t < a.T - 1) {
            // the inverses of frame t + 1: both layers' through scalar loads, the visible layer's result selected per lane
            const double* I = A + a.L * 12 + 6;
            double qx = (I[0] * u + I[1] * v) + I[2];
            double qy = (I[3] * u + I[4] * v) + I[5];
            if (a.L == 2) {
                const double qx1 = (I[12] * u + I[13] * v) + I[14];
                const double qy1 = (I[15] * u + I[16] * v) + I[17];
                if (vis) { qx = qx1; qy = qy1; }
            }
            flo[0] = qx - px;
            flo[a.N] = qy - py;
            flo += 2 * (size_t)a.N;
        }
    }
}

}  // namespace eig
