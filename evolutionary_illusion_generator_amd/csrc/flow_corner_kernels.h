// flow_corner_kernels.h -- per-sample membership of the flow objective's scores from the fitness's own corners (DESIGN.md section 13,
// "The corner members").  The fitness scores the vectors of the at most max_corners points goodFeaturesToTrack picks on the reference
// image; this stage picks the same points on the device and hands them to the solve and score kernels as a per-sample mask:
//   1. the reference as the bytes the fitness would see: a byte reference as it is, a float one through tcorner_quant_kernel;
//   2. gray_kernel, mineig_kernel and corner_select_kernel of flow_kernels.h, the kernels of the fitness path itself, with its launch
//      shapes and scale (eigen_engine.hip, eigen_flow);
//   3. tcorner_member_kernel: the member plane [B][H W] uint8, 1 at every selected corner the shared mask (if any) counts.
// The plane is a constant of the graph, as every membership rule is.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flow_kernels.h"
#include "train_common.h"

namespace eigt {

constexpr int CORNER_MAX = 128;  // most corners of one sample (eigen_flow_members.max_corners)
constexpr int CORNER_T = 256;    // threads of tcorner_member_kernel's one block per sample

// The byte of every element of a float reference: clamped to [0, 1], then terr_fed_fwd_kernel's rule, (uint8_t)(int)(v * 255.0f).
// Sample b of ref at + b * r_bstride, per = C H W elements; out [B][per]; n = B per.
__global__ void __launch_bounds__(EW_T) tcorner_quant_kernel(const float* __restrict__ ref, long long r_bstride, long long per, long long n,
                                                             uint8_t* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const long long b = i / per;
    const float v = fminf(fmaxf(ref[b * r_bstride + (i - b * per)], 0.f), 1.f);
    out[i] = (uint8_t)(int)(v * 255.0f);
}

// The member plane of sample blockIdx.x: cleared, then 1 at each of its ncorners[b] corners (corners [B][K][2], x then y, whole
// numbers) that the shared mask [H][W] counts (mask nullptr: all).  The corners of one sample are distinct pixels and every store
// writes the same value, so the order of the stores plays no part.
__global__ void __launch_bounds__(CORNER_T) tcorner_member_kernel(const float* __restrict__ corners, const int* __restrict__ ncorners, int K, int H, int W,
                                                                  const uint8_t* __restrict__ mask, uint8_t* __restrict__ member)
{
    const int b = blockIdx.x;
    const long long HW = (long long)H * W;
    uint8_t* m = member + b * HW;
    for (long long p = threadIdx.x; p < HW; p += CORNER_T) m[p] = 0;
    __syncthreads();
    const int n = ncorners[b] < K ? ncorners[b] : K;
    for (int i = threadIdx.x; i < n; i += CORNER_T) {
        const int x = (int)corners[((long long)b * K + i) * 2], y = (int)corners[((long long)b * K + i) * 2 + 1];
        if (x < 0 || x >= W || y < 0 || y >= H) continue;
        const long long p = (long long)y * W + x;
        if (!mask || mask[p] != 0) m[p] = 1;
    }
}

}  // namespace eigt
