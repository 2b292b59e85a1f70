// dense_member_kernels.h -- HIP kernels of the dense motion fitness under members (eigen_dense_score_members, DESIGN.md section 14,
// "Members"): the pair pass of the Free structure over a compacted list of the members in place of a walk over every pixel.
//   tdense_member_list_kernel     the members of a sample, in ascending pixel order, from the flag plane tflow_free_prepare_kernel wrote
//   tdense_free_pair_list_kernel  tdense_free_pair_kernel over that list: one thread per member, the list walked in LDS tiles
// Every owner adds its members in ascending pixel order with the operations of tdense_free_pair_kernel, and a pixel that is no member
// gets the 0.0 that kernel stores for it, so L is that kernel's bytes for the same flags (tests/test_gpu_dense_members.py).  Float64,
// one IEEE operation per operation written (the build's -ffp-contract=off), fixed orders, no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flow_struct_kernels.h"

namespace eigt {

constexpr int LIST_T = 256;               // threads of tdense_member_list_kernel's one block per sample, and the pixels of one chunk
constexpr int LIST_WAVES = LIST_T / 64;   // a wave is 64 lanes on gfx950

// The member list of sample blockIdx.x: idx [B][cap] the members' pixel indices ascending, th [B][cap] their theta, count [B].  The flag
// plane is walked in ascending chunks of LIST_T pixels; within a chunk a lane's slot is the members before it in its wave (the ballot's
// bits below the lane) plus the earlier waves' totals plus the running offset: integers, exact.  Every L[b][p] is set to 0.0.  A sample
// has at most cap members by construction (its flags are a subset of a plane of at most cap ones, or cap is H W); a slot at or past cap
// is not written all the same, and count stops at cap.
__global__ void __launch_bounds__(LIST_T) tdense_member_list_kernel(const double* __restrict__ theta, const uint8_t* __restrict__ flag, int HW, int cap,
                                                                   int* __restrict__ idx, double* __restrict__ th, int* __restrict__ count, double* __restrict__ L)
{
    __shared__ int wtot[LIST_WAVES];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long base = (long long)b * HW, lbase = (long long)b * cap;
    int offset = 0;
    for (int p0 = 0; p0 < HW; p0 += LIST_T) {
        const int p = p0 + threadIdx.x;
        const bool m = p < HW && flag[base + p] != 0;
        const unsigned long long bits = __ballot(m);
        const int before = __popcll(bits & ((1ull << lane) - 1ull));
        if (lane == 0) wtot[wave] = __popcll(bits);
        __syncthreads();
        int slot = offset + before, total = 0;
        for (int w = 0; w < LIST_WAVES; ++w) {
            if (w < wave) slot += wtot[w];
            total += wtot[w];
        }
        if (p < HW) L[base + p] = 0.0;
        if (m && slot < cap) {
            idx[lbase + slot] = p;
            th[lbase + slot] = theta[base + p];
        }
        offset += total;
        __syncthreads();   // wtot is written again by the next chunk
    }
    if (threadIdx.x == 0) count[b] = offset < cap ? offset : cap;
}

// The pair pass over the list (blockIdx: block of PAIR_T slots, sample): thread k < count[b] owns member idx[k] and walks the list in
// ascending order in tiles of PAIR_T staged in LDS (the position, formed from the index as ym = idx / W, xm = idx - ym W, and theta), every
// lane reading the same LDS word.  Per pair the operations of tdense_free_pair_kernel, from 0.0, stored at L[b][idx[k]].  A block whose
// first slot is at or past count leaves as a whole before any barrier; in a partly filled block every thread stages and waits.
__global__ void __launch_bounds__(PAIR_T) tdense_free_pair_list_kernel(const int* __restrict__ idx, const double* __restrict__ th, const int* __restrict__ count, int cap,
                                                                       int HW, int W, double DD, double* __restrict__ L)
{
    __shared__ double sth[PAIR_T];
    __shared__ int sx[PAIR_T], sy[PAIR_T];
    const int b = blockIdx.y;
    const int cnt = count[b] < cap ? count[b] : cap;
    if ((int)(blockIdx.x * PAIR_T) >= cnt) return;   // uniform over the block
    const long long lbase = (long long)b * cap;
    const int k = blockIdx.x * PAIR_T + threadIdx.x;
    const bool own = k < cnt;
    const int pk = own ? idx[lbase + k] : 0;
    const double th_k = own ? th[lbase + k] : 0.0;
    const int yk = pk / W, xk = pk - yk * W;
    double Lk = 0.0;
    for (int m0 = 0; m0 < cnt; m0 += PAIR_T) {
        const int m = m0 + threadIdx.x;
        const int pm = m < cnt ? idx[lbase + m] : 0;
        const int ys = pm / W;
        sy[threadIdx.x] = ys;
        sx[threadIdx.x] = pm - ys * W;
        sth[threadIdx.x] = m < cnt ? th[lbase + m] : 0.0;
        __syncthreads();
        if (own) {
            const int n = cnt - m0 < PAIR_T ? cnt - m0 : PAIR_T;
            for (int j = 0; j < n; ++j) {
                const double ddx = (double)(sx[j] - xk), ddy = (double)(sy[j] - yk);
                double f = (ddx * ddx + ddy * ddy) / DD;
                f = f > 1.0 ? 1.0 : f;
                if (f < 1.0) {
                    double o = th_k + f * STRUCT_PI;
                    o = (o - 2.0 * floor(o * 0.5)) * STRUCT_PI;
                    Lk += fabs(sth[j] - o);
                }
            }
        }
        __syncthreads();
    }
    if (own && pk < HW) L[(long long)b * HW + pk] = Lk;
}

}  // namespace eigt
