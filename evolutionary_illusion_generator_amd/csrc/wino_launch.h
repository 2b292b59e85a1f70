// wino_launch.h -- what the engine's translation unit (eigen_engine.hip) needs to know of the Winograd kernels: their geometry (wino_geom.h) and the launcher.
// The kernels themselves are compiled in translation units of their own (wino4_kernels.hip: the wide blocks; wino4t_kernels.hip: the tall ones; wino4h_kernels.hip: the half blocks; wino4p_kernels.hip: half blocks of packed tiles), so that
// the hipcc runs of a build go side by side (__graft_entry__.build()).
#pragma once
#include <hip/hip_runtime.h>
#include "conv_mfma.h"   // ConvArgs, EPI_*
#include "wino_geom.h"   // W4_WAVES, W4_KC, ..., the block shapes W4_WIDE / W4_TALL / W4_HALF / W4_PACK

namespace eig {

// grid blocks of wino4_kernel<NI, epi, shape> on stream st (NI = 3 or 4; epi = EPI_LSTM (NI = 4 only), EPI_CONVA, EPI_CONVP; shape: wino_geom.h); the first launch of an
// instantiation sets its dynamic-LDS attribute.
hipError_t launch_wino4(int NI, int epi, int shape, const ConvArgs& a, int grid, hipStream_t st);

}  // namespace eig
