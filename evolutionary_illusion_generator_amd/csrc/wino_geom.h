// wino_geom.h -- host-only constants of the Winograd F(4x4, 3x3) kernels (conv_wino4.h): block geometry and the packed-weight layout.  No HIP header:
// the weight packer (weight_pack.h) and the planner (conv_plan.h) read them as well as the kernels (through wino_launch.h).
#pragma once

namespace eig {

// F(4x4, 3x3), conv_wino4.h: twelve waves per block
constexpr int W4_WAVES = 12;
constexpr int W4_THREADS = 64 * W4_WAVES;
constexpr int W4_KC = 4;
constexpr int W4_NPOS = 36;
constexpr int wino4_u_floats(int NI) { return W4_NPOS * 4 * 16 * NI; }   // one 4-channel K-block of the packed weights: [36 pos][4 ch][16 cols][NI] (the buffer ends in one K-block of padding: the fetch runs one K-block past the end)

// block shapes of wino4_kernel: W4_WIDE 16 x 32-pixel blocks, W4_TALL 32 x 16, W4_HALF 8 x 32 (one region; six waves, twelve for 64-column ConvLSTMs / ConvPs),
// W4_PACK half blocks of packed tiles for 16- / 20-column maps (ConvLSTM / ConvP only)
enum { W4_WIDE = 0, W4_TALL = 1, W4_HALF = 2, W4_PACK = 3 };

}  // namespace eig
