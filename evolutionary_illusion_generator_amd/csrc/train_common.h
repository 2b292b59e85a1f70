// train_common.h -- what the kernel headers of training (train_kernels.h) and of the flow objective (flow_*_kernels.h, dense_*_kernels.h)
// share with each other and with the two host units behind them, prednet_train.hip and flow_stage.hip.  It holds no kernel: a header that
// defines a __global__ goes into exactly one translation unit (every non-template eigt:: kernel is a strong symbol on the host side), this
// one goes into all of them.
#pragma once

namespace eigt {

constexpr int WAVE = 64;
constexpr int EW_T = 256;             // threads per block of the element-wise kernels
constexpr int STEP_LOSS_BLOCKS = 64;  // blocks of one step's loss reduction, and of the sum that finishes a displacement term's value

// eigen_flow_score once checked (flow_score_kernels.h takes it by value)
struct TFlowScore {
    double max_norm, min_norm, r_min, r_max, w_direction, w_strength;
    int min_count;
};

// eigen_flow_structure_score once checked (flow_struct_kernels.h); DD = max_distance max_distance, middle = (int)(lim_hi / 2)
struct TFlowStruct {
    double max_norm, min_norm, lim_lo, lim_hi, DD, w0, w1, w2;
    int structure, min_count, middle;
};

}  // namespace eigt
