// dense_stage.h -- what eigen_engine.hip and prednet_train.hip share of the dense motion fitness (eigen_dense_score, DESIGN.md section
// 14).  The stage is the flow objective's, whose kernels and setting rules live in the trainer's translation unit: it is defined
// there, over plain pointers, and the engine owns the handle, the workspace and the entries.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/eigen_engine.h"

namespace eigd {

constexpr int DENSE_REC = 10;      // doubles of one sample's record (SCORE_REC, STRUCT_REC)
constexpr int DENSE_PART = 16 * 5; // doubles of one sample's reduction partials (SCORE_SLICES * SCORE_K, which covers the structures')

// The workspace of a handle, one batch each: planes [3][B H W] (Ix, Iy, It), u [B][2][H W], for Free theta, L [B][H W] and the member
// flags [B][H W]; the records [B][DENSE_REC] and the partials [B][DENSE_PART]
struct DenseWork {
    double *planes = nullptr, *u = nullptr, *theta = nullptr, *L = nullptr, *rec = nullptr, *part = nullptr;
    uint8_t* flag = nullptr;
};

// The settings against an H x W image, before anything is launched: the trainer's own rules in the trainer's own words (eigen_last_error).
int dense_check(const eigen_dense_settings* s, int device, int H, int W, const uint8_t* d_mask);

// The launches of the stage on checked settings: the records of the B samples into w.rec, the field into d_flow (null: w.u)
void dense_launch(const eigen_dense_settings* s, int C, int H, int W, const uint8_t* img0, long long stride0, const uint8_t* img1, long long stride1, int B,
                  const uint8_t* d_mask, const DenseWork& w, double* d_flow, hipStream_t st);

}  // namespace eigd
