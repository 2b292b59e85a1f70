// dense_stage.h -- the engine's view of the dense motion fitness's stage (eigen_dense_score).  flow_stage.hip
// defines the stage, over plain pointers; eigen_engine.hip owns the handle, the workspace and the entries.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/eigen_engine.h"

namespace eigd {

constexpr int DENSE_REC = 10;      // doubles of one sample's record (SCORE_REC, STRUCT_REC)
constexpr int DENSE_PART = 16 * 5; // doubles of one sample's reduction partials (SCORE_SLICES * SCORE_K, which covers the structures')

// The workspace of a handle, one batch each: planes [3][B H W] (Ix, Iy, It), u [B][2][H W], for Free theta, L [B][H W] and the member
// flags [B][H W]; the records [B][DENSE_REC] and the partials [B][DENSE_PART]
// pyr: the pyramid of the iterated solve (eigen_dense_solve), one block of pyr_doubles(max_batch, H, W) doubles made by the first call that
// needs it: per level l the gray planes I0_l, I1_l [B][H_l][W_l] and, for l >= 1, the level's field [B][2][H_l][W_l].
struct DenseWork {
    double *planes = nullptr, *u = nullptr, *theta = nullptr, *L = nullptr, *rec = nullptr, *part = nullptr, *pyr = nullptr;
    uint8_t* flag = nullptr;
    // the members' (eigen_dense_score_members), made by the first call that needs them and recorded in member_allocs, which the handle
    // frees.  Corner members: the gray plane, the eigenvalue plane, the candidate keys and the member plane [B][H W] each, the corners
    // [B][128][2] and their counts [B] (flow_stage.hip, corner_workspace).  The Free structure's list (dense_member_kernels.h): one block
    // of max_batch * list_cap slots of 12 bytes, theta then the index, and the counts [B]
    uint8_t *c_gray = nullptr, *c_member = nullptr;
    float *c_eig = nullptr, *c_corners = nullptr;
    unsigned long long* c_cand = nullptr;
    int *c_count = nullptr, *list_idx = nullptr, *list_count = nullptr;
    double* list_th = nullptr;
    long long list_cap = 0;
    // float frames (EIGEN_DENSE_FLOAT_FRAMES, dense_gray_workspace), in member_allocs too: the two gray planes [2][max_batch H W] of the single
    // step (the iterated solve keeps them as level 0 of pyr), and the byte copy [max_batch][C H W] of a float img0 for the corner members
    double* gray = nullptr;
    uint8_t* fbytes = nullptr;
    std::vector<void*> member_allocs;
};

constexpr int DENSE_MAX_LEVELS = 6, DENSE_MAX_ITERS = 32, DENSE_MIN_COARSE = 4;

// The solve of one call.  iterated: the launches of dense_pyr_kernels.h; false (levels = iters = 1): today's prepare and solve kernels.
struct DenseSolve {
    int levels = 1, iters = 1;
    bool iterated = false;
};

// The members of one call once checked (null members: given is false and the call is the namesake's)
struct DenseMembers {
    bool given = false, by_corners = false;
    int max_corners = 0, block_size = 0;
    double quality = 0.0, min_distance = 0.0;
    long long mask_bstride = 0;   // planes: sample b's plane is d_mask + b * mask_bstride
    int list_cap = 0;             // slots per sample of the Free structure's list: max_corners under corners, H W under planes
};

// doubles of the pyramid of B images of H x W at DENSE_MAX_LEVELS levels: four planes per pixel of a level
inline long long pyr_doubles(long long B, int H, int W)
{
    long long total = 0;
    for (int l = 0; l < DENSE_MAX_LEVELS; ++l, H = (H + 1) / 2, W = (W + 1) / 2) total += 4 * B * H * W;
    return total;
}

// The settings and the solve (null: one level, one iteration) against an H x W image, before anything is launched: the flow
// objective's own rules in its own words (eigen_last_error).  force_iterated: levels = iters = 1 goes through the iteration kernel too.
int dense_check(const eigen_dense_settings* s, const eigen_dense_solve* solve, bool force_iterated, int device, int H, int W, const uint8_t* d_mask, DenseSolve& out);

// The same with members (null: dense_check itself): the trainer's rules for them in its words (check_flow_members), every refusal ahead of
// any allocation; then the members' workspace on w, all of a group or none.  Under per-sample planes d_mask is not read as a shared plane.
int dense_check_members(const eigen_dense_settings* s, const eigen_dense_solve* solve, bool force_iterated, int device, int C, int H, int W, int max_batch,
                        const uint8_t* d_mask, const eigen_flow_members* members, int B, DenseWork& w, DenseSolve& out, DenseMembers& mem, int32_t allowed_flags = 0);

// The launches of the stage on checked settings: the records of the B samples into w.rec, the field into d_flow (null: w.u)
void dense_launch(const eigen_dense_settings* s, const DenseSolve& solve, int C, int H, int W, const uint8_t* img0, long long stride0, const uint8_t* img1,
                  long long stride1, int B, const uint8_t* d_mask, const DenseWork& w, double* d_flow, hipStream_t st, const DenseMembers& mem = DenseMembers());

// ---- float frames ("Float frames"): the stage from the float64 gray planes I0, I1 [B][H W] of its pair
// What a float call needs beyond the stage's workspace, made by the first call that needs it and freed with the handle: under the single step
// the two gray planes at max_batch, and for a float img0 under corner members its byte copy.  The iterated solve needs w.pyr, which the caller
// has made.
int dense_gray_workspace(int device, int H, int W, int max_batch, const DenseSolve& solve, bool float_img0, bool by_corners, int C, DenseWork& w);

// Where the two gray planes of a call of B samples lie: level 0 of the pyramid under the iterated solve (w.pyr, then w.pyr + B H W), else w.gray
void dense_gray_planes(const DenseWork& w, const DenseSolve& solve, int H, int W, int B, double*& I0, double*& I1);

// The gray plane of one batch of planar images (image b at img + b * stride, elements) into dst [B][H W]: one launch on st
void dense_gray_launch(const float* img, long long stride, int C, int H, int W, int B, double* dst, hipStream_t st);
void dense_gray_launch(const uint8_t* img, long long stride, int C, int H, int W, int B, double* dst, hipStream_t st);

// The bytes (uint8)(int)(v * 255.0f) of a float batch into w.fbytes, packed: the image the corner members are picked on
void dense_quant_launch(const float* img, long long stride, int C, int H, int W, int B, const DenseWork& w, hipStream_t st);

// dense_launch from ready gray planes at dense_gray_planes(w, solve, ...).  img0, stride0: the bytes of the first image of the pair, read
// under corner members only (else null).
void dense_launch_gray(const eigen_dense_settings* s, const DenseSolve& solve, int C, int H, int W, const uint8_t* img0, long long stride0, int B, const uint8_t* d_mask,
                       const DenseWork& w, double* d_flow, hipStream_t st, const DenseMembers& mem = DenseMembers());

}  // namespace eigd
