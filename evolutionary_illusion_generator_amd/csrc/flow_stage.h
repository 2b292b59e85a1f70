// flow_stage.h -- the interface between the trainer's unit (prednet_train.hip) and the flow objective's (flow_stage.hip), host only.
// flow_stage.hip holds every flow and dense kernel header, the rules of a flow call, the stage of one term and the dense fitness's stage
// (dense_stage.h is the engine's view of that one); it works on a FlowWork and never sees the trainer's handle.  prednet_train.hip holds
// the handle, every eigen_trainer_* entry and the trainer's own kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdarg>
#include <cstdio>
#include <vector>

#include "../../include/eigen_engine.h"
#include "dense_stage.h"
#include "train_common.h"

int eig_set_error(int code, const char* msg);  // eigen_engine.hip: eigen_last_error's text

namespace eigf {

inline int tfail(int code, const char* fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return eig_set_error(code, buf);
}

#define TCHK(x)                                                                                                            \
    do {                                                                                                                   \
        hipError_t _e = (x);                                                                                               \
        if (_e != hipSuccess) return tfail(EIGEN_ERR_HIP, "%s:%d %s -> %s", __FILE__, __LINE__, #x, hipGetErrorString(_e)); \
    } while (0)

inline unsigned blocks(long long n) { return (unsigned)((n + eigt::EW_T - 1) / eigt::EW_T); }

// launch of an element-wise kernel over n elements
template <typename K, typename... A>
void ew(hipStream_t st, K kernel, long long n, A... a) { hipLaunchKernelGGL(kernel, dim3(blocks(n)), dim3(eigt::EW_T), 0, st, a...); }

// doubles per sample of a score's record (SCORE_REC, STRUCT_REC) and of the partials of the score mode's and the structure scores'
// reductions (SLICES * K), for the owner of the buffers; flow_stage.hip holds them against the kernel headers' constants
constexpr int FLOW_REC = 10, SCORE_PART = 16 * 5, STRUCT_PART = 16 * 3;

// What the flow stage works on: the image it sees and its buffers, one batch each unless said otherwise.  The owner (the trainer's handle)
// fills the image and the up-front buffers; the three lazy workspaces (corners, stats, the iterated block) are made here by the first
// call that needs them and recorded in the owner's list, which frees them.
struct FlowWork {
    int device = 0, C = 0, H = 0, W = 0, max_batch = 0, max_steps = 0;  // C, H, W: the image layer's
    long long HW = 0;
    long long CHW() const { return C * HW; }
    std::vector<void*>* allocs = nullptr;  // the owner's list of what it frees
    // the flow objective's float64 planes: Ix, Iy, It [3][B H W]; q [2][B H W]; the masked value [B H W]
    double *f_planes = nullptr, *f_q = nullptr, *f_mv = nullptr;
    // the moving reference's: the flow u [B][2][H W], which the solve writes there when that mode asks, and rx, ry, e [3][B H W]
    double *f_u = nullptr, *f_r = nullptr;
    // the score mode's: one record per sample [B][SCORE_REC] and the partials of its reductions [B][SCORE_SLICES][SCORE_K]
    double *f_rec = nullptr, *f_spart = nullptr;
    // the structure scores' (flow_struct_kernels.h): g [B][2][H W], the record [B][STRUCT_REC] and the partials [B][STRUCT_SLICES][STRUCT_K];
    // for Free theta and L [B][H W] each, rowS and colS [B][H W] each, and the member flags [B][H W]
    double *f_g = nullptr, *f_srec = nullptr, *f_sspart = nullptr, *f_theta = nullptr, *f_L = nullptr;
    int *f_rowS = nullptr, *f_colS = nullptr;
    uint8_t* f_flag = nullptr;
    // the corner members' (flow_corner_kernels.h), made by the first call that needs them (corner_workspace): the reference as bytes
    // [B][C H W], its gray plane [B][H W], the eigenvalue plane and the candidate keys [B][H W] each, the corners [B][CORNER_MAX][2],
    // their counts [B] and the member plane [B][H W]
    uint8_t *c_bytes = nullptr, *c_gray = nullptr, *c_member = nullptr;
    float *c_eig = nullptr, *c_corners = nullptr;
    unsigned long long* c_cand = nullptr;
    int* c_count = nullptr;
    bool c_byte_refs = false;   // every reference of this record is bytes (the dense fitness): corner_workspace makes no c_bytes
    double* f_vr = nullptr;     // the validity planes' (flow_valid_kernels.h): r_b of the current term [B]
    double* f_stats = nullptr;  // the records of a training call's terms [max_steps][max_batch][SCORE_REC], made by the first call that asks for them
    // the iterated solve's (flow_iter_kernels.h): one block that holds the pyramid, the tape and the adjoint planes of it_levels levels at
    // it_iters iterations, made by the first iterated call (iter_workspace); it_force: a {1, 1} solve takes that path too
    double* it_ws = nullptr;
    long long it_doubles = 0;
    int it_levels = 0, it_iters = 0;
    bool it_force = false;
};

// The flow objective's settings once checked: the window, the direction field and the mask (device, may be null) and the mask's count
struct FlowSpec {
    int r = 0;
    double eps = 0.0;
    const float* dir = nullptr;
    const uint8_t* mask = nullptr;
    long long mask_bstride = 0;  // the mask byte of sample b, pixel p is mask[b * mask_bstride + p]; 0: one plane shared by the batch
    long long n_mask = 0;
    bool moving = false;  // EIGEN_FLOW_MOVING_REFERENCE: a training call adds every term's reference path to the frame gradient
    bool pair_pred = false;  // EIGEN_FLOW_PAIR_PREDICTION: the reference of term s is the float P0_{s-1}, in the graph
    bool by_score = false;   // the score mode (flow_score_kernels.h): the value and q come from `score`, kappa loses the mask's count
    eigt::TFlowScore score = {};
    bool by_struct = false;  // a structure score (flow_struct_kernels.h): the value and q come from `sscore`, kappa as in the score mode
    eigt::TFlowStruct sscore = {};
    // EIGEN_FLOW_MEMBERS_CORNERS: every term's members are the corners of its own reference, under the shared `mask`
    bool by_corners = false;
    // eigen_dense_solve: the stage solves over `levels` pyramid levels with `iters` iterations each and differentiates that solve
    bool iterated = false;
    int levels = 1, iters = 1;
    int max_corners = 0, block_size = 0;
    double quality = 0.0, min_distance = 0.0;
    // the target field of the third displacement mode (flow_target_kernels.h; null: none), doubles: sample b of term s at
    // + b * bstride + s * tstride as [2][H W]
    struct Target { const double* p = nullptr; long long bstride = 0, tstride = 0; } target;
    // the validity planes under a target (flow_valid_kernels.h; null: none), bytes: sample b of term s at + b * bstride + s * tstride as [H W]
    struct Valid { const uint8_t* p = nullptr; long long bstride = 0, tstride = 0; } valid;
    // what divides a term's scale in kappa: B N_m, or B in the score mode, whose value is a mean over the samples alone
    double kappa_div(int B) const { return by_score || by_struct ? (double)B : (double)(B * n_mask); }
    // the solve as dense_solve_check found it
    void set_solve(const eigd::DenseSolve& s) { iterated = s.iterated; levels = s.levels; iters = s.iters; }
};

// One term for the flow stage and what is wanted of it; every target may be null.  Sample b of an image is at its pointer + b * its stride.
struct FlowTerm {
    const float* pred = nullptr; long long p_bstride = 0;
    const uint8_t* ref = nullptr; const float* fref = nullptr; long long r_bstride = 0;  // the reference as bytes, or as floats (flow_pair_kernels.h): exactly one
    double kappa = 0.0;                                                   // the scale of the seed and of the reference gradient
    double *part = nullptr, *d_value = nullptr;                           // the value into d_value, through the STEP_LOSS_BLOCKS partials at part
    double* d_flow = nullptr;                                             // the flow u [B][2][H W]
    float* d_seed = nullptr; long long s_bstride = 0; int s_accumulate = 0;   // kappa d value / d pred, added in float or stored
    float* d_refg = nullptr; long long rg_bstride = 0; int rg_accumulate = 0; // kappa d value / d reference (flow_ref_kernels.h), likewise
    const double* target = nullptr;                                           // this term's target field (null: none), sample b at + b * FlowSpec's target.bstride
    const uint8_t* valid = nullptr;                                           // this term's validity planes (null: none), sample b at + b * FlowSpec's valid.bstride
};

// ---- the rules of a flow call, before anything is launched; each states its own above its definition (flow_stage.hip)
int check_flow_on(int device, long long HW, const eigen_flow_settings* flow, const float* d_dir, const uint8_t* d_mask, int32_t allowed_flags, FlowSpec& f);
int check_flow_score(const eigen_flow_score* sc, const float* d_dir, FlowSpec& f);
int check_flow_struct(const eigen_flow_structure_score* sc, const float* d_dir, FlowSpec& f);
bool per_sample_mask(const eigen_flow_members* mem);
int check_flow_members(FlowWork& w, const eigen_flow_members* mem, const uint8_t* d_mask, int B, FlowSpec& f);
int check_flow_target(const FlowWork& w, const double* d_target, long long t_bstride, long long t_tstride, int n_terms, bool by_flow, const float* d_dir,
                      const void* score, const void* sscore, const void* members, FlowSpec& f);
int check_flow_valid(const FlowWork& w, const uint8_t* d_valid, long long v_bstride, long long v_tstride, int n_terms, FlowSpec& f);

// ---- the lazy workspaces a training call asks for, and the stage
int stats_workspace(FlowWork& w);
int iter_workspace(FlowWork& w, int levels, int iters);
void flow_stage(FlowWork& w, hipStream_t st, int B, const FlowSpec& f, const FlowTerm& m);
void flow_ref_path(FlowWork& w, hipStream_t st, int B, const FlowSpec& f, double kappa, const double* d_flow, float* d_refg, long long rg_bstride, int rg_accumulate);
void iter_store(FlowWork& w, hipStream_t st, int B, const FlowSpec& f, bool by_ref, double kappa, float* out, long long bstride, int accumulate);

// The one trainer kernel the stage launches (tloss_step_final_kernel, prednet_train.hip defines this): a displacement term's value into
// d_value, the STEP_LOSS_BLOCKS partials at part added in order, over numel
void flow_value_final(hipStream_t st, const double* part, double numel, double* d_value);

// Everything a stage-alone call takes: the arguments of the widest exported entry, eigen_trainer_flow_term_valid.  An entry lists the
// leading members, which every entry has, names the others it takes, and leaves the rest at these defaults, which are what it implies.
struct FlowTermCall {
    const float* d_pred; int64_t p_bstride, r_bstride; int32_t batch; const eigen_flow_settings* flow; const uint8_t* d_mask; double scale; double* h_value;
    double* d_flow; float* d_seed; int64_t s_bstride; void* stream;
    const uint8_t* d_ref = nullptr;  // the reference as bytes, or
    const float* d_fref = nullptr;   // as floats
    const float* d_dir = nullptr;
    float* d_refg = nullptr; int64_t rg_bstride = 0;
    const eigen_flow_score* score = nullptr;
    const eigen_flow_structure_score* sscore = nullptr;
    const eigen_flow_members* members = nullptr;
    double* h_stats = nullptr;
    const eigen_dense_solve* solve = nullptr;
    const double* d_target = nullptr; int64_t t_bstride = 0;
    const uint8_t* d_valid = nullptr; int64_t v_bstride = 0;
};

// The stage-alone call behind every eigen_trainer_flow_term* entry: the checks in the order of the function, one FlowTerm whose seed and
// reference gradient are stored, not added, and the value and the records read back.  part, d_value: the owner's STEP_LOSS_BLOCKS
// partials and the double the value goes through.
int flow_term_call(FlowWork& w, const FlowTermCall& c, double* part, double* d_value);

// eigen_trainer_flow_members once its own arguments are checked: the members' rules, the corner stage and the read-backs
int flow_members_call(FlowWork& w, const uint8_t* d_ref, const float* d_fref, int64_t r_bstride, int32_t batch, const eigen_flow_members* members, const uint8_t* d_mask,
                      uint8_t* h_members, int32_t* h_counts, void* stream);

}  // namespace eigf

namespace eigd {

// The solve's own rules: 1 .. 6 levels, 1 .. 32 iterations, a coarsest level of at least 4 pixels on its shorter side
int dense_solve_check(const eigen_dense_solve* solve, bool force_iterated, int H, int W, DenseSolve& out);

}  // namespace eigd
