// flow_stage.hip -- the flow objective's stage and the dense fitness's (flow_stage.h, dense_stage.h; DESIGN.md sections 13 and 14): the
// rules of a flow call, the launches of one term over a FlowWork, the stage-alone call behind the eigen_trainer_flow_term* entries, and
// the dense fitness's stage over the engine's plain pointers.  All compute is in the kernels of flow_obj_kernels.h, flow_ref_kernels.h,
// flow_pair_kernels.h, flow_score_kernels.h, flow_struct_kernels.h, flow_corner_kernels.h, flow_iter_kernels.h (the iterated solve and
// its gradient), flow_target_kernels.h, flow_valid_kernels.h, dense_fitness_kernels.h, dense_member_kernels.h and dense_pyr_kernels.h, which
// this unit alone includes.  It knows no trainer: prednet_train.hip owns the handle and the entries.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "flow_stage.h"
#include "flow_obj_kernels.h"
#include "flow_ref_kernels.h"
#include "flow_pair_kernels.h"
#include "flow_score_kernels.h"
#include "flow_struct_kernels.h"
#include "flow_corner_kernels.h"
#include "dense_fitness_kernels.h"
#include "dense_member_kernels.h"
#include "dense_pyr_kernels.h"
#include "dense_float_kernels.h"
#include "flow_iter_kernels.h"
#include "flow_target_kernels.h"
#include "flow_valid_kernels.h"

using namespace eigt;

namespace eigf {

static_assert(FLOW_REC == SCORE_REC && FLOW_REC == STRUCT_REC, "one record size for every score");
static_assert(SCORE_PART == SCORE_SLICES * SCORE_K && STRUCT_PART == STRUCT_SLICES * STRUCT_K, "the partials as their owner allocates them");

// the grid of a tiled kernel over B images of H x W
static dim3 flow_grid(int H, int W, int B) { return dim3((unsigned)((W + FLOW_TILE - 1) / FLOW_TILE), (unsigned)((H + FLOW_TILE - 1) / FLOW_TILE), (unsigned)B); }

// A structure score's settings, before anything is launched; a direction field does not go with them.  Every structure's rules cover
// the fields it reads: the limits are Bands', max_distance and the weights are Free's.
int check_flow_struct(const eigen_flow_structure_score* sc, const float* d_dir, FlowSpec& f)
{
    if (!sc) return EIGEN_OK;
    if (sc->structure == 1 || sc->structure == 3)
        return tfail(EIGEN_ERR_INVALID, "flow structure score: structure %d (Circles, CirclesFree) is the score mode's, eigen_flow_score", sc->structure);
    if (sc->structure != STRUCT_BANDS && sc->structure != STRUCT_FREE) return tfail(EIGEN_ERR_INVALID, "flow structure score: unknown structure %d", sc->structure);
    if (d_dir) return tfail(EIGEN_ERR_INVALID, "a flow structure score takes no direction field");
    if (!std::isfinite(sc->max_norm) || !(sc->max_norm > 0.0)) return tfail(EIGEN_ERR_INVALID, "flow structure score max_norm %g: must be finite and > 0", sc->max_norm);
    if (!(sc->min_norm >= 0.0) || !(sc->min_norm < sc->max_norm))
        return tfail(EIGEN_ERR_INVALID, "flow structure score min_norm %g: must be in [0, max_norm = %g)", sc->min_norm, sc->max_norm);
    if (sc->min_count < 1) return tfail(EIGEN_ERR_INVALID, "flow structure score min_count %d: must be >= 1", sc->min_count);
    TFlowStruct s = {};
    s.structure = sc->structure; s.min_count = sc->min_count; s.max_norm = sc->max_norm; s.min_norm = sc->min_norm;
    if (sc->structure == STRUCT_BANDS) {
        // |lim_hi| <= 2e9: middle = (int)(lim_hi / 2) must be representable
        if (!std::isfinite(sc->lim_lo) || !std::isfinite(sc->lim_hi) || !(sc->lim_hi >= sc->lim_lo) || std::fabs(sc->lim_hi) > 2e9)
            return tfail(EIGEN_ERR_INVALID, "flow structure score limits %g .. %g: must be finite with lim_lo <= lim_hi and |lim_hi| <= 2e9", sc->lim_lo, sc->lim_hi);
        s.lim_lo = sc->lim_lo; s.lim_hi = sc->lim_hi; s.middle = (int)(sc->lim_hi / 2.0);
    } else {
        if (!std::isfinite(sc->max_distance) || !(sc->max_distance > 0.0))
            return tfail(EIGEN_ERR_INVALID, "flow structure score max_distance %g: must be finite and > 0", sc->max_distance);
        double sum = 0.0;
        for (double w : sc->w) {
            if (!std::isfinite(w) || !(w >= 0.0)) return tfail(EIGEN_ERR_INVALID, "flow structure score weight %g: weights must be finite and >= 0", w);
            sum += w;
        }
        if (!(sum > 0.0)) return tfail(EIGEN_ERR_INVALID, "all flow structure score weights are zero");
        s.DD = sc->max_distance * sc->max_distance;
        if (!std::isfinite(s.DD) || !(s.DD > 0.0)) return tfail(EIGEN_ERR_INVALID, "flow structure score max_distance %g: its square must be finite and > 0", sc->max_distance);
        s.w0 = sc->w[0]; s.w1 = sc->w[1]; s.w2 = sc->w[2];
    }
    f.by_struct = true;
    f.sscore = s;
    return EIGEN_OK;
}

// The score mode's settings, before anything is launched; a direction field does not go with them.
int check_flow_score(const eigen_flow_score* sc, const float* d_dir, FlowSpec& f)
{
    if (!sc) return EIGEN_OK;
    if (d_dir) return tfail(EIGEN_ERR_INVALID, "a flow score takes no direction field");
    if (sc->reserved != 0) return tfail(EIGEN_ERR_INVALID, "flow score: reserved must be 0, got %d", sc->reserved);
    if (!std::isfinite(sc->max_norm) || !(sc->max_norm > 0.0)) return tfail(EIGEN_ERR_INVALID, "flow score max_norm %g: must be finite and > 0", sc->max_norm);
    if (!(sc->min_norm >= 0.0) || !(sc->min_norm < sc->max_norm)) return tfail(EIGEN_ERR_INVALID, "flow score min_norm %g: must be in [0, max_norm = %g)", sc->min_norm, sc->max_norm);
    if (!std::isfinite(sc->r_min) || !std::isfinite(sc->r_max) || !(sc->r_min >= 0.0) || !(sc->r_max >= sc->r_min))
        return tfail(EIGEN_ERR_INVALID, "flow score limits %g .. %g: must be finite with 0 <= r_min <= r_max", sc->r_min, sc->r_max);
    if (sc->min_count < 2) return tfail(EIGEN_ERR_INVALID, "flow score min_count %d: must be >= 2", sc->min_count);
    for (double w : {sc->w_direction, sc->w_strength})
        if (!std::isfinite(w) || !(w >= 0.0)) return tfail(EIGEN_ERR_INVALID, "flow score weight %g: weights must be finite and >= 0", w);
    if (!(sc->w_direction + sc->w_strength > 0.0)) return tfail(EIGEN_ERR_INVALID, "both flow score weights are zero");
    f.by_score = true;
    f.score = TFlowScore{sc->max_norm, sc->min_norm, sc->r_min, sc->r_max, sc->w_direction, sc->w_strength, sc->min_count};
    return EIGEN_OK;
}

// The settings of a flow call against an image of HW pixels on `device`, before anything is launched (a trainer's image layer, or the
// engine's image: eigen_dense_score has no trainer).  The direction field and the mask are read back to the host: every d must be
// finite, and kappa needs the mask's count.
int check_flow_on(int device, long long HW, const eigen_flow_settings* flow, const float* d_dir, const uint8_t* d_mask, int32_t allowed_flags, FlowSpec& f)
{
    if (!flow) return tfail(EIGEN_ERR_INVALID, "EIGEN_OBJ_FLOW needs its settings");
    if (flow->radius < 1 || flow->radius > FLOW_MAX_R) return tfail(EIGEN_ERR_INVALID, "flow radius %d outside 1 .. %d", flow->radius, FLOW_MAX_R);
    if (!std::isfinite(flow->eps) || !(flow->eps > 0.0)) return tfail(EIGEN_ERR_INVALID, "flow eps %g: must be finite and > 0", flow->eps);
    if (flow->flags & ~allowed_flags) return tfail(EIGEN_ERR_INVALID, "flow flags 0x%x: this entry takes 0x%x at most", (unsigned)flow->flags, (unsigned)allowed_flags);
    f.moving = (flow->flags & EIGEN_FLOW_MOVING_REFERENCE) != 0;
    f.r = flow->radius; f.eps = flow->eps; f.dir = d_dir; f.mask = d_mask; f.n_mask = HW;
    TCHK(hipSetDevice(device));
    if (d_dir) {
        std::vector<float> d(2 * HW);
        TCHK(hipMemcpy(d.data(), d_dir, 2 * HW * 4, hipMemcpyDeviceToHost));
        for (long long i = 0; i < 2 * HW; ++i) if (!std::isfinite(d[i])) return tfail(EIGEN_ERR_INVALID, "flow direction element %lld is not finite", i);
    }
    if (d_mask) {
        std::vector<uint8_t> m(HW);
        TCHK(hipMemcpy(m.data(), d_mask, HW, hipMemcpyDeviceToHost));
        f.n_mask = 0;
        for (long long i = 0; i < HW; ++i) f.n_mask += m[i] != 0;
        if (f.n_mask == 0) return tfail(EIGEN_ERR_INVALID, "the flow mask counts no pixel");
    }
    return EIGEN_OK;
}

// The corner members' workspace, made by the first call that needs it and freed with its owner; the tape and every other use of the
// handle keep the memory they had.  A record whose references are all bytes (the dense fitness's view) gets no byte copy of a float one.
static int corner_workspace(FlowWork& w)
{
    if (w.c_member) return EIGEN_OK;
    const long long B = w.max_batch, HW = w.HW;
    TCHK(hipSetDevice(w.device));
    std::vector<std::pair<void**, long long>> want = {{(void**)&w.c_gray, B * HW}, {(void**)&w.c_eig, B * HW * 4}, {(void**)&w.c_cand, B * HW * 8},
                                                      {(void**)&w.c_corners, B * CORNER_MAX * 2 * 4}, {(void**)&w.c_count, B * 4}, {(void**)&w.c_member, B * HW}};
    if (!w.c_byte_refs) want.push_back({(void**)&w.c_bytes, B * w.CHW()});
    // all or nothing: the record takes the buffers once every one of them exists, a failure frees what it made
    std::vector<void*> made;
    for (const auto& b : want) {
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, (size_t)b.second);
        if (e != hipSuccess) {
            for (void* q : made) (void)hipFree(q);
            return tfail(EIGEN_ERR_HIP, "hipMalloc(%lld): %s", b.second, hipGetErrorString(e));
        }
        made.push_back(p);
    }
    for (size_t i = 0; i < made.size(); ++i) {
        *want[i].first = made[i];
        w.allocs->push_back(made[i]);
    }
    return EIGEN_OK;
}

// The records of a training call's terms, [max_steps][max_batch][SCORE_REC] doubles on the device, made by the first call that asks for
// them (h_stats) and freed with their owner
int stats_workspace(FlowWork& w)
{
    if (w.f_stats) return EIGEN_OK;
    TCHK(hipSetDevice(w.device));
    void* p = nullptr;
    TCHK(hipMalloc(&p, (size_t)w.max_steps * w.max_batch * SCORE_REC * 8));
    w.f_stats = (double*)p;
    w.allocs->push_back(p);
    return EIGEN_OK;
}

// The members of a call, before anything is launched (eigen_flow_members): f.mask, its stride and the corner settings.  check_flow_on has
// seen d_mask only where it is the shared plane (per_sample_mask says when it is not).
bool per_sample_mask(const eigen_flow_members* mem) { return mem && mem->kind == EIGEN_FLOW_MEMBERS_MASK; }

int check_flow_members(FlowWork& w, const eigen_flow_members* mem, const uint8_t* d_mask, int B, FlowSpec& f)
{
    if (!mem) return EIGEN_OK;
    if (!f.by_score && !f.by_struct) return tfail(EIGEN_ERR_INVALID, "flow members need a score: the displacement modes divide by the shared mask's count");
    if (mem->kind != EIGEN_FLOW_MEMBERS_MASK && mem->kind != EIGEN_FLOW_MEMBERS_CORNERS) return tfail(EIGEN_ERR_INVALID, "flow members: unknown kind %d", mem->kind);
    if (mem->reserved != 0) return tfail(EIGEN_ERR_INVALID, "flow members: reserved must be 0, got %d", mem->reserved);
    const long long HW = w.HW;
    if (mem->kind == EIGEN_FLOW_MEMBERS_MASK) {
        if (!d_mask) return tfail(EIGEN_ERR_INVALID, "flow members: EIGEN_FLOW_MEMBERS_MASK needs d_mask, one plane per sample");
        if (mem->mask_bstride < HW) return tfail(EIGEN_ERR_INVALID, "flow members: mask_bstride %lld is smaller than one plane (%lld bytes)", (long long)mem->mask_bstride, HW);
        // one copy of the B planes; a score does not read the count (kappa divides by the batch), so the first counted pixel settles it
        std::vector<uint8_t> m((size_t)B * HW);
        TCHK(hipMemcpy2D(m.data(), HW, d_mask, mem->mask_bstride, HW, B, hipMemcpyDeviceToHost));
        if (std::find_if(m.begin(), m.end(), [](uint8_t v) { return v != 0; }) == m.end()) return tfail(EIGEN_ERR_INVALID, "the flow mask counts no pixel");
        f.mask = d_mask; f.mask_bstride = mem->mask_bstride;
        return EIGEN_OK;
    }
    if (mem->max_corners < 1 || mem->max_corners > CORNER_MAX) return tfail(EIGEN_ERR_INVALID, "flow members: max_corners %d outside 1 .. %d", mem->max_corners, CORNER_MAX);
    if (mem->block_size < 1 || mem->block_size > eig::EIG_MAXB) return tfail(EIGEN_ERR_INVALID, "flow members: block_size %d outside 1 .. %d", mem->block_size, eig::EIG_MAXB);
    if (!(mem->quality_level > 0.0) || !(mem->quality_level <= 1.0)) return tfail(EIGEN_ERR_INVALID, "flow members: quality_level %g: must be in (0, 1]", mem->quality_level);
    if (!std::isfinite(mem->min_distance) || !(mem->min_distance >= 0.0)) return tfail(EIGEN_ERR_INVALID, "flow members: min_distance %g: must be finite and >= 0", mem->min_distance);
    if (mem->mask_bstride != 0) return tfail(EIGEN_ERR_INVALID, "flow members: mask_bstride %lld: must be 0 with EIGEN_FLOW_MEMBERS_CORNERS (d_mask is the shared plane)", (long long)mem->mask_bstride);
    f.by_corners = true;
    f.max_corners = mem->max_corners; f.block_size = mem->block_size; f.quality = mem->quality_level; f.min_distance = mem->min_distance;
    return corner_workspace(w);
}

// The member planes of one reference into w.c_member, the corner counts into w.c_count (flow_corner_kernels.h): the fitness path's own
// launches of eigen_flow on the bytes the fitness would see.  f.mask is the shared plane, or null.
static void corner_stage(FlowWork& w, hipStream_t st, int B, const FlowSpec& f, const uint8_t* ref, const float* fref, long long r_bstride)
{
    const int H = w.H, W = w.W, HW = (int)w.HW;
    if (fref) {
        ew(st, tcorner_quant_kernel, B * w.CHW(), fref, r_bstride, w.CHW(), B * w.CHW(), w.c_bytes);
        ref = w.c_bytes; r_bstride = w.CHW();
    }
    hipLaunchKernelGGL(eig::gray_kernel, dim3((HW + 255) / 256, B), dim3(256), 0, st, ref, r_bstride, w.C, HW, w.c_gray, B);
    const double sc = 1.0 / ((double)(1 << 2) * f.block_size * 255.0);
    const float SC = (float)(sc * sc);
    hipLaunchKernelGGL(eig::mineig_kernel, dim3((W + eig::EIG_T - 1) / eig::EIG_T, (H + eig::EIG_T - 1) / eig::EIG_T, B), dim3(256), 0, st, (const uint8_t*)w.c_gray, H, W,
                       f.block_size, SC, w.c_eig);
    hipLaunchKernelGGL(eig::corner_select_kernel, dim3(B), dim3(1024), 0, st, (const float*)w.c_eig, H, W, f.quality, (float)f.min_distance, f.max_corners, w.c_cand,
                       w.c_corners, w.c_count);
    hipLaunchKernelGGL(tcorner_member_kernel, dim3(B), dim3(CORNER_T), 0, st, (const float*)w.c_corners, (const int*)w.c_count, f.max_corners, H, W, f.mask,
                       w.c_member);
}

// The gradient of the term by its reference, from the planes and q the flow stage of the same term left in the workspace and its flow
// at d_flow: into d_refg (sample b at + b * rg_bstride), added in float or stored.  A training call under the prediction pairing runs
// this apart from the stage, once layer 0's terr_bwd of the step has written dP0_{s-1}.
void flow_ref_path(FlowWork& w, hipStream_t st, int B, const FlowSpec& f, double kappa, const double* d_flow, float* d_refg, long long rg_bstride, int rg_accumulate)
{
    const long long n = (long long)B * w.HW;
    hipLaunchKernelGGL(tflow_ref_sums_kernel, flow_grid(w.H, w.W, B), dim3(FLOW_T), 0, st, (const double*)w.f_planes, (const double*)w.f_q, d_flow, n, w.H, w.W, f.r, kappa, w.f_r);
    ew(st, tflow_ref_fold_kernel, n, (const double*)w.f_r, n, w.H, w.W, w.C, d_refg, rg_bstride, rg_accumulate);
}

// A target field's rules, before anything is launched or allocated (null: none, and the strides are not read): it is a displacement mode
// of its own, so no direction, score or members go with it, and a sample's [2][H W] doubles must fit its strides.
int check_flow_target(const FlowWork& w, const double* d_target, long long t_bstride, long long t_tstride, int n_terms, bool by_flow, const float* d_dir,
                      const void* score, const void* sscore, const void* members, FlowSpec& f)
{
    if (!d_target) return EIGEN_OK;
    if (!by_flow) return tfail(EIGEN_ERR_INVALID, "a flow target goes with EIGEN_OBJ_FLOW only");
    if (d_dir || score || sscore || members) return tfail(EIGEN_ERR_INVALID, "a flow target takes no direction field, score or members");
    const long long field = 2 * w.HW;
    if (t_bstride < field) return tfail(EIGEN_ERR_INVALID, "t_bstride %lld is smaller than one field (%lld doubles)", t_bstride, field);
    if (n_terms > 1 && t_tstride < field) return tfail(EIGEN_ERR_INVALID, "t_tstride %lld is smaller than one field (%lld doubles)", t_tstride, field);
    f.target.p = d_target; f.target.bstride = t_bstride; f.target.tstride = t_tstride;
    return EIGEN_OK;
}

// The validity planes' rules, after check_flow_target and before anything is launched or allocated (null: none, and the strides are not
// read): they weigh a target's endpoint error, and a sample's [H W] bytes must fit their strides.
int check_flow_valid(const FlowWork& w, const uint8_t* d_valid, long long v_bstride, long long v_tstride, int n_terms, FlowSpec& f)
{
    if (!d_valid) return EIGEN_OK;
    if (!f.target.p) return tfail(EIGEN_ERR_INVALID, "validity planes go with a flow target only");
    const long long HW = w.HW;
    if (v_bstride < HW) return tfail(EIGEN_ERR_INVALID, "v_bstride %lld is smaller than one plane (%lld bytes)", v_bstride, HW);
    if (n_terms > 1 && v_tstride < HW) return tfail(EIGEN_ERR_INVALID, "v_tstride %lld is smaller than one plane (%lld bytes)", v_tstride, HW);
    f.valid.p = d_valid; f.valid.bstride = v_bstride; f.valid.tstride = v_tstride;
    return EIGEN_OK;
}

// The two passes of moments of a structure score over the field u, for Free the prepare and the pair pass between them: the samples'
// records into rec, the value into d_value (may be null).  This is the one statement of that launch list, over plain pointers.  rowS,
// colS: where the pair pass leaves what the gradient needs; null (the dense fitness, which takes no gradient) runs the pair kernel
// without them, or, where the call carries members (list non-null), the compacted pair pass of dense_member_kernels.h.
struct FreeList {
    int* idx; double* th; int* count; int cap;   // cap slots per sample
};

template <int STRUCT>
static void struct_passes(hipStream_t st, int H, int W, int B, const uint8_t* mask, long long mask_bstride, const TFlowStruct& s, const double* u, double* theta, uint8_t* flag,
                   double* L, int* rowS, int* colS, double* rec, double* part, double* d_value, const FreeList* list = nullptr)
{
    const long long HW = (long long)H * W, n = B * HW;
    const dim3 sgrid(STRUCT_SLICES, (unsigned)B), pgrid((unsigned)((HW + PAIR_T - 1) / PAIR_T), (unsigned)B);
    if (STRUCT == STRUCT_FREE) ew(st, tflow_free_prepare_kernel, n, u, n, H, W, mask, mask_bstride, s, theta, flag);
    hipLaunchKernelGGL((tflow_struct_moment_kernel<STRUCT, 1>), sgrid, dim3(EW_T), 0, st, u, H, W, mask, mask_bstride, s, (const double*)rec, (const double*)L, part);
    hipLaunchKernelGGL((tflow_struct_final_kernel<STRUCT, 1>), dim3(B), dim3(64), 0, st, (const double*)part, B, s, rec, (double*)nullptr);
    if (STRUCT == STRUCT_FREE && rowS)
        hipLaunchKernelGGL(tflow_free_pair_kernel, pgrid, dim3(PAIR_T), 0, st, (const double*)theta, (const uint8_t*)flag, H, W, s.DD, L, rowS, colS);
    else if (STRUCT == STRUCT_FREE && list) {
        hipLaunchKernelGGL(tdense_member_list_kernel, dim3(B), dim3(LIST_T), 0, st, (const double*)theta, (const uint8_t*)flag, (int)HW, list->cap, list->idx, list->th,
                           list->count, L);
        hipLaunchKernelGGL(tdense_free_pair_list_kernel, dim3((unsigned)((list->cap + PAIR_T - 1) / PAIR_T), (unsigned)B), dim3(PAIR_T), 0, st, (const int*)list->idx,
                           (const double*)list->th, (const int*)list->count, list->cap, (int)HW, W, s.DD, L);
    } else if (STRUCT == STRUCT_FREE)
        hipLaunchKernelGGL(tdense_free_pair_kernel, pgrid, dim3(PAIR_T), 0, st, (const double*)theta, (const uint8_t*)flag, H, W, s.DD, L);
    hipLaunchKernelGGL((tflow_struct_moment_kernel<STRUCT, 2>), sgrid, dim3(EW_T), 0, st, u, H, W, mask, mask_bstride, s, (const double*)rec, (const double*)L, part);
    hipLaunchKernelGGL((tflow_struct_final_kernel<STRUCT, 2>), dim3(B), dim3(64), 0, st, (const double*)part, B, s, rec, d_value);
}

// The value and q of a structure score from the u the solve just wrote (flow_struct_kernels.h): the passes, then (want_q) the gradient
// g and q over what the solve left in f_q.
// with_q false (the iterated solve, whose gradient takes g itself): g is left in f_g and q is not formed.
template <int STRUCT>
static void struct_stage_of(FlowWork& w, hipStream_t st, int B, const FlowSpec& f, const double* u, double* d_value, bool want_q, bool with_q)
{
    const long long n = (long long)B * w.HW;
    const TFlowStruct& s = f.sscore;
    struct_passes<STRUCT>(st, w.H, w.W, B, f.mask, f.mask_bstride, s, u, w.f_theta, w.f_flag, w.f_L, w.f_rowS, w.f_colS, w.f_srec, w.f_sspart, d_value);
    if (!want_q) return;
    ew(st, tflow_struct_grad_kernel<STRUCT>, n, u, n, w.H, w.W, f.mask, f.mask_bstride, s, (const double*)w.f_srec, (const int*)w.f_rowS, (const int*)w.f_colS, w.f_g);
    if (!with_q) return;
    hipLaunchKernelGGL(tflow_struct_q_kernel, flow_grid(w.H, w.W, B), dim3(FLOW_T), 0, st, (const double*)w.f_planes, (const double*)w.f_g, n, w.H, w.W, f.r, f.eps, w.f_q);
}

static void struct_stage(FlowWork& w, hipStream_t st, int B, const FlowSpec& f, const double* u, double* d_value, bool want_q, bool with_q = true)
{
    if (f.sscore.structure == STRUCT_BANDS) struct_stage_of<STRUCT_BANDS>(w, st, B, f, u, d_value, want_q, with_q);
    else struct_stage_of<STRUCT_FREE>(w, st, B, f, u, d_value, want_q, with_q);
}

// The value of the score mode from the u a solve wrote: two passes of moments into the samples' records at rec, the value into d_value
// (may be null).  The one statement of that launch list, over plain pointers.
static void score_passes(hipStream_t st, int H, int W, int B, const uint8_t* mask, long long mask_bstride, const TFlowScore& sc, const double* u, double* rec, double* part,
                  double* d_value)
{
    const dim3 sgrid(SCORE_SLICES, (unsigned)B);
    hipLaunchKernelGGL(tflow_score_moment_kernel<1>, sgrid, dim3(EW_T), 0, st, u, H, W, mask, mask_bstride, sc, (const double*)rec, part);
    hipLaunchKernelGGL(tflow_score_final_kernel<1>, dim3(B), dim3(64), 0, st, (const double*)part, B, sc, rec, (double*)nullptr);
    hipLaunchKernelGGL(tflow_score_moment_kernel<2>, sgrid, dim3(EW_T), 0, st, u, H, W, mask, mask_bstride, sc, (const double*)rec, part);
    hipLaunchKernelGGL(tflow_score_final_kernel<2>, dim3(B), dim3(64), 0, st, (const double*)part, B, sc, rec, d_value);
}

// the value of a displacement term from the masked values the solve left in f_mv: STEP_LOSS_BLOCKS partials, then the trainer's final kernel
static void displacement_value(FlowWork& w, hipStream_t st, int B, const FlowSpec& f, const FlowTerm& m)
{
    hipLaunchKernelGGL(tflow_sum_kernel, dim3(STEP_LOSS_BLOCKS), dim3(EW_T), 0, st, (const double*)w.f_mv, (long long)B * w.HW, m.part);
    flow_value_final(st, m.part, (double)(B * f.n_mask), m.d_value);
}

// ---- the iterated solve and its gradient (flow_iter_kernels.h, DESIGN.md section 13, "The iterated solve's gradient")
// One level's planes in the record's block, each over max_batch samples: the gray images, the Scharr pair, the tape and beta
// [iters][B][2][H W], the gradient arriving at the level's field, the level's field (levels >= 1; level 0's goes where the call wants it)
// and the gradients by the level's images
struct IterLevel {
    int H, W;
    double *I0, *I1, *gxy, *tape, *beta, *ubK, *u, *I0b, *I1b;
};

// and what the levels share, at level 0's size: ub_0 [B][2], (ab, bb, cb) [B][3], (Ixb, Iyb) [B][2], I0b's direct term [B], max |u| [B]
struct IterPlan {
    IterLevel lv[eigd::DENSE_MAX_LEVELS];
    double *ub0, *abc, *rxy, *dir, *umax;
    long long doubles;
};

// the block's layout for a solve of `levels` x `iters` (pointers relative to `at`, which may be null: the size alone)
static IterPlan iter_plan(const FlowWork& w, double* at, int levels, int iters)
{
    IterPlan pl;
    const long long Bm = w.max_batch;
    double* p = at;
    auto take = [&](long long n) { double* q = p; p += n; return q; };
    int h = w.H, ww = w.W;
    for (int l = 0; l < levels; ++l, h = (h + 1) / 2, ww = (ww + 1) / 2) {
        const long long n = Bm * h * ww;
        IterLevel& v = pl.lv[l];
        v.H = h; v.W = ww;
        v.I0 = take(n); v.I1 = take(n); v.gxy = take(2 * n); v.tape = take(2 * n * iters); v.beta = take(2 * n * iters);
        v.ubK = take(2 * n); v.u = take(2 * n); v.I0b = take(n); v.I1b = take(n);
    }
    const long long n0 = Bm * w.HW;
    pl.ub0 = take(2 * n0); pl.abc = take(3 * n0); pl.rxy = take(2 * n0); pl.dir = take(n0); pl.umax = take(Bm);
    pl.doubles = (long long)(p - at);
    return pl;
}

// The block, made by the first iterated call and freed with its owner: one allocation, so all of it or none.  A later call with more
// levels or iterations replaces it by one that holds both; a record that never asks holds none.
int iter_workspace(FlowWork& w, int levels, int iters)
{
    if (w.it_ws && levels <= w.it_levels && iters <= w.it_iters) return EIGEN_OK;
    const int L = std::max(levels, w.it_levels), K = std::max(iters, w.it_iters);
    const long long doubles = iter_plan(w, nullptr, L, K).doubles;
    TCHK(hipSetDevice(w.device));
    if (!w.it_ws) {
        // once per record, checked: the two tiled kernels may ask for the dynamic LDS of the largest radius (radius 11 and above is more than
        // a launch gets without the attribute)
        const int lds = pyr_lds_doubles(FLOW_MAX_R) * 8;
        TCHK(hipFuncSetAttribute((const void*)tfiter_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        TCHK(hipFuncSetAttribute((const void*)tfiter_adj_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    }
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, (size_t)doubles * 8);
    if (e != hipSuccess) return tfail(EIGEN_ERR_HIP, "hipMalloc(%lld): %s", doubles * 8, hipGetErrorString(e));
    if (w.it_ws) {
        TCHK(hipFree(w.it_ws));  // waits for whatever still reads it
        w.allocs->erase(std::find(w.allocs->begin(), w.allocs->end(), (void*)w.it_ws));
    }
    w.allocs->push_back(p);
    w.it_ws = (double*)p; w.it_doubles = doubles; w.it_levels = L; w.it_iters = K;
    return EIGEN_OK;
}

// The forward: the gray planes, the pyramid, then one launch per level from the coarsest to the finest; level 0's field goes into d_flow
static void iter_forward(FlowWork& w, hipStream_t st, int B, const FlowSpec& f, const float* pred, long long p_bstride, const uint8_t* ref, const float* fref,
                  long long r_bstride, double* d_flow)
{
    IterPlan pl = iter_plan(w, w.it_ws, f.levels, f.iters);
    IterLevel* lv = pl.lv;
    const long long n0 = (long long)B * w.HW;
    if (fref) ew(st, tfiter_gray_kernel<float>, n0, pred, p_bstride, fref, r_bstride, w.C, w.H, w.W, n0, lv[0].I0, lv[0].I1);
    else ew(st, tfiter_gray_kernel<uint8_t>, n0, pred, p_bstride, ref, r_bstride, w.C, w.H, w.W, n0, lv[0].I0, lv[0].I1);
    for (int l = 1; l < f.levels; ++l) {
        const long long n = (long long)B * lv[l].H * lv[l].W;
        ew(st, tdense_pyrdown_kernel, n, (const double*)lv[l - 1].I0, (const double*)lv[l - 1].I1, lv[l - 1].H, lv[l - 1].W, lv[l].H, lv[l].W, n, lv[l].I0, lv[l].I1);
    }
    const int lds = pyr_lds_doubles(f.r) * 8;  // iter_workspace has set the attribute that lets a launch ask for it
    for (int l = f.levels - 1; l >= 0; --l) {
        const bool top = l == f.levels - 1;
        hipLaunchKernelGGL(tfiter_fwd_kernel, flow_grid(lv[l].H, lv[l].W, B), dim3(FLOW_T), (size_t)lds, st, (const double*)lv[l].I0, (const double*)lv[l].I1, lv[l].H,
                           lv[l].W, f.r, f.eps, f.iters, top ? (const double*)nullptr : (const double*)lv[l + 1].u, top ? 0 : lv[l + 1].H, top ? 0 : lv[l + 1].W,
                           l ? lv[l].u : d_flow, lv[l].tape, lv[l].gxy);
    }
}

// The backward from g = d value / d u of level 0 [B][2][H W]: the levels from the finest to the coarsest, then the pyramid's adjoint from
// the coarsest to the finest.  Leaves the gradients by the gray images of level 0 in the plan's lv[0].I1b (prediction) and lv[0].I0b
// (reference), unscaled.
static void iter_backward(FlowWork& w, hipStream_t st, int B, const FlowSpec& f, const double* g)
{
    IterPlan pl = iter_plan(w, w.it_ws, f.levels, f.iters);
    IterLevel* lv = pl.lv;
    const int lds = pyr_lds_doubles(f.r) * 8;
    for (int l = 0; l < f.levels; ++l) {
        const IterLevel& v = lv[l];
        const long long HW = (long long)v.H * v.W, n = B * HW;
        const double* ubK = l ? (const double*)v.ubK : g;
        hipLaunchKernelGGL(tfiter_umax_kernel, dim3(B), dim3(EW_T), 0, st, (const double*)v.tape, f.iters, HW, pl.umax);
        hipLaunchKernelGGL(tfiter_adj_kernel, flow_grid(v.H, v.W, B), dim3(FLOW_T), (size_t)lds, st, (const double*)v.I0, (const double*)v.I1, v.H, v.W, f.r, f.eps, f.iters,
                           (const double*)v.tape, ubK, v.beta, pl.abc, pl.ub0);
        ew(st, tfiter_i1_kernel, n, (const double*)v.tape, (const double*)v.beta, (const double*)v.gxy, (const double*)pl.umax, B, v.H, v.W, f.r, f.iters, n, v.I1b);
        ew(st, tfiter_q_kernel, n, (const double*)v.I0, (const double*)v.I1, (const double*)v.tape, (const double*)v.beta, (const double*)pl.abc, (const double*)v.gxy, B,
           v.H, v.W, f.r, f.iters, n, pl.rxy, pl.dir);
        ew(st, tfiter_i0_kernel, n, (const double*)pl.rxy, (const double*)pl.dir, v.H, v.W, n, v.I0b);
        if (l < f.levels - 1) {
            const long long nc = (long long)B * lv[l + 1].H * lv[l + 1].W;
            ew(st, tfiter_down_kernel, nc, (const double*)pl.ub0, v.H, v.W, lv[l + 1].H, lv[l + 1].W, nc, lv[l + 1].ubK);
        }
    }
    for (int l = f.levels - 2; l >= 0; --l) {
        const long long n = (long long)B * lv[l].H * lv[l].W;
        ew(st, tfiter_pyr_adj_kernel, n, (const double*)lv[l + 1].I0b, (const double*)lv[l + 1].I1b, lv[l].H, lv[l].W, lv[l + 1].H, lv[l + 1].W, n, lv[l].I0b, lv[l].I1b);
    }
}

// kappa times the gradient by the prediction (by_ref false) or by the reference (true) the last iter_backward left, as floats: stored or
// added at out (sample b at + b * bstride).  A training call under the prediction pairing adds the reference's apart from the stage, where
// the single step runs flow_ref_path.
void iter_store(FlowWork& w, hipStream_t st, int B, const FlowSpec& f, bool by_ref, double kappa, float* out, long long bstride, int accumulate)
{
    const IterPlan pl = iter_plan(w, w.it_ws, f.levels, f.iters);
    const long long n = (long long)B * w.HW;
    ew(st, tfiter_store_kernel, n, (const double*)(by_ref ? pl.lv[0].I0b : pl.lv[0].I1b), kappa, w.C, w.HW, n, out, bstride, accumulate);
}

// mv and g of the target mode from the field u, for either solve: tflow_target_kernel, or under the term's validity planes the samples'
// counts and tflow_target_valid_kernel (flow_valid_kernels.h)
static void target_value(FlowWork& w, hipStream_t st, int B, const FlowSpec& f, const FlowTerm& m, const double* u)
{
    const long long n = (long long)B * w.HW;
    if (!m.valid) {
        ew(st, tflow_target_kernel, n, u, m.target, f.target.bstride, f.mask, f.mask_bstride, w.HW, n, w.f_mv, w.f_g);
        return;
    }
    hipLaunchKernelGGL(tflow_valid_count_kernel, dim3(B), dim3(EW_T), 0, st, m.valid, f.valid.bstride, f.mask, f.mask_bstride, w.HW, f.n_mask, w.f_vr);
    ew(st, tflow_target_valid_kernel, n, u, m.target, f.target.bstride, f.mask, f.mask_bstride, m.valid, f.valid.bstride, (const double*)w.f_vr, w.HW, n, w.f_mv, w.f_g);
}

// The flow stage of one term under an iterated solve: the field of level 0 from iter_forward, the unchanged value / score kernels on it,
// which leave g = d value / d u (masked) in f_g, then iter_backward and the level-0 stores.  The field goes to the record's workspace
// unless the caller wants it.
static void iter_flow_stage(FlowWork& w, hipStream_t st, int B, const FlowSpec& f, const FlowTerm& m)
{
    const long long n = (long long)B * w.HW;
    double* u = m.d_flow ? m.d_flow : w.f_u;
    iter_forward(w, st, B, f, m.pred, m.p_bstride, m.ref, m.fref, m.r_bstride, u);
    const bool grads = m.d_seed || m.d_refg;
    if (f.by_score) {
        score_passes(st, w.H, w.W, B, f.mask, f.mask_bstride, f.score, u, w.f_rec, w.f_spart, m.d_value);
        if (grads) ew(st, tfiter_score_g_kernel, n, (const double*)u, w.H, w.W, n, f.mask, f.mask_bstride, f.score, (const double*)w.f_rec, w.f_g);
    } else if (f.by_struct) {
        struct_stage(w, st, B, f, u, m.d_value, grads, false);
    } else {
        if (m.target) target_value(w, st, B, f, m, u);
        else ew(st, tfiter_value_kernel, n, (const double*)u, f.dir, f.mask, f.mask_bstride, w.HW, n, w.f_mv, w.f_g);
        if (m.d_value) displacement_value(w, st, B, f, m);
    }
    if (!grads) return;
    iter_backward(w, st, B, f, w.f_g);
    if (m.d_seed) iter_store(w, st, B, f, false, m.kappa, m.d_seed, m.s_bstride, m.s_accumulate);
    if (m.d_refg) iter_store(w, st, B, f, true, m.kappa, m.d_refg, m.rg_bstride, m.rg_accumulate);
}

// The flow stage of one term (eigen_trainer_flow_term states the arithmetic): the planes, the tiled solve, then what is wanted of the
// value, the flow and the seed.  A reference gradient is formed from the planes, q and u this stage leaves: u is then written to the
// record's workspace unless the caller wants it anyway.
void flow_stage(FlowWork& w, hipStream_t st, int B, const FlowSpec& f, const FlowTerm& m)
{
    if (f.by_corners) {
        // the term's members from its own reference, then the stage under them as a per-sample mask
        corner_stage(w, st, B, f, m.ref, m.fref, m.r_bstride);
        FlowSpec g = f;
        g.by_corners = false; g.mask = w.c_member; g.mask_bstride = w.HW;
        return flow_stage(w, st, B, g, m);
    }
    if (f.iterated) return iter_flow_stage(w, st, B, f, m);
    double* d_flow = (m.d_refg || f.by_score || f.by_struct || m.target) && !m.d_flow ? w.f_u : m.d_flow;
    const long long n = (long long)B * w.HW;
    if (m.fref) ew(st, tflow_pair_prep_kernel, n, m.pred, m.p_bstride, m.fref, m.r_bstride, w.C, w.H, w.W, n, w.f_planes);
    else ew(st, tflow_prep_kernel, n, m.pred, m.p_bstride, m.ref, m.r_bstride, w.C, w.H, w.W, n, w.f_planes);
    const dim3 grid = flow_grid(w.H, w.W, B);
    hipLaunchKernelGGL(tflow_solve_kernel, grid, dim3(FLOW_T), 0, st, (const double*)w.f_planes, n, w.H, w.W, f.r, f.eps, f.dir, f.mask, f.mask_bstride, w.f_q, w.f_mv, d_flow);
    if (f.by_score) {
        // the value and q of the score mode, from the u the solve just wrote: two passes of moments, then q over what the solve left in f_q
        const double* u = d_flow;
        score_passes(st, w.H, w.W, B, f.mask, f.mask_bstride, f.score, u, w.f_rec, w.f_spart, m.d_value);
        if (m.d_seed || m.d_refg)
            hipLaunchKernelGGL(tflow_score_q_kernel, grid, dim3(FLOW_T), 0, st, (const double*)w.f_planes, u, n, w.H, w.W, f.r, f.eps, f.mask, f.mask_bstride, f.score,
                               (const double*)w.f_rec, w.f_q);
    } else if (f.by_struct) {
        struct_stage(w, st, B, f, d_flow, m.d_value, m.d_seed || m.d_refg);
    } else if (m.target) {
        // the target mode: mv and g from the u the solve just wrote, then q from g over the solve's own a, b, c and det
        target_value(w, st, B, f, m, d_flow);
        if (m.d_seed || m.d_refg)
            hipLaunchKernelGGL(tflow_struct_q_kernel, grid, dim3(FLOW_T), 0, st, (const double*)w.f_planes, (const double*)w.f_g, n, w.H, w.W, f.r, f.eps, w.f_q);
    }
    if (!f.by_score && !f.by_struct && m.d_value) displacement_value(w, st, B, f, m);
    if (m.d_seed)
        hipLaunchKernelGGL(tflow_seed_kernel, grid, dim3(FLOW_T), 0, st, (const double*)w.f_planes, (const double*)w.f_q, n, w.H, w.W, w.C, f.r, m.kappa, m.d_seed,
                           m.s_bstride, m.s_accumulate);
    if (m.d_refg) flow_ref_path(w, st, B, f, m.kappa, d_flow, m.d_refg, m.rg_bstride, m.rg_accumulate);
}

int flow_term_call(FlowWork& w, const FlowTermCall& c, double* part, double* d_value)
{
    if (!c.d_pred || (!c.d_ref && !c.d_fref) || !c.flow) return tfail(EIGEN_ERR_INVALID, "null argument");
    if (c.batch < 1) return tfail(EIGEN_ERR_INVALID, "batch >= 1 required");
    if (c.batch > w.max_batch) return tfail(EIGEN_ERR_CAPACITY, "batch %d exceeds the trainer's %d", c.batch, w.max_batch);
    const long long C0HW = w.CHW();
    if (c.p_bstride < C0HW || c.r_bstride < C0HW || (c.d_seed && c.s_bstride < C0HW) || (c.d_refg && c.rg_bstride < C0HW))
        return tfail(EIGEN_ERR_INVALID, "a batch stride is smaller than one image (%lld elements)", C0HW);
    if (!std::isfinite(c.scale)) return tfail(EIGEN_ERR_INVALID, "scale %g is not finite", c.scale);
    FlowSpec f;
    int rc = check_flow_target(w, c.d_target, c.t_bstride, 0, 1, true, c.d_dir, c.score, c.sscore, c.members, f);
    if (rc) return rc;
    rc = check_flow_valid(w, c.d_valid, c.v_bstride, 0, 1, f);
    if (rc) return rc;
    eigd::DenseSolve solve;
    rc = eigd::dense_solve_check(c.solve, w.it_force, w.H, w.W, solve);  // ahead of the mask's read-back and of every allocation
    if (rc) return rc;
    f.set_solve(solve);
    rc = check_flow_on(w.device, w.HW, c.flow, c.d_dir, per_sample_mask(c.members) ? nullptr : c.d_mask, 0, f);
    if (rc) return rc;
    rc = check_flow_score(c.score, c.d_dir, f);
    if (rc) return rc;
    rc = check_flow_struct(c.sscore, c.d_dir, f);
    if (rc) return rc;
    rc = check_flow_members(w, c.members, c.d_mask, c.batch, f);
    if (rc) return rc;
    if (f.iterated) {
        rc = iter_workspace(w, f.levels, f.iters);
        if (rc) return rc;
    }
    hipStream_t st = (hipStream_t)c.stream;
    FlowTerm m;
    m.pred = c.d_pred; m.p_bstride = c.p_bstride; m.ref = c.d_ref; m.fref = c.d_fref; m.r_bstride = c.r_bstride;
    m.kappa = c.scale / f.kappa_div(c.batch); m.part = part; m.d_value = c.h_value ? d_value : nullptr;
    m.d_flow = c.d_flow; m.d_seed = c.d_seed; m.s_bstride = c.s_bstride; m.d_refg = c.d_refg; m.rg_bstride = c.rg_bstride;
    m.target = f.target.p; m.valid = f.valid.p;
    flow_stage(w, st, c.batch, f, m);
    TCHK(hipGetLastError());
    if (c.h_value) {
        TCHK(hipMemcpyAsync(c.h_value, d_value, 8, hipMemcpyDeviceToHost, st));
        TCHK(hipStreamSynchronize(st));
    }
    if (c.h_stats && f.by_score) {
        TCHK(hipMemcpyAsync(c.h_stats, w.f_rec, (size_t)c.batch * SCORE_REC * 8, hipMemcpyDeviceToHost, st));
        TCHK(hipStreamSynchronize(st));
    }
    if (c.h_stats && f.by_struct) {
        TCHK(hipMemcpyAsync(c.h_stats, w.f_srec, (size_t)c.batch * STRUCT_REC * 8, hipMemcpyDeviceToHost, st));
        TCHK(hipStreamSynchronize(st));
    }
    return EIGEN_OK;
}

int flow_members_call(FlowWork& w, const uint8_t* d_ref, const float* d_fref, int64_t r_bstride, int32_t batch, const eigen_flow_members* members, const uint8_t* d_mask,
                      uint8_t* h_members, int32_t* h_counts, void* stream)
{
    FlowSpec f;
    f.by_score = true;  // the stage alone stands for a scored term
    f.mask = d_mask;
    TCHK(hipSetDevice(w.device));
    int rc = check_flow_members(w, members, d_mask, batch, f);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    corner_stage(w, st, batch, f, d_ref, d_fref, r_bstride);
    TCHK(hipGetLastError());
    if (h_members) TCHK(hipMemcpyAsync(h_members, w.c_member, (size_t)batch * w.HW, hipMemcpyDeviceToHost, st));
    if (h_counts) TCHK(hipMemcpyAsync(h_counts, w.c_count, (size_t)batch * 4, hipMemcpyDeviceToHost, st));
    TCHK(hipStreamSynchronize(st));
    return EIGEN_OK;
}

}  // namespace eigf

// ---------------------------------------------------------------------------------------------------- the dense fitness's stage
// (dense_stage.h; eigen_engine.hip holds the entries and the workspace).  The score's rules are check_flow_score's and
// check_flow_struct's, the passes are score_passes and struct_passes, behind the score-only kernels of dense_fitness_kernels.h in
// place of the prepare and solve kernels.
namespace eigd {

using namespace eigf;

static_assert(DENSE_REC == SCORE_REC && DENSE_REC == STRUCT_REC, "one record size for every score");
static_assert(DENSE_PART >= SCORE_SLICES * SCORE_K && DENSE_PART >= STRUCT_SLICES * STRUCT_K, "the partials of every score fit");

int dense_solve_check(const eigen_dense_solve* solve, bool force_iterated, int H, int W, DenseSolve& out)
{
    out = DenseSolve();
    out.iterated = force_iterated;
    if (!solve) return EIGEN_OK;
    if (solve->levels < 1 || solve->levels > DENSE_MAX_LEVELS) return tfail(EIGEN_ERR_INVALID, "dense solve levels %d outside 1 .. %d", solve->levels, DENSE_MAX_LEVELS);
    if (solve->iters < 1 || solve->iters > DENSE_MAX_ITERS) return tfail(EIGEN_ERR_INVALID, "dense solve iters %d outside 1 .. %d", solve->iters, DENSE_MAX_ITERS);
    int h = H, w = W;
    for (int l = 1; l < solve->levels; ++l) { h = (h + 1) / 2; w = (w + 1) / 2; }
    if ((h < w ? h : w) < DENSE_MIN_COARSE)
        return tfail(EIGEN_ERR_INVALID, "dense solve levels %d: the coarsest level of a %d x %d image is %d x %d, below %d pixels", solve->levels, W, H, w, h, DENSE_MIN_COARSE);
    out.levels = solve->levels; out.iters = solve->iters;
    out.iterated = force_iterated || solve->levels > 1 || solve->iters > 1;
    return EIGEN_OK;
}

// allowed_flags: 0, or EIGEN_DENSE_FLOAT_FRAMES where the entry takes float frames
static int dense_spec(const eigen_dense_settings* s, int device, int H, int W, const uint8_t* d_mask, int32_t allowed_flags, FlowSpec& f)
{
    if (!s) return tfail(EIGEN_ERR_INVALID, "null argument");
    if ((s->score != nullptr) == (s->sscore != nullptr)) return tfail(EIGEN_ERR_INVALID, "exactly one of the flow score and the flow structure score must be given");
    if (!allowed_flags && s->flow.flags == EIGEN_DENSE_FLOAT_FRAMES)
        return tfail(EIGEN_ERR_INVALID, "flow flags 0x%x: the byte stage takes no float frames, eigen_dense_score_float does", (unsigned)s->flow.flags);
    int rc = check_flow_on(device, (long long)H * W, &s->flow, nullptr, d_mask, allowed_flags, f);
    if (rc) return rc;
    rc = check_flow_score(s->score, nullptr, f);
    if (rc) return rc;
    return check_flow_struct(s->sscore, nullptr, f);
}

int dense_check(const eigen_dense_settings* s, const eigen_dense_solve* solve, bool force_iterated, int device, int H, int W, const uint8_t* d_mask, DenseSolve& out)
{
    FlowSpec f;
    const int rc = dense_solve_check(solve, force_iterated, H, W, out);   // ahead of the mask's read-back
    if (rc) return rc;
    return dense_spec(s, device, H, W, d_mask, 0, f);
}

// The engine's image and the members' buffers of a DenseWork as the record the corner stage and check_flow_members work on: every
// reference is bytes, so no byte copy of a float one is kept.  allocs: where corner_workspace records what it makes (null: a launch).
static FlowWork members_view(int device, int C, int H, int W, int max_batch, const DenseWork& w, std::vector<void*>* allocs)
{
    FlowWork v;
    v.device = device; v.C = C; v.H = H; v.W = W; v.HW = (long long)H * W; v.max_batch = max_batch; v.allocs = allocs;
    v.c_byte_refs = true;
    v.c_gray = w.c_gray; v.c_member = w.c_member; v.c_eig = w.c_eig; v.c_corners = w.c_corners; v.c_cand = w.c_cand; v.c_count = w.c_count;
    return v;
}

// The Free structure's list at `cap` slots per sample, made by the first call that needs it: one block (theta, the indices, the counts),
// so all of it or none.  A later call that needs more slots replaces it.
static int list_workspace(int device, int max_batch, long long cap, DenseWork& w)
{
    if (w.list_th && cap <= w.list_cap) return EIGEN_OK;
    TCHK(hipSetDevice(device));
    const long long slots = (long long)max_batch * cap, bytes = slots * 12 + (long long)max_batch * 4;
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, (size_t)bytes);
    if (e != hipSuccess) return tfail(EIGEN_ERR_HIP, "hipMalloc(%lld) for the dense fitness's member list: %s", bytes, hipGetErrorString(e));
    if (w.list_th) {
        TCHK(hipFree(w.list_th));  // waits for whatever still reads it
        w.member_allocs.erase(std::find(w.member_allocs.begin(), w.member_allocs.end(), (void*)w.list_th));
    }
    w.member_allocs.push_back(p);
    w.list_th = (double*)p; w.list_idx = (int*)(w.list_th + slots); w.list_count = w.list_idx + slots; w.list_cap = cap;
    return EIGEN_OK;
}

int dense_check_members(const eigen_dense_settings* s, const eigen_dense_solve* solve, bool force_iterated, int device, int C, int H, int W, int max_batch,
                        const uint8_t* d_mask, const eigen_flow_members* members, int B, DenseWork& w, DenseSolve& out, DenseMembers& mem, int32_t allowed_flags)
{
    mem = DenseMembers();
    FlowSpec f;
    int rc = dense_solve_check(solve, force_iterated, H, W, out);
    if (rc) return rc;
    rc = dense_spec(s, device, H, W, per_sample_mask(members) ? nullptr : d_mask, allowed_flags, f);   // per-sample planes are check_flow_members' to read
    if (rc || !members) return rc;
    FlowWork v = members_view(device, C, H, W, max_batch, w, &w.member_allocs);
    rc = check_flow_members(v, members, d_mask, B, f);   // every refusal of it comes ahead of its one allocation, the corner buffers
    if (rc) return rc;
    w.c_gray = v.c_gray; w.c_member = v.c_member; w.c_eig = v.c_eig; w.c_corners = v.c_corners; w.c_cand = v.c_cand; w.c_count = v.c_count;
    mem.given = true; mem.by_corners = f.by_corners;
    mem.max_corners = f.max_corners; mem.block_size = f.block_size; mem.quality = f.quality; mem.min_distance = f.min_distance;
    mem.mask_bstride = f.mask_bstride;
    if (!f.by_struct || f.sscore.structure != STRUCT_FREE) return EIGEN_OK;
    mem.list_cap = f.by_corners ? f.max_corners : H * W;
    return list_workspace(device, max_batch, f.by_corners ? (long long)CORNER_MAX : (long long)H * W, w);
}

// The iterated solve from the gray planes of level 0, which the caller has launched: the reduced levels, then one launch per level from
// the coarsest to the finest, whose field goes into u.  w.pyr holds, level after level, I0_l, I1_l and (l >= 1) the level's field.
static void dense_pyr_levels(const DenseSolve& solve, int r, double eps, int H, int W, int B, const DenseWork& w, double* u, hipStream_t st)
{
    struct Level { int H, W; double *I0, *I1, *u; } lv[DENSE_MAX_LEVELS];
    double* at = w.pyr;
    for (int l = 0, h = H, ww = W; l < solve.levels; ++l, h = (h + 1) / 2, ww = (ww + 1) / 2) {
        const long long n = (long long)B * h * ww;
        lv[l] = Level{h, ww, at, at + n, l ? at + 2 * n : u};
        at += 4 * n;
    }
    for (int l = 1; l < solve.levels; ++l) {
        const long long n = (long long)B * lv[l].H * lv[l].W;
        ew(st, tdense_pyrdown_kernel, n, (const double*)lv[l - 1].I0, (const double*)lv[l - 1].I1, lv[l - 1].H, lv[l - 1].W, lv[l].H, lv[l].W, n, lv[l].I0, lv[l].I1);
    }
    const int lds = pyr_lds_doubles(r) * 8;
    if (lds > 64 * 1024)   // radius 11 and above: more dynamic LDS than a launch gets without the attribute (set on the current device, as the CPPN launches do)
        (void)hipFuncSetAttribute((const void*)tdense_iter_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    for (int l = solve.levels - 1; l >= 0; --l) {
        const bool top = l == solve.levels - 1;
        hipLaunchKernelGGL(tdense_iter_kernel, flow_grid(lv[l].H, lv[l].W, B), dim3(FLOW_T), (size_t)lds, st, (const double*)lv[l].I0, (const double*)lv[l].I1, lv[l].H,
                           lv[l].W, r, eps, solve.iters, top ? (const double*)nullptr : (const double*)lv[l + 1].u, top ? 0 : lv[l + 1].H, top ? 0 : lv[l + 1].W, lv[l].u);
    }
}

// The spec of checked settings: the same fields give the same spec, without the mask's read-back
static FlowSpec dense_checked_spec(const eigen_dense_settings* s)
{
    FlowSpec f;
    f.r = s->flow.radius; f.eps = s->flow.eps;
    (void)check_flow_score(s->score, nullptr, f);
    (void)check_flow_struct(s->sscore, nullptr, f);
    return f;
}

// What follows the solve, for byte and float frames alike: who is counted, then the score's passes on the field u.  img0: the bytes of the
// image the solve treats as the reference, read under corner members only.
static void dense_score_launch(const FlowSpec& f, int C, int H, int W, const uint8_t* img0, long long stride0, int B, const uint8_t* d_mask, const DenseWork& w,
                               const double* u, hipStream_t st, const DenseMembers& mem)
{
    // Who is counted.  No members: one plane shared by the batch (mask stride 0).  Corner members: the trainer's membership stage on
    // img0, the image the solve treats as the reference, under the shared plane; its member planes then take the mask's place.
    // Per-sample planes: d_mask holds them.  Members change nothing of the solve above.
    const uint8_t* mask = d_mask;
    long long mask_bstride = 0;
    if (mem.by_corners) {
        FlowWork v = members_view(0, C, H, W, B, w, nullptr);
        FlowSpec g;
        g.mask = d_mask; g.max_corners = mem.max_corners; g.block_size = mem.block_size; g.quality = mem.quality; g.min_distance = mem.min_distance;
        corner_stage(v, st, B, g, img0, nullptr, stride0);
        mask = w.c_member; mask_bstride = (long long)H * W;
    } else if (mem.given) {
        mask_bstride = mem.mask_bstride;
    }
    // no value beside the records, and for Free no rowS / colS: the fitness takes no gradient; under members the compacted pair pass
    const FreeList list = {w.list_idx, w.list_th, w.list_count, mem.list_cap};
    if (f.by_score) score_passes(st, H, W, B, mask, mask_bstride, f.score, u, w.rec, w.part, nullptr);
    else if (f.sscore.structure == STRUCT_BANDS)
        struct_passes<STRUCT_BANDS>(st, H, W, B, mask, mask_bstride, f.sscore, u, w.theta, w.flag, w.L, nullptr, nullptr, w.rec, w.part, nullptr);
    else
        struct_passes<STRUCT_FREE>(st, H, W, B, mask, mask_bstride, f.sscore, u, w.theta, w.flag, w.L, nullptr, nullptr, w.rec, w.part, nullptr, mem.given ? &list : nullptr);
}

void dense_launch(const eigen_dense_settings* s, const DenseSolve& solve, int C, int H, int W, const uint8_t* img0, long long stride0, const uint8_t* img1,
                  long long stride1, int B, const uint8_t* d_mask, const DenseWork& w, double* d_flow, hipStream_t st, const DenseMembers& mem)
{
    const FlowSpec f = dense_checked_spec(s);
    const long long n = (long long)B * H * W;
    double* u = d_flow ? d_flow : w.u;
    if (solve.iterated) {
        ew(st, tdense_gray_kernel, n, img0, stride0, img1, stride1, C, H, W, n, w.pyr, w.pyr + n);
        dense_pyr_levels(solve, f.r, f.eps, H, W, B, w, u, st);
    } else {
        ew(st, tdense_prep_kernel, n, img0, stride0, img1, stride1, C, H, W, n, w.planes);
        hipLaunchKernelGGL(tdense_solve_kernel, flow_grid(H, W, B), dim3(FLOW_T), 0, st, (const double*)w.planes, n, H, W, f.r, f.eps, u);
    }
    dense_score_launch(f, C, H, W, img0, stride0, B, d_mask, w, u, st, mem);
}

// ---- float frames (dense_float_kernels.h, DESIGN.md section 14, "Float frames")
int dense_gray_workspace(int device, int H, int W, int max_batch, const DenseSolve& solve, bool float_img0, bool by_corners, int C, DenseWork& w)
{
    TCHK(hipSetDevice(device));
    const std::pair<void**, long long> want[] = {{(void**)&w.gray, solve.iterated ? 0 : 2ll * max_batch * H * W * 8},
                                                 {(void**)&w.fbytes, float_img0 && by_corners ? (long long)max_batch * C * H * W : 0}};
    // all or none: the record takes what this call made once every buffer it asked for exists, a failure frees what it made
    void* made[2] = {nullptr, nullptr};
    for (int i = 0; i < 2; ++i) {
        if (!want[i].second || *want[i].first) continue;
        const hipError_t e = hipMalloc(&made[i], (size_t)want[i].second);
        if (e != hipSuccess) {
            if (made[0]) (void)hipFree(made[0]);
            return tfail(EIGEN_ERR_HIP, "hipMalloc(%lld) for the dense fitness's float frames: %s", want[i].second, hipGetErrorString(e));
        }
    }
    for (int i = 0; i < 2; ++i) {
        if (!made[i]) continue;
        *want[i].first = made[i];
        w.member_allocs.push_back(made[i]);
    }
    return EIGEN_OK;
}

void dense_gray_planes(const DenseWork& w, const DenseSolve& solve, int H, int W, int B, double*& I0, double*& I1)
{
    I0 = solve.iterated ? w.pyr : w.gray;
    I1 = I0 + (long long)B * H * W;
}

void dense_gray_launch(const float* img, long long stride, int C, int H, int W, int B, double* dst, hipStream_t st)
{
    const long long HW = (long long)H * W;
    ew(st, tdense_gray_of_kernel<float>, B * HW, img, stride, C, HW, B * HW, dst);
}

void dense_gray_launch(const uint8_t* img, long long stride, int C, int H, int W, int B, double* dst, hipStream_t st)
{
    const long long HW = (long long)H * W;
    ew(st, tdense_gray_of_kernel<uint8_t>, B * HW, img, stride, C, HW, B * HW, dst);
}

void dense_quant_launch(const float* img, long long stride, int C, int H, int W, int B, const DenseWork& w, hipStream_t st)
{
    const long long CHW = (long long)C * H * W;
    ew(st, tcorner_quant_kernel, B * CHW, img, stride, CHW, B * CHW, w.fbytes);
}

void dense_launch_gray(const eigen_dense_settings* s, const DenseSolve& solve, int C, int H, int W, const uint8_t* img0, long long stride0, int B, const uint8_t* d_mask,
                       const DenseWork& w, double* d_flow, hipStream_t st, const DenseMembers& mem)
{
    const FlowSpec f = dense_checked_spec(s);
    const long long n = (long long)B * H * W;
    double* u = d_flow ? d_flow : w.u;
    if (solve.iterated) {
        dense_pyr_levels(solve, f.r, f.eps, H, W, B, w, u, st);   // the planes are level 0 of the pyramid: tdense_gray_kernel is not launched
    } else {
        double *I0, *I1;
        dense_gray_planes(w, solve, H, W, B, I0, I1);
        ew(st, tdense_prep_gray_kernel, n, (const double*)I0, (const double*)I1, H, W, n, w.planes);
        hipLaunchKernelGGL(tdense_solve_kernel, flow_grid(H, W, B), dim3(FLOW_T), 0, st, (const double*)w.planes, n, H, W, f.r, f.eps, u);
    }
    dense_score_launch(f, C, H, W, img0, stride0, B, d_mask, w, u, st, mem);
}

}  // namespace eigd
