// prednet_train.hip -- C ABI of PredNet training (include/eigen_engine.h, eigen_trainer_*): parameter
// layout, tape, and the launch sequence of the training forward, backprop through time, wgrad and Adam.  All compute is in
// the kernels of train_kernels.h, for the frame gradient and the refinement of stills frame_grad_kernels.h, and for
// the optimiser controls (gradient norms, accumulation, clipping, weight decay) optim_kernels.h.  The flow objective's stage and its
// kernels are flow_stage.hip's: this unit holds its workspace (FlowWork) and reaches it through flow_stage.h alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/eigen_engine.h"
#include "train_kernels.h"
#include "frame_grad_kernels.h"
#include "optim_kernels.h"
#include "flow_stage.h"

using namespace eigt;
using namespace eigf;

// flow_stage.h: the one kernel of this unit that the flow stage launches
void eigf::flow_value_final(hipStream_t st, const double* part, double numel, double* d_value)
{
    hipLaunchKernelGGL(tloss_step_final_kernel, dim3(1), dim3(64), 0, st, part, STEP_LOSS_BLOCKS, 1, numel, d_value, 1);
}

namespace {

constexpr long long SLAB_FLOATS = 16ll << 20;  // split-K slab budget of one wgrad (floats)
constexpr int WGRAD_WAVES = 2048;              // split-K target: waves of one wgrad launch
constexpr int LOSS_BLOCKS = 256;
constexpr int BIAS_SLICES = 64;                // slices of one bias-gradient reduction

// offsets (floats) of one layer's parameters in the flat device table; gate tensors of one source are stacked i, f, c, o
struct LayerParams {
    long long aW = -1, ab = -1;   // ConvA (l > 0)
    long long pW, pb;             // ConvP
    long long x0, x1 = -1, hW, hb; // ConvLSTM sources (stacked [4C][Cin][3][3]) and h bias [4C]
    long long peep;               // c_i, c_f, c_o [3][C][H][W]
};

struct TLayer {
    int C, H, W, Cb, Ca;          // channels, size, channels of the layer below (Cb) and above (Ca, 0 at the top)
    long long HW;
    // tape: [slot][batch][ch][H][W], addressed through the accessors below and nowhere else.  Two slot conventions:
    //   tape slot s of E [2C], G (gates) [4C], ZA [C at the size of the layer below = 4 C HW; l > 0] and dV [C]: what step s
    //     wrote; max_steps slots;
    //   state slot s of h, c and P [C]: slot 0 is the start state, step s reads slot s and writes slot s + 1; max_steps + 1 slots.
    float *E = nullptr, *G = nullptr, *ZA = nullptr, *dV = nullptr, *h = nullptr, *c = nullptr, *P = nullptr;
    // backward work buffers, one batch each
    float *dE = nullptr, *dhP = nullptr, *dhc = nullptr, *dc = nullptr, *dPn = nullptr, *dup = nullptr;

    long long CHW() const { return C * HW; }
    float* E_at(int slot, int B) const { return E + (long long)slot * B * 2 * CHW(); }
    float* G_at(int slot, int B) const { return G + (long long)slot * B * 4 * CHW(); }
    float* ZA_at(int slot, int B) const { return ZA ? ZA + (long long)slot * B * 4 * CHW() : nullptr; }
    float* dV_at(int slot, int B) const { return dV + (long long)slot * B * CHW(); }
    float* state_at(int part, int slot, int B) const { return (part == 0 ? h : part == 1 ? c : P) + (long long)slot * B * CHW(); }
    float* h_at(int slot, int B) const { return state_at(0, slot, B); }
    float* c_at(int slot, int B) const { return state_at(1, slot, B); }
    float* P_at(int slot, int B) const { return state_at(2, slot, B); }
};

}  // namespace

struct eigen_trainer {
    eigen_trainer_config cfg;
    int L = 0;
    TLayer ly[EIGEN_MAX_LAYERS];
    LayerParams lp[EIGEN_MAX_LAYERS];
    long long n_params = 0;
    float *prm = nullptr, *grd = nullptr, *mom = nullptr, *var = nullptr;
    float* slab = nullptr;
    long long slab_floats = 0;
    double *d_part = nullptr, *d_loss = nullptr;
    double *d_spart = nullptr, *d_step = nullptr;  // per-step loss: partials [max_steps][STEP_LOSS_BLOCKS], losses [max_steps]
    double* d_err = nullptr;                       // error-unit means err[s][l]: [max_steps][n_layers]
    float* d_absmax = nullptr;                     // eigen_trainer_still_step: max |g| of every image, [max_batch]
    FlowWork fw;                                   // the flow objective's image and buffers (flow_stage.h); allocate() makes the up-front ones
    double* d_jstep = nullptr;                     // the joint objective's: the squared error of every step [max_steps]
    // the optimiser controls' (optim_kernels.h): the (offset, count) of every tensor [n_tensors][2], the partials of the sums of squares
    // [n_tensors][NORM_SLICES], the sums [n_tensors] and the global norm [1]; the gradient accumulator [n_params], made by the first
    // call that adds to it (accumulator), and how many gradients it holds (0: empty)
    int n_tensors = 0;
    long long* o_tab = nullptr;
    double *o_part = nullptr, *o_sumsq = nullptr, *o_norm = nullptr;
    float* acc = nullptr;
    int acc_count = 0;
    long long tape_bytes = 0;
    bool have_weights = false;
    int state_batch = 0, state_slot = 0;  // batch and final slot of the last loss_grad / evaluate call (0: no state kept)
    int adam_t = 0;
    std::vector<void*> allocs;
};

namespace {

using Table = std::vector<std::pair<long long, long long>>;

// (offset, elements) of every tensor in the order of weights.tensor_names
Table tensor_table(const eigen_trainer* t)
{
    Table tab;
    for (int l = 0; l < t->L; ++l) {
        const TLayer& y = t->ly[l];
        const LayerParams& p = t->lp[l];
        const long long C = y.C;
        if (l > 0) {
            tab.push_back({p.aW, C * y.Cb * 2 * 9});
            tab.push_back({p.ab, C});
        }
        tab.push_back({p.pW, C * C * 9});
        tab.push_back({p.pb, C});
        for (int g = 0; g < 4; ++g) {
            tab.push_back({p.x0 + g * C * 2 * C * 9, C * 2 * C * 9});
            if (l < t->L - 1) tab.push_back({p.x1 + g * C * y.Ca * 9, C * y.Ca * 9});
            tab.push_back({p.hW + g * C * C * 9, C * C * 9});
            tab.push_back({p.hb + g * C, C});
        }
        for (int g = 0; g < 3; ++g) tab.push_back({p.peep + g * C * y.HW, C * y.HW});
    }
    return tab;
}

TSrc src(const float* p, long long nstride, int cin, int up, const float* w, int wmode)
{
    TSrc s;
    s.p = p; s.w = w; s.nstride = nstride; s.cin = cin; s.up = up; s.wmode = wmode; s.pad_ = 0;
    return s;
}

template <int MT>
void launch_conv_mt(const TConvArgs& a, hipStream_t st)
{
    constexpr int NT = 4;
    const long long P = (long long)a.N * a.H * a.W;
    dim3 grid((unsigned)((P + 16 * NT - 1) / (16 * NT)), (unsigned)((a.cout + 16 * MT - 1) / (16 * MT)));
    hipLaunchKernelGGL((tconv3x3_kernel<MT, NT>), grid, dim3(WAVE), 0, st, a);
}

// 3x3 'same' convolution over up to three summed sources, out [N][cout][H][W] (contiguous samples)
void conv(hipStream_t st, float* out, int cout, int H, int W, int N, const float* bias, int accumulate, std::initializer_list<TSrc> srcs)
{
    TConvArgs a;
    memset(&a, 0, sizeof(a));
    a.nsrc = 0;
    for (const TSrc& s : srcs) a.s[a.nsrc++] = s;
    a.out = out; a.out_nstride = (long long)cout * H * W; a.bias = bias;
    a.cout = cout; a.H = H; a.W = W; a.N = N; a.accumulate = accumulate;
    if (cout <= 16) launch_conv_mt<1>(a, st);
    else if (cout <= 32) launch_conv_mt<2>(a, st);
    else launch_conv_mt<4>(a, st);
}

template <int MT>
void launch_wgrad_mt(const TWgradArgs& a, unsigned gx, unsigned gy, hipStream_t st)
{
    hipLaunchKernelGGL((twgrad_kernel<MT, 4>), dim3(gx, gy, (unsigned)a.nsplit), dim3(WAVE), 0, st, a);
}

// dW [cout][cin][3][3] = sum over N samples of dy (x) im2col(x): split-K over fixed pixel ranges, slabs added in order
void wgrad(eigen_trainer* t, hipStream_t st, float* dW, const float* dy, int cout, int H, int W, int N, const TSrc& x)
{
    const long long P = (long long)N * H * W;
    const long long K = (long long)x.cin * 9;
    const int MT = cout <= 16 ? 1 : cout <= 32 ? 2 : 4;
    const unsigned gx = (unsigned)((K + 63) / 64), gy = (unsigned)((cout + 16 * MT - 1) / (16 * MT));
    long long ns = WGRAD_WAVES / (long long)(gx * gy);
    ns = std::min<long long>(ns, t->slab_floats / (cout * K));
    ns = std::min<long long>(ns, (P + 255) / 256);
    ns = std::max<long long>(ns, 1);
    long long chunk = (P + ns - 1) / ns;
    chunk = (chunk + 3) & ~3ll;
    ns = (P + chunk - 1) / chunk;
    TWgradArgs a;
    a.dy = dy; a.dy_nstride = (long long)cout * H * W; a.x = x; a.slab = t->slab;
    a.cout = cout; a.H = H; a.W = W; a.N = N; a.nsplit = (int)ns; a.chunk = chunk;
    if (MT == 1) launch_wgrad_mt<1>(a, gx, gy, st);
    else if (MT == 2) launch_wgrad_mt<2>(a, gx, gy, st);
    else launch_wgrad_mt<4>(a, gx, gy, st);
    const long long n = cout * K;
    ew(st, tsum_slabs_kernel, n, (const float*)t->slab, (int)ns, n, dW);
}

// db [C] = sum over N samples and all pixels of dy [N][C][HW]: BIAS_SLICES fixed slices per channel, added in order
void bias_grad(eigen_trainer* t, hipStream_t st, float* db, const float* dy, int C, long long HW, int N)
{
    hipLaunchKernelGGL(tbias_grad_kernel, dim3(C, BIAS_SLICES), dim3(EW_T), 0, st, dy, C, (int)HW, N, t->slab);
    ew(st, tsum_slabs_kernel, C, (const float*)t->slab, BIAS_SLICES, (long long)C, db);
}

// shapes of every layer, offsets of its parameters in the flat table, and the split-K slab that holds the largest wgrad
void plan_layout(eigen_trainer* t)
{
    const eigen_trainer_config& cfg = t->cfg;
    const int L = t->L;
    long long off = 0, slab = 0;
    for (int l = 0; l < L; ++l) {
        TLayer& y = t->ly[l];
        y.C = cfg.channels[l]; y.H = cfg.height >> l; y.W = cfg.width >> l; y.HW = (long long)y.H * y.W;
        y.Cb = l > 0 ? cfg.channels[l - 1] : 0;
        y.Ca = l < L - 1 ? cfg.channels[l + 1] : 0;
        const long long C = y.C;
        LayerParams& p = t->lp[l];
        if (l > 0) { p.aW = off; off += C * 2 * y.Cb * 9; p.ab = off; off += C; slab = std::max(slab, C * 2 * y.Cb * 9); }
        p.pW = off; off += C * C * 9; p.pb = off; off += C;
        p.x0 = off; off += 4 * C * 2 * C * 9;
        if (l < L - 1) { p.x1 = off; off += 4 * C * y.Ca * 9; slab = std::max(slab, 4 * C * y.Ca * 9); }
        p.hW = off; off += 4 * C * C * 9; p.hb = off; off += 4 * C;
        p.peep = off; off += 3 * C * y.HW;
        slab = std::max(slab, std::max(4 * C * 2 * C * 9, BIAS_SLICES * 4 * C));
    }
    t->slab_floats = std::max(slab, SLAB_FLOATS);
    t->n_params = off;
    // the flow stage sees the image layer and the handle's capacity, and records its lazy workspaces in the handle's list
    FlowWork& w = t->fw;
    w.device = cfg.device; w.C = t->ly[0].C; w.H = t->ly[0].H; w.W = t->ly[0].W; w.HW = t->ly[0].HW;
    w.max_batch = cfg.max_batch; w.max_steps = cfg.max_steps; w.allocs = &t->allocs;
}

// every device buffer of the handle, parameters and gradients zeroed; after a failure the caller destroys t, which frees what was made
int allocate(eigen_trainer* t)
{
    const long long B = t->cfg.max_batch, T = t->cfg.max_steps, L = t->L, np = t->n_params;
    std::vector<std::pair<void**, size_t>> want;
    auto add = [&](void** p, long long bytes) { want.push_back({p, (size_t)bytes}); };
    auto tape = [&](float** p, long long floats) { add((void**)p, floats * 4); t->tape_bytes += floats * 4; };
    for (void** p : {(void**)&t->prm, (void**)&t->grd, (void**)&t->mom, (void**)&t->var}) add(p, np * 4);
    add((void**)&t->slab, t->slab_floats * 4);
    add((void**)&t->d_part, LOSS_BLOCKS * 8); add((void**)&t->d_loss, 8);
    add((void**)&t->d_spart, T * STEP_LOSS_BLOCKS * 8); add((void**)&t->d_step, T * 8); add((void**)&t->d_err, T * L * 8);
    add((void**)&t->d_absmax, B * 4);
    FlowWork& fw = t->fw;
    add((void**)&fw.f_planes, 3 * B * fw.HW * 8); add((void**)&fw.f_q, 2 * B * fw.HW * 8); add((void**)&fw.f_mv, B * fw.HW * 8);
    add((void**)&fw.f_u, 2 * B * fw.HW * 8); add((void**)&fw.f_r, 3 * B * fw.HW * 8);
    add((void**)&fw.f_rec, B * FLOW_REC * 8); add((void**)&fw.f_spart, B * SCORE_PART * 8);
    for (int l = 0; l < L; ++l) {
        TLayer& y = t->ly[l];
        const long long CHW = y.CHW();
        tape(&y.E, T * B * 2 * CHW);
        tape(&y.G, T * B * 4 * CHW);
        tape(&y.dV, T * B * CHW);
        if (l > 0) tape(&y.ZA, T * B * 4 * CHW);
        for (float** p : {&y.h, &y.c, &y.P}) tape(p, (T + 1) * B * CHW);
        add((void**)&y.dE, B * 2 * CHW * 4);
        for (float** p : {&y.dhP, &y.dhc, &y.dc, &y.dPn}) add((void**)p, B * CHW * 4);
        if (l > 0) add((void**)&y.dup, B * 4 * CHW * 4);  // [B][C_l][H_{l-1}][W_{l-1}]
    }
    // the structure scores' workspace comes last: the allocations above keep the order they had without it
    add((void**)&fw.f_g, 2 * B * fw.HW * 8); add((void**)&fw.f_srec, B * FLOW_REC * 8); add((void**)&fw.f_sspart, B * STRUCT_PART * 8);
    add((void**)&fw.f_theta, B * fw.HW * 8); add((void**)&fw.f_L, B * fw.HW * 8);
    add((void**)&fw.f_rowS, B * fw.HW * 4); add((void**)&fw.f_colS, B * fw.HW * 4); add((void**)&fw.f_flag, B * fw.HW);
    // and behind it the optimiser controls' tensor table and reduction buffers
    const Table tab = tensor_table(t);
    const long long nt = t->n_tensors = (int)tab.size();
    add((void**)&t->o_tab, nt * 16); add((void**)&t->o_part, nt * NORM_SLICES * 8); add((void**)&t->o_sumsq, nt * 8); add((void**)&t->o_norm, 8);
    // and last the validity planes' r_b and the joint objective's squared-error steps
    add((void**)&fw.f_vr, B * 8); add((void**)&t->d_jstep, T * 8);
    for (auto& w : want) {
        const hipError_t e = hipMalloc(w.first, w.second);
        if (e != hipSuccess) return tfail(EIGEN_ERR_HIP, "hipMalloc(%zu): %s", w.second, hipGetErrorString(e));
        t->allocs.push_back(*w.first);
    }
    hipError_t e = hipMemset(t->grd, 0, np * 4);
    if (e == hipSuccess) e = hipMemset(t->prm, 0, np * 4);
    if (e != hipSuccess) return tfail(EIGEN_ERR_HIP, "hipMemset: %s", hipGetErrorString(e));
    std::vector<long long> flat;
    for (const auto& r : tab) { flat.push_back(r.first); flat.push_back(r.second); }
    TCHK(hipMemcpy(t->o_tab, flat.data(), flat.size() * 8, hipMemcpyHostToDevice));
    return EIGEN_OK;
}

// Up to two host tables (eigen_set_prednet_weights order) to or from the flat device arrays d0, d1: h1 / d1 may be null.  The count and every
// pointer are checked before anything reaches the device.
int copy_tables(eigen_trainer* t, int32_t n, bool to_device, float* d0, const float* const* h0, float* d1 = nullptr, const float* const* h1 = nullptr)
{
    if (!t || !h0) return tfail(EIGEN_ERR_INVALID, "null argument");
    const Table tab = tensor_table(t);
    if (n != (int32_t)tab.size()) return tfail(EIGEN_ERR_INVALID, "expected %d weight tensors for %d layers, got %d", (int)tab.size(), t->L, n);
    for (int i = 0; i < n; ++i) if (!h0[i] || (h1 && !h1[i])) return tfail(EIGEN_ERR_INVALID, "tensor %d is NULL", i);
    TCHK(hipSetDevice(t->cfg.device));
    TCHK(hipDeviceSynchronize());
    for (int k = 0; k < (h1 ? 2 : 1); ++k)
        for (int i = 0; i < n; ++i) {
            float *dev = (k ? d1 : d0) + tab[i].first, *host = const_cast<float*>((k ? h1 : h0)[i]);
            TCHK(to_device ? hipMemcpy(dev, host, tab[i].second * 4, hipMemcpyHostToDevice) : hipMemcpy(host, dev, tab[i].second * 4, hipMemcpyDeviceToHost));
        }
    return EIGEN_OK;
}

// argument rules shared by loss_grad_frames and evaluate_err; max_steps < 0: n_steps is not bounded
int check_call(const eigen_trainer* t, const uint8_t* d_frames, int64_t bstride, int32_t batch, int32_t n_steps, int32_t n_fed, int32_t requant, int32_t reset, int max_steps)
{
    if (!t || !d_frames) return tfail(EIGEN_ERR_INVALID, "null argument");
    if (!t->have_weights) return tfail(EIGEN_ERR_STATE, "eigen_trainer_set_weights has not been called");
    if (batch < 1 || n_steps < 1) return tfail(EIGEN_ERR_INVALID, "batch >= 1 and n_steps >= 1 required");
    if (batch > t->cfg.max_batch || (max_steps >= 0 && n_steps > max_steps))
        return tfail(EIGEN_ERR_CAPACITY, "batch %d / %d steps exceed the trainer's %d / %d", batch, n_steps, t->cfg.max_batch, t->cfg.max_steps);
    if (reset && n_steps < 2) return tfail(EIGEN_ERR_INVALID, "a reset call needs n_steps >= 2 (one loss term per next frame)");
    if (n_fed < 0 || n_fed > n_steps) return tfail(EIGEN_ERR_INVALID, "n_fed %d outside [0, n_steps = %d]", n_fed, n_steps);
    if (n_fed == 0 && reset) return tfail(EIGEN_ERR_INVALID, "n_fed = 0 needs reset = 0: a self-fed step continues a kept prediction");
    if (requant != 0 && requant != 1) return tfail(EIGEN_ERR_INVALID, "requant must be 0 or 1");
    if (!reset && t->state_batch != batch)
        return tfail(EIGEN_ERR_STATE, t->state_batch ? "reset = 0 needs the previous call's batch (%d, got %d)" : "reset = 0 with no previous call (%d, got %d)",
                     t->state_batch, batch);
    const long long C0HW = t->ly[0].CHW();
    if (bstride < (long long)n_steps * C0HW && batch > 1)
        return tfail(EIGEN_ERR_INVALID, "bstride %lld is smaller than a sequence (%lld bytes)", (long long)bstride, (long long)n_steps * C0HW);
    return EIGEN_OK;
}

// the handle's device made current, and the start state into state slot 0: zeros, or the state the previous call left
int start_state(eigen_trainer* t, hipStream_t st, int B, int reset)
{
    TCHK(hipSetDevice(t->cfg.device));
    for (int l = 0; l < t->L; ++l) {
        const TLayer& y = t->ly[l];
        const long long bytes = (long long)B * y.CHW() * 4;
        for (int part = 0; part < 3; ++part) {
            if (reset) TCHK(hipMemsetAsync(y.state_at(part, 0, B), 0, bytes, st));
            else if (t->state_slot != 0) TCHK(hipMemcpyAsync(y.state_at(part, 0, B), y.state_at(part, t->state_slot, B), bytes, hipMemcpyDeviceToDevice, st));
        }
    }
    t->state_batch = t->state_slot = 0;
    return EIGEN_OK;
}

// One forward step: reads state slot `in`, writes state slot `out` and tape slot `tp`.  xs: this step's frames (frame of sample b
// at xs + b * bstride), or nullptr for a self-fed step, whose image layer reads P0 of slot `in` (requant: through the byte).
// pred (may be null): P0 of this step for sample b at pred + b * pred_bstride.
void forward_step(eigen_trainer* t, hipStream_t st, int B, int in, int out, int tp, const uint8_t* xs, long long bstride, int requant, float* pred, long long pred_bstride)
{
    const int L = t->L;
    const float* prm = t->prm;
    for (int l = 0; l < L; ++l) {
        const TLayer& y = t->ly[l];
        const long long CHW = y.CHW();
        float* E = y.E_at(tp, B);
        const float* Pp = y.P_at(in, B);
        if (l == 0 && xs) {
            ew(st, terr_fwd_kernel, B * CHW, xs, (long long)bstride, (const float*)nullptr, Pp, E, y.C, y.H, y.W, B);
        } else if (l == 0) {
            ew(st, terr_fed_fwd_kernel, B * CHW, Pp, E, requant, CHW, (long long)B * CHW);
        } else {
            const TLayer& yb = t->ly[l - 1];
            float* ZA = y.ZA_at(tp, B);
            conv(st, ZA, y.C, yb.H, yb.W, B, prm + t->lp[l].ab, 0, {src(yb.E_at(tp, B), 2 * yb.CHW(), 2 * yb.C, 0, prm + t->lp[l].aW, 0)});
            ew(st, terr_fwd_kernel, B * CHW, (const uint8_t*)nullptr, 0ll, (const float*)ZA, Pp, E, y.C, y.H, y.W, B);
        }
    }
    for (int l = L - 1; l >= 0; --l) {
        const TLayer& y = t->ly[l];
        const LayerParams& p = t->lp[l];
        const long long CHW = y.CHW();
        float* G = y.G_at(tp, B);
        const TSrc se = src(y.E_at(tp, B), 2 * CHW, 2 * y.C, 0, prm + p.x0, 0);
        const TSrc sh = src(y.h_at(in, B), CHW, y.C, 0, prm + p.hW, 0);
        if (l < L - 1) {
            const TLayer& ya = t->ly[l + 1];
            conv(st, G, 4 * y.C, y.H, y.W, B, prm + p.hb, 0, {se, src(ya.h_at(out, B), ya.CHW(), ya.C, 1, prm + p.x1, 0), sh});
        } else {
            conv(st, G, 4 * y.C, y.H, y.W, B, prm + p.hb, 0, {se, sh});
        }
        const float* pk = prm + p.peep;
        ew(st, tlstm_fwd_kernel, B * CHW, G, (const float*)y.c_at(in, B), y.c_at(out, B), y.h_at(out, B), pk, pk + CHW, pk + 2 * CHW, y.C, (int)y.HW, B);
        float* P = y.P_at(out, B);
        conv(st, P, y.C, y.H, y.W, B, prm + p.pb, 0, {src(y.h_at(out, B), CHW, y.C, 0, prm + p.pW, 0)});
        ew(st, tpact_fwd_kernel, B * CHW, P, (long long)B * CHW, l == 0 ? 1 : 0, l == 0 ? pred : (float*)nullptr, CHW, pred_bstride);
    }
}

// n per-step means into dst[0], dst[stride], ...  Row r: the sum of `term` over the B samples of `per` floats at p + r * B * per, against the frames at
// x + r * per (sample b at + b * bstride), over div; STEP_LOSS_BLOCKS fixed slices per row, added in order.  Its three uses, with C0HW = C_0 H W:
//   TERM_SQ, div B C0HW: the mse of P0 of n consecutive steps against the frames they predict, the numbers eigen_trainer_evaluate returns;
//   TERM_ABS, div 2 B C0HW, stride L: the image-layer column of the error table err[s][l], the mean of [relu(x - P0), relu(P0 - x)] against the TRUE frame;
//   TERM_SUM, per 2 C_l H_l W_l, no frames, stride L: a column l > 0 of the table, the mean of E_l over n consecutive tape slots (upper_errors).
void reduce_steps(decltype(TERM_SQ) term, eigen_trainer* t, hipStream_t st, const float* p, const uint8_t* x, long long bstride, long long per, int n, int B, double div,
                  double* dst, int stride)
{
    static constexpr decltype(&tloss_step_partial_kernel<TERM_SQ>) partial[] = {tloss_step_partial_kernel<TERM_SQ>, tloss_step_partial_kernel<TERM_ABS>,
                                                                                 tloss_step_partial_kernel<TERM_SUM>};  // [term], in the enum's order
    hipLaunchKernelGGL(partial[term], dim3(STEP_LOSS_BLOCKS, n), dim3(EW_T), 0, st, p, x, bstride, B, per, t->d_spart);
    hipLaunchKernelGGL(tloss_step_final_kernel, dim3((n + 63) / 64), dim3(64), 0, st, (const double*)t->d_spart, STEP_LOSS_BLOCKS, n, div, dst, stride);
}

// columns l > 0 of n consecutive rows of the error table, from tape slot `slot` and the row at err on
void upper_errors(eigen_trainer* t, hipStream_t st, int slot, int n, int B, double* err)
{
    for (int l = 1; l < t->L; ++l)
        reduce_steps(TERM_SUM, t, st, t->ly[l].E_at(slot, B), nullptr, 0ll, 2 * t->ly[l].CHW(), n, B, (double)(B * 2 * t->ly[l].CHW()), err + l, t->L);
}

// The loss of one loss_grad call: the weights of its terms and the seeds they put into the backward pass.
struct Objective {
    bool by_error = false;
    bool by_flow = false;
    FlowSpec flow;                      // by_flow
    double* h_terms = nullptr;          // by_flow: host, T - 1 terms, may be null
    double mu = 0.0;                    // by_flow, the joint objective: the weight of the squared-error term beside the flow terms (0: none)
    double* h_parts = nullptr;          // by_flow: host, (L_flow, L_mse) out, may be null
    bool keep_stats = false;            // by_flow with a score: the records of every computed term are kept in f_stats [T - 1][B][10]
    double weight(int s) const { return step_w ? step_w[s] : 1.0; }
    double total_weight() const { return step_w ? sum_w : (double)(T - 1); }
    const double* step_w = nullptr;     // host, T - 1 weights; NULL: all one
    double sum_w = 0.0;                 // of step_w
    double lam[EIGEN_MAX_LAYERS] = {};  // layer weights of the error-unit objective
    int T = 0, B = 0;
    const TLayer* ly = nullptr;
    long long n_terms() const { return (long long)(T - 1) * B * ly[0].CHW(); }
    // the flow objective: kappa of term s, (w_s / sum w) / (B N_m); in the score mode (w_s / sum w) / B
    double flow_kappa(int s) const { return (weight(s) / total_weight()) / flow.kappa_div(B); }
    // squared error: d loss / d P0_s = loss_scale(s) * (P0_s - x_{s+1})
    double loss_scale64(int s) const { return step_w ? 2.0 * step_w[s] / (sum_w * (double)(B * ly[0].CHW())) : 2.0 / (double)n_terms(); }
    float loss_scale(int s) const { return T < 2 ? 0.f : (float)loss_scale64(s); }
    // the joint objective: mu times the squared error's scale, formed in double and rounded once
    float joint_scale(int s) const { return T < 2 ? 0.f : (float)(mu * loss_scale64(s)); }
    // error units: d loss / d (one element of E_l of term s) = w_s lambda_l / (sum w * numel(E_l)), formed in double
    float err_scale(int s, int l) const
    {
        const double numel = (double)B * 2.0 * (double)ly[l].CHW();
        return step_w ? (float)(step_w[s] * lam[l] / (sum_w * numel)) : (float)(lam[l] / ((double)(T - 1) * numel));
    }
};

// o from the call's arguments: the objective, the layer weights (NULL is L_0, [1, 0, ...]; checked whenever given), the step weights
int make_objective(const eigen_trainer* t, int32_t objective, const double* h_layer_w, const double* h_step_w, int T, int B, Objective& o)
{
    if (objective == EIGEN_OBJ_FLOW) return tfail(EIGEN_ERR_INVALID, "EIGEN_OBJ_FLOW needs the settings eigen_trainer_loss_grad_flow takes");
    if (objective != EIGEN_OBJ_MSE && objective != EIGEN_OBJ_ERROR) return tfail(EIGEN_ERR_INVALID, "objective %d is neither EIGEN_OBJ_MSE nor EIGEN_OBJ_ERROR", objective);
    o.by_error = objective == EIGEN_OBJ_ERROR; o.step_w = h_step_w; o.T = T; o.B = B; o.ly = t->ly;
    if (h_layer_w || o.by_error) {
        double sum = 0.0;
        for (int l = 0; l < t->L; ++l) {
            o.lam[l] = h_layer_w ? h_layer_w[l] : (l == 0 ? 1.0 : 0.0);
            if (!(o.lam[l] >= 0.0) || !std::isfinite(o.lam[l])) return tfail(EIGEN_ERR_INVALID, "layer weight %d is %g: weights must be finite and >= 0", l, o.lam[l]);
            sum += o.lam[l];
        }
        if (!(sum > 0.0)) return tfail(EIGEN_ERR_INVALID, "all %d layer weights are zero", t->L);
    }
    if (h_step_w) {
        for (int s = 0; s < T - 1; ++s) {
            if (!(h_step_w[s] >= 0.0) || !std::isfinite(h_step_w[s])) return tfail(EIGEN_ERR_INVALID, "step weight %d is %g: weights must be finite and >= 0", s, h_step_w[s]);
            o.sum_w += h_step_w[s];
        }
        if (T >= 2 && !(o.sum_w > 0.0)) return tfail(EIGEN_ERR_INVALID, "all %d step weights are zero", T - 1);
    }
    return EIGEN_OK;
}

// The error table (when wanted) into d_err and the squared-error loss into d_loss or d_step.  There are two squared-error reductions on
// purpose.  Without step weights the loss is ONE sum over all terms in LOSS_BLOCKS slices, scaled on the device: eigen_trainer_loss_grad's
// arithmetic, kept to the bit.  With step weights it is the per-step means eigen_trainer_evaluate returns, combined on the host in step order
// (read_loss).  One in place of the other would change the low bits of the returned loss.
int reduce_losses(eigen_trainer* t, hipStream_t st, const Objective& o, const uint8_t* d_frames, long long bstride, bool want_table)
{
    const int T = o.T, B = o.B;
    const long long C0HW = t->ly[0].CHW();
    const float* P0 = t->ly[0].P_at(1, B);  // of step 0: term s is P0 of step s against frame s + 1, and E_l of step s + 1
    if (T < 2) TCHK(hipMemsetAsync(t->d_loss, 0, 8, st));
    if (want_table) {
        reduce_steps(TERM_ABS, t, st, P0, d_frames + C0HW, bstride, C0HW, T - 1, B, (double)(B * 2 * C0HW), t->d_err, t->L);
        upper_errors(t, st, 1, T - 1, B, t->d_err);
    }
    // the error objective's loss is formed from the table, the flow objective's from the terms the backward steps leave, on the host; the
    // joint objective adds the squared error as the "mse" call with the same step weights reduces it, its steps beside the terms' d_step
    if (T < 2 || o.by_error || (o.by_flow && !(o.mu > 0.0))) return EIGEN_OK;
    if (o.step_w) {
        reduce_steps(TERM_SQ, t, st, P0, d_frames + C0HW, bstride, C0HW, T - 1, B, (double)(B * C0HW), o.by_flow ? t->d_jstep : t->d_step, 1);
    } else {
        hipLaunchKernelGGL(tloss_partial_kernel, dim3(LOSS_BLOCKS), dim3(EW_T), 0, st, (const float*)t->ly[0].P_at(0, B), d_frames, bstride, T - 1, B, C0HW, t->d_part);
        hipLaunchKernelGGL(tloss_final_kernel, dim3(1), dim3(64), 0, st, (const double*)t->d_part, LOSS_BLOCKS, 1.0 / (double)o.n_terms(), t->d_loss);
    }
    return EIGEN_OK;
}

// Where a call wants d loss / d frames: sample b, step s at p + b * bstride + s * tstride (floats); tstride == 0 is the tied mode,
// one image per sample into which every step is added.  p == nullptr: not wanted.
struct FrameGrad {
    float* p = nullptr;
    long long bstride = 0, tstride = 0;
};

// One step of backprop through time: the cells bottom up (dP, dh, dc and dZ of step s), then the error units top down.  fg: under
// the flow objective's moving reference, where term s adds its reference path, which belongs to frame s + 1.
int backward_step(eigen_trainer* t, hipStream_t st, const Objective& o, int s, const uint8_t* d_frames, long long bstride, const FrameGrad& fg)
{
    const int L = t->L, T = o.T, B = o.B;
    const float* prm = t->prm;
    for (int l = 0; l < L; ++l) {
        const TLayer& y = t->ly[l];
        const LayerParams& p = t->lp[l];
        const long long CHW = y.CHW();
        const float* P = y.P_at(s + 1, B);
        float* dV = y.dV_at(s, B);
        const uint8_t* xn = (l == 0 && s < T - 1) ? d_frames + (long long)(s + 1) * CHW : nullptr;
        if (o.by_flow && xn) {
            // term s: its value into d_step[s] and its seed added to dP0_s, which tpact_bwd then masks; a term of weight zero is not computed
            // with the moving reference and a frame gradient wanted, the term's reference path is added in float to g_{s+1}, which
            // frame_grad_step(s + 1) stored earlier (per frame), or to the one image of the tied mode ahead of this step's input path
            // under the prediction pairing the reference is P0_{s-1}, state slot s (for s = 0 the call's start state, a constant); the
            // flow is kept in the workspace for the reference path, which follows this step's terr_bwd
            if (o.weight(s) != 0.0) {
                FlowTerm m;
                m.pred = P; m.p_bstride = CHW; m.kappa = o.flow_kappa(s);
                m.part = t->d_spart + (long long)s * STEP_LOSS_BLOCKS; m.d_value = t->d_step + s;
                m.d_seed = y.dPn; m.s_bstride = CHW; m.s_accumulate = 1;
                if (o.flow.target.p) m.target = o.flow.target.p + (long long)s * o.flow.target.tstride;
                if (o.flow.valid.p) m.valid = o.flow.valid.p + (long long)s * o.flow.valid.tstride;
                if (o.flow.pair_pred) {
                    m.fref = y.P_at(s, B); m.r_bstride = CHW;
                    m.d_flow = s >= 1 ? t->fw.f_u : nullptr;
                } else {
                    m.ref = xn; m.r_bstride = bstride;
                    m.d_refg = o.flow.moving && fg.p ? fg.p + (long long)(s + 1) * fg.tstride : nullptr; m.rg_bstride = fg.bstride; m.rg_accumulate = 1;
                }
                flow_stage(t->fw, st, B, o.flow, m);
                // the samples' records of this term, which the next term's stage overwrites: kept on the device, read once the call is done
                if (o.keep_stats)
                    TCHK(hipMemcpyAsync(t->fw.f_stats + (long long)s * B * FLOW_REC, o.flow.by_score ? t->fw.f_rec : t->fw.f_srec, (size_t)B * FLOW_REC * 8,
                                        hipMemcpyDeviceToDevice, st));
            }
            // the joint objective keeps the frame: the squared error's seed joins the flow term's in dP0_s
            if (!(o.mu > 0.0)) xn = nullptr;
        }
        const float scale = !xn ? 0.f : o.by_error ? o.err_scale(s, 0) : o.by_flow ? o.joint_scale(s) : o.loss_scale(s);
        // an error-unit term whose seed is zero is left out, not added as +0.0f (which would turn a -0 gradient into +0)
        if (o.by_error && scale == 0.f) xn = nullptr;
        if (o.by_error && xn)
            ew(st, tpact_bwd_kernel<1>, B * CHW, P, (const float*)y.dPn, xn, (long long)bstride, CHW, scale, 1, (long long)B * CHW, dV);
        else
            ew(st, tpact_bwd_kernel<0>, B * CHW, P, (const float*)y.dPn, xn, (long long)bstride, CHW, scale, l == 0 ? 1 : 0, (long long)B * CHW, dV);
        conv(st, y.dhP, y.C, y.H, y.W, B, nullptr, 0, {src(dV, CHW, y.C, 0, prm + p.pW, 1)});
        float* G = y.G_at(s, B);
        const float* pk = prm + p.peep;
        ew(st, tlstm_bwd_kernel, B * CHW, G, (const float*)y.c_at(s, B), (const float*)y.c_at(s + 1, B), (const float*)y.dhP, (const float*)(s < T - 1 ? y.dhc : nullptr),
           (const float*)(l > 0 ? y.dup : nullptr), y.dc, pk, pk + CHW, pk + 2 * CHW, y.C, y.H, y.W, B);
        // dZ through the three sources: h of the previous step, E of this step, the upsampled h of the layer above
        if (s > 0) conv(st, y.dhc, y.C, y.H, y.W, B, nullptr, 0, {src(G, 4 * CHW, 4 * y.C, 0, prm + p.hW, 1)});
        conv(st, y.dE, 2 * y.C, y.H, y.W, B, nullptr, 0, {src(G, 4 * CHW, 4 * y.C, 0, prm + p.x0, 1)});
        if (l < L - 1) conv(st, t->ly[l + 1].dup, y.Ca, y.H, y.W, B, nullptr, 0, {src(G, 4 * CHW, 4 * y.C, 0, prm + p.x1, 1)});
    }
    // the error units, top down; layer 0 sends dE_0 into dP0_{s-1} under the mask E_0 > 0 on every step: on a teacher-forced
    // step the other path ends in the frame (frame_grad_step takes it from there when the call wants d loss / d frames), on a
    // self-fed one in the constant fed-back value
    for (int l = L - 1; l >= 0; --l) {
        const TLayer& y = t->ly[l];
        const long long CHW = y.CHW();
        const float* E = y.E_at(s, B);
        float* ZA = y.ZA_at(s, B);
        // E_l of step s belongs to term s - 1 (the errors of a call's first step belong to no call)
        const float seed = o.by_error && l > 0 && s >= 1 ? o.err_scale(s - 1, l) : 0.f;
        if (seed != 0.f)
            ew(st, terr_bwd_kernel<1>, B * CHW, (const float*)y.dE, E, y.dPn, ZA, y.C, y.H, y.W, B, seed);
        else
            ew(st, terr_bwd_kernel<0>, B * CHW, (const float*)y.dE, E, y.dPn, ZA, y.C, y.H, y.W, B, 0.f);
        if (l > 0) {
            const TLayer& yb = t->ly[l - 1];
            conv(st, yb.dE, 2 * yb.C, yb.H, yb.W, B, nullptr, 1, {src(ZA, 4 * CHW, y.C, 0, prm + t->lp[l].aW, 1)});
        }
    }
    // the prediction pairing: dP0_{s-1} holds what layer 0's terr_bwd of this step left; term s adds its gradient by its reference
    // P0_{s-1} now, and the seed of term s - 1 follows in backward_step(s - 1), ahead of that step's clamp mask
    if (o.by_flow && o.flow.pair_pred && s >= 1 && s < T - 1 && o.weight(s) != 0.0) {
        if (o.flow.iterated) iter_store(t->fw, st, B, o.flow, true, o.flow_kappa(s), t->ly[0].dPn, t->ly[0].CHW(), 1);
        else flow_ref_path(t->fw, st, B, o.flow, o.flow_kappa(s), t->fw.f_u, t->ly[0].dPn, t->ly[0].CHW(), 1);
    }
    return EIGEN_OK;
}

// g_s of backward step s, after layer 0's terr_bwd of that step (dE_0 and E_0 of step s are what that kernel read): the input path on
// a teacher-forced step, and the target path of term s - 1, whose prediction P0_{s-1} is state slot s
void frame_grad_step(eigen_trainer* t, hipStream_t st, const Objective& o, int s, int n_fed, const uint8_t* d_frames, long long bstride, const FrameGrad& fg)
{
    const TLayer& y = t->ly[0];
    const int B = o.B;
    const long long CHW = y.CHW();
    // under the flow objective this kernel adds no target path: the frames are constants of every term, or, with the moving reference,
    // backward_step(s - 1) adds term s - 1's reference path to what is stored here; the joint objective's squared error has its target path
    const float scale = s < 1 ? 0.f : o.by_flow ? (o.mu > 0.0 ? o.joint_scale(s - 1) : 0.f) : o.by_error ? o.err_scale(s - 1, 0) : o.loss_scale(s - 1);
    const int has_input = s < n_fed, has_target = s >= 1 && scale != 0.f;
    float* out = fg.p + (long long)s * fg.tstride;
    const int acc = fg.tstride == 0;
    if (o.by_error)
        ew(st, tframe_grad_kernel<1>, B * CHW, (const float*)y.dE, (const float*)y.E_at(s, B), (const float*)y.P_at(s, B), d_frames + (long long)s * CHW, bstride, scale,
           has_input, has_target, CHW, (long long)B * CHW, out, fg.bstride, acc);
    else
        ew(st, tframe_grad_kernel<0>, B * CHW, (const float*)y.dE, (const float*)y.E_at(s, B), (const float*)y.P_at(s, B), d_frames + (long long)s * CHW, bstride, scale,
           has_input, has_target, CHW, (long long)B * CHW, out, fg.bstride, acc);
}

// every weight gradient over the tape's T * B samples: dV, the gates and ZA hold the deltas the backward steps left there
void weight_gradients(eigen_trainer* t, hipStream_t st, int T, int B)
{
    const int L = t->L, N = T * B;
    float* grd = t->grd;
    for (int l = 0; l < L; ++l) {
        const TLayer& y = t->ly[l];
        const LayerParams& p = t->lp[l];
        const long long CHW = y.CHW();
        const float *dV = y.dV_at(0, B), *G = y.G_at(0, B);
        wgrad(t, st, grd + p.pW, dV, y.C, y.H, y.W, N, src(y.h_at(1, B), CHW, y.C, 0, nullptr, 0));
        bias_grad(t, st, grd + p.pb, dV, y.C, y.HW, N);
        wgrad(t, st, grd + p.x0, G, 4 * y.C, y.H, y.W, N, src(y.E_at(0, B), 2 * CHW, 2 * y.C, 0, nullptr, 0));
        wgrad(t, st, grd + p.hW, G, 4 * y.C, y.H, y.W, N, src(y.h_at(0, B), CHW, y.C, 0, nullptr, 0));
        if (l < L - 1) {
            const TLayer& ya = t->ly[l + 1];
            wgrad(t, st, grd + p.x1, G, 4 * y.C, y.H, y.W, N, src(ya.h_at(1, B), ya.CHW(), ya.C, 1, nullptr, 0));
        }
        bias_grad(t, st, grd + p.hb, G, 4 * y.C, y.HW, N);
        ew(st, tpeep_grad_kernel, CHW, G, (const float*)y.c_at(0, B), y.C, (int)y.HW, N, grd + p.peep, grd + p.peep + CHW, grd + p.peep + 2 * CHW);
        if (l > 0) {
            const TLayer& yb = t->ly[l - 1];
            wgrad(t, st, grd + p.aW, y.ZA_at(0, B), y.C, yb.H, yb.W, N, src(yb.E_at(0, B), 2 * yb.CHW(), 2 * yb.C, 0, nullptr, 0));
            bias_grad(t, st, grd + p.ab, y.ZA_at(0, B), y.C, yb.HW, N);
        }
    }
}

// the table to h_layer_err and the loss to h_loss (either may be NULL); everything combined here is added in double, in order
int read_loss(eigen_trainer* t, hipStream_t st, const Objective& o, bool want_table, double* h_loss, double* h_layer_err)
{
    const int T = o.T, L = t->L;
    std::vector<double> tab(want_table ? (size_t)(T - 1) * L : 0);
    if (want_table) {
        TCHK(hipMemcpyAsync(tab.data(), t->d_err, tab.size() * 8, hipMemcpyDeviceToHost, st));
        TCHK(hipStreamSynchronize(st));
        if (h_layer_err) memcpy(h_layer_err, tab.data(), tab.size() * 8);
    }
    if (o.by_flow && T >= 2) {
        // sum_s w_s f_s / sum_s w_s in step order; a term of weight zero was not computed and is 0.0
        std::vector<double> f(T - 1);
        TCHK(hipMemcpyAsync(f.data(), t->d_step, (T - 1) * 8, hipMemcpyDeviceToHost, st));
        TCHK(hipStreamSynchronize(st));
        double acc = 0.0;
        for (int s = 0; s < T - 1; ++s) {
            if (o.weight(s) == 0.0) f[s] = 0.0;
            acc += o.weight(s) * f[s];
        }
        if (o.h_terms) memcpy(o.h_terms, f.data(), (T - 1) * 8);
        const double l_flow = acc / o.total_weight();
        double l_mse = 0.0;
        if (o.mu > 0.0) {
            // the squared error, combined as the "mse" call combines it below
            if (o.step_w) {
                std::vector<double> sl(T - 1);
                TCHK(hipMemcpyAsync(sl.data(), t->d_jstep, (T - 1) * 8, hipMemcpyDeviceToHost, st));
                TCHK(hipStreamSynchronize(st));
                double sq = 0.0;
                for (int s = 0; s < T - 1; ++s) sq += o.step_w[s] * sl[s];
                l_mse = sq / o.sum_w;
            } else {
                TCHK(hipMemcpyAsync(&l_mse, t->d_loss, 8, hipMemcpyDeviceToHost, st));
                TCHK(hipStreamSynchronize(st));
            }
        }
        if (o.h_parts) { o.h_parts[0] = l_flow; o.h_parts[1] = l_mse; }
        if (h_loss) {
            const double weighed = o.mu * l_mse;
            *h_loss = o.mu > 0.0 ? l_flow + weighed : l_flow;
        }
        return EIGEN_OK;
    }
    if (o.by_flow && o.h_parts) o.h_parts[0] = o.h_parts[1] = 0.0;  // fewer than two steps: no term
    if (!h_loss) return EIGEN_OK;
    if (o.by_error && T >= 2) {
        // sum_s w_s sum_l lambda_l err[s][l] / sum_s w_s, in (step, layer) order (train.combine_terms states the same sums)
        double acc = 0.0, tot = 0.0;
        for (int s = 0; s < T - 1; ++s) {
            double row = 0.0;
            for (int l = 0; l < L; ++l) row += o.lam[l] * tab[(size_t)s * L + l];
            const double w = o.step_w ? o.step_w[s] : 1.0;
            acc += w * row;
            tot += w;
        }
        *h_loss = acc / tot;
    } else if (o.step_w && T >= 2) {
        std::vector<double> sl(T - 1);
        TCHK(hipMemcpyAsync(sl.data(), t->d_step, (T - 1) * 8, hipMemcpyDeviceToHost, st));
        TCHK(hipStreamSynchronize(st));
        double acc = 0.0;
        for (int s = 0; s < T - 1; ++s) acc += o.step_w[s] * sl[s];
        *h_loss = acc / o.sum_w;
    } else {
        TCHK(hipMemcpyAsync(h_loss, t->d_loss, 8, hipMemcpyDeviceToHost, st));
        TCHK(hipStreamSynchronize(st));
    }
    return EIGEN_OK;
}

// Everything a training call takes: the arguments of the widest exported entry, eigen_trainer_loss_grad_flow_score.  An entry lists the
// leading members, which every entry has, names the others it takes, and leaves the rest at these defaults, which are what it implies.
struct LossGradCall {
    const uint8_t* d_frames; int64_t bstride; int32_t batch, n_steps, n_fed, requant, reset; double* h_loss; float* d_pred; void* stream;
    const double* h_step_w = nullptr;
    int32_t objective = EIGEN_OBJ_MSE;
    const double* h_layer_w = nullptr;
    double* h_layer_err = nullptr;
    FrameGrad fg;
    const eigen_flow_settings* flow = nullptr;
    const float* d_dir = nullptr;
    const uint8_t* d_mask = nullptr;
    double* h_terms = nullptr;
    int32_t pairing = EIGEN_FLOW_PAIR_FRAME;
    const eigen_flow_score* score = nullptr;
    const eigen_flow_structure_score* sscore = nullptr;
    const eigen_flow_members* members = nullptr;
    double* h_stats = nullptr;
    const eigen_dense_solve* solve = nullptr;
    const double* d_target = nullptr; int64_t t_bstride = 0, t_tstride = 0;
    const eigen_flow_joint* joint = nullptr;
};

// The training call behind every exported eigen_trainer_loss_grad* entry.  The order of the checks is the order of this function: the
// call's own arguments (check_call), the pairing, the frame gradient's strides, the objective with its weights, the flow settings; then
// the launches.  An entry that cannot state EIGEN_OBJ_FLOW's settings refuses that objective in its own body, ahead of all of these.
int loss_grad_call(eigen_trainer* t, const LossGradCall& c)
{
    int rc = check_call(t, c.d_frames, c.bstride, c.batch, c.n_steps, c.n_fed, c.requant, c.reset, t ? t->cfg.max_steps : 0);
    if (rc) return rc;
    if (c.pairing != EIGEN_FLOW_PAIR_FRAME && c.pairing != EIGEN_FLOW_PAIR_PREDICTION)
        return tfail(EIGEN_ERR_INVALID, "pairing %d is neither EIGEN_FLOW_PAIR_FRAME nor EIGEN_FLOW_PAIR_PREDICTION", c.pairing);
    if (c.pairing != EIGEN_FLOW_PAIR_FRAME && c.objective != EIGEN_OBJ_FLOW) return tfail(EIGEN_ERR_INVALID, "EIGEN_FLOW_PAIR_PREDICTION goes with EIGEN_OBJ_FLOW only");
    const int T = c.n_steps, B = c.batch;
    const long long C0HW = t->ly[0].CHW();
    const FrameGrad& fg = c.fg;
    if (fg.p) {
        if (fg.tstride != 0 && fg.tstride < C0HW)
            return tfail(EIGEN_ERR_INVALID, "g_tstride %lld is neither 0 (tied) nor at least a frame (%lld floats)", fg.tstride, C0HW);
        const long long extent = fg.tstride == 0 ? C0HW : (long long)(T - 1) * fg.tstride + C0HW;
        if (fg.bstride < extent) return tfail(EIGEN_ERR_INVALID, "g_bstride %lld is smaller than one sample's gradient (%lld floats)", fg.bstride, extent);
    }
    Objective o;
    const bool by_flow = c.objective == EIGEN_OBJ_FLOW;
    rc = check_flow_target(t->fw, c.d_target, c.t_bstride, c.t_tstride, T - 1, by_flow, c.d_dir, c.score, c.sscore, c.members, o.flow);
    if (rc) return rc;
    if (c.joint) {
        const double mu = c.joint->frame_weight;
        if (!std::isfinite(mu) || mu < 0.0) return tfail(EIGEN_ERR_INVALID, "frame_weight %g: must be finite and >= 0", mu);
        if (mu > 0.0 && !by_flow) return tfail(EIGEN_ERR_INVALID, "a frame weight goes with EIGEN_OBJ_FLOW only");
        rc = check_flow_valid(t->fw, c.joint->d_valid, c.joint->v_bstride, c.joint->v_tstride, T - 1, o.flow);
        if (rc) return rc;
        o.mu = mu; o.h_parts = c.joint->h_parts;
    }
    if (!by_flow && (c.flow || c.d_dir || c.d_mask)) return tfail(EIGEN_ERR_INVALID, "flow settings, direction and mask go with EIGEN_OBJ_FLOW only");
    if (!by_flow && c.score) return tfail(EIGEN_ERR_INVALID, "a flow score goes with EIGEN_OBJ_FLOW only");
    if (!by_flow && c.sscore) return tfail(EIGEN_ERR_INVALID, "a flow structure score goes with EIGEN_OBJ_FLOW only");
    if (!by_flow && c.members) return tfail(EIGEN_ERR_INVALID, "flow members go with EIGEN_OBJ_FLOW only");
    // the step and layer weights follow the same rules under every objective
    rc = make_objective(t, by_flow ? (int32_t)EIGEN_OBJ_MSE : c.objective, c.h_layer_w, c.h_step_w, T, B, o);
    if (rc) return rc;
    if (!by_flow && c.solve) return tfail(EIGEN_ERR_INVALID, "a dense solve goes with EIGEN_OBJ_FLOW only");
    if (by_flow) {
        FlowWork& fw = t->fw;
        eigd::DenseSolve solve;
        rc = eigd::dense_solve_check(c.solve, fw.it_force, fw.H, fw.W, solve);  // ahead of the mask's read-back and of every allocation
        if (rc) return rc;
        o.flow.set_solve(solve);
        rc = check_flow_on(fw.device, fw.HW, c.flow, c.d_dir, per_sample_mask(c.members) ? nullptr : c.d_mask, EIGEN_FLOW_MOVING_REFERENCE, o.flow);
        if (rc) return rc;
        o.flow.pair_pred = c.pairing == EIGEN_FLOW_PAIR_PREDICTION;
        // a frame is no reference under the prediction pairing: there is nothing the flag could move
        if (o.flow.pair_pred && o.flow.moving) return tfail(EIGEN_ERR_INVALID, "EIGEN_FLOW_PAIR_PREDICTION does not take EIGEN_FLOW_MOVING_REFERENCE");
        rc = check_flow_score(c.score, c.d_dir, o.flow);
        if (rc) return rc;
        rc = check_flow_struct(c.sscore, c.d_dir, o.flow);
        if (rc) return rc;
        if (c.score && c.sscore) return tfail(EIGEN_ERR_INVALID, "a flow score and a flow structure score do not go together");
        rc = check_flow_members(fw, c.members, c.d_mask, B, o.flow);
        if (rc) return rc;
        o.by_flow = true;
        o.h_terms = c.h_terms;
        if (c.h_stats && T >= 2 && (o.flow.by_score || o.flow.by_struct)) {
            rc = stats_workspace(fw);
            if (rc) return rc;
            o.keep_stats = true;
        }
        if (o.flow.iterated) {
            rc = iter_workspace(fw, o.flow.levels, o.flow.iters);
            if (rc) return rc;
        }
    }
    hipStream_t st = (hipStream_t)c.stream;
    rc = start_state(t, st, B, c.reset);
    if (rc) return rc;
    // forward with tape: step s reads state slot s, writes state slot s + 1 and tape slot s
    for (int s = 0; s < T; ++s)
        forward_step(t, st, B, s, s + 1, s, s < c.n_fed ? c.d_frames + s * C0HW : nullptr, c.bstride, c.requant, c.d_pred ? c.d_pred + s * C0HW : nullptr, T * C0HW);
    const bool want_table = T >= 2 && (c.h_layer_err || (o.by_error && c.h_loss));
    rc = reduce_losses(t, st, o, c.d_frames, c.bstride, want_table);
    if (rc) return rc;
    // backward through time, from zero carries
    for (int l = 0; l < t->L; ++l)
        for (float* a : {t->ly[l].dPn, t->ly[l].dhc, t->ly[l].dc}) TCHK(hipMemsetAsync(a, 0, B * t->ly[l].CHW() * 4, st));
    // the tied frame gradient starts from zero; only the C0 H W floats of every sample are touched, whatever g_bstride is
    for (int b = 0; fg.p && fg.tstride == 0 && b < B; ++b) TCHK(hipMemsetAsync(fg.p + b * fg.bstride, 0, C0HW * 4, st));
    // the records of the terms that are not computed read zero
    if (o.keep_stats) TCHK(hipMemsetAsync(t->fw.f_stats, 0, (size_t)(T - 1) * B * FLOW_REC * 8, st));
    for (int s = T - 1; s >= 0; --s) {
        rc = backward_step(t, st, o, s, c.d_frames, c.bstride, fg);
        if (rc) return rc;
        if (fg.p) frame_grad_step(t, st, o, s, c.n_fed, c.d_frames, c.bstride, fg);
    }
    weight_gradients(t, st, T, B);
    TCHK(hipGetLastError());
    t->state_batch = B;
    t->state_slot = T;
    if (o.keep_stats) {
        TCHK(hipMemcpyAsync(c.h_stats, t->fw.f_stats, (size_t)(T - 1) * B * FLOW_REC * 8, hipMemcpyDeviceToHost, st));
        TCHK(hipStreamSynchronize(st));
    }
    return read_loss(t, st, o, want_table, c.h_loss, c.h_layer_err);
}

// the evaluation behind eigen_trainer_evaluate and eigen_trainer_evaluate_err
int evaluate_call(eigen_trainer* t, const uint8_t* d_frames, int64_t bstride, int32_t batch, int32_t n_steps, int32_t n_fed, int32_t requant, int32_t reset,
                  double* h_step_loss, double* h_layer_err, float* d_pred, void* stream)
{
    int rc = check_call(t, d_frames, bstride, batch, n_steps, n_fed, requant, reset, -1);
    if (rc) return rc;
    const int T = n_steps, B = batch, M = t->cfg.max_steps, L = t->L;
    const long long C0HW = t->ly[0].CHW();
    hipStream_t st = (hipStream_t)stream;
    rc = start_state(t, st, B, reset);
    if (rc) return rc;
    // state slots 0 and 1 in turn, tape slot 0; the loss of step s goes to d_step[s % max_steps], read back whenever that table is
    // full.  Row r of the error table lives at d_err[r % max_steps]: its image-layer entry is reduced after step r, its upper entries
    // (E_l of step r + 1) after step r + 1, and the rows are read back once the table's last row, or the call's, is complete --
    // ahead of the image-layer entry that reuses row 0.
    auto flush = [&](double* host, const double* dev, int r, int width) {  // rows r - r % M .. r, once r is the table's last row or the call's
        if (r % M != M - 1 && r != T - 2) return hipSuccess;
        return hipMemcpyAsync(host + (long long)(r - r % M) * width, dev, (long long)(r % M + 1) * width * 8, hipMemcpyDeviceToHost, st);
    };
    for (int s = 0; s < T; ++s) {
        const int in = s & 1, out = in ^ 1;
        forward_step(t, st, B, in, out, 0, s < n_fed ? d_frames + s * C0HW : nullptr, bstride, requant, d_pred ? d_pred + s * C0HW : nullptr, T * C0HW);
        const float* P0 = t->ly[0].P_at(out, B);
        const uint8_t* next = d_frames + (s + 1) * C0HW;  // the frame P0 predicts (read only while s < T - 1)
        if (h_layer_err && s >= 1) {
            upper_errors(t, st, 0, 1, B, t->d_err + (long long)((s - 1) % M) * L);
            TCHK(flush(h_layer_err, t->d_err, s - 1, L));
        }
        if (h_layer_err && s < T - 1) reduce_steps(TERM_ABS, t, st, P0, next, bstride, C0HW, 1, B, (double)(B * 2 * C0HW), t->d_err + (long long)(s % M) * L, L);
        if (s < T - 1) reduce_steps(TERM_SQ, t, st, P0, next, bstride, C0HW, 1, B, (double)(B * C0HW), t->d_step + s % M, 1);
        if (s < T - 1 && h_step_loss) TCHK(flush(h_step_loss, t->d_step, s, 1));
    }
    TCHK(hipGetLastError());
    t->state_batch = B;
    t->state_slot = T & 1;
    if (h_step_loss || h_layer_err) TCHK(hipStreamSynchronize(st));
    return EIGEN_OK;
}

// what eigen_trainer_adam accepts, and its refusal
bool adam_values_ok(double alpha, double beta1, double beta2, double eps) { return alpha > 0 && beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1 && eps > 0; }
int refuse_adam_values() { return tfail(EIGEN_ERR_INVALID, "Adam needs alpha > 0, 0 <= beta1, beta2 < 1 and eps > 0"); }

// the one launch of eigen_trainer_adam: the step count advances, tadam_kernel runs on the gradient table
void plain_adam(eigen_trainer* t, double alpha, double beta1, double beta2, double eps, hipStream_t st)
{
    const int step = ++t->adam_t;
    const double lr_t = alpha * std::sqrt(1.0 - std::pow(beta2, step)) / (1.0 - std::pow(beta1, step));
    ew(st, tadam_kernel, t->n_params, t->prm, t->mom, t->var, (const float*)t->grd, t->n_params, (float)lr_t, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps);
}

// the sums of squares of every tensor of the gradient table into o_sumsq and the global norm into o_norm, on the device
void grad_norms(eigen_trainer* t, hipStream_t st)
{
    hipLaunchKernelGGL(tgrad_sumsq_kernel, dim3(NORM_SLICES, (unsigned)t->n_tensors), dim3(EW_T), 0, st, (const float*)t->grd, (const long long*)t->o_tab, t->o_part);
    hipLaunchKernelGGL(tgrad_norm_final_kernel, dim3(1), dim3(NORM_FINAL_T), 0, st, (const double*)t->o_part, NORM_SLICES, t->n_tensors, t->o_sumsq, t->o_norm);
}

// The gradient accumulator, n_params floats, made by the first call that adds to it and freed with the handle; eigen_trainer_tape_bytes
// does not count it
int accumulator(eigen_trainer* t)
{
    if (t->acc) return EIGEN_OK;
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, (size_t)t->n_params * 4);
    if (e != hipSuccess) return tfail(EIGEN_ERR_HIP, "hipMalloc(%lld): %s", t->n_params * 4, hipGetErrorString(e));
    t->acc = (float*)p;
    t->allocs.push_back(p);
    return EIGEN_OK;
}

// EIGEN_OBJ_FLOW through an entry that has nowhere to take the flow settings from
int refuse_flow_objective() { return tfail(EIGEN_ERR_INVALID, "EIGEN_OBJ_FLOW needs the settings eigen_trainer_loss_grad_flow takes"); }

// What the eigen_trainer_loss_grad_* entries share beyond the leading members: the objective with its weights and where the frame gradient
// goes (null: not wanted),
void set_objective(LossGradCall& c, const double* h_step_w, int32_t objective, const double* h_layer_w, double* h_layer_err, float* d_frame_grad = nullptr,
                   int64_t g_bstride = 0, int64_t g_tstride = 0)
{
    c.h_step_w = h_step_w; c.objective = objective; c.h_layer_w = h_layer_w; c.h_layer_err = h_layer_err;
    c.fg.p = d_frame_grad; c.fg.bstride = g_bstride; c.fg.tstride = g_tstride;
}

// and the flow settings
void set_flow(LossGradCall& c, const eigen_flow_settings* flow, const float* d_dir, const uint8_t* d_mask, double* h_terms, int32_t pairing = EIGEN_FLOW_PAIR_FRAME)
{
    c.flow = flow; c.d_dir = d_dir; c.d_mask = d_mask; c.h_terms = h_terms; c.pairing = pairing;
}

// The stage-alone call on a handle's work record, through the handle's step partials and step value.  A null handle is the first of
// flow_term_call's "null argument" refusals.
int flow_term(eigen_trainer* t, const FlowTermCall& c)
{
    if (!t) return tfail(EIGEN_ERR_INVALID, "null argument");
    return flow_term_call(t->fw, c, t->d_spart, t->d_step);
}

// what the stage-alone entries with a solve refuse ahead of the shared call
int refuse_solve_term(const uint8_t* d_ref, const float* d_fref, const eigen_flow_score* score, const eigen_flow_structure_score* sscore, const eigen_flow_members* members)
{
    if ((d_ref != nullptr) == (d_fref != nullptr)) return tfail(EIGEN_ERR_INVALID, "exactly one of the byte and the float reference must be given");
    if (members && !score && !sscore) return tfail(EIGEN_ERR_INVALID, "flow members need a score: the displacement modes divide by the shared mask's count");
    if (score && sscore) return tfail(EIGEN_ERR_INVALID, "a flow score and a flow structure score do not go together");
    return EIGEN_OK;
}

}  // namespace

extern "C" {

int eigen_trainer_destroy(eigen_trainer* t)
{
    if (!t) return EIGEN_OK;
    (void)hipSetDevice(t->cfg.device);
    for (void* p : t->allocs) (void)hipFree(p);
    delete t;
    return EIGEN_OK;
}

int eigen_trainer_create(const eigen_trainer_config* cfg, eigen_trainer** out)
{
    if (!cfg || !out) return tfail(EIGEN_ERR_INVALID, "null argument");
    *out = nullptr;
    const int L = cfg->n_layers;
    if (L < 1 || L > EIGEN_MAX_LAYERS) return tfail(EIGEN_ERR_INVALID, "n_layers %d out of range", L);
    if (cfg->width < 1 || cfg->height < 1 || cfg->width % (1 << (L - 1)) || cfg->height % (1 << (L - 1)))
        return tfail(EIGEN_ERR_INVALID, "image %dx%d must be divisible by 2^(layers-1)=%d", cfg->width, cfg->height, 1 << (L - 1));
    if (cfg->channels[0] != 1 && cfg->channels[0] != 3) return tfail(EIGEN_ERR_INVALID, "channels[0] must be 1 or 3");
    for (int l = 0; l < L; ++l) if (cfg->channels[l] < 1) return tfail(EIGEN_ERR_INVALID, "channels[%d] < 1", l);
    if (cfg->max_batch < 1 || cfg->max_steps < 2) return tfail(EIGEN_ERR_INVALID, "max_batch >= 1 and max_steps >= 2 required");
    TCHK(hipSetDevice(cfg->device));
    hipDeviceProp_t prop;
    TCHK(hipGetDeviceProperties(&prop, cfg->device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return tfail(EIGEN_ERR_INVALID, "device %d is %s; this library is built for gfx950 (MI355X) only", cfg->device, prop.gcnArchName);
    eigen_trainer* t = new eigen_trainer();
    t->cfg = *cfg;
    t->L = L;
    plan_layout(t);
    const int rc = allocate(t);
    if (rc) eigen_trainer_destroy(t);
    else *out = t;
    return rc;
}

int64_t eigen_trainer_tape_bytes(const eigen_trainer* t) { return t ? t->tape_bytes : 0; }

int eigen_trainer_set_weights(eigen_trainer* t, const float* const* h_tensors, int32_t n_tensors)
{
    if (!t || !h_tensors) return tfail(EIGEN_ERR_INVALID, "null argument");
    int rc = copy_tables(t, n_tensors, true, t->prm, h_tensors);
    if (rc) return rc;
    TCHK(hipMemset(t->mom, 0, t->n_params * 4));
    TCHK(hipMemset(t->var, 0, t->n_params * 4));
    TCHK(hipDeviceSynchronize());
    t->have_weights = true;
    t->adam_t = 0;
    t->state_batch = 0;
    t->acc_count = 0;
    return EIGEN_OK;
}

int eigen_trainer_get_weights(eigen_trainer* t, float* const* h_tensors, int32_t n_tensors)
{
    if (!t || !h_tensors) return tfail(EIGEN_ERR_INVALID, "null argument");
    if (!t->have_weights) return tfail(EIGEN_ERR_STATE, "eigen_trainer_set_weights has not been called");
    return copy_tables(t, n_tensors, false, t->prm, h_tensors);
}

int eigen_trainer_get_grads(eigen_trainer* t, float* const* h_tensors, int32_t n_tensors)
{
    return copy_tables(t, n_tensors, false, t->grd, h_tensors);
}

int eigen_trainer_loss_grad_flow_pair(eigen_trainer* t, const uint8_t* d_frames, int64_t bstride, int32_t batch, int32_t n_steps, int32_t n_fed,
                                      int32_t requant, int32_t reset, const double* h_step_w, int32_t objective, const double* h_layer_w, double* h_loss,
                                      double* h_layer_err, float* d_pred, float* d_frame_grad, int64_t g_bstride, int64_t g_tstride,
                                      const eigen_flow_settings* flow, const float* d_dir, const uint8_t* d_mask, double* h_terms, int32_t pairing, void* stream)
{
    LossGradCall c{d_frames, bstride, batch, n_steps, n_fed, requant, reset, h_loss, d_pred, stream};
    set_objective(c, h_step_w, objective, h_layer_w, h_layer_err, d_frame_grad, g_bstride, g_tstride);
    set_flow(c, flow, d_dir, d_mask, h_terms, pairing);
    return loss_grad_call(t, c);
}

int eigen_trainer_loss_grad_flow_score(eigen_trainer* t, const uint8_t* d_frames, int64_t bstride, int32_t batch, int32_t n_steps, int32_t n_fed,
                                       int32_t requant, int32_t reset, const double* h_step_w, int32_t objective, const double* h_layer_w, double* h_loss,
                                       double* h_layer_err, float* d_pred, float* d_frame_grad, int64_t g_bstride, int64_t g_tstride,
                                       const eigen_flow_settings* flow, const float* d_dir, const uint8_t* d_mask, double* h_terms, int32_t pairing,
                                       const eigen_flow_score* score, void* stream)
{
    LossGradCall c{d_frames, bstride, batch, n_steps, n_fed, requant, reset, h_loss, d_pred, stream};
    set_objective(c, h_step_w, objective, h_layer_w, h_layer_err, d_frame_grad, g_bstride, g_tstride);
    set_flow(c, flow, d_dir, d_mask, h_terms, pairing);
    c.score = score;
    return loss_grad_call(t, c);
}

int eigen_trainer_loss_grad_flow(eigen_trainer* t, const uint8_t* d_frames, int64_t bstride, int32_t batch, int32_t n_steps, int32_t n_fed,
                                 int32_t requant, int32_t reset, const double* h_step_w, int32_t objective, const double* h_layer_w, double* h_loss,
                                 double* h_layer_err, float* d_pred, float* d_frame_grad, int64_t g_bstride, int64_t g_tstride, const eigen_flow_settings* flow,
                                 const float* d_dir, const uint8_t* d_mask, double* h_terms, void* stream)
{
    LossGradCall c{d_frames, bstride, batch, n_steps, n_fed, requant, reset, h_loss, d_pred, stream};
    set_objective(c, h_step_w, objective, h_layer_w, h_layer_err, d_frame_grad, g_bstride, g_tstride);
    set_flow(c, flow, d_dir, d_mask, h_terms);
    return loss_grad_call(t, c);
}

int eigen_trainer_loss_grad_frames(eigen_trainer* t, const uint8_t* d_frames, int64_t bstride, int32_t batch, int32_t n_steps, int32_t n_fed,
                                   int32_t requant, int32_t reset, const double* h_step_w, int32_t objective, const double* h_layer_w, double* h_loss,
                                   double* h_layer_err, float* d_pred, float* d_frame_grad, int64_t g_bstride, int64_t g_tstride, void* stream)
{
    if (objective == EIGEN_OBJ_FLOW) return refuse_flow_objective();
    LossGradCall c{d_frames, bstride, batch, n_steps, n_fed, requant, reset, h_loss, d_pred, stream};
    set_objective(c, h_step_w, objective, h_layer_w, h_layer_err, d_frame_grad, g_bstride, g_tstride);
    return loss_grad_call(t, c);
}

int eigen_trainer_flow_term(eigen_trainer* t, const float* d_pred, int64_t p_bstride, const uint8_t* d_ref, int64_t r_bstride, int32_t batch,
                            const eigen_flow_settings* flow, const float* d_dir, const uint8_t* d_mask, double scale, double* h_value, double* d_flow,
                            float* d_seed, int64_t s_bstride, void* stream)
{
    FlowTermCall c{d_pred, p_bstride, r_bstride, batch, flow, d_mask, scale, h_value, d_flow, d_seed, s_bstride, stream};
    c.d_ref = d_ref; c.d_dir = d_dir;
    return flow_term(t, c);
}

int eigen_trainer_flow_term_ref(eigen_trainer* t, const float* d_pred, int64_t p_bstride, const uint8_t* d_ref, int64_t r_bstride, int32_t batch,
                                const eigen_flow_settings* flow, const float* d_dir, const uint8_t* d_mask, double scale, double* h_value, double* d_flow,
                                float* d_seed, int64_t s_bstride, float* d_ref_grad, int64_t rg_bstride, void* stream)
{
    if (!d_ref_grad) return tfail(EIGEN_ERR_INVALID, "null argument");
    FlowTermCall c{d_pred, p_bstride, r_bstride, batch, flow, d_mask, scale, h_value, d_flow, d_seed, s_bstride, stream};
    c.d_ref = d_ref; c.d_dir = d_dir; c.d_refg = d_ref_grad; c.rg_bstride = rg_bstride;
    return flow_term(t, c);
}

int eigen_trainer_flow_term_pair(eigen_trainer* t, const float* d_pred, int64_t p_bstride, const float* d_prev, int64_t r_bstride, int32_t batch,
                                 const eigen_flow_settings* flow, const float* d_dir, const uint8_t* d_mask, double scale, double* h_value, double* d_flow,
                                 float* d_seed, int64_t s_bstride, float* d_prev_grad, int64_t pg_bstride, void* stream)
{
    if (!d_prev) return tfail(EIGEN_ERR_INVALID, "null argument");
    FlowTermCall c{d_pred, p_bstride, r_bstride, batch, flow, d_mask, scale, h_value, d_flow, d_seed, s_bstride, stream};
    c.d_fref = d_prev; c.d_dir = d_dir; c.d_refg = d_prev_grad; c.rg_bstride = pg_bstride;
    return flow_term(t, c);
}

int eigen_trainer_flow_term_score(eigen_trainer* t, const float* d_pred, int64_t p_bstride, const uint8_t* d_ref, const float* d_fref, int64_t r_bstride,
                                  int32_t batch, const eigen_flow_settings* flow, const uint8_t* d_mask, const eigen_flow_score* score, double scale,
                                  double* h_value, double* h_stats, double* d_flow, float* d_seed, int64_t s_bstride, float* d_ref_grad, int64_t rg_bstride,
                                  void* stream)
{
    if (!score) return tfail(EIGEN_ERR_INVALID, "null argument");
    if ((d_ref != nullptr) == (d_fref != nullptr)) return tfail(EIGEN_ERR_INVALID, "exactly one of the byte and the float reference must be given");
    FlowTermCall c{d_pred, p_bstride, r_bstride, batch, flow, d_mask, scale, h_value, d_flow, d_seed, s_bstride, stream};
    c.d_ref = d_ref; c.d_fref = d_fref; c.d_refg = d_ref_grad; c.rg_bstride = rg_bstride; c.score = score; c.h_stats = h_stats;
    return flow_term(t, c);
}

int eigen_trainer_flow_term_structure(eigen_trainer* t, const float* d_pred, int64_t p_bstride, const uint8_t* d_ref, const float* d_fref, int64_t r_bstride,
                                      int32_t batch, const eigen_flow_settings* flow, const uint8_t* d_mask, const eigen_flow_structure_score* score, double scale,
                                      double* h_value, double* h_stats, double* d_flow, float* d_seed, int64_t s_bstride, float* d_ref_grad, int64_t rg_bstride,
                                      void* stream)
{
    if (!score) return tfail(EIGEN_ERR_INVALID, "null argument");
    if ((d_ref != nullptr) == (d_fref != nullptr)) return tfail(EIGEN_ERR_INVALID, "exactly one of the byte and the float reference must be given");
    FlowTermCall c{d_pred, p_bstride, r_bstride, batch, flow, d_mask, scale, h_value, d_flow, d_seed, s_bstride, stream};
    c.d_ref = d_ref; c.d_fref = d_fref; c.d_refg = d_ref_grad; c.rg_bstride = rg_bstride; c.sscore = score; c.h_stats = h_stats;
    return flow_term(t, c);
}

int eigen_trainer_flow_term_members(eigen_trainer* t, const float* d_pred, int64_t p_bstride, const uint8_t* d_ref, const float* d_fref, int64_t r_bstride,
                                    int32_t batch, const eigen_flow_settings* flow, const uint8_t* d_mask, const eigen_flow_score* score,
                                    const eigen_flow_structure_score* sscore, const eigen_flow_members* members, double scale, double* h_value, double* h_stats,
                                    double* d_flow, float* d_seed, int64_t s_bstride, float* d_ref_grad, int64_t rg_bstride, void* stream)
{
    if ((d_ref != nullptr) == (d_fref != nullptr)) return tfail(EIGEN_ERR_INVALID, "exactly one of the byte and the float reference must be given");
    if (members && !score && !sscore) return tfail(EIGEN_ERR_INVALID, "flow members need a score: the displacement modes divide by the shared mask's count");
    if ((score != nullptr) == (sscore != nullptr)) return tfail(EIGEN_ERR_INVALID, "exactly one of the flow score and the flow structure score must be given");
    FlowTermCall c{d_pred, p_bstride, r_bstride, batch, flow, d_mask, scale, h_value, d_flow, d_seed, s_bstride, stream};
    c.d_ref = d_ref; c.d_fref = d_fref; c.d_refg = d_ref_grad; c.rg_bstride = rg_bstride; c.score = score; c.sscore = sscore; c.members = members; c.h_stats = h_stats;
    return flow_term(t, c);
}

int eigen_trainer_flow_members(eigen_trainer* t, const uint8_t* d_ref, const float* d_fref, int64_t r_bstride, int32_t batch, const eigen_flow_members* members,
                               const uint8_t* d_mask, uint8_t* h_members, int32_t* h_counts, void* stream)
{
    if (!t || !members) return tfail(EIGEN_ERR_INVALID, "null argument");
    if ((d_ref != nullptr) == (d_fref != nullptr)) return tfail(EIGEN_ERR_INVALID, "exactly one of the byte and the float reference must be given");
    if (batch < 1) return tfail(EIGEN_ERR_INVALID, "batch >= 1 required");
    if (batch > t->cfg.max_batch) return tfail(EIGEN_ERR_CAPACITY, "batch %d exceeds the trainer's %d", batch, t->cfg.max_batch);
    if (r_bstride < t->ly[0].CHW()) return tfail(EIGEN_ERR_INVALID, "r_bstride %lld is smaller than one image (%lld elements)", (long long)r_bstride, t->ly[0].CHW());
    if (members->kind != EIGEN_FLOW_MEMBERS_CORNERS) return tfail(EIGEN_ERR_INVALID, "flow members: kind %d: this entry derives EIGEN_FLOW_MEMBERS_CORNERS", members->kind);
    return flow_members_call(t->fw, d_ref, d_fref, r_bstride, batch, members, d_mask, h_members, h_counts, stream);
}

int eigen_trainer_loss_grad_flow_members(eigen_trainer* t, const uint8_t* d_frames, int64_t bstride, int32_t batch, int32_t n_steps, int32_t n_fed,
                                         int32_t requant, int32_t reset, const double* h_step_w, int32_t objective, const double* h_layer_w, double* h_loss,
                                         double* h_layer_err, float* d_pred, float* d_frame_grad, int64_t g_bstride, int64_t g_tstride,
                                         const eigen_flow_settings* flow, const float* d_dir, const uint8_t* d_mask, double* h_terms, int32_t pairing,
                                         const eigen_flow_score* score, const eigen_flow_structure_score* sscore, const eigen_flow_members* members,
                                         double* h_stats, void* stream)
{
    LossGradCall c{d_frames, bstride, batch, n_steps, n_fed, requant, reset, h_loss, d_pred, stream};
    set_objective(c, h_step_w, objective, h_layer_w, h_layer_err, d_frame_grad, g_bstride, g_tstride);
    set_flow(c, flow, d_dir, d_mask, h_terms, pairing);
    c.score = score; c.sscore = sscore;
    c.members = members; c.h_stats = h_stats;
    return loss_grad_call(t, c);
}

int eigen_trainer_debug_free_planes(eigen_trainer* t, int32_t batch, double* h_theta, double* h_L, int32_t* h_rowS, int32_t* h_colS, uint8_t* h_flag, void* stream)
{
    if (!t) return tfail(EIGEN_ERR_INVALID, "null argument");
    if (batch < 1 || batch > t->cfg.max_batch) return tfail(EIGEN_ERR_INVALID, "batch %d outside 1 .. %d", batch, t->cfg.max_batch);
    TCHK(hipSetDevice(t->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)batch * t->ly[0].HW;
    if (h_theta) TCHK(hipMemcpyAsync(h_theta, t->fw.f_theta, n * 8, hipMemcpyDeviceToHost, st));
    if (h_L) TCHK(hipMemcpyAsync(h_L, t->fw.f_L, n * 8, hipMemcpyDeviceToHost, st));
    if (h_rowS) TCHK(hipMemcpyAsync(h_rowS, t->fw.f_rowS, n * 4, hipMemcpyDeviceToHost, st));
    if (h_colS) TCHK(hipMemcpyAsync(h_colS, t->fw.f_colS, n * 4, hipMemcpyDeviceToHost, st));
    if (h_flag) TCHK(hipMemcpyAsync(h_flag, t->fw.f_flag, n, hipMemcpyDeviceToHost, st));
    TCHK(hipStreamSynchronize(st));
    return EIGEN_OK;
}

int eigen_trainer_loss_grad_flow_structure(eigen_trainer* t, const uint8_t* d_frames, int64_t bstride, int32_t batch, int32_t n_steps, int32_t n_fed,
                                           int32_t requant, int32_t reset, const double* h_step_w, int32_t objective, const double* h_layer_w, double* h_loss,
                                           double* h_layer_err, float* d_pred, float* d_frame_grad, int64_t g_bstride, int64_t g_tstride,
                                           const eigen_flow_settings* flow, const float* d_dir, const uint8_t* d_mask, double* h_terms, int32_t pairing,
                                           const eigen_flow_structure_score* score, void* stream)
{
    LossGradCall c{d_frames, bstride, batch, n_steps, n_fed, requant, reset, h_loss, d_pred, stream};
    set_objective(c, h_step_w, objective, h_layer_w, h_layer_err, d_frame_grad, g_bstride, g_tstride);
    set_flow(c, flow, d_dir, d_mask, h_terms, pairing);
    c.sscore = score;
    return loss_grad_call(t, c);
}

int eigen_trainer_loss_grad_obj(eigen_trainer* t, const uint8_t* d_frames, int64_t bstride, int32_t batch, int32_t n_steps, int32_t n_fed,
                                int32_t requant, int32_t reset, const double* h_step_w, int32_t objective, const double* h_layer_w, double* h_loss,
                                double* h_layer_err, float* d_pred, void* stream)
{
    if (objective == EIGEN_OBJ_FLOW) return refuse_flow_objective();
    LossGradCall c{d_frames, bstride, batch, n_steps, n_fed, requant, reset, h_loss, d_pred, stream};
    set_objective(c, h_step_w, objective, h_layer_w, h_layer_err);
    return loss_grad_call(t, c);
}

int eigen_trainer_still_step(eigen_trainer* t, uint8_t* d_images, const float* d_grad, int64_t g_bstride, const uint8_t* d_mask, double step_bytes,
                             int32_t batch, void* stream)
{
    if (!t || !d_images || !d_grad) return tfail(EIGEN_ERR_INVALID, "null argument");
    if (!std::isfinite(step_bytes) || !(step_bytes > 0.0)) return tfail(EIGEN_ERR_INVALID, "step_bytes %g: the step must be finite and > 0", step_bytes);
    if (batch < 1) return tfail(EIGEN_ERR_INVALID, "batch >= 1 required");
    if (batch > t->cfg.max_batch) return tfail(EIGEN_ERR_CAPACITY, "batch %d exceeds the trainer's %d", batch, t->cfg.max_batch);
    const TLayer& y = t->ly[0];
    const long long C0HW = y.CHW();
    if (g_bstride < C0HW) return tfail(EIGEN_ERR_INVALID, "g_bstride %lld is smaller than one image (%lld floats)", (long long)g_bstride, C0HW);
    TCHK(hipSetDevice(t->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    const float k = (float)(step_bytes / 255.0);
    hipLaunchKernelGGL(tstill_absmax_kernel, dim3(batch), dim3(EW_T), 0, st, d_grad, (long long)g_bstride, d_mask, (int)y.HW, C0HW, t->d_absmax);
    ew(st, tstill_step_kernel, batch * C0HW, d_images, d_grad, (long long)g_bstride, d_mask, (const float*)t->d_absmax, k, (int)y.HW, C0HW, (long long)batch * C0HW);
    TCHK(hipGetLastError());
    return EIGEN_OK;
}

int eigen_trainer_loss_grad_ext(eigen_trainer* t, const uint8_t* d_frames, int64_t bstride, int32_t batch, int32_t n_steps, int32_t n_fed,
                                int32_t requant, int32_t reset, const double* h_step_w, double* h_loss, float* d_pred, void* stream)
{
    LossGradCall c{d_frames, bstride, batch, n_steps, n_fed, requant, reset, h_loss, d_pred, stream};
    c.h_step_w = h_step_w;
    return loss_grad_call(t, c);
}

int eigen_trainer_loss_grad(eigen_trainer* t, const uint8_t* d_frames, int64_t bstride, int32_t batch, int32_t n_steps,
                            int32_t reset, double* h_loss, float* d_pred, void* stream)
{
    return loss_grad_call(t, LossGradCall{d_frames, bstride, batch, n_steps, n_steps, 0, reset, h_loss, d_pred, stream});
}

int eigen_trainer_evaluate_err(eigen_trainer* t, const uint8_t* d_frames, int64_t bstride, int32_t batch, int32_t n_steps, int32_t n_fed,
                               int32_t requant, int32_t reset, double* h_step_loss, double* h_layer_err, float* d_pred, void* stream)
{
    return evaluate_call(t, d_frames, bstride, batch, n_steps, n_fed, requant, reset, h_step_loss, h_layer_err, d_pred, stream);
}

int eigen_trainer_evaluate(eigen_trainer* t, const uint8_t* d_frames, int64_t bstride, int32_t batch, int32_t n_steps, int32_t n_fed,
                           int32_t requant, int32_t reset, double* h_step_loss, float* d_pred, void* stream)
{
    return evaluate_call(t, d_frames, bstride, batch, n_steps, n_fed, requant, reset, h_step_loss, nullptr, d_pred, stream);
}

// Adam moments, step count and the kept sequence state, out.  h_m / h_v: host tables in eigen_set_prednet_weights order (both or
// neither); h_seq: 3 * n_layers host arrays (h, c, P of layer 0, then of layer 1, ...), each [*seq_batch][C_l][H_l][W_l].
int eigen_trainer_get_state(eigen_trainer* t, float* const* h_m, float* const* h_v, int32_t n_tensors, int32_t* adam_t, int32_t* seq_batch, float* const* h_seq, int32_t n_seq)
{
    if (!t) return tfail(EIGEN_ERR_INVALID, "null argument");
    if (!t->have_weights) return tfail(EIGEN_ERR_STATE, "eigen_trainer_set_weights has not been called");
    if ((h_m == nullptr) != (h_v == nullptr)) return tfail(EIGEN_ERR_INVALID, "h_m and h_v go together");
    if (h_seq && n_seq != 3 * t->L) return tfail(EIGEN_ERR_INVALID, "expected %d state arrays for %d layers, got %d", 3 * t->L, t->L, n_seq);
    const int rc = h_m ? copy_tables(t, n_tensors, false, t->mom, h_m, t->var, h_v) : EIGEN_OK;
    if (rc) return rc;
    if (adam_t) *adam_t = t->adam_t;
    if (seq_batch) *seq_batch = t->state_batch;
    if (h_seq && t->state_batch > 0) {
        TCHK(hipSetDevice(t->cfg.device));
        TCHK(hipDeviceSynchronize());
        for (int i = 0; i < 3 * t->L; ++i) {
            const TLayer& y = t->ly[i / 3];
            if (!h_seq[i]) return tfail(EIGEN_ERR_INVALID, "state array %d is NULL", i);
            TCHK(hipMemcpy(h_seq[i], y.state_at(i % 3, t->state_slot, t->state_batch), (long long)t->state_batch * y.CHW() * 4, hipMemcpyDeviceToHost));
        }
    }
    return EIGEN_OK;
}

int eigen_trainer_set_state(eigen_trainer* t, const float* const* h_m, const float* const* h_v, int32_t n_tensors, int32_t adam_t, int32_t seq_batch,
                            const float* const* h_seq, int32_t n_seq)
{
    if (!t || !h_m || !h_v) return tfail(EIGEN_ERR_INVALID, "null argument");
    if (!t->have_weights) return tfail(EIGEN_ERR_STATE, "eigen_trainer_set_weights has not been called");
    if (adam_t < 0) return tfail(EIGEN_ERR_INVALID, "adam_t %d < 0", adam_t);
    if (seq_batch < 0) return tfail(EIGEN_ERR_INVALID, "seq_batch %d < 0", seq_batch);
    if (seq_batch > t->cfg.max_batch) return tfail(EIGEN_ERR_CAPACITY, "seq_batch %d exceeds the trainer's %d", seq_batch, t->cfg.max_batch);
    if (seq_batch > 0) {
        if (!h_seq) return tfail(EIGEN_ERR_INVALID, "seq_batch %d without state arrays", seq_batch);
        if (n_seq != 3 * t->L) return tfail(EIGEN_ERR_INVALID, "expected %d state arrays for %d layers, got %d", 3 * t->L, t->L, n_seq);
        for (int i = 0; i < n_seq; ++i) if (!h_seq[i]) return tfail(EIGEN_ERR_INVALID, "state array %d is NULL", i);
    }
    const int rc = copy_tables(t, n_tensors, true, t->mom, h_m, t->var, h_v);
    if (rc) return rc;
    t->adam_t = adam_t;
    t->state_batch = t->state_slot = 0;
    for (int i = 0; seq_batch > 0 && i < 3 * t->L; ++i) {
        const TLayer& y = t->ly[i / 3];
        TCHK(hipMemcpy(y.state_at(i % 3, 0, seq_batch), h_seq[i], (long long)seq_batch * y.CHW() * 4, hipMemcpyHostToDevice));
    }
    t->state_batch = seq_batch;
    return EIGEN_OK;
}

int eigen_trainer_adam(eigen_trainer* t, double alpha, double beta1, double beta2, double eps, void* stream)
{
    if (!t) return tfail(EIGEN_ERR_INVALID, "null argument");
    if (!t->have_weights) return tfail(EIGEN_ERR_STATE, "eigen_trainer_set_weights has not been called");
    if (!adam_values_ok(alpha, beta1, beta2, eps)) return refuse_adam_values();
    TCHK(hipSetDevice(t->cfg.device));
    plain_adam(t, alpha, beta1, beta2, eps, (hipStream_t)stream);
    TCHK(hipGetLastError());
    return EIGEN_OK;
}

int eigen_trainer_grad_norms(eigen_trainer* t, double* h_global, double* h_per_tensor, int32_t n_tensors, void* stream)
{
    if (!t) return tfail(EIGEN_ERR_INVALID, "null argument");
    if (n_tensors != t->n_tensors) return tfail(EIGEN_ERR_INVALID, "expected %d weight tensors for %d layers, got %d", t->n_tensors, t->L, n_tensors);
    if (!t->have_weights) return tfail(EIGEN_ERR_STATE, "eigen_trainer_set_weights has not been called");
    TCHK(hipSetDevice(t->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    grad_norms(t, st);
    TCHK(hipGetLastError());
    std::vector<double> sq(h_per_tensor ? t->n_tensors : 0);
    if (h_per_tensor) TCHK(hipMemcpyAsync(sq.data(), t->o_sumsq, sq.size() * 8, hipMemcpyDeviceToHost, st));
    if (h_global) TCHK(hipMemcpyAsync(h_global, t->o_norm, 8, hipMemcpyDeviceToHost, st));
    if (h_per_tensor || h_global) TCHK(hipStreamSynchronize(st));
    for (size_t k = 0; k < sq.size(); ++k) h_per_tensor[k] = std::sqrt(sq[k]);
    return EIGEN_OK;
}

int eigen_trainer_adam_ex(eigen_trainer* t, const eigen_adam_settings* s, eigen_adam_report* h_report, void* stream)
{
    if (!t || !s) return tfail(EIGEN_ERR_INVALID, "null argument");
    if (!adam_values_ok(s->alpha, s->beta1, s->beta2, s->eps)) return refuse_adam_values();
    if (!(std::isfinite(s->weight_decay) && s->weight_decay >= 0) || !(std::isfinite(s->clip_norm) && s->clip_norm >= 0))
        return tfail(EIGEN_ERR_INVALID, "weight_decay and clip_norm must be finite and >= 0 (0: off)");
    if ((s->skip_nonfinite != 0 && s->skip_nonfinite != 1) || s->reserved != 0) return tfail(EIGEN_ERR_INVALID, "skip_nonfinite must be 0 or 1 and reserved 0");
    if (!t->have_weights) return tfail(EIGEN_ERR_STATE, "eigen_trainer_set_weights has not been called");
    TCHK(hipSetDevice(t->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    if (s->weight_decay == 0 && s->clip_norm == 0 && !s->skip_nonfinite && !h_report) {
        plain_adam(t, s->alpha, s->beta1, s->beta2, s->eps, st);   // eigen_trainer_adam's launch, hence its bits
        TCHK(hipGetLastError());
        return EIGEN_OK;
    }
    grad_norms(t, st);
    TCHK(hipGetLastError());
    double norm = 0.0;
    if (s->skip_nonfinite) {
        TCHK(hipMemcpyAsync(&norm, t->o_norm, 8, hipMemcpyDeviceToHost, st));
        TCHK(hipStreamSynchronize(st));
        if (!std::isfinite(norm)) {   // nothing is launched: weights, moments and the step count stay as they are
            if (h_report) *h_report = eigen_adam_report{norm, 1.0, 0, 0};
            return EIGEN_OK;
        }
    }
    const int step = ++t->adam_t;
    const double lr_t = s->alpha * std::sqrt(1.0 - std::pow(s->beta2, step)) / (1.0 - std::pow(s->beta1, step));
    ew(st, tadam_ex_kernel, t->n_params, t->prm, t->mom, t->var, (const float*)t->grd, t->n_params, (float)lr_t, (float)(1.0 - s->beta1),
       (float)(1.0 - s->beta2), (float)s->eps, (float)s->weight_decay, s->clip_norm, (const double*)t->o_norm);
    TCHK(hipGetLastError());
    if (h_report) {
        if (!s->skip_nonfinite) {
            TCHK(hipMemcpyAsync(&norm, t->o_norm, 8, hipMemcpyDeviceToHost, st));
            TCHK(hipStreamSynchronize(st));
        }
        *h_report = eigen_adam_report{norm, (s->clip_norm > 0 && norm > s->clip_norm) ? s->clip_norm / norm : 1.0, 1, 0};
    }
    return EIGEN_OK;
}

int eigen_trainer_accumulate(eigen_trainer* t, int32_t op, double scale, void* stream)
{
    if (!t) return tfail(EIGEN_ERR_INVALID, "null argument");
    if (op != EIGEN_ACC_CLEAR && op != EIGEN_ACC_ADD && op != EIGEN_ACC_LOAD) return tfail(EIGEN_ERR_INVALID, "unknown accumulator op %d", op);
    if (!std::isfinite(scale)) return tfail(EIGEN_ERR_INVALID, "scale must be finite");
    if (!t->have_weights) return tfail(EIGEN_ERR_STATE, "eigen_trainer_set_weights has not been called");
    if (op == EIGEN_ACC_LOAD && t->acc_count == 0) return tfail(EIGEN_ERR_STATE, "EIGEN_ACC_LOAD with nothing accumulated");
    TCHK(hipSetDevice(t->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    const size_t bytes = (size_t)t->n_params * 4;
    if (op == EIGEN_ACC_CLEAR) {
        if (t->acc) TCHK(hipMemsetAsync(t->acc, 0, bytes, st));
        t->acc_count = 0;
    } else if (op == EIGEN_ACC_ADD) {
        const int rc = accumulator(t);
        if (rc) return rc;
        if (t->acc_count == 0) TCHK(hipMemsetAsync(t->acc, 0, bytes, st));   // an empty accumulator starts from zero
        ew(st, tgrad_axpy_kernel, t->n_params, t->acc, (const float*)t->grd, (float)scale, t->n_params);
        TCHK(hipGetLastError());
        ++t->acc_count;
    } else {
        TCHK(hipMemcpyAsync(t->grd, t->acc, bytes, hipMemcpyDeviceToDevice, st));
    }
    return EIGEN_OK;
}

// ---- the flow entries with a solve
int eigen_trainer_flow_term_iter(eigen_trainer* t, const float* d_pred, int64_t p_bstride, const uint8_t* d_ref, const float* d_fref, int64_t r_bstride,
                                 int32_t batch, const eigen_flow_settings* flow, const uint8_t* d_mask, const eigen_flow_score* score,
                                 const eigen_flow_structure_score* sscore, const eigen_flow_members* members, double scale, double* h_value, double* h_stats,
                                 double* d_flow, float* d_seed, int64_t s_bstride, float* d_ref_grad, int64_t rg_bstride, void* stream, const float* d_dir,
                                 const eigen_dense_solve* solve)
{
    const int rc = refuse_solve_term(d_ref, d_fref, score, sscore, members);
    if (rc) return rc;
    FlowTermCall c{d_pred, p_bstride, r_bstride, batch, flow, d_mask, scale, h_value, d_flow, d_seed, s_bstride, stream};
    c.d_ref = d_ref; c.d_fref = d_fref; c.d_dir = d_dir; c.d_refg = d_ref_grad; c.rg_bstride = rg_bstride;
    c.score = score; c.sscore = sscore; c.members = members; c.h_stats = h_stats; c.solve = solve;
    return flow_term(t, c);
}

int eigen_trainer_loss_grad_flow_iter(eigen_trainer* t, const uint8_t* d_frames, int64_t bstride, int32_t batch, int32_t n_steps, int32_t n_fed, int32_t requant,
                                      int32_t reset, const double* h_step_w, int32_t objective, const double* h_layer_w, double* h_loss, double* h_layer_err,
                                      float* d_pred, float* d_frame_grad, int64_t g_bstride, int64_t g_tstride, const eigen_flow_settings* flow, const float* d_dir,
                                      const uint8_t* d_mask, double* h_terms, int32_t pairing, const eigen_flow_score* score,
                                      const eigen_flow_structure_score* sscore, const eigen_flow_members* members, double* h_stats, void* stream,
                                      const eigen_dense_solve* solve)
{
    LossGradCall c{d_frames, bstride, batch, n_steps, n_fed, requant, reset, h_loss, d_pred, stream};
    set_objective(c, h_step_w, objective, h_layer_w, h_layer_err, d_frame_grad, g_bstride, g_tstride);
    set_flow(c, flow, d_dir, d_mask, h_terms, pairing);
    c.score = score; c.sscore = sscore;
    c.members = members; c.h_stats = h_stats; c.solve = solve;
    return loss_grad_call(t, c);
}

int eigen_trainer_flow_term_target(eigen_trainer* t, const float* d_pred, int64_t p_bstride, const uint8_t* d_ref, const float* d_fref, int64_t r_bstride,
                                   int32_t batch, const eigen_flow_settings* flow, const uint8_t* d_mask, const eigen_flow_score* score,
                                   const eigen_flow_structure_score* sscore, const eigen_flow_members* members, double scale, double* h_value, double* h_stats,
                                   double* d_flow, float* d_seed, int64_t s_bstride, float* d_ref_grad, int64_t rg_bstride, void* stream, const float* d_dir,
                                   const eigen_dense_solve* solve, const double* d_target, int64_t t_bstride)
{
    const int rc = refuse_solve_term(d_ref, d_fref, score, sscore, members);
    if (rc) return rc;
    FlowTermCall c{d_pred, p_bstride, r_bstride, batch, flow, d_mask, scale, h_value, d_flow, d_seed, s_bstride, stream};
    c.d_ref = d_ref; c.d_fref = d_fref; c.d_dir = d_dir; c.d_refg = d_ref_grad; c.rg_bstride = rg_bstride;
    c.score = score; c.sscore = sscore; c.members = members; c.h_stats = h_stats; c.solve = solve; c.d_target = d_target; c.t_bstride = t_bstride;
    return flow_term(t, c);
}

int eigen_trainer_loss_grad_flow_target(eigen_trainer* t, const uint8_t* d_frames, int64_t bstride, int32_t batch, int32_t n_steps, int32_t n_fed, int32_t requant,
                                        int32_t reset, const double* h_step_w, int32_t objective, const double* h_layer_w, double* h_loss, double* h_layer_err,
                                        float* d_pred, float* d_frame_grad, int64_t g_bstride, int64_t g_tstride, const eigen_flow_settings* flow, const float* d_dir,
                                        const uint8_t* d_mask, double* h_terms, int32_t pairing, const eigen_flow_score* score,
                                        const eigen_flow_structure_score* sscore, const eigen_flow_members* members, double* h_stats, void* stream,
                                        const eigen_dense_solve* solve, const double* d_target, int64_t t_bstride, int64_t t_tstride)
{
    LossGradCall c{d_frames, bstride, batch, n_steps, n_fed, requant, reset, h_loss, d_pred, stream};
    set_objective(c, h_step_w, objective, h_layer_w, h_layer_err, d_frame_grad, g_bstride, g_tstride);
    set_flow(c, flow, d_dir, d_mask, h_terms, pairing);
    c.score = score; c.sscore = sscore;
    c.members = members; c.h_stats = h_stats; c.solve = solve; c.d_target = d_target; c.t_bstride = t_bstride; c.t_tstride = t_tstride;
    return loss_grad_call(t, c);
}

int eigen_trainer_flow_term_valid(eigen_trainer* t, const float* d_pred, int64_t p_bstride, const uint8_t* d_ref, const float* d_fref, int64_t r_bstride,
                                  int32_t batch, const eigen_flow_settings* flow, const uint8_t* d_mask, const eigen_flow_score* score,
                                  const eigen_flow_structure_score* sscore, const eigen_flow_members* members, double scale, double* h_value, double* h_stats,
                                  double* d_flow, float* d_seed, int64_t s_bstride, float* d_ref_grad, int64_t rg_bstride, void* stream, const float* d_dir,
                                  const eigen_dense_solve* solve, const double* d_target, int64_t t_bstride, const uint8_t* d_valid, int64_t v_bstride)
{
    const int rc = refuse_solve_term(d_ref, d_fref, score, sscore, members);
    if (rc) return rc;
    FlowTermCall c{d_pred, p_bstride, r_bstride, batch, flow, d_mask, scale, h_value, d_flow, d_seed, s_bstride, stream};
    c.d_ref = d_ref; c.d_fref = d_fref; c.d_dir = d_dir; c.d_refg = d_ref_grad; c.rg_bstride = rg_bstride;
    c.score = score; c.sscore = sscore; c.members = members; c.h_stats = h_stats; c.solve = solve; c.d_target = d_target; c.t_bstride = t_bstride;
    c.d_valid = d_valid; c.v_bstride = v_bstride;
    return flow_term(t, c);
}

int eigen_trainer_loss_grad_flow_joint(eigen_trainer* t, const uint8_t* d_frames, int64_t bstride, int32_t batch, int32_t n_steps, int32_t n_fed, int32_t requant,
                                       int32_t reset, const double* h_step_w, int32_t objective, const double* h_layer_w, double* h_loss, double* h_layer_err,
                                       float* d_pred, float* d_frame_grad, int64_t g_bstride, int64_t g_tstride, const eigen_flow_settings* flow, const float* d_dir,
                                       const uint8_t* d_mask, double* h_terms, int32_t pairing, const eigen_flow_score* score,
                                       const eigen_flow_structure_score* sscore, const eigen_flow_members* members, double* h_stats, void* stream,
                                       const eigen_dense_solve* solve, const double* d_target, int64_t t_bstride, int64_t t_tstride, const eigen_flow_joint* joint)
{
    LossGradCall c{d_frames, bstride, batch, n_steps, n_fed, requant, reset, h_loss, d_pred, stream};
    set_objective(c, h_step_w, objective, h_layer_w, h_layer_err, d_frame_grad, g_bstride, g_tstride);
    set_flow(c, flow, d_dir, d_mask, h_terms, pairing);
    c.score = score; c.sscore = sscore;
    c.members = members; c.h_stats = h_stats; c.solve = solve; c.d_target = d_target; c.t_bstride = t_bstride; c.t_tstride = t_tstride;
    c.joint = joint;
    return loss_grad_call(t, c);
}

int eigen_trainer_debug_flow_iter(eigen_trainer* t, int32_t force, int64_t* workspace_bytes)
{
    if (!t) return tfail(EIGEN_ERR_INVALID, "null argument");
    if (force >= 0) t->fw.it_force = force != 0;
    if (workspace_bytes) *workspace_bytes = t->fw.it_ws ? t->fw.it_doubles * 8 : 0;
    return EIGEN_OK;
}

}  // extern "C"
