// eigen_engine.hip -- C ABI (include/eigen_engine.h) of the MI355X fitness engine: handle, device workspaces,
// weight packing, kernel launch sequencing.  All compute is in the HIP kernels of conv_mfma.h / cppn_kernel.h /
// flow_kernels.h / score_kernels.h; there is no CPU fallback anywhere in this library.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/eigen_engine.h"
#define EIG_ENGINE_UNIT 1   // (conv_mfma.h: the non-template kernels are defined in this unit)
#include "conv_mfma.h"
#include "wino_launch.h"   // the Winograd kernels live in wino4_kernels.hip / wino4t_kernels.hip / wino4h_kernels.hip / wino4p_kernels.hip
#include "weight_pack.h"   // host: weight tensors -> the kernels' layouts
#include "conv_plan.h"     // host: which operators run (plan_prednet) and in which launch shape (plan_launch)
#include "cppn_kernel.h"
#include "cppn_grad_kernel.h"
#include "cppn_motion_kernel.h"
#include "cppn_valid_kernel.h"
#include "farneback_kernels.h"
#include "flow_kernels.h"
#include "score_kernels.h"
#include "dense_stage.h"   // the dense fitness's stage lives with the flow objective's kernels, in flow_stage.hip

using namespace eig;

static thread_local std::string g_err;
static int fail(int code, const char* fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
// (prednet_train.hip reports its errors through the same thread-local text)
int eig_set_error(int code, const char* msg)
{
    g_err = msg;
    return code;
}
#define HIPCHK(x)                                                                                      \
    do {                                                                                               \
        hipError_t _e = (x);                                                                           \
        if (_e != hipSuccess) return fail(EIGEN_ERR_HIP, "%s:%d %s -> %s", __FILE__, __LINE__, #x, hipGetErrorString(_e)); \
    } while (0)

namespace {

template <typename T> struct DevBuf {   // an owned device allocation that only grows
    T* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    int ensure(size_t n)
    {
        if (n <= cap) return 0;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        if (hipMalloc((void**)&p, n * sizeof(T)) != hipSuccess) return -1;
        cap = n;
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

static int upload(DevBuf<float>& dst, const float* src, size_t n)
{
    if (dst.ensure(n)) return -1;
    return hipMemcpy(dst.p, src, n * sizeof(float), hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}

// An operator of the plan (conv_plan.h: OpDesc is its geometry) with its device weights and its counters
struct ConvOp : OpDesc {
    DevBuf<float> wpk;   // the packed weights of the form the operator runs
    DevBuf<float> wraw;  // image layer only (OpDesc::raw): the unpacked table of convp0_direct_kernel / lstm0_direct_kernel
    double ms = 0;       // profiling accumulator
    int launches = 0;
    int tl_seen = 0;     // EIG_TIMING builds: launches seen (timeline dump)
    int last_grid = 0, last_waves = 4;  // timeline records of the last launch (launch_conv), for the EIG_TIMING read-back
    void replan(const OpDesc& d) { OpDesc::operator=(d); ms = 0; launches = 0; tl_seen = 0; }   // the allocations stay
};

struct Layer {
    int C = 0, H = 0, W = 0;
    float* h[2] = {nullptr, nullptr};
    float *c = nullptr, *P = nullptr, *E = nullptr;
    DevBuf<float> bias_lstm, peep, biasA, biasP;
    ConvOp convA, lstm, convP, convA_t0, lstm_t0, up4;   // conv_plan.h: LayerPlan
};


}  // namespace

struct eigen_engine {
    eigen_config cfg;
    int L = 0, B = 0, C0 = 0, H = 0, W = 0, K = 0;
    Layer layer[EIGEN_MAX_LAYERS];
    bool have_weights = false, have_grid = false;
    int n_planes = 0;
    double* d_planes = nullptr;
    // genome staging
    DevBuf<int32_t> g_node_off, g_edge_off, g_edge_src, g_out_node;
    DevBuf<uint8_t> g_node_act;
    DevBuf<double> g_node_bias, g_node_resp, g_edge_w;
    DevBuf<double> g_grad_slabs, g_grad_sum;   // eigen_cppn_param_grads: one slab per pixel block, and their sum
    DevBuf<double> g_affine;                   // eigen_render_moving_cppn: every affine beside its inverse
    std::vector<double> h_affine;              // ... as packed on the host (kept: the upload is asynchronous)
    DevBuf<double> g_valid_affine;             // eigen_moving_cppn_valid: the same records, in buffers of its own (a render may be in flight)
    std::vector<double> h_valid_affine;
    // images / frames
    uint8_t* d_images = nullptr;  // [B][C0][H][W]
    uint8_t* d_frames = nullptr;  // [B][3][C0][H][W]
    // flow
    int n_levels = 1;             // pyramid levels that exist (max_level + 1)
    int lvH[FLOW_MAX_LEVELS], lvW[FLOW_MAX_LEVELS];
    uint8_t* d_gray[2][FLOW_MAX_LEVELS] = {{nullptr}};
    short2* d_deriv[FLOW_MAX_LEVELS] = {nullptr};
    float* d_eig = nullptr;
    unsigned long long* d_cand = nullptr;
    float *d_corners = nullptr, *d_next = nullptr, *d_vectors = nullptr;
    uint8_t* d_status = nullptr;
    int *d_ncorners = nullptr, *d_counts = nullptr;
    double* d_fitness = nullptr;
    float* d_zeros = nullptr;  // DMA source for zero fill (conv_mfma.h)
    eigd::DenseWork dense;     // the dense fitness's workspace (eigen_dense_score): allocated by the first dense call, all of it or none
    bool have_dense = false;
    bool dense_force_iter = false;  // eigen_debug_dense_solve: one level, one iteration goes through the iteration kernel too
    // eigen_debug_dense_gray: where the last float dense call left its gray planes (I0, then I1 behind batch * H * W doubles); 0: none, or overwritten
    const double* dense_gray_at = nullptr;
    int dense_gray_batch = 0;
    // Farneback dense flow (cfg.flow_method == EIGEN_FLOW_FARNEBACK): allocated on first use
    float *fb_I = nullptr, *fb_R0 = nullptr, *fb_R1 = nullptr, *fb_M = nullptr, *fb_V = nullptr, *fb_flow[2] = {nullptr, nullptr};
    DevBuf<float> raw4;   // partial chains of the unpooled source, [B][4 classes][n_nblk*NB][H/2][W/2], reused by all layers
    // timing
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    hipEvent_t pev0 = nullptr, pev1 = nullptr;
    int n_cu = 256;  // compute units of the device (launch-shape heuristics)
    bool profile_convs = false;
    double ms[6] = {0, 0, 0, 0, 0, 0};
    int hflip = 0;  // which h buffer holds the current R
    int seq_batch = 0;  // batch of the state the last eigen_prednet_sequence left (0: none; eigen_prednet_rollout overwrites it)
    // ConvP_l (l > 0) is read by nobody until ConvA_l of the NEXT step: forked onto a side stream it can fill the CUs the last round of the ConvLSTM below it leaves idle
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join[EIGEN_MAX_LAYERS] = {nullptr};
};

// ------------------------------------------------------------------------------------------------ helpers

// ---- Farneback constants (host; the same double-precision recipe as oracle/farneback.c, checked by tests/test_gpu_parity.py) ----
static int fb_levels_used(int H, int W, int levels)  // calcOpticalFlowFarneback: no level below 32 pixels
{
    int k = 0;
    double scale = 1;
    for (; k < levels; ++k) {
        scale *= 0.5;
        if (W * scale < 32 || H * scale < 32) break;
    }
    return k;
}
static int fb_grid_step(int H, int W, int step, int max_vectors)
{
    int s = step;
    while ((H / s) * (W / s) > max_vectors) s += step;
    return s;
}
static FbBlur fb_blur_kernel(int k)  // GaussianBlur of pyramid level k: sigma = (2^k - 1) / 2, ksize = max(cvRound(5 sigma) | 1, 3)
{
    FbBlur b;
    memset(&b, 0, sizeof(b));
    const double sigma = ((double)(1 << k) - 1) * 0.5;
    int ksize = (int)lrint(sigma * 5) | 1;
    if (ksize < 3) ksize = 3;
    b.r = ksize / 2;
    if (sigma <= 0 && ksize == 3) { b.k[0] = 0.5f; b.k[1] = 0.25f; return b; }
    const double sx = sigma > 0 ? sigma : ((ksize - 1) * 0.5 - 1) * 0.3 + 0.8;
    const double s2 = -0.5 / (sx * sx);
    std::vector<double> c(ksize);
    double sum = 0;
    for (int i = 0; i < ksize; ++i) { const double x = i - (ksize - 1) * 0.5; c[i] = exp(s2 * x * x); sum += c[i]; }
    sum = 1.0 / sum;
    for (int j = 0; j <= b.r; ++j) b.k[j] = (float)(c[b.r + j] * sum);
    return b;
}
static FbConst fb_poly_constants(int n, double sigma)  // FarnebackPrepareGaussian
{
    FbConst c;
    memset(&c, 0, sizeof(c));
    c.poly_n = n;
    if (sigma < 1.1920928955078125e-07) sigma = n * 0.3;
    std::vector<double> gd(2 * n + 1);
    std::vector<float> gf(2 * n + 1);
    double s = 0;
    for (int x = -n; x <= n; ++x) { gd[x + n] = exp(-x * x / (2 * sigma * sigma)); s += gd[x + n]; }
    s = 1.0 / s;
    for (int x = -n; x <= n; ++x) gf[x + n] = (float)(gd[x + n] * s);
    for (int x = 0; x <= n; ++x) { c.g[x] = gf[x + n]; c.xg[x] = (float)(x * gf[x + n]); c.xxg[x] = (float)(x * x * gf[x + n]); }
    double G[6][6];
    memset(G, 0, sizeof(G));
    for (int y = -n; y <= n; ++y)
        for (int x = -n; x <= n; ++x) {
            const double w = (double)gf[y + n] * (double)gf[x + n];
            G[0][0] += w;
            G[1][1] += w * x * x;
            G[3][3] += w * x * x * x * x;
            G[5][5] += w * x * x * y * y;
        }
    G[2][2] = G[0][3] = G[0][4] = G[3][0] = G[4][0] = G[1][1];
    G[4][4] = G[3][3];
    G[3][4] = G[4][3] = G[5][5];
    double A[6][12];  // Gauss-Jordan with partial pivoting
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 12; ++j) A[i][j] = j < 6 ? G[i][j] : (j - 6 == i ? 1.0 : 0.0);
    for (int col = 0; col < 6; ++col) {
        int p = col;
        for (int r = col + 1; r < 6; ++r) if (fabs(A[r][col]) > fabs(A[p][col])) p = r;
        if (p != col) for (int j = 0; j < 12; ++j) std::swap(A[col][j], A[p][j]);
        const double d = 1.0 / A[col][col];
        for (int j = 0; j < 12; ++j) A[col][j] *= d;
        for (int r = 0; r < 6; ++r) {
            if (r == col) continue;
            const double f = A[r][col];
            if (f != 0.0) for (int j = 0; j < 12; ++j) A[r][j] -= f * A[col][j];
        }
    }
    c.ig[0] = (float)A[1][7]; c.ig[1] = (float)A[0][9]; c.ig[2] = (float)A[3][9]; c.ig[3] = (float)A[5][11];
    return c;
}

// the effective mask of this process: EIGEN_WINOGRAD (default EIGEN_WINO_DEFAULT, conv_plan.h), bit 24 cleared by EIGEN_WINO_FUSEUP=0 (eigen_winograd_mask; oracle.wino_mask_default)
static int wino_mask_env()
{
    static const int mask = [] {
        int m = getenv("EIGEN_WINOGRAD") && *getenv("EIGEN_WINOGRAD") ? (int)strtol(getenv("EIGEN_WINOGRAD"), nullptr, 0) : EIGEN_WINO_DEFAULT;
        if (getenv("EIGEN_WINO_FUSEUP") && !atoi(getenv("EIGEN_WINO_FUSEUP"))) m &= ~(1 << 24);
        return m;
    }();
    return mask;
}
// The A/B switches of this process (conv_plan.h: Switches says what each is for): read from the environment once, before the first use
static const Switches& switches()
{
    static const Switches sw = [] {
        Switches s;
        auto num = [](const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; };
        s.tile_map = num("EIGEN_TILE_MAP", 1);
        s.w8 = num("EIGEN_W8", -1);
        s.w4_tall = num("EIGEN_W4_TALL", -1); s.w4_half = num("EIGEN_W4_HALF", -1); s.w4_pack = num("EIGEN_W4_PACK", -1);
        s.w4_parts = num("EIGEN_W4_PARTS", 0);
        if (getenv("EIGEN_TW8_FACTOR")) s.tw8_factor = atof(getenv("EIGEN_TW8_FACTOR"));
        s.convp0_direct = !num("EIGEN_CONVP0_MFMA", 0); s.lstm0_direct = !num("EIGEN_LSTM0_MFMA", 0);
        s.onekb = !num("EIGEN_NO_ONEKB", 0); s.up4c = !num("EIGEN_NO_UP4C", 0); s.skip_zero_sources = !num("EIGEN_NO_T0", 0);
        s.side_stream = num("EIGEN_SIDE_STREAM", -1);
        return s;
    }();
    return sw;
}

// The packed weights of the form an operator runs; wt[WT_*][gate]: the layer's weight tensors (conv_plan.h)
static std::vector<float> pack_op(const OpDesc& d, const float* const wt[5][4])
{
    const float* sw[3][4] = {{nullptr}, {nullptr}, {nullptr}};
    for (int s = 0; s < d.npk; ++s)
        for (int g = 0; g < 4; ++g) sw[s][g] = wt[d.pk_w[s]][g];
    switch (d.pack) {
        case PACK_WINO: return pack_weights_wino(d.Cout, d.NI, d.n_nblk, d.lstm_mode != 0, d.npk, d.pk_C, d.pk_Ct, sw);
        case PACK_UP4: return pack_weights_up4(d, sw[0], d.lstm_mode);
        case PACK_UP4C: return pack_weights_up4c(d, sw[0], d.lstm_mode);
        default: return pack_weights(d, sw, d.lstm_mode);
    }
}


template <int NI, int TW, int EPI, bool VEC, bool ONEKB = false, int SPLIT = 0> static hipError_t launch_inst2(const ConvArgs& a, int grid, hipStream_t st)
{
    constexpr int NT = SPLIT == 1 ? 512 : CONV_THREADS;
    constexpr int lds = conv_lds_bytes<NI, TW, VEC, epi_taps(EPI), ONEKB, NT, false>();
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute((const void*)conv3x3_mfma<NI, TW, EPI, VEC, ONEKB, false, SPLIT>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        attr_done = true;
    }
    hipLaunchKernelGGL((conv3x3_mfma<NI, TW, EPI, VEC, ONEKB, false, SPLIT>), dim3(grid), dim3(NT), lds, st, a);
    return hipGetLastError();
}

// w8: the eight-wave instantiation (conv_mfma.h: W8) -- ConvA only (the image layer's ConvA at small launches; every other direct operator class lost its
// eight-wave / half-block / strip instantiations in round 6: with the Winograd forms as the default nothing at any BASELINE shape ran them)
template <int NI, int TW, int EPI> static hipError_t launch_inst(const ConvArgs& a, int grid, hipStream_t st, bool vec, int w8 = 0)
{
    if constexpr (EPI == EPI_CONVA && TW == 16 && NI < 4) {   // (16-wide tiles only: the image layer's ConvA never runs on 8 x 8 tiles at a reference shape; a 64-column ConvA is a Winograd operator)
        if (w8 && vec) return launch_inst2<NI, TW, EPI, true, false, 1>(a, grid, st);
    }
    return vec ? launch_inst2<NI, TW, EPI, true>(a, grid, st) : launch_inst2<NI, TW, EPI, false>(a, grid, st);
}

template <int EPI> static hipError_t launch_epi(int NI, int TW, const ConvArgs& a, int grid, hipStream_t st, bool vec, int w8 = 0)
{
    if (TW == 16) {
        switch (NI) {
            case 1: return launch_inst<1, 16, EPI>(a, grid, st, vec, w8);
            case 2: return launch_inst<2, 16, EPI>(a, grid, st, vec, w8);
            case 3: return launch_inst<3, 16, EPI>(a, grid, st, vec, w8);
            default: return launch_inst<4, 16, EPI>(a, grid, st, vec, w8);
        }
    }
    switch (NI) {
        case 1: return launch_inst<1, 8, EPI>(a, grid, st, vec, w8);
        case 2: return launch_inst<2, 8, EPI>(a, grid, st, vec, w8);
        case 3: return launch_inst<3, 8, EPI>(a, grid, st, vec, w8);
        default: return launch_inst<4, 8, EPI>(a, grid, st, vec, w8);
    }
}

// Timeline of one launch (measurement builds, -DEIG_TIMING=1, with EIGEN_TIMELINE=<dir>): the record buffer of a steady-state launch of every ConvLSTM op and
// 2x2-form pass (EIGEN_TIMELINE_ALL: every Winograd operator), sized from the plan; read back and written to <dir> after the launch.
#if EIG_TIMING
static unsigned long long* timeline_begin(ConvOp& op, ConvArgs& a, const LaunchPlan& p)
{
    if (!(getenv("EIGEN_TIMELINE") && (op.epi == EPI_LSTM || (op.epi == EPI_UP4 && op.NI == 4) || (op.wino && getenv("EIGEN_TIMELINE_ALL"))) && ++op.tl_seen == 6)) return nullptr;
    unsigned long long* d = nullptr;
    const size_t bytes = (size_t)p.last_grid * p.last_waves * 64;
    if (hipMalloc((void**)&d, bytes) != hipSuccess) return nullptr;
    (void)hipMemset(d, 0, bytes);
    a.dbg = d;
    return d;
}
static void timeline_end(const ConvOp& op, ConvArgs& a, const LaunchPlan& p, unsigned long long* d, hipStream_t st)
{
    if (!d) return;
    (void)hipStreamSynchronize(st);
    std::vector<unsigned long long> h((size_t)p.last_grid * p.last_waves * 8);
    (void)hipMemcpy(h.data(), d, h.size() * 8, hipMemcpyDeviceToHost);
    char name[256];
    snprintf(name, sizeof(name), "%s/timeline_H%d_C%d%s.bin", getenv("EIGEN_TIMELINE"), op.H, op.Cout, op.epi == EPI_UP4 ? "_up4" : op.epi == EPI_CONVA ? "_convA" : op.epi == EPI_CONVP ? "_convP" : "");
    if (FILE* f = fopen(name, "wb")) { fwrite(h.data(), 8, h.size(), f); fclose(f); }
    (void)hipFree(d);
    a.dbg = nullptr;
}
#else
static inline unsigned long long* timeline_begin(ConvOp&, ConvArgs&, const LaunchPlan&) { return nullptr; }
static inline void timeline_end(const ConvOp&, ConvArgs&, const LaunchPlan&, unsigned long long*, hipStream_t) {}
#endif

// The launch the plan names (conv_plan.h: LaunchPlan)
static hipError_t dispatch_conv(const ConvOp& op, const LaunchPlan& p, const ConvArgs& a, int batch, hipStream_t st)
{
    const int grid = p.grid;
    const bool vec = p.vec;
    switch (p.kernel) {
        case K_WINO: return launch_wino4(op.NI, op.epi, p.shape, a, grid, st);
        case K_CONVP0: {
            const dim3 g(p.gx, p.gy, batch);
            if (op.Cout == 3) hipLaunchKernelGGL(convp0_direct_kernel<3>, g, dim3(p.threads), 0, st, a.src[0].ptr, op.wraw.p, a);
            else hipLaunchKernelGGL(convp0_direct_kernel<1>, g, dim3(p.threads), 0, st, a.src[0].ptr, op.wraw.p, a);
            return hipGetLastError();
        }
        case K_LSTM0: {   // the step-0 operator has one source
            const dim3 g(p.gx, p.gy, batch), blk(p.threads);
            const float *sE = a.src[0].ptr, *sH = a.src[1].ptr;
            if (op.nsrc == 1) {
                if (op.Cout == 3) hipLaunchKernelGGL((lstm0_direct_kernel<3, true>), g, blk, 0, st, sE, sH, op.wraw.p, a);
                else hipLaunchKernelGGL((lstm0_direct_kernel<1, true>), g, blk, 0, st, sE, sH, op.wraw.p, a);
            } else {
                if (op.Cout == 3) hipLaunchKernelGGL((lstm0_direct_kernel<3, false>), g, blk, 0, st, sE, sH, op.wraw.p, a);
                else hipLaunchKernelGGL((lstm0_direct_kernel<1, false>), g, blk, 0, st, sE, sH, op.wraw.p, a);
            }
            return hipGetLastError();
        }
        default: break;
    }
    switch (op.epi) {
        case EPI_LSTM: return (op.TW == 16) ? launch_inst<4, 16, EPI_LSTM>(a, grid, st, vec) : launch_inst<4, 8, EPI_LSTM>(a, grid, st, vec);
        case EPI_LSTM_PACKED: return (op.TW == 16) ? launch_inst<1, 16, EPI_LSTM_PACKED>(a, grid, st, vec) : launch_inst<1, 8, EPI_LSTM_PACKED>(a, grid, st, vec);
        case EPI_CONVA:
            if (p.onekb) return launch_inst2<3, 16, EPI_CONVA, true, true>(a, grid, st);
            return launch_epi<EPI_CONVA>(op.NI, op.TW, a, grid, st, vec, p.w8);
        case EPI_CONVP: return launch_epi<EPI_CONVP>(op.NI, op.TW, a, grid, st, vec, p.w8);
        case EPI_UP4: return launch_epi<EPI_UP4>(op.NI, op.TW, a, grid, st, vec, p.w8);
        case EPI_UP4C: return launch_inst2<4, 16, EPI_UP4C, true>(a, grid, st);  // chosen only for 16-wide tiles and 16-byte staging
        default: return launch_epi<EPI_RAW>(op.NI, op.TW, a, grid, st, vec, p.w8);  // (eigen_test_conv)
    }
}

// Plan the launch (conv_plan.h), fill the geometry half of ConvArgs, launch, profile.  The caller has filled the pointers.
static hipError_t launch_conv(eigen_engine* e, ConvOp& op, ConvArgs& a, int batch, hipStream_t st)
{
    const LaunchPlan p = plan_launch(op, batch, e->n_cu, a.up_src != nullptr, a.acc_init != nullptr, switches());
    if (!p.ok) return hipErrorInvalidConfiguration;
    op.last_grid = p.last_grid; op.last_waves = p.last_waves;
    a.H = op.H; a.W = op.W; a.B = batch;
    a.tilesX = p.tilesX; a.tilesY = p.tilesY; a.tile_map = p.tile_map;
    a.n_nblk = op.n_nblk; a.krows = op.krows; a.wpk = op.wpk.p; a.Cout = op.Cout; a.zeros = e->d_zeros;
    a.nsrc = op.nsrc;
    for (int s = 0; s < op.nsrc; ++s) { a.src[s].C = op.src_C[s]; a.src[s].Cpad = pad4(op.src_C[s]); a.src[s]._reserved = 0; a.src[s].Ct = op.src_Ct[s] ? op.src_Ct[s] : op.src_C[s]; }
    if (p.kernel == K_WINO) { a.nparts = p.nparts; a.nwalk = p.nwalk; for (int i = 0; i < 3; ++i) a.mg[i] = p.mg[i]; }
    unsigned long long* tl = timeline_begin(op, a, p);
    if (e->profile_convs) (void)hipEventRecord(e->pev0, st);
    const hipError_t r = dispatch_conv(op, p, a, batch, st);
    timeline_end(op, a, p, tl, st);
    if (e->profile_convs && r == hipSuccess) {
        (void)hipEventRecord(e->pev1, st);
        (void)hipEventSynchronize(e->pev1);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e->pev0, e->pev1);
        op.ms += ms; op.launches++;
    }
    return r;
}



// ------------------------------------------------------------------------------------------------ ABI
extern "C" {

int eigen_abi_version(void) { return EIGEN_ABI_VERSION; }
int eigen_gate_order(void) { return EIG_GATE_ORDER; }
int eigen_winograd_mask(void) { return wino_mask_env(); }
const char* eigen_last_error(void) { return g_err.c_str(); }

void eigen_config_defaults(eigen_config* c)
{
    c->n_repeat = 20; c->n_ext = 2; c->requant_feedback = 0;
    c->lk_max_corners = 100; c->lk_block_size = 7; c->lk_win = 15; c->lk_max_level = 2; c->lk_max_iter = 10;
    c->flow_method = EIGEN_FLOW_LK;
    c->fb_levels = 3; c->fb_winsize = 15; c->fb_iterations = 3; c->fb_poly_n = 5; c->fb_step = 16; c->reserved1 = 0; c->fb_poly_sigma = 1.2;
    c->lk_quality_level = 0.3; c->lk_min_distance = 7.0; c->lk_epsilon = 0.03; c->lk_min_eig_thr = 1e-4;
}

int eigen_destroy(eigen_engine* e)
{
    if (!e) return EIGEN_OK;
    (void)hipSetDevice(e->cfg.device);
    for (int l = 0; l < e->L; ++l) {
        Layer& y = e->layer[l];
        float* ptrs[] = {y.h[0], y.h[1], y.c, y.P, y.E};   // (the weights are owned buffers: ~DevBuf)
        for (float* p : ptrs) if (p) (void)hipFree(p);
    }
    if (e->d_planes) (void)hipFree(e->d_planes);
    e->g_node_off.release(); e->g_edge_off.release(); e->g_edge_src.release(); e->g_out_node.release();
    e->g_node_act.release(); e->g_node_bias.release(); e->g_node_resp.release(); e->g_edge_w.release();
    e->g_grad_slabs.release(); e->g_grad_sum.release();
    void* misc[] = {e->d_images, e->d_frames, e->d_eig, e->d_cand, e->d_corners, e->d_next, e->d_vectors, e->d_status,
                    e->d_ncorners, e->d_counts, e->d_fitness, e->d_zeros,
                    e->fb_I, e->fb_R0, e->fb_R1, e->fb_M, e->fb_V, e->fb_flow[0], e->fb_flow[1]};
    for (void* p : misc) if (p) (void)hipFree(p);
    void* dense[] = {e->dense.planes, e->dense.u, e->dense.theta, e->dense.L, e->dense.rec, e->dense.part, e->dense.flag, e->dense.pyr};
    for (void* p : dense) if (p) (void)hipFree(p);
    for (void* p : e->dense.member_allocs) (void)hipFree(p);
    for (int i = 0; i < 2; ++i)
        for (int l = 0; l < FLOW_MAX_LEVELS; ++l) if (e->d_gray[i][l]) (void)hipFree(e->d_gray[i][l]);
    for (int l = 0; l < FLOW_MAX_LEVELS; ++l) if (e->d_deriv[l]) (void)hipFree(e->d_deriv[l]);
    if (e->side) (void)hipStreamDestroy(e->side);
    if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
    for (auto& ev : e->ev_join) if (ev) (void)hipEventDestroy(ev);
    for (auto& ev : e->ev) if (ev) (void)hipEventDestroy(ev);
    if (e->pev0) (void)hipEventDestroy(e->pev0);
    if (e->pev1) (void)hipEventDestroy(e->pev1);
    delete e;
    return EIGEN_OK;
}

int eigen_create(const eigen_config* cfg, eigen_engine** out)
{
    if (!cfg || !out) return fail(EIGEN_ERR_INVALID, "null argument");
    *out = nullptr;
    const int L = cfg->n_layers;
    if (L < 1 || L > EIGEN_MAX_LAYERS) return fail(EIGEN_ERR_INVALID, "n_layers %d out of range", L);
    if (cfg->width <= 0 || cfg->height <= 0 || (cfg->width % (1 << (L - 1))) || (cfg->height % (1 << (L - 1))))
        return fail(EIGEN_ERR_INVALID, "image %dx%d must be divisible by 2^(layers-1)=%d (2x2 pooling per PredNet layer)",
                    cfg->width, cfg->height, 1 << (L - 1));
    if (cfg->channels[0] != 1 && cfg->channels[0] != 3) return fail(EIGEN_ERR_INVALID, "channels[0] (c_dim) must be 1 or 3");
    if (cfg->max_batch < 1) return fail(EIGEN_ERR_INVALID, "max_batch must be >= 1");
    if (cfg->lk_max_corners < 1 || cfg->lk_max_corners > SCORE_T) return fail(EIGEN_ERR_INVALID, "lk_max_corners must be in 1..%d", SCORE_T);
    if (cfg->lk_win < 3 || cfg->lk_win > 16) return fail(EIGEN_ERR_INVALID, "lk_win must be in 3..16");
    if (cfg->lk_block_size < 1 || cfg->lk_block_size > EIG_MAXB) return fail(EIGEN_ERR_INVALID, "lk_block_size must be in 1..%d", EIG_MAXB);
    if (cfg->lk_max_level < 0 || cfg->lk_max_level >= FLOW_MAX_LEVELS) return fail(EIGEN_ERR_INVALID, "lk_max_level must be in 0..%d", FLOW_MAX_LEVELS - 1);
    if (cfg->n_repeat < 1 || cfg->n_ext < 0) return fail(EIGEN_ERR_INVALID, "n_repeat >= 1 and n_ext >= 0 required");
    if (cfg->flow_method != EIGEN_FLOW_LK && cfg->flow_method != EIGEN_FLOW_FARNEBACK) return fail(EIGEN_ERR_INVALID, "unknown flow_method %d", cfg->flow_method);
    if (cfg->flow_method == EIGEN_FLOW_FARNEBACK) {
        if (cfg->fb_poly_n < 1 || cfg->fb_poly_n > FB_MAX_POLY_N) return fail(EIGEN_ERR_INVALID, "fb_poly_n must be in 1..%d", FB_MAX_POLY_N);
        if (cfg->fb_winsize < 1 || !(cfg->fb_winsize & 1) || cfg->fb_winsize / 2 > FB_MAX_WIN_R) return fail(EIGEN_ERR_INVALID, "fb_winsize must be odd and <= %d", 2 * FB_MAX_WIN_R + 1);
        if (cfg->fb_levels < 0 || cfg->fb_levels > 4) return fail(EIGEN_ERR_INVALID, "fb_levels must be in 0..4 (Gaussian radius <= %d)", FB_MAX_BLUR_R);
        if (cfg->fb_iterations < 1 || cfg->fb_step < 1) return fail(EIGEN_ERR_INVALID, "fb_iterations >= 1 and fb_step >= 1 required");
        const int lv = fb_levels_used(cfg->height, cfg->width, cfg->fb_levels);
        if ((cfg->height % (1 << lv)) || (cfg->width % (1 << lv))) return fail(EIGEN_ERR_INVALID, "Farneback flow with %d pyramid levels needs an image divisible by %d", lv, 1 << lv);
    }
    for (int l = 0; l < L; ++l) if (cfg->channels[l] < 1) return fail(EIGEN_ERR_INVALID, "channels[%d] < 1", l);
    HIPCHK(hipSetDevice(cfg->device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, cfg->device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(EIGEN_ERR_INVALID, "device %d is %s; this library is built for gfx950 (MI355X) only", cfg->device, prop.gcnArchName);

    eigen_engine* e = new eigen_engine();
    e->cfg = *cfg;
    e->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    e->L = L; e->B = cfg->max_batch; e->C0 = cfg->channels[0]; e->H = cfg->height; e->W = cfg->width; e->K = cfg->lk_max_corners;
    const size_t B = (size_t)e->B;
#define ALLOC(ptr, n)                                                                              \
    do {                                                                                           \
        hipError_t _e = hipMalloc((void**)&(ptr), (n));                                            \
        if (_e != hipSuccess) { eigen_destroy(e); return fail(EIGEN_ERR_HIP, "hipMalloc(%zu) for %s: %s", (size_t)(n), #ptr, hipGetErrorString(_e)); } \
    } while (0)
    for (int l = 0; l < L; ++l) {
        Layer& y = e->layer[l];
        y.C = cfg->channels[l]; y.H = e->H >> l; y.W = e->W >> l;
        const size_t n = B * y.C * y.H * y.W * sizeof(float);
        ALLOC(y.h[0], n); ALLOC(y.h[1], n); ALLOC(y.c, n); ALLOC(y.P, n); ALLOC(y.E, 2 * n);
    }
    const size_t HW = (size_t)e->H * e->W;
    ALLOC(e->d_images, B * e->C0 * HW);
    ALLOC(e->d_frames, B * 3 * e->C0 * HW);
    // flow pyramids: a level exists only while both dims stay > winSize (buildOpticalFlowPyramid)
    e->lvH[0] = e->H; e->lvW[0] = e->W; e->n_levels = 1;
    for (int l = 1; l <= cfg->lk_max_level; ++l) {
        const int hd = (e->lvH[l - 1] + 1) / 2, wd = (e->lvW[l - 1] + 1) / 2;
        if (wd <= cfg->lk_win || hd <= cfg->lk_win) break;
        e->lvH[l] = hd; e->lvW[l] = wd; e->n_levels = l + 1;
    }
    for (int l = 0; l < e->n_levels; ++l) {
        const size_t n = B * e->lvH[l] * e->lvW[l];
        ALLOC(e->d_gray[0][l], n); ALLOC(e->d_gray[1][l], n);
        ALLOC(e->d_deriv[l], n * sizeof(short2));
    }
    ALLOC(e->d_eig, B * HW * sizeof(float));
    ALLOC(e->d_cand, B * HW * sizeof(unsigned long long));
    ALLOC(e->d_corners, B * e->K * 2 * sizeof(float));
    ALLOC(e->d_next, B * e->K * 2 * sizeof(float));
    ALLOC(e->d_vectors, B * e->K * 4 * sizeof(float));
    ALLOC(e->d_status, B * e->K);
    ALLOC(e->d_ncorners, B * sizeof(int));
    ALLOC(e->d_counts, B * sizeof(int));
    ALLOC(e->d_fitness, B * sizeof(double));
    ALLOC(e->d_zeros, 256);
    (void)hipMemset(e->d_zeros, 0, 256);
#undef ALLOC
    for (auto& ev : e->ev) HIPCHK(hipEventCreate(&ev));
    HIPCHK(hipStreamCreateWithFlags(&e->side, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
    for (int l = 0; l < L; ++l) HIPCHK(hipEventCreateWithFlags(&e->ev_join[l], hipEventDisableTiming));
    HIPCHK(hipEventCreate(&e->pev0));
    HIPCHK(hipEventCreate(&e->pev1));
    *out = e;
    return EIGEN_OK;
}
int eigen_set_prednet_weights(eigen_engine* e, const float* const* t, int32_t n_tensors)
{
    if (!e || !t) return fail(EIGEN_ERR_INVALID, "null argument");
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(hipDeviceSynchronize());   // a second call overwrites the weights in place: no roll-out still running on any stream may be reading them
    const int L = e->L;
    int expect = 0;
    for (int l = 0; l < L; ++l) expect += (l > 0 ? 2 : 0) + 2 + 4 * (l < L - 1 ? 4 : 3) + 3;
    if (n_tensors != expect) return fail(EIGEN_ERR_INVALID, "expected %d weight tensors for %d layers, got %d", expect, L, n_tensors);
    int Cs[EIGEN_MAX_LAYERS], Hs[EIGEN_MAX_LAYERS], Ws[EIGEN_MAX_LAYERS];
    for (int l = 0; l < L; ++l) { Cs[l] = e->layer[l].C; Hs[l] = e->layer[l].H; Ws[l] = e->layer[l].W; }
    std::vector<LayerPlan> plan(L);
    plan_prednet(L, Cs, Hs, Ws, wino_mask_env(), switches(), plan.data());
    int k = 0;
    for (int l = 0; l < L; ++l) {
        Layer& y = e->layer[l];
        const int C = y.C;
        // the layer's weight tensors, [WT_*][gate] (conv_plan.h)
        const float* wt[5][4] = {{nullptr}, {nullptr}, {nullptr}, {nullptr}, {nullptr}};
        const float *convA_b = nullptr, *bh[4];
        if (l > 0) { wt[WT_CONVA][0] = t[k++]; convA_b = t[k++]; }
        wt[WT_CONVP][0] = t[k++];
        const float* convP_b = t[k++];
        for (int g = 0; g < 4; ++g) {
            wt[WT_X0][g] = t[k++];
            if (l < L - 1) wt[WT_X1][g] = t[k++];
            wt[WT_H][g] = t[k++];
            bh[g] = t[k++];
        }
        const float* peep[3] = {t[k], t[k + 1], t[k + 2]};
        k += 3;
        for (int i = 0; i < k; ++i) if (!t[i]) return fail(EIGEN_ERR_INVALID, "weight tensor %d is NULL", i);

        // every operator: the form it will run, packed once and uploaded
        const LayerPlan& pl = plan[l];
        const std::vector<float> raw0 = pl.lstm.raw ? lstm0_raw_table(C, wt[WT_X0], wt[WT_H]) : std::vector<float>();
        const struct { ConvOp* op; const OpDesc* d; const char* name; } ops[6] = {{&y.convA, &pl.convA, "ConvA"}, {&y.convA_t0, &pl.convA_t0, "ConvA, step 0"}, {&y.lstm, &pl.lstm, "ConvLSTM"},
                                                                                   {&y.lstm_t0, &pl.lstm_t0, "ConvLSTM, step 0"}, {&y.up4, &pl.up4, "ConvLSTM, unpooled source"}, {&y.convP, &pl.convP, "ConvP"}};
        for (const auto& o : ops) {
            o.op->replan(*o.d);
            if (!o.d->present) continue;
            const std::vector<float> pk = pack_op(*o.d, wt);
            bool bad = upload(o.op->wpk, pk.data(), pk.size()) != 0;
            if (o.d->raw && !bad)   // image layer: ConvP's OIHW tensor itself; the ConvLSTM's table -- the step-0 operator reads the table's second part from a copy of its OWN (a few KB: every operator owns what it reads)
                bad = o.d->epi == EPI_CONVP ? upload(o.op->wraw, wt[WT_CONVP][0], (size_t)C * C * 9) : upload(o.op->wraw, raw0.data(), raw0.size());
            if (bad) return fail(EIGEN_ERR_HIP, "weight upload failed (%s, layer %d%s)", o.name, l, o.d->wino ? ", Winograd form" : "");
        }
        if (e->raw4.ensure((size_t)e->B * pl.up4.scratch_floats)) return fail(EIGEN_ERR_HIP, "hipMalloc(%zu) for the unpooled-source partial chains", (size_t)e->B * pl.up4.scratch_floats * sizeof(float));
        std::vector<float> bias(4 * (size_t)C);
        for (int g = 0; g < 4; ++g) memcpy(&bias[(size_t)g * C], bh[g], sizeof(float) * C);
        const size_t chw = (size_t)C * y.H * y.W;
        std::vector<float> pp(3 * chw);
        for (int g = 0; g < 3; ++g) memcpy(&pp[g * chw], peep[g], sizeof(float) * chw);
        if ((l > 0 && upload(y.biasA, convA_b, C)) || upload(y.biasP, convP_b, C) || upload(y.bias_lstm, bias.data(), bias.size()) || upload(y.peep, pp.data(), pp.size()))
            return fail(EIGEN_ERR_HIP, "weight upload failed (biases and peepholes, layer %d)", l);
    }
    e->have_weights = true;
    return EIGEN_OK;
}

double eigen_prednet_flops_per_step(const eigen_engine* e)
{
    if (!e) return 0;
    double macs = 0;
    for (int l = 0; l < e->L; ++l) {
        const Layer& y = e->layer[l];
        const int C = y.C;
        const double hw = (double)y.H * y.W;
        if (l > 0) macs += (double)e->layer[l - 1].H * e->layer[l - 1].W * C * 2.0 * e->layer[l - 1].C * 9;
        double cin = 3.0 * C + (l < e->L - 1 ? e->layer[l + 1].C : 0);
        macs += hw * 4 * C * cin * 9;
        macs += hw * C * C * 9;
    }
    return 2.0 * macs;
}

int eigen_set_grid(eigen_engine* e, const double* h_planes, int32_t n_planes)
{
    if (!e || !h_planes) return fail(EIGEN_ERR_INVALID, "null argument");
    if (n_planes < 1 || n_planes > 4) return fail(EIGEN_ERR_INVALID, "n_planes must be 1..4");
    HIPCHK(hipSetDevice(e->cfg.device));
    const size_t n = (size_t)n_planes * e->H * e->W;
    if (e->d_planes) { (void)hipFree(e->d_planes); e->d_planes = nullptr; }
    HIPCHK(hipMalloc((void**)&e->d_planes, n * sizeof(double)));
    HIPCHK(hipMemcpy(e->d_planes, h_planes, n * sizeof(double), hipMemcpyHostToDevice));
    e->n_planes = n_planes;
    e->have_grid = true;
    return EIGEN_OK;
}

// What both CPPN entry points do before they launch: the call-order and genome checks, then the batch on the device.
// lds_of(max_nodes, max_edges): the caller's LDS need; above 160 KiB the batch is refused before anything is uploaded.
struct GenomeExtent { int total_nodes = 0, total_edges = 0, max_nodes = 0, max_edges = 0; size_t lds = 0; };

// the host-side checks alone, against n_planes leaf planes; fills the extents but for x.lds
static int check_genomes(const eigen_genome_batch* g, int need_out, int n_planes, GenomeExtent& x)
{
    const int G = g->n_genomes;
    if (G < 1) return fail(EIGEN_ERR_INVALID, "n_genomes < 1");
    if (g->c_out < need_out) return fail(EIGEN_ERR_INVALID, "genome batch provides %d outputs per genome, %d needed", g->c_out, need_out);
    const int total_nodes = g->node_off[G];
    const int total_edges = g->edge_off[total_nodes];
    int max_nodes = 0, max_edges = 0;
    for (int i = 0; i < G; ++i) {
        const int nn = g->node_off[i + 1] - g->node_off[i];
        const int ne = g->edge_off[g->node_off[i + 1]] - g->edge_off[g->node_off[i]];
        if (nn < 1) return fail(EIGEN_ERR_INVALID, "genome %d has no nodes", i);
        max_nodes = std::max(max_nodes, nn); max_edges = std::max(max_edges, ne);
    }
    // every edge must point at a leaf, the constant-1 leaf, or an EARLIER node of the same genome (topological order)
    for (int gi = 0; gi < G; ++gi) {
        const int n0 = g->node_off[gi], n1 = g->node_off[gi + 1];
        for (int n = n0; n < n1; ++n)
            for (int k = g->edge_off[n]; k < g->edge_off[n + 1]; ++k) {
                const int src = g->edge_src[k];
                if (src < -(n_planes + 1))
                    return fail(EIGEN_ERR_INVALID, "genome %d: edge %d references leaf %d but only %d planes are set", gi, k, -src - 1, n_planes);
                if (src >= n - n0)
                    return fail(EIGEN_ERR_INVALID, "genome %d: edge %d of node %d reads node %d (not topologically earlier)", gi, k, n - n0, src);
            }
        for (int c = 0; c < g->c_out; ++c) {
            const int o = g->out_node[gi * g->c_out + c];
            if (o < 0 || o >= n1 - n0) return fail(EIGEN_ERR_INVALID, "genome %d: output %d names node %d of %d", gi, c, o, n1 - n0);
        }
    }
    x.total_nodes = total_nodes; x.total_edges = total_edges; x.max_nodes = max_nodes; x.max_edges = max_edges;
    return EIGEN_OK;
}

// the checked batch on the device; GENOME_ARGS(a): the fields every CPPN kernel's arguments share, from the staging buffers
static int upload_genomes(eigen_engine* e, const eigen_genome_batch* g, const GenomeExtent& x, hipStream_t st)
{
    const int G = g->n_genomes, total_nodes = x.total_nodes, total_edges = x.total_edges;
    if (e->g_node_off.ensure(G + 1) || e->g_edge_off.ensure(total_nodes + 1) || e->g_node_act.ensure(total_nodes) ||
        e->g_node_bias.ensure(total_nodes) || e->g_node_resp.ensure(total_nodes) || e->g_edge_src.ensure(std::max(total_edges, 1)) ||
        e->g_edge_w.ensure(std::max(total_edges, 1)) || e->g_out_node.ensure((size_t)G * g->c_out))
        return fail(EIGEN_ERR_HIP, "hipMalloc for the genome batch failed");
    HIPCHK(hipMemcpyAsync(e->g_node_off.p, g->node_off, sizeof(int32_t) * (G + 1), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(e->g_edge_off.p, g->edge_off, sizeof(int32_t) * (total_nodes + 1), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(e->g_node_act.p, g->node_act, total_nodes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(e->g_node_bias.p, g->node_bias, sizeof(double) * total_nodes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(e->g_node_resp.p, g->node_resp, sizeof(double) * total_nodes, hipMemcpyHostToDevice, st));
    if (total_edges) {
        HIPCHK(hipMemcpyAsync(e->g_edge_src.p, g->edge_src, sizeof(int32_t) * total_edges, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(e->g_edge_w.p, g->edge_w, sizeof(double) * total_edges, hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipMemcpyAsync(e->g_out_node.p, g->out_node, sizeof(int32_t) * G * g->c_out, hipMemcpyHostToDevice, st));
    return EIGEN_OK;
}
#define GENOME_ARGS(a)                                                                                                          \
    do {                                                                                                                        \
        (a).node_off = e->g_node_off.p; (a).edge_off = e->g_edge_off.p; (a).node_act = e->g_node_act.p;                         \
        (a).node_bias = e->g_node_bias.p; (a).node_resp = e->g_node_resp.p; (a).edge_src = e->g_edge_src.p;                     \
        (a).edge_w = e->g_edge_w.p; (a).out_node = e->g_out_node.p; (a).N = e->H * e->W; (a).c_out = g->c_out; (a).c_dim = e->C0; \
    } while (0)

static int stage_genomes(eigen_engine* e, const eigen_genome_batch* g, int need_out, size_t (*lds_of)(int, int), hipStream_t st, GenomeExtent& x, CppnArgs& a)
{
    if (!e->have_grid) return fail(EIGEN_ERR_STATE, "eigen_set_grid has not been called");
    HIPCHK(hipSetDevice(e->cfg.device));
    int rc = check_genomes(g, need_out, e->n_planes, x);
    if (rc != EIGEN_OK) return rc;
    x.lds = lds_of(x.max_nodes, x.max_edges);
    if (x.lds > 160 * 1024) return fail(EIGEN_ERR_CAPACITY, "genome with %d nodes / %d edges needs %zu B of LDS (> 160 KiB)", x.max_nodes, x.max_edges, x.lds);
    rc = upload_genomes(e, g, x, st);
    if (rc != EIGEN_OK) return rc;
    GENOME_ARGS(a);
    a.planes = e->d_planes; a.n_planes = e->n_planes; a.max_nodes = x.max_nodes;
    return EIGEN_OK;
}

// the genome program (bias, resp, weights, offsets, sources, activations) beside `columns` float64 [node][thread] columns
static size_t cppn_lds(size_t columns, int max_nodes, int max_edges)
{
    return columns + (size_t)max_nodes * 16 + (size_t)max_edges * 8 + (size_t)(max_nodes + 1) * 4 + (size_t)max_edges * 4 + max_nodes + 64;
}
static size_t render_lds(int max_nodes, int max_edges) { return cppn_lds((size_t)max_nodes * CPPN_THREADS * 8, max_nodes, max_edges); }
static size_t grad_lds(int max_nodes, int max_edges) { return cppn_lds((size_t)2 * max_nodes * CPPN_GRAD_THREADS * 8, max_nodes, max_edges); }

static int render_cppn_impl(eigen_engine* e, const eigen_genome_batch* g, int32_t bg, int mode, uint8_t* d_images, double* d_nodes, void* stream)
{
    hipStream_t st = (hipStream_t)stream;
    GenomeExtent x;
    CppnArgs a;
    const int rc = stage_genomes(e, g, (mode == 0) ? e->C0 : (mode == 4 ? 3 : 1), render_lds, st, x, a);
    if (rc != EIGEN_OK) return rc;
    a.bg = bg; a.mode = mode; a.out = d_images; a.out_f64 = d_nodes;
    (void)hipFuncSetAttribute((const void*)cppn_render_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)x.lds);
    hipLaunchKernelGGL(cppn_render_kernel, dim3((a.N + CPPN_THREADS - 1) / CPPN_THREADS, g->n_genomes), dim3(CPPN_THREADS), x.lds, st, a);
    HIPCHK(hipGetLastError());
    return EIGEN_OK;
}

int eigen_render_cppn(eigen_engine* e, const eigen_genome_batch* g, int32_t bg, int32_t gradient, uint8_t* d_images, void* stream)
{
    if (!e || !g || !d_images) return fail(EIGEN_ERR_INVALID, "null argument");
    if (gradient == 2) {  // get_equilum_image_from_cppn: three output nodes read as h, s, v
        if (e->C0 != 3) return fail(EIGEN_ERR_INVALID, "the h,s,v renderer needs c_dim = 3");
        if (g->c_out < 3) return fail(EIGEN_ERR_INVALID, "the h,s,v renderer needs 3 outputs per genome, the batch has %d", g->c_out);
        return render_cppn_impl(e, g, bg, 4, d_images, nullptr, stream);
    }
    if (gradient != 0 && gradient != 1) return fail(EIGEN_ERR_INVALID, "gradient must be 0, 1 or 2 (h,s,v renderer)");
    return render_cppn_impl(e, g, bg, (gradient == 1) ? 0 : (e->C0 == 1 ? 1 : 2), d_images, nullptr, stream);
}

int eigen_eval_cppn_nodes(eigen_engine* e, const eigen_genome_batch* g, double* d_nodes, void* stream)
{
    if (!e || !g || !d_nodes) return fail(EIGEN_ERR_INVALID, "null argument");
    return render_cppn_impl(e, g, 1, 3, nullptr, d_nodes, stream);
}

int eigen_render_moving_cppn(eigen_engine* e, const eigen_genome_batch* g, int32_t n, int32_t n_frames, int32_t n_layers, const double* h_affine,
                             const double* h_affine_inv, uint8_t* d_frames, int64_t f_bstride, double* d_flow, uint8_t* d_layer, void* stream)
{
    if (!e || !g || !h_affine || !d_frames) return fail(EIGEN_ERR_INVALID, "null argument");
    if (n_layers < 1 || n_layers > 2) return fail(EIGEN_ERR_INVALID, "n_layers %d outside 1..2", n_layers);
    if (n_frames < 1) return fail(EIGEN_ERR_INVALID, "n_frames %d < 1", n_frames);
    if (n < 1) return fail(EIGEN_ERR_INVALID, "n %d < 1", n);
    if (d_flow && n_frames < 2) return fail(EIGEN_ERR_INVALID, "a flow needs two frames, n_frames is %d", n_frames);
    if (d_flow && !h_affine_inv) return fail(EIGEN_ERR_INVALID, "d_flow without h_affine_inv");
    if (!d_flow && h_affine_inv) return fail(EIGEN_ERR_INVALID, "h_affine_inv without d_flow");
    if (n > 65535) return fail(EIGEN_ERR_CAPACITY, "n %d exceeds the 65535 samples of one launch", n);
    if ((long long)g->n_genomes != (long long)n * n_layers)
        return fail(EIGEN_ERR_INVALID, "the batch holds %d genomes, n * n_layers = %lld", g->n_genomes, (long long)n * n_layers);
    const long long seq = (long long)n_frames * e->C0 * e->H * e->W;
    if (f_bstride < seq) return fail(EIGEN_ERR_INVALID, "f_bstride %lld < n_frames*C*H*W = %lld", (long long)f_bstride, seq);
    if (!g->node_off || !g->edge_off || !g->node_act || !g->node_bias || !g->node_resp || !g->edge_src || !g->edge_w || !g->out_node)
        return fail(EIGEN_ERR_INVALID, "null array in the genome batch");
    GenomeExtent x;
    int rc = check_genomes(g, e->C0, 2, x);   // the two leaves are u and v, whatever grid the handle has or has not
    if (rc != EIGEN_OK) return rc;
    // a block holds the columns of its sample's larger program beside both of its programs
    for (int b = 0; b < n; ++b) {
        size_t progs = 0;
        int mn = 0;
        for (int gi = b * n_layers; gi < (b + 1) * n_layers; ++gi) {
            const int nn = g->node_off[gi + 1] - g->node_off[gi], ne = g->edge_off[g->node_off[gi + 1]] - g->edge_off[g->node_off[gi]];
            progs += cppn_program_bytes(nn, ne);
            mn = std::max(mn, nn);
        }
        const size_t lds = (size_t)mn * CPPN_THREADS * sizeof(double) + progs;
        if (lds > 160 * 1024) return fail(EIGEN_ERR_CAPACITY, "sample %d: %d nodes in its larger program need %zu B of LDS (> 160 KiB)", b, mn, lds);
        x.lds = std::max(x.lds, lds);
    }
    HIPCHK(hipSetDevice(e->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    CppnMotionArgs a;
    rc = upload_genomes(e, g, x, st);
    if (rc != EIGEN_OK) return rc;
    GENOME_ARGS(a);
    // one record of twelve per sample, frame and layer: the affine, then its inverse (zeros without a flow, never read)
    const size_t n_aff = (size_t)n * n_frames * n_layers;
    std::vector<double>& packed = e->h_affine;
    packed.assign(n_aff * 12, 0.0);
    for (size_t i = 0; i < n_aff; ++i) {
        std::copy(h_affine + i * 6, h_affine + i * 6 + 6, packed.begin() + i * 12);
        if (d_flow) std::copy(h_affine_inv + i * 6, h_affine_inv + i * 6 + 6, packed.begin() + i * 12 + 6);
    }
    if (e->g_affine.ensure(n_aff * 12)) return fail(EIGEN_ERR_HIP, "hipMalloc for the affines failed");
    HIPCHK(hipMemcpyAsync(e->g_affine.p, packed.data(), sizeof(double) * n_aff * 12, hipMemcpyHostToDevice, st));
    a.affine = e->g_affine.p;
    a.W = e->W; a.H = e->H; a.T = n_frames; a.L = n_layers;
    a.frames = d_frames; a.f_bstride = f_bstride; a.flow = d_flow; a.layer = d_layer;
    (void)hipFuncSetAttribute((const void*)cppn_motion_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)x.lds);
    hipLaunchKernelGGL(cppn_motion_kernel, dim3((a.N + CPPN_THREADS - 1) / CPPN_THREADS, n), dim3(CPPN_THREADS), x.lds, st, a);
    HIPCHK(hipGetLastError());
    return EIGEN_OK;
}

int eigen_moving_cppn_valid(eigen_engine* e, int32_t n, int32_t n_frames, int32_t n_layers, const double* h_affine, const double* h_affine_inv, uint8_t* d_valid,
                            void* stream)
{
    if (!e || !h_affine || !h_affine_inv || !d_valid) return fail(EIGEN_ERR_INVALID, "null argument");
    if (n_layers < 1 || n_layers > 2) return fail(EIGEN_ERR_INVALID, "n_layers %d outside 1..2", n_layers);
    if (n_frames < 2) return fail(EIGEN_ERR_INVALID, "a validity plane needs two frames, n_frames is %d", n_frames);
    if (n < 1) return fail(EIGEN_ERR_INVALID, "n %d < 1", n);
    if (n > 65535) return fail(EIGEN_ERR_CAPACITY, "n %d exceeds the 65535 samples of one launch", n);
    HIPCHK(hipSetDevice(e->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    // the packed records of eigen_render_moving_cppn: the affine, then its inverse
    const size_t n_aff = (size_t)n * n_frames * n_layers;
    std::vector<double>& packed = e->h_valid_affine;
    packed.resize(n_aff * 12);
    for (size_t i = 0; i < n_aff; ++i) {
        std::copy(h_affine + i * 6, h_affine + i * 6 + 6, packed.begin() + i * 12);
        std::copy(h_affine_inv + i * 6, h_affine_inv + i * 6 + 6, packed.begin() + i * 12 + 6);
    }
    if (e->g_valid_affine.ensure(n_aff * 12)) return fail(EIGEN_ERR_HIP, "hipMalloc for the affines failed");
    HIPCHK(hipMemcpyAsync(e->g_valid_affine.p, packed.data(), sizeof(double) * n_aff * 12, hipMemcpyHostToDevice, st));
    CppnValidArgs a;
    a.affine = e->g_valid_affine.p;
    a.W = e->W; a.H = e->H; a.N = e->H * e->W; a.T = n_frames; a.L = n_layers;
    a.valid = d_valid;
    hipLaunchKernelGGL(cppn_valid_kernel, dim3((a.N + CPPN_THREADS - 1) / CPPN_THREADS, n), dim3(CPPN_THREADS), 0, st, a);
    HIPCHK(hipGetLastError());
    return EIGEN_OK;
}

int eigen_cppn_param_grads(eigen_engine* e, const eigen_genome_batch* g, int32_t bg, int32_t gradient, const float* d_image_grad, int64_t g_bstride,
                           double* h_grad_bias, double* h_grad_resp, double* h_grad_w, void* stream)
{
    if (!e || !g || !d_image_grad || !h_grad_bias || !h_grad_resp || !h_grad_w) return fail(EIGEN_ERR_INVALID, "null argument");
    if (!e->have_grid) return fail(EIGEN_ERR_STATE, "eigen_set_grid has not been called");
    if (gradient != 1) return fail(EIGEN_ERR_INVALID, "gradient %d: only the gradient = 1 render is differentiable (not the palette, the rounded gray or the h,s,v renderer)", gradient);
    const long long per = (long long)e->C0 * e->H * e->W;
    if (g_bstride < per) return fail(EIGEN_ERR_INVALID, "g_bstride %lld < C*H*W = %lld", (long long)g_bstride, per);
    hipStream_t st = (hipStream_t)stream;
    GenomeExtent x;
    CppnGradArgs ga;
    const int rc = stage_genomes(e, g, e->C0, grad_lds, st, x, ga.c);
    if (rc != EIGEN_OK) return rc;
    ga.c.bg = bg; ga.c.mode = 0;   // (the fill itself never reaches a gradient: background pixels get no seed)
    ga.c.out = nullptr; ga.c.out_f64 = nullptr;
    const int n_blocks = (ga.c.N + CPPN_GRAD_THREADS - 1) / CPPN_GRAD_THREADS;
    const size_t n_params = 2 * (size_t)x.total_nodes + x.total_edges;
    if (e->g_grad_slabs.ensure((size_t)n_blocks * n_params) || e->g_grad_sum.ensure(n_params))
        return fail(EIGEN_ERR_HIP, "hipMalloc(%zu) for the gradient slabs failed", (size_t)n_blocks * n_params * sizeof(double));
    ga.image_grad = d_image_grad; ga.g_bstride = g_bstride; ga.total_nodes = x.total_nodes; ga.total_edges = x.total_edges; ga.slabs = e->g_grad_slabs.p;
    (void)hipFuncSetAttribute((const void*)cppn_grad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)x.lds);
    hipLaunchKernelGGL(cppn_grad_kernel, dim3(n_blocks, g->n_genomes), dim3(CPPN_GRAD_THREADS), x.lds, st, ga);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(cppn_grad_sum_kernel, dim3((unsigned)((n_params + 255) / 256)), dim3(256), 0, st, e->g_grad_slabs.p, e->g_grad_sum.p, (int)n_params, n_blocks);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_grad_bias, e->g_grad_sum.p, sizeof(double) * x.total_nodes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_grad_resp, e->g_grad_sum.p + x.total_nodes, sizeof(double) * x.total_nodes, hipMemcpyDeviceToHost, st));
    if (x.total_edges) HIPCHK(hipMemcpyAsync(h_grad_w, e->g_grad_sum.p + 2 * (size_t)x.total_nodes, sizeof(double) * x.total_edges, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return EIGEN_OK;
}

}  // extern "C"

// What one roll-out runs (eigen_prednet_rollout, eigen_prednet_sequence).  The input of step t < n_in is the uint8 image
// in + b * in_bstride + t * in_tstride (elements) of state slot b; every later step is fed the previous prediction (cfg.requant_feedback).
struct RollSnap {
    int step = -1;          // the roll-out step behind whose ConvP0 launch the gray of the float prediction P0 is taken (-1: none)
    double* dst = nullptr;  // [batch][H][W] float64 (dense_stage.h, dense_gray_launch)
};

struct RollPlan {
    RollSnap snap[2];  // the float frames of the dense fitness (EIGEN_DENSE_FLOAT_FRAMES); a roll-out that names none launches what it always did
    const uint8_t* in;
    long long in_bstride, in_tstride;
    int batch, n_in, n_steps, first_out;
    uint8_t* out;     // [batch][n_steps - first_out][C0][H][W]
    bool reset;       // start from reset_state(); otherwise from the state the previous roll-out of the same batch left
    bool keep_state;  // leave a state the next roll-out can continue from: the last step also runs ConvP_l (l > 0), on the caller's stream
};

static int prednet_run(eigen_engine* e, const RollPlan& p, hipStream_t st)
{
    const int L = e->L;
    const size_t HW = (size_t)e->H * e->W;
    const int batch = p.batch, n_steps = p.n_steps, first_out_step = p.first_out;
    const int n_out = n_steps - first_out_step;
    if (p.reset) {
        for (int l = 0; l < L; ++l) {  // reset_state()
            Layer& y = e->layer[l];
            const size_t n = (size_t)batch * y.C * y.H * y.W * sizeof(float);
            HIPCHK(hipMemsetAsync(y.h[0], 0, n, st));
            HIPCHK(hipMemsetAsync(y.c, 0, n, st));
            HIPCHK(hipMemsetAsync(y.P, 0, n, st));
        }
    }
    int cur = p.reset ? 0 : e->hflip;  // h[cur] holds the state of the previous step
    // (The step's dependency chain is serial; only ConvP_l (l > 0) may leave it, onto the side stream below, and only for small launches.  Two half-populations on
    // two streams were byte-identical and slower or equal at every shape: profiles/r04_b_ab_pipe2.txt.)
    const Switches& sw = switches();
    if (p.reset) hipLaunchKernelGGL(e0_init_kernel, dim3(1024), dim3(256), 0, st, p.in, p.in_bstride, e->layer[0].E, e->C0, (int)HW, batch);
    else  // E_0 of the first step from the kept P_0 and the first input (the epilogue's arithmetic: e0_resume_kernel)
        hipLaunchKernelGGL(e0_resume_kernel, dim3(1024), dim3(256), 0, st, (const float*)e->layer[0].P, p.n_in > 0 ? p.in : nullptr, p.in_bstride,
                           e->cfg.requant_feedback, e->layer[0].E, e->C0, (int)HW, batch);
    HIPCHK(hipGetLastError());
    // ConvP_l (l > 0) on a side stream: pays where the launches are a fraction of a round of the chip -- configs[0] (pop 10 at 64 x 64: 10 to 40 blocks per launch) +7.5 %;
    // neutral at configs[1], -0.7 % at 160 x 120 colour pop 50, -2 % at the headline (profiles/r06_q_side_stream_ab.txt), as in round 3.  Hence: only while the layer-1 maps of
    // the batch are less than one block per CU.  A scheduling choice of the launch, not of the arithmetic.  EIGEN_SIDE_STREAM = 0 / 1 forces it (A/B, tests).
    const bool side_auto = L > 1 && (long long)batch * e->layer[1].H * e->layer[1].W < 512ll * e->n_cu;
    const bool side_on = (sw.side_stream >= 0 ? sw.side_stream != 0 : side_auto) && !e->profile_convs;
    // One PredNet step of genomes [b0, b0 + nb) on stream s; raw4: that range's partial-chain scratch.
    auto run_step = [&](int t, int b0, int nb, hipStream_t s, float* raw4) -> int {
        auto off = [&](float* p, const Layer& y, int mult = 1) { return p + (size_t)b0 * mult * y.C * y.H * y.W; };
        // the step-0 operators skip the sources that are zero after reset_state(): never on a kept state
        const bool t0 = (t == 0 && p.reset && sw.skip_zero_sources);
        // bottom-up: E_l from E_{l-1} and the previous prediction P_l
        for (int l = 1; l < L; ++l) {
            Layer& y = e->layer[l];
            ConvArgs a;
            memset(&a, 0, sizeof(a));
            a.src[0].ptr = off(e->layer[l - 1].E, e->layer[l - 1], 2);
            a.bias = y.biasA.p; a.P = off(y.P, y); a.E = off(y.E, y, 2);
            // P_l of the previous step came from the side stream (a call's last step never forks: nothing is pending at its start)
            if (side_on && t > 0) HIPCHK(hipStreamWaitEvent(s, e->ev_join[l], 0));
            HIPCHK(launch_conv(e, t0 ? y.convA_t0 : y.convA, a, nb, s));
        }
        // top-down: R_l, then P_l
        for (int l = L - 1; l >= 0; --l) {
            Layer& y = e->layer[l];
            {
                ConvArgs a;
                memset(&a, 0, sizeof(a));
                int k = 0;
                if (l < L - 1 && y.lstm.fused) {  // R_{l+1} of THIS step: its chain runs inside the ConvLSTM launch
                    a.up_src = off(e->layer[l + 1].h[cur ^ 1], e->layer[l + 1]);
                    a.up_C = y.lstm.up_C; a.up_kb = y.lstm.up_kb;
                } else if (l < L - 1) {  // R_{l+1} of THIS step, 2x2 form -> partial chains
                    ConvArgs u;
                    memset(&u, 0, sizeof(u));
                    u.src[0].ptr = off(e->layer[l + 1].h[cur ^ 1], e->layer[l + 1]);
                    u.raw = raw4;
                    HIPCHK(launch_conv(e, y.up4, u, nb, s));
                    a.acc_init = raw4;
                }
                a.src[k++].ptr = off(y.E, y, 2);
                if (!t0) a.src[k++].ptr = off(y.h[cur], y);
                a.bias = y.bias_lstm.p; a.c_state = off(y.c, y); a.h_out = off(y.h[cur ^ 1], y); a.peep = y.peep.p;
                HIPCHK(launch_conv(e, t0 ? y.lstm_t0 : y.lstm, a, nb, s));
            }
            // P_l (l > 0) is only read by ConvA_l of the NEXT step: nothing in this roll-out reads it after the last one
            const bool last = t + 1 == n_steps;
            if (l == 0 || !last || p.keep_state) {
                ConvArgs a;
                memset(&a, 0, sizeof(a));
                a.src[0].ptr = off(y.h[cur ^ 1], y);
                a.bias = y.biasP.p; a.Pout = off(y.P, y); a.clip = (l == 0) ? 1 : 0;
                if (l == 0) {
                    if (!last) {  // error units of the next step
                        a.E0 = off(y.E, y, 2);
                        a.img = (t + 1 < p.n_in) ? p.in + (size_t)b0 * p.in_bstride + (size_t)(t + 1) * p.in_tstride : nullptr;
                        a.img_bstride = p.in_bstride;
                        a.requant = e->cfg.requant_feedback;
                    }
                    if (t >= first_out_step) {
                        a.frame_bstride = (long long)n_out * e->C0 * HW;
                        a.frame = p.out + (size_t)b0 * a.frame_bstride + (size_t)(t - first_out_step) * e->C0 * HW;
                    }
                }
                if (side_on && l > 0 && !last) {   // fork: behind the ConvLSTM that produced R_l, beside everything that follows on the main stream
                    HIPCHK(hipEventRecord(e->ev_fork, s));
                    HIPCHK(hipStreamWaitEvent(e->side, e->ev_fork, 0));
                    HIPCHK(launch_conv(e, y.convP, a, nb, e->side));
                    HIPCHK(hipEventRecord(e->ev_join[l], e->side));
                } else
                HIPCHK(launch_conv(e, y.convP, a, nb, s));
                if (l == 0)  // ConvP0 never leaves the step's stream: the snapshot reads P0 behind it, before the next step overwrites it
                    for (const RollSnap& g : p.snap)
                        if (g.dst && g.step == t) eigd::dense_gray_launch((const float*)off(y.P, y), (long long)e->C0 * HW, e->C0, e->H, e->W, nb, g.dst + (size_t)b0 * HW, s);
            }
        }
        return EIGEN_OK;
    };
    for (int t = 0; t < n_steps; ++t) {
        const int rc = run_step(t, 0, batch, st, e->raw4.p);
        if (rc) return rc;
        cur ^= 1;
    }
    e->hflip = cur;
    return EIGEN_OK;
}

// eigen_prednet_rollout; snaps (may be null): the gray snapshots of a float dense call
static int prednet_rollout_impl(eigen_engine* e, const uint8_t* d_images, int32_t batch, int32_t n_steps, int32_t first_out_step, uint8_t* d_frames, void* stream,
                                const RollSnap* snaps)
{
    if (!e || !d_images || !d_frames) return fail(EIGEN_ERR_INVALID, "null argument");
    if (!e->have_weights) return fail(EIGEN_ERR_STATE, "eigen_set_prednet_weights has not been called");
    if (batch < 1 || batch > e->B) return fail(EIGEN_ERR_CAPACITY, "batch %d exceeds max_batch %d", batch, e->B);
    if (n_steps < 1 || n_steps > e->cfg.n_repeat + e->cfg.n_ext) return fail(EIGEN_ERR_INVALID, "n_steps %d out of range", n_steps);
    if (first_out_step < 0 || first_out_step >= n_steps) return fail(EIGEN_ERR_INVALID, "first_out_step %d out of range", first_out_step);
    HIPCHK(hipSetDevice(e->cfg.device));
    e->seq_batch = 0;  // the layer state is overwritten: no eigen_prednet_sequence call may continue from it
    RollPlan p;
    p.in = d_images; p.in_bstride = (long long)e->C0 * e->H * e->W; p.in_tstride = 0;  // one still image per genome
    p.batch = batch; p.n_in = std::min(e->cfg.n_repeat, (int)n_steps); p.n_steps = n_steps; p.first_out = first_out_step; p.out = d_frames;
    p.reset = true; p.keep_state = false;
    if (snaps) { p.snap[0] = snaps[0]; p.snap[1] = snaps[1]; }
    return prednet_run(e, p, (hipStream_t)stream);
}

extern "C" {

int eigen_prednet_rollout(eigen_engine* e, const uint8_t* d_images, int32_t batch, int32_t n_steps, int32_t first_out_step,
                          uint8_t* d_frames, void* stream)
{
    return prednet_rollout_impl(e, d_images, batch, n_steps, first_out_step, d_frames, stream, nullptr);
}

int eigen_prednet_sequence(eigen_engine* e, const uint8_t* d_in, int64_t in_bstride, int32_t batch, int32_t n_in, int32_t n_ext,
                           int32_t reset, int32_t first_out_step, uint8_t* d_out, void* stream)
{
    if (!e || !d_out || (n_in > 0 && !d_in)) return fail(EIGEN_ERR_INVALID, "null argument");
    if (!e->have_weights) return fail(EIGEN_ERR_STATE, "eigen_set_prednet_weights has not been called");
    if (batch < 1 || batch > e->B) return fail(EIGEN_ERR_CAPACITY, "batch %d exceeds max_batch %d", batch, e->B);
    if (n_in < 0 || n_ext < 0) return fail(EIGEN_ERR_INVALID, "n_in %d and n_ext %d must be >= 0", n_in, n_ext);
    if (reset && n_in == 0) return fail(EIGEN_ERR_INVALID, "a call that resets the state needs at least one input frame (n_in = 0)");
    if (in_bstride < 0) return fail(EIGEN_ERR_INVALID, "in_bstride %lld < 0", (long long)in_bstride);
    const long long n_steps = (long long)n_in + n_ext;
    if (n_steps < 1 || n_steps > INT32_MAX) return fail(EIGEN_ERR_INVALID, "n_in + n_ext = %lld steps out of range", n_steps);
    if (first_out_step < 0 || first_out_step >= n_steps) return fail(EIGEN_ERR_INVALID, "first_out_step %d out of range (0..%lld)", first_out_step, n_steps - 1);
    if (!reset && e->seq_batch != batch) {
        if (e->seq_batch == 0) return fail(EIGEN_ERR_STATE, "reset = 0: no state to continue from (none kept yet, or a roll-out / evaluation overwrote it)");
        return fail(EIGEN_ERR_STATE, "reset = 0: the kept state is of a batch of %d, not %d", e->seq_batch, batch);
    }
    HIPCHK(hipSetDevice(e->cfg.device));
    e->seq_batch = 0;  // valid again only once every step of this call has been enqueued
    RollPlan p;
    p.in = d_in; p.in_bstride = in_bstride; p.in_tstride = (long long)e->C0 * e->H * e->W;
    p.batch = batch; p.n_in = n_in; p.n_steps = (int)n_steps; p.first_out = first_out_step; p.out = d_out;
    p.reset = reset != 0; p.keep_state = true;
    const int rc = prednet_run(e, p, (hipStream_t)stream);
    if (rc) return rc;
    e->seq_batch = batch;
    return EIGEN_OK;
}

// Dense Farneback flow between the gray images d_gray[0][0] -> d_gray[1][0], sampled into vectors (farneback_kernels.h)
static int farneback_flow(eigen_engine* e, int batch, float* d_vectors, int32_t* d_counts, hipStream_t st)
{
    const int H = e->H, W = e->W;
    const size_t HW = (size_t)H * W, B = (size_t)e->B;
    const eigen_config& c = e->cfg;
    if (!e->fb_I) {
        hipError_t r = hipMalloc((void**)&e->fb_I, B * HW * sizeof(float));
        float** five[] = {&e->fb_R0, &e->fb_R1, &e->fb_M, &e->fb_V};
        for (float** p : five) if (r == hipSuccess) r = hipMalloc((void**)p, B * 5 * HW * sizeof(float));
        for (int i = 0; i < 2 && r == hipSuccess; ++i) r = hipMalloc((void**)&e->fb_flow[i], B * 2 * HW * sizeof(float));
        if (r != hipSuccess) return fail(EIGEN_ERR_HIP, "hipMalloc for the Farneback workspaces: %s", hipGetErrorString(r));
    }
    const int levels = fb_levels_used(H, W, c.fb_levels);
    const FbConst pc = fb_poly_constants(c.fb_poly_n, c.fb_poly_sigma);
    const int m = c.fb_winsize / 2;
    int cur = 0;
    for (int k = levels; k >= 0; --k) {
        const int Hk = H >> k, Wk = W >> k, hw = Hk * Wk;
        const dim3 g1((hw + 255) / 256, batch);
        float* fl = e->fb_flow[cur];
        if (k == levels) HIPCHK(hipMemsetAsync(fl, 0, (size_t)batch * 2 * hw * sizeof(float), st));
        else hipLaunchKernelGGL(fb_upsample_kernel, g1, dim3(256), 0, st, e->fb_flow[cur ^ 1], H >> (k + 1), W >> (k + 1), fl, Hk, Wk);
        const FbBlur bl = fb_blur_kernel(k);
        const dim3 gp((Wk + FB_PX - 1) / FB_PX, (Hk + FB_PY - 1) / FB_PY, batch);
        for (int i = 0; i < 2; ++i) {
            hipLaunchKernelGGL(fb_blur_down_kernel, g1, dim3(256), 0, st, e->d_gray[i][0], H, W, k, bl, e->fb_I);
            hipLaunchKernelGGL(fb_polyexp_kernel, gp, dim3(FB_PX, FB_PY), 0, st, e->fb_I, Hk, Wk, pc, i == 0 ? e->fb_R0 : e->fb_R1);
        }
        hipLaunchKernelGGL(fb_update_matrices_kernel, g1, dim3(256), 0, st, e->fb_R0, e->fb_R1, fl, Hk, Wk, e->fb_M);
        for (int it = 0; it < c.fb_iterations; ++it) {
            hipLaunchKernelGGL(fb_box_v_kernel, g1, dim3(256), 0, st, e->fb_M, Hk, Wk, m, e->fb_V);
            hipLaunchKernelGGL(fb_box_h_solve_kernel, dim3((Wk + FB_HT - 1) / FB_HT, Hk, batch), dim3(FB_HT), 0, st, e->fb_V, Hk, Wk, m, fl);
            if (it + 1 < c.fb_iterations) hipLaunchKernelGGL(fb_update_matrices_kernel, g1, dim3(256), 0, st, e->fb_R0, e->fb_R1, fl, Hk, Wk, e->fb_M);
        }
        cur ^= 1;
    }
    const int step = fb_grid_step(H, W, c.fb_step, e->K);
    hipLaunchKernelGGL(fb_sample_kernel, dim3(batch), dim3(64), 0, st, e->fb_flow[cur ^ 1], H, W, step, e->K, d_vectors, d_counts);
    HIPCHK(hipGetLastError());
    return EIGEN_OK;
}

int eigen_flow(eigen_engine* e, const uint8_t* d_img0, int64_t stride0, const uint8_t* d_img1, int64_t stride1, int32_t batch,
               float* d_vectors, int32_t* d_counts, void* stream)
{
    if (!e || !d_img0 || !d_img1 || !d_vectors || !d_counts) return fail(EIGEN_ERR_INVALID, "null argument");
    if (batch < 1 || batch > e->B) return fail(EIGEN_ERR_CAPACITY, "batch %d exceeds max_batch %d", batch, e->B);
    HIPCHK(hipSetDevice(e->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    const int H = e->H, W = e->W, HW = H * W;
    const eigen_config& c = e->cfg;
    hipLaunchKernelGGL(gray_kernel, dim3((HW + 255) / 256, batch), dim3(256), 0, st, d_img0, (long long)stride0, e->C0, HW, e->d_gray[0][0], batch);
    hipLaunchKernelGGL(gray_kernel, dim3((HW + 255) / 256, batch), dim3(256), 0, st, d_img1, (long long)stride1, e->C0, HW, e->d_gray[1][0], batch);
    if (c.flow_method == EIGEN_FLOW_FARNEBACK) return farneback_flow(e, batch, d_vectors, d_counts, st);
    for (int l = 1; l < e->n_levels; ++l)
        for (int i = 0; i < 2; ++i)
            hipLaunchKernelGGL(pyrdown_kernel, dim3((e->lvH[l] * e->lvW[l] + 255) / 256, batch), dim3(256), 0, st, e->d_gray[i][l - 1],
                               e->lvH[l - 1], e->lvW[l - 1], e->d_gray[i][l], e->lvH[l], e->lvW[l]);
    for (int l = 0; l < e->n_levels; ++l)
        hipLaunchKernelGGL(scharr_kernel, dim3((e->lvH[l] * e->lvW[l] + 255) / 256, batch), dim3(256), 0, st, e->d_gray[0][l], e->lvH[l], e->lvW[l], e->d_deriv[l]);
    const double sc = 1.0 / ((double)(1 << 2) * c.lk_block_size * 255.0);
    const float SC = (float)(sc * sc);
    hipLaunchKernelGGL(mineig_kernel, dim3((W + EIG_T - 1) / EIG_T, (H + EIG_T - 1) / EIG_T, batch), dim3(256), 0, st, e->d_gray[0][0], H, W,
                       c.lk_block_size, SC, e->d_eig);
    hipLaunchKernelGGL(corner_select_kernel, dim3(batch), dim3(1024), 0, st, e->d_eig, H, W, c.lk_quality_level, (float)c.lk_min_distance,
                       c.lk_max_corners, e->d_cand, e->d_corners, e->d_ncorners);
    LKArgs a;
    memset(&a, 0, sizeof(a));
    for (int l = 0; l < e->n_levels; ++l) {
        a.I[l] = e->d_gray[0][l]; a.J[l] = e->d_gray[1][l]; a.dI[l] = e->d_deriv[l];
        a.Hs[l] = e->lvH[l]; a.Ws[l] = e->lvW[l];
    }
    a.max_level = e->n_levels - 1; a.win = c.lk_win; a.K = e->K;
    a.max_iter = std::min(std::max(c.lk_max_iter, 0), 100);
    const double eps = std::min(std::max(c.lk_epsilon, 0.0), 10.0);
    a.eps_sq = eps * eps; a.min_eig_thr = c.lk_min_eig_thr;
    a.corners = e->d_corners; a.ncorners = e->d_ncorners; a.next_pts = e->d_next; a.status = e->d_status;
    hipLaunchKernelGGL(lk_track_kernel, dim3(e->K, batch), dim3(64), 0, st, a);
    hipLaunchKernelGGL(compact_vectors_kernel, dim3(batch), dim3(128), 0, st, e->d_corners, e->d_next, e->d_status, e->d_ncorners, e->K, d_vectors, d_counts);
    HIPCHK(hipGetLastError());
    return EIGEN_OK;
}

int eigen_score(eigen_engine* e, int32_t structure, int32_t width, int32_t height, const float* d_vectors, const int32_t* d_counts, int32_t batch,
                double* d_fitness, void* stream)
{
    if (!e || !d_vectors || !d_counts || !d_fitness) return fail(EIGEN_ERR_INVALID, "null argument");
    if (structure < 0 || structure > EIGEN_SCORE_INSIDE_OUTSIDE)
        return fail(EIGEN_ERR_INVALID, "unknown structure %d (the reference raises NameError, generate_illusion.py:606-607)", structure);
    if (batch < 1) return fail(EIGEN_ERR_INVALID, "batch < 1");
    HIPCHK(hipSetDevice(e->cfg.device));
    ScoreArgs a;
    a.vectors = d_vectors; a.counts = d_counts; a.K = e->K; a.structure = structure; a.w = width > 0 ? width : e->W; a.h = height > 0 ? height : e->H; a.fitness = d_fitness;
    if (structure == EIGEN_SCORE_INSIDE_OUTSIDE) {
        const double step = (double)a.w / 5.0;
        const long cells = ((long)((double)a.w / step) + 1) * ((long)((double)a.h / step) + 1);
        if (cells > IO_MAX_CELLS) return fail(EIGEN_ERR_CAPACITY, "inside_outside_score: %ld cells of %dx%d exceed %d", cells, a.w, a.h, IO_MAX_CELLS);
        hipLaunchKernelGGL(inside_outside_kernel, dim3(batch), dim3(64), 0, (hipStream_t)stream, a);
        HIPCHK(hipGetLastError());
        return EIGEN_OK;
    }
    hipLaunchKernelGGL(score_kernel, dim3(batch), dim3(SCORE_T), 0, (hipStream_t)stream, a);
    HIPCHK(hipGetLastError());
    return EIGEN_OK;
}

// The dense fitness's workspace (dense_stage.h), made by the first call that needs it: the handle takes the buffers once every one of
// them exists, a failure frees what it made.
static int dense_workspace(eigen_engine* e)
{
    if (e->have_dense) return EIGEN_OK;
    const size_t n = (size_t)e->B * e->H * e->W;
    eigd::DenseWork& w = e->dense;
    const std::pair<void**, size_t> want[] = {{(void**)&w.planes, 3 * n * 8}, {(void**)&w.u, 2 * n * 8}, {(void**)&w.theta, n * 8}, {(void**)&w.L, n * 8},
                                              {(void**)&w.rec, (size_t)e->B * eigd::DENSE_REC * 8}, {(void**)&w.part, (size_t)e->B * eigd::DENSE_PART * 8},
                                              {(void**)&w.flag, n}};
    std::vector<void*> made;
    for (const auto& x : want) {
        void* p = nullptr;
        const hipError_t err = hipMalloc(&p, x.second);
        if (err != hipSuccess) {
            for (void* q : made) (void)hipFree(q);
            return fail(EIGEN_ERR_HIP, "hipMalloc(%zu) for the dense fitness: %s", x.second, hipGetErrorString(err));
        }
        made.push_back(p);
    }
    for (size_t i = 0; i < made.size(); ++i) *want[i].first = made[i];
    e->have_dense = true;
    return EIGEN_OK;
}

// The pyramid of the iterated solve, made by the first call that asks for one: one block, so all of it or none
static int dense_pyramid(eigen_engine* e)
{
    if (e->dense.pyr) return EIGEN_OK;
    const size_t bytes = (size_t)eigd::pyr_doubles(e->B, e->H, e->W) * 8;
    void* p = nullptr;
    const hipError_t err = hipMalloc(&p, bytes);
    if (err != hipSuccess) return fail(EIGEN_ERR_HIP, "hipMalloc(%zu) for the dense fitness's pyramid: %s", bytes, hipGetErrorString(err));
    e->dense.pyr = (double*)p;
    return EIGEN_OK;
}

// The one record behind the plain dense entries, their _iter and their _members forms: the settings, the mask, the checked solve and the
// checked members of a call
struct DenseCall {
    const eigen_dense_settings* settings = nullptr;
    const uint8_t* d_mask = nullptr;
    eigd::DenseSolve solve;
    eigd::DenseMembers mem;
    bool float_frames = false;  // EIGEN_DENSE_FLOAT_FRAMES: the stage starts from the gray planes at dense_gray_planes
};

// What every dense entry refuses before anything is launched (the roll-out included), then the workspace
// float_entry: 0 a byte entry, which refuses EIGEN_DENSE_FLOAT_FRAMES; 1 an eval entry, which takes the flag or 0; 2 eigen_dense_score_float, float with
// either, 3 the same with a float img0.  A float call's own workspace comes last, behind every refusal.
static int dense_prepare(eigen_engine* e, DenseCall& c, const eigen_dense_settings* settings, const eigen_dense_solve* solve, const uint8_t* d_mask, int batch,
                         const eigen_flow_members* members = nullptr, int float_entry = 0)
{
    if (!settings) return fail(EIGEN_ERR_INVALID, "null argument");
    if (batch < 1 || batch > e->B) return fail(EIGEN_ERR_INVALID, "batch %d outside 1 .. max_batch %d", batch, e->B);
    HIPCHK(hipSetDevice(e->cfg.device));
    c.settings = settings; c.d_mask = d_mask;
    // without members dense_check_members is dense_check; with them the members' buffers come behind every refusal
    int rc = eigd::dense_check_members(settings, solve, e->dense_force_iter, e->cfg.device, e->C0, e->H, e->W, e->B, d_mask, members, batch, e->dense, c.solve, c.mem,
                                       float_entry ? EIGEN_DENSE_FLOAT_FRAMES : 0);
    if (rc) return rc;
    c.float_frames = float_entry >= 2 || (settings->flow.flags & EIGEN_DENSE_FLOAT_FRAMES) != 0;
    rc = dense_workspace(e);
    if (rc) return rc;
    if (c.solve.iterated) {
        rc = dense_pyramid(e);
        if (rc) return rc;
    }
    if (!c.float_frames) {
        if (c.solve.iterated) e->dense_gray_batch = 0;  // level 0 of the pyramid is about to hold the gray of bytes
        return EIGEN_OK;
    }
    rc = eigd::dense_gray_workspace(e->cfg.device, e->H, e->W, e->B, c.solve, float_entry == 3, c.mem.by_corners, e->C0, e->dense);
    return rc;
}

// The stage on a prepared call, and its host outputs: S_b alone comes back where the records are not asked for
// (a float call: the gray planes of the pair are in place or enqueued on st; d_img0 is the byte image the corner members are picked on, d_img1 is not read)
static int dense_run(eigen_engine* e, const uint8_t* d_img0, int64_t stride0, const uint8_t* d_img1, int64_t stride1, int batch, const DenseCall& c, double* h_fitness,
                     double* h_stats, double* d_flow, hipStream_t st, bool sync)
{
    if (c.float_frames) {
        eigd::dense_launch_gray(c.settings, c.solve, e->C0, e->H, e->W, d_img0, (long long)stride0, batch, c.d_mask, e->dense, d_flow, st, c.mem);
        double *I0, *I1;
        eigd::dense_gray_planes(e->dense, c.solve, e->H, e->W, batch, I0, I1);
        e->dense_gray_at = I0; e->dense_gray_batch = batch;
    } else
    eigd::dense_launch(c.settings, c.solve, e->C0, e->H, e->W, d_img0, (long long)stride0, d_img1, (long long)stride1, batch, c.d_mask, e->dense, d_flow, st,
                       c.mem);
    HIPCHK(hipGetLastError());
    const size_t rec = eigd::DENSE_REC * sizeof(double);
    if (h_stats) HIPCHK(hipMemcpyAsync(h_stats, e->dense.rec, rec * batch, hipMemcpyDeviceToHost, st));
    if (h_fitness && !h_stats) HIPCHK(hipMemcpy2DAsync(h_fitness, sizeof(double), e->dense.rec + 8, rec, sizeof(double), batch, hipMemcpyDeviceToHost, st));
    if ((h_stats || h_fitness) && sync) {
        HIPCHK(hipStreamSynchronize(st));
        if (h_fitness && h_stats)
            for (int b = 0; b < batch; ++b) h_fitness[b] = h_stats[(size_t)b * eigd::DENSE_REC + 8];
    }
    return EIGEN_OK;
}

int eigen_dense_score_members(eigen_engine* e, const uint8_t* d_img0, int64_t stride0, const uint8_t* d_img1, int64_t stride1, int32_t batch,
                              const eigen_dense_settings* settings, const uint8_t* d_mask, double* h_fitness, double* h_stats, double* d_flow, void* stream,
                              const eigen_dense_solve* solve, const eigen_flow_members* members, uint8_t* h_members, int32_t* h_counts)
{
    if (!e || !d_img0 || !d_img1 || !settings) return fail(EIGEN_ERR_INVALID, "null argument");
    const int64_t per = (int64_t)e->C0 * e->H * e->W;
    if (stride0 < per || stride1 < per) return fail(EIGEN_ERR_INVALID, "a batch stride is smaller than one image (%lld elements)", (long long)per);
    DenseCall c;
    int rc = dense_prepare(e, c, settings, solve, d_mask, batch, members);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = dense_run(e, d_img0, stride0, d_img1, stride1, batch, c, h_fitness, h_stats, d_flow, st, true);
    if (rc || !c.mem.by_corners || (!h_members && !h_counts)) return rc;
    // the corner members' planes and the corner counts before the mask, as eigen_trainer_flow_members gives them
    if (h_members) HIPCHK(hipMemcpyAsync(h_members, e->dense.c_member, (size_t)batch * e->H * e->W, hipMemcpyDeviceToHost, st));
    if (h_counts) HIPCHK(hipMemcpyAsync(h_counts, e->dense.c_count, (size_t)batch * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return EIGEN_OK;
}

int eigen_dense_score_iter(eigen_engine* e, const uint8_t* d_img0, int64_t stride0, const uint8_t* d_img1, int64_t stride1, int32_t batch,
                           const eigen_dense_settings* settings, const uint8_t* d_mask, double* h_fitness, double* h_stats, double* d_flow, void* stream,
                           const eigen_dense_solve* solve)
{
    return eigen_dense_score_members(e, d_img0, stride0, d_img1, stride1, batch, settings, d_mask, h_fitness, h_stats, d_flow, stream, solve, nullptr, nullptr, nullptr);
}

int eigen_dense_score(eigen_engine* e, const uint8_t* d_img0, int64_t stride0, const uint8_t* d_img1, int64_t stride1, int32_t batch,
                      const eigen_dense_settings* settings, const uint8_t* d_mask, double* h_fitness, double* h_stats, double* d_flow, void* stream)
{
    return eigen_dense_score_iter(e, d_img0, stride0, d_img1, stride1, batch, settings, d_mask, h_fitness, h_stats, d_flow, stream, nullptr);
}

int eigen_dense_score_float(eigen_engine* e, const uint8_t* d_img0, const float* d_fimg0, int64_t stride0, const float* d_img1, int64_t stride1, int32_t batch,
                            const eigen_dense_settings* settings, const eigen_dense_solve* solve, const eigen_flow_members* members, const uint8_t* d_mask,
                            double* h_fitness, double* h_stats, double* d_flow, void* stream)
{
    if (!e || !d_img1 || !settings) return fail(EIGEN_ERR_INVALID, "null argument");
    if ((d_img0 != nullptr) == (d_fimg0 != nullptr)) return fail(EIGEN_ERR_INVALID, "exactly one of d_img0 (bytes) and d_fimg0 (floats) must be given");
    const int64_t per = (int64_t)e->C0 * e->H * e->W;
    if (stride0 < per || stride1 < per) return fail(EIGEN_ERR_INVALID, "a batch stride is smaller than one image (%lld elements)", (long long)per);
    DenseCall c;
    int rc = dense_prepare(e, c, settings, solve, d_mask, batch, members, d_fimg0 ? 3 : 2);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    double *I0, *I1;
    eigd::dense_gray_planes(e->dense, c.solve, e->H, e->W, batch, I0, I1);
    e->dense_gray_batch = 0;
    if (d_fimg0) eigd::dense_gray_launch(d_fimg0, (long long)stride0, e->C0, e->H, e->W, batch, I0, st);
    else eigd::dense_gray_launch(d_img0, (long long)stride0, e->C0, e->H, e->W, batch, I0, st);
    eigd::dense_gray_launch(d_img1, (long long)stride1, e->C0, e->H, e->W, batch, I1, st);
    if (d_fimg0 && c.mem.by_corners) {  // the corners are picked on the byte image of img0, as the trainer's membership stage does for a float reference
        eigd::dense_quant_launch(d_fimg0, (long long)stride0, e->C0, e->H, e->W, batch, e->dense, st);
        d_img0 = e->dense.fbytes; stride0 = per;
    }
    return dense_run(e, d_img0, stride0, nullptr, 0, batch, c, h_fitness, h_stats, d_flow, st, true);
}

int eigen_debug_dense_gray(eigen_engine* e, int32_t batch, double* h_I0, double* h_I1, void* stream)
{
    if (!e || !h_I0 || !h_I1) return fail(EIGEN_ERR_INVALID, "null argument");
    if (!e->dense_gray_batch) return fail(EIGEN_ERR_STATE, "no float dense call has left its gray planes on this handle (or an iterated byte call overwrote them)");
    if (batch != e->dense_gray_batch) return fail(EIGEN_ERR_STATE, "the last float dense call was of a batch of %d, not %d", e->dense_gray_batch, batch);
    HIPCHK(hipSetDevice(e->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)batch * e->H * e->W;
    HIPCHK(hipMemcpyAsync(h_I0, e->dense_gray_at, n * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_I1, e->dense_gray_at + n, n * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return EIGEN_OK;
}

// dense != nullptr: the dense stage (already prepared) in place of flow and score; h_stats is its records
static int eval_images_impl(eigen_engine* e, const uint8_t* d_images, int batch, int structure, int pairing, double* h_fitness,
                            float* h_vectors, int32_t* h_counts, hipStream_t st, bool rendered, const DenseCall* dense = nullptr, double* h_stats = nullptr)
{
    const size_t HW = (size_t)e->H * e->W, img_bytes = (size_t)e->C0 * HW;
    const int nr = e->cfg.n_repeat;
    int n_steps, first;
    if (pairing == EIGEN_PAIR_POPULATION) { n_steps = nr + 1; first = nr - 1; }  // prediction@n_repeat and 1st extension
    else { n_steps = nr + 2; first = nr + 1; }                                    // 2nd extension
    if (n_steps > nr + e->cfg.n_ext) return fail(EIGEN_ERR_INVALID, "pairing needs %d extension steps, engine has n_ext=%d", n_steps - nr, e->cfg.n_ext);
    if (!rendered) HIPCHK(hipEventRecord(e->ev[0], st));
    HIPCHK(hipEventRecord(e->ev[1], st));
    // float frames: the gray of P0 at the pair's steps, taken inside the roll-out (its entry of eigen_get_timings); under PAIR_SINGLE img0 is the input image
    RollSnap snaps[2];
    double *I0 = nullptr, *I1 = nullptr;
    if (dense && dense->float_frames) {
        eigd::dense_gray_planes(e->dense, dense->solve, e->H, e->W, batch, I0, I1);
        e->dense_gray_batch = 0;
        if (pairing == EIGEN_PAIR_POPULATION) { snaps[0].step = nr - 1; snaps[0].dst = I0; snaps[1].step = nr; snaps[1].dst = I1; }
        else { snaps[0].step = nr + 1; snaps[0].dst = I1; }
    }
    int rc = prednet_rollout_impl(e, d_images, batch, n_steps, first, e->d_frames, st, snaps);
    if (rc) return rc;
    HIPCHK(hipEventRecord(e->ev[2], st));
    const int n_out = n_steps - first;
    if (dense) {
        const int64_t fs = (int64_t)(n_out * img_bytes);
        if (dense->float_frames && pairing != EIGEN_PAIR_POPULATION) eigd::dense_gray_launch(d_images, (long long)img_bytes, e->C0, e->H, e->W, batch, I0, st);
        if (pairing == EIGEN_PAIR_POPULATION) rc = dense_run(e, e->d_frames, fs, e->d_frames + img_bytes, fs, batch, *dense, h_fitness, h_stats, nullptr, st, false);
        else rc = dense_run(e, d_images, (int64_t)img_bytes, e->d_frames, fs, batch, *dense, h_fitness, h_stats, nullptr, st, false);
        if (rc) return rc;
        HIPCHK(hipEventRecord(e->ev[3], st));
        HIPCHK(hipEventRecord(e->ev[4], st));
        HIPCHK(hipStreamSynchronize(st));
        if (h_stats)
            for (int b = 0; b < batch; ++b) h_fitness[b] = h_stats[(size_t)b * eigd::DENSE_REC + 8];
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, e->ev[0], e->ev[1])); e->ms[0] = ms;
        HIPCHK(hipEventElapsedTime(&ms, e->ev[1], e->ev[2])); e->ms[1] = ms;
        HIPCHK(hipEventElapsedTime(&ms, e->ev[2], e->ev[3])); e->ms[2] = ms;
        e->ms[3] = 0;
        return EIGEN_OK;
    }
    if (pairing == EIGEN_PAIR_POPULATION)
        rc = eigen_flow(e, e->d_frames, (int64_t)(n_out * img_bytes), e->d_frames + img_bytes, (int64_t)(n_out * img_bytes), batch, e->d_vectors, e->d_counts, st);
    else
        rc = eigen_flow(e, d_images, (int64_t)img_bytes, e->d_frames, (int64_t)(n_out * img_bytes), batch, e->d_vectors, e->d_counts, st);
    if (rc) return rc;
    HIPCHK(hipEventRecord(e->ev[3], st));
    rc = eigen_score(e, structure, 0, 0, e->d_vectors, e->d_counts, batch, e->d_fitness, st);
    if (rc) return rc;
    HIPCHK(hipEventRecord(e->ev[4], st));
    HIPCHK(hipMemcpyAsync(h_fitness, e->d_fitness, sizeof(double) * batch, hipMemcpyDeviceToHost, st));
    if (h_vectors) HIPCHK(hipMemcpyAsync(h_vectors, e->d_vectors, sizeof(float) * batch * e->K * 4, hipMemcpyDeviceToHost, st));
    if (h_counts) HIPCHK(hipMemcpyAsync(h_counts, e->d_counts, sizeof(int32_t) * batch, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e->ev[0], e->ev[1])); e->ms[0] = ms;
    HIPCHK(hipEventElapsedTime(&ms, e->ev[1], e->ev[2])); e->ms[1] = ms;
    HIPCHK(hipEventElapsedTime(&ms, e->ev[2], e->ev[3])); e->ms[2] = ms;
    HIPCHK(hipEventElapsedTime(&ms, e->ev[3], e->ev[4])); e->ms[3] = ms;
    return EIGEN_OK;
}

int eigen_eval_population(eigen_engine* e, const eigen_genome_batch* g, int32_t structure, int32_t bg, int32_t gradient, int32_t pairing,
                          double* h_fitness, void* stream)
{
    if (!e || !g || !h_fitness) return fail(EIGEN_ERR_INVALID, "null argument");
    if (g->n_genomes < 1 || g->n_genomes > e->B) return fail(EIGEN_ERR_CAPACITY, "batch %d exceeds max_batch %d", g->n_genomes, e->B);
    if (structure < 0 || structure > 3) return fail(EIGEN_ERR_INVALID, "unknown structure %d", structure);
    HIPCHK(hipSetDevice(e->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipEventRecord(e->ev[0], st));
    int rc = eigen_render_cppn(e, g, bg, gradient, e->d_images, st);
    if (rc) return rc;
    return eval_images_impl(e, e->d_images, g->n_genomes, structure, pairing, h_fitness, nullptr, nullptr, st, true);
}

int eigen_eval_images(eigen_engine* e, const uint8_t* d_images, int32_t batch, int32_t structure, int32_t pairing, double* h_fitness,
                      float* h_vectors, int32_t* h_counts, void* stream)
{
    if (!e || !d_images || !h_fitness) return fail(EIGEN_ERR_INVALID, "null argument");
    if (batch < 1 || batch > e->B) return fail(EIGEN_ERR_CAPACITY, "batch %d exceeds max_batch %d", batch, e->B);
    if (structure < 0 || structure > 3) return fail(EIGEN_ERR_INVALID, "unknown structure %d", structure);
    HIPCHK(hipSetDevice(e->cfg.device));
    return eval_images_impl(e, d_images, batch, structure, pairing, h_fitness, h_vectors, h_counts, (hipStream_t)stream, false);
}

// What the two population entries refuse ahead of the settings' own checks, the workspace and the render: a structure the settings'
// score does not belong to (settings with both scores or neither pass here and are refused by dense_prepare) and a pairing the
// handle's n_ext cannot serve (eval_images_impl's own rule and words)
static int dense_call_check(const eigen_engine* e, int structure, int pairing, const eigen_dense_settings* s)
{
    if (structure < 0 || structure > 3) return fail(EIGEN_ERR_INVALID, "unknown structure %d", structure);
    const bool circles = structure == EIGEN_CIRCLES || structure == EIGEN_CIRCLES_FREE;
    if ((s->score != nullptr) != (s->sscore != nullptr) && (circles ? s->score == nullptr : (s->sscore == nullptr || s->sscore->structure != structure)))
        return fail(EIGEN_ERR_INVALID, "structure %d: the dense settings carry the score of another structure", structure);
    const int need = pairing == EIGEN_PAIR_POPULATION ? 1 : 2;
    if (need > e->cfg.n_ext) return fail(EIGEN_ERR_INVALID, "pairing needs %d extension steps, engine has n_ext=%d", need, e->cfg.n_ext);
    return EIGEN_OK;
}

int eigen_eval_population_dense_members(eigen_engine* e, const eigen_genome_batch* g, int32_t structure, int32_t bg, int32_t gradient, int32_t pairing,
                                        const eigen_dense_settings* settings, const uint8_t* d_mask, double* h_fitness, double* h_stats, void* stream,
                                        const eigen_dense_solve* solve, const eigen_flow_members* members)
{
    if (!e || !g || !h_fitness || !settings) return fail(EIGEN_ERR_INVALID, "null argument");
    int rc = dense_call_check(e, structure, pairing, settings);
    if (rc) return rc;
    DenseCall c;
    rc = dense_prepare(e, c, settings, solve, d_mask, g->n_genomes, members, 1);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipEventRecord(e->ev[0], st));
    rc = eigen_render_cppn(e, g, bg, gradient, e->d_images, st);
    if (rc) return rc;
    return eval_images_impl(e, e->d_images, g->n_genomes, structure, pairing, h_fitness, nullptr, nullptr, st, true, &c, h_stats);
}

int eigen_eval_population_dense_iter(eigen_engine* e, const eigen_genome_batch* g, int32_t structure, int32_t bg, int32_t gradient, int32_t pairing,
                                     const eigen_dense_settings* settings, const uint8_t* d_mask, double* h_fitness, double* h_stats, void* stream,
                                     const eigen_dense_solve* solve)
{
    return eigen_eval_population_dense_members(e, g, structure, bg, gradient, pairing, settings, d_mask, h_fitness, h_stats, stream, solve, nullptr);
}

int eigen_eval_population_dense(eigen_engine* e, const eigen_genome_batch* g, int32_t structure, int32_t bg, int32_t gradient, int32_t pairing,
                                const eigen_dense_settings* settings, const uint8_t* d_mask, double* h_fitness, double* h_stats, void* stream)
{
    return eigen_eval_population_dense_iter(e, g, structure, bg, gradient, pairing, settings, d_mask, h_fitness, h_stats, stream, nullptr);
}

int eigen_eval_images_dense_members(eigen_engine* e, const uint8_t* d_images, int32_t batch, int32_t structure, int32_t pairing,
                                    const eigen_dense_settings* settings, const uint8_t* d_mask, double* h_fitness, double* h_stats, void* stream,
                                    const eigen_dense_solve* solve, const eigen_flow_members* members)
{
    if (!e || !d_images || !h_fitness || !settings) return fail(EIGEN_ERR_INVALID, "null argument");
    int rc = dense_call_check(e, structure, pairing, settings);
    if (rc) return rc;
    DenseCall c;
    rc = dense_prepare(e, c, settings, solve, d_mask, batch, members, 1);
    if (rc) return rc;
    return eval_images_impl(e, d_images, batch, structure, pairing, h_fitness, nullptr, nullptr, (hipStream_t)stream, false, &c, h_stats);
}

int eigen_eval_images_dense_iter(eigen_engine* e, const uint8_t* d_images, int32_t batch, int32_t structure, int32_t pairing,
                                 const eigen_dense_settings* settings, const uint8_t* d_mask, double* h_fitness, double* h_stats, void* stream,
                                 const eigen_dense_solve* solve)
{
    return eigen_eval_images_dense_members(e, d_images, batch, structure, pairing, settings, d_mask, h_fitness, h_stats, stream, solve, nullptr);
}

int eigen_eval_images_dense(eigen_engine* e, const uint8_t* d_images, int32_t batch, int32_t structure, int32_t pairing,
                            const eigen_dense_settings* settings, const uint8_t* d_mask, double* h_fitness, double* h_stats, void* stream)
{
    return eigen_eval_images_dense_iter(e, d_images, batch, structure, pairing, settings, d_mask, h_fitness, h_stats, stream, nullptr);
}

// Test hook of the iterated solve: force >= 0 sets whether one level with one iteration goes through the iteration kernel too;
// pyramid_bytes (may be null): the bytes of the pyramid the handle holds, 0 before the first iterated call
int eigen_debug_dense_solve(eigen_engine* e, int32_t force, int64_t* pyramid_bytes)
{
    if (!e) return fail(EIGEN_ERR_INVALID, "null argument");
    if (force >= 0) e->dense_force_iter = force != 0;
    if (pyramid_bytes) *pyramid_bytes = e->dense.pyr ? (int64_t)eigd::pyr_doubles(e->B, e->H, e->W) * 8 : 0;
    return EIGEN_OK;
}

int eigen_get_timings(eigen_engine* e, double* h_ms6)
{
    if (!e || !h_ms6) return fail(EIGEN_ERR_INVALID, "null argument");
    double conv = 0; int launches = 0;
    for (int l = 0; l < e->L; ++l) {
        conv += e->layer[l].convA.ms + e->layer[l].lstm.ms + e->layer[l].convP.ms + e->layer[l].convA_t0.ms + e->layer[l].lstm_t0.ms + e->layer[l].up4.ms;
        launches += e->layer[l].convA.launches + e->layer[l].lstm.launches + e->layer[l].convP.launches + e->layer[l].convA_t0.launches + e->layer[l].lstm_t0.launches + e->layer[l].up4.launches;
    }
    for (int i = 0; i < 4; ++i) h_ms6[i] = e->ms[i];
    h_ms6[4] = conv; h_ms6[5] = launches;
    return EIGEN_OK;
}

// Per-op profile of the roll-out convolutions.  enable=1 brackets every conv launch with HIP events on its stream
// (serialising the stream per launch); rows of h_out (8 doubles each, up to max_ops):
// [layer, epi (+16 for the step-0 operators), NI, TW, launches, total_ms, FLOPs per launch per image (2*MACs of the terms executed), n_nblk]
int eigen_conv_profile(eigen_engine* e, int32_t enable, int32_t reset, double* h_out, int32_t max_ops, int32_t* n_ops)
{
    if (!e) return fail(EIGEN_ERR_INVALID, "null argument");
    e->profile_convs = enable != 0;
    int n = 0;
    for (int l = 0; l < e->L; ++l) {
        ConvOp* ops[6] = {l > 0 ? &e->layer[l].convA : nullptr, &e->layer[l].lstm, &e->layer[l].convP,
                          l > 0 ? &e->layer[l].convA_t0 : nullptr, &e->layer[l].lstm_t0, l < e->L - 1 ? &e->layer[l].up4 : nullptr};
        for (ConvOp* op : ops) {
            if (!op) continue;
            if (h_out && n < max_ops) {
                double* r = h_out + (size_t)n * 8;
                r[0] = op->layer; r[1] = op->epi + ((op == &e->layer[l].convA_t0 || op == &e->layer[l].lstm_t0) ? 16 : 0) + (op->wino ? 32 : 0); r[2] = op->NI; r[3] = op->TW; r[4] = op->launches; r[5] = op->ms; r[6] = 2.0 * op->macs; r[7] = op->n_nblk;
            }
            if (reset) { op->ms = 0; op->launches = 0; }
            ++n;
        }
    }
    if (n_ops) *n_ops = n;
    return EIGEN_OK;
}

static int test_conv_impl(eigen_engine* e, int32_t n_src, const float* const* d_src, const int32_t* cin, const int32_t* up, const float* const* h_w,
                          int32_t cout, int32_t H, int32_t W, int32_t batch, float* d_out, void* stream, int iters, double* h_ms)
{
    if (!e || !d_src || !cin || !up || !h_w || !d_out) return fail(EIGEN_ERR_INVALID, "null argument");
    if (n_src < 1 || n_src > 3) return fail(EIGEN_ERR_INVALID, "n_src must be 1..3");
    HIPCHK(hipSetDevice(e->cfg.device));
    // canonical arithmetic: one chain over the full-resolution sources in list order, plus the chain of the
    // unpooled source in its 2x2 form (EPI_UP4 launch at the source resolution), one fp32 addition
    int n_up = 0, i_up = -1, n_full = 0;
    for (int s = 0; s < n_src; ++s) { if (up[s]) { ++n_up; i_up = s; } else ++n_full; }
    if (n_up > 1 || n_full < 1) return fail(EIGEN_ERR_INVALID, "at most one unpooled source and at least one full-resolution source");
    if (n_up && ((H | W) & 1)) return fail(EIGEN_ERR_INVALID, "an unpooled source needs even H and W");
    // the operator and its 2x2-form companion as the planner describes them (conv_plan.h); one weight tensor per source
    const float* sw[3][4] = {{nullptr}, {nullptr}, {nullptr}};
    int cfull[3] = {0, 0, 0};
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    for (int s = 0, k = 0; s < n_src; ++s) {
        if (up[s]) continue;
        cfull[k] = cin[s]; sw[k][0] = h_w[s]; a.src[k].ptr = d_src[s];
        ++k;
    }
    ConvOp op, u;
    op.replan(plain_conv_desc(EPI_RAW, 0, cout, H, W, n_full, cfull, 0, switches()));
    const std::vector<float> pk = pack_weights(op, sw, 0);
    if (upload(op.wpk, pk.data(), pk.size())) return fail(EIGEN_ERR_HIP, "weight upload failed");
    a.raw = d_out;
    ConvArgs ua;
    memset(&ua, 0, sizeof(ua));
    DevBuf<float> raw4;
    if (n_up) {
        u.replan(up4_desc(op, cin[i_up], H / 2, W / 2, switches()));
        const float* uw[4] = {h_w[i_up], nullptr, nullptr, nullptr};
        const std::vector<float> pku = pack_weights_up4(u, uw, 0);
        if (upload(u.wpk, pku.data(), pku.size()) || raw4.ensure((size_t)batch * u.scratch_floats)) return fail(EIGEN_ERR_HIP, "weight upload failed (unpooled source)");
        ua.src[0].ptr = d_src[i_up];
        ua.raw = raw4.p;
        a.acc_init = raw4.p;
    }
    auto launch_both = [&]() -> hipError_t {
        if (n_up) { hipError_t ru = launch_conv(e, u, ua, batch, (hipStream_t)stream); if (ru != hipSuccess) return ru; }
        return launch_conv(e, op, a, batch, (hipStream_t)stream);
    };
    const bool prof = e->profile_convs;
    e->profile_convs = false;
    hipError_t r = launch_both();  // also the warm-up of a timed run
#if EIG_TIMING
    {
        // geometry of THIS operator's launches as launch_conv chose it for the warm-up above (tile shape, half blocks, eight-wave
        // blocks): ADVICE r3 -- the round-2 formula here no longer described the round-3 launches
        const int grid_ = op.last_grid, waves_ = op.last_waves;
        unsigned long long* dbg = nullptr;
        (void)hipMalloc((void**)&dbg, (size_t)grid_ * waves_ * 8 * 8);
        (void)hipMemset(dbg, 0, (size_t)grid_ * waves_ * 8 * 8);
        a.dbg = dbg;
        (void)launch_conv(e, op, a, batch, (hipStream_t)stream);
        (void)hipStreamSynchronize((hipStream_t)stream);
        std::vector<unsigned long long> h((size_t)grid_ * waves_ * 8);
        (void)hipMemcpy(h.data(), dbg, h.size() * 8, hipMemcpyDeviceToHost);
        double s4[4] = {0, 0, 0, 0};
        for (size_t i = 0; i < h.size(); i += 8) { s4[0] += (double)h[i + 5]; s4[1] += (double)h[i + 6]; s4[2] += (double)h[i + 7]; s4[3] += (double)(h[i + 2] - h[i + 1]); }
        const double n = (double)grid_ * waves_;
        fprintf(stderr, "[EIG_TIMING] blocks=%d waves/block=%d per-wave cycles: mfma+dma-issue %.0f  vmcnt-wait %.0f  barrier %.0f  loop-total %.0f\n", grid_, waves_, s4[0] / n, s4[1] / n, s4[2] / n, s4[3] / n);
        a.dbg = nullptr;
        (void)hipFree(dbg);
    }
#endif
    if (iters > 0 && r == hipSuccess) {
        (void)hipEventRecord(e->pev0, (hipStream_t)stream);
        for (int i = 0; i < iters && r == hipSuccess; ++i) r = launch_both();
        (void)hipEventRecord(e->pev1, (hipStream_t)stream);
        (void)hipEventSynchronize(e->pev1);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e->pev0, e->pev1);
        if (h_ms) *h_ms = ms / iters;
    }
    e->profile_convs = prof;
    hipError_t r2 = hipStreamSynchronize((hipStream_t)stream);
    if (r != hipSuccess) return fail(EIGEN_ERR_HIP, "conv launch: %s", hipGetErrorString(r));
    if (r2 != hipSuccess) return fail(EIGEN_ERR_HIP, "conv sync: %s", hipGetErrorString(r2));
    return EIGEN_OK;
}

int eigen_test_conv(eigen_engine* e, int32_t n_src, const float* const* d_src, const int32_t* cin, const int32_t* up, const float* const* h_w,
                    int32_t cout, int32_t H, int32_t W, int32_t batch, float* d_out, void* stream)
{
    return test_conv_impl(e, n_src, d_src, cin, up, h_w, cout, H, W, batch, d_out, stream, 0, nullptr);
}

// Same launch repeated `iters` times between two HIP events on the launch stream: average kernel time in ms.
int eigen_time_conv(eigen_engine* e, int32_t n_src, const float* const* d_src, const int32_t* cin, const int32_t* up, const float* const* h_w,
                    int32_t cout, int32_t H, int32_t W, int32_t batch, float* d_out, int32_t iters, double* h_ms, void* stream)
{
    if (iters < 1 || !h_ms) return fail(EIGEN_ERR_INVALID, "iters >= 1 and h_ms required");
    return test_conv_impl(e, n_src, d_src, cin, up, h_w, cout, H, W, batch, d_out, stream, iters, h_ms);
}

// Host-only: the graph part of genome flattening (genome.py: _flatten_lists is the specification, statement by statement).
// Keys are mapped to dense local ids once per genome (sorted key table + binary search), after which every set / map of the
// specification is a flat array indexed by id and reused from genome to genome: ~3 us per genome instead of ~20 us with
// node-based hash containers (256 genomes: 5.3 -> 0.8 ms, scripts/host_overhead.py).
namespace {
struct FlattenScratch {
    std::vector<int> keys;                    // sorted unique keys of this genome (fallback when the key range is huge)
    std::vector<int> dmap, dstamp;            // direct table key - kmin -> id, valid where dstamp == epoch
    int epoch = 0, kmin = 0, n_ids = 0;
    bool direct = false;
    std::vector<int> leaf, is_out, required, seen, node_at, state, index, has_c32;
    std::vector<float> c32;
    std::vector<int> ci, co;                  // connection ends as ids
    std::vector<int> in_off, in_src;          // incoming (ALL connections), CSR by out id
    std::vector<int> ex_off, ex_src, ex_fill; // expressed connections, CSR by out id, genome.connections order kept
    std::vector<double> ex_w;
    std::vector<int> last, next, order;
    std::vector<std::pair<int, int>> stack;
    int id_of(int key)
    {
        if (!direct) return (int)(std::lower_bound(keys.begin(), keys.end(), key) - keys.begin());
        const int at = key - kmin;
        if (dstamp[at] != epoch) { dstamp[at] = epoch; dmap[at] = n_ids++; }
        return dmap[at];
    }
    // ids for one genome's keys: NEAT keys are small integers (inputs -1..-n, nodes 0..), so a direct table serves; a
    // sorted table + binary search is the fallback for pathological ranges
    int begin(const int32_t* in_keys, int n_in, const int32_t* out_keys, int n_out, const int32_t* nk, int n_nodes,
              const int32_t* ci_, const int32_t* co_, int nc)
    {
        int lo = 0, hi = 0;
        bool first = true;
        auto span = [&](const int32_t* p, int n) { for (int i = 0; i < n; ++i) { if (first) { lo = hi = p[i]; first = false; } lo = std::min(lo, (int)p[i]); hi = std::max(hi, (int)p[i]); } };
        span(in_keys, n_in); span(out_keys, n_out); span(nk, n_nodes); span(ci_, nc); span(co_, nc);
        const long range = (long)hi - lo + 1;
        direct = range <= (1L << 18);  // 2 MB of tables at most; NEAT keys grow by one per added node
        if (direct) {
            kmin = lo; n_ids = 0;
            if ((long)dstamp.size() < range) { dstamp.assign(range, 0); dmap.resize(range); epoch = 0; }
            if (++epoch == 0x7fffffff) { std::fill(dstamp.begin(), dstamp.end(), 0); epoch = 1; }
            auto reg = [&](const int32_t* p, int n) { for (int i = 0; i < n; ++i) id_of(p[i]); };
            reg(in_keys, n_in); reg(out_keys, n_out); reg(nk, n_nodes); reg(ci_, nc); reg(co_, nc);
            return n_ids;
        }
        keys.clear();
        keys.insert(keys.end(), in_keys, in_keys + n_in); keys.insert(keys.end(), out_keys, out_keys + n_out);
        keys.insert(keys.end(), nk, nk + n_nodes); keys.insert(keys.end(), ci_, ci_ + nc); keys.insert(keys.end(), co_, co_ + nc);
        std::sort(keys.begin(), keys.end());
        keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
        return (int)keys.size();
    }
};
}  // namespace

int eigen_flatten_genomes(int32_t G, int32_t n_in, const int32_t* in_keys, int32_t n_out, const int32_t* out_keys, const int32_t* conn_off,
                          const int32_t* conn_in, const int32_t* conn_out, const double* conn_w, const uint8_t* conn_en, const int32_t* node_off,
                          const int32_t* node_key, const uint8_t* node_act, const uint8_t* node_agg_sum, const double* node_bias,
                          const double* node_resp, int32_t cap_nodes, int32_t cap_edges, int32_t* o_node_off, int32_t* o_edge_off, uint8_t* o_act,
                          double* o_bias, double* o_resp, int32_t* o_edge_src, double* o_edge_w, int32_t* o_out_node, uint8_t* o_status)
{
    if (G < 0 || !in_keys || !out_keys || !conn_off || !node_off || !o_node_off || !o_edge_off || !o_status) return fail(EIGEN_ERR_INVALID, "null argument");
    static thread_local FlattenScratch S;
    const int ONE = -(n_in + 1);
    int nn = 0, ne = 0;  // nodes / edges emitted so far
    o_node_off[0] = 0;
    o_edge_off[0] = 0;
    for (int g = 0; g < G; ++g) {
        const int c0 = conn_off[g], c1 = conn_off[g + 1], m0 = node_off[g], m1 = node_off[g + 1];
        const int nc = c1 - c0;
        const int nn0 = nn, ne0 = ne;
        uint8_t status = 0;
        // dense ids
        const int N = S.begin(in_keys, n_in, out_keys, n_out, node_key + m0, m1 - m0, conn_in + c0, conn_out + c0, nc);
        S.leaf.assign(N, -1); S.is_out.assign(N, 0); S.required.assign(N, 0); S.seen.assign(N, 0); S.node_at.assign(N, -1);
        S.state.assign(N, 0); S.index.assign(N, -1); S.has_c32.assign(N, 0); S.c32.assign(N, 0.0f);
        for (int i = 0; i < n_in; ++i) S.leaf[S.id_of(in_keys[i])] = i;
        for (int m = m0; m < m1; ++m) S.node_at[S.id_of(node_key[m])] = m;   // a later duplicate key wins, as in a dict
        S.ci.resize(nc); S.co.resize(nc);
        for (int c = 0; c < nc; ++c) { S.ci[c] = S.id_of(conn_in[c0 + c]); S.co[c] = S.id_of(conn_out[c0 + c]); }
        // incoming lists over ALL connection keys
        S.in_off.assign(N + 1, 0);
        for (int c = 0; c < nc; ++c) ++S.in_off[S.co[c] + 1];
        for (int i = 0; i < N; ++i) S.in_off[i + 1] += S.in_off[i];
        S.in_src.resize(nc);
        S.ex_fill.assign(S.in_off.begin(), S.in_off.end() - 1);
        for (int c = 0; c < nc; ++c) S.in_src[S.ex_fill[S.co[c]]++] = S.ci[c];
        // required_for_output, layer by layer
        S.last.clear();
        for (int k = 0; k < n_out; ++k) {
            const int o = S.id_of(out_keys[k]);
            S.is_out[o] = 1;
            if (!S.seen[o]) { S.seen[o] = 1; S.required[o] = 1; S.last.push_back(o); }
        }
        for (;;) {
            S.next.clear();   // t: sources of connections into the layer added last that were not seen before
            for (int b : S.last)
                for (int j = S.in_off[b]; j < S.in_off[b + 1]; ++j) {
                    const int a = S.in_src[j];
                    if (!S.seen[a] && S.state[a] == 0) { S.state[a] = 1; S.next.push_back(a); }   // state doubles as "in t" here
                }
            if (S.next.empty()) break;
            bool any_layer = false;
            for (int x : S.next) if (S.leaf[x] < 0) any_layer = true;
            for (int x : S.next) S.state[x] = 0;
            if (!any_layer) break;
            for (int x : S.next) { if (S.leaf[x] < 0) S.required[x] = 1; S.seen[x] = 1; }
            S.last.swap(S.next);
        }
        // expressed connections, per destination, in genome.connections order
        S.ex_off.assign(N + 1, 0);
        for (int c = 0; c < nc; ++c) {
            if (!conn_en[c0 + c]) continue;
            const int i = S.ci[c], o = S.co[c];
            if ((!S.required[o] && !S.required[i]) || S.is_out[i]) continue;
            ++S.ex_off[o + 1];
        }
        for (int i = 0; i < N; ++i) S.ex_off[i + 1] += S.ex_off[i];
        const int nex = S.ex_off[N];
        S.ex_src.resize(nex); S.ex_w.resize(nex);
        S.ex_fill.assign(S.ex_off.begin(), S.ex_off.end() - 1);
        for (int c = 0; c < nc; ++c) {
            if (!conn_en[c0 + c]) continue;
            const int i = S.ci[c], o = S.co[c];
            if ((!S.required[o] && !S.required[i]) || S.is_out[i]) continue;
            const int at = S.ex_fill[o]++;
            S.ex_src[at] = i; S.ex_w[at] = conn_w[c0 + c];
        }
        // depth-first post-order from the outputs
        S.order.clear();
        for (int k = 0; k < n_out && !status; ++k) {
            S.stack.clear();
            S.stack.emplace_back(S.id_of(out_keys[k]), 0);
            while (!S.stack.empty() && !status) {
                const int n = S.stack.back().first, ci = S.stack.back().second;
                S.stack.pop_back();
                if (S.leaf[n] >= 0 || S.state[n] == 2) continue;
                const int cn = S.ex_off[n + 1] - S.ex_off[n];
                if (ci == 0) {
                    if (S.state[n] == 1) { status = 2; break; }  // cycle
                    S.state[n] = 1;
                }
                if (ci < cn) {
                    S.stack.emplace_back(n, ci + 1);
                    const int child = S.ex_src[S.ex_off[n] + ci];
                    if (S.leaf[child] < 0 && S.state[child] != 2) {
                        if (S.state[child] == 1) { status = 2; break; }  // cycle
                        S.stack.emplace_back(child, 0);
                    }
                } else {
                    S.state[n] = 2;
                    S.order.push_back(n);
                }
            }
        }
        auto emit_node = [&](uint8_t act, double bias, double resp) -> bool {
            if (nn >= cap_nodes) return false;
            o_act[nn] = act; o_bias[nn] = bias; o_resp[nn] = resp;
            return true;
        };
        auto emit_edge = [&](int src, double w) -> bool {
            if (ne >= cap_edges) return false;
            o_edge_src[ne] = src; o_edge_w[ne] = w; ++ne;
            return true;
        };
        bool full = false, any_c32 = false;
        for (size_t oi = 0; oi < S.order.size() && !status && !full; ++oi) {
            const int n = S.order[oi];
            const int m = S.node_at[n];
            if (m < 0) { status = 2; break; }
            const int e0 = S.ex_off[n], e1 = S.ex_off[n + 1];
            if ((!node_agg_sum[m] && e1 > e0) || node_act[m] == 255) { status = 2; break; }
            if (e1 == e0) { S.has_c32[n] = 1; S.c32[n] = (float)node_bias[m]; any_c32 = true; continue; }
            bool all_const = any_c32;
            if (all_const) for (int j = e0; j < e1; ++j) if (!S.has_c32[S.ex_src[j]]) { all_const = false; break; }
            if (all_const) { status = 1; break; }  // numpy float32 activation of a constant sub-graph: the caller's job
            S.index[n] = nn - nn0;
            if (!emit_node(node_act[m], node_bias[m], node_resp[m])) { full = true; break; }
            int lead = e0;
            if (any_c32) while (lead < e1 && S.has_c32[S.ex_src[lead]]) ++lead;
            if (lead > e0) {  // Python's sum(): the leading run of float32 constants accumulates in float32
                float pre = 0.0f;
                for (int j = e0; j < lead; ++j) {
                    const float t = (float)S.ex_w[j] * S.c32[S.ex_src[j]];
                    pre = j == e0 ? t : (float)(pre + t);
                }
                if (!emit_edge(ONE, (double)pre)) { full = true; break; }
            }
            for (int j = lead; j < e1 && !full; ++j) {
                const int i = S.ex_src[j];
                if (S.leaf[i] >= 0) full = !emit_edge(-(S.leaf[i] + 1), S.ex_w[j]);
                else if (S.has_c32[i]) full = !emit_edge(ONE, (double)((float)S.ex_w[j] * S.c32[i]));
                else full = !emit_edge(S.index[i], S.ex_w[j]);
            }
            if (full) break;
            ++nn;
            o_edge_off[nn] = ne;
        }
        for (int k = 0; k < n_out && !status && !full; ++k) {
            const int o = S.id_of(out_keys[k]);
            if (S.has_c32[o]) {  // constant output plane: identity(1 * (k * 1.0) + 0) == k
                S.index[o] = nn - nn0;
                if (!emit_node(EIGEN_ACT_IDENTITY, 0.0, 1.0) || !emit_edge(ONE, (double)S.c32[o])) { full = true; break; }
                ++nn;
                o_edge_off[nn] = ne;
            }
            if (S.index[o] < 0) { status = 2; break; }
            o_out_node[(size_t)g * n_out + k] = S.index[o];
        }
        if (full) return fail(EIGEN_ERR_CAPACITY, "eigen_flatten_genomes: output capacity (%d nodes, %d edges) exceeded at genome %d", cap_nodes, cap_edges, g);
        if (status) { nn = nn0; ne = ne0; }  // empty segment: the caller handles this genome
        o_status[g] = status;
        o_node_off[g + 1] = nn;
    }
    return EIGEN_OK;
}

// Host-only: the launches of one PredNet step as prednet_run issues them, planned by the same two functions (conv_plan.h) under the switches `sw` and the mask `mask`.
static int plan_text(int32_t n_layers, const int32_t* channels, int32_t width, int32_t height, int32_t batch, int32_t n_cu, int mask, int32_t step0, const Switches& sw,
                     char* out, int32_t cap)
{
    const int L = n_layers;
    if (!channels || !out || cap < 1) return fail(EIGEN_ERR_INVALID, "null argument");
    if (L < 1 || L > EIGEN_MAX_LAYERS) return fail(EIGEN_ERR_INVALID, "n_layers %d out of range", L);
    if (width <= 0 || height <= 0 || (width % (1 << (L - 1))) || (height % (1 << (L - 1)))) return fail(EIGEN_ERR_INVALID, "image %dx%d must be divisible by 2^(layers-1)", width, height);
    if (batch < 1 || n_cu < 1) return fail(EIGEN_ERR_INVALID, "batch and n_cu must be >= 1");
    int C[EIGEN_MAX_LAYERS], H[EIGEN_MAX_LAYERS], W[EIGEN_MAX_LAYERS];
    for (int l = 0; l < L; ++l) { C[l] = channels[l]; H[l] = height >> l; W[l] = width >> l; if (C[l] < 1) return fail(EIGEN_ERR_INVALID, "channels[%d] < 1", l); }
    LayerPlan plan[EIGEN_MAX_LAYERS];
    plan_prednet(L, C, H, W, mask, sw, plan);
    std::string text;
    auto line = [&](const char* name, const OpDesc& op, bool up_src, bool acc_init) {
        const LaunchPlan p = plan_launch(op, batch, n_cu, up_src, acc_init, sw);
        static const char* const shapes[4] = {"wide", "tall", "half", "pack"};
        const char* kernel = p.kernel == K_WINO ? "wino" : p.kernel == K_CONVP0 ? "convp0" : p.kernel == K_LSTM0 ? "lstm0" : p.onekb ? "mfma_onekb" : p.w8 ? "mfma_w8" : "mfma";
        char buf[320];
        snprintf(buf, sizeof(buf), "%s layer=%d kernel=%s shape=%s epi=%d wino=%d fused=%d vec=%d NI=%d n_nblk=%d tilesX=%d tilesY=%d nparts=%d nwalk=%d grid=%d threads=%d\n", name, op.layer, kernel,
                 p.kernel == K_WINO ? shapes[p.shape] : p.kernel == K_MFMA ? (op.TW == 8 ? "tw8" : "tw16") : "pixel", op.epi, (int)op.wino, (int)op.fused, (int)p.vec, op.NI, op.n_nblk,
                 p.tilesX, p.tilesY, p.nparts, p.nwalk, p.grid, p.threads);
        text += buf;
    };
    for (int l = 1; l < L; ++l) line("convA", step0 ? plan[l].convA_t0 : plan[l].convA, false, false);
    for (int l = L - 1; l >= 0; --l) {
        const bool fused = l < L - 1 && plan[l].lstm.fused;
        if (l < L - 1 && !fused) line("up4", plan[l].up4, false, false);
        line("lstm", step0 ? plan[l].lstm_t0 : plan[l].lstm, fused, l < L - 1 && !fused);
        line("convP", plan[l].convP, false, false);
    }
    snprintf(out, (size_t)cap, "%s", text.c_str());
    return (int)text.size();
}

// every switch at its default: the environment is not read
int eigen_plan_text(int32_t n_layers, const int32_t* channels, int32_t width, int32_t height, int32_t batch, int32_t n_cu, int32_t wino_mask, int32_t step0,
                    char* out, int32_t cap)
{
    return plan_text(n_layers, channels, width, height, batch, n_cu, wino_mask < 0 ? EIGEN_WINO_DEFAULT : wino_mask, step0, Switches(), out, cap);
}

// w4 = {w4_tall, w4_half, w4_pack, w4_parts} over the defaults; NULL: what THIS process launches -- switches(), and wino_mask < 0 its effective mask
int eigen_plan_text_sw(int32_t n_layers, const int32_t* channels, int32_t width, int32_t height, int32_t batch, int32_t n_cu, int32_t wino_mask, int32_t step0,
                       const int32_t* w4, char* out, int32_t cap)
{
    if (!w4) return plan_text(n_layers, channels, width, height, batch, n_cu, wino_mask < 0 ? wino_mask_env() : wino_mask, step0, switches(), out, cap);
    Switches sw;
    sw.w4_tall = w4[0]; sw.w4_half = w4[1]; sw.w4_pack = w4[2]; sw.w4_parts = w4[3];
    return plan_text(n_layers, channels, width, height, batch, n_cu, wino_mask < 0 ? EIGEN_WINO_DEFAULT : wino_mask, step0, sw, out, cap);
}

int eigen_test_det_math(eigen_engine* e, const float* d_x, int32_t n, float* d_exp, float* d_sig, float* d_tanh, void* stream)
{
    if (!e || !d_x) return fail(EIGEN_ERR_INVALID, "null argument");
    HIPCHK(hipSetDevice(e->cfg.device));
    hipLaunchKernelGGL(det_math_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_x, n, d_exp, d_sig, d_tanh);
    HIPCHK(hipGetLastError());
    return EIGEN_OK;
}

// Stage-level access for the parity tests: the dense field of the last Farneback eigen_flow call, float [batch][2][H][W] (dx, dy planes).
int eigen_debug_dense_flow(eigen_engine* e, int32_t batch, float* h_flow, void* stream)
{
    if (!e || !h_flow) return fail(EIGEN_ERR_INVALID, "null argument");
    if (e->cfg.flow_method != EIGEN_FLOW_FARNEBACK || !e->fb_I) return fail(EIGEN_ERR_STATE, "no Farneback flow has been computed by this engine");
    if (batch < 1 || batch > e->B) return fail(EIGEN_ERR_CAPACITY, "batch %d exceeds max_batch %d", batch, e->B);
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    const int levels = fb_levels_used(e->H, e->W, e->cfg.fb_levels);
    // level k writes fb_flow[(levels - k) & 1]; the full-resolution field is level 0's
    HIPCHK(hipMemcpy(h_flow, e->fb_flow[levels & 1], sizeof(float) * (size_t)batch * 2 * e->H * e->W, hipMemcpyDeviceToHost));
    return EIGEN_OK;
}

// Stage-level access for the parity tests: one tensor of the layer state the last eigen_prednet_sequence call left (that call's last step runs ConvP_l for
// l > 0 too -- RollPlan::keep_state -- and forks nothing onto the side stream, so the state is complete behind the caller's stream).
// which: EIGEN_STATE_R (h[hflip]) / _C / _P, float [batch][C_l][H_l][W_l]; EIGEN_STATE_E, float [batch][2 C_l][H_l][W_l].
int eigen_debug_state(eigen_engine* e, int32_t batch, int32_t layer, int32_t which, float* h_out, void* stream)
{
    if (!e || !h_out) return fail(EIGEN_ERR_INVALID, "null argument");
    if (layer < 0 || layer >= e->L) return fail(EIGEN_ERR_INVALID, "layer %d out of range (0..%d)", layer, e->L - 1);
    if (which < EIGEN_STATE_R || which > EIGEN_STATE_E) return fail(EIGEN_ERR_INVALID, "which %d is none of EIGEN_STATE_R / _C / _P / _E", which);
    if (e->seq_batch == 0) return fail(EIGEN_ERR_STATE, "no kept state (no eigen_prednet_sequence call yet, or a roll-out / evaluation overwrote it)");
    if (e->seq_batch != batch) return fail(EIGEN_ERR_STATE, "the kept state is of a batch of %d, not %d", e->seq_batch, batch);
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    const Layer& y = e->layer[layer];
    const float* src = which == EIGEN_STATE_R ? y.h[e->hflip] : which == EIGEN_STATE_C ? y.c : which == EIGEN_STATE_P ? y.P : y.E;
    const size_t n = (size_t)batch * (which == EIGEN_STATE_E ? 2 : 1) * y.C * y.H * y.W;
    HIPCHK(hipMemcpy(h_out, src, sizeof(float) * n, hipMemcpyDeviceToHost));
    return EIGEN_OK;
}

// Stage-level access for the parity tests: corner list of the last eigen_flow call.
int eigen_debug_corners(eigen_engine* e, int32_t batch, float* h_corners, int32_t* h_ncorners, float* h_next, uint8_t* h_status, void* stream)
{
    if (!e) return fail(EIGEN_ERR_INVALID, "null argument");
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    if (h_corners) HIPCHK(hipMemcpy(h_corners, e->d_corners, sizeof(float) * batch * e->K * 2, hipMemcpyDeviceToHost));
    if (h_ncorners) HIPCHK(hipMemcpy(h_ncorners, e->d_ncorners, sizeof(int32_t) * batch, hipMemcpyDeviceToHost));
    if (h_next) HIPCHK(hipMemcpy(h_next, e->d_next, sizeof(float) * batch * e->K * 2, hipMemcpyDeviceToHost));
    if (h_status) HIPCHK(hipMemcpy(h_status, e->d_status, (size_t)batch * e->K, hipMemcpyDeviceToHost));
    return EIGEN_OK;
}

}  // extern "C"
