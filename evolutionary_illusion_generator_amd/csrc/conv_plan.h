// conv_plan.h -- host-only and pure: WHAT runs (plan_prednet: one operator descriptor per convolution of a PredNet step) and IN WHICH SHAPE (plan_launch: kernel
// family, block shape, tiles, grid, walk).  No HIP call, no getenv, no engine: everything is a function of its arguments, so a machine without a GPU can check
// it (eigen_plan_text, tests/test_launch_plan.py).  The launch shape is a property of the launch only -- no result bit depends on it -- which is why only such
// a test can see it.
#pragma once
#include <algorithm>

#include "conv_mfma.h"    // EPI_*, KC, P0_TX / L0_TX, CONV_THREADS
#include "weight_pack.h"  // pad4, PackGeom
#include "wino_geom.h"

namespace eig {

// The A/B switches (EIGEN_* environment variables), read once per process by eigen_engine.hip: switches().  The defaults here ARE the product's behaviour.
struct Switches {
    // EIGEN_TILE_MAP: 0 only for A/B measurements: tiles interleaved over the XCDs instead of a contiguous tile range per XCD
    int tile_map = 1;
    // EIGEN_W8: eight-wave instantiation of the direct ConvA (conv_mfma.h: W8): launches of at most four rounds of the device's block slots gain 4-5 % from twice as
    // many waves out of the same few blocks (profiles/r03_b_ab_w8.txt); 0 / 1 forces it off / on (A/B measurements and the parity tests), -1: by launch size
    int w8 = -1;
    // EIGEN_W4_TALL / EIGEN_W4_HALF / EIGEN_W4_PACK = 0 / 1: forbid / force the Winograd block shape (A/B, tests); -1: plan_launch's rules
    int w4_tall = -1, w4_half = -1, w4_pack = -1;
    // EIGEN_W4_PARTS = n forces min(n, n_nblk) rounded down to a divisor (n >= n_nblk: one N-block per block), for A/B measurements and the parity tests; 0: the walk rule
    int w4_parts = 0;
    // EIGEN_TW8_FACTOR: 8 x 8 tiles only where they cover the map this much better than 16 x 16 (choose_tw)
    double tw8_factor = 1.15;
    // A/B measurements only: EIGEN_CONVP0_MFMA / EIGEN_LSTM0_MFMA = 1 run the image layer's ConvP / ConvLSTM on the MFMA kernel instead of the per-pixel ones;
    // EIGEN_NO_ONEKB = 1 drops the one-K-block ConvA instantiation; EIGEN_NO_UP4C = 1 the four-classes-in-one-block 2x2-form pass; EIGEN_NO_T0 = 1 the step-0 operators
    // (the fields say what RUNS: convp0_direct = !EIGEN_CONVP0_MFMA, lstm0_direct = !EIGEN_LSTM0_MFMA, onekb = !EIGEN_NO_ONEKB, up4c = !EIGEN_NO_UP4C, skip_zero_sources = !EIGEN_NO_T0)
    bool convp0_direct = true, lstm0_direct = true, onekb = true, up4c = true, skip_zero_sources = true;
    // EIGEN_SIDE_STREAM = 0 / 1 forces ConvP_l (l > 0) off / onto the side stream (A/B, tests); -1: by launch size (prednet_run)
    int side_stream = -1;
};

// ------------------------------------------------------------------------------------------------ operator plan
enum { PACK_DIRECT = 0, PACK_UP4 = 1, PACK_UP4C = 2, PACK_WINO = 3 };   // which packer of weight_pack.h
enum { WT_CONVA = 0, WT_CONVP = 1, WT_X0 = 2, WT_X1 = 3, WT_H = 4 };    // which weight tensor(s) of the layer: ConvA, ConvP, or the four gates' W_x (on E_l), W_x (on R_{l+1}), W_h

// Everything about one operator that is geometry.  PackGeom's source list is the one the LAUNCH reads (ConvArgs::src); pk_* is the list the packer walks, which
// differs only for a Winograd ConvLSTM with its unpooled source inside the chains (E_l, R_{l+1}, h_l).
struct OpDesc : PackGeom {
    bool present = false;   // false: the layer has no such operator (ConvA_0, the 2x2-form pass of a fused or top-layer ConvLSTM)
    int epi = 0, TW = 16, layer = 0;
    int H = 0, W = 0;
    double macs = 0;        // algorithmic multiply-accumulates per image (real channels only; Winograd: executed)
    bool wino = false;      // Winograd F(4x4, 3x3) form (conv_wino4.h); epi stays the operator's epilogue
    // Winograd ConvLSTM below the top layer: its unpooled source R_{l+1} rides inside the same chains (conv_wino4.h: up_fused)
    bool fused = false;
    int up_C = 0, up_kb = 0;
    bool raw = false;       // image layer: an unpacked table for convp0_direct_kernel / lstm0_direct_kernel exists beside the packed weights
    int pack = PACK_DIRECT, lstm_mode = 0;   // lstm_mode: the packers' column rule (0 plain, 1 four 16-channel gate tiles, 2 packed gates for C <= 4)
    int npk = 0, pk_w[3] = {0, 0, 0}, pk_C[3] = {0, 0, 0}, pk_Ct[3] = {0, 0, 0};   // packer sources in order: weight tensor, channels read, channels of the tensor
    size_t scratch_floats = 0;   // 2x2-form pass: floats of partial chains per image ([4 classes][columns][H][W])
};

struct LayerPlan {
    OpDesc convA, lstm, convP;
    // Step-0 operators: after reset_state() h_l = 0 and P_l = 0, hence the second half of every E_l (relu(P - A), A >= 0)
    // is 0 as well.  Their terms fma(0, w, acc) leave the chain untouched, so the first step runs the same chains over the
    // non-zero sources only: ConvA reads the first half of E_{l-1}, the ConvLSTM the first half of E_l and R_{l+1}.
    OpDesc convA_t0, lstm_t0;
    // The unpooled source R_{l+1} of the ConvLSTM in its 2x2 form (conv_mfma.h: EPI_UP4), launched at the resolution of
    // layer l+1 ahead of the ConvLSTM launch, which adds the result to its own chain.
    OpDesc up4;
};

inline void choose_ni(int Cout, bool lstm, int* NI, int* n_nblk)
{
    if (lstm) { *NI = 4; *n_nblk = (Cout + 15) / 16; return; }
    int best = 1; double beste = -1;
    for (int ni = 1; ni <= 4; ++ni) {
        const int nb = (Cout + 16 * ni - 1) / (16 * ni);
        const double eff = (double)Cout / (nb * 16.0 * ni) + 1e-3 * ni;  // ties -> larger tile
        if (eff > beste) { beste = eff; best = ni; }
    }
    *NI = best; *n_nblk = (Cout + 16 * best - 1) / (16 * best);
}

// Tile shape of an operator: 16 x 16, or 8 x 8 where that covers the map at least 15 % better.
inline int choose_tw(int H, int W, double tw8_factor)
{
    auto util = [&](int tw) {
        const int th = (tw == 8) ? 8 : 16;
        const int ty = (H + th - 1) / th, tx = (W + tw - 1) / tw;
        return (double)H * W / ((double)ty * th * tx * tw);
    };
    // 16 x 16 tiles unless 8 x 8 tiles cover the map at least 15 % better: the 8-wide instantiations have no branch-free staging path
    // and a conflicted LDS row stride (conv_mfma.h) -- measured at 160 x 120 maps (640x480 colour, layer 2: profiles/r04_c_perop_shapes.txt):
    // 8 x 8 tiles at 100 % cover ran at 0.78 of peak, 16 x 16 tiles at 93.75 % cover at 0.86.  EIGEN_TW8_FACTOR for A/Bs.
    return (util(16) * tw8_factor + 1e-9 >= util(8)) ? 16 : 8;
}

// EIGEN_WINOGRAD: bit l = ConvLSTM_l, bit 8 + l = ConvA_l, bit 16 + l = ConvP_l may take the Winograd form (if eligible) AND bit 25 / 26 / 27 enables it for the
// ConvLSTMs / ConvAs / ConvPs as a class (rounds 4-5 had an F(2x2, 3x3) kernel behind the per-operator bits and F(4x4) behind the class bits; round 6 removed the
// F(2x2) kernel -- nothing ran it -- and an operator whose class bit is clear now runs direct).  Default: all of them -- measured faster at every shape tried,
// 256^2 / 512^2 / 640x480 / 160x120, colour and gray.  Eligibility (the same rule in oracle/eig_oracle.c: eig_wino_op) is a property
// of the operator's shape only, never of the batch: results must not depend on the device batch a genome lands in.
// Every setting of the mask is ANOTHER canonical summation order, which the oracle follows through the same variable; EIGEN_WINOGRAD=0 = the direct chains of
// rounds 1-3.  Every rank of a multi-GPU run must use the same value (eigen_winograd_mask).
//   kind 0 ConvLSTM_l, 1 ConvA_l, 2 ConvP_l; Cin = channels of the full-resolution sources (multiples of 8 each), Cout per gate;
//   H x W = the resolution the convolution runs at; odd H only for an operator of the TOP layer (nothing is pooled / unpooled from it)
#ifndef EIGEN_WINO_DEFAULT
#define EIGEN_WINO_DEFAULT 0x0FFFFFFE   // every eligible operator in Winograd form, the unpooled source inside the ConvLSTM chains (bit 24), F(4x4, 3x3) tiles (bits 25-27)
#endif
inline bool wino_op(int mask, int kind, int l, int Cin, int Cout, int H, int W, bool top)
{
    if (!((mask >> (8 * kind + l)) & 1) || !((mask >> (25 + kind)) & 1) || l < 1) return false;
    if ((Cin % 8) || (Cout % 16) || (W % 4)) return false;
    if ((H % 2) && !(top && kind != 1)) return false;
    if (kind != 0 && (Cout % 48) && (Cout % 64)) return false;  // plain convolutions: N-blocks of 48 or 64 columns without padding
    return true;
}
// The chain of the unpooled source R_{l+1}.  Direct ConvLSTM (the image layer, ineligible shapes, EIGEN_WINOGRAD=0): a pass of its own at the source resolution
// in 2x2 form (EPI_UP4 / EPI_UP4C), added to the ConvLSTM's chain with one fp32 addition.  Winograd ConvLSTM: INSIDE the same chains, between E_l and h_l
// (conv_wino4.h: up_fused; oracle/eig_oracle.c: eig_wino_lstm) -- below the top layer the Winograd form exists only that way (16-byte rows at the
// source resolution: W % 8 == 0, 8-channel K-blocks: C_{l+1} % 8 == 0, bit 24 of the mask); an operator that cannot is a direct one.
// That is bit 24 of the EIGEN_WINOGRAD mask (above).
inline bool wino_fuse(int mask, int l, int L, int W, int Cup) { return ((mask >> 24) & 1) && l < L - 1 && (W % 8) == 0 && (Cup % 8) == 0; }

inline double wino_tiles(int H, int W) { const int wt = 4; return (double)((H + wt - 1) / wt) * ((W + wt - 1) / wt); }   // F(4x4, 3x3) tiles of a map

// A plain convolution (epi: EPI_CONVA / EPI_CONVP / EPI_RAW) over the listed full-resolution sources, direct form
inline OpDesc plain_conv_desc(int epi, int layer, int Cout, int H, int W, int nsrc, const int* cin, int wtensor, const Switches& sw)
{
    OpDesc op;
    op.present = true; op.epi = epi; op.layer = layer; op.H = H; op.W = W; op.Cout = Cout; op.nsrc = nsrc;
    choose_ni(Cout, false, &op.NI, &op.n_nblk);
    op.TW = choose_tw(H, W, sw.tw8_factor);
    op.npk = nsrc;
    for (int s = 0; s < nsrc; ++s) {
        op.src_C[s] = op.pk_C[s] = op.pk_Ct[s] = cin[s]; op.pk_w[s] = wtensor;
        op.krows += pad4(cin[s]) * 9; op.macs += (double)H * W * Cout * cin[s] * 9;
    }
    return op;
}
// The step-0 twin of a one-source operator: only the first C channels of source 0 are read, whatever else it had is zero
inline OpDesc step0_desc(const OpDesc& full, int C, int gates)
{
    OpDesc t0 = full;
    t0.nsrc = t0.npk = 1;
    t0.src_C[0] = t0.pk_C[0] = C; t0.src_Ct[0] = t0.pk_Ct[0] = full.src_C[0]; t0.src_C[1] = 0;
    t0.krows = pad4(C) * 9;
    t0.macs = (double)full.H * full.W * gates * full.Cout * C * 9;
    return t0;
}
// A plain convolution's Winograd form: N-blocks of 48 or 64 columns (wino_op), 16-wide tiles; krows stays the direct form's (ConvArgs carries it)
inline void to_wino_plain(OpDesc& op)
{
    op.wino = true; op.pack = PACK_WINO; op.TW = 16;
    op.NI = (op.Cout % 64) ? 3 : 4; op.n_nblk = op.Cout / (16 * op.NI);
    op.macs = wino_tiles(op.H, op.W) * W4_NPOS * op.Cout * op.src_C[0];   // executed: tiles x positions
}
// The 2x2-form pass of the unpooled source (Cup channels at Hs x Ws) of `consumer`, whose columns it shares
inline OpDesc up4_desc(const OpDesc& consumer, int Cup, int Hs, int Ws, const Switches& sw)
{
    OpDesc u;
    u.present = true; u.epi = EPI_UP4; u.layer = consumer.layer; u.nsrc = u.npk = 1; u.src_C[0] = u.pk_C[0] = u.pk_Ct[0] = Cup; u.pk_w[0] = WT_X1;
    u.H = Hs; u.W = Ws; u.Cout = consumer.Cout;
    u.NI = consumer.NI; u.n_nblk = consumer.n_nblk; u.TW = choose_tw(Hs, Ws, sw.tw8_factor);
    u.krows = pad4(Cup) * 4;
    u.macs = (double)consumer.H * consumer.W * (consumer.lstm_mode ? 4 : 1) * consumer.Cout * Cup * 4;  // 4 taps per output pixel and channel instead of 9
    u.pack = PACK_UP4; u.lstm_mode = consumer.lstm_mode;
    u.scratch_floats = (size_t)4 * u.n_nblk * u.NI * 16 * Hs * Ws;
    // <= 16 columns (the packed image-layer ConvLSTM): all four classes in one block (EPI_UP4C) where the wide staging path exists
    if (sw.up4c && consumer.NI == 1 && consumer.lstm_mode == 2 && u.TW == 16 && (Ws % 4) == 0) { u.epi = EPI_UP4C; u.NI = 4; u.pack = PACK_UP4C; }
    return u;
}

// The operators of one PredNet step, per layer l < L: C[l] channels at H[l] x W[l].
inline void plan_prednet(int L, const int* C, const int* H, const int* W, int wino_mask, const Switches& sw, LayerPlan* out)
{
    for (int l = 0; l < L; ++l) {
        LayerPlan& y = out[l];
        y = LayerPlan();
        const int Cl = C[l];
        const bool top = l == L - 1;
        // ---- ConvA_l: E_{l-1} (2 C_{l-1} ch at the finer resolution) -> C_l, fused relu / 2x2 max-pool / error unit
        if (l > 0) {
            const int cin = 2 * C[l - 1];
            y.convA = plain_conv_desc(EPI_CONVA, l, Cl, H[l - 1], W[l - 1], 1, &cin, WT_CONVA, sw);
            y.convA_t0 = step0_desc(y.convA, C[l - 1], 1);   // step 0: first half of E_{l-1} only
            if (wino_op(wino_mask, 1, l, C[l - 1], Cl, H[l - 1], W[l - 1], false))   // (the step-0 operator reads C_{l-1} channels: multiples of 8 too)
                for (OpDesc* f : {&y.convA, &y.convA_t0}) to_wino_plain(*f);
        }
        // ---- ConvLSTM_l: 4 gates fused on N.  Chain over E_l, h_l + chain of the unpooled R_{l+1}: inside the same chains (Winograd form) or in its 2x2 form (own launch, up4)
        {
            OpDesc& op = y.lstm;
            op.present = true; op.epi = EPI_LSTM; op.layer = l; op.H = H[l]; op.W = W[l]; op.Cout = Cl;
            op.nsrc = op.npk = 2;
            op.src_C[0] = 2 * Cl; op.src_C[1] = Cl;
            choose_ni(Cl, true, &op.NI, &op.n_nblk);
            if (Cl <= 4) { op.epi = EPI_LSTM_PACKED; op.NI = 1; op.n_nblk = 1; }  // 4 gates x <=4 channels in one MFMA tile
            op.lstm_mode = (op.epi == EPI_LSTM_PACKED) ? 2 : 1;
            op.TW = choose_tw(op.H, op.W, sw.tw8_factor);
            for (int s = 0; s < 2; ++s) {
                op.pk_C[s] = op.pk_Ct[s] = op.src_C[s]; op.pk_w[s] = s ? WT_H : WT_X0;
                op.krows += pad4(op.src_C[s]) * 9; op.macs += (double)op.H * op.W * 4 * Cl * op.src_C[s] * 9;
            }
            op.raw = op.epi == EPI_LSTM_PACKED && (Cl == 1 || Cl == 3);   // image layer: lstm0_direct_kernel's table, which holds the step-0 table too
            y.lstm_t0 = step0_desc(op, Cl, 4);   // step 0: first half of E_l only; h_l = 0 is not read
            const int Cup = top ? 0 : C[l + 1];
            const bool fuse = wino_fuse(wino_mask, l, L, W[l], Cup);
            if (op.epi == EPI_LSTM && wino_op(wino_mask, 0, l, 3 * Cl, Cl, op.H, op.W, top) && (top || fuse)) {
                const int Cu = fuse ? Cup : 0;
                const double tiles = wino_tiles(op.H, op.W);
                const double pf = 36, pu = 25;   // positions of a tile: full-resolution sources, the unpooled one
                for (OpDesc* f : {&op, &y.lstm_t0}) {
                    const bool t0 = f != &op;
                    f->wino = true; f->pack = PACK_WINO; f->TW = 16;
                    // executed: 16 / 36 (unpooled source: 9 / 25) multiply-adds per channel and tile
                    f->macs = tiles * pf * 4 * Cl * ((t0 ? 1.0 : 3.0) * Cl) + tiles * pu * 4 * Cl * Cu;
                    if (fuse) {   // packer sources: E_l, R_{l+1}, h_l (the step-0 operator: E_l, R_{l+1})
                        f->fused = true; f->up_C = Cu; f->up_kb = Cu / KC;
                        f->npk = t0 ? 2 : 3;
                        f->pk_w[2] = WT_H; f->pk_C[2] = f->pk_Ct[2] = Cl;
                        f->pk_w[1] = WT_X1; f->pk_C[1] = f->pk_Ct[1] = Cu;
                    }
                }
            } else if (!top)   // R_{l+1}, at ITS resolution; columns = the ConvLSTM's
                y.up4 = up4_desc(op, Cup, H[l + 1], W[l + 1], sw);
        }
        // ---- ConvP_l
        y.convP = plain_conv_desc(EPI_CONVP, l, Cl, H[l], W[l], 1, &Cl, WT_CONVP, sw);
        y.convP.raw = l == 0 && (Cl == 1 || Cl == 3);   // image layer: convp0_direct_kernel reads the OIHW tensor itself
        if (wino_op(wino_mask, 2, l, Cl, Cl, H[l], W[l], top)) to_wino_plain(y.convP);
    }
}

// ------------------------------------------------------------------------------------------------ launch plan
enum { K_MFMA = 0, K_CONVP0 = 1, K_LSTM0 = 2, K_WINO = 3 };   // kernel family: conv3x3_mfma, the image layer's two per-pixel kernels, wino4_kernel

struct LaunchPlan {
    bool ok = true;        // false: an operator / argument pairing no kernel runs (a Winograd ConvLSTM handed a separate unpooled chain)
    int kernel = K_MFMA;
    bool vec = false, onekb = false;   // K_MFMA: 16-byte DMA staging; the one-K-block ConvA instantiation
    int w8 = 0;                        // K_MFMA: the eight-wave ConvA instantiation
    int shape = W4_WIDE;               // K_WINO: W4_WIDE / W4_TALL / W4_HALF / W4_PACK
    int tilesX = 0, tilesY = 0;        // ConvArgs::tilesX / tilesY
    int grid = 0, threads = 0;         // blocks and threads per block of the launch (K_CONVP0 / K_LSTM0: grid = gx * gy * batch)
    int gx = 0, gy = 0;
    int nparts = 0, nwalk = 0;         // K_WINO only (ConvArgs::nparts / nwalk); 0 otherwise
    unsigned mg[3] = {0, 0, 0};
    bool tile_map = true;
    int last_grid = 0, last_waves = 4; // timeline records of the launch: last_grid x last_waves (EIG_TIMING read-back)
};

// has_up_src: an unpooled source is attached (ConvArgs::up_src); has_acc_init: a separate chain of the unpooled source (ConvArgs::acc_init)
inline LaunchPlan plan_launch(const OpDesc& op, int batch, int n_cu, bool has_up_src, bool has_acc_init, const Switches& sw)
{
    LaunchPlan p;
    const int TH = (op.TW == 8) ? 8 : 16;
    const int NIMG = 256 / (TH * op.TW);
    p.tilesX = (op.W + op.TW - 1) / op.TW;
    p.tilesY = (op.H + TH - 1) / TH;
    const int ntile = ((batch + NIMG - 1) / NIMG) * p.tilesX * p.tilesY;
    const int per_tile = op.n_nblk * (op.epi == EPI_UP4 ? 4 : 1);
    p.grid = per_tile * ((ntile + 7) / 8) * 8;  // XCD-aware tile map (conv_mfma.h): tiles padded to a multiple of 8
    // 16-byte DMA staging needs chunk-aligned rows: W % 4 == 0
    p.vec = (op.W % 4) == 0;
    p.tile_map = sw.tile_map != 0;
    p.w8 = (p.vec && op.epi == EPI_CONVA && op.TW == 16 && op.NI < 4 && (sw.w8 >= 0 ? sw.w8 != 0 : p.grid <= 8 * n_cu)) ? 1 : 0;   // (Switches::w8)
    p.last_grid = p.grid;
    if (op.wino) {  // Winograd form: F(4x4, 3x3), conv_wino4.h
        p.kernel = K_WINO;
        if (op.epi == EPI_LSTM && has_acc_init) { p.ok = false; return p; }   // (plan_prednet never pairs F(4x4) with a separate unpooled chain)
        // Block shape (conv_wino4.h): 16 rows x 32 columns, or 32 x 16 ("tall") where that covers the MAP with fewer blocks -- 80 x 60: 10 instead of 12, 40 x 30: 3
        // instead of 4 (the reference's 160 x 120); a function of the operator's map size alone, and the chains do not depend on it.  EIGEN_W4_TALL = 0 / 1 forces it (A/B, tests).
        const bool tall = sw.w4_tall >= 0 ? sw.w4_tall != 0 : ((op.W + 15) / 16) * ((op.H + 31) / 32) < ((op.W + 31) / 32) * ((op.H + 15) / 16);
        p.tilesX = tall ? (op.W + 15) / 16 : (op.W + 31) / 32; p.tilesY = tall ? (op.H + 31) / 32 : (op.H + 15) / 16;
        // Half blocks (conv_wino4.h: HALF, 8 x 32 pixels, six or twelve waves) while even THEY are at most one block per CU: the launch's time is then ONE block's time, and a half
        // block has the CU's matrix pipe to itself for half the multiply-adds (c1: +15 %; with more half blocks than CUs the second round costs more than the halving gains --
        // c2's 20 x 15 top layer, 200 full blocks: -7 %).  A choice by launch size, like the walk.  EIGEN_W4_HALF = 0 / 1 forces it (A/B, tests).
        const bool half = !tall && (sw.w4_half >= 0 ? sw.w4_half != 0 : (long long)op.n_nblk * batch * p.tilesX * ((op.H + 7) / 8) <= n_cu);
        if (half) p.tilesY = (op.H + 7) / 8;
        // Packed tiles (conv_wino4.h: PACK): maps of 4 x 4 or 5 x 4 tiles -- the 20 x 15 top layer of the reference's 160 x 120 fills 62 % of a wide block -- on half blocks
        // whose sixteen MFMA rows are all real tiles: tile columns 0-3 of one image, or tile column 4 of four images (five blocks per four images).  For ConvLSTMs without
        // an unpooled source and ConvPs.  Taken when its rounds of half blocks (a half block takes about two thirds of a full one's time) cost less than the rounds of
        // full blocks: ref160's ConvLSTM_3, 600 blocks = 3 rounds -> 756 half blocks = 3 rounds of two thirds; configs[1]'s, 200 blocks -> 252 half blocks, one round each.  A choice
        // by map and launch size; the chains do not depend on it.  EIGEN_W4_PACK = 0 / 1 forbids / forces it for every operator it can run.
        const int ptx = (op.W + 3) / 4, pty = (op.H + 3) / 4;
        const bool pack_can = op.epi != EPI_CONVA && !has_up_src && (ptx == 4 || ptx == 5) && pty == 4 && sw.w4_tall < 0 && sw.w4_half < 0;
        bool pack = false;
        if (pack_can) {
            const long long nhalf = (long long)op.n_nblk * (batch + (ptx == 5 ? (batch + 3) / 4 : 0)), nfull = (long long)op.n_nblk * batch;
            pack = sw.w4_pack >= 0 ? sw.w4_pack != 0 : 2 * ((nhalf + n_cu - 1) / n_cu) < 3 * ((nfull + n_cu - 1) / n_cu);
        }
        if (pack) { p.tilesX = ptx; p.tilesY = pty; }
        const int ntile4 = pack ? batch + (ptx == 5 ? (batch + 3) / 4 : 0) : batch * p.tilesX * p.tilesY;
        // WALK (conv_wino4.h): nparts blocks per tile, each computing nwalk = n_nblk / nparts consecutive N-blocks of it: walks of three N-blocks where n_nblk allows, of
        // two otherwise (the blocks of a tile share its planes through the XCD's L2), no walk while the launch would not give every CU four blocks.  A property of the
        // launch only -- the bits do not depend on it.  EIGEN_W4_PARTS: Switches::w4_parts.
        int nparts;
        if (sw.w4_parts > 0) { nparts = std::min(sw.w4_parts, op.n_nblk); while (op.n_nblk % nparts) --nparts; }
        else {   // walks of three N-blocks where n_nblk allows (two otherwise), shorter while the launch would not give every CU four blocks
            int nwalk = (op.n_nblk % 3 == 0) ? 3 : ((op.n_nblk % 2 == 0) ? 2 : 1);
            if ((long long)(op.n_nblk / nwalk) * ntile4 < 4ll * n_cu) nwalk = 1;
            nparts = op.n_nblk / nwalk;
        }
        if (tall || half || pack) nparts = op.n_nblk;   // (tall and half blocks do not walk)
        p.nparts = nparts; p.nwalk = op.n_nblk / nparts;
        const int g4 = nparts * ((ntile4 + 7) / 8) * 8;
        {   // q = umulhi(x, ceil(2^32 / d)) = x / d for every x with x * d < 2^32 (x < number of blocks here)
            auto magic = [&](long long d) -> unsigned { return (d > 1 && (long long)g4 * 16 * d < (1ll << 32)) ? (unsigned)(((1ll << 32) + d - 1) / d) : 0u; };   // (x 16: a packed block divides its first TILE's index)
            p.mg[0] = magic(nparts); p.mg[1] = magic((long long)p.tilesX * p.tilesY); p.mg[2] = magic(p.tilesX);
        }
        const bool six = (half || pack) && !(op.NI == 4 && op.epi != EPI_CONVA);   // (64-column ConvLSTM / ConvP half blocks: twelve waves, conv_wino4.h: NSPLIT)
        p.last_grid = g4 * p.nwalk; p.last_waves = six ? W4_WAVES / 2 : W4_WAVES;   // (timeline records: one per block and N-block of its walk)
        p.shape = pack ? W4_PACK : (tall ? W4_TALL : (half ? W4_HALF : W4_WIDE));
        p.grid = g4; p.threads = 64 * p.last_waves; p.w8 = 0;
    } else if (op.epi == EPI_CONVP && op.raw && sw.convp0_direct) {  // image layer: HBM-bound, one thread per pixel (conv_mfma.h)
        p.kernel = K_CONVP0;
        p.gx = (op.W + P0_TX - 1) / P0_TX; p.gy = (op.H + P0_TY - 1) / P0_TY; p.threads = P0_TX * P0_TY;
        p.grid = p.gx * p.gy * batch;
    } else if (op.epi == EPI_LSTM_PACKED && op.raw && sw.lstm0_direct && (op.Cout == 1 || op.Cout == 3)) {
        // image layer: one thread per pixel (conv_mfma.h: lstm0_direct_kernel); the step-0 operator has one source
        p.kernel = K_LSTM0;
        p.gx = (op.W + L0_TX - 1) / L0_TX; p.gy = (op.H + L0_TY - 1) / L0_TY; p.threads = L0_TX * L0_TY;
        p.grid = p.gx * p.gy * batch;
    } else {
        // the image layer's ConvA (K = 9 x 6 channels): one K-block, its own instantiation (conv_mfma.h: ONEKB)
        p.onekb = op.epi == EPI_CONVA && sw.onekb && op.NI == 3 && op.TW == 16 && p.vec && op.nsrc == 1 && pad4(op.src_C[0]) <= KC;
        if (p.onekb) p.w8 = 0;
        p.threads = p.w8 ? 2 * CONV_THREADS : CONV_THREADS;
        p.last_waves = p.threads / 64;
    }
    return p;
}

}  // namespace eig
