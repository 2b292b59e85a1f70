// weight_pack.h -- host-only: OIHW weight tensors -> the layouts the kernels stream (conv_mfma.h, conv_wino4.h).  Plain geometry in, std::vector<float> out;
// no HIP header, no engine.  The arithmetic here (presum_up_weight, wino4_w1d) is canonical: the oracle states the same operations in
// the same order, and this code is compiled with -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

#include "wino_geom.h"

namespace eig {

inline int pad4(int c) { return (c + 3) & ~3; }

// What a direct-form packer needs to know of an operator (conv_plan.h: OpDesc extends it)
struct PackGeom {
    int NI = 4, n_nblk = 0, krows = 0, Cout = 0;
    int nsrc = 0;
    int src_C[3] = {0, 0, 0};
    int src_Ct[3] = {0, 0, 0};  // channels of the source TENSOR when only its first src_C channels are read (0: = src_C)
};

// Pack OIHW weights of one fused conv into [n_nblk][krows][NB]; row = (source, channel (padded to 4), tap).
// srcw[s][g] points at [Cout][Cin_s][3][3]; g = 0 for plain convs, 0..3 (i,f,c,o) for the LSTM.
// lstm: 0 plain conv, 1 gates as four 16-channel tiles (column = gate*16 + channel), 2 packed for C <= 4
// (ONE 16-column tile, column = gate*4 + channel).
inline std::vector<float> pack_weights(const PackGeom& op, const float* const srcw[3][4], int lstm)
{
    const int NB = op.NI * 16;
    std::vector<float> out((size_t)op.n_nblk * op.krows * NB, 0.0f);
    for (int nb = 0; nb < op.n_nblk; ++nb) {
        size_t row = 0;
        for (int s = 0; s < op.nsrc; ++s) {
            const int Cin = op.src_C[s], Cp = pad4(Cin);
            const int Cw = op.src_Ct[s] ? op.src_Ct[s] : Cin;  // input channels of the weight tensor
            for (int c = 0; c < Cp; ++c)
                for (int tap = 0; tap < 9; ++tap, ++row) {
                    if (c >= Cin) continue;
                    float* dst = &out[((size_t)nb * op.krows + row) * NB];
                    for (int n = 0; n < NB; ++n) {
                        int g = 0, o;
                        if (lstm == 1) { g = n / 16; o = nb * 16 + (n % 16); }
                        else if (lstm == 2) { g = n / 4; o = n % 4; }
                        else o = nb * NB + n;
                        if (o >= op.Cout) continue;
                        // LDS/slab column order: [16 lanes (n % 16)][NI tiles (n / 16)] so that a lane reads its NI values
                        // of a row with one ds_read_b128 (conv_mfma.h: boff)
                        dst[(n % 16) * op.NI + (n / 16)] = srcw[s][g][((size_t)o * Cw + c) * 9 + tap];
                    }
                }
        }
    }
    return out;
}

// Weights of the 2x2 form of `unpool x2 -> conv3x3` for parity class (py, px) of the output pixel (oracle/eig_oracle.c:
// presum_up_weights states the same rule).  Output row 2Y+py reads source rows Y-1, Y, Y (py = 0) or Y, Y, Y+1 (py = 1): tap a
// stands for source row Y+a-1+py and collects ky in {0} / {1,2} (py = 0) or {0,1} / {2} (py = 1); columns likewise.  The
// collected weights are added in fp32 in (ky, kx) row-major order starting from the first one.
inline float presum_up_weight(const float* w9, int py, int px, int a, int b)
{
    const int ky0 = py ? (a ? 2 : 0) : (a ? 1 : 0), ky1 = py ? (a ? 2 : 1) : (a ? 2 : 0);
    const int kx0 = px ? (b ? 2 : 0) : (b ? 1 : 0), kx1 = px ? (b ? 2 : 1) : (b ? 2 : 0);
    volatile float s = 0.0f;  // volatile: one fp32 rounding per addition whatever the host compiler's flags
    bool first = true;
    for (int ky = ky0; ky <= ky1; ++ky)
        for (int kx = kx0; kx <= kx1; ++kx) {
            if (first) { s = w9[ky * 3 + kx]; first = false; }
            else s = s + w9[ky * 3 + kx];
        }
    return s;
}

// Pack the 2x2-form weights of ONE unpooled source into [4 classes][n_nblk][krows = Cpad*4][NB]; row = (channel, a, b);
// column order as pack_weights (lstm: 0 plain, 1 four 16-channel gate tiles, 2 packed gates for C <= 4).
inline std::vector<float> pack_weights_up4(const PackGeom& op, const float* const srcw[4], int lstm)
{
    const int NB = op.NI * 16;
    const int Cin = op.src_C[0];
    std::vector<float> out((size_t)4 * op.n_nblk * op.krows * NB, 0.0f);
    for (int cls = 0; cls < 4; ++cls)
        for (int nb = 0; nb < op.n_nblk; ++nb)
            for (int c = 0; c < Cin; ++c)
                for (int tap = 0; tap < 4; ++tap) {
                    float* dst = &out[(((size_t)cls * op.n_nblk + nb) * op.krows + (size_t)c * 4 + tap) * NB];
                    for (int n = 0; n < NB; ++n) {
                        int g = 0, o;
                        if (lstm == 1) { g = n / 16; o = nb * 16 + (n % 16); }
                        else if (lstm == 2) { g = n / 4; o = n % 4; }
                        else o = nb * NB + n;
                        if (o >= op.Cout) continue;
                        dst[(n % 16) * op.NI + (n / 16)] = presum_up_weight(srcw[g] + ((size_t)o * Cin + c) * 9, cls >> 1, cls & 1, tap >> 1, tap & 1);
                    }
                }
    return out;
}

// EPI_UP4C (conv_mfma.h): the four classes are the four N-tiles of ONE block: [n_nblk][krows][16 columns][4 classes]
inline std::vector<float> pack_weights_up4c(const PackGeom& op, const float* const srcw[4], int lstm)
{
    const int Cin = op.src_C[0];
    std::vector<float> out((size_t)op.n_nblk * op.krows * 64, 0.0f);
    for (int nb = 0; nb < op.n_nblk; ++nb)
        for (int c = 0; c < Cin; ++c)
            for (int tap = 0; tap < 4; ++tap)
                for (int n = 0; n < 16; ++n) {
                    int g = 0, o;
                    if (lstm == 2) { g = n / 4; o = n % 4; }
                    else o = nb * 16 + n;
                    if (o >= op.Cout) continue;
                    for (int cls = 0; cls < 4; ++cls)
                        out[(((size_t)nb * op.krows + (size_t)c * 4 + tap) * 16 + n) * 4 + cls] =
                            presum_up_weight(srcw[g] + ((size_t)o * Cin + c) * 9, cls >> 1, cls & 1, tap >> 1, tap & 1);
                }
    return out;
}

// ---- Winograd F(4x4, 3x3) form of the 3x3 convolutions of layers >= 1 (conv_wino4.h; oracle/eig_oracle.c: wino4_* state the same rule)
// F(4x4, 3x3): U = G g G^T, 6 x 6 (oracle/eig_oracle.c: wino4_w1d / wino4_weights state the same operations in the same order; fmaf = one rounding, this file
// is compiled with -ffp-contract=off)
inline void wino4_w1d(float g0, float g1, float g2, float* W)
{
    const float c6 = -1.0f / 6.0f, c24 = 1.0f / 24.0f;
    W[0] = 0.25f * g0;
    const float a = g0 + g2;
    W[1] = (a + g1) * c6; W[2] = (a - g1) * c6;
    const float b = fmaf(4.0f, g2, g0);
    W[3] = fmaf(2.0f, g1, b) * c24; W[4] = fmaf(-2.0f, g1, b) * c24;
    W[5] = g2;
}
inline void wino4_weight(const float* g, float* U)
{
    float s[6][3], W[6];
    for (int j = 0; j < 3; ++j) { wino4_w1d(g[j], g[3 + j], g[6 + j], W); for (int i = 0; i < 6; ++i) s[i][j] = W[i]; }
    for (int i = 0; i < 6; ++i) wino4_w1d(s[i][0], s[i][1], s[i][2], U + i * 6);
}
// [n_nblk][K-blocks: 4 channels of one source, sources in order][36 positions][4 channels][16 columns][NI N-tiles]
// lstm: N-tile = gate, output channel = 16 nb + column (srcw[s][gate]); plain convolution: output channel = 16 (NI nb + N-tile) + column (srcw[s][0])
inline std::vector<float> pack_weights_wino(int C, int NI, int n_nblk, bool lstm, int nsrc, const int* src_C, const int* src_Cw, const float* const srcw[3][4])
{
    const int kc = W4_KC;   // channels of a packed K-block (conv_wino4.h streams them with a running offset, and one K-block past the end: padding)
    int nkb = 0;
    for (int s = 0; s < nsrc; ++s) nkb += src_C[s] / kc;
    const int npos = W4_NPOS;
    const int uf = wino4_u_floats(NI);
    std::vector<float> out((size_t)n_nblk * nkb * uf + uf, 0.0f);
    float U[36];
    for (int nb = 0; nb < n_nblk; ++nb) {
        int kb0 = 0;
        for (int s = 0; s < nsrc; ++s) {
            for (int c = 0; c < src_C[s]; ++c)
                for (int ni = 0; ni < NI; ++ni)
                    for (int n = 0; n < 16; ++n) {
                        const int o = lstm ? nb * 16 + n : (nb * NI + ni) * 16 + n;
                        if (o >= C) continue;
                        wino4_weight(srcw[s][lstm ? ni : 0] + ((size_t)o * src_Cw[s] + c) * 9, U);
                        float* dst = &out[((size_t)nb * nkb + kb0 + c / kc) * uf];
                        for (int pos = 0; pos < npos; ++pos) dst[((pos * kc + (c % kc)) * 16 + n) * NI + ni] = U[pos];
                    }
            kb0 += src_C[s] / kc;
        }
    }
    return out;
}

// Image layer, lstm0_direct_kernel (conv_mfma.h): [C outputs][K taps = (channel, ky, kx) over E_0 then h_0][4 gates], then the step-0 table (first half of E_0 only)
inline std::vector<float> lstm0_raw_table(int C, const float* const wx0[4], const float* const wh[4])
{
    const int K = 3 * C * 9, K0 = C * 9;
    std::vector<float> raw((size_t)C * K * 4 + (size_t)C * K0 * 4);
    for (int o = 0; o < C; ++o)
        for (int g = 0; g < 4; ++g) {
            for (int c = 0; c < 2 * C; ++c)
                for (int t9 = 0; t9 < 9; ++t9) {
                    const float wv = wx0[g][((size_t)o * 2 * C + c) * 9 + t9];
                    raw[((size_t)o * K + c * 9 + t9) * 4 + g] = wv;
                    if (c < C) raw[(size_t)C * K * 4 + ((size_t)o * K0 + c * 9 + t9) * 4 + g] = wv;
                }
            for (int c = 0; c < C; ++c)
                for (int t9 = 0; t9 < 9; ++t9) raw[((size_t)o * K + (2 * C + c) * 9 + t9) * 4 + g] = wh[g][((size_t)o * C + c) * 9 + t9];
        }
    return raw;
}

}  // namespace eig
