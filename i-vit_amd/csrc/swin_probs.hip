// swin_probs.hip -- the softmax probabilities of the Swin window attention, written to memory: the P that window_attention_kernel
// (swin.hip) keeps in registers and multiplies with V.  An inspection path (SwinTransformer.attention_maps), not the hot path: it lives
// in a file of its own so that swin.hip and the instruction sequences of its tuned kernels are not touched by it.
// What must not drift from swin.hip, the conditions on the arguments and the choice of the softmax form (x0, ksat, mask value, tables),
// is not restated here: both files take it from win_attn_host.h.
// Reference: models/swin_quant.py WindowAttention.forward (:121-169): the tensor attn.log_int_softmax returns, divided by its scale.
#include "common.h"
#include "rowsum.h"

#if IVIT_LAB
extern int g_winattn_dry_run;       // swin.hip (ivit_debug_window_attention_dry_run)
extern int32_t g_winattn_plan[16];
#endif

namespace {

constexpr int NT = 256;
constexpr int WPB = NT / 64;
constexpr int WHD = 32;

#include "attn_parts.h"

// ------------------------------------------------------------------------------------------------
// probs[win][head][query][ldp] uint8 (scale 2^-7), queries and keys in window order.  The arithmetic per score is that of
// window_attention_kernel, statement by statement (scores on v_mfma_i32_16x16x32_i8, qact_attn1, the two-operand qact2 with the bias
// operand, shift mask, one exponent branch per SM, row sum, factor, p); what differs is where a row lives.  Modelled on
// attention_probs_kernel (attention.hip): rows live in LDS, every loop runs over the run-time token count, one body serves every
// window of 2..144 tokens.  No RQ32 form (the float64 requantisation is the exact one), no ORD switch (a Shiftmax row whose exact
// sum reaches SHIFTMAX_ORDER_SUM always takes the ordered sum).
//
// One wave per (window, head), four pairs per workgroup, as window_attention_kernel: a window's K is 1.5 .. 4.6 KB and every query
// tile reads its fragments again from L1, so no workgroup stages anything for another wave and there is no workgroup barrier behind
// the tables.  A wave per query tile would leave the fourth wave of a 49-token window (tiles of 16, 16, 16, 1 queries) one row of
// work; with a wave per pair every wave of the grid does the same work.
//
// Per query tile of 16 queries (lane = 16 g + l15: query l15, keys 16 kt + 4 g + r), the wave's LDS slice [16][kp + 4] dwords:
//   1. per key tile: score ka (int8), the shift mask, the slot's code into the slice -- SM 0: ka (+ mask_value under the mask), SM 1:
//      the float view phi[ka] / phim[ka], SM 2 / 3: ka or -50000 under the mask; the row maximum over the four lanes of a query
//   2. per key tile: the lane's own codes -> exponents (one branch per SM), written back over the codes (Shiftmax: the integer,
//      I-BERT: the float32), keys at and behind the token count 0; Shiftmax: the exact integer sum and shiftmax_factor.  I-BERT
//      rows, and Shiftmax rows whose sum reaches SHIFTMAX_ORDER_SUM, take the float32 sum in torch's order with torch_rowsum_half
//      (rowsum.h) over the row in LDS, two rows at a time, as attention_probs_kernel does
//   3. the tile's rows x dwords of four keys spread over the 64 lanes: p = top byte of trunc(fl32(e * factor)) (I-BERT: the halved
//      factor, p in [0, 128], 128 is the byte 0x80), top_bytes, one dword store where probs and ldp are multiples of four, bytes
//      otherwise and for the last keys of a row.  Bytes tokens .. ldp - 1 of a row are never written.
// ------------------------------------------------------------------------------------------------
struct WinProbsArgs {
    const int8_t* qkv;      // [3][nwin][heads][T][32]
    uint8_t* probs;         // [nwin][heads][T][ldp]
    int64_t ldp;
    const int16_t* bias;    // [heads][T][kp]
    const uint8_t* region;  // [nW][kp] or NULL
    int mask_value;
    int nwin, heads, T, nW, kp;
    double Ms, Mb;          // qact_attn1; qact2 main operand
    int x0, ksat;
    const float* phi;       // SM 1 (WinAttnArgs of swin.hip)
    const float* phim;
    const unsigned* band;   // SM 2: [256][band_w]
    int band_w;
    const unsigned* band1;  // SM 0 on the one-row table [band_w]
    const float* ib_tab;    // SM 3: [256][256], or [256][band_w]
    float ib_sat;
    int dwords;             // probs and ldp are multiples of four: packed stores
};

constexpr int WPROBS_PAD = 4;      // dwords: rows of the slice stay 16-byte aligned and rotate their banks

inline int wprobs_key_pad(int tokens) { return tokens <= 64 ? 64 : 16 * ((tokens + 15) >> 4); }      // swin_engine.key_pad
inline size_t wprobs_lds_bytes(int tokens) { return (size_t)WPB * 16 * (wprobs_key_pad(tokens) + WPROBS_PAD) * sizeof(unsigned); }

IVIT_DEV void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int SM>
__global__ __launch_bounds__(NT) void window_attention_probs_kernel(WinProbsArgs a)
{
    __shared__ unsigned lut[256];
    __shared__ float s_phi[2][256];
    __shared__ float s_fac[WPB][16];
    extern __shared__ __attribute__((aligned(16))) unsigned wprobs_rows[];      // [4 waves][16 queries][kp + WPROBS_PAD]
    constexpr bool compat = SM == 1, band = SM == 2, ibert = SM == 3;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, l15 = lane & 15;
    const int T = a.T, nkt = (T + 15) >> 4, kp = a.kp, rs = kp + WPROBS_PAD;
    if constexpr (SM == 0) lut[tid] = a.band1 ? a.band1[min(tid, a.band_w - 1)] : shiftexp_int(-tid, a.x0, 15);
    if constexpr (compat) {
        s_phi[0][tid] = a.phi[tid];
        s_phi[1][tid] = a.phim[tid];
    }
    __syncthreads();
    const int pair = blockIdx.x * WPB + wave;
    if (pair >= a.nwin * a.heads) return;      // (the only workgroup barrier is behind it)
    const int win = pair / a.heads, hh = pair - win * a.heads;
    const int64_t plane = (int64_t)a.nwin * a.heads * T * WHD;
    const int8_t* qg = a.qkv + (int64_t)pair * T * WHD;
    const int8_t* kg = qg + plane;
    const uint8_t* regrow = a.region ? a.region + (int64_t)(win % a.nW) * kp : nullptr;
    unsigned* slice = wprobs_rows + wave * 16 * rs;
    unsigned* myrow = slice + l15 * rs;
    float* fac = s_fac[wave];
    uint8_t* obase = a.probs + (int64_t)pair * T * a.ldp;
    const int nd = (T + 3) >> 2;
    const int W = a.band_w;

    for (int qt = 0; qt < nkt; ++qt) {
        const int qld = min(16 * qt + l15, T - 1);      // rows past T repeat row T - 1: computed, never stored
        const long qf = *reinterpret_cast<const long*>(qg + (int64_t)qld * WHD + 8 * g);
        const int16_t* brow = a.bias + ((int64_t)hh * T + qld) * kp + 4 * g;
        const unsigned qreg = regrow ? regrow[qld] : 0u;
        __builtin_amdgcn_wave_barrier();      // the previous tile's pass 3 has read the slice

        // ---- pass 1: scores -> codes
        int rmax = -100000;
        float xmax = -__builtin_inff();
        for (int kt = 0; kt < nkt; ++kt) {
            const long kf = *reinterpret_cast<const long*>(kg + (int64_t)min(16 * kt + l15, T - 1) * WHD + 8 * g);
            const unsigned kreg = regrow ? *reinterpret_cast<const unsigned*>(regrow + 16 * kt + 4 * g) : 0u;
            v4i acc = {0, 0, 0, 0};
            acc = __builtin_amdgcn_mfma_i32_16x16x32_i8(kf, qf, acc, 0, 0, 0);
            const int2 bw = *reinterpret_cast<const int2*>(brow + 16 * kt);
            const int bv[4] = {(int)(int16_t)bw.x, bw.x >> 16, (int)(int16_t)bw.y, bw.y >> 16};
            v4i code;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool live = 16 * kt + 4 * g + r < T;
                const int kS = clamp_i32(requant_exact(acc[r], a.Ms), -128, 127);        // qact_attn1
                int ka = clamp_i32(requant_exact(kS, a.Mb) + bv[r], -128, 127);          // qact2 (two operands)
                const bool masked = regrow && ((kreg >> (8 * r)) & 0xffu) != qreg;       // shift mask, after the clamp
                if constexpr (compat) {
                    const float xv = s_phi[masked ? 1 : 0][ka + 128];
                    xmax = live ? fmaxf(xmax, xv) : xmax;
                    code[r] = __float_as_int(xv);
                } else {
                    if (masked) ka = (band || ibert) ? -50000 : ka + a.mask_value;
                    rmax = live ? max(rmax, ka) : rmax;
                    code[r] = ka;
                }
            }
            *reinterpret_cast<v4i*>(myrow + 16 * kt + 4 * g) = code;
        }
        rmax = rows_allmax_i32(rmax);      // over the four lanes of a query
        if constexpr (compat) {
            xmax = fmaxf(xmax, __shfl_xor(xmax, 16));
            xmax = fmaxf(xmax, __shfl_xor(xmax, 32));
        }

        // ---- pass 2: the lane's own codes -> exponents, in place
        const int rm = max(rmax, -128);
        const float x0f = (float)a.x0;
        unsigned esum = 0;
        for (int kt = 0; kt < nkt; ++kt) {
            const v4i code = *reinterpret_cast<const v4i*>(myrow + 16 * kt + 4 * g);
            v4i ev;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool live = 16 * kt + 4 * g + r < T;
                const int sc = code[r];
                unsigned e;
                if constexpr (ibert) {
                    // IBERTIntSoftmax: e = table[row max][q] (float32), a masked score the saturated value
                    const float* trow = a.ib_tab + (W ? (rm + 128) * W : ((rm + 128) << 8) + 128);
                    const int sq = live ? clamp_i32(sc, -128, rm) : rm;      // (a slot without a score reads a valid entry)
                    const float ef = sc == -50000 ? a.ib_sat : (W ? trow[min(rm - sq, W - 1)] : trow[sq]);
                    e = (unsigned)__float_as_int(live ? ef : 0.0f);
                } else if constexpr (compat) {
                    e = live ? (unsigned)shiftexp_lit(__int_as_float(sc) - xmax, x0f) : 0u;      // ivit_modules.py:150-170
                } else if constexpr (band) {
                    const int idx = live ? min(rm - max(sc, -50000), W - 1) : 0;      // under the mask: the saturated last entry
                    e = a.band[(size_t)(rm + 128) * W + idx];
                    e = live ? e : 0u;
                } else {
                    // the table entry while the distance is inside it (any distance on the one-row table), beyond it the exact form
                    const int d = live ? rmax - sc : 0;
                    const bool in_table = d <= a.ksat || a.band1;
                    e = in_table ? lut[min(d, a.ksat) & 255] : shiftexp_int(-d, a.x0, 15);
                    e = live ? e : 0u;
                }
                ev[r] = (int)e;
                if constexpr (!ibert) esum += e;
            }
            *reinterpret_cast<v4i*>(myrow + 16 * kt + 4 * g) = ev;
        }
        unsigned order_rows = 0;      // Shiftmax: the rows whose exact sum reaches 2^24 (wave-uniform)
        if constexpr (!ibert) {
            const unsigned tot = rows_allsum_u32(esum);
            if (g == 0) fac[l15] = shiftmax_factor(tot);
            order_rows = (unsigned)__builtin_amdgcn_ballot_w64(tot >= SHIFTMAX_ORDER_SUM) & 0xffffu;      // bit r: query r of the tile
        }
        wave_lds_sync();
        if (ibert || order_rows != 0) {
            // I-BERT: S = e.sum() in float32 in torch's order, factor = floor(2^32 / S) (ibert_modules.py:313), halved (pass 3).
            // Shiftmax rows from 2^24 on: the reference's float32 sum is the one of torch's order (attn_parts.h SHIFTMAX_ORDER_SUM)
            for (int it = 0; it < 8; ++it) {
                if (!ibert && ((order_rows >> (2 * it)) & 3u) == 0) continue;      // uniform
                const int row = 2 * it + (lane >> 5);
                const unsigned* er = slice + row * rs;
                const float S = torch_rowsum_half([&](int i) { return ibert ? __int_as_float((int)er[i]) : (float)er[i]; }, T, lane);
                if ((lane & 31) == 0 && (ibert || ((order_rows >> row) & 1u)))
                    fac[row] = ibert ? floorf(4294967296.0f / S) * 0.5f : shiftmax_factor(S);
            }
            wave_lds_sync();
        }

        // ---- pass 3: p = floor(fl32(e * factor) / 2^24) (ivit_modules.py:175); I-BERT floor(fl32(e * factor) / 2^25) from the halved factor
        const int nrows = min(16, T - 16 * qt);
        uint8_t* otile = obase + (int64_t)16 * qt * a.ldp;
        for (int item = lane; item < nrows * nd; item += 64) {
            const int row = item / nd, d = item - row * nd;
            const v4i e4 = *reinterpret_cast<const v4i*>(slice + row * rs + 4 * d);
            const float f = fac[row];
            unsigned p[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float evf = ibert ? __int_as_float(e4[r]) : (float)(unsigned)e4[r];
                p[r] = (unsigned)(evf * f);      // float32 product, <= 2^31
            }
            const unsigned w = top_bytes(p);
            uint8_t* orow = otile + (int64_t)row * a.ldp;
            if (a.dwords && 4 * d + 3 < T) {
                *reinterpret_cast<unsigned*>(orow + 4 * d) = w;
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (4 * d + r < T) orow[4 * d + r] = (uint8_t)(w >> (8 * r));
            }
        }
    }
}

using WinProbsKernel = void (*)(WinProbsArgs);
const WinProbsKernel WPROBS_KERNELS[4] = {window_attention_probs_kernel<0>, window_attention_probs_kernel<1>,
                                          window_attention_probs_kernel<2>, window_attention_probs_kernel<3>};      // [SM]

#include "win_attn_host.h"     // WinAttnDesc, win_attn_check, win_attn_form: the conditions and the softmax form, shared with swin.hip

int window_probs_launch(WinAttnDesc d)
{
    if (const int rc = win_attn_check(d)) return rc;
    const WinSoftmaxForm f = win_attn_form(d);
    WinProbsArgs a{};
    a.qkv = d.qkv; a.probs = static_cast<uint8_t*>(d.out); a.ldp = d.ldo; a.bias = d.bias; a.region = d.region;
    a.nwin = d.windows; a.heads = d.heads; a.T = d.tokens; a.nW = d.windows_per_image; a.kp = wprobs_key_pad(d.tokens);
    a.Ms = d.Ms; a.Mb = d.Mb;
    a.x0 = f.x0; a.ksat = f.ksat; a.mask_value = f.mask_value;
    a.phi = f.phi; a.phim = f.phim;
    a.band = f.band; a.band1 = f.band1; a.band_w = f.band_w;
    a.ib_tab = f.ib_tab; a.ib_sat = f.ib_sat;
    a.dwords = ((uintptr_t)d.out % 4 == 0) && d.ldo % 4 == 0;
    const int npairs = d.windows * d.heads, grid = (npairs + WPB - 1) / WPB;
    const size_t lds_bytes = wprobs_lds_bytes(d.tokens);
#if IVIT_LAB
    if (g_winattn_dry_run) return win_plan_record(d, f, 0, 0, 0, grid, lds_bytes, a.kp, 0, 0, a.dwords);
#endif
    hipLaunchKernelGGL(WPROBS_KERNELS[f.sm], dim3(grid), dim3(NT), lds_bytes, ivit_stream(d.stream), a);
    IVIT_CHECK_LAUNCH(d.name);
}

}  // namespace

// The two entries (contracts: include/ivit_hip.h).  Descriptor order as in swin.hip; no output requantisation (m_o = 0 passes the
// check's bound), no geometry, window order.
IVIT_EXPORT int ivit_window_attention_probs_u8(const int8_t* qkv, uint8_t* probs, int64_t ldp, const int16_t* bias, const uint8_t* region,
                                               int mask_value, int nwin, int windows_per_image, int heads, int tokens, int head_dim,
                                               uint32_t m_s, int32_t e_s, uint32_t m_b, int32_t e_b, float s_attn, const float* phi,
                                               const float* phim, const uint32_t* band, int band_w, int band_rows, ivit_stream_t stream)
{
    return window_probs_launch({"ivit_window_attention_probs_u8", WIN_SHIFTMAX_PROBS, qkv, probs, ldp, bias, region, mask_value, nwin,
                                windows_per_image, heads, tokens, head_dim, m_s, e_s, m_b, e_b, s_attn, 0, 0, phi, phim, band, band_w,
                                band_rows, nullptr, 0.0f, 0, 0, 0, 0, 0, stream, 0});
}

IVIT_EXPORT int ivit_window_attention_probs_u8_ibert(const int8_t* qkv, uint8_t* probs, int64_t ldp, const int16_t* bias,
                                                     const uint8_t* region, float masked_exp, int nwin, int windows_per_image, int heads,
                                                     int tokens, int head_dim, uint32_t m_s, int32_t e_s, uint32_t m_b, int32_t e_b,
                                                     const float* table, int band_w, ivit_stream_t stream)
{
    return window_probs_launch({"ivit_window_attention_probs_u8_ibert", WIN_IBERT_PROBS, qkv, probs, ldp, bias, region, 0, nwin,
                                windows_per_image, heads, tokens, head_dim, m_s, e_s, m_b, e_b, 1.0f, 0, 0, nullptr, nullptr, nullptr,
                                band_w, 256, table, masked_exp, 0, 0, 0, 0, 0, stream, 0});
}
