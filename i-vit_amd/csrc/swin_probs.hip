// swin_probs.hip -- the softmax probabilities of the Swin window attention, written to memory: the P that window_attention_kernel
// (swin.hip) keeps in registers and multiplies with V.  An inspection path (SwinTransformer.attention_maps), not the hot path: it lives
// in a file of its own so that swin.hip and the instruction sequences of its tuned kernels are not touched by it.
// Reference: models/swin_quant.py WindowAttention.forward (:121-169): the tensor attn.log_int_softmax returns, divided by its scale.
#include "common.h"
#include "rowsum.h"

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

// the checks the two entries share, in the style of attention_check (attention.hip); fills what both forms use
int window_probs_check(const char* who, WinProbsArgs& a, const int8_t* qkv, uint8_t* probs, int64_t ldp, const int16_t* bias,
                       const uint8_t* region, int nwin, int windows_per_image, int heads, int tokens, int head_dim, uint32_t m_s,
                       int32_t e_s, uint32_t m_b, int32_t e_b)
{
    IVIT_REQUIRE(qkv && probs && bias, "%s: NULL operand", who);
    if (head_dim != WHD || tokens < 2 || tokens > 144) {
        ivit_set_error("%s: unsupported geometry head_dim=%d tokens=%d (need 32, 2..144)", who, head_dim, tokens);
        return IVIT_ERR_UNSUPPORTED;
    }
    IVIT_REQUIRE(nwin > 0 && heads > 0 && (int64_t)nwin * heads <= 0x7fffffff / 4 && windows_per_image >= 1,
                 "%s: bad window counts", who);
    IVIT_REQUIRE(!region || nwin % windows_per_image == 0, "%s: %d windows are no whole number of images of %d", who, nwin,
                 windows_per_image);
    IVIT_REQUIRE(ldp >= tokens, "%s: ldp=%lld below tokens=%d", who, (long long)ldp, tokens);
    IVIT_REQUIRE(((uintptr_t)qkv % 16 == 0) && ((uintptr_t)bias % 16 == 0) && ((uintptr_t)region % 4 == 0),
                 "%s: misaligned operand (qkv, bias: 16 bytes; region: 4)", who);
    a.qkv = qkv; a.probs = probs; a.ldp = ldp; a.bias = bias; a.region = region;
    a.nwin = nwin; a.heads = heads; a.T = tokens; a.nW = windows_per_image; a.kp = wprobs_key_pad(tokens);
    a.Ms = ivit_dyadic_to_double(m_s, e_s);
    a.Mb = ivit_dyadic_to_double(m_b, e_b);
    IVIT_REQUIRE(a.Ms < 2048.0 && a.Mb < 1048576.0, "%s: requant multiplier too large", who);
    a.dwords = ((uintptr_t)probs % 4 == 0) && ldp % 4 == 0;
    a.mask_value = 0; a.x0 = -1; a.ksat = 255;
    a.phi = a.phim = nullptr; a.band = a.band1 = nullptr; a.band_w = 0; a.ib_tab = nullptr; a.ib_sat = 0.0f;
    return IVIT_OK;
}

int window_probs_launch(const char* who, int sm, const WinProbsArgs& a, ivit_stream_t stream)
{
    const int npairs = a.nwin * a.heads;
    hipLaunchKernelGGL(WPROBS_KERNELS[sm], dim3((npairs + WPB - 1) / WPB), dim3(NT), wprobs_lds_bytes(a.T), ivit_stream(stream), a);
    IVIT_CHECK_LAUNCH(who);
}

}  // namespace

IVIT_EXPORT int ivit_window_attention_probs_u8(const int8_t* qkv, uint8_t* probs, int64_t ldp, const int16_t* bias, const uint8_t* region,
                                               int mask_value, int nwin, int windows_per_image, int heads, int tokens, int head_dim,
                                               uint32_t m_s, int32_t e_s, uint32_t m_b, int32_t e_b, float s_attn, const float* phi,
                                               const float* phim, const uint32_t* band, int band_w, int band_rows, ivit_stream_t stream)
{
    const char* who = "ivit_window_attention_probs_u8";
    WinProbsArgs a;
    if (const int rc = window_probs_check(who, a, qkv, probs, ldp, bias, region, nwin, windows_per_image, heads, tokens, head_dim, m_s,
                                          e_s, m_b, e_b))
        return rc;
    IVIT_REQUIRE(band ? (band_w >= 16 && band_w <= 192 && band_w % 16 == 0 && (uintptr_t)band % 16 == 0 && (band_rows == 256 || band_rows == 1))
                      : band_w == 0,
                 "%s: the band table must be 16-byte aligned, its width a multiple of 16 in [16, 192], band_rows 256 or 1", who);
    IVIT_REQUIRE((phi == nullptr) == (phim == nullptr), "%s: phi and phim go together", who);
    IVIT_REQUIRE(((uintptr_t)phi % 4 == 0) && ((uintptr_t)phim % 4 == 0), "%s: misaligned table", who);
    IVIT_REQUIRE(mask_value <= 0 && mask_value >= -32768, "%s: mask_value=%d outside [-32768, 0]", who, mask_value);
    IVIT_REQUIRE(s_attn > 0.0f, "%s: scale must be positive", who);
    const float x0f = __builtin_floorf((1.0f / s_attn) * -1.0f);
    IVIT_REQUIRE(x0f <= -1.0f && x0f >= -4096.0f, "%s: x0=%g outside [-4096,-1]", who, (double)x0f);
    a.x0 = (int)x0f;
    // exact u32 row sum: tokens * |x0| * 2^15 must stay below 2^32
    IVIT_REQUIRE((double)tokens * (double)(-a.x0) * 32768.0 < 4294967296.0, "%s: Shiftmax row sum could overflow 32 bits (x0=%d)", who, a.x0);
    a.mask_value = mask_value;
    for (int i = 0; i < 256; ++i) {      // the first distance at which the table of distances has saturated (255: it has not)
        const int d = -i;
        if (d + (d >> 1) - (d >> 4) <= 15 * a.x0) { a.ksat = i; break; }
    }
    int sm = 0;
    if (band && band_rows == 256) {
        a.band = band; a.band_w = band_w;
        sm = 2;
    } else if (band) {      // one row for every maximum: the table of distances with the host's values
        a.band1 = band; a.band_w = band_w;
        a.ksat = band_w - 1;
        a.mask_value = -1024;      // a masked score lands beyond the last (saturated) entry whatever the maximum
    } else if (phi) {
        a.phi = phi; a.phim = phim;
        sm = 1;
    }
    return window_probs_launch(who, sm, a, stream);
}

IVIT_EXPORT int ivit_window_attention_probs_u8_ibert(const int8_t* qkv, uint8_t* probs, int64_t ldp, const int16_t* bias,
                                                     const uint8_t* region, float masked_exp, int nwin, int windows_per_image, int heads,
                                                     int tokens, int head_dim, uint32_t m_s, int32_t e_s, uint32_t m_b, int32_t e_b,
                                                     const float* table, int band_w, ivit_stream_t stream)
{
    const char* who = "ivit_window_attention_probs_u8_ibert";
    WinProbsArgs a;
    IVIT_REQUIRE(table, "%s: NULL operand", who);
    if (const int rc = window_probs_check(who, a, qkv, probs, ldp, bias, region, nwin, windows_per_image, heads, tokens, head_dim, m_s,
                                          e_s, m_b, e_b))
        return rc;
    IVIT_REQUIRE((uintptr_t)table % 4 == 0, "%s: misaligned table", who);
    IVIT_REQUIRE(band_w == 0 || (band_w >= 16 && band_w <= 256 && band_w % 16 == 0),
                 "%s: bad band width %d (a multiple of 16 in [16, 256], or 0 for the full table)", who, band_w);
    IVIT_REQUIRE(!region || (masked_exp >= 0.0f && masked_exp <= 32768.0f), "%s: masked_exp=%g outside [0, 32768]", who, (double)masked_exp);
    a.ib_tab = table; a.ib_sat = masked_exp; a.band_w = band_w;
    return window_probs_launch(who, 3, a, stream);
}
