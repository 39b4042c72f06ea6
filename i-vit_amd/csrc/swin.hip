// swin.hip -- the additional integer kernels of the Swin path (config 5): 16-bit residual stream, windowed
// attention with relative-position bias and shift mask, patch merging, token average pooling.
// Reference: /root/reference/models/swin_quant.py (WindowAttention :121-169, SwinTransformerBlock :251-301,
// PatchMerging :328-349, SwinTransformer.forward_features :539-558); operators as in rowops.hip / attention.hip.
// The fork's swin_quant.py does not run as shipped (SURVEY.md finding 6); semantics are SURVEY Appendix A.8, pinned by
// tests/golden/swin_tiny.npz (generated from the reference with harness-side shims).
#include <type_traits>

#include "common.h"
#include "rowsum.h"

#if IVIT_LAB
extern int g_ln_ablate;     // rowops.hip; bits 16-19: workgroup cap of the tiled 16-bit LayerNorm in units of 256 (0 = default);
                            // bit 20: natural-scale 16-bit LayerNorm sums its rows through LDS (the round-3 form);
                            // bit 23: window attention requantises its scores in float64 also where float32 is exact
int g_winattn_dry_run = 0;  // ivit_debug_window_attention_dry_run: the eight window-attention entries (here and in swin_probs.hip) stop
int32_t g_winattn_plan[16]; // in front of their launch and leave its plan here (ivit_debug_window_attention_last_plan)
#else
constexpr int g_ln_ablate = 0;
#endif

namespace {

constexpr int NT = 256;
constexpr int WPB = NT / 64;

static inline int ew_grid(int64_t n)
{
    int64_t b = (n + NT - 1) / NT;
    return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

static inline int grid_for_rows(int64_t rows, int rpw = 1)
{
    int64_t blocks = (rows + WPB * rpw - 1) / (WPB * rpw);
    return (int)(blocks < 4096 ? blocks : 4096);
}

IVIT_DEV int pack4(int a, int b, int c, int d)
{
    return (a & 0xff) | ((b & 0xff) << 8) | ((c & 0xff) << 16) | ((d & 0xff) << 24);
}

#include "ln_chain.h"
#include "attn_parts.h"

#include "win_map.h"     // WinMap, win_row, win_row_inv: the window partition / cyclic shift as row maps

// ------------------------------------------------------------------------------------------------
// 8 -> 16 bit QuantAct (SwinTransformer.qact1, swin_quant.py:546; also used as an exact int8 -> int16 widening)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void requant_i8_i16_kernel(const int8_t* x, double Mq, int16_t* out, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT)
        out[i] = (int16_t)clamp_i32(requant_exact((int)x[i], Mq), -32768, 32767);
}

// ------------------------------------------------------------------------------------------------
// Two-operand 16-bit QuantAct of the residual connections (swin_quant.py:293, 299; quant_utils.py:232-245):
//   out[r] = clamp16(RNE(a[map(r)] * Ma) + RNE(res[r] * Mr));  a is int16 (attn.qact4) or int8 (mlp.qact2)
// ------------------------------------------------------------------------------------------------
template <typename TA>
__global__ __launch_bounds__(NT) void residual_i16_kernel(const TA* a, const uint32_t* m_pre, const int32_t* e_pre, double Ma,
                                                          const int16_t* res, double Mr, int16_t* out, int64_t rows, int C,
                                                          WinMap map)
{
    const int c4 = C >> 2;
    const int64_t total = rows * c4;
    for (int64_t q = (int64_t)blockIdx.x * NT + threadIdx.x; q < total; q += (int64_t)gridDim.x * NT) {
        const int64_t r = q / c4;
        const int c = (int)(q - r * c4) * 4;
        const int64_t ra = win_row(map, r);
        int av[4];
        if (sizeof(TA) == 1) {
            const int w = *reinterpret_cast<const int*>(reinterpret_cast<const int8_t*>(a) + ra * C + c);
#pragma unroll
            for (int i = 0; i < 4; ++i) av[i] = (int)(int8_t)(w >> (8 * i));
        } else if (sizeof(TA) == 2) {
            const int2 w = *reinterpret_cast<const int2*>(reinterpret_cast<const int16_t*>(a) + ra * C + c);
            av[0] = (int)(int16_t)w.x; av[1] = w.x >> 16; av[2] = (int)(int16_t)w.y; av[3] = w.y >> 16;
        } else {  // raw GEMM accumulators: the 16-bit QuantAct behind the projection first (attn.qact4, swin_quant.py:166)
            const v4i w = *reinterpret_cast<const v4i*>(reinterpret_cast<const int32_t*>(a) + ra * C + c);
            const v4i mm = *reinterpret_cast<const v4i*>(m_pre + c);
            const v4i ee = *reinterpret_cast<const v4i*>(e_pre + c);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                av[i] = clamp_i32(requant_exact(w[i], dyadic_mult((uint32_t)mm[i], ee[i])), -32768, 32767);
        }
        const int2 rw = *reinterpret_cast<const int2*>(res + r * C + c);
        const int rv[4] = {(int)(int16_t)rw.x, rw.x >> 16, (int)(int16_t)rw.y, rw.y >> 16};
        int o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = clamp_i32(requant_exact(av[i], Ma) + requant_exact(rv[i], Mr), -32768, 32767);
        int2 ow;
        ow.x = (o[0] & 0xffff) | (o[1] << 16);
        ow.y = (o[2] & 0xffff) | (o[3] << 16);
        *reinterpret_cast<int2*>(out + r * C + c) = ow;
    }
}

// ------------------------------------------------------------------------------------------------
// I-LayerNorm on the 16-bit stream + QuantAct(8) (+ optional row map on the OUTPUT: window partition)
// ivit_modules.py:30-65 with 16-bit inputs: var up to ~3.5e10 -> the Newton iteration runs on RN24(var) in float32
// with correctly rounded divisions, exactly as the reference does.
// ------------------------------------------------------------------------------------------------
struct Ln16Args {
    const int16_t* x;
    int rows, C;
    const float* bias_int;
    const float* s_ln;
    const uint32_t* m;
    const int32_t* e;
    int8_t* out;
    int64_t ldo;
    WinMap map;
    int outer;     // compat kernels, > 0: the reference takes the mean over a transposed view of contiguous extent `outer` (the first
                   // LayerNorm behind the Swin patch embedding, whose layout travels through the elementwise QuantActs): torch's
                   // outer-reduction order (rowsum.h torch_outer_rowsum), row = image * outer + column
    int lab_lds_sum;   // lab A/B: the row sums through LDS (the round-3 form) where the register form applies
};

// :41  y_int ** 2 on an int32 tensor keeps the low 32 bits of the product: from |d| = 46 341 on the square wraps (a 16-bit row with
// |mean| >= 13 573 and an element at the opposite rail); :42 sums the wrapped values in int64.
constexpr unsigned LN16_WRAP_FROM = 46341u;
IVIT_DEV long long ln16_square(int d) { return (long long)(int)((unsigned)d * (unsigned)d); }

// One 16-bit row literally, a wave per row, from the integers to y = floor((x - mean) * factor / 2) + bias_int (:36-61); every
// element goes to tail(c, y): the QuantAct of the int8-emitting kernels below, the float product of the token-feature kernel
// (ln_tokens.h).  phi: nullptr_t for integers (a power-of-two scale), else phi(c) = fl(fl(q * s) / s), the float the reference's
// operator sees at a natural scale -- its mean is the float32 sum over the phi values in torch's CPU reduction order (rowsum.h;
// outer > 0: the outer-reduction order for the row `row`), its integers are `.to(int32)` truncations.
template <class PHI, class TAIL>
IVIT_DEV void ln16_row(const int16_t* xr, int C, PHI phi, int outer, int row, const float* bias_int, int lane, TAIL tail)
{
    constexpr bool INTEGERS = std::is_same<PHI, decltype(nullptr)>::value;
    auto seen = [&](int c) -> int {
        if constexpr (INTEGERS) return xr[c];
        else return (int)truncf(phi(c));                                                   // :38
    };
    int mean_int;
    if constexpr (INTEGERS) {
        int sum = 0;  // |sum| < 2^31 for C <= 4096
        for (int c = lane; c < C; c += 64) sum += xr[c];
        sum = wave_reduce_sum_i32(sum);
        float fsum = (float)sum;                                      // :37 exact in any order below 2^24 ...
        if (__builtin_amdgcn_readfirstlane(abs(sum) >= (1 << 24)))    // ... from there on torch's order of additions (rowsum.h)
            fsum = torch_rowsum([&](int c) { return (float)xr[c]; }, C, lane);
        mean_int = (int)rintf(fsum / (float)C);
    } else {
        const float S = outer ? torch_outer_rowsum(phi, C, row % outer >= (outer & ~31)) : torch_rowsum(phi, C, lane);
        mean_int = (int)rintf(S / (float)C);                         // :37
    }
    long long var = 0;
    for (int c = lane; c < C; c += 64) var += ln16_square(seen(c) - mean_int);            // :38-42
    const float t = ln_newton10_literal((float)(long long)lanes_allsum_u64<64>(var));       // :45-49
    const float factor = floorf((1.0f / t) * 2147483648.0f);         // :51
    for (int c = lane; c < C; c += 64) {
        float dl = (float)(seen(c) - mean_int);
        float v = floorf((dl * factor) * 0.5f);                       // :52
        tail(c, v + bias_int[c]);                                     // :61
    }
}

// the QuantAct behind the LayerNorm for one element, literally
IVIT_DEV int8_t ln16_quantact(const Ln16Args& a, int c, float y)
{
    float s = a.s_ln[c];
    float x = y * s;                                          // :63
    float z = rintf(x / s);                                   // quant_utils.py:220 (correctly rounded quotient)
    double p = (double)z * dyadic_mult(a.m[c], a.e[c]);       // :229
    double tt = p + IVIT_MAGIC;                               // :230
    return (int8_t)clamp_i32((int)(unsigned)__double_as_longlong(tt), -128, 127);
}

__global__ __launch_bounds__(NT) void layernorm_i16_i8_kernel(Ln16Args a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int C = a.C;
    for (int row = blockIdx.x * WPB + wave; row < a.rows; row += gridDim.x * WPB) {
        int8_t* orow = a.out + win_row(a.map, row) * a.ldo;
        ln16_row(a.x + (int64_t)row * C, C, nullptr, 0, row, a.bias_int, lane, [&](int c, float y) { orow[c] = ln16_quantact(a, c, y); });
    }
}

// Natural (non power-of-two) scale of the 16-bit input: IVITIntLayerNorm sees phi(q) = fl(fl(q*s)/s) (QuantAct hands on q*s,
// quant_modules.py:387; ivit_modules.py:36 divides by s again).  Literal: the float32 mean over the phi values in torch's
// CPU reduction order (rowsum.h), `.to(int32)` truncation, then the usual chain.  One wave per row.
struct Ln16LitArgs {
    Ln16Args b;
    float s_in;
};

__global__ __launch_bounds__(NT) void layernorm_i16_i8_literal_kernel(Ln16LitArgs al)
{
    const Ln16Args& a = al.b;
    const float s_in = al.s_in;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int C = a.C;
    for (int row = blockIdx.x * WPB + wave; row < a.rows; row += gridDim.x * WPB) {
        const int16_t* xr = a.x + (int64_t)row * C;
        auto xint = [&](int c) { return ((float)xr[c] * s_in) / s_in; };       // :36 on the float view q * s
        int8_t* orow = a.out + win_row(a.map, row) * a.ldo;
        ln16_row(xr, C, xint, a.outer, row, a.bias_int, lane, [&](int c, float y) { orow[c] = ln16_quantact(a, c, y); });
    }
}

#include "ln_tokens.h"

// one int16 row of the token-feature kernel: ln16_row with the float product as its tail.  s_in == 0: the integers themselves.
template <bool COMPAT, bool FASTDIV>
struct LnTokRowI16 {
    static constexpr int TAB = 0;
    const int16_t* x;
    int C;
    float s_in, r_in;
    const float* bias_int;
    const float* s_ln;

    IVIT_DEV void setup(int, unsigned char*, float*) {}

    template <class EMIT>
    IVIT_DEV void row(int64_t xoff, int lane, EMIT emit) const
    {
        const int16_t* xr = x + xoff;
        auto tail = [&](int c, float y) { emit(c, ln_f32(y, s_ln[c])); };
        if constexpr (COMPAT) ln16_row(xr, C, [&](int c) { return ln_tok_phi16<FASTDIV>(xr[c], s_in, r_in); }, 0, 0, bias_int, lane, tail);
        else ln16_row(xr, C, nullptr, 0, 0, bias_int, lane, tail);
    }
};

// Round 4: the per-channel constants (bias, float32 bracket (lo, hi) of the QuantAct multiplier: the certificate of
// ln_chain.h) of the tiled 16-bit kernels are derived ONCE PER WORKGROUP into LDS -- one or two channels per
// thread -- and read per chunk of 8 channels where the element chain needs them.  Rounds 1-3 kept them in 72 registers per lane
// (NJ = 3), derived by every lane for its 24 channels in float64: 195-244 VGPRs = two waves per SIMD, where this VALU-bound chain
// issues its half-rate instructions at 4.4 cycles instead of 3.2, and a prologue that a launch of few rows
// (Swin stages 2-3: 14-29 MB) spent most of its time in.
// The ten float32 Newton steps of ivit_modules.py:45-49 on varf = RN24(var) WITHOUT iterating, where that is provably the same
// (round 4; scripts/probes/ln16_newton_exhaustive.py walks every float32 value in [2^24, 2^42), ln_newton_exhaustive.py every
// integer below 2^24; a sum of C <= 1536 int32 squares stays below 1536 * 2^31 < 2^42): t10 == floor(sqrt(varf)) unless varf lies
// within 2^(ex - 22) below the next square (then t10 is that or one more).  Those rows (sqrt(varf) * 2^-23 of all values: <= 3 % below
// 2^36, a quarter at 2^42), and rows below 2^24 that rowops.hip's rule sends there, run the literal loop -- wave-uniformly.  A wrapped
// sum that is zero or negative (outside the reference's own domain: its Newton steps divide by zero) takes the literal loop too.
// 40 % of the instructions of a C = 384 / 768 row group were this loop (ten IEEE divisions per group of 4 / 2 rows).
IVIT_DEV float ln16_std10(float varf)
{
    const double v = (double)varf;                          // an integer below 2^42, exact
    double s = __builtin_floor(__builtin_sqrt(v));
    s = (s * s > v) ? s - 1.0 : s;                          // (exact products: s < 2^21)
    s = ((s + 1.0) * (s + 1.0) <= v) ? s + 1.0 : s;
    const double gap = (s + 1.0) * (s + 1.0) - v;
    const bool slow = varf < 16777216.0f ? (varf < 142883.0f || gap == 1.0)      // rowops.hip LN_NEWTON_CONVERGED, ln_std10
                                          : gap <= (double)(varf * 2.384185791015625e-07f);   // 2^-22
    if (__builtin_amdgcn_ballot_w64(slow) != 0) return ln_newton10_literal(varf);
    return (float)s;
}

IVIT_DEV void ln16_build_table(const Ln16Args& a, float* t_bias, float* t_lo, float* t_hi)
{
    ln_build_table<NT>(a.m, a.e, a.s_ln, a.bias_int, a.C, t_bias, t_lo, t_hi);      // common.h: every load before the first use
}

// channel c (0-7) of a chunk of eight int16 held as four packed pairs
IVIT_DEV int ln16_channel(const v4i& w, int c) { return (c & 1) ? (w[c >> 1] >> 16) : (int)(int16_t)w[c >> 1]; }

// The tiled kernels from (w, mean_int) to the stores: w[j] = chunk sub + LPR * j of the lane's row (the integers the reference's
// LayerNorm sees: q, or k' = trunc(phi(q)) at a natural scale), LPR lanes per row.  Variance (:40-42) -> ten Newton steps and the
// factor (:45-52) -> the chain of ln_chain.h per channel: certificate, a wave with any uncertified element is redone literally.
// `row` is clamped to the matrix, `live` says whether it exists.
template <int LPR, int NJ>
IVIT_DEV void ln16_tail(const Ln16Args& a, const v4i (&w)[NJ], int mean_int, int sub, bool live, int row, const float* t_bias,
                        const float* t_lo, const float* t_hi)
{
    const int nd = a.C >> 3;
    unsigned long long var = 0;
    unsigned dmax = 0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (sub + LPR * j < nd) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const unsigned d0 = (unsigned)abs((int)(int16_t)w[j][q] - mean_int);
                const unsigned d1 = (unsigned)abs((w[j][q] >> 16) - mean_int);
                var += (unsigned long long)d0 * d0;
                var += (unsigned long long)d1 * d1;
                dmax = max(dmax, max(d0, d1));
            }
        }
    }
    // :41 the reference's squares are int32: where an element of the wave's rows reaches 46 341 the sum is taken again over the wrapped
    // values (wave-uniform, unlikely); below, the 64-bit products above are the same numbers.  (Measured alternatives, 6272 x 768: the
    // test on |mean_int| >= 46 341 - 32 768 with the two loops as if / else cost 0.06 us more per launch than this maximum; a second
    // instantiation of this function for such waves spilled to scratch.)
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(dmax >= LN16_WRAP_FROM) != 0, 0)) {
        long long wv = 0;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (sub + LPR * j < nd) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    wv += ln16_square((int)(int16_t)w[j][q] - mean_int) + ln16_square((w[j][q] >> 16) - mean_int);
            }
        }
        var = (unsigned long long)wv;
    }
    var = lanes_allsum_u64<LPR>(var);                                       // (two's complement: a wrapped sum may be negative)
    const float t = ln16_std10((float)(long long)var);                      // :45-49
    const float hfactor = floorf((1.0f / t) * 2147483648.0f) * 0.5f;        // :51; the /2 of :52 commutes (exact scaling)
    int8_t* orow = a.out + win_row(a.map, row) * a.ldo;
    int2 res[NJ];
    unsigned unc = 0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        int o[8];
        const int dt = min(sub + LPR * j, nd - 1);      // this chunk's constants: 6 x 16 bytes from the workgroup's table
        float bias8[8], lo8[8], hi8[8];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float4 b4 = *reinterpret_cast<const float4*>(t_bias + 8 * dt + 4 * h);
            const float4 l4 = *reinterpret_cast<const float4*>(t_lo + 8 * dt + 4 * h);
            const float4 h4 = *reinterpret_cast<const float4*>(t_hi + 8 * dt + 4 * h);
            bias8[4 * h] = b4.x; bias8[4 * h + 1] = b4.y; bias8[4 * h + 2] = b4.z; bias8[4 * h + 3] = b4.w;
            lo8[4 * h] = l4.x; lo8[4 * h + 1] = l4.y; lo8[4 * h + 2] = l4.z; lo8[4 * h + 3] = l4.w;
            hi8[4 * h] = h4.x; hi8[4 * h + 1] = h4.y; hi8[4 * h + 2] = h4.z; hi8[4 * h + 3] = h4.w;
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float dl = (float)(ln16_channel(w[j], c) - mean_int);
            const float v = floorf(dl * hfactor);                           // :52
            o[c] = ln_cert(v + bias8[c], lo8[c], hi8[c], unc);              // :61
        }
        res[j].x = pack4(o[0], o[1], o[2], o[3]);
        res[j].y = pack4(o[4], o[5], o[6], o[7]);
        __builtin_amdgcn_sched_barrier(0);      // one chunk's constants live at a time
    }
    if (__builtin_amdgcn_ballot_w64(unc != 0) != 0) {      // wave-uniform
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int d = min(sub + LPR * j, nd - 1);
            int o[8];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float4 s4 = *reinterpret_cast<const float4*>(a.s_ln + 8 * d + 4 * h);
                const uint4 m4 = *reinterpret_cast<const uint4*>(a.m + 8 * d + 4 * h);
                const int4 e4 = *reinterpret_cast<const int4*>(a.e + 8 * d + 4 * h);
                const float ss[4] = {s4.x, s4.y, s4.z, s4.w};
                const double MM[4] = {dyadic_mult(m4.x, e4.x), dyadic_mult(m4.y, e4.y), dyadic_mult(m4.z, e4.z),
                                      dyadic_mult(m4.w, e4.w)};
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) {
                    const int c = 4 * h + cc;
                    const float dl = (float)(ln16_channel(w[j], c) - mean_int);
                    const float v = floorf(dl * hfactor);
                    o[c] = ln_literal(v + t_bias[8 * d + c], ss[cc], MM[cc]);
                }
            }
            res[j].x = pack4(o[0], o[1], o[2], o[3]);
            res[j].y = pack4(o[4], o[5], o[6], o[7]);
        }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int d = sub + LPR * j;
        if (live && d < nd) *reinterpret_cast<int2*>(orow + 8 * d) = res[j];
    }
}

// :37 for the rows of a wave whose integer sum reaches 2^24 in magnitude: x_int.mean() is a float32 sum, and from there on its value is
// the one torch's CPU kernel reaches in its order of additions (rowsum.h; tests/golden/ln16_bigrows_kat.npz holds rows on which the
// exact sum rounded once gives another mean_int).  The whole wave sums one such row at a time from memory (the row was just loaded:
// L1 / L2); rows below 2^24 keep (float)sum, which every order gives.  Called by all lanes under a wave-uniform condition.
template <int LPR>
IVIT_DEV float ln16_ordered_sum(const int16_t* x, int C, int row0, int rows, int grp, int lane, int sum)
{
    float S = (float)sum;
#pragma unroll 1
    for (int g = 0; g < 64 / LPR; ++g) {
        const int sg = __builtin_amdgcn_readlane(sum, g * LPR);                 // the sum of row row0 + g: uniform
        if (abs(sg) < (1 << 24)) continue;
        const int16_t* xr = x + (int64_t)min(row0 + g, rows - 1) * C;
        const float Sg = torch_rowsum([&](int c) { return (float)xr[c]; }, C, lane);
        S = (grp == g) ? Sg : S;
    }
    return S;
}

// Sub-wave tiling of the same computation for C % 8 == 0, C <= 1536: LPR lanes share a row (64 / LPR rows per wave and
// iteration), each lane owns NJ chunks of 8 channels (one 16-byte load each) and keeps their per-channel constants in
// registers for the whole kernel.  The per-row scalar work (mean division, Newton steps) is evaluated once per
// wave-iteration for all rows of the wave in parallel; with LPR = C / 24 every lane is busy (C = 96 * 2^k: NJ = 3).
template <int LPR, int NJ>
__global__ __launch_bounds__(NT, 4) void layernorm_i16_i8_tiled_kernel(Ln16Args a)
{
    extern __shared__ __attribute__((aligned(16))) float ln16_tab[];      // [C] bias | [C] lo | [C] hi
    constexpr int RPW = 64 / LPR;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & (LPR - 1), grp = lane / LPR;
    const int C = a.C, nd = C >> 3;
    float* t_bias = ln16_tab;
    float* t_lo = ln16_tab + C;
    float* t_hi = ln16_tab + 2 * C;
    ln16_build_table(a, t_bias, t_lo, t_hi);
    __syncthreads();
    const float fC = (float)C;
    for (int row0 = (blockIdx.x * WPB + wave) * RPW; row0 < a.rows; row0 += gridDim.x * WPB * RPW) {
        const int row = row0 + grp;
        const bool live = row < a.rows;
        const int16_t* xr = a.x + (int64_t)min(row, a.rows - 1) * C;
        v4i w[NJ];
        int sum = 0;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int d = sub + LPR * j;
            w[j] = (d < nd) ? *reinterpret_cast<const v4i*>(xr + 8 * d) : v4i{0, 0, 0, 0};
#pragma unroll
            for (int q = 0; q < 4; ++q) sum += (int)(int16_t)w[j][q] + (w[j][q] >> 16);
        }
        sum = lanes_allsum_i32<LPR>(sum);      // common.h: DPP / permlane swaps instead of ds_bpermute butterflies
        float fsum = (float)sum;                                                // :37 exact in any order below 2^24
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(abs(sum) >= (1 << 24)) != 0, 0))
            fsum = ln16_ordered_sum<LPR>(a.x, C, row0, a.rows, grp, lane, sum);
        const int mean_int = (int)rintf(fsum / fC);
        ln16_tail<LPR, NJ>(a, w, mean_int, sub, live, min(row, a.rows - 1), t_bias, t_lo, t_hi);
    }
}

// The tiled kernel for a 16-bit input carried at a NATURAL scale s_in (ivit_layernorm_i16_i8_compat): per element
//   phi = fl(fl(q * s_in) / s_in)   -- the float the reference's LayerNorm sees (quant_modules.py:387, ivit_modules.py:36); the
//       quotient by the invariant s_in is the 3-instruction form q0 = x * r, e = fma(-s, q0, x), phi = fma(e, r, q0) with
//       r = RN(1 / s_in), correctly rounded for every 16-bit q at this s_in (checked exhaustively on the host,
//       prepare.markstein_division_ok; the literal kernel above is the fallback);
//   k' = trunc(phi) replaces q in everything downstream (ivit_modules.py:38);
//   the mean is round(fl(S / C)) with S the float32 sum of the phi values in torch's CPU reduction order: the phi values of
//   the wave's rows go through LDS once and two rows at a time are summed by the two halves of the wave (rowsum32 below).
template <int CTRL>
IVIT_DEV float dpp_f32(float x)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, true));
}

template <class F>
IVIT_DEV float rowsum32(F elem, int n, int l32, int base)
{
    // rowsum.h torch_rowsum on 32 lanes (lanes base .. base + 31 of the wave): same partial sums, same order
    const int vec_size = n >> 3, size_ilp = vec_size >> 2;
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;
    {
        int lg = 0;
        while ((1 << lg) < size_ilp) ++lg;
        const int lp = max(4, lg / 4), step = 1 << lp, mask = step - 1;
        int i = 0;
        while (i + step <= size_ilp) {
            for (int j = 0; j < step; ++j, ++i) acc0 += elem(i * 32 + l32);
            acc1 += acc0; acc0 = 0.f;
            if ((i & (mask << lp)) == 0) {
                acc2 += acc1; acc1 = 0.f;
                if ((i & (mask << (2 * lp))) == 0) { acc3 += acc2; acc2 = 0.f; }
            }
        }
        for (; i < size_ilp; ++i) acc0 += elem(i * 32 + l32);
        acc0 += acc1; acc0 += acc2; acc0 += acc3;
    }
    if (l32 < 8)
        for (int i = size_ilp * 4; i < vec_size; ++i) acc0 += elem(i * 8 + l32);
    const float p1 = __shfl(acc0, base + ((l32 + 8) & 31)), p2 = __shfl(acc0, base + ((l32 + 16) & 31)),
                p3 = __shfl(acc0, base + ((l32 + 24) & 31));
    const float v = ((acc0 + p1) + p2) + p3;    // lanes base .. base + 7: the 8 vector lanes
    float fin = 0.f;
    for (int i = vec_size * 8; i < n; ++i) fin += elem(i);
#pragma unroll
    for (int l = 0; l < 8; ++l) fin += __shfl(v, base + l);
    return fin;
}

template <int LPR, int NJ>
__global__ __launch_bounds__(NT, NJ >= 2 ? 3 : 4) void layernorm_i16_i8_tiled_compat_kernel(Ln16Args a, float s_in, float r_in)
{
    __shared__ float s_phi[WPB][64 * 8 * NJ];      // [wave][row of the wave][channel]
    __shared__ float s_sum[WPB][64];
    constexpr int RPW = 64 / LPR;
    constexpr bool REGSUM = LPR <= 16 && LPR * NJ < 64;      // fewer than 16 steps per vector lane, a row inside one DPP row
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & (LPR - 1), grp = lane / LPR;
    const int C = a.C, nd = C >> 3;
    const bool regsum = a.outer == 0 && nd == LPR * NJ && !(IVIT_LAB && a.lab_lds_sum);     // uniform
    // transposed view: groups of 16 need C < 256 (no second-level fold) and no tail columns (outer % 32 == 0: rowsum.h)
    const bool regouter = a.outer != 0 && (a.outer & 31) == 0 && nd == LPR * NJ && C < 256 && !(IVIT_LAB && a.lab_lds_sum);
    extern __shared__ __attribute__((aligned(16))) float ln16_tab[];      // [C] bias | [C] lo | [C] hi (ln16_build_table)
    float* t_bias = ln16_tab;
    float* t_lo = ln16_tab + C;
    float* t_hi = ln16_tab + 2 * C;
    ln16_build_table(a, t_bias, t_lo, t_hi);
    __syncthreads();
    const float fC = (float)C;
    for (int row0 = (blockIdx.x * WPB + wave) * RPW; row0 < a.rows; row0 += gridDim.x * WPB * RPW) {
        const int row = row0 + grp;
        const bool live = row < a.rows;
        const int16_t* xr = a.x + (int64_t)min(row, a.rows - 1) * C;
        v4i w[NJ];
        float ph[NJ][8];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int d = sub + LPR * j;
            w[j] = (d < nd) ? *reinterpret_cast<const v4i*>(xr + 8 * d) : v4i{0, 0, 0, 0};
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float x = (float)ln16_channel(w[j], c) * s_in;                                  // quant_modules.py:387
                const float q0 = x * r_in;                                          // :36  x / s_in (Markstein, see above)
                const float e = __builtin_fmaf(-s_in, q0, x);
                ph[j][c] = __builtin_fmaf(e, r_in, q0);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {                                           // :38 .to(int32) truncates
                const int k0 = (int)ph[j][2 * q], k1 = (int)ph[j][2 * q + 1];
                w[j][q] = (k0 & 0xffff) | (k1 << 16);
            }
        }
        float S;
        if (REGSUM && regouter) {
            // The reference's mean over the TRANSPOSED view (a.outer, every LayerNorm of Swin stage 0): torch's outer reduction adds a
            // row's elements in sequence, 16 at a time, and the group sums in sequence (rowsum.h torch_cascade_sum: no second-level
            // fold below 256 elements).  A group is two chunks of 8 = the chunks j of an even lane and its odd neighbour: the even
            // lane adds its 8, the odd lane CONTINUES that sum with its own 8; the group sums sit on the odd lanes and are added in
            // the order (j, lane) by the group's first lane.
            float gsum[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                float p = ph[j][0];
#pragma unroll
                for (int c = 1; c < 8; ++c) p += ph[j][c];
                float q = dpp_f32<0xa0>(p);                         // quad_perm [0,0,2,2]: the even neighbour's partial sum
#pragma unroll
                for (int c = 0; c < 8; ++c) q += ph[j][c];
                gsum[j] = q;                                        // meaningful on odd lanes
            }
            float fin = 0.f;
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int o = 1; o < LPR; o += 2) {
                    float t = gsum[j];
                    if (o == 1) t = dpp_f32<0x101>(t);              // row_shl:o -- lane l reads lane l + o
                    if (o == 3) t = dpp_f32<0x103>(t);
                    if (o == 5) t = dpp_f32<0x105>(t);
                    if (o == 7) t = dpp_f32<0x107>(t);
                    if (o == 9) t = dpp_f32<0x109>(t);
                    if (o == 11) t = dpp_f32<0x10b>(t);
                    if (o == 13) t = dpp_f32<0x10d>(t);
                    if (o == 15) t = dpp_f32<0x10f>(t);
                    fin = (j == 0 && o == 1) ? t : fin + t;
                }
            S = __shfl(fin, lane & ~(LPR - 1));
        } else if (REGSUM && regsum) {
            // torch's order without leaving the registers.  C = 8 LPR NJ < 512: 32 vector lanes p = e mod 32 each add their C / 32
            // elements in sequence (no cascade fold below 16 steps), the 8 lanes of a vector are ((a[l] + a[l+8]) + a[l+16]) + a[l+24],
            // the 8 results are added in sequence (rowsum.h).  Element e = 8 d + c of chunk d = sub + LPR j is vector lane
            // 8 (sub & 3) + c, step (LPR / 4) j + (sub >> 2): lane (sub & 3) of the row's first quad accumulates its own three
            // chunks and those of lanes sub + 4, + 8, + 12 (DPP row shifts: a row group never straddles a DPP row of 16), the quad
            // combines, everybody reads the result from the group's first lane.
            constexpr int H = LPR / 4;
            float acc[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[c] = ph[0][c];
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int hh = 0; hh < H; ++hh) {
                    if (j == 0 && hh == 0) continue;
#pragma unroll
                    for (int c = 0; c < 8; ++c) {
                        float t = ph[j][c];
                        if (hh == 1) t = dpp_f32<0x104>(t);         // row_shl:4: lane l reads lane l + 4
                        if (hh == 2) t = dpp_f32<0x108>(t);
                        if (hh == 3) t = dpp_f32<0x10c>(t);
                        acc[c] += t;
                    }
                }
            float fin = 0.f;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                float v = dpp_f32<0x00>(acc[c]);                    // quad_perm [0,0,0,0]
                v += dpp_f32<0x55>(acc[c]);
                v += dpp_f32<0xaa>(acc[c]);
                v += dpp_f32<0xff>(acc[c]);
                fin = c ? fin + v : v;
            }
            S = __shfl(fin, lane & ~(LPR - 1));
        } else {
        float* prow = s_phi[wave] + grp * C;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int d = sub + LPR * j;
            if (d < nd) {
                *reinterpret_cast<float4*>(prow + 8 * d) = make_float4(ph[j][0], ph[j][1], ph[j][2], ph[j][3]);
                *reinterpret_cast<float4*>(prow + 8 * d + 4) = make_float4(ph[j][4], ph[j][5], ph[j][6], ph[j][7]);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (a.outer) {   // transposed view in the reference: a lane sums one row in the outer-reduction order (serial cascade)
            if (lane < RPW) {
                const float* pr = s_phi[wave] + lane * C;
                const int rw = min(row0 + lane, a.rows - 1);
                s_sum[wave][lane] = torch_outer_rowsum([&](int i) { return pr[i]; }, C, rw % a.outer >= (a.outer & ~31));
            }
        } else {   // float32 row sums in torch's order: the two halves of the wave take two rows per round
            const int half = lane >> 5, l32 = lane & 31;
#pragma unroll 1
            for (int r0 = 0; r0 < RPW; r0 += 2) {
                const int rr = min(r0 + half, RPW - 1);
                const float* pr = s_phi[wave] + rr * C;
                const float Sr = rowsum32([&](int i) { return pr[i]; }, C, l32, 32 * half);
                if (l32 == 0 && r0 + half < RPW) s_sum[wave][rr] = Sr;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        S = s_sum[wave][grp];
        __builtin_amdgcn_wave_barrier();                                        // before the next iteration overwrites s_phi
        }
        const int mean_int = (int)rintf(S / fC);                                // :37
        ln16_tail<LPR, NJ>(a, w, mean_int, sub, live, min(row, a.rows - 1), t_bias, t_lo, t_hi);
    }
}

// ------------------------------------------------------------------------------------------------
// PatchMerging gather (swin_quant.py:337-344): [B, H*W, C] int16 -> [B, H/2*W/2, 4C], channel blocks
// (0::2,0::2), (1::2,0::2), (0::2,1::2), (1::2,1::2)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void patch_merge_kernel(const int16_t* x, int16_t* out, int B, int H, int W, int C)
{
    const int c4 = C >> 2;
    const int H2 = H >> 1, W2 = W >> 1;
    const int64_t total = (int64_t)B * H2 * W2 * 4 * c4;
    for (int64_t q = (int64_t)blockIdx.x * NT + threadIdx.x; q < total; q += (int64_t)gridDim.x * NT) {
        int cc = (int)(q % c4);
        int64_t r = q / c4;
        int blk = (int)(r & 3);
        r >>= 2;
        int x2 = (int)(r % W2);
        r /= W2;
        int y2 = (int)(r % H2);
        int b = (int)(r / H2);
        const int dy = blk & 1, dx = blk >> 1;
        const int2 v = *reinterpret_cast<const int2*>(x + (((int64_t)b * H + 2 * y2 + dy) * W + 2 * x2 + dx) * C + 4 * cc);
        *reinterpret_cast<int2*>(out + (((int64_t)b * H2 + y2) * W2 + x2) * (4 * C) + blk * C + 4 * cc) = v;
    }
}

// ------------------------------------------------------------------------------------------------
// Window partition + cyclic shift (or their inverse) of whole rows, any element type: a gather of 16-byte chunks.  Consecutive
// lanes walk the chunks of one destination row, then the next row: 16-byte loads and stores on both sides.  No LDS.
//   inverse == 0: dst row R (window order) = src row win_row_inv(R);   inverse == 1: dst row r (image order) = src row win_row(r)
// ------------------------------------------------------------------------------------------------
constexpr int WINDOW_ROWS_MAX_GRID = 2048;   // 8 workgroups per CU on 256 CUs; larger tensors take further trips of the loop

__global__ __launch_bounds__(NT) void window_rows_kernel(const v4i* src, v4i* dst, int64_t rows, int chunks, WinMap map, int inverse)
{
    const int64_t total = rows * chunks;
    for (int64_t q = (int64_t)blockIdx.x * NT + threadIdx.x; q < total; q += (int64_t)gridDim.x * NT) {
        const int64_t R = q / chunks;
        const int c = (int)(q - R * chunks);
        const int64_t r = inverse ? win_row(map, R) : win_row_inv(map, R);
        dst[q] = src[r * chunks + c];
    }
}

// ------------------------------------------------------------------------------------------------
// Token average pooling + QuantAct (swin_quant.py:554-555): z = round(fl32(sum_t k[t][c] / T)), requant -> int8
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void avgpool_kernel(const int8_t* x, int8_t* out, int B, int T, int C, double Mq)
{
    const int64_t total = (int64_t)B * C;
    for (int64_t q = (int64_t)blockIdx.x * NT + threadIdx.x; q < total; q += (int64_t)gridDim.x * NT) {
        const int b = (int)(q / C), c = (int)(q - (int64_t)b * C);
        int sum = 0;
        for (int t = 0; t < T; ++t) sum += x[((int64_t)b * T + t) * C + c];
        const float z = rintf((float)sum / (float)T);
        out[q] = (int8_t)clamp_i32(requant_exact((int)z, Mq), -128, 127);
    }
}

// ------------------------------------------------------------------------------------------------
// Windowed attention: one wave per (window, head); T = ws*ws tokens in NKT key tiles of 16, head_dim 32.
//   S^T = K . Q^T on v_mfma_i32_16x16x32_i8 (the head dimension is one instruction deep), qact_attn1 (8 bit),
//   + relative position bias through the two-operand qact2 (the bias operand RNE(k_tab * m / 2^e) is a load-time
//   constant table [nH, T, kp] int16, keys padded to whole key tiles), + shift mask (the integer -100/s wherever the region ids of
//   query and key differ, added after the clamp, swin_quant.py:149-155), Shiftmax, O^T = Vt . P^T on v_mfma_i32_16x16x64_i8 in
//   key steps of 64 (slots past T are zero probabilities), qact3.
//   NKT 4: 2..64 tokens (windows up to 8x8, Swin at 224 px): a row of scores is 16 per lane, P.V one key step, kp = 64, four
//          workgroups per CU.
//   NKT 9: 65..144 tokens (9x9 .. 12x12, Swin at 384 px): 36 scores per lane (and the literal form's 36 float views) stay in
//          registers at three workgroups per CU (<= 168 VGPRs), P.V up to 3 key steps, kp = 16 * ceil(T / 16).
//   The bias rows stay in global memory (L2): per score they are 2 bytes against the 16 of the score's 16x16x32 operand rows, and
//   staging them in LDS would add a wave barrier per query tile for data each wave reads once.
// ------------------------------------------------------------------------------------------------
struct WinAttnArgs {
    const int8_t* qkv;      // [3][B_][nH][T][32]
    int8_t* out;            // [B_*T, nH*32] with row stride ldo
    int64_t ldo;
    const int16_t* bias;    // [nH][T][kp]
    const uint8_t* region;  // [nW][kp] or NULL
    int mask_value;
    int nwin, heads, T, nW;
    double Ms, Mb, Mo;      // qact_attn1; qact2 main operand; qact3
    float Ms32, Mb32;       // rq32: the same as float32 -- both powers of two (every scale of the power-of-two regime): |S| <= 2^19 and
    int rq32;               // |kS| <= 128 make both products exact in float32, each fma rounds once, to nearest even, as the float64 form
    int x0, ksat;
    // natural Shiftmax input scale: phi[q + 128] = fl(fl(q*s)/s) for unmasked scores and phim[q + 128] =
    // fl(fl(fl(q*s) - 100)/s) for scores under the shift mask (swin_quant.py:151-156 adds float -100 to q*s before the softmax
    // divides by s), both float32 [256] on the device; NULL: power-of-two scale
    const float* phi;
    const float* phim;
    // natural scale, table form (round 4): band[(qmax + 128) * band_w + min(qmax - q, band_w - 1)] = Shiftmax's exp_int of the score
    // q under the row maximum qmax (prepare.shiftexp_band: the float32 sequence of ivit_modules.py:150-170 evaluated on the host for
    // every pair; entry band_w - 1 is the saturated value).  The host hands this over only when every score under the shift mask
    // saturates whatever the maximum and no masked score can be the maximum (prepare.window_shiftexp_band): masked scores then take
    // the saturated entry.  NULL: the literal form above (phi / phim) or the power-of-two form.
    const unsigned* band;
    int band_w;
    const unsigned* band1;  // ... and when the rows of that table do not depend on the maximum (often: prepare.window_shiftexp_band):
                            // its one row [band_w], used like the power-of-two form's table of distances
    // ws != 0: the output rows go to their IMAGE positions (window reverse + roll back applied here): the projection is
    // row-wise, so attn.proj and the residual QuantAct behind it then need no row map (and fuse into one GEMM)
    WinMap omap;
    int omap_inv;           // 65536 / ws + 1: (q * omap_inv) >> 16 == q / ws for q < T (NKT 4: q < 64)
    // SM 3, IBERTIntSoftmax (ibert_modules.py:237-319): exp_int behind its internal 16-bit QuantAct as the float32 the reference sums,
    // ib_tab[(qmax + 128) * 256 + q + 128] (ivit_ibert_softmax_build_table), or with band_w > 0 its band form
    // ib_tab[(qmax + 128) * band_w + min(qmax - q, band_w - 1)]; ib_sat: the one value of a score under the shift mask (the host
    // proves that every such score lands on int_exp's clamp and none is a row maximum, prepare.ibert_window_mask_ok)
    const float* ib_tab;
    float ib_sat;
};

constexpr int WHD = 32;
constexpr int WBAND_PAD = 4;     // dwords: keeps the slices 16-byte aligned and rotates their banks

// SM 3: IBERTIntSoftmax from its (row max, q) table; the 16 x T exponents of a query tile pass through the wave's slice of the dynamic
// LDS so that the four lanes of a query add them in torch's float32 order (window_rowsum below); p reaches 128 (split_p128).
// SM: Shiftmax form -- 0 the table of distances to the row maximum (power-of-two scales; natural scales whose band table has one
// row), 1 the literal float32 sequence on the phi tables, 2 band rows per row maximum staged through LDS.  Template parameters, not
// run-time branches: with all three forms in one body the kernel took 135 VGPRs = three workgroups per CU instead of four, and the
// power-of-two form lost 12 % (44 -> 49.5 us per call in Swin-T, profiles/r04q vs r04h).
// NKT: key tiles of 16 per row, 4 or 9; everything the two sizes differ in follows from it.  `if constexpr (NKT == 4)` keeps the
// statements that make the short form cheap where the uniform statement generated other code (profiles/HISTORY.md §9), and
// `if constexpr (NKT > 4)` the one arithmetic difference ("Large windows").
// kp_long: the bias / region row stride of NKT 9 (NKT 4 folds the literal 64).  A kernel parameter of its own, not a field of
// WinAttnArgs: as a field its scalar load merges with the neighbouring ones and the six NKT 9 forms lose the instruction sequence
// they were measured with (HISTORY.md §9).
// Occupancy: NKT 4 is compiled for four workgroups per CU, NKT 9 for three: the long form used 150-158 VGPRs and ran three per CU; with
// the ordered-sum branch of the Shiftmax forms (attn_parts.h SHIFTMAX_ORDER_SUM) a bound of two let it grow to 171-177 and lose the
// third workgroup, under a bound of three it stays at 165-168 without scratch (csrc/check_resources.py holds both).
// float32 sum of e[0 .. n - 1], 2 <= n <= 144, in the order of torch's CPU sum kernel (rowsum.h torch_rowsum, restated for ONE row per
// four lanes): with n / 8 <= 18 vectors the cascade never folds (its level step is 16 groups of four vectors), so partial p = key % 32
// adds its n / 32 elements in turn, the vectors past the last whole group of four join partials 0..7, lane sum l is
// ((P[l] + P[l+8]) + P[l+16]) + P[l+24], and the scalar tail goes first into the accumulator that then takes the eight lane sums.
// Lane g of the query computes lane sums 2g and 2g + 1; every lane of the wave calls it (gather4 exchanges).
IVIT_DEV float window_rowsum(const float* e, int n, int g)
{
    if (n < 8) {      // scalar_inner_sum: four accumulators
        float ps[4] = {0.f, 0.f, 0.f, 0.f};
        const int size_ilp = n >> 2;
        for (int i = 0; i < size_ilp; ++i)
            for (int k = 0; k < 4; ++k) ps[k] += e[i * 4 + k];
        for (int i = size_ilp * 4; i < n; ++i) ps[0] += e[i];
        for (int k = 1; k < 4; ++k) ps[0] += ps[k];
        return ps[0];
    }
    const int vec_size = n >> 3, size_ilp = vec_size >> 2;
    float v[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int l = 2 * g + j;
        float P[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            float acc = 0.f;
            for (int i = 0; i < size_ilp; ++i) acc += e[i * 32 + l + 8 * m];
            P[m] = acc;
        }
        for (int i = size_ilp * 4; i < vec_size; ++i) P[0] += e[i * 8 + l];
        v[j] = ((P[0] + P[1]) + P[2]) + P[3];
    }
    float t0[4], t1[4];
    gather4(v[0], t0);
    gather4(v[1], t1);
    float fin = 0.f;
    for (int i = vec_size * 8; i < n; ++i) fin += e[i];
#pragma unroll
    for (int gp = 0; gp < 4; ++gp) {
        fin += t0[gp];
        fin += t1[gp];
    }
    return fin;
}

// ORD (Shiftmax forms): the branch that gives a row whose exact sum reaches 2^24 its float32 sum in torch's order (attn_parts.h
// SHIFTMAX_ORDER_SUM).  Its registers cost the power-of-two form of NKT 4 its fifth workgroup per CU (94 -> 118 VGPRs, 80.6 -> 87.1 us
// per call at 8192 windows x 3 heads), so the launcher leaves it out (ORD false: the kernel as it was) where no row can get there:
// an exponent is at most |x0| * 2^15, T of them stay below 2^24 while T * |x0| < 512 -- Swin-T's 49 keys up to |x0| = 10.
template <int SM, bool RQ32, int NKT, bool ORD = true>
__global__ __launch_bounds__(NT, NKT == 4 ? 4 : 3) void window_attention_kernel(WinAttnArgs a, int kp_long)
{
    constexpr int NKS = (NKT + 3) / 4;               // P.V key steps of 64
    constexpr int VT_ROW = 64 * NKS;                 // Vt row: 64 key slots per step
    constexpr int VT_BYTES = WHD * VT_ROW;           // 2 / 6 KiB per wave
    constexpr int LUT_OFF = WPB * VT_BYTES;
    __shared__ __attribute__((aligned(16))) char smem[LUT_OFF + 256 * 4];
    __shared__ float s_phi[2][256];
    extern __shared__ __attribute__((aligned(16))) unsigned band_lds[];     // [4 waves][16 queries][band_w + WBAND_PAD], band form; SM 3:
                                                                            // [4 waves][16 queries][kp + 1] exponents
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, l15 = lane & 15;
    const int T = a.T;
    const int nkt = NKT == 4 ? NKT : (T + 15) >> 4, nks = (nkt + 3) >> 2;     // NKT 9: 5..9 key tiles, 2..3 key steps
    const int kp = NKT == 4 ? 64 : kp_long;
    constexpr bool band = SM == 2, compat = SM == 1, ibert = SM == 3;
    if constexpr (!ibert) reinterpret_cast<unsigned*>(smem + LUT_OFF)[tid] = a.band1 ? a.band1[min(tid, a.band_w - 1)] : shiftexp_int(-tid, a.x0, 15);
    if constexpr (compat) {
        s_phi[0][tid] = a.phi[tid];
        s_phi[1][tid] = a.phim[tid];
    }
    __syncthreads();
    const unsigned* lut = reinterpret_cast<const unsigned*>(smem + LUT_OFF);
    char* vt = smem + wave * VT_BYTES;
    const int64_t plane = (int64_t)a.nwin * a.heads * T * WHD;
    const int npairs = a.nwin * a.heads;

    for (int pair = blockIdx.x * WPB + wave; pair < npairs; pair += gridDim.x * WPB) {
        const int win = pair / a.heads, hh = pair - win * a.heads;
        // image position of the window (wave-uniform): its image, its window row / column
        int64_t img_base = 0;
        int wy0 = 0, wx0 = 0;
        if (a.omap.ws) {
            const int nwx = a.omap.W / a.omap.ws;
            const int bimg = win / a.nW, wrem = win - bimg * a.nW;
            const int wy = wrem / nwx;
            wy0 = wy * a.omap.ws + a.omap.shift;
            wx0 = (wrem - wy * nwx) * a.omap.ws + a.omap.shift;
            img_base = (int64_t)bimg * a.omap.H * a.omap.W;
        }
        const int8_t* qg = a.qkv + (int64_t)pair * T * WHD;
        const int8_t* kg = qg + plane;
        const int8_t* vg = qg + 2 * plane;
        // ---- V transposed into this wave's LDS tile: Vt[d][64 s + slot(chunk g') + 4t + r] = V[key 64 s + 16t + 4g' + r][d];
        //      chunk j of row d at slot (j + 2*((d>>2)&1)) & 3.  Work item = 4 keys x 16 d.  NKT 4: one guarded pass over the keys below T
        //      (13 x 2 items at 49 tokens); NKT 9: every slot of the nks segments written (keys past T repeat key T - 1: their
        //      probabilities are 0).
        __builtin_amdgcn_wave_barrier();
        const int nitems = NKT == 4 ? ((T + 3) >> 2) * 2 : nks * 32;
        for (int item = lane; item < nitems; item += 64) {
            const int kg4 = item >> 1, c = item & 1;
            v4i v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = *reinterpret_cast<const v4i*>(vg + (int64_t)min(4 * kg4 + r, T - 1) * WHD + 16 * c);
            const int key0 = 4 * kg4, seg = NKT == 4 ? 0 : key0 >> 6;
            const int j = (key0 >> 2) & 3, boff = 4 * ((key0 >> 4) & 3);
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const unsigned a0 = (unsigned)v[0][w], a1 = (unsigned)v[1][w], a2 = (unsigned)v[2][w], a3 = (unsigned)v[3][w];
                unsigned t4[4];
                bytes4x4_transpose(a0, a1, a2, a3, t4);
#pragma unroll
                for (int bb = 0; bb < 4; ++bb) {
                    const int d = 16 * c + 4 * w + bb;
                    *reinterpret_cast<unsigned*>(vt + d * VT_ROW + 64 * seg + (((j + 2 * ((d >> 2) & 1)) & 3) << 4) + boff) = t4[bb];
                }
            }
            if constexpr (NKT == 4) break;      // at most 32 items: a guarded pass, not a loop
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)

        // K fragments of the key tiles: lane (key 16kt + l15, 8 bytes at 8g); shift mask (swin_quant.py:223-249): tokens of different
        // regions of the rolled image do not attend to each other, kreg = the region ids of the lane's keys
        long kf[NKT];
        unsigned kreg[NKT];
        const uint8_t* regrow;
        if constexpr (NKT == 4) {      // all four tiles, unguarded (rows past T repeat row T - 1), the region row behind one branch
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt) {
                kf[kt] = *reinterpret_cast<const long*>(kg + (int64_t)min(16 * kt + l15, T - 1) * WHD + 8 * g);
                kreg[kt] = 0u;
            }
            regrow = a.region ? a.region + (win % a.nW) * 64 : nullptr;
            if (regrow) {
#pragma unroll
                for (int kt = 0; kt < NKT; ++kt) kreg[kt] = *reinterpret_cast<const unsigned*>(regrow + 16 * kt + 4 * g);
            }
        } else {
            regrow = a.region ? a.region + (int64_t)(win % a.nW) * kp : nullptr;
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt) {
                kf[kt] = 0;
                kreg[kt] = 0u;
                if (kt < nkt) {
                    kf[kt] = *reinterpret_cast<const long*>(kg + (int64_t)min(16 * kt + l15, T - 1) * WHD + 8 * g);
                    if (regrow) kreg[kt] = *reinterpret_cast<const unsigned*>(regrow + 16 * kt + 4 * g);
                }
            }
        }
        for (int qt = 0; qt < nkt; ++qt) {
            const int qrow = 16 * qt + l15;
            if constexpr (NKT == 4) {
                if (16 * qt >= T) break;  // uniform
            }
            const int qld = min(qrow, T - 1);
            const long qf = *reinterpret_cast<const long*>(qg + (int64_t)qld * WHD + 8 * g);
            const int16_t* brow = a.bias + ((int64_t)hh * T + qld) * kp + 4 * g;
            const unsigned qreg = regrow ? regrow[qld] : 0u;
            int s[NKT][4];
            int rmax = -100000;
            float xv[NKT][4], xmax = -__builtin_inff();     // compat: the float view x / s of every score
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt) {
                if constexpr (NKT > 4) {      // -100000 / -inf: no score (key or whole tile past T)
#pragma unroll
                    for (int r = 0; r < 4; ++r) { s[kt][r] = -100000; xv[kt][r] = -__builtin_inff(); }
                    if (kt >= nkt) continue;     // uniform
                }
                v4i acc = {0, 0, 0, 0};
                acc = __builtin_amdgcn_mfma_i32_16x16x32_i8(kf[kt], qf, acc, 0, 0, 0);
                const int2 bw = *reinterpret_cast<const int2*>(brow + 16 * kt);
                const int bv[4] = {(int)(int16_t)bw.x, bw.x >> 16, (int)(int16_t)bw.y, bw.y >> 16};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = 16 * kt + 4 * g + r;
                    int ka = -100000;
                    if constexpr (NKT == 4) xv[kt][r] = -__builtin_inff();      // NKT 4: the defaults per score, one store behind the branch
                    if (key < T) {
                        if constexpr (RQ32) {      // round 4: 7 float32 / integer instructions instead of 6 float64 ones + 3 (attention.hip RQ32)
                            const int tb = clamp_i32(__float_as_int(__builtin_fmaf((float)acc[r], a.Ms32, 12582912.0f)), 0x4B400000 - 128, 0x4B400000 + 127);
                            const float kSf = __int_as_float(tb) - 12582912.0f;                  // qact_attn1, exact small integer
                            ka = clamp_i32(__float_as_int(__builtin_fmaf(kSf, a.Mb32, 12582912.0f)) - 0x4B400000 + bv[r], -128, 127);
                        } else {
                            const int kS = clamp_i32(requant_exact(acc[r], a.Ms), -128, 127);        // qact_attn1
                            ka = clamp_i32(requant_exact(kS, a.Mb) + bv[r], -128, 127);              // qact2 (two operands)
                        }
                        const bool masked = ((kreg[kt] >> (8 * r)) & 0xffu) != qreg;
                        if constexpr (compat) xv[kt][r] = s_phi[masked ? 1 : 0][ka + 128];
                        if (masked) ka = (band || ibert) ? -50000 : ka + a.mask_value;           // shift mask, after the clamp
                        if constexpr (NKT > 4) s[kt][r] = ka;
                    }
                    if constexpr (NKT == 4) s[kt][r] = ka;
                    rmax = max(rmax, s[kt][r]);
                    xmax = fmaxf(xmax, xv[kt][r]);
                }
            }
            rmax = rows_allmax_i32(rmax);      // over the four lanes of a query (common.h: permlane swaps, no LDS round trip)
            unsigned esum = 0;
            float isum = 0.0f;
            if constexpr (ibert) {
                // IBERTIntSoftmax: e = table[row max][q] (float32), a masked score the saturated value (never the maximum: its own key
                // is unmasked), S = e.sum() in torch's float32 order over the T keys of the row (:311)
                const int rm = max(rmax, -128);
                const float* trow = a.ib_tab + (a.band_w ? (rm + 128) * a.band_w : ((rm + 128) << 8) + 128);
                float* erow = reinterpret_cast<float*>(band_lds) + (wave * 16 + l15) * (kp + 1);
                __builtin_amdgcn_wave_barrier();      // the previous tile's sums are done
#pragma unroll
                for (int kt = 0; kt < NKT; ++kt) {
                    if (NKT > 4 && kt >= nkt) {      // uniform; no key here
#pragma unroll
                        for (int r = 0; r < 4; ++r) s[kt][r] = 0;
                        continue;
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int sc = s[kt][r];
                        float e = 0.0f;
                        if (sc == -50000) e = a.ib_sat;
                        else if (sc != -100000) e = a.band_w ? trow[min(rm - sc, a.band_w - 1)] : trow[sc];
                        s[kt][r] = __float_as_int(e);
                        erow[16 * kt + 4 * g + r] = e;
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                isum = window_rowsum(erow, T, g);
            } else if constexpr (compat) {
                // Shiftmax's float32 sequence on the phi values themselves (ivit_modules.py:150-170), per score
                xmax = fmaxf(xmax, __shfl_xor(xmax, 16));
                xmax = fmaxf(xmax, __shfl_xor(xmax, 32));
                const float x0f = (float)a.x0;
#pragma unroll
                for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const unsigned e = (s[kt][r] == -100000) ? 0u : (unsigned)shiftexp_lit(xv[kt][r] - xmax, x0f);      // :168
                        s[kt][r] = ORD ? __float_as_int((float)e) : (int)e;      // ORD: the float32 value the product below takes
                        esum += e;
                    }
            } else if constexpr (band) {
                // the band rows of this tile's 16 queries go through LDS (as attention.hip MODE 1): the four lanes of a query copy
                // its row (band_w dwords, 16 bytes per lane and step), then every score is one LDS gather.  (Gathers straight from
                // the L2-resident table were as slow as the literal float sequence: profiles/r04m_*.)
                const int W = a.band_w, W1 = W - 1, stride = W + WBAND_PAD;
                const int rm = max(rmax, -128);
                unsigned* slice = band_lds + (wave * 16 + l15) * stride;
                __builtin_amdgcn_wave_barrier();      // the previous tile's gathers are done
                {
                    const uint4* src = reinterpret_cast<const uint4*>(a.band + (size_t)(rm + 128) * W);
                    uint4* dst = reinterpret_cast<uint4*>(slice);
                    for (int i = g; i < (W >> 2); i += 4) dst[i] = src[i];
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                unsigned ev[NKT][4];
                if constexpr (NKT == 4) {      // all sixteen gathers in flight before the first is used
#pragma unroll
                    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) ev[kt][r] = slice[min(rm - max(s[kt][r], -50000), W1)];
                }
#pragma unroll
                for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if constexpr (NKT > 4) ev[kt][r] = slice[min(rm - max(s[kt][r], -50000), W1)];
                        const unsigned e = (s[kt][r] == -100000) ? 0u : ev[kt][r];
                        s[kt][r] = ORD ? __float_as_int((float)e) : (int)e;      // ORD: the float32 value the product below takes
                        esum += e;
                    }
            } else {
#pragma unroll
                for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int d = rmax - s[kt][r];
                        unsigned e = 0u;
                        // NKT 9: a masked score lies |mask_value| - 255 or more below the maximum: beyond the table's 256 distances
                        // when Shiftmax has not saturated by distance 255 (|x0| above about 24), so those take the exact integer
                        // form (band1: the host's saturated entry).  NKT 4 takes the table's last entry, and its launcher rejects
                        // the geometries where that is not the saturated value.
                        bool in_table = true;
                        if constexpr (NKT > 4) in_table = d <= a.ksat || a.band1;
                        if (s[kt][r] != -100000) e = in_table ? lut[min(d, a.ksat) & 255] : shiftexp_int(-d, a.x0, 15);
                        s[kt][r] = ORD ? __float_as_int((float)e) : (int)e;      // ORD: the float32 value the product below takes
                        esum += e;
                    }
            }
            float factor;
            if constexpr (ibert) factor = floorf(4294967296.0f / isum) * 0.5f;      // ibert_modules.py:313; the half: see below
            else {
                const unsigned tot = rows_allsum_u32(esum);
                factor = shiftmax_factor(tot);
                // a row whose exact sum reaches 2^24: the reference's float32 sum is the one of torch's order (attn_parts.h
                // SHIFTMAX_ORDER_SUM).  Wave-uniform and rare; the other rows of the tile keep their factor.
                if (ORD && __builtin_expect(__builtin_amdgcn_ballot_w64(tot >= SHIFTMAX_ORDER_SUM) != 0, 0)) {
                    const float S = torch_rowsum_tiles<NKT>(s, [](int v) { return __int_as_float(v); }, T);
                    factor = tot >= SHIFTMAX_ORDER_SUM ? shiftmax_factor(S) : factor;
                }
            }
            // NKS 1: built in pk0 -- with element writes into an array of ONE vector the compiler unrolled the query-tile loop four times
            // (SM 1: 128 VGPRs and scratch)
            v4i pk[NKS], pk0;
            // I-BERT: p = floor(fl32(e * factor) / 2^25) in [0, 128] (:314, output_bit 8).  Halving the factor is exact, so
            // trunc(fl32(e * (factor / 2))) <= 2^31 has p in its top byte; p = 128 (a one-hot row) is the byte 0x80, one more than an int8
            // MFMA operand holds: 127 stays in pk, the 1 goes to pkh, a second P.V operand issued only where a wave holds such a byte
            v4i pkh[ibert ? NKS : 1];
            unsigned any_u = 0;
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    unsigned w = 0;
                    if (4 * ks + t < NKT) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            float pr;
                            if constexpr (ibert || ORD) pr = __int_as_float(s[4 * ks + t][r]) * factor;     // :175; I-BERT :314
                            else pr = (float)(unsigned)s[4 * ks + t][r] * factor;
                            if constexpr (ibert) any_u |= (unsigned)pr;
                            w |= ((((unsigned)pr) >> 24) & 0xffu) << (8 * r);
                        }
                    }
                    if constexpr (NKS == 1) pk0[t] = (int)w;
                    else pk[ks][t] = (int)w;
                }
            if constexpr (NKS == 1) pk[0] = pk0;
            bool any_hi = false;
            if constexpr (ibert) {
                any_hi = __builtin_amdgcn_ballot_w64((any_u >> 31) != 0) != 0;      // wave-uniform, rare
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        unsigned lo = (unsigned)pk[ks][t], hi = 0u;
                        if (any_hi) split_p128((unsigned)pk[ks][t], lo, hi);
                        pk[ks][t] = (int)lo;
                        pkh[ks][t] = (int)hi;
                    }
            }
            int64_t orow_idx = (int64_t)win * T + qrow;
            if (a.omap.ws) {      // window reverse + roll back: (iy, ix) of the query in its window -> (y, x) of the image
                const int qr = min(qrow, T - 1);
                const int iy = (qr * a.omap_inv) >> 16, ix = qr - iy * a.omap.ws;      // qr / ws for qr < T (checked by the launcher)
                int y = wy0 + iy, x = wx0 + ix;
                y = y >= a.omap.H ? y - a.omap.H : y;
                x = x >= a.omap.W ? x - a.omap.W : x;
                orow_idx = img_base + y * a.omap.W + x;
            }
            int8_t* orow = a.out + orow_idx * a.ldo + hh * WHD;
            unsigned wq[2];      // wq[dt]: bytes d = 16 dt + 4 g + 0..3 of this lane's query
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const int d = 16 * dt + l15;
                const char* vrow = vt + d * VT_ROW + (((g + 2 * ((d >> 2) & 1)) & 3) << 4);
                v4i acc = {0, 0, 0, 0};
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks)
                    if (ks < nks) {
                        acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(*reinterpret_cast<const v4i*>(vrow + 64 * ks), pk[ks], acc, 0, 0, 0);
                        if constexpr (ibert) {
                            if (any_hi) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(*reinterpret_cast<const v4i*>(vrow + 64 * ks), pkh[ks], acc, 0, 0, 0);
                        }
                    }
                unsigned w = 0;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    w |= ((unsigned)clamp_i32(requant_exact(acc[r], a.Mo), -128, 127) & 0xffu) << (8 * r);
                wq[dt] = w;
            }
            // the query's 32 bytes sit as 2 x 4 dwords in its four lanes: a word exchange (v_permlane32_swap, v_permlane16_swap)
            // leaves lane g with the 8 contiguous bytes d = 8 g .. 8 g + 7 -> one 8-byte store instead of two 4-byte ones
            {
                const v2u ab = __builtin_amdgcn_permlane32_swap(wq[0], wq[1], false, false);   // g < 2: (w0[g], w0[g+2]); g >= 2: (w1[g-2], w1[g])
                const v2u pr = __builtin_amdgcn_permlane16_swap(ab.x, ab.y, false, false);     // lane g: words 2 (g & 1), 2 (g & 1) + 1 of w_{g >> 1}
                if (qrow < T) *reinterpret_cast<int2*>(orow + 8 * g) = make_int2((int)pr.x, (int)pr.y);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Token average pooling + QuantAct at a natural input scale, literally (swin_quant.py:554-555 on the float view): the reference's
// avgpool(x.transpose(1, 2)) on y = fl(q * s) is torch's CPU mean over the transposed view, i.e. the outer-reduction sum of rowsum.h
// (column c of the contiguous extent C, a tail column when c >= 32 * (C / 32)) divided by float32(T); then qact3's own steps:
// z = rint(fl(mean / s)) and the requantisation to int8.  One thread per output (b, c).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void avgpool_literal_kernel(const int8_t* x, int8_t* out, int B, int T, int C, float s, double Mq)
{
    const int64_t total = (int64_t)B * C;
    const int cfull = C & ~31;
    for (int64_t q = (int64_t)blockIdx.x * NT + threadIdx.x; q < total; q += (int64_t)gridDim.x * NT) {
        const int b = (int)(q / C), c = (int)(q - (int64_t)b * C);
        const int8_t* col = x + (int64_t)b * T * C + c;
        const float sum = torch_outer_rowsum([&](int t) { return (float)col[(int64_t)t * C] * s; }, T, c >= cfull);
        const float mean = sum / (float)T;
        const float z = rintf(mean / s);
        out[q] = (int8_t)clamp_i32(requant_exact((int)z, Mq), -128, 127);
    }
}

// The float mean of that pooling alone, for the module path (swin_quant.py:554 on the float tensor it is handed): x [B, T, C] float32,
// out [B, C] = the same outer-reduction sum / float32(T).  One thread per output (b, c).
__global__ __launch_bounds__(NT) void avgpool_f32_literal_kernel(const float* x, float* out, int B, int T, int C)
{
    const int64_t total = (int64_t)B * C;
    const int cfull = C & ~31;
    for (int64_t q = (int64_t)blockIdx.x * NT + threadIdx.x; q < total; q += (int64_t)gridDim.x * NT) {
        const int b = (int)(q / C), c = (int)(q - (int64_t)b * C);
        const float* col = x + (int64_t)b * T * C + c;
        const float sum = torch_outer_rowsum([&](int t) { return col[(int64_t)t * C]; }, T, c >= cfull);
        out[q] = sum / (float)T;
    }
}

}  // namespace

// ================================================================================================
IVIT_EXPORT int ivit_requant_i8_i16(const int8_t* x, uint32_t m, int32_t e, int16_t* out, int64_t n, ivit_stream_t stream)
{
    IVIT_REQUIRE(x && out && n > 0, "ivit_requant_i8_i16: bad operand");
    const double Mq = ivit_dyadic_to_double(m, e);
    IVIT_REQUIRE(Mq < 8388608.0, "ivit_requant_i8_i16: multiplier too large");
    hipLaunchKernelGGL(requant_i8_i16_kernel, dim3(ew_grid(n)), dim3(NT), 0, ivit_stream(stream), x, Mq, out, n);
    IVIT_CHECK_LAUNCH("ivit_requant_i8_i16");
}

static int check_map(const char* who, int64_t rows, int H, int W, int ws, int shift)
{
    IVIT_REQUIRE(win_map_ok(rows, H, W, ws, shift), "%s: bad window map H=%d W=%d ws=%d shift=%d rows=%lld", who, H, W, ws, shift, (long long)rows);
    return IVIT_OK;
}

IVIT_EXPORT int ivit_residual_requant_i16(const void* a, int a_bits, const uint32_t* m_pre, const int32_t* e_pre,
                                          uint32_t m_a, int32_t e_a, const int16_t* res, uint32_t m_r, int32_t e_r,
                                          int16_t* out, int64_t rows, int C, int H, int W, int ws, int shift,
                                          ivit_stream_t stream)
{
    IVIT_REQUIRE(a && res && out && rows > 0 && C > 0 && C % 4 == 0, "ivit_residual_requant_i16: bad operand");
    IVIT_REQUIRE(a_bits == 8 || a_bits == 16 || a_bits == 32, "ivit_residual_requant_i16: a_bits must be 8, 16 or 32");
    IVIT_REQUIRE((a_bits == 32) == (m_pre != nullptr && e_pre != nullptr),
                 "ivit_residual_requant_i16: (m_pre, e_pre) are required for, and only for, int32 accumulators");
    IVIT_REQUIRE(((uintptr_t)a % 16 == 0) && ((uintptr_t)res % 8 == 0) && ((uintptr_t)out % 8 == 0) &&
                     ((uintptr_t)m_pre % 16 == 0) && ((uintptr_t)e_pre % 16 == 0),
                 "ivit_residual_requant_i16: misaligned operand");
    int rc = check_map("ivit_residual_requant_i16", rows, H, W, ws, shift);
    if (rc) return rc;
    const double Ma = ivit_dyadic_to_double(m_a, e_a), Mr = ivit_dyadic_to_double(m_r, e_r);
    IVIT_REQUIRE(Ma < 32768.0 && Mr < 32768.0, "ivit_residual_requant_i16: multiplier too large");
    WinMap map{H, W, ws, shift};
    const int grid = ew_grid(rows * (C / 4));
    hipStream_t st = ivit_stream(stream);
    if (a_bits == 8)
        hipLaunchKernelGGL(residual_i16_kernel<int8_t>, dim3(grid), dim3(NT), 0, st, reinterpret_cast<const int8_t*>(a),
                           m_pre, e_pre, Ma, res, Mr, out, rows, C, map);
    else if (a_bits == 16)
        hipLaunchKernelGGL(residual_i16_kernel<int16_t>, dim3(grid), dim3(NT), 0, st, reinterpret_cast<const int16_t*>(a),
                           m_pre, e_pre, Ma, res, Mr, out, rows, C, map);
    else
        hipLaunchKernelGGL(residual_i16_kernel<int32_t>, dim3(grid), dim3(NT), 0, st, reinterpret_cast<const int32_t*>(a),
                           m_pre, e_pre, Ma, res, Mr, out, rows, C, map);
    IVIT_CHECK_LAUNCH("ivit_residual_requant_i16");
}

// Do the tiled 16-bit LayerNorm kernels take this operand, and with which tiling: lpr = the smallest group of lanes that covers a
// row with nj <= 3 chunks of 8 channels per lane.
static bool ln16_tiling(const int16_t* x, int C, int64_t ldo, const float* bias_int, const float* s_ln, const uint32_t* m, const int32_t* e,
                        const int8_t* out, int* lpr, int* nj)
{
    if (!(C % 8 == 0 && C <= 1536 && ldo % 8 == 0 && ((uintptr_t)x % 16 == 0) && ((uintptr_t)out % 8 == 0) &&
          ((uintptr_t)bias_int % 16 == 0) && ((uintptr_t)s_ln % 16 == 0) && ((uintptr_t)m % 16 == 0) && ((uintptr_t)e % 16 == 0)))
        return false;
    const int nd = C / 8;
    *lpr = 4;
    while ((nd + *lpr - 1) / *lpr > 3) *lpr *= 2;
    *nj = (nd + *lpr - 1) / *lpr;
    return true;
}

// launch(integral_constant<LPR>, integral_constant<NJ>) for the tiling ln16_tiling chose: the eleven pairs it can return
template <class F>
static void ln16_dispatch(int lpr, int nj, F launch)
{
#define LN16_CASE(L, J) \
    if (lpr == L && nj == J) launch(std::integral_constant<int, L>(), std::integral_constant<int, J>())
    LN16_CASE(4, 1); LN16_CASE(4, 2); LN16_CASE(4, 3);
    LN16_CASE(8, 2); LN16_CASE(8, 3);
    LN16_CASE(16, 2); LN16_CASE(16, 3);
    LN16_CASE(32, 2); LN16_CASE(32, 3);
    LN16_CASE(64, 2); LN16_CASE(64, 3);
#undef LN16_CASE
}

IVIT_EXPORT int ivit_layernorm_i16_i8(const int16_t* x, int rows, int C, const float* bias_int, const float* s_ln,
                                      const uint32_t* m, const int32_t* e, int8_t* out, int64_t ldo, int H, int W, int ws,
                                      int shift, ivit_stream_t stream)
{
    IVIT_REQUIRE(x && out && bias_int && s_ln && m && e && rows > 0 && C > 0 && C <= 4096 && ldo >= C,
                 "ivit_layernorm_i16_i8: bad operand");
    int rc = check_map("ivit_layernorm_i16_i8", rows, H, W, ws, shift);
    if (rc) return rc;
    Ln16Args a{x, rows, C, bias_int, s_ln, m, e, out, ldo, WinMap{H, W, ws, shift}, 0, 0};
    hipStream_t st = ivit_stream(stream);
    int lpr, nj;
    if (!ln16_tiling(x, C, ldo, bias_int, s_ln, m, e, out, &lpr, &nj)) {
        hipLaunchKernelGGL(layernorm_i16_i8_kernel, dim3(grid_for_rows(rows)), dim3(NT), 0, st, a);
        IVIT_CHECK_LAUNCH("ivit_layernorm_i16_i8");
    }
    // four workgroups per CU (128 VGPRs since the constants moved to LDS, round 4); each builds the table once and strides over rows
    int nblk = grid_for_rows(rows, 64 / lpr);
    const int cap = ((g_ln_ablate >> 16) & 15) ? 256 * ((g_ln_ablate >> 16) & 15) : 1024;
    if (nblk > cap) nblk = cap;
    const size_t tab_bytes = (size_t)3 * C * sizeof(float);
    ln16_dispatch(lpr, nj, [&](auto L, auto J) {
        hipLaunchKernelGGL((layernorm_i16_i8_tiled_kernel<L.value, J.value>), dim3(nblk), dim3(NT), tab_bytes, st, a);
    });
    IVIT_CHECK_LAUNCH("ivit_layernorm_i16_i8");
}

IVIT_EXPORT int ivit_layernorm_i16_i8_compat(const int16_t* x, int rows, int C, float s_in, int fast_division,
                                             const float* bias_int, const float* s_ln, const uint32_t* m, const int32_t* e,
                                             int8_t* out, int64_t ldo, int H, int W, int ws, int shift, ivit_stream_t stream)
{
    IVIT_REQUIRE(x && out && bias_int && s_ln && m && e && rows > 0 && C > 0 && C <= 4096 && ldo >= C && s_in > 0.0f,
                 "ivit_layernorm_i16_i8_compat: bad operand");
    int rc = check_map("ivit_layernorm_i16_i8_compat", rows, H, W, ws, shift);
    if (rc) return rc;
    const int outer = fast_division >> 8;     // IVIT_LN_OUTER_MEAN(L)
    fast_division &= 255;
    IVIT_REQUIRE(outer >= 0 && (outer == 0 || rows % outer == 0) && fast_division <= 1, "ivit_layernorm_i16_i8_compat: bad flags");
    Ln16Args b{x, rows, C, bias_int, s_ln, m, e, out, ldo, WinMap{H, W, ws, shift}, outer, (g_ln_ablate >> 20) & 1};   // lab bit 20: sums through LDS
    hipStream_t st = ivit_stream(stream);
    int lpr, nj;
    if (fast_division && ln16_tiling(x, C, ldo, bias_int, s_ln, m, e, out, &lpr, &nj)) {
        int nblk = grid_for_rows(rows, 64 / lpr);
        if (nblk > (nj >= 2 ? 768 : 1024)) nblk = nj >= 2 ? 768 : 1024;      // = the kernel's launch bounds: 3 / 4 workgroups per CU
        const size_t tab_bytes = (size_t)3 * C * sizeof(float);
        const float r_in = 1.0f / s_in;
        ln16_dispatch(lpr, nj, [&](auto L, auto J) {
            hipLaunchKernelGGL((layernorm_i16_i8_tiled_compat_kernel<L.value, J.value>), dim3(nblk), dim3(NT), tab_bytes, st, b, s_in, r_in);
        });
        IVIT_CHECK_LAUNCH("ivit_layernorm_i16_i8_compat");
    }
    Ln16LitArgs a{b, s_in};
    hipLaunchKernelGGL(layernorm_i16_i8_literal_kernel, dim3(grid_for_rows(rows)), dim3(NT), 0, st, a);
    IVIT_CHECK_LAUNCH("ivit_layernorm_i16_i8_compat");
}

IVIT_EXPORT int ivit_layernorm_i16_f32(const int16_t* x, int64_t ldx, int B, int T_all, int t0, int T, int C, float s_in,
                                       const float* bias_int, const float* s_ln, float* out, int64_t ldo, int flags,
                                       ivit_stream_t stream)
{
    const char* who = "ivit_layernorm_i16_f32";
    const bool fast = (flags & IVIT_LN_F32_FAST_DIV) != 0;
    LnTok o;
    size_t lds;
    IVIT_REQUIRE(s_in >= 0.0f && (s_in > 0.0f || !fast), "%s: s_in is 0 (integers) or a positive scale; IVIT_LN_F32_FAST_DIV needs a scale", who);
    if (const int rc = ln_tok_check(who, x, 2, ldx, B, T_all, t0, T, C, bias_int, s_ln, out, ldo, flags & ~IVIT_LN_F32_FAST_DIV, 0, &o, &lds))
        return rc;
    const float r_in = s_in > 0.0f ? 1.0f / s_in : 0.0f;
    if (s_in == 0.0f) return ln_tok_launch(who, LnTokRowI16<false, false>{x, C, s_in, r_in, bias_int, s_ln}, o, lds, stream);
    if (fast) return ln_tok_launch(who, LnTokRowI16<true, true>{x, C, s_in, r_in, bias_int, s_ln}, o, lds, stream);
    return ln_tok_launch(who, LnTokRowI16<true, false>{x, C, s_in, r_in, bias_int, s_ln}, o, lds, stream);
}

IVIT_EXPORT int ivit_patch_merge_i16(const int16_t* x, int16_t* out, int batch, int H, int W, int C, ivit_stream_t stream)
{
    IVIT_REQUIRE(x && out && batch > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && C % 4 == 0,
                 "ivit_patch_merge_i16: bad operand");
    IVIT_REQUIRE(((uintptr_t)x % 8 == 0) && ((uintptr_t)out % 8 == 0), "ivit_patch_merge_i16: misaligned operand");
    const int64_t total = (int64_t)batch * (H / 2) * (W / 2) * C;
    hipLaunchKernelGGL(patch_merge_kernel, dim3(ew_grid(total)), dim3(NT), 0, ivit_stream(stream), x, out, batch, H, W, C);
    IVIT_CHECK_LAUNCH("ivit_patch_merge_i16");
}

IVIT_EXPORT int ivit_window_rows(const void* src, void* dst, int batch, int H, int W, int64_t row_bytes, int ws, int shift,
                                 int inverse, ivit_stream_t stream)
{
    IVIT_REQUIRE(src && dst, "ivit_window_rows: NULL operand");
    IVIT_REQUIRE(((uintptr_t)src % 16 == 0) && ((uintptr_t)dst % 16 == 0), "ivit_window_rows: misaligned operand (16 bytes)");
    IVIT_REQUIRE(batch > 0 && H > 0 && W > 0 && (int64_t)H * W <= (1 << 30), "ivit_window_rows: bad shape");
    IVIT_REQUIRE(row_bytes > 0 && row_bytes % 16 == 0 && row_bytes <= (1 << 20),
                 "ivit_window_rows: row_bytes must be a positive multiple of 16");
    IVIT_REQUIRE(ws > 0 && H % ws == 0 && W % ws == 0, "ivit_window_rows: the window does not divide the map");
    IVIT_REQUIRE(shift >= 0 && shift < ws, "ivit_window_rows: shift outside [0, ws)");
    IVIT_REQUIRE(inverse == 0 || inverse == 1, "ivit_window_rows: inverse must be 0 or 1");
    const int64_t rows = (int64_t)batch * H * W;
    const int64_t bytes = rows * row_bytes;
    const uintptr_t s = (uintptr_t)src, d = (uintptr_t)dst;
    IVIT_REQUIRE(s + (uintptr_t)bytes <= d || d + (uintptr_t)bytes <= s, "ivit_window_rows: src and dst overlap (not an in-place pass)");
    const int chunks = (int)(row_bytes / 16);
    const int64_t blocks = (rows * chunks + NT - 1) / NT;
    const int grid = (int)(blocks > WINDOW_ROWS_MAX_GRID ? WINDOW_ROWS_MAX_GRID : blocks);
    hipLaunchKernelGGL(window_rows_kernel, dim3(grid), dim3(NT), 0, ivit_stream(stream), reinterpret_cast<const v4i*>(src),
                       reinterpret_cast<v4i*>(dst), rows, chunks, WinMap{H, W, ws, shift}, inverse);
    IVIT_CHECK_LAUNCH("ivit_window_rows");
}

IVIT_EXPORT int ivit_avgpool_requant_i8(const int8_t* x, int8_t* out, int batch, int tokens, int C, uint32_t m, int32_t e,
                                        ivit_stream_t stream)
{
    IVIT_REQUIRE(x && out && batch > 0 && tokens > 0 && C > 0, "ivit_avgpool_requant_i8: bad operand");
    const double Mq = ivit_dyadic_to_double(m, e);
    IVIT_REQUIRE(Mq < 1048576.0, "ivit_avgpool_requant_i8: multiplier too large");
    hipLaunchKernelGGL(avgpool_kernel, dim3(ew_grid((int64_t)batch * C)), dim3(NT), 0, ivit_stream(stream), x, out, batch,
                       tokens, C, Mq);
    IVIT_CHECK_LAUNCH("ivit_avgpool_requant_i8");
}

// ---- window attention, host side: every exported entry fills a WinAttnDesc and returns window_attention_launch(desc)
namespace {

#include "win_attn_host.h"     // WinAttnDesc, win_attn_check, win_attn_form: shared with swin_probs.hip

// The instantiations of window_attention_kernel, by what selects them: SM, RQ32, long rows (NKT 9), ORD.  An empty slot is never
// selected: ORD false exists for the short Shiftmax forms only.  The table is written down from SM 3 to 0, RQ32 before the float64
// form and NKT 9 before 4, because a template is instantiated, and placed in the code object, where it is first named: this is the
// order the kernels have always had there, and their addresses were part of every measurement.  winattn_kernel does the indexing.
typedef void (*WinAttnKernel)(WinAttnArgs, int);
#define WINATTN_SHIFTMAX(SM)                                                                                                          \
    {{{nullptr, window_attention_kernel<SM, true, 9>}, {window_attention_kernel<SM, true, 4, false>, window_attention_kernel<SM, true, 4>}}, \
     {{nullptr, window_attention_kernel<SM, false, 9>}, {window_attention_kernel<SM, false, 4, false>, window_attention_kernel<SM, false, 4>}}}
const WinAttnKernel WINATTN_KERNELS[4][2][2][2] = {      // [3 - SM][!RQ32][!long][ORD]
    {{{nullptr, window_attention_kernel<3, true, 9>}, {nullptr, window_attention_kernel<3, true, 4>}},
     {{nullptr, window_attention_kernel<3, false, 9>}, {nullptr, window_attention_kernel<3, false, 4>}}},
    WINATTN_SHIFTMAX(2), WINATTN_SHIFTMAX(1), WINATTN_SHIFTMAX(0)};
#undef WINATTN_SHIFTMAX
inline WinAttnKernel winattn_kernel(int sm, bool rq32, bool long_rows, bool ord) { return WINATTN_KERNELS[3 - sm][!rq32][!long_rows][ord]; }

int window_attention_launch(WinAttnDesc d)
{
    if (const int rc = win_attn_check(d)) return rc;
    const WinSoftmaxForm f = win_attn_form(d);
    const int tokens = d.tokens;
    WinAttnArgs a{};
    a.qkv = d.qkv; a.out = static_cast<int8_t*>(d.out); a.ldo = d.ldo; a.bias = d.bias; a.region = d.region;
    a.nwin = d.windows; a.heads = d.heads; a.T = tokens; a.nW = d.windows_per_image;
    a.Ms = d.Ms; a.Mb = d.Mb; a.Mo = d.Mo;
    a.Ms32 = (float)d.Ms;
    a.Mb32 = (float)d.Mb;
    a.x0 = f.x0; a.ksat = f.ksat; a.mask_value = f.mask_value;
    a.phi = f.phi; a.phim = f.phim;
    a.band = f.band; a.band1 = f.band1; a.band_w = f.band_w;
    a.ib_tab = f.ib_tab; a.ib_sat = f.ib_sat;
    if (d.image_order) {
        a.omap = WinMap{d.H, d.W, d.ws, d.shift};
        a.omap_inv = 65536 / d.ws + 1;
    }
    // ---- the plan: kernel slot, grid, dynamic LDS, the key stride of the long rows
    const bool long_rows = tokens > 64;
    // both score multipliers powers of two (m = 2^k) and in float32's range: the float32 form of the two requantisations is exact
    a.rq32 = d.m_s != 0 && (d.m_s & (d.m_s - 1)) == 0 && d.m_b != 0 && (d.m_b & (d.m_b - 1)) == 0 && a.Ms >= 1e-30 && a.Mb >= 1e-30 &&
             a.Mb <= 4096.0 && !(g_ln_ablate & (1 << 23));      // lab bit 23: the float64 form (A/B, parity of both forms)
    // no row of `tokens` exponents of at most |x0| * 2^15 reaches 2^24: the short Shiftmax forms then run without the ordered-sum branch
    const bool ord = long_rows || f.sm == 3 || (int64_t)tokens * -(int64_t)f.x0 >= 512;
    const int npairs = d.windows * d.heads, blocks = (npairs + WPB - 1) / WPB, grid = blocks < 8192 ? blocks : 8192;
    const int kp = 16 * ((tokens + 15) >> 4);
    // I-BERT: the exponents of a query tile, [4 waves][16 queries][kp + 1] float32 (37 KB at 144 tokens, beside the kernel's 27 KB);
    // band rows: [4 waves][16 queries][band_w + WBAND_PAD] dwords
    const size_t lds_bytes = f.sm == 3 ? (size_t)WPB * 16 * ((long_rows ? kp : 64) + 1) * sizeof(float)
                             : f.band  ? (size_t)WPB * 16 * (f.band_w + WBAND_PAD) * sizeof(unsigned)
                                       : 0;
#if IVIT_LAB
    if (g_winattn_dry_run) return win_plan_record(d, f, a.rq32, long_rows, ord, grid, lds_bytes, kp, a.omap.ws, a.omap_inv, 0);
#endif
    hipLaunchKernelGGL(winattn_kernel(f.sm, a.rq32 != 0, long_rows, ord), dim3(grid), dim3(NT), lds_bytes, ivit_stream(d.stream), a, kp);
    IVIT_CHECK_LAUNCH(d.name);
}

}  // namespace

// The six fused entries (contracts: include/ivit_hip.h).  Descriptor order: name, family, qkv, out, ldo, bias, region, mask_value,
// windows, windows_per_image, heads, tokens, head_dim, m_s, e_s, m_b, e_b, s_attn, m_o, e_o, phi, phim, band, band_w, band_rows, ib_tab,
// masked_exp, H, W, ws, shift, image_order, stream, needs.
IVIT_EXPORT int ivit_window_attention_i8(const int8_t* qkv, int8_t* out, int64_t ldo, const int16_t* bias_add,
                                         const uint8_t* mask_region, int mask_value, int windows, int windows_per_image,
                                         int heads, int tokens, int head_dim, uint32_t m_s, int32_t e_s, uint32_t m_b,
                                         int32_t e_b, float s_attn, uint32_t m_o, int32_t e_o, ivit_stream_t stream)
{
    return window_attention_launch({"ivit_window_attention_i8", WIN_SHORT, qkv, out, ldo, bias_add, mask_region, mask_value, windows,
                                    windows_per_image, heads, tokens, head_dim, m_s, e_s, m_b, e_b, s_attn, m_o, e_o, nullptr, nullptr,
                                    nullptr, 0, 256, nullptr, 0.0f, 0, 0, 0, 0, 0, stream, 0});
}

IVIT_EXPORT int ivit_window_attention_i8_compat(const int8_t* qkv, int8_t* out, int64_t ldo, const int16_t* bias_add,
                                                const uint8_t* mask_region, int mask_value, int windows, int windows_per_image,
                                                int heads, int tokens, int head_dim, uint32_t m_s, int32_t e_s, uint32_t m_b,
                                                int32_t e_b, float s_attn, uint32_t m_o, int32_t e_o, const float* phi,
                                                const float* phi_masked, ivit_stream_t stream)
{
    return window_attention_launch({"ivit_window_attention_i8_compat", WIN_SHORT, qkv, out, ldo, bias_add, mask_region, mask_value,
                                    windows, windows_per_image, heads, tokens, head_dim, m_s, e_s, m_b, e_b, s_attn, m_o, e_o, phi,
                                    phi_masked, nullptr, 0, 256, nullptr, 0.0f, 0, 0, 0, 0, 0, stream, 0});
}

// (the band table carries the mask: mask_value 0; the geometry, where given, means image order)
IVIT_EXPORT int ivit_window_attention_i8_band(const int8_t* qkv, int8_t* out, int64_t ldo, const int16_t* bias_add,
                                              const uint8_t* mask_region, int windows, int windows_per_image, int heads, int tokens,
                                              int head_dim, uint32_t m_s, int32_t e_s, uint32_t m_b, int32_t e_b, float s_attn,
                                              uint32_t m_o, int32_t e_o, const uint32_t* band, int band_w, int band_rows, int H, int W,
                                              int ws, int shift, ivit_stream_t stream)
{
    return window_attention_launch({"ivit_window_attention_i8_band", WIN_SHORT, qkv, out, ldo, bias_add, mask_region, 0, windows,
                                    windows_per_image, heads, tokens, head_dim, m_s, e_s, m_b, e_b, s_attn, m_o, e_o, nullptr, nullptr,
                                    band, band_w, band_rows, nullptr, 0.0f, H, W, ws, shift, ws != 0, stream, WIN_NEEDS_BAND});
}

IVIT_EXPORT int ivit_window_attention_i8_unwindow(const int8_t* qkv, int8_t* out, int64_t ldo, const int16_t* bias_add,
                                                  const uint8_t* mask_region, int mask_value, int windows, int windows_per_image,
                                                  int heads, int tokens, int head_dim, uint32_t m_s, int32_t e_s, uint32_t m_b,
                                                  int32_t e_b, float s_attn, uint32_t m_o, int32_t e_o, const float* phi,
                                                  const float* phi_masked, int H, int W, int ws, int shift, ivit_stream_t stream)
{
    return window_attention_launch({"ivit_window_attention_i8_unwindow", WIN_SHORT, qkv, out, ldo, bias_add, mask_region, mask_value,
                                    windows, windows_per_image, heads, tokens, head_dim, m_s, e_s, m_b, e_b, s_attn, m_o, e_o, phi,
                                    phi_masked, nullptr, 0, 256, nullptr, 0.0f, H, W, ws, shift, 1, stream, WIN_NEEDS_GEOMETRY});
}

// (without a band table band_w and band_rows are not read, and with one mask_value is not)
IVIT_EXPORT int ivit_window_attention_i8_long(const int8_t* qkv, int8_t* out, int64_t ldo, const int16_t* bias_add,
                                              const uint8_t* mask_region, int mask_value, int windows, int windows_per_image, int heads,
                                              int tokens, int head_dim, uint32_t m_s, int32_t e_s, uint32_t m_b, int32_t e_b, float s_attn,
                                              uint32_t m_o, int32_t e_o, const float* phi, const float* phi_masked, const uint32_t* band,
                                              int band_w, int band_rows, int H, int W, int ws, int shift, int image_order,
                                              ivit_stream_t stream)
{
    return window_attention_launch({"ivit_window_attention_i8_long", WIN_LONG, qkv, out, ldo, bias_add, mask_region, band ? 0 : mask_value,
                                    windows, windows_per_image, heads, tokens, head_dim, m_s, e_s, m_b, e_b, s_attn, m_o, e_o, phi,
                                    phi_masked, band, band ? band_w : 0, band ? band_rows : 256, nullptr, 0.0f, H, W, ws, shift,
                                    image_order, stream, 0});
}

IVIT_EXPORT int ivit_window_attention_i8_ibert(const int8_t* qkv, int8_t* out, int64_t ldo, const int16_t* bias_add,
                                               const uint8_t* mask_region, float masked_exp, int windows, int windows_per_image, int heads,
                                               int tokens, int head_dim, uint32_t m_s, int32_t e_s, uint32_t m_b, int32_t e_b, uint32_t m_o,
                                               int32_t e_o, const float* table, int band_w, int H, int W, int ws, int shift, int image_order,
                                               ivit_stream_t stream)
{
    return window_attention_launch({"ivit_window_attention_i8_ibert", WIN_IBERT, qkv, out, ldo, bias_add, mask_region, 0, windows,
                                    windows_per_image, heads, tokens, head_dim, m_s, e_s, m_b, e_b, 1.0f, m_o, e_o, nullptr, nullptr,
                                    nullptr, band_w, 256, table, masked_exp, H, W, ws, shift, image_order, stream, 0});
}

#if IVIT_LAB
IVIT_EXPORT int ivit_debug_window_attention_dry_run(int on)
{
    g_winattn_dry_run = on;
    return IVIT_OK;
}

IVIT_EXPORT int ivit_debug_window_attention_last_plan(int32_t out[16])
{
    IVIT_REQUIRE(out, "ivit_debug_window_attention_last_plan: NULL operand");
    for (int i = 0; i < 16; ++i) out[i] = g_winattn_plan[i];
    return IVIT_OK;
}
#endif

IVIT_EXPORT int ivit_avgpool_requant_i8_literal(const int8_t* x, int8_t* out, int batch, int tokens, int C, float s_in, uint32_t m,
                                                int32_t e, ivit_stream_t stream)
{
    IVIT_REQUIRE(x && out && batch > 0 && tokens > 0 && C > 0 && s_in > 0.0f, "ivit_avgpool_requant_i8_literal: bad operand");
    const double Mq = ivit_dyadic_to_double(m, e);
    IVIT_REQUIRE(Mq < 1048576.0, "ivit_avgpool_requant_i8_literal: multiplier too large");
    hipLaunchKernelGGL(avgpool_literal_kernel, dim3(ew_grid((int64_t)batch * C)), dim3(NT), 0, ivit_stream(stream), x, out, batch,
                       tokens, C, s_in, Mq);
    IVIT_CHECK_LAUNCH("ivit_avgpool_requant_i8_literal");
}

IVIT_EXPORT int ivit_avgpool_f32_literal(const float* x, float* out, int batch, int tokens, int C, ivit_stream_t stream)
{
    IVIT_REQUIRE(x && out && batch > 0 && tokens > 0 && C > 0, "ivit_avgpool_f32_literal: bad operand");
    IVIT_REQUIRE(((uintptr_t)x % 4 == 0) && ((uintptr_t)out % 4 == 0), "ivit_avgpool_f32_literal: misaligned");
    hipLaunchKernelGGL(avgpool_f32_literal_kernel, dim3(ew_grid((int64_t)batch * C)), dim3(NT), 0, ivit_stream(stream), x, out, batch,
                       tokens, C);
    IVIT_CHECK_LAUNCH("ivit_avgpool_f32_literal");
}
