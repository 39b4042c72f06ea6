// ln_chain.h -- the tail of the reference's LayerNorm + QuantAct chain for one element, stated ONCE for every int8-output I-ViT
// LayerNorm kernel (rowops.hip, ln_stream.h, swin.hip).  Included inside the anonymous namespace of those files, after common.h.
// Arithmetic only: loads, stores, scheduling barriers and the lab ablation branches stay in the kernels.  The float-emitting
// token-feature kernel (ln_tokens.h) takes the chain up to y (ln_y) and ends in ln_f32 instead of the QuantAct.
// Reference: ivit_modules.py:45-63 (IVITIntLayerNorm), quant_utils.py:220, 229-230 (fixedpoint_mul).
//
// With y = floor((x - mean) * factor / 2) + bias_int (:52, :61) the tail for one element is  x = y * s_ln (:63, float32),
// z = round(x / s_ln) (quant_utils.py:220, float32 quotient),  out = clamp8(RNE(float64(z) * M)) (:229-230), M = m * 2^-e.  It costs
// six float64 instructions per element when evaluated literally (ln_literal).  Fast path (ln_cert): z = y * (1 + eps) with
// |eps| <= 2^-22 (two float32 roundings of relative size 2^-24 each, plus the round() step, which is a no-op for |y| >= 2^23, moves
// 2^22 <= |y| < 2^23 by at most 1/2 <= |y| * 2^-23 and gives back z = y exactly for |y| < 2^22), so the real number
// the reference rounds lies between y * lo and y * hi for float32 lo <= M * (1 - 1.25 * 2^-22), hi >= M * (1 + 1.25 * 2^-22)
// (common.h ln_build_table derives the bracket).
// t_lo = fma(y, lo, 1.5 * 2^23) and t_hi = fma(y, hi, 1.5 * 2^23) are RNE(y * lo) and RNE(y * hi) exactly (one rounding,
// ulp 1) while |y * hi| < 2^22; RNE is monotone, so t_lo == t_hi certifies the reference's result.  Products beyond
// 2^22 saturate the int8 clamp on either side whatever their rounding (float bit patterns are monotone), so they need
// no separate range test.  Whatever shares an `unc` accumulator with an uncertified element (a row, a row pair, a 16-byte chunk:
// about 1 % of the rows) is redone literally by its kernel, wave-uniformly.
#pragma once

typedef float v2f __attribute__((ext_vector_type(2)));

// :45-49  the ten Newton steps as the reference runs them: float32, every division correctly rounded
IVIT_DEV float ln_newton10_literal(float varf)
{
    float t = 65536.0f;
#pragma unroll 1
    for (int it = 0; it < 10; ++it) t = floorf((t + floorf(varf / t)) * 0.5f);
    return t;
}

// The certificate on the two biased bit patterns: |tl - th| accumulates into unc (v_sad_u32: one instruction), the clamp on the
// biased pattern leaves the int8 result in the low byte.
IVIT_DEV int ln_cert_bits(int tl, int th, unsigned& unc)
{
    asm("v_sad_u32 %0, %1, %2, %3" : "=v"(unc) : "v"(tl), "v"(th), "v"(unc));
    return clamp_i32(tl, 0x4B400000 - 128, 0x4B400000 + 127);
}

IVIT_DEV int ln_cert(float y, float lo, float hi, unsigned& unc)
{
    return ln_cert_bits(__float_as_int(__builtin_fmaf(y, lo, 12582912.0f)), __float_as_int(__builtin_fmaf(y, hi, 12582912.0f)), unc);
}

// the low bytes of four certified patterns as one dword
IVIT_DEV int ln_cert_pack(const int (&o)[4])
{
    const unsigned w01 = __builtin_amdgcn_perm((unsigned)o[1], (unsigned)o[0], 0x0c0c0400u);
    const unsigned w23 = __builtin_amdgcn_perm((unsigned)o[3], (unsigned)o[2], 0x04000c0cu);
    return (int)(w01 | w23);
}

// The literal tail of one element.
IVIT_DEV int ln_literal(float y, float s, double M)
{
    const float x = y * s;                                      // :63  float32 product
    // quant_utils.py:220  z = round(x / s): the correctly rounded float32 quotient, obtained as RN24(RN53(x * RN53(1/s)))
    // (no midpoint can lie within 2^-52 of x/s)
    const float z = rintf((float)((double)x * (1.0 / (double)s)));
    const double t = (double)z * M + IVIT_MAGIC;                // :229 float64 product, :230 round half to even
    return clamp_i32((int)(unsigned)__double_as_longlong(t), -128, 127);
}

// One dword of int8 inputs, given as wu = bytes x + 128 (v_cvt_f32_ubyteN) with mean128 = mean + 128; hfactor = factor / 2 (the
// halving of :52 is an exact scaling, so it commutes with the float32 product).  Scalar float32 form.
IVIT_DEV int ln_cert4(unsigned wu, float mean128, float hfactor, const float (&bias)[4], const float (&lo)[4], const float (&hi)[4],
                      unsigned& unc)
{
    int o[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float dl = (float)((wu >> (8 * c)) & 0xffu) - mean128;   // x - mean, exact
        const float v = floorf(dl * hfactor);                          // :52
        const float y = v + bias[c];                                   // :61
        o[c] = ln_cert(y, lo[c], hi[c], unc);
    }
    return ln_cert_pack(o);
}

// The same with two channels per packed float32 instruction (v_pk_add / v_pk_mul / v_pk_fma: the same IEEE operations, two lanes
// of data per issue slot); floor, the certificate and the clamp stay scalar.  Which kernel takes which form: DESIGN.md section 4
// (the price list) and the streaming kernel's 128-VGPR limit.
IVIT_DEV int ln_cert4_pk(unsigned wu, float mean128, float hfactor, const float (&bias)[4], const float (&lo)[4], const float (&hi)[4],
                         unsigned& unc)
{
    int o[4];
#pragma unroll
    for (int c = 0; c < 4; c += 2) {
        const v2f xf = {(float)((wu >> (8 * c)) & 0xffu), (float)((wu >> (8 * c + 8)) & 0xffu)};
        const v2f dl = xf - (v2f){mean128, mean128};                   // x - mean, exact
        const v2f pr = dl * (v2f){hfactor, hfactor};                   // :52
        const v2f vv = {floorf(pr.x), floorf(pr.y)};
        const v2f y = vv + (v2f){bias[c], bias[c + 1]};                // :61
        const v2f tlv = __builtin_elementwise_fma(y, (v2f){lo[c], lo[c + 1]}, (v2f){12582912.0f, 12582912.0f});
        const v2f thv = __builtin_elementwise_fma(y, (v2f){hi[c], hi[c + 1]}, (v2f){12582912.0f, 12582912.0f});
#pragma unroll
        for (int k = 0; k < 2; ++k) o[c + k] = ln_cert_bits(__float_as_int(tlv[k]), __float_as_int(thv[k]), unc);
    }
    return ln_cert_pack(o);
}

// y of one element from the integer the LayerNorm sees, literally (hfactor = factor / 2, as above)
IVIT_DEV float ln_y(int x, int mean_int, float hfactor, float bias)
{
    const float dl = (float)(x - mean_int);
    const float v = floorf(dl * hfactor);                              // :52
    return v + bias;                                                   // :61
}

// One dword of (signed) int8 inputs, literally.
IVIT_DEV int ln_literal4(int w, int mean_int, float hfactor, const float (&bias)[4], const float (&sl)[4], const double (&Mq)[4])
{
    int o[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = ln_literal(ln_y((int)(int8_t)(w >> (8 * c)), mean_int, hfactor, bias[c]), sl[c], Mq[c]);
    return pack4(o[0], o[1], o[2], o[3]);
}

// The float-emitting end of the chain (ln_tokens.h: the token-feature kernels): what IVITIntLayerNorm itself returns, x = y * s_ln
// (:63, one float32 product), without the QuantAct behind it.
IVIT_DEV float ln_f32(float y, float s) { return y * s; }
