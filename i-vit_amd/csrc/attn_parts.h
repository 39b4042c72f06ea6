// attn_parts.h -- the device pieces the fused attention kernels share, stated ONCE (attention.hip: attention_kernel,
// attention_long_kernel, attention_cls_kernel; swin.hip: window_attention_kernel; literal.hip: shiftmax_f32_kernel).  Included inside
// the anonymous namespace of those files, after common.h.  Arithmetic and lane exchanges only: loads, stores and their addresses,
// loop structure, scheduling barriers and the lab ablation branches stay in the kernels.  Every helper is force-inlined and leaves
// each kernel's instruction sequence as it was (scripts/kernel_table.py, profiles/attn_parts_kernel_table.csv,
// profiles/window_attention_kernel_table.csv); where a kernel keeps a copy of its own, a helper in its place changed that sequence.
// Lane roles throughout: lane = 16 g + l15 owns query l15 of its tile and the keys 16 kt + 4 g + r of every key tile; the lanes
// l, l ^ 16, l ^ 32, l ^ 48 are "the four lanes of a query".
#pragma once

typedef unsigned v2u __attribute__((ext_vector_type(2)));

// ---- V^T staging: the 4 x 4 byte block of four consecutive keys (rows a0 .. a3, each holding d .. d + 3 in its bytes) transposed
// in registers with eight v_perm_b32: t[bb] = the 4 keys of d + bb, so every LDS write of V^T is a whole dword
IVIT_DEV void bytes4x4_transpose(unsigned a0, unsigned a1, unsigned a2, unsigned a3, unsigned (&t)[4])
{
    const unsigned lo01 = __builtin_amdgcn_perm(a1, a0, 0x05010400u);  // a0.b0 a1.b0 a0.b1 a1.b1
    const unsigned hi01 = __builtin_amdgcn_perm(a1, a0, 0x07030602u);  // a0.b2 a1.b2 a0.b3 a1.b3
    const unsigned lo23 = __builtin_amdgcn_perm(a3, a2, 0x05010400u);
    const unsigned hi23 = __builtin_amdgcn_perm(a3, a2, 0x07030602u);
    t[0] = __builtin_amdgcn_perm(lo23, lo01, 0x05040100u);   // d+0: a0.b0 a1.b0 a2.b0 a3.b0
    t[1] = __builtin_amdgcn_perm(lo23, lo01, 0x07060302u);   // d+1
    t[2] = __builtin_amdgcn_perm(hi23, hi01, 0x05040100u);   // d+2
    t[3] = __builtin_amdgcn_perm(hi23, hi01, 0x07060302u);   // d+3
}

// ---- Shiftmax's exponent on a float32 argument: int_exp_shift, ivit_modules.py:150-162 verbatim (n = 15), for d = x / s - max
// (:168) at ANY input scale.  The one statement of the literal sequence (literal.hip shiftmax_f32_kernel; the SM == 1 form of
// swin.hip window_attention_kernel on its phi values)
IVIT_DEV float shiftexp_lit(float d, float x0)
{
    float x = (d + floorf(d / 2.0f)) - floorf(d / 16.0f);     // :151
    x = fmaxf(x, 15.0f * x0);                                  // :155
    const float q = floorf(x / x0);                            // :157
    const float r = x - x0 * q;                                // :158
    float ex = r / 2.0f - x0;                                  // :159
    ex = floorf(ex * ldexpf(1.0f, 15 - (int)q));               // :160
    return fmaxf(ex, 0.0f);
}

// ---- Shiftmax factor (ivit_modules.py:171-174) from the row sum.  The reference's sum is a float32 sum of integers: below 2^24 it
// is exact whatever the order, and the integer forms below give it (the exact integer sum converts without rounding).  From
// SHIFTMAX_ORDER_SUM on, the reference's value is the one torch's CPU kernel reaches in ITS order of additions, every one rounded
// (rowsum.h; tests/golden/shiftmax_bigsum_kat.npz holds rows where the exact sum rounded once gives another factor): a kernel
// tests the exact sum against SHIFTMAX_ORDER_SUM and hands such rows' sum, taken in that order, to the float32 form.
// A kernel that holds the exponents as float32 only (attention_kernel MODE 0: one table gather per score) takes the test and the
// sum from a float32 sum in ITS OWN order, fsum.  Every exponent is a non-negative integer that float32 holds exactly
// ((r - 2 x0) 2^(14 - q), |x0| <= 4096: at most 15 significant bits).  (a) Exact total below 2^24: every term and every partial
// sum, of any grouping, is an integer below 2^24 and is held exactly, so fsum is the exact total = the reference's float32 sum.
// (b) Exact total at least 2^24: take, in the tree of additions that leads to fsum, a lowest node whose exact value reaches 2^24
// (the root's does).  It is a term, held exactly, or an addition of two nodes below 2^24, both exact by (a), whose exact sum
// rounds to no less than 2^24 (2^24 is representable, rounding is monotone).  Every addition above it adds a non-negative value,
// and fl(x + y) >= x for y >= 0.  So fsum >= 2^24 exactly when the exact total >= SHIFTMAX_ORDER_SUM, in every lane, whatever
// the lanes' order of additions; below it shiftmax_factor receives the same float as from the integer sum.
constexpr unsigned SHIFTMAX_ORDER_SUM = 1u << 24;
IVIT_DEV float shiftmax_factor(float S)
{
    S = fminf(S, 2147483648.0f);                               // clamp_max_(2**31-1) in float32 (:173)
    return floorf((1.0f / S) * 2147483648.0f);                 // (:174)
}
IVIT_DEV float shiftmax_factor(unsigned esum) { return shiftmax_factor((float)esum); }                // exp_int.sum (:171) below 2^24
IVIT_DEV float shiftmax_factor(unsigned long long esum) { return shiftmax_factor((float)esum); }      // long rows: the sum passes 2^32
// float32 sum over the four lanes of a query, (row 0 + row 1) + (row 2 + row 3) in every lane (common.h rows_allreduce_u32)
IVIT_DEV float rows_allsum_f32(float v)
{
    return __int_as_float((int)rows_allreduce_u32((unsigned)__float_as_int(v), [](unsigned x, unsigned y) {
        return (unsigned)__float_as_int(__int_as_float((int)x) + __int_as_float((int)y));
    }));
}

// ---- 8-bit probabilities: p = floor(fl32(e * factor) / 2^24) (:175) = the top byte of each product u, four gathered with two
// byte permutes
IVIT_DEV unsigned top_bytes(const unsigned (&u)[4])
{
    return __builtin_amdgcn_perm(u[1], u[0], 0x0c0c0703u) |     // [u0.b3, u1.b3, 0, 0]
           __builtin_amdgcn_perm(u[3], u[2], 0x07030c0cu);      // [0, 0, u2.b3, u3.b3]
}

// ---- 16-bit probabilities as 7-bit planes.  u = trunc(fl32(e * factor)) <= 2^31 and p16 = u >> 16 = floor(fl32(e * factor) / 2^16)
// (Shiftmax :175 with output_bit 16; I-BERT :314 is / 2^17, taken from the product with the halved factor): p16 = c + 128 b +
// 16384 a with plane c = bits 16..22 of u (byte 2 & 0x7f), plane b = bits 23..29 (byte 3 of u << 1, & 0x7f), plane a = bits 30, 31.
// One P.V MFMA set per plane; a is needed only where some u of the wave reaches 2^30, and is then taken from the products again.
IVIT_DEV unsigned plane_c(const unsigned (&u)[4])
{
    return (__builtin_amdgcn_perm(u[1], u[0], 0x0c0c0602u) | __builtin_amdgcn_perm(u[3], u[2], 0x06020c0cu)) & 0x7f7f7f7fu;
}
IVIT_DEV unsigned plane_b(const unsigned (&u)[4])
{
    return (__builtin_amdgcn_perm(u[1] << 1, u[0] << 1, 0x0c0c0703u) | __builtin_amdgcn_perm(u[3] << 1, u[2] << 1, 0x07030c0cu)) & 0x7f7f7f7fu;
}
IVIT_DEV unsigned plane_a_byte(unsigned u, int r) { return (u >> 30) << (8 * r); }      // key r's byte of the packed plane a

// ---- I-BERT: probabilities reach 128 (a one-hot row), one more than an int8 MFMA operand holds.  128 = 127 + 1: a byte 0x80 of w
// becomes 0x7f in lo and 1 in hi, the operand of a second P.V MFMA that is issued only where a wave holds such a byte.
IVIT_DEV void split_p128(unsigned w, unsigned& lo, unsigned& hi)
{
    const unsigned h128 = (w >> 7) & 0x01010101u;          // 1 in every byte that is 0x80
    lo = w - h128;                                         // 0x80 -> 0x7f (no borrow: the byte is >= 1)
    hi = h128;
}

// ---- all-gather over the four lanes of a query in VALU instructions: v_permlane32_swap of a value with itself leaves every lane
// with the values of rows {0,1} and {2,3} of 16 lanes, v_permlane16_swap of each of those with itself then separates row 0 / 1
// and row 2 / 3: out[g'] = the value lane 16 g' + l15 held
IVIT_DEV void gather4(float x, float (&out)[4])
{
    const unsigned xb = (unsigned)__float_as_int(x);
    const v2u h = __builtin_amdgcn_permlane32_swap(xb, xb, false, false);       // h.x: rows 0,1,0,1; h.y: rows 2,3,2,3
    const v2u a01 = __builtin_amdgcn_permlane16_swap(h.x, h.x, false, false);   // .x: row 0 everywhere, .y: row 1
    const v2u a23 = __builtin_amdgcn_permlane16_swap(h.y, h.y, false, false);   // .x: row 2, .y: row 3
    out[0] = __int_as_float((int)a01.x);
    out[1] = __int_as_float((int)a01.y);
    out[2] = __int_as_float((int)a23.x);
    out[3] = __int_as_float((int)a23.y);
}

// ---- torch's CPU float32 row sum (rowsum.h torch_rowsum) of a row of T >= 1 exponents spread over the four lanes of a query as the
// fused kernels hold it: key = 16 kt + 4 g + r.  With V = T >> 3 vectors of 8 and I = V >> 2 = T >> 5 interleaved steps of 32 keys,
// partial j = key % 32 takes keys j + 32 i, i < I: a lane owns the whole sequence of its eight partials (hi = kt & 1, r), which the
// caller adds up in that order (cascade included) into P[hi][r].  The at most 31 keys behind them -- key tiles 2 I (t0[r]) and
// 2 I + 1 (t1[r]): up to three vectors of 8 that join partials 0 .. 7, then the scalar tail -- are exchanged among the four lanes
// together with the partials, and every lane finishes the sum alike.  Keys at or behind T and absent tiles must be +0.0f, which
// changes no sum of non-negative terms.  Every lane of the wave calls it.
IVIT_DEV float torch_rowsum_finish(const float (&P)[2][4], const float (&t0)[4], const float (&t1)[4], int T)
{
    if (T < 8) {       // scalar_inner_sum: four accumulators over keys 0 .. 7 = t0 of the lanes g = 0, 1
        float x[8];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float G[4];
            gather4(t0[r], G);
            x[r] = G[0];
            x[4 + r] = G[1];
        }
        float ps0 = T >= 4 ? x[0] : 0.0f;
#pragma unroll
        for (int i = 0; i < 8; ++i)
            ps0 += (i >= (T & 4) && i < T) ? x[i] : 0.0f;      // the keys behind the whole group of four (T >= 4) or all of them, in order
        if (T >= 4) {
            ps0 += x[1];
            ps0 += x[2];
            ps0 += x[3];
        }
        return ps0;
    }
    // partials 0 .. 7 (hi = 0 of the lanes g = 0, 1) take the vectors behind the interleaved part: vector 0 = this lane's own keys of
    // tile 2 I, vector 1 = those of lane g + 2, vector 2 = its own of tile 2 I + 1; then v_l = ((P_l + P_{l+8}) + P_{l+16}) + P_{l+24},
    // l = 4 g + r: P_{l+8}, P_{l+24} are lane g + 2's.  v_permlane32_swap of a value with itself: .y = the value of lane + 32 in the
    // lanes below 32 (the other lanes' results are not used)
    auto upper = [&](float x) -> float {
        const unsigned xb = (unsigned)__float_as_int(x);
        const v2u h = __builtin_amdgcn_permlane32_swap(xb, xb, false, false);
        return __int_as_float((int)h.y);
    };
    const int nx = (T >> 3) - 4 * (T >> 5);    // 0 .. 3 vectors of 8 behind the interleaved part
    float vl[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float Q = P[0][r];
        Q += nx > 0 ? t0[r] : 0.0f;
        Q += nx > 1 ? upper(t0[r]) : 0.0f;
        Q += nx > 2 ? t1[r] : 0.0f;
        vl[r] = ((Q + upper(P[0][r])) + P[1][r]) + upper(P[1][r]);
    }
    // scalar tail: keys 8 V .. T - 1 (at most 7, in the half tile behind the last vector) in order, first into the final accumulator;
    // then v_0 .. v_7
    float fin = 0.0f;
    const bool odd = nx & 1, second = nx >= 2;
    float lo[4], hi[4];                        // the tail's half tile: lanes g' = 2 (nx & 1) and + 1
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float G[4];
        gather4(second ? t1[r] : t0[r], G);
        lo[r] = odd ? G[2] : G[0];
        hi[r] = odd ? G[3] : G[1];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) fin += lo[r];
#pragma unroll
    for (int r = 0; r < 4; ++r) fin += hi[r];
    float v0[4], v1[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float G[4];
        gather4(vl[r], G);
        v0[r] = G[0];
        v1[r] = G[1];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) fin += v0[r];
#pragma unroll
    for (int r = 0; r < 4; ++r) fin += v1[r];
    return fin;
}

// the same for a row that sits in registers as s[kt][r] (val(s[kt][r]) = the float32 exponent of key 16 kt + 4 g + r, +0.0f at and
// behind T), NKT <= 31 key tiles: fewer than 16 interleaved steps, so the cascade never folds and partial (hi, r) is the plain
// sequence of the tiles 2 m + hi, m < I.  I is a run-time value: the tiles are selected by value, never by a register index.
template <int NKT, class VAL>
IVIT_DEV float torch_rowsum_tiles(const int (&s)[NKT][4], VAL val, int T)
{
    static_assert(NKT <= 31, "the cascade of torch's sum folds after 16 steps of 32 keys");
    const int I = T >> 5;
    float P[2][4], t0[4], t1[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        P[0][r] = P[1][r] = t0[r] = t1[r] = 0.0f;
#pragma unroll
        for (int m = 0; 2 * m < NKT; ++m) {
            const float e0 = val(s[2 * m][r]);
            P[0][r] += m < I ? e0 : 0.0f;
            t0[r] = m == I ? e0 : t0[r];
            if (2 * m + 1 < NKT) {
                const float e1 = val(s[2 * m + 1][r]);
                P[1][r] += m < I ? e1 : 0.0f;
                t1[r] = m == I ? e1 : t1[r];
            }
        }
    }
    return torch_rowsum_finish(P, t0, t1, T);
}

// ---- output tail: O^T = Vt . P^T requantised (attn.qact2) to int8, one accumulator element.
//   PB 4, 8 (one byte plane of probabilities):  |O| <= 1025 * 127 * 128 < 2^24: the float64 product is exact, one fma against the magic constant (requant_exact).
//   PB 16: O = o + (o_b << 7) + (o_a << 14) = sum p16 * v over the three planes, below 2^30 (bounds: attention_long_kernel); the
//          reference's float64 product rounds at 53 bits first (quant_utils.py:229-230), so product and rounding are two steps.
template <int PB>
IVIT_DEV int attn_out_requant(int o, int o_b, int o_a, double Mo)
{
    if constexpr (PB == 16) {
        const int O = o + (o_b << 7) + (o_a << 14);
        const double t = (double)O * Mo + IVIT_MAGIC;
        return clamp_i32((int)(unsigned)__double_as_longlong(t), -128, 127);
    } else {
        return clamp_i32(requant_exact(o, Mo), -128, 127);
    }
}
// the low bytes of four values in one dword, by two byte permutes and an OR
IVIT_DEV unsigned low_bytes(const int (&v)[4])
{
    return __builtin_amdgcn_perm((unsigned)v[1], (unsigned)v[0], 0x0c0c0400u) | __builtin_amdgcn_perm((unsigned)v[3], (unsigned)v[2], 0x04000c0cu);
}
// one 16 d x 16 queries accumulator tile -> bytes d = 16 dt + 4 g + 0..3 of this lane's query
template <int PB>
IVIT_DEV unsigned attn_out_word(const v4i& o, const v4i& o_b, const v4i& o_a, double Mo)
{
    int ob[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) ob[r] = attn_out_requant<PB>(o[r], o_b[r], o_a[r], Mo);
    return low_bytes(ob);
}
// A query's 64 output bytes sit as 4 x 4 dwords in its four lanes (wq[dt] of lane g).  A 4 x 4 word transpose across those lanes --
// two v_permlane32_swap, two v_permlane16_swap -- leaves lane g with the 16 CONTIGUOUS bytes d = 16 g .. 16 g + 15: one 16-byte
// store per lane instead of four 4-byte ones (a quarter of the store instructions and of the segments the memory pipeline has to
// merge).  Every lane of the wave takes part.
IVIT_DEV v4i attn_out_transpose(const unsigned (&wq)[4])
{
    const v2u ab = __builtin_amdgcn_permlane32_swap(wq[0], wq[2], false, false);    // g < 2: (w0[g], w0[g+2]); g >= 2: (w2[g-2], w2[g])
    const v2u cd = __builtin_amdgcn_permlane32_swap(wq[1], wq[3], false, false);    // g < 2: (w1[g], w1[g+2]); g >= 2: (w3[g-2], w3[g])
    const v2u ac = __builtin_amdgcn_permlane16_swap(ab.x, cd.x, false, false);      // (w_g[0], w_g[1]) of the lanes 0, 1
    const v2u bd = __builtin_amdgcn_permlane16_swap(ab.y, cd.y, false, false);      // (w_g[2], w_g[3])
    return v4i{(int)ac.x, (int)ac.y, (int)bd.x, (int)bd.y};
}
