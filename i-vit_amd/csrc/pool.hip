// pool.hip -- pooled backbone features: the mean over the patch tokens of LayerNorm + qact2, as exact integers.
// The first pass lives in ln_pool.h (one kernel template over the row types of the token-feature entries, instantiated where those
// types are: rowops.hip, swin.hip, ibert.hip); it leaves one int32 [C] partial sum per (image, slab) in a workspace.  Here: the slab
// rule's two host functions, the operand checks all four entries share, and the second pass, which adds the slabs and rounds.
//
// Rounding.  mean = floor((2 * sum + T) / (2 * T)): sum / T rounded to the nearest integer, halves up (towards +infinity), in integer
// arithmetic -- C++ division truncates, so a negative numerator with a remainder takes one more step down.  A mean of int8 values
// lies in [-128, 127], and so does its rounding: no clamp.  Integer sums do not depend on the slab count or on the order of the
// waves, so (sum, mean) are unique for any tiling; no float, no atomics.
#include "pool.h"

namespace {

constexpr int PF_NT = 256;

IVIT_DEV int pool_round_mean(int s, int T)
{
    const int num = 2 * s + T, den = 2 * T;      // |num| <= 2 * 128 * 1025 + 1025
    const int q = num / den;
    return q - (num % den < 0 ? 1 : 0);
}

// one thread per four channels of an image: 16-byte loads of every slab's partial, one 16-byte store of the sums, one dword of means
__global__ __launch_bounds__(PF_NT) void ln_pool_finish_kernel(const int32_t* __restrict__ ws, int B, int slabs, int C, int T,
                                                               int32_t* __restrict__ sum, int8_t* __restrict__ out, int64_t ldo)
{
    const int c4 = C >> 2;
    const int64_t idx = (int64_t)blockIdx.x * PF_NT + threadIdx.x;
    if (idx >= (int64_t)B * c4) return;
    const int b = (int)(idx / c4), c = (int)(idx - (int64_t)b * c4) * 4;
    const int32_t* p = ws + (int64_t)b * slabs * C + c;
    v4i s = {0, 0, 0, 0};
    for (int k = 0; k < slabs; ++k) s += *reinterpret_cast<const v4i*>(p + (int64_t)k * C);
    if (sum) *reinterpret_cast<v4i*>(sum + (int64_t)b * C + c) = s;
    unsigned w = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) w |= ((unsigned)pool_round_mean(s[k], T) & 0xffu) << (8 * k);
    *reinterpret_cast<unsigned*>(out + (int64_t)b * ldo + c) = w;
}

int pool_shape(const char* who, int B, int T)
{
    IVIT_REQUIRE(B >= 1 && T >= 1, "%s: B=%d T=%d must both be at least 1", who, B, T);
    if (T > LN_POOL_T_MAX) {
        ivit_set_error("%s: T=%d unsupported (at most %d tokens are pooled)", who, T, LN_POOL_T_MAX);
        return IVIT_ERR_UNSUPPORTED;
    }
    return IVIT_OK;
}

}      // namespace

int ln_pool_check(const char* who, const void* x, size_t esz, int64_t ldx, int B, int T_all, int t0, int T, int C, const float* bias_int,
                  const float* s_ln, const uint32_t* m, const int32_t* e, const int32_t* sum, const int8_t* out, int64_t ldo, int64_t col0,
                  const void* workspace, int64_t workspace_bytes, int tab_bytes, LnPool* o)
{
    IVIT_REQUIRE(x && out && bias_int && s_ln && m && e && workspace, "%s: NULL operand", who);
    if (const int rc = pool_shape(who, B, T)) return rc;
    IVIT_REQUIRE(C >= 1, "%s: C=%d must be at least 1", who, C);
    IVIT_REQUIRE(t0 >= 0 && (int64_t)t0 + T <= T_all, "%s: tokens %d .. %lld of T_all=%d", who, t0, (long long)t0 + T - 1, T_all);
    IVIT_REQUIRE(ldx >= C && col0 >= 0 && ldo >= col0 + C, "%s: ldx=%lld below C=%d, or columns %lld .. %lld outside a row of ldo=%lld", who,
                 (long long)ldx, C, (long long)col0, (long long)col0 + C - 1, (long long)ldo);
    IVIT_REQUIRE((uintptr_t)x % esz == 0 && (uintptr_t)bias_int % 4 == 0 && (uintptr_t)s_ln % 4 == 0 && (uintptr_t)m % 4 == 0 &&
                     (uintptr_t)e % 4 == 0,
                 "%s: a pointer is not aligned to its element", who);
    // the second pass moves four channels per thread: 16-byte partials and sums, one dword of means
    IVIT_REQUIRE((uintptr_t)out % 4 == 0 && (B == 1 || ldo % 4 == 0), "%s: out + col0 and ldo must be multiples of 4 bytes", who);
    IVIT_REQUIRE((uintptr_t)sum % 16 == 0 && (uintptr_t)workspace % 16 == 0, "%s: sum and workspace must be 16-byte aligned", who);
    if (C % 4 != 0 || C > LN_POOL_C_MAX || (size_t)28 * C + (size_t)tab_bytes > 65536) {
        ivit_set_error("%s: C=%d unsupported (a multiple of 4, at most %d)", who, C, LN_POOL_C_MAX);
        return IVIT_ERR_UNSUPPORTED;
    }
    const int L = ln_pool_slab_rows(B, T), slabs = (T + L - 1) / L;
    IVIT_REQUIRE(workspace_bytes >= (int64_t)B * slabs * C * 4, "%s: workspace of %lld bytes, %lld needed (ivit_layernorm_pool_workspace_bytes)",
                 who, (long long)workspace_bytes, (long long)B * slabs * C * 4);
    o->B = B; o->T_all = T_all; o->t0 = t0; o->T = T; o->C = C;
    o->ldx = ldx; o->bias_int = bias_int; o->s_ln = s_ln; o->m = m; o->e = e;
    o->L = L; o->slabs = slabs;
    o->ws = static_cast<int32_t*>(const_cast<void*>(workspace));
    return IVIT_OK;
}

int ln_pool_finish(const char* who, const LnPool& o, int32_t* sum, int8_t* out, int64_t ldo, hipStream_t st)
{
    const int64_t threads = (int64_t)o.B * (o.C >> 2);
    hipLaunchKernelGGL(ln_pool_finish_kernel, dim3((unsigned)((threads + PF_NT - 1) / PF_NT)), dim3(PF_NT), 0, st, o.ws, o.B, o.slabs, o.C,
                       o.T, sum, out, ldo);
    IVIT_CHECK_LAUNCH(who);
}

IVIT_EXPORT int ivit_layernorm_pool_slab_rows(int B, int T, int* rows)
{
    IVIT_REQUIRE(rows, "ivit_layernorm_pool_slab_rows: NULL operand");
    if (const int rc = pool_shape("ivit_layernorm_pool_slab_rows", B, T)) return rc;
    *rows = ln_pool_slab_rows(B, T);
    return IVIT_OK;
}

IVIT_EXPORT int ivit_layernorm_pool_workspace_bytes(int B, int T, int C, int64_t* bytes)
{
    IVIT_REQUIRE(bytes && C >= 1, "ivit_layernorm_pool_workspace_bytes: NULL operand or C=%d below 1", C);
    if (const int rc = pool_shape("ivit_layernorm_pool_workspace_bytes", B, T)) return rc;
    const int L = ln_pool_slab_rows(B, T);
    *bytes = (int64_t)B * ((T + L - 1) / L) * C * 4;
    return IVIT_OK;
}
