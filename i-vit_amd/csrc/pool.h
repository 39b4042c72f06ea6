// pool.h -- what the pooled-LayerNorm entries (ln_pool.h, instantiated in rowops.hip, swin.hip and ibert.hip) share with pool.hip:
// the description of a launch, the one statement of the slab rule, the operand checks and the second pass.
#pragma once
#include "common.h"

// One pooled launch: tokens t0 .. t0 + T - 1 of each of the B images of a token-major stream (row (b, t) at
// (b * T_all + t0 + t) * ldx), cut into `slabs` slabs of L consecutive tokens per image (the last one may be short).
struct LnPool {
    int B, T_all, t0, T, C;
    int64_t ldx;
    const float* bias_int;
    const float* s_ln;
    const uint32_t* m;      // qact2: dyadic(s_ln[c] / s_feat)
    const int32_t* e;
    int L, slabs;
    int32_t* ws;            // [B][slabs][C] partial sums
};

constexpr int LN_POOL_T_MAX = 1025;      // |sum| <= 128 * 1025: far inside int32 (and the sequence limit of the attention entries)
constexpr int LN_POOL_C_MAX = 2048;      // 28 bytes of LDS per channel (three float tables, four waves' accumulators) + a kind's tables

// The slab rule, stated once: L = max(4, ceil(B * T / 1024)) tokens per slab.
//  - at least 4: a slab writes 4 C bytes of partial sums and reads at least 4 C bytes of int8 rows, so no launch writes more
//    partials than it reads rows, and each of a workgroup's four waves has a row;
//  - about 1024 workgroups (four per CU on 256 CUs) once B * T exceeds 4096 rows; below that one workgroup per 4 rows, so that a
//    single image of 196 patch tokens still spreads over 49 CUs.
static inline int ln_pool_slab_rows(int B, int T)
{
    const int64_t rows = (int64_t)B * T;
    const int64_t L = (rows + 1023) / 1024;
    return (int)(L < 4 ? 4 : L);
}

// Operand checks of all four entries, then the plan into *o.  esz: bytes per element of x; tab_bytes: the static LDS tables of the
// kind.  `out` is the first byte written (the caller's out + col0).  Nothing is launched on an error.
int ln_pool_check(const char* who, const void* x, size_t esz, int64_t ldx, int B, int T_all, int t0, int T, int C, const float* bias_int,
                  const float* s_ln, const uint32_t* m, const int32_t* e, const int32_t* sum, const int8_t* out, int64_t ldo, int64_t col0,
                  const void* workspace, int64_t workspace_bytes, int tab_bytes, LnPool* o);

// Second pass: sum[b][c] = sum over the slabs of ws[b][slab][c], mean = floor((2 * sum + T) / (2 * T)) as int8 at out[b * ldo + c].
int ln_pool_finish(const char* who, const LnPool& o, int32_t* sum, int8_t* out, int64_t ldo, hipStream_t st);
