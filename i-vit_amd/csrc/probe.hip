// probe.hip -- the exact integer statistics a closed-form linear classifier needs from an int8 feature bank.
//   ivit_gram_i8_i64         gram[i][j] = sum_r x[r][i] * x[r][j] on v_mfma_i32_16x16x64_i8: int32 partial Grams of row ranges in the
//                            workspace, summed into int64 by a second small kernel (no float, no atomics: unique for any tiling)
//   ivit_group_sums_i8_i64   sums[g][c] = sum of x[perm[t]][c] over the rows t of group g (the CSR form of the labels): the
//                            inverted-index form of a scatter-add, every row read once, 16 bytes per lane, nothing added atomically
//
// The Gram kernel.  The contraction runs over bank rows, the strided dimension of the bank, so both MFMA operands are transposed
// reads of one row tile.  A workgroup (4 waves) owns one pair (bi <= bj) of 64-channel blocks and one row range of at most GR_CHUNK
// rows; wave w walks the 64-row tiles w, w + 4, ... of the range and keeps the whole 64 x 64 block in 16 accumulator quads.  A tile
// (64 rows x 64 bytes per block) goes into the wave's LDS stage as it lies, 16 bytes per lane; lane (g = lane >> 4, l15 = lane & 15)
// then reads the dword of channels 4 l15 .. 4 l15 + 3 of the rows 4 t + g, t = 0 .. 15 (ds_read_b32: 32 banks per 32-lane half,
// g = 0 / 1 on banks 0-15 / 16-31: no conflict) and transposes every four of them in registers (eight v_perm_b32): fragment f of the
// lane is channel 4 l15 + f in the K slots (g, t) <-> tile row 4 t + g.  The order of the K slots is free -- the sum is over rows --
// and both operands use the same one.  mfma(frag fa of block bi, frag fb of block bj): acc[r] of lane (g, l15) is the entry
// (4 (4 g + r) + fa, 4 l15 + fb) of the block.  Rows beyond the range are staged as zeros.
// No int32 overflows: a product is at most 2^14 and a range holds at most GR_CHUNK = 65536 rows, so |sum| <= 2^30 -- per wave and
// for the four waves together.  A segment longer than that is cut into ranges with a slab each: the widening happens in the reducer.
// At the end the four waves add their blocks in LDS one after the other and the workgroup writes the block, and for bi < bj its
// mirror image, into the range's slab.
#include "common.h"

namespace {

#include "attn_parts.h"

constexpr int GR_NT = 256;                   // threads per workgroup (four waves)
constexpr int GR_RT = 64;                    // bank rows per tile = the K of one MFMA
constexpr int GR_CB = 64;                    // channels per block
constexpr int GR_CHUNK = 65536;              // rows per int32 slab: 65536 * 2^14 = 2^30
constexpr int GR_LDB = GR_CB + 1;            // row stride (ints) of the block image the epilogue transposes

struct GramArgs {
    const int8_t* x;
    int64_t ldx, rows;
    int C, nb;                // nb = C / 64
    int64_t seg;              // rows per segment (a multiple of GR_RT)
    int cps;                  // ranges (slabs) per segment
    int pairs;                // nb (nb + 1) / 2
    int32_t* ws;              // [splits * cps][C][C]
};

// the 16 x 64-row transposed fragments of one 64-channel block: fr[f] = channel 4 l15 + f, K slot (g, t) = tile row 4 t + g
IVIT_DEV void gram_frags(const unsigned* st, int g, int l15, v4i (&fr)[4])
{
    unsigned d[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) d[t] = st[(4 * t + g) * (GR_CB / 4) + l15];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        unsigned o[4];
        bytes4x4_transpose(d[4 * q], d[4 * q + 1], d[4 * q + 2], d[4 * q + 3], o);
#pragma unroll
        for (int f = 0; f < 4; ++f) fr[f][q] = (int)o[f];
    }
}

__global__ __launch_bounds__(GR_NT, 2) void gram_partial_kernel(GramArgs a)
{
    __shared__ __attribute__((aligned(16))) unsigned stage[4][2][GR_RT * GR_CB / 4];      // per wave: block bi, block bj
    __shared__ int blk[GR_CB * GR_LDB];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l15 = lane & 15;
    const int p = (int)(blockIdx.x % (unsigned)a.pairs);
    const int64_t slab = blockIdx.x / (unsigned)a.pairs;
    int bi = 0, bj = p;
    while (bj >= a.nb - bi) {
        bj -= a.nb - bi;
        ++bi;
    }
    bj += bi;
    const bool diag = bi == bj;
    const int64_t s = slab / a.cps, c = slab % a.cps;
    int64_t r_begin = s * a.seg + c * GR_CHUNK, r_end = r_begin + GR_CHUNK;
    if (r_end > (s + 1) * a.seg) r_end = (s + 1) * a.seg;
    if (r_end > a.rows) r_end = a.rows;
    if (r_begin > r_end) r_begin = r_end;
    const int ntiles = (int)((r_end - r_begin + GR_RT - 1) / GR_RT);      // <= GR_CHUNK / GR_RT

    v4i acc[4][4];
#pragma unroll
    for (int fa = 0; fa < 4; ++fa)
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) acc[fa][fb] = v4i{0, 0, 0, 0};

    // lane -> (row lane >> 2 of each 16-row quarter, 16-byte piece lane & 3) of the 64 x 64-byte tile: 1 KiB contiguous in LDS per store
    const int8_t* xa = a.x + GR_CB * bi + 16 * (lane & 3);
    const int8_t* xb = a.x + GR_CB * bj + 16 * (lane & 3);
    v4i ra[4], rb[4];
    auto fetch = [&](int tile) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t row = r_begin + (int64_t)tile * GR_RT + 16 * i + (lane >> 2);
            ra[i] = rb[i] = v4i{0, 0, 0, 0};
            if (tile < ntiles && row < r_end) {
                ra[i] = *reinterpret_cast<const v4i*>(xa + row * a.ldx);
                if (!diag) rb[i] = *reinterpret_cast<const v4i*>(xb + row * a.ldx);
            }
        }
    };
    fetch(wave);
    for (int t0 = 0; t0 < ntiles; t0 += 4) {      // the same number of rounds for every wave: the barriers are uniform
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<v4i*>(&stage[wave][0][(16 * i) * (GR_CB / 4) + 4 * lane]) = ra[i];
            if (!diag) *reinterpret_cast<v4i*>(&stage[wave][1][(16 * i) * (GR_CB / 4) + 4 * lane]) = rb[i];
        }
        __syncthreads();
        fetch(t0 + 4 + wave);
        if (t0 + wave < ntiles) {
            v4i fa_[4], fb_[4];
            gram_frags(stage[wave][0], g, l15, fa_);
            if (diag) {
#pragma unroll
                for (int f = 0; f < 4; ++f) fb_[f] = fa_[f];
            } else {
                gram_frags(stage[wave][1], g, l15, fb_);
            }
#pragma unroll
            for (int fa = 0; fa < 4; ++fa)
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) acc[fa][fb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa_[fa], fb_[fb], acc[fa][fb], 0, 0, 0);
        }
        __syncthreads();
    }

    // the four waves' blocks, added in LDS one wave after the other (every lane owns the same 64 entries in each)
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int fa = 0; fa < 4; ++fa)
#pragma unroll
                for (int fb = 0; fb < 4; ++fb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        int* e = &blk[(4 * (4 * g + r) + fa) * GR_LDB + 4 * l15 + fb];
                        *e = (w ? *e : 0) + acc[fa][fb][r];
                    }
        }
        __syncthreads();
    }
    int32_t* out = a.ws + slab * ((int64_t)a.C * a.C);
    for (int e = tid; e < GR_CB * GR_CB; e += GR_NT) {
        const int i = e >> 6, j = e & 63;
        out[(int64_t)(GR_CB * bi + i) * a.C + GR_CB * bj + j] = blk[i * GR_LDB + j];
        if (!diag) out[(int64_t)(GR_CB * bj + i) * a.C + GR_CB * bi + j] = blk[j * GR_LDB + i];
    }
}

// gram[e] = (accumulate ? gram[e] : 0) + the sum of the slabs' entry e, in int64
__global__ __launch_bounds__(GR_NT) void gram_reduce_kernel(const int32_t* __restrict__ ws, int slabs, int n, int accumulate, int64_t* __restrict__ gram)
{
    const int e = (int)(blockIdx.x * GR_NT + threadIdx.x);
    if (e >= n) return;
    int64_t v = accumulate ? gram[e] : 0;
    for (int k = 0; k < slabs; ++k) v += ws[(int64_t)k * n + e];
    gram[e] = v;
}

// ---- group sums: one workgroup per group.  C / 16 lanes cover a row (16 bytes each), the workgroup's GR_NT / (C / 16) row slots walk
// the group's rows side by side; a lane adds its 16 channels in int32 for at most 2^16 rows (|sum| <= 2^23) and widens, the slots are
// added in LDS
__global__ __launch_bounds__(GR_NT) void group_sums_kernel(const int8_t* __restrict__ x, int64_t ldx, int C, const int32_t* __restrict__ perm,
                                                           const int64_t* __restrict__ group_ptr, int accumulate, int64_t* __restrict__ sums)
{
    __shared__ int64_t part[GR_NT * 16];      // [slot][C]
    const int tid = threadIdx.x, lpr = C >> 4, slots = GR_NT / lpr, slot = tid / lpr, lc = tid - slot * lpr;
    const int64_t grp = blockIdx.x, begin = group_ptr[grp], end = group_ptr[grp + 1];
    int64_t tot[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) tot[k] = 0;
    if (slot < slots) {
        const int8_t* xc = x + 16 * lc;
        int64_t t = begin + slot;
        while (t < end) {
            int s32[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) s32[k] = 0;
            for (int n = 0; n < 65536 && t < end; n += 4, t += 4 * (int64_t)slots) {
                int64_t row[4];
                v4i v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int64_t tu = t + (int64_t)u * slots;
                    row[u] = tu < end ? (int64_t)perm[tu] : -1;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    v[u] = v4i{0, 0, 0, 0};
                    if (row[u] >= 0) v[u] = *reinterpret_cast<const v4i*>(xc + row[u] * ldx);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        const int w = v[u][d];
                        s32[4 * d + 0] += (int)(int8_t)(w & 0xff);
                        s32[4 * d + 1] += (int)(int8_t)((w >> 8) & 0xff);
                        s32[4 * d + 2] += (int)(int8_t)((w >> 16) & 0xff);
                        s32[4 * d + 3] += w >> 24;
                    }
            }
#pragma unroll
            for (int k = 0; k < 16; ++k) tot[k] += s32[k];
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) part[(int64_t)slot * C + 16 * lc + k] = tot[k];
    }
    __syncthreads();
    for (int c = tid; c < C; c += GR_NT) {
        int64_t* o = sums + grp * C + c;
        int64_t v = accumulate ? *o : 0;
        for (int sl = 0; sl < slots; ++sl) v += part[sl * C + c];
        *o = v;
    }
}

// the bank geometry both entries share (knn.FeatureBank's)
int probe_check_shape(const char* who, int64_t rows, int C)
{
    if (C < 64 || C > 1024 || C % 64 != 0) {
        ivit_set_error("%s: unsupported geometry (C=%d: multiples of 64 from 64 to 1024)", who, C);
        return IVIT_ERR_UNSUPPORTED;
    }
    IVIT_REQUIRE(rows >= 0 && rows <= 0x7fffffffLL, "%s: rows=%lld outside [0, 2^31)", who, (long long)rows);
    return IVIT_OK;
}

int probe_check_rows(const char* who, const int8_t* x, int64_t ldx, int C)
{
    IVIT_REQUIRE(ldx >= C, "%s: ldx=%lld below C=%d", who, (long long)ldx, C);
    IVIT_REQUIRE(((uintptr_t)x | (uintptr_t)ldx) % 16 == 0, "%s: x and ldx must be multiples of 16 bytes", who);
    return IVIT_OK;
}

// row segments: the caller's count, or (0) enough workgroups for two rounds of the 256 CUs without segments below 1024 rows
int gram_splits(int64_t rows, int C, int splits)
{
    if (splits > 0) return splits;
    const int nb = C / GR_CB, pairs = nb * (nb + 1) / 2;
    const int64_t want = (512 + pairs - 1) / pairs, cap = rows / 1024;
    const int64_t sp = want < cap ? want : cap;
    return (int)(sp < 1 ? 1 : sp > IVIT_GRAM_SPLITS_MAX ? IVIT_GRAM_SPLITS_MAX : sp);
}

// -> segment length, slabs per segment and the workspace size for a checked shape
int gram_plan(const char* who, int64_t rows, int C, int splits, int* sp, int64_t* seg, int* cps, int64_t* bytes)
{
    if (const int rc = probe_check_shape(who, rows, C)) return rc;
    IVIT_REQUIRE(splits >= 0 && splits <= IVIT_GRAM_SPLITS_MAX, "%s: splits=%d outside [0, %d]", who, splits, IVIT_GRAM_SPLITS_MAX);
    *sp = gram_splits(rows, C, splits);
    *seg = ((rows + *sp - 1) / *sp + GR_RT - 1) / GR_RT * GR_RT;
    *cps = (int)((*seg + GR_CHUNK - 1) / GR_CHUNK);
    *bytes = (int64_t)*sp * *cps * C * C * (int64_t)sizeof(int32_t);      // rows == 0: no slab, no workspace
    return IVIT_OK;
}

}      // namespace

IVIT_EXPORT int ivit_gram_workspace_bytes(int64_t rows, int C, int splits, int64_t* bytes)
{
    const char* who = "ivit_gram_workspace_bytes";
    IVIT_REQUIRE(bytes, "%s: NULL pointer", who);
    int sp, cps;
    int64_t seg, need;
    const int rc = gram_plan(who, rows, C, splits, &sp, &seg, &cps, &need);
    if (rc != IVIT_OK) return rc;
    *bytes = need;
    return IVIT_OK;
}

IVIT_EXPORT int ivit_gram_i8_i64(const int8_t* x, int64_t ldx, int64_t rows, int C, int splits, int accumulate, int64_t* gram, void* workspace,
                                 int64_t workspace_bytes, ivit_stream_t stream)
{
    const char* who = "ivit_gram_i8_i64";
    IVIT_REQUIRE(x && gram, "%s: NULL operand", who);
    int sp, cps;
    int64_t seg, need;
    int rc = gram_plan(who, rows, C, splits, &sp, &seg, &cps, &need);
    if (rc != IVIT_OK) return rc;
    rc = probe_check_rows(who, x, ldx, C);
    if (rc != IVIT_OK) return rc;
    IVIT_REQUIRE(accumulate == 0 || accumulate == 1, "%s: accumulate=%d is neither 0 nor 1", who, accumulate);
    IVIT_REQUIRE((uintptr_t)gram % 8 == 0, "%s: gram is not aligned to its element", who);
    IVIT_REQUIRE(need == 0 || (workspace && (uintptr_t)workspace % 4 == 0 && workspace_bytes >= need), "%s: workspace of %lld bytes (aligned to 4) needed, %lld given", who,
                 (long long)need, (long long)workspace_bytes);
    GramArgs a;
    a.x = x, a.ldx = ldx, a.rows = rows, a.C = C, a.nb = C / GR_CB, a.seg = seg, a.cps = cps, a.pairs = a.nb * (a.nb + 1) / 2;
    a.ws = static_cast<int32_t*>(workspace);
    const int64_t slabs = (int64_t)sp * cps, grid = slabs * a.pairs;
    IVIT_REQUIRE(grid <= 0x7fffffff, "%s: rows=%lld with %d segments: too many workgroups", who, (long long)rows, sp);
    const hipStream_t st = ivit_stream(stream);
    if (rows == 0 && accumulate) return IVIT_OK;      // a sum over nothing, added
    if (grid > 0) hipLaunchKernelGGL(gram_partial_kernel, dim3((unsigned)grid), dim3(GR_NT), 0, st, a);
    hipLaunchKernelGGL(gram_reduce_kernel, dim3((unsigned)((C * C + GR_NT - 1) / GR_NT)), dim3(GR_NT), 0, st, a.ws, (int)slabs, C * C, accumulate, gram);
    IVIT_CHECK_LAUNCH(who);
}

IVIT_EXPORT int ivit_group_sums_i8_i64(const int8_t* x, int64_t ldx, int64_t rows, int C, const int32_t* perm, const int64_t* group_ptr, int groups,
                                       int accumulate, int64_t* sums, ivit_stream_t stream)
{
    const char* who = "ivit_group_sums_i8_i64";
    IVIT_REQUIRE(x && perm && group_ptr && sums, "%s: NULL operand", who);
    if (const int rc = probe_check_shape(who, rows, C)) return rc;
    if (const int rc = probe_check_rows(who, x, ldx, C)) return rc;
    IVIT_REQUIRE(groups >= 1 && groups <= IVIT_GROUPS_MAX, "%s: groups=%d outside [1, %d]", who, groups, IVIT_GROUPS_MAX);
    IVIT_REQUIRE(accumulate == 0 || accumulate == 1, "%s: accumulate=%d is neither 0 nor 1", who, accumulate);
    IVIT_REQUIRE((uintptr_t)perm % 4 == 0 && ((uintptr_t)group_ptr | (uintptr_t)sums) % 8 == 0, "%s: perm, group_ptr or sums is not aligned to its element", who);
    hipLaunchKernelGGL(group_sums_kernel, dim3((unsigned)groups), dim3(GR_NT), 0, ivit_stream(stream), x, ldx, C, perm, group_ptr, accumulate, sums);
    IVIT_CHECK_LAUNCH(who);
}
