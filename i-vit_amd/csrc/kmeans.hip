// kmeans.hip -- Lloyd's iteration on the int8 feature bank with fixed-point centroids (include/ivit_hip.h, "k-means on the int8
// feature bank").  A centroid is an int16 vector c16 with 7 fractional bits, kept as two dense int8 planes
// hi = c16 >> 7 and lo = c16 & 127, so both halves of dot(x, c16) = 128 dot(x, hi) + dot(x, lo) are exact int32 sums on
// v_mfma_i32_16x16x64_i8 and every step is one answer whatever the tiling:
//   ivit_kmeans_assign_i8     label[r] = the k of smallest D(r, k) = cnorm[k] - 256 dot(x_r, c16_k), equal D to the lower k, and
//                             dist[r] = |128 x_r - c16_label|^2: the hot pass, rows * K * C * 2 multiply-adds, no [rows][K] matrix
//   ivit_kmeans_update_i16    c16[k] = 128 * the mean of the rows labelled k, rounded half up, from their int64 sums and count
// (the sums between the two are ivit_group_sums_i8_i64 of probe.hip on the CSR form of the labels).
//
// kmeans_assign_kernel.  The roles of the search kernel reversed: the many bank rows are resident, the few centroids stream.  One
// workgroup (4 waves) per tile of KM_RT = 128 bank rows; wave w owns rows 32 w .. 32 w + 31, whose MFMA operands stay in its
// registers for the whole pass (128 VGPRs at C = 1024): every bank row is read from HBM exactly once, and |x_r|^2 for dist comes from
// the same registers.  The centroids walk through LDS in tiles of KT = 64 and, inside a tile, in channel chunks of KC = 2 K steps:
// a stage holds 64 rows x 128 bytes of both planes (18 KiB), two stages.  While the MFMAs of a chunk run every thread has the
// four 16-byte pieces of the next chunk in flight from L2; they go into the other stage behind the MFMAs and one barrier ends the
// step.  One L2 read of a centroid byte serves all 128 rows of the tile; a ds_read_b128 feeds two MFMAs (the wave's two row
// sub-tiles).  A staged row is 64 KC + 16 bytes, so the 16 rows a ds_read_b128 touches start in 16 different 16-byte bank groups.
// The accumulators of a tile -- [plane][16 centroids x 4][16 rows x 2], 64 VGPRs -- live across the chunks.  Above C = 512, where
// the row operands take up to 128 VGPRs, that does not fit 256 registers: the form for those widths has KT = 32 (32 accumulator
// registers) and KC = 4 (32 rows x 256 bytes of both planes, 17 KiB a stage; as many MFMAs per barrier as the other form).
// Epilogue, once per centroid tile: acc[p][sub][qt][i] of lane (g, l15) belongs to centroid KT t + 16 sub + 4 g + i and row
// 16 qt + l15.  With the tile the workgroup stages cn[k] = ((cnorm[k] + 2^41) << 16) | k (2^62 for k >= K: the mask), so
//   key = cn[k] - dot_hi * 2^31 - dot_lo * 2^24 = ((D + 2^41) << 16) | k      in 64-bit arithmetic (dot_hi * 2^31 reaches 2^55)
// is positive, below 2^58 and ordered as (D, k): one 64-bit minimum per value keeps the running best, the lower k winning a tie.
// At the end the four lanes (g) that share a row fold their minima by permlane swaps and every row is written once.
// No atomics, no float.  LDS 37.5 KiB; two workgroups (8 waves) per CU.
#include "common.h"

namespace {

typedef unsigned long long u64;

constexpr int KM_NT = 256;                    // threads per workgroup (four waves)
constexpr int KM_WR = 32;                     // bank rows per wave
constexpr int KM_RT = 4 * KM_WR;              // bank rows per workgroup
constexpr int KM_STAGE = 18432;                // bytes per stage: the larger of the two forms below
constexpr u64 KM_BIAS = 1ull << 41;           // D + KM_BIAS > 0: |D| < 2^40
constexpr u64 KM_MASKED = 1ull << 62;         // the cn of a centroid index >= K: above every key of a centroid that exists

struct KmLds {
    __attribute__((aligned(16))) int8_t stage[2][KM_STAGE];      // [stage][plane * KT + centroid][LD]
    u64 cn[3][64];      // per tile, a ring of three: tile t + 2 is staged while a slow wave may still fold tile t
};

// the sum of the squares of 16 int8 channels
IVIT_DEV unsigned sq16_i8(v4i a)
{
    unsigned s = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int v = (int)(int8_t)(a[w] >> (8 * q));
            s += (unsigned)(v * v);
        }
    return s;
}

// the minimum over the four lanes l, l ^ 16, l ^ 32, l ^ 48 (both halves move with the same swap)
IVIT_DEV u64 rows_allmin_u64(u64 v)
{
    typedef unsigned v2u_ __attribute__((ext_vector_type(2)));
    const v2u_ al = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
    const v2u_ ah = __builtin_amdgcn_permlane16_swap((unsigned)(v >> 32), (unsigned)(v >> 32), false, false);
    u64 a = ((u64)ah.x << 32) | al.x, b = ((u64)ah.y << 32) | al.y;
    v = a < b ? a : b;
    const v2u_ bl = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
    const v2u_ bh = __builtin_amdgcn_permlane32_swap((unsigned)(v >> 32), (unsigned)(v >> 32), false, false);
    a = ((u64)bh.x << 32) | bl.x, b = ((u64)bh.y << 32) | bl.y;
    return a < b ? a : b;
}

// SUB: 16-centroid sub-tiles per tile (KT = 16 SUB centroids), KC: K steps (64 bytes each) per staged chunk
template <int KSMAX, int SUB, int KC>
__global__ __launch_bounds__(KM_NT, 2) void kmeans_assign_kernel(const int8_t* __restrict__ x, int64_t ldx, int64_t rows, int KS,
                                                                 const int8_t* __restrict__ hi, const int8_t* __restrict__ lo,
                                                                 const int64_t* __restrict__ cnorm, int K, int tiles, int32_t* __restrict__ label,
                                                                 int64_t* __restrict__ dist)
{
    constexpr int KT = 16 * SUB, LD = KC * 64 + 16, PPR = 4 * KC, RPP = KM_NT / PPR;      // pieces per staged row, rows per pass
    static_assert(2 * KT * LD <= KM_STAGE && 2 * RPP == KT && KT <= 64, "a thread stages two centroids per plane");
    __shared__ KmLds S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l15 = lane & 15;
    const int C = 64 * KS;
    const int64_t r0 = (int64_t)blockIdx.x * KM_RT + KM_WR * wave;

    // the wave's 32 rows as MFMA operands (a row beyond rows - 1 reads row rows - 1: a row that exists) and their squared norms
    v4i xf[2][KSMAX];
    unsigned xsq[2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const int64_t r = r0 + 16 * qt + l15;
        const int8_t* xp = x + (r < rows ? r : rows - 1) * ldx + 16 * g;
        unsigned s = 0;
#pragma unroll
        for (int ks = 0; ks < KSMAX; ++ks) {
            xf[qt][ks] = v4i{0, 0, 0, 0};
            if (ks < KS) {
                xf[qt][ks] = *reinterpret_cast<const v4i*>(xp + 64 * ks);
                s += sq16_i8(xf[qt][ks]);
            }
        }
        xsq[qt] = rows_allsum_u32(s);      // the four lanes (g) of a row: at most 1024 * 2^14 = 2^24
    }

    // staging: thread (srow, sc) moves piece sc (16 bytes) of the centroids srow and srow + RPP of a chunk, in both planes; a piece
    // beyond C is not loaded; a centroid past K - 1 reads centroid K - 1 (its cn is the mask)
    const int srow = tid / PPR, sc = tid % PPR;
    v4i st[4] = {v4i{0, 0, 0, 0}, v4i{0, 0, 0, 0}, v4i{0, 0, 0, 0}, v4i{0, 0, 0, 0}};
    u64 cnv = KM_MASKED;
    auto fetch = [&](int t, int c) {
        if (KC * c + (sc >> 2) < KS) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int64_t off = (int64_t)min(KT * t + srow + RPP * i, K - 1) * C + (KC * 64) * c + 16 * sc;
                st[i] = *reinterpret_cast<const v4i*>(hi + off);
                st[2 + i] = *reinterpret_cast<const v4i*>(lo + off);
            }
        }
        if (c == 0 && tid < KT) {
            const int k = KT * t + tid;
            cnv = k < K ? ((((u64)cnorm[k] + KM_BIAS) << 16) | (u64)k) : KM_MASKED;
        }
    };
    auto stash = [&](int buf, int slot, int c) {
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<v4i*>(S.stage[buf] + ((i >> 1) * KT + srow + RPP * (i & 1)) * LD + 16 * sc) = st[i];
        if (c == 0 && tid < KT) S.cn[slot][tid] = cnv;
    };

    const int nch = (KS + KC - 1) / KC;
    fetch(0, 0);
    stash(0, 0, 0);
    __syncthreads();
    int buf = 0, slot = 0;
    u64 best[2] = {~0ull, ~0ull};
    for (int t = 0; t < tiles; ++t) {
        const int next_slot = slot == 2 ? 0 : slot + 1;
        v4i acc[2][SUB][2];      // [plane][sub][qt]
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int sub = 0; sub < SUB; ++sub) acc[p][sub][0] = acc[p][sub][1] = v4i{0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < KSMAX / KC; ++c) {
            if (KC * c < KS) {
                // the next step (the last one asks for the last tile's first chunk again: centroids that exist)
                const bool wrap = c + 1 == nch;
                const int cnext = wrap ? 0 : c + 1;
                fetch(wrap ? min(t + 1, tiles - 1) : t, cnext);
                const int8_t* kp = S.stage[buf] + l15 * LD + 16 * g;
#pragma unroll
                for (int u = 0; u < KC; ++u) {
                    const int ks = KC * c + u;
                    if (ks < KS) {
#pragma unroll
                        for (int p = 0; p < 2; ++p)
#pragma unroll
                            for (int sub = 0; sub < SUB; ++sub) {
                                const v4i kf = *reinterpret_cast<const v4i*>(kp + (p * KT + 16 * sub) * LD + 64 * u);
                                acc[p][sub][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(kf, xf[0][ks], acc[p][sub][0], 0, 0, 0);
                                acc[p][sub][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(kf, xf[1][ks], acc[p][sub][1], 0, 0, 0);
                            }
                    }
                }
                stash(buf ^ 1, next_slot, cnext);      // last read in the step before this one, which a barrier ended
                __syncthreads();
                buf ^= 1;
            }
        }
        const u64* cnp = S.cn[slot] + 4 * g;
#pragma unroll
        for (int sub = 0; sub < SUB; ++sub)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const u64 cnk = cnp[16 * sub + i];
#pragma unroll
                for (int qt = 0; qt < 2; ++qt) {
                    const u64 key = cnk - ((u64)(long long)acc[0][sub][qt][i] << 31) - ((u64)(long long)acc[1][sub][qt][i] << 24);
                    best[qt] = key < best[qt] ? key : best[qt];
                }
            }
        slot = next_slot;
    }
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const u64 b = rows_allmin_u64(best[qt]);
        const int64_t r = r0 + 16 * qt + l15;
        if (g == 0 && r < rows) {
            label[r] = (int32_t)(b & 0xffffu);
            dist[r] = (int64_t)(b >> 16) - (int64_t)KM_BIAS + 16384ll * (int64_t)xsq[qt];
        }
    }
}

// one wave per centroid: lane l owns the channels l, l + 64, ...
__global__ __launch_bounds__(KM_NT) void kmeans_update_kernel(const int64_t* __restrict__ sums, const int64_t* __restrict__ counts, int K, int C,
                                                              int8_t* __restrict__ hi, int8_t* __restrict__ lo, int64_t* __restrict__ cnorm,
                                                              int32_t* __restrict__ changed)
{
    const int lane = threadIdx.x & 63, k = (int)blockIdx.x * (KM_NT / 64) + (int)(threadIdx.x >> 6);
    if (k >= K) return;
    const int64_t n = counts[k];
    if (n <= 0) {      // an empty cluster keeps its centroid (and its cnorm)
        if (lane == 0) changed[k] = 0;
        return;
    }
    u64 sq = 0;
    bool moved = false;
    for (int c = lane; c < C; c += 64) {
        const int64_t at = (int64_t)k * C + c;
        const int64_t num = 256 * sums[at] + n, den = 2 * n;      // |sums| <= 128 n: |num| < 2^47
        int64_t q = num / den;
        if (num % den < 0) --q;                                   // floor towards -inf
        q = q < -16384 ? -16384 : q > 16383 ? 16383 : q;          // (the mean of int8 values lies inside: whatever sums holds)
        const int8_t h = (int8_t)(q >> 7), l = (int8_t)(q & 127);
        moved = moved || h != hi[at] || l != lo[at];
        hi[at] = h;
        lo[at] = l;
        sq += (u64)(q * q);
    }
    sq = lanes_allsum_u64<64>(sq);
    const bool any = __builtin_amdgcn_ballot_w64(moved) != 0;
    if (lane == 0) {
        cnorm[k] = (int64_t)sq;
        changed[k] = any ? 1 : 0;
    }
}

int kmeans_geometry(const char* who, int K, int C)
{
    IVIT_REQUIRE(K >= 1 && K <= IVIT_KMEANS_K_MAX, "%s: K=%d outside [1, %d]", who, K, IVIT_KMEANS_K_MAX);
    if (C < 64 || C > 1024 || C % 64 != 0) {
        ivit_set_error("%s: unsupported geometry (C=%d: multiples of 64 from 64 to 1024)", who, C);
        return IVIT_ERR_UNSUPPORTED;
    }
    return IVIT_OK;
}

}      // namespace

IVIT_EXPORT int ivit_kmeans_assign_i8(const int8_t* x, int64_t ldx, int64_t rows, int C, const int8_t* hi, const int8_t* lo, const int64_t* cnorm,
                                      int K, int32_t* label, int64_t* dist, ivit_stream_t stream)
{
    const char* who = "ivit_kmeans_assign_i8";
    IVIT_REQUIRE(x && hi && lo && cnorm && label && dist, "%s: NULL operand", who);
    IVIT_REQUIRE(rows >= 0 && rows < (1ll << 31), "%s: rows=%lld outside [0, 2^31)", who, (long long)rows);
    const int rc = kmeans_geometry(who, K, C);
    if (rc != IVIT_OK) return rc;
    IVIT_REQUIRE(ldx >= C, "%s: ldx=%lld below C=%d", who, (long long)ldx, C);
    IVIT_REQUIRE(((uintptr_t)x | (uintptr_t)ldx | (uintptr_t)hi | (uintptr_t)lo) % 16 == 0,
                 "%s: x, ldx=%lld, hi and lo must be multiples of 16 bytes", who, (long long)ldx);
    IVIT_REQUIRE(((uintptr_t)cnorm | (uintptr_t)dist) % 8 == 0 && (uintptr_t)label % 4 == 0, "%s: cnorm, dist or label is not aligned to its element", who);
    if (rows == 0) return IVIT_OK;
    const int KS = C / 64;
    const dim3 gd((unsigned)((rows + KM_RT - 1) / KM_RT)), bd(KM_NT);
    const hipStream_t st = ivit_stream(stream);
    // C <= 512: tiles of 64 centroids in chunks of two K steps; above, where the row operands take up to 128 VGPRs, tiles of 32
    // centroids (half the accumulators) in chunks of four
    if (KS <= 4) hipLaunchKernelGGL((kmeans_assign_kernel<4, 4, 2>), gd, bd, 0, st, x, ldx, rows, KS, hi, lo, cnorm, K, (K + 63) / 64, label, dist);
    else if (KS <= 8) hipLaunchKernelGGL((kmeans_assign_kernel<8, 4, 2>), gd, bd, 0, st, x, ldx, rows, KS, hi, lo, cnorm, K, (K + 63) / 64, label, dist);
    else hipLaunchKernelGGL((kmeans_assign_kernel<16, 2, 4>), gd, bd, 0, st, x, ldx, rows, KS, hi, lo, cnorm, K, (K + 31) / 32, label, dist);
    IVIT_CHECK_LAUNCH(who);
}

IVIT_EXPORT int ivit_kmeans_update_i16(const int64_t* sums, const int64_t* counts, int K, int C, int8_t* hi, int8_t* lo, int64_t* cnorm,
                                       int32_t* changed, ivit_stream_t stream)
{
    const char* who = "ivit_kmeans_update_i16";
    IVIT_REQUIRE(sums && counts && hi && lo && cnorm && changed, "%s: NULL operand", who);
    const int rc = kmeans_geometry(who, K, C);
    if (rc != IVIT_OK) return rc;
    IVIT_REQUIRE(((uintptr_t)sums | (uintptr_t)counts | (uintptr_t)cnorm) % 8 == 0 && (uintptr_t)changed % 4 == 0,
                 "%s: sums, counts, cnorm or changed is not aligned to its element", who);
    hipLaunchKernelGGL(kmeans_update_kernel, dim3((unsigned)((K + KM_NT / 64 - 1) / (KM_NT / 64))), dim3(KM_NT), 0, ivit_stream(stream), sums, counts,
                       K, C, hi, lo, cnorm, changed);
    IVIT_CHECK_LAUNCH(who);
}
