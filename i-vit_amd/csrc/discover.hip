// discover.hip -- unsupervised single-object discovery on the int8 patch tokens of one image (the LOST protocol scored by CorLoc;
// include/ivit_hip.h, "object discovery on int8 patch tokens").  With d(i, j) the int8 dot product of two
// tokens of the same image -- an exact integer on v_mfma_i32_16x16x64_i8, so every step below is one answer whatever the tiling:
//   ivit_token_degrees_i8    deg[i] = #{ j != i : d(i, j) > 0 }: the hot pass, B * hw^2 * C multiply-adds, no [hw, hw] matrix
//   ivit_discover_boxes_i8   the tail: seed, potentials, similars, the map M, its mask, the seed's 4-connected component, the box
//
// token_degrees_kernel.  One workgroup (4 waves) per (query tile of DG_QT = 64 tokens, image).  Wave w = (qh, kh) = (w & 1, w >> 1)
// owns the query half qh -- 32 queries, whose MFMA operands stay in its registers for the whole C (knn_load_queries of knn_parts.h:
// a query beyond hw - 1 reads row hw - 1, a row of the image) -- and the key half kh of every key tile.  The image's tokens are the
// keys: tiles of DG_KT = 64 rows walk through LDS in chunks of DG_KC = 4 K steps (64 rows x 256 bytes), two stages.  While the
// MFMAs of a chunk run, every thread has the four 16-byte pieces of the next chunk in flight from global memory; they go into the
// other stage behind the MFMAs and one barrier ends the step.  A stage row is 256 + 16 bytes long, so the 16 rows a ds_read_b128
// touches start in 16 different 16-byte bank groups.  Keys are shared by the two query halves (each staged byte feeds four
// MFMAs), queries by nobody: LDS traffic is half of the MFMA time.
// Epilogue, once per key tile: acc[sub][qt][r] of lane (g, l15) is d(key 64 t + 32 kh + 16 sub + 4 g + r, query q0 + 16 qt + l15); a
// lane counts acc > 0 with key != query and key < hw (a key row past hw - 1 was read from row hw - 1 and never counts) into one
// register per qt, across all key tiles.  At the end the four lanes (g) that share a query add up by permlane swaps, the kh = 1
// waves hand their sums to the kh = 0 waves through LDS, and every deg[i] is written once.  No atomics.
// Bounds: hw <= 4096 (deg < 4096), C <= 1024 (128 VGPRs of query operands); LDS 2 x 17 KiB; two workgroups per CU.
//
// discover_boxes_kernel.  One workgroup per image:
//   (a) a histogram of deg in LDS, its prefix sums (16 bins per thread, wave scan) give the degree T of the min(k, hw)-th token in
//       the order (deg, index) and the number of tokens below T; one wave then walks the tokens in index order with ballots and
//       lists the potentials: all of deg < T and the first ones of deg == T.  The seed is the minimum of (deg << 12) | index.
//   (b) d(seed, p) per potential, one wave-reduced dot each; similars = the seed and every potential with d > 0
//   (c) the summed similar row in LDS (int32 [C]) and M[j] = dot(sum, t[j]) for every token: lpt = C / 16 rounded up to a power of
//       two lanes per token (16 channels per lane), 64 / lpt tokens per wave pass; M > 0 goes into a byte per token
//   (d) the mask as Gh row words of 64 bits (Gw <= 64), one lane per row; the fill grows the seed's bit by
//       (cur | cur << 1 | cur >> 1 | up | down) & mask until a wave vote sees no change, at most Gh * Gw rounds
//   (e) the box from the OR of the rows and the first and last non-empty row.
// LDS 25 KiB, nothing indexed at run time in registers: no scratch.
#include "knn_parts.h"      // the workgroup's resident query operands: knn_load_queries

namespace {

constexpr int DG_NT = 256;                    // threads per workgroup (four waves)
constexpr int DG_QT = 64;                     // queries per workgroup, 32 per query half
constexpr int DG_KT = 64;                     // keys per tile, 32 per key half
constexpr int DG_KC = 4;                      // K steps (64 bytes each) per staged chunk
constexpr int DG_LD = DG_KC * 64 + 16;        // bytes per staged row
constexpr int DG_GRID_MAX = IVIT_DISCOVER_GRID_MAX;
constexpr int DG_HW_MAX = DG_GRID_MAX * DG_GRID_MAX;      // 4096 tokens: deg < 4096
static_assert(DG_QT == 2 * KN_QT && DG_QT == DG_KT, "a query half is what knn_load_queries loads; query and key tiles are counted alike");

struct DegLds {
    __attribute__((aligned(16))) int8_t stage[2][DG_KT * DG_LD];
    unsigned part[2][KN_QT];      // the counts of the kh = 1 waves
};

template <int KSMAX>
__global__ __launch_bounds__(DG_NT, 2) void token_degrees_kernel(const int8_t* __restrict__ tok, int64_t ld, int64_t img, int hw, int KS, int tiles,
                                                                 int32_t* __restrict__ deg)
{
    __shared__ DegLds S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l15 = lane & 15;
    const int qh = wave & 1, kh = wave >> 1;
    const int b = (int)(blockIdx.x / (unsigned)tiles), qtile = (int)(blockIdx.x % (unsigned)tiles);
    const int8_t* X = tok + (int64_t)b * img;
    const int q0 = qtile * DG_QT + KN_QT * qh;

    v4i qf[2][KSMAX];
    knn_load_queries<KSMAX>(qf, X, ld, hw, KS, q0, g, l15);

    // staging: thread (srow, sc) moves piece sc (16 bytes) of the rows srow + 16 i of a chunk; a piece beyond C is not loaded
    const int srow = tid >> 4, sc = tid & 15;
    v4i st[4] = {v4i{0, 0, 0, 0}, v4i{0, 0, 0, 0}, v4i{0, 0, 0, 0}, v4i{0, 0, 0, 0}};
    auto fetch = [&](int t, int c) {
        if (DG_KC * c + (sc >> 2) < KS) {
#pragma unroll
            for (int i = 0; i < 4; ++i)      // a row past hw - 1 reads row hw - 1: a row of the image
                st[i] = *reinterpret_cast<const v4i*>(X + (int64_t)min(DG_KT * t + srow + 16 * i, hw - 1) * ld + (DG_KC * 64) * c + 16 * sc);
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<v4i*>(S.stage[buf] + (srow + 16 * i) * DG_LD + 16 * sc) = st[i];
    };

    const int nch = (KS + DG_KC - 1) / DG_KC;
    fetch(0, 0);
    stash(0);
    __syncthreads();
    int buf = 0;
    unsigned cnt[2] = {0u, 0u};
    for (int t = 0; t < tiles; ++t) {
        v4i acc[2][2] = {{v4i{0, 0, 0, 0}, v4i{0, 0, 0, 0}}, {v4i{0, 0, 0, 0}, v4i{0, 0, 0, 0}}};      // [sub][qt]
#pragma unroll
        for (int c = 0; c < KSMAX / DG_KC; ++c) {
            if (DG_KC * c < KS) {
                // the next step (the last one asks for the last tile's first chunk again: rows that exist)
                const bool wrap = c + 1 == nch;
                fetch(wrap ? min(t + 1, tiles - 1) : t, wrap ? 0 : c + 1);
                const int8_t* kp = S.stage[buf] + (KN_QT * kh + l15) * DG_LD + 16 * g;
#pragma unroll
                for (int u = 0; u < DG_KC; ++u) {
                    const int ks = DG_KC * c + u;
                    if (ks < KS) {
#pragma unroll
                        for (int sub = 0; sub < 2; ++sub) {
                            const v4i kf = *reinterpret_cast<const v4i*>(kp + sub * 16 * DG_LD + 64 * u);
                            acc[sub][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(kf, qf[0][ks], acc[sub][0], 0, 0, 0);
                            acc[sub][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(kf, qf[1][ks], acc[sub][1], 0, 0, 0);
                        }
                    }
                }
                stash(buf ^ 1);      // last read in the step before this one, which a barrier ended
                __syncthreads();
                buf ^= 1;
            }
        }
        const int jbase = DG_KT * t + KN_QT * kh + 4 * g;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int qt = 0; qt < 2; ++qt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = jbase + 16 * sub + r, i = q0 + 16 * qt + l15;
                    cnt[qt] += (acc[sub][qt][r] > 0 && j != i && j < hw) ? 1u : 0u;
                }
    }
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        cnt[qt] = rows_allsum_u32(cnt[qt]);      // the four lanes (g) of a query
        if (kh == 1 && g == 0) S.part[qh][16 * qt + l15] = cnt[qt];
    }
    __syncthreads();
    if (kh == 0 && g == 0) {
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            const int i = q0 + 16 * qt + l15;
            if (i < hw) deg[(int64_t)b * hw + i] = (int32_t)(cnt[qt] + S.part[qh][16 * qt + l15]);
        }
    }
}

// ---- the tail ---------------------------------------------------------------------------------------------------------------------
struct BoxArgs {
    const int8_t* tok;
    int64_t ld, img;
    int Gh, Gw, C, k;
    const int32_t* deg;
    int32_t *boxes, *seed;
    u64* rows;
};

struct BoxLds {
    __attribute__((aligned(16))) int hist[DG_HW_MAX];      // tokens per degree
    int sum[1024];                                         // the summed similar row
    unsigned char mk[DG_HW_MAX];                           // M[j] > 0
    int pot[IVIT_DISCOVER_K_MAX], sim[IVIT_DISCOVER_K_MAX];
    int wtot[4], wmin[4], T, less;
};

// 16 int8 channels against 16 int8 channels / 16 int32 values
IVIT_DEV int dot16_i8(v4i a, v4i b)
{
    int s = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
        for (int q = 0; q < 4; ++q) s += (int)(int8_t)(a[w] >> (8 * q)) * (int)(int8_t)(b[w] >> (8 * q));
    return s;
}

IVIT_DEV int token_degree(const int32_t* deg, int i) { return (int)min((unsigned)deg[i], (unsigned)(DG_HW_MAX - 1)); }      // a histogram bin, whatever the buffer holds

__global__ __launch_bounds__(DG_NT) void discover_boxes_kernel(BoxArgs a)
{
    __shared__ BoxLds S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x, Gh = a.Gh, Gw = a.Gw, hw = Gh * Gw, C = a.C, kk = min(a.k, hw), np = C >> 4;      // np: 16-byte pieces per row
    const int8_t* X = a.tok + (int64_t)b * a.img;
    const int32_t* deg = a.deg + (int64_t)b * hw;

    // (a) histogram, seed, the degree T of the kk-th token
    for (int i = tid; i < DG_HW_MAX; i += DG_NT) S.hist[i] = 0;
    __syncthreads();
    int best = 0x7fffffff;
    for (int i = tid; i < hw; i += DG_NT) {
        const int d = token_degree(deg, i);
        atomicAdd(&S.hist[d], 1);      // LDS, integers: any order, one histogram
        best = min(best, (d << 12) | i);
    }
    best = -wave_allmax_i32(-best);
    if (lane == 0) S.wmin[wave] = best;
    __syncthreads();
    int h[16], s = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const v4i v = *reinterpret_cast<const v4i*>(&S.hist[16 * tid + 4 * u]);
#pragma unroll
        for (int q = 0; q < 4; ++q) h[4 * u + q] = v[q], s += v[q];
    }
    int inc = s;
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o);
        if (lane >= o) inc += v;
    }
    if (lane == 63) S.wtot[wave] = inc;
    __syncthreads();
    for (int w = 0; w < wave; ++w) inc += S.wtot[w];
    if (inc - s < kk && kk <= inc) {      // one thread: 1 <= kk <= hw = the sum of all bins
        int c = inc - s;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            if (c < kk && kk <= c + h[u]) S.T = 16 * tid + u, S.less = c;
            c += h[u];
        }
    }
    __syncthreads();
    const int seed = min(min(S.wmin[0], S.wmin[1]), min(S.wmin[2], S.wmin[3])) & (DG_HW_MAX - 1);
    if (wave == 0) {      // the potentials in index order: every token below T, the first kk - less of degree T
        const int T = S.T, need_eq = kk - S.less;
        const u64 below = (1ull << lane) - 1;
        int base = 0, eqbase = 0;
        for (int i0 = 0; i0 < hw && base < kk; i0 += 64) {
            const int i = i0 + lane, d = i < hw ? token_degree(deg, i) : DG_HW_MAX;
            const u64 eqm = __builtin_amdgcn_ballot_w64(d == T);
            const bool sel = d < T || (d == T && eqbase + __builtin_popcountll(eqm & below) < need_eq);
            const u64 sm = __builtin_amdgcn_ballot_w64(sel);
            if (sel) S.pot[base + __builtin_popcountll(sm & below)] = i;      // < kk: less + need_eq tokens are selected in all
            base += __builtin_popcountll(sm);
            eqbase += __builtin_popcountll(eqm);
        }
    }
    __syncthreads();

    // (b) similars: the seed, and every potential p with d(seed, p) > 0 (|d| <= 1024 * 127^2 < 2^24)
    const v4i zero = v4i{0, 0, 0, 0};
    const v4i sd = lane < np ? *reinterpret_cast<const v4i*>(X + (int64_t)seed * a.ld + 16 * lane) : zero;
    for (int p = wave; p < kk; p += 4) {
        const int row = S.pot[p];
        const v4i v = lane < np ? *reinterpret_cast<const v4i*>(X + (int64_t)row * a.ld + 16 * lane) : zero;
        const int d = wave_reduce_sum_i32(dot16_i8(sd, v));
        if (lane == 0) S.sim[p] = (row == seed || d > 0) ? 1 : 0;
    }
    __syncthreads();

    // (c) the summed similar row, four channels per thread: at most 128 rows, |sum| <= 128 * 127
    if (4 * tid < C) {
        int s4[4] = {0, 0, 0, 0};
        for (int p = 0; p < kk; ++p) {
            if (S.sim[p]) {
                const int w = *reinterpret_cast<const int*>(X + (int64_t)S.pot[p] * a.ld + 4 * tid);
#pragma unroll
                for (int q = 0; q < 4; ++q) s4[q] += (int)(int8_t)(w >> (8 * q));
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) S.sum[4 * tid + q] = s4[q];
    }
    __syncthreads();
    {
        int lpt = 4;                        // lanes per token: np = C / 16 (4 .. 64) rounded up to a power of two
        while (lpt < np) lpt <<= 1;
        const int tpp = 64 / lpt, piece = lane & (lpt - 1), sub = lane / lpt;
        int sv[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) sv[u] = piece < np ? S.sum[16 * piece + u] : 0;
        for (int j0 = wave * tpp; j0 < hw; j0 += 4 * tpp) {      // (uniform trip count in a wave: the shuffles want every lane)
            const int j = j0 + sub;
            const v4i v = (j < hw && piece < np) ? *reinterpret_cast<const v4i*>(X + (int64_t)j * a.ld + 16 * piece) : zero;
            // M[j] in int32: |M| <= 127^2 * 1024 * 128 = 2 114 060 288 < 2^31 (at most 128 similars, C <= 1024); every partial sum is
            // a sum of a subset of its terms' magnitudes at most, so no step overflows either
            int m = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w)
#pragma unroll
                for (int q = 0; q < 4; ++q) m += sv[4 * w + q] * (int)(int8_t)(v[w] >> (8 * q));
            for (int o = 1; o < lpt; o <<= 1) m += __shfl_xor(m, o);
            if (piece == 0 && j < hw) S.mk[j] = m > 0 ? 1 : 0;
        }
    }
    __syncthreads();

    // (d) the mask's row words, one lane per row, and the fill from the seed's bit; (e) the box
    if (wave == 0) {
        u64 word = 0;
        if (lane < Gh)
            for (int x = 0; x < Gw; ++x) word |= (u64)S.mk[lane * Gw + x] << x;
        const int sy = seed / Gw, sx = seed - sy * Gw;
        u64 cur = lane == sy ? 1ull << sx : 0;
        // a seed outside the mask (an all-zero row, M == 0 everywhere): its cell alone, no fill
        const bool inside = __builtin_amdgcn_ballot_w64(lane == sy && ((word >> sx) & 1)) != 0;
        for (int round = 0; inside && round < hw; ++round) {      // a round adds a cell or ends the fill: at most Gh * Gw rounds
            const u64 up = __shfl_up(cur, 1), down = __shfl_down(cur, 1);      // (lanes 0 and 63 get their own word back: no change)
            const u64 grow = (cur | (cur << 1) | (cur >> 1) | up | down) & word;
            const bool changed = (grow | cur) != cur;
            cur |= grow;
            if (__builtin_amdgcn_ballot_w64(changed) == 0) break;
        }
        u64 orw = cur;
        for (int o = 1; o < 64; o <<= 1) orw |= __shfl_xor(orw, o);
        const u64 nz = __builtin_amdgcn_ballot_w64(cur != 0);      // never 0: the seed's bit
        if (lane == 0) {
            int32_t* box = a.boxes + 4 * (int64_t)b;
            box[0] = __builtin_ctzll(orw), box[1] = __builtin_ctzll(nz), box[2] = 63 - __builtin_clzll(orw), box[3] = 63 - __builtin_clzll(nz);
            a.seed[b] = seed;
        }
        if (a.rows && lane < Gh) a.rows[(int64_t)b * Gh + lane] = cur;
    }
}

int discover_check(const char* who, const int8_t* tokens, int64_t ld, int64_t image_stride, int B, int Gh, int Gw, int C)
{
    IVIT_REQUIRE(tokens, "%s: NULL operand", who);
    IVIT_REQUIRE(B >= 1 && Gh >= 1 && Gw >= 1, "%s: B=%d, Gh=%d and Gw=%d must be at least 1", who, B, Gh, Gw);
    if (Gh > DG_GRID_MAX || Gw > DG_GRID_MAX) {
        ivit_set_error("%s: unsupported geometry (grid %d x %d above %d x %d)", who, Gh, Gw, DG_GRID_MAX, DG_GRID_MAX);
        return IVIT_ERR_UNSUPPORTED;
    }
    if (C < 64 || C > 1024 || C % 64 != 0) {
        ivit_set_error("%s: unsupported geometry (C=%d: multiples of 64 from 64 to 1024)", who, C);
        return IVIT_ERR_UNSUPPORTED;
    }
    IVIT_REQUIRE(ld >= C && image_stride >= 0, "%s: ld=%lld below C=%d or image_stride=%lld below 0", who, (long long)ld, C, (long long)image_stride);
    IVIT_REQUIRE(((uintptr_t)tokens | (uintptr_t)ld | (uintptr_t)image_stride) % 16 == 0,
                 "%s: tokens, ld=%lld and image_stride=%lld must be multiples of 16 bytes", who, (long long)ld, (long long)image_stride);
    return IVIT_OK;
}

}      // namespace

IVIT_EXPORT int ivit_token_degrees_i8(const int8_t* tokens, int64_t ld, int64_t image_stride, int B, int Gh, int Gw, int C, int32_t* deg,
                                      ivit_stream_t stream)
{
    const char* who = "ivit_token_degrees_i8";
    const int rc = discover_check(who, tokens, ld, image_stride, B, Gh, Gw, C);
    if (rc != IVIT_OK) return rc;
    IVIT_REQUIRE(deg && (uintptr_t)deg % 4 == 0, "%s: deg is NULL or not aligned to its element", who);
    const int hw = Gh * Gw, KS = C / 64, tiles = (hw + DG_QT - 1) / DG_QT;
    IVIT_REQUIRE((int64_t)B * tiles <= 0x7fffffff, "%s: B=%d images of %d tokens: too many workgroups", who, B, hw);
    const dim3 gd((unsigned)((int64_t)B * tiles)), bd(DG_NT);
    const hipStream_t st = ivit_stream(stream);
    if (KS <= 4) hipLaunchKernelGGL(token_degrees_kernel<4>, gd, bd, 0, st, tokens, ld, image_stride, hw, KS, tiles, deg);
    else if (KS <= 8) hipLaunchKernelGGL(token_degrees_kernel<8>, gd, bd, 0, st, tokens, ld, image_stride, hw, KS, tiles, deg);
    else hipLaunchKernelGGL(token_degrees_kernel<16>, gd, bd, 0, st, tokens, ld, image_stride, hw, KS, tiles, deg);
    IVIT_CHECK_LAUNCH(who);
}

IVIT_EXPORT int ivit_discover_boxes_i8(const int8_t* tokens, int64_t ld, int64_t image_stride, int B, int Gh, int Gw, int C, const int32_t* deg,
                                       int k, int32_t* boxes, int32_t* seed, uint64_t* rows, ivit_stream_t stream)
{
    const char* who = "ivit_discover_boxes_i8";
    const int rc = discover_check(who, tokens, ld, image_stride, B, Gh, Gw, C);
    if (rc != IVIT_OK) return rc;
    IVIT_REQUIRE(deg && boxes && seed, "%s: NULL operand", who);
    IVIT_REQUIRE(k >= 1 && k <= IVIT_DISCOVER_K_MAX, "%s: k=%d outside [1, %d]", who, k, IVIT_DISCOVER_K_MAX);
    IVIT_REQUIRE(((uintptr_t)deg | (uintptr_t)boxes | (uintptr_t)seed) % 4 == 0 && (uintptr_t)rows % 8 == 0,
                 "%s: deg, boxes, seed or rows is not aligned to its element", who);
    BoxArgs a;
    a.tok = tokens, a.ld = ld, a.img = image_stride, a.Gh = Gh, a.Gw = Gw, a.C = C, a.k = k, a.deg = deg, a.boxes = boxes, a.seed = seed;
    a.rows = reinterpret_cast<u64*>(rows);
    hipLaunchKernelGGL(discover_boxes_kernel, dim3((unsigned)B), dim3(DG_NT), 0, ivit_stream(stream), a);
    IVIT_CHECK_LAUNCH(who);
}
