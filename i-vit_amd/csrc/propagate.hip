// propagate.hip -- label propagation between the patch tokens of video frames (the DAVIS protocol of the DINO evaluation suite) on
// the int8 path: every target token looks at the context tokens of F frames inside a spatial window around its own position.
//   ivit_local_topk_i8          per target the k context tokens of largest score inside its window, in the search's order
//   ivit_propagate_labels_f32   the weighted mix of the soft labels of a target's k neighbours
//
// The windowed search.  Score, key and order are the search's (knn.hip, "Order"): score = fl32((float)dot * rnorm[row]), one 64-bit
// key per (score, bank row), larger for the better neighbour; keys are unique, so "the k largest keys of the window" is one answer
// whatever the tiling or the number of frame segments.  What differs is the candidate set: a window per target, not the whole bank.
// Work split.  A workgroup (4 waves) owns a SPATIAL tile of 32 targets, LP_TH x LP_TW = 4 rows x 8 columns of the token grid, so that
// their windows overlap: the union of the 32 windows is (4 + 2R) x (8 + 2R) positions (clipped to the grid) against 32 x (1 + 2R)^2
// for 32 unrelated targets.  Every wave holds the fragments of all 32 targets in registers for the whole pass (knn.hip); a target
// beyond the grid's right or bottom edge reads the clamped position -- a row that exists -- and is masked in the epilogue.
// Streaming.  The union window is walked frame after frame in steps of KN_BT = 64 positions (row-major inside the window, the last
// step of a frame padded with the window's last position), 16 per wave, from global memory straight into MFMA operand registers;
// the next step's loads are issued right behind the MFMAs that consumed the current one.  The bank row of a position comes from the
// window geometry (one integer division per lane for the loads, one for the four rows of its epilogue), not from a running row.
// Epilogue.  acc[qt][r] of lane (g, l15) is dot(position 16 wave + 4 g + r of the step, target 16 qt + l15).  A pair passes when the
// position is no padding, the target is inside the grid, |dy| <= R and |dx| <= R, and the key beats the target's threshold (the
// smallest key of its full list; 0 while the list fills).  Passing keys go into the step's candidate buffer in LDS (whole keys: the
// rows of a step are not consecutive); behind a barrier wave w inserts those of the targets t % 4 == w into their lists (knn_insert
// of knn_parts.h, lists of IVIT_LOCAL_K_MAX = 32 keys).  At the end every list is ranked and written in order.
// Segments.  A small grid has few tiles (24 x 40: 30), so the launcher cuts the FRAMES into `splits` segments, one workgroup per (tile,
// segment); the lists go to the workspace [T][splits][k] as keys (0 = no entry), the layout of the search, and knn_merge_kernel
// ranks them across segments.
// LDS: 8 KiB lists + 16 KiB candidate keys + 2 KiB candidate targets + thresholds = 26.7 KiB; registers as the search kernel (up to
// 192 VGPRs at C = 1024): two workgroups per CU.
#define KNN_PARTS_MERGE      // knn_merge_kernel
#include "knn_parts.h"

namespace {

constexpr int LP_KCAP = IVIT_LOCAL_K_MAX;      // list capacity
constexpr int LP_TH = 4, LP_TW = 8;            // the tile of targets: LP_TH * LP_TW == KN_QT
static_assert(LP_TH * LP_TW == KN_QT && LP_TW == 8, "target 16 qt + l15 of a tile is (2 qt + (l15 >> 3), l15 & 7)");

struct LocalArgs {
    const int8_t* q;
    int64_t ldq;
    int Gh, Gw;
    const int8_t* bank;
    int64_t ldb;
    int F, KS;                // KS = C / 64
    const float* rnorm;
    int radius, k, splits, fps;      // radius: clamped to max(Gh, Gw); fps: frames per segment
    int32_t* idx;
    float* score;
    u64* ws;
    int tiles_x, tiles;
};

struct LocalSel {
    __attribute__((aligned(16))) u64 lists[KN_QT * LP_KCAP];
    u64 thr[KN_QT];
    u64 ckey[KN_CAND];                  // the candidates of a step: key and target in tile
    unsigned char cq[KN_CAND];
    int cntl[KN_QT], minpos[KN_QT], cnt[2];
};

// behind the barrier that ends the epilogues: wave w inserts the candidates of the targets t % 4 == w
IVIT_DEV void local_drain(LocalSel& S, int cs, int k, int tid, int lane, int wave)
{
    const int n = S.cnt[cs];
    if (tid == 0) S.cnt[cs ^ 1] = 0;      // next step's counter: last read before the barrier that ended the previous step's epilogues
    for (int e0 = 0; e0 < n; e0 += 64) {
        const int e = e0 + lane;
        u64 key = 0;
        int ql = 0;
        bool mine = false;
        if (e < n) {
            key = S.ckey[e];
            ql = S.cq[e];
            mine = (ql & 3) == wave;
        }
        u64 mask = __builtin_amdgcn_ballot_w64(mine);
        while (mask) {
            const int src = __builtin_ctzll(mask);
            mask &= mask - 1;
            const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)key, src), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(key >> 32), src);
            knn_insert<LP_KCAP>(S.lists, S.thr, S.cntl, S.minpos, __builtin_amdgcn_readlane(ql, src), ((u64)hi << 32) | lo, k, lane);
        }
    }
}

template <int KSMAX>
__global__ __launch_bounds__(KN_NT, 2) void local_topk_kernel(LocalArgs a)
{
    __shared__ LocalSel S;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l15 = lane & 15;
    // consecutive workgroups: the tiles of one frame segment
    const int tile = (int)(blockIdx.x % (unsigned)a.tiles), s = (int)(blockIdx.x / (unsigned)a.tiles);
    const int ty0 = (tile / a.tiles_x) * LP_TH, tx0 = (tile % a.tiles_x) * LP_TW;
    const int R = a.radius, KS = a.KS, k = a.k, Gw = a.Gw, GG = a.Gh * a.Gw;
    // the union of the tile's windows, clipped to the grid (64-bit: R may be as large as the grid)
    const int y0 = max(ty0 - R, 0), x0 = max(tx0 - R, 0);
    const int y1 = (int)min((int64_t)ty0 + (LP_TH - 1) + R, (int64_t)a.Gh - 1), x1 = (int)min((int64_t)tx0 + (LP_TW - 1) + R, (int64_t)Gw - 1);
    const int ww = x1 - x0 + 1, wn = (y1 - y0 + 1) * ww;      // positions per frame: at most Gh * Gw
    const int tpf = (int)(((unsigned)wn + KN_BT - 1) / KN_BT);      // steps per frame
    const int f0 = min(s * a.fps, a.F), f1 = min(f0 + a.fps, a.F);
    const int ntiles = (f1 - f0) * tpf;

    if (tid < KN_QT) {
        S.thr[tid] = 0;
        S.cntl[tid] = 0;
        S.minpos[tid] = 0;
    }
    if (tid < 2) S.cnt[tid] = 0;

    // the fragments of the tile's 32 targets (one beyond the grid reads the clamped position: a row that exists)
    v4i qf[2][KSMAX];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const int qy = min(ty0 + 2 * qt + (l15 >> 3), a.Gh - 1), qx = min(tx0 + (l15 & 7), Gw - 1);
        const int8_t* qp = a.q + (int64_t)(qy * Gw + qx) * a.ldq + 16 * g;
#pragma unroll
        for (int ks = 0; ks < KSMAX; ++ks) {
            qf[qt][ks] = v4i{0, 0, 0, 0};
            if (ks < KS) qf[qt][ks] = *reinterpret_cast<const v4i*>(qp + 64 * ks);
        }
    }
    __syncthreads();

    // the row a lane loads for step tt of frame f: position 64 tt + 16 wave + l15 of the window (padding repeats the last position)
    auto load_row = [&](int f, int tt) {
        const int p = (int)min((unsigned)KN_BT * (unsigned)tt + (unsigned)(16 * wave + l15), (unsigned)(wn - 1)), dy = p / ww;      // unsigned: a step may reach 63 positions beyond wn < 2^31
        return a.bank + (int64_t)(f * GG + (y0 + dy) * Gw + x0 + (p - dy * ww)) * a.ldb + 16 * g;
    };
    v4i bf[KSMAX];
    if (ntiles > 0) {
        const int8_t* p = load_row(f0, 0);
#pragma unroll
        for (int ks = 0; ks < KSMAX; ++ks) {
            bf[ks] = v4i{0, 0, 0, 0};
            if (ks < KS) bf[ks] = *reinterpret_cast<const v4i*>(p + 64 * ks);
        }
    }
    int f = f0, tt = 0;
    for (int t = 0; t < ntiles; ++t) {
        // the next step (the last one asks for itself again: rows that exist)
        int fn = f, ttn = tt + 1;
        if (ttn == tpf) ttn = 0, fn = f + 1;
        if (t + 1 == ntiles) fn = f, ttn = tt;
        const int8_t* pn = load_row(fn, ttn);
        // the four positions of this lane's epilogue: 64 tt + 16 wave + 4 g + r
        const unsigned pbase = (unsigned)KN_BT * (unsigned)tt + (unsigned)(16 * wave + 4 * g);
        int py[4], px[4];
        unsigned row[4];
        float rn[4];
        {
            const int p = (int)min(pbase, (unsigned)(wn - 1)), dy = p / ww;
            int y = y0 + dy, x = x0 + (p - dy * ww);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                py[r] = y, px[r] = x;
                row[r] = (unsigned)(f * GG + y * Gw + x);
                rn[r] = a.rnorm[row[r]];
                if (x < x1) ++x;
                else if (y < y1) x = x0, ++y;      // (the window's last position repeats: padding)
            }
        }
        v4i acc[2] = {v4i{0, 0, 0, 0}, v4i{0, 0, 0, 0}};
#pragma unroll
        for (int ks = 0; ks < KSMAX; ++ks) {
            if (ks < KS) {
                acc[0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(bf[ks], qf[0][ks], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(bf[ks], qf[1][ks], acc[1], 0, 0, 0);
                bf[ks] = *reinterpret_cast<const v4i*>(pn + 64 * ks);
            }
        }
        const int cs = t & 1;
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            const int ql = 16 * qt + l15, qy = ty0 + 2 * qt + (l15 >> 3), qx = tx0 + (l15 & 7);
            const u64 th = S.thr[ql];
            const bool qok = qy < a.Gh && qx < Gw;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned sk = knn_skey((float)acc[qt][r] * rn[r]);      // ONE float32 multiplication (-ffp-contract=off)
                const u64 key = knn_key(sk, row[r]);
                const bool inside = abs(py[r] - qy) <= R && abs(px[r] - qx) <= R;
                if (qok && pbase + r < (unsigned)wn && inside && key > th) {
                    const int slot = atomicAdd(&S.cnt[cs], 1);                // < KN_CAND: one per (position, target) of the step
                    S.ckey[slot] = key;
                    S.cq[slot] = (unsigned char)ql;
                }
            }
        }
        __syncthreads();
        local_drain(S, cs, k, tid, lane, wave);
        __syncthreads();
        f = fn, tt = ttn;
    }

    // rank and write: wave w the targets t % 4 == w (its own lists; a segment without a frame leaves them empty)
    for (int ql = wave; ql < KN_QT; ql += 4) {
        const int qy = ty0 + (ql >> 3), qx = tx0 + (ql & 7);
        if (qy >= a.Gh || qx >= Gw) continue;
        const int q = qy * Gw + qx;
        const u64* L = S.lists + ql * LP_KCAP;
        const int c = S.cntl[ql];
        if (lane < k) {                     // k <= 32: one pass
            u64 key = 0;
            int rank = lane;                // positions c .. k - 1: no entry
            if (lane < c) {
                key = L[lane];
                rank = 0;
                for (int i = 0; i < c; ++i) rank += L[i] > key ? 1 : 0;
            }
            if (a.splits == 1) {            // c == k: k is at most the smallest window
                const int64_t o = (int64_t)q * k + rank;
                a.idx[o] = (int32_t)(0xffffffffu - (unsigned)key);
                a.score[o] = knn_score_of((unsigned)(key >> 32));
            } else {
                a.ws[((int64_t)q * a.splits + s) * k + rank] = key;
            }
        }
    }
}

// ---- the label mix: one wave per target, lanes over the classes.  Lane j < k holds w[t][j] and idx[t][j]; both sums run in rank order
// from 0.0f, every product and every sum rounded on its own (-ffp-contract=off), then one IEEE division
__global__ __launch_bounds__(KN_NT) void propagate_labels_kernel(const int32_t* __restrict__ idx, const float* __restrict__ w, int T, int k,
                                                                 const float* __restrict__ seg, int K, float* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * (KN_NT / 64) + (threadIdx.x >> 6);
    if (t >= T) return;
    float wj = 0.0f;
    int ij = 0;
    if (lane < k) {
        wj = w[t * k + lane];
        ij = idx[t * k + lane];
    }
    float sw = 0.0f;
    for (int j = 0; j < k; ++j) sw += __shfl(wj, j);
    for (int c0 = 0; c0 < K; c0 += 64) {      // (uniform trip count: the shuffles below want every lane)
        const int c = c0 + lane;
        float acc = 0.0f;
        for (int j = 0; j < k; ++j) {
            const float wv = __shfl(wj, j);
            const int64_t row = __shfl(ij, j);
            if (c < K) acc += wv * seg[row * K + c];
        }
        if (c < K) out[t * K + c] = acc / sw;
    }
}

// frame segments: the caller's count, or (0) enough workgroups for two rounds of the 256 CUs, at most one per frame
int local_splits(int tiles, int F, int splits)
{
    if (splits > 0) return splits;
    const int cap = F < IVIT_KNN_SPLITS_MAX ? F : IVIT_KNN_SPLITS_MAX;
    const int want = (512 + tiles - 1) / tiles;
    return want < cap ? want : cap;
}

int local_check_shape(const char* who, int Gh, int Gw, int F, int radius, int k, int splits)
{
    IVIT_REQUIRE(Gh >= 1 && Gw >= 1 && F >= 1 && radius >= 0, "%s: Gh=%d, Gw=%d and F=%d must be at least 1, radius=%d at least 0", who, Gh, Gw, F, radius);
    IVIT_REQUIRE((int64_t)F * Gh * Gw < ((int64_t)1 << 31), "%s: F * Gh * Gw = %d * %d * %d context tokens (below 2^31)", who, F, Gh, Gw);
    if (k > IVIT_LOCAL_K_MAX) {
        ivit_set_error("%s: unsupported geometry (k=%d above %d)", who, k, IVIT_LOCAL_K_MAX);
        return IVIT_ERR_UNSUPPORTED;
    }
    const int64_t corner = (int64_t)F * ((radius < Gh - 1 ? radius : Gh - 1) + 1) * ((radius < Gw - 1 ? radius : Gw - 1) + 1);
    IVIT_REQUIRE(k >= 1 && k <= corner, "%s: k=%d outside [1, %lld], the window of a corner token", who, k, (long long)corner);
    const int smax = F < IVIT_KNN_SPLITS_MAX ? F : IVIT_KNN_SPLITS_MAX;
    IVIT_REQUIRE(splits >= 0 && splits <= smax, "%s: splits=%d outside [0, %d]", who, splits, smax);
    return IVIT_OK;
}

int local_tiles_x(int Gw) { return (Gw + LP_TW - 1) / LP_TW; }
int64_t local_tiles(int Gh, int Gw) { return (int64_t)((Gh + LP_TH - 1) / LP_TH) * local_tiles_x(Gw); }

}      // namespace

IVIT_EXPORT int ivit_local_topk_workspace_bytes(int Gh, int Gw, int F, int k, int splits, int64_t* bytes)
{
    const char* who = "ivit_local_topk_workspace_bytes";
    IVIT_REQUIRE(bytes, "%s: NULL pointer", who);
    const int rc = local_check_shape(who, Gh, Gw, F, 0, k < 1 ? k : 1, splits);      // (k against the window: the search entry's check)
    if (rc != IVIT_OK) return rc;
    if (k > IVIT_LOCAL_K_MAX) {
        ivit_set_error("%s: unsupported geometry (k=%d above %d)", who, k, IVIT_LOCAL_K_MAX);
        return IVIT_ERR_UNSUPPORTED;
    }
    const int sp = local_splits((int)local_tiles(Gh, Gw), F, splits);
    *bytes = sp > 1 ? (int64_t)Gh * Gw * sp * k * (int64_t)sizeof(u64) : 0;
    return IVIT_OK;
}

IVIT_EXPORT int ivit_local_topk_i8(const int8_t* q, int64_t ldq, int Gh, int Gw, const int8_t* bank, int64_t ldb, int F, int C, const float* rnorm,
                                   int radius, int k, int splits, int32_t* idx, float* score, void* workspace, int64_t workspace_bytes,
                                   ivit_stream_t stream)
{
    const char* who = "ivit_local_topk_i8";
    IVIT_REQUIRE(q && bank && rnorm && idx && score, "%s: NULL operand", who);
    const int rc = local_check_shape(who, Gh, Gw, F, radius, k, splits);
    if (rc != IVIT_OK) return rc;
    if (C < 64 || C > 1024 || C % 64 != 0) {
        ivit_set_error("%s: unsupported geometry (C=%d: multiples of 64 from 64 to 1024)", who, C);
        return IVIT_ERR_UNSUPPORTED;
    }
    IVIT_REQUIRE(ldq >= C && ldb >= C, "%s: ldq=%lld / ldb=%lld below C=%d", who, (long long)ldq, (long long)ldb, C);
    IVIT_REQUIRE(((uintptr_t)q | (uintptr_t)bank | (uintptr_t)ldq | (uintptr_t)ldb) % 16 == 0, "%s: q, bank, ldq and ldb must be multiples of 16 bytes", who);
    IVIT_REQUIRE(((uintptr_t)rnorm | (uintptr_t)idx | (uintptr_t)score) % 4 == 0, "%s: rnorm, idx or score is not aligned to its element", who);
    const int64_t tiles = local_tiles(Gh, Gw);
    const int sp = local_splits((int)tiles, F, splits);
    const int T = Gh * Gw;
    const int64_t need = sp > 1 ? (int64_t)T * sp * k * (int64_t)sizeof(u64) : 0;
    IVIT_REQUIRE(need == 0 || (workspace && (uintptr_t)workspace % 8 == 0 && workspace_bytes >= need),
                 "%s: workspace of %lld bytes (aligned to 8) needed, %lld given", who, (long long)need, (long long)workspace_bytes);
    LocalArgs a;
    a.q = q, a.ldq = ldq, a.Gh = Gh, a.Gw = Gw, a.bank = bank, a.ldb = ldb, a.F = F, a.KS = C / 64, a.rnorm = rnorm;
    const int gmax = Gh > Gw ? Gh : Gw;
    a.radius = radius < gmax ? radius : gmax;      // the whole frame either way
    a.k = k, a.splits = sp, a.fps = (F + sp - 1) / sp;
    a.idx = idx, a.score = score, a.ws = static_cast<u64*>(workspace);
    a.tiles_x = local_tiles_x(Gw), a.tiles = (int)tiles;
    const int64_t grid = tiles * sp;
    const int bpq = (sp * k + KN_NT - 1) / KN_NT;
    IVIT_REQUIRE(grid <= 0x7fffffff && (int64_t)T * bpq <= 0x7fffffff, "%s: %d x %d tokens with %d segments: too many workgroups", who, Gh, Gw, sp);
    const hipStream_t st = ivit_stream(stream);
    const dim3 gd((unsigned)grid), bd(KN_NT);
    if (a.KS <= 4) hipLaunchKernelGGL(local_topk_kernel<4>, gd, bd, 0, st, a);
    else if (a.KS <= 8) hipLaunchKernelGGL(local_topk_kernel<8>, gd, bd, 0, st, a);
    else hipLaunchKernelGGL(local_topk_kernel<16>, gd, bd, 0, st, a);
    if (sp > 1)
        hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)((int64_t)T * bpq)), dim3(KN_NT), 0, st, a.ws, sp, k, bpq, idx, score);
    IVIT_CHECK_LAUNCH(who);
}

IVIT_EXPORT int ivit_propagate_labels_f32(const int32_t* idx, const float* w, int T, int k, const float* seg, int N, int K, float* out,
                                          ivit_stream_t stream)
{
    const char* who = "ivit_propagate_labels_f32";
    IVIT_REQUIRE(idx && w && seg && out, "%s: NULL operand", who);
    IVIT_REQUIRE(T >= 0 && N >= 1 && k >= 1 && k <= IVIT_LOCAL_K_MAX && K >= 1 && K <= IVIT_PROPAGATE_CLASSES_MAX,
                 "%s: T=%d N=%d k=%d (1 .. %d) K=%d (1 .. %d)", who, T, N, k, IVIT_LOCAL_K_MAX, K, IVIT_PROPAGATE_CLASSES_MAX);
    IVIT_REQUIRE(((uintptr_t)idx | (uintptr_t)w | (uintptr_t)seg | (uintptr_t)out) % 4 == 0, "%s: a pointer is not aligned to its element", who);
    if (T == 0) return IVIT_OK;
    hipLaunchKernelGGL(propagate_labels_kernel, dim3((unsigned)((T + KN_NT / 64 - 1) / (KN_NT / 64))), dim3(KN_NT), 0, ivit_stream(stream), idx, w, T, k,
                       seg, K, out);
    IVIT_CHECK_LAUNCH(who);
}
