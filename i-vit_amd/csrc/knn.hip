// knn.hip -- k-NN evaluation on an int8 feature bank: cosine neighbours of int8 queries without a score matrix in memory.
//   ivit_rows_rnorm_i8_f32   rnorm[j] = 1 / sqrt(sum_c b[j][c]^2) in float32 (0 for a zero row), one wave per bank row
//   ivit_knn_topk_i8         score[i][j] = fl32((float)dot(q_i, b_j) * rnorm[j]) on v_mfma_i32_16x16x64_i8, the k best per query selected
//                            in the epilogue; a second small kernel merges the lists of the bank segments
//   ivit_knn_topk_i8_wide    the same search for rows of up to 4096 channels: knn_splitc_kernel splits the channels, not the bank rows, over the waves
//   ivit_knn_vote_f32        weighted vote among a query's own k neighbours
//
// The search kernel.  A workgroup (4 waves) owns KN_QT = 32 queries and one bank segment.  Every wave holds the fragments of all 32
// queries in registers for the whole pass (2 x C / 64 x 4 VGPRs: 128 at C = 1024) and walks its own 16 of the 64 bank rows of a tile:
// a bank row is needed by one wave only, so the bank goes from global memory straight into MFMA operand registers (one 16-byte load
// per lane and 64 channels, re-issued for the next tile right behind the MFMAs that consumed it) and LDS carries no operand at all.
// Bank = A operand, queries = B operand: acc[r] of lane (g = lane >> 4, l15 = lane & 15) is dot(bank row 4g + r, query l15).
// Order.  (score, index) is packed into one 64-bit key that is larger for the better neighbour: the float's bits mapped monotonically
// to an unsigned (-0 first made +0) in the high word, 2^32 - 1 - index in the low word.  Keys are unique, so "the k largest keys,
// descending" is the contract's order whatever the tiling, the segments or the order of insertion.
// Selection.  LDS holds the 32 candidate lists (k <= 256 keys each, unsorted, 64 KiB), per query the smallest key of a full list
// (the threshold; 0 while the list fills) and its position.  The epilogue compares each key with its query's threshold; a key that
// passes is appended to a per-tile candidate buffer (LDS atomic counter).  After a barrier wave w inserts the candidates of the
// queries q with q % 4 == w -- no list has two writers: the candidate replaces the list's minimum if it (still) beats it, then the 64
// lanes rescan the list for the new minimum.  After warm-up almost no key passes and the tile costs its two barriers.
// At the end every list is ranked (rank = number of larger keys) and written in order: to idx / score with one segment, else to the
// workspace [Q][splits][k] as keys (0 = no entry), which knn_merge_kernel ranks across segments by binary searches.
// The geometry, the key and the epilogue's threshold test are shared with the rank kernels (knn_ranks.hip): knn_parts.h.
#define KNN_PARTS_MERGE      // knn_merge_kernel
#include "knn_parts.h"

namespace {

constexpr int KN_KCAP = IVIT_KNN_K_MAX;      // list capacity

struct KnnArgs {
    const int8_t* q;
    int64_t ldq;
    int Q;
    const int8_t* bank;
    int64_t ldb;
    int N, KS;                // KS = C / 64
    const float* rnorm;
    int k, splits, seg;       // seg: bank rows per segment (a multiple of KN_BT)
    int32_t* idx;
    float* score;
    u64* ws;
    int qtiles;
};

// the selection state of a workgroup in LDS (header comment, "Selection") and its three steps, shared by both search kernels
struct KnnSel {
    __attribute__((aligned(16))) u64 lists[KN_QT * KN_KCAP];
    u64 thr[KN_QT];
    unsigned cskey[KN_CAND];
    unsigned short cmeta[KN_CAND];      // (row in tile) << 5 | query in tile
    int cntl[KN_QT], minpos[KN_QT], cnt[2];
};

IVIT_DEV void knn_sel_init(KnnSel& S, int tid)
{
    if (tid < KN_QT) {
        S.thr[tid] = 0;
        S.cntl[tid] = 0;
        S.minpos[tid] = 0;
    }
    if (tid < 2) S.cnt[tid] = 0;
}

// behind the barrier that ends the epilogues: wave w inserts the candidates of the queries q % 4 == w
IVIT_DEV void knn_drain(KnnSel& S, unsigned tile_base, int cs, int k, int tid, int lane, int wave)
{
    const int n = S.cnt[cs];
    if (tid == 0) S.cnt[cs ^ 1] = 0;      // next tile's counter: last read before the barrier that ended the previous tile's epilogues
    for (int e0 = 0; e0 < n; e0 += 64) {
        const int e = e0 + lane;
        unsigned sk = 0, me = 0;
        bool mine = false;
        if (e < n) {
            sk = S.cskey[e];
            me = S.cmeta[e];
            mine = (int)(me & 3u) == wave;
        }
        u64 mask = __builtin_amdgcn_ballot_w64(mine);
        while (mask) {
            const int src = __builtin_ctzll(mask);
            mask &= mask - 1;
            const unsigned sk1 = (unsigned)__builtin_amdgcn_readlane((int)sk, src), me1 = (unsigned)__builtin_amdgcn_readlane((int)me, src);
            const u64 key = knn_key(sk1, tile_base + (me1 >> 5));
            knn_insert<KN_KCAP>(S.lists, S.thr, S.cntl, S.minpos, (int)(me1 & 31u), key, k, lane);
        }
    }
}

// rank and write: wave w the queries q % 4 == w (its own lists; with no tile at all the lists are empty)
IVIT_DEV void knn_finish(const KnnSel& S, const KnnArgs& a, int q0, int s, int lane, int wave)
{
    const int k = a.k;
    for (int ql = wave; ql < KN_QT; ql += 4) {
        const int q = q0 + ql;
        if (q >= a.Q) break;
        const u64* L = S.lists + ql * KN_KCAP;
        const int c = S.cntl[ql];
        for (int j = lane; j < k; j += 64) {
            u64 key = 0;
            int rank = j;               // positions c .. k - 1: no entry
            if (j < c) {
                key = L[j];
                rank = 0;
                for (int i = 0; i < c; ++i) rank += L[i] > key ? 1 : 0;
            }
            if (a.splits == 1) {        // c == k: k <= N
                const int64_t o = (int64_t)q * k + rank;
                a.idx[o] = (int32_t)(0xffffffffu - (unsigned)key);
                a.score[o] = knn_score_of((unsigned)(key >> 32));
            } else {
                a.ws[((int64_t)q * a.splits + s) * k + rank] = key;
            }
        }
    }
}

template <int KSMAX>
__global__ __launch_bounds__(KN_NT, 2) void knn_topk_kernel(KnnArgs a)
{
    __shared__ KnnSel S;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l15 = lane & 15;
    // consecutive workgroups: the query tiles of one segment, so that the workgroups in flight walk the same bank rows
    const int qtile = (int)(blockIdx.x % (unsigned)a.qtiles), s = (int)(blockIdx.x / (unsigned)a.qtiles);
    const int q0 = qtile * KN_QT;
    const int64_t rb64 = (int64_t)s * a.seg, re64 = rb64 + a.seg;
    const int r_begin = rb64 < a.N ? (int)rb64 : a.N, r_end = re64 < a.N ? (int)re64 : a.N;
    const int KS = a.KS, k = a.k;

    knn_sel_init(S, tid);

    v4i qf[2][KSMAX];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const int8_t* qp = a.q + (int64_t)min(q0 + 16 * qt + l15, a.Q - 1) * a.ldq + 16 * g;
#pragma unroll
        for (int ks = 0; ks < KSMAX; ++ks) {
            qf[qt][ks] = v4i{0, 0, 0, 0};
            if (ks < KS) qf[qt][ks] = *reinterpret_cast<const v4i*>(qp + 64 * ks);
        }
    }
    __syncthreads();

    const int ntiles = (r_end - r_begin + KN_BT - 1) / KN_BT;
    v4i bf[KSMAX];
    if (ntiles > 0) {
        const int8_t* p = a.bank + (int64_t)min((unsigned)(r_begin + 16 * wave + l15), (unsigned)(a.N - 1)) * a.ldb + 16 * g;
#pragma unroll
        for (int ks = 0; ks < KSMAX; ++ks) {
            bf[ks] = v4i{0, 0, 0, 0};
            if (ks < KS) bf[ks] = *reinterpret_cast<const v4i*>(p + 64 * ks);
        }
    }
    for (int t = 0; t < ntiles; ++t) {
        const unsigned tile_base = (unsigned)r_begin + (unsigned)(KN_BT * t);      // unsigned: N < 2^31, a tile may reach 63 rows beyond it
        // the next tile's rows (the last tile asks for itself again: rows that exist)
        const int8_t* pn = a.bank + (int64_t)min((unsigned)r_begin + (unsigned)(KN_BT * min(t + 1, ntiles - 1) + 16 * wave + l15), (unsigned)(a.N - 1)) * a.ldb + 16 * g;
        const unsigned rbase = tile_base + (unsigned)(16 * wave + 4 * g);
        float rn[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) rn[r] = a.rnorm[min(rbase + r, (unsigned)(a.N - 1))];
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
        knn_epilogue(S, acc, rn, rbase, 16 * wave + 4 * g, q0, a.Q, r_end, cs, l15);
        __syncthreads();
        knn_drain(S, tile_base, cs, k, tid, lane, wave);
        __syncthreads();
    }
    knn_finish(S, a, q0, s, lane, wave);
}

// The wide search kernel (C up to IVIT_KNN_C_WIDE_MAX): the CHANNELS are split over the four waves, not the bank rows.  Wave w owns the K
// steps w, w + 4, ... of the C / 64 (at most SPW = 16 of them) and holds only those of the 32 queries (2 x SPW x 4 VGPRs: today's 128 at
// C = 4096).  All four waves walk the same bank rows in sub-tiles of 16: a wave's fragments of a sub-tile (SPW x 4 VGPRs) go from
// global memory straight into MFMA operand registers and are re-issued, PF sub-tiles ahead, right behind the MFMAs that consumed them.
// The partial accumulators of the four sub-tiles of a 64-row tile (2 x v4i per lane and sub-tile) go to LDS, [sub-tile][wave][query
// half][lane] in 16-byte pieces (32 KiB); behind one barrier wave w adds the four partials of sub-tile w -- int32, exact, any order --
// and holds dot(row 16 w + 4 g + r, query l15) in the lane layout of knn_topk_kernel: from there on the code is the shared one.
// A wave without a K step (C = 64, 128, 192) writes zeros.
// Barriers: two per tile.  The partials of tile t are last read before the barrier that ends tile t's epilogues, and everything the
// insertions of tile t write (lists, thresholds, the next counter) is first read behind the barrier that follows tile t + 1's MFMAs,
// so the insertions of one tile and the MFMAs of the next need no barrier between them.
// LDS is 108.5 KiB: ONE workgroup per CU (one wave per SIMD, up to 512 registers each), which is why the bank is prefetched deeper.
template <int SPW, int PF>
__global__ __launch_bounds__(KN_NT, 1) void knn_splitc_kernel(KnnArgs a)
{
    static_assert(PF == 1 || PF == 2 || PF == 4, "the prefetch ring must divide the four sub-tiles of a tile");
    __shared__ KnnSel S;
    __shared__ __attribute__((aligned(16))) v4i part[4][4][2][64];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4, l15 = lane & 15;
    const int qtile = (int)(blockIdx.x % (unsigned)a.qtiles), s = (int)(blockIdx.x / (unsigned)a.qtiles);
    const int q0 = qtile * KN_QT;
    const int64_t rb64 = (int64_t)s * a.seg, re64 = rb64 + a.seg;
    const int r_begin = rb64 < a.N ? (int)rb64 : a.N, r_end = re64 < a.N ? (int)re64 : a.N;
    const int k = a.k;
    const int steps = (a.KS - wave + 3) >> 2;      // this wave's K steps: wave + 4 i, i < steps <= SPW (0 for a wave beyond C / 64)
    const int koff = 64 * wave + 16 * g;           // its 16 bytes of step i: koff + 256 i

    knn_sel_init(S, tid);

    v4i qf[2][SPW];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const int8_t* qp = a.q + (int64_t)min(q0 + 16 * qt + l15, a.Q - 1) * a.ldq + koff;
#pragma unroll
        for (int i = 0; i < SPW; ++i) {
            qf[qt][i] = v4i{0, 0, 0, 0};
            if (i < steps) qf[qt][i] = *reinterpret_cast<const v4i*>(qp + 256 * i);
        }
    }
    __syncthreads();

    const int ntiles = (r_end - r_begin + KN_BT - 1) / KN_BT;
    // sub-tile j of the segment: rows r_begin + 16 j .. + 15, for every wave (unsigned: N < 2^31; a sub-tile beyond the bank asks for
    // row N - 1: a row that exists)
    auto subtile = [&](int j) { return a.bank + (int64_t)min((unsigned)r_begin + (unsigned)(16 * j + l15), (unsigned)(a.N - 1)) * a.ldb + koff; };
    v4i bf[PF][SPW];
    if (ntiles > 0) {
#pragma unroll
        for (int d = 0; d < PF; ++d) {
            const int8_t* p = subtile(d);
#pragma unroll
            for (int i = 0; i < SPW; ++i) {
                bf[d][i] = v4i{0, 0, 0, 0};
                if (i < steps) bf[d][i] = *reinterpret_cast<const v4i*>(p + 256 * i);
            }
        }
    }
    for (int t = 0; t < ntiles; ++t) {
        const unsigned tile_base = (unsigned)r_begin + (unsigned)(KN_BT * t);
        const unsigned rbase = tile_base + (unsigned)(16 * wave + 4 * g);      // the rows whose epilogue is this wave's
        float rn[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) rn[r] = a.rnorm[min(rbase + r, (unsigned)(a.N - 1))];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int8_t* pn = subtile(4 * t + u + PF);
            v4i pa[2] = {v4i{0, 0, 0, 0}, v4i{0, 0, 0, 0}};
#pragma unroll
            for (int i = 0; i < SPW; ++i) {
                if (i < steps) {
                    pa[0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(bf[u % PF][i], qf[0][i], pa[0], 0, 0, 0);
                    pa[1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(bf[u % PF][i], qf[1][i], pa[1], 0, 0, 0);
                    bf[u % PF][i] = *reinterpret_cast<const v4i*>(pn + 256 * i);
                }
            }
            part[u][wave][0][lane] = pa[0];
            part[u][wave][1][lane] = pa[1];
        }
        __syncthreads();
        v4i acc[2];
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) acc[qt] = (part[wave][0][qt][lane] + part[wave][1][qt][lane]) + (part[wave][2][qt][lane] + part[wave][3][qt][lane]);
        const int cs = t & 1;
        knn_epilogue(S, acc, rn, rbase, 16 * wave + 4 * g, q0, a.Q, r_end, cs, l15);
        __syncthreads();
        knn_drain(S, tile_base, cs, k, tid, lane, wave);
    }
    knn_finish(S, a, q0, s, lane, wave);
}

// ---- rnorm: one wave per row; 16-byte loads where the row starts on a 16-byte boundary, bytes otherwise
IVIT_DEV int sq4(unsigned w)
{
    const int a = (int8_t)(w & 0xffu), b = (int8_t)((w >> 8) & 0xffu), c = (int8_t)((w >> 16) & 0xffu), d = (int8_t)(w >> 24);
    return a * a + b * b + c * c + d * d;
}

__global__ __launch_bounds__(KN_NT) void rows_rnorm_kernel(const int8_t* __restrict__ x, int64_t ldx, int64_t rows, int C, float* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (KN_NT / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int8_t* xr = x + row * ldx;
    int s = 0, c0 = 0;
    if (((uintptr_t)xr & 15) == 0) {
        const int nv = C >> 4;
        for (int c = lane; c < nv; c += 64) {
            const uint4 w = *reinterpret_cast<const uint4*>(xr + 16 * c);
            s += sq4(w.x) + sq4(w.y) + sq4(w.z) + sq4(w.w);
        }
        c0 = nv << 4;
    }
    for (int c = c0 + lane; c < C; c += 64) s += (int)xr[c] * (int)xr[c];
    s = wave_reduce_sum_i32(s);
    if (lane == 0) out[row] = s ? 1.0f / sqrtf((float)s) : 0.0f;      // correctly rounded sqrt and division
}

// ---- vote: one wave per query, everything among its k neighbours
__global__ __launch_bounds__(64) void knn_vote_kernel(const int32_t* __restrict__ idx, const int32_t* __restrict__ labels, const float* __restrict__ w,
                                                      int k, int r, int32_t* __restrict__ classes, float* __restrict__ votes)
{
    __shared__ int lab[KN_KCAP], first[KN_KCAP];
    __shared__ float ww[KN_KCAP], vt[KN_KCAP];
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    for (int j = lane; j < k; j += 64) {
        lab[j] = labels[idx[q * k + j]];
        ww[j] = w[q * k + j];
    }
    __syncthreads();
    for (int j = lane; j < k; j += 64) {
        const int l = lab[j];
        int f = 1;
        float v = 0.0f;
        for (int i = 0; i < k; ++i)
            if (lab[i] == l) {
                if (i < j) f = 0;
                v += ww[i];             // rank order, from 0
            }
        vt[j] = v;
        first[j] = f;
    }
    __syncthreads();
    int distinct = 0;
    for (int i = 0; i < k; ++i) distinct += first[i];
    for (int j = lane; j < k; j += 64) {
        if (!first[j]) continue;
        const int l = lab[j];
        const float v = vt[j];
        int rank = 0;
        for (int i = 0; i < k; ++i) rank += (first[i] && (vt[i] > v || (vt[i] == v && lab[i] < l))) ? 1 : 0;
        if (rank < r) {
            classes[q * r + rank] = l;
            votes[q * r + rank] = v;
        }
    }
    for (int p = distinct + lane; p < r; p += 64) {
        classes[q * r + p] = -1;
        votes[q * r + p] = 0.0f;
    }
}

int knn_check_shape(const char* who, int Q, int N, int k, int splits)
{
    IVIT_REQUIRE(Q >= 0 && N >= 1, "%s: Q=%d must be at least 0, N=%d at least 1", who, Q, N);
    IVIT_REQUIRE(k >= 1 && k <= N, "%s: k=%d outside [1, N=%d]", who, k, N);
    IVIT_REQUIRE(splits >= 0 && splits <= IVIT_KNN_SPLITS_MAX, "%s: splits=%d outside [0, %d]", who, splits, IVIT_KNN_SPLITS_MAX);
    if (k > IVIT_KNN_K_MAX) {
        ivit_set_error("%s: unsupported geometry (k=%d above %d)", who, k, IVIT_KNN_K_MAX);
        return IVIT_ERR_UNSUPPORTED;
    }
    return IVIT_OK;
}

}      // namespace

IVIT_EXPORT int ivit_rows_rnorm_i8_f32(const int8_t* x, int64_t ldx, int64_t rows, int C, float* out, ivit_stream_t stream)
{
    const char* who = "ivit_rows_rnorm_i8_f32";
    IVIT_REQUIRE(x && out, "%s: NULL pointer", who);
    IVIT_REQUIRE(C >= 1 && C <= 65536 && rows >= 0, "%s: C=%d outside [1, 65536] or rows=%lld below 0", who, C, (long long)rows);
    IVIT_REQUIRE(ldx >= C, "%s: ldx=%lld below C=%d", who, (long long)ldx, C);
    IVIT_REQUIRE((uintptr_t)out % sizeof(float) == 0, "%s: out is not aligned to its element", who);
    if (rows == 0) return IVIT_OK;
    const int64_t grid = (rows + KN_NT / 64 - 1) / (KN_NT / 64);
    IVIT_REQUIRE(grid <= 0x7fffffff, "%s: rows=%lld (at most 2^33 - 4)", who, (long long)rows);
    hipLaunchKernelGGL(rows_rnorm_kernel, dim3((unsigned)grid), dim3(KN_NT), 0, ivit_stream(stream), x, ldx, rows, C, out);
    IVIT_CHECK_LAUNCH(who);
}

IVIT_EXPORT int ivit_knn_workspace_bytes(int Q, int N, int k, int splits, int64_t* bytes)
{
    const char* who = "ivit_knn_workspace_bytes";
    IVIT_REQUIRE(bytes, "%s: NULL pointer", who);
    const int rc = knn_check_shape(who, Q, N, k, splits);
    if (rc != IVIT_OK) return rc;
    const int sp = knn_splits(Q, N, splits);
    *bytes = sp > 1 ? (int64_t)Q * sp * k * (int64_t)sizeof(u64) : 0;
    return IVIT_OK;
}

namespace {

// both search entries: the checks, the segment plan and the merge are shared; cmax picks the kernel family
int knn_search(const char* who, int cmax, const int8_t* q, int64_t ldq, int Q, const int8_t* bank, int64_t ldb, int N, int C, const float* rnorm, int k,
               int splits, int32_t* idx, float* score, void* workspace, int64_t workspace_bytes, ivit_stream_t stream)
{
    IVIT_REQUIRE(q && bank && rnorm && idx && score, "%s: NULL operand", who);
    const int rc = knn_check_shape(who, Q, N, k, splits);
    if (rc != IVIT_OK) return rc;
    if (C < 64 || C > cmax || C % 64 != 0) {
        ivit_set_error("%s: unsupported geometry (C=%d: multiples of 64 from 64 to %d)", who, C, cmax);
        return IVIT_ERR_UNSUPPORTED;
    }
    IVIT_REQUIRE(ldq >= C && ldb >= C, "%s: ldq=%lld / ldb=%lld below C=%d", who, (long long)ldq, (long long)ldb, C);
    IVIT_REQUIRE(((uintptr_t)q | (uintptr_t)bank | (uintptr_t)ldq | (uintptr_t)ldb) % 16 == 0, "%s: q, bank, ldq and ldb must be multiples of 16 bytes", who);
    IVIT_REQUIRE(((uintptr_t)rnorm | (uintptr_t)idx | (uintptr_t)score) % 4 == 0, "%s: rnorm, idx or score is not aligned to its element", who);
    const int sp = knn_splits(Q, N, splits);
    const int64_t need = sp > 1 ? (int64_t)Q * sp * k * (int64_t)sizeof(u64) : 0;
    IVIT_REQUIRE(need == 0 || (workspace && (uintptr_t)workspace % 8 == 0 && workspace_bytes >= need),
                 "%s: workspace of %lld bytes (aligned to 8) needed, %lld given", who, (long long)need, (long long)workspace_bytes);
    if (Q == 0) return IVIT_OK;
    KnnArgs a;
    a.q = q, a.ldq = ldq, a.Q = Q, a.bank = bank, a.ldb = ldb, a.N = N, a.KS = C / 64, a.rnorm = rnorm, a.k = k, a.splits = sp;
    a.seg = knn_segment_rows(N, sp);
    a.idx = idx, a.score = score, a.ws = static_cast<u64*>(workspace);
    a.qtiles = (Q + KN_QT - 1) / KN_QT;
    const int64_t grid = (int64_t)a.qtiles * sp;
    const int bpq = (sp * k + KN_NT - 1) / KN_NT;
    IVIT_REQUIRE(grid <= 0x7fffffff && (int64_t)Q * bpq <= 0x7fffffff, "%s: Q=%d with %d segments: too many workgroups", who, Q, sp);
    const hipStream_t st = ivit_stream(stream);
    const dim3 gd((unsigned)grid), bd(KN_NT);
    if (cmax == IVIT_KNN_C_WIDE_MAX) {
        const int spw = (a.KS + 3) / 4;      // K steps of wave 0, the most any wave owns
        if (spw <= 4) hipLaunchKernelGGL((knn_splitc_kernel<4, 4>), gd, bd, 0, st, a);
        else if (spw <= 6) hipLaunchKernelGGL((knn_splitc_kernel<6, 4>), gd, bd, 0, st, a);
        else if (spw <= 8) hipLaunchKernelGGL((knn_splitc_kernel<8, 4>), gd, bd, 0, st, a);
        else if (spw <= 12) hipLaunchKernelGGL((knn_splitc_kernel<12, 2>), gd, bd, 0, st, a);
        else hipLaunchKernelGGL((knn_splitc_kernel<16, 2>), gd, bd, 0, st, a);
    } else if (a.KS <= 4) hipLaunchKernelGGL(knn_topk_kernel<4>, gd, bd, 0, st, a);
    else if (a.KS <= 8) hipLaunchKernelGGL(knn_topk_kernel<8>, gd, bd, 0, st, a);
    else if (a.KS <= 12) hipLaunchKernelGGL(knn_topk_kernel<12>, gd, bd, 0, st, a);
    else hipLaunchKernelGGL(knn_topk_kernel<16>, gd, bd, 0, st, a);
    if (sp > 1)
        hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)((int64_t)Q * bpq)), dim3(KN_NT), 0, st, a.ws, sp, k, bpq, idx, score);
    IVIT_CHECK_LAUNCH(who);
}

}      // namespace

IVIT_EXPORT int ivit_knn_topk_i8(const int8_t* q, int64_t ldq, int Q, const int8_t* bank, int64_t ldb, int N, int C, const float* rnorm, int k,
                                 int splits, int32_t* idx, float* score, void* workspace, int64_t workspace_bytes, ivit_stream_t stream)
{
    return knn_search("ivit_knn_topk_i8", 1024, q, ldq, Q, bank, ldb, N, C, rnorm, k, splits, idx, score, workspace, workspace_bytes, stream);
}

IVIT_EXPORT int ivit_knn_topk_i8_wide(const int8_t* q, int64_t ldq, int Q, const int8_t* bank, int64_t ldb, int N, int C, const float* rnorm, int k,
                                      int splits, int32_t* idx, float* score, void* workspace, int64_t workspace_bytes, ivit_stream_t stream)
{
    return knn_search("ivit_knn_topk_i8_wide", IVIT_KNN_C_WIDE_MAX, q, ldq, Q, bank, ldb, N, C, rnorm, k, splits, idx, score, workspace,
                      workspace_bytes, stream);
}

IVIT_EXPORT int ivit_knn_vote_f32(const int32_t* idx, const int32_t* labels, const float* w, int Q, int N, int k, int r, int32_t* classes,
                                  float* votes, ivit_stream_t stream)
{
    const char* who = "ivit_knn_vote_f32";
    IVIT_REQUIRE(idx && labels && w && classes && votes, "%s: NULL operand", who);
    IVIT_REQUIRE(Q >= 0 && N >= 1 && k >= 1 && k <= IVIT_KNN_K_MAX && r >= 1 && r <= k, "%s: Q=%d N=%d k=%d (1 .. %d) r=%d (1 .. k)", who, Q, N, k,
                 IVIT_KNN_K_MAX, r);
    IVIT_REQUIRE(((uintptr_t)idx | (uintptr_t)labels | (uintptr_t)w | (uintptr_t)classes | (uintptr_t)votes) % 4 == 0, "%s: a pointer is not aligned to its element", who);
    if (Q == 0) return IVIT_OK;
    hipLaunchKernelGGL(knn_vote_kernel, dim3((unsigned)Q), dim3(64), 0, ivit_stream(stream), idx, labels, w, k, r, classes, votes);
    IVIT_CHECK_LAUNCH(who);
}
