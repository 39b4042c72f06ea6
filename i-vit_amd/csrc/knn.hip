// knn.hip -- k-NN evaluation on an int8 feature bank: cosine neighbours of int8 queries without a score matrix in memory.
//   ivit_rows_rnorm_i8_f32   rnorm[j] = 1 / sqrt(sum_c b[j][c]^2) in float32 (0 for a zero row), one wave per bank row
//   ivit_knn_topk_i8         score[i][j] = fl32((float)dot(q_i, b_j) * rnorm[j]) on v_mfma_i32_16x16x64_i8, the k best per query selected
//                            in the epilogue; a second small kernel merges the lists of the bank segments
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
#include "common.h"

namespace {

typedef unsigned long long u64;

constexpr int KN_NT = 256;                   // threads per workgroup (four waves)
constexpr int KN_QT = 32;                    // queries per workgroup
constexpr int KN_BT = 64;                    // bank rows per tile (16 per wave)
constexpr int KN_KCAP = IVIT_KNN_K_MAX;      // list capacity
constexpr int KN_CAND = KN_QT * KN_BT;       // candidates a tile can produce

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

IVIT_DEV unsigned knn_skey(float s)
{
    unsigned b = (unsigned)__float_as_int(s);
    if (b == 0x80000000u) b = 0;                                   // -0 == +0
    return b ^ ((unsigned)((int)b >> 31) | 0x80000000u);           // monotone: larger float, larger unsigned
}
IVIT_DEV float knn_score_of(unsigned k) { return __int_as_float((int)((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k)); }

IVIT_DEV u64 wave_allmin_u64(u64 v) { return ~wave_allmax_u64(~v); }

// one candidate into the list of query q, by the whole wave (the only writer of that list)
IVIT_DEV void knn_insert(u64* lists, u64* thr, int* cntl, int* minpos, int q, u64 key, int k, int lane)
{
    u64* L = lists + q * KN_KCAP;
    const int c = cntl[q];
    if (c < k) {
        if (lane == 0) {
            L[c] = key;
            cntl[q] = c + 1;
        }
        if (c + 1 < k) {                // the next candidate of this query reads the count lane 0 wrote
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            return;
        }
    } else {
        if (key <= thr[q]) return;      // an earlier candidate of this tile raised the threshold
        if (lane == 0) L[minpos[q]] = key;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    u64 m = ~0ull;
    int p = 0;
    for (int j = lane; j < k; j += 64) {
        const u64 v = L[j];
        if (v < m) {
            m = v;
            p = j;
        }
    }
    const u64 wm = wave_allmin_u64(m);
    if (m == wm) {                      // keys are unique: one lane
        thr[q] = wm;
        minpos[q] = p;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int KSMAX>
__global__ __launch_bounds__(KN_NT, 2) void knn_topk_kernel(KnnArgs a)
{
    __shared__ __attribute__((aligned(16))) u64 lists[KN_QT * KN_KCAP];
    __shared__ u64 thr[KN_QT];
    __shared__ unsigned cskey[KN_CAND];
    __shared__ unsigned short cmeta[KN_CAND];      // (row in tile) << 5 | query in tile
    __shared__ int cntl[KN_QT], minpos[KN_QT], cnt[2];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l15 = lane & 15;
    // consecutive workgroups: the query tiles of one segment, so that the workgroups in flight walk the same bank rows
    const int qtile = (int)(blockIdx.x % (unsigned)a.qtiles), s = (int)(blockIdx.x / (unsigned)a.qtiles);
    const int q0 = qtile * KN_QT;
    const int64_t rb64 = (int64_t)s * a.seg, re64 = rb64 + a.seg;
    const int r_begin = rb64 < a.N ? (int)rb64 : a.N, r_end = re64 < a.N ? (int)re64 : a.N;
    const int KS = a.KS, k = a.k;

    if (tid < KN_QT) {
        thr[tid] = 0;
        cntl[tid] = 0;
        minpos[tid] = 0;
    }
    if (tid < 2) cnt[tid] = 0;

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
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            const int ql = 16 * qt + l15;
            const u64 th = thr[ql];
            const bool qok = q0 + ql < a.Q;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned row = rbase + r;
                const unsigned sk = knn_skey((float)acc[qt][r] * rn[r]);      // ONE float32 multiplication (-ffp-contract=off)
                const u64 key = ((u64)sk << 32) | (u64)(0xffffffffu - row);
                if (qok && row < (unsigned)r_end && key > th) {
                    const int slot = atomicAdd(&cnt[cs], 1);                  // < KN_CAND: one per (row, query) of the tile
                    cskey[slot] = sk;
                    cmeta[slot] = (unsigned short)(((16 * wave + 4 * g + r) << 5) | ql);
                }
            }
        }
        __syncthreads();
        const int n = cnt[cs];
        if (tid == 0) cnt[cs ^ 1] = 0;      // next tile's counter: last read before the previous tile's second barrier
        for (int e0 = 0; e0 < n; e0 += 64) {
            const int e = e0 + lane;
            unsigned sk = 0, me = 0;
            bool mine = false;
            if (e < n) {
                sk = cskey[e];
                me = cmeta[e];
                mine = (int)(me & 3u) == wave;
            }
            u64 mask = __builtin_amdgcn_ballot_w64(mine);
            while (mask) {
                const int src = __builtin_ctzll(mask);
                mask &= mask - 1;
                const unsigned sk1 = (unsigned)__builtin_amdgcn_readlane((int)sk, src), me1 = (unsigned)__builtin_amdgcn_readlane((int)me, src);
                const u64 key = ((u64)sk1 << 32) | (u64)(0xffffffffu - (tile_base + (me1 >> 5)));
                knn_insert(lists, thr, cntl, minpos, (int)(me1 & 31u), key, k, lane);
            }
        }
        __syncthreads();
    }

    // rank and write: wave w the queries q % 4 == w (its own lists; with no tile at all the lists are empty)
    for (int ql = wave; ql < KN_QT; ql += 4) {
        const int q = q0 + ql;
        if (q >= a.Q) break;
        const u64* L = lists + ql * KN_KCAP;
        const int c = cntl[ql];
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

// the lists of a query's segments (each descending, 0 = no entry, all keys distinct) -> the k largest keys, descending
__global__ __launch_bounds__(KN_NT) void knn_merge_kernel(const u64* __restrict__ ws, int splits, int k, int bpq, int32_t* __restrict__ idx,
                                                          float* __restrict__ score)
{
    const int64_t q = blockIdx.x / (unsigned)bpq;
    const int t = (int)(blockIdx.x % (unsigned)bpq) * KN_NT + threadIdx.x;
    if (t >= splits * k) return;
    const int s = t / k, p = t - s * k;
    const u64* base = ws + q * splits * k;
    const u64 key = base[t];
    if (key == 0) return;
    int rank = p;
    for (int s2 = 0; s2 < splits && rank < k; ++s2) {
        if (s2 == s) continue;
        const u64* L = base + s2 * k;
        int lo = 0, hi = k;             // number of entries of L above key
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (L[mid] > key) lo = mid + 1;
            else hi = mid;
        }
        rank += lo;
    }
    if (rank < k) {
        idx[q * k + rank] = (int32_t)(0xffffffffu - (unsigned)key);
        score[q * k + rank] = knn_score_of((unsigned)(key >> 32));
    }
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

// bank segments: the caller's count, or (0) enough workgroups for two rounds of the 256 CUs without segments below 2048 rows
int knn_splits(int Q, int N, int splits)
{
    if (splits > 0) return splits;
    const int64_t qtiles = ((int64_t)Q + KN_QT - 1) / KN_QT;
    if (qtiles <= 0) return 1;
    const int64_t want = (512 + qtiles - 1) / qtiles, cap = N / 2048;
    const int64_t sp = want < cap ? want : cap;
    return (int)(sp < 1 ? 1 : sp > IVIT_KNN_SPLITS_MAX ? IVIT_KNN_SPLITS_MAX : sp);
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

IVIT_EXPORT int ivit_knn_topk_i8(const int8_t* q, int64_t ldq, int Q, const int8_t* bank, int64_t ldb, int N, int C, const float* rnorm, int k,
                                 int splits, int32_t* idx, float* score, void* workspace, int64_t workspace_bytes, ivit_stream_t stream)
{
    const char* who = "ivit_knn_topk_i8";
    IVIT_REQUIRE(q && bank && rnorm && idx && score, "%s: NULL operand", who);
    const int rc = knn_check_shape(who, Q, N, k, splits);
    if (rc != IVIT_OK) return rc;
    if (C < 64 || C > 1024 || C % 64 != 0) {
        ivit_set_error("%s: unsupported geometry (C=%d: multiples of 64 from 64 to 1024)", who, C);
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
    a.seg = (int)((((int64_t)N + sp - 1) / sp + KN_BT - 1) / KN_BT * KN_BT);
    a.idx = idx, a.score = score, a.ws = static_cast<u64*>(workspace);
    a.qtiles = (Q + KN_QT - 1) / KN_QT;
    const int64_t grid = (int64_t)a.qtiles * sp;
    const int bpq = (sp * k + KN_NT - 1) / KN_NT;
    IVIT_REQUIRE(grid <= 0x7fffffff && (int64_t)Q * bpq <= 0x7fffffff, "%s: Q=%d with %d segments: too many workgroups", who, Q, sp);
    const hipStream_t st = ivit_stream(stream);
    if (a.KS <= 4) hipLaunchKernelGGL(knn_topk_kernel<4>, dim3((unsigned)grid), dim3(KN_NT), 0, st, a);
    else if (a.KS <= 8) hipLaunchKernelGGL(knn_topk_kernel<8>, dim3((unsigned)grid), dim3(KN_NT), 0, st, a);
    else if (a.KS <= 12) hipLaunchKernelGGL(knn_topk_kernel<12>, dim3((unsigned)grid), dim3(KN_NT), 0, st, a);
    else hipLaunchKernelGGL(knn_topk_kernel<16>, dim3((unsigned)grid), dim3(KN_NT), 0, st, a);
    if (sp > 1)
        hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)((int64_t)Q * bpq)), dim3(KN_NT), 0, st, a.ws, sp, k, bpq, idx, score);
    IVIT_CHECK_LAUNCH(who);
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
