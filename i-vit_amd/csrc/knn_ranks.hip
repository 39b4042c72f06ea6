// knn_ranks.hip -- retrieval ranks on the int8 feature bank: the exact position of listed bank rows ("targets") in the full ranking
// of the bank against a query, in the order of the search (knn.hip, "Order"), without a sort and without a score matrix.
//   ivit_knn_ranks_i8   rank[p] = number of bank rows whose 64-bit key beats the key of target p of its query; score[p] its score
//
// Keys are unique per (query, bank row), so a rank is a count of integers comparisons: one right answer for any tiling and any number
// of bank segments.  Two kernels:
// knn_rank_keys_kernel, one workgroup per query.  A wave per target computes the exact int32 dot on 16-byte pieces (dot4, a lane per
// piece: the sum is an integer, any order), takes the ONE float32 product, writes the score, zeroes the rank and puts the key into LDS.
// Then the list (at most 256 keys) is sorted by counting -- equal keys, a target listed twice, by list position -- and goes to the
// workspace in descending order, with each target's number of strictly larger keys of its own list ("first": the position of the
// first entry equal to it).  Sorting once per query here, not once per (query tile, bank segment) in the counting pass, is why the
// counting workgroups only copy their lists.
// knn_rank_count_kernel, the grid of the search: (tiles of KN_QT = 32 queries) x (bank segments).  The main loop and the epilogue are
// the search's (knn_parts.h): query fragments resident in registers, bank rows from global memory straight into MFMA operands, and
// per score one comparison with its query's threshold -- here the query's SMALLEST target key, fixed for the whole pass.  A score
// that beats no target costs that comparison and nothing else; with the positives near the top that is almost every score.  A score
// that passes goes into the tile's candidate buffer; behind the tile's barrier every thread takes candidates, finds by binary search
// c = the number of sorted keys >= its key ("it beats the targets from position c on") and adds one to bucket c of its query's LDS
// histogram (T + 1 buckets).  A bank row that IS a target has the target's key: it lands behind every copy of itself and is never
// counted against it.  At the end of the segment an inclusive prefix sum over the buckets is the segment's count for every sorted
// position, and target p adds the count at its `first` to rank[p] (int32 atomics on the zeroed output: integer sums are unique).
// LDS: 64 KiB sorted keys + 32.1 KiB histogram + 12 KiB candidates + thresholds = 108.5 KiB: ONE workgroup per CU.
// Nothing here trusts tptr / tidx for an address: list bounds are clamped to [0, nnz) and 256, a target index to [0, N).
#include "knn_parts.h"

namespace {

constexpr int KR_T = IVIT_KNN_RANK_TARGETS_MAX;      // targets per query

struct RankArgs {
    const int8_t* q;
    int64_t ldq;
    int Q;
    const int8_t* bank;
    int64_t ldb;
    int N, KS;                // KS = C / 64
    const float* rnorm;
    const int32_t* tptr;
    int nnz, seg;             // seg: bank rows per segment (a multiple of KN_BT)
    u64* skeys;               // workspace: [nnz] keys, each query's list descending
    int32_t* first;           // workspace: [nnz], list order
    int32_t* rank;
    int qtiles;
};

// targets [b, b + T) of query q
IVIT_DEV void rank_list(const RankArgs& a, int q, int& b, int& T)
{
    b = min(max(a.tptr[q], 0), a.nnz);
    T = min(max(a.tptr[q + 1] - b, 0), min(KR_T, a.nnz - b));
}

IVIT_DEV int dot16(const v4i& x, const v4i& y, int s)
{
#pragma unroll
    for (int w = 0; w < 4; ++w) s = __builtin_amdgcn_sdot4(x[w], y[w], s, false);
    return s;
}

__global__ __launch_bounds__(KN_NT) void knn_rank_keys_kernel(RankArgs a, const int32_t* __restrict__ tidx, float* __restrict__ score)
{
    __shared__ u64 keys[KR_T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x;
    int b, T;
    rank_list(a, q, b, T);
    const int nv = 4 * a.KS;      // 16-byte pieces of a row: at most 64, one per lane
    v4i qv = v4i{0, 0, 0, 0};
    if (lane < nv) qv = *reinterpret_cast<const v4i*>(a.q + (int64_t)q * a.ldq + 16 * lane);
    for (int t = wave; t < T; t += KN_NT / 64) {
        const unsigned j = min((unsigned)tidx[b + t], (unsigned)(a.N - 1));
        int d = 0;
        if (lane < nv) d = dot16(*reinterpret_cast<const v4i*>(a.bank + (int64_t)j * a.ldb + 16 * lane), qv, 0);
        d = wave_reduce_sum_i32(d);
        if (lane == 0) {
            const unsigned sk = knn_skey((float)d * a.rnorm[j]);      // ONE float32 multiplication (-ffp-contract=off)
            score[b + t] = knn_score_of(sk);
            a.rank[b + t] = 0;
            keys[t] = knn_key(sk, j);
        }
    }
    __syncthreads();
    for (int t = tid; t < T; t += KN_NT) {
        const u64 key = keys[t];
        int above = 0, ahead = 0;       // larger keys; equal keys listed earlier
        for (int i = 0; i < T; ++i) {
            const u64 v = keys[i];
            above += v > key ? 1 : 0;
            ahead += (v == key && i < t) ? 1 : 0;
        }
        a.skeys[b + above + ahead] = key;
        a.first[b + t] = above;
    }
}

// the counting state of a workgroup in LDS (header comment); thr, cskey, cmeta and cnt are what knn_epilogue fills
struct RankSel {
    __attribute__((aligned(16))) u64 lists[KN_QT * KR_T];
    u64 thr[KN_QT];
    int hist[KN_QT][KR_T + 1];
    unsigned cskey[KN_CAND];
    unsigned short cmeta[KN_CAND];      // (row in tile) << 5 | query in tile
    int base[KN_QT], len[KN_QT], cnt[2];
};

// behind the barrier that ends the epilogues: a thread per candidate
IVIT_DEV void rank_drain(RankSel& S, unsigned tile_base, int cs, int tid)
{
    const int n = S.cnt[cs];
    if (tid == 0) S.cnt[cs ^ 1] = 0;      // next tile's counter: last read before the barrier that ended the previous tile's epilogues
    for (int e = tid; e < n; e += KN_NT) {
        const unsigned me = S.cmeta[e];
        const int ql = (int)(me & 31u);
        const u64 key = knn_key(S.cskey[e], tile_base + (me >> 5));
        const u64* L = S.lists + ql * KR_T;
        int lo = 0, hi = S.len[ql];       // number of entries of L at or above key
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (L[mid] >= key) lo = mid + 1;
            else hi = mid;
        }
        atomicAdd(&S.hist[ql][lo], 1);
    }
}

// wave w, its queries q % 4 == w: the buckets' inclusive prefix sum in place (four buckets per lane), then every target's count
IVIT_DEV void rank_finish(RankSel& S, const RankArgs& a, int lane, int wave)
{
    for (int ql = wave; ql < KN_QT; ql += KN_NT / 64) {
        const int T = S.len[ql], b = S.base[ql];
        if (T == 0) continue;
        int* H = S.hist[ql];
        int h[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) h[i] = H[4 * lane + i] + (i ? h[i - 1] : 0);      // 4 * 63 + 3 = 255 < KR_T + 1
        int x = h[3];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(x, d);
            if (lane >= d) x += o;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) H[4 * lane + i] = h[i] + (x - h[3]);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int t = lane; t < T; t += 64) {
            const int c = H[min(max(a.first[b + t], 0), KR_T)];
            if (c) atomicAdd(&a.rank[b + t], c);
        }
    }
}

template <int KSMAX>
__global__ __launch_bounds__(KN_NT, 1) void knn_rank_count_kernel(RankArgs a)
{
    __shared__ RankSel S;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l15 = lane & 15;
    // consecutive workgroups: the query tiles of one segment, so that the workgroups in flight walk the same bank rows
    const int qtile = (int)(blockIdx.x % (unsigned)a.qtiles), s = (int)(blockIdx.x / (unsigned)a.qtiles);
    const int q0 = qtile * KN_QT;
    const int64_t rb64 = (int64_t)s * a.seg, re64 = rb64 + a.seg;
    const int r_begin = rb64 < a.N ? (int)rb64 : a.N, r_end = re64 < a.N ? (int)re64 : a.N;

    // wave w copies the sorted lists of the queries q % 4 == w; a query beyond Q - 1 and an empty list let nothing pass
    for (int ql = wave; ql < KN_QT; ql += KN_NT / 64) {
        int b = 0, T = 0;
        if (q0 + ql < a.Q) rank_list(a, q0 + ql, b, T);
        for (int t = lane; t < T; t += 64) S.lists[ql * KR_T + t] = a.skeys[b + t];
        for (int c = lane; c <= KR_T; c += 64) S.hist[ql][c] = 0;
        if (lane == 0) {
            S.base[ql] = b;
            S.len[ql] = T;
            S.thr[ql] = T ? a.skeys[b + T - 1] : ~0ull;
        }
    }
    if (tid < 2) S.cnt[tid] = 0;

    v4i qf[2][KSMAX];
    knn_load_queries<KSMAX>(qf, a.q, a.ldq, a.Q, a.KS, q0, g, l15);
    __syncthreads();

    knn_walk_rows<KSMAX>(qf, a.bank, a.ldb, a.N, a.KS, a.rnorm, r_begin, r_end, wave, g, l15,
                         [&](int t, unsigned tile_base, unsigned rbase, const v4i (&acc)[2], const float (&rn)[4]) {
                             const int cs = t & 1;
                             knn_epilogue(S, acc, rn, rbase, 16 * wave + 4 * g, q0, a.Q, r_end, cs, l15);
                             __syncthreads();
                             rank_drain(S, tile_base, cs, tid);
                             __syncthreads();
                         });
    rank_finish(S, a, lane, wave);
}

// [nnz] keys, then [nnz] int32, rounded up to 8 bytes
int64_t rank_workspace(int nnz) { return ((int64_t)nnz * (int64_t)(sizeof(u64) + sizeof(int32_t)) + 7) / 8 * 8; }

int rank_check_shape(const char* who, int Q, int N, int nnz, int splits)
{
    IVIT_REQUIRE(Q >= 0 && N >= 1 && nnz >= 0, "%s: Q=%d and nnz=%d must be at least 0, N=%d at least 1", who, Q, nnz, N);
    IVIT_REQUIRE(splits >= 0 && splits <= IVIT_KNN_SPLITS_MAX, "%s: splits=%d outside [0, %d]", who, splits, IVIT_KNN_SPLITS_MAX);
    if ((int64_t)nnz > (int64_t)Q * IVIT_KNN_RANK_TARGETS_MAX) {
        ivit_set_error("%s: unsupported geometry (nnz=%d targets for Q=%d queries: at most %d per query)", who, nnz, Q, IVIT_KNN_RANK_TARGETS_MAX);
        return IVIT_ERR_UNSUPPORTED;
    }
    return IVIT_OK;
}

}      // namespace

IVIT_EXPORT int ivit_knn_ranks_workspace_bytes(int Q, int N, int nnz, int splits, int64_t* bytes)
{
    const char* who = "ivit_knn_ranks_workspace_bytes";
    IVIT_REQUIRE(bytes, "%s: NULL pointer", who);
    const int rc = rank_check_shape(who, Q, N, nnz, splits);
    if (rc != IVIT_OK) return rc;
    *bytes = rank_workspace(nnz);
    return IVIT_OK;
}

IVIT_EXPORT int ivit_knn_ranks_i8(const int8_t* q, int64_t ldq, int Q, const int8_t* bank, int64_t ldb, int N, int C, const float* rnorm,
                                  const int32_t* tptr, const int32_t* tidx, int nnz, int splits, int32_t* rank, float* score, void* workspace,
                                  int64_t workspace_bytes, ivit_stream_t stream)
{
    const char* who = "ivit_knn_ranks_i8";
    IVIT_REQUIRE(q && bank && rnorm && tptr, "%s: NULL operand", who);
    const int rc = rank_check_shape(who, Q, N, nnz, splits);
    if (rc != IVIT_OK) return rc;
    if (C < 64 || C > 1024 || C % 64 != 0) {
        ivit_set_error("%s: unsupported geometry (C=%d: multiples of 64 from 64 to 1024)", who, C);
        return IVIT_ERR_UNSUPPORTED;
    }
    IVIT_REQUIRE(ldq >= C && ldb >= C, "%s: ldq=%lld / ldb=%lld below C=%d", who, (long long)ldq, (long long)ldb, C);
    IVIT_REQUIRE(((uintptr_t)q | (uintptr_t)bank | (uintptr_t)ldq | (uintptr_t)ldb) % 16 == 0, "%s: q, bank, ldq and ldb must be multiples of 16 bytes", who);
    IVIT_REQUIRE(((uintptr_t)rnorm | (uintptr_t)tptr | (uintptr_t)tidx | (uintptr_t)rank | (uintptr_t)score) % 4 == 0,
                 "%s: rnorm, tptr, tidx, rank or score is not aligned to its element", who);
    if (nnz == 0) return IVIT_OK;      // (Q == 0 included)
    IVIT_REQUIRE(tidx && rank && score, "%s: NULL operand", who);
    const int64_t need = rank_workspace(nnz);
    IVIT_REQUIRE(workspace && (uintptr_t)workspace % 8 == 0 && workspace_bytes >= need, "%s: workspace of %lld bytes (aligned to 8) needed, %lld given", who,
                 (long long)need, (long long)workspace_bytes);
    const int sp = knn_splits(Q, N, splits);
    RankArgs a;
    a.q = q, a.ldq = ldq, a.Q = Q, a.bank = bank, a.ldb = ldb, a.N = N, a.KS = C / 64, a.rnorm = rnorm, a.tptr = tptr, a.nnz = nnz;
    a.seg = knn_segment_rows(N, sp);
    a.skeys = static_cast<u64*>(workspace), a.first = reinterpret_cast<int32_t*>(a.skeys + nnz), a.rank = rank;
    a.qtiles = (Q + KN_QT - 1) / KN_QT;
    const int64_t grid = (int64_t)a.qtiles * sp;
    IVIT_REQUIRE(grid <= 0x7fffffff, "%s: Q=%d with %d segments: too many workgroups", who, Q, sp);
    const hipStream_t st = ivit_stream(stream);
    const dim3 gd((unsigned)grid), bd(KN_NT);
    hipLaunchKernelGGL(knn_rank_keys_kernel, dim3((unsigned)Q), bd, 0, st, a, tidx, score);
    if (a.KS <= 4) hipLaunchKernelGGL(knn_rank_count_kernel<4>, gd, bd, 0, st, a);
    else if (a.KS <= 8) hipLaunchKernelGGL(knn_rank_count_kernel<8>, gd, bd, 0, st, a);
    else if (a.KS <= 12) hipLaunchKernelGGL(knn_rank_count_kernel<12>, gd, bd, 0, st, a);
    else hipLaunchKernelGGL(knn_rank_count_kernel<16>, gd, bd, 0, st, a);
    IVIT_CHECK_LAUNCH(who);
}
