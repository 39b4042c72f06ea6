// knn_parts.h -- the device parts shared by the kernels that stream an int8 bank past 32 resident queries: the search (knn.hip), the
// retrieval ranks (knn_ranks.hip) and the windowed search of the label propagation (propagate.hip).  The geometry of a workgroup, the
// 64-bit (score, index) key, the main loop on v_mfma_i32_16x16x64_i8 and the threshold test of its epilogue live here once; what a
// kernel does with the scores that pass the test (insert them into a top-k list, count them against a sorted list of targets) is
// its own.  The insertion into a top-k list (knn_insert) and the merge of the segments' lists (knn_merge_kernel) serve both searches.
#pragma once
#include "common.h"

namespace {

typedef unsigned long long u64;

constexpr int KN_NT = 256;                   // threads per workgroup (four waves)
constexpr int KN_QT = 32;                    // queries per workgroup
constexpr int KN_BT = 64;                    // bank rows per tile (16 per wave)
constexpr int KN_CAND = KN_QT * KN_BT;       // candidates a tile can produce

IVIT_DEV unsigned knn_skey(float s)
{
    unsigned b = (unsigned)__float_as_int(s);
    if (b == 0x80000000u) b = 0;                                   // -0 == +0
    return b ^ ((unsigned)((int)b >> 31) | 0x80000000u);           // monotone: larger float, larger unsigned
}
IVIT_DEV float knn_score_of(unsigned k) { return __int_as_float((int)((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k)); }

// larger for the better neighbour: the score's key in the high word, 2^32 - 1 - index in the low word
IVIT_DEV u64 knn_key(unsigned sk, unsigned row) { return ((u64)sk << 32) | (u64)(0xffffffffu - row); }

// the fragments of the workgroup's 32 queries (a query beyond Q - 1 reads row Q - 1: a row that exists)
template <int KSMAX>
IVIT_DEV void knn_load_queries(v4i (&qf)[2][KSMAX], const int8_t* q, int64_t ldq, int Q, int KS, int q0, int g, int l15)
{
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const int8_t* qp = q + (int64_t)min(q0 + 16 * qt + l15, Q - 1) * ldq + 16 * g;
#pragma unroll
        for (int ks = 0; ks < KSMAX; ++ks) {
            qf[qt][ks] = v4i{0, 0, 0, 0};
            if (ks < KS) qf[qt][ks] = *reinterpret_cast<const v4i*>(qp + 64 * ks);
        }
    }
}

// The main loop over the bank rows [r_begin, r_end) in tiles of KN_BT: wave w multiplies rows 16 w .. 16 w + 15 of a tile with the 32
// queries, the bank going from global memory straight into MFMA operand registers (re-issued for the next tile right behind the
// MFMAs that consumed it).  tile(t, tile_base, rbase, acc, rn) is called by every wave once per tile: acc[qt][r] of lane (g, l15) is
// dot(bank row rbase + r, query 16 qt + l15), rn[r] that row's rnorm; rows from r_end on are padding (they repeat row N - 1).
// knn_topk_kernel (knn.hip) keeps this loop written out in its own body: routed through this template its KSMAX = 4 form came out
// of the compiler with 225 VGPRs instead of 94, and its instruction stream is kept as it was.
template <int KSMAX, class Tile>
IVIT_DEV void knn_walk_rows(const v4i (&qf)[2][KSMAX], const int8_t* bank, int64_t ldb, int N, int KS, const float* rnorm, int r_begin, int r_end,
                            int wave, int g, int l15, Tile tile)
{
    const int ntiles = (r_end - r_begin + KN_BT - 1) / KN_BT;
    v4i bf[KSMAX];
    if (ntiles > 0) {
        const int8_t* p = bank + (int64_t)min((unsigned)(r_begin + 16 * wave + l15), (unsigned)(N - 1)) * ldb + 16 * g;
#pragma unroll
        for (int ks = 0; ks < KSMAX; ++ks) {
            bf[ks] = v4i{0, 0, 0, 0};
            if (ks < KS) bf[ks] = *reinterpret_cast<const v4i*>(p + 64 * ks);
        }
    }
    for (int t = 0; t < ntiles; ++t) {
        const unsigned tile_base = (unsigned)r_begin + (unsigned)(KN_BT * t);      // unsigned: N < 2^31, a tile may reach 63 rows beyond it
        // the next tile's rows (the last tile asks for itself again: rows that exist)
        const int8_t* pn = bank + (int64_t)min((unsigned)r_begin + (unsigned)(KN_BT * min(t + 1, ntiles - 1) + 16 * wave + l15), (unsigned)(N - 1)) * ldb + 16 * g;
        const unsigned rbase = tile_base + (unsigned)(16 * wave + 4 * g);
        float rn[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) rn[r] = rnorm[min(rbase + r, (unsigned)(N - 1))];
        v4i acc[2] = {v4i{0, 0, 0, 0}, v4i{0, 0, 0, 0}};
#pragma unroll
        for (int ks = 0; ks < KSMAX; ++ks) {
            if (ks < KS) {
                acc[0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(bf[ks], qf[0][ks], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(bf[ks], qf[1][ks], acc[1], 0, 0, 0);
                bf[ks] = *reinterpret_cast<const v4i*>(pn + 64 * ks);
            }
        }
        tile(t, tile_base, rbase, acc, rn);
    }
}

// the epilogue of 16 bank rows x 32 queries: acc[qt][r] of lane (g, l15) = dot(row rbase + r, query 16 qt + l15), rt0 = the tile row of
// rbase.  A key above its query's threshold S.thr goes into the tile's candidate buffer S.cskey / S.cmeta (counter S.cnt[cs]); a
// score that does not pass costs this one comparison.  Sel: the LDS state of the kernel (KnnSel of knn.hip, RankSel of knn_ranks.hip)
template <class Sel>
IVIT_DEV void knn_epilogue(Sel& S, const v4i (&acc)[2], const float (&rn)[4], unsigned rbase, int rt0, int q0, int Q, int r_end, int cs, int l15)
{
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const int ql = 16 * qt + l15;
        const u64 th = S.thr[ql];
        const bool qok = q0 + ql < Q;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const unsigned row = rbase + r;
            const unsigned sk = knn_skey((float)acc[qt][r] * rn[r]);      // ONE float32 multiplication (-ffp-contract=off)
            const u64 key = knn_key(sk, row);
            if (qok && row < (unsigned)r_end && key > th) {
                const int slot = atomicAdd(&S.cnt[cs], 1);                // < KN_CAND: one per (row, query) of the tile
                S.cskey[slot] = sk;
                S.cmeta[slot] = (unsigned short)(((rt0 + r) << 5) | ql);
            }
        }
    }
}

IVIT_DEV u64 wave_allmin_u64(u64 v) { return ~wave_allmax_u64(~v); }

// one candidate into the list of query q (lists of KCAP keys each, k <= KCAP of them in use), by the whole wave (the only writer of that list)
template <int KCAP>
IVIT_DEV void knn_insert(u64* lists, u64* thr, int* cntl, int* minpos, int q, u64 key, int k, int lane)
{
    u64* L = lists + q * KCAP;
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

// (only where the including file asks for it with KNN_PARTS_MERGE: a kernel in a header is emitted into every object that sees it)
#ifdef KNN_PARTS_MERGE
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
#endif

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

// rows per segment: ceil(N / splits) rounded up to a tile
int knn_segment_rows(int N, int sp) { return (int)((((int64_t)N + sp - 1) / sp + KN_BT - 1) / KN_BT * KN_BT); }

}      // namespace
