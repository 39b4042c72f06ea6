// calib.hip -- percentile calibration statistics: two exact quantiles of a float tensor by radix selection
// (QuantAct with `percentile` set, quant_modules.py:319-329 of the reference: torch.quantile(x_flat, q) twice).
//
// torch.quantile sorts x to read (at most) four of its elements: the floor(rank)-th and ceil(rank)-th smallest for each q.  Here the
// four order statistics are SELECTED: the float becomes an order-preserving 32-bit key (the mapping of ivit_head_topk / ivit_minmax_f32),
// and four passes over x, most significant byte first, each narrow every wanted rank to one of 256 bins:
//   quantile_hist_kernel<PASS>   streams x; an element whose key starts with one of the (up to four distinct) prefixes found so far
//                                counts in that prefix's 256-bin histogram -- in LDS per workgroup, then vector atomics into the workspace;
//   quantile_select_kernel<PASS> one workgroup, one wave per wanted rank: scans the 256 counters, finds the bin that holds the rank,
//                                extends the prefix by that byte and rebases the rank to the bin.  After the last pass the prefix IS the
//                                key: the kernel turns the four keys back into floats and writes the two interpolations.
// Everything is stream-ordered, nothing is read back, the workspace is cleared by the first kernel.
//
// Second half: the integer parameters of a QuantLinear / QuantConv2d while the ranges still move (ivit_weight_quant_rows_f32_i8,
// ivit_bias_quant_f32_i32): the per-row weight scale, the 8-bit weights and the 32-bit bias of quant_modules.py:202-220 / 486-504 of
// the reference, in the float32 operations of prepare.weight_scale / quant_sym / LinearParams, one rounding each.
#include "common.h"
#include <cfloat>

namespace {

constexpr int QNT = 256;              // threads per workgroup (four waves: the select kernel gives one wave to each wanted rank)
constexpr int QUNROLL = 4;            // float4 loads in flight per thread
constexpr int QTILE = QNT * 4 * QUNROLL;   // elements one workgroup takes per round (4096)
constexpr int QMAXGRID = 2048;        // grid-stride beyond (256 CUs x 8; only a cap, nothing is sized by an assumed occupancy)

// workspace, in uint32 words (IVIT_QUANTILE_WS_BYTES = 4 * QWS_WORDS)
constexpr int QWS_HIST = 0;                    // [4 passes][4 slots][256 bins]
constexpr int QWS_STATE = 4 * 4 * 256;         // [5 stages][prefix[4], rank[4], slot[4]]: stage p is read by pass p
constexpr int QWS_NAN = QWS_STATE + 5 * 12;    // number of NaNs in x
constexpr int QWS_WORDS = QWS_NAN + 4;
static_assert(QWS_WORDS * 4 == IVIT_QUANTILE_WS_BYTES, "IVIT_QUANTILE_WS_BYTES (include/ivit_hip.h) is the layout above");

IVIT_DEV unsigned q_key(float v)
{
    const unsigned b = (unsigned)__float_as_int(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

IVIT_DEV float q_unkey(unsigned k) { return __int_as_float((int)((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k)); }

__global__ __launch_bounds__(QNT) void quantile_init_kernel(unsigned* ws, unsigned r0, unsigned r1, unsigned r2, unsigned r3)
{
    for (int i = threadIdx.x; i < QWS_WORDS; i += QNT) ws[i] = 0u;     // histograms, prefixes, slots (all ranks share the empty prefix), NaNs
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned* st = ws + QWS_STATE;
        st[4] = r0;
        st[5] = r1;
        st[6] = r2;
        st[7] = r3;
    }
}

// One count into h[idx] (idx < 0: this lane has none).  Called by whole waves.  Real inputs are multiples of one scale: most lanes of a
// wave hold the same bin, and 64 LDS atomics on one counter serialise.  So twice the first lane that still has a count announces its bin,
// every lane with the same bin joins, and that lane adds them all at once; what is left after two rounds goes one by one.
IVIT_DEV void hist_add(unsigned* h, int idx)
{
    bool act = idx >= 0;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const unsigned long long m = __ballot(act);
        if (m == 0) return;                                         // wave-uniform
        const int leader = __ffsll((long long)m) - 1;
        const int li = __builtin_amdgcn_readlane(idx, leader);
        const bool same = act && idx == li;
        const unsigned long long sm = __ballot(same);
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&h[li], (unsigned)__popcll(sm));
        act = act && !same;
    }
    if (act) atomicAdd(&h[idx], 1u);
}

struct QState { unsigned prefix[4]; int slot[4]; };

// histogram index of one element in pass PASS: 256 * (slot of the prefix its key starts with) + the next byte; -1 if it starts with none
template <int PASS>
IVIT_DEV int hist_index(float v, const QState& s)
{
    const unsigned k = q_key(v);
    const int digit = (int)((k >> (24 - 8 * PASS)) & 255u);
    if constexpr (PASS == 0) {
        return digit;
    } else {
        const unsigned hp = k >> (32 - 8 * PASS);
        int slot = -1;
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (s.slot[t] == t && hp == s.prefix[t]) slot = t;      // distinct prefixes: at most one matches
        return slot < 0 ? -1 : slot * 256 + digit;
    }
}

template <int PASS>
__global__ __launch_bounds__(QNT) void quantile_hist_kernel(const float* x, int64_t n, unsigned* ws)
{
    constexpr int NH = PASS == 0 ? 256 : 1024;
    __shared__ unsigned h[NH];
    for (int i = threadIdx.x; i < NH; i += QNT) h[i] = 0u;
    QState s;
    const unsigned* st = ws + QWS_STATE + 12 * PASS;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        s.prefix[t] = st[t];
        s.slot[t] = (int)st[8 + t];
    }
    __syncthreads();

    // x is 4-byte aligned only: up to 3 elements before the first 16-byte boundary, whole float4 from there, up to 3 elements behind
    const int64_t head = min<int64_t>(n, (int64_t)((4u - (unsigned)(((uintptr_t)x >> 2) & 3u)) & 3u));
    const int64_t nv = (n - head) >> 2;
    const int64_t tail0 = head + 4 * nv;                            // first element behind the vectors; n - tail0 <= 3
    const float4* xv = reinterpret_cast<const float4*>(x + head);
    unsigned nans = 0;

    if (blockIdx.x == 0) {                                          // the (at most 6) edge elements: lanes 0.. of the first workgroup
        const int e = (int)threadIdx.x;
        const int ne = (int)head + (int)(n - tail0);
        int idx = -1;
        if (e < ne) {
            const float v = e < head ? x[e] : x[tail0 + (e - head)];
            if (PASS == 0 && v != v) ++nans;
            idx = hist_index<PASS>(v, s);
        }
        hist_add(h, idx);
    }

    const int64_t stride = (int64_t)gridDim.x * QNT;
    for (int64_t base = (int64_t)blockIdx.x * QNT; base < nv; base += QUNROLL * stride) {     // workgroup-uniform trip count
        float4 v[QUNROLL];
        bool ok[QUNROLL];
#pragma unroll
        for (int u = 0; u < QUNROLL; ++u) {
            const int64_t i = base + u * stride + threadIdx.x;
            ok[u] = i < nv;
            v[u] = ok[u] ? xv[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < QUNROLL; ++u) {
            const float c[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (PASS == 0 && ok[u] && c[j] != c[j]) ++nans;
                hist_add(h, ok[u] ? hist_index<PASS>(c[j], s) : -1);
            }
        }
    }
    __syncthreads();
    unsigned* g = ws + QWS_HIST + PASS * 1024;
    for (int i = threadIdx.x; i < NH; i += QNT) {
        const unsigned c = h[i];
        if (c) atomicAdd(&g[i], c);
    }
    if constexpr (PASS == 0) {
        nans = (unsigned)lanes_allsum_i32<64>((int)nans);
        if ((threadIdx.x & 63) == 0 && nans) atomicAdd(&ws[QWS_NAN], nans);
    }
}

// lerp's two branches (torch.quantile's default interpolation).  torch's kernels are compiled with contraction: the product and the sum
// are ONE fused multiply-add there, on the CPU and on the GPU alike, so they are written as one here (the file is built with
// -ffp-contract=off: nothing else fuses).
IVIT_DEV float q_lerp(float a, float b, float w)
{
    const float d = b - a;
    return w < 0.5f ? __builtin_fmaf(w, d, a) : __builtin_fmaf(-d, 1.0f - w, b);
}

template <int PASS>
__global__ __launch_bounds__(QNT) void quantile_select_kernel(unsigned* ws, float w_lo, float w_hi, float* out2)
{
    __shared__ unsigned nprefix[4], nrank[4];
    const int t = threadIdx.x >> 6, lane = threadIdx.x & 63;        // wave t serves wanted rank t
    const unsigned* st = ws + QWS_STATE + 12 * PASS;
    const unsigned prefix = st[t], rank = st[4 + t];
    const int slot = (int)st[8 + t];
    const unsigned* g = ws + QWS_HIST + PASS * 1024 + slot * 256 + lane * 4;
    const unsigned c0 = g[0], c1 = g[1], c2 = g[2], c3 = g[3];
    if (lane == 0) {                                                // never used when the counts add up to more than the rank
        nprefix[t] = (prefix << 8) | 255u;
        nrank[t] = 0u;
    }
    // inclusive scan of the lanes' sums (the total is at most n < 2^31: 32 bits hold every partial sum)
    const unsigned mine = c0 + c1 + c2 + c3;
    unsigned incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = (unsigned)__shfl_up((int)incl, o);
        if (lane >= o) incl += up;
    }
    __syncthreads();
    unsigned below = incl - mine;                                   // elements in the bins before this lane's four
    if (rank >= below && rank < incl) {                             // exactly one lane (incl <= n < 2^31: no wrap)
        int d = 0;
        if (rank >= below + c0) { below += c0; d = 1;
            if (rank >= below + c1) { below += c1; d = 2;
                if (rank >= below + c2) { below += c2; d = 3; } } }
        nprefix[t] = (prefix << 8) | (unsigned)(lane * 4 + d);
        nrank[t] = rank - below;
    }
    __syncthreads();
    if constexpr (PASS < 3) {
        if (threadIdx.x == 0) {
            unsigned* nx = ws + QWS_STATE + 12 * (PASS + 1);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                int sl = i;
                for (int j = i - 1; j >= 0; --j)
                    if (nprefix[j] == nprefix[i]) sl = j;           // the first rank with the same prefix owns the histogram
                nx[i] = nprefix[i];
                nx[4 + i] = nrank[i];
                nx[8 + i] = (unsigned)sl;
            }
        }
    } else if (threadIdx.x < 2) {
        // One result per lane: written for one thread, the two interpolations were packed into v_pk_add_f32 / v_pk_fma_f32, whose
        // result on denormal operands was one unit off the single rounding v_fma_f32 (and the CPU's fma) gives.
        const int i = (int)threadIdx.x;
        const bool nan = ws[QWS_NAN] != 0u;                         // torch: a NaN anywhere makes every quantile NaN
        const float r = q_lerp(q_unkey(nprefix[2 * i]), q_unkey(nprefix[2 * i + 1]), i ? w_hi : w_lo);
        out2[i] = nan ? __int_as_float(0x7fc00000) : r;
    }
}

// The rank arithmetic of torch.quantile for one q (float32, each operation rounded on its own): depends on n and q only, so it runs here
// on the host.  tests/quantile_ref.py restates it in numpy and is pinned against torch.quantile.
void quantile_rank(int64_t n, float q, unsigned* lo, unsigned* hi, float* w)
{
    const float nm1 = (float)(n - 1);                 // round to nearest; exact up to 2^24
    const float rank = q * nm1;
    const float fl = __builtin_floorf(rank), ce = __builtin_ceilf(rank);
    *w = rank - fl;
    const int64_t last = n - 1;
    const int64_t l = (int64_t)fl, h = (int64_t)ce;   // above 2^24 fl(n - 1) may exceed n - 1: clamp
    *lo = (unsigned)(l < last ? l : last);
    *hi = (unsigned)(h < last ? h : last);
}

template <int PASS>
void launch_pass(const float* x, int64_t n, unsigned* ws, float w_lo, float w_hi, float* out2, int grid, hipStream_t st)
{
    hipLaunchKernelGGL(quantile_hist_kernel<PASS>, dim3(grid), dim3(QNT), 0, st, x, n, ws);
    hipLaunchKernelGGL(quantile_select_kernel<PASS>, dim3(1), dim3(QNT), 0, st, ws, w_lo, w_hi, out2);
}

// ----------------------------------------------------------------------------------------------- weight and bias quantisation
constexpr int WQ_NT = 256;            // four waves: one row each
constexpr int WQ_CHUNK = 256;         // columns a wave takes per step: one float4 per lane
constexpr int WQ_KEEP = 16;           // steps whose float4 stay in registers between the two passes: rows of up to 4096 columns
constexpr int WQ_OUT4 = 1;            // flags: w8 rows admit dword stores;
constexpr int WQ_INT4 = 2;            //        w_int rows admit 16-byte stores

// order-preserving signed key of a float (-0 below +0; denormals keep their place: no float comparison is involved) and back
IVIT_DEV int wq_key(float v)
{
    const int b = __float_as_int(v);
    return b ^ ((b >> 31) & 0x7fffffff);
}
IVIT_DEV float wq_unkey(int k) { return __int_as_float(k ^ ((k >> 31) & 0x7fffffff)); }

// column of element t of the float4 a lane holds of step `step`: VEC four consecutive columns (one 16-byte load), else four columns
// 64 apart (four dword loads, each coalesced over the wave)
template <bool VEC>
IVIT_DEV int64_t wq_col(int64_t step, int lane, int t)
{
    return VEC ? step * WQ_CHUNK + 4 * lane + t : step * WQ_CHUNK + 64 * t + lane;
}

// columns at and behind `cols` are never read: they take `fill`, an element of the row (neutral for its minimum and maximum)
template <bool VEC>
IVIT_DEV float4 wq_load(const float* wr, int64_t step, int lane, int cols, float fill)
{
    if (VEC && wq_col<VEC>(step, lane, 3) < cols) return *reinterpret_cast<const float4*>(wr + wq_col<VEC>(step, lane, 0));
    float c[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int64_t col = wq_col<VEC>(step, lane, t);
        c[t] = col < cols ? wr[col] : fill;
    }
    return make_float4(c[0], c[1], c[2], c[3]);
}

IVIT_DEV void wq_minmax(const float4& v, int& kmin, int& kmax)
{
    const int k0 = wq_key(v.x), k1 = wq_key(v.y), k2 = wq_key(v.z), k3 = wq_key(v.w);
    kmin = min(min(kmin, k0), min(k1, min(k2, k3)));
    kmax = max(max(kmax, k0), max(k1, max(k2, k3)));
}

// clamp(rint(fl(rs * v)), -128, 127): SymmetricQuantFunction on one weight (the file is built without contraction)
IVIT_DEV int wq_quant(float v, float rs)
{
    const float p = rs * v;
    return (int)fminf(fmaxf(__builtin_rintf(p), -128.0f), 127.0f);
}

template <bool VEC>
IVIT_DEV void wq_store(const float4& v, float rs, int8_t* o8, float* oi, int64_t step, int lane, int cols, int flags)
{
    const int q[4] = {wq_quant(v.x, rs), wq_quant(v.y, rs), wq_quant(v.z, rs), wq_quant(v.w, rs)};
    if (VEC && wq_col<VEC>(step, lane, 3) < cols) {
        const int64_t c0 = wq_col<VEC>(step, lane, 0);
        if (flags & WQ_OUT4) {
            *reinterpret_cast<uint32_t*>(o8 + c0) = (unsigned)(q[0] & 255) | ((unsigned)(q[1] & 255) << 8) | ((unsigned)(q[2] & 255) << 16) |
                                                    ((unsigned)q[3] << 24);
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t) o8[c0 + t] = (int8_t)q[t];
        }
        if (oi) {
            if (flags & WQ_INT4) {
                *reinterpret_cast<float4*>(oi + c0) = make_float4((float)q[0], (float)q[1], (float)q[2], (float)q[3]);
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) oi[c0 + t] = (float)q[t];
            }
        }
        return;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int64_t col = wq_col<VEC>(step, lane, t);
        if (col < cols) {
            o8[col] = (int8_t)q[t];
            if (oi) oi[col] = (float)q[t];
        }
    }
}

// One wave per row.  Pass 1 reads the row and reduces its minimum and maximum over the wave; pass 2 quantises.  KEEP: the row is at
// most WQ_KEEP steps long and stays in registers (constant indices only: no scratch); else it is read a second time.
template <bool VEC, bool KEEP>
__global__ __launch_bounds__(WQ_NT) void weight_quant_rows_kernel(const float* w, int64_t ldw, int rows, int cols, float* scale, int8_t* w8,
                                                                   int64_t ldo, float* w_int, int flags)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (WQ_NT / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;                                        // whole waves leave; there is no barrier in this kernel
    const float* wr = w + row * ldw;
    const float first = wr[0];
    int kmin = wq_key(first), kmax = kmin;
    const int64_t steps = ((int64_t)cols + WQ_CHUNK - 1) / WQ_CHUNK;
    float4 keep[KEEP ? WQ_KEEP : 1];
    if constexpr (KEEP) {
#pragma unroll
        for (int j = 0; j < WQ_KEEP; ++j) {
            if (j < steps) {                                        // wave-uniform
                keep[j] = wq_load<VEC>(wr, j, lane, cols, first);
                wq_minmax(keep[j], kmin, kmax);
            }
        }
    } else {
        for (int64_t j = 0; j < steps; ++j) {
            const float4 v = wq_load<VEC>(wr, j, lane, cols, first);
            wq_minmax(v, kmin, kmax);
        }
    }
    kmax = wave_allmax_i32(kmax);
    kmin = ~wave_allmax_i32(~kmin);
    // mx = max(-min, max), in keys; scale = max(fl(mx / 127), eps); rs = fl(1 / scale): two correctly rounded divisions
    const float mx = wq_unkey(max(wq_key(-wq_unkey(kmin)), kmax));
    const float q = mx / 127.0f;
    const float sc = q > FLT_EPSILON ? q : FLT_EPSILON;
    const float rs = 1.0f / sc;
    if (lane == 0) scale[row] = sc;
    int8_t* o8 = w8 + row * ldo;
    float* oi = w_int ? w_int + row * (int64_t)cols : nullptr;
    if constexpr (KEEP) {
#pragma unroll
        for (int j = 0; j < WQ_KEEP; ++j)
            if (j < steps) wq_store<VEC>(keep[j], rs, o8, oi, j, lane, cols, flags);
    } else {
        for (int64_t j = 0; j < steps; ++j) wq_store<VEC>(wq_load<VEC>(wr, j, lane, cols, first), rs, o8, oi, j, lane, cols, flags);
    }
}

// s_acc = fl(scale * s_in); b32 = clamp(rint(fl(fl(1 / s_acc) * bias))): quant_sym at 32 bits clips the float to [-2^31, 2^31] (the
// upper bound 2^31 - 1 is not a float32) and then takes the integer minimum with 2^31 - 1
__global__ __launch_bounds__(256) void bias_quant_kernel(const float* bias, const float* scale, int n, float s_in, float* s_acc, int32_t* b32,
                                                         float* b_int)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float sa = scale[i] * s_in;
    s_acc[i] = sa;
    if (bias == nullptr) return;
    const float rs = 1.0f / sa;
    const float p = rs * bias[i];
    const float r = __builtin_rintf(p);
    const int32_t b = r >= 2147483648.0f ? 2147483647 : r <= -2147483648.0f ? (-2147483647 - 1) : (int32_t)r;
    b32[i] = b;
    if (b_int) b_int[i] = (float)b;
}

}  // namespace

IVIT_EXPORT int ivit_quantile_pair_f32(const float* x, int64_t n, float q_lo, float q_hi, float* out2, void* workspace,
                                       int64_t workspace_bytes, ivit_stream_t stream)
{
    IVIT_REQUIRE(x && out2 && workspace, "ivit_quantile_pair_f32: NULL operand");
    IVIT_REQUIRE(n > 0 && n <= 2147483647ll, "ivit_quantile_pair_f32: n = %lld is outside 1 .. 2^31 - 1", (long long)n);
    IVIT_REQUIRE(((uintptr_t)x % 4 == 0) && ((uintptr_t)out2 % 4 == 0) && ((uintptr_t)workspace % 4 == 0),
                 "ivit_quantile_pair_f32: misaligned operand (4 bytes)");
    IVIT_REQUIRE(workspace_bytes >= IVIT_QUANTILE_WS_BYTES, "ivit_quantile_pair_f32: workspace of %lld bytes, IVIT_QUANTILE_WS_BYTES = %d",
                 (long long)workspace_bytes, IVIT_QUANTILE_WS_BYTES);
    IVIT_REQUIRE(q_lo >= 0.0f && q_lo <= 1.0f && q_hi >= 0.0f && q_hi <= 1.0f, "ivit_quantile_pair_f32: q = (%g, %g) is not in [0, 1]",
                 (double)q_lo, (double)q_hi);       // a NaN fails every comparison
    hipStream_t st = ivit_stream(stream);
    unsigned* ws = static_cast<unsigned*>(workspace);
    unsigned r[4];
    float w_lo, w_hi;
    quantile_rank(n, q_lo, &r[0], &r[1], &w_lo);
    quantile_rank(n, q_hi, &r[2], &r[3], &w_hi);
    const int64_t tiles = (n + QTILE - 1) / QTILE;
    const int grid = (int)(tiles < QMAXGRID ? tiles : QMAXGRID);
    hipLaunchKernelGGL(quantile_init_kernel, dim3(1), dim3(QNT), 0, st, ws, r[0], r[1], r[2], r[3]);
    launch_pass<0>(x, n, ws, w_lo, w_hi, out2, grid, st);
    launch_pass<1>(x, n, ws, w_lo, w_hi, out2, grid, st);
    launch_pass<2>(x, n, ws, w_lo, w_hi, out2, grid, st);
    launch_pass<3>(x, n, ws, w_lo, w_hi, out2, grid, st);
    IVIT_CHECK_LAUNCH("ivit_quantile_pair_f32");
}

IVIT_EXPORT int ivit_weight_quant_rows_f32_i8(const float* w, int64_t ldw, int rows, int cols, float* scale, int8_t* w8, int64_t ldo,
                                              float* w_int, ivit_stream_t stream)
{
    IVIT_REQUIRE(rows >= 1 && cols >= 1, "ivit_weight_quant_rows_f32_i8: rows = %d, cols = %d (both at least 1)", rows, cols);
    IVIT_REQUIRE(ldw >= cols && ldo >= cols, "ivit_weight_quant_rows_f32_i8: ldw = %lld, ldo = %lld below cols = %d", (long long)ldw,
                 (long long)ldo, cols);
    IVIT_REQUIRE(w && scale && w8, "ivit_weight_quant_rows_f32_i8: NULL operand");
    IVIT_REQUIRE(((uintptr_t)w % 4 == 0) && ((uintptr_t)scale % 4 == 0) && ((uintptr_t)w_int % 4 == 0),
                 "ivit_weight_quant_rows_f32_i8: misaligned operand (4 bytes)");
    hipStream_t st = ivit_stream(stream);
    const bool vec = ((uintptr_t)w % 16 == 0) && (ldw % 4 == 0);    // every row starts on a 16-byte boundary
    const bool keep = cols <= WQ_KEEP * WQ_CHUNK;
    const int flags = ((((uintptr_t)w8 % 4 == 0) && (ldo % 4 == 0)) ? WQ_OUT4 : 0) |
                      ((w_int && ((uintptr_t)w_int % 16 == 0) && (cols % 4 == 0)) ? WQ_INT4 : 0);
    const dim3 grid((unsigned)(((int64_t)rows + WQ_NT / 64 - 1) / (WQ_NT / 64))), block(WQ_NT);
#define IVIT_WQ_LAUNCH(V, K) hipLaunchKernelGGL((weight_quant_rows_kernel<V, K>), grid, block, 0, st, w, ldw, rows, cols, scale, w8, ldo, w_int, flags)
    if (vec && keep) IVIT_WQ_LAUNCH(true, true);
    else if (vec) IVIT_WQ_LAUNCH(true, false);
    else if (keep) IVIT_WQ_LAUNCH(false, true);
    else IVIT_WQ_LAUNCH(false, false);
#undef IVIT_WQ_LAUNCH
    IVIT_CHECK_LAUNCH("ivit_weight_quant_rows_f32_i8");
}

IVIT_EXPORT int ivit_bias_quant_f32_i32(const float* bias, const float* scale, int n, float s_in, float* s_acc, int32_t* b32, float* b_int,
                                        ivit_stream_t stream)
{
    IVIT_REQUIRE(n >= 1, "ivit_bias_quant_f32_i32: n = %d (at least 1)", n);
    IVIT_REQUIRE(scale && s_acc, "ivit_bias_quant_f32_i32: NULL operand");
    IVIT_REQUIRE(bias ? b32 != nullptr : (b32 == nullptr && b_int == nullptr),
                 "ivit_bias_quant_f32_i32: b32 goes with bias, b_int only with both");
    IVIT_REQUIRE(((uintptr_t)bias % 4 == 0) && ((uintptr_t)scale % 4 == 0) && ((uintptr_t)s_acc % 4 == 0) && ((uintptr_t)b32 % 4 == 0) &&
                     ((uintptr_t)b_int % 4 == 0),
                 "ivit_bias_quant_f32_i32: misaligned operand (4 bytes)");
    hipStream_t st = ivit_stream(stream);
    hipLaunchKernelGGL(bias_quant_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, bias, scale, n, s_in, s_acc, b32, b_int);
    IVIT_CHECK_LAUNCH("ivit_bias_quant_f32_i32");
}
