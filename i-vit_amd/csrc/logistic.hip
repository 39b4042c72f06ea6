// logistic.hip -- one minibatch step of a softmax (logistic) linear probe trained on the int8 feature bank in place.
//   ivit_probe_ce_forward_i8   logits of the gathered rows against the bf16 compute copy of the weights, softmax, cross-entropy loss,
//                              argmax and the bf16 gradient of the logits G = p - onehot, class-major: the [B][K] logits never leave
//                              the chip unless the caller asks for them
//   ivit_probe_sgd_update_i8   D = G x^T on the same gathered rows, and as the epilogue the weight-decay / momentum / SGD chain on
//                              the float32 master weights with their new bf16 copy; one tile owns one weight: no atomics
// Both GEMMs run on v_mfma_f32_16x16x32_bf16 (A: lane (g = lane >> 4, i = lane & 15) holds row i, K slots 8 g .. 8 g + 7; B: column i,
// the same K slots; C: acc[r] of the lane is the entry (4 g + r, i)).  The order of the K slots is free -- the sum runs over them --
// as long as both operands agree, and both kernels use that: a lane takes 16 CONSECUTIVE elements of the reduction index (32 bytes
// of bf16: a whole 128-byte line per matrix row for the 16 lanes of four g) and feeds them to two MFMAs, the first eight and the
// last eight, so one "step" of either kernel is 64 reduction indices.
//
// The forward kernel.  A workgroup (4 waves) owns a strip of LG_R = 16 gathered rows and ALL Kp classes; wave w owns the classes
// w Kp / 4 .. (w + 1) Kp / 4 - 1 in nt = Kp / 64 tiles of 16 (NTMAX = 1, 4 or 16 is the template argument, a tile beyond nt is
// skipped by a uniform branch): at Kp = 1024 a lane holds 64 float32 accumulators.  The classes are the M side (A = Wh, read from
// L2 straight into fragment order, 32 bytes per lane and tile) and the rows the N side, so a lane holds ONE row (its i) and 4 nt
// classes: the row maximum, the row sum and the argmax are per-lane loops, two permlane swaps over the four g, and one trip through
// LDS over the four waves.  The strip itself is gathered through idx 16 bytes per lane, converted to bf16 once (exact) and staged in
// LDS in slabs of LG_CS = 512 channels (16.25 KiB; the row stride of 1040 bytes puts the 16 rows of a ds_read_b128 on 16 different
// bank quads); the next slab's loads are in flight while the current one is multiplied.
// 16 rows, not 32: the logits of B = 1024 rows are 64 workgroups either way far below the 256 CUs, and every workgroup streams the
// whole of Wh (3 MiB at K = 1000, C = 1536) from L2 whatever its height -- the launch is bound by that stream per CU, not by the
// MFMAs -- so the lower strip halves the accumulators (two workgroups per CU fit) and doubles the CUs that pull on L2.
//
// The update kernel.  A workgroup owns 64 classes x 64 channels of W, wave w the 16 classes 16 w .. 16 w + 15 of them (A = G, which
// the forward kernel left class-major: 32 contiguous bytes per lane from L2) against all 64 channels (four accumulator quads).
// The reduction runs over the batch rows, the strided dimension of the bank, so the B operand is a transposed read: per step 64
// gathered rows x 64 channels (wave = 16-byte piece, lane = row: one 16-byte load per thread) are converted to bf16 and written
// transposed into LDS, 16 ds_write_b16 per thread (the 64 lanes of a wave fill 128 contiguous bytes of one channel: no conflict),
// channel rows of 144 bytes, from which the lane (g, i) reads its 32 bytes of channel 16 n + i with two conflict-free
// ds_read_b128.  Two LDS tiles alternate (one barrier per step); the gather of step s + 1 and its row indices of step s + 2 are in
// flight during step s.  No split over the batch: one tile owns one element of W.
//
// Every float32 chain is written out one operation per statement and the file is compiled with -ffp-contract=off.
#include "common.h"

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef __bf16 v8bf __attribute__((ext_vector_type(8)));

constexpr int LG_NT = 256;                       // threads per workgroup (four waves)
constexpr int LG_R = 16;                         // gathered rows per strip of the forward kernel = the N of one MFMA
constexpr int LG_CS = 512;                       // channels per LDS slab of the forward kernel
constexpr int LG_LDA = 2 * LG_CS + 16;           // bytes per staged row: 260 dwords, row i on bank 4 i
constexpr int UP_T = 64;                         // classes, channels and batch rows per tile / step of the update kernel
constexpr int UP_LDT = 2 * UP_T + 16;            // bytes per channel row of the transposed tile: 36 dwords

IVIT_DEV v4f mfma_bf16(v4i a, v4i b, v4f c)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, a), __builtin_bit_cast(v8bf, b), c, 0, 0, 0);
}

// an int8 as bf16 bits: exact (8 significant bits)
IVIT_DEV unsigned bf16_of_i8(int v) { return __float_as_uint((float)v) >> 16; }

// 16 int8 (one 16-byte piece of a row) -> 16 bf16 in the same order, two v4i
IVIT_DEV void bf16x16_of_i8x16(v4i v, v4i& lo, v4i& hi)
{
    unsigned o[8];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const int w = v[d];
        o[2 * d] = bf16_of_i8((int)(int8_t)(w & 0xff)) | (bf16_of_i8((int)(int8_t)((w >> 8) & 0xff)) << 16);
        o[2 * d + 1] = bf16_of_i8((int)(int8_t)((w >> 16) & 0xff)) | (bf16_of_i8(w >> 24) << 16);
    }
    lo = v4i{(int)o[0], (int)o[1], (int)o[2], (int)o[3]};
    hi = v4i{(int)o[4], (int)o[5], (int)o[6], (int)o[7]};
}

// float32 -> bf16, round to nearest even, on the bits (finite values)
IVIT_DEV unsigned bf16_rne(float f)
{
    const unsigned u = __float_as_uint(f);
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// a (logit, class) pair as one key: larger logit first, equal logits to the lower class.  Never 0 for a finite logit
IVIT_DEV unsigned long long key_of(float z, int k)
{
    const unsigned u = __float_as_uint(z);
    const unsigned o = (u >> 31) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)o << 32) | (0xffffffffu - (unsigned)k);
}
IVIT_DEV float key_logit(unsigned long long key)
{
    const unsigned o = (unsigned)(key >> 32);
    return __uint_as_float((o >> 31) ? (o ^ 0x80000000u) : ~o);
}
IVIT_DEV int key_class(unsigned long long key) { return (int)(0xffffffffu - (unsigned)key); }

// the largest key of the four lanes l, l ^ 16, l ^ 32, l ^ 48, in every one of them
IVIT_DEV unsigned long long rows_allmax_u64(unsigned long long v)
{
    typedef unsigned v2u_ __attribute__((ext_vector_type(2)));
    const v2u_ al = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
    const v2u_ ah = __builtin_amdgcn_permlane16_swap((unsigned)(v >> 32), (unsigned)(v >> 32), false, false);
    unsigned long long x = ((unsigned long long)ah.x << 32) | al.x, y = ((unsigned long long)ah.y << 32) | al.y;
    v = x > y ? x : y;
    const v2u_ bl = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
    const v2u_ bh = __builtin_amdgcn_permlane32_swap((unsigned)(v >> 32), (unsigned)(v >> 32), false, false);
    x = ((unsigned long long)bh.x << 32) | bl.x;
    y = ((unsigned long long)bh.y << 32) | bl.y;
    return x > y ? x : y;
}
// (v(g=0) + v(g=1)) + (v(g=2) + v(g=3)) of the same four lanes, the same bits in every one of them
IVIT_DEV float rows_allsum_f32(float v)
{
    return __uint_as_float(rows_allreduce_u32(__float_as_uint(v), [](unsigned x, unsigned y) { return __float_as_uint(__uint_as_float(x) + __uint_as_float(y)); }));
}

struct FwdArgs {
    const int8_t* x;
    int64_t ldx;
    int C, K, Kp, B, Bp;
    float s;
    const int32_t* idx;
    const int32_t* y;
    const uint16_t* Wh;      // [Kp][C]
    const float* b;          // [Kp]
    uint16_t* G;             // [Kp][Bp]
    float* loss;             // [B]
    int32_t* top1;           // [B]
    float* z_out;            // [B][Kp] or NULL
};

template <int NTMAX>
__global__ __launch_bounds__(LG_NT, 2) void probe_ce_forward_kernel(FwdArgs a)
{
    __shared__ __attribute__((aligned(16))) unsigned char slab[LG_R * LG_LDA];
    __shared__ unsigned long long red_key[4][LG_R];
    __shared__ float red_sum[4][LG_R];
    __shared__ float zy_s[LG_R];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, i = lane & 15;
    const int row0 = (int)blockIdx.x * LG_R;              // < Bp: the grid is Bp / LG_R strips
    const int nt = a.Kp >> 6;                             // this wave's tiles of 16 classes (<= NTMAX)
    const int kbase = wave * (a.Kp >> 2);
    const int brow = row0 + i;                            // the lane's batch row
    const bool live = brow < a.B;

    if (row0 >= a.B) {      // a strip of padding columns only (uniform): zeros
#pragma unroll
        for (int t = 0; t < NTMAX; ++t)
            if (t < nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) a.G[(int64_t)(kbase + 16 * t + 4 * g + r) * a.Bp + brow] = 0;
        return;
    }

    v4f acc[NTMAX];
#pragma unroll
    for (int t = 0; t < NTMAX; ++t) acc[t] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
    if (tid < LG_R) zy_s[tid] = 0.0f;

    // staging: thread -> row tid >> 4 of the strip, the 16-byte pieces (tid & 15) and (tid & 15) + 16 of the slab's 32
    const int sr = tid >> 4, sp = tid & 15;
    const int8_t* xrow = nullptr;
    if (row0 + sr < a.B) xrow = a.x + (int64_t)a.idx[row0 + sr] * a.ldx;
    v4i pre[2];
    auto fetch = [&](int c0) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int ch = c0 + 16 * (sp + 16 * u);
            pre[u] = v4i{0, 0, 0, 0};
            if (xrow && ch < a.C) pre[u] = *reinterpret_cast<const v4i*>(xrow + ch);      // ch % 16 == 0, C % 64 == 0: ch + 16 <= C
        }
    };
    fetch(0);
    for (int c0 = 0; c0 < a.C; c0 += LG_CS) {
        __syncthreads();      // the previous slab has been read
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            v4i lo, hi;
            bf16x16_of_i8x16(pre[u], lo, hi);
            v4i* dst = reinterpret_cast<v4i*>(&slab[sr * LG_LDA + 32 * (sp + 16 * u)]);
            dst[0] = lo;
            dst[1] = hi;
        }
        __syncthreads();
        fetch(c0 + LG_CS);
        const int cs = min(LG_CS, a.C - c0);
        for (int kk = 0; kk < cs; kk += 64) {
            const v4i* xp = reinterpret_cast<const v4i*>(&slab[i * LG_LDA + 2 * (kk + 16 * g)]);
            const v4i xb0 = xp[0], xb1 = xp[1];
#pragma unroll
            for (int t = 0; t < NTMAX; ++t)
                if (t < nt) {
                    const v4i* wp = reinterpret_cast<const v4i*>(a.Wh + (int64_t)(kbase + 16 * t + i) * a.C + c0 + kk + 16 * g);
                    const v4i w0 = wp[0], w1 = wp[1];
                    acc[t] = mfma_bf16(w0, xb0, acc[t]);
                    acc[t] = mfma_bf16(w1, xb1, acc[t]);
                }
        }
    }

    // acc[t][r]: class kbase + 16 t + 4 g + r of row brow.  z = fl(fl(acc * s) + b[k]); the key carries (z, k)
    const int yb = live ? a.y[brow] : -1;
    unsigned long long key = 0;
#pragma unroll
    for (int t = 0; t < NTMAX; ++t)
        if (t < nt) {
            const int k4 = kbase + 16 * t + 4 * g;
            const v4f bias = *reinterpret_cast<const v4f*>(a.b + k4);
            v4f zo = v4f{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (k4 + r < a.K) {
                    float z = acc[t][r] * a.s;
                    z = z + bias[r];
                    z = z + 0.0f;      // -0 -> +0: equal logits have equal keys
                    acc[t][r] = z;
                    zo[r] = z;
                    const unsigned long long kz = key_of(z, k4 + r);
                    key = kz > key ? kz : key;
                }
            if (a.z_out && live) *reinterpret_cast<v4f*>(a.z_out + (int64_t)brow * a.Kp + k4) = zo;
        }
    key = rows_allmax_u64(key);
    if (g == 0) red_key[wave][i] = key;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const unsigned long long kw = red_key[w][i];
        key = kw > key ? kw : key;
    }
    const float m = key_logit(key);

    // e = expf(z - m), summed t ascending, r ascending in the lane, then over g, then over the waves
    float sum = 0.0f;
#pragma unroll
    for (int t = 0; t < NTMAX; ++t)
        if (t < nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = kbase + 16 * t + 4 * g + r;
                float e = 0.0f;
                if (k < a.K) {
                    const float d = acc[t][r] - m;
                    if (k == yb) zy_s[i] = d;
                    e = expf(d);
                    sum = sum + e;
                }
                acc[t][r] = e;
            }
    sum = rows_allsum_f32(sum);
    if (g == 0) red_sum[wave][i] = sum;
    __syncthreads();
    float S = red_sum[0][i] + red_sum[1][i];
    S = S + red_sum[2][i];
    S = S + red_sum[3][i];

#pragma unroll
    for (int t = 0; t < NTMAX; ++t)
        if (t < nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = kbase + 16 * t + 4 * g + r;
                unsigned gv = 0;
                if (k < a.K && live) {
                    const float p = acc[t][r] / S;
                    gv = bf16_rne(p - (k == yb ? 1.0f : 0.0f));
                }
                a.G[(int64_t)k * a.Bp + brow] = (uint16_t)gv;
            }
    if (wave == 0 && g == 0 && live) {
        a.loss[brow] = logf(S) - zy_s[i];
        a.top1[brow] = key_class(key);
    }
}

struct UpdArgs {
    const int8_t* x;
    int64_t ldx;
    int C, K, Kp, B, Bp;
    const int32_t* idx;
    const uint16_t* G;       // [Kp][Bp]
    float sB, lr, mu, wd;
    float* W;                // [Kp][C]
    float* mW;
    float* b;                // [Kp]
    float* mb;
    uint16_t* Wh;            // [Kp][C]
};

__global__ __launch_bounds__(LG_NT, 2) void probe_sgd_update_kernel(UpdArgs a)
{
    __shared__ __attribute__((aligned(16))) unsigned char xt[2][UP_T * UP_LDT];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, i = lane & 15;
    const int c0 = (int)blockIdx.x * UP_T, k0 = (int)blockIdx.y * UP_T;
    const int ns = a.Bp / UP_T;

    // staging: wave = 16-byte piece of the 64 channels, lane = batch row of the step
    const int8_t* xc = a.x + c0 + 16 * wave;
    auto row_of = [&](int s) {
        const int b = UP_T * s + lane;
        return (s < ns && b < a.B) ? a.idx[b] : -1;
    };
    auto gather = [&](int r) {
        v4i v = v4i{0, 0, 0, 0};
        if (r >= 0) v = *reinterpret_cast<const v4i*>(xc + (int64_t)r * a.ldx);
        return v;
    };
    const uint16_t* gp = a.G + (int64_t)(k0 + 16 * wave + i) * a.Bp + 16 * g;      // + 64 s: the lane's 16 columns of step s
    v4i xv = gather(row_of(0));
    int r_next = row_of(1);
    v4i ga0 = *reinterpret_cast<const v4i*>(gp), ga1 = *reinterpret_cast<const v4i*>(gp + 8);

    v4f acc[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[n] = v4f{0.0f, 0.0f, 0.0f, 0.0f};

    for (int s = 0; s < ns; ++s) {
        unsigned char* buf = xt[s & 1];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int w = xv[d];
            uint16_t* col = reinterpret_cast<uint16_t*>(buf + (16 * wave + 4 * d) * UP_LDT + 2 * lane);
            col[0] = (uint16_t)bf16_of_i8((int)(int8_t)(w & 0xff));
            col[UP_LDT / 2] = (uint16_t)bf16_of_i8((int)(int8_t)((w >> 8) & 0xff));
            col[UP_LDT] = (uint16_t)bf16_of_i8((int)(int8_t)((w >> 16) & 0xff));
            col[3 * UP_LDT / 2] = (uint16_t)bf16_of_i8(w >> 24);
        }
        __syncthreads();      // one barrier per step: the tile written two steps on is the one every wave has finished reading
        const v4i a0 = ga0, a1 = ga1;
        xv = gather(r_next);
        r_next = row_of(s + 2);
        if (s + 1 < ns) {
            ga0 = *reinterpret_cast<const v4i*>(gp + UP_T * (s + 1));
            ga1 = *reinterpret_cast<const v4i*>(gp + UP_T * (s + 1) + 8);
        }
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const v4i* xp = reinterpret_cast<const v4i*>(buf + (16 * n + i) * UP_LDT + 32 * g);
            const v4i xb0 = xp[0], xb1 = xp[1];
            acc[n] = mfma_bf16(a0, xb0, acc[n]);
            acc[n] = mfma_bf16(a1, xb1, acc[n]);
        }
    }

    // acc[n][r] = D of class k0 + 16 wave + 4 g + r, channel c0 + 16 n + i
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = k0 + 16 * wave + 4 * g + r;
        if (k >= a.K) continue;      // a padded class: its rows stay zero
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int64_t off = (int64_t)k * a.C + c0 + 16 * n + i;
            float w = a.W[off], mom = a.mW[off];
            float gr = acc[n][r] * a.sB;
            const float dec = a.wd * w;
            gr = gr + dec;
            mom = a.mu * mom;
            mom = mom + gr;
            const float stp = a.lr * mom;
            w = w - stp;
            a.mW[off] = mom;
            a.W[off] = w;
            a.Wh[off] = (uint16_t)bf16_rne(w);
        }
    }

    // the bias, by the tiles of the first channel block: thread -> class k0 + (tid >> 2), quarter q = tid & 3 of the columns:
    // the 16-byte chunks q, q + 4, ... of the class's row of G, their eight values added in ascending order into one float32;
    // then (q0 + q1) + (q2 + q3)
    if (blockIdx.x == 0) {
        const int k = k0 + (tid >> 2), q = tid & 3;
        const uint16_t* row = a.G + (int64_t)k * a.Bp;
        float sum = 0.0f;
        for (int ch = q; ch < a.Bp / 8; ch += 4) {
            const v4i v = *reinterpret_cast<const v4i*>(row + 8 * ch);
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                sum = sum + __uint_as_float((unsigned)v[d] << 16);
                sum = sum + __uint_as_float((unsigned)v[d] & 0xffff0000u);
            }
        }
        sum = sum + __shfl_xor(sum, 1);
        sum = sum + __shfl_xor(sum, 2);
        if (q == 0 && k < a.K) {
            const float gb = sum / (float)a.B;
            float mom = a.mu * a.mb[k];
            mom = mom + gb;
            const float stp = a.lr * mom;
            a.mb[k] = mom;
            a.b[k] = a.b[k] - stp;
        }
    }
}

// the geometry both entries share: the bank's of the wide probe entries, the class and batch ranges
int logistic_check(const char* who, const int8_t* x, int64_t ldx, int C, int B, int K)
{
    IVIT_REQUIRE(K >= 1, "%s: K=%d below 1", who, K);
    if (C < 64 || C > IVIT_KNN_C_WIDE_MAX || C % 64 != 0 || K > IVIT_PROBE_CLASSES_MAX) {
        ivit_set_error("%s: unsupported geometry (C=%d: multiples of 64 from 64 to %d; K=%d: at most %d)", who, C, IVIT_KNN_C_WIDE_MAX, K, IVIT_PROBE_CLASSES_MAX);
        return IVIT_ERR_UNSUPPORTED;
    }
    IVIT_REQUIRE(B >= 1 && B <= IVIT_PROBE_BATCH_MAX, "%s: B=%d outside [1, %d]", who, B, IVIT_PROBE_BATCH_MAX);
    IVIT_REQUIRE(ldx >= C, "%s: ldx=%lld below C=%d", who, (long long)ldx, C);
    IVIT_REQUIRE(((uintptr_t)x | (uintptr_t)ldx) % 16 == 0, "%s: x and ldx must be multiples of 16 bytes", who);
    return IVIT_OK;
}

}      // namespace

IVIT_EXPORT int ivit_probe_ce_forward_i8(const int8_t* x, int64_t ldx, int C, const int32_t* idx, const int32_t* y, int B, int K, float s,
                                         const uint16_t* Wh, const float* b, uint16_t* G, float* loss, int32_t* top1, float* z_out,
                                         ivit_stream_t stream)
{
    const char* who = "ivit_probe_ce_forward_i8";
    IVIT_REQUIRE(x && idx && y && Wh && b && G && loss && top1, "%s: NULL operand", who);
    if (const int rc = logistic_check(who, x, ldx, C, B, K)) return rc;
    IVIT_REQUIRE(((uintptr_t)idx | (uintptr_t)y | (uintptr_t)loss | (uintptr_t)top1) % 4 == 0, "%s: idx, y, loss or top1 is not aligned to its element", who);
    IVIT_REQUIRE(((uintptr_t)Wh | (uintptr_t)b | (uintptr_t)G | (uintptr_t)z_out) % 16 == 0, "%s: Wh, b, G and z_out must be multiples of 16 bytes", who);
    FwdArgs a;
    a.x = x, a.ldx = ldx, a.C = C, a.K = K, a.Kp = (K + 63) / 64 * 64, a.B = B, a.Bp = (B + 63) / 64 * 64, a.s = s;
    a.idx = idx, a.y = y, a.Wh = Wh, a.b = b, a.G = G, a.loss = loss, a.top1 = top1, a.z_out = z_out;
    const dim3 grid((unsigned)(a.Bp / LG_R)), block(LG_NT);
    const hipStream_t st = ivit_stream(stream);
    if (a.Kp <= 64)
        hipLaunchKernelGGL(probe_ce_forward_kernel<1>, grid, block, 0, st, a);
    else if (a.Kp <= 256)
        hipLaunchKernelGGL(probe_ce_forward_kernel<4>, grid, block, 0, st, a);
    else
        hipLaunchKernelGGL(probe_ce_forward_kernel<16>, grid, block, 0, st, a);
    IVIT_CHECK_LAUNCH(who);
}

IVIT_EXPORT int ivit_probe_sgd_update_i8(const int8_t* x, int64_t ldx, int C, const int32_t* idx, int B, int K, float s, const uint16_t* G,
                                         float lr, float mu, float wd, float* W, float* b, float* mW, float* mb, uint16_t* Wh,
                                         ivit_stream_t stream)
{
    const char* who = "ivit_probe_sgd_update_i8";
    IVIT_REQUIRE(x && idx && G && W && b && mW && mb && Wh, "%s: NULL operand", who);
    if (const int rc = logistic_check(who, x, ldx, C, B, K)) return rc;
    IVIT_REQUIRE((uintptr_t)idx % 4 == 0, "%s: idx is not aligned to its element", who);
    IVIT_REQUIRE(((uintptr_t)G | (uintptr_t)W | (uintptr_t)b | (uintptr_t)mW | (uintptr_t)mb | (uintptr_t)Wh) % 16 == 0,
                 "%s: G, W, b, mW, mb and Wh must be multiples of 16 bytes", who);
    UpdArgs a;
    a.x = x, a.ldx = ldx, a.C = C, a.K = K, a.Kp = (K + 63) / 64 * 64, a.B = B, a.Bp = (B + 63) / 64 * 64, a.idx = idx, a.G = G;
    a.sB = s / (float)B, a.lr = lr, a.mu = mu, a.wd = wd;
    a.W = W, a.mW = mW, a.b = b, a.mb = mb, a.Wh = Wh;
    hipLaunchKernelGGL(probe_sgd_update_kernel, dim3((unsigned)(C / UP_T), (unsigned)(a.Kp / UP_T)), dim3(LG_NT), 0, ivit_stream(stream), a);
    IVIT_CHECK_LAUNCH(who);
}
