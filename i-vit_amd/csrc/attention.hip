// attention.hip -- fused integer attention core, one workgroup per (image, head).
// Replaces, for one head, the chain of /root/reference/models/vit_quant.py:72-85
//   matmul_1 (QuantMatMul, quant_modules.py:404-409) -> * scale -> qact_attn1 (fixedpoint_mul)
//   -> IVITIntSoftmax (Shiftmax, ivit_modules.py:150-179) -> matmul_2 -> qact2
// without materialising the [B,H,T,T] score tensor.
//
// MFMA formulation (v_mfma_i32_16x16x64_i8: the whole head dimension is ONE instruction deep):
//   S^T tile (16 keys x 16 queries) = K_tile . Q_tile^T: keys are the "A" rows, queries the "B" columns, so a
//   lane owns ONE query (col = lane&15) and 4 keys of each 16-key tile (key = 16kt + 4(lane>>4) + r); the lanes
//   l, l^16, l^32, l^48 share a query.  A whole Shiftmax row (<= 208 keys) is 13 x 4 registers in four lanes:
//   row max / row sum are register reductions plus two cross-lane exchanges.  ~110 VGPRs, so several
//   workgroups share a CU and one wave's Shiftmax arithmetic (VALU) runs under another's MFMAs.
//   O^T tile (16 d x 16 queries) = Vt . P^T over key steps of 64: the packed int8 probabilities of four
//   consecutive key tiles ARE the "B" fragment (byte 4t + r of step s = key 64s + 16t + 4g + r); V is transposed
//   once per workgroup into LDS with its keys stored in exactly that byte order, so the "A" fragment is a single
//   ds_read_b128.  Both LDS images are swizzled for conflict-free 16-lane-group reads.
// Shiftmax's integer exponential depends only on (row max - k) in [0,255]: tabulated once per workgroup in LDS
// (256 x float32, every entry an integer that float32 holds exactly) with the reference's arithmetic (shiftexp_int), ONE gather per score; the
// row sum is a float32 sum of the gathered values, which below 2^24 is exact and IS the reference's float32 sum (the natural-scale
// forms keep an exact u32 sum of their u32 tables); a row that reaches 2^24 takes its float32 sum in the order of torch's CPU
// kernel instead (attn_parts.h SHIFTMAX_ORDER_SUM, torch_rowsum_tiles), behind one wave-uniform branch per query tile.
#include "common.h"
#include "rowsum.h"

#if IVIT_LAB
static int g_attn_debug = 0;     // ivit_debug_attention (include/ivit_hip_debug.h): phase ablations, score form, part count
IVIT_EXPORT int ivit_debug_attention(int bits) { g_attn_debug = bits; return IVIT_OK; }
#else
constexpr int g_attn_debug = 0;
#endif

namespace {

constexpr int NT = 256;
constexpr int HD = 64;                 // head dim = one 16x16x64 MFMA deep
constexpr int NKT = 13;                // key tiles of 16 (tokens <= 208)
constexpr int KP = NKT * 16;           // 208 K rows in LDS
constexpr int NKS = 4;                 // key steps of 64 for P.V (256 key slots; P = 0 beyond T)
constexpr int VT_ROW = NKS * 64;       // 256 B per d row: one bank row, chunk j stored at j ^ (d & 15)
constexpr int K_BYTES = KP * HD;       // 13312
constexpr int VT_BYTES = HD * VT_ROW;  // 16384
constexpr int LUT_OFF = K_BYTES + VT_BYTES;
constexpr int SMEM_BYTES = LUT_OFF + 2 * 256 * 4;   // the natural-scale and I-BERT forms (tables elsewhere): K, V^T and 2 KB of slack, the footprint their occupancy was measured with
// MODE 0: the exponent table as float32, the one value both the row sum and the product of :175 take (attn_parts.h
// SHIFTMAX_ORDER_SUM).  Entry i on bank i % 32: the indices of a row cluster, and neighbouring indices never meet on a bank
// (lane-interleaved copies of the table narrow each copy to fewer banks and measured MORE conflicts: DESIGN.md section 8)
constexpr int SMEM0_BYTES = LUT_OFF + 256 * 4;

#include "attn_parts.h"

struct AttnArgs {
    const int8_t* qkv;
    int8_t* out;
    int batch, heads, tokens;
    double Ms, Mo;
    int x0;    // floor(-1/s_attn)
    int ksat;  // first table index whose argument is clamped at n*x0: every later entry is identical
    int out_blocks;   // output in the GEMM block layout (common.h: ivit_block_offset), row length heads * 64
    // natural-scale ("compat") Shiftmax: exp_int as a function of (row max q, q), [256][256] u32 indexed
    // (qmax + 128) * 256 + (q + 128).  The reference's Shiftmax runs its whole float32 sequence on phi(q) = fl(fl(q*s)/s)
    // (ivit_modules.py:165-170; the .to(int32) of :166 is discarded), so the exponent is no longer a function of qmax - q
    // alone; the host tabulates it with the reference's float32 steps (prepare.shiftexp2d).  NULL: power-of-two scale.
    const unsigned* exp2d;
    // The same table in BAND form for the LDS path: band[(qmax + 128) * band_w + j] = exp_int of (qmax, q = qmax - j),
    // j < band_w; band_w is a multiple of 16 and entry band_w - 1 is already the saturated value -|x0| (the argument is
    // clamped at n * x0 from there on, ivit_modules.py:155), so index min(qmax - q, band_w - 1) covers every q.  Each wave
    // stages the band rows of its 16 queries in LDS per query tile: 64 LDS lanes per cycle instead of one table address per
    // cycle through the texture addresser (the full-table gather made the kernel 2.6x slower).  0: use exp2d.
    const unsigned* band;
    int band_w;
    // I-BERT softmax (MODE 3): exp_int after the internal QuantAct(16), as the float32 the reference sums and multiplies, for
    // every (row max, q): [256][256], built by ivit_ibert_softmax_build_table
    const float* ib_table;
    float nMs32;  // RQ32 kernels: -Ms as float32 (a power of two: the float32 product with a score accumulator is exact)
    int parts;  // workgroups per (image, head): the query tiles are dealt out among them (small batches: batch * heads << CUs)
    int abl;   // lab build: 1 no score requant, 2 no table lookups, 4 no probability products, 8 no P.V + output, 16 one query tile per wave
};

constexpr int BAND_PAD = 4;   // dwords: keeps slice rows 16-byte aligned and rotates their banks

// K image: 64-byte rows; 16-byte chunk c of row r at slot (c + 2*((r>>2)&1)) & 3.  A 16x16x64 fragment read has
// lanes 0-15 on rows 0-15 chunk 0, lanes 16-31 chunk 1, ...; with this rotation every ds_read_b128 lane group
// ({0-3,12-15,20-27}, {4-11,16-19,28-31}, ...) touches 16 distinct 16-byte slots of the 256-byte bank row.
IVIT_DEV int kswz(int r, int c) { return r * HD + (((c + 2 * ((r >> 2) & 1)) & 3) << 4); }

// MODE 0: power-of-two input scale (256-entry table); 1: natural scale, band rows in LDS; 2: natural scale, full-table gather;
// 3 / 4: the I-BERT softmax (ibert_modules.py:237-319) from its (row max, q) table (3: gathered from global memory, 4: band rows
// staged in LDS like mode 1), row sum in torch's float32 reduction order
// PB: width of the softmax output (softmax_bw, vit_quant.py:184): 8, or 16 -- probabilities up to 2^15 as three 7-bit planes
// (p = c + 128 b + 16384 a), one P.V MFMA set per plane (the a plane only when a wave has such a score) -- or 4: the code path of
// 8 with the factor scaled by 2^-4, probabilities below 8 (Shiftmax) or up to 8 inclusive (I-BERT) in the one byte plane
// GENT ("general T", Shiftmax modes only): any token count up to 207 -- every key tile takes the masked path of the last one
// (keys >= T carry the sentinel), all 13 key tiles are still walked: for geometries other than 14 x 14 patches, not tuned.
// RQ32 (MODE 0, PB 8): the requantisation of the scores in float32 -- one v_cvt_f32_i32 + one v_fma_f32 against the magic constant
// instead of v_cvt_f64_i32 + v_fma_f64 (4 + 4 cycles per wave instruction against 3.2 + 2, profiles/r04_valu_price_list.txt) --
// when the multiplier Ms is a power of two (every scale of the power-of-two regime is, and head_dim^-0.5 = 1/8): |S| <= 2^20 is
// exact in float32, S * Ms is exact, the fma rounds once, to nearest even at integer granularity, exactly as the float64 path.
// The scores are then carried with the magic constant's exponent bits in place (RQ_OFF + nk): differences and minima commute
// with the offset, so the table index nk + rmax needs no correction.
constexpr int RQ_OFF = 0x4B400000;
template <int MODE, int PB = 8, int OCC = (PB == 8 ? 4 : 3), bool GENT = false, bool RQ32 = false>
__global__ __launch_bounds__(NT, OCC) void attention_kernel(AttnArgs a)
{
    static_assert(PB == 4 || PB == 8 || PB == 16, "softmax output width");
    static_assert(!RQ32 || (MODE == 0 && PB <= 8), "RQ32: Shiftmax with a power-of-two input scale, one plane of probabilities");
    constexpr int SOFF = RQ32 ? RQ_OFF : 0;       // offset the (negated) scores are carried with
    constexpr int PADK = SOFF + 1000;             // sentinel of the padding keys
    __shared__ __attribute__((aligned(16))) char smem[MODE == 0 ? SMEM0_BYTES : SMEM_BYTES];
    extern __shared__ __attribute__((aligned(16))) unsigned band_lds[];   // [4 waves][16 queries][band_w + BAND_PAD], compat only
    const int T = a.tokens;
    const int bh = blockIdx.x / a.parts, part = blockIdx.x - bh * a.parts;
    const int b = bh / a.heads, hh = bh - b * a.heads;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, l15 = lane & 15;
    const int64_t plane = (int64_t)a.batch * a.heads * T * HD;
    const int8_t* qg = a.qkv + (int64_t)bh * T * HD;
    const int8_t* kg = qg + plane;
    const int8_t* vg = qg + 2 * plane;

    // ---- Shiftmax exponent table: lut[i] = int_exp_shift(-i) as float32 (exact: attn_parts.h), i = kmax - k in [0,255]
    if constexpr (MODE == 0) reinterpret_cast<float*>(smem + LUT_OFF)[tid] = (float)shiftexp_int(-tid, a.x0, 15);

    // ---- K tile [key][64]; rows >= T are never consumed unmasked.  ALL of a thread's K and V chunks are requested before the
    //      first is written to LDS (T <= 208: at most 4 K chunks and one V work item of 4 chunks per thread): one memory latency
    //      per workgroup instead of one per loop iteration (round 4: a staging-only launch took 24 us = 8 us per round of
    //      workgroups, profiles/r04g_*)
    static_assert(KP * 4 <= 4 * NT && (KP / 4) * 4 <= NT, "staging: four K chunks and one V work item per thread");
    v4i kst[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = min(tid + NT * i, T * 4 - 1);
        kst[i] = *reinterpret_cast<const v4i*>(kg + (int64_t)(q >> 2) * HD + 16 * (q & 3));
    }
    // ---- V transposed: Vt[d][chunk j = 4s + g'][byte 4t + r] = V[key = 64s + 16t + 4g' + r][d], chunk j of row d
    //      stored at position j ^ (d & 15).  One work item = 4 consecutive keys x 16 d: the 4x4 byte blocks are
    //      transposed in registers (v_perm_b32), so every LDS write is a whole dword (4 keys of one d).
    const bool v_item = tid < ((T + 3) >> 2) * 4;
    v4i vst[4];
    {
        const int kg4 = min(tid, ((T + 3) >> 2) * 4 - 1) >> 2, c = tid & 3;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            vst[r] = *reinterpret_cast<const v4i*>(vg + (int64_t)min(4 * kg4 + r, T - 1) * HD + 16 * c);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = tid + NT * i;
        if (q < T * 4) *reinterpret_cast<v4i*>(smem + kswz(q >> 2, q & 3)) = kst[i];
    }
    if (v_item) {
        const int q = tid;
        const int kg4 = q >> 2, c = q & 3;      // keys 4*kg4 .. 4*kg4+3, d = 16c .. 16c+15
        v4i (&v)[4] = vst;
        const int key0 = 4 * kg4;
        const int j = 4 * (key0 >> 6) + ((key0 >> 2) & 3);
        const int boff = 4 * ((key0 >> 4) & 3);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            // rows = keys r (v[r][w] holds d = 16c+4w .. +3 in its bytes) -> columns: dword bb = 4 keys of d = 16c+4w+bb
            const unsigned a0 = (unsigned)v[0][w], a1 = (unsigned)v[1][w], a2 = (unsigned)v[2][w], a3 = (unsigned)v[3][w];
            unsigned t[4];
            bytes4x4_transpose(a0, a1, a2, a3, t);
#pragma unroll
            for (int bb = 0; bb < 4; ++bb) {
                const int d = 16 * c + 4 * w + bb;
                *reinterpret_cast<unsigned*>(smem + K_BYTES + d * VT_ROW + ((j ^ (d & 15)) << 4) + boff) = t[bb];
            }
        }
    }
    __syncthreads();

    const float* lut = reinterpret_cast<const float*>(smem + LUT_OFF);
    const int nqt = (T + 15) >> 4;

    // 13 query tiles over 4 waves: one wave gets four tiles, the others three.  Which wave that is rotates with the
    // workgroup index, so that the co-resident workgroups of a CU do not all put their extra tile on the same SIMD
    // the Q fragment of a wave's NEXT query tile is requested while the current tile's probabilities are multiplied with V (its
    // registers are free there): the load's latency no longer opens every tile
    const int qt0 = ((wave + bh) & 3) + 4 * part, qt_end = (IVIT_LAB && (a.abl & 16)) ? 4 : nqt;
    v4i qf_next = *reinterpret_cast<const v4i*>(qg + (int64_t)min(qt0 * 16 + l15, T - 1) * HD + 16 * g);
    for (int qt = qt0; qt < qt_end; qt += 4 * a.parts) {
        const int qrow = qt * 16 + l15;  // this lane's query
        const v4i qf = qf_next;

        // ---- S^T = K . Q^T, requantised to the 8-bit Shiftmax input (qact_attn1)
        // scores are kept NEGATED (nk = -k = RNE(S * -Ms): RNE is symmetric): the table index max - k = nk + max is then one
        // v_add_lshl_u32 per score instead of a subtract and a shift
        int s[NKT][4];
        int nmin = PADK;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            const v4i kf = *reinterpret_cast<const v4i*>(smem + kswz(16 * kt + l15, g));
            v4i acc = {0, 0, 0, 0};
            acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(kf, qf, acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                // |S| <= 64*128*128 = 2^20, m < 2^32: the product is exact in float64
                int nk;
                if constexpr (RQ32) {
                    const int tb = __float_as_int(__builtin_fmaf((float)acc[r], a.nMs32, 12582912.0f));     // RQ_OFF + RNE(-S * Ms)
                    nk = (IVIT_LAB && (a.abl & 1)) ? SOFF + (acc[r] & 127) : clamp_i32(tb, SOFF - 127, SOFF + 128);
                } else {
                    nk = (IVIT_LAB && (a.abl & 1)) ? (acc[r] & 127) : clamp_i32(requant_exact(acc[r], -a.Ms), -127, 128);
                }
                if (GENT || kt == NKT - 1) nk = (16 * kt + 4 * g + r < T) ? nk : PADK;
                s[kt][r] = nk;
                nmin = min(nmin, nk);
            }
            if ((kt & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // at most 4 K fragments in flight (registers)
        }
        nmin = rows_allmin_i32(nmin);      // over the four lanes of a query (common.h: permlane swaps, no LDS round trip)
        int rmax = -nmin;                // RQ32: -(RQ_OFF + nmin), so that nk + rmax is the plain difference
        asm volatile("" : "+v"(rmax));   // opaque: keeps (nk + rmax) << 2 one v_add_lshl_u32 instead of a subtract and a shift

        // ---- Shiftmax (ivit_modules.py:164-175): e = exp_int(k - max), sum, factor, e*factor >> 24
        // k - max is in [-255, 0] for every real key: the 256-entry table covers it without a clamp (the entries from
        // ksat on are identical anyway); only the padding keys of the last tile carry the -1000 sentinel
        unsigned esum = 0;      // natural scales: exact integer row sum; I-BERT: the float32 sum's bits
        float fsum = 0.0f;      // MODE 0: float32 row sum of the gathered float32 exponents
        if constexpr (MODE == 1) {     // natural input scale, band rows of this tile's 16 queries staged in LDS
            const int W = a.band_w, stride = W + BAND_PAD;
            unsigned* slice = band_lds + (wave * 16 + l15) * stride;
            {
                const uint4* src = reinterpret_cast<const uint4*>(a.band + (size_t)(rmax + 128) * W) + g * (W >> 4);
                uint4* dst = reinterpret_cast<uint4*>(slice) + g * (W >> 4);
                for (int i = 0; i < (W >> 4); ++i) dst[i] = src[i];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int nk = s[kt][r];
                    unsigned e = slice[min(nk + rmax, W - 1)];     // the 1000 sentinel of the padding keys clamps, too
                    if (GENT || kt == NKT - 1) e = (nk == 1000) ? 0u : e;
                    s[kt][r] = __float_as_int((float)e);     // float32 value of the exponent, as MODE 0 keeps it: what the product below takes
                    esum += e;
                }
            __builtin_amdgcn_wave_barrier();    // every lane has read its slice before the next tile overwrites it
        } else if constexpr (MODE >= 3) {
            // IBERTIntSoftmax: e = table[row max][q] (float32), S = e.sum() in float32 IN TORCH'S ORDER (ATen SumKernel, rowsum.h:
            // for 192 <= T < 208 the 32 partials p = key % 32 take their six elements key = p, p + 32, .. in turn, vectors of
            // keys 192.. join partials 0..7, the scalar tail goes first into the final accumulator, then the eight lane sums
            // ((P[l] + P[l+8]) + P[l+16]) + P[l+24] are added left to right).  With key = 16 kt + 4 g + r a lane holds the whole
            // sequence of its eight partials (hi = kt & 1, r): they are summed in registers, exchanged among the four lanes of
            // a query and combined by every lane alike.  The values are integers for a power-of-two range of the internal
            // QuantAct and fl(fl(k * s) / s) otherwise: the order matters then.
            const float* row2d = a.ib_table + ((rmax + 128) << 8) + 128;       // mode 3: entry of q = -nk
            const int W = a.band_w, stride = W + BAND_PAD;
            const unsigned* slice = band_lds + (wave * 16 + l15) * stride;     // mode 4: this query's band row
            if constexpr (MODE == 4) {
                const uint4* src = reinterpret_cast<const uint4*>(a.band + (size_t)(rmax + 128) * W) + g * (W >> 4);
                uint4* dst = reinterpret_cast<uint4*>(band_lds + (wave * 16 + l15) * stride) + g * (W >> 4);
                for (int i = 0; i < (W >> 4); ++i) dst[i] = src[i];
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
            float e12[4];
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int nk = s[kt][r];
                    float e;
                    if constexpr (MODE == 4) e = __int_as_float((int)slice[min(nk + rmax, W - 1)]);   // the 1000 sentinel clamps, too
                    else e = row2d[-min(nk, 128)];
                    if (kt == NKT - 1) {
                        e = (nk == 1000) ? 0.0f : e;
                        e12[r] = e;
                    }
                    s[kt][r] = __float_as_int(e);
                }
            if constexpr (MODE == 4) __builtin_amdgcn_wave_barrier();    // every lane has read its slice before the next tile overwrites it
            const int nv = T >> 3;                 // 8-float vectors: 24 or 25 (the launcher keeps T < 208)
            float Pp[2][4];
#pragma unroll
            for (int hi = 0; hi < 2; ++hi)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float acc = 0.0f;
#pragma unroll
                    for (int m = 0; m < 6; ++m) acc += __int_as_float(s[2 * m + hi][r]);
                    Pp[hi][r] = acc;
                }
            if (nv > 24 && g < 2) {                // vector 24 = keys 192 .. 199 -> partials 0 .. 7 (lanes g = 0, 1; hi = 0)
#pragma unroll
                for (int r = 0; r < 4; ++r) Pp[0][r] += e12[r];
            }
            // the tail and the partials are exchanged among the four lanes of the query (gather4)
            float fin = 0.0f;
            {
                float t12[4][4];                   // [r][g']
#pragma unroll
                for (int r = 0; r < 4; ++r) gather4(e12[r], t12[r]);
#pragma unroll
                for (int gp = 0; gp < 4; ++gp)     // scalar tail: keys 8 nv .. T - 1 in order
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int key = 192 + 4 * gp + r;
                        if (key >= 8 * nv && key < T) fin += t12[r][gp];
                    }
            }
            float A[4][2][4];
#pragma unroll
            for (int hi = 0; hi < 2; ++hi)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float t[4];
                    gather4(Pp[hi][r], t);
#pragma unroll
                    for (int gp = 0; gp < 4; ++gp) A[gp][hi][r] = t[gp];
                }
#pragma unroll
            for (int l = 0; l < 8; ++l) {
                const int gm = l >> 2, r = l & 3;
                const float v = ((A[gm][0][r] + A[2 + gm][0][r]) + A[gm][1][r]) + A[2 + gm][1][r];
                fin += v;
            }
            esum = (unsigned)__float_as_int(fin);   // carried as bits to the common code below
        } else if constexpr (MODE == 2) {      // one L2-resident gather per score instead of the LDS lookup
            const unsigned* row2d = a.exp2d + ((rmax + 128) << 8) + 128;       // entry of q = -nk
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int nk = s[kt][r];
                    unsigned e = row2d[-min(nk, 128)];
                    if (GENT || kt == NKT - 1) e = (nk == 1000) ? 0u : e;
                    s[kt][r] = __float_as_int((float)e);
                    esum += e;
                }
        } else {
            // ONE gather per score: the float32 entry is the factor of the product below AND the term of the row sum, which is
            // taken in float32 (attn_parts.h SHIFTMAX_ORDER_SUM: exact below 2^24, and at or above 2^24 exactly when the exact sum
            // is)
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float ef;
                    if (GENT || kt == NKT - 1) {
                        ef = lut[min(rmax + s[kt][r], 255)];
                        ef = s[kt][r] == PADK ? 0.0f : ef;
                    } else if (IVIT_LAB && (a.abl & 2)) {
                        ef = 1.0f;
                    } else {
                        ef = lut[rmax + s[kt][r]];
                    }
                    s[kt][r] = __float_as_int(ef);       // float32 bit pattern of the exponent
                    fsum += ef;
                }
        }
        // every mode has left the exponents in s[][] as float32 bit patterns
        float factor;
        if constexpr (MODE >= 3) {
            factor = floorf(4294967296.0f / __int_as_float((int)esum));        // ibert_modules.py:313
        } else {
            bool ordered;
            if constexpr (MODE == 0) {
                const float tot = rows_allsum_f32(fsum);      // the four lanes may round differently only at or above 2^24
                ordered = tot >= (float)SHIFTMAX_ORDER_SUM;
                factor = shiftmax_factor(tot);
            } else {
                const unsigned tot = rows_allsum_u32(esum);
                ordered = tot >= SHIFTMAX_ORDER_SUM;
                factor = shiftmax_factor(tot);
            }
            // a row whose exact sum reaches 2^24: the reference's float32 sum depends on torch's order of additions (attn_parts.h).
            // Wave-uniform and rare (no row of the model fixtures gets here); the other rows of the tile keep their factor.
            if (__builtin_expect(__builtin_amdgcn_ballot_w64(ordered) != 0, 0)) {
                const float S = torch_rowsum_tiles<NKT>(s, [](int v) { return __int_as_float(v); }, T);
                factor = ordered ? shiftmax_factor(S) : factor;
            }
        }
        if constexpr (PB == 4) factor *= 0.0625f;      // the last shift is 2^(31 - 4 + 1) (:175; I-BERT :313-314): see below

        // packed probabilities: dword t of key step ks = bytes r = 0..3 of key tile 4ks + t
        v4i pk[NKS];
        v4i pkb[PB == 16 ? NKS : 1];       // 16-bit probabilities: the second 7-bit plane
        // I-BERT at 4 bits: p = floor(fl32(e * factor) / 2^29) in [0, 8]; the 8 of a one-hot row is an ordinary int8 value and needs no
        // second operand
        constexpr bool HI_PLANE = (MODE >= 3 && PB == 8) || PB == 16;
        v4i pkh[HI_PLANE ? NKS : 1];      // I-BERT: probabilities reach 128 (a one-hot row): 128 = 127 + 1, the 1 in a second operand
        // I-BERT: p = floor(fl32(e * factor) / 2^25) in [0, 128] (ibert_modules.py:314, output_bit = 8).  factor / 2 is an exact
        // scaling, so u = trunc(e * (factor / 2)) has p in its top byte like the Shiftmax product below -- except p = 128, which
        // shows as the sign bit of u: the OR of all u of the tile is tested once and the tile repacked in that rare case.
        const float factor_h = factor * 0.5f;
        unsigned any_u = 0;
        constexpr bool SDWA_PACK = MODE < 3 && PB <= 8;
        if constexpr (SDWA_PACK) {
            // p = floor(fl32(e * factor) / 2^24) (:175) = trunc(fl32(e * (factor * 2^-24))): the scaling by a power of two commutes
            // with the float32 rounding of the product (no operand or result is subnormal: factor >= 1, e >= 1 or e == 0), and
            // p < 128.  For a width PB <= 8 in general the shift is 2^(32 - PB): the scaling by 2^-(32 - PB) is as exact (at PB = 4
            // the smallest non-zero product, 2^-28, is far from subnormal) and p < 2^(PB - 1) (8 at PB = 4); `factor` already
            // carries the 2^-(8 - PB).  v_cvt_u32_f32 with SDWA destination select writes the truncated value straight into byte r of the packed
            // dword (UNUSED_PRESERVE keeps the other bytes; semantics checked by scripts/probes/cvt_pack_probe.hip): one
            // instruction per score instead of a conversion plus 3/4 of a byte permute / OR.  The four dwords of a key step are
            // written round-robin, so that no instruction reads the register the previous one wrote with a destination select
            // (gfx940+ dst_sel forwarding hazard: one wait state, which the compiler cannot insert inside inline asm).
            const float factor24 = factor * 5.9604644775390625e-08f;     // 2^-24, exact
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                float pf[4][4];
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int kt2 = 4 * ks + t < NKT ? 4 * ks + t : 0;
                        const float ev = __int_as_float(s[kt2][r]);
                        pf[t][r] = (IVIT_LAB && (a.abl & 4)) ? 1.0f : ev * factor24;     // lab bit 2: no products
                    }
                unsigned w0 = 0, w1 = 0, w2 = 0, w3 = 0;
                if (4 * ks + 3 < NKT) {
                    // (the first write of each dword zero-fills its other bytes: UNUSED_PAD, early-clobber outputs, no initialisation)
                    asm("v_cvt_u32_f32_sdwa %0, %4 dst_sel:BYTE_0 dst_unused:UNUSED_PAD src0_sel:DWORD\n\t"
                        "v_cvt_u32_f32_sdwa %1, %5 dst_sel:BYTE_0 dst_unused:UNUSED_PAD src0_sel:DWORD\n\t"
                        "v_cvt_u32_f32_sdwa %2, %6 dst_sel:BYTE_0 dst_unused:UNUSED_PAD src0_sel:DWORD\n\t"
                        "v_cvt_u32_f32_sdwa %3, %7 dst_sel:BYTE_0 dst_unused:UNUSED_PAD src0_sel:DWORD\n\t"
                        "v_cvt_u32_f32_sdwa %0, %8 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD\n\t"
                        "v_cvt_u32_f32_sdwa %1, %9 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD\n\t"
                        "v_cvt_u32_f32_sdwa %2, %10 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD\n\t"
                        "v_cvt_u32_f32_sdwa %3, %11 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD\n\t"
                        "v_cvt_u32_f32_sdwa %0, %12 dst_sel:BYTE_2 dst_unused:UNUSED_PRESERVE src0_sel:DWORD\n\t"
                        "v_cvt_u32_f32_sdwa %1, %13 dst_sel:BYTE_2 dst_unused:UNUSED_PRESERVE src0_sel:DWORD\n\t"
                        "v_cvt_u32_f32_sdwa %2, %14 dst_sel:BYTE_2 dst_unused:UNUSED_PRESERVE src0_sel:DWORD\n\t"
                        "v_cvt_u32_f32_sdwa %3, %15 dst_sel:BYTE_2 dst_unused:UNUSED_PRESERVE src0_sel:DWORD\n\t"
                        "v_cvt_u32_f32_sdwa %0, %16 dst_sel:BYTE_3 dst_unused:UNUSED_PRESERVE src0_sel:DWORD\n\t"
                        "v_cvt_u32_f32_sdwa %1, %17 dst_sel:BYTE_3 dst_unused:UNUSED_PRESERVE src0_sel:DWORD\n\t"
                        "v_cvt_u32_f32_sdwa %2, %18 dst_sel:BYTE_3 dst_unused:UNUSED_PRESERVE src0_sel:DWORD\n\t"
                        "v_cvt_u32_f32_sdwa %3, %19 dst_sel:BYTE_3 dst_unused:UNUSED_PRESERVE src0_sel:DWORD\n\t"
                        "s_nop 0"
                        : "=&v"(w0), "=&v"(w1), "=&v"(w2), "=&v"(w3)
                        : "v"(pf[0][0]), "v"(pf[1][0]), "v"(pf[2][0]), "v"(pf[3][0]), "v"(pf[0][1]), "v"(pf[1][1]), "v"(pf[2][1]), "v"(pf[3][1]),
                          "v"(pf[0][2]), "v"(pf[1][2]), "v"(pf[2][2]), "v"(pf[3][2]), "v"(pf[0][3]), "v"(pf[1][3]), "v"(pf[2][3]), "v"(pf[3][3]));
                } else if (4 * ks < NKT) {      // the last key step: one key tile (13 = 3 x 4 + 1), a chain on one register
                    static_assert(NKT % 4 == 1, "the tail key step packs exactly one key tile");
                    asm("v_cvt_u32_f32_sdwa %0, %1 dst_sel:BYTE_0 dst_unused:UNUSED_PAD src0_sel:DWORD\n\ts_nop 0\n\t"
                        "v_cvt_u32_f32_sdwa %0, %2 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD\n\ts_nop 0\n\t"
                        "v_cvt_u32_f32_sdwa %0, %3 dst_sel:BYTE_2 dst_unused:UNUSED_PRESERVE src0_sel:DWORD\n\ts_nop 0\n\t"
                        "v_cvt_u32_f32_sdwa %0, %4 dst_sel:BYTE_3 dst_unused:UNUSED_PRESERVE src0_sel:DWORD\n\ts_nop 0"
                        : "=&v"(w0)
                        : "v"(pf[0][0]), "v"(pf[0][1]), "v"(pf[0][2]), "v"(pf[0][3]));
                }
                pk[ks] = v4i{(int)w0, (int)w1, (int)w2, (int)w3};
            }
        } else
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                unsigned w = 0;
                if constexpr (HI_PLANE) pkh[ks][t] = 0;
                if constexpr (PB == 16) pkb[ks][t] = 0;
                if (4 * ks + t < NKT) {
                    unsigned p[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float ev = __int_as_float(s[4 * ks + t][r]);
                        if constexpr (MODE >= 3) {
                            p[r] = (unsigned)(ev * factor_h);
                            any_u |= p[r];
                        } else if (IVIT_LAB && (a.abl & 4)) {
                            p[r] = (unsigned)s[4 * ks + t][r];
                        } else {
                            p[r] = (unsigned)(ev * factor);  // float32 product (:175), < 2^31
                        }
                    }
                    if constexpr (PB == 16) {
                        // planes c and b of p16 (attn_parts.h plane_c, plane_b): this kernel keeps its own copy, the helpers reorder
                        // the schedule of the natural-scale forms
                        if constexpr (MODE < 3) any_u |= p[0] | p[1] | p[2] | p[3];
                        const unsigned c4 = __builtin_amdgcn_perm(p[1], p[0], 0x0c0c0602u) | __builtin_amdgcn_perm(p[3], p[2], 0x06020c0cu);
                        const unsigned b4 = __builtin_amdgcn_perm(p[1] << 1, p[0] << 1, 0x0c0c0703u) |
                                            __builtin_amdgcn_perm(p[3] << 1, p[2] << 1, 0x07030c0cu);
                        w = c4 & 0x7f7f7f7fu;
                        pkb[ks][t] = (int)(b4 & 0x7f7f7f7fu);
                    } else {
                        w = top_bytes(p);
                    }
                }
                pk[ks][t] = (int)w;
            }
        const bool any_hi = HI_PLANE &&
                            __builtin_amdgcn_ballot_w64((any_u >> (PB == 16 ? 30 : 31)) != 0) != 0;   // wave-uniform, almost never
        if constexpr (PB == 16) {
            if (any_hi) {      // plane a (bits 30, 31 of u: p16 >= 16384) from the products again
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        unsigned w = 0;
                        if (4 * ks + t < NKT) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const float ev = __int_as_float(s[4 * ks + t][r]);
                                const unsigned u = (unsigned)(ev * (MODE >= 3 ? factor_h : factor));
                                w |= plane_a_byte(u, r);
                            }
                        }
                        pkh[ks][t] = (int)w;
                    }
            }
        } else if constexpr (MODE >= 3 && PB == 8) {
            if (any_hi) {      // p = 128 = 127 in pk + 1 in pkh (split_p128)
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        unsigned lo, hi;
                        split_p128((unsigned)pk[ks][t], lo, hi);
                        pk[ks][t] = (int)lo;
                        pkh[ks][t] = (int)hi;
                    }
            }
        }

        const bool hi_pass = any_hi;
        qf_next = *reinterpret_cast<const v4i*>(qg + (int64_t)min((qt + 4 * a.parts) * 16 + l15, T - 1) * HD + 16 * g);
        // ---- O^T = Vt . P^T, requantised (attn.qact2), 4 consecutive d per dword
        const int64_t orow_idx = (int64_t)b * T + qrow;
        const BlockRow obrow = block_row((int)orow_idx, a.heads * HD);
        int8_t* orow = a.out + orow_idx * ((int64_t)a.heads * HD) + hh * HD;
        if (IVIT_LAB && (a.abl & 8)) {
            if (pk[0][0] == 0x12345678) a.out[0] = 1;
            continue;
        }
        unsigned wq[4];    // wq[dt]: bytes d = 16 dt + 4 g + 0..3 of this lane's query
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            v4i acc = {0, 0, 0, 0};
            v4i accb = {0, 0, 0, 0}, acca = {0, 0, 0, 0};
            const int d = 16 * dt + l15;
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                const v4i vf = *reinterpret_cast<const v4i*>(smem + K_BYTES + d * VT_ROW + (((4 * ks + g) ^ (d & 15)) << 4));
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(vf, pk[ks], acc, 0, 0, 0);
                if constexpr (PB == 16) {
                    accb = __builtin_amdgcn_mfma_i32_16x16x64_i8(vf, pkb[ks], accb, 0, 0, 0);
                    if (hi_pass) acca = __builtin_amdgcn_mfma_i32_16x16x64_i8(vf, pkh[ks], acca, 0, 0, 0);
                } else if constexpr (MODE >= 3 && PB == 8) {
                    if (hi_pass) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(vf, pkh[ks], acc, 0, 0, 0);
                }
            }
            wq[dt] = attn_out_word<PB>(acc, accb, acca, a.Mo);
        }
        // lane g ends with the 16 contiguous bytes d = 16 g .. 16 g + 15 of its query (attn_out_transpose): one 16-byte store
        {
            const v4i chunk = attn_out_transpose(wq);
            if (qrow < T) {
                if (a.out_blocks)   // column = 64 hh + 16 g: chunk index g, column block hh
                    *reinterpret_cast<v4i*>(a.out + obrow.base + (unsigned)hh * 1024u + (((unsigned)g ^ obrow.rs) << 4)) = chunk;
                else
                    *reinterpret_cast<v4i*>(orow + 16 * g) = chunk;
            }
        }
    }
}

// Workgroups per (image, head).  Every workgroup stages K and V^T of its head in LDS (~3 us) and walks query tiles (13 at
// T = 197: 4 per wave, ~3.5 us each); `slots` workgroups are resident at once.  With batch * heads a multiple of the slots one
// workgroup per head is right (DeiT-B b256: 3072 = 3 rounds of 1024; 4 of 768 before round 3); a launch that fills only part of a round is bound by that
// walk -- DeiT-S b64 (384 heads) took a whole round's 17 us -- so the tiles are dealt out among 2 or 4 workgroups per head when
// the model below says the launch gets shorter (each stages K / V^T itself: L2 hits).
// The long kernel is the same model with one workgroup per CU (256 slots) and `waves` waves walking the tiles, staging and a query
// tile both growing with T alike.
int attention_parts(int batch_heads, int nqt, int waves, int slots)
{
    int best = 1;
    double best_t = 0.0;
    for (int p = 1; p <= 4; p *= 2) {
        if (p > 1 && waves * (p / 2) >= nqt) break;     // no wave would lose a tile
        const int rounds = (batch_heads * p + slots - 1) / slots, tiles = (nqt + waves * p - 1) / (waves * p);
        const double t = rounds * (3.0 + 3.45 * tiles);
        if (p == 1 || t < 0.95 * best_t) { best = p; best_t = t; }
    }
    return best;
}

// ---- long rows: 208 <= T <= 1025 tokens (384 / 16 -> 577, 224 / 8 -> 785, 512 / 16 -> 1025)
// The same arithmetic as attention_kernel MODE 0 / 1 / 2 with PB = 8, but a row no longer fits 13 x 4 int registers.  After the
// requantisation a score is one byte: k + 128 in [0, 255], and a lane keeps its four keys of a key tile packed in ONE dword
// (sc[kt], byte r = key 16 kt + 4 g + r): a 1025-key row is 65 dwords in each of its four lanes.  Three passes over those registers:
//   1. S^T tile = K . Q^T (one 16x16x64 MFMA per key tile), requantised, packed; row max over the packed bytes' sources
//   2. idx = max - k for four keys at once (the row max replicated into every byte: no byte borrows), exp_int from the
//      table, exact row sum: 16 exponents (<= 16 * 2^27) in u32, then u64 (1025 * 255 * 2^15 exceeds 2^32)
//   3. the exponents again from idx, 8-bit probabilities, P . V per key step of 64 (attention_kernel's operand orders)
// K and V^T of one (image, head) sit whole in LDS (150 KiB at 1025 tokens) and are shared by the waves of one workgroup per
// CU (16 waves up to 655 tokens, 12 above: registers), each wave walking query tiles of 16.  V^T rows are padded to a multiple of 256 bytes, so that
// attention_kernel's chunk swizzle j ^ (d & 15) stays inside the row.  MODE 0: power-of-two input scale, exponent table in LDS;
// MODE 1: natural scale, the host's table gathered from global memory (band form when band_w > 0, else the [256][256] exp2d):
// the band rows of every wave do not fit next to K and V^T.
// MODE 2: the I-BERT softmax (attention_kernel MODE 3 / 4 on this row organisation): the float32 (row max, q) table of
// ivit_ibert_softmax_build_table gathered from global memory like MODE 1 (band form when band_w > 0), the row sum in float32 in
// torch's CPU reduction order (rowsum.h), p = floor(fl32(e * floor(2^32 / S)) / 2^25) in [0, 128]; 128 = 127 + 1, the 1 in a
// second P . V operand that is issued only for a key step that holds one.
constexpr int LONG_T_MIN = 208, LONG_T_MAX = 1025;
constexpr int LONG_LUT_BYTES = 2 * 256 * 4;

struct LongArgs {
    const int8_t* qkv;
    int8_t* out;
    int batch, heads, tokens;
    double Ms, Mo;
    float Ms32;                // RQ32: Ms as float32 (a power of two)
    int x0;                    // floor(-1/s_attn)
    int out_blocks;            // output in the GEMM block layout (common.h: ivit_block_offset)
    const unsigned* table;     // MODE 1: band[(qmax + 128) * band_w + j] (band_w > 0) or exp2d[(qmax + 128) * 256 + q + 128]
                               // MODE 2: the same two forms of the I-BERT table, float32 bit patterns
    int band_w;
    int parts;                 // workgroups per (image, head)
    int vt_row;                // bytes per d row of V^T: ceil(key steps / 4) * 256
};

// NKT: full key tiles held in registers (T >> 4 <= NKT); NTH: threads per workgroup, one workgroup per CU (1024: 128 VGPRs, enough
// for 40 tiles; 768: 168 VGPRs, 142-149 used, for 64 tiles)
// PB: width of the Shiftmax output as in attention_kernel: 8, or 16 -- passes 1 and 2 are the same, pass 3 takes
// p16 = floor(fl32(e * factor) / 2^16) in [0, 2^15] as three 7-bit planes p = c + 128 b + 16384 a with one P . V accumulator set
// each (the a plane only for a key step in which a wave holds such a probability), and the output is requantised in the
// reference's two steps.  The two further accumulator sets are 32 registers: 40 tiles in the 12-wave form, 64 in an 8-wave one
// (512 threads: 256 VGPRs).
template <int MODE, bool RQ32, int NKT, int NTH, int PB = 8>
__global__ __launch_bounds__(NTH, 1) void attention_long_kernel(LongArgs a)
{
    static_assert(!RQ32 || MODE != 1, "RQ32: a power-of-two score multiplier (Shiftmax: power-of-two input scale)");
    static_assert(PB == 8 || ((PB == 16 || PB == 4) && MODE != 2), "4- and 16-bit probabilities: Shiftmax only");
    constexpr int NKS = NKT / 4 + 1;          // key steps of 64: NKT full key tiles and the partial one
    constexpr int KOFF = RQ32 ? RQ_OFF : 0;    // RQ32: scores carry the magic constant's exponent bits (low byte = k + 128)
    extern __shared__ __attribute__((aligned(16))) char lsm[];
    const int T = a.tokens, nkt = (T + 15) >> 4, nks = (nkt + 3) >> 2;
    const int bh = blockIdx.x / a.parts, part = blockIdx.x - bh * a.parts;
    const int b = bh / a.heads, hh = bh - b * a.heads;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, l15 = lane & 15;
    const int64_t plane = (int64_t)a.batch * a.heads * T * HD;
    const int8_t* qg = a.qkv + (int64_t)bh * T * HD;
    const int8_t* kg = qg + plane;
    const int8_t* vg = qg + 2 * plane;
    unsigned* lut = reinterpret_cast<unsigned*>(lsm);                 // [256] u32 exponent, [256] the same as float32
    char* ksm = lsm + LONG_LUT_BYTES;                                  // K image, nkt * 16 rows of 64 bytes (kswz)
    char* vt = ksm + nkt * 16 * HD;                                    // V^T, 64 rows of vt_row bytes
    const int vt_row = a.vt_row;

    if (MODE == 0 && tid < 256) {
        const unsigned e0 = shiftexp_int(-tid, a.x0, 15);
        lut[tid] = e0;
        reinterpret_cast<float*>(lut)[256 + tid] = (float)e0;
    }
    // ---- K: 4 T chunks of 16 bytes, all requested before the first is written (as attention_kernel)
    constexpr int NW = NTH / 64;
    constexpr int KI = (4 * LONG_T_MAX + NTH - 1) / NTH;
    v4i kst[KI];
#pragma unroll
    for (int i = 0; i < KI; ++i) {
        const int q = min(tid + NTH * i, 4 * T - 1);
        kst[i] = *reinterpret_cast<const v4i*>(kg + (int64_t)(q >> 2) * HD + 16 * (q & 3));
    }
    // ---- V^T: work item = 4 consecutive keys x 16 d, transposed in registers, written as dwords (attention_kernel's layout:
    //      chunk j = 4 s + g' of row d holds keys 64 s + 16 t + 4 g' + r at byte 4 t + r, stored at chunk position j ^ (d & 15))
    constexpr int VI = (((LONG_T_MAX + 3) / 4) * 4 + NTH - 1) / NTH;
    const int nvi = ((T + 3) >> 2) * 4;
    v4i vst[VI][4];
#pragma unroll
    for (int i = 0; i < VI; ++i) {
        const int q = min(tid + NTH * i, nvi - 1);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            vst[i][r] = *reinterpret_cast<const v4i*>(vg + (int64_t)min(4 * (q >> 2) + r, T - 1) * HD + 16 * (q & 3));
    }
#pragma unroll
    for (int i = 0; i < KI; ++i) {
        const int q = tid + NTH * i;
        if (q < 4 * T) *reinterpret_cast<v4i*>(ksm + kswz(q >> 2, q & 3)) = kst[i];
    }
#pragma unroll
    for (int i = 0; i < VI; ++i) {
        const int q = tid + NTH * i;
        if (q >= nvi) continue;
        const int key0 = 4 * (q >> 2), c = q & 3;
        const int j = 4 * (key0 >> 6) + ((key0 >> 2) & 3);
        const int boff = 4 * ((key0 >> 4) & 3);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const unsigned a0 = (unsigned)vst[i][0][w], a1 = (unsigned)vst[i][1][w], a2 = (unsigned)vst[i][2][w], a3 = (unsigned)vst[i][3][w];
            unsigned t[4];
            bytes4x4_transpose(a0, a1, a2, a3, t);
#pragma unroll
            for (int bb = 0; bb < 4; ++bb) {
                const int d = 16 * c + 4 * w + bb;
                *reinterpret_cast<unsigned*>(vt + d * vt_row + ((j ^ (d & 15)) << 4) + boff) = t[bb];
            }
        }
    }
    __syncthreads();

    const float* lutf = reinterpret_cast<const float*>(lut) + 256;
    // the full key tiles live in sc[]; the partial one (T % 16 != 0: tile nfull, the only one with padding keys) in its own register,
    // so that no unrolled tile carries a padding test.  Its key 16 nfull + 4 g + r is real for r < vr.
    const int nfull = T >> 4, vr = T - 16 * nfull - 4 * g;
    const bool partial = (T & 15) != 0;
    const int W = a.band_w;
    for (int qt = part * NW + wave; qt < nkt; qt += NW * a.parts) {
        const int qrow = qt * 16 + l15;
        const v4i qf = *reinterpret_cast<const v4i*>(qg + (int64_t)min(qrow, T - 1) * HD + 16 * g);
        int nf = nfull;
        asm volatile("" : "+s"(nf));   // opaque per query tile: the per-tile tests are not hoisted out as live masks (SGPR spills)

        // ---- pass 1: scores, requantised (qact_attn1) to u = k + 128 (+ KOFF), packed four to a dword
        int umax = KOFF;
        auto score_tile = [&](int kt, int nreal) -> unsigned {
            const v4i kf = *reinterpret_cast<const v4i*>(ksm + kswz(16 * kt + l15, g));
            v4i acc = {0, 0, 0, 0};
            acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(kf, qf, acc, 0, 0, 0);
            int u[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if constexpr (RQ32)    // RNE(S * Ms) + 128 in the low byte: exact, one rounding (see attention_kernel RQ32)
                    u[r] = clamp_i32(__float_as_int(__builtin_fmaf((float)acc[r], a.Ms32, 12583040.0f)), KOFF, KOFF + 255);
                else
                    u[r] = clamp_i32(requant_exact(acc[r], a.Ms), -128, 127) + 128;
                u[r] = r < nreal ? u[r] : KOFF;    // padding keys: byte 0, never the maximum; their exponent is masked below
            }
            umax = max(umax, max(max(u[0], u[1]), max(u[2], u[3])));
            return __builtin_amdgcn_perm((unsigned)u[1], (unsigned)u[0], 0x0c0c0400u) |
                   __builtin_amdgcn_perm((unsigned)u[3], (unsigned)u[2], 0x04000c0cu);
        };
        unsigned sc[NKT];
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            if (kt < nf) sc[kt] = score_tile(kt, 4);    // uniform test; the loop stays unrolled (sc[] in registers)
            if ((kt & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // at most 4 K fragments in flight
        }
        const unsigned sl = partial ? score_tile(nf, vr) : 0u;
        umax = rows_allmax_i32(umax) & 255;    // qmax + 128
        const unsigned rep = (unsigned)umax * 0x01010101u;

        // exp_int of a key from idx = qmax - k in [0, 255] (and k + 128 = umax - idx)
        const unsigned* trow = MODE != 0 ? a.table + (W ? umax * W : umax * 257) : nullptr;
        auto expo = [&](unsigned idx) -> unsigned {
            if constexpr (MODE == 0) return lut[idx];
            else return W ? trow[min((int)idx, W - 1)] : trow[-(int)idx];
        };

        // ---- the row's float32 sum in torch's order (rowsum.h torch_rowsum; attention_kernel MODE 3 is the same for T < 208): what
        // IBERTIntSoftmax's e.sum() is for every row, and Shiftmax's exp_int.sum() for the rows whose exact sum reaches 2^24
        // (attn_parts.h SHIFTMAX_ORDER_SUM).  V = T >> 3 vectors of 8, I = V >> 2 = T >> 5 interleaved steps of 32 keys: partial
        // j = key % 32 takes keys j + 32 i, i < I, in groups of 16 steps (each group summed from zero, the group sums added up, the
        // remainder's sum added last); I <= 32, so the cascade never passes its second level.  With key = 16 kt + 4 g + r a lane owns
        // the whole sequence of its eight partials (hi = kt & 1, r), step kt >> 1: key tiles 0 .. 2 I - 1.  The at most 31 keys behind
        // them (key tiles 2 I and 2 I + 1) go to torch_rowsum_finish (attn_parts.h) together with the partials.  Padding keys and
        // absent tiles are +0.0f, which changes no sum of non-negative terms: the selections below are by value.
        auto expf_of = [&](unsigned idx) -> float {
            if constexpr (MODE == 0) return lutf[idx];
            else if constexpr (MODE == 2) return __int_as_float((int)expo(idx));
            else return (float)expo(idx);
        };
        auto torch_order_sum = [&]() -> float {
            int I2 = (T >> 5) << 1;                    // key tiles of the interleaved part; nf is I2 or I2 + 1
            asm volatile("" : "+s"(I2));               // opaque per query tile, as nf: no hoisted masks
            float p0[2][4], p1[2][4], t0[4], t1[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) p0[0][r] = p0[1][r] = p1[0][r] = p1[1][r] = t0[r] = t1[r] = 0.0f;
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt) {
                if (kt < nf) {
                    const unsigned dk = rep - sc[kt];
                    float e[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) e[r] = expf_of((dk >> (8 * r)) & 255u);
                    if (kt < I2) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            p0[kt & 1][r] += e[r];
                            if (((kt >> 1) & 15) == 15) {      // a full group of 16 steps ends here
                                p1[kt & 1][r] += p0[kt & 1][r];
                                p0[kt & 1][r] = 0.0f;
                            }
                        }
                    } else if (kt == I2) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) t0[r] = e[r];
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r) t1[r] = e[r];
                    }
                }
            }
            if (partial) {
                const unsigned dk = rep - sl;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float e = r < vr ? expf_of((dk >> (8 * r)) & 255u) : 0.0f;
                    if (nf == I2) t0[r] = e;
                    else t1[r] = e;
                }
            }
            float P[2][4];
#pragma unroll
            for (int hi = 0; hi < 2; ++hi)
#pragma unroll
                for (int r = 0; r < 4; ++r) P[hi][r] = p0[hi][r] + p1[hi][r];      // the remainder's sum plus the groups' total
            return torch_rowsum_finish(P, t0, t1, T);
        };
        float factor;
        if constexpr (MODE == 2) {
            const float fin = torch_order_sum();        // ---- pass 2 (I-BERT): S = e.sum() (ibert_modules.py:311)
            factor = floorf(4294967296.0f / fin) * 0.5f;     // ibert_modules.py:313; the half: see prob_word
        } else {
            // ---- pass 2: Shiftmax row sum (ivit_modules.py:171): the exact integer sum; in torch's order where it reaches 2^24
            unsigned long long esum = 0;
            unsigned sum16 = 0;
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt) {
                if (kt < nf) {
                    const unsigned dk = rep - sc[kt];  // bytes: idx of the four keys (every k <= qmax: no borrow)
#pragma unroll
                    for (int r = 0; r < 4; ++r) sum16 += expo((dk >> (8 * r)) & 255u);
                }
                if ((kt & 3) == 3) {
                    esum += sum16;
                    sum16 = 0;
                }
            }
            if (partial) {
                const unsigned dk = rep - sl;
#pragma unroll
                for (int r = 0; r < 4; ++r) sum16 += r < vr ? expo((dk >> (8 * r)) & 255u) : 0u;
            }
            const unsigned long long tot = rows_allsum_u64(esum + sum16);
            factor = shiftmax_factor(tot);
            if (__builtin_amdgcn_ballot_w64(tot >= SHIFTMAX_ORDER_SUM) != 0) {      // wave-uniform, rare: some row of the tile
                const float S = torch_order_sum();
                factor = tot >= SHIFTMAX_ORDER_SUM ? shiftmax_factor(S) : factor;
            }
            if constexpr (PB == 4) factor *= 0.0625f;    // p = floor(fl32(e * factor) / 2^28) < 8: an exact scaling, as in attention_kernel
        }

        // ---- pass 3: p = floor(fl32(e * factor) / 2^24) (:175) as bytes, P . V per key step of 64
        // I-BERT: p = floor(fl32(e * factor) / 2^25) in [0, 128] (ibert_modules.py:314).  factor / 2 is an exact scaling, so
        // trunc(e * (factor / 2)) has p in its top byte as well; p = 128 is the byte 0x80, split below.
        auto prob_word = [&](unsigned packed, int nreal) -> unsigned {
            const unsigned dk = rep - packed;
            unsigned p[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned idx = (dk >> (8 * r)) & 255u;
                const float ev = MODE == 0 ? lutf[idx] : MODE == 2 ? __int_as_float((int)expo(idx)) : (float)expo(idx);
                p[r] = r < nreal ? (unsigned)(ev * factor) : 0u;          // float32 product (:175), < 2^31
            }
            return top_bytes(p);
        };
        // PB 16: the planes c and b of p16 = u >> 16 (plane_c, plane_b).  -> the OR of the four u (whether plane a is needed)
        auto prob_planes = [&](unsigned packed, int nreal, unsigned& wc, unsigned& wb) -> unsigned {
            const unsigned dk = rep - packed;
            unsigned p[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned idx = (dk >> (8 * r)) & 255u;
                const float ev = MODE == 0 ? lutf[idx] : (float)expo(idx);
                p[r] = r < nreal ? (unsigned)(ev * factor) : 0u;
            }
            wc = plane_c(p);
            wb = plane_b(p);
            return p[0] | p[1] | p[2] | p[3];
        };
        auto prob_plane_a = [&](unsigned packed, int nreal) -> unsigned {      // from the products again: rare
            const unsigned dk = rep - packed;
            unsigned w = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned idx = (dk >> (8 * r)) & 255u;
                const float ev = MODE == 0 ? lutf[idx] : (float)expo(idx);
                const unsigned u = r < nreal ? (unsigned)(ev * factor) : 0u;
                w |= plane_a_byte(u, r);
            }
            return w;
        };
        unsigned wl = 0u, wlb = 0u, ul = 0u;       // the partial tile's words (PB 16: planes c and b, and the OR of its u)
        if constexpr (PB == 16) {
            if (partial) ul = prob_planes(sl, vr, wl, wlb);
        } else {
            wl = partial ? prob_word(sl, vr) : 0u;
        }
        // PB 16: three accumulator sets, O = o + (o_b << 7) + (o_a << 14) = sum p16 * v.  Bounds for T <= 1025 keys, |v| <= 128:
        //   S not clamped: factor <= 2^31 / S, so the row's p16 sum to at most 2^15 (+ the float32 roundings) and |O| <= 2^22 for any T;
        //   S clamped at 2^31 (:173): factor = 1, p16 = e >> 16 with e <= 2 |x0| 2^14 <= 2^27 (x0 >= -4096), i.e. p16 <= 2^11 per key
        //   and |O| <= 1025 * 2^11 * 128 = 1025 * 2^18 < 2^28.01.
        // Every plane term is bounded by the same sum: c, 128 b and 16384 a are each <= p16, so |o|, |o_b << 7| and |o_a << 14| are
        // each <= 128 * sum p16 <= 1025 * 2^18, the accumulators themselves |o|, |o_b| <= 1025 * 127 * 128 < 2^24 and |o_a| <=
        // 1025 * 2 * 128 < 2^19, and any partial sum of the three terms is below 3 * 2^28.01 < 2^30: all in int32.
        v4i o[4];
        v4i o_b[PB == 16 ? 4 : 1], o_a[PB == 16 ? 4 : 1];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] = v4i{0, 0, 0, 0};
        if constexpr (PB == 16) {
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) o_b[dt] = o_a[dt] = v4i{0, 0, 0, 0};
        }
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            if (ks >= nks) continue;
            if constexpr (PB == 16) {
                v4i pc, pb;
                unsigned any_u = 0;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int kt = 4 * ks + t;
                    unsigned wc = kt == nf ? wl : 0u, wb = kt == nf ? wlb : 0u;
                    any_u |= kt == nf ? ul : 0u;
                    if (kt < NKT && kt < nf) any_u |= prob_planes(sc[kt < NKT ? kt : 0], 4, wc, wb);
                    pc[t] = (int)wc;
                    pb[t] = (int)wb;
                }
                const bool hi_pass = __builtin_amdgcn_ballot_w64((any_u >> 30) != 0) != 0;      // wave-uniform, rare
                v4i pa = {0, 0, 0, 0};
                if (hi_pass) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int kt = 4 * ks + t;
                        unsigned w = (partial && kt == nf) ? prob_plane_a(sl, vr) : 0u;
                        if (kt < NKT && kt < nf) w = prob_plane_a(sc[kt < NKT ? kt : 0], 4);
                        pa[t] = (int)w;
                    }
                }
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    const int d = 16 * dt + l15;
                    const v4i vf = *reinterpret_cast<const v4i*>(vt + d * vt_row + (((4 * ks + g) ^ (d & 15)) << 4));
                    o[dt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(vf, pc, o[dt], 0, 0, 0);
                    o_b[dt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(vf, pb, o_b[dt], 0, 0, 0);
                    if (hi_pass) o_a[dt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(vf, pa, o_a[dt], 0, 0, 0);
                }
                continue;
            }
            v4i pk;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int kt = 4 * ks + t;
                unsigned w = kt == nf ? wl : 0u;
                if (kt < NKT && kt < nf) w = prob_word(sc[kt < NKT ? kt : 0], 4);
                pk[t] = (int)w;
            }
            v4i ph = {0, 0, 0, 0};
            bool hi_pass = false;
            if constexpr (MODE == 2) {             // p = 128: split_p128
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    unsigned lo, hi;
                    split_p128((unsigned)pk[t], lo, hi);
                    pk[t] = (int)lo;
                    ph[t] = (int)hi;
                }
                hi_pass = __builtin_amdgcn_ballot_w64((ph[0] | ph[1] | ph[2] | ph[3]) != 0) != 0;    // wave-uniform, rare
            }
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const int d = 16 * dt + l15;
                const v4i vf = *reinterpret_cast<const v4i*>(vt + d * vt_row + (((4 * ks + g) ^ (d & 15)) << 4));
                o[dt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(vf, pk, o[dt], 0, 0, 0);
                if constexpr (MODE == 2) {
                    if (hi_pass) o[dt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(vf, ph, o[dt], 0, 0, 0);
                }
            }
        }

        // ---- O^T requantised (qact2): |O| <= 1025 * 127 * 128 < 2^24, the float64 product is exact
        unsigned wq[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            int ob[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                ob[r] = attn_out_requant<PB>(o[dt][r], PB == 16 ? o_b[PB == 16 ? dt : 0][r] : 0, PB == 16 ? o_a[PB == 16 ? dt : 0][r] : 0, a.Mo);
            }
            wq[dt] = low_bytes(ob);
        }
        // lane g ends with bytes d = 16 g .. 16 g + 15 of its query
        const v4i chunk = attn_out_transpose(wq);
        if (qrow < T) {
            const int64_t orow_idx = (int64_t)b * T + qrow;
            if (a.out_blocks) {
                const BlockRow obrow = block_row((int)orow_idx, a.heads * HD);
                *reinterpret_cast<v4i*>(a.out + obrow.base + (unsigned)hh * 1024u + (((unsigned)g ^ obrow.rs) << 4)) = chunk;
            } else {
                *reinterpret_cast<v4i*>(a.out + orow_idx * ((int64_t)a.heads * HD) + hh * HD + 16 * g) = chunk;
            }
        }
    }
}

// ---- one query per (image, head): the class row of the last block, the only row of its output the classifier reads
// (vit_quant.py:302-304).  attention_kernel's arithmetic for that query -- score requantisation, row maximum over the T real keys,
// exponent from the 256-entry table (MODE 0) or from the host's band / [256][256] table (MODE 1 / 2), exact u32 sum, float32
// factor, p = floor(fl32(e * factor) / 2^24), P.V in int32, output requantisation -- without MFMAs: the work is reading 25 KB of
// K and V once.  One wave per (image, head).  K and V are walked as 16-byte chunks, chunk c = lane + 64 i (c >> 2 = key, c & 3 =
// quarter of the head dimension): every load instruction reads 1 KB contiguous, and the 2 x 13 loads are written ahead of the
// first use of any of them so that the compiler may have them all in flight (it keeps all 104 dwords in registers: no scratch,
// csrc/check_resources.py; their order in the instruction stream is the compiler's).
// A lane's four v_dot4 give a quarter of a score, two quad DPP adds leave the score of key (lane >> 2) + 16 i in all four lanes of
// the quad -- the same lanes that hold that key's V chunks, so the probability needs no exchange: 16 int32 accumulators per lane
// (d = 16 (lane & 3) + j), reduced over the 16 lanes of equal lane & 3 at the end.
// The scores are requantised in float64 for every multiplier: for a power-of-two one that is what attention_kernel's float32 form
// computes (its proof is that equality), and 13 v_fma_f64 per lane are not what this kernel waits for.
struct ClsArgs {
    const int8_t *k, *v, *q;     // k, v: [batch][heads][tokens][64] planes; q: [batch][heads * 64]
    int8_t* out;                 // [batch][ldo], heads * 64 bytes per row
    int64_t ldo;
    int pairs, heads, tokens;    // pairs = batch * heads
    double Ms, Mo;
    int x0;
    const unsigned* exp2d;       // as AttnArgs
    const unsigned* band;
    int band_w;
};

constexpr int CLS_NCH = (KP * 4 + 63) / 64;      // 13 chunks of K (and of V) per lane
// CLS_OCC: the occupancy the kernel is compiled for.  3 workgroups per CU is what one round of DeiT-B at batch 256 needs (3072
// pairs = 768 workgroups on 256 CUs) and leaves 168 VGPRs; the compiler uses 118-124, so 4 are resident where a launch has them.
// Measured at that shape, kernel trace of the bench command, 100 replays each: compiled for 2 / 3 / 4 the kernel takes
// 13.92 / 13.88 / 13.85 us (116-118, 118-124, 122-126 VGPRs: four fit per CU each time), spread of one build 13.5-14.6 us.  The
// value does not matter there; 3 stays because it is the round the launcher counts on.
constexpr int CLS_WAVES = NT / 64, CLS_OCC = 3;

template <int MODE>
__global__ __launch_bounds__(NT, CLS_OCC) void attention_cls_kernel(ClsArgs a)
{
    __shared__ unsigned lut[256];
    __shared__ float order_row[CLS_WAVES][KP];      // a row whose sum reaches 2^24 (below)
    const int tid = threadIdx.x, lane = tid & 63;
    if constexpr (MODE == 0) {
        lut[tid] = shiftexp_int(-tid, a.x0, 15);
        __syncthreads();
    }
    const int bh = blockIdx.x * CLS_WAVES + (tid >> 6);
    if (bh >= a.pairs) return;
    const int b = bh / a.heads, hh = bh - b * a.heads;
    const int T = a.tokens, c4 = lane & 3;
    const int8_t* kg = a.k + (int64_t)bh * T * HD;
    const int8_t* vg = a.v + (int64_t)bh * T * HD;

    v4i kc[CLS_NCH], vc[CLS_NCH];
#pragma unroll
    for (int i = 0; i < CLS_NCH; ++i)
        kc[i] = *reinterpret_cast<const v4i*>(kg + 16 * min(lane + 64 * i, 4 * T - 1));       // unconditional, clamped
    const v4i qf = *reinterpret_cast<const v4i*>(a.q + ((int64_t)b * a.heads + hh) * HD + 16 * c4);
#pragma unroll
    for (int i = 0; i < CLS_NCH; ++i)
        vc[i] = *reinterpret_cast<const v4i*>(vg + 16 * min(lane + 64 * i, 4 * T - 1));

    // ---- scores, negated like attention_kernel's: nk = -k = RNE(S * -Ms) in [-127, 128]; keys >= T carry the sentinel
    int nk[CLS_NCH];
    int nmin = 1000;
#pragma unroll
    for (int i = 0; i < CLS_NCH; ++i) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) s = __builtin_amdgcn_sdot4(kc[i][w], qf[w], s, false);
        s += (int)IVIT_DPP_U32(s, 0xB1);
        s += (int)IVIT_DPP_U32(s, 0x4E);
        const int n = clamp_i32(requant_exact(s, -a.Ms), -127, 128);       // |S| <= 2^20: exact float64 product
        nk[i] = ((lane >> 2) + 16 * i < T) ? n : 1000;
        nmin = min(nmin, nk[i]);
    }
    const int rmax = wave_allmax_i32(-nmin);

    // ---- Shiftmax (ivit_modules.py:164-175)
    unsigned ev[CLS_NCH], esum = 0;
#pragma unroll
    for (int i = 0; i < CLS_NCH; ++i) {
        const int idx = min(nk[i] + rmax, 255);       // max - k in [0, 255] for a real key
        unsigned e;
        if constexpr (MODE == 0) e = lut[idx];
        else if constexpr (MODE == 1) e = a.band[(size_t)(rmax + 128) * a.band_w + min(idx, a.band_w - 1)];
        else e = a.exp2d[((rmax + 128) << 8) + 128 - min(nk[i], 128)];      // entry of q = -nk
        e = nk[i] == 1000 ? 0u : e;
        ev[i] = e;
        esum += c4 == 0 ? e : 0u;                     // the four lanes of a quad hold the same key
    }
    esum = (unsigned)lanes_allsum_i32<64>((int)esum);
    float factor = shiftmax_factor(esum);
    if (esum >= SHIFTMAX_ORDER_SUM) {      // wave-uniform, rare: the float32 sum in torch's order (attn_parts.h), the row passed through LDS
        float* erow = order_row[tid >> 6];
#pragma unroll
        for (int i = 0; i < CLS_NCH; ++i)
            if (c4 == 0) erow[(lane >> 2) + 16 * i] = (float)ev[i];      // key < KP; 0 for a padding key
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        factor = shiftmax_factor(torch_rowsum([&](int i) { return erow[i]; }, T, lane));
    }

    // ---- O = P . V over this lane's chunks
    int acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0;
#pragma unroll
    for (int i = 0; i < CLS_NCH; ++i) {
        const int p = (int)((unsigned)((float)ev[i] * factor) >> 24);      // float32 product (:175), <= 2^31; 0 for a padding key
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] += p * (int)(int8_t)((unsigned)vc[i][j >> 2] >> (8 * (j & 3)));
    }
    // sum over the 16 lanes of equal lane & 3: rotations by 4 and 8 inside a row of 16, then the rows
    int ob[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        int t = acc[j];
        t += (int)IVIT_DPP_U32(t, 0x124);      // row_ror:4
        t += (int)IVIT_DPP_U32(t, 0x128);      // row_ror:8
        const v2u r = __builtin_amdgcn_permlane16_swap((unsigned)t, (unsigned)t, false, false);
        t = (int)(r.x + r.y);
        const v2u q = __builtin_amdgcn_permlane32_swap((unsigned)t, (unsigned)t, false, false);
        t = (int)(q.x + q.y);
        ob[j] = clamp_i32(requant_exact(t, a.Mo), -128, 127);      // |O| <= 208 * 128 * 128 < 2^22
    }
    if (lane < 4) {
        v4i chunk;
#pragma unroll
        for (int w = 0; w < 4; ++w)
            chunk[w] = (int)(__builtin_amdgcn_perm((unsigned)ob[4 * w + 1], (unsigned)ob[4 * w], 0x0c0c0400u) |
                             __builtin_amdgcn_perm((unsigned)ob[4 * w + 3], (unsigned)ob[4 * w + 2], 0x04000c0cu));
        *reinterpret_cast<v4i*>(a.out + (int64_t)b * a.ldo + hh * HD + 16 * c4) = chunk;
    }
}

// ---- the probabilities themselves: P of the fused kernels above (8-bit softmax output), written to memory instead of multiplied
// with V.  [batch][heads][q_rows][ldp] uint8, row r of an (image, head) = query r over the keys 0 .. tokens - 1; scale 2^-7.
// One workgroup of four waves per (image, head, group of four query tiles); only the tiles that hold one of the first q_rows
// queries are computed (q_rows = 1: the class token's row, one wave).  K is staged once per workgroup (kswz); a wave takes one
// query tile and makes three passes:
//   1. S^T tile = K . Q^T per key tile (v_mfma_i32_16x16x64_i8), requantised (qact_attn1) to the byte u = k + 128, stored in the
//      wave's LDS slice [16 queries][16 * ceil(T / 16) + pad] -- no row lives in registers, so one form serves 1 .. 1025 tokens;
//      the row maximum over the four lanes of a query
//   2. the row sum.  Shiftmax: exact integer sum of exp_int over the lane's own keys, u64 (attention_long_kernel pass 2), then the
//      float32 factor; rows whose sum reaches 2^24 take the I-BERT route below afterwards.  I-BERT: float32 in torch's CPU order by torch_rowsum_half (rowsum.h), two rows at a time, the exponents
//      looked up from the slice's bytes -- the order is the general one, not a lane pattern per token count
//   3. row by row, lane d takes the dword of keys 4 d .. 4 d + 3: exponent again from the table, p = floor(fl32(e * factor) / 2^24)
//      (I-BERT: the halved factor, p in [0, 128]), packed (top_bytes), stored as a dword where every row of probs starts on one,
//      byte by byte otherwise and for the last keys of a row whose length is no multiple of four.  Bytes tokens .. ldp - 1 stay.
// MODE 0: Shiftmax, power-of-two input scale (256-entry table in LDS); 1: Shiftmax, natural scale (band or [256][256] table in
// global memory, as attention_long_kernel MODE 1); 2: I-BERT (its float32 table, band or full).
// LDS at 1025 tokens: 1.5 KB + 65 KB of K + 4 x 16.3 KB of slices = 132 KB.  Wave barriers and one __syncthreads; no scratch
// (csrc/check_resources.py).
struct ProbsArgs {
    const int8_t* qkv;
    uint8_t* probs;
    int64_t ldp;
    int batch, heads, tokens, q_rows;
    double Ms;
    int x0;
    const unsigned* table;     // as LongArgs
    int band_w;
    int groups;                // workgroups per (image, head): ceil(ceil(q_rows / 16) / 4)
    int dwords;                // probs and ldp are multiples of four: packed stores
};

constexpr int PROBS_HEAD_BYTES = 256 * 4 + 2 * 4 * 16 * 4;    // exponent table; row maximum and factor of every wave's 16 queries
constexpr int PROBS_ROW_PAD = 4;                              // bytes: an odd number of dwords per slice row
inline size_t probs_lds_bytes(int tokens)
{
    const int nkt = (tokens + 15) >> 4;
    return (size_t)PROBS_HEAD_BYTES + (size_t)nkt * 16 * HD + (size_t)4 * 16 * (16 * nkt + PROBS_ROW_PAD);
}

template <int MODE>
__global__ __launch_bounds__(NT) void attention_probs_kernel(ProbsArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char psm[];
    const int T = a.tokens, nkt = (T + 15) >> 4, rs = 16 * nkt + PROBS_ROW_PAD;
    const int bh = blockIdx.x / a.groups, grp = blockIdx.x - bh * a.groups;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, l15 = lane & 15;
    const int64_t plane = (int64_t)a.batch * a.heads * T * HD;
    const int8_t* qg = a.qkv + (int64_t)bh * T * HD;
    const int8_t* kg = qg + plane;
    unsigned* lut = reinterpret_cast<unsigned*>(psm);
    int* rowmax = reinterpret_cast<int*>(psm + 1024) + 16 * wave;
    float* rowfac = reinterpret_cast<float*>(psm + 1024 + 256) + 16 * wave;
    char* ksm = psm + PROBS_HEAD_BYTES;                                // K image, nkt * 16 rows of 64 bytes (kswz)
    unsigned char* slice = reinterpret_cast<unsigned char*>(ksm + nkt * 16 * HD) + wave * 16 * rs;

    if constexpr (MODE == 0) lut[tid] = shiftexp_int(-tid, a.x0, 15);
    // ---- K: 4 T chunks of 16 bytes, four per thread requested before the first is written; rows >= T are never consumed unmasked
    for (int q0 = tid; q0 < 4 * T; q0 += 4 * NT) {
        v4i kst[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = min(q0 + NT * i, 4 * T - 1);
            kst[i] = *reinterpret_cast<const v4i*>(kg + (int64_t)(q >> 2) * HD + 16 * (q & 3));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = q0 + NT * i;
            if (q < 4 * T) *reinterpret_cast<v4i*>(ksm + kswz(q >> 2, q & 3)) = kst[i];
        }
    }
    __syncthreads();
    const int qt = 4 * grp + wave;
    if (16 * qt >= a.q_rows) return;          // no requested row in this wave's tile (the only workgroup barrier is behind it)
    const int nrows = min(16, a.q_rows - 16 * qt);
    const v4i qf = *reinterpret_cast<const v4i*>(qg + (int64_t)min(16 * qt + l15, T - 1) * HD + 16 * g);

    // ---- pass 1: scores, requantised to u = k + 128, four keys to a dword of the slice; padding keys: byte 0, never the maximum
    int umax = 0;
    for (int kt = 0; kt < nkt; ++kt) {
        const v4i kf = *reinterpret_cast<const v4i*>(ksm + kswz(16 * kt + l15, g));
        v4i acc = {0, 0, 0, 0};
        acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(kf, qf, acc, 0, 0, 0);
        int u[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            u[r] = clamp_i32(requant_exact(acc[r], a.Ms), -128, 127) + 128;      // |S| <= 2^20: the float64 product is exact
            u[r] = (16 * kt + 4 * g + r < T) ? u[r] : 0;
            umax = max(umax, u[r]);
        }
        *reinterpret_cast<unsigned*>(slice + l15 * rs + 16 * kt + 4 * g) = low_bytes(u);
    }
    umax = rows_allmax_i32(umax);             // qmax + 128, over the four lanes of the query

    // exp_int of a key from idx = qmax - k in [0, 255], as attention_long_kernel takes it
    const int W = a.band_w;
    auto table_row = [&](int um) -> const unsigned* { return MODE == 0 ? nullptr : a.table + (W ? um * W : um * 257); };
    auto expo = [&](const unsigned* trow, int idx) -> unsigned {
        if constexpr (MODE == 0) return lut[idx];
        else return W ? trow[min(idx, W - 1)] : trow[-idx];
    };

    // ---- pass 2: the row sum and its factor, left in LDS for pass 3 (which walks the rows with all 64 lanes)
    unsigned order_rows = 0;      // Shiftmax: the rows whose exact sum reaches 2^24 (wave-uniform)
    if constexpr (MODE != 2) {
        const unsigned* trow = table_row(umax);
        unsigned long long esum = 0;           // exp_int <= 2^27, 1025 keys: beyond 32 bits
        for (int kt = 0; kt < nkt; ++kt) {
            const unsigned word = *reinterpret_cast<const unsigned*>(slice + l15 * rs + 16 * kt + 4 * g);      // this lane's own store
#pragma unroll
            for (int r = 0; r < 4; ++r)
                esum += (16 * kt + 4 * g + r < T) ? expo(trow, umax - (int)((word >> (8 * r)) & 255u)) : 0u;
        }
        const unsigned long long tot = rows_allsum_u64(esum);
        if (g == 0) rowfac[l15] = shiftmax_factor(tot);
        order_rows = (unsigned)__builtin_amdgcn_ballot_w64(tot >= SHIFTMAX_ORDER_SUM) & 0xffffu;      // bit r: query r of the tile
    }
    if (g == 0) rowmax[l15] = umax;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if constexpr (MODE == 2) {
        // IBERTIntSoftmax: S = e.sum() in float32 in torch's order, factor = floor(2^32 / S) (ibert_modules.py:313); the half: pass 3
        for (int it = 0; 2 * it < nrows; ++it) {
            const int row = 2 * it + (lane >> 5);          // the second row of the last pair may lie behind nrows: computed, not written
            const int um = rowmax[row];
            const unsigned* trow = table_row(um);
            const unsigned char* srow = slice + row * rs;
            const float S = torch_rowsum_half([&](int i) { return __int_as_float((int)expo(trow, um - (int)srow[i])); }, T, lane);
            if ((lane & 31) == 0) rowfac[row] = floorf(4294967296.0f / S) * 0.5f;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else if (order_rows != 0) {
        // Shiftmax rows whose exact sum reaches 2^24: the reference's float32 sum is the one of torch's order (attn_parts.h
        // SHIFTMAX_ORDER_SUM), taken like the I-BERT sum above, a pair of rows at a time; the other rows keep their factor.  Rare.
        for (int it = 0; 2 * it < 16; ++it) {
            if (((order_rows >> (2 * it)) & 3u) == 0) continue;      // uniform
            const int row = 2 * it + (lane >> 5);
            const int um = rowmax[row];
            const unsigned* trow = table_row(um);
            const unsigned char* srow = slice + row * rs;
            const float S = torch_rowsum_half([&](int i) { return (float)expo(trow, um - (int)srow[i]); }, T, lane);
            if ((lane & 31) == 0 && ((order_rows >> row) & 1u)) rowfac[row] = shiftmax_factor(S);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }

    // ---- pass 3: p = floor(fl32(e * factor) / 2^24) (ivit_modules.py:175) = the top byte of the truncated product.  I-BERT:
    // floor(fl32(e * factor) / 2^25) in [0, 128] (ibert_modules.py:314) from the halved factor, an exact scaling
    uint8_t* obase = a.probs + ((int64_t)bh * a.q_rows + 16 * qt) * a.ldp;
    const int nd = (T + 3) >> 2;
    for (int row = 0; row < nrows; ++row) {
        const int um = rowmax[row];
        const float fac = rowfac[row];
        const unsigned* trow = table_row(um);
        const unsigned char* srow = slice + row * rs;
        uint8_t* orow = obase + (int64_t)row * a.ldp;
        for (int d = lane; d < nd; d += 64) {
            const unsigned word = *reinterpret_cast<const unsigned*>(srow + 4 * d);
            unsigned p[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned e = expo(trow, um - (int)((word >> (8 * r)) & 255u));
                const float ev = MODE == 2 ? __int_as_float((int)e) : (float)e;
                p[r] = (unsigned)(ev * fac);      // float32 product, <= 2^31
            }
            const unsigned w = top_bytes(p);
            if (a.dwords && 4 * d + 3 < T) {
                *reinterpret_cast<unsigned*>(orow + 4 * d) = w;
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (4 * d + r < T) orow[4 * d + r] = (uint8_t)(w >> (8 * r));
            }
        }
    }
}


// ---- host side: every exported entry fills an AttnDesc and returns attention_launch(desc)
enum AttnFamily {
    SHIFTMAX_SHORT,   // attention_kernel MODE 0 / 1 / 2, 1 .. 208 tokens
    SHIFTMAX_LONG,    // attention_long_kernel MODE 0 / 1, 208 .. 1025 tokens
    IBERT_SHORT,      // attention_kernel MODE 3 / 4, 193 .. 207 tokens (the 13-tile form; the float32 row-sum order of rowsum.h)
    IBERT_LONG,       // attention_long_kernel MODE 2, 208 .. 1025 tokens
    SHIFTMAX_CLS,     // attention_cls_kernel, 1 .. 208 tokens
    SHIFTMAX_PROBS,   // attention_probs_kernel MODE 0 / 1, 1 .. 1025 tokens
    IBERT_PROBS       // attention_probs_kernel MODE 2, 1 .. 1025 tokens
};

struct AttnDesc {     // never passed to a kernel
    const char* name;             // the called entry, for the messages
    AttnFamily family;
    const int8_t* qkv;            // cls: k
    int8_t* out;                  // probs: the uint8 probabilities
    int batch, heads, tokens, head_dim;
    uint32_t m_s;
    int32_t e_s;
    float s_attn;                 // Shiftmax families
    uint32_t m_o;
    int32_t e_o;
    const void* table;            // Shiftmax: exp2d (u32) or NULL; I-BERT: the (row max, q) table (float32), required
    const void* band;
    int band_w;
    int softmax_bits, out_blocks;
    ivit_stream_t stream;
    const int8_t *v, *q;          // cls only
    int64_t ldo;                  // cls; probs: ldp
    int q_rows;                   // probs only
    double Ms, Mo;                // filled by attention_check
    int x0;
};

// Every check the entries share; a family's own checks are marked.  On success the two multipliers and x0 are in the descriptor.
int attention_check(AttnDesc& d)
{
    const char* fn = d.name;
    const bool probs = d.family == SHIFTMAX_PROBS || d.family == IBERT_PROBS;
    const bool ibert = d.family == IBERT_SHORT || d.family == IBERT_LONG || d.family == IBERT_PROBS, cls = d.family == SHIFTMAX_CLS;
    const bool lng = d.family == SHIFTMAX_LONG || d.family == IBERT_LONG || (probs && d.tokens >= LONG_T_MIN);
    IVIT_REQUIRE(d.softmax_bits == 4 || d.softmax_bits == 8 || d.softmax_bits == 16, "%s: softmax_bits must be 4, 8 or 16", fn);
    const bool operands = d.qkv && d.out && (!ibert || d.table) && (!cls || (d.v && d.q));
    if (d.family == IBERT_SHORT) {
        IVIT_REQUIRE(operands && d.batch > 0 && d.heads > 0, "%s: bad operand", fn);
    } else {
        IVIT_REQUIRE(operands, ibert ? "%s: bad operand (NULL qkv, out or table)" : "%s: NULL operand", fn);
        IVIT_REQUIRE(d.batch > 0 && d.heads > 0 && (int64_t)d.batch * d.heads < 2147483648ll, "%s: empty batch", fn);
    }
    const int t_min = probs ? 1 : lng ? LONG_T_MIN : d.family == IBERT_SHORT ? 16 * (NKT - 1) + 1 : 1;
    const int t_max = probs || lng ? LONG_T_MAX : d.family == IBERT_SHORT ? KP - 1 : KP;
    if (d.head_dim != HD || d.tokens < t_min || d.tokens > t_max) {
        ivit_set_error("%s: unsupported geometry head_dim=%d tokens=%d (need 64, %d..%d)", fn, d.head_dim, d.tokens, t_min, t_max);
        return IVIT_ERR_UNSUPPORTED;
    }
    // probs: the output may start on any byte (the kernel packs dwords where the rows allow it)
    const bool aligned = ((uintptr_t)d.qkv % 16 == 0) && (probs || (uintptr_t)d.out % 16 == 0) && (!ibert || (uintptr_t)d.table % 4 == 0) &&
                         (!cls || (((uintptr_t)d.v % 16 == 0) && ((uintptr_t)d.q % 16 == 0) &&
                                   d.ldo >= (int64_t)d.heads * d.head_dim && d.ldo % 16 == 0));
    IVIT_REQUIRE(aligned, d.family == IBERT_SHORT ? "%s: misaligned operand" : "%s: misaligned operand (16-byte rows)", fn);
    if (probs)
        IVIT_REQUIRE(d.q_rows >= 1 && d.q_rows <= d.tokens && d.ldo >= d.tokens, "%s: q_rows must be in 1..tokens and ldp >= tokens", fn);
    if (!ibert) IVIT_REQUIRE(d.s_attn > 0.0f, "%s: scale must be positive", fn);
    IVIT_REQUIRE(d.out_blocks == 0 || (d.out_blocks == 1 && ((int64_t)d.batch * d.tokens + 15) * d.heads * d.head_dim < 2147483648ll),
                 "%s: bad output layout (block-layout buffers stay below 2 GiB)", fn);
    if (lng)      // long rows only
        IVIT_REQUIRE((int64_t)d.batch * d.heads * d.tokens * d.head_dim * 3 < ((int64_t)1 << 40), "%s: qkv too large", fn);
    IVIT_REQUIRE((uintptr_t)d.table % 4 == 0, "%s: misaligned exponent table", fn);
    IVIT_REQUIRE(d.band_w == 0 || (d.band && d.band_w >= 16 && d.band_w <= 256 && d.band_w % 16 == 0 && (uintptr_t)d.band % 16 == 0),
                 "%s: band table must be 16-byte aligned, width a multiple of 16 in [16, 256]", fn);
    d.Ms = ivit_dyadic_to_double(d.m_s, d.e_s);
    d.Mo = ivit_dyadic_to_double(d.m_o, d.e_o);
    IVIT_REQUIRE(d.Ms < 2048.0 && d.Mo < 512.0, "%s: requant multiplier too large", fn);
    d.x0 = 0;
    if (!ibert) {
        if (const int rc = shiftmax_x0(d.s_attn, -4096, fn, &d.x0)) return rc;
        // short rows only: the exact u32 row sum, tokens * |x0| * 2^15, must stay below 2^32.  Long rows: exp_int <= 2 |x0| * 2^14
        // <= 2^27, 16 of them in u32, the row in u64 (common.h rows_allsum_u64)
        if (!lng)
            IVIT_REQUIRE((double)d.tokens * (double)(-d.x0) * 32768.0 < 4294967296.0,
                         "%s: Shiftmax row sum could overflow 32 bits (x0=%d)", fn, d.x0);
    }
    return IVIT_OK;
}

// The instantiations, by what selects them.  An empty slot is never selected (RQ32 exists for 8-bit probabilities only, the I-BERT
// long form for 8-bit only).
typedef void (*ShortKernel)(AttnArgs);
typedef void (*LongKernel)(LongArgs);
typedef void (*ClsKernel)(ClsArgs);
// The width index PBI: 0 = 8-bit probabilities, 1 = 16, 2 = 4 (instantiations of their own: the 8- and 16-bit ones keep their code)
// [GENT: tokens <= 192][PBI][MODE 0, MODE 1 (band), MODE 2 (exp2d), MODE 0 with RQ32]
const ShortKernel SHIFTMAX_SHORT_KERNELS[2][3][4] = {
    {{attention_kernel<0>, attention_kernel<1>, attention_kernel<2>, attention_kernel<0, 8, 4, false, true>},
     {attention_kernel<0, 16>, attention_kernel<1, 16>, attention_kernel<2, 16>, nullptr},
     {attention_kernel<0, 4, 4>, attention_kernel<1, 4, 4>, attention_kernel<2, 4, 4>, attention_kernel<0, 4, 4, false, true>}},
    {{attention_kernel<0, 8, 4, true>, attention_kernel<1, 8, 4, true>, attention_kernel<2, 8, 4, true>, attention_kernel<0, 8, 4, true, true>},
     {attention_kernel<0, 16, 3, true>, attention_kernel<1, 16, 3, true>, attention_kernel<2, 16, 3, true>, nullptr},
     {attention_kernel<0, 4, 4, true>, attention_kernel<1, 4, 4, true>, attention_kernel<2, 4, 4, true>, attention_kernel<0, 4, 4, true, true>}}};
// [PBI][MODE 3 (table), MODE 4 (band)]
const ShortKernel IBERT_SHORT_KERNELS[3][2] = {{attention_kernel<3>, attention_kernel<4>}, {attention_kernel<3, 16>, attention_kernel<4, 16>},
                                               {attention_kernel<3, 4, 4>, attention_kernel<4, 4, 4>}};
// [PBI][(tokens >> 4) > 40][MODE 0, MODE 0 with RQ32, MODE 1 (natural), MODE 2 (I-BERT), MODE 2 with RQ32]; the threads per
// workgroup alongside: 16-bit probabilities are two more accumulator sets, so each token range takes the next smaller workgroup
const int LONG_THREADS[3][2] = {{1024, 768}, {768, 512}, {1024, 768}};
const LongKernel LONG_KERNELS[3][2][5] = {
    {{attention_long_kernel<0, false, 40, 1024>, attention_long_kernel<0, true, 40, 1024>, attention_long_kernel<1, false, 40, 1024>,
      attention_long_kernel<2, false, 40, 1024>, attention_long_kernel<2, true, 40, 1024>},
     {attention_long_kernel<0, false, 64, 768>, attention_long_kernel<0, true, 64, 768>, attention_long_kernel<1, false, 64, 768>,
      attention_long_kernel<2, false, 64, 768>, attention_long_kernel<2, true, 64, 768>}},
    {{attention_long_kernel<0, false, 40, 768, 16>, attention_long_kernel<0, true, 40, 768, 16>, attention_long_kernel<1, false, 40, 768, 16>,
      nullptr, nullptr},
     {attention_long_kernel<0, false, 64, 512, 16>, attention_long_kernel<0, true, 64, 512, 16>, attention_long_kernel<1, false, 64, 512, 16>,
      nullptr, nullptr}},
    {{attention_long_kernel<0, false, 40, 1024, 4>, attention_long_kernel<0, true, 40, 1024, 4>, attention_long_kernel<1, false, 40, 1024, 4>,
      nullptr, nullptr},
     {attention_long_kernel<0, false, 64, 768, 4>, attention_long_kernel<0, true, 64, 768, 4>, attention_long_kernel<1, false, 64, 768, 4>,
      nullptr, nullptr}}};
const ClsKernel CLS_KERNELS[3] = {attention_cls_kernel<0>, attention_cls_kernel<1>, attention_cls_kernel<2>};   // [MODE]
typedef void (*ProbsKernel)(ProbsArgs);
const ProbsKernel PROBS_KERNELS[3] = {attention_probs_kernel<0>, attention_probs_kernel<1>, attention_probs_kernel<2>};   // [MODE]

int attention_launch(AttnDesc d)
{
    if (const int rc = attention_check(d)) return rc;
    const bool ibert = d.family == IBERT_SHORT || d.family == IBERT_LONG || d.family == IBERT_PROBS;
    const int pairs = d.batch * d.heads, pb16 = d.softmax_bits == 16, pbi = pb16 ? 1 : d.softmax_bits == 4 ? 2 : 0;
    // a power-of-two score multiplier (m = 2^k): the float32 requantisation of the RQ32 kernels is exact
    const bool ms_pow2 = d.m_s != 0 && (d.m_s & (d.m_s - 1)) == 0 && d.Ms >= 1e-30;
    hipStream_t st = ivit_stream(d.stream);
    if (d.family == SHIFTMAX_PROBS || d.family == IBERT_PROBS) {
        ProbsArgs a{};
        a.qkv = d.qkv; a.probs = reinterpret_cast<uint8_t*>(d.out); a.ldp = d.ldo;
        a.batch = d.batch; a.heads = d.heads; a.tokens = d.tokens; a.q_rows = d.q_rows;
        a.Ms = d.Ms; a.x0 = d.x0;
        a.table = static_cast<const unsigned*>(d.band_w ? d.band : d.table);
        a.band_w = d.band_w;
        a.groups = (((d.q_rows + 15) >> 4) + 3) >> 2;
        a.dwords = (uintptr_t)d.out % 4 == 0 && d.ldo % 4 == 0;
        IVIT_REQUIRE((int64_t)pairs * a.groups < 2147483648ll, "%s: too many workgroups", d.name);
        hipLaunchKernelGGL(PROBS_KERNELS[ibert ? 2 : (d.band_w || d.table) ? 1 : 0], dim3(pairs * a.groups), dim3(NT),
                           probs_lds_bytes(d.tokens), st, a);
        IVIT_CHECK_LAUNCH(d.name);
    }
    if (d.family == SHIFTMAX_CLS) {
        ClsArgs a{};
        a.k = d.qkv; a.v = d.v; a.q = d.q; a.out = d.out; a.ldo = d.ldo;
        a.pairs = pairs; a.heads = d.heads; a.tokens = d.tokens;
        a.exp2d = static_cast<const unsigned*>(d.table); a.band = static_cast<const unsigned*>(d.band); a.band_w = d.band_w;
        a.Ms = d.Ms; a.Mo = d.Mo; a.x0 = d.x0;
        hipLaunchKernelGGL(CLS_KERNELS[d.band_w ? 1 : d.table ? 2 : 0], dim3((pairs + CLS_WAVES - 1) / CLS_WAVES), dim3(NT), 0, st, a);
        IVIT_CHECK_LAUNCH(d.name);
    }
    const int nqt = (d.tokens + 15) >> 4;
    if (d.family == SHIFTMAX_LONG || d.family == IBERT_LONG) {
        LongArgs a{};
        a.qkv = d.qkv; a.out = d.out; a.batch = d.batch; a.heads = d.heads; a.tokens = d.tokens;
        a.out_blocks = d.out_blocks;
        a.Ms = d.Ms; a.Mo = d.Mo; a.Ms32 = (float)d.Ms; a.x0 = d.x0;
        a.table = static_cast<const unsigned*>(d.band_w ? d.band : d.table);
        a.band_w = d.band_w;
        a.vt_row = ((((nqt + 3) >> 2) + 3) >> 2) * 256;
        const size_t lds = (size_t)LONG_LUT_BYTES + (size_t)nqt * 16 * HD + (size_t)HD * a.vt_row;    // <= 150528 bytes at 1025 tokens
        const int wide = (d.tokens >> 4) > 40, nth = LONG_THREADS[pbi][wide];
        a.parts = attention_parts(pairs, nqt, nth / 64, 256);
        const int sel = ibert ? (ms_pow2 ? 4 : 3) : (d.band_w || d.table) ? 2 : ms_pow2 ? 1 : 0;
        hipLaunchKernelGGL(LONG_KERNELS[pbi][wide][sel], dim3(pairs * a.parts), dim3(nth), lds, st, a);
        IVIT_CHECK_LAUNCH(d.name);
    }
    AttnArgs a{};
    a.qkv = d.qkv; a.out = d.out; a.batch = d.batch; a.heads = d.heads; a.tokens = d.tokens;
    a.out_blocks = d.out_blocks;
    a.Ms = d.Ms; a.Mo = d.Mo;
    a.band = static_cast<const unsigned*>(d.band);
    a.band_w = d.band_w;
    const size_t band_lds_bytes = d.band_w ? (size_t)4 * 16 * (d.band_w + BAND_PAD) * sizeof(unsigned) : 0;
    {   // resident workgroups: 4 per CU for 8-bit probabilities (128 VGPRs), 3 for the 16-bit planes; the band rows add dynamic LDS
        const int smem_bytes = (ibert || d.band_w || d.table) ? SMEM_BYTES : SMEM0_BYTES;     // MODE 0: one float32 table
        const int by_regs = pb16 ? 3 : 4, by_lds = (int)(163840 / (smem_bytes + 512 + band_lds_bytes));
        a.parts = attention_parts(pairs, nqt, NT / 64, 256 * (by_regs < by_lds ? by_regs : by_lds));
#if IVIT_LAB
        if ((g_attn_debug >> 8) & 7) a.parts = (g_attn_debug >> 8) & 7;      // lab: forced (scripts/attn_parts.py), this form only
#endif
    }
    ShortKernel kernel;
    if (ibert) {
        a.ib_table = static_cast<const float*>(d.table);
        kernel = IBERT_SHORT_KERNELS[pbi][d.band_w ? 1 : 0];
    } else {
        a.abl = g_attn_debug & 31;
        a.exp2d = static_cast<const unsigned*>(d.table);
        a.nMs32 = (float)-d.Ms;
        a.x0 = d.x0;
        a.ksat = shiftmax_ksat(d.x0);
        const bool rq32 = ms_pow2 && !pb16 && !(IVIT_LAB && (g_attn_debug & (1 << 5)));     // lab bit 5: off, A/B
        kernel = SHIFTMAX_SHORT_KERNELS[d.tokens <= 16 * (NKT - 1)][pbi][d.band_w ? 1 : d.table ? 2 : rq32 ? 3 : 0];
    }
    hipLaunchKernelGGL(kernel, dim3(pairs * a.parts), dim3(NT), band_lds_bytes, st, a);
    IVIT_CHECK_LAUNCH(d.name);
}

}  // namespace

// The thirteen entries (contracts: include/ivit_hip.h).  Descriptor order: name, family, qkv, out, batch, heads, tokens, head_dim, m_s,
// e_s, s_attn, m_o, e_o, table, band, band_w, softmax_bits, out_blocks, stream (cls: + v, q, ldo; probs: + NULL, NULL, ldp, q_rows).
IVIT_EXPORT int ivit_attention_cls_i8(const int8_t* k, const int8_t* v, const int8_t* q, int8_t* out, int64_t ldo, int batch,
                                      int heads, int tokens, int head_dim, uint32_t m_s, int32_t e_s, float s_attn, uint32_t m_o,
                                      int32_t e_o, const uint32_t* exp2d, const uint32_t* band, int band_w, ivit_stream_t stream)
{
    return attention_launch({"ivit_attention_cls_i8", SHIFTMAX_CLS, k, out, batch, heads, tokens, head_dim, m_s, e_s, s_attn, m_o, e_o,
                             exp2d, band, band_w, 8, 0, stream, v, q, ldo});
}

IVIT_EXPORT int ivit_attention_fused_i8(const int8_t* qkv, int8_t* out, int batch, int heads, int tokens,
                                        int head_dim, uint32_t m_s, int32_t e_s, float s_attn, uint32_t m_o,
                                        int32_t e_o, ivit_stream_t stream)
{
    return attention_launch({"ivit_attention_fused_i8", SHIFTMAX_SHORT, qkv, out, batch, heads, tokens, head_dim, m_s, e_s, s_attn, m_o,
                             e_o, nullptr, nullptr, 0, 8, 0, stream});
}

IVIT_EXPORT int ivit_attention_fused_i8_ex(const int8_t* qkv, int8_t* out, int batch, int heads, int tokens,
                                        int head_dim, uint32_t m_s, int32_t e_s, float s_attn, uint32_t m_o,
                                        int32_t e_o, int out_blocks, ivit_stream_t stream)
{
    return attention_launch({"ivit_attention_fused_i8_ex", SHIFTMAX_SHORT, qkv, out, batch, heads, tokens, head_dim, m_s, e_s, s_attn, m_o,
                             e_o, nullptr, nullptr, 0, 8, out_blocks, stream});
}

IVIT_EXPORT int ivit_attention_fused_i8_compat(const int8_t* qkv, int8_t* out, int batch, int heads, int tokens,
                                               int head_dim, uint32_t m_s, int32_t e_s, float s_attn, uint32_t m_o,
                                               int32_t e_o, const uint32_t* exp2d, int out_blocks, ivit_stream_t stream)
{
    return attention_launch({"ivit_attention_fused_i8_compat", SHIFTMAX_SHORT, qkv, out, batch, heads, tokens, head_dim, m_s, e_s, s_attn,
                             m_o, e_o, exp2d, nullptr, 0, 8, out_blocks, stream});
}

IVIT_EXPORT int ivit_attention_fused_i8_compat_band(const int8_t* qkv, int8_t* out, int batch, int heads, int tokens,
                                                    int head_dim, uint32_t m_s, int32_t e_s, float s_attn, uint32_t m_o,
                                                    int32_t e_o, const uint32_t* exp2d, const uint32_t* band, int band_w,
                                                    int out_blocks, ivit_stream_t stream)
{
    return attention_launch({"ivit_attention_fused_i8_compat_band", SHIFTMAX_SHORT, qkv, out, batch, heads, tokens, head_dim, m_s, e_s,
                             s_attn, m_o, e_o, exp2d, band, band_w, 8, out_blocks, stream});
}

IVIT_EXPORT int ivit_attention_fused_i8_wide(const int8_t* qkv, int8_t* out, int batch, int heads, int tokens, int head_dim,
                                             uint32_t m_s, int32_t e_s, float s_attn, uint32_t m_o, int32_t e_o,
                                             const uint32_t* exp2d, const uint32_t* band, int band_w, int softmax_bits,
                                             int out_blocks, ivit_stream_t stream)
{
    return attention_launch({"ivit_attention_fused_i8_wide", SHIFTMAX_SHORT, qkv, out, batch, heads, tokens, head_dim, m_s, e_s, s_attn,
                             m_o, e_o, exp2d, band, band_w, softmax_bits, out_blocks, stream});
}

IVIT_EXPORT int ivit_attention_fused_i8_long(const int8_t* qkv, int8_t* out, int batch, int heads, int tokens, int head_dim,
                                             uint32_t m_s, int32_t e_s, float s_attn, uint32_t m_o, int32_t e_o,
                                             const uint32_t* exp2d, const uint32_t* band, int band_w, int out_blocks,
                                             ivit_stream_t stream)
{
    return attention_launch({"ivit_attention_fused_i8_long", SHIFTMAX_LONG, qkv, out, batch, heads, tokens, head_dim, m_s, e_s, s_attn,
                             m_o, e_o, exp2d, band, band_w, 8, out_blocks, stream});
}

IVIT_EXPORT int ivit_attention_fused_i8_wide_long(const int8_t* qkv, int8_t* out, int batch, int heads, int tokens, int head_dim,
                                                  uint32_t m_s, int32_t e_s, float s_attn, uint32_t m_o, int32_t e_o,
                                                  const uint32_t* exp2d, const uint32_t* band, int band_w, int softmax_bits,
                                                  int out_blocks, ivit_stream_t stream)
{
    return attention_launch({"ivit_attention_fused_i8_wide_long", SHIFTMAX_LONG, qkv, out, batch, heads, tokens, head_dim, m_s, e_s,
                             s_attn, m_o, e_o, exp2d, band, band_w, softmax_bits, out_blocks, stream});
}

IVIT_EXPORT int ivit_attention_fused_i8_ibert(const int8_t* qkv, int8_t* out, int batch, int heads, int tokens, int head_dim,
                                              uint32_t m_s, int32_t e_s, uint32_t m_o, int32_t e_o, const float* table,
                                              const float* band, int band_w, int out_blocks, ivit_stream_t stream)
{
    return attention_launch({"ivit_attention_fused_i8_ibert", IBERT_SHORT, qkv, out, batch, heads, tokens, head_dim, m_s, e_s, 0.0f, m_o,
                             e_o, table, band, band_w, 8, out_blocks, stream});
}

IVIT_EXPORT int ivit_attention_fused_i8_ibert_wide(const int8_t* qkv, int8_t* out, int batch, int heads, int tokens, int head_dim,
                                                   uint32_t m_s, int32_t e_s, uint32_t m_o, int32_t e_o, const float* table,
                                                   const float* band, int band_w, int softmax_bits, int out_blocks,
                                                   ivit_stream_t stream)
{
    return attention_launch({"ivit_attention_fused_i8_ibert_wide", IBERT_SHORT, qkv, out, batch, heads, tokens, head_dim, m_s, e_s, 0.0f,
                             m_o, e_o, table, band, band_w, softmax_bits, out_blocks, stream});
}

IVIT_EXPORT int ivit_attention_fused_i8_ibert_long(const int8_t* qkv, int8_t* out, int batch, int heads, int tokens, int head_dim,
                                                   uint32_t m_s, int32_t e_s, uint32_t m_o, int32_t e_o, const float* table,
                                                   const float* band, int band_w, int out_blocks, ivit_stream_t stream)
{
    return attention_launch({"ivit_attention_fused_i8_ibert_long", IBERT_LONG, qkv, out, batch, heads, tokens, head_dim, m_s, e_s, 0.0f,
                             m_o, e_o, table, band, band_w, 8, out_blocks, stream});
}

// the two probability entries have no output requantisation: m_o = 0 passes attention_check's bound
IVIT_EXPORT int ivit_attention_probs_u8(const int8_t* qkv, uint8_t* probs, int64_t ldp, int batch, int heads, int tokens,
                                        int head_dim, int q_rows, uint32_t m_s, int32_t e_s, float s_attn,
                                        const uint32_t* exp2d, const uint32_t* band, int band_w, ivit_stream_t stream)
{
    return attention_launch({"ivit_attention_probs_u8", SHIFTMAX_PROBS, qkv, reinterpret_cast<int8_t*>(probs), batch, heads, tokens,
                             head_dim, m_s, e_s, s_attn, 0, 0, exp2d, band, band_w, 8, 0, stream, nullptr, nullptr, ldp, q_rows});
}

IVIT_EXPORT int ivit_attention_probs_u8_ibert(const int8_t* qkv, uint8_t* probs, int64_t ldp, int batch, int heads, int tokens,
                                              int head_dim, int q_rows, uint32_t m_s, int32_t e_s,
                                              const float* table, const float* band, int band_w, ivit_stream_t stream)
{
    return attention_launch({"ivit_attention_probs_u8_ibert", IBERT_PROBS, qkv, reinterpret_cast<int8_t*>(probs), batch, heads, tokens,
                             head_dim, m_s, e_s, 0.0f, 0, 0, table, band, band_w, 8, 0, stream, nullptr, nullptr, ldp, q_rows});
}
