// features.hip -- what a backbone returns.  Feature maps: a token-major integer stream [B][T_all][ldx] -> dense channel-major maps
// [B][C][T] (ivit_tokens_to_nchw_*: forward_intermediates of both engines); embeddings: int8 rows -> float32 rows
// (ivit_dequant_rows_i8_f32: forward_features, further down).  Feature maps, per image this is a C x T transposition; one workgroup moves a
// tile of FT_TOK tokens x (128 bytes of) channels through LDS so that both sides of it are coalesced:
//   load   a token row of the tile is 128 contiguous source bytes (one cache line when the row is aligned); lanes take consecutive
//          VB-byte pieces of a row, VB = the widest of 16 / 8 / 4 bytes that x and ldx admit (else one element).  A piece that
//          crosses channel C is read element by element, nothing past channel C - 1 or outside tokens t0 .. t0 + T - 1 is read.
//   LDS    one dword per element, row = token, row stride TC + 1 dwords (odd): the transposed read of a wave -- lane = token, one
//          channel -- touches the banks (lane * (TC + 1) + c) mod 32, all different inside each half-wave (ds_read_b32's groups).
//          The writes of a 16-byte piece are at most 2-way, which a ds_write_b32 absorbs.
//   store  each wave stores one channel at a time: 64 lanes = 64 consecutive t of out[b][c][:], 256 contiguous bytes as float32.
// Every global offset is 64-bit (DeiT-B at 384 px, batch 256: 113 M elements per map).  (float)q * s is ONE float32 multiplication
// (-ffp-contract=off): torch's q.float() * s bit for bit.
#include "common.h"

namespace {

constexpr int FT_NT = 256;        // threads per workgroup (four waves)
constexpr int FT_TOK = 64;        // tokens per tile = lanes of a wave

template <typename TI> struct ft_tile { static constexpr int TC = 128 / (int)sizeof(TI); };    // channels per tile: 128 source bytes

template <typename TI, typename TO>
IVIT_DEV TO ft_convert(int q, float s)
{
    if constexpr (sizeof(TO) == 4) return (float)q * s;
    else return (TO)q;
}

// VB: bytes per load (16, 8, 4, or sizeof(TI) = the scalar form)
template <typename TI, typename TO, int VB>
__global__ __launch_bounds__(FT_NT) void tokens_to_nchw_kernel(const TI* __restrict__ x, int64_t ldx, int T_all, int t0, int T, int C, float s,
                                                                TO* __restrict__ out, int tiles_t, int tiles_c)
{
    constexpr int TC = ft_tile<TI>::TC, LD = TC + 1, EPV = VB / (int)sizeof(TI), PPR = TC / EPV;      // elements per piece, pieces per row
    __shared__ int tile[FT_TOK * LD];
    // consecutive workgroups: the channel tiles of one token tile (neighbouring lines of the same source rows), then the next token tile
    const unsigned bid = blockIdx.x;
    const int ct = (int)(bid % (unsigned)tiles_c), tt = (int)((bid / (unsigned)tiles_c) % (unsigned)tiles_t);
    const int b = (int)(bid / ((unsigned)tiles_c * (unsigned)tiles_t));
    const int tb = tt * FT_TOK, cb = ct * TC;
    const TI* src = x + ((int64_t)b * T_all + t0 + tb) * ldx + cb;

    // every load of the thread first, then its LDS writes (pieces outside the map are written as zeros and never read back)
    constexpr int NP = FT_TOK * PPR / FT_NT;
    static_assert(FT_TOK * PPR % FT_NT == 0, "whole pieces per thread");
    alignas(16) TI v[NP][EPV];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int i = threadIdx.x + k * FT_NT, r = i / PPR, c = (i % PPR) * EPV;
        const TI* p = src + (int64_t)r * ldx + c;
#pragma unroll
        for (int j = 0; j < EPV; ++j) v[k][j] = (TI)0;
        if (tb + r < T && cb + c + EPV <= C) {
            if constexpr (EPV == 1) v[k][0] = p[0];
            else if constexpr (VB == 16) { const uint4 w = *reinterpret_cast<const uint4*>(p); __builtin_memcpy(v[k], &w, 16); }
            else if constexpr (VB == 8) { const uint2 w = *reinterpret_cast<const uint2*>(p); __builtin_memcpy(v[k], &w, 8); }
            else { const unsigned w = *reinterpret_cast<const unsigned*>(p); __builtin_memcpy(v[k], &w, 4); }
        } else if (tb + r < T) {      // the piece that crosses channel C, or lies behind it
#pragma unroll
            for (int j = 0; j < EPV; ++j)
                if (cb + c + j < C) v[k][j] = p[j];
        }
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int i = threadIdx.x + k * FT_NT, r = i / PPR, c = (i % PPR) * EPV;
#pragma unroll
        for (int j = 0; j < EPV; ++j) tile[r * LD + c + j] = (int)v[k][j];
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = tb + lane;
    if (t >= T) return;
    const int nc = min(TC, C - cb);
    TO* dst = out + ((int64_t)b * C + cb) * T + t;
    for (int c = wave; c < nc; c += FT_NT / 64) dst[(int64_t)c * T] = ft_convert<TI, TO>(tile[lane * LD + c], s);
}

template <typename TI, typename TO>
int tokens_to_nchw(const char* who, const TI* x, int64_t ldx, int B, int T_all, int t0, int T, int C, float s, TO* out, ivit_stream_t stream)
{
    IVIT_REQUIRE(x && out, "%s: NULL pointer", who);
    IVIT_REQUIRE(B >= 1 && T >= 1 && C >= 1, "%s: B=%d T=%d C=%d must all be at least 1", who, B, T, C);
    IVIT_REQUIRE(t0 >= 0 && (int64_t)t0 + T <= T_all, "%s: tokens %d .. %lld of T_all=%d", who, t0, (long long)t0 + T - 1, T_all);
    IVIT_REQUIRE(ldx >= C, "%s: ldx=%lld below C=%d", who, (long long)ldx, C);
    IVIT_REQUIRE((uintptr_t)x % sizeof(TI) == 0 && (uintptr_t)out % sizeof(TO) == 0, "%s: a pointer is not aligned to its element", who);
    constexpr int TC = ft_tile<TI>::TC;
    const int tiles_t = (T + FT_TOK - 1) / FT_TOK, tiles_c = (C + TC - 1) / TC;
    const int64_t grid = (int64_t)B * tiles_t * tiles_c;
    IVIT_REQUIRE(grid <= 0x7fffffff, "%s: %lld tiles (at most 2^31 - 1)", who, (long long)grid);
    // the widest load every piece of every row admits: the tile's first channel is a multiple of 128 bytes
    const uintptr_t mis = (uintptr_t)x | (uintptr_t)((uint64_t)ldx * sizeof(TI));
    const int vb = mis % 16 == 0 ? 16 : mis % 8 == 0 ? 8 : mis % 4 == 0 ? 4 : (int)sizeof(TI);
    const hipStream_t st = ivit_stream(stream);
#define IVIT_FT(VBv) hipLaunchKernelGGL((tokens_to_nchw_kernel<TI, TO, VBv>), dim3((unsigned)grid), dim3(FT_NT), 0, st, x, ldx, T_all, t0, T, C, s, out, tiles_t, tiles_c)
    if (vb == 16) IVIT_FT(16);
    else if (vb == 8) IVIT_FT(8);
    else if (vb == 4) IVIT_FT(4);
    else IVIT_FT((int)sizeof(TI));
#undef IVIT_FT
    IVIT_CHECK_LAUNCH(who);
}

// ---- backbone outputs: rows of int8 integers -> float32 rows, out[r][c] = (float)x[r][c] * s (forward_features of both engines) ----
// A pure stream: 1 byte in, 4 bytes out per element, both sides strided by rows.  A row is cut into slots of 16 channels, one thread
// per slot, and consecutive threads take consecutive slots of a row, then the next row (256 threads: 5 rows of 768 channels), so
// that a wave's loads are 1 KB contiguous and its four stores cover 4 KB contiguous.  Per row, from the two row pointers alone:
//   wide   h = the channels up to the first 16-byte boundary of the input row; if out + h is on a 16-byte boundary too, the slots
//          k < nb = (C - h) / 16 are one 16-byte load and four float4 stores each, all aligned; slot nb takes the h head channels
//          and slot nb + 1 the (C - h) % 16 tail channels, element by element;
//   scalar otherwise (the two rows never reach a 16-byte boundary at the same channel): slot k takes the channels k, k + spr,
//          k + 2 spr, ... -- a byte load and a dword store per lane, consecutive lanes on consecutive channels.
// spr = C / 16 + 2 slots per row in either form.  Row offsets are 64-bit products; nothing outside channels 0 .. C - 1 of a row is
// read or written.
constexpr int DQ_NT = 256;

IVIT_DEV float4 dq_four(unsigned w, float s)
{
    return make_float4((float)(int8_t)(w & 0xffu) * s, (float)(int8_t)((w >> 8) & 0xffu) * s, (float)(int8_t)((w >> 16) & 0xffu) * s,
                       (float)(int8_t)(w >> 24) * s);
}

__global__ __launch_bounds__(DQ_NT) void dequant_rows_kernel(const int8_t* __restrict__ x, int64_t ldx, int64_t rows, int C, float s,
                                                             float* __restrict__ out, int64_t ldo, int spr)
{
    // the workgroup's first slot as (row, slot) once, in 64 bits; the thread's own from it in 32
    const int64_t g0 = (int64_t)blockIdx.x * DQ_NT;
    const int64_t row0 = g0 / spr;
    const unsigned t = (unsigned)(g0 - row0 * spr) + threadIdx.x;
    const int64_t r = row0 + t / (unsigned)spr;
    const int k = (int)(t % (unsigned)spr);
    if (r >= rows) return;
    const int8_t* xr = x + r * ldx;
    float* orow = out + r * ldo;
    int h = (int)((0 - (uintptr_t)xr) & 15);
    if (((((uintptr_t)orow >> 2) + (unsigned)h) & 3) != 0) {
        for (int c = k; c < C; c += spr) orow[c] = (float)xr[c] * s;
        return;
    }
    h = min(h, C);
    const int nb = (C - h) >> 4;
    if (k < nb) {
        const int c = h + (k << 4);
        const uint4 w = *reinterpret_cast<const uint4*>(xr + c);
        float4* dst = reinterpret_cast<float4*>(orow + c);
        dst[0] = dq_four(w.x, s);
        dst[1] = dq_four(w.y, s);
        dst[2] = dq_four(w.z, s);
        dst[3] = dq_four(w.w, s);
    } else if (k == nb) {
        for (int c = 0; c < h; ++c) orow[c] = (float)xr[c] * s;
    } else if (k == nb + 1) {
        for (int c = h + (nb << 4); c < C; ++c) orow[c] = (float)xr[c] * s;
    }
}

}      // namespace

IVIT_EXPORT int ivit_dequant_rows_i8_f32(const int8_t* x, int64_t ldx, int64_t rows, int C, float s, float* out, int64_t ldo,
                                         ivit_stream_t stream)
{
    const char* who = "ivit_dequant_rows_i8_f32";
    IVIT_REQUIRE(x && out, "%s: NULL pointer", who);
    IVIT_REQUIRE(C >= 1 && rows >= 0, "%s: C=%d must be at least 1, rows=%lld at least 0", who, C, (long long)rows);
    IVIT_REQUIRE(ldx >= C && ldo >= C, "%s: ldx=%lld / ldo=%lld below C=%d", who, (long long)ldx, (long long)ldo, C);
    IVIT_REQUIRE((uintptr_t)out % sizeof(float) == 0, "%s: out is not aligned to its element", who);
    if (rows == 0) return IVIT_OK;
    const int spr = C / 16 + 2;
    IVIT_REQUIRE(rows <= (INT64_MAX - DQ_NT) / spr, "%s: rows=%lld", who, (long long)rows);
    const int64_t grid = (rows * spr + DQ_NT - 1) / DQ_NT;
    IVIT_REQUIRE(grid <= 0x7fffffff, "%s: %lld workgroups of %d slots of 16 channels (at most 2^31 - 1)", who, (long long)grid, DQ_NT);
    hipLaunchKernelGGL(dequant_rows_kernel, dim3((unsigned)grid), dim3(DQ_NT), 0, ivit_stream(stream), x, ldx, rows, C, s, out, ldo, spr);
    IVIT_CHECK_LAUNCH(who);
}

IVIT_EXPORT int ivit_tokens_to_nchw_i8_f32(const int8_t* x, int64_t ldx, int B, int T_all, int t0, int T, int C, float s, float* out,
                                           ivit_stream_t stream)
{
    return tokens_to_nchw("ivit_tokens_to_nchw_i8_f32", x, ldx, B, T_all, t0, T, C, s, out, stream);
}

IVIT_EXPORT int ivit_tokens_to_nchw_i16_f32(const int16_t* x, int64_t ldx, int B, int T_all, int t0, int T, int C, float s, float* out,
                                            ivit_stream_t stream)
{
    return tokens_to_nchw("ivit_tokens_to_nchw_i16_f32", x, ldx, B, T_all, t0, T, C, s, out, stream);
}

IVIT_EXPORT int ivit_tokens_to_nchw_i8(const int8_t* x, int64_t ldx, int B, int T_all, int t0, int T, int C, int8_t* out, ivit_stream_t stream)
{
    return tokens_to_nchw("ivit_tokens_to_nchw_i8", x, ldx, B, T_all, t0, T, C, 1.0f, out, stream);
}

IVIT_EXPORT int ivit_tokens_to_nchw_i16(const int16_t* x, int64_t ldx, int B, int T_all, int t0, int T, int C, int16_t* out, ivit_stream_t stream)
{
    return tokens_to_nchw("ivit_tokens_to_nchw_i16", x, ldx, B, T_all, t0, T, C, 1.0f, out, stream);
}
