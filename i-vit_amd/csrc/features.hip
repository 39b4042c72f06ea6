// features.hip -- feature maps: a token-major integer stream [B][T_all][ldx] -> dense channel-major maps [B][C][T]
// (ivit_tokens_to_nchw_*: forward_intermediates of both engines).  Per image this is a C x T transposition; one workgroup moves a
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

}      // namespace

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
