// ln_tokens.h -- token features: the final LayerNorm of a backbone on every selected token, emitted as the float32 tensor the
// module returns (ivit_modules.py:63, ibert_modules.py:153: x = y * s_ln[c]) straight from the integer stream.  Included by
// rowops.hip (int8 rows), swin.hip (int16 rows) and ibert.hip (both, I-BERT's operator) inside their anonymous namespaces, after
// NT / WPB and the row arithmetic of that file: a ROW type there states one row's statistics and element chain ONCE per kind --
// through the same device functions its int8-emitting siblings run (ln_chain.h, ln16_row, ib_ln_row) -- and hands every element to
// an `emit(c, value)`; this header owns everything else: which rows, where they go, and the launch.
//
// Rows.  The stream is token-major with a leading dimension, as ivit_tokens_to_nchw_* addresses it: row (b, t) of the selection
// (B, T_all, t0, T) is read at (b * T_all + t0 + t) * ldx.  t0 = 1 skips a class token, (t0, T) = (0, 1) takes it alone: no gather.
// Outputs.  rows form: out[(b * T + t) * ldo + c] (NLC).  Channel-major form (IVIT_LN_F32_CHANNEL_MAJOR): out[(b * C + c) * ldo + t],
// dense [B, C, T] at ldo == T (NCHW for a Gh x Gw grid), with no float intermediate in HBM: a lane-per-channel store of one token
// would write one 4-byte element per cache line, so a workgroup normalises a RUN of tr consecutive tokens of one image (one wave
// per token), parks the floats in LDS and stores them as runs of tr consecutive floats per channel (tr = 16: 64 contiguous bytes,
// 16 lanes; four channels per wave instruction).  16 tokens x 768 channels are 48 KB: three workgroups per CU.  Where 16 tokens
// of C channels (plus the kind's tables) exceed 64 KB the run is halved (C = 1024 at a natural 8-bit scale: 8 tokens).
// LDS tile, tr = 16: element (c, i) at (c >> 2) * 64 + (((c + (c >> 2) + (c >> 6)) & 3) << 4) + (i ^ ((c >> 2) & 15)) -- a
// bijection of each block of 4 channels x 16 tokens onto 64 dwords that is free of bank conflicts for a wave writing one token
// with lane = channel (16-bit kinds), with lane = dword of 4 channels (8-bit kinds: the rotation by c >> 6), and for the read-out
// (lane = token within 4 consecutive channels).  Shorter runs use a row of tr + 1 dwords per channel (odd stride).
// Every global offset is 64-bit.  Vector stores only; nothing is kept in scratch (csrc/check_resources.py `ln_tokens`).

struct LnTok {
    int B, T_all, t0, T, C;
    int64_t ldx;
    float* out;
    int64_t ldo;
    int chan_major;
    int tr;          // tokens per run: 16, 8, 4, 2 or 1
    int runs;        // runs per image
};

IVIT_DEV int ln_tok_tile(int c, int i, int tr)
{
    if (tr == 16) return ((c >> 2) << 6) + (((c + (c >> 2) + (c >> 6)) & 3) << 4) + (i ^ ((c >> 2) & 15));
    return c * (tr + 1) + i;
}

// where a row's elements go: emit(c, v) for one channel, emit.four(c, v4) for channels c .. c + 3 (c % 4 == 0)
struct LnTokEmitRow {
    float* orow;
    bool vec;        // the row admits 16-byte stores
    IVIT_DEV void operator()(int c, float v) const { orow[c] = v; }
    IVIT_DEV void four(int c, float4 v) const
    {
        if (vec) {
            *reinterpret_cast<float4*>(orow + c) = v;
        } else {
            orow[c] = v.x; orow[c + 1] = v.y; orow[c + 2] = v.z; orow[c + 3] = v.w;
        }
    }
};

struct LnTokEmitTile {
    float* lds;
    int i, tr;
    IVIT_DEV void operator()(int c, float v) const { lds[ln_tok_tile(c, i, tr)] = v; }
    IVIT_DEV void four(int c, float4 v) const
    {
        (*this)(c, v.x); (*this)(c + 1, v.y); (*this)(c + 2, v.z); (*this)(c + 3, v.w);
    }
};

template <class ROW>
__global__ __launch_bounds__(NT) void ln_tokens_f32_kernel(ROW r, LnTok o)
{
    extern __shared__ __attribute__((aligned(16))) float ln_tok_lds[];
    __shared__ unsigned char s_tab8[ROW::TAB ? ROW::TAB : 4];
    __shared__ float s_tab32[ROW::TAB ? ROW::TAB : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    r.setup(tid, s_tab8, s_tab32);
    const int64_t n_runs = (int64_t)o.B * o.runs;
    for (int64_t run = blockIdx.x; run < n_runs; run += gridDim.x) {
        const int b = (int)(run / o.runs), tb = (int)(run - (int64_t)b * o.runs) * o.tr, n = min(o.tr, o.T - tb);
        for (int i = wave; i < n; i += WPB) {
            const int64_t xoff = ((int64_t)b * o.T_all + o.t0 + tb + i) * o.ldx;
            if (o.chan_major) {
                r.row(xoff, lane, LnTokEmitTile{ln_tok_lds, i, o.tr});
            } else {
                float* orow = o.out + ((int64_t)b * o.T + tb + i) * o.ldo;
                r.row(xoff, lane, LnTokEmitRow{orow, (uintptr_t)orow % 16 == 0});
            }
        }
        if (o.chan_major) {
            __syncthreads();
            float* dst = o.out + (int64_t)b * o.C * o.ldo + tb;
            const int lg = 31 - __builtin_clz((unsigned)o.tr), total = o.C << lg;
            for (int idx = tid; idx < total; idx += NT) {
                const int c = idx >> lg, i = idx & (o.tr - 1);
                if (i < n) dst[(int64_t)c * o.ldo + i] = ln_tok_lds[ln_tok_tile(c, i, o.tr)];
            }
            __syncthreads();
        }
    }
}

#define IVIT_LN_TOK_UNSUPPORTED(cond, ...)  \
    do {                                    \
        if (!(cond)) {                      \
            ivit_set_error(__VA_ARGS__);    \
            return IVIT_ERR_UNSUPPORTED;    \
        }                                   \
    } while (0)

// The plan of the token runs (host): tokens per run and the dynamic LDS of a launch.  tab_bytes: the static tables of the kind.
static inline void ln_tok_plan(int C, int T, int chan_major, int tab_bytes, int* tr, int* runs, size_t* lds)
{
    int t = 16;
    size_t bytes = 0;
    if (chan_major) {
        // tr = 16: whole blocks of 4 channels x 16 tokens (ln_tok_tile), else a row of t + 1 dwords per channel
        auto tile = [C](int tt) { return tt == 16 ? (size_t)((C + 3) / 4) * 256 : (size_t)C * (tt + 1) * 4; };
        while (t > 1 && tile(t) + (size_t)tab_bytes > 65536) t >>= 1;
        bytes = tile(t);
    }
    *tr = t;
    *runs = (T + t - 1) / t;
    *lds = bytes;
}

// The operand checks every token-feature entry shares, then the plan.  `flags` is what is left of the entry's flags once its own
// bits are taken out, apart from IVIT_LN_F32_CHANNEL_MAJOR.  Nothing is launched on an error.
static int ln_tok_check(const char* who, const void* x, size_t esz, int64_t ldx, int B, int T_all, int t0, int T, int C, const float* bias_int,
                        const float* s_ln, float* out, int64_t ldo, int flags, int tab_bytes, LnTok* o, size_t* lds)
{
    IVIT_REQUIRE(x && out && bias_int && s_ln, "%s: NULL operand", who);
    IVIT_REQUIRE((flags & ~IVIT_LN_F32_CHANNEL_MAJOR) == 0, "%s: unknown flags %d", who, flags);
    IVIT_REQUIRE(B >= 1 && T >= 1 && C >= 1, "%s: B=%d T=%d C=%d must all be at least 1", who, B, T, C);
    IVIT_REQUIRE(t0 >= 0 && (int64_t)t0 + T <= T_all, "%s: tokens %d .. %lld of T_all=%d", who, t0, (long long)t0 + T - 1, T_all);
    const int cm = flags & IVIT_LN_F32_CHANNEL_MAJOR;
    IVIT_REQUIRE(ldx >= C && ldo >= (cm ? T : C), "%s: ldx=%lld below C=%d, or ldo=%lld below %s", who, (long long)ldx, C, (long long)ldo,
                 cm ? "T" : "C");
    IVIT_REQUIRE((uintptr_t)x % esz == 0 && (uintptr_t)out % 4 == 0 && (uintptr_t)bias_int % 4 == 0 && (uintptr_t)s_ln % 4 == 0,
                 "%s: a pointer is not aligned to its element", who);
    IVIT_LN_TOK_UNSUPPORTED(C <= 4096, "%s: C=%d unsupported (at most 4096)", who, C);
    o->B = B; o->T_all = T_all; o->t0 = t0; o->T = T; o->C = C;
    o->ldx = ldx; o->out = out; o->ldo = ldo; o->chan_major = cm;
    ln_tok_plan(C, T, cm, tab_bytes, &o->tr, &o->runs, lds);
    return IVIT_OK;
}

template <class ROW>
static int ln_tok_launch(const char* who, const ROW& r, const LnTok& o, size_t lds, ivit_stream_t stream)
{
    const int64_t n_runs = (int64_t)o.B * o.runs;
    const int grid = (int)(n_runs < 2048 ? n_runs : 2048);      // at most eight workgroups per CU, each walking its runs
    hipLaunchKernelGGL((ln_tokens_f32_kernel<ROW>), dim3(grid), dim3(NT), lds, ivit_stream(stream), r, o);
    IVIT_CHECK_LAUNCH(who);
}

// phi(q) = fl(fl(q * s) / s) of a 16-bit q, the value an operator of the reference sees at a natural scale; FASTDIV: the
// three-instruction quotient with r = RN(1 / s), which the caller has checked to be correctly rounded for all 65536 inputs
template <bool FASTDIV>
IVIT_DEV float ln_tok_phi16(int q, float s_in, float r_in)
{
    const float x = (float)q * s_in;
    if constexpr (FASTDIV) {
        const float q0 = x * r_in;
        const float e = __builtin_fmaf(-s_in, q0, x);
        return __builtin_fmaf(e, r_in, q0);
    } else {
        return x / s_in;
    }
}
