// ln_pool.h -- pooled features, first pass: the final LayerNorm + qact2 on every selected token of a block, summed over the tokens
// in the same pass; the [B, T, C] int8 map is never written.  Included by rowops.hip, swin.hip and ibert.hip inside their anonymous
// namespaces, behind ln_tokens.h (pool.h is included by those files at file scope): the ROW types of the token-feature entries state
// a row's statistics and its chain up to y ONCE per kind; an emit with RAW = true receives y itself, and LnPoolEmit below ends the
// chain in the QuantAct of the int8-emitting entries -- ln_chain.h's certificate (ln_cert) on a per-workgroup (lo, hi) table
// (common.h ln_build_table), ln_literal for an element it does not certify -- so every token's int8 value is byte for byte theirs.
//
// Split.  Grid = (image, slab of L consecutive tokens) (pool.h: the slab rule).  The four waves of a workgroup walk the rows of
// their slab, wave w the rows w, w + 4, ...  A ROW fixes which lane owns which channel for the whole kernel (int8 rows: lane d + 64 j
// the dword d; 16-bit and I-BERT rows: lane c + 64 j the channel c), so each lane adds its values into its own int32 slots of its
// wave's accumulator row: no two lanes ever touch the same slot, no ordering matters.  The slots are in LDS, not in registers: the
// ROW types loop over the channels with a trip count known only at run time, and a register array indexed by such a loop goes to
// scratch.  A ds_read_b128 / ds_write_b128 pair per four channels rides under the ~12 VALU instructions per channel of the chain.
// At the end of the slab the four accumulator rows are added and the workgroup stores one int32 [C] partial (vector stores) to
// ws[b][slab][:]; pool.hip's second kernel adds the slabs.  LDS: 28 C bytes (three float tables, 4 x C int32) + the kind's tables.
// Every global offset is 64-bit; nothing is kept in scratch (csrc/check_resources.py `ln_pool`).  (ln_chain.h: included by the file.)

struct LnPoolEmit {
    static constexpr bool RAW = true;
    int* acc;               // this wave's accumulators [C]
    const float* lo;        // [C] each, LDS
    const float* hi;
    const float* s_ln;      // global: the literal tail of an uncertified element
    const uint32_t* m;
    const int32_t* e;

    IVIT_DEV int q8(int c, float y, float l, float h) const
    {
        unsigned unc = 0;
        int q = ln_cert(y, l, h, unc) - 0x4B400000;
        if (unc) q = ln_literal(y, s_ln[c], dyadic_mult(m[c], e[c]));
        return q;
    }
    IVIT_DEV void operator()(int c, float y) const { acc[c] += q8(c, y, lo[c], hi[c]); }
    IVIT_DEV void four(int c, float4 y) const
    {
        const float4 l = *reinterpret_cast<const float4*>(lo + c), h = *reinterpret_cast<const float4*>(hi + c);
        v4i a = *reinterpret_cast<v4i*>(acc + c);
        a[0] += q8(c, y.x, l.x, h.x);
        a[1] += q8(c + 1, y.y, l.y, h.y);
        a[2] += q8(c + 2, y.z, l.z, h.z);
        a[3] += q8(c + 3, y.w, l.w, h.w);
        *reinterpret_cast<v4i*>(acc + c) = a;
    }
};

// no packed float32 instructions in this kernel, whatever the flags of the file that instantiates it (the host pass does not know
// the feature)
#if defined(__HIP_DEVICE_COMPILE__)
#define LN_POOL_NO_PK __attribute__((target("no-packed-fp32-ops")))
#else
#define LN_POOL_NO_PK
#endif

template <class ROW>
__global__ __launch_bounds__(NT) LN_POOL_NO_PK void ln_pool_kernel(ROW r, LnPool o)
{
    extern __shared__ __attribute__((aligned(16))) float ln_pool_lds[];      // [bias | lo | hi][C] float, [WPB][C] int32
    __shared__ unsigned char s_tab8[ROW::TAB ? ROW::TAB : 4];
    __shared__ float s_tab32[ROW::TAB ? ROW::TAB : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = o.C;
    float* t_lo = ln_pool_lds + C;
    float* t_hi = ln_pool_lds + 2 * C;
    int* acc0 = reinterpret_cast<int*>(ln_pool_lds + 3 * C);
    int* acc = acc0 + wave * C;
    ln_build_table<NT>(o.m, o.e, o.s_ln, o.bias_int, C, ln_pool_lds, t_lo, t_hi);
    for (int c = lane; c < C; c += 64) acc[c] = 0;
    r.setup(tid, s_tab8, s_tab32);
    __syncthreads();
    const int b = blockIdx.x / o.slabs, slab = blockIdx.x - b * o.slabs;
    const int tb = slab * o.L, n = min(o.L, o.T - tb);
    const LnPoolEmit emit{acc, t_lo, t_hi, o.s_ln, o.m, o.e};
    for (int i = wave; i < n; i += WPB) r.row(((int64_t)b * o.T_all + o.t0 + tb + i) * o.ldx, lane, emit);
    __syncthreads();
    int32_t* dst = o.ws + ((int64_t)b * o.slabs + slab) * C;
    for (int c = tid * 4; c < C; c += NT * 4) {      // C % 4 == 0
        v4i s = *reinterpret_cast<const v4i*>(acc0 + c);
#pragma unroll
        for (int w = 1; w < WPB; ++w) s += *reinterpret_cast<const v4i*>(acc0 + w * C + c);
        *reinterpret_cast<v4i*>(dst + c) = s;
    }
}

// the first pass on `stream`, then pool.hip's second one; `out` is the first byte written (out + col0 of the entry)
template <class ROW>
static int ln_pool_launch(const char* who, const ROW& r, const LnPool& o, int32_t* sum, int8_t* out, int64_t ldo, ivit_stream_t stream)
{
    const int64_t grid = (int64_t)o.B * o.slabs;
    IVIT_REQUIRE(grid <= 2147483647ll, "%s: %lld workgroups", who, (long long)grid);
    hipLaunchKernelGGL((ln_pool_kernel<ROW>), dim3((unsigned)grid), dim3(NT), (size_t)28 * o.C, ivit_stream(stream), r, o);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) {
        ivit_set_error("%s: launch failed: %s", who, hipGetErrorString(err));
        return IVIT_ERR_LAUNCH;
    }
    return ln_pool_finish(who, o, sum, out, ldo, ivit_stream(stream));
}
