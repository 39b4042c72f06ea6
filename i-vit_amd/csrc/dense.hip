// dense.hip -- dense (per-pixel) evaluation of a linear head on the patch tokens: bilinear upsample, argmax and confusion matrix in
// one launch, without the upsampled logits in memory.
//   ivit_dense_argmax_u8   labels[b][y][x] = argmax_k fl64(I_k * s_acc[k]), I_k the exact int64 bilinear combination of the head's
//                          int32 accumulators (integer weights of denominator 2r per axis); conf[t][p] += 1 per valid pixel
//   ivit_patch_mode_u8     the most frequent valid class of every r x r patch of a label map (the training side's patch labels)
//
// The argmax kernel.  A workgroup (4 waves) owns one image, one patch row py and a chunk of at most DN_NC = 16 patch columns: an
// output tile of r rows x nc * r columns.  Every output row of the tile has its two source rows among the patch rows py - 1, py,
// py + 1 (clamped), every column its two source columns among the chunk's columns and one more on each side (clamped), so the
// workgroup stages 3 x (nc + 2) accumulator rows once into LDS as [row][column][class] with an odd class pitch -- at most
// 3 * 18 * 255 * 4 = 55 080 bytes, sized by the class count at launch -- beside the float32 scales.
// Clamping IS the specification's edge rule: a negative source coordinate has i0 = 0, f = 0, and the floor form used here gives it
// the weights (2r - f', f') on (clamp(-1), 0) = (0, 0): the same 2r * acc[0].  Likewise i1 = min(i0 + 1, g - 1).
// A lane owns a pixel; the 256 lanes walk the tile row-major, so the 64 pixels of a wave lie in one output row (or two) and the
// lanes inside one patch cell read the same four LDS addresses: broadcasts; neighbouring cells are an odd pitch apart, on different
// banks.  Per class a lane makes four ds_read_b32 and four v_mad_i64_i32 (the products wy * wx <= 4 r^2 = 4096 are formed once per
// pixel, |I_k| < 2^43), one exact conversion, ONE v_mul_f64 and one compare; the running (score, class) stays in registers and `>`
// over ascending classes is the tie rule.  There is no vertically interpolated line in LDS: it would need int64 entries (36 KB more
// at 255 classes, one workgroup per CU instead of two), two barriers per output row and would leave lanes idle for r < 16, to save
// two of the four multiply-adds.
// Labels leave as one dword per four lanes (DPP quad exchange) where the map's rows are dword aligned, else as bytes.
// Confusion matrix.  A wave first merges its equal (target, prediction) pairs (ballots: a tile sees few distinct pairs, a one-class
// image exactly one), and one lane per distinct pair adds the count into the workgroup's LDS table of DN_SLOTS pairs (open
// addressing, 8 probes); a pair that finds no slot goes straight to memory.  At the end every occupied slot is one 64-bit global
// atomic: a workgroup touches conf a handful of times, whatever the class statistics.
#include "bilinear_tap.h"      // dense_tap: the weights of one axis

namespace {

typedef unsigned long long u64;

constexpr int DN_NT = 256;        // threads per workgroup (four waves)
constexpr int DN_NC = 16;         // patch columns per workgroup
constexpr int DN_SLOTS = 256;     // (target, prediction) pairs a workgroup keeps in LDS
constexpr int DN_PROBES = 8;

struct DenseArgs {
    const int32_t* acc;
    const float* s_acc;
    int gh, gw, np, classes, r, chunks;
    uint8_t* labels;
    const uint8_t* target;
    int ignore_index;
    u64* conf;
    int packed;                   // labels rows are dword aligned: W % 4 == 0 and labels % 4 == 0
};

IVIT_DEV void dense_pair_add(int* keys, unsigned* cnts, u64* conf, int classes, int key, unsigned n)
{
    const unsigned h = ((unsigned)key * 0x9E3779B1u) >> 24;
    for (int p = 0; p < DN_PROBES; ++p) {
        const int slot = (int)((h + (unsigned)p) & (DN_SLOTS - 1));
        const int old = atomicCAS(&keys[slot], -1, key);
        if (old == -1 || old == key) {
            atomicAdd(&cnts[slot], n);
            return;
        }
    }
    atomicAdd(&conf[(int64_t)(key >> 8) * classes + (key & 255)], (u64)n);
}

__global__ __launch_bounds__(DN_NT) void dense_argmax_kernel(DenseArgs a)
{
    extern __shared__ __attribute__((aligned(16))) int dn_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int classes = a.classes, r = a.r, pitch = classes | 1;
    const int chunk = (int)(blockIdx.x % (unsigned)a.chunks);
    const int rowid = (int)(blockIdx.x / (unsigned)a.chunks);      // b * gh + py
    const int py = rowid % a.gh;
    const int64_t b = rowid / a.gh;
    const int px0 = chunk * DN_NC, nc = min(DN_NC, a.gw - px0), ns = nc + 2;

    int* raw = dn_lds;                                              // [3][ns][pitch]
    float* sc = reinterpret_cast<float*>(raw + 3 * (DN_NC + 2) * pitch);
    int* keys = reinterpret_cast<int*>(sc + pitch);
    unsigned* cnts = reinterpret_cast<unsigned*>(keys + DN_SLOTS);

    for (int p = wave; p < 3 * ns; p += DN_NT / 64) {
        const int ar = p / ns, s = p - ar * ns;
        const int row = clamp_i32(py - 1 + ar, 0, a.gh - 1), col = clamp_i32(px0 - 1 + s, 0, a.gw - 1);
        const int32_t* src = a.acc + ((b * a.gh + row) * a.gw + col) * a.np;
        for (int k = lane; k < classes; k += 64) raw[p * pitch + k] = src[k];
    }
    for (int k = tid; k < classes; k += DN_NT) sc[k] = a.s_acc[k];
    if (tid < DN_SLOTS) {
        keys[tid] = -1;
        cnts[tid] = 0;
    }
    __syncthreads();

    const int width = nc * r, npix = r * width;
    const int64_t W = (int64_t)a.gw * r;
    const int64_t tile0 = (b * a.gh + py) * r * W + (int64_t)px0 * r;      // pixel (row 0, column 0) of the tile
    for (int q0 = 0; q0 < npix; q0 += DN_NT) {
        const int q = q0 + tid;
        const bool live = q < npix;
        const int qc = live ? q : npix - 1;
        const int j = qc / width, xl = qc - j * width;
        const int pc = xl / r, jx = xl - pc * r;
        int ay, fy, ax, fx;
        dense_tap(j, r, ay, fy);
        dense_tap(jx, r, ax, fx);
        const int w00 = (2 * r - fy) * (2 * r - fx), w01 = (2 * r - fy) * fx, w10 = fy * (2 * r - fx), w11 = fy * fx;
        const int* t00 = raw + (ay * ns + pc + ax) * pitch;
        const int* t10 = t00 + ns * pitch;
        double best = 0.0;
        int bk = 0;
#pragma unroll 4
        for (int k = 0; k < classes; ++k) {
            const long long I = (long long)w00 * t00[k] + (long long)w01 * t00[pitch + k] + (long long)w10 * t10[k] + (long long)w11 * t10[pitch + k];
            const double s = (double)I * (double)sc[k];             // ONE float64 multiplication (-ffp-contract=off)
            const bool up = k == 0 || s > best;
            best = up ? s : best;
            bk = up ? k : bk;
        }
        const int64_t o = tile0 + j * W + xl;
        if (a.labels) {
            if (a.packed) {          // width % 4 == 0: a quad of lanes is four pixels of one row, all live or none
                unsigned v = (unsigned)bk << (8 * (lane & 3));
                v |= IVIT_DPP_U32(v, 0xB1);
                v |= IVIT_DPP_U32(v, 0x4E);
                if (live && (lane & 3) == 0) *reinterpret_cast<unsigned*>(a.labels + o) = v;
            } else if (live) {
                a.labels[o] = (uint8_t)bk;
            }
        }
        if (a.conf) {
            int key = -1;
            if (live) {
                const int t = a.target[o];
                if (t < classes && t != a.ignore_index) key = (t << 8) | bk;
            }
            u64 todo = __builtin_amdgcn_ballot_w64(key >= 0);
            while (todo) {
                const int src = __builtin_ctzll(todo);
                const int k1 = __builtin_amdgcn_readlane(key, src);
                const u64 same = __builtin_amdgcn_ballot_w64(key == k1);
                todo &= ~same;
                if (lane == src) dense_pair_add(keys, cnts, a.conf, classes, k1, (unsigned)__builtin_popcountll(same));
            }
        }
    }
    if (a.conf) {
        __syncthreads();
        if (tid < DN_SLOTS) {
            const int key = keys[tid];
            if (key >= 0) atomicAdd(&a.conf[(int64_t)(key >> 8) * classes + (key & 255)], (u64)cnts[tid]);
        }
    }
}

// ---- patch labels: one wave per patch, a 256-bin histogram per wave in LDS
__global__ __launch_bounds__(DN_NT) void patch_mode_kernel(const uint8_t* __restrict__ target, int64_t patches, int gh, int gw, int r, int classes,
                                                           int ignore_index, uint8_t* __restrict__ out)
{
    __shared__ int hist[DN_NT / 64][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t patch = (int64_t)blockIdx.x * (DN_NT / 64) + wave;
    const bool live = patch < patches;
    const int64_t p = live ? patch : patches - 1;
    const int px = (int)(p % gw);
    const int64_t rowid = p / gw;                                   // b * gh + py
    const int64_t W = (int64_t)gw * r;
    const uint8_t* src = target + rowid * r * W + (int64_t)px * r;
    for (int k = lane; k < 256; k += 64) hist[wave][k] = 0;
    __syncthreads();
    int valid = 0;
    for (int i = lane; i < r * r; i += 64) {
        const int y = i / r, x = i - y * r;
        const int t = src[y * W + x];
        if (t < classes && t != ignore_index) {
            atomicAdd(&hist[wave][t], 1);
            ++valid;
        }
    }
    valid = wave_reduce_sum_i32(valid);
    __syncthreads();
    int key = 0;                                                    // count << 8 | 255 - class: the largest count, then the lowest class
    for (int k = lane; k < classes; k += 64) key = max(key, (hist[wave][k] << 8) | (255 - k));
    key = wave_allmax_i32(key);
    if (live && lane == 0) out[patch] = (uint8_t)(2 * valid < r * r ? ignore_index : 255 - (key & 255));
}

int dense_check_shape(const char* who, int batch, int gh, int gw, int r, int classes, int ignore_index)
{
    IVIT_REQUIRE(batch >= 1 && gh >= 1 && gw >= 1, "%s: batch=%d, gh=%d and gw=%d must be at least 1", who, batch, gh, gw);
    IVIT_REQUIRE(ignore_index >= 0 && ignore_index <= 255, "%s: ignore_index=%d outside [0, 255]", who, ignore_index);
    if (classes < 1 || classes > IVIT_DENSE_CLASSES_MAX || r < 1 || r > IVIT_DENSE_R_MAX) {
        ivit_set_error("%s: unsupported geometry (classes=%d outside [1, %d] or r=%d outside [1, %d])", who, classes, IVIT_DENSE_CLASSES_MAX, r,
                       IVIT_DENSE_R_MAX);
        return IVIT_ERR_UNSUPPORTED;
    }
    const int64_t rows = (int64_t)batch * gh;                      // < 2^62; the products below are checked step by step
    IVIT_REQUIRE(rows < (1ll << 31) && rows * gw < (1ll << 31) && rows * gw * r * r < (1ll << 31),
                 "%s: batch=%d x gh=%d x gw=%d patches of %d x %d pixels: 2^31 pixels or more", who, batch, gh, gw, r, r);
    return IVIT_OK;
}

}      // namespace

IVIT_EXPORT int ivit_dense_argmax_u8(const int32_t* acc, const float* s_acc, int batch, int gh, int gw, int np, int classes, int r, uint8_t* labels,
                                     const uint8_t* target, int ignore_index, int64_t* conf, ivit_stream_t stream)
{
    const char* who = "ivit_dense_argmax_u8";
    IVIT_REQUIRE(acc && s_acc, "%s: NULL operand", who);
    IVIT_REQUIRE(labels || conf, "%s: neither labels nor conf is given", who);
    IVIT_REQUIRE(!conf || target, "%s: conf without a target", who);
    const int rc = dense_check_shape(who, batch, gh, gw, r, classes, ignore_index);
    if (rc != IVIT_OK) return rc;
    IVIT_REQUIRE(np >= classes, "%s: np=%d below classes=%d", who, np, classes);
    IVIT_REQUIRE(((uintptr_t)acc | (uintptr_t)s_acc) % 4 == 0 && (uintptr_t)conf % 8 == 0, "%s: acc, s_acc or conf is not aligned to its element", who);
    DenseArgs a;
    a.acc = acc, a.s_acc = s_acc, a.gh = gh, a.gw = gw, a.np = np, a.classes = classes, a.r = r;
    a.chunks = (gw + DN_NC - 1) / DN_NC;
    a.labels = labels, a.target = target, a.ignore_index = ignore_index, a.conf = reinterpret_cast<u64*>(conf);
    a.packed = ((int64_t)gw * r) % 4 == 0 && (uintptr_t)labels % 4 == 0;
    const int64_t grid = (int64_t)batch * gh * a.chunks;            // < 2^31: at most one workgroup per patch
    const int pitch = classes | 1;
    const size_t lds = (size_t)(3 * (DN_NC + 2) * pitch + pitch + 2 * DN_SLOTS) * 4;      // at most 58 148 bytes
    hipLaunchKernelGGL(dense_argmax_kernel, dim3((unsigned)grid), dim3(DN_NT), lds, ivit_stream(stream), a);
    IVIT_CHECK_LAUNCH(who);
}

IVIT_EXPORT int ivit_patch_mode_u8(const uint8_t* target, int batch, int gh, int gw, int r, int classes, int ignore_index, uint8_t* out,
                                   ivit_stream_t stream)
{
    const char* who = "ivit_patch_mode_u8";
    IVIT_REQUIRE(target && out, "%s: NULL operand", who);
    const int rc = dense_check_shape(who, batch, gh, gw, r, classes, ignore_index);
    if (rc != IVIT_OK) return rc;
    const int64_t patches = (int64_t)batch * gh * gw;
    hipLaunchKernelGGL(patch_mode_kernel, dim3((unsigned)((patches + DN_NT / 64 - 1) / (DN_NT / 64))), dim3(DN_NT), 0, ivit_stream(stream), target,
                       patches, gh, gw, r, classes, ignore_index, out);
    IVIT_CHECK_LAUNCH(who);
}
