// davis.hip -- what follows the label propagation of a video frame (propagate.hip) in the DAVIS protocol: the frame's label map and
// the counts of the region similarity J and the boundary measure F (include/ivit_hip.h, "video segmentation scoring").
//   ivit_upsample_argmax_u8   soft labels on the token grid -> label map: exact bilinear upsample by r and argmax, planes never stored
//   ivit_mask_scores_u8       inter, union, n_fg, n_gt, fg_match, gt_match per (frame, object) of two stacks of label maps
//
// The upsample kernel.  A workgroup owns a block of CY x CX source cells (up_plan: about 16 rows x 64 columns of pixels, 1024 at the
// most, whole cells) and stages the (CY + 2) x (CX + 2) cells around it -- clamped, which IS the edge rule y1 = min(y0 + 1, G - 1) --
// as [row][column][class] floats with an odd class pitch, UP_LDS floats per slab of classes (K = 256 at r = 32 is two slabs).  A
// thread owns four horizontally adjacent pixels for the whole launch: per pixel the four tap addresses and the four weights
// ay * ax as doubles, per class four ds_read_b32, four exact conversions, four v_mul_f64 (exact products), three v_add_f64 in the
// order of the specification and one compare; the running (value, class) of its pixels stay in registers across the slabs, `>` over
// ascending classes is the tie rule.  The four labels leave as one dword where the rows of the map are dword aligned, else as bytes.
// The first cell of an axis: n = max(2y + 1 - r, 0) puts the pixels before the first cell centre on (y0, a1) = (0, 0) -- weight 2r on
// cell 0 and 0 on cell 1 -- where dense_tap's floor form gives (2r - f, f) on (clamp(-1), 0): the same value in integers, not the same
// float64 sums, so up_tap restates the rule of the header for that half cell.
//
// The score kernel: bit-parallel rows.  A workgroup owns MS_COLS = 64 columns x TR = 128 - 2h rows of one frame with a halo of
// h = radius + 1 pixels on every side: 64 + 2 * 25 = 114 columns, so a tile row with its halo is one 128-bit word (W128), bit i the
// column tx0 - h + i.  The label bytes of both maps for the 128 rows x (64 + 2h) columns are staged in LDS once, from CLAMPED
// coordinates: every address exists, and a replicated row / column is exactly the boundary rule of the last row and column
// (S = m gives m ^ S = 0 and SE = E; E = m gives m ^ E = 0 and SE = S; both: 0).  Bits outside the image are cleared from the
// boundary words afterwards, so the dilation and the counts see the image alone.  While staging, every thread marks the labels it
// saw in a 256-bit set (one LDS atomic per change of label down its column); an object absent from both maps of the staged region
// has empty masks there and is skipped by a uniform branch.
// Per object present, thread (map, row) -- waves 0 / 1 the 128 rows of pred, waves 2 / 3 those of truth:
//   1. the mask word by comparison: 29 dwords of labels at the most, four labels per dword against o * 0x01010101 (exact zero-byte
//      flags, gathered into a nibble by one multiplication); the word goes to LDS for the neighbours
//   2. the boundary word from its own word, the south neighbour's (LDS) and their shifts by one; cleared outside the image; to LDS
//   3. the disk: OR over dy of the horizontally dilated boundary words of the rows y +- dy, half width floor(sqrt(R^2 - dy^2)) from
//      the host's table; rows of equal half width are ORed first and dilated once, by doubling (OR of shifts 1, 2, 4, ...)
//   4. three popcounts on the 64 interior bits (its own boundary; the OTHER map's boundary inside its own dilation; the masks'
//      intersection for pred, union for truth), reduced over the wave and the two waves of a map, then one 64-bit atomic per counter.
// LDS: 2 x 128 rows x 33 dwords of labels (an odd pitch: a wave's 64 rows on 64 banks) + 2 x 2 x 128 words = 41.2 KiB.
#include "bilinear_tap.h"

namespace {

typedef unsigned long long u64;

constexpr int DV_NT = 256;        // threads per workgroup (four waves)

// ---------------------------------------------------------------------------- upsample + argmax
constexpr int UP_PX = 4;          // pixels per thread
constexpr int UP_LDS = 2048;      // floats a slab of classes may take (8 KiB)

struct UpPlan { int CY, CX, gpr, pitch; };      // cells per block, groups of UP_PX pixels per block row, class pitch (odd)

constexpr UpPlan up_plan(int r)
{
    UpPlan p{};
    p.CY = r < 16 ? 16 / r : 1;
    const int rows = p.CY * r;
    p.CX = (DV_NT * UP_PX / rows) / r;
    if (p.CX >= 4) p.CX &= ~3;                  // CX * r % 4 == 0 wherever it can be: blocks start on a dword
    p.gpr = (p.CX * r + UP_PX - 1) / UP_PX;
    while (rows * p.gpr > DV_NT) {
        --p.CX;
        p.gpr = (p.CX * r + UP_PX - 1) / UP_PX;
    }
    p.pitch = (UP_LDS / ((p.CY + 2) * (p.CX + 2)) - 1) | 1;
    return p;
}

constexpr bool up_plans_ok()
{
    for (int r = 1; r <= IVIT_UPSAMPLE_R_MAX; ++r) {
        const UpPlan p = up_plan(r);
        if (p.CX < 1 || p.CY * r * p.gpr > DV_NT || p.gpr * UP_PX < p.CX * r || p.pitch < 1 || (p.CY + 2) * (p.CX + 2) * p.pitch > UP_LDS) return false;
    }
    return true;
}
static_assert(up_plans_ok(), "a thread per group of four pixels, a slab of at least one class");

struct UpArgs {
    const float* seg;
    int Gh, Gw, r, K;
    uint8_t* pred;
    int CY, CX, gpr, pitch, bx;   // bx: blocks per row of blocks
    int packed;                   // every block row of the map starts on a dword
};

// one axis, offset j inside the cell `first ? 0 : later`: staged slots (s, s + 1), weights (2r - f, f)
IVIT_DEV void up_tap(int j, int r, bool first, int& s, int& f)
{
    dense_tap(j, r, s, f);
    if (first && s == 0) s = 1, f = 0;      // n = max(2y + 1 - r, 0) = 0: (y0, a1) = (0, 0)
}

__global__ __launch_bounds__(DV_NT) void upsample_argmax_kernel(UpArgs a)
{
    __shared__ float S[UP_LDS];
    const int tid = threadIdx.x, r = a.r, K = a.K, pitch = a.pitch;
    const int by = (int)(blockIdx.x / (unsigned)a.bx), bxi = (int)(blockIdx.x % (unsigned)a.bx);
    const int cy0 = by * a.CY, cx0 = bxi * a.CX;
    const int ncy = min(a.CY, a.Gh - cy0), ncx = min(a.CX, a.Gw - cx0), ns = ncx + 2, cells = (ncy + 2) * ns;
    const int width = ncx * r;

    // this thread's four pixels: row `row` of the block, columns 4 g .. 4 g + 3 (a dead thread computes pixel (0, 0) and stores nothing)
    const int row_ = tid / a.gpr, g_ = tid - row_ * a.gpr;
    const bool live = row_ < ncy * r && UP_PX * g_ < width;
    const int row = live ? row_ : 0, g = live ? g_ : 0;
    const int cyl = row / r;
    int sy, fy;
    up_tap(row - cyl * r, r, cy0 + cyl == 0, sy, fy);
    int t00[UP_PX];
    double w00[UP_PX], w01[UP_PX], w10[UP_PX], w11[UP_PX];
#pragma unroll
    for (int p = 0; p < UP_PX; ++p) {
        const int xl = min(UP_PX * g + p, width - 1), cxl = xl / r;
        int sx, fx;
        up_tap(xl - cxl * r, r, cx0 + cxl == 0, sx, fx);
        t00[p] = ((cyl + sy) * ns + cxl + sx) * pitch;
        w00[p] = (double)((2 * r - fy) * (2 * r - fx)), w01[p] = (double)((2 * r - fy) * fx);
        w10[p] = (double)(fy * (2 * r - fx)), w11[p] = (double)(fy * fx);
    }
    double best[UP_PX] = {0.0, 0.0, 0.0, 0.0};
    int bk[UP_PX] = {0, 0, 0, 0};

    for (int k0 = 0; k0 < K; k0 += pitch) {
        const int kn = min(pitch, K - k0);
        if (k0) __syncthreads();
        for (int e = tid; e < cells * kn; e += DV_NT) {
            const int cell = e / kn, kk = e - cell * kn, ar = cell / ns, s = cell - ar * ns;
            const int sr = clamp_i32(cy0 - 1 + ar, 0, a.Gh - 1), sc = clamp_i32(cx0 - 1 + s, 0, a.Gw - 1);
            S[cell * pitch + kk] = a.seg[((int64_t)sr * a.Gw + sc) * K + k0 + kk];
        }
        __syncthreads();
        for (int kk = 0; kk < kn; ++kk) {
#pragma unroll
            for (int p = 0; p < UP_PX; ++p) {
                const float* t = S + t00[p] + kk;
                // four exact products, three float64 additions in this order (-ffp-contract=off)
                const double v = (w00[p] * (double)t[0] + w01[p] * (double)t[pitch]) + (w10[p] * (double)t[ns * pitch] + w11[p] * (double)t[ns * pitch + pitch]);
                const bool up = k0 + kk == 0 || v > best[p];
                best[p] = up ? v : best[p];
                bk[p] = up ? k0 + kk : bk[p];
            }
        }
    }
    if (!live) return;
    uint8_t* o = a.pred + ((int64_t)cy0 * r + row) * ((int64_t)a.Gw * r) + (int64_t)cx0 * r + UP_PX * g;
    if (a.packed) {               // width % 4 == 0: the group is inside the block
        *reinterpret_cast<unsigned*>(o) = (unsigned)bk[0] | ((unsigned)bk[1] << 8) | ((unsigned)bk[2] << 16) | ((unsigned)bk[3] << 24);
    } else {
#pragma unroll
        for (int p = 0; p < UP_PX; ++p)
            if (UP_PX * g + p < width) o[p] = (uint8_t)bk[p];
    }
}

// ---------------------------------------------------------------------------- J and F counts
constexpr int MS_RT = 128;        // rows of a tile with its halo: a thread per (map, row)
constexpr int MS_COLS = 64;       // interior columns
constexpr int MS_PITCH = 33;      // dwords of labels per staged row: 4 * 29 = 116 >= 64 + 2 * 25 used, odd
constexpr int MS_RMAX = IVIT_SCORES_RADIUS_MAX;
static_assert(MS_COLS + 2 * (MS_RMAX + 1) <= 4 * (MS_PITCH - 4) && 2 * MS_RT == DV_NT, "a row with its halo in one 128-bit word, a thread per (map, row)");

struct W128 { u64 lo, hi; };
IVIT_DEV W128 operator|(W128 a, W128 b) { return W128{a.lo | b.lo, a.hi | b.hi}; }
IVIT_DEV W128 operator&(W128 a, W128 b) { return W128{a.lo & b.lo, a.hi & b.hi}; }
IVIT_DEV W128 operator^(W128 a, W128 b) { return W128{a.lo ^ b.lo, a.hi ^ b.hi}; }
IVIT_DEV W128 shl(W128 w, int s) { return W128{w.lo << s, (w.hi << s) | (w.lo >> (64 - s))}; }      // 0 < s < 64
IVIT_DEV W128 shr(W128 w, int s) { return W128{(w.lo >> s) | (w.hi << (64 - s)), w.hi >> s}; }      // 0 < s < 64
IVIT_DEV W128 ones(int n)         // bits 0 .. n - 1, 0 <= n < 128
{
    return W128{n >= 64 ? ~0ull : (1ull << n) - 1, n <= 64 ? 0ull : (1ull << (n - 64)) - 1};
}

// bit p of the result = OR of the bits p - hw .. p + hw of w: OR of the shifts 0 .. 2 hw by doubling, then back by hw.  Bits that
// leave the word at 127 would land beyond bit 127 - hw >= 103, outside the interior (at most bit 88)
IVIT_DEV W128 dilate(W128 w, int hw)
{
    if (hw == 0) return w;
    for (int have = 0; have < 2 * hw;) {          // w holds the OR of the shifts 0 .. have
        const int step = min(have + 1, 2 * hw - have);
        w = w | shl(w, step);
        have += step;
    }
    return shr(w, hw);
}

// four labels against zero: bit j of the result = (byte j of v == 0).  0x80 per zero byte, exact (no borrow between bytes), then
// bits 0, 8, 16, 24 gathered into 21 .. 24 by one multiplication (the sixteen partial products fall on sixteen different bits)
IVIT_DEV unsigned zero_bytes(unsigned v)
{
    const unsigned t = ~(((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) | v | 0x7f7f7f7fu);
    return (((t >> 7) * 0x00204081u) >> 21) & 15u;
}

struct MaskArgs {
    const uint8_t* pred;
    const uint8_t* truth;
    int H, W, O, R, tiles_x, tiles_y;
    u64* counts;
    unsigned char hw[MS_RMAX + 1];      // half width of the disk's row dy
};

__global__ __launch_bounds__(DV_NT, 2) void mask_scores_kernel(MaskArgs a)
{
    __shared__ unsigned lab[2][MS_RT * MS_PITCH];
    __shared__ W128 M[2][MS_RT], B[2][MS_RT];
    __shared__ unsigned present[8];
    __shared__ int hwt[MS_RMAX + 2];
    __shared__ int part[DV_NT / 64][3];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, which = tid >> 7, rr = tid & (MS_RT - 1);
    const int H = a.H, W = a.W, R = a.R, h = R + 1, TR = MS_RT - 2 * h, nb = (MS_COLS + 2 * h + 3) >> 2;
    const int tx = (int)(blockIdx.x % (unsigned)a.tiles_x), tyf = (int)(blockIdx.x / (unsigned)a.tiles_x);
    const int ty = tyf % a.tiles_y;
    const int64_t f = tyf / a.tiles_y;
    const int ry0 = ty * TR - h, rx0 = tx * MS_COLS - h;

    if (tid < 8) present[tid] = 0;
    if (tid <= R + 1) hwt[tid] = tid <= R ? (int)a.hw[tid] : -1;
    __syncthreads();

    // staging: thread (column j, row parity); clamped coordinates, so every address is inside the frame
    {
        const int j = tid & 127;
        if (j < 4 * nb) {
            const int x = clamp_i32(rx0 + j, 0, W - 1);
            const int64_t base = f * H * W + x;
            unsigned char* l0 = reinterpret_cast<unsigned char*>(lab[0]) + j;
            unsigned char* l1 = reinterpret_cast<unsigned char*>(lab[1]) + j;
            unsigned last0 = 0, last1 = 0;          // label 0 is no object: never looked up
            for (int i = tid >> 7; i < MS_RT; i += 2) {
                const int64_t off = base + (int64_t)clamp_i32(ry0 + i, 0, H - 1) * W;
                const unsigned v0 = a.pred[off], v1 = a.truth[off];
                l0[i * (4 * MS_PITCH)] = (unsigned char)v0;
                l1[i * (4 * MS_PITCH)] = (unsigned char)v1;
                if (v0 != last0) atomicOr(&present[v0 >> 5], 1u << (v0 & 31)), last0 = v0;
                if (v1 != last1) atomicOr(&present[v1 >> 5], 1u << (v1 & 31)), last1 = v1;
            }
        }
    }
    __syncthreads();

    // what does not depend on the object: the columns and rows of the region inside the image, the interior
    const W128 left = ones(max(-rx0, 0));       // columns before the image
    const W128 colvalid = ones(min(MS_COLS + 2 * h, W - rx0)) & W128{~left.lo, ~left.hi};
    const bool rowvalid = ry0 + rr >= 0 && ry0 + rr < H;
    const bool active = rr >= h && rr < h + TR && ry0 + rr < H;
    const int rc = active ? rr : h;                 // rows rc - R .. rc + R exist
    const int nvalid = min(MS_COLS, W - tx * MS_COLS);
    const u64 cv = nvalid == 64 ? ~0ull : (1ull << nvalid) - 1;
    const unsigned* rowp = lab[which] + rr * MS_PITCH;
    const int other = which ^ 1;

    for (int o = 1; o <= a.O; ++o) {
        if (!((__builtin_amdgcn_readfirstlane((int)present[o >> 5]) >> (o & 31)) & 1)) continue;      // absent from both maps: nothing from this tile
        // 1. the mask word
        const unsigned pat = (unsigned)o * 0x01010101u;
        W128 m{0, 0};
#pragma unroll
        for (int j = 0; j < 16; ++j) m.lo |= (u64)zero_bytes(rowp[j] ^ pat) << (4 * j);
        for (int j = 16; j < nb; ++j) m.hi |= (u64)zero_bytes(rowp[j] ^ pat) << (4 * (j - 16));
        M[which][rr] = m;
        __syncthreads();
        // 2. the boundary word (row 127 has no staged south neighbour; no interior row reaches it: 127 - h + R = 126)
        const W128 s = M[which][min(rr + 1, MS_RT - 1)];
        W128 b = (m ^ shr(m, 1)) | (m ^ s) | (m ^ shr(s, 1));
        b = rowvalid ? b & colvalid : W128{0, 0};
        B[which][rr] = b;
        __syncthreads();
        // 3. the disk
        W128 dil{0, 0}, grp{0, 0};
        for (int dy = 0; dy <= R; ++dy) {
            grp = grp | B[which][rc + dy] | B[which][rc - dy];
            const int hw = __builtin_amdgcn_readfirstlane(hwt[dy]);
            if (__builtin_amdgcn_readfirstlane(hwt[dy + 1]) != hw) {      // (hwt[R + 1] = -1: the last group)
                dil = dil | dilate(grp, hw);
                grp = W128{0, 0};
            }
        }
        // 4. the counts on the interior bits
        const W128 ob = B[other][rc], om = M[other][rc];
        const W128 mm = which ? m | om : m & om;
        int c0 = __builtin_popcountll(shr(b, h).lo & cv), c1 = __builtin_popcountll(shr(ob & dil, h).lo & cv), c2 = __builtin_popcountll(shr(mm, h).lo & cv);
        c0 = wave_reduce_sum_i32(active ? c0 : 0), c1 = wave_reduce_sum_i32(active ? c1 : 0), c2 = wave_reduce_sum_i32(active ? c2 : 0);
        if (lane == 0) part[wave][0] = c0, part[wave][1] = c1, part[wave][2] = c2;
        __syncthreads();
        if (tid < 6) {                              // pred: n_fg, gt_match, inter; truth: n_gt, fg_match, union
            const int mp = tid / 3, c = tid - 3 * mp, total = part[2 * mp][c] + part[2 * mp + 1][c];
            const int slot = (0x143052 >> (4 * tid)) & 7;
            if (total) atomicAdd(&a.counts[(f * a.O + (o - 1)) * 6 + slot], (u64)total);
        }
    }
}

__global__ __launch_bounds__(DV_NT) void zero_u64_kernel(u64* p, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * DV_NT + threadIdx.x;
    if (i < n) p[i] = 0;
}

}      // namespace

IVIT_EXPORT int ivit_upsample_argmax_u8(const float* seg, int Gh, int Gw, int r, int K, uint8_t* pred, ivit_stream_t stream)
{
    const char* who = "ivit_upsample_argmax_u8";
    IVIT_REQUIRE(seg && pred, "%s: NULL operand", who);
    IVIT_REQUIRE((uintptr_t)seg % 4 == 0, "%s: seg is not aligned to its element", who);
    IVIT_REQUIRE(Gh >= 1 && Gw >= 1, "%s: Gh=%d and Gw=%d must be at least 1", who, Gh, Gw);
    if (r < 1 || r > IVIT_UPSAMPLE_R_MAX || K < 1 || K > IVIT_PROPAGATE_CLASSES_MAX) {
        ivit_set_error("%s: unsupported geometry (r=%d outside [1, %d] or K=%d outside [1, %d])", who, r, IVIT_UPSAMPLE_R_MAX, K, IVIT_PROPAGATE_CLASSES_MAX);
        return IVIT_ERR_UNSUPPORTED;
    }
    const int64_t cells = (int64_t)Gh * Gw;
    IVIT_REQUIRE(cells < (1ll << 31) && cells * K < (1ll << 31) && cells * r * r < (1ll << 31),
                 "%s: %d x %d cells of %d x %d pixels and %d classes: 2^31 pixels or elements or more", who, Gh, Gw, r, r, K);
    const UpPlan p = up_plan(r);
    UpArgs a;
    a.seg = seg, a.Gh = Gh, a.Gw = Gw, a.r = r, a.K = K, a.pred = pred;
    a.CY = p.CY, a.CX = p.CX, a.gpr = p.gpr, a.pitch = p.pitch, a.bx = (Gw + p.CX - 1) / p.CX;
    a.packed = (uintptr_t)pred % 4 == 0 && ((int64_t)Gw * r) % 4 == 0 && (a.bx == 1 || (p.CX * r) % 4 == 0);
    const int64_t grid = (int64_t)((Gh + p.CY - 1) / p.CY) * a.bx;      // at most one workgroup per cell
    hipLaunchKernelGGL(upsample_argmax_kernel, dim3((unsigned)grid), dim3(DV_NT), 0, ivit_stream(stream), a);
    IVIT_CHECK_LAUNCH(who);
}

IVIT_EXPORT int ivit_mask_scores_u8(const uint8_t* pred, const uint8_t* truth, int n, int H, int W, int num_objects, int radius, int64_t* counts,
                                    ivit_stream_t stream)
{
    const char* who = "ivit_mask_scores_u8";
    IVIT_REQUIRE(pred && truth && counts, "%s: NULL operand", who);
    IVIT_REQUIRE((uintptr_t)counts % 8 == 0, "%s: counts is not aligned to its element", who);
    IVIT_REQUIRE(n >= 0, "%s: n=%d below 0", who, n);
    if (num_objects < 1 || num_objects > IVIT_SCORES_OBJECTS_MAX || radius < 0 || radius > MS_RMAX || H < 2 || W < 2 || (int64_t)H * W >= (1ll << 31)) {
        ivit_set_error("%s: unsupported geometry (num_objects=%d outside [1, %d], radius=%d outside [0, %d] or H=%d x W=%d: at least 2 each, below 2^31 pixels)",
                       who, num_objects, IVIT_SCORES_OBJECTS_MAX, radius, MS_RMAX, H, W);
        return IVIT_ERR_UNSUPPORTED;
    }
    MaskArgs a;
    a.pred = pred, a.truth = truth, a.H = H, a.W = W, a.O = num_objects, a.R = radius;
    const int TR = MS_RT - 2 * (radius + 1);
    a.tiles_x = (W + MS_COLS - 1) / MS_COLS, a.tiles_y = (H + TR - 1) / TR;
    a.counts = reinterpret_cast<u64*>(counts);
    for (int dy = 0; dy <= MS_RMAX; ++dy) {
        int w = 0;
        while (dy <= radius && (w + 1) * (w + 1) + dy * dy <= radius * radius) ++w;
        a.hw[dy] = (unsigned char)w;
    }
    const int64_t grid = (int64_t)n * a.tiles_x * a.tiles_y, cells = (int64_t)n * num_objects * 6;
    IVIT_REQUIRE(grid <= 0x7fffffff, "%s: %d frames of %d x %d pixels: too many workgroups", who, n, H, W);
    if (n == 0) return IVIT_OK;
    const hipStream_t st = ivit_stream(stream);
    hipLaunchKernelGGL(zero_u64_kernel, dim3((unsigned)((cells + DV_NT - 1) / DV_NT)), dim3(DV_NT), 0, st, a.counts, cells);
    hipLaunchKernelGGL(mask_scores_kernel, dim3((unsigned)grid), dim3(DV_NT), 0, st, a);
    IVIT_CHECK_LAUNCH(who);
}
