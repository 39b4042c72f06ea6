// transform.hip -- the reference's evaluation resize + crop on the device: torchvision Resize([s], BICUBIC) on a PIL image, then
// CenterCrop(c), byte for byte (Pillow's 8-bit bicubic resample, libImaging/Resample.c; DESIGN.md "Eval transform").
//
// Separable, horizontal pass first, uint8 between the passes, exactly as Pillow; only the crop is computed: the horizontal pass
// runs at the crop's columns over the source rows the crop's rows reach, the vertical pass at the crop's pixels.  Every output
// pixel depends on its own taps only, so the bytes are those of the full resize, cropped.  Three launches over a caller-owned
// workspace (any downscale factor: nothing is sized by the filter support except that workspace):
//   coeffs_kernel      per (image, axis, crop index): xmin, tap count and the 22-bit taps, float64 in Pillow's operation order
//   horizontal_kernel  per (image, intermediate row, crop column): 3 channels -> uint8 intermediate [rows][crop_w][3]
//   vertical_kernel    per (image, crop row, crop column): 3 channels -> planar uint8 out [B][3][crop_h][crop_w]
// The crop is crop_h x crop_w at a signed offset per axis (the _hw entries; the square entries pass crop_h = crop_w and refuse a
// negative offset): a crop longer than the resized axis is torchvision's CenterCrop zero padding.  The crop indices inside the
// resized image (span_of) are the only ones with taps, intermediate rows and intermediate columns; the vertical pass writes 0 at
// the others.
// -ffp-contract=off (Makefile) keeps every float64 step a single IEEE rounding; host and device evaluate the same functions.
#include <math.h>

#include "common.h"

namespace {

constexpr int kPrecisionBits = 22;
constexpr int kGeomCols = 6;            // h, w, new_h, new_w, top, left
constexpr int kTileX = 64, kTileY = 4;  // 256-thread blocks: 64 crop columns x 4 rows

__host__ __device__ inline double bicubic_filter(double x)
{
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

struct Axis {
    double scale, filterscale, support;
    int ksize;
};

__host__ __device__ inline Axis axis_of(int in, int out)
{
    Axis a;
    a.scale = (double)in / (double)out;
    a.filterscale = a.scale < 1.0 ? 1.0 : a.scale;
    a.support = 2.0 * a.filterscale;   // bicubic support 2.0
    a.ksize = (int)ceil(a.support) * 2 + 1;
    return a;
}

// first tap and tap count of output index o (Pillow's precompute_coeffs)
__host__ __device__ inline void axis_bounds(const Axis& a, int in, int o, int* xmin, int* xmax, double* center)
{
    const double c = (o + 0.5) * a.scale;
    int lo = (int)(c - a.support + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(c + a.support + 0.5);
    if (hi > in) hi = in;
    *xmin = lo;
    *xmax = hi - lo;
    *center = c;
}

// one axis: a crop of c at offset off of a resized axis of n pixels lies inside it (0 <= off <= n - c), or contains it with
// off = -(zeros in front), -(c - n) <= off <= 0
__host__ __device__ inline bool axis_ok(int n, int c, int off)
{
    return n >= 1 && (c <= n ? off >= 0 && off <= n - c : off <= 0 && off >= n - c);
}

__host__ __device__ inline bool geometry_ok(const int32_t* g, int crop_h, int crop_w)
{
    return g[0] >= 1 && g[1] >= 1 && axis_ok(g[2], crop_h, g[4]) && axis_ok(g[3], crop_w, g[5]);
}

// crop indices [lo, hi) of an axis_ok axis that lie inside the resized image (never empty); the others are zero padding
struct Span {
    int lo, hi;
};

__host__ __device__ inline Span span_of(int n, int c, int off)
{
    Span s;
    s.lo = off < 0 ? -off : 0;
    s.hi = n - off < c ? n - off : c;
    return s;
}

// intermediate rows image g needs: [ymin(first row inside), ymin(last row inside) + ymax(last row inside))
__host__ __device__ inline int rows_needed(const int32_t* g, int crop_h)
{
    const Axis a = axis_of(g[0], g[2]);
    const Span ys = span_of(g[2], crop_h, g[4]);
    int y0, n0, y1, n1;
    double c;
    axis_bounds(a, g[0], g[4] + ys.lo, &y0, &n0, &c);
    axis_bounds(a, g[0], g[4] + ys.hi - 1, &y1, &n1, &c);
    return y1 + n1 - y0;
}

// Workspace layout, int32 words then bytes, every block 16-byte aligned:
//   hcoef [B][2 + kh][crop_w]   row 0: xmin, row 1: tap count, rows 2..: taps (tap-major: a wave reads one tap of 64 columns at once)
//   vcoef [B][2 + kv][crop_h]
//   inter [B][rows][crop_w][3]  uint8 (padded columns are never written or read)
struct Layout {
    int64_t hcoef, vcoef, inter, bytes;   // byte offsets, total
};

inline int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

inline Layout layout_of(int batch, int crop_h, int crop_w, int kh, int kv, int rows)
{
    Layout L;
    L.hcoef = 0;
    L.vcoef = align16(L.hcoef + (int64_t)batch * (2 + kh) * crop_w * 4);
    L.inter = align16(L.vcoef + (int64_t)batch * (2 + kv) * crop_h * 4);
    L.bytes = align16(L.inter + (int64_t)batch * rows * crop_w * 3);
    return L;
}

// kRect = false, in all three kernels: the instantiation of the square entries -- the crop lies inside the resized image or the
// image gets no taps at all, so the two passes carry no span arithmetic (they are the kernels from before there were h x w crops).
// grid (ceil(max(crop_h, crop_w) / 64), B, 2): axis 0 horizontal (crop columns), 1 vertical (crop rows)
template <bool kRect>
__global__ void __launch_bounds__(64) coeffs_kernel(const int32_t* __restrict__ geom, int crop_h, int crop_w, int kh, int kv,
                                                    int32_t* hcoef, int32_t* vcoef)
{
    const int o = blockIdx.x * 64 + threadIdx.x;
    const int b = blockIdx.y, axis = blockIdx.z;
    const int crop = axis ? crop_h : crop_w;
    if (o >= crop) return;
    const int32_t* g = geom + (int64_t)b * kGeomCols;
    const int kmax = axis ? kv : kh;
    int32_t* rec = (axis ? vcoef : hcoef) + (int64_t)b * (2 + kmax) * crop + o;
    const int in = axis ? g[0] : g[1], out = axis ? g[2] : g[3], first = axis ? g[4] : g[5];
    // no taps (zero output), nothing out of bounds: a table the host did not validate, and the zero padding around the image
    bool taps = geometry_ok(g, crop_h, crop_w) && (kRect || (g[2] >= crop_h && g[3] >= crop_w));
    if (kRect && taps) {
        const Span s = span_of(out, crop, first);
        taps = o >= s.lo && o < s.hi;
    }
    if (!taps) {
        rec[0] = 0;
        rec[crop] = 0;
        return;
    }
    const Axis a = axis_of(in, out);
    int xmin, xmax;
    double center;
    axis_bounds(a, in, first + o, &xmin, &xmax, &center);
    if (xmax > kmax) xmax = kmax;
    const double ss = 1.0 / a.filterscale;
    double ww = 0.0;   // sequential, left to right, as Pillow
    for (int i = 0; i < xmax; i++) ww += bicubic_filter((i + xmin - center + 0.5) * ss);
    for (int i = 0; i < xmax; i++) {
        double k = bicubic_filter((i + xmin - center + 0.5) * ss);
        if (ww != 0.0) k /= ww;
        rec[(int64_t)(2 + i) * crop] = k < 0 ? (int)(-0.5 + k * (1 << kPrecisionBits)) : (int)(0.5 + k * (1 << kPrecisionBits));
    }
    rec[0] = xmin;
    rec[crop] = xmax;
}

IVIT_DEV uint8_t clip8(int v)
{
    v >>= kPrecisionBits;
    return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// grid (ceil(crop_w / 64), row_blocks, B), block (64, 4): rows strided by row_blocks * 4
template <bool kRect>
__global__ void __launch_bounds__(kTileX* kTileY) horizontal_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ offsets,
                                                                    const int32_t* __restrict__ geom, int crop_h, int crop_w, int kh,
                                                                    int kv, int rows, const int32_t* __restrict__ hcoef,
                                                                    const int32_t* __restrict__ vcoef, uint8_t* __restrict__ inter)
{
    const int x = blockIdx.x * kTileX + threadIdx.x;
    const int b = blockIdx.z;
    if (x >= crop_w) return;
    const int32_t* g = geom + (int64_t)b * kGeomCols;
    Span ys = {0, crop_h};
    if (kRect) {
        if (!geometry_ok(g, crop_h, crop_w)) return;
        const Span xs = span_of(g[3], crop_w, g[5]);
        if (x < xs.lo || x >= xs.hi) return;   // a padded column: the vertical pass does not read it
        ys = span_of(g[2], crop_h, g[4]);
    }
    const int w = g[1];
    const int32_t* hr = hcoef + (int64_t)b * (2 + kh) * crop_w + x;
    const int32_t* vr = vcoef + (int64_t)b * (2 + kv) * crop_h;
    const int ybase = vr[ys.lo];
    int nrows = vr[ys.hi - 1] + vr[crop_h + ys.hi - 1] - ybase;   // last inside crop row's ymin + ymax
    if (nrows > rows) nrows = rows;
    const int xmin = hr[0], xmax = hr[crop_w];
    const uint8_t* s = src + offsets[b] + (int64_t)xmin * 3;
    uint8_t* d = inter + ((int64_t)b * rows * crop_w + x) * 3;
    for (int r = blockIdx.y * kTileY + threadIdx.y; r < nrows; r += gridDim.y * kTileY) {
        const uint8_t* p = s + (int64_t)(ybase + r) * w * 3;
        int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
        for (int i = 0; i < xmax; i++) {
            const int k = hr[(int64_t)(2 + i) * crop_w];
            a0 += p[3 * i] * k;
            a1 += p[3 * i + 1] * k;
            a2 += p[3 * i + 2] * k;
        }
        uint8_t* q = d + (int64_t)r * crop_w * 3;
        q[0] = clip8(a0);
        q[1] = clip8(a1);
        q[2] = clip8(a2);
    }
}

// grid (ceil(crop_w / 64), ceil(crop_h / 4), B), block (64, 4); every pixel of out is written, the padding as 0
template <bool kRect>
__global__ void __launch_bounds__(kTileX* kTileY) vertical_kernel(const int32_t* __restrict__ geom, int crop_h, int crop_w, int kv,
                                                                  int rows, const int32_t* __restrict__ vcoef,
                                                                  const uint8_t* __restrict__ inter, uint8_t* __restrict__ out)
{
    const int x = blockIdx.x * kTileX + threadIdx.x, y = blockIdx.y * kTileY + threadIdx.y;
    const int b = blockIdx.z;
    if (x >= crop_w || y >= crop_h) return;
    const int32_t* g = geom + (int64_t)b * kGeomCols;
    const int32_t* vr = vcoef + (int64_t)b * (2 + kv) * crop_h;
    int y0 = 0, ymax = 0;   // no taps: 0
    if (!kRect) {
        y0 = vr[y] - vr[0];
        ymax = vr[crop_h + y];
    } else if (geometry_ok(g, crop_h, crop_w)) {
        const Span xs = span_of(g[3], crop_w, g[5]), ys = span_of(g[2], crop_h, g[4]);
        if (x >= xs.lo && x < xs.hi && y >= ys.lo && y < ys.hi) {
            y0 = vr[y] - vr[ys.lo];
            ymax = vr[crop_h + y];
        }
    }
    if (y0 + ymax > rows) ymax = rows - y0;
    const uint8_t* p = inter + (((int64_t)b * rows + y0) * crop_w + x) * 3;
    int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
    for (int j = 0; j < ymax; j++) {
        const int k = vr[(int64_t)(2 + j) * crop_h + y];
        const uint8_t* q = p + (int64_t)j * crop_w * 3;
        a0 += q[0] * k;
        a1 += q[1] * k;
        a2 += q[2] * k;
    }
    const int64_t plane = (int64_t)crop_h * crop_w;
    uint8_t* o = out + (int64_t)b * 3 * plane + (int64_t)y * crop_w + x;
    o[0] = clip8(a0);
    o[plane] = clip8(a1);
    o[2 * plane] = clip8(a2);
}

// plan3 and bytes of a batch whose rows the caller has validated (geometry_ok)
void plan_batch(const int32_t* geom, int batch, int crop_h, int crop_w, int32_t* plan3, int64_t* bytes)
{
    int kh = 1, kv = 1, rows = 1;
    for (int b = 0; b < batch; b++) {
        const int32_t* g = geom + (int64_t)b * kGeomCols;
        const int k1 = axis_of(g[1], g[3]).ksize, k2 = axis_of(g[0], g[2]).ksize, r = rows_needed(g, crop_h);
        kh = k1 > kh ? k1 : kh;
        kv = k2 > kv ? k2 : kv;
        rows = r > rows ? r : rows;
    }
    plan3[0] = kh;
    plan3[1] = kv;
    plan3[2] = rows;
    *bytes = layout_of(batch, crop_h, crop_w, kh, kv, rows).bytes;
}

// the two resize + crop entries behind their own crop checks (`who`: the entry's name in the messages)
template <bool kRect>
int resize_crop(const char* who, const uint8_t* src, const int64_t* offsets, const int32_t* geom, int batch, int crop_h, int crop_w,
                int ksize_h, int ksize_v, int rows, void* workspace, int64_t workspace_bytes, uint8_t* out, ivit_stream_t stream)
{
    IVIT_REQUIRE(ksize_h >= 1 && ksize_v >= 1 && rows >= 1, "%s: plan (%d, %d, %d) is not a workspace plan", who, ksize_h, ksize_v, rows);
    const Layout L = layout_of(batch, crop_h, crop_w, ksize_h, ksize_v, rows);
    IVIT_REQUIRE(workspace_bytes >= L.bytes, "%s: workspace of %lld bytes < %lld", who, (long long)workspace_bytes, (long long)L.bytes);
    if (batch == 0) return IVIT_OK;
    hipStream_t st = ivit_stream(stream);
    char* ws = static_cast<char*>(workspace);
    int32_t* hcoef = reinterpret_cast<int32_t*>(ws + L.hcoef);
    int32_t* vcoef = reinterpret_cast<int32_t*>(ws + L.vcoef);
    uint8_t* inter = reinterpret_cast<uint8_t*>(ws + L.inter);
    const int cx = (crop_w + kTileX - 1) / kTileX, cmax = crop_h > crop_w ? crop_h : crop_w;
    hipLaunchKernelGGL(coeffs_kernel<kRect>, dim3((cmax + 63) / 64, batch, 2), dim3(64), 0, st, geom, crop_h, crop_w, ksize_h, ksize_v, hcoef,
                       vcoef);
    // rows of one image strided over at most 128 row blocks: an ImageNet-size image (<= ~700 rows) in one sweep, a 4000 x 3000
    // source in a few
    const int ry = (rows + kTileY - 1) / kTileY < 128 ? (rows + kTileY - 1) / kTileY : 128;
    hipLaunchKernelGGL(horizontal_kernel<kRect>, dim3(cx, ry, batch), dim3(kTileX, kTileY), 0, st, src, offsets, geom, crop_h, crop_w, ksize_h,
                       ksize_v, rows, hcoef, vcoef, inter);
    hipLaunchKernelGGL(vertical_kernel<kRect>, dim3(cx, (crop_h + kTileY - 1) / kTileY, batch), dim3(kTileX, kTileY), 0, st, geom, crop_h,
                       crop_w, ksize_v, rows, vcoef, inter, out);
    IVIT_CHECK_LAUNCH(who);
}

// int(round(d / 2.0)) of d >= 0, Python's round half to even
inline int half_even(int d)
{
    const int q = d / 2;
    return (d & 1) ? q + (q & 1) : q;
}

// torchvision's Resize([s]): short side -> s, long side int(s * long / short) in float64; false where that leaves int32
bool short_side_resize(int h, int w, int s, int* nh, int* nw)
{
    const int sh = w <= h ? w : h, lg = w <= h ? h : w;
    const double nl = (double)((int64_t)s * lg) / (double)sh;   // Python: int(s * long / short)
    if (!(nl < 2147483647.0)) return false;
    *nh = w <= h ? (int)nl : s;
    *nw = w <= h ? s : (int)nl;
    return true;
}

}  // namespace


IVIT_EXPORT int ivit_eval_geometry(int h, int w, int resize_short, int crop, int32_t* out4)
{
    IVIT_REQUIRE(out4 != nullptr, "ivit_eval_geometry: NULL operand");
    if (h < 1 || w < 1 || resize_short < 1 || crop <= 32) {
        ivit_set_error("ivit_eval_geometry: unsupported geometry (%d x %d, resize %d, crop %d)", h, w, resize_short, crop);
        return IVIT_ERR_UNSUPPORTED;
    }
    int nh, nw;
    if (!short_side_resize(h, w, resize_short, &nh, &nw)) {
        ivit_set_error("ivit_eval_geometry: unsupported geometry (%d x %d, resize %d)", h, w, resize_short);
        return IVIT_ERR_UNSUPPORTED;
    }
    if (crop > nh || crop > nw) {   // torchvision would zero-pad: not a case of the reference's rules
        ivit_set_error("ivit_eval_geometry: unsupported geometry (crop %d > resized %d x %d)", crop, nh, nw);
        return IVIT_ERR_UNSUPPORTED;
    }
    out4[0] = nh;
    out4[1] = nw;
    out4[2] = half_even(nh - crop);
    out4[3] = half_even(nw - crop);
    return IVIT_OK;
}

IVIT_EXPORT int ivit_eval_geometry_hw(int h, int w, int resize_h, int resize_w, int crop_h, int crop_w, int pad, int32_t* out4)
{
    IVIT_REQUIRE(out4 != nullptr, "ivit_eval_geometry_hw: NULL operand");
    if (h < 1 || w < 1 || resize_h < 1 || resize_w < 0 || crop_h <= 32 || crop_w <= 32) {
        ivit_set_error("ivit_eval_geometry_hw: unsupported geometry (%d x %d, resize %d x %d, crop %d x %d)", h, w, resize_h, resize_w,
                       crop_h, crop_w);
        return IVIT_ERR_UNSUPPORTED;
    }
    int nh = resize_h, nw = resize_w;   // Resize((h, w)): exactly that size
    if (resize_w == 0 && !short_side_resize(h, w, resize_h, &nh, &nw)) {
        ivit_set_error("ivit_eval_geometry_hw: unsupported geometry (%d x %d, resize %d)", h, w, resize_h);
        return IVIT_ERR_UNSUPPORTED;
    }
    if (!pad && (crop_h > nh || crop_w > nw)) {   // torchvision would zero-pad, and the caller did not ask for that
        ivit_set_error("ivit_eval_geometry_hw: unsupported geometry (crop %d x %d > resized %d x %d without pad)", crop_h, crop_w, nh,
                       nw);
        return IVIT_ERR_UNSUPPORTED;
    }
    // CenterCrop pads (c - n) // 2 zeros in front (and (c - n + 1) // 2 behind): the offset of the crop is minus that
    out4[0] = nh;
    out4[1] = nw;
    out4[2] = crop_h <= nh ? half_even(nh - crop_h) : -((crop_h - nh) / 2);
    out4[3] = crop_w <= nw ? half_even(nw - crop_w) : -((crop_w - nw) / 2);
    return IVIT_OK;
}

IVIT_EXPORT int ivit_resize_crop_workspace(const int32_t* geom, int batch, int crop, int32_t* plan3, int64_t* bytes)
{
    IVIT_REQUIRE(geom != nullptr && plan3 != nullptr && bytes != nullptr, "ivit_resize_crop_workspace: NULL operand");
    IVIT_REQUIRE(batch >= 0, "ivit_resize_crop_workspace: batch %d < 0", batch);
    if (crop <= 32) {
        ivit_set_error("ivit_resize_crop_workspace: unsupported geometry (crop %d <= 32)", crop);
        return IVIT_ERR_UNSUPPORTED;
    }
    for (int b = 0; b < batch; b++) {
        const int32_t* g = geom + (int64_t)b * kGeomCols;
        if (g[2] < crop || g[3] < crop || !geometry_ok(g, crop, crop)) {   // this entry does not pad
            ivit_set_error("ivit_resize_crop_workspace: unsupported geometry (image %d: %d x %d -> %d x %d, crop %d at (%d, %d))", b,
                           g[0], g[1], g[2], g[3], crop, g[4], g[5]);
            return IVIT_ERR_UNSUPPORTED;
        }
    }
    plan_batch(geom, batch, crop, crop, plan3, bytes);
    return IVIT_OK;
}

IVIT_EXPORT int ivit_resize_crop_workspace_hw(const int32_t* geom, int batch, int crop_h, int crop_w, int32_t* plan3, int64_t* bytes)
{
    IVIT_REQUIRE(geom != nullptr && plan3 != nullptr && bytes != nullptr, "ivit_resize_crop_workspace_hw: NULL operand");
    IVIT_REQUIRE(batch >= 0, "ivit_resize_crop_workspace_hw: batch %d < 0", batch);
    if (crop_h <= 32 || crop_w <= 32) {
        ivit_set_error("ivit_resize_crop_workspace_hw: unsupported geometry (crop %d x %d: a side <= 32)", crop_h, crop_w);
        return IVIT_ERR_UNSUPPORTED;
    }
    for (int b = 0; b < batch; b++) {
        const int32_t* g = geom + (int64_t)b * kGeomCols;
        if (!geometry_ok(g, crop_h, crop_w)) {
            ivit_set_error("ivit_resize_crop_workspace_hw: unsupported geometry (image %d: %d x %d -> %d x %d, crop %d x %d at (%d, %d))",
                           b, g[0], g[1], g[2], g[3], crop_h, crop_w, g[4], g[5]);
            return IVIT_ERR_UNSUPPORTED;
        }
    }
    plan_batch(geom, batch, crop_h, crop_w, plan3, bytes);
    return IVIT_OK;
}

IVIT_EXPORT int ivit_resize_crop_bicubic_u8(const uint8_t* src, const int64_t* offsets, const int32_t* geom, int batch, int crop,
                                            int ksize_h, int ksize_v, int rows, void* workspace, int64_t workspace_bytes,
                                            uint8_t* out, ivit_stream_t stream)
{
    IVIT_REQUIRE(src && offsets && geom && workspace && out, "ivit_resize_crop_bicubic_u8: NULL operand");
    IVIT_REQUIRE(((uintptr_t)offsets & 7) == 0 && ((uintptr_t)geom & 3) == 0 && ((uintptr_t)workspace & 15) == 0,
                 "ivit_resize_crop_bicubic_u8: misaligned operand (offsets 8, geometry 4, workspace 16 bytes)");
    IVIT_REQUIRE(batch >= 0 && batch <= 65535, "ivit_resize_crop_bicubic_u8: batch %d outside 0..65535", batch);
    if (crop <= 32) {
        ivit_set_error("ivit_resize_crop_bicubic_u8: unsupported geometry (crop %d <= 32)", crop);
        return IVIT_ERR_UNSUPPORTED;
    }
    return resize_crop<false>("ivit_resize_crop_bicubic_u8", src, offsets, geom, batch, crop, crop, ksize_h, ksize_v, rows, workspace,
                       workspace_bytes, out, stream);
}

IVIT_EXPORT int ivit_resize_crop_bicubic_hw_u8(const uint8_t* src, const int64_t* offsets, const int32_t* geom, int batch, int crop_h,
                                               int crop_w, int ksize_h, int ksize_v, int rows, void* workspace,
                                               int64_t workspace_bytes, uint8_t* out, ivit_stream_t stream)
{
    IVIT_REQUIRE(src && offsets && geom && workspace && out, "ivit_resize_crop_bicubic_hw_u8: NULL operand");
    IVIT_REQUIRE(((uintptr_t)offsets & 7) == 0 && ((uintptr_t)geom & 3) == 0 && ((uintptr_t)workspace & 15) == 0,
                 "ivit_resize_crop_bicubic_hw_u8: misaligned operand (offsets 8, geometry 4, workspace 16 bytes)");
    IVIT_REQUIRE(batch >= 0 && batch <= 65535, "ivit_resize_crop_bicubic_hw_u8: batch %d outside 0..65535", batch);
    if (crop_h <= 32 || crop_w <= 32) {
        ivit_set_error("ivit_resize_crop_bicubic_hw_u8: unsupported geometry (crop %d x %d: a side <= 32)", crop_h, crop_w);
        return IVIT_ERR_UNSUPPORTED;
    }
    IVIT_REQUIRE(crop_h <= 65535 * kTileY, "ivit_resize_crop_bicubic_hw_u8: crop_h %d above %d (one launch)", crop_h, 65535 * kTileY);
    return resize_crop<true>("ivit_resize_crop_bicubic_hw_u8", src, offsets, geom, batch, crop_h, crop_w, ksize_h, ksize_v, rows, workspace,
                       workspace_bytes, out, stream);
}
