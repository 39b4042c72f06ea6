// transform.hip -- the reference's evaluation resize + crop on the device: torchvision Resize([s], BICUBIC) on a PIL image, then
// CenterCrop(c), byte for byte (Pillow's 8-bit bicubic resample, libImaging/Resample.c; DESIGN.md "Eval transform").
//
// Separable, horizontal pass first, uint8 between the passes, exactly as Pillow; only the crop is computed: the horizontal pass
// runs at the crop's columns over the source rows the crop's rows reach, the vertical pass at the crop's pixels.  Every output
// pixel depends on its own taps only, so the bytes are those of the full resize, cropped.  Three launches over a caller-owned
// workspace (any downscale factor: nothing is sized by the filter support except that workspace):
//   coeffs_kernel      per (image, axis, crop index): xmin, tap count and the 22-bit taps, float64 in Pillow's operation order
//   horizontal_kernel  per (image, intermediate row, crop column): 3 channels -> uint8 intermediate [rows][crop][3]
//   vertical_kernel    per (image, crop row, crop column): 3 channels -> planar uint8 out [B][3][crop][crop]
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

__host__ __device__ inline bool geometry_ok(const int32_t* g, int crop)
{
    const int h = g[0], w = g[1], nh = g[2], nw = g[3], top = g[4], left = g[5];
    return h >= 1 && w >= 1 && nh >= crop && nw >= crop && top >= 0 && left >= 0 && top <= nh - crop && left <= nw - crop;
}

// intermediate rows image g needs: [ymin(top), ymin(top + crop - 1) + ymax(top + crop - 1))
__host__ __device__ inline int rows_needed(const int32_t* g, int crop)
{
    const Axis a = axis_of(g[0], g[2]);
    int y0, n0, y1, n1;
    double c;
    axis_bounds(a, g[0], g[4], &y0, &n0, &c);
    axis_bounds(a, g[0], g[4] + crop - 1, &y1, &n1, &c);
    return y1 + n1 - y0;
}

// Workspace layout, int32 words then bytes, every block 16-byte aligned:
//   hcoef [B][2 + kh][crop]   row 0: xmin, row 1: tap count, rows 2..: taps (tap-major: a wave reads one tap of 64 columns at once)
//   vcoef [B][2 + kv][crop]
//   inter [B][rows][crop][3]  uint8
struct Layout {
    int64_t hcoef, vcoef, inter, bytes;   // byte offsets, total
};

inline int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

inline Layout layout_of(int batch, int crop, int kh, int kv, int rows)
{
    Layout L;
    L.hcoef = 0;
    L.vcoef = align16(L.hcoef + (int64_t)batch * (2 + kh) * crop * 4);
    L.inter = align16(L.vcoef + (int64_t)batch * (2 + kv) * crop * 4);
    L.bytes = align16(L.inter + (int64_t)batch * rows * crop * 3);
    return L;
}

// grid (ceil(crop / 64), B, 2): axis 0 horizontal (crop columns), 1 vertical (crop rows)
__global__ void __launch_bounds__(64) coeffs_kernel(const int32_t* __restrict__ geom, int crop, int kh, int kv, int32_t* hcoef,
                                                    int32_t* vcoef)
{
    const int o = blockIdx.x * 64 + threadIdx.x;
    const int b = blockIdx.y, axis = blockIdx.z;
    if (o >= crop) return;
    const int32_t* g = geom + (int64_t)b * kGeomCols;
    const int kmax = axis ? kv : kh;
    int32_t* rec = (axis ? vcoef : hcoef) + (int64_t)b * (2 + kmax) * crop + o;
    if (!geometry_ok(g, crop)) {   // a table the host did not validate: no taps (zero output), nothing out of bounds
        rec[0] = 0;
        rec[crop] = 0;
        return;
    }
    const int in = axis ? g[0] : g[1], out = axis ? g[2] : g[3], first = axis ? g[4] : g[5];
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

// grid (ceil(crop / 64), row_blocks, B), block (64, 4): rows strided by row_blocks * 4
__global__ void __launch_bounds__(kTileX* kTileY) horizontal_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ offsets,
                                                                    const int32_t* __restrict__ geom, int crop, int kh, int kv, int rows,
                                                                    const int32_t* __restrict__ hcoef, const int32_t* __restrict__ vcoef,
                                                                    uint8_t* __restrict__ inter)
{
    const int x = blockIdx.x * kTileX + threadIdx.x;
    const int b = blockIdx.z;
    if (x >= crop) return;
    const int32_t* g = geom + (int64_t)b * kGeomCols;
    const int w = g[1];
    const int32_t* hr = hcoef + (int64_t)b * (2 + kh) * crop + x;
    const int32_t* vr = vcoef + (int64_t)b * (2 + kv) * crop;
    const int ybase = vr[0];
    int nrows = vr[crop - 1] + vr[2 * crop - 1] - ybase;   // last crop row's ymin + ymax
    if (nrows > rows) nrows = rows;
    const int xmin = hr[0], xmax = hr[crop];
    const uint8_t* s = src + offsets[b] + (int64_t)xmin * 3;
    uint8_t* d = inter + ((int64_t)b * rows * crop + x) * 3;
    for (int r = blockIdx.y * kTileY + threadIdx.y; r < nrows; r += gridDim.y * kTileY) {
        const uint8_t* p = s + (int64_t)(ybase + r) * w * 3;
        int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
        for (int i = 0; i < xmax; i++) {
            const int k = hr[(int64_t)(2 + i) * crop];
            a0 += p[3 * i] * k;
            a1 += p[3 * i + 1] * k;
            a2 += p[3 * i + 2] * k;
        }
        uint8_t* q = d + (int64_t)r * crop * 3;
        q[0] = clip8(a0);
        q[1] = clip8(a1);
        q[2] = clip8(a2);
    }
}

// grid (ceil(crop / 64), ceil(crop / 4), B), block (64, 4)
__global__ void __launch_bounds__(kTileX* kTileY) vertical_kernel(const int32_t* __restrict__ geom, int crop, int kv, int rows,
                                                                  const int32_t* __restrict__ vcoef, const uint8_t* __restrict__ inter,
                                                                  uint8_t* __restrict__ out)
{
    const int x = blockIdx.x * kTileX + threadIdx.x, y = blockIdx.y * kTileY + threadIdx.y;
    const int b = blockIdx.z;
    if (x >= crop || y >= crop) return;
    const int32_t* vr = vcoef + (int64_t)b * (2 + kv) * crop;
    const int y0 = vr[y] - vr[0];
    int ymax = vr[crop + y];
    if (y0 + ymax > rows) ymax = rows - y0;
    const uint8_t* p = inter + (((int64_t)b * rows + y0) * crop + x) * 3;
    int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
    for (int j = 0; j < ymax; j++) {
        const int k = vr[(int64_t)(2 + j) * crop + y];
        const uint8_t* q = p + (int64_t)j * crop * 3;
        a0 += q[0] * k;
        a1 += q[1] * k;
        a2 += q[2] * k;
    }
    const int64_t plane = (int64_t)crop * crop;
    uint8_t* o = out + (int64_t)b * 3 * plane + (int64_t)y * crop + x;
    o[0] = clip8(a0);
    o[plane] = clip8(a1);
    o[2 * plane] = clip8(a2);
}

}  // namespace

IVIT_EXPORT int ivit_eval_geometry(int h, int w, int resize_short, int crop, int32_t* out4)
{
    IVIT_REQUIRE(out4 != nullptr, "ivit_eval_geometry: NULL operand");
    if (h < 1 || w < 1 || resize_short < 1 || crop <= 32) {
        ivit_set_error("ivit_eval_geometry: unsupported geometry (%d x %d, resize %d, crop %d)", h, w, resize_short, crop);
        return IVIT_ERR_UNSUPPORTED;
    }
    const int sh = w <= h ? w : h, lg = w <= h ? h : w;
    const double nl = (double)((int64_t)resize_short * lg) / (double)sh;   // Python: int(s * long / short)
    if (!(nl < 2147483647.0)) {
        ivit_set_error("ivit_eval_geometry: unsupported geometry (%d x %d, resize %d)", h, w, resize_short);
        return IVIT_ERR_UNSUPPORTED;
    }
    const int new_long = (int)nl;
    const int nh = w <= h ? new_long : resize_short, nw = w <= h ? resize_short : new_long;
    if (crop > nh || crop > nw) {   // torchvision would zero-pad: not a case of the reference's rules
        ivit_set_error("ivit_eval_geometry: unsupported geometry (crop %d > resized %d x %d)", crop, nh, nw);
        return IVIT_ERR_UNSUPPORTED;
    }
    // int(round(d / 2.0)), Python's round half to even
    auto half_even = [](int d) { const int q = d / 2; return (d & 1) ? q + (q & 1) : q; };
    out4[0] = nh;
    out4[1] = nw;
    out4[2] = half_even(nh - crop);
    out4[3] = half_even(nw - crop);
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
    int kh = 1, kv = 1, rows = 1;
    for (int b = 0; b < batch; b++) {
        const int32_t* g = geom + (int64_t)b * kGeomCols;
        if (!geometry_ok(g, crop)) {
            ivit_set_error("ivit_resize_crop_workspace: unsupported geometry (image %d: %d x %d -> %d x %d, crop %d at (%d, %d))", b,
                           g[0], g[1], g[2], g[3], crop, g[4], g[5]);
            return IVIT_ERR_UNSUPPORTED;
        }
        const int k1 = axis_of(g[1], g[3]).ksize, k2 = axis_of(g[0], g[2]).ksize, r = rows_needed(g, crop);
        kh = k1 > kh ? k1 : kh;
        kv = k2 > kv ? k2 : kv;
        rows = r > rows ? r : rows;
    }
    plan3[0] = kh;
    plan3[1] = kv;
    plan3[2] = rows;
    *bytes = layout_of(batch, crop, kh, kv, rows).bytes;
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
    IVIT_REQUIRE(ksize_h >= 1 && ksize_v >= 1 && rows >= 1, "ivit_resize_crop_bicubic_u8: plan (%d, %d, %d) is not a workspace plan",
                 ksize_h, ksize_v, rows);
    const Layout L = layout_of(batch, crop, ksize_h, ksize_v, rows);
    IVIT_REQUIRE(workspace_bytes >= L.bytes, "ivit_resize_crop_bicubic_u8: workspace of %lld bytes < %lld", (long long)workspace_bytes,
                 (long long)L.bytes);
    if (batch == 0) return IVIT_OK;
    hipStream_t st = ivit_stream(stream);
    char* ws = static_cast<char*>(workspace);
    int32_t* hcoef = reinterpret_cast<int32_t*>(ws + L.hcoef);
    int32_t* vcoef = reinterpret_cast<int32_t*>(ws + L.vcoef);
    uint8_t* inter = reinterpret_cast<uint8_t*>(ws + L.inter);
    const int cx = (crop + kTileX - 1) / kTileX;
    hipLaunchKernelGGL(coeffs_kernel, dim3(cx, batch, 2), dim3(64), 0, st, geom, crop, ksize_h, ksize_v, hcoef, vcoef);
    // rows of one image strided over at most 128 row blocks: an ImageNet-size image (<= ~700 rows) in one sweep, a 4000 x 3000
    // source in a few
    const int ry = (rows + kTileY - 1) / kTileY < 128 ? (rows + kTileY - 1) / kTileY : 128;
    hipLaunchKernelGGL(horizontal_kernel, dim3(cx, ry, batch), dim3(kTileX, kTileY), 0, st, src, offsets, geom, crop, ksize_h, ksize_v,
                       rows, hcoef, vcoef, inter);
    hipLaunchKernelGGL(vertical_kernel, dim3(cx, (crop + kTileY - 1) / kTileY, batch), dim3(kTileX, kTileY), 0, st, geom, crop, ksize_v,
                       rows, vcoef, inter, out);
    IVIT_CHECK_LAUNCH("ivit_resize_crop_bicubic_u8");
}
