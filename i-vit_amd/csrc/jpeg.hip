// jpeg.hip -- baseline JPEG decoding on the device, byte for byte what libjpeg-turbo gives at its defaults (JDCT_ISLOW, fancy
// upsampling) under Pillow's Image.open(f).convert("RGB") (DESIGN.md §11 "JPEG decoding").
//
// Host side (no HIP runtime call: callable in loader worker processes):
//   ivit_jpeg_probe        header probe: size, components, sampling; IVIT_ERR_UNSUPPORTED with the reason for every other file
//   ivit_jpeg_plan_image   one image's self-contained plan section: natural-order quantisation tables, derived Huffman tables,
//                          component geometry, restart segments and the de-stuffed entropy bytes
//   ivit_jpeg_workspace    a batch index over a run of sections (+ workspace size)
//   ivit_jpeg_decode_host  one image, serially, with the same primitives as the kernels (the CPU tests' reference)
// Device side (ivit_jpeg_decode_u8, seven launches on one stream):
//   sync_kernel    every lane decodes one kSubBits subsequence of a restart segment from a guessed state, then the lanes of a
//                  workgroup take their left neighbour's exit state until nothing changes (self-synchronising decoding)
//   fix_kernel     workgroup boundaries: one lane per image continues serially from the true state until it meets a recorded one
//   scan_kernel    per image: segmented exclusive prefix sum of the blocks each subsequence completes -> every block's slot
//   write_kernel   every lane decodes its subsequence again and writes int16 coefficients (DC as differences) to the slots
//   dc_kernel      per image: segmented prefix sum of the DC differences per (component, restart segment)
//   idct_kernel    per block: dequantise + jpeg_idct_islow -> component planes at padded stride
//   color_kernel   per pixel: fancy upsampling + YCbCr -> RGB, HWC uint8 at the caller's packed offsets
// The primitives -- huff_step (one codeword of a block), idct_islow (one block), pixel_rgb (one output pixel) -- are
// __host__ __device__ and shared with ivit_jpeg_decode_host.
#include <string.h>

#include <vector>

#include "common.h"

namespace {

constexpr int kSubBits = 4096;   // subsequence length in bits (512 entropy bytes)
constexpr int kSyncLanes = 256;  // subsequences synchronised inside one workgroup
constexpr int kLook = 9;         // Huffman lookahead bits

// jpeg_natural_order + 16 entries of 63 "for safety in decoder" (jutils.c): a corrupt run past 63 lands on 63, as in libjpeg
constexpr int kNatural[80] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13,
                              6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                              39, 46, 53, 60, 61, 54, 47, 55, 62, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63};

// jdhuff.c d_derived_tbl
struct HuffTab {
    int32_t maxcode[18];       // largest code of length l, -1 if none
    int32_t valoffset[18];     // huffval index of a code of length l = code + valoffset[l]
    uint16_t look[1 << kLook];  // (length << 8) | symbol for codes of <= kLook bits, 0 otherwise
    uint8_t huffval[256];
};

struct Seg {                  // one restart segment
    int64_t off;              // its de-stuffed bytes: section + ent_off + off
    int32_t nbytes, sub_first, nsub, first_mcu, nmcu, pad;
};

// One image's plan section (16-byte aligned, relocatable: every offset is relative to the section)
struct Sec {
    int64_t bytes;
    int32_t h, w, ncomp, hmax, vmax, mcux, mcuy, bpm, nseg, nsub, ntab, sampling;
    int32_t ch[3], cv[3], cdc[3], cac[3], dw[3], dh[3], pw[3], ph[3];
    int32_t blk_comp[8];      // block of the MCU -> component
    int32_t blk_first[3];     // first block of component c in the MCU
    int32_t pad0;
    int64_t plane_off[3], plane_bytes, tab_off, seg_off, ent_off, nblocks;
    uint16_t qt[3][64];       // per component, natural order
};

struct Idx {                  // the batch index (host-built, one row per image)
    int64_t sec;              // section offset in the plan, -1: not decoded here (fallback image)
    int64_t out;              // HWC output offset
    int64_t coef;             // first block slot
    int64_t plane;            // first plane byte
    int32_t sub_first, nsub;
};

struct Dec {
    int32_t p, blk, z;        // bit position in the segment, block of the MCU, next coefficient (0: the DC)
};

inline int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }
inline int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

__host__ __device__ inline uint64_t pack_state(const Dec& s) { return ((uint64_t)(uint32_t)s.p << 16) | ((uint64_t)s.blk << 8) | (uint64_t)s.z; }
__host__ __device__ inline Dec unpack_state(uint64_t v)
{
    Dec s;
    s.p = (int32_t)(uint32_t)(v >> 16);
    s.blk = (int32_t)((v >> 8) & 255);
    s.z = (int32_t)(v & 255);
    return s;
}

// 32 bits of the segment from bit p, MSB first; bytes past the segment read as 0 (libjpeg inserts zeros at a marker)
__host__ __device__ inline uint32_t peek32(const uint8_t* d, int32_t n, int32_t p)
{
    const int32_t byte = p >> 3;
    uint64_t v = 0;
    if (byte + 5 <= n) {
        for (int i = 0; i < 5; i++) v = (v << 8) | d[byte + i];
    } else {
        for (int i = 0; i < 5; i++) v = (v << 8) | (byte + i < n ? d[byte + i] : 0);
    }
    return (uint32_t)(v >> (8 - (p & 7)));
}

// Primitive 1: one codeword of the block in progress (jdhuff.c decode_mcu_slow: DC difference + HUFF_EXTEND, AC run/size, EOB,
// ZRL).  pos / val: the coefficient written (natural index, -1 if none).  Returns false for a code that matches no table entry;
// the state still advances (16 bits, symbol 0) so that decoding from a wrong guessed state stays deterministic.  A finished block
// moves the state to the next block of the MCU.
__host__ __device__ inline bool huff_step(const Sec* S, const HuffTab* tabs, const uint8_t* d, int32_t n, Dec& s, int& pos, int& val,
                                          bool& block_done)
{
    const int c = S->blk_comp[s.blk];
    const HuffTab& T = tabs[s.z == 0 ? S->cdc[c] : S->cac[c]];
    const uint32_t w = peek32(d, n, s.p);
    int len, sym;
    bool ok = true;
    const uint32_t e = T.look[w >> (32 - kLook)];
    if (e) {
        len = (int)(e >> 8);
        sym = (int)(e & 255);
    } else {
        len = kLook + 1;
        while (len <= 16 && (int32_t)(w >> (32 - len)) > T.maxcode[len]) len++;
        if (len > 16) {
            ok = false;
            len = 16;
            sym = 0;
        } else {
            sym = T.huffval[((int32_t)(w >> (32 - len)) + T.valoffset[len]) & 255];
        }
    }
    const int size = s.z == 0 ? sym : (sym & 15);
    int v = 0;
    if (size) {
        const int x = (int)((w << len) >> (32 - size));
        v = x < (1 << (size - 1)) ? x - (1 << size) + 1 : x;   // HUFF_EXTEND
    }
    s.p += len + size;
    pos = -1;
    if (s.z == 0) {
        pos = 0;
        val = v;
        s.z = 1;
    } else if (size) {
        s.z += sym >> 4;
        pos = kNatural[s.z];
        val = v;
        s.z++;
    } else if ((sym >> 4) == 15) {
        s.z += 16;
    } else {
        s.z = 64;
    }
    block_done = s.z >= 64;
    if (block_done) {
        s.z = 0;
        s.blk = s.blk + 1 == S->bpm ? 0 : s.blk + 1;
    }
    return ok;
}

// Primitive 2: dequantise + jpeg_idct_islow (jidctint.c), 8 x 8 uint8 at out (stride)
#define JFIX_0_298631336 2446
#define JFIX_0_390180644 3196
#define JFIX_0_541196100 4433
#define JFIX_0_765366865 6270
#define JFIX_0_899976223 7373
#define JFIX_1_175875602 9633
#define JFIX_1_501321110 12299
#define JFIX_1_847759065 15137
#define JFIX_1_961570560 16069
#define JFIX_2_053119869 16819
#define JFIX_2_562915447 20995
#define JFIX_3_072711026 25172

// range_limit[x & RANGE_MASK] of the post-IDCT table (jdmaster.c prepare_range_limit_table): x + 128 clamped, wrapping mod 1024
__host__ __device__ inline uint8_t idct_limit(int x)
{
    x &= 1023;
    if (x >= 512) x -= 1024;
    x += 128;
    return (uint8_t)(x < 0 ? 0 : x > 255 ? 255 : x);
}

__host__ __device__ inline void idct_islow(const int16_t* coef, const uint16_t* q, uint8_t* out, int stride)
{
    constexpr int CB = 13, P1 = 2;
    int ws[64];
    for (int col = 0; col < 8; col++) {
        const int16_t* in = coef + col;
        const uint16_t* qq = q + col;
        int* w = ws + col;
        if (in[8] == 0 && in[16] == 0 && in[24] == 0 && in[32] == 0 && in[40] == 0 && in[48] == 0 && in[56] == 0) {
            const int dc = (int)((unsigned)(in[0] * (int)qq[0]) << P1);
            for (int r = 0; r < 8; r++) w[8 * r] = dc;
            continue;
        }
        int64_t z1, z2, z3, z4, z5, t0, t1, t2, t3, t10, t11, t12, t13;
        z2 = in[16] * (int)qq[16];
        z3 = in[48] * (int)qq[48];
        z1 = (z2 + z3) * JFIX_0_541196100;
        t2 = z1 + z3 * -JFIX_1_847759065;
        t3 = z1 + z2 * JFIX_0_765366865;
        z2 = in[0] * (int)qq[0];
        z3 = in[32] * (int)qq[32];
        t0 = (z2 + z3) * (1 << CB);
        t1 = (z2 - z3) * (1 << CB);
        t10 = t0 + t3;
        t13 = t0 - t3;
        t11 = t1 + t2;
        t12 = t1 - t2;
        t0 = in[56] * (int)qq[56];
        t1 = in[40] * (int)qq[40];
        t2 = in[24] * (int)qq[24];
        t3 = in[8] * (int)qq[8];
        z1 = t0 + t3;
        z2 = t1 + t2;
        z3 = t0 + t2;
        z4 = t1 + t3;
        z5 = (z3 + z4) * JFIX_1_175875602;
        t0 = t0 * JFIX_0_298631336;
        t1 = t1 * JFIX_2_053119869;
        t2 = t2 * JFIX_3_072711026;
        t3 = t3 * JFIX_1_501321110;
        z1 = z1 * -JFIX_0_899976223;
        z2 = z2 * -JFIX_2_562915447;
        z3 = z3 * -JFIX_1_961570560;
        z4 = z4 * -JFIX_0_390180644;
        z3 += z5;
        z4 += z5;
        t0 += z1 + z3;
        t1 += z2 + z4;
        t2 += z2 + z3;
        t3 += z1 + z4;
        constexpr int sh = CB - P1;
        constexpr int64_t rnd = (int64_t)1 << (sh - 1);
        w[0] = (int)((t10 + t3 + rnd) >> sh);
        w[56] = (int)((t10 - t3 + rnd) >> sh);
        w[8] = (int)((t11 + t2 + rnd) >> sh);
        w[48] = (int)((t11 - t2 + rnd) >> sh);
        w[16] = (int)((t12 + t1 + rnd) >> sh);
        w[40] = (int)((t12 - t1 + rnd) >> sh);
        w[24] = (int)((t13 + t0 + rnd) >> sh);
        w[32] = (int)((t13 - t0 + rnd) >> sh);
    }
    for (int row = 0; row < 8; row++) {
        const int* w = ws + 8 * row;
        uint8_t* o = out + (int64_t)row * stride;
        if (w[1] == 0 && w[2] == 0 && w[3] == 0 && w[4] == 0 && w[5] == 0 && w[6] == 0 && w[7] == 0) {
            const uint8_t dc = idct_limit((int)(((int64_t)w[0] + (1 << (P1 + 2))) >> (P1 + 3)));
            for (int i = 0; i < 8; i++) o[i] = dc;
            continue;
        }
        int64_t z1, z2, z3, z4, z5, t0, t1, t2, t3, t10, t11, t12, t13;
        z2 = w[2];
        z3 = w[6];
        z1 = (z2 + z3) * JFIX_0_541196100;
        t2 = z1 + z3 * -JFIX_1_847759065;
        t3 = z1 + z2 * JFIX_0_765366865;
        t0 = ((int64_t)w[0] + w[4]) * (1 << CB);
        t1 = ((int64_t)w[0] - w[4]) * (1 << CB);
        t10 = t0 + t3;
        t13 = t0 - t3;
        t11 = t1 + t2;
        t12 = t1 - t2;
        t0 = w[7];
        t1 = w[5];
        t2 = w[3];
        t3 = w[1];
        z1 = t0 + t3;
        z2 = t1 + t2;
        z3 = t0 + t2;
        z4 = t1 + t3;
        z5 = (z3 + z4) * JFIX_1_175875602;
        t0 = t0 * JFIX_0_298631336;
        t1 = t1 * JFIX_2_053119869;
        t2 = t2 * JFIX_3_072711026;
        t3 = t3 * JFIX_1_501321110;
        z1 = z1 * -JFIX_0_899976223;
        z2 = z2 * -JFIX_2_562915447;
        z3 = z3 * -JFIX_1_961570560;
        z4 = z4 * -JFIX_0_390180644;
        z3 += z5;
        z4 += z5;
        t0 += z1 + z3;
        t1 += z2 + z4;
        t2 += z2 + z3;
        t3 += z1 + z4;
        constexpr int sh = CB + P1 + 3;
        constexpr int64_t rnd = (int64_t)1 << (sh - 1);
        o[0] = idct_limit((int)((t10 + t3 + rnd) >> sh));
        o[7] = idct_limit((int)((t10 - t3 + rnd) >> sh));
        o[1] = idct_limit((int)((t11 + t2 + rnd) >> sh));
        o[6] = idct_limit((int)((t11 - t2 + rnd) >> sh));
        o[2] = idct_limit((int)((t12 + t1 + rnd) >> sh));
        o[5] = idct_limit((int)((t12 - t1 + rnd) >> sh));
        o[3] = idct_limit((int)((t13 + t0 + rnd) >> sh));
        o[4] = idct_limit((int)((t13 - t0 + rnd) >> sh));
    }
}

// Primitive 3: one output pixel -- fancy upsampling (jdsample.c h2v1 / h2v2_fancy_upsample, edge rows and columns replicated as
// jdmainct.c and the SIMD paths do) + ycc_rgb_convert (jdcolor.c, SCALEBITS 16); grayscale replicated to RGB
__host__ __device__ inline uint8_t clamp255(int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

__host__ __device__ inline int chroma(const Sec* S, const uint8_t* plane, int c, int y, int x)
{
    const int pw = S->pw[c], dw = S->dw[c], dh = S->dh[c];
    if (S->sampling == 1) return plane[(int64_t)y * pw + x];
    const int j = x >> 1;
    if (dw <= 2) return plane[(int64_t)(S->sampling == 3 ? y >> 1 : y) * pw + j];   // jdsample.c: fancy only for widths > 2
    const int jn = (x & 1) ? (j + 1 < dw ? j + 1 : dw - 1) : (j > 0 ? j - 1 : 0);
    if (S->sampling == 2) {   // h2v1: 3/4 nearer + 1/4 further, biases +1 / +2, >> 2
        const uint8_t* r = plane + (int64_t)y * pw;
        return (3 * r[j] + r[jn] + ((x & 1) ? 2 : 1)) >> 2;
    }
    // h2v2: column sums 3 * nearest row + next nearest (above for even rows, below for odd), then 3/4 + 1/4, biases +8 / +7, >> 4
    const int i = y >> 1;
    const int in = (y & 1) ? (i + 1 < dh ? i + 1 : dh - 1) : (i > 0 ? i - 1 : 0);
    const uint8_t* r0 = plane + (int64_t)i * pw;
    const uint8_t* r1 = plane + (int64_t)in * pw;
    const int cj = 3 * r0[j] + r1[j], cn = 3 * r0[jn] + r1[jn];
    return (3 * cj + cn + ((x & 1) ? 7 : 8)) >> 4;
}

__host__ __device__ inline void pixel_rgb(const Sec* S, const uint8_t* planes, int y, int x, uint8_t* rgb)
{
    const int Y = planes[S->plane_off[0] + (int64_t)y * S->pw[0] + x];
    if (S->ncomp == 1) {
        rgb[0] = rgb[1] = rgb[2] = (uint8_t)Y;
        return;
    }
    const int cb = chroma(S, planes + S->plane_off[1], 1, y, x) - 128;
    const int cr = chroma(S, planes + S->plane_off[2], 2, y, x) - 128;
    constexpr int kHalf = 1 << 15;
    const int r_cr = (int)(((int64_t)91881 * cr + kHalf) >> 16);               // FIX(1.40200)
    const int b_cb = (int)(((int64_t)116130 * cb + kHalf) >> 16);              // FIX(1.77200)
    const int g = (int)(((int64_t)-22554 * cb + kHalf + (int64_t)-46802 * cr) >> 16);   // FIX(0.34414), FIX(0.71414)
    rgb[0] = clamp255(Y + r_cr);
    rgb[1] = clamp255(Y + g);
    rgb[2] = clamp255(Y + b_cb);
}

__host__ __device__ inline const HuffTab* tabs_of(const Sec* S) { return reinterpret_cast<const HuffTab*>(reinterpret_cast<const char*>(S) + S->tab_off); }
__host__ __device__ inline const Seg* segs_of(const Sec* S) { return reinterpret_cast<const Seg*>(reinterpret_cast<const char*>(S) + S->seg_off); }
__host__ __device__ inline const uint8_t* ent_of(const Sec* S, const Seg& g) { return reinterpret_cast<const uint8_t*>(S) + S->ent_off + g.off; }

// block slot (MCU-major: mcu * bpm + block of the MCU) -> plane position
__host__ __device__ inline void block_origin(const Sec* S, int64_t slot, int* comp, int* px, int* py)
{
    const int mcu = (int)(slot / S->bpm), blk = (int)(slot % S->bpm);
    const int c = S->blk_comp[blk], li = blk - S->blk_first[c];
    *comp = c;
    *px = ((mcu % S->mcux) * S->ch[c] + li % S->ch[c]) * 8;
    *py = ((mcu / S->mcux) * S->cv[c] + li / S->ch[c]) * 8;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Host: parsing

struct Parsed {
    int h = 0, w = 0, ncomp = 0, precision = 0, sof = -1, restart = 0;
    int cid[4] = {}, ch[4] = {}, cv[4] = {}, ctq[4] = {}, ctd[4] = {}, cta[4] = {};
    uint16_t qt[4][64] = {};
    bool qt_ok[4] = {};
    uint8_t bits[8][17] = {}, vals[8][256] = {};
    bool ht_ok[8] = {};   // 0-3 DC, 4-7 AC
    bool jfif = false, adobe = false;
    int adobe_transform = -1;
    std::vector<int64_t> seg_begin, seg_len;   // de-stuffed segment bytes
    int64_t ent_bytes = 0;
    int64_t scan_pos = 0;                      // first entropy byte in the file
};

#define JFAIL(...)                         \
    do {                                   \
        ivit_set_error(__VA_ARGS__);       \
        return IVIT_ERR_UNSUPPORTED;       \
    } while (0)

int u16be(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// jdhuff.c jpeg_make_d_derived_tbl; false where libjpeg stops with JERR_BAD_HUFF_TABLE
bool derive(const uint8_t* bits, const uint8_t* vals, bool dc, HuffTab* T)
{
    int huffsize[257], p = 0;
    unsigned huffcode[257];
    for (int l = 1; l <= 16; l++) {
        const int i = bits[l];
        if (p + i > 256) return false;
        for (int k = 0; k < i; k++) huffsize[p++] = l;
    }
    huffsize[p] = 0;
    const int nsym = p;
    unsigned code = 0;
    int si = huffsize[0];
    p = 0;
    while (huffsize[p]) {
        while (huffsize[p] == si) huffcode[p++] = code++;
        if ((int64_t)code >= ((int64_t)1 << si)) return false;
        code <<= 1;
        si++;
    }
    memset(T, 0, sizeof(*T));
    p = 0;
    for (int l = 1; l <= 16; l++) {
        if (bits[l]) {
            T->valoffset[l] = p - (int)huffcode[p];
            p += bits[l];
            T->maxcode[l] = (int)huffcode[p - 1];
        } else {
            T->maxcode[l] = -1;
        }
    }
    T->maxcode[0] = -1;
    T->maxcode[17] = 0xFFFFF;
    p = 0;
    for (int l = 1; l <= kLook; l++) {
        for (int i = 1; i <= bits[l]; i++, p++) {
            const unsigned base = huffcode[p] << (kLook - l);
            for (unsigned k = 0; k < (1u << (kLook - l)); k++) T->look[base + k] = (uint16_t)((l << 8) | vals[p]);
        }
    }
    memcpy(T->huffval, vals, 256);
    if (dc)
        for (int i = 0; i < nsym; i++)
            if (vals[i] > 15) return false;
    return true;
}

// Walks the markers of one file; with ent != nullptr also writes the de-stuffed entropy bytes.  IVIT_ERR_UNSUPPORTED + the reason
// for every file the device does not decode.
int parse(const uint8_t* d, int64_t n, Parsed& P, uint8_t* ent)
{
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) JFAIL("not a JPEG file (no SOI marker)");
    int64_t pos = 2;
    bool sos = false;
    for (;;) {
        if (pos >= n) JFAIL("truncated file (no scan)");
        if (d[pos] != 0xFF) JFAIL("corrupt file (bytes between markers)");
        while (pos < n && d[pos] == 0xFF) pos++;
        if (pos >= n) JFAIL("truncated file (no scan)");
        const int m = d[pos++];
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) JFAIL("corrupt file (marker 0x%02X outside a scan)", m);
        if (m == 0xD9) JFAIL("no scan before EOI");
        if (pos + 2 > n) JFAIL("truncated file (marker 0x%02X)", m);
        const int len = u16be(d + pos);
        if (len < 2 || pos + len > n) JFAIL("truncated file (marker 0x%02X of %d bytes)", m, len);
        const uint8_t* s = d + pos + 2;
        const int L = len - 2;
        pos += len;
        if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
            if (P.sof >= 0) JFAIL("corrupt file (two frame headers)");
            P.sof = m - 0xC0;
            if (m == 0xC2 || m == 0xC6) JFAIL("progressive JPEG (SOF%d)", m - 0xC0);
            if (m == 0xC3 || m == 0xC7) JFAIL("lossless JPEG (SOF%d)", m - 0xC0);
            if (m == 0xC5) JFAIL("hierarchical JPEG (SOF5)");
            if (m >= 0xC9) JFAIL("arithmetic-coded JPEG (SOF%d)", m - 0xC0);
            if (L < 6) JFAIL("corrupt frame header");
            P.precision = s[0];
            P.h = u16be(s + 1);
            P.w = u16be(s + 3);
            P.ncomp = s[5];
            if (P.precision != 8) JFAIL("%d-bit samples", P.precision);
            if (P.h == 0) JFAIL("height defined by a DNL marker");
            if (P.w == 0) JFAIL("corrupt frame header (width 0)");
            if (P.ncomp != 1 && P.ncomp != 3) JFAIL("%d components (CMYK / YCCK or other)", P.ncomp);
            if (L < 6 + 3 * P.ncomp) JFAIL("corrupt frame header");
            for (int c = 0; c < P.ncomp; c++) {
                P.cid[c] = s[6 + 3 * c];
                P.ch[c] = s[7 + 3 * c] >> 4;
                P.cv[c] = s[7 + 3 * c] & 15;
                P.ctq[c] = s[8 + 3 * c];
                if (P.ch[c] < 1 || P.ch[c] > 4 || P.cv[c] < 1 || P.cv[c] > 4 || P.ctq[c] > 3) JFAIL("corrupt frame header (component %d)", c);
            }
        } else if (m == 0xC4) {   // DHT
            int k = 0;
            while (k < L) {
                if (k + 17 > L) JFAIL("corrupt Huffman table");
                const int tc = s[k] >> 4, th = s[k] & 15;
                if (tc > 1 || th > 3) JFAIL("corrupt Huffman table (class %d, id %d)", tc, th);
                const int t = tc * 4 + th;
                int cnt = 0;
                P.bits[t][0] = 0;
                for (int i = 1; i <= 16; i++) cnt += (P.bits[t][i] = s[k + i]);
                if (cnt > 256 || k + 17 + cnt > L) JFAIL("corrupt Huffman table");
                memset(P.vals[t], 0, 256);
                memcpy(P.vals[t], s + k + 17, cnt);
                P.ht_ok[t] = true;
                k += 17 + cnt;
            }
        } else if (m == 0xDB) {   // DQT
            int k = 0;
            while (k < L) {
                const int pq = s[k] >> 4, tq = s[k] & 15;
                if (pq > 1 || tq > 3 || k + 1 + 64 * (pq + 1) > L) JFAIL("corrupt quantisation table");
                for (int i = 0; i < 64; i++)   // zig-zag -> natural
                    P.qt[tq][kNatural[i]] = pq ? (uint16_t)u16be(s + k + 1 + 2 * i) : s[k + 1 + i];
                P.qt_ok[tq] = true;
                k += 1 + 64 * (pq + 1);
            }
        } else if (m == 0xDD) {   // DRI
            if (L < 2) JFAIL("corrupt restart interval");
            P.restart = u16be(s);
        } else if (m == 0xE0) {   // jdmarker.c examine_app0: "JFIF\0" in >= 14 bytes
            if (L >= 14 && s[0] == 0x4A && s[1] == 0x46 && s[2] == 0x49 && s[3] == 0x46 && s[4] == 0) P.jfif = true;
        } else if (m == 0xEE) {   // examine_app14: "Adobe" in >= 12 bytes
            if (L >= 12 && s[0] == 0x41 && s[1] == 0x64 && s[2] == 0x6F && s[3] == 0x62 && s[4] == 0x65) {
                P.adobe = true;
                P.adobe_transform = s[11];
            }
        } else if (m == 0xDA) {   // SOS
            if (P.sof < 0) JFAIL("corrupt file (scan before the frame header)");
            if (L < 1) JFAIL("corrupt scan header");
            const int ns = s[0];
            if (ns != P.ncomp) JFAIL("multi-scan file (a scan of %d of %d components)", ns, P.ncomp);
            if (L < 4 + 2 * ns) JFAIL("corrupt scan header");
            for (int c = 0; c < ns; c++) {
                if (s[1 + 2 * c] != P.cid[c]) JFAIL("scan components out of frame order");
                P.ctd[c] = s[2 + 2 * c] >> 4;
                P.cta[c] = s[2 + 2 * c] & 15;
                if (P.ctd[c] > 3 || P.cta[c] > 3) JFAIL("corrupt scan header (table ids)");
            }
            const int ss = s[1 + 2 * ns], se = s[2 + 2 * ns], ahl = s[3 + 2 * ns];
            if (ss != 0 || se != 63 || ahl != 0) JFAIL("not a sequential scan (Ss %d, Se %d, Ah/Al 0x%02X)", ss, se, ahl);
            sos = true;
            break;
        }
        // other APPn / COM / DNL-free markers: skipped by length
    }
    (void)sos;
    // colour space: jdapimin.c default_decompress_parms
    if (P.ncomp == 3) {
        bool ycc = true;
        if (P.jfif) ycc = true;
        else if (P.adobe) ycc = P.adobe_transform != 0;
        else if (P.cid[0] == 82 && P.cid[1] == 71 && P.cid[2] == 66) ycc = false;
        if (!ycc) JFAIL(P.adobe && !P.jfif ? "RGB colour space (Adobe transform 0)" : "RGB colour space (component ids R, G, B)");
        const bool chroma11 = P.ch[1] == 1 && P.cv[1] == 1 && P.ch[2] == 1 && P.cv[2] == 1;
        const bool luma = (P.ch[0] == 1 && P.cv[0] == 1) || (P.ch[0] == 2 && P.cv[0] == 1) || (P.ch[0] == 2 && P.cv[0] == 2);
        if (!chroma11 || !luma)
            JFAIL("sampling factors %dx%d,%dx%d,%dx%d", P.ch[0], P.cv[0], P.ch[1], P.cv[1], P.ch[2], P.cv[2]);
    }
    for (int c = 0; c < P.ncomp; c++) {
        if (!P.qt_ok[P.ctq[c]]) JFAIL("corrupt file (missing quantisation table %d)", P.ctq[c]);
        if (!P.ht_ok[P.ctd[c]] || !P.ht_ok[4 + P.cta[c]]) JFAIL("corrupt file (missing Huffman table)");
    }
    // entropy data: 0xFF 0x00 -> 0xFF, fill 0xFF bytes skipped, RSTn closes a segment, any other marker ends the scan
    P.scan_pos = pos;
    int64_t out = 0;
    int nrst = 0;
    P.seg_begin.assign(1, 0);
    int end_marker = -1;
    while (pos < n) {
        const uint8_t b = d[pos++];
        if (b != 0xFF) {
            if (ent) ent[out] = b;
            out++;
            continue;
        }
        while (pos < n && d[pos] == 0xFF) pos++;
        if (pos >= n) break;
        const int m = d[pos++];
        if (m == 0) {
            if (ent) ent[out] = 0xFF;
            out++;
        } else if (m >= 0xD0 && m <= 0xD7) {
            if (m != 0xD0 + (nrst & 7)) JFAIL("restart markers out of sequence");
            nrst++;
            P.seg_len.push_back(out - P.seg_begin.back());
            P.seg_begin.push_back(out);
        } else {
            end_marker = m;
            break;
        }
    }
    if (end_marker < 0) JFAIL("truncated file (no marker after the scan)");
    if (end_marker != 0xD9) JFAIL("more than one scan or data after the scan (marker 0x%02X)", end_marker);
    P.seg_len.push_back(out - P.seg_begin.back());
    P.ent_bytes = out;
    for (int64_t L : P.seg_len)
        if (L >= ((int64_t)1 << 28) - 64) JFAIL("restart segment of %lld bytes", (long long)L);
    return IVIT_OK;
}

struct Geometry {
    int hmax, vmax, mcux, mcuy, bpm, sampling;
};

Geometry geometry_of(const Parsed& P)
{
    Geometry G;
    if (P.ncomp == 1) {   // one component: a non-interleaved scan, one block per MCU
        G.hmax = G.vmax = 1;
        G.bpm = 1;
        G.sampling = 0;
    } else {
        G.hmax = P.ch[0];
        G.vmax = P.cv[0];
        G.bpm = P.ch[0] * P.cv[0] + 2;
        G.sampling = P.ch[0] == 1 ? 1 : P.cv[0] == 1 ? 2 : 3;
    }
    G.mcux = (P.w + 8 * G.hmax - 1) / (8 * G.hmax);
    G.mcuy = (P.h + 8 * G.vmax - 1) / (8 * G.vmax);
    return G;
}

int section_bytes(const Parsed& P, int64_t* bytes, int* ntab)
{
    int used = 0;
    for (int t = 0; t < 8; t++) used += P.ht_ok[t];
    *ntab = used;
    const int64_t nseg = (int64_t)P.seg_len.size();
    *bytes = align16(sizeof(Sec)) + align16((int64_t)used * sizeof(HuffTab)) + align16(nseg * (int64_t)sizeof(Seg)) + align16(P.ent_bytes + 8);
    return IVIT_OK;
}

// The plan section of a parsed file (ent already written at its place by parse())
int build_section(const Parsed& P, uint8_t* out, int64_t bytes)
{
    const Geometry G = geometry_of(P);
    const int64_t nmcu = (int64_t)G.mcux * G.mcuy;
    const int64_t nseg = P.restart ? (nmcu + P.restart - 1) / P.restart : 1;
    if ((int64_t)P.seg_len.size() != nseg)
        JFAIL("%lld restart segments where the restart interval gives %lld", (long long)P.seg_len.size(), (long long)nseg);
    Sec* S = reinterpret_cast<Sec*>(out);
    memset(S, 0, sizeof(Sec));
    S->bytes = bytes;
    S->h = P.h;
    S->w = P.w;
    S->ncomp = P.ncomp;
    S->hmax = G.hmax;
    S->vmax = G.vmax;
    S->mcux = G.mcux;
    S->mcuy = G.mcuy;
    S->bpm = G.bpm;
    S->nseg = (int)nseg;
    S->sampling = G.sampling;
    int slot[8], ntab = 0;
    for (int t = 0; t < 8; t++) slot[t] = P.ht_ok[t] ? ntab++ : -1;
    S->ntab = ntab;
    S->tab_off = align16(sizeof(Sec));
    S->seg_off = S->tab_off + align16((int64_t)ntab * sizeof(HuffTab));
    S->ent_off = S->seg_off + align16(nseg * (int64_t)sizeof(Seg));
    int64_t plane = 0;
    int blk = 0;
    for (int c = 0; c < P.ncomp; c++) {
        const int h = P.ncomp == 1 ? 1 : P.ch[c], v = P.ncomp == 1 ? 1 : P.cv[c];
        S->ch[c] = h;
        S->cv[c] = v;
        S->cdc[c] = slot[P.ctd[c]];
        S->cac[c] = slot[4 + P.cta[c]];
        S->dw[c] = (int)(((int64_t)P.w * h + G.hmax - 1) / G.hmax);   // jdinput.c downsampled_width / height
        S->dh[c] = (int)(((int64_t)P.h * v + G.vmax - 1) / G.vmax);
        S->pw[c] = G.mcux * h * 8;
        S->ph[c] = G.mcuy * v * 8;
        S->plane_off[c] = plane;
        plane += align256((int64_t)S->pw[c] * S->ph[c]);
        S->blk_first[c] = blk;
        for (int k = 0; k < h * v; k++) S->blk_comp[blk++] = c;
        memcpy(S->qt[c], P.qt[P.ctq[c]], sizeof(S->qt[c]));
    }
    S->plane_bytes = plane;
    S->nblocks = nmcu * G.bpm;
    HuffTab* T = reinterpret_cast<HuffTab*>(out + S->tab_off);
    for (int t = 0; t < 8; t++)
        if (slot[t] >= 0 && !derive(P.bits[t], P.vals[t], t < 4, T + slot[t])) JFAIL("corrupt Huffman table (class %d, id %d)", t / 4, t & 3);
    Seg* sg = reinterpret_cast<Seg*>(out + S->seg_off);
    int nsub = 0;
    for (int64_t i = 0; i < nseg; i++) {
        sg[i].off = P.seg_begin[i];
        sg[i].nbytes = (int32_t)P.seg_len[i];
        sg[i].sub_first = nsub;
        const int64_t bits = (int64_t)P.seg_len[i] * 8;
        sg[i].nsub = bits ? (int)((bits + kSubBits - 1) / kSubBits) : 1;
        sg[i].first_mcu = (int)(i * (P.restart ? P.restart : nmcu));
        const int64_t left = nmcu - sg[i].first_mcu;
        sg[i].nmcu = (int)(P.restart && P.restart < left ? P.restart : left);
        sg[i].pad = 0;
        nsub += sg[i].nsub;
    }
    S->nsub = nsub;
    return IVIT_OK;
}

int plan_into(const uint8_t* d, int64_t n, std::vector<uint8_t>& buf)
{
    Parsed P;
    int rc = parse(d, n, P, nullptr);
    if (rc) return rc;
    int64_t bytes;
    int ntab;
    section_bytes(P, &bytes, &ntab);
    buf.assign(bytes, 0);
    Parsed Q;
    // the entropy bytes go straight to their place in the section
    const int64_t ent_off = align16(sizeof(Sec)) + align16((int64_t)ntab * sizeof(HuffTab)) + align16((int64_t)P.seg_len.size() * sizeof(Seg));
    rc = parse(d, n, Q, buf.data() + ent_off);
    if (rc) return rc;
    return build_section(Q, buf.data(), bytes);
}

// ------------------------------------------------------------------------------------------------------------------------------
// Device

__device__ inline int find_image(const Idx* idx, int batch, int64_t v, bool by_coef)
{
    int lo = 0, hi = batch - 1;   // last image whose first subsequence / block is <= v
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        const int64_t f = by_coef ? idx[mid].coef : (int64_t)idx[mid].sub_first;
        if (f <= v) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ inline int find_seg(const Seg* sg, int nseg, int local)
{
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (sg[mid].sub_first <= local) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// decodes the codewords that start in [start, end) from state s; returns the exit state and the blocks completed
__host__ __device__ inline uint64_t run_sub(const Sec* S, const HuffTab* T, const uint8_t* d, int32_t nbytes, Dec s, int32_t end, int* count)
{
    int k = 0, pos, val;
    bool done;
    while (s.p < end) {
        huff_step(S, T, d, nbytes, s, pos, val, done);
        k += done;
    }
    *count = k;
    return pack_state(s);
}

struct SubRef {
    const Sec* S;
    const Seg* g;
    int b, local, start, end;
    bool first;
};

__device__ inline bool locate(const uint8_t* plan, const Idx* idx, int batch, int64_t gsub, SubRef& r)
{
    r.b = find_image(idx, batch, gsub, false);
    const Idx& I = idx[r.b];
    if (I.sec < 0 || gsub < I.sub_first || gsub >= I.sub_first + I.nsub) return false;
    r.S = reinterpret_cast<const Sec*>(plan + I.sec);
    r.local = (int)(gsub - I.sub_first);
    const Seg* sg = segs_of(r.S);
    r.g = sg + find_seg(sg, r.S->nseg, r.local);
    const int k = r.local - r.g->sub_first;
    r.first = k == 0;
    r.start = k * kSubBits;
    const int bits = r.g->nbytes * 8;
    r.end = r.start + kSubBits < bits ? r.start + kSubBits : bits;
    return true;
}

__global__ void __launch_bounds__(kSyncLanes) sync_kernel(const uint8_t* __restrict__ plan, const Idx* __restrict__ idx, int batch, int64_t nsub,
                                                          uint64_t* st_in, uint64_t* st_out, int32_t* cnt)
{
    __shared__ uint64_t sh_exit[kSyncLanes];
    __shared__ int64_t sh_seg[kSyncLanes];
    const int tid = threadIdx.x;
    const int64_t g = (int64_t)blockIdx.x * kSyncLanes + tid;
    SubRef r;
    const bool valid = g < nsub && locate(plan, idx, batch, g, r);
    uint64_t entry = 0, exit = 0;
    int count = 0;
    if (valid) {
        Dec s = {r.start, 0, 0};   // a segment's first subsequence starts in a known state; the others guess
        entry = pack_state(s);
        exit = run_sub(r.S, tabs_of(r.S), ent_of(r.S, *r.g), r.g->nbytes, s, r.end, &count);
        sh_seg[tid] = g - (r.local - r.g->sub_first);   // global index of the segment's first subsequence
    } else {
        sh_seg[tid] = -1 - tid;
    }
    sh_exit[tid] = exit;
    for (int round = 0; round < kSyncLanes; round++) {
        __syncthreads();
        bool changed = false;
        if (valid && !r.first && tid > 0 && sh_seg[tid - 1] == sh_seg[tid] && sh_exit[tid - 1] != entry) {
            entry = sh_exit[tid - 1];
            exit = run_sub(r.S, tabs_of(r.S), ent_of(r.S, *r.g), r.g->nbytes, unpack_state(entry), r.end, &count);
            changed = true;
        }
        __syncthreads();
        if (changed) sh_exit[tid] = exit;
        if (!__syncthreads_or(changed)) break;
    }
    if (valid) {
        st_in[g] = entry;
        st_out[g] = exit;
        cnt[g] = count;
    }
}

// workgroup boundaries inside a segment: serial continuation from the true state until it meets the recorded one
__global__ void __launch_bounds__(64) fix_kernel(const uint8_t* __restrict__ plan, const Idx* __restrict__ idx, int batch, uint64_t* st_in,
                                                 uint64_t* st_out, int32_t* cnt)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= batch) return;
    const Idx I = idx[b];
    if (I.sec < 0 || I.nsub == 0) return;
    const Sec* S = reinterpret_cast<const Sec*>(plan + I.sec);
    const Seg* sg = segs_of(S);
    const HuffTab* T = tabs_of(S);
    int64_t gb = ((I.sub_first + kSyncLanes) / kSyncLanes) * kSyncLanes;   // first workgroup boundary after the image's first
    for (; gb < (int64_t)I.sub_first + I.nsub; gb += kSyncLanes) {
        int local = (int)(gb - I.sub_first);
        const Seg& seg = sg[find_seg(sg, S->nseg, local)];
        if (local == seg.sub_first) continue;
        const int bits = seg.nbytes * 8;
        for (; local < seg.sub_first + seg.nsub; local++) {
            const int64_t g = I.sub_first + local;
            const uint64_t e = st_out[g - 1];
            if (e == st_in[g]) break;
            st_in[g] = e;
            const int start = (local - seg.sub_first) * kSubBits;
            const int end = start + kSubBits < bits ? start + kSubBits : bits;
            int count;
            const uint64_t x = run_sub(S, T, ent_of(S, seg), seg.nbytes, unpack_state(e), end, &count);
            cnt[g] = count;
            const uint64_t old = st_out[g];
            st_out[g] = x;
            if (x == old) break;
        }
        if (gb < (int64_t)I.sub_first + local) gb = ((I.sub_first + local) / kSyncLanes) * kSyncLanes;   // continued past boundaries
    }
}

// Inclusive segmented scan over the 256 lanes of a workgroup (Hillis-Steele: a lane whose window holds a segment start stops adding
// from its left); f: the lane's value starts a segment.  Returns whether a start lies at or before the lane in this chunk.
template <int N>
__device__ inline bool segmented_scan(int (*sh)[256], int* shf, int* v, bool f)
{
    const int tid = threadIdx.x;
    for (int c = 0; c < N; c++) sh[c][tid] = v[c];
    shf[tid] = f;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        int u[N], uf = 0;
        for (int c = 0; c < N; c++) u[c] = tid >= off ? sh[c][tid - off] : 0;
        if (tid >= off) uf = shf[tid - off];
        __syncthreads();
        if (!shf[tid])
            for (int c = 0; c < N; c++) sh[c][tid] += u[c];
        shf[tid] |= uf;
        __syncthreads();
    }
    for (int c = 0; c < N; c++) v[c] = sh[c][tid];
    return shf[tid] != 0;
}

// exclusive prefix sum of the completed blocks per restart segment (one segmented scan over the image's subsequences) -> block
// slot of every subsequence's first block; a segment that completes fewer blocks than its MCUs hold is corrupt
__global__ void __launch_bounds__(256) scan_kernel(const uint8_t* __restrict__ plan, const Idx* __restrict__ idx, const int32_t* __restrict__ cnt,
                                                   int32_t* base, int32_t* err)
{
    __shared__ int sh[1][256];
    __shared__ int shf[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const Idx I = idx[b];
    if (I.sec < 0) return;
    const Sec* S = reinterpret_cast<const Sec*>(plan + I.sec);
    const Seg* sg = segs_of(S);
    int carry = 0;
    for (int k0 = 0; k0 < S->nsub; k0 += 256) {
        const int k = k0 + tid;
        const bool in = k < S->nsub;
        const Seg* seg = in ? sg + find_seg(sg, S->nseg, k) : nullptr;
        int v[1] = {in ? cnt[I.sub_first + k] : 0};
        const int mine = v[0];
        const bool started = segmented_scan<1>(sh, shf, v, in && k == seg->sub_first);
        const int incl = v[0] + (started ? 0 : carry);
        if (in) {
            base[I.sub_first + k] = seg->first_mcu * S->bpm + incl - mine;
            if (k == seg->sub_first + seg->nsub - 1 && incl < seg->nmcu * S->bpm) err[b] |= 1;
        }
        const int last = sh[0][255];
        carry = shf[255] ? last : carry + last;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) write_kernel(const uint8_t* __restrict__ plan, const Idx* __restrict__ idx, int batch, int64_t nsub,
                                                    const uint64_t* __restrict__ st_in, const int32_t* __restrict__ base, int16_t* coef,
                                                    int32_t* err)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    SubRef r;
    if (g >= nsub || !locate(plan, idx, batch, g, r)) return;
    const Sec* S = r.S;
    const HuffTab* T = tabs_of(S);
    const uint8_t* d = ent_of(S, *r.g);
    const int64_t limit = (int64_t)(r.g->first_mcu + r.g->nmcu) * S->bpm;
    int64_t slot = base[g];
    int16_t* C0 = coef + idx[r.b].coef * 64;
    Dec s = unpack_state(st_in[g]);
    bool bad = false;
    while (s.p < r.end && slot < limit) {
        int pos, val;
        bool done;
        const bool ok = huff_step(S, T, d, r.g->nbytes, s, pos, val, done);
        bad |= !ok;
        if (pos >= 0) C0[slot * 64 + pos] = (int16_t)val;
        slot += done;
    }
    if (bad) atomicOr(err + r.b, 2);
}

// per image: DC differences -> DC values, a prefix sum per (component, restart segment) in MCU order (dummy blocks included): one
// segmented scan over the image's MCUs, the predictor reset at every restart
__global__ void __launch_bounds__(256) dc_kernel(const uint8_t* __restrict__ plan, const Idx* __restrict__ idx, int16_t* coef)
{
    __shared__ int sh[3][256];
    __shared__ int shf[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const Idx I = idx[b];
    if (I.sec < 0) return;
    const Sec* S = reinterpret_cast<const Sec*>(plan + I.sec);
    int16_t* C0 = coef + I.coef * 64;
    const int bpm = S->bpm;
    const int nmcu = S->mcux * S->mcuy;
    const int rst = S->nseg > 1 ? segs_of(S)[0].nmcu : nmcu;   // MCUs per restart interval
    int blk_comp[8];
    for (int k = 0; k < bpm; k++) blk_comp[k] = S->blk_comp[k];
    int carry[3] = {0, 0, 0};
    for (int m0 = 0; m0 < nmcu; m0 += 256) {
        const int m = m0 + tid;
        const bool in = m < nmcu;
        int16_t* mc = C0 + (int64_t)m * bpm * 64;
        int t[3] = {0, 0, 0}, v[3];
        if (in)
            for (int k = 0; k < bpm; k++) t[blk_comp[k]] += mc[k * 64];
        for (int c = 0; c < 3; c++) v[c] = t[c];
        const bool started = segmented_scan<3>(sh, shf, v, in && m % rst == 0);
        if (in) {
            int acc[3];
            for (int c = 0; c < 3; c++) acc[c] = (started ? 0 : carry[c]) + v[c] - t[c];
            for (int k = 0; k < bpm; k++) {
                const int c = blk_comp[k];
                acc[c] += mc[k * 64];
                mc[k * 64] = (int16_t)acc[c];
            }
        }
        for (int c = 0; c < 3; c++) carry[c] = shf[255] ? sh[c][255] : carry[c] + sh[c][255];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) idct_kernel(const uint8_t* __restrict__ plan, const Idx* __restrict__ idx, int batch, int64_t nblocks,
                                                   const int16_t* __restrict__ coef, uint8_t* planes)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nblocks) return;
    const int b = find_image(idx, batch, k, true);
    const Idx& I = idx[b];
    if (I.sec < 0) return;
    const Sec* S = reinterpret_cast<const Sec*>(plan + I.sec);
    const int64_t slot = k - I.coef;
    if (slot < 0 || slot >= S->nblocks) return;
    int c, px, py;
    block_origin(S, slot, &c, &px, &py);
    alignas(16) int16_t blk[64];
    const int4* src = reinterpret_cast<const int4*>(coef + k * 64);
    for (int i = 0; i < 8; i++) reinterpret_cast<int4*>(blk)[i] = src[i];
    alignas(8) uint8_t px8[64];
    idct_islow(blk, S->qt[c], px8, 8);
    uint8_t* dst = planes + I.plane + S->plane_off[c] + (int64_t)py * S->pw[c] + px;
    for (int r = 0; r < 8; r++) *reinterpret_cast<uint2*>(dst + (int64_t)r * S->pw[c]) = reinterpret_cast<const uint2*>(px8)[r];
}

// grid (x, batch): pixels of image b strided over gridDim.x * 256 lanes
__global__ void __launch_bounds__(256) color_kernel(const uint8_t* __restrict__ plan, const Idx* __restrict__ idx, const uint8_t* __restrict__ planes,
                                                    uint8_t* out)
{
    const int b = blockIdx.y;
    const Idx I = idx[b];
    if (I.sec < 0) return;
    const Sec* S = reinterpret_cast<const Sec*>(plan + I.sec);
    const int w = S->w;
    const int64_t npix = (int64_t)S->h * w;
    const uint8_t* P = planes + I.plane;
    uint8_t* o = out + I.out;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
        const int y = (int)(i / w), x = (int)(i % w);
        uint8_t rgb[3];
        pixel_rgb(S, P, y, x, rgb);
        o[i * 3] = rgb[0];
        o[i * 3 + 1] = rgb[1];
        o[i * 3 + 2] = rgb[2];
    }
}

struct WsLayout {
    int64_t st_in, st_out, cnt, base, coef, planes, bytes;
};

WsLayout ws_layout(int64_t nsub, int64_t nblocks, int64_t plane_bytes)
{
    WsLayout L;
    L.st_in = 0;
    L.st_out = align256(L.st_in + nsub * 8);
    L.cnt = align256(L.st_out + nsub * 8);
    L.base = align256(L.cnt + nsub * 4);
    L.coef = align256(L.base + nsub * 4);
    L.planes = align256(L.coef + nblocks * 128);
    L.bytes = align256(L.planes + plane_bytes);
    return L;
}

bool section_ok(const uint8_t* plan, int64_t plan_bytes, int64_t off)
{
    if (off < 0 || (off & 15) || off + (int64_t)sizeof(Sec) > plan_bytes) return false;
    const Sec* S = reinterpret_cast<const Sec*>(plan + off);
    return S->bytes >= (int64_t)sizeof(Sec) && off + S->bytes <= plan_bytes && S->ent_off < S->bytes;
}

}  // namespace

IVIT_EXPORT int ivit_jpeg_probe(const uint8_t* data, int64_t nbytes, int32_t* info4)
{
    IVIT_REQUIRE(data != nullptr && info4 != nullptr, "ivit_jpeg_probe: NULL operand");
    Parsed P;
    const int rc = parse(data, nbytes, P, nullptr);
    info4[0] = P.h;
    info4[1] = P.w;
    info4[2] = P.ncomp;
    info4[3] = -1;
    if (rc) return rc;
    const Geometry G = geometry_of(P);
    const int64_t nmcu = (int64_t)G.mcux * G.mcuy;
    const int64_t nseg = P.restart ? (nmcu + P.restart - 1) / P.restart : 1;
    if ((int64_t)P.seg_len.size() != nseg)
        JFAIL("%lld restart segments where the restart interval gives %lld", (long long)P.seg_len.size(), (long long)nseg);
    HuffTab T;
    for (int t = 0; t < 8; t++)
        if (P.ht_ok[t] && !derive(P.bits[t], P.vals[t], t < 4, &T)) JFAIL("corrupt Huffman table (class %d, id %d)", t / 4, t & 3);
    info4[3] = G.sampling;
    return IVIT_OK;
}

IVIT_EXPORT int ivit_jpeg_plan_image(const uint8_t* data, int64_t nbytes, uint8_t* section, int64_t capacity, int64_t* section_bytes_out)
{
    IVIT_REQUIRE(data != nullptr && section_bytes_out != nullptr, "ivit_jpeg_plan_image: NULL operand");
    IVIT_REQUIRE(((uintptr_t)section & 15) == 0, "ivit_jpeg_plan_image: misaligned section (16 bytes)");
    Parsed P;
    int rc = parse(data, nbytes, P, nullptr);
    if (rc) return rc;
    int64_t bytes;
    int ntab;
    section_bytes(P, &bytes, &ntab);
    *section_bytes_out = bytes;
    if (section == nullptr) return IVIT_OK;
    IVIT_REQUIRE(capacity >= bytes, "ivit_jpeg_plan_image: section of %lld bytes < %lld", (long long)capacity, (long long)bytes);
    memset(section, 0, bytes);
    Parsed Q;
    const int64_t ent_off = align16(sizeof(Sec)) + align16((int64_t)ntab * sizeof(HuffTab)) + align16((int64_t)P.seg_len.size() * sizeof(Seg));
    rc = parse(data, nbytes, Q, section + ent_off);
    if (rc) return rc;
    return build_section(Q, section, bytes);
}

IVIT_EXPORT int ivit_jpeg_workspace(const uint8_t* plan, int64_t plan_bytes, const int64_t* sec_offsets, const int64_t* out_offsets, int batch,
                                    void* index, int64_t* sizes4)
{
    IVIT_REQUIRE(plan && sec_offsets && out_offsets && index && sizes4, "ivit_jpeg_workspace: NULL operand");
    IVIT_REQUIRE(batch >= 0 && batch <= 65535, "ivit_jpeg_workspace: batch %d outside 0..65535", batch);
    Idx* I = static_cast<Idx*>(index);
    int64_t nsub = 0, nblocks = 0, planes = 0, maxpix = 0;
    for (int b = 0; b < batch; b++) {
        I[b].out = out_offsets[b];
        I[b].coef = nblocks;
        I[b].plane = planes;
        I[b].sub_first = (int32_t)nsub;
        I[b].nsub = 0;
        I[b].sec = -1;
        if (sec_offsets[b] < 0) continue;
        if (!section_ok(plan, plan_bytes, sec_offsets[b])) {
            ivit_set_error("ivit_jpeg_workspace: image %d: offset %lld is not a plan section", b, (long long)sec_offsets[b]);
            return IVIT_ERR_INVALID;
        }
        const Sec* S = reinterpret_cast<const Sec*>(plan + sec_offsets[b]);
        I[b].sec = sec_offsets[b];
        I[b].nsub = S->nsub;
        nsub += S->nsub;
        nblocks += S->nblocks;
        planes += S->plane_bytes;
        const int64_t px = (int64_t)S->h * S->w;
        maxpix = px > maxpix ? px : maxpix;
        if (nsub > INT32_MAX) {
            ivit_set_error("ivit_jpeg_workspace: more than 2^31 subsequences");
            return IVIT_ERR_UNSUPPORTED;
        }
    }
    sizes4[0] = ws_layout(nsub, nblocks, planes).bytes;
    sizes4[1] = nsub;
    sizes4[2] = nblocks;
    sizes4[3] = maxpix;
    return IVIT_OK;
}

IVIT_EXPORT int ivit_jpeg_decode_u8(const uint8_t* plan, const void* index, int batch, int64_t nsub, int64_t nblocks, int64_t max_pixels,
                                    void* workspace, int64_t workspace_bytes, uint8_t* out, int32_t* errors, ivit_stream_t stream)
{
    IVIT_REQUIRE(plan && index && workspace && out && errors, "ivit_jpeg_decode_u8: NULL operand");
    IVIT_REQUIRE(((uintptr_t)plan & 15) == 0 && ((uintptr_t)index & 7) == 0 && ((uintptr_t)workspace & 255) == 0 && ((uintptr_t)errors & 3) == 0,
                 "ivit_jpeg_decode_u8: misaligned operand (plan 16, index 8, workspace 256, errors 4 bytes)");
    IVIT_REQUIRE(batch >= 0 && batch <= 65535, "ivit_jpeg_decode_u8: batch %d outside 0..65535", batch);
    IVIT_REQUIRE(nsub >= 0 && nsub <= INT32_MAX && nblocks >= 0 && max_pixels >= 0, "ivit_jpeg_decode_u8: sizes are not those of ivit_jpeg_workspace");
    const WsLayout L = ws_layout(nsub, nblocks, 0);
    IVIT_REQUIRE(workspace_bytes >= L.bytes, "ivit_jpeg_decode_u8: workspace of %lld bytes < %lld", (long long)workspace_bytes, (long long)L.bytes);
    if (batch == 0) return IVIT_OK;
    hipStream_t st = ivit_stream(stream);
    char* ws = static_cast<char*>(workspace);
    uint64_t* st_in = reinterpret_cast<uint64_t*>(ws + L.st_in);
    uint64_t* st_out = reinterpret_cast<uint64_t*>(ws + L.st_out);
    int32_t* cnt = reinterpret_cast<int32_t*>(ws + L.cnt);
    int32_t* base = reinterpret_cast<int32_t*>(ws + L.base);
    int16_t* coef = reinterpret_cast<int16_t*>(ws + L.coef);
    uint8_t* planes = reinterpret_cast<uint8_t*>(ws + L.planes);
    const Idx* I = static_cast<const Idx*>(index);
    if (hipMemsetAsync(errors, 0, (size_t)batch * 4, st) != hipSuccess || hipMemsetAsync(coef, 0, (size_t)nblocks * 128, st) != hipSuccess) {
        ivit_set_error("ivit_jpeg_decode_u8: hipMemsetAsync failed");
        return IVIT_ERR_LAUNCH;
    }
    if (nsub > 0) {
        const int gs = (int)((nsub + kSyncLanes - 1) / kSyncLanes);
        hipLaunchKernelGGL(sync_kernel, dim3(gs), dim3(kSyncLanes), 0, st, plan, I, batch, nsub, st_in, st_out, cnt);
        hipLaunchKernelGGL(fix_kernel, dim3((batch + 63) / 64), dim3(64), 0, st, plan, I, batch, st_in, st_out, cnt);
        hipLaunchKernelGGL(scan_kernel, dim3(batch), dim3(256), 0, st, plan, I, cnt, base, errors);
        hipLaunchKernelGGL(write_kernel, dim3((unsigned)((nsub + 255) / 256)), dim3(256), 0, st, plan, I, batch, nsub, st_in, base, coef, errors);
    }
    if (nblocks > 0) {
        hipLaunchKernelGGL(dc_kernel, dim3(batch), dim3(256), 0, st, plan, I, coef);
        hipLaunchKernelGGL(idct_kernel, dim3((unsigned)((nblocks + 255) / 256)), dim3(256), 0, st, plan, I, batch, nblocks, coef, planes);
        int64_t gx = (max_pixels + 255) / 256;
        gx = gx < 1 ? 1 : gx > 256 ? 256 : gx;
        hipLaunchKernelGGL(color_kernel, dim3((unsigned)gx, batch), dim3(256), 0, st, plan, I, planes, out);
    }
    IVIT_CHECK_LAUNCH("ivit_jpeg_decode_u8");
}

IVIT_EXPORT int ivit_jpeg_decode_host(const uint8_t* data, int64_t nbytes, uint8_t* out, int64_t out_bytes)
{
    IVIT_REQUIRE(data != nullptr && out != nullptr, "ivit_jpeg_decode_host: NULL operand");
    std::vector<uint8_t> buf;
    const int rc = plan_into(data, nbytes, buf);
    if (rc) return rc;
    const Sec* S = reinterpret_cast<const Sec*>(buf.data());
    IVIT_REQUIRE(out_bytes >= (int64_t)S->h * S->w * 3, "ivit_jpeg_decode_host: output of %lld bytes < %d x %d x 3", (long long)out_bytes, S->h, S->w);
    const HuffTab* T = tabs_of(S);
    const Seg* sg = segs_of(S);
    std::vector<int16_t> coef((size_t)S->nblocks * 64, 0);
    for (int si = 0; si < S->nseg; si++) {   // the device's subsequences decoded one after the other from the segment's start
        const Seg& g = sg[si];
        const uint8_t* d = ent_of(S, g);
        const int end = g.nbytes * 8;
        const int64_t limit = (int64_t)(g.first_mcu + g.nmcu) * S->bpm;
        int64_t slot = (int64_t)g.first_mcu * S->bpm;
        Dec s = {0, 0, 0};
        while (s.p < end && slot < limit) {
            int pos, val;
            bool done;
            if (!huff_step(S, T, d, g.nbytes, s, pos, val, done)) {
                ivit_set_error("ivit_jpeg_decode_host: corrupt data (a Huffman code no table holds, segment %d)", si);
                return IVIT_ERR_INVALID;
            }
            if (pos >= 0) coef[slot * 64 + pos] = (int16_t)val;
            slot += done;
        }
        if (slot < limit) {
            ivit_set_error("ivit_jpeg_decode_host: corrupt data (segment %d ends after %lld of %lld blocks)", si,
                           (long long)(slot - (int64_t)g.first_mcu * S->bpm), (long long)((int64_t)g.nmcu * S->bpm));
            return IVIT_ERR_INVALID;
        }
        int pred[3] = {0, 0, 0};
        for (int64_t k = (int64_t)g.first_mcu * S->bpm; k < limit; k++) {
            const int c = S->blk_comp[k % S->bpm];
            pred[c] += coef[k * 64];
            coef[k * 64] = (int16_t)pred[c];
        }
    }
    std::vector<uint8_t> planes(S->plane_bytes);
    for (int64_t k = 0; k < S->nblocks; k++) {
        int c, px, py;
        block_origin(S, k, &c, &px, &py);
        idct_islow(coef.data() + k * 64, S->qt[c], planes.data() + S->plane_off[c] + (int64_t)py * S->pw[c] + px, S->pw[c]);
    }
    for (int y = 0; y < S->h; y++)
        for (int x = 0; x < S->w; x++) pixel_rgb(S, planes.data(), y, x, out + ((int64_t)y * S->w + x) * 3);
    return IVIT_OK;
}
