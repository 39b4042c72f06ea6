// win_attn_host.h -- the host side the eight Swin window-attention entries share: the six fused ones of swin.hip and the two
// probability entries of swin_probs.hip.  Descriptor, check, softmax form.  Host code only: nothing here is passed to a kernel, and each
// file fills its own kernel argument struct (WinAttnArgs, WinProbsArgs) from the form.  Included inside the anonymous namespace of both
// files, as attn_parts.h is; needs WHD (the head dimension, 32) from the including file.
//
// The probabilities must be byte for byte the P of the fused kernel: both files take x0, ksat, the effective mask value and the tables
// the kernel receives from win_attn_form below, so the two cannot choose differently.

enum WinFamily {
    WIN_SHORT,            // window_attention_kernel NKT 4, Shiftmax, 2 .. 64 tokens (_i8, _compat, _band, _unwindow)
    WIN_LONG,             // window_attention_kernel NKT 9, Shiftmax, 65 .. 144 tokens (_long)
    WIN_IBERT,            // window_attention_kernel SM 3, 2 .. 144 tokens (_ibert)
    WIN_SHIFTMAX_PROBS,   // window_attention_probs_kernel SM 0 / 1 / 2, 2 .. 144 tokens
    WIN_IBERT_PROBS       // window_attention_probs_kernel SM 3, 2 .. 144 tokens
};

// what an entry's contract requires beyond its family's
enum { WIN_NEEDS_BAND = 1,         // _band: a band table
       WIN_NEEDS_GEOMETRY = 2 };   // _unwindow (_long: the family): H, W, ws, shift; else they are checked where ws != 0

struct WinAttnDesc {      // never passed to a kernel
    const char* name;             // the called entry, for the messages
    WinFamily family;
    const int8_t* qkv;
    void* out;                    // int8 rows; probs: the uint8 probabilities
    int64_t ldo;                  // probs: ldp
    const int16_t* bias;
    const uint8_t* region;
    int mask_value;               // Shiftmax families
    int windows, windows_per_image, heads, tokens, head_dim;
    uint32_t m_s;
    int32_t e_s;
    uint32_t m_b;
    int32_t e_b;
    float s_attn;                 // Shiftmax families
    uint32_t m_o;                 // fused families
    int32_t e_o;
    const float *phi, *phim;      // Shiftmax: the literal form's tables, or NULL
    const uint32_t* band;         // Shiftmax: the band table, or NULL
    int band_w, band_rows;        // I-BERT: band_w is the width of the table's band form, 0 = the full table
    const float* ib_tab;          // I-BERT: the (row max, q) table, required
    float masked_exp;
    int H, W, ws, shift;          // window geometry, fused families
    int image_order;              // the output rows go to their image positions
    ivit_stream_t stream;
    int needs;                    // WIN_NEEDS_*
    double Ms, Mb, Mo;            // filled by win_attn_check
    int x0;
};

#define WIN_UNSUPPORTED(cond, ...)           \
    do {                                     \
        if (!(cond)) {                       \
            ivit_set_error(__VA_ARGS__);     \
            return IVIT_ERR_UNSUPPORTED;     \
        }                                    \
    } while (0)

// Every condition of the eight entries, in the order, with the return code and with the text each entry has always answered with.
// The fused entries grew out of ivit_window_attention_i8: what they share names that entry (or the variant a table came with)
// whichever entry was called; the probability entries name themselves.  A family's or an entry's own conditions are marked.
// On success the multipliers and x0 are in the descriptor.
int win_attn_check(WinAttnDesc& d)
{
    const char* fn = d.name;
    const bool ibert = d.family == WIN_IBERT || d.family == WIN_IBERT_PROBS;
    const bool probs = d.family == WIN_SHIFTMAX_PROBS || d.family == WIN_IBERT_PROBS;
    const char* wa = probs ? fn : "ivit_window_attention_i8";      // the name in the texts of the shared conditions
    const bool band_rows_ok = d.band_rows == 256 || d.band_rows == 1;
    const bool band_ok = d.band_w >= 16 && d.band_w <= 192 && d.band_w % 16 == 0 && (uintptr_t)d.band % 16 == 0;      // Shiftmax
    const bool ib_band_ok = d.band_w == 0 || (d.band_w >= 16 && d.band_w <= 256 && d.band_w % 16 == 0);              // I-BERT
    const bool masked_exp_ok = !d.region || (d.masked_exp >= 0.0f && d.masked_exp <= 32768.0f);
    d.Ms = ivit_dyadic_to_double(d.m_s, d.e_s);
    d.Mb = ivit_dyadic_to_double(d.m_b, d.e_b);
    d.Mo = ivit_dyadic_to_double(d.m_o, d.e_o);

    if (probs) {
        if (ibert) IVIT_REQUIRE(d.ib_tab, "%s: NULL operand", fn);
        IVIT_REQUIRE(d.qkv && d.out && d.bias, "%s: NULL operand", fn);
        WIN_UNSUPPORTED(d.head_dim == WHD && d.tokens >= 2 && d.tokens <= 144,
                        "%s: unsupported geometry head_dim=%d tokens=%d (need 32, 2..144)", fn, d.head_dim, d.tokens);
        IVIT_REQUIRE(d.windows > 0 && d.heads > 0 && (int64_t)d.windows * d.heads <= 0x7fffffff / 4 && d.windows_per_image >= 1,
                     "%s: bad window counts", fn);
        IVIT_REQUIRE(!d.region || d.windows % d.windows_per_image == 0, "%s: %d windows are no whole number of images of %d", fn,
                     d.windows, d.windows_per_image);
        IVIT_REQUIRE(d.ldo >= d.tokens, "%s: ldp=%lld below tokens=%d", fn, (long long)d.ldo, d.tokens);
        // the probabilities may start on any byte (the kernel packs dwords where the rows allow it)
        IVIT_REQUIRE(((uintptr_t)d.qkv % 16 == 0) && ((uintptr_t)d.bias % 16 == 0) && ((uintptr_t)d.region % 4 == 0),
                     "%s: misaligned operand (qkv, bias: 16 bytes; region: 4)", fn);
        IVIT_REQUIRE(d.Ms < 2048.0 && d.Mb < 1048576.0, "%s: requant multiplier too large", fn);
        if (ibert) {
            IVIT_REQUIRE((uintptr_t)d.ib_tab % 4 == 0, "%s: misaligned table", fn);
            IVIT_REQUIRE(ib_band_ok, "%s: bad band width %d (a multiple of 16 in [16, 256], or 0 for the full table)", fn, d.band_w);
            IVIT_REQUIRE(masked_exp_ok, "%s: masked_exp=%g outside [0, 32768]", fn, (double)d.masked_exp);
        } else {
            IVIT_REQUIRE(d.band ? (band_ok && band_rows_ok) : d.band_w == 0,
                         "%s: the band table must be 16-byte aligned, its width a multiple of 16 in [16, 192], band_rows 256 or 1", fn);
            IVIT_REQUIRE((d.phi == nullptr) == (d.phim == nullptr), "%s: phi and phim go together", fn);
            // probabilities only: the fused entries leave the phi tables' alignment to the caller
            IVIT_REQUIRE(((uintptr_t)d.phi % 4 == 0) && ((uintptr_t)d.phim % 4 == 0), "%s: misaligned table", fn);
            IVIT_REQUIRE(d.mask_value <= 0 && d.mask_value >= -32768, "%s: mask_value=%d outside [-32768, 0]", fn, d.mask_value);
            IVIT_REQUIRE(d.s_attn > 0.0f, "%s: scale must be positive", fn);
        }
    } else {
        // ---- what an entry checks of its own arguments, before the part the six share
        if (ibert)
            WIN_UNSUPPORTED(d.head_dim == WHD && d.tokens >= 2 && d.tokens <= 144,
                            "%s: unsupported geometry head_dim=%d tokens=%d (need 32, 2..144)", fn, d.head_dim, d.tokens);
        if (d.needs & WIN_NEEDS_BAND) IVIT_REQUIRE(d.band && d.band_w > 0, "%s: no band table", fn);
        // The window geometry, once: required by _unwindow and _long, checked by _band and _ibert where it is given (ws != 0).
        // The short entries answer IVIT_ERR_INVALID, _long and _ibert IVIT_ERR_UNSUPPORTED.
        if ((d.needs & WIN_NEEDS_GEOMETRY) || d.family == WIN_LONG || d.ws != 0) {
            if (!(d.ws > 0 && d.ws * d.ws == d.tokens && d.H > 0 && d.W > 0 && d.H % d.ws == 0 && d.W % d.ws == 0 && d.shift >= 0 &&
                  d.shift < d.ws && d.windows_per_image == (d.H / d.ws) * (d.W / d.ws))) {
                ivit_set_error("%s: H=%d W=%d ws=%d shift=%d do not describe %d windows of %d tokens per image", fn, d.H, d.W, d.ws,
                               d.shift, d.windows_per_image, d.tokens);
                return d.family == WIN_SHORT ? IVIT_ERR_INVALID : IVIT_ERR_UNSUPPORTED;
            }
        }
        if (d.family == WIN_LONG) {
            WIN_UNSUPPORTED(!d.band || (band_ok && band_rows_ok && !d.phi && !d.phim),
                            "%s: bad band table (16-byte aligned, width a multiple of 16 in [16, 192], 256 or 1 rows, "
                            "no phi tables beside it)", fn);
            IVIT_REQUIRE(d.image_order == 0 || d.image_order == 1, "%s: image_order must be 0 or 1", fn);
        }
        if (ibert) {
            WIN_UNSUPPORTED(ib_band_ok, "%s: bad band table (width a multiple of 16 in [16, 256], or 0 for the full table)", fn);
            IVIT_REQUIRE(d.ib_tab, "%s: NULL operand", fn);
            IVIT_REQUIRE((uintptr_t)d.ib_tab % 16 == 0, "%s: misaligned table", fn);
            IVIT_REQUIRE(d.image_order == 0 || (d.image_order == 1 && d.ws != 0),
                         "%s: image_order must be 0 or 1, and 1 needs the windows' geometry", fn);
            IVIT_REQUIRE(masked_exp_ok, "%s: masked_exp=%g outside [0, 32768]", fn, (double)d.masked_exp);
        }
        // ---- the part the six share
        IVIT_REQUIRE(d.qkv && d.out && d.bias, "%s: NULL operand", wa);
        // Shiftmax only (16 band rows per wave in LDS: 4 x 16 x (192 + 4) dwords = 49 KB beside the kernel's 11 KB stay below the 64 KB of
        // a default launch)
        if (!ibert)
            IVIT_REQUIRE(d.band_w == 0 ? d.band == nullptr : (d.band && band_ok),
                         "ivit_window_attention_i8_band: the band table must be 16-byte aligned, its width a multiple of 16 in [16, 192]");
        IVIT_REQUIRE(d.windows > 0 && d.heads > 0 && d.windows_per_image > 0 && d.windows % d.windows_per_image == 0,
                     "%s: bad window counts", wa);
        if (d.family == WIN_SHORT)
            WIN_UNSUPPORTED(d.head_dim == WHD && d.tokens >= 2 && d.tokens <= 64,
                            "%s: unsupported geometry head_dim=%d tokens=%d (need 32, 2..64)", wa, d.head_dim, d.tokens);
        if (d.family == WIN_LONG)
            WIN_UNSUPPORTED(d.head_dim == WHD && d.tokens >= 65 && d.tokens <= 144,
                            "%s: unsupported geometry head_dim=%d tokens=%d (need 32, 65..144)", fn, d.head_dim, d.tokens);
        IVIT_REQUIRE(((uintptr_t)d.qkv % 16 == 0) && ((uintptr_t)d.out % 8 == 0) && d.ldo % 8 == 0 && d.ldo >= (int64_t)d.heads * d.head_dim,
                     "%s: misaligned operand or ldo too small", wa);
        IVIT_REQUIRE(((uintptr_t)d.bias % 8 == 0) && ((uintptr_t)d.region % 4 == 0), "%s: misaligned table", wa);
        IVIT_REQUIRE(d.mask_value <= 0 && d.mask_value >= -32768, "%s: mask_value=%d outside [-32768, 0]", wa, d.mask_value);
        IVIT_REQUIRE(ibert || d.s_attn > 0.0f, "%s: scale must be positive", wa);
        IVIT_REQUIRE((d.phi == nullptr) == (d.phim == nullptr), "ivit_window_attention_i8_compat: phi and phi_masked go together");
        // image order: the kernel divides a query index by ws with (q * (65536 / ws + 1)) >> 16
        for (int qv = 0; qv < (d.tokens > 64 ? d.tokens : 64) && d.image_order; ++qv)
            IVIT_REQUIRE(((qv * (65536 / d.ws + 1)) >> 16) == qv / d.ws, "ivit_window_attention_i8_unwindow: window size %d unsupported", d.ws);
        IVIT_REQUIRE(band_rows_ok, "ivit_window_attention_i8_band: band_rows must be 256 or 1");
        IVIT_REQUIRE(d.Ms < 2048.0 && d.Mb < 1048576.0 && d.Mo < 512.0, "%s: requant multiplier too large", wa);
    }

    d.x0 = -1;      // I-BERT: no Shiftmax constant is read
    if (!ibert) {
        if (const int rc = shiftmax_x0(d.s_attn, -4096, wa, &d.x0)) return rc;
        // exact u32 row sum: tokens * |x0| * 2^15 must stay below 2^32
        IVIT_REQUIRE((double)d.tokens * (double)(-d.x0) * 32768.0 < 4294967296.0, "%s: Shiftmax row sum could overflow 32 bits (x0=%d)",
                     wa, d.x0);
    }
    if (d.family == WIN_SHORT && d.region && !d.phi && !d.band) {
        // Short fused form only, the integer form under a shift mask: its distance table gives a masked score the table's last entry,
        // the saturated value only if the table gets there within its 256 distances (x0 >= -24); the literal form (phi tables) is exact
        // at any scale.  The long form and the probabilities compute the exponent beyond ksat themselves.
        bool saturates;
        shiftmax_ksat(d.x0, &saturates);
        IVIT_REQUIRE(saturates, "%s: x0=%d: the integer form cannot place masked scores (use the phi tables)", wa, d.x0);
    }
    return IVIT_OK;
}

// The softmax form of a checked descriptor: which exponent branch the kernel takes and what it reads there.  The order is band,
// then phi, then the integer form.
struct WinSoftmaxForm {
    int sm;                   // 0 table of distances (power-of-two scales; the one-row band table), 1 literal (phi), 2 band rows, 3 I-BERT
    int x0, ksat;             // ksat: the distance from which the SM 0 table is constant
    int mask_value;           // SM 0: added to a score under the shift mask
    const uint32_t *band, *band1;
    int band_w;
    const float *phi, *phim;
    const float* ib_tab;
    float ib_sat;
};

WinSoftmaxForm win_attn_form(const WinAttnDesc& d)
{
    WinSoftmaxForm f{};
    f.x0 = d.x0;
    f.ksat = shiftmax_ksat(d.x0);
    f.mask_value = d.mask_value;
    f.band_w = d.band_w;
    if (d.family == WIN_IBERT || d.family == WIN_IBERT_PROBS) {
        f.sm = 3;
        f.ib_tab = d.ib_tab;
        f.ib_sat = d.masked_exp;
        if (d.family == WIN_IBERT_PROBS) f.ksat = 255;      // (SM 3 reads neither x0 nor ksat; each struct keeps the value it always carried)
    } else if (d.band && d.band_rows == 256) {
        f.sm = 2;
        f.band = d.band;
    } else if (d.band) {      // one row for every maximum: the distance table of the power-of-two form, with the host's values
        f.band1 = d.band;
        f.ksat = d.band_w - 1;
        f.mask_value = -1024;      // a masked score lands beyond the last (saturated) entry whatever the maximum
    } else if (d.phi) {
        f.sm = 1;
        f.phi = d.phi;
        f.phim = d.phim;
    }
    return f;
}

#undef WIN_UNSUPPORTED

#if IVIT_LAB
// ivit_debug_window_attention_dry_run: the plan of the launch an entry would have made (include/ivit_hip_debug.h has the layout)
enum { WIN_TAB_BAND = 1, WIN_TAB_BAND1 = 2, WIN_TAB_PHI = 4, WIN_TAB_IBERT = 8 };
int win_plan_record(const WinAttnDesc& d, const WinSoftmaxForm& f, int rq32, int long_rows, int ord, unsigned grid, size_t lds_bytes,
                    int kp, int omap_ws, int omap_inv, int dwords)
{
    const int tables = (f.band ? WIN_TAB_BAND : 0) | (f.band1 ? WIN_TAB_BAND1 : 0) | (f.phi ? WIN_TAB_PHI : 0) | (f.ib_tab ? WIN_TAB_IBERT : 0);
    const int32_t plan[16] = {f.sm, rq32, long_rows, ord, (int32_t)grid, (int32_t)lds_bytes, kp, f.x0, f.ksat,
                              f.sm == 0 ? f.mask_value : 0,      // only SM 0 reads it
                              f.band_w, tables, omap_ws, omap_inv, dwords, (int32_t)d.family};
    for (int i = 0; i < 16; ++i) g_winattn_plan[i] = plan[i];
    return IVIT_OK;
}
#endif
