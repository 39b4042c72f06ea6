/*
 * ivit_hip.h -- C ABI of libivit_hip.so: the MI355X (gfx950) integer-only ViT
 * operators that replace the hot path of lionnus/I-ViT
 * (models/quantization_utils/{quant_modules,ivit_modules,quant_utils}.py).
 *
 * The reference has no native interface at all (it is pure PyTorch, float32
 * "fake-quant" emulation), so each entry point below cites the Python code it
 * replaces; INTEGRATION.md shows the ctypes stub a maintainer of the reference
 * would add.  Conventions:
 *   - every function returns 0 on success, a negative IVIT_ERR_* code otherwise;
 *     ivit_last_error_string() describes the last failure on the calling thread;
 *   - all pointers are DEVICE pointers (hipMalloc / torch tensor .data_ptr())
 *     unless a parameter is documented as host scalar; the library allocates
 *     nothing and keeps no state: the caller owns inputs, outputs and tables;
 *   - launches are asynchronous on `stream` (a hipStream_t passed as void*;
 *     NULL = the default stream); functions are re-entrant;
 *   - integer tensors are row-major; `ld*` are leading dimensions in ELEMENTS;
 *   - a dyadic requantiser is the pair (m, e) of the reference's batch_frexp
 *     (quant_utils.py:151-175): out = RNE(z * m / 2^e), 2^30 <= m <= 2^31,
 *     e = 31 - exponent.  Per-channel tables are `const uint32_t* m,
 *     const int32_t* e`; per-tensor requantisers are passed by value.
 */
#ifndef IVIT_HIP_H
#define IVIT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IVIT_OK 0
#define IVIT_ERR_INVALID (-1)     /* bad argument (shape, alignment, NULL)        */
#define IVIT_ERR_UNSUPPORTED (-2) /* valid request this build has no kernel for  */
#define IVIT_ERR_LAUNCH (-3)      /* HIP reported an error at launch              */

typedef void* ivit_stream_t; /* hipStream_t */

int ivit_version(void);
const char* ivit_last_error_string(void);

/* ---- calibration statistics -----------------------------------------------------------------
 * QuantAct running_stat mode (quant_modules.py:310-349) observes x.min() / x.max() of the float view it is handed.
 * out_min_max[0] = min, out_min_max[1] = max over x[0..n) (device float[2]; NaNs are skipped). */
int ivit_minmax_f32(const float* x, int64_t n, float* out_min_max, ivit_stream_t stream);

/* QuantAct with `percentile` set (quant_modules.py:319-329) observes torch.quantile(x_flat, q_lo) and torch.quantile(x_flat, q_hi)
 * instead, q_lo = (100 - p) / 2 / 100, q_hi = (100 - (100 - p) / 2) / 100, rounded to float32 by the caller.
 * out2[0], out2[1] (device float[2]) are those two values, default linear interpolation, bit for bit (a zero may carry either sign):
 *   rank = fl32(q * fl32(n - 1)), lo = floor(rank), hi = ceil(rank), w = rank - lo, a / b = the lo-th / hi-th smallest element,
 *   d = b - a, result = fma(w, d, a) if w < 0.5, else fma(-d, 1 - w, b)   (float32; the last product and sum are one fused
 *   multiply-add, as in torch's lerp kernels; everything else is rounded on its own).
 * A NaN anywhere in x makes both results NaN (torch's rule; ivit_minmax_f32 skips NaNs).  torch refuses n > 2^24; here 1 <= n < 2^31,
 * with fl32(n - 1) rounded to nearest and both indices clamped to n - 1.
 * Exact selection, not a sort: a radix select over an order-preserving 32-bit key, four passes over x, nothing read back.
 * `workspace`: at least IVIT_QUANTILE_WS_BYTES device bytes, 4-byte aligned, any contents; cleared on the stream by the entry itself.
 * x needs 4-byte alignment only. */
#define IVIT_QUANTILE_WS_BYTES 16640
int ivit_quantile_pair_f32(const float* x, int64_t n, float q_lo, float q_hi, float* out2, void* workspace, int64_t workspace_bytes,
                           ivit_stream_t stream);

/* ---- integer parameters of a linear layer while the ranges move -------------------------------
 * QuantLinear / QuantConv2d recompute their integer weights and bias inside every forward (quant_modules.py:202-220, 486-504); a
 * frozen model derives them once on the host (prepare.LinearParams), a calibrating one here, on the device, on every batch.
 *
 * Per-output-row symmetric 8-bit weight quantisation (quant_modules.py:204-215, 488-500; quant_utils.py:52-70, 79-97).
 * For each row r of w [rows, ldw]:
 *   mx       = max(-min_c w[r][c], max_c w[r][c])
 *   scale[r] = max(fl32(mx / 127), FLT_EPSILON)
 *   rs       = fl32(1 / scale[r])
 *   q        = clamp(rint(fl32(rs * w[r][c])), -128, 127)
 *   w8[r * ldo + c] = q   for c < cols
 * Columns >= cols of w8 are not written: the caller zero-fills the K padding.
 * w_int (may be NULL): dense [rows, cols] float32 = (float)q, converted from the integer, so a zero is +0.0f.
 * Every operation is a single IEEE float32 rounding (correctly rounded division, round-to-nearest-even rint, no contraction):
 * prepare.weight_scale and prepare.quant_sym bit for bit.  Denormal weights are not flushed.  Finite weights; on a non-finite one
 * the values are unspecified, the access pattern is the same.
 * One wave per row; 16-byte loads when w is 16-byte aligned and ldw % 4 == 0, dword loads otherwise; a row of up to 4096 columns is
 * read once, a longer one twice.  w, scale and w_int need 4-byte alignment, w8 none.
 * Errors: IVIT_ERR_INVALID for rows or cols below 1, ldw or ldo below cols, a NULL w, scale or w8, a misaligned float pointer. */
int ivit_weight_quant_rows_f32_i8(const float* w, int64_t ldw, int rows, int cols, float* scale, int8_t* w8, int64_t ldo, float* w_int,
                                  ivit_stream_t stream);

/* bias_scaling_factor and the 32-bit bias (quant_modules.py:217-220), s_in the (host scalar) scale of the layer's input:
 *   s_acc[i] = fl32(scale[i] * s_in)
 *   b32[i]   = clamp(rint(fl32(fl32(1 / s_acc[i]) * bias[i])), -2^31, 2^31 - 1)
 * The clamp is prepare.quant_sym's for bits = 32: the float clip bound 2^31 - 1 rounds to 2^31, then the integer minimum applies.
 * bias == NULL (PatchMerging's reduction): b32 and b_int must be NULL too; only s_acc is written.  With a bias, b32 is required.
 * b_int (may be NULL): (float)b32[i].  Finite biases, s_in a positive normal float.
 * Errors: IVIT_ERR_INVALID for n below 1, a NULL scale or s_acc, b32 without bias or bias without b32, b_int without bias, a
 * misaligned pointer (4 bytes). */
int ivit_bias_quant_f32_i32(const float* bias, const float* scale, int n, float s_in, float* s_acc, int32_t* b32, float* b_int,
                            ivit_stream_t stream);

/* ---- input quantisation ---------------------------------------------------------------
 * QuantAct input mode = SymmetricQuantFunction.forward (quant_utils.py:79-97,
 * linear_quantize :13-49):  q = clamp(round(inv_scale * x), -128, 127), inv_scale = fl(1/s)
 * computed by the caller in float32. */
int ivit_quantize_input_f32_i8(const float* x, int8_t* out, int64_t n, float inv_scale, ivit_stream_t stream);
/* the same at any width `bits` <= 32 (e.g. the 16-bit position embedding of pos_encoding_bw = 16), int32 out */
int ivit_quantize_input_f32_i32(const float* x, int32_t* out, int64_t n, float inv_scale, int bits, ivit_stream_t stream);

/* The same fused with the im2col of PatchEmbed's strided convolution
 * (layers_quant.py:197-198, quant_modules.py:506-511):
 *   img [B, chans, hw, hw] float32 -> A [B*(hw/patch)^2, chans*patch*patch] int8,
 *   column order (c, kh, kw) = the flattening of the conv weight [out, c, kh, kw]. */
int ivit_quantize_patchify_f32_i8(const float* img, int8_t* A, int batch, int chans, int hw, int patch,
                                  float inv_scale, ivit_stream_t stream);
/* as above with an explicit row stride lda >= chans*patch*patch (Swin: patch 4 -> K = 48, padded to the GEMM's
 * K granularity of 64); columns [K, lda) are not written: the caller zero-fills them once. */
int ivit_quantize_patchify_ld_f32_i8(const float* img, int8_t* A, int64_t lda, int batch, int chans, int hw, int patch,
                                     float inv_scale, ivit_stream_t stream);
/* The same from uint8 pixels [batch, chans, hw, hw]: lut[c * 256 + v] is the int8 the float pipeline in front of the model gives
 * pixel value v of channel c -- ToTensor (v / 255), Normalize ((x - mean[c]) / std[c]) and the input QuantAct
 * (clamp(round(x / s)), quant_utils.py:79-97), evaluated by the caller in float32 in that order (ivit_amd.prepare.input_lut_u8):
 * the results are identical to the float path on the same pixels and the input is a quarter of the bytes. */
int ivit_quantize_patchify_u8_i8(const uint8_t* img, int8_t* A, int64_t lda, int batch, int chans, int hw, int patch,
                                 const int8_t* lut, ivit_stream_t stream);
/* The two above for images that are not square (img_size = (h, w) of PatchEmbed, layers_quant.py:168-175):
 *   img [batch, chans, h, w] -> A [batch*(h/patch)*(w/patch), chans*patch*patch] int8 with row stride lda,
 *   row (b, py, px) at (b * (h/patch) + py) * (w/patch) + px, column order (c, kh, kw) as above; columns [K, lda) are not written.
 * Every element is computed as in the square forms (h == w gives their bytes): quant_sym of float pixels with inv_scale, the
 * 3 x 256 table `lut` for uint8 pixels (at most 4 channels).
 * Errors: IVIT_ERR_INVALID for a NULL pointer, batch or chans below 1, h or w not a multiple of patch, patch not a multiple of 4
 * (one thread moves 4 consecutive pixels of a row), lda below chans*patch*patch or not a multiple of 4, a misaligned pointer
 * (img: 4 pixels; A: 4 bytes). */
int ivit_quantize_patchify_hw_f32_i8(const float* img, int8_t* A, int64_t lda, int batch, int chans, int h, int w, int patch,
                                     float inv_scale, ivit_stream_t stream);
int ivit_quantize_patchify_hw_u8_i8(const uint8_t* img, int8_t* A, int64_t lda, int batch, int chans, int h, int w, int patch,
                                    const int8_t* lut, ivit_stream_t stream);

/* ---- INT8 GEMM on v_mfma_i32_32x32x32_i8 with fused epilogues -------------------------------
 * QuantLinear.forward / QuantConv2d.forward (quant_modules.py:186-226, 478-511) followed by
 * the QuantAct that always consumes them (quant_modules.py:302-387 -> fixedpoint_mul,
 * quant_utils.py:193-253).
 *   acc[t][n] = sum_k A[t][k] * W[n][k] + bias[n]          (exact int32)
 * A [M, K] int8 (lda), W [N, K] int8 (ldw), bias [N] int32 or NULL.  K % 64 == 0.
 * Contract for the requantising forms: e[n] >= 31 (multiplier <= 1: int32 accumulators -> 8 bits).
 */

/* ---- operand layouts of the GEMMs.  IVIT_LAYOUT_ROWS: row-major with a leading dimension (the default of every
 * entry point).  IVIT_LAYOUT_BLOCKS: 1 KB blocks of 16 rows x 64 bytes, block (row / 16, k / 64) at
 * ((row / 16) * (K / 64) + k / 64) * 1024, and inside a block the 16-byte chunk (r, c) at position 4r + (c ^ ((r >> 2) & 3))
 * -- the order in which the GEMM's LDS-DMA lays a piece into its LDS stage, so that one instruction reads 1 KB
 * contiguous.  Rows padded to a multiple of 16 (ceil(rows / 16) * 16 * K bytes), K % 64 == 0.  The `_ex` forms take
 * `layouts` = IVIT_A_BLOCKS | IVIT_W_BLOCKS; block operands need M >= 2048 and N >= 128.  Producers that can write the
 * block layout directly: ivit_layernorm_i8_ex, ivit_attention_fused_i8_ex, ivit_shiftgelu_lut_i8_ex.  Block offsets are 32-bit: every
 * entry that writes the layout wants (rows + 15) * K < 2^31 and is IVIT_ERR_INVALID beyond.
 *
 * Operands of 2 GiB and more.  Leading dimensions and flat sizes are int64_t and row-major operands are addressed in 64 bits: a row
 * may start at any byte offset.  The exceptions are stated where they apply and refuse (IVIT_ERR_INVALID, nothing launched): the
 * block layout above, IVIT_W_FRAGS16 below, and the dense head-major q/k/v outputs (M * N < 2^31 bytes; planes form
 * 3 * M * heads * head_dim < 2^31).  Fast paths with 32-bit offsets that have a 64-bit form behind them (the streaming int8
 * LayerNorm below 2^31 bytes per matrix, the skinny-K GEMM below M * ldo = 2^32) fall back to it without a visible difference. */
#define IVIT_A_BLOCKS 1
#define IVIT_W_BLOCKS 2
#define IVIT_OUT_BLOCKS 4   /* ivit_gemm_i8_requant_ex only: the int8 output in the block layout (ldo == N, N % 64 == 0) */
/* IVIT_W_FRAGS: `W` is the copy made by ivit_pack_weight_frags_i8 -- the weights in the order the MFMA consumes them, so that
 * a wave loads its fragments straight into registers (1 KB contiguous per instruction) and only the token tile goes through
 * the LDS: channel n, byte k at ((n / 64) * (K / 64) + k / 64) * 4096 + (((n / 32) % 2 * 2 + (k / 32) % 2) * 2 + (k / 16) % 2) * 512
 * + (n % 32) * 16 + k % 16, channels padded with zero rows to a multiple of 64 (ceil(N / 64) * 64 * K bytes).  Needs M >= 2048,
 * N >= 128, N % 64 == 0, K % 192 == 0; combines with IVIT_A_BLOCKS / IVIT_OUT_BLOCKS, not with IVIT_W_BLOCKS.  `ldw` is
 * ignored.  Results are identical to every other form. */
#define IVIT_W_FRAGS 8
int ivit_pack_weight_frags_i8(const int8_t* W, int64_t ldw, int N, int K, int8_t* dst, ivit_stream_t stream);
/* IVIT_W_FRAGS16: the same idea for v_mfma_i32_16x16x64_i8 (the chip holds a higher clock on that shape under the power limit:
 * DESIGN.md section 5): channel n, byte k at ((n / 64) * (K / 64) + k / 64) * 4096 + ((n / 16) % 4) * 1024 + ((k / 16) % 4) * 256
 * + (n % 16) * 16 + k % 16 (copy made by ivit_pack_weight_frags16_i8; same size, same constraints as IVIT_W_FRAGS; the two bits
 * exclude each other).  Accepted by the int8-output `_ex` forms (requant, requant_lut, residual, residual_i16, qkv).  Its epilogue
 * addresses the output and the residual with 32-bit byte offsets: (M + 16) * ldo < 2^32 and (M + 16) * ldr < 2^32, otherwise
 * IVIT_ERR_INVALID (IVIT_W_FRAGS has no such bound). */
#define IVIT_W_FRAGS16 16
int ivit_pack_weight_frags16_i8(const int8_t* W, int64_t ldw, int N, int K, int8_t* dst, ivit_stream_t stream);
int ivit_tile_operand_i8(const int8_t* src, int64_t ld, int64_t rows, int K, int8_t* dst, ivit_stream_t stream);
int ivit_untile_operand_i8(const int8_t* src, int64_t rows, int K, int8_t* dst, int64_t ld, ivit_stream_t stream);

/* out[t][n] = clamp8(RNE(acc * m[n] / 2^e[n]));  N % 16 == 0 */
int ivit_gemm_i8_requant(const int8_t* A, int64_t lda, const int8_t* W, int64_t ldw, const int32_t* bias,
                         const uint32_t* m, const int32_t* e, int8_t* out, int64_t ldo,
                         int M, int N, int K, ivit_stream_t stream);

int ivit_gemm_i8_requant_ex(const int8_t* A, int64_t lda, const int8_t* W, int64_t ldw, const int32_t* bias,
                            const uint32_t* m, const int32_t* e, int8_t* out, int64_t ldo,
                            int M, int N, int K, int layouts, ivit_stream_t stream);

/* ivit_gemm_i8_requant_ex with the width of the QuantAct as a parameter (the width knobs of vit_quant.py:180-187):
 *   out[t][n] = clampB(RNE(acc * m[n] / 2^e[n])),  clamp4 = [-8, 7] (quant_utils.py:209,247-249), the value in an int8 byte.
 * bits = 4 or 8; any other value is IVIT_ERR_INVALID ("bits=.. must be 4 or 8") ahead of everything else, nothing is launched.
 * Every shape, layout and kernel form of ivit_gemm_i8_requant_ex; at bits = 8 the same kernels, byte for byte. */
int ivit_gemm_i8_requant_bits_ex(const int8_t* A, int64_t lda, const int8_t* W, int64_t ldw, const int32_t* bias,
                                 const uint32_t* m, const int32_t* e, int8_t* out, int64_t ldo,
                                 int M, int N, int K, int layouts, int bits, ivit_stream_t stream);

/* ivit_gemm_i8_requant_ex followed by an elementwise int8 -> int8 map on every output: out = lut[k + 128], lut int8[256] -- an
 * operator behind the QuantAct that depends on the value alone (I-BERT GELU + mlp.qact1: ivit_ibert_gelu_build_lut row 0),
 * applied in the epilogue instead of by a kernel of its own.  Needs IVIT_W_FRAGS (the weights-in-registers kernel). */
int ivit_gemm_i8_requant_lut_ex(const int8_t* A, int64_t lda, const int8_t* W, int64_t ldw, const int32_t* bias,
                                const uint32_t* m, const int32_t* e, const int8_t* lut, int8_t* out, int64_t ldo,
                                int M, int N, int K, int layouts, ivit_stream_t stream);

/* as above, then the two-operand QuantAct of the residual connection
 * (vit_quant.py:147,153; quant_utils.py:232-245):
 *   k = clamp8(RNE(acc * m[n] / 2^e[n]))
 *   out = clamp8(RNE(k * m_main / 2^e_main) + RNE(res[t][n] * m_res / 2^e_res))
 * `out` may be `res` itself (in place: one thread reads a residual chunk and writes the same chunk). */
int ivit_gemm_i8_requant_residual(const int8_t* A, int64_t lda, const int8_t* W, int64_t ldw,
                                  const int32_t* bias, const uint32_t* m, const int32_t* e,
                                  const int8_t* res, int64_t ldr, uint32_t m_main, int32_t e_main,
                                  uint32_t m_res, int32_t e_res, int8_t* out, int64_t ldo,
                                  int M, int N, int K, ivit_stream_t stream);

int ivit_gemm_i8_requant_residual_ex(const int8_t* A, int64_t lda, const int8_t* W, int64_t ldw,
                                     const int32_t* bias, const uint32_t* m, const int32_t* e,
                                     const int8_t* res, int64_t ldr, uint32_t m_main, int32_t e_main,
                                     uint32_t m_res, int32_t e_res, int8_t* out, int64_t ldo,
                                     int M, int N, int K, int layouts, ivit_stream_t stream);

/* the same with the widths of its two QuantActs as parameters (attention_out_bw / mlp_out_bw and norm2_in_bw / att_block_out_bw
 * are separate knobs, vit_quant.py:180-187):
 *   k = clamp_mid(RNE(acc * m[n] / 2^e[n]))
 *   out = clamp_out(RNE(k * m_main / 2^e_main) + RNE(res[t][n] * m_res / 2^e_res))
 * bits_mid, bits_out = 4 or 8 independently (clamp4 = [-8, 7]); any other value is IVIT_ERR_INVALID ahead of everything else,
 * nothing is launched.  `out` may be `res` itself.  At (8, 8) the kernels of ivit_gemm_i8_requant_residual_ex, byte for byte. */
int ivit_gemm_i8_requant_residual_bits_ex(const int8_t* A, int64_t lda, const int8_t* W, int64_t ldw,
                                          const int32_t* bias, const uint32_t* m, const int32_t* e,
                                          const int8_t* res, int64_t ldr, uint32_t m_main, int32_t e_main,
                                          uint32_t m_res, int32_t e_res, int8_t* out, int64_t ldo,
                                          int M, int N, int K, int layouts, int bits_mid, int bits_out, ivit_stream_t stream);

/* Swin form of the above: the residual stream is 16 bits wide (swin_quant.py:299, mlp.fc2 + shortcut):
 *   k = clamp8(RNE(acc * m[n] / 2^e[n]))                       (mlp.qact2)
 *   out = clamp16(RNE(k * m_main / 2^e_main) + RNE(res[t][n] * m_res / 2^e_res))   (qact4, 16 bit)
 * res / out: int16 rows, ldr / ldo in elements and multiples of 8.  Replaces ivit_gemm_i8_requant followed by
 * ivit_residual_requant_i16(a_bits = 8). */
int ivit_gemm_i8_requant_residual_i16(const int8_t* A, int64_t lda, const int8_t* W, int64_t ldw,
                                      const int32_t* bias, const uint32_t* m, const int32_t* e,
                                      const int16_t* res, int64_t ldr, uint32_t m_main, int32_t e_main,
                                      uint32_t m_res, int32_t e_res, int16_t* out, int64_t ldo,
                                      int M, int N, int K, ivit_stream_t stream);
int ivit_gemm_i8_requant_residual_i16_ex(const int8_t* A, int64_t lda, const int8_t* W, int64_t ldw,
                                         const int32_t* bias, const uint32_t* m, const int32_t* e,
                                         const int16_t* res, int64_t ldr, uint32_t m_main, int32_t e_main,
                                         uint32_t m_res, int32_t e_res, int16_t* out, int64_t ldo,
                                         int M, int N, int K, int layouts, ivit_stream_t stream);

/* as ivit_gemm_i8_requant but the output is written head-major for the attention kernel:
 * N = 3 * heads * head_dim, row t = b * tokens + tok  ->
 *   qkv[which][b][h][tok][d],  n = which*heads*head_dim + h*head_dim + d
 * (the reshape/permute of vit_quant.py:65-71).  head_dim % 16 == 0. */
int ivit_gemm_i8_requant_qkv(const int8_t* A, int64_t lda, const int8_t* W, int64_t ldw, const int32_t* bias,
                             const uint32_t* m, const int32_t* e, int8_t* qkv, int tokens, int heads,
                             int head_dim, int M, int N, int K, ivit_stream_t stream);
int ivit_gemm_i8_requant_qkv_ex(const int8_t* A, int64_t lda, const int8_t* W, int64_t ldw, const int32_t* bias,
                                const uint32_t* m, const int32_t* e, int8_t* qkv, int tokens, int heads,
                                int head_dim, int M, int N, int K, int layouts, ivit_stream_t stream);
/* the same for `nplanes` consecutive planes of q / k / v starting at `plane0` (0 <= plane0, 1 <= nplanes, plane0 + nplanes <= 3):
 * N = nplanes * heads * head_dim.  W, bias, m, e point at the FIRST SELECTED channel (plane0 * heads * head_dim rows into the
 * weight: the same byte offset in every weight layout when heads * head_dim % 64 == 0); `qkv` is the whole [3][B][H][T][d]
 * buffer, of which only the selected planes are written. */
int ivit_gemm_i8_requant_qkv_planes_ex(const int8_t* A, int64_t lda, const int8_t* W, int64_t ldw, const int32_t* bias,
                                       const uint32_t* m, const int32_t* e, int8_t* qkv, int tokens, int heads,
                                       int head_dim, int plane0, int nplanes, int M, int N, int K, int layouts,
                                       ivit_stream_t stream);

/* 16-bit per-channel QuantAct of the accumulators (Swin attn.proj + attn.qact4, swin_quant.py:164-166):
 *   out[t][n] = clamp16(RNE(acc * m[n] / 2^e[n])),  out int16 [M, N] (ldo in elements), N % 4 == 0, ldo % 4 == 0.
 * Followed by ivit_residual_requant_i16(a_bits = 16) it replaces ivit_gemm_i8_i32 + ivit_residual_requant_i16(a_bits = 32)
 * with half the intermediate bytes. */
int ivit_gemm_i8_requant_i16(const int8_t* A, int64_t lda, const int8_t* W, int64_t ldw, const int32_t* bias,
                             const uint32_t* m, const int32_t* e, int16_t* out, int64_t ldo, int M, int N, int K,
                             ivit_stream_t stream);

/* the two calls above in one (ViT attn.proj + attn.qact3 at 16 bits + qact2, mlp.fc2 + mlp.qact2 at 16 bits + qact4,
 * vit_quant.py:131-150 with attention_out_bw = mlp_out_bw = norm2_in_bw = att_block_out_bw = 16):
 *   k16 = clamp16(RNE(acc * m[n] / 2^e[n])),  out = clamp16(RNE(k16 * M_main) + RNE(res * M_res)),  res / out int16 rows.
 * `layouts`: IVIT_W_FRAGS (optionally | IVIT_A_BLOCKS) where that form applies -- the epilogue is then transposed through LDS --
 * or 0: any shape, the 128 x 128-tile kernel with the epilogue straight from its registers (Swin attn.proj at C = 96 .. 384).
 * N % 8 == 0, ldr / ldo multiples of 8, res / out 16-byte aligned; out may alias res. */
int ivit_gemm_i8_requant_i16_residual_i16_ex(const int8_t* A, int64_t lda, const int8_t* W, int64_t ldw, const int32_t* bias,
                                             const uint32_t* m, const int32_t* e, const int16_t* res, int64_t ldr,
                                             uint32_t m_main, int32_t e_main, uint32_t m_res, int32_t e_res, int16_t* out,
                                             int64_t ldo, int M, int N, int K, int layouts, ivit_stream_t stream);

/* raw accumulators (classifier head; module-level QuantLinear): out int32 [M, N], N % 4 == 0 */
int ivit_gemm_i8_i32(const int8_t* A, int64_t lda, const int8_t* W, int64_t ldw, const int32_t* bias,
                     int32_t* out, int64_t ldo, int M, int N, int K, ivit_stream_t stream);

/* ivit_gemm_plan: HOST function -- which kernel an ivit_gemm_i8_* entry runs for a shape and on which grid, by the very function
 * the launcher calls (csrc/gemm.hip gemm_plan).  The weight copy a caller hands over has to match that form: row-major for
 * SMALL and SKINNY, any of row-major / IVIT_W_BLOCKS for PERS, the fragment copies for WREG / WREG16.  The rule in short:
 *   SKINNY  requant / qkv epilogue, no layout bit, M >= 8192, 32 <= K <= 128, K % 32 == 0, 16 <= N <= 320, N % 16 == 0
 *   WREG(16) IVIT_W_FRAGS(16): needs M >= 2048, N >= 128, N % 64 == 0, K % 192 == 0, refuses otherwise
 *   PERS    a requantising epilogue with int8 accumulator QuantAct, M >= 2048, N >= 128 (block operands refuse below that)
 *   SMALL   everything else
 * epilogue: IVIT_GEMM_EPI_*, the epilogue of the entry asked about (requant_ex / _bits_ex / _lut_ex: RQ; requant_residual(_bits)_ex:
 * RESID; requant_qkv(_planes)_ex: QKV; i8_i32: I32; requant_residual_i16_ex: RESID16; requant_i16: RQ16;
 * requant_i16_residual_i16_ex: RQ16_RES16).  Operands are taken as dense (lda = ldw = K, ldo = ldr = N) and 16-byte aligned.
 * out8 (host) = form (IVIT_GEMM_FORM_*), workgroups, tiles_m, tiles_n, split_from (tiles from this one on run as two half tiles),
 * skinny variant (K / 32 of the instantiation: 4, 2; 0 = run-time K), dynamic LDS bytes, 1 if 256-channel tiles waste at most an
 * eighth of their columns at this N (the callers' condition for a fragment copy whose consumer has no 128-channel items).
 * Errors: the launcher's own -- IVIT_ERR_INVALID with its message where a launch of that shape and layout would refuse -- and
 * IVIT_ERR_INVALID for a NULL out8 or an unknown epilogue.  Launches nothing, calls no HIP function. */
#define IVIT_GEMM_EPI_RQ 0
#define IVIT_GEMM_EPI_RESID 1
#define IVIT_GEMM_EPI_QKV 2
#define IVIT_GEMM_EPI_I32 3
#define IVIT_GEMM_EPI_RESID16 4
#define IVIT_GEMM_EPI_RQ16 5
#define IVIT_GEMM_EPI_RQ16_RES16 6
#define IVIT_GEMM_FORM_SMALL 0
#define IVIT_GEMM_FORM_PERS 1
#define IVIT_GEMM_FORM_WREG 2
#define IVIT_GEMM_FORM_WREG16 3
#define IVIT_GEMM_FORM_SKINNY 4
int ivit_gemm_plan(int epilogue, int M, int N, int K, int layouts, int32_t* out8);

/* ---- fused attention core -------------------------------------------------------------------
 * vit_quant.py:72-85: matmul_1 (q.k^T) -> qact_attn1 -> IVITIntSoftmax (Shiftmax,
 * ivit_modules.py:150-179) -> matmul_2 (P.v) -> qact2, per (image, head), never
 * materialising the [B,H,T,T] score tensor.
 *   qkv   [3][B][H][T][head_dim] int8 (as written by ivit_gemm_i8_requant_qkv)
 *   out   [B*T, H*head_dim] int8, column h*head_dim + d (the transpose(1,2).reshape of :83)
 *   (m_s, e_s): requantiser of q.k^T into the Shiftmax input (8 bit)
 *   s_attn: float32 scale of the Shiftmax input (x0 = floor(-1/s_attn), n = 15)
 *   (m_o, e_o): requantiser of P.v into the 8-bit output.
 * Supported: head_dim 64, 1 <= tokens <= 208 (13 key tiles of 16; 193 .. 208 take the tuned form in which only the last key tile is
 * partial, fewer tokens the general one); IVIT_ERR_UNSUPPORTED ("unsupported geometry") otherwise.
 * All ivit_attention_* entries below share one argument check and one launcher; a message names the entry that was called. */
int ivit_attention_fused_i8(const int8_t* qkv, int8_t* out, int batch, int heads, int tokens, int head_dim,
                            uint32_t m_s, int32_t e_s, float s_attn, uint32_t m_o, int32_t e_o,
                            ivit_stream_t stream);
/* out_blocks = 1: `out` ([batch*tokens, heads*head_dim]) is written in IVIT_LAYOUT_BLOCKS (the A operand of attn.proj) */
int ivit_attention_fused_i8_ex(const int8_t* qkv, int8_t* out, int batch, int heads, int tokens, int head_dim,
                               uint32_t m_s, int32_t e_s, float s_attn, uint32_t m_o, int32_t e_o, int out_blocks,
                               ivit_stream_t stream);

/* Natural ("as calibrated", non power-of-two) Shiftmax input scale.  The reference's Shiftmax then runs its float32
 * sequence on phi(q) = fl(fl(q*s)/s) instead of q (ivit_modules.py:165-170: QuantAct returned q*s, quant_modules.py:387;
 * the .to(int32) of :166 is discarded), so exp_int depends on (row max, q) jointly.  exp2d: [256][256] uint32 on the
 * device, entry (qmax+128)*256 + (q+128) = exp_int of that pair, tabulated by the caller with the reference's float32
 * steps (i-vit_amd/prepare.py shiftexp2d); NULL = power-of-two scale (identical to ivit_attention_fused_i8_ex). */
int ivit_attention_fused_i8_compat(const int8_t* qkv, int8_t* out, int batch, int heads, int tokens, int head_dim,
                                   uint32_t m_s, int32_t e_s, float s_attn, uint32_t m_o, int32_t e_o,
                                   const uint32_t* exp2d, int out_blocks, ivit_stream_t stream);

/* The same with the table also in BAND form, staged per query tile in LDS (the fast path; exp2d may then be NULL):
 * band[(qmax+128)*band_w + j] = exp_int of (qmax, q = qmax - j) for j < band_w, band_w a multiple of 16 in [16, 256] (4 x 16 x (band_w + 4) x 4 bytes of dynamic LDS on top of 31 KiB static: 97 KiB at 256, within the 160 KiB of a CU; launches above 64 KiB are covered by test_attention_fused_compat) chosen
 * by the caller such that entry band_w - 1 is already the saturated value (the exponent's argument is clamped at n*x0,
 * ivit_modules.py:155, so every larger distance gives the same entry); i-vit_amd/prepare.py shiftexp_band. */
int ivit_attention_fused_i8_compat_band(const int8_t* qkv, int8_t* out, int batch, int heads, int tokens, int head_dim,
                                        uint32_t m_s, int32_t e_s, float s_attn, uint32_t m_o, int32_t e_o,
                                        const uint32_t* exp2d, const uint32_t* band, int band_w, int out_blocks,
                                        ivit_stream_t stream);
/* the same with the softmax output width as a parameter (softmax_bw, vit_quant.py:184): softmax_bits = 4, 8 or 16.  16:
 * p = floor(fl32(e * factor) / 2^16) <= 2^15 at scale 2^-15 (ivit_modules.py:175-176), carried into P.V as three 7-bit planes;
 * (m_o, e_o) then is the requantiser of 2^-15 * s_v.  4: p = floor(fl32(e * factor) / 2^28) < 8 at scale 2^-3, the 8-bit code
 * path with another power-of-two scale; (m_o, e_o) is the requantiser of 2^-3 * s_v. */
int ivit_attention_fused_i8_wide(const int8_t* qkv, int8_t* out, int batch, int heads, int tokens, int head_dim, uint32_t m_s,
                                 int32_t e_s, float s_attn, uint32_t m_o, int32_t e_o, const uint32_t* exp2d,
                                 const uint32_t* band, int band_w, int softmax_bits, int out_blocks, ivit_stream_t stream);

/* Long rows: the same Shiftmax attention (8-bit probabilities) for 208 <= tokens <= 1025 (e.g. 384 / 16 -> 577, 224 / 8 -> 785,
 * 512 / 16 -> 1025 tokens), which ivit_attention_fused_i8_compat_band rejects.  Arguments as there.
 * Preconditions: head_dim 64; qkv, out non-NULL and 16-byte aligned; x0 = floor(-1/s_attn) in [-4096, -1] (the row sum is exact
 * in 64 bits for every such x0); multipliers m_s * 2^-e_s < 2048, m_o * 2^-e_o < 512; band_w = 0 or a band table as above
 * (16-byte aligned, width a multiple of 16 in [16, 256], entry band_w - 1 saturated); band_w = 0 and exp2d non-NULL: the
 * full [256][256] table; both absent: power-of-two scale.  out_blocks = 1: IVIT_LAYOUT_BLOCKS output below 2 GiB.
 * Errors: IVIT_ERR_UNSUPPORTED ("unsupported geometry") outside the token range or for another head_dim, IVIT_ERR_INVALID
 * ("NULL operand", ...) otherwise. */
int ivit_attention_fused_i8_long(const int8_t* qkv, int8_t* out, int batch, int heads, int tokens, int head_dim, uint32_t m_s,
                                 int32_t e_s, float s_attn, uint32_t m_o, int32_t e_o, const uint32_t* exp2d,
                                 const uint32_t* band, int band_w, int out_blocks, ivit_stream_t stream);

/* Long rows with the softmax output width as a parameter: ivit_attention_fused_i8_long's arguments, layouts, tables and
 * preconditions (208 <= tokens <= 1025, head_dim 64, x0 in [-4096, -1], the same multiplier bounds, all three Shiftmax regimes,
 * both output layouts) plus softmax_bits = 4, 8 or 16, as ivit_attention_fused_i8_wide has it for up to 208 keys.
 *   16: p = floor(fl32(e * factor) / 2^16) <= 2^15 at scale 2^-15 (ivit_modules.py:175-176) on the long kernel's row organisation
 *       (packed scores, exact 64-bit row sum, the clamp at 2^31), carried into P.V as three 7-bit planes; (m_o, e_o) is the
 *       requantiser of 2^-15 * s_v, applied to O = sum p * v (|O| < 2^29 for 1025 keys) in the reference's two steps: the
 *       float64 product rounded at 53 bits, then the rounding to an integer (quant_utils.py:229-230).
 *   8:  exactly ivit_attention_fused_i8_long.
 *   4:  p = floor(fl32(e * factor) / 2^28) < 8 at scale 2^-3: the 8-bit kernels with the factor scaled by 2^-4 (exact).
 * Errors: any other softmax_bits is IVIT_ERR_INVALID ("softmax_bits must be 4, 8 or 16") ahead of everything else; then as
 * ivit_attention_fused_i8_long: IVIT_ERR_UNSUPPORTED ("unsupported geometry") outside the token range or for another
 * head_dim, IVIT_ERR_INVALID ("NULL operand", ...) otherwise. */
int ivit_attention_fused_i8_wide_long(const int8_t* qkv, int8_t* out, int batch, int heads, int tokens, int head_dim,
                                      uint32_t m_s, int32_t e_s, float s_attn, uint32_t m_o, int32_t e_o, const uint32_t* exp2d,
                                      const uint32_t* band, int band_w, int softmax_bits, int out_blocks, ivit_stream_t stream);

/* One query per (image, head): the attention of a block whose output is read for one token only (the class token of the last
 * block, vit_quant.py:302-304).  The arithmetic of ivit_attention_fused_i8_compat_band for that query, bit for bit.
 *   k, v  [batch][heads][tokens][64] int8: planes 1 and 2 of the head-major qkv buffer
 *   q     [batch][heads * 64] int8, row-major, dense: the query of each image
 *   out   [batch][ldo] int8, heads * 64 bytes per row, column h * 64 + d
 * Requantisers and tables as ivit_attention_fused_i8_compat_band (band_w > 0: the band table; else exp2d non-NULL: the full
 * table; both absent: power-of-two scale).  Preconditions: head_dim 64, 1 <= tokens <= 208 (IVIT_ERR_UNSUPPORTED otherwise);
 * operands 16-byte aligned, ldo >= heads * 64 and a multiple of 16; x0 and the multipliers in the ranges stated there. */
int ivit_attention_cls_i8(const int8_t* k, const int8_t* v, const int8_t* q, int8_t* out, int64_t ldo, int batch, int heads,
                          int tokens, int head_dim, uint32_t m_s, int32_t e_s, float s_attn, uint32_t m_o, int32_t e_o,
                          const uint32_t* exp2d, const uint32_t* band, int band_w, ivit_stream_t stream);

/* ---- I-LayerNorm + the QuantAct behind it ---------------------------------------------------
 * IVITIntLayerNorm.forward (ivit_modules.py:30-65) then QuantAct (fixedpoint_mul).
 *   x [rows, C] int8 (ldx), per channel: bias_int[c] = floor((beta/gamma)/(sqrt(C)/2^30)),
 *   s_ln[c] = (sqrt(C)/2^30)*gamma[c] (both float32, prepared by the caller as the reference
 *   computes them, :53-62), (m[c], e[c]) requantiser s_ln[c] -> output scale; contract e[c] >= 40
 *   (multiplier <= 2^-9: I-LayerNorm outputs are ~30-bit integers requantised to 8 bits).
 *   out [rows, C] int8 (ldo).  C % 4 == 0, C <= 4096. */
int ivit_layernorm_i8(const int8_t* x, int64_t ldx, int rows, int C, const float* bias_int, const float* s_ln,
                      const uint32_t* m, const int32_t* e, int8_t* out, int64_t ldo, ivit_stream_t stream);
/* out_blocks = 1: `out` is written in IVIT_LAYOUT_BLOCKS (C % 64 == 0, ldo == C, rows padded to 16) */
int ivit_layernorm_i8_ex(const int8_t* x, int64_t ldx, int rows, int C, const float* bias_int, const float* s_ln,
                         const uint32_t* m, const int32_t* e, int8_t* out, int64_t ldo, int out_blocks,
                         ivit_stream_t stream);

/* The same for an input carried at a natural (non power-of-two) scale s: IVITIntLayerNorm sees phi(q) = fl(fl(q*s)/s)
 * (ivit_modules.py:36).  remap[q+128] = trunc(phi(q)) (int8, the `.to(int32)` of :38) and phi[q+128] (float32; the mean of
 * :37 is taken over these: equal to RNE(sum q / C) except on rows whose integer sum is an exact .5 tie, where torch's CPU
 * float32 reduction order decides -- restated in the kernel).  Both tables on the device, prepared by the caller
 * (i-vit_amd/prepare.py phi_tables).  C % 8 == 0, C >= 32. */
int ivit_layernorm_i8_compat(const int8_t* x, int64_t ldx, int rows, int C, const float* bias_int, const float* s_ln,
                             const uint32_t* m, const int32_t* e, const int8_t* remap /* [256] */,
                             const float* phi /* [256] */, int8_t* out, int64_t ldo, int flags,
                             ivit_stream_t stream);
#define IVIT_LN_OUT_BLOCKS 1              /* `flags` of ivit_layernorm_i8_compat: `out` in IVIT_LAYOUT_BLOCKS */
#define IVIT_LN_OUTER_MEAN(L) ((L) << 8)  /* tie rows in torch's outer-reduction order for a transposed view of contiguous extent L
                                           * (see ivit_layernorm_f32_f32_ex): the Swin patch embedding */

/* module-level form: int32 input (8 or 16 bit values), float32 output y*s_ln (ivit_modules.py:63) */
int ivit_layernorm_i32_f32(const int32_t* x, int64_t ldx, int rows, int C, const float* bias_int,
                           const float* s_ln, float* out, int64_t ldo, ivit_stream_t stream);

/* ---- Token features: the LayerNorm's own float32 output from the integer stream -----------------
 * The tensor the module returns, out = fl(y_int * s_ln[c]) (ivit_modules.py:63; ibert_modules.py:153 for the I-BERT entries
 * further down), computed straight from the int8 / int16 rows the engines carry: the statistics and the element chain of the
 * int8-emitting entries above, without the QuantAct behind them (csrc/ln_tokens.h).  Four entries share the row selection and
 * the output forms:
 *   rows     token-major with a leading dimension, as ivit_tokens_to_nchw_* addresses them: row (b, t) of the selection
 *            (B, T_all, t0, T) is read at (b * T_all + t0 + t) * ldx.  t0 = 1 skips a class token, (t0, T) = (0, 1) takes it alone.
 *   flags    0: rows, out[(b * T + t) * ldo + c], ldo >= C (NLC).  IVIT_LN_F32_CHANNEL_MAJOR: out[(b * C + c) * ldo + t], ldo >= T;
 *            ldo == T is the dense [B, C, T] tensor (NCHW for a Gh x Gw grid), written in one launch through LDS in runs of up to
 *            16 consecutive tokens per channel, no float intermediate in memory.
 * Preconditions of all four: B, T, C >= 1, 0 <= t0, t0 + T <= T_all, ldx >= C, pointers aligned to their elements
 * (IVIT_ERR_INVALID, as a NULL operand or an unknown flag); C <= 4096 (IVIT_ERR_UNSUPPORTED).  Nothing is launched on an error.
 *
 * ivit_layernorm_i8_f32: int8 rows.  remap == phi == NULL: the integers (ivit_layernorm_i8); both given: the natural-scale form
 * of ivit_layernorm_i8_compat, tie rows in the inner reduction order.  Preconditions of those entries, IVIT_ERR_UNSUPPORTED:
 * C % 4 == 0 (with tables: C % 8 == 0, C >= 32), ldx % 4 == 0 and x 4-byte aligned, bias_int and s_ln 16-byte aligned. */
#define IVIT_LN_F32_CHANNEL_MAJOR 1
#define IVIT_LN_F32_FAST_DIV 2       /* the 16-bit entries at a scale: the Markstein quotient, as fast_division = 1 of their siblings */
int ivit_layernorm_i8_f32(const int8_t* x, int64_t ldx, int B, int T_all, int t0, int T, int C, const float* bias_int,
                          const float* s_ln, const int8_t* remap /* [256] or NULL */, const float* phi /* [256] or NULL */,
                          float* out, int64_t ldo, int flags, ivit_stream_t stream);
/* int16 rows (any C <= 4096, rows aligned to 2 bytes).  s_in == 0: the integers (ivit_layernorm_i16_i8: float32 mean in torch's
 * order from |sum| = 2^24 on, int32 squares that wrap, the ten Newton steps literally).  s_in > 0: the natural-scale form of
 * ivit_layernorm_i16_i8_compat on phi(q) = fl(fl(q * s_in) / s_in), flags | IVIT_LN_F32_FAST_DIV where the caller has checked the
 * three-instruction quotient for all 65536 inputs (prepare.markstein_division_ok); with s_in == 0 that flag is IVIT_ERR_INVALID. */
int ivit_layernorm_i16_f32(const int16_t* x, int64_t ldx, int B, int T_all, int t0, int T, int C, float s_in, const float* bias_int,
                           const float* s_ln, float* out, int64_t ldo, int flags, ivit_stream_t stream);

/* module-level LITERAL form, any input scale: x is the float view q*s the reference's module receives, s_in its scale
 * (n_s = 1 per tensor, or C per channel).  Every float32 step of ivit_modules.py:36-63 as written, including the mean over
 * x/s in torch's CPU reduction order (decides rows whose mean is an exact .5 tie when s is not a power of two) and the
 * truncating .to(int32).  Equals ivit_layernorm_i32_f32 on round(x/s) when s is a power of two. */
int ivit_layernorm_f32_f32(const float* x, int64_t ldx, int rows, int C, const float* s_in, int n_s,
                           const float* bias_int, const float* s_ln, float* out, int64_t ldo, ivit_stream_t stream);
/* outer_mean = L > 0: the caller's tensor reaches the reference's `x_int.mean(axis=2)` as a TRANSPOSED view (the reduced dimension
 * is not the contiguous one: the Swin patch embedding, layers_quant.py:198-201, whose elementwise QuantAct keeps the strides of
 * `x.flatten(2).transpose(1, 2)`); L = extent of the contiguous dimension (tokens per image), rows % L == 0, row = image * L +
 * column.  ATen then sums every row with its outer-reduction order (csrc/rowsum.h: one cascade over the reduced index for
 * columns below 32 * (L / 32), four interleaved cascades for the last L % 32 columns) instead of the 32-partial-sum order of a
 * contiguous row; rows whose mean is an exact .5 tie come out differently.  `x` itself is still passed row-contiguous. */
int ivit_layernorm_f32_f32_ex(const float* x, int64_t ldx, int rows, int C, const float* s_in, int n_s,
                              const float* bias_int, const float* s_ln, float* out, int64_t ldo, int outer_mean,
                              ivit_stream_t stream);

/* ---- ShiftGELU -----------------------------------------------------------------------------
 * IVITIntGELU.forward (ivit_modules.py:89-126, n = 23, output_bit = 8) on rows of L int8 values
 * with input scale s, followed by the per-tensor QuantAct (m, e) -> int8.
 * Direct arithmetic form: */
int ivit_shiftgelu_i8(const int8_t* x, int64_t ldx, int rows, int L, float s, uint32_t m, int32_t e,
                      int8_t* out, int64_t ldo, ivit_stream_t stream);
/* module-level form: int32 output k*sigmoid_int (ivit_modules.py:123), no requant */
int ivit_shiftgelu_i8_i32(const int8_t* x, int64_t ldx, int rows, int L, float s, int32_t* out, int64_t ldo,
                          ivit_stream_t stream);
/* Table form used by the engine: for a fixed (s, m, e) the result depends only on (row max, k):
 * lut[(kmax+128)*256 + (k+128)] = int8 result.  Build once per layer at load time ... */
int ivit_shiftgelu_build_lut(float s, uint32_t m, int32_t e, int8_t* lut /* [256*256] */, ivit_stream_t stream);
/* natural input scale: remap[q+128] = trunc(phi(q)) (device, [256] int8; ivit_modules.py:106-107) is applied to k and to the
 * row maximum before the arithmetic; remap == NULL is ivit_shiftgelu_build_lut */
int ivit_shiftgelu_build_lut_ex(float s, uint32_t m, int32_t e, const int8_t* remap, int8_t* lut /* [256*256] */,
                                ivit_stream_t stream);
/* ... then per call: wave-per-row max reduction + LDS-staged table row + byte gather.  L % 4 == 0. */
int ivit_shiftgelu_lut_i8(const int8_t* x, int64_t ldx, int rows, int L, const int8_t* lut, int8_t* out,
                          int64_t ldo, ivit_stream_t stream);
/* layouts bit 0: `out` is written in IVIT_LAYOUT_BLOCKS (L % 64 == 0, ldo == L, rows padded to 16); bit 1: `x` is read in
 * it (ldx == L).  In place (out == x) is allowed when both sides use the same layout and, row-major, the same stride (ldx == ldo):
 * with two strides the rows of `out` overlap other rows of `x`, IVIT_ERR_INVALID. */
int ivit_shiftgelu_lut_i8_ex(const int8_t* x, int64_t ldx, int rows, int L, const int8_t* lut, int8_t* out,
                             int64_t ldo, int layouts, ivit_stream_t stream);

/* ---- stand-alone Shiftmax (module-level IVITIntSoftmax, ivit_modules.py:164-179) -----------------
 * x [rows, L] int8 with scale s -> out [rows, L] int8 in [0, 127] (scale 2^-7).  L >= 2, no upper limit (a one-column row would
 * give 128 = 1.0, which int8 cannot hold: refused, as by every form below); x0 = floor(-1 / s) in [-65535, -1] (the row sum is
 * kept in 64 bits). */
int ivit_shiftmax_i8(const int8_t* x, int64_t ldx, int rows, int L, float s, int8_t* out, int64_t ldo,
                     ivit_stream_t stream);
/* module-level LITERAL form, any input scale: x is the float view the reference's module receives (q*s, plus Swin's float
 * mask); every float32 step of ivit_modules.py:150-176 on x/s as written (the reference discards its .to(int32), :166),
 * the row sum in torch's CPU reduction order.  L >= 2 (see above), x0 = floor(-1 / s) in [-1048576, -1]. */
int ivit_shiftmax_f32_i8(const float* x, int64_t ldx, int rows, int L, float s, int8_t* out, int64_t ldo,
                         ivit_stream_t stream);
/* the same with a wider output (IVITIntSoftmax(output_bit), the reference's softmax_bw knob, vit_quant.py:184): int16 values in
 * [0, 2^(output_bit-1) - 1], scale 2^-(output_bit-1); output_bit 2 .. 16, L >= 2 */
int ivit_shiftmax_f32_i16(const float* x, int64_t ldx, int rows, int L, float s, int output_bit, int16_t* out, int64_t ldo,
                          ivit_stream_t stream);
/* the same on int32 inputs, |x| < 2^28: Swin adds the shift mask (-100/s, beyond 8 bits) to the scores in front of
 * the softmax (swin_quant.py:151-156); L and s as for ivit_shiftmax_i8 */
int ivit_shiftmax_i32_i8(const int32_t* x, int64_t ldx, int rows, int L, float s, int8_t* out, int64_t ldo,
                         ivit_stream_t stream);

/* ---- generic QuantAct on integers (fixedpoint_mul, quant_utils.py:193-253) ---------------------
 * z [rows, C] int32; (m,e) per channel (n_me == C) or per tensor (n_me == 1); optional identity
 * branch z2 with (m2,e2) (n_me2 in {0,1,C}); bits in {8,16,32}; out int32 [rows, C]. */
int ivit_requant_i32(const int32_t* z, int64_t rows, int C, const uint32_t* m, const int32_t* e, int n_me,
                     const int32_t* z2, const uint32_t* m2, const int32_t* e2, int n_me2, int bits,
                     int32_t* out, ivit_stream_t stream);

/* int8 two-operand form (Block.qact2 / qact4 as a stand-alone op) */
int ivit_residual_requant_i8(const int8_t* a, uint32_t m_a, int32_t e_a, const int8_t* b, uint32_t m_b,
                             int32_t e_b, int8_t* out, int64_t n, ivit_stream_t stream);
/* the same with the output width as a parameter: out = clampB(RNE(a * m_a / 2^e_a) + RNE(b * m_b / 2^e_b)), bits = 4 ([-8, 7]) or 8;
 * any other value is IVIT_ERR_INVALID and nothing is launched.  At 8 exactly ivit_residual_requant_i8. */
int ivit_residual_requant_i8_bits(const int8_t* a, uint32_t m_a, int32_t e_a, const int8_t* b, uint32_t m_b,
                                  int32_t e_b, int8_t* out, int64_t n, int bits, ivit_stream_t stream);

/* ---- cls token + position embedding (vit_quant.py:290-296) -------------------------------------
 * patch [B*(T-1), C] int8 (PatchEmbed output); out [B*T, C] int8:
 *   out[b][0][:]   = cls_row[:]                    (constant, prepared by the caller)
 *   out[b][1+p][c] = clamp8(RNE(patch*m/2^e) + pos_add[1+p][c])
 * pos_add [T, C] int16 = RNE(qact_pos(pos_embed) * m_pos / 2^e_pos) prepared by the caller. */
int ivit_embed_assemble_i8(const int8_t* patch, const int16_t* pos_add, const int8_t* cls_row, uint32_t m,
                           int32_t e, int8_t* out, int batch, int tokens, int C, ivit_stream_t stream);
/* the same with the width of qact1 (block_input_bw) as a parameter: out[b][1+p][c] = clampB(RNE(patch*m/2^e) + pos_add[1+p][c]),
 * bits = 4 ([-8, 7]) or 8; any other value is IVIT_ERR_INVALID and nothing is launched.  The caller prepares cls_row (copied as it
 * is) and pos_add at the widths of their own QuantActs.  At 8 exactly ivit_embed_assemble_i8. */
int ivit_embed_assemble_i8_bits(const int8_t* patch, const int16_t* pos_add, const int8_t* cls_row, uint32_t m,
                                int32_t e, int8_t* out, int batch, int tokens, int C, int bits, ivit_stream_t stream);

/* the same for a 16-bit patch embedding and block input (patch_embed_bw = block_input_bw = 16, vit_quant.py:180-187):
 * out16 = clamp16(RNE(patch16 * m / 2^e) + pos_add[tok][c]) for tok >= 1, out16[b][0] = cls_row; pos_add int32 [tokens, C]. */
int ivit_embed_assemble_i16(const int16_t* patch, const int32_t* pos_add, const int16_t* cls_row, uint32_t m,
                            int32_t e, int16_t* out, int batch, int tokens, int C, ivit_stream_t stream);

/* ---- classifier output (quant_modules.py:225-226; scripts/inference.py:249-250) ----------------
 * logits_f32[b][n] = fl(float(acc[b][n]) * s_acc[n]); top1[b] = argmax_n logits_f32 (first max).
 * logits_f32 may be NULL. */
int ivit_head_argmax(const int32_t* acc, const float* s_acc, int batch, int N, float* logits_f32,
                     int32_t* top1, ivit_stream_t stream);

/* Top-k classes per row (scripts/inference.py:245-254 takes top-1/3/5).  acc [batch][ld] int32, s_acc [ld]:
 *   logits_f32[b][n] = fl(float(acc[b*ld+n]) * s_acc[n]) for n < ld -- the values ivit_head_argmax writes (may be NULL);
 *   topk [batch][k] int32 = the k largest of logits_f32[b][0..N), value descending, equal values by ascending index
 *   (= torch.sort(logits[:, :N], descending=True, stable=True).indices[:, :k]; -0.0 == +0.0).  Column 0 is
 *   ivit_head_argmax's top1.  Columns N..ld-1 (the padded classes of a head whose width is rounded up) are never selected.
 * targets (int32 [batch], may be NULL) with hits (uint64 [k]): hits[r] += 1 for every row whose target is topk[b][r]; hits
 * accumulates over calls (never zeroed here); a target outside [0, N) never hits.  Logits must be finite (NaN: unspecified).
 * IVIT_ERR_INVALID, nothing launched: k outside [1, min(N, IVIT_TOPK_MAX)], N > ld, NULL topk, or exactly one of
 * targets / hits given. */
#define IVIT_TOPK_MAX 8
int ivit_head_topk(const int32_t* acc, const float* s_acc, int batch, int ld, int N, int k, float* logits_f32,
                   int32_t* topk, const int32_t* targets, uint64_t* hits, ivit_stream_t stream);
/* the same selection and hit count on float32 logits rows [batch][ld] (module path: any caller's logits) */
int ivit_logits_topk_f32(const float* logits, int batch, int ld, int N, int k, int32_t* topk, const int32_t* targets,
                         uint64_t* hits, ivit_stream_t stream);

/* ---- module-level QuantMatMul (quant_modules.py:404-409): batched int8 matmul -> int32 ----------
 * qk: S[b][i][j] = sum_d Q[b][i][d] * K[b][j][d];  pv: O[b][i][d] = sum_j P[b][i][j] * V[b][j][d].
 * All operands dense row-major per batch entry. */
int ivit_bgemm_qk_i8(const int8_t* Q, const int8_t* K, int32_t* S, int batch, int Tq, int Tk, int D,
                     ivit_stream_t stream);
int ivit_bgemm_pv_i8(const int8_t* P, const int8_t* V, int32_t* O, int batch, int Tq, int Tk, int D,
                     ivit_stream_t stream);
/* P of more than 8 bits.  CONTRACT: P is a softmax output -- every row of P sums to at most 2^15 + Tk (Shiftmax with output_bit
 * up to 16), so |acc| <= 128 * (2^15 + Tk) < 2^23; arbitrary int16 P would overflow the int32 accumulator from Tk = 512 on and is
 * not checked (for wider or unbounded P use ivit_bgemm_pv_i32_i8, which takes and checks a bound) */
int ivit_bgemm_pv_i16_i8(const int16_t* P, const int8_t* V, int32_t* O, int batch, int Tq, int Tk, int D,
                         ivit_stream_t stream);
/* P as int32 with |P| <= p_absmax (I-BERT's softmax with output_bit = 16 reaches 2^15 on a one-hot row, ibert_modules.py:314);
 * refused when p_absmax * 128 * Tk does not fit int32 */
int ivit_bgemm_pv_i32_i8(const int32_t* P, const int8_t* V, int32_t* O, int batch, int Tq, int Tk, int D, int64_t p_absmax,
                         ivit_stream_t stream);

/* ---- float <-> integer views at module edges (quant_utils.py:220; quant_modules.py:223,385-387) --
 * z = round(x / s[c]) (mode 0) or trunc(x / s[c]) (mode 1, the `.to(int32)` of ivit_modules.py:38,107);
 * y = float(z) * s[c].  n_s in {1, C}. */
int ivit_f32_to_i32(const float* x, int64_t rows, int C, const float* s, int n_s, int mode, int32_t* z,
                    ivit_stream_t stream);
int ivit_i32_to_f32(const int32_t* z, int64_t rows, int C, const float* s, int n_s, float* y,
                    ivit_stream_t stream);

/* int32 integer view -> int8 operand of the GEMM / matmul kernels (module-level path).  Values outside
 * [-128, 127] saturate and set *overflow_flag (device int32, may be NULL) to 1. */
int ivit_narrow_i32_i8(const int32_t* z, int8_t* out, int64_t n, int32_t* overflow_flag, ivit_stream_t stream);

/* =================================================================================================
 * Swin (models/swin_quant.py): 16-bit residual stream, windowed attention, patch merging, pooling.
 * The window partition, cyclic shift and their inverses (swin_quant.py:18-50, 258-271, 278-289) are row
 * permutations of a [B, H*W, C] tensor; kernels that take (H, W, ws, shift) apply
 *   win_row(b, y, x) = window-major index of token (b, (y - shift) mod H, (x - shift) mod W)
 * on the fly (ws == 0: identity), so no partitioned copy of the activations is ever materialised.
 * ================================================================================================= */

/* 8 -> 16 bit QuantAct (SwinTransformer.qact1, swin_quant.py:546): out = clamp16(RNE(x * m / 2^e)).
 * With (m, e) = (2^30, 30) it is the exact int8 -> int16 widening used behind PatchMerging. */
int ivit_requant_i8_i16(const int8_t* x, uint32_t m, int32_t e, int16_t* out, int64_t n, ivit_stream_t stream);

/* Two-operand 16-bit QuantAct of the residual connections (SwinTransformerBlock.qact2 / qact4,
 * swin_quant.py:293,299; quant_utils.py:232-245):
 *   out[r][c] = clamp16(RNE(k[win_row(r)][c] * m_a / 2^e_a) + RNE(res[r][c] * m_r / 2^e_r))
 * a_bits = 8 / 16: k = a (int8 / int16 [rows, C]);
 * a_bits = 32: a holds raw int32 accumulators of attn.proj and k = clamp16(RNE(a * m_pre[c] / 2^e_pre[c]))
 *   is the 16-bit attn.qact4 (swin_quant.py:166) fused in; (m_pre, e_pre) must be NULL otherwise.
 * The window map applies to `a` only (window_reverse + un-shift, swin_quant.py:278-289). C % 4 == 0. */
int ivit_residual_requant_i16(const void* a, int a_bits, const uint32_t* m_pre, const int32_t* e_pre, uint32_t m_a,
                              int32_t e_a, const int16_t* res, uint32_t m_r, int32_t e_r, int16_t* out, int64_t rows,
                              int C, int H, int W, int ws, int shift, ivit_stream_t stream);

/* I-LayerNorm on the 16-bit stream + 8-bit QuantAct (ivit_modules.py:30-65 with the Newton iteration on
 * float32(var), as the reference runs it); row r of x is written to row win_row(r) of out (stride ldo >= C):
 * norm1 writes straight into window order (swin_quant.py:258-271).  Same constants and contract as
 * ivit_layernorm_i8.  Domain: every int16 row whose variance sum the reference itself can take, its two float32 / int32 effects
 * included -- a row whose integer sum reaches 2^24 in magnitude takes the mean from the float32 sum in torch's CPU reduction order
 * (:37), and the squares are int32 as the reference's (:41: they wrap from |x - mean| = 46 341 on), summed in int64.  A row whose
 * wrapped sum is zero or negative is outside it (the reference divides by zero): its bytes are unspecified, nothing else is written.
 * ivit_layernorm_i16_i8_compat, ivit_layernorm_i32_f32 and ivit_layernorm_f32_f32(_ex) treat both steps the same way
 * (tests/golden/ln16_bigrows_kat.npz). */
int ivit_layernorm_i16_i8(const int16_t* x, int rows, int C, const float* bias_int, const float* s_ln,
                          const uint32_t* m, const int32_t* e, int8_t* out, int64_t ldo, int H, int W, int ws, int shift,
                          ivit_stream_t stream);
/* the same for a 16-bit input carried at a natural scale s_in: the reference's LayerNorm sees fl(fl(q*s_in)/s_in) (float32 mean
 * over those values in torch's CPU reduction order, truncating .to(int32), ivit_modules.py:36-38).  fast_division = 1: the
 * caller has verified (exhaustively over the 65 536 inputs, prepare.markstein_division_ok) that the 3-instruction quotient by
 * the invariant s_in -- q0 = x*r, e = fma(-s, q0, x), fma(e, r, q0) with r = RN(1/s_in) -- is the correctly rounded one for this
 * s_in, which enables the tiled kernel; 0: the literal one-wave-per-row kernel with IEEE divisions.  fast_division |
 * IVIT_LN_OUTER_MEAN(L): the reference takes this mean over a transposed view of contiguous extent L (see
 * ivit_layernorm_f32_f32_ex: Swin's first norm1, whose input still carries the patch embedding's layout). */
int ivit_layernorm_i16_i8_compat(const int16_t* x, int rows, int C, float s_in, int fast_division, const float* bias_int,
                                 const float* s_ln, const uint32_t* m, const int32_t* e, int8_t* out, int64_t ldo, int H, int W,
                                 int ws, int shift, ivit_stream_t stream);

/* PatchMerging gather (swin_quant.py:337-344): x [B, H*W, C] int16 -> out [B, (H/2)*(W/2), 4C],
 * channel blocks (even y, even x), (odd y, even x), (even y, odd x), (odd y, odd x). */
int ivit_patch_merge_i16(const int16_t* x, int16_t* out, int batch, int H, int W, int C, ivit_stream_t stream);

/* Window partition + cyclic shift of whole rows (swin_quant.py:258-271: reshape(B, H, W, C), roll by -shift, window_partition),
 * or the way back (window_reverse, roll by +shift, :281-289), for rows of row_bytes bytes of any element type (int8 rows of C
 * bytes, int16 rows of 2C bytes): src, dst [batch * H * W, row_bytes].
 *   inverse = 0: dst row (b, wy, wx, iy, ix), window order, = src row (b, (wy ws + iy + shift) % H, (wx ws + ix + shift) % W)
 *   inverse = 1: dst row (b, (wy ws + iy + shift) % H, (wx ws + ix + shift) % W) = src row (b, wy, wx, iy, ix)
 * Refused: NULL pointers or pointers not aligned to 16 bytes, row_bytes % 16 != 0 or row_bytes > 2^20 (the chunk index of a row is
 * 32-bit; rows * row_bytes is 64-bit and may pass 4 GiB), H * W > 2^30, H % ws or W % ws != 0, shift outside [0, ws),
 * overlapping src and dst (src == dst among them: the pass is not in place). */
int ivit_window_rows(const void* src, void* dst, int batch, int H, int W, int64_t row_bytes, int ws, int shift, int inverse,
                     ivit_stream_t stream);

/* AdaptiveAvgPool1d over the tokens + qact3 (swin_quant.py:554-555):
 *   out[b][c] = clamp8(RNE(round(fl32(sum_t x[b][t][c] / tokens)) * m / 2^e)) */
int ivit_avgpool_requant_i8(const int8_t* x, int8_t* out, int batch, int tokens, int C, uint32_t m, int32_t e,
                            ivit_stream_t stream);
/* The same at a natural input scale s_in, literally: y = fl(x * s_in), the float32 mean over the tokens in the order of torch's CPU
 * reduction over the transposed view (per column c the outer-reduction cascade of csrc/rowsum.h, the four-partial form for the tail
 * columns c >= 32 * (C / 32)) divided by float32(tokens), then qact3's steps: z = rint(fl(mean / s_in)), out = clamp8(RNE(z * m / 2^e)).
 * That is the order torch's serial reduction takes; above 32768 input elements torch splits the work over its threads, along the batch
 * when batch >= the thread count (same order), else along the columns (a different order for the tail columns). */
int ivit_avgpool_requant_i8_literal(const int8_t* x, int8_t* out, int batch, int tokens, int C, float s_in, uint32_t m, int32_t e,
                                    ivit_stream_t stream);
/* The float mean of that pooling alone, for a caller that holds the float tensor (the module path's avgpool(x.transpose(1, 2)) on the
 * GPU): x [batch, tokens, C] float32, dense; out [batch, C] = the same outer-reduction sum over the tokens / float32(tokens).
 * Errors: IVIT_ERR_INVALID for a NULL or misaligned (4 bytes) pointer or a dimension below 1. */
int ivit_avgpool_f32_literal(const float* x, float* out, int batch, int tokens, int C, ivit_stream_t stream);

/* WindowAttention core (swin_quant.py:137-161): matmul_1 -> qact_attn1 -> + relative position bias through the
 * two-operand qact2 -> + shift mask -> Shiftmax -> matmul_2 -> qact3, one wave per (window, head).
 *   qkv      [3][windows][heads][tokens][32] int8 (ivit_gemm_i8_requant_qkv on window-ordered rows)
 *   out      [windows*tokens, ldo] int8, column h*32 + d
 *   bias_add [heads][tokens][64] int16 = RNE(qact_table(table)[index] * m2 / 2^e2) (key index padded to 64): the
 *            identity operand of qact2, a load-time constant
 *   mask_region [windows_per_image][64] uint8 or NULL (un-shifted block): region id of every token of a window of
 *            the rolled image (the img_mask of swin_quant.py:223-243); scores of (query, key) pairs from different
 *            regions get mask_value = -100 / s_attn (an integer in the supported regime) added after qact2's clamp,
 *            as the reference adds the float mask to the fake-quantised scores (:149-155, 243-246)
 *   (m_s,e_s): q.k^T -> qact_attn1;  (m_b,e_b): qact_attn1 -> qact2;  s_attn: scale of qact2 (Shiftmax input);
 *   (m_o,e_o): P.v -> qact3.
 * Supported: head_dim 32, 2 <= tokens <= 64; with a mask, s_attn >= 1 / 24 (x0 = floor(-1 / s_attn) >= -24: the exponent table
 * over the 256 distances to the row maximum has saturated by its last entry, which masked scores take) -- below that the
 * entry refuses and the literal form of ivit_window_attention_i8_compat applies (exact at any scale). */
int ivit_window_attention_i8(const int8_t* qkv, int8_t* out, int64_t ldo, const int16_t* bias_add,
                             const uint8_t* mask_region, int mask_value, int windows, int windows_per_image, int heads,
                             int tokens, int head_dim, uint32_t m_s, int32_t e_s, uint32_t m_b, int32_t e_b,
                             float s_attn, uint32_t m_o, int32_t e_o, ivit_stream_t stream);
/* Natural (non power-of-two) scale s_attn of the Shiftmax input: phi[q+128] = fl(fl(q*s)/s) is what the reference's Shiftmax
 * sees of an unmasked score q, phi_masked[q+128] = fl(fl(fl(q*s) - 100)/s) of a score under the shift mask
 * (swin_quant.py:151-156 adds float -100 to q*s; ivit_modules.py:165 divides by s); the kernel runs the float32 sequence of
 * ivit_modules.py:150-170 on those values per score.  Both tables float32 [256] on the device (prepare.py); both NULL =
 * ivit_window_attention_i8. */
int ivit_window_attention_i8_compat(const int8_t* qkv, int8_t* out, int64_t ldo, const int16_t* bias_add,
                                    const uint8_t* mask_region, int mask_value, int windows, int windows_per_image, int heads,
                                    int tokens, int head_dim, uint32_t m_s, int32_t e_s, uint32_t m_b, int32_t e_b,
                                    float s_attn, uint32_t m_o, int32_t e_o, const float* phi, const float* phi_masked,
                                    ivit_stream_t stream);
/* Natural scale, table form (round 4): Shiftmax's exp_int of a score q under the row maximum qmax is read from
 * band[(qmax + 128) * band_w + min(qmax - q, band_w - 1)] (uint32 [256][band_w] on the device, band_w a multiple of 16 in [16, 192],
 * 16-byte aligned; prepare.shiftexp_band: the float32 sequence of ivit_modules.py:150-170 evaluated for every pair on the host, as
 * ivit_attention_fused_i8_compat_band does for ViT).  Scores under the shift mask take the saturated entry band_w - 1: the caller
 * hands the table over only when that is what the reference computes for every masked score and no masked score can be a row
 * maximum (prepare.window_shiftexp_band checks both; otherwise the literal form above runs).  band_rows = 256, or 1 when the rows
 * of the table do not depend on the maximum (the host compares them): `band` is then that one row [band_w] and the kernel runs
 * exactly as at a power-of-two scale, on these values.  (The saturation rule itself -- from which distance the exponent's
 * argument is clamped at 15 x0 -- has one home on the host, shiftmax_ksat in csrc/common.h; every attention launcher takes it there,
 * and the conditions and the form selection of all eight window-attention entries are csrc/win_attn_host.h.)
 * ws != 0: output rows at their image positions as in
 * ivit_window_attention_i8_unwindow (H, W, ws, shift); ws == 0: window order. */
int ivit_window_attention_i8_band(const int8_t* qkv, int8_t* out, int64_t ldo, const int16_t* bias_add, const uint8_t* mask_region,
                                  int windows, int windows_per_image, int heads, int tokens, int head_dim, uint32_t m_s, int32_t e_s,
                                  uint32_t m_b, int32_t e_b, float s_attn, uint32_t m_o, int32_t e_o, const uint32_t* band,
                                  int band_w, int band_rows, int H, int W, int ws, int shift, ivit_stream_t stream);
/* The same with the output rows at their IMAGE positions: window_reverse and the roll back (swin_quant.py:278-287) applied to
 * the row index here, `out` [batch * H * W, heads * head_dim].  attn.proj is row-wise, so it and the residual QuantAct behind it
 * then work on image-ordered rows without a map (ivit_gemm_i8_requant_i16_residual_i16_ex).  tokens == ws * ws, windows_per_image
 * == (H / ws) * (W / ws), 0 <= shift < ws. */
int ivit_window_attention_i8_unwindow(const int8_t* qkv, int8_t* out, int64_t ldo, const int16_t* bias_add,
                                      const uint8_t* mask_region, int mask_value, int windows, int windows_per_image, int heads,
                                      int tokens, int head_dim, uint32_t m_s, int32_t e_s, uint32_t m_b, int32_t e_b,
                                      float s_attn, uint32_t m_o, int32_t e_o, const float* phi, const float* phi_masked,
                                      int H, int W, int ws, int shift, ivit_stream_t stream);
/* Windows of 65..144 tokens (ws = 9..12, Swin at 384 px with 12 x 12 windows): the arithmetic of ivit_window_attention_i8 with every
 * form of the entries above in one entry.  Layouts differ from the short entries in the key padding only: bias_add [heads][tokens][kp]
 * int16 and mask_region [windows_per_image][kp] uint8 (or NULL), kp = 16 * ceil(tokens / 16).  Shiftmax form: band != NULL the table
 * form of ivit_window_attention_i8_band (band_w, band_rows = 256 or 1; mask_value unused; phi tables NULL); else phi / phi_masked the
 * literal form of ivit_window_attention_i8_compat; else the power-of-two form with the integer mask_value.  H, W, ws, shift describe
 * the windows (tokens == ws * ws, windows_per_image == (H / ws) * (W / ws), 0 <= shift < ws) in both output orders; image_order = 1
 * writes the rows at their image positions as ivit_window_attention_i8_unwindow does, 0 in window order.
 * Errors: IVIT_ERR_UNSUPPORTED for tokens outside 65..144, head_dim != 32, a bad band table or a window description that does not
 * match; IVIT_ERR_INVALID ("NULL operand", alignment, multipliers) otherwise. */
int ivit_window_attention_i8_long(const int8_t* qkv, int8_t* out, int64_t ldo, const int16_t* bias_add, const uint8_t* mask_region,
                                  int mask_value, int windows, int windows_per_image, int heads, int tokens, int head_dim, uint32_t m_s,
                                  int32_t e_s, uint32_t m_b, int32_t e_b, float s_attn, uint32_t m_o, int32_t e_o, const float* phi,
                                  const float* phi_masked, const uint32_t* band, int band_w, int band_rows, int H, int W, int ws,
                                  int shift, int image_order, ivit_stream_t stream);
/* Window attention with IBERTIntSoftmax (ibert_modules.py:237-319, output_bit 8) in place of Shiftmax: Swin built with
 * softmax_type='ibert'.  Operands and layouts of ivit_window_attention_i8_long for every window of 2..144 tokens: head-major qkv,
 * bias_add [heads][tokens][kp] int16 and mask_region [windows_per_image][kp] uint8 (or NULL) with kp = 64 up to 64 tokens and
 * 16 * ceil(tokens / 16) above, (m_s,e_s), (m_b,e_b), (m_o,e_o).  table: float32 on the device, 16-byte aligned -- band_w == 0 the
 * [256][256] table of ivit_ibert_softmax_build_table for the scale of attn.qact2, band_w > 0 (a multiple of 16, at most 256) its band
 * form table[(qmax + 128) * band_w + min(qmax - q, band_w - 1)] as ivit_attention_fused_i8_ibert takes it.  Behind the lookup the
 * arithmetic is that entry's: the row sum in float32 in torch's CPU order (csrc/rowsum.h), factor = floor(2^32 / sum),
 * p = floor(fl(e * factor) / 2^25) in [0, 128] -- 128 reaches P.V --, then (m_o,e_o).
 * ws == 0: no window geometry, rows out in window order (image_order must be 0); ws != 0: H, W, ws, shift describe the windows
 * (tokens == ws * ws, windows_per_image == (H / ws) * (W / ws), 0 <= shift < ws) and image_order = 1 writes the rows at their image
 * positions as ivit_window_attention_i8_unwindow does.
 * PRECONDITION the caller proves and the entry cannot check (prepare.ibert_window_mask_ok does, for all 256 x 256 pairs of a
 * masked score q and a row maximum qm, in the reference's float32 sequence): the reference adds float -100 to q * s_attn under the
 * shift mask, so a masked score lies off the integer grid; with mask_region != NULL every masked score must land on int_exp's clamp
 * 30 * x0_int whatever the maximum, and none may be a row maximum (about s_attn <= 0.29).  Each masked score then contributes
 * masked_exp, the one saturated value (c_int through the softmax's internal 16-bit QuantAct), and takes no part in the maximum.
 * Where the proof fails the caller runs the attention core literally.
 * Errors: IVIT_ERR_UNSUPPORTED for tokens outside 2..144, head_dim != 32, a bad band width or a window description that does not
 * match; IVIT_ERR_INVALID ("NULL operand", alignment, multipliers, masked_exp outside [0, 32768]) otherwise. */
int ivit_window_attention_i8_ibert(const int8_t* qkv, int8_t* out, int64_t ldo, const int16_t* bias_add, const uint8_t* mask_region,
                                   float masked_exp, int windows, int windows_per_image, int heads, int tokens, int head_dim,
                                   uint32_t m_s, int32_t e_s, uint32_t m_b, int32_t e_b, uint32_t m_o, int32_t e_o, const float* table,
                                   int band_w, int H, int W, int ws, int shift, int image_order, ivit_stream_t stream);
/* The softmax probabilities of a window attention, written to memory: the P the entries above multiply with V (attention maps; an
 * inspection path of one launch, csrc/swin_probs.hip).  probs: uint8 [nwin][heads][tokens][ldp], scale 2^-7, ldp >= tokens; row
 * (window, head, query) holds the query's probabilities over the keys 0 .. tokens - 1, queries and keys in window order, windows in
 * the order of window_partition on the rolled map: the tensor attn.log_int_softmax returns (swin_quant.py:121-169), divided by its
 * scale.  Bytes tokens .. ldp - 1 of a row are never written; rows are stored as dwords where probs and ldp are multiples of four.
 * Inputs as the entries above for every window of 2..144 tokens: qkv int8 [3][nwin][heads][tokens][32] (16-byte aligned), bias
 * int16 [heads][tokens][kp] (16-byte aligned) and region uint8 [windows_per_image][kp] (4-byte aligned, or NULL: no shift mask; a
 * window's row is region[win % windows_per_image]) with kp = 64 up to 64 tokens and 16 * ceil(tokens / 16) above, (m_s,e_s) of
 * qact_attn1 and (m_b,e_b) of qact2's main operand.  Shiftmax form, as swin_engine.window_attention selects it: band != NULL with
 * band_rows = 256 the band table [256][band_w] of ivit_window_attention_i8_band, with band_rows = 1 its one-row form (band 16-byte
 * aligned, band_w a multiple of 16 in [16, 192]; mask_value and the phi tables are not used); else phi / phim (float32 [256] each)
 * the literal form of ivit_window_attention_i8_compat; else the power-of-two form with the integer mask_value in [-32768, 0].  The
 * power-of-two form places a masked score at any input scale (beyond the table of distances it evaluates exp_int itself).  A row
 * whose exact sum of exponents reaches 2^24 takes the float32 sum in torch's order (csrc/rowsum.h), as the reference does.
 * Errors: IVIT_ERR_UNSUPPORTED for tokens outside 2..144 or head_dim != 32; IVIT_ERR_INVALID otherwise (NULL operand, ldp < tokens,
 * alignment, band width or rows, multipliers, window counts: windows_per_image >= 1, and nwin a multiple of it when region is
 * given).  A rejected call writes nothing. */
int ivit_window_attention_probs_u8(const int8_t* qkv, uint8_t* probs, int64_t ldp, const int16_t* bias, const uint8_t* region,
                                   int mask_value, int nwin, int windows_per_image, int heads, int tokens, int head_dim,
                                   uint32_t m_s, int32_t e_s, uint32_t m_b, int32_t e_b, float s_attn,
                                   const float* phi, const float* phim, const uint32_t* band, int band_w, int band_rows, ivit_stream_t stream);
/* The same for IBERTIntSoftmax (ivit_window_attention_i8_ibert, its PRECONDITION on the shift mask included): table float32 on the
 * device, 4-byte aligned -- band_w == 0 the [256][256] table of ivit_ibert_softmax_build_table, band_w > 0 (a multiple of 16, at
 * most 256) its band form; masked_exp the one value of a score under the shift mask.  The row sum is float32 in torch's order,
 * factor = floor(2^32 / sum), p = floor(fl(e * factor) / 2^25) in [0, 128]; a one-hot row's 128 is the byte 0x80.  probs, layouts
 * and errors as ivit_window_attention_probs_u8 (and masked_exp outside [0, 32768] with a region: IVIT_ERR_INVALID). */
int ivit_window_attention_probs_u8_ibert(const int8_t* qkv, uint8_t* probs, int64_t ldp, const int16_t* bias, const uint8_t* region,
                                         float masked_exp, int nwin, int windows_per_image, int heads, int tokens, int head_dim,
                                         uint32_t m_s, int32_t e_s, uint32_t m_b, int32_t e_b, const float* table, int band_w, ivit_stream_t stream);

/* =================================================================================================
 * I-BERT operator family (models/quantization_utils/ibert_modules.py; registry key 'ibert', the fork's default,
 * vit_quant.py:188-190).  Module-level kernels: integer activations in, the module's output out.  The scalar
 * constants are the float32 values the reference computes on the host side of every call (floor(coef / scale) ...);
 * the caller passes them by value.  Each kernel performs the reference's float32 operations in the reference's
 * order (see csrc/ibert.hip), the row sums of the softmax and of the LayerNorm included: they are added in torch's CPU
 * reduction order (csrc/rowsum.h), which matters as soon as a sum passes 2^24 (16-bit LayerNorm inputs, long near-flat
 * softmax rows): the integer-input kernels equal the literal forms below on x = k * s for every power-of-two s.
 * ================================================================================================= */

/* IBERTIntGELU.forward (:220-235) on integers k (= x / scaling_factor):
 *   sigmoid_int = floor(sign(k) * ((min(|k|, -b_int) + b_int)^2 + c_int) / 2^6);  out = k * (sigmoid_int + shift_int)
 * out holds the integer x_int of :231; the module's float output is out * s_out (s_out computed by the caller, :232). */
int ivit_ibert_gelu_i32(const int32_t* k, int64_t n, float b_int, float c_int, float shift_int, int32_t* out,
                        ivit_stream_t stream);

/* IBERTIntSoftmax.forward (:297-319) on rows of L integers: int_exp (:285-295, n = 30) with x0_int, b_int, c_int and
 * scale exp_sf; the module's internal QuantAct(16) (self.act, :260,308) as the dyadic (m_act, e_act) = batch_frexp(
 * exp_sf / act_sf) with the fake-quant round trip through act_sf; row sum; factor = floor(2^32 / sum);
 * out = floor(exp_int * factor / 2^(32 - output_bit + 1)) in [0, 2^(output_bit-1)], scale 2 / 2^output_bit.
 * If exp_out != NULL only exp_int (float, [rows, L] dense) is produced: the statistics pass of the internal QuantAct
 * in calibration mode (out may then be NULL). */
int ivit_ibert_softmax_i32(const int32_t* k, int64_t ldx, int rows, int L, float x0_int, float b_int, float c_int,
                           float exp_sf, float act_sf, uint32_t m_act, int32_t e_act, int output_bit, int32_t* out,
                           int64_t ldo, float* exp_out, ivit_stream_t stream);

/* IBERTIntLayerNorm.forward (:112-158, use_int_sqrt = False): mean_int = round(sum / C); y = k - mean_int;
 * var = sum floor(y / 2^shift)^2; std = floor(sqrt(var)) * 2^shift; factor = floor(2^31 / std);
 * out[c] = (floor(y * factor / 2) + bias_int[c]) * s_out[c]  (float32, the module's output; s_out = sqrt(C)/2^30 * gamma). */
int ivit_ibert_layernorm_i32_f32(const int32_t* k, int64_t ldx, int rows, int C, const float* bias_int,
                                 const float* s_out, float shift_pow2, float* out, int64_t ldo, ivit_stream_t stream);

/* use_int_sqrt = True (:142-143): std = integer_sqrt(var) * 2^shift in every I-BERT LayerNorm entry below that takes this flag.
 * integer_sqrt (:85-109) on the float32 row sum n = var:
 *   0 for n <= 0;  bits = floor(log2(max(n, 1))) + 1 with the log2 a correctly rounded FLOAT32 -- it is E for a value within
 *   floor(ln 2 * 2^P) float32 steps below 2^E, P = ceil(log2 E) - 1 (e.g. 2^24 - 11 .. 2^24 - 1 -> bits 25), so bits is not the bit
 *   length;  x = 2^ceil(bits / 2);  four times:  inv = floor(n / max(x, 1)),  x = floor((x + inv) / 2)  in float32;  int32(x).
 * It is not floor(sqrt(n)) either: four steps can stop on the upper value of a two-cycle (3 -> 2, 15 -> 4, 255 -> 16,
 * 16777215 -> 4096).  The kernels run the four steps literally (csrc/isqrt.h).  n = 0 gives std = 0 and factor = floor(2^31 / 0) as
 * in the reference.
 * The flag is the whole of `flags` in the _ex entries; in ivit_ibert_layernorm_i8 it is OR-ed into `out_blocks`, in
 * ivit_ibert_layernorm_i16_i8_ex into `fast_division` (as ivit_layernorm_i8_compat takes IVIT_LN_OUTER_MEAN above its layout bit).
 * Without it every entry computes what it computed before the flag existed. */
#define IVIT_IBERT_LN_INT_SQRT 0x100
/* ivit_ibert_layernorm_i32_f32 with flags = 0 or IVIT_IBERT_LN_INT_SQRT; IVIT_ERR_INVALID for any other bit */
int ivit_ibert_layernorm_i32_f32_ex(const int32_t* k, int64_t ldx, int rows, int C, const float* bias_int,
                                    const float* s_out, float shift_pow2, float* out, int64_t ldo, int flags,
                                    ivit_stream_t stream);

/* LITERAL forms of the three I-BERT operators: the float view x = q*s and its scale in, the reference's float32 sequence on
 * x / s itself (ibert_modules.py:126, 226, 303) -- any scale, not only the power-of-two ones for which x / s is the integer q;
 * row sums in torch's CPU reduction order.  Outputs are the modules' float outputs (GELU :234, Softmax :319, LayerNorm :153). */
int ivit_ibert_gelu_f32_f32(const float* x, int64_t n, float s, float b_int, float c_int, float shift_int, float s_out,
                            float* out, ivit_stream_t stream);
int ivit_ibert_softmax_f32_f32(const float* x, int64_t ldx, int rows, int L, float s, float x0_int, float b_int, float c_int,
                               float exp_sf, float act_sf, uint32_t m_act, int32_t e_act, int output_bit, float* out,
                               int64_t ldo, float* exp_out, ivit_stream_t stream);
int ivit_ibert_layernorm_f32_f32(const float* x, int64_t ldx, int rows, int C, const float* s_in, int n_s,
                                 const float* bias_int, const float* s_out, float shift_pow2, float* out, int64_t ldo,
                                 ivit_stream_t stream);
/* the literal LayerNorm with flags = 0 or IVIT_IBERT_LN_INT_SQRT (above); IVIT_ERR_INVALID for any other bit */
int ivit_ibert_layernorm_f32_f32_ex(const float* x, int64_t ldx, int rows, int C, const float* s_in, int n_s,
                                    const float* bias_int, const float* s_out, float shift_pow2, float* out, int64_t ldo,
                                    int flags, ivit_stream_t stream);

/* ---- the I-BERT family inside the fused int8 engine (engine.py, family "ibert"; ibert_modules.py:12-319) ---------------
 * int8 activations in and out; every operator runs the reference's float32 sequence on fl(q * s) (what its float tensors hold)
 * and fuses the QuantAct behind it, so power-of-two scales and scales as calibrated are covered alike.
 *  - ivit_ibert_gelu_build_lut: IBERTIntGELU (:203-235) + the 8-bit QuantAct `mlp.qact1` as a function of q, written as all
 *    256 rows of a (row max, q) table: ivit_shiftgelu_lut_i8(_ex) applies it.  (m_q, e_q) = dyadic(s_out / s_next).
 *  - ivit_ibert_softmax_build_table: exp_int after the softmax's internal 16-bit QuantAct (:303-310) as the float32 the
 *    reference sums and multiplies, for every (row max qm, q <= qm): table[(qm + 128) * 256 + q + 128], 65 536 floats.
 *  - ivit_attention_fused_i8_ibert: ivit_attention_fused_i8 with that softmax: row sum in float32 in torch's CPU reduction
 *    order, factor = floor(2^32 / sum), p = floor(fl(e * factor) / 2^25) in [0, 128] (output_bit 8, scale 2^-7).  tokens 193..207.
 *    band / band_w: the table in the band form of ivit_attention_fused_i8_compat_band (band[(qm + 128) * band_w + j] = entry of
 *    q = qm - j, entry band_w - 1 already the saturated value), staged in LDS per query tile; band_w = 0: gather from `table`.
 *  - ivit_attention_fused_i8_ibert_long: the same attention on rows of 208..1025 tokens (384 / 16 -> 577, 224 / 8 -> 785,
 *    512 / 16 -> 1025), the row organisation of ivit_attention_fused_i8_long; 8-bit probabilities only.  The row sum is torch's
 *    for these lengths: 32 interleaved partials (key % 32) over the first 32 * (tokens >> 5) keys, each summed in groups of 16 steps,
 *    the up to three 8-key vectors behind them added to partials 0..7, ((P[l] + P[l+8]) + P[l+16]) + P[l+24] for l = 0..7, and the
 *    final accumulator takes the scalar tail (tokens % 8 keys) first, then those eight sums.  table / band / band_w as above, both
 *    gathered from global memory (no LDS staging: K and V^T of the head fill it).  Errors as ivit_attention_fused_i8_long:
 *    IVIT_ERR_UNSUPPORTED ("unsupported geometry") for head_dim != 64 or tokens outside 208..1025; IVIT_ERR_INVALID for a NULL
 *    qkv / out / table ("bad operand"), misalignment, a bad band, multipliers out of range, a block-layout buffer >= 2 GiB.
 *  - ivit_ibert_layernorm_i8: IBERTIntLayerNorm (:126-153; mean and variance sums in torch's order) + the QuantAct behind it.
 *    bias_int / s_out / (m, e) as for ivit_layernorm_i8; shift_pow2 = 2^shift (the module's overflow buffer).
 *    out_blocks = 0 / 1 (row-major / IVIT_LAYOUT_BLOCKS), optionally | IVIT_IBERT_LN_INT_SQRT.  With the flag the kernel decides
 *    std from the exact integer sum V of the squares only where V < 2^24 (the float32 sum then equals V in any order); a row with
 *    V >= 2^24 is evaluated literally, its sum added in torch's order. */
int ivit_ibert_gelu_build_lut(float s, float b_int, float c_int, float shift_int, float s_out, uint32_t m_q, int32_t e_q,
                              int8_t* lut, ivit_stream_t stream);
int ivit_ibert_softmax_build_table(float s, float x0_int, float b_int, float c_int, float exp_sf, float act_sf, uint32_t m_act,
                                   int32_t e_act, float* table, ivit_stream_t stream);
int ivit_attention_fused_i8_ibert(const int8_t* qkv, int8_t* out, int batch, int heads, int tokens, int head_dim, uint32_t m_s,
                                  int32_t e_s, uint32_t m_o, int32_t e_o, const float* table, const float* band, int band_w,
                                  int out_blocks, ivit_stream_t stream);
/* softmax_bits = 16: p = floor(fl32(e * factor) / 2^17) <= 2^15 at scale 2 / 2^16 (ibert_modules.py:314-317);
 * softmax_bits = 4: p = floor(fl32(e * factor) / 2^29) in [0, 8] at scale 2 / 2^4, one byte plane (the 8 of a one-hot row included) */
int ivit_attention_fused_i8_ibert_wide(const int8_t* qkv, int8_t* out, int batch, int heads, int tokens, int head_dim, uint32_t m_s,
                                       int32_t e_s, uint32_t m_o, int32_t e_o, const float* table, const float* band, int band_w,
                                       int softmax_bits, int out_blocks, ivit_stream_t stream);
int ivit_attention_fused_i8_ibert_long(const int8_t* qkv, int8_t* out, int batch, int heads, int tokens, int head_dim,
                                       uint32_t m_s, int32_t e_s, uint32_t m_o, int32_t e_o, const float* table,
                                       const float* band, int band_w, int out_blocks, ivit_stream_t stream);
/* ---- attention maps: the probabilities P that the fused attention entries multiply with V, written to memory ----------
 * qkv: the head-major [3, batch, heads, tokens, 64] int8 of the fused entries (16-byte aligned); V is not read.
 * probs: [batch][heads][q_rows][ldp] uint8, ldp >= tokens, any alignment (rows are stored as packed dwords when probs and ldp are
 *   multiples of four, byte by byte otherwise).  Row r of an (image, head) holds the probabilities of query r over the keys
 *   0 .. tokens - 1 at scale 2^-7; bytes tokens .. ldp - 1 of a row are not written.  q_rows in 1 .. tokens: 1 = the class
 *   token's row alone, tokens = the full map; only the 16-query tiles that hold a requested row are computed.
 * Arithmetic: exactly that of the fused entries with an 8-bit softmax output.
 *  - ivit_attention_probs_u8 (Shiftmax, ivit_modules.py:150-175): scores requantised by (m_s, e_s) and clamped to int8; exp_int from
 *    the power-of-two table (exp2d = NULL, band_w = 0), the band table or the full [256][256] table as
 *    ivit_attention_fused_i8_compat_band takes them; the reference's float32 row sum (the exact integer sum below 2^24, the sum in
 *    torch's CPU reduction order from there on, as in every Shiftmax entry), factor, p = (e * factor) >> 24 in [0, 127].
 *  - ivit_attention_probs_u8_ibert (IBERTIntSoftmax, ibert_modules.py:303-314): e from the (row max, q) table of
 *    ivit_ibert_softmax_build_table or its band form; row sum in float32 in torch's CPU reduction order for ANY row length (the
 *    scalar form below 8 keys, 32 interleaved partials with the cascade above); factor = floor(2^32 / S),
 *    p = floor(fl32(e * factor) / 2^25) in [0, 128] -- 128 for a one-hot row, hence the unsigned output.
 * tokens 1 .. 1025 in both families, head_dim 64.  Errors: IVIT_ERR_UNSUPPORTED for head_dim != 64 or tokens outside 1..1025;
 * IVIT_ERR_INVALID for a NULL qkv / probs (I-BERT: table), q_rows outside 1..tokens, ldp < tokens, a misaligned qkv or table, a bad
 * band width, a score multiplier >= 2048, s_attn <= 0 or x0 outside [-4096, -1], and below 208 tokens a Shiftmax row sum that
 * could pass 32 bits (the bound of the fused short-row entries).  Nothing is written on an error. */
int ivit_attention_probs_u8(const int8_t* qkv, uint8_t* probs, int64_t ldp, int batch, int heads, int tokens,
                            int head_dim, int q_rows, uint32_t m_s, int32_t e_s, float s_attn,
                            const uint32_t* exp2d, const uint32_t* band, int band_w, ivit_stream_t stream);
int ivit_attention_probs_u8_ibert(const int8_t* qkv, uint8_t* probs, int64_t ldp, int batch, int heads, int tokens,
                                  int head_dim, int q_rows, uint32_t m_s, int32_t e_s,
                                  const float* table, const float* band, int band_w, ivit_stream_t stream);
int ivit_ibert_layernorm_i8(const int8_t* x, int64_t ldx, int rows, int C, float s_in, const float* bias_int, const float* s_out,
                            float shift_pow2, const uint32_t* m, const int32_t* e, int8_t* out, int64_t ldo, int out_blocks,
                            ivit_stream_t stream);
/* the same on an int16 row (norm2_in_bw / att_block_out_bw = 16: the 16-bit residual stream); literal form, row-major output */
int ivit_ibert_layernorm_i16_i8(const int16_t* x, int64_t ldx, int rows, int C, float s_in, const float* bias_int,
                                const float* s_out, float shift_pow2, const uint32_t* m, const int32_t* e, int8_t* out, int64_t ldo,
                                ivit_stream_t stream);
/* fast_division = 0 / 1, optionally | IVIT_IBERT_LN_INT_SQRT (the variance sum is the float32 sum in torch's order in either form).
 * fast_division = 1: the caller has checked (for all 65536 inputs at this s_in) that the three-instruction quotient by the
 * invariant s_in -- q0 = x * r, e = fma(-s, q0, x), fma(e, r, q0), r = RN(1 / s_in) -- is the correctly rounded x / s_in */
int ivit_ibert_layernorm_i16_i8_ex(const int16_t* x, int64_t ldx, int rows, int C, float s_in, const float* bias_int,
                                   const float* s_out, float shift_pow2, const uint32_t* m, const int32_t* e, int8_t* out, int64_t ldo,
                                   int fast_division, ivit_stream_t stream);
/* ivit_ibert_layernorm_i16_i8_ex with the rows of `out` in Swin's window order, as ivit_layernorm_i16_i8 stores them: row r = (b, y, x)
 * of x [rows = batch * H * W, C] is written to row win_row(r) of out -- the cyclic shift by -shift and the partition into ws x ws windows
 * of SwinTransformerBlock.forward (swin_quant.py:258-271) applied to the store address, so that norm1 of a block needs no gather behind
 * it.  ws == 0: rows in order, identical to the _ex entry (H, W, shift are not read).  The arithmetic, the kernels and the meaning of
 * every other argument are the _ex entry's; ldo may exceed C (the pad columns are not written).
 * Errors, nothing launched: a bit of fast_division other than 1 and IVIT_IBERT_LN_INT_SQRT is IVIT_ERR_INVALID; with ws != 0 a window
 * description other than H, W > 0, H % ws == 0, W % ws == 0, 0 <= shift < ws, rows % (H * W) == 0 is IVIT_ERR_UNSUPPORTED ("unsupported
 * geometry"); then as the _ex entry: IVIT_ERR_INVALID ("bad operand") for a NULL operand, ldx < C, ldo < C, s_in <= 0. */
int ivit_ibert_layernorm_i16_i8_win(const int16_t* x, int64_t ldx, int rows, int C, float s_in, const float* bias_int,
                                    const float* s_out, float shift_pow2, const uint32_t* m, const int32_t* e, int8_t* out, int64_t ldo,
                                    int fast_division, int H, int W, int ws, int shift, ivit_stream_t stream);
/* Token features with IBERTIntLayerNorm: out = fl(v * s_out[c]) (ibert_modules.py:153), the module's own float32 output, from int8 /
 * int16 rows at scale s_in -- the literal row of the entries above without their QuantAct.  Row selection (B, T_all, t0, T), output
 * forms and common preconditions: see ivit_layernorm_i8_f32.  flags = IVIT_LN_F32_CHANNEL_MAJOR | IVIT_IBERT_LN_INT_SQRT, and on the
 * int16 entry | IVIT_LN_F32_FAST_DIV (as fast_division = 1 above; on the int8 entry IVIT_ERR_INVALID).  Any C <= 4096, rows aligned
 * to their element; s_in > 0 and shift_pow2 >= 1 (IVIT_ERR_INVALID otherwise). */
int ivit_ibert_layernorm_i8_f32(const int8_t* x, int64_t ldx, int B, int T_all, int t0, int T, int C, float s_in, const float* bias_int,
                                const float* s_out, float shift_pow2, float* out, int64_t ldo, int flags, ivit_stream_t stream);
int ivit_ibert_layernorm_i16_f32(const int16_t* x, int64_t ldx, int B, int T_all, int t0, int T, int C, float s_in, const float* bias_int,
                                 const float* s_out, float shift_pow2, float* out, int64_t ldo, int flags, ivit_stream_t stream);

/* ---- evaluation transform (the reference's data pipeline in front of the model) ----------------------------------------
 * torchvision Resize([resize_short], BICUBIC) on a PIL image, then CenterCrop(crop) (scripts/inference.py:63-66,
 * utils/data_utils.py:82-91), byte for byte: Pillow's 8-bit bicubic resample (a = -0.5, 22-bit fixed-point taps, horizontal pass
 * first, uint8 between the passes), of which only the crop's pixels are computed.  DESIGN.md "Eval transform".
 *
 * ivit_eval_geometry: HOST function, host out4 = (new_h, new_w, top, left) for an h x w source: short side -> resize_short, long
 * side int(resize_short * long / short) in float64; top / left = round((new - crop) / 2), half to even.  IVIT_ERR_UNSUPPORTED
 * ("unsupported geometry") for an empty image, crop <= 32 (input sizes without a resize) or crop > the resized short side
 * (torchvision would pad); IVIT_ERR_INVALID for a NULL out4. */
int ivit_eval_geometry(int h, int w, int resize_short, int crop, int32_t* out4);
/* HOST function: geom = host int32 [batch][6] rows (h, w, new_h, new_w, top, left); plan3 (host) = (ksize_h, ksize_v, rows), the
 * largest horizontal / vertical tap count and intermediate row count of the batch; *bytes = the workspace
 * ivit_resize_crop_bicubic_u8 needs for that plan.  IVIT_ERR_UNSUPPORTED ("unsupported geometry") for a row with an empty image,
 * a crop that does not fit inside the resized image, or crop <= 32. */
int ivit_resize_crop_workspace(const int32_t* geom, int batch, int crop, int32_t* plan3, int64_t* bytes);
/* src: packed uint8 HWC RGB images, image b at src + offsets[b] (device int64 [batch]); geom: the same rows as above on the device,
 * validated by ivit_resize_crop_workspace (the kernels clamp every index to the plan, so a table that disagrees with the plan reads
 * and writes nothing outside the images, workspace and out); (ksize_h, ksize_v, rows) and workspace_bytes from
 * ivit_resize_crop_workspace.  out: uint8 [batch][3][crop][crop], planar (the engines' uint8 input).  Alignment: offsets 8,
 * geom 4, workspace 16 bytes.  IVIT_ERR_INVALID for NULL or misaligned operands, batch outside 0..65535, a plan or workspace that
 * is too small; IVIT_ERR_UNSUPPORTED for crop <= 32.  Three launches on `stream`. */
int ivit_resize_crop_bicubic_u8(const uint8_t* src, const int64_t* offsets, const int32_t* geom, int batch, int crop, int ksize_h,
                                int ksize_v, int rows, void* workspace, int64_t workspace_bytes, uint8_t* out, ivit_stream_t stream);

/* The same transform with an h x w crop, an exact-size resize and torchvision's zero padding (DESIGN.md §11 "h x w crops").  The three
 * entries above are these with crop_h = crop_w, the short-side resize and no padding, and keep their own refusals.
 *
 * The rule, per axis and independent per axis, for a resized length n and a crop length c:
 *   c <= n   offset round((n - c) / 2), half to even (as above)
 *   c >  n   CenterCrop pads (c - n) / 2 zeros in front and (c - n + 1) / 2 behind (integer division); the offset is reported as
 *            the negative number -((c - n) / 2)
 * and output pixel y is resized pixel y + offset, or 0 where that lies outside [0, n).  The zeros are pixel value 0, in front of
 * ToTensor / Normalize.
 *
 * ivit_eval_geometry_hw: HOST function, host out4 = (new_h, new_w, top, left).  resize_w == 0: torchvision Resize([resize_h]), the
 * short-side rule of ivit_eval_geometry; resize_w > 0: Resize((resize_h, resize_w)), exactly that size.  top and left can be
 * negative with pad != 0 only: with pad == 0 a crop longer than the resized image on either axis is IVIT_ERR_UNSUPPORTED
 * ("unsupported geometry"), as are an empty image, resize_h < 1, resize_w < 0 and a crop side <= 32.  IVIT_ERR_INVALID for a
 * NULL out4. */
int ivit_eval_geometry_hw(int h, int w, int resize_h, int resize_w, int crop_h, int crop_w, int pad, int32_t* out4);
/* HOST function: ivit_resize_crop_workspace for a crop_h x crop_w crop, over the same host int32 [batch][6] rows (h, w, new_h,
 * new_w, top, left).  Per axis a row is accepted with 0 <= offset <= n - c, or, where c > n, with -(c - n) <= offset <= 0;
 * everything else, an empty image or resized image, and a crop side <= 32 are IVIT_ERR_UNSUPPORTED ("unsupported geometry").
 * plan3 = (ksize_h, ksize_v, rows); rows counts the source rows that the crop's rows inside the resized image reach. */
int ivit_resize_crop_workspace_hw(const int32_t* geom, int batch, int crop_h, int crop_w, int32_t* plan3, int64_t* bytes);
/* ivit_resize_crop_bicubic_u8 for a crop_h x crop_w crop at signed offsets: out = dense planar uint8 [batch][3][crop_h][crop_w],
 * every byte of it written (out need not be cleared): the padding as 0 by the vertical pass, the pixels inside the resized image
 * from their taps.  Taps, intermediate rows and intermediate columns exist for the part of the crop inside the resized image
 * only.  geom, the plan and workspace_bytes from ivit_resize_crop_workspace_hw for the same (crop_h, crop_w); as above the kernels
 * clamp every index to the plan, so a table that disagrees with the plan reads and writes nothing outside the images, the
 * workspace and out.  Alignment and IVIT_ERR_INVALID as for the square entry, and for crop_h > 262140 (one launch);
 * IVIT_ERR_UNSUPPORTED for a crop side <= 32.  Three launches on `stream`. */
int ivit_resize_crop_bicubic_hw_u8(const uint8_t* src, const int64_t* offsets, const int32_t* geom, int batch, int crop_h, int crop_w,
                                   int ksize_h, int ksize_v, int rows, void* workspace, int64_t workspace_bytes, uint8_t* out,
                                   ivit_stream_t stream);

/* ---- JPEG decoding (the reference's image loader, Image.open(f).convert("RGB")) -------------------------------------------
 * Baseline JPEG byte for byte as libjpeg-turbo decodes it at its defaults (JDCT_ISLOW, fancy upsampling): sequential Huffman
 * (SOF0 / SOF1), 8-bit samples, one scan of all components, restart intervals, 1 component (replicated to RGB) or 3 components
 * libjpeg-turbo takes as YCbCr with sampling 4:4:4, 4:2:2 or 4:2:0.  DESIGN.md §11 "JPEG decoding".  The first four functions
 * are HOST functions that make no HIP runtime call (loader worker processes may call them).
 *
 * ivit_jpeg_probe: info4 (host) = (h, w, components, sampling: 0 gray, 1 4:4:4, 2 4:2:2, 3 4:2:0; -1 when unsupported).
 * IVIT_ERR_UNSUPPORTED for every other file, ivit_last_error_string() the reason (progressive, CMYK, truncated, ...). */
int ivit_jpeg_probe(const uint8_t* data, int64_t nbytes, int32_t* info4);
/* One image's plan section (16-byte aligned, relocatable): quantisation tables in natural order, derived Huffman tables,
 * component geometry, restart segments, the de-stuffed entropy bytes.  section == NULL: *section_bytes only.  The errors of
 * ivit_jpeg_probe; IVIT_ERR_INVALID for a capacity below *section_bytes. */
int ivit_jpeg_plan_image(const uint8_t* data, int64_t nbytes, uint8_t* section, int64_t capacity, int64_t* section_bytes);
/* Batch index over a plan (host buffer of plan_bytes holding sections): sec_offsets[b] = section of image b, -1 for an image not
 * decoded on the device; out_offsets[b] = its HWC offset in the output.  index (host, 40 bytes per image) is the operand of
 * ivit_jpeg_decode_u8 once copied to the device; sizes4 (host) = (workspace bytes, subsequences, blocks, largest pixel count). */
int ivit_jpeg_workspace(const uint8_t* plan, int64_t plan_bytes, const int64_t* sec_offsets, const int64_t* out_offsets, int batch,
                        void* index, int64_t* sizes4);
/* Decodes one image serially with the device's primitives into out (host, h x w x 3).  IVIT_ERR_UNSUPPORTED as the probe;
 * IVIT_ERR_INVALID for corrupt entropy data (a code no table holds, a segment that ends early) or a short output. */
int ivit_jpeg_decode_host(const uint8_t* data, int64_t nbytes, uint8_t* out, int64_t out_bytes);
/* Device decode of a batch: plan (the host plan's bytes, copied), index (ivit_jpeg_workspace's, copied), (nsub, nblocks,
 * max_pixels) = sizes4[1..3], workspace of sizes4[0] bytes; writes HWC uint8 at out + out_offsets[b] for every device image and
 * errors[b] (device int32 [batch]) = 0, or non-zero for corrupt entropy data.  Alignment: plan 16, index 8, workspace 256, errors 4
 * bytes.  Seven launches and two memsets on `stream`. */
int ivit_jpeg_decode_u8(const uint8_t* plan, const void* index, int batch, int64_t nsub, int64_t nblocks, int64_t max_pixels,
                        void* workspace, int64_t workspace_bytes, uint8_t* out, int32_t* errors, ivit_stream_t stream);

/* ---- feature maps: a token-major integer stream as dense channel-major maps (forward_intermediates) -----------------------
 * x: the residual stream of an engine, rows of ldx >= C elements: element (b, t, c) of the selection is
 *   x[(b * T_all + t0 + t) * ldx + c], 0 <= t < T, t0 + T <= T_all (t0 = 1 drops the class token of a ViT).  Rows outside the
 *   selection and elements C .. ldx - 1 of a row are not read.
 * out: dense [B][C][T], out[(b * C + c) * T + t] -- NCHW once T is viewed as H x W.
 *  - ivit_tokens_to_nchw_i8_f32 / _i16_f32: out = (float)q * s, ONE float32 multiplication (torch's q.float() * s bit for bit: the
 *    tensor a QuantAct of the reference returns, quant_act_int * act_scaling_factor).
 *  - ivit_tokens_to_nchw_i8 / _i16: out = q, the integers themselves.
 * Any T >= 1 and C >= 1.  x is read with 16-, 8- or 4-byte loads when x and ldx * sizeof(element) are multiples of that size,
 * element by element otherwise (and for the piece of a row that crosses channel C); every offset is 64-bit.  One launch.
 * Errors: IVIT_ERR_INVALID for a NULL x or out, B, T or C below 1, t0 < 0, t0 + T > T_all, ldx < C, x or out not aligned to its
 * element, or more than 2^31 - 1 tiles of 64 tokens x 128 source bytes.  Nothing is launched on an error. */
int ivit_tokens_to_nchw_i8_f32(const int8_t* x, int64_t ldx, int B, int T_all, int t0, int T, int C, float s, float* out,
                               ivit_stream_t stream);
int ivit_tokens_to_nchw_i16_f32(const int16_t* x, int64_t ldx, int B, int T_all, int t0, int T, int C, float s, float* out,
                                ivit_stream_t stream);
int ivit_tokens_to_nchw_i8(const int8_t* x, int64_t ldx, int B, int T_all, int t0, int T, int C, int8_t* out, ivit_stream_t stream);
int ivit_tokens_to_nchw_i16(const int16_t* x, int64_t ldx, int B, int T_all, int t0, int T, int C, int16_t* out, ivit_stream_t stream);

/* ---- backbone outputs: int8 rows as float32 rows (forward_features) ---------------------------------------------------------
 * out[r * ldo + c] = (float)x[r * ldx + c] * s for 0 <= r < rows, 0 <= c < C: ONE float32 multiplication, the arithmetic of
 * ivit_tokens_to_nchw_i8_f32 (the reference's quant_act_int * act_scaling_factor bit for bit).  Rows are strided on both sides
 * (ldx >= C, ldo >= C, in elements): out may be a block of rows and columns of a larger feature bank.  Elements C .. ldx - 1 of an
 * input row are not read, elements C .. ldo - 1 of an output row are not written, nor is anything outside the rows.
 * The far dimension is `rows`: r * ldx and r * ldo are 64-bit products, so a row may start beyond 2^31 bytes of x and beyond 2^32
 * bytes of out; one row (C) stays an int.
 * x and ldx may have any alignment, out that of a float.  Per row: where the input row and the output row reach a 16-byte
 * boundary at the same channel, 16 int8 are one load and four float4 stores, with a scalar head and tail; any other row goes
 * element by element.  One launch; rows == 0 is IVIT_OK without one.
 * Errors: IVIT_ERR_INVALID for a NULL x or out, C < 1, rows < 0, ldx < C, ldo < C, out not aligned to a float, or more than
 * 2^31 - 1 workgroups of 256 slots (a row has C / 16 + 2 slots).  Nothing is launched on an error. */
int ivit_dequant_rows_i8_f32(const int8_t* x, int64_t ldx, int64_t rows, int C, float s, float* out, int64_t ldo, ivit_stream_t stream);

/* ---- k-NN evaluation on an int8 feature bank: cosine neighbours, exact and unique ---------------------------------------------
 * Bank rows b_j and query rows q_i are int8 rows of C channels under one per-tensor scale each (the scales cancel in a cosine).
 *   n2_j     = sum_c b_jc^2 (integer)
 *   rnorm_j  = 1.0f / sqrtf((float)n2_j), sqrt and division correctly rounded (no rsqrt form); 0.0f where n2_j == 0
 *   score_ij = fl32((float)dot_ij * rnorm_j), dot_ij the exact int32 dot product: ONE float32 multiplication.  With C <= 1024
 *              both |dot| and n2 are at most 2^24 and convert exactly.
 * The neighbours of query i are the k bank rows with the largest score_ij, score descending, equal scores (float comparison,
 * -0 == +0) by ascending bank index -- the rule of ivit_head_topk.  The order is total, so the result is unique whatever the
 * tiling or the number of bank segments, and the neighbours for a smaller k are a prefix.  The cosine is
 * fl32(score_ij * rnorm(q_i)), one more float32 product, left to the caller.
 *
 * ivit_rows_rnorm_i8_f32: out[r] = rnorm of row r of x (rows x C, row stride ldx >= C in elements), 1 <= C <= 65536.  The far
 * dimension is `rows`: r * ldx is a 64-bit product, a row may start beyond 2^32 bytes of x.  x and ldx may have any alignment (rows
 * on a 16-byte boundary are read 16 bytes at a time), out that of a float; elements C .. ldx - 1 of a row are not read.  One launch,
 * rows == 0 is IVIT_OK without one.  Errors: IVIT_ERR_INVALID for a NULL pointer, C outside [1, 65536], rows < 0, ldx < C, a
 * misaligned out; nothing is launched.
 *
 * ivit_knn_topk_i8: idx[i * k + n] / score[i * k + n] = bank index and score_ij of the n-th neighbour of query i, 0 <= i < Q.
 * q is Q x C with row stride ldq, bank N x C with row stride ldb, rnorm [N] as ivit_rows_rnorm_i8_f32 writes it.  Geometry:
 * C % 64 == 0, 64 <= C <= 1024, 1 <= k <= IVIT_KNN_K_MAX, k <= N < 2^31, Q >= 0 (Q == 0: IVIT_OK, nothing launched).  q, bank, ldq
 * and ldb are multiples of 16 bytes; row offsets are 64-bit products on q, bank, idx and score.  Elements C .. ld - 1 of a row are
 * not read.  splits: the bank is cut into that many segments of ceil(N / splits) rows rounded up to 64, searched by separate
 * workgroups and merged by a second launch -- 1 .. IVIT_KNN_SPLITS_MAX as given (a segment may hold fewer than k rows, or none),
 * 0 = chosen from Q and N for the 256 CUs the other launchers assume.  workspace: ivit_knn_workspace_bytes(Q, N, k, splits)
 * bytes aligned to 8 (0 bytes with one segment: workspace may then be NULL).  The [Q][N] scores never reach memory.
 * Errors, nothing launched and nothing written: IVIT_ERR_INVALID for a NULL operand, Q < 0, N < 1, k < 1, k > N, splits outside
 * [0, IVIT_KNN_SPLITS_MAX], ldq or ldb below C, a misaligned pointer or leading dimension, a workspace that is NULL, misaligned or
 * too small; IVIT_ERR_UNSUPPORTED ("unsupported geometry") for k > IVIT_KNN_K_MAX and for any other C.
 *
 * ivit_knn_workspace_bytes: a host function; *bytes for that call (the same checks of Q, N, k and splits).
 *
 * ivit_knn_vote_f32: the weighted vote of a query's neighbours.  idx [Q][k] (as above), labels [N] int32, w [Q][k] float32.  The
 * vote of a label is the float32 sum of the w of the neighbours that carry it, added in rank order starting from 0.0f; classes /
 * votes [Q][r], 1 <= r <= k <= IVIT_KNN_K_MAX: the r labels with the largest vote, vote descending, equal votes by ascending
 * label; with fewer than r distinct labels the rest is (-1, 0.0f).  Computed among the query's own k neighbours: no per-class
 * table (any number of classes), no atomics (deterministic).  An index outside [0, N) is NOT checked on the device: idx must be
 * what ivit_knn_topk_i8 wrote for a bank of N rows.  Errors: IVIT_ERR_INVALID for a NULL or misaligned pointer, Q < 0, N < 1, k
 * outside [1, IVIT_KNN_K_MAX], r outside [1, k]. */
#define IVIT_KNN_K_MAX 256
#define IVIT_KNN_SPLITS_MAX 64
int ivit_rows_rnorm_i8_f32(const int8_t* x, int64_t ldx, int64_t rows, int C, float* out, ivit_stream_t stream);
int ivit_knn_topk_i8(const int8_t* q, int64_t ldq, int Q, const int8_t* bank, int64_t ldb, int N, int C, const float* rnorm, int k,
                     int splits, int32_t* idx, float* score, void* workspace, int64_t workspace_bytes, ivit_stream_t stream);
int ivit_knn_workspace_bytes(int Q, int N, int k, int splits, int64_t* bytes);
int ivit_knn_vote_f32(const int32_t* idx, const int32_t* labels, const float* w, int Q, int N, int k, int r, int32_t* classes,
                      float* votes, ivit_stream_t stream);

/* ---- linear probe on an int8 feature bank: the exact integer statistics of a closed-form classifier ---------------------------
 * Everything least squares onto one-hot targets (or a class-mean classifier) needs from a bank x of `rows` int8 rows of C channels
 * (row stride ldx >= C in elements) is a sum of integers: the Gram matrix, the per-class row sums and the class counts.  They are
 * computed exactly, so they are unique for any tiling and additive over batches and ranks (accumulate = 1).  Geometry of both
 * entries, that of ivit_knn_topk_i8: C % 64 == 0, 64 <= C <= 1024, 0 <= rows < 2^31, x and ldx multiples of 16 bytes; row offsets
 * are 64-bit products; elements C .. ldx - 1 of a row are not read.  No float anywhere, no atomics on a result.
 *
 * ivit_gram_i8_i64: gram[i * C + j] = sum_r x[r][i] * x[r][j], the exact integer, for all 0 <= i, j < C (dense [C][C] int64, both
 * triangles written; the blocks on or above the diagonal are computed on v_mfma_i32_16x16x64_i8 and mirrored).  accumulate: 0
 * overwrites, 1 adds to the int64 values already there.  rows == 0 is a sum over nothing: zeros with accumulate = 0, no change
 * (and no launch) with 1.  splits: the rows are cut into that many segments of ceil(rows / splits) rows rounded up to 64 -- 1 ..
 * IVIT_GRAM_SPLITS_MAX as given (a segment may be short or empty), 0 = chosen from rows and C for the 256 CUs the other launchers
 * assume.  Every segment leaves int32 partial Grams in the workspace -- one per 65536 rows, over which no int32 sum of products of
 * int8 can overflow (65536 * 2^14 = 2^30), so a longer segment widens inside itself -- and a second kernel sums the partials into
 * int64.  The result does not depend on splits.  workspace: ivit_gram_workspace_bytes(rows, C, splits) bytes aligned to 4 (0
 * bytes for rows == 0: workspace may then be NULL).
 * Errors, nothing launched and nothing written: IVIT_ERR_INVALID for a NULL x or gram, rows outside [0, 2^31), splits outside
 * [0, IVIT_GRAM_SPLITS_MAX], accumulate other than 0 or 1, ldx < C, a misaligned x, ldx or gram, a workspace that is NULL,
 * misaligned or too small; IVIT_ERR_UNSUPPORTED ("unsupported geometry") for any other C.
 *
 * ivit_gram_workspace_bytes: a host function; *bytes for that call (the same checks of rows, C and splits).
 *
 * ivit_group_sums_i8_i64: sums[g * C + c] = sum over t in [group_ptr[g], group_ptr[g + 1]) of x[perm[t]][c], exact, for
 * 0 <= g < groups (int64 [groups][C]; added to the values already there with accumulate = 1).  perm int32 [group_ptr[groups]]: row
 * indices grouped by class; group_ptr int64 [groups + 1], non-decreasing from 0 -- the CSR form of the labels, which the caller
 * builds from a stable sort of them.  An empty group gives zeros.  1 <= groups <= IVIT_GROUPS_MAX.  The inverted-index form of a
 * scatter-add: one workgroup per group, every row read once, 16 bytes per lane.  An entry of perm outside [0, rows) is NOT checked
 * on the device.  One launch.  Errors, nothing launched: IVIT_ERR_INVALID for a NULL or misaligned operand, rows outside [0, 2^31),
 * ldx < C, groups outside [1, IVIT_GROUPS_MAX], accumulate other than 0 or 1; IVIT_ERR_UNSUPPORTED for any other C. */
#define IVIT_GRAM_SPLITS_MAX 64
#define IVIT_GROUPS_MAX 1048576
int ivit_gram_i8_i64(const int8_t* x, int64_t ldx, int64_t rows, int C, int splits, int accumulate, int64_t* gram, void* workspace,
                     int64_t workspace_bytes, ivit_stream_t stream);
int ivit_gram_workspace_bytes(int64_t rows, int C, int splits, int64_t* bytes);
int ivit_group_sums_i8_i64(const int8_t* x, int64_t ldx, int64_t rows, int C, const int32_t* perm, const int64_t* group_ptr, int groups,
                           int accumulate, int64_t* sums, ivit_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* IVIT_HIP_H */
