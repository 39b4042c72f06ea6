/*
 * ivit_hip_debug.h -- test and measurement hooks of libivit_hip_lab.so (csrc built with IVIT_LAB = 1).  NOT part of the
 * drop-in boundary (include/ivit_hip.h) and not in libivit_hip.so: process-wide, not thread-safe, for tests/ and scripts/ only.
 *
 * Three kinds of hook, nothing else:
 *   form selector   forces a kernel form that the product library itself launches for some other shape or scale, so that tests
 *                   pin every product form on the same inputs.  Results stay correct.
 *   instrument      time stamps, or "skip this phase" timing ablations, of a kernel the product ships.  Ablations make the
 *                   results WRONG; they exist to be timed.
 *   probe           runs one device function of a product kernel on the caller's array, for inputs no row of activations can be
 *                   made to produce on demand.  No state.
 * Forms that were tried and lost are not kept here: profiles/HISTORY.md and the git history are their record.
 * Every bit of every word has one meaning and one reader; bits not listed are ignored.  0 restores the product's behaviour.
 */
#ifndef IVIT_HIP_DEBUG_H
#define IVIT_HIP_DEBUG_H

#ifdef __cplusplus
extern "C" {
#endif

/* ivit_gemm_i8_* (csrc/gemm.hip)
 *   value | meaning                                                                 | results | used by
 *   ------+-------------------------------------------------------------------------+---------+--------------------------------
 *   0     | automatic: the persistent 256 x 128 LDS-DMA kernel for M >= 2048,       | correct |
 *         | N >= 128, the 128 x 128 register-staged kernel otherwise                |         |
 *   != 0  | always the 128 x 128 kernel (selector; also keeps the skinny-K form off) | correct | tests/test_gpu_ops.py,
 *         |                                                                         |         | scripts/gemm_ab.py */
int ivit_debug_force_small_gemm(int on);

/* ivit_gemm_i8_* (csrc/gemm.hip), first flag word
 * (csrc/gemm_common.h names the bits for their reader, gemm_plan: LAB_WR_ABLATION bits 0-4, LAB_WR_STAMPS 4, LAB_NO_STAGGER 6,
 * LAB_SPLIT_ALL_SLOTS 11, LAB_ONE_PER_CU 12, LAB_CU_TURNS 15, LAB_DELAY_SHIFT / LAB_DELAY_MASK 16-21, LAB_GRID_256 26, LAB_NO_HALVES 27)
 *   bits      | meaning                                                              | results | used by
 *   ----------+----------------------------------------------------------------------+---------+-----------------------------
 *   0-3       | weights-in-registers kernel, 32x32x32 form, ivit_gemm_i8_requant_ex: | WRONG   | scripts/gemm_ab.py --frags,
 *             | timing ablations 1 no epilogue, 2 no weight loads in the loop, 4 no  |         | scripts/gemm_ablate.py
 *             | DMA in the loop, 8 no MFMA; the sums 6, 7, 14, 15 exist too          |         |
 *   4 (16)    | the same kernel writes its stamps: 32 x uint64 per                   | WRONG   | scripts/wreg_timeline.py
 *             | (workgroup, tile < 4) into the stamp buffer; alone in bits 0-4       |         |
 *   6 (64)    | persistent kernel: no start stagger of the co-resident workgroups    | correct | scripts/gemm_ab.py
 *   11 (2048) | both large kernels: split a sparse last round into half tiles up to  | correct | tests/test_gpu_ops.py,
 *             | 2R <= all workgroup slots (the product stops at 2R <= 256)           |         | scripts/gemm_ab.py
 *   12 (4096) | persistent kernel: one workgroup per CU (with bit 4: the stamped     | correct | tests/test_gpu_ops.py,
 *             | kernel likewise)                                                     |         | scripts/wreg_timeline.py,
 *             |                                                                      |         | scripts/gemm_one.py
 *   15 (32768)| persistent kernel: co-resident workgroups take turns in their main   | correct | scripts/gemm_ab.py
 *             | loops through a per-CU token                                         |         |
 *   16-21     | persistent kernel: start delay of the second co-resident workgroup,  | correct | scripts/gemm_ab.py
 *             | in ~1K-cycle units                                                   |         |
 *   26        | persistent kernel: a 256-workgroup grid without the LDS blocker      | correct | scripts/dual_stream_probe.py
 *   27        | both large kernels: no half tiles at all                             | correct | scripts/gemm_ab.py */
int ivit_debug_set_gemm_flags(int flags);

/* ivit_gemm_i8_* (csrc/gemm.hip), second flag word
 * (csrc/gemm_common.h: LAB2_WR16_STAMPS 8, LAB2_WR16_NARROW 13, LAB2_NO_SKINNY 20, LAB2_SKINNY_ANY_K 21)
 *   bits      | meaning                                                              | results | used by
 *   ----------+----------------------------------------------------------------------+---------+-----------------------------
 *   8 (256)   | weights-in-registers kernel, 16x16x64 form, plain and residual       | correct | scripts/wreg_timeline.py
 *             | epilogue: the stamped instantiation, if a stamp buffer is set (stamps|         | --s16
 *             | kept in registers until the tile ends: the timing is the product's)  |         |
 *   13 (8192) | the same kernel: narrow 128 x 128 work items.  The product compiles  | correct | tests/test_gpu_ops.py,
 *             | this arm into its kernels (a run-time branch) and launches it for no |         | scripts/gemm_narrow_ab.py
 *             | shape: measured slower (x 1.08 - 1.44, profiles/HISTORY.md)          |         |
 *   20        | no skinny-K form (K <= 128, N <= 320, M >= 8192): the tile kernels   | correct | tests/test_gpu_ops.py,
 *             | the product uses for every other shape (selector)                    |         | scripts/gemm_ab.py
 *   21        | the skinny-K form's run-time-K instantiation also for K = 64 / 128   | correct | tests/test_gpu_ops.py
 *             | (the product uses it for every other K; selector)                    |         | */
int ivit_debug_set_gemm_flags2(int flags);

/* Device buffer for the stamped weights-in-registers kernels (flags bit 4, flags2 bit 8): 32 x uint64 per (workgroup,
 * tile < 4) -- tile start, loop start, loop end, epilogue end, K-step starts / epilogue phases, s_memrealtime at [16].
 * NULL = off.  scripts/wreg_timeline.py */
int ivit_debug_set_stamp_buffer(void* buf);

/* ivit_layernorm_i8(_ex, _compat) kernel form (csrc/rowops.hip); every value is a selector, results correct
 *   value | meaning                                                                            | used by
 *   ------+------------------------------------------------------------------------------------+-----------------------------
 *   0     | automatic: the streaming kernel of ln_stream.h for C = 192 / 384 / 512 / 768 / 1024 |
 *         | from ~12 MB of rows, else half a wave per row for C <= 384, the grouped kernel up   |
 *         | to 1024, a wave per row above                                                       |
 *   1     | always a wave per row                                                              | tests/test_gpu_ops.py,
 *   2     | half a wave per row wherever it exists (C <= 1536)                                 | tests/test_gpu_compat.py,
 *   3     | the automatic choice without the streaming kernel                                  | scripts/ln_ab.py,
 *   4     | the streaming kernel wherever it applies, whatever the size                        | scripts/ln_ablate.py */
int ivit_debug_ln_wave_per_row(int on);

/* streaming LayerNorm kernel (csrc/ln_stream.h), A/B timing; results correct
 *   bits | meaning                                                                   | used by
 *   -----+---------------------------------------------------------------------------+----------------------------------------
 *   0-3  | C = 768 only: ring depth / occupancy variant (1, 3-7; 0 = the product's)  | scripts/ln_ab.py, scripts/ln_one.py,
 *   4-7  | workgroups per CU the grid and the LDS request are sized for (0 = 4)      | scripts/ln_timeline.py */
int ivit_debug_ln_stream_cfg(int cfg);

/* wave timeline of the streaming LayerNorm kernel: 8 x uint64 per wave (s_memrealtime, 100 MHz: entry, table ready, slots 0-2 of
 * the first round computed, -, all stores done, groups of the wave); NULL = off; scripts/ln_timeline.py */
int ivit_debug_ln_stamp_buffer(void* buf);

/* row operators (csrc/rowops.hip, csrc/ln_stream.h) and Swin kernels (csrc/swin.hip)
 *   bits   | reader     | meaning                                                       | results | used by
 *   -------+------------+---------------------------------------------------------------+---------+--------------------------
 *   0-3    | rowops.hip,| int8 LayerNorm, grouped and streaming kernels: timing         | WRONG   | scripts/ln_ablate.py,
 *          | ln_stream.h| ablations 1 no element chain, 2 no row statistics, 4 no       |         | scripts/ln_timeline.py
 *          |            | stores, 8 no per-workgroup table build (grouped kernel only)  |         |
 *   4-5    | rowops.hip | grouped int8 LayerNorm: 1 groups of 8 rows on an              | correct | scripts/ln_ablate.py,
 *          |            | oversubscribed grid, 2 groups of 16 rows on one resident set  |         | scripts/ln_ab.py
 *          |            | (the product picks by row count; selector)                    |         |
 *   16-19  | swin.hip   | workgroup cap of the tiled 16-bit LayerNorm, x 256 (0 = 1024) | correct | scripts/probes/ln16_cap.py
 *   20     | swin.hip   | natural-scale 16-bit LayerNorm: row sums through LDS also     | correct | tests/test_gpu_swin.py,
 *          |            | where the register form applies (selector)                    |         | scripts/time_swin_kernels.py
 *   21-22  | rowops.hip | half-wave int8 LayerNorm: 1 / 2 / 3 = 4 / 2 / 1 row pairs per | correct | scripts/ln_ab.py --small
 *          |            | wave whatever the row count (selector)                        |         |
 *   23     | swin.hip   | window attention: scores requantised in float64 also where    | correct | tests/test_gpu_swin.py,
 *          |            | the float32 form is exact (selector)                          |         | scripts/time_swin_kernels.py
 *   24     | rowops.hip | ShiftGELU table pass: a whole wave per row also for rows of   | correct | tests/test_gpu_ops.py
 *          |            | at most 384 bytes (selector)                                  |         |
 *   26     | rowops.hip | one-dword half-wave LayerNorm (C <= 128): 4 row pairs per     | correct | scripts/ln_ab.py --small
 *          |            | wave also from 64 K rows (selector)                           |         |
 * No attention kernel reads this word: see ivit_debug_attention. */
int ivit_debug_ln_ablate(int bits);

/* ivit_attention_fused_i8* for at most 208 tokens (csrc/attention.hip)
 *   bits  | meaning                                                                      | results | used by
 *   ------+------------------------------------------------------------------------------+---------+--------------------------
 *   0-4   | phase ablations of attention_kernel<0>: 1 no score requantisation, 2 no      | WRONG   | scripts/attn_ablate.py
 *         | table lookups, 4 no probability products, 8 no P.V and output, 16 one query  |         |
 *         | tile per wave                                                                |         |
 *   5     | no float32 score requantisation where the multiplier is a power of two: the  | correct | scripts/attn_ablate.py
 *         | general form instead (selector)                                              |         |
 *   8-10  | forced number of workgroups per (image, head), 1-7 (0 = the model's choice;  | correct | scripts/attn_parts.py,
 *         | selector)                                                                    |         | */
int ivit_debug_attention(int bits);

/* ivit_window_attention_i8* and ivit_window_attention_probs_u8* (csrc/swin.hip, csrc/swin_probs.hip, csrc/win_attn_host.h): dry run.
 * on != 0: the eight entries check their arguments and choose their softmax form and kernel as ever, then return IVIT_OK in front of
 * the launch (nothing reaches the device, no operand is read) and leave the plan of that launch for ivit_debug_window_attention_last_plan:
 *   out[0..3]   SM (0 table of distances, 1 literal, 2 band rows, 3 I-BERT), RQ32, long rows (NKT 9), ORD -- the slot of the kernel
 *               table; the probability entries have SM only (the other three 0)
 *   out[4..6]   grid (workgroups), dynamic LDS bytes, kp (the key stride of the bias / region rows)
 *   out[7..10]  x0, ksat, the effective mask_value (0 for SM 1 - 3, which do not read it), band_w as the kernel receives them
 *   out[11]     the tables the kernel receives: 1 band, 2 the one-row band, 4 phi / phim, 8 the I-BERT table
 *   out[12..13] omap.ws, omap_inv (0 0: window order)
 *   out[14]     probabilities: packed dword stores
 *   out[15]     family: 0 short, 1 long, 2 I-BERT, 3 Shiftmax probabilities, 4 I-BERT probabilities
 * A rejected call leaves the last plan as it was.  tests/test_window_attention_plan_cpu.py */
int ivit_debug_window_attention_dry_run(int on);
int ivit_debug_window_attention_last_plan(int32_t out[16]);

/* probe: out[i] = integer_sqrt(n[i]) for i < count, the device function every I-BERT LayerNorm kernel calls under
 * IVIT_IBERT_LN_INT_SQRT (csrc/isqrt.h; ibert_modules.py:85-109 -- four float32 Newton steps from 2^ceil(bits / 2), bits from the
 * float32 log2).  n: device float32 (the row sum var_int), out: device int32.  tests/test_gpu_ibert_intsqrt.py runs it over
 * tests/golden/ibert_intsqrt_kat.npz: the values next to the powers of two where log2 rounds up and the two-cycle values k^2 - 1. */
int ivit_debug_ibert_integer_sqrt(const float* n, int64_t count, int32_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IVIT_HIP_DEBUG_H */
