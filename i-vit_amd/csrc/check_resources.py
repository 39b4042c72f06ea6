#!/usr/bin/env python3
"""Build-time guard for the inline-asm GEMM kernels (csrc/Makefile runs it on the remarks of
`hipcc -Rpass-analysis=kernel-resource-usage`).

gemm_i8_wreg_kernel / gemm_i8_pers_kernel issue global loads, LDS-DMA and ds_reads through inline asm and tie each
destination register to its consumer only by a later asm `s_waitcnt` with "+v" operands.  That is sound only while the
register allocator never spills or copies those registers between the issue and the wait, i.e. while the kernel fits its
register budget: no scratch, no VGPR spills, at most 256 VGPRs (two workgroups of four waves per CU).  A toolchain or flag
change that breaks the budget must fail the build here, on the CPU, not on the GPU.

"No spill" is a NECESSARY condition, not a sufficient one: the compiler may still copy such a register between the load and the
wait without spilling.  csrc/check_isa.py checks the emitted instruction stream for exactly that; the bit-exact GEMM tests on the
GPU remain the proof of the result.

Second use (`check_resources.py <remarks> attention|rowops|swin|calib|features|knn|probe`): the occupancy the launchers of those files assume
when they size their grids (occupancy_rules below)."""
import re
import sys

GUARDED = ("gemm_i8_wreg_kernel", "gemm_i8_pers_kernel")
FIELDS = {"VGPRs": r"\bVGPRs: (\d+)", "AGPRs": r"AGPRs: (\d+)", "Scratch": r"ScratchSize \[bytes/lane\]: (\d+)",
          "Occupancy": r"Occupancy \[waves/SIMD\]: (\d+)", "VGPRSpill": r"VGPRs Spill: (\d+)", "SGPRSpill": r"SGPRs Spill: (\d+)",
          "LDS": r"LDS Size \[bytes/block\]: (\d+)"}


def parse(text):
    kernels, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        if cur is None:
            continue
        for k, pat in FIELDS.items():
            m = re.search(pat, line)
            if m and k not in cur:
                cur[k] = int(m.group(1))
    return kernels


def twin_of(name):
    """the 8-bit instantiation a 4-bit one was made from, by its mangled name, or None: the width flags 0x100 / 0x200 on the first
    template argument of the GEMM kernels (gemm_common.h EPI_NARROW_*), PB = 4 of attention_kernel<MODE, PB, ..> and
    attention_long_kernel<.., PB>"""
    m = re.search(r"(gemm_i8_\w*kernelILi)(\d+)E", name)
    if m and int(m.group(2)) >= 256:
        return name.replace(m.group(0), m.group(1) + str(int(m.group(2)) & 255) + "E")
    m = re.search(r"(?:embed|residual_requant)_kernelI(Lin8ELi7E)", name)      # rowops.hip: <LO, HI> = <-8, 7> against <-128, 127>
    if m:
        return name[:m.start(1)] + "Lin128ELi127E" + name[m.end(1):]
    m = re.search(r"attention_kernelILi\d+E(Li4E)", name)
    if m:
        return name[:m.start(1)] + "Li8E" + name[m.end(1):]
    m = re.search(r"attention_long_kernelILi\d+ELb[01]ELi\d+ELi\d+E(Li4E)", name)
    if m:
        return name[:m.start(1)] + "Li8E" + name[m.end(1):]
    return None


def narrow_rule(kernels, name):
    """a narrow form differs from its twin in constants only: it may not need more registers or any more scratch.  -> error text or None"""
    twin = twin_of(name)
    if twin is None:
        return None
    if twin not in kernels:
        return f"no 8-bit twin {twin}"
    r, t = kernels[name], kernels[twin]
    regs, tregs = r.get("VGPRs", 0) + r.get("AGPRs", 0), t.get("VGPRs", 0) + t.get("AGPRs", 0)
    if regs > tregs or r.get("Scratch", 0) > t.get("Scratch", 0):
        return f"VGPR+AGPR {regs}, scratch {r.get('Scratch')} against {tregs}, {t.get('Scratch')} of its 8-bit twin"
    return None


def occupancy_rules(path, what):
    """attention.hip / rowops.hip: kernels whose launchers size their grids for a number of resident workgroups.  The number is a
    template argument (the OCC of attention_kernel<MODE, PB, OCC, ...>, the last argument of layernorm_i8_stream_kernel<LPR, NC, NG,
    COMPAT, OCC>) or follows from them (the other int8 LayerNorm kernels): the compiler must reach it (waves per SIMD) and, for the
    variants on the headline path, without scratch."""
    kernels = parse(open(path, errors="replace").read())
    bad, seen = [], 0
    for name, r in sorted(kernels.items()):
        if "ln_tokens_f32_kernel" in name:
            # ln_tokens_f32_kernel<ROW> (ln_tokens.h; rowops.hip: int8 rows, swin.hip: int16 rows): every loop runs over the channel
            # count and nothing is indexed at run time, so no form keeps anything in scratch at any C; three workgroups of four
            # waves fit a CU beside their 48 KB token tiles at C = 768 (its launcher assumes no number of resident workgroups)
            occ, need_no_scratch = 3, True
        elif what == "attention" and "attention_long_kernel" in name:
            # attention_long_kernel<MODE, RQ32, NKT, NTH, PB>: one workgroup of NTH threads per CU (the launcher's 256 slots), i.e.
            # NTH / 256 waves per SIMD; the packed score rows must stay in registers: no scratch.  PB = 16 (the three probability
            # planes): 768 threads up to 40 key tiles, 512 above
            m = re.search(r"attention_long_kernelILi(\d+)ELb([01])ELi(\d+)ELi(\d+)ELi(4|8|16)E", name)
            occ, need_no_scratch = int(m.group(4)) // 256, True
        elif what == "attention" and "attention_cls_kernel" in name:
            # attention_cls_kernel<MODE>: CLS_OCC = 3 workgroups of four waves per CU (its __launch_bounds__; DeiT-B at batch 256
            # is then one round); the 26 K / V chunks a lane requests up front must stay in registers: no scratch
            occ, need_no_scratch = 3, True
        elif what == "attention" and "attention_probs_kernel" in name:
            # attention_probs_kernel<MODE>: rows live in LDS and every loop runs over the token count, so nothing may be indexed
            # dynamically in registers: no scratch.  Its launcher assumes no number of resident workgroups
            occ, need_no_scratch = 1, True
        elif what == "attention":
            m = re.search(r"attention_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb([01])E", name)
            if not m:
                continue
            # scratch-free: the forms of 193-208 tokens (14 x 14 patches + cls: every BASELINE config); the general-T forms
            # (other geometries, "not tuned") may keep a few dwords of the Q prefetch in scratch
            occ, need_no_scratch = int(m.group(3)), m.group(4) == "0"
        elif what == "calib":
            # weight_quant_rows_kernel<VEC, KEEP>: one wave per row, four per workgroup; KEEP holds up to 64 dwords of the row per lane
            # between its two passes, with constant indices only: no scratch in any form
            if "weight_quant_rows_kernel" not in name and "bias_quant_kernel" not in name:
                continue
            occ, need_no_scratch = 1, True
        elif what == "features":
            # tokens_to_nchw_kernel<TI, TO, VB>: up to 32 loaded pieces per thread are indexed by constants only: no scratch; four
            # workgroups of four waves per CU fit beside their LDS tiles (the launcher assumes no more than that they are resident together)
            if "tokens_to_nchw_kernel" not in name:
                continue
            occ, need_no_scratch = 4, True
        elif what == "knn":
            # knn_topk_kernel<KSMAX>: two workgroups of four waves per CU (its __launch_bounds__, beside 2 x 76.5 KiB of LDS); the query
            # and bank fragments (up to 192 VGPRs) are indexed by constants only: no scratch.  The merge, rnorm and vote kernels
            # assume no number of resident workgroups and keep nothing indexed in registers: no scratch
            if not re.search(r"knn_(topk|merge|vote)_kernel|rows_rnorm_kernel", name):
                continue
            occ, need_no_scratch = (2 if "knn_topk_kernel" in name else 1), True
            if "knn_topk_kernel" in name and r.get("LDS", 0) > 81920:
                print("FAIL", name, "LDS", r.get("LDS"), "above 80 KiB: two workgroups no longer fit a CU")
                return 1
        elif what == "probe":
            # gram_partial_kernel: two workgroups of four waves per CU (its __launch_bounds__); accumulators, fragments and staged
            # loads are indexed by constants only: no scratch, no spills.  The reducer and the group sums assume no number of
            # resident workgroups and keep their per-lane sums in registers: no scratch
            if not re.search(r"gram_(partial|reduce)_kernel|group_sums_kernel", name):
                continue
            occ, need_no_scratch = (2 if "gram_partial_kernel" in name else 1), True
        elif what == "swin":
            if (m := re.search(r"window_attention_kernelILi(\d+)ELb([01])ELi(\d+)E", name)):
                # window_attention_kernel<SM, RQ32, NKT>: = its __launch_bounds__.  NKT 4 (2..64 tokens): four workgroups per CU;
                # NKT 9 (65..144 tokens): three, the 36 scores per lane stay in registers.  No scratch in either
                occ, need_no_scratch = (4 if int(m.group(3)) == 4 else 3), True
            elif re.search(r"window_attention_probs_kernelILi[0-3]EE", name):
                # window_attention_probs_kernel<SM> (swin_probs.hip): rows live in LDS and every loop runs over the token count, so
                # nothing may be indexed dynamically in registers: no scratch.  Its launcher assumes no number of resident workgroups
                occ, need_no_scratch = 1, True
            elif "window_attention" in name:
                print("check_resources: unknown window attention kernel", name)
                return 1
            else:
                m = re.search(r"layernorm_i16_i8_tiled(_compat)?_kernelILi(\d+)ELi(\d+)E", name)
                if not m:
                    continue
                occ, need_no_scratch = (3 if m.group(1) and int(m.group(3)) >= 2 else 4), True      # = their __launch_bounds__
        elif re.search(r"(embed|residual_requant)_kernelILin", name):
            # the two elementwise kernels with a clamp as template arguments (8-bit and 4-bit forms): one row each, no scratch
            occ, need_no_scratch = 1, True
        elif "patchify_hw_kernel" in name:
            # patchify_hw_kernel<float | uint8_t>: an elementwise grid-stride kernel whose launcher assumes no number of resident
            # workgroups; the index chain and the four table reads stay in registers: no scratch
            occ, need_no_scratch = 1, True
        elif "head_topk_kernel" in name:
            # the per-lane top-k lists live in registers (constant indices only): no scratch, full occupancy for any k <= 8
            occ, need_no_scratch = 8, True
        elif re.search(r"layernorm_i8_(pair_|v2_)?kernelI", name):
            # the other int8 LayerNorm kernels of the product: the occupancy is their __launch_bounds__ (`resident` and `grid > 1024`
            # in their launchers), restated here from the template arguments; no scratch
            if (m := re.search(r"layernorm_i8_kernelILi(\d+)ELb([01])E", name)):
                nj, compat = int(m.group(1)), m.group(2) == "1"
                occ = 3 if nj <= 3 and not compat else 2 if nj <= 8 else 1
            elif (m := re.search(r"layernorm_i8_pair_kernelILi(\d+)ELi(\d+)E", name)):
                occ = 4 if int(m.group(1)) <= 3 else 3
            else:
                m = re.search(r"layernorm_i8_v2_kernelILi(\d+)ELb([01])ELi(\d+)E", name)
                nj, compat, g = int(m.group(1)), m.group(2) == "1", int(m.group(3))
                occ = (3 if compat else 4) if g == 8 and nj <= 3 else 4 if nj <= 1 else 3 if nj <= 3 else 2
            # the one exception: layernorm_i8_v2_kernel<3, true, 16> (natural scales, 512 < C <= 768, more than 131 072 rows that the
            # streaming kernel does not take) spills three dwords, 12 bytes per lane
            need_no_scratch = "layernorm_i8_v2_kernelILi3ELb1ELi16E" not in name
        else:
            m = re.search(r"layernorm_i8_stream_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELi(\d+)E", name)
            if not m:
                continue
            occ = int(m.group(5))
            # scratch-free: every plain form, and the natural-scale form of the widths the BASELINE configs run (C = 768, 384, 192);
            # the natural-scale C = 1024 form spills a few loop-invariant dwords into cold paths (ln_stream.h)
            need_no_scratch = m.group(4) == "0" or int(m.group(2)) == 3
        seen += 1
        ok = r.get("Occupancy", 0) >= occ and (r.get("Scratch") == 0 and r.get("VGPRSpill", 0) == 0 or not need_no_scratch)
        narrow = narrow_rule(kernels, name)
        ok = ok and narrow is None
        print(("ok   " if ok else "FAIL ") + f"{name}: VGPR {r.get('VGPRs')}, scratch {r.get('Scratch')}, occupancy {r.get('Occupancy')} (launcher assumes {occ}"
              f"{', no scratch' if need_no_scratch else ''})" + (f" -- {narrow}" if narrow else ""))
        if not ok:
            bad.append(name)
    if seen == 0:
        print("check_resources: no", what, "kernel found in", path)
        return 1
    if bad:
        print("check_resources: occupancy / scratch assumption of the launchers violated:", ", ".join(bad))
        return 1
    return 0


def main(path):
    kernels = parse(open(path, errors="replace").read())
    bad, seen = [], 0
    for name, r in sorted(kernels.items()):
        if not any(g in name for g in GUARDED):
            narrow = narrow_rule(kernels, name)      # the small-tile and skinny-K kernels: no budget of their own, but a narrow form
            if twin_of(name):                        # still may not need more than its 8-bit twin
                print(("ok   " if narrow is None else "FAIL ") + f"{name}: VGPR+AGPR {r.get('VGPRs', 0) + r.get('AGPRs', 0)}, scratch "
                      f"{r.get('Scratch')}" + (f" -- {narrow}" if narrow else ""))
                if narrow:
                    bad.append(name)
            continue
        seen += 1
        regs = r.get("VGPRs", 0) + r.get("AGPRs", 0)
        line = (f"{name}: VGPR+AGPR {regs}, scratch {r.get('Scratch')}, VGPR spill {r.get('VGPRSpill')}, "
                f"SGPR spill {r.get('SGPRSpill')}, occupancy {r.get('Occupancy')}, LDS {r.get('LDS')}")
        ok = (r.get("Scratch") == 0 and r.get("VGPRSpill") == 0 and regs <= 256 and r.get("Occupancy", 0) >= 2
              and r.get("LDS", 0) <= 81920)
        narrow = narrow_rule(kernels, name)
        ok = ok and narrow is None
        print(("ok   " if ok else "FAIL ") + line + (f" -- {narrow}" if narrow else ""))
        if not ok:
            bad.append(name)
    if seen == 0:
        print("check_resources: no guarded kernel found in", path)
        return 1
    if bad:
        print("check_resources: register / scratch budget of the inline-asm GEMM kernels violated:", ", ".join(bad))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(occupancy_rules(sys.argv[1], sys.argv[2]) if len(sys.argv) > 2 else main(sys.argv[1]))
