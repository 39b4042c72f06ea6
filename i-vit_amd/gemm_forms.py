"""Which kernel an int8 GEMM launch runs, and the weight copy that goes with it -- the one place where Python restates the
launcher's rule (csrc/gemm.hip gemm_plan; include/ivit_hip.h ivit_gemm_plan describes it).

The launcher picks the kernel from the shape and the layout bits; the caller has to hand over the weight copy in that kernel's
order: row-major for the small-tile and skinny-K kernels, row-major or the block layout for the persistent kernel, a fragment copy
for the weights-in-registers kernels.  `form` mirrors the launcher's choice, `weight` picks the copy, and
tests/test_gemm_plan_cpu.py holds `form` against ivit_gemm_plan over every epilogue, layout and a sweep of shapes, so the two
cannot drift apart unnoticed.  Pure host arithmetic: nothing here loads the library or touches a tensor's data."""
from __future__ import annotations

# layout bits of the `_ex` entries (IVIT_A_BLOCKS ... IVIT_W_FRAGS16 of include/ivit_hip.h)
A_BLOCKS, W_BLOCKS, OUT_BLOCKS, W_FRAGS, W_FRAGS16 = 1, 2, 4, 8, 16
FRAGS = W_FRAGS | W_FRAGS16
# epilogue kinds (IVIT_GEMM_EPI_*) and kernel forms (IVIT_GEMM_FORM_*)
RQ, RESID, QKV, I32, RESID16, RQ16, RQ16_RES16 = range(7)
SMALL, PERS, WREG, WREG16, SKINNY = range(5)
# the layout bits each epilogue's entry takes
LAYOUTS = {RQ: A_BLOCKS | W_BLOCKS | OUT_BLOCKS | FRAGS, RESID: A_BLOCKS | W_BLOCKS | FRAGS, QKV: A_BLOCKS | W_BLOCKS | FRAGS, I32: 0,
           RESID16: A_BLOCKS | W_BLOCKS | FRAGS, RQ16: 0, RQ16_RES16: A_BLOCKS | W_FRAGS}

# dispatch thresholds (csrc/gemm_common.h: BIG_MIN_M, SK_MIN_M, BCH, WR_WASTE_DEN; csrc/gemm.hip: SK_MAXK, SK_MAXN, WR_CH)
BIG_MIN_M, BIG_MIN_N = 2048, 128      # the tile-looping kernels (persistent, weights-in-registers)
SK_MIN_M, SK_MAXK, SK_MAXN = 8192, 128, 320
WR_CH, WR_WASTE_DEN = 256, 8

_INT8_OUT = (RQ, RESID, QKV)              # epilogues with 128-channel work items in the 16x16x64 order
_NO_TILE_LOOP = (I32, RQ16)               # small-tile kernel only


def skinny_applies(epi: int, M: int, N: int, K: int) -> bool:
    """the skinny-K form as the launcher states it (dense rows; no layout bit, no output map)"""
    return (epi in (RQ, QKV) and M >= SK_MIN_M and 32 <= K <= SK_MAXK and K % 32 == 0 and 16 <= N <= SK_MAXN and N % 16 == 0
            and M * N < 1 << 32)


def pers_applies(epi: int, M: int, N: int) -> bool:
    """the persistent LDS-DMA kernel: what block-layout operands need"""
    return epi not in _NO_TILE_LOOP and epi != RQ16_RES16 and M >= BIG_MIN_M and N >= BIG_MIN_N


def frags_shape(N: int, K: int) -> bool:
    """the weights a fragment copy exists for"""
    return N >= BIG_MIN_N and N % 64 == 0 and K % 192 == 0


def frags_apply(epi: int, M: int, N: int, K: int, bit: int = W_FRAGS16) -> bool:
    """a launch with fragment copy `bit` is accepted (the 16-bit-stream epilogue exists for the 32x32x32 order only)"""
    return (epi not in _NO_TILE_LOOP and (bit == W_FRAGS or epi != RQ16_RES16) and M >= BIG_MIN_M and frags_shape(N, K)
            and (bit == W_FRAGS or (M + 16) * N < 1 << 32))


def tiles_fit(N: int) -> bool:
    """256-channel tiles waste at most an eighth of their columns"""
    return -(-N // WR_CH) * WR_CH * WR_WASTE_DEN <= N * (WR_WASTE_DEN + 1)


def frag_items_ok(bit: int, narrow: bool, N: int) -> bool:
    """a fragment copy pays for this consumer: the 128-channel work items exist only for the 16x16x64 order with an int8
    epilogue (`narrow`); every other consumer works in 256-channel tiles, used only where they fit"""
    return (bit == W_FRAGS16 and narrow) or tiles_fit(N)


def blocks_shape(N: int, K: int) -> bool:
    """the weights a block-layout copy exists for"""
    return N >= BIG_MIN_N and N % 16 == 0 and K % 64 == 0


def block_operands_apply(M: int, N: int, K: int) -> bool:
    """operands in the block layout: the consuming GEMM [M, K] x [N, K] is a tile-looping kernel"""
    return M >= BIG_MIN_M and blocks_shape(N, K)


def form(epi: int, M: int, N: int, K: int, layouts: int = 0):
    """The kernel form of a launch with dense, aligned operands, or None where the launcher refuses: gemm_check's conditions on
    the shape, the entry's layout mask, then gemm_plan's choice."""
    int8_acc = epi not in (I32, RQ16, RQ16_RES16)
    if min(M, N, K) <= 0 or K % 64 or N % (16 if int8_acc else 8 if epi == RQ16_RES16 else 4):
        return None
    if layouts & ~LAYOUTS[epi] or layouts & FRAGS == FRAGS or (epi == RQ16_RES16 and layouts & A_BLOCKS and not layouts & FRAGS):
        return None
    if layouts & OUT_BLOCKS and (N % 64 or (M + 15) * N >= 1 << 31):
        return None
    if epi == QKV and M * N >= 1 << 31:
        return None
    if not layouts and skinny_applies(epi, M, N, K):
        return SKINNY
    if layouts & (A_BLOCKS | W_BLOCKS) and not layouts & FRAGS and not pers_applies(epi, M, N):
        return None
    if layouts & FRAGS:
        bit = layouts & FRAGS
        if layouts & W_BLOCKS or not frags_apply(epi, M, N, K, bit):
            return None
        return WREG if bit == W_FRAGS else WREG16
    return PERS if pers_applies(epi, M, N) else SMALL


def weight(lin: dict, epi: int, M: int, frags: bool = True, blocks: bool = True):
    """(weight tensor, layout bits) for a launch of M rows with epilogue `epi`.  lin: N, K, the row-major "W" and whichever copies
    the linear holds -- "Wf" + "Wf_bit" (engine_common.frag_copy), "Wf32" (a second, 32x32x32 copy), "Wb" (block_copy).
    frags / blocks = False: the caller rules those copies out (A/B switches, a consumer that reads rows)."""
    N, K = lin["N"], lin["K"]
    if frags:
        for W, bit in ((lin.get("Wf"), lin.get("Wf_bit")), (lin.get("Wf32"), W_FRAGS)):
            if W is not None and frags_apply(epi, M, N, K, bit) and frag_items_ok(bit, epi in _INT8_OUT, N):
                return W, bit
    if blocks and lin.get("Wb") is not None and not skinny_applies(epi, M, N, K) and pers_applies(epi, M, N):
        return lin["Wb"], W_BLOCKS
    return lin["W"], 0
