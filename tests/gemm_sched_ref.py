"""Fast exact reference and shape tables for the tests of the int8 GEMM's tile scheduling (tests/test_gemm_sched_cpu.py,
tests/test_gpu_gemm_schedule.py).

Which tiles a workgroup of gemm_i8_wreg_kernel / gemm_i8_pers_kernel computes after its first one, and how a sparse last round
is split into half tiles, depends on the NUMBER of tiles of a launch and not on K.  With K = 192 an exact product of 20-30 M
outputs is one float32 BLAS call, so the whole output of launches with several rounds can be held against a reference.

Nothing here imports the product: the launcher's arithmetic (csrc/gemm.hip launch_gemm, wr_tile / wr_work, pers_tile /
pers_work) is RESTATED from its comments; the CPU test holds the shape tables against the restatement, and the restatement
against the launcher's own plan (ivit_gemm_plan)."""
import numpy as np

K_SCHED = 192          # the smallest K the fragment forms accept ((K / 64) % 3 == 0); above the skinny-K form's 128
SLOTS = 512            # two resident workgroups on each of 256 CUs
WREG_TILE = (128, 256)     # tokens x channels of a work item of gemm_i8_wreg_kernel (IVIT_W_FRAGS / IVIT_W_FRAGS16)
PERS_TILE = (256, 128)     # ... of gemm_i8_pers_kernel

# id -> (M, N).  The regime of each entry is what REGIMES[id] says; test_gemm_sched_cpu.py checks it.
WREG_SHAPES = {
    "A": (21966, 768),     # 172 x 3 = 516: one round, R = 4, split; ntiles & 7 = 4; last token tile has 78 rows
    "B": (13224, 1152),    # 104 x 5 = 520: split, R = 8; ntiles & 7 = 0; last token tile has 40 rows; channel tile beyond N
    "C": (20477, 1024),    # 160 x 4 = 640: R = 128, the last split (2R = 256)
    "D": (27315, 768),     # 214 x 3 = 642: R = 130, the first non-split
    "E": (16284, 1024),    # 128 x 4 = 512: R = 0, exactly one round
    "F": (33200, 1024),    # 260 x 4 = 1040: two rounds, R = 16: full, full, half in one workgroup
    "G": (12723, 768),     # 100 x 3 = 300: no round completed, one full tile per workgroup
}
PERS_SHAPES = {
    "A": (43950, 384),
    "B": (26444, 576),
    "C": (40900, 512),
    "D": (54700, 384),
    "E": (32700, 512),
    "F": (66500, 512),
    "G": (25500, 384),
}
TABLES = {"wreg": (WREG_TILE, WREG_SHAPES), "pers": (PERS_TILE, PERS_SHAPES)}


def regime(M, N, tile_tokens, tile_channels):
    """(ntiles, rounds, R, split, ntiles & 7) of a launch, by the launcher's published arithmetic: 512 workgroup slots, a last
    round of R tiles runs as 2R half tiles when 0 < 2R <= 256 and at least one round of full tiles precedes it"""
    ntiles = -(-M // tile_tokens) * -(-N // tile_channels)
    rounds, R = divmod(ntiles, SLOTS)
    split = rounds > 0 and 0 < 2 * R <= 256
    return ntiles, rounds, R, split, ntiles & 7


# what each table entry is there for, as a predicate over (M, N, tile_tokens, tile_channels)
def _last_rows(M, tt):
    return M - (-(-M // tt) - 1) * tt


REGIMES = {
    "A": lambda M, N, tt, tc: regime(M, N, tt, tc)[1:4] == (1, 4, True) and regime(M, N, tt, tc)[4] != 0 and tt // 2 < _last_rows(M, tt) < tt,
    "B": lambda M, N, tt, tc: regime(M, N, tt, tc)[1:] == (1, 8, True, 0) and _last_rows(M, tt) <= tt // 2 and N % tc != 0,
    "C": lambda M, N, tt, tc: regime(M, N, tt, tc)[1:4] == (1, 128, True),
    "D": lambda M, N, tt, tc: regime(M, N, tt, tc)[1:4] == (1, 130, False),
    "E": lambda M, N, tt, tc: regime(M, N, tt, tc)[:4] == (512, 1, 0, False),
    "F": lambda M, N, tt, tc: regime(M, N, tt, tc)[1:4] == (2, 16, True),
    "G": lambda M, N, tt, tc: regime(M, N, tt, tc)[1] == 0 and 256 < regime(M, N, tt, tc)[0] < 512,
}


def tile_order(ntiles):
    """lid[t]: the tile (row-major index tm * tiles_n + tn) that position t of the launch order names.  The eight XCDs take
    workgroups round robin (xcd = t & 7), and each walks a contiguous range of tiles: the first ntiles & 7 XCDs have one more."""
    t = np.arange(ntiles)
    q8, r8, xcd = ntiles >> 3, ntiles & 7, t & 7
    return np.where(xcd < r8, xcd * (q8 + 1), r8 * (q8 + 1) + (xcd - r8) * q8) + (t >> 3)


def work_items(M, N, tile_tokens, tile_channels, split=None):
    """Every work item of a launch as (workgroup, index within the workgroup, first row, rows of the item, first column):
    restates wr_work / pers_work.  `split`: None = the product's threshold, else forced (the lab build's bits 27 / 11)."""
    tiles_n = -(-N // tile_channels)
    ntiles, rounds, R, sp, _ = regime(M, N, tile_tokens, tile_channels)
    if split is not None:
        sp = bool(split) and rounds > 0 and R > 0
    G = min(ntiles, SLOTS)
    split_from = rounds * SLOTS if sp else ntiles
    lid = tile_order(ntiles)
    items = []
    for t in range(split_from):
        tm, tn = divmod(int(lid[t]), tiles_n)
        items.append((t % G, t // G, tm * tile_tokens, tile_tokens, tn * tile_channels))
    half = tile_tokens // 2
    for b in range(2 * (ntiles - split_from)):
        tm, tn = divmod(int(lid[split_from + (b >> 1)]), tiles_n)
        m0 = tm * tile_tokens + half * (b & 1)
        if m0 < M:          # a second half that starts at or beyond M has no rows: that workgroup ends
            nfull = (split_from - b + G - 1) // G if b < split_from else 0
            items.append((b, nfull, m0, half, tn * tile_channels))
    return items


def gemm_ref(A, W, bias=None):
    """A [M, K] int8, W [N, K] int8 -> int32 [M, N] = A W^T + bias, exactly.  float32 BLAS over K chunks of at most 1024: a
    chunk's partial sums stay within 1024 * 128 * 128 = 2^24 in magnitude, where every integer is a float32."""
    A = np.ascontiguousarray(A, dtype=np.int8)
    W = np.ascontiguousarray(W, dtype=np.int8)
    (M, K), N = A.shape, W.shape[0]
    assert W.shape[1] == K
    out = np.zeros((M, N), np.int32)
    for k0 in range(0, K, 1024):
        p = A[:, k0:k0 + 1024].astype(np.float32) @ W[:, k0:k0 + 1024].astype(np.float32).T
        out += p.astype(np.int32)
    if bias is not None:
        out += np.asarray(bias, np.int32)[None, :]
    return out


def tie_operands(M, N, K, seed):
    """The operands of test_gemm_weights_in_registers_ties_and_failed_certificates: every seventh row of A all ones, so that
    its accumulators are bias + row sums of W and meet power-of-two multipliers in exact .5 ties; bias in +-50000"""
    rng = np.random.default_rng(seed)
    A = rng.integers(-128, 128, size=(M, K), dtype=np.int8)
    A[::7] = 1
    W = rng.integers(-128, 128, size=(N, K), dtype=np.int8)
    b = rng.integers(-50000, 50000, size=N).astype(np.int32)
    return rng, A, W, b
