"""attention_kernel MODE 0 with ONE float32 exponent gather per score and a float32 row sum (csrc/attention.hip; the argument
for the sum: csrc/attn_parts.h, SHIFTMAX_ORDER_SUM): every case byte for byte against the oracle through ivit_attention_fused_i8.

What the cases are for:
  * T = 197, B = 1, H = 4: the launcher deals the 13 query tiles out among four workgroups per head (asserted from a restatement of
    its model) -- the multi-part launch; the same problem with the lab build's part count forced to 1 is the full 13-tile walk of
    one workgroup, the wave that takes the fourth tile rotating with the head index; B * H = 528 is the product library's own
    one-workgroup-per-head launch.
  * T = 33, 17: waves with one query tile or none, a last key tile that is mostly padding (the general-T instantiations);
    T = 192: their largest row; T = 193, 207: the 13-tile instantiations with 1 and 15 real keys in the last key tile.
  * multiplier 2^k (the float32 score requantisation, RQ32) and 1.3 * 2^k (the float64 one): the two MODE 0 forms of each T.
  * a crafted head whose requantised scores take every value the 8-bit Shiftmax input has.  A row holds at most 207 keys, so no
    single row can hold all 256 values: every crafted row spans the whole range (its maximum is 127 and its minimum -128, table
    entries 0 and 255) and the rows of the two crafted heads together hold every value, i.e. read every table entry; the queries
    of a tile differ (+64, -64, 32, 127 in every d: the row as is, mirrored, halved, saturated on both sides) and the keys are
    shuffled, so that every lane position (g, l15) gathers entries from the low, the middle and the saturated part of the table.
    All of that is asserted on the oracle's scores before anything is launched.
  * two rows whose exact exponent sum is just below and at 2^24 (constructed; sums asserted first): the float32 sum must hand
    the first to the plain factor and the second to torch's order of additions."""
import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
from ivit_amd.prepare import dyadic  # noqa: E402
import attention_ref as A  # noqa: E402
import shiftmax_order_ref as smo  # noqa: E402
from attention_ref import release  # noqa: E402,F401  (the autouse fixture)

ENTRY = "ivit_attention_fused_i8"
HD = A.HD


def parts_model(batch_heads, nqt, waves=4, slots=1024):
    """attention_parts of csrc/attention.hip for the 8-bit short kernels (four resident workgroups on each of 256 CUs)"""
    best, best_t = 1, 0.0
    p = 1
    while p <= 4:
        if p > 1 and waves * (p // 2) >= nqt:
            break
        rounds, tiles = (batch_heads * p + slots - 1) // slots, (nqt + waves * p - 1) // (waves * p)
        t = rounds * (3.0 + 3.45 * tiles)
        if p == 1 or t < 0.95 * best_t:
            best, best_t = p, t
        p *= 2
    return best


def run(qkv, s_at, ms, es, mo, eo):
    return A.launch(ENTRY, qkv, (int(ms[0]), int(es[0]), float(s_at), int(mo[0]), int(eo[0])), 0)


def random_case(T, B, H, s_mult):
    s_at, ms, es, mo, eo = A.scales(False, s_mult, 8)
    qkv = A.inputs(np.random.default_rng(7919 * T + 31 * B + H + int(10 * s_mult)), B, H, T)
    exp, P00, _ = A.expected(qkv, s_at, ms, es, mo, eo, False, 8)
    if T > 17:
        assert P00[5].max() == 127 and P00[6].max() <= 1 + 128 // T      # the one-hot and the flat row of attention_ref.inputs
    return qkv, (s_at, ms, es, mo, eo), exp


@pytest.mark.parametrize("s_mult", [1.0, 1.3])
@pytest.mark.parametrize("T,B,H", [(197, 1, 4), (33, 1, 4), (17, 1, 4), (192, 1, 2), (193, 1, 2), (207, 1, 2)])
def test_random_rows(T, B, H, s_mult):
    qkv, sc, exp = random_case(T, B, H, s_mult)
    if T == 197:
        assert parts_model(B * H, 13) == 4, "the multi-part launch"
    got = run(qkv, *sc)
    assert np.array_equal(got, exp), f"{int((got != exp).sum())} bytes differ"


def test_full_tile_walk_one_workgroup_per_head():
    """T = 197, B = 1, H = 4 with the part count forced to 1 (lab build: bits 8-10 of ivit_debug_attention)"""
    qkv, sc, exp = random_case(197, 1, 4, 1.0)
    with _lib.lab_session() as L:
        L.ivit_debug_attention(1 << 8)
        got = run(qkv, *sc)
    assert np.array_equal(got, exp), f"{int((got != exp).sum())} bytes differ"


def test_one_workgroup_per_head_product_launch():
    """B * H = 528 heads: more than half of the 1024 slots, so the launcher's model keeps one workgroup per head"""
    B, H = 44, 12
    assert parts_model(B * H, 13) == 1
    qkv, sc, exp = random_case(197, B, H, 1.0)
    got = run(qkv, *sc)
    assert np.array_equal(got, exp), f"{int((got != exp).sum())} bytes differ"


# ------------------------------------------------------------------------------------------------ crafted rows
def crafted_scales(s_at=2.0 ** -3):
    """query = c in every d, key j = a_j in every d: S = 64 c a_j, and with the multiplier 2^-12 a query of 64 sees the row a"""
    ms, es = dyadic(np.float32(2.0 ** -12), np.float32(1.0))
    mo, eo = dyadic(np.float32(2.0 ** -8), np.float32(1.0))
    return np.float32(s_at), ms, es, mo, eo


QUERY_KINDS = (64, -64, 32, 127)


def query_value(i):
    """the crafted query i: the kinds rotate within a tile and shift from tile to tile, so that every position l15 = i % 16 holds each"""
    return QUERY_KINDS[(i + i // 16) % 4]


def every_score_head(T, rng):
    """-> qkv [3, 1, 2, T, 64]: two heads whose key rows hold 127, -128 and, together, every value of [-128, 127], shuffled"""
    qkv = np.clip(np.rint(rng.normal(0, 40, size=(3, 1, 2, T, HD))), -128, 127).astype(np.int8)
    vals = rng.permutation(np.arange(-127, 127))                 # the 254 values between the two ends
    first, second = vals[:T - 2], vals[T - 2:]
    second = np.concatenate([second, rng.choice(first, T - 2 - len(second), replace=False)])
    for h, body in enumerate((first, second)):
        qkv[1, 0, h] = rng.permutation(np.concatenate([[127, -128], body]))[:, None].astype(np.int8)
        qkv[0, 0, h] = np.array([query_value(i) for i in range(T)], np.int8)[:, None]
    return qkv


@pytest.mark.parametrize("T", [197, 207])
def test_every_table_entry_from_every_lane(T):
    s_at, ms, es, mo, eo = crafted_scales()
    qkv = every_score_head(T, np.random.default_rng(4242 + T))
    seen = np.zeros(256, bool)
    low = np.zeros((4, 16), bool)
    mid, sat = low.copy(), low.copy()
    x0 = int(smo.x0_of(s_at))
    ksat = next(i for i in range(256) if -i + (-i >> 1) - (-i >> 4) <= 15 * x0)      # first entry at the clamp of ivit_modules.py:155
    assert 48 < ksat < 255
    for h in range(2):
        ka = orc.requant(orc.gemm_i8(qkv[0, 0, h], qkv[1, 0, h]), ms.astype(np.float64), es, 8)          # [query, key]
        for i in range(T):
            if query_value(i) == 64:
                assert np.array_equal(ka[i], qkv[1, 0, h, :, 0]), "a query of 64 sees the key row itself"
            if abs(query_value(i)) >= 64:
                assert ka[i].max() == 127 and ka[i].min() <= -127
        idx = ka.max(axis=1, keepdims=True) - ka                # the table entry each score reads
        assert idx.min() == 0 and idx.max() == 255
        seen[np.unique(idx[[i for i in range(T) if query_value(i) == 64]])] = True
        g = (np.arange(T) % 16) // 4                           # the lane group that holds key j of a 16-key tile
        for i in range(T):
            for gg in range(4):
                e = idx[i][g == gg]
                low[gg, i % 16] |= bool((e < ksat // 3).any())
                mid[gg, i % 16] |= bool(((e >= ksat // 3) & (e < ksat)).any())
                sat[gg, i % 16] |= bool((e >= ksat).any())
    assert seen.all(), f"table entries no crafted row reads: {np.flatnonzero(~seen).tolist()}"
    assert low.all() and mid.all() and sat.all(), "a lane position that misses a part of the table"
    exp, _, _ = A.expected(qkv, s_at, ms, es, mo, eo, False, 8)
    got = run(qkv, s_at, ms, es, mo, eo)
    assert np.array_equal(got, exp), f"{int((got != exp).sum())} bytes differ"


def threshold_rows(T, s_at):
    """-> (row just below 2^24, row at or just above it) as int scores, their exact exponent sums.  63 keys at the maximum carry
    63 |x0| 2^15; the other keys are filled greedily from the exponent table towards 2^24 - 1, resp. 2^24"""
    e = smo.shiftexp(-np.arange(256, dtype=np.float32), smo.x0_of(s_at)).astype(np.int64)      # entry i = exponent of max - i
    assert e[0] * 64 == 1 << 24, "the construction wants |x0| 2^15 = 2^18"
    rows, sums = [], []
    for target in ((1 << 24) - 1, 1 << 24):
        idx, left = [0] * 63, target - 63 * int(e[0])
        for n in range(T - 63, 0, -1):
            ok = np.flatnonzero(e + (n - 1) * int(e.min()) <= left)          # the later keys still fit at the smallest exponent
            i = int(ok[np.argmax(e[ok])]) if len(ok) else 255
            idx.append(i)
            left -= int(e[i])
        rows.append(127 - np.array(idx))
        sums.append(int(e[idx].sum()))
    return rows, sums


@pytest.mark.parametrize("T", [197, 130])
def test_row_sums_at_the_order_threshold(T):
    s_at, ms, es, mo, eo = crafted_scales()
    rows, sums = threshold_rows(T, s_at)
    assert (1 << 24) - 64 <= sums[0] < (1 << 24) <= sums[1] < (1 << 24) + 64, sums
    rng = np.random.default_rng(99 + T)
    qkv = np.clip(np.rint(rng.normal(0, 40, size=(3, 1, 2, T, HD))), -128, 127).astype(np.int8)
    for h in range(2):
        assert rows[h].min() >= -128 and rows[h].max() == 127
        qkv[1, 0, h] = rng.permutation(rows[h])[:, None].astype(np.int8)
        qkv[0, 0, h, 0] = 64
        qkv[0, 0, h, T // 2] = 64
        ka = orc.requant(orc.gemm_i8(qkv[0, 0, h, :1], qkv[1, 0, h]), ms.astype(np.float64), es, 8)
        ef = smo.exponents(ka[0], s_at)
        assert int(ef.astype(np.int64).sum()) == sums[h]
        S = orc.torch_rowsum(ef)                   # the oracle's float32 sum of this row
        assert (float(S) == float(sums[h])) if h == 0 else (float(S) >= float(1 << 24))
    exp, _, _ = A.expected(qkv, s_at, ms, es, mo, eo, False, 8)
    got = run(qkv, s_at, ms, es, mo, eo)
    assert np.array_equal(got, exp), f"{int((got != exp).sum())} bytes differ"
