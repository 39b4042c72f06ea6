"""The reference and the shape tables of tests/test_gpu_gemm_schedule.py, checked without a GPU: the fast product equals the
oracle's, every table holds every scheduling regime it claims, and the restated tile order covers each launch exactly once."""
import numpy as np
import pytest

from oracle import oracle as orc

import gemm_sched_ref as gs


@pytest.mark.parametrize("M,N,K", [(700, 320, 192), (300, 192, 1536), (257, 64, 3072)])
def test_gemm_ref_equals_oracle(M, N, K):
    """gemm_ref == orc.gemm_i8: one, two and three K chunks; the largest magnitude a chunk must hold (every operand -128:
    1024 * 128 * 128 = 2^24 per chunk), and the tie data of the GPU tests"""
    A = np.full((M, K), -128, np.int8)
    W = np.full((N, K), -128, np.int8)
    b = np.arange(N, dtype=np.int32) * 1001 - 50000
    got = gs.gemm_ref(A, W, b)
    assert got.dtype == np.int32 and np.array_equal(got, orc.gemm_i8(A, W, b))
    assert got.max() == K * 16384 + int(b.max())
    W[::2] = 127                            # and the most negative sums
    assert np.array_equal(gs.gemm_ref(A, W, None), orc.gemm_i8(A, W))
    _, A, W, b = gs.tie_operands(M, N, K, M + N + K)
    assert (A[::7] == 1).all()
    assert np.array_equal(gs.gemm_ref(A, W, b), orc.gemm_i8(A, W, b))


@pytest.mark.parametrize("table", ["wreg", "pers"])
def test_shape_tables_hold_every_regime(table):
    """each entry is in the regime its id stands for: an edit of a table cannot quietly lose one"""
    (tt, tc), shapes = gs.TABLES[table]
    assert sorted(shapes) == sorted(gs.REGIMES)
    for sid, (M, N) in shapes.items():
        assert gs.REGIMES[sid](M, N, tt, tc), (table, sid, gs.regime(M, N, tt, tc))
        # what the kernels' entry points ask of a shape, so that no launch falls to another kernel
        assert M >= 2048 and N >= 128 and N % 64 == 0
    # the thresholds from both sides, and both values of ntiles & 7 == 0 among the split launches
    reg = {sid: gs.regime(M, N, tt, tc) for sid, (M, N) in shapes.items()}
    assert 2 * reg["C"][2] == 256 and reg["C"][3] and 2 * reg["D"][2] == 260 and not reg["D"][3]
    assert reg["E"][2] == 0 and reg["G"][1] == 0 and reg["F"][1] == 2
    assert reg["A"][4] != 0 and reg["B"][4] == 0
    # the numbers written beside the tables
    assert [reg[s][0] for s in "ABCDEFG"] == [516, 520, 640, 642, 512, 1040, 300]


@pytest.mark.parametrize("table", ["wreg", "pers"])
def test_tile_order_and_work_items_cover_the_output_once(table):
    """the restated tile order is a permutation of [0, ntiles) for every entry, and the work items it gives (full tiles, then
    the half tiles of a split last round), with the product's threshold and with the split forced off and on, cover every row
    of every channel tile exactly once"""
    (tt, tc), shapes = gs.TABLES[table]
    for sid, (M, N) in shapes.items():
        ntiles = gs.regime(M, N, tt, tc)[0]
        assert np.array_equal(np.sort(gs.tile_order(ntiles)), np.arange(ntiles)), (table, sid)
        tiles_n = -(-N // tc)
        for split in (None, False, True):
            cover = np.zeros((-(-M // (tt // 2)), tiles_n), np.int32)      # in half tiles of rows
            seen = set()
            for (wg, idx, m0, rows, n0) in gs.work_items(M, N, tt, tc, split):
                assert 0 <= wg < min(ntiles, gs.SLOTS) and (wg, idx) not in seen and m0 < M
                seen.add((wg, idx))
                cover[m0 // (tt // 2):(m0 + rows) // (tt // 2), n0 // tc] += 1
            assert (cover == 1).all(), (table, sid, split)
            for (wg, idx) in seen:           # a workgroup's items are numbered without a gap: its loop ends at the first miss
                assert idx == 0 or (wg, idx - 1) in seen


@pytest.mark.parametrize("table", ["wreg", "pers"])
def test_entry_b_has_a_split_tile_with_a_dead_second_half(table):
    """entry B: tile 519 of 520 (ntiles & 7 == 0: the last position of the order names the last tile) is the partial last token
    tile, one of the 8 tiles that are split, and its second half starts at or beyond M: that workgroup has no half tile"""
    (tt, tc), shapes = gs.TABLES[table]
    M, N = shapes["B"]
    ntiles, rounds, R, split, low = gs.regime(M, N, tt, tc)
    assert (ntiles, rounds, R, split, low) == (520, 1, 8, True, 0)
    lid = gs.tile_order(ntiles)
    tiles_n = -(-N // tc)
    split_tiles = [divmod(int(lid[t]), tiles_n) for t in range(gs.SLOTS, ntiles)]
    last_tm = -(-M // tt) - 1
    dead = [(tm, tn) for (tm, tn) in split_tiles if tm == last_tm and tm * tt + tt // 2 >= M]
    assert (last_tm, tiles_n - 1) in dead and int(lid[519]) == 519
    items = gs.work_items(M, N, tt, tc)
    halves = [it for it in items if it[3] == tt // 2]
    assert len(halves) == 2 * R - len(dead) and len(dead) >= 1
    # the workgroups of the dead halves end after their full tile
    for b in range(2 * R):
        tm, tn = divmod(int(lid[gs.SLOTS + (b >> 1)]), tiles_n)
        has_half = any(it[0] == b and it[1] == 1 for it in items)
        assert has_half == (not ((tm, tn) in dead and (b & 1))), b


@pytest.mark.parametrize("table", ["wreg", "pers"])
def test_restated_arithmetic_is_the_launchers(table):
    """the launcher's own plan (ivit_gemm_plan: the function launch_gemm calls, a host function) reports for every table entry
    the tile counts, the grid and the first split tile that regime / work_items restate: the reference file is held against
    the launcher, not only against itself"""
    import ctypes

    pytest.importorskip("ivit_amd")
    from ivit_amd import _lib, gemm_forms

    (tt, tc), shapes = gs.TABLES[table]
    out = (ctypes.c_int32 * 8)()
    for layouts in {"wreg": (gemm_forms.W_FRAGS, gemm_forms.W_FRAGS16), "pers": (0, gemm_forms.W_BLOCKS)}[table]:
        form = {0: gemm_forms.PERS, gemm_forms.W_BLOCKS: gemm_forms.PERS, gemm_forms.W_FRAGS: gemm_forms.WREG,
                gemm_forms.W_FRAGS16: gemm_forms.WREG16}[layouts]
        for sid, (M, N) in shapes.items():
            assert _lib.lib().ivit_gemm_plan(gemm_forms.RQ, M, N, gs.K_SCHED, layouts, out) == 0, (table, sid)
            got_form, grid, tiles_m, tiles_n, split_from = list(out)[:5]
            ntiles, rounds, R, split, _ = gs.regime(M, N, tt, tc)
            assert got_form == form and (tiles_m, tiles_n) == (-(-M // tt), -(-N // tc)) and tiles_m * tiles_n == ntiles, (table, sid)
            assert grid == min(ntiles, gs.SLOTS) and split_from == (rounds * gs.SLOTS if split else ntiles), (table, sid, list(out))
            items = gs.work_items(M, N, tt, tc)
            assert max(it[0] for it in items) + 1 == grid, (table, sid)
            assert sum(1 for it in items if it[3] == tt) == split_from, (table, sid)
