"""Search for the crafted score rows of tests/ibert_long_ref.py (CPU only): rows of the long-row I-BERT attention for which the
ORDER of the float32 row sum changes the probabilities.

Random rows do not show a wrong order: floor(2^32 / S) and floor(e * factor / 2^25) absorb a last-bit change of S on all but about
one row in 1 500.  The rows here are constructed instead (ibert_long_ref.crafted_row): the exponents of every key but the dominant
one are fixed by (T, seed) and add up to about 0.6 * 2^30; the dominant key's table entry x is free.  torch's sum S(x) is
non-decreasing in x, so a bisection finds the x at which it passes 2^30, where factor = floor(2^32 / S) drops from 4 to 3; the
floats around that x are then scanned for one at which torch's order (oracle torch_rowsum) and another order stand on different
sides of 2^30 -- there the probabilities differ by a quarter.  Orders compared: (a) left to right, (b) each lane's keys in
register order, then a tree over the query's four lanes.

    python scripts/find_rowsum_rows.py            # prints the CRAFTED / CRAFTED_B lists of tests/ibert_long_ref.py

Search of record: token counts 301, 577, 785, 1000, 1024, 1025 (the three cascade classes), seeds 0 .. 7 per token count, window of
+-48 floats around the crossing (1.8 s in all).  Seeds with an x at which (a) differs: 8 of 8 at every token count; with an x at
which (a) and (b) both differ: 301: 3/8, 577: 6/8, 785: 7/8, 1000: 1/8, 1024: 5/8, 1025: 3/8.  The first such seed is kept
for every token count."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from oracle import oracle as orc  # noqa: E402
import ibert_long_ref as R  # noqa: E402

TOKENS = (301, 577, 785, 1000, 1024, 1025)
SEEDS = 8
WINDOW = 48
LIMIT = np.float32(2.0 ** 30)


def with_x(row, e, bits):
    e = e.copy()
    e[row["pos"]] = np.array([bits], np.uint32).view(np.float32)[0]
    return e


def search(T, seed):
    """-> (bits with (a) differing or None, bits with (a) and (b) differing or None)"""
    row = R.crafted_row(T, seed)
    e0 = R.crafted_exponents(row)
    lo = int(np.array([2.0 ** 27], np.float32).view(np.uint32)[0])
    hi = int(np.array([2.0 ** 30], np.float32).view(np.uint32)[0])      # positive floats order as their bit patterns
    assert orc.torch_rowsum(with_x(row, e0, lo)) <= LIMIT < orc.torch_rowsum(with_x(row, e0, hi))
    while hi - lo > 1:          # the last x with S(x) <= 2^30
        mid = (lo + hi) // 2
        if orc.torch_rowsum(with_x(row, e0, mid)) <= LIMIT:
            lo = mid
        else:
            hi = mid
    hit_a = hit_ab = None
    for bits in range(lo - WINDOW, lo + WINDOW + 1):
        e = with_x(row, e0, bits)
        pt = R.probabilities(e, orc.torch_rowsum(e))
        da = not np.array_equal(pt, R.probabilities(e, R.sum_left_to_right(e)))
        db = not np.array_equal(pt, R.probabilities(e, R.sum_lane_tree(e)))
        if da and hit_a is None:
            hit_a = bits
        if da and db and hit_ab is None:
            hit_ab = bits
    return hit_a, hit_ab


def main():
    orc.build()
    crafted = []
    for T in TOKENS:
        na = nab = 0
        kept = None
        for seed in range(SEEDS):
            a, ab = search(T, seed)
            na += a is not None
            nab += ab is not None
            if kept is None and ab is not None:
                kept = (T, seed, ab)
        print(f"# T={T}: (a) {na}/{SEEDS} seeds, (a) and (b) {nab}/{SEEDS} seeds")
        assert kept is not None, T
        crafted.append(kept)
    print("CRAFTED = [" + ", ".join(f"({T}, {s}, 0x{b:08x})" for T, s, b in crafted) + "]")
    print("CRAFTED_B = CRAFTED")


if __name__ == "__main__":
    main()
