// bilinear_tap.h -- the integer weights of a bilinear upsample by the factor r with align_corners = False (include/ivit_hip.h, "dense
// linear probe"), for the kernels that stage a source cell with its predecessor and successor (clamped) in LDS: dense.hip, davis.hip.
#pragma once
#include "common.h"

// weights of one axis for the offset j (0 .. r - 1) inside a cell: source slots (s, s + 1) relative to the cell's predecessor, (2r - f, f)
IVIT_DEV void dense_tap(int j, int r, int& s, int& f)
{
    const int n = 2 * j + 1 - r;
    s = n < 0 ? 0 : 1;
    f = n < 0 ? n + 2 * r : n;
}
