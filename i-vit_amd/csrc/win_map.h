// win_map.h -- the row maps of the Swin window partition, stated ONCE for every kernel that stores or gathers rows in window order
// (swin.hip: residual QuantAct, the 16-bit I-LayerNorm, window attention, ivit_window_rows; ibert.hip: the 16-bit I-BERT LayerNorm).
// Included inside the anonymous namespace of those files, after common.h.  Host restatement: swin_engine.window_row_map.
//
// The window partition / cyclic shift of SwinTransformerBlock.forward (swin_quant.py:258-271, 278-289) are pure row permutations of
// a [B, H*W, C] tensor.  win_row(r) = index, in window-major order (image, window row, window col, row in window, col in window),
// of token r = (b, y, x) after rolling by -shift.
#pragma once

struct WinMap {
    int H, W, ws, shift;  // ws == 0: identity
};

IVIT_DEV int64_t win_row(const WinMap& m, int64_t r)
{
    if (m.ws == 0) return r;
    const int L = m.H * m.W;
    const int b = (int)(r / L);
    const int t = (int)(r - (int64_t)b * L);
    int y = t / m.W, x = t - y * m.W;
    // shifted_x[y'] = x[(y' + shift) mod H]  =>  token (y, x) lands at y' = (y - shift) mod H
    y = y - m.shift; if (y < 0) y += m.H;
    x = x - m.shift; if (x < 0) x += m.W;
    const int wy = y / m.ws, iy = y - wy * m.ws, wx = x / m.ws, ix = x - wx * m.ws;
    const int nwx = m.W / m.ws;
    return ((int64_t)b * (m.H / m.ws) * nwx + (int64_t)wy * nwx + wx) * (m.ws * m.ws) + iy * m.ws + ix;
}

// the inverse: row R of the window-ordered tensor (window index, position in the window) -> row of the image-ordered one
// (window_reverse + the roll back, swin_quant.py:278-287)
IVIT_DEV int64_t win_row_inv(const WinMap& m, int64_t R)
{
    if (m.ws == 0) return R;
    const int T = m.ws * m.ws, nwx = m.W / m.ws, nwy = m.H / m.ws;
    const int64_t widx = R / T;
    const int pos = (int)(R - widx * T);
    const int iy = pos / m.ws, ix = pos - iy * m.ws;
    const int b = (int)(widx / (nwy * nwx)), wrem = (int)(widx - (int64_t)b * (nwy * nwx));
    const int wy = wrem / nwx, wx = wrem - wy * nwx;
    int y = wy * m.ws + iy + m.shift; if (y >= m.H) y -= m.H;
    int x = wx * m.ws + ix + m.shift; if (x >= m.W) x -= m.W;
    return (int64_t)b * m.H * m.W + (int64_t)y * m.W + x;
}

// the window description every entry with (H, W, ws, shift) accepts; ws == 0: no map, the other three are not read
static inline bool win_map_ok(int64_t rows, int H, int W, int ws, int shift)
{
    return ws == 0 || (H > 0 && W > 0 && ws > 0 && H % ws == 0 && W % ws == 0 && shift >= 0 && shift < ws && rows % ((int64_t)H * W) == 0);
}
