"""The float-emitting LayerNorm entries of the token features (csrc/ln_tokens.h): ivit_layernorm_i8_f32, ivit_layernorm_i16_f32,
ivit_ibert_layernorm_i8_f32, ivit_ibert_layernorm_i16_f32, bit for bit against
  (a) the pinned module-level entries on the same rows: ivit_layernorm_i32_f32 on the widened integers, ivit_layernorm_f32_f32_ex on
      fl(q * s) at a natural scale, ivit_ibert_layernorm_i32_f32_ex / _f32_f32_ex with and without the integer square root, and
  (b) the oracle: oracle.layernorm / layernorm_compat / layernorm_scaled and, for I-BERT, the float64-sum restatement of
      tests/ibert_intsqrt_ref.py on the rows whose two sums stay below 2^24 (where no order of additions matters).
One reference per (kind, C, scale) over 394 rows -- crafted rows first: exact .5 ties of the mean at a natural 8-bit scale,
saturated 16-bit rows (variance >= 2^37 from C = 192 on: ADVICE.md's binade) and a row whose int32 squares wrap -- and every row
selection and both output forms are launches over that one buffer: 1 and 3 rows, B = 2 with (T_all, t0, T) = (197, 1, 196),
(7, 1, 6), (50, 0, 1); channel-major at T = 6, 49, 144, 196 (tails of the 16-token runs, runs that end at an image boundary).
Then every entry with ldx > C into ldo > C between fences, and the header's preconditions as refusals that write nothing."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import ibert as ib
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
from ivit_amd.engine_common import IBERT_LN_INT_SQRT as ISQ, LN_F32_CHANNEL_MAJOR as CM, LN_F32_FAST_DIV as FAST  # noqa: E402
from ivit_amd.prepare import markstein_division_ok, phi_tables  # noqa: E402

import fenced  # noqa: E402
import ibert_intsqrt_ref as iref  # noqa: E402

DEV = "cuda:0"
f32 = np.float32
N_ROWS = 2 * 197
ROW_SELECTIONS = [(1, 1, 0, 1), (1, 3, 0, 3), (2, 197, 1, 196), (2, 7, 1, 6), (2, 50, 0, 1)]
CM_SELECTIONS = [(2, 7, 1, 6), (2, 50, 1, 49), (2, 197, 3, 144), (2, 197, 1, 196)]
S8 = {"pow2": f32(2.0 ** -4), "natural": f32(0.0371)}
S16 = {"pow2": f32(2.0 ** -9), "natural": f32(1.37e-4)}


def st():
    return _lib.stream_ptr()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def p(t):
    return _lib.ptr(t)


def fbits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.int32)


# ---------------------------------------------------------------------------------------------------------------- rows
def rows_i8(C, seed):
    rng = np.random.default_rng(seed)
    sig = rng.uniform(0.5, 60.0, (N_ROWS, 1))
    k = np.clip(np.rint(rng.normal(rng.normal(0, 20, (N_ROWS, 1)), sig, (N_ROWS, C))), -128, 127).astype(np.int64)
    for r in range(12):      # exact .5 ties of the mean: sum q == C * m + C / 2 (C is even)
        target = C * int(rng.integers(-20, 20)) + C // 2
        row = k[r]
        while row.sum() != target:
            i = int(rng.integers(0, C))
            step = int(np.clip(target - row.sum(), -100, 100))
            row[i] = np.clip(row[i] + step, -128, 127)
        assert (2 * row.sum() - C) % (2 * C) == 0
    k[12] = np.where(np.arange(C) % 2 == 0, 127, -128)      # the largest variance 8-bit rows reach
    k[13] = 5                                                # (a constant row: the Newton iteration on variance 0)
    k[13, 0] = 6
    return k.astype(np.int8)


def rows_i16(C, seed, sigma=None):
    rng = np.random.default_rng(seed)
    sig = rng.uniform(5.0, 6000.0, (N_ROWS, 1)) if sigma is None else sigma
    k = np.clip(np.rint(rng.normal(rng.normal(0, 200, (N_ROWS, 1)), sig, (N_ROWS, C))), -32768, 32767).astype(np.int64)
    if sigma is None:
        alt = np.where(np.arange(C) % 2 == 0, 32767, -32768)
        k[0] = alt                                           # saturated: variance C * 2^30
        k[1] = alt
        k[1, : C // 8] = rng.integers(-3000, 3000, C // 8)
        k[2] = np.where(rng.random(C) < 0.5, 32767, -32767)
        k[3] = 20000                                         # |mean| >= 13 573 and elements at the opposite rail: int32 squares wrap
        k[3, :: 7] = -32768
        k[4] = 32767                                         # |sum| >= 2^24 from C = 513 on: the float32 mean in torch's order
        k[4, :: 5] = 32001
    return k.astype(np.int16)


# ---------------------------------------------------------------------------------------------------------------- references
class Case:
    """one (kind, C, scale): rows, constants on the device, the reference (a) over all rows and the agreement of (b) with it"""

    def __init__(self, kind, C, scale, isq=False, fast=False):
        self.kind, self.C, self.isq, self.fast = kind, C, isq, fast
        bits = 16 if "16" in kind else 8
        ibert = kind.startswith("ibert")
        rng = np.random.default_rng(C + bits)
        self.gamma = gamma = rng.uniform(0.5, 1.5, C).astype(f32)
        self.beta = beta = rng.normal(0, 0.3, C).astype(f32)
        self.s_in = s_in = (S16 if bits == 16 else S8)[scale]
        self.natural = scale == "natural"
        self.shift_pow2 = 4.0 if ibert and bits == 16 else 1.0
        if bits == 8:
            self.k = rows_i8(C, C)
        else:
            self.k = rows_i16(C, C, sigma=300.0 if ibert else None)
        if ibert:
            self.bias, self.s = ib.layernorm_constants(gamma, beta)
        else:
            _, self.s, self.bias = orc.layernorm(self.k[:1].astype(np.int32), gamma, beta)
        self.d_k, self.d_bias, self.d_s = dev(self.k), dev(self.bias), dev(self.s)
        self.tabs = None
        if kind == "i8_compat":
            remap, phi = phi_tables(float(s_in))
            self.tabs = (dev(remap), dev(phi))
        if fast:
            assert markstein_division_ok(float(s_in), 16)
        self.ref = self.reference_entry()
        want = self.reference_oracle()
        if want is not None:
            rows = np.isfinite(want).all(axis=1)
            assert rows.sum() >= N_ROWS * 3 // 4
            bad = (fbits(self.ref)[rows] != fbits(want)[rows]).any(axis=1)
            assert not bad.any(), f"(a) and (b) differ on {int(bad.sum())} rows, first {int(np.argmax(bad))}"

    def reference_entry(self):
        """(a): the pinned module-level entries"""
        C, k = self.C, self.k
        out = torch.empty(N_ROWS, C, dtype=torch.float32, device=DEV)
        s_vec = dev(np.array([self.s_in], f32))
        xf = dev((k.astype(f32) * self.s_in).astype(f32))
        flags = ISQ if self.isq else 0
        if self.kind in ("i8", "i16"):
            _lib.call("ivit_layernorm_i32_f32", p(dev(k.astype(np.int32))), C, N_ROWS, C, p(self.d_bias), p(self.d_s), p(out), C, st())
        elif self.kind in ("i8_compat", "i16_compat"):
            _lib.call("ivit_layernorm_f32_f32_ex", p(xf), C, N_ROWS, C, p(s_vec), 1, p(self.d_bias), p(self.d_s), p(out), C, 0, st())
        elif not self.natural:
            _lib.call("ivit_ibert_layernorm_i32_f32_ex", p(dev(k.astype(np.int32))), C, N_ROWS, C, p(self.d_bias), p(self.d_s),
                      float(self.shift_pow2), p(out), C, flags, st())
            lit = torch.empty_like(out)
            _lib.call("ivit_ibert_layernorm_f32_f32_ex", p(xf), C, N_ROWS, C, p(s_vec), 1, p(self.d_bias), p(self.d_s),
                      float(self.shift_pow2), p(lit), C, flags, st())
            assert torch.equal(out.view(torch.int32), lit.view(torch.int32)), "the two pinned I-BERT entries disagree at a power-of-two scale"
        else:
            _lib.call("ivit_ibert_layernorm_f32_f32_ex", p(xf), C, N_ROWS, C, p(s_vec), 1, p(self.d_bias), p(self.d_s),
                      float(self.shift_pow2), p(out), C, flags, st())
        return out.cpu().numpy()

    def reference_oracle(self):
        """(b): the oracle, [N_ROWS, C] float32 (NaN rows: outside what this restatement decides)"""
        k, g, b = self.k.astype(np.int32), self.gamma, self.beta
        if self.kind in ("i8", "i16"):
            y, s_ln, _ = orc.layernorm(k, g, b)
        elif self.kind == "i8_compat":
            y, s_ln, _, ties = orc.layernorm_compat(k, self.s_in, g, b)
            assert ties >= 12
        elif self.kind == "i16_compat":
            y, s_ln, _ = orc.layernorm_scaled(k, self.s_in, g, b)
        else:
            x_int = iref.x_int_of(k, self.s_in)
            want = iref.layernorm(x_int, self.bias, self.s, self.shift_pow2, int_sqrt=self.isq)
            sx = np.abs(x_int.astype(np.float64).sum(-1))
            mean = np.rint((x_int.astype(np.float64).sum(-1, keepdims=True).astype(f32) / f32(self.C)).astype(f32))
            ys = np.floor(((x_int - mean).astype(f32) / f32(self.shift_pow2)).astype(f32)).astype(np.float64)
            exact = (sx < 2 ** 24) & ((ys * ys).sum(-1) < 2 ** 24)
            if self.natural:      # an exact .5 tie of the integer mean: the float32 order of the phi values decides it, (a) alone pins it
                frac = k.sum(-1) / self.C
                exact &= np.abs(frac - np.floor(frac) - 0.5) > 1e-3
            assert exact.sum() >= N_ROWS * 3 // 4      # (at C = 32 one random row in 32 is a tie too)
            want[~exact] = np.nan
            if not self.isq:      # oracle/ibert.py::layernorm, the same rows
                y, s_out, _ = ib.layernorm(k, self.s_in, g, b, shift=float(np.log2(self.shift_pow2)))
                w2 = (y * s_out).astype(f32)
                assert np.array_equal(fbits(w2)[exact], fbits(want)[exact])
            return want
        return (y * s_ln).astype(f32)

    def launch(self, sel, out_ptr, ldo, cm, x_ptr=None, ldx=None):
        B, T_all, t0, T = sel
        C = self.C
        x_ptr = p(self.d_k) if x_ptr is None else x_ptr
        ldx = C if ldx is None else ldx
        flags = (CM if cm else 0)
        if self.kind in ("i8", "i8_compat"):
            r, ph = (None, None) if self.tabs is None else (p(self.tabs[0]), p(self.tabs[1]))
            _lib.call("ivit_layernorm_i8_f32", x_ptr, ldx, B, T_all, t0, T, C, p(self.d_bias), p(self.d_s), r, ph, out_ptr, ldo, flags, st())
        elif self.kind in ("i16", "i16_compat"):
            _lib.call("ivit_layernorm_i16_f32", x_ptr, ldx, B, T_all, t0, T, C, float(self.s_in) if self.kind == "i16_compat" else 0.0,
                      p(self.d_bias), p(self.d_s), out_ptr, ldo, flags | (FAST if self.fast else 0), st())
        elif self.kind == "ibert_i8":
            _lib.call("ivit_ibert_layernorm_i8_f32", x_ptr, ldx, B, T_all, t0, T, C, float(self.s_in), p(self.d_bias), p(self.d_s),
                      float(self.shift_pow2), out_ptr, ldo, flags | (ISQ if self.isq else 0), st())
        else:
            _lib.call("ivit_ibert_layernorm_i16_f32", x_ptr, ldx, B, T_all, t0, T, C, float(self.s_in), p(self.d_bias), p(self.d_s),
                      float(self.shift_pow2), out_ptr, ldo, flags | (ISQ if self.isq else 0) | (FAST if self.fast else 0), st())

    def expected(self, sel, cm):
        B, T_all, t0, T = sel
        e = self.ref[: B * T_all].reshape(B, T_all, self.C)[:, t0:t0 + T]
        return np.ascontiguousarray(e.transpose(0, 2, 1) if cm else e)


def sweep(case):
    for cm, sels in ((False, ROW_SELECTIONS), (True, CM_SELECTIONS)):
        for sel in sels:
            exp = case.expected(sel, cm)
            out = torch.full(exp.shape, float("nan"), dtype=torch.float32, device=DEV)
            case.launch(sel, p(out), sel[3] if cm else case.C, cm)
            got = out.cpu().numpy()
            bad = fbits(got) != fbits(exp)
            assert not bad.any(), f"{'channel-major' if cm else 'rows'} {sel}: {int(bad.sum())} elements differ, first {tuple(np.argwhere(bad)[0])}"


CS8 = [32, 96, 192, 768, 1024]
CS16 = CS8 + [1536]


@pytest.mark.parametrize("scale", ["pow2", "natural"])
@pytest.mark.parametrize("C", CS8)
def test_layernorm_i8_f32(C, scale):
    sweep(Case("i8" if scale == "pow2" else "i8_compat", C, scale))


@pytest.mark.parametrize("scale,fast", [("pow2", False), ("natural", False), ("natural", True)])
@pytest.mark.parametrize("C", CS16)
def test_layernorm_i16_f32(C, scale, fast):
    if fast and not markstein_division_ok(float(S16[scale]), 16):
        pytest.fail("the natural 16-bit scale of this file must admit the Markstein quotient")
    sweep(Case("i16" if scale == "pow2" else "i16_compat", C, scale, fast=fast))


@pytest.mark.parametrize("isq", [False, True], ids=["sqrt", "int_sqrt"])
@pytest.mark.parametrize("scale", ["pow2", "natural"])
@pytest.mark.parametrize("C", CS8)
def test_ibert_layernorm_i8_f32(C, scale, isq):
    sweep(Case("ibert_i8", C, scale, isq=isq))


@pytest.mark.parametrize("fast", [False, True], ids=["division", "markstein"])
@pytest.mark.parametrize("isq", [False, True], ids=["sqrt", "int_sqrt"])
@pytest.mark.parametrize("scale", ["pow2", "natural"])
@pytest.mark.parametrize("C", CS16)
def test_ibert_layernorm_i16_f32(C, scale, isq, fast):
    sweep(Case("ibert_i16", C, scale, isq=isq, fast=fast))


# ---------------------------------------------------------------------------------------------------------------- strides
def _fenced_pair(case, sel, cm, lead_in=0):
    """the case's rows with ldx > C between poisoned pads; the output with ldo > width between sentinels"""
    B, T_all, t0, T = sel
    C = case.C
    item = case.k.itemsize
    src = case.k[: B * T_all]
    x = fenced.input(src, C + 12 // item * item, fenced.POISON[src.dtype], lead_bytes=lead_in, device=DEV)
    exp = case.expected(sel, cm)
    exp2 = exp.reshape(-1, exp.shape[-1])
    o = fenced.output(exp2.shape[0], exp2.shape[1], exp2.shape[1] + 5, np.float32, expected=exp2, device=DEV)
    return x, o, exp2


@pytest.mark.parametrize("cm", [False, True], ids=["rows", "channel_major"])
def test_layernorm_i8_f32_fenced(cm):
    for kind, scale in (("i8", "pow2"), ("i8_compat", "natural")):
        case = Case(kind, 96, scale)
        sel = (2, 50, 1, 49)
        x, o, exp = _fenced_pair(case, sel, cm)
        B, T_all, t0, T = sel
        r, ph = (None, None) if case.tabs is None else (p(case.tabs[0]), p(case.tabs[1]))
        _lib.call("ivit_layernorm_i8_f32", x.ptr, x.ld, B, T_all, t0, T, case.C, p(case.d_bias), p(case.d_s), r, ph, o.ptr, o.ld,
                  CM if cm else 0, st())
        fenced.check(o, exp)
        fenced.check(x)


@pytest.mark.parametrize("cm", [False, True], ids=["rows", "channel_major"])
def test_layernorm_i16_f32_fenced(cm):
    for kind, scale, fast in (("i16", "pow2", False), ("i16_compat", "natural", True)):
        case = Case(kind, 100, scale, fast=fast)
        sel = (2, 50, 1, 49)
        x, o, exp = _fenced_pair(case, sel, cm, lead_in=2)
        B, T_all, t0, T = sel
        _lib.call("ivit_layernorm_i16_f32", x.ptr, x.ld, B, T_all, t0, T, case.C, float(case.s_in) if fast else 0.0, p(case.d_bias),
                  p(case.d_s), o.ptr, o.ld, (CM if cm else 0) | (FAST if fast else 0), st())
        fenced.check(o, exp)
        fenced.check(x)


@pytest.mark.parametrize("cm", [False, True], ids=["rows", "channel_major"])
def test_ibert_layernorm_i8_f32_fenced(cm):
    case = Case("ibert_i8", 100, "natural", isq=True)
    sel = (2, 50, 1, 49)
    x, o, exp = _fenced_pair(case, sel, cm, lead_in=1)
    B, T_all, t0, T = sel
    _lib.call("ivit_ibert_layernorm_i8_f32", x.ptr, x.ld, B, T_all, t0, T, case.C, float(case.s_in), p(case.d_bias), p(case.d_s),
              float(case.shift_pow2), o.ptr, o.ld, (CM if cm else 0) | ISQ, st())
    fenced.check(o, exp)
    fenced.check(x)


@pytest.mark.parametrize("cm", [False, True], ids=["rows", "channel_major"])
def test_ibert_layernorm_i16_f32_fenced(cm):
    case = Case("ibert_i16", 100, "natural", fast=True)
    sel = (2, 50, 1, 49)
    x, o, exp = _fenced_pair(case, sel, cm, lead_in=2)
    B, T_all, t0, T = sel
    _lib.call("ivit_ibert_layernorm_i16_f32", x.ptr, x.ld, B, T_all, t0, T, case.C, float(case.s_in), p(case.d_bias), p(case.d_s),
              float(case.shift_pow2), o.ptr, o.ld, (CM if cm else 0) | FAST, st())
    fenced.check(o, exp)
    fenced.check(x)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_preconditions_are_refused_and_nothing_is_written():
    L = _lib.lib()
    C = 96
    x8 = torch.zeros(64 * 128, dtype=torch.int8, device=DEV)
    x16 = torch.zeros(64 * 128, dtype=torch.int16, device=DEV)
    tab = torch.ones(4096 + 8, dtype=torch.float32, device=DEV)
    t8 = torch.zeros(256, dtype=torch.int8, device=DEV)
    out = torch.full((64 * 128,), -7.5, dtype=torch.float32, device=DEV)
    V, F, I = ctypes.c_void_p, ctypes.c_float, ctypes.c_int64
    xp, x16p, tp, t8p, op = x8.data_ptr(), x16.data_ptr(), tab.data_ptr(), t8.data_ptr(), out.data_ptr()

    def i8(x=xp, ldx=C, sel=(2, 8, 1, 7), C=C, bias=tp, s=tp, remap=None, phi=None, o=op, ldo=C, flags=0):
        return L.ivit_layernorm_i8_f32(V(x), I(ldx), *sel, C, V(bias), V(s), V(remap), V(phi), V(o), I(ldo), flags, st())

    def i16(x=x16p, ldx=C, sel=(2, 8, 1, 7), C=C, s_in=0.0, o=op, ldo=C, flags=0):
        return L.ivit_layernorm_i16_f32(V(x), I(ldx), *sel, C, F(s_in), V(tp), V(tp), V(o), I(ldo), flags, st())

    def ib8(x=xp, ldx=C, sel=(2, 8, 1, 7), C=C, s_in=0.5, shift=1.0, o=op, ldo=C, flags=0):
        return L.ivit_ibert_layernorm_i8_f32(V(x), I(ldx), *sel, C, F(s_in), V(tp), V(tp), F(shift), V(o), I(ldo), flags, st())

    def ib16(x=x16p, ldx=C, sel=(2, 8, 1, 7), C=C, s_in=0.5, shift=1.0, o=op, ldo=C, flags=0):
        return L.ivit_ibert_layernorm_i16_f32(V(x), I(ldx), *sel, C, F(s_in), V(tp), V(tp), F(shift), V(o), I(ldo), flags, st())

    UNSUPPORTED, INVALID = -2, -1
    refused = [
        # the header's preconditions: IVIT_ERR_UNSUPPORTED
        (i8(C=98, ldx=100, ldo=100), UNSUPPORTED), (i8(ldx=C + 2), UNSUPPORTED), (i8(x=xp + 2), UNSUPPORTED),
        (i8(bias=tp + 4), UNSUPPORTED), (i8(s=tp + 8), UNSUPPORTED),
        (i8(C=24, ldx=24, ldo=24, remap=t8p, phi=tp), UNSUPPORTED), (i8(C=100, ldx=100, ldo=100, remap=t8p, phi=tp), UNSUPPORTED),
        (i8(C=4100, ldx=4100, ldo=4100, sel=(1, 1, 0, 1)), UNSUPPORTED), (i16(C=4098, ldx=4098, ldo=4098, sel=(1, 1, 0, 1)), UNSUPPORTED),
        (ib8(C=4097, ldx=4097, ldo=4097, sel=(1, 1, 0, 1)), UNSUPPORTED), (ib16(C=5000, ldx=5000, ldo=5000, sel=(1, 1, 0, 1)), UNSUPPORTED),
        # bad operands: IVIT_ERR_INVALID
        (i8(x=None), INVALID), (i8(o=None), INVALID), (i8(remap=t8p), INVALID), (i8(ldx=C - 4), INVALID), (i8(ldo=C - 1), INVALID),
        (i8(sel=(2, 8, 2, 7)), INVALID), (i8(sel=(0, 8, 1, 7)), INVALID), (i8(sel=(2, 8, -1, 7)), INVALID), (i8(flags=4), INVALID),
        (i8(flags=CM, ldo=6), INVALID), (i8(o=op + 2), INVALID),
        (i16(x=x16p + 1), INVALID), (i16(flags=FAST), INVALID), (i16(s_in=-1.0), INVALID), (i16(flags=ISQ), INVALID),
        (ib8(s_in=0.0), INVALID), (ib8(shift=0.5), INVALID), (ib8(flags=FAST), INVALID), (ib8(flags=8), INVALID),
        (ib16(x=x16p + 1), INVALID), (ib16(shift=0.25), INVALID), (ib16(ldx=C - 1), INVALID),
    ]
    for i, (rc, want) in enumerate(refused):
        assert rc == want, f"refusal {i}: {rc}, expected {want}"
    assert "ivit_ibert_layernorm_i16_f32" in L.ivit_last_error_string().decode()
    torch.cuda.synchronize()
    assert bool((out == -7.5).all()), "a refused call wrote"
    assert i8() == 0 and i16() == 0 and ib8() == 0 and ib16() == 0      # (the same arguments without the fault are taken)
