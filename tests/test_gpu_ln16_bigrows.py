"""16-bit I-LayerNorm rows whose float32 sum reaches 2^24, whose int32 squares wrap, or whose variance lies at the edge of the Newton
shortcut: every entry and kernel form that takes such rows, byte for byte against the outputs of the reference module + its 8-bit
QuantAct (tests/golden/ln16_bigrows_kat.npz; the classes are those of tests/ln16_order_ref.py, the host side is
tests/test_ln16_bigrows_cpu.py).  Outputs are fenced (tests/fenced.py).  Rows of all classes share a launch, in a seeded order, so
that the wave-uniform branches run with neighbours on the other side; each class also runs alone in a launch of 1..5 rows.

Forms:  ivit_layernorm_i16_i8          tiled (C 768 / 776 / 1024 / 1536), wave per row (C 772 / 2048, and C 768 through an ldo that the
                                       tiled form refuses), window-order output
        ivit_layernorm_i16_i8_compat   fast_division 0 (literal, wave per row) and 1 (tiled where C allows), both scales
        ivit_layernorm_i32_f32, ivit_layernorm_f32_f32 / _ex    the float outputs, taken through the same QuantAct on the host
        IVITIntLayerNorm + QuantAct    the module path carrying int16
Class (v): the tiled forms take ln16_std10's shortcut or its literal loop, the wave-per-row forms always run the ten literal steps;
both are compared with the reference's bytes (the lab build has no knob that forces the loop in the 16-bit kernels); launches that hold
only the rows just outside the band pin the shortcut where a wave holds several rows.  Rows whose wrapped variance sum is zero or
less (outside the reference's domain) are checked for what they must not touch."""
import os

import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
from ivit_amd.prepare import LayerNormParams, markstein_division_ok, sym_scale  # noqa: E402
import fenced  # noqa: E402
import ln16_order_ref as lno  # noqa: E402

DEV = "cuda:0"
f32 = np.float32
_KEEP = []
WIDTHS = lno.TILED_C + lno.OTHER_C


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    _KEEP.append(t)
    return t


@pytest.fixture(autouse=True)
def _release_device_tensors():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def st():
    return _lib.stream_ptr()


@pytest.fixture(scope="module")
def kat(golden_dir):
    return np.load(os.path.join(golden_dir, "ln16_bigrows_kat.npz"))


_GROUPS = {}


def group(kat, C, si):
    """the rows of one width and scale in a seeded order that mixes the classes -> dict (cached: the fixture is read once)"""
    if (C, si) not in _GROUPS:
        key = f"{C}_{si}"
        order = np.random.default_rng(C + si).permutation(len(kat[f"q_{key}"]))
        hi = float(kat["ranges"][si])
        lp = LayerNormParams(kat[f"gamma_{C}"], kat[f"beta_{C}"], sym_scale(-hi, hi, 8))
        _GROUPS[(C, si)] = dict(q=np.ascontiguousarray(kat[f"q_{key}"][order]), ref=np.ascontiguousarray(kat[f"ref_{key}"][order]),
                                cls=kat[f"cls_{key}"][order].astype(np.int64), vkind=kat[f"vkind_{key}"][order], s=f32(kat["scales"][si]), hi=hi, lp=lp, C=C,
                                gamma=kat[f"gamma_{C}"], beta=kat[f"beta_{C}"])
    return _GROUPS[(C, si)]


def tables(lp):
    return (_lib.ptr(dev(lp.bias_int)), _lib.ptr(dev(lp.s_ln)), _lib.ptr(dev(lp.m.view(np.int32))), _lib.ptr(dev(lp.e)))


def compare(name, got, ref, cls):
    """print how many rows of each class differ, then assert that none does"""
    bad = np.any(np.asarray(got) != ref, axis=1)
    per = {lno.CLASS_NAMES[c]: f"{int(bad[cls == c].sum())}/{int((cls == c).sum())}" for c in lno.CLASS_NAMES if (cls == c).any()}
    print(f"{name}: rows that differ from the reference, per class: {per}")
    assert not bad.any(), f"{name}: {int(bad.sum())} of {len(bad)} rows differ from the reference's bytes, per class {per}"


def run_i16(g, idx, ldo, geo=(0, 0, 0, 0), compat=None, expected=None):
    """ivit_layernorm_i16_i8 (compat=None) or ivit_layernorm_i16_i8_compat (compat = fast_division) on the rows idx of the group into a
    fenced int8 output -> (the fenced buffer, its data)"""
    q, C = g["q"][idx], g["C"]
    exp = g["ref"][idx] if expected is None else expected
    o = fenced.output(len(q), C, ldo, np.int8, expected=exp)
    if compat is None:
        _lib.call("ivit_layernorm_i16_i8", _lib.ptr(dev(q)), len(q), C, *tables(g["lp"]), o.ptr, o.ld, *geo, st())
    else:
        _lib.call("ivit_layernorm_i16_i8_compat", _lib.ptr(dev(q)), len(q), C, float(g["s"]), compat, *tables(g["lp"]), o.ptr, o.ld, *geo, st())
    torch.cuda.synchronize()
    return o, o.rows2d(o.fetch())[:, :C].copy()


@pytest.mark.parametrize("C", WIDTHS)
def test_pow2_entry_all_classes_in_one_launch(kat, C):
    """the tiled kernel (C 768 .. 1536) and the wave-per-row kernel (772, 2048); ldo = C + 8 keeps the tiled form"""
    g = group(kat, C, 0)
    idx = np.arange(len(g["q"]))
    o, got = run_i16(g, idx, C + 8)
    compare(f"ivit_layernorm_i16_i8 C={C}", got, g["ref"], g["cls"])
    fenced.check(o, g["ref"])


@pytest.mark.parametrize("C", [768, 1536])
def test_pow2_wave_per_row_kernel_through_a_refused_ldo(kat, C):
    """ldo = C + 5 is no multiple of 8: ln16_tiling refuses it and the wave-per-row kernel runs at a tiled width"""
    g = group(kat, C, 0)
    o, got = run_i16(g, np.arange(len(g["q"])), C + 5)
    compare(f"ivit_layernorm_i16_i8 C={C} ldo=C+5", got, g["ref"], g["cls"])
    fenced.check(o, g["ref"])


def test_pow2_window_order_output(kat):
    """the row map on the output (H, W, ws, shift): 48 rows = 3 images of 4 x 4 tokens, windows of 2, shift 1, permuted as
    tests/test_gpu_swin.py test_layernorm_i16_i8_window_order does"""
    C, B, H, ws, shift = 768, 3, 4, 2, 1
    g = group(kat, C, 0)
    rows = B * H * H
    pick = np.concatenate([np.flatnonzero(np.isin(g["cls"], (lno.CLASS_C, lno.CLASS_W))), np.flatnonzero(~np.isin(g["cls"], (lno.CLASS_C, lno.CLASS_W)))])
    idx = np.sort(pick[:rows])
    assert np.isin(g["cls"][idx], (lno.CLASS_C,)).sum() >= 8 and (g["cls"][idx] == lno.CLASS_W).sum() >= 8
    exp = orc._win_partition(np.roll(g["ref"][idx].reshape(B, H, H, C), (-shift, -shift), axis=(1, 2)), ws).reshape(rows, C)
    o, got = run_i16(g, idx, C, geo=(H, H, ws, shift), expected=exp)
    # the classes of the output rows: the same permutation on the row classes
    cls = orc._win_partition(np.roll(g["cls"][idx].reshape(B, H, H, 1), (-shift, -shift), axis=(1, 2)), ws).reshape(rows)
    compare("ivit_layernorm_i16_i8 window order", got, exp, cls)
    fenced.check(o, exp)


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("si", [0, 1])
@pytest.mark.parametrize("C", WIDTHS)
def test_compat_entry_all_classes_in_one_launch(kat, C, si, fast):
    """fast_division 0: the literal wave-per-row kernel; 1: the tiled kernel with the three-instruction quotient where ln16_tiling takes C"""
    g = group(kat, C, si)
    assert markstein_division_ok(g["s"], 16)
    o, got = run_i16(g, np.arange(len(g["q"])), C + 8, compat=fast)
    compare(f"ivit_layernorm_i16_i8_compat C={C} s={float(g['s']):.6g} fast={fast}", got, g["ref"], g["cls"])
    fenced.check(o, g["ref"])


def quantact_of_float(x, g):
    """the 8-bit QuantAct of the fixture on a float LayerNorm output x = y * s_ln (quant_utils.py:220, :229-230)"""
    lp = g["lp"]
    z = np.rint((x / lp.s_ln).astype(f32)).astype(f32)
    m, e = orc.dyadic(lp.s_ln, sym_scale(-g["hi"], g["hi"], 8))
    return orc.requant(z, m, e, 8).astype(np.int8)


def launch_float(entry, g, q, o):
    """ivit_layernorm_i32_f32 on the integers q, or ivit_layernorm_f32_f32 / _ex (outer = 0) on the float view q * s, into the fenced o"""
    C, lp = g["C"], g["lp"]
    if entry == "ivit_layernorm_i32_f32":
        _lib.call(entry, _lib.ptr(dev(q.astype(np.int32))), C, len(q), C, _lib.ptr(dev(lp.bias_int)), _lib.ptr(dev(lp.s_ln)), o.ptr, o.ld, st())
    else:
        x = (q.astype(f32) * g["s"]).astype(f32)
        args = [_lib.ptr(dev(x)), C, len(q), C, _lib.ptr(dev(np.array([g["s"]], f32))), 1, _lib.ptr(dev(lp.bias_int)), _lib.ptr(dev(lp.s_ln)), o.ptr, o.ld]
        if entry.endswith("_ex"):
            args.append(0)
        _lib.call(entry, *args, st())
    torch.cuda.synchronize()


def run_float(entry, g, idx, name):
    """a float-output entry on the rows idx: its output bit for bit against the restatement with torch's order and int32 squares (fenced),
    and through the fixture's QuantAct against the reference's bytes"""
    q, C = g["q"][idx], g["C"]
    r = lno.layernorm(q, g["s"], g["gamma"], g["beta"])
    exp = (r["y"] * r["s_ln"]).astype(f32)
    assert np.array_equal(r["s_ln"], g["lp"].s_ln)
    o = fenced.output(len(q), C, C + 3, np.float32, expected=exp)
    launch_float(entry, g, q, o)
    got = o.rows2d(o.fetch())[:, :C].copy()
    compare(name, quantact_of_float(got, g), g["ref"][idx], g["cls"][idx])
    fenced.check(o, exp)


@pytest.mark.parametrize("C", WIDTHS)
def test_i32_f32_entry(kat, C):
    """ivit_layernorm_i32_f32 on the integers (the power-of-two scale)"""
    g = group(kat, C, 0)
    run_float("ivit_layernorm_i32_f32", g, np.arange(len(g["q"])), f"ivit_layernorm_i32_f32 C={C}")


@pytest.mark.parametrize("entry", ["ivit_layernorm_f32_f32", "ivit_layernorm_f32_f32_ex"])
@pytest.mark.parametrize("si", [0, 1])
@pytest.mark.parametrize("C", [768, 1536, 772, 2048])
def test_literal_float_entries(kat, C, si, entry):
    """csrc/literal.hip on the float view q * s (outer = 0): the module path's literal kernel"""
    g = group(kat, C, si)
    run_float(entry, g, np.arange(len(g["q"])), f"{entry} C={C} s={float(g['s']):.6g}")


ALONE = {lno.CLASS_A: 2, lno.CLASS_B: 2, lno.CLASS_C: 4, lno.CLASS_W: 5, lno.CLASS_V: 3}


@pytest.mark.parametrize("kind", sorted(ALONE), ids=[lno.CLASS_NAMES[k] for k in sorted(ALONE)])
@pytest.mark.parametrize("C", [768, 1536, 2048])
def test_each_class_alone_in_a_small_launch(kat, C, kind):
    """1..5 rows of one class in every entry: each wave-uniform branch with all its rows on one side (and most lanes of the tiled forms
    on clamped rows)"""
    for si, compat in ((0, None), (1, 1), (1, 0)):
        g = group(kat, C, si)
        idx = np.flatnonzero(g["cls"] == kind)[:ALONE[kind]]
        assert len(idx) == ALONE[kind]
        o, got = run_i16(g, idx, C, compat=compat)
        compare(f"class {lno.CLASS_NAMES[kind]} alone, C={C} si={si} compat={compat}", got, g["ref"][idx], g["cls"][idx])
        fenced.check(o, g["ref"][idx])
    for si, entry in ((0, "ivit_layernorm_i32_f32"), (0, "ivit_layernorm_f32_f32"), (1, "ivit_layernorm_f32_f32_ex")):
        g = group(kat, C, si)
        idx = np.flatnonzero(g["cls"] == kind)[:ALONE[kind]]
        run_float(entry, g, idx, f"class {lno.CLASS_NAMES[kind]} alone, {entry} C={C} si={si}")


@pytest.mark.parametrize("side", [lno.V_OUTSIDE, lno.V_INSIDE, None], ids=["outside", "inside", "all"])
@pytest.mark.parametrize("C", lno.TILED_C)
def test_newton_band_rows_by_side(kat, C, side):
    """class (v) by side of ln16_std10's band, in the tiled kernels: the ballot sends a whole wave down the literal loop when one of its
    rows is in the band, so a launch that holds only the rows just OUTSIDE it is what pins the shortcut at the widths with several rows
    per wave (C = 768 / 776 / 1024: two); only the rows INSIDE: the loop; all (v) rows: both, as neighbours"""
    for si, compat in ((0, None), (0, 1), (1, 1)):
        g = group(kat, C, si)
        pick = (g["cls"] == lno.CLASS_V) & ((g["vkind"] == side) if side is not None else True)
        idx = np.flatnonzero(pick)
        assert len(idx) >= 15
        if side is not None:      # what the rule says of these rows is what the fixture says
            slow = lno.std10_rule(lno.layernorm(g["q"][idx], g["s"], g["gamma"], g["beta"])["var"].astype(f32))[0]
            assert slow.all() if side == lno.V_INSIDE else not slow.any()
        o, got = run_i16(g, idx, C, compat=compat)
        compare(f"class v {'all' if side is None else side}, C={C} si={si} compat={compat}", got, g["ref"][idx], g["cls"][idx])
        fenced.check(o, g["ref"][idx])


def degenerate_rows(C, s, n=3):
    """rows whose wrapped variance sum is zero or negative: a tight cluster at a mean of 14 000 or more and one element at the opposite
    rail, whose square wraps to about -2^31.  Outside the reference's domain (its Newton steps divide by zero)"""
    rng = np.random.default_rng(C)
    q = np.empty((n, C), np.int64)
    for i in range(n):
        sg = 1 if i % 2 == 0 else -1
        q[i] = sg * 15000 + rng.integers(-3, 4, size=C)
        q[i, int(rng.integers(0, C))] = -32768 if sg > 0 else 32767
    assert (lno.layernorm(q, s, np.ones(C, f32), np.zeros(C, f32))["var"] <= 0).all()
    return q.astype(np.int16)


@pytest.mark.parametrize("C", [768, 1536, 772])
def test_rows_with_a_wrapped_variance_of_zero_or_less_stay_inside_their_row(kat, C):
    """what such a row stores is not pinned; that nothing else is written is: the rows around it (controls of the fixture) hold the
    reference's bytes, and pads, guards and slack their fill -- every entry"""
    for si in (0, 1):
        g = group(kat, C, si)
        ctl = np.flatnonzero(np.isin(g["cls"], (lno.CLASS_A, lno.CLASS_V)))[:4]
        bad = degenerate_rows(C, g["s"])
        q = np.concatenate([g["q"][ctl[:2]], bad[:2], g["q"][ctl[2:]], bad[2:]])      # controls and degenerate rows as neighbours
        is_ctl = np.array([True, True, False, False, True, True, False])
        ref8 = g["ref"][ctl]
        lp = g["lp"]

        def check(o, exp_ctl, name):
            raw = o.fetch()
            body = fenced._bits(o.rows2d(raw))
            fill = fenced._bits(np.array([o.fill]))[0]
            assert np.array_equal(body[is_ctl][:, :C], fenced._bits(exp_ctl.astype(o.dtype))), f"{name}: a control row next to a degenerate row changed"
            assert (body[:, C:] == fill).all(), f"{name}: pad columns written"
            item = o.dtype.itemsize
            assert (fenced._bits(raw[:o.start // item * item].view(o.dtype)) == fill).all(), f"{name}: guard in front written"
            assert (fenced._bits(raw[o.start + o.body:].view(o.dtype)) == fill).all(), f"{name}: guard or slack behind written"

        forms = [(None, C + 8), (None, C + 5)] if si == 0 else []
        forms += [(0, C + 8), (1, C + 8)]
        for compat, ldo in forms:
            o = fenced.output(len(q), C, ldo, np.int8, sentinel=-86)
            if compat is None:
                _lib.call("ivit_layernorm_i16_i8", _lib.ptr(dev(q)), len(q), C, *tables(lp), o.ptr, o.ld, 0, 0, 0, 0, st())
            else:
                _lib.call("ivit_layernorm_i16_i8_compat", _lib.ptr(dev(q)), len(q), C, float(g["s"]), compat, *tables(lp), o.ptr, o.ld, 0, 0, 0, 0, st())
            torch.cuda.synchronize()
            check(o, ref8, f"i16_i8 C={C} si={si} compat={compat} ldo={ldo}")
        r = lno.layernorm(g["q"][ctl], g["s"], g["gamma"], g["beta"])
        expf = (r["y"] * r["s_ln"]).astype(f32)
        for entry in (("ivit_layernorm_i32_f32",) if si == 0 else ()) + ("ivit_layernorm_f32_f32_ex",):
            o = fenced.output(len(q), C, C + 3, np.float32, sentinel=fenced.SENTINELS[4][0])
            launch_float(entry, g, q, o)
            check(o, expf, f"{entry} C={C} si={si}")


@pytest.mark.parametrize("si", [0, 1])
def test_module_path_carrying_int16(kat, si):
    """IVITIntLayerNorm + QuantAct(8) of the module mirror on an int16-carrying tensor (quantization_utils/lazy.py, as the 16-bit ViT
    configurations reach it): one fused launch, the reference's bytes on the C = 768 rows"""
    import ivit_amd.quantization_utils as qu
    from ivit_amd.quantization_utils import lazy
    C = 768
    g = group(kat, C, si)
    n = len(g["q"])
    ln = qu.IVITIntLayerNorm(C).to(DEV)
    ln.weight.data, ln.bias.data = torch.from_numpy(g["gamma"]).to(DEV), torch.from_numpy(g["beta"]).to(DEV)
    act = qu.QuantAct(8).to(DEV)
    act.x_min.fill_(-g["hi"])
    act.x_max.fill_(g["hi"])
    act.fix()
    qs = lazy.QS.make(g["s"], DEV)
    x = lazy.QT.wrap((1, n, C), DEV, q16=dev(g["q"]).reshape(1, n, C), scale=qs)
    names = []
    orig = _lib.call

    def traced(name, *a):
        names.append(name)
        return orig(name, *a)

    _lib.call = traced
    try:
        with lazy.scope(True), torch.no_grad():
            y, s_ln = ln(x, qs)
            out, s_out = act(y, s_ln)
            assert isinstance(out, lazy.QT) and lazy.int_width(out) == 8
            got = lazy.int_payload(out).reshape(n, C).cpu().numpy()
    finally:
        _lib.call = orig
    assert names == ["ivit_layernorm_i16_i8" if si == 0 else "ivit_layernorm_i16_i8_compat"], names
    assert float(s_out.reshape(-1)[0]) == float(sym_scale(-g["hi"], g["hi"], 8))
    compare(f"IVITIntLayerNorm + QuantAct on int16, s={float(g['s']):.6g}", got, g["ref"], g["cls"])
