"""IBERTIntLayerNorm(use_int_sqrt=True) on the GPU: the device function over the known-answer values, the five entry-point forms and the
module against the reference's operator vectors, and three DeiT-T models against the reference's logits.

Expected values: tests/ibert_intsqrt_ref.py (numpy, op for op), which tests/test_ibert_intsqrt_cpu.py and the generator hold to the
reference's own outputs; the float outputs of the module are also compared with the reference's row digests directly.  Every element
is compared; nothing is excluded, so there is no tolerance.  (A constant row has std = 0: factor = inf and 0 * inf = NaN in the
reference; NaNs are compared by position, not by payload.)"""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib, synth  # noqa: E402
from ivit_amd.checkpoint import load_synthetic_model  # noqa: E402
from ivit_amd.engine_common import IBERT_LN_INT_SQRT as FLAG  # noqa: E402
from ivit_amd.prepare import LayerNormParams, markstein_division_ok  # noqa: E402
import ivit_amd.quantization_utils as q  # noqa: E402

import ibert_intsqrt_ref as R  # noqa: E402

DEV = "cuda:0"
ISQRT = "ibert_use-int-sqrt_true"
S_NEXT = np.float32(3.1 / 127)           # scale of the QuantAct behind the LayerNorm (the int8 / int16 -> int8 forms)
f32 = np.float32


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def canon(y):
    """float32 -> int32 bits, every NaN as one value"""
    y = np.ascontiguousarray(y, f32)
    return np.where(np.isnan(y), np.int32(0x7FC00000), y.view(np.int32))


@pytest.fixture(scope="module")
def ops(golden_dir):
    return np.load(os.path.join(golden_dir, "ibert_intsqrt_ops.npz"))


@functools.lru_cache(maxsize=None)
def expected(case):
    """-> the case, its constants and the restatement's outputs with and without use_int_sqrt (float, and int8 behind the QuantAct)"""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ibert_intsqrt_ops.npz"))
    d, key = R.make_case(case), R.case_key(case)
    bias_int, s_out = R.layernorm_constants(d["gamma"], d["beta"])
    lp = LayerNormParams(d["gamma"], d["beta"], float(S_NEXT))
    assert np.array_equal(lp.bias_int, bias_int) and np.array_equal(lp.s_ln, s_out)
    M = lp.m.astype(np.float64) * np.exp2(-lp.e.astype(np.float64))
    x_int = R.x_int_of(d["q"], d["s_in"])
    out = dict(d, key=key, bias_int=bias_int, s_out=s_out, lp=lp)
    for name, flag in (("y", True), ("y0", False)):
        y = R.layernorm(x_int, bias_int, s_out, d["shift_pow2"], mean_int=z[key + "/mean_int"].reshape(-1, 1),
                        var_int=z[key + "/var_int"].reshape(-1, 1), int_sqrt=flag)
        with np.errstate(invalid="ignore"):
            zq = np.rint((y / s_out).astype(f32))                                           # QuantAct: quant_utils.py:220
            r = np.fmin(np.fmax(np.rint(zq.astype(np.float64) * M), -128.0), 127.0)         # :229-245 (a NaN leaves the clamp as -128)
        out[name], out[name + "_i8"] = y, r.astype(np.int8)
    assert np.array_equal(R.row_crcs(out["y"]), z[key + "/row_crc32"]), key                 # the reference's rows
    assert (out["y"][1:] != out["y0"][1:]).any() and np.isnan(out["y"][0]).all()
    out["var_int"] = z[key + "/var_int"]
    return out


def cases_of(C, name):
    return [c for c in R.CASES if c[0] == C and c[1] == name]


# ------------------------------------------------------------------------------------------------------------ the device function
def test_lab_hook_equals_the_reference_on_the_whole_kat(golden_dir):
    z = np.load(os.path.join(golden_dir, "ibert_intsqrt_kat.npz"))
    n = t(z["n"])
    out = torch.full((n.numel() + 8,), -7, dtype=torch.int32, device=DEV)
    with _lib.lab_session() as L:
        assert L.ivit_debug_ibert_integer_sqrt(_lib.ptr(n), n.numel(), _lib.ptr(out), _lib.stream_ptr()) == 0
    got = out.cpu().numpy()
    bad = np.nonzero(got[:-8] != z["isqrt"])[0]
    assert bad.size == 0, (bad.size, z["n"][bad[:5]], got[bad[:5]], z["isqrt"][bad[:5]])
    assert (got[-8:] == -7).all()


# ------------------------------------------------------------------------------------------------------------ the entry points
def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("name", list(R.SETS))
@pytest.mark.parametrize("C", [192, 384, 768, 1024])
def test_literal_entry_f32(C, name):
    """ivit_ibert_layernorm_f32_f32_ex on the float view q * s_in, with the flag, with flags = 0, and the entry without `flags`"""
    for case in cases_of(C, name):
        e = expected(case)
        x = t((e["q"].astype(f32) * e["s_in"]).astype(f32))
        s, b, so = t(np.array([e["s_in"]], f32)), t(e["bias_int"]), t(e["s_out"])
        outs = []
        for entry, extra in (("ivit_ibert_layernorm_f32_f32_ex", (FLAG,)), ("ivit_ibert_layernorm_f32_f32_ex", (0,)), ("ivit_ibert_layernorm_f32_f32", ())):
            out = torch.full((R.ROWS, C), 7.0, dtype=torch.float32, device=DEV)
            _lib.call(entry, _lib.ptr(x), C, R.ROWS, C, _lib.ptr(s), 1, _lib.ptr(b), _lib.ptr(so), e["shift_pow2"], _lib.ptr(out), C,
                      *extra, _lib.stream_ptr())
            outs.append(out.cpu().numpy())
        _same(canon(outs[0]), canon(e["y"]), e["key"])
        _same(canon(outs[1]), canon(e["y0"]), e["key"] + " flags=0")
        _same(canon(outs[2]), canon(e["y0"]), e["key"] + " plain entry")
    with pytest.raises(_lib.IvitError, match="flags"):
        _lib.call("ivit_ibert_layernorm_f32_f32_ex", _lib.ptr(x), C, R.ROWS, C, _lib.ptr(s), 1, _lib.ptr(b), _lib.ptr(so), 1.0, _lib.ptr(out), C,
                  FLAG | 1, _lib.stream_ptr())


@pytest.mark.parametrize("name", list(R.SETS))
@pytest.mark.parametrize("C", [192, 384, 768, 1024])
def test_integer_entry_i32(C, name):
    """ivit_ibert_layernorm_i32_f32_ex on the integers k: the literal form at every power-of-two scale"""
    for case in cases_of(C, name):
        if case[3] != 0:
            continue
        e = expected(case)
        k, b, so = t(e["q"].astype(np.int32)), t(e["bias_int"]), t(e["s_out"])
        outs = []
        for entry, extra in (("ivit_ibert_layernorm_i32_f32_ex", (FLAG,)), ("ivit_ibert_layernorm_i32_f32_ex", (0,)), ("ivit_ibert_layernorm_i32_f32", ())):
            out = torch.full((R.ROWS, C), 7.0, dtype=torch.float32, device=DEV)
            _lib.call(entry, _lib.ptr(k), C, R.ROWS, C, _lib.ptr(b), _lib.ptr(so), e["shift_pow2"], _lib.ptr(out), C, *extra, _lib.stream_ptr())
            outs.append(out.cpu().numpy())
        _same(canon(outs[0]), canon(e["y"]), e["key"])
        _same(canon(outs[1]), canon(e["y0"]), e["key"] + " flags=0")
        _same(canon(outs[2]), canon(e["y0"]), e["key"] + " plain entry")
    with pytest.raises(_lib.IvitError, match="flags"):
        _lib.call("ivit_ibert_layernorm_i32_f32_ex", _lib.ptr(k), C, R.ROWS, C, _lib.ptr(b), _lib.ptr(so), 1.0, _lib.ptr(out), C, 2, _lib.stream_ptr())


@pytest.mark.parametrize("name", ["q8", "q8max"])
@pytest.mark.parametrize("C", [192, 384, 768, 1024])
def test_engine_entry_i8(C, name):
    """ivit_ibert_layernorm_i8 (the fast kernel: std from the exact integer sum below 2^24) + QuantAct, row-major and block layout"""
    for case in cases_of(C, name):
        e = expected(case)
        lp = e["lp"]
        x, b, so = t(e["q"].astype(np.int8)), t(e["bias_int"]), t(e["s_out"])
        m, ex = t(lp.m.view(np.int32)), t(lp.e)
        got = {}
        for flags in (FLAG, 0, FLAG | 1, 1):
            out = torch.full((R.ROWS + 15, C), 7, dtype=torch.int8, device=DEV)
            _lib.call("ivit_ibert_layernorm_i8", _lib.ptr(x), C, R.ROWS, C, float(e["s_in"]), _lib.ptr(b), _lib.ptr(so), e["shift_pow2"],
                      _lib.ptr(m), _lib.ptr(ex), _lib.ptr(out), C, flags, _lib.stream_ptr())
            got[flags] = out
        _same(got[FLAG][:R.ROWS].cpu().numpy(), e["y_i8"], e["key"])
        _same(got[0][:R.ROWS].cpu().numpy(), e["y0_i8"], e["key"] + " without the flag")
        assert (got[FLAG][R.ROWS:] == 7).all()
        blocks = _blocks_to_rows(got[FLAG | 1], R.ROWS, C), _blocks_to_rows(got[1], R.ROWS, C)
        _same(blocks[0], e["y_i8"], e["key"] + " block layout")
        _same(blocks[1], e["y0_i8"], e["key"] + " block layout without the flag")


def _blocks_to_rows(buf, rows, C):
    """IVIT_LAYOUT_BLOCKS of include/ivit_hip.h read back on the host: element (r, c) of a [rows, C] matrix sits at
    ((r >> 4) * (C >> 6) + (c >> 6)) * 1024 + ((((r & 15) << 2) + (((c >> 4) & 3) ^ (((r & 15) >> 2) & 3))) << 4) + (c & 15)"""
    a = buf.cpu().numpy().reshape(-1)
    r, c = np.meshgrid(np.arange(rows), np.arange(C), indexing="ij")
    rl = r & 15
    off = ((r >> 4) * (C >> 6) + (c >> 6)) * 1024 + (((rl << 2) + (((c >> 4) & 3) ^ ((rl >> 2) & 3))) << 4) + (c & 15)
    return a[off]


@pytest.mark.parametrize("name", list(R.SETS))
@pytest.mark.parametrize("C", [192, 384, 768, 1024])
def test_engine_entry_i16(C, name):
    """ivit_ibert_layernorm_i16_i8_ex (the 16-bit stream: var_int is the float32 sum in torch's order, 2^24 and above) + QuantAct,
    fast_division 0 and, where the host check allows it, 1"""
    for case in cases_of(C, name):
        e = expected(case)
        lp = e["lp"]
        x, b, so = t(e["q"].astype(np.int16)), t(e["bias_int"]), t(e["s_out"])
        m, ex = t(lp.m.view(np.int32)), t(lp.e)
        for fd in (0, 1) if markstein_division_ok(e["s_in"], 16) else (0,):
            for flags, want in ((FLAG | fd, e["y_i8"]), (fd, e["y0_i8"])):
                out = torch.full((R.ROWS + 1, C), 7, dtype=torch.int8, device=DEV)
                _lib.call("ivit_ibert_layernorm_i16_i8_ex", _lib.ptr(x), C, R.ROWS, C, float(e["s_in"]), _lib.ptr(b), _lib.ptr(so), e["shift_pow2"],
                          _lib.ptr(m), _lib.ptr(ex), _lib.ptr(out), C, flags, _lib.stream_ptr())
                _same(out[:R.ROWS].cpu().numpy(), want, f"{e['key']} flags={flags:#x}")
                assert (out[R.ROWS:] == 7).all()
        if name == "q16":
            assert (e["var_int"] >= 2 ** 24).sum() > 60
    # a width without a register kernel: the wave-per-row literal kernel on int16
    rng = np.random.default_rng(C)
    Co = C - 64 + 6
    qv = np.clip(np.rint(rng.normal(0, 1500, size=(9, Co))), -32768, 32767).astype(np.int16)
    gamma, beta = rng.uniform(0.5, 1.5, size=Co).astype(f32), rng.uniform(-1, 1, size=Co).astype(f32)
    bias_int, s_out = R.layernorm_constants(gamma, beta)
    lp = LayerNormParams(gamma, beta, float(S_NEXT))
    out = torch.zeros(9, Co, dtype=torch.int8, device=DEV)
    x, b, so, m, ex = t(qv), t(bias_int), t(s_out), t(lp.m.view(np.int32)), t(lp.e)
    _lib.call("ivit_ibert_layernorm_i16_i8_ex", _lib.ptr(x), Co, 9, Co, 2.0 ** -9, _lib.ptr(b), _lib.ptr(so), 1.0, _lib.ptr(m), _lib.ptr(ex),
              _lib.ptr(out), Co, FLAG, _lib.stream_ptr())
    ln = q.IBERTIntLayerNorm(Co, use_int_sqrt=True).to(DEV)
    ln.weight.data, ln.bias.data = t(gamma), t(beta)
    ln.fix()
    act = q.QuantAct().to(DEV)
    act.x_min.fill_(-float(S_NEXT) * 127)
    act.x_max.fill_(float(S_NEXT) * 127)
    act.fix()
    s_t = torch.tensor([2.0 ** -9], dtype=torch.float32, device=DEV)
    with torch.no_grad():
        yy, s_ln = ln(t(qv.astype(f32)) * s_t, s_t)
        zz, s_z = act(yy, s_ln)
    assert float(s_z) == float(S_NEXT)
    _same(out.cpu().numpy().astype(np.int32), torch.round(zz / s_z).to(torch.int32).cpu().numpy(), f"C={Co}")


# ------------------------------------------------------------------------------------------------------------ the module
@pytest.mark.parametrize("C", [192, 384, 768, 1024])
def test_module_equals_the_reference_rows(C, ops):
    """IBERTIntLayerNorm(use_int_sqrt=True), with the overflow guard on (unfrozen) and off (frozen): the reference's rows by CRC-32,
    then element by element against the restatement"""
    for case in [c for c in R.CASES if c[0] == C]:
        e = expected(case)
        ln = q.IBERTIntLayerNorm(C, use_int_sqrt=True).to(DEV)
        ln.weight.data, ln.bias.data = t(e["gamma"]), t(e["beta"])
        ln.shift.fill_(float(np.log2(e["shift_pow2"])))
        s = t(np.array([e["s_in"]], f32))
        x = t((e["q"].astype(f32) * e["s_in"]).astype(f32)).reshape(1, R.ROWS, C)
        for frozen in (False, True):
            if frozen:
                ln.fix()
            with torch.no_grad():
                y, so = ln(x, s)
            assert float(ln.shift) == float(np.log2(e["shift_pow2"])) and np.array_equal(so.cpu().numpy(), e["s_out"])
            y = y.cpu().numpy().reshape(R.ROWS, C)
            assert np.isnan(y[0]).all()
            assert np.array_equal(R.row_crcs(y)[1:], ops[e["key"] + "/row_crc32"][1:]), (e["key"], frozen)
            _same(canon(y), canon(e["y"]), e["key"])


# ------------------------------------------------------------------------------------------------------------ whole models
@pytest.mark.parametrize("tag", ["deit_tiny_ibert_isqrt", "deit_tiny_ibert_isqrt_natural", "deit_tiny_ibert_isqrt_w16all"])
def test_models_equal_the_reference(tag):
    """DeiT-T, I-BERT operators, layernorm_type 'ibert_use-int-sqrt_true', batch 4: the fused engine's INT32 logits and top-1 are the
    reference's; the integer-carrying module path gives the same logits; the graph replay equals
    the eager forward"""
    fs, ranges, cfg, meta, z = load_synthetic_model(tag)
    model = ivit.deit_tiny_patch16_224(gelu_type="ibert", softmax_type="ibert", layernorm_type=meta["layernorm_type"], **meta["widths"])
    assert meta["layernorm_type"] == ISQRT and model.ln_int_sqrt
    model.load_state_dict({k: torch.from_numpy(v) for k, v in fs.items()}, strict=False)
    mods = dict(model.named_modules())
    for name, bw in zip([str(n) for n in z["range_names"]], z["range_bits"]):
        assert int(mods[name].activation_bit) == int(bw), name
        mods[name].x_min.fill_(float(ranges[name][0]))
        mods[name].x_max.fill_(float(ranges[name][1]))
    for name, sh in meta["ln_shifts"].items():
        mods[name].shift.fill_(float(sh))
    model.to(DEV)
    ivit.freeze_model(model)
    imgs = torch.from_numpy(synth.make_images(4, meta["image_seed"])).to(DEV)
    assert model.takes_engine(imgs), model.engine_unsupported_reason()
    eng = model.engine(4)
    wide = tag.endswith("w16all")
    assert (eng.family, eng.int_sqrt, eng.stream_bits) == ("ibert", True, 16 if wide else 8)
    li, lf, t1 = eng.forward(imgs)
    li, lf, t1 = li.cpu().numpy().copy(), lf.cpu().numpy().copy(), t1.cpu().numpy().astype(np.int64)
    assert np.array_equal(li, z["logits_int32"]), "INT32 logits differ from the reference's"
    assert np.array_equal(t1, z["top1"])
    if meta["regime"] == "pow2":
        assert np.array_equal(lf.view(np.int32), z["logits_f32_bits"])
    gi, gf, g1 = eng.forward_graph(imgs)
    assert np.array_equal(gi.cpu().numpy(), li) and np.array_equal(gf.cpu().numpy().view(np.int32), lf.view(np.int32))
    assert np.array_equal(g1.cpu().numpy().astype(np.int64), t1)
    with torch.no_grad():
        ye = model(imgs).cpu().numpy()
    assert np.array_equal(ye.view(np.int32), lf.view(np.int32))
    # module by module (the integer-carrying path)
    model.use_engine = False
    with torch.no_grad():
        y = model(imgs)
    lm = np.rint(y.cpu().numpy().astype(np.float64) / z["head_scale"].astype(np.float64)).astype(np.int32)
    assert np.array_equal(lm, z["logits_int32"]) and np.array_equal(y.argmax(dim=1).cpu().numpy(), z["top1"])
    assert np.array_equal(y.cpu().numpy().view(np.int32), lf.view(np.int32))
