"""Swin with the I-BERT operators in the fused engine (IntSwinEngine(family="ibert"), swin_engine.engine_from_model), and the kernel
form it needs: ivit_ibert_layernorm_i16_i8_win, the int16 I-BERT LayerNorm that stores its rows in window order.

  kernel   against ivit_ibert_layernorm_i16_i8_ex on the same input, permuted by swin_engine.window_row_map, byte for byte, for all
           four (fast_division, IVIT_IBERT_LN_INT_SQRT) combinations; one case against oracle/ibert.py's LayerNorm + the oracle's
           requant; strided rows into a fenced output (tests/fenced.py); the documented error codes
  engine   against the reference's own forward (tests/golden/swin_ibert_small.npz: INT32 logits, top-1, the CRC32 of every tap), and
           against the module path of model A of tests/test_gpu_swin_ibert_lazy.py and of B2, its model B with a second stage (float32 logits bit for bit, every tap), at
           the batch sizes on each side of the 2048-row and 8192-row weight-layout switches of IntSwinEngine._w; use_int_sqrt;
           forward_topk / forward_graph / uint8 input; the shift-mask precondition; which kernels it launches.
Nothing here has a tolerance."""
import json
import zlib

import numpy as np
import pytest
import torch

from oracle import ibert as ib
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib, synth  # noqa: E402
from ivit_amd.engine_common import IBERT_LN_INT_SQRT as ISQ  # noqa: E402
from ivit_amd.prepare import LayerNormParams, markstein_division_ok  # noqa: E402
from ivit_amd.swin_engine import IntSwinEngine, _pad64, engine_from_model, window_row_map  # noqa: E402
from ivit_amd.transforms import EvalTransform  # noqa: E402

import fenced  # noqa: E402
from test_gpu_strides import ibert_ln_oracle  # noqa: E402
from test_gpu_swin_ibert_lazy import GOLDEN, MODELS, _images, built, module_run  # noqa: E402  (models A and B, built once per process)

DEV = "cuda:0"
f32 = np.float32
WIN = "ivit_ibert_layernorm_i16_i8_win"
EX = "ivit_ibert_layernorm_i16_i8_ex"
INT_SQRT_OPS = ("ibert", "ibert", "ibert_use-int-sqrt_true")
# Model B (96 px, 12 x 12 windows, depths (2,)) ends with 96 features, which no fused Swin engine takes (the classifier GEMM steps K
# in 64-byte slabs: engine_structure_reason) -- engine_from_model refuses it by that reason, below.  B2 is B with a second stage
# (24 x 24 map in four shifted 144-token windows, then a 12 x 12 map that is one window; 192 features): the 144-token attention and
# the 12 x 12 row map through the engine
MODELS.setdefault("B2", dict(img_size=96, window_size=12, depths=(2, 2), num_heads=(3, 6)))
_KEEP = []


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    _KEEP.append(t)
    return t


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def st():
    return _lib.stream_ptr()


def p(t):
    return _lib.ptr(t)


def tables(C, seed, s_out=3.1 / 127):
    rng = np.random.default_rng(seed)
    gamma = rng.uniform(0.5, 1.5, size=C).astype(f32)
    beta = rng.uniform(-1, 1, size=C).astype(f32)
    lp = LayerNormParams(gamma, beta, float(f32(s_out)))
    return gamma, beta, lp, (p(dev(lp.bias_int)), p(dev(lp.s_ln)), p(dev(lp.m.view(np.int32))), p(dev(lp.e)))


def run_ln(name, x, ldx, rows, C, s_in, tabs, shift_pow2, out, ldo, flags, geo=()):
    bias, s_ln, m, e = tabs
    _lib.call(name, p(x), ldx, rows, C, float(s_in), bias, s_ln, float(shift_pow2), m, e, p(out), ldo, flags, *geo, st())


# =========================================================================================== the kernel against the existing entry
LN_CASES = [(2, 14, 14, 7, 3, 96), (2, 14, 14, 7, 0, 192), (1, 24, 24, 12, 6, 96), (3, 7, 7, 7, 0, 384), (1, 14, 14, 7, 6, 768)]
S_NATURAL, S_POW2 = f32(1.37e-4), f32(2.0 ** -9)


def stream_rows(rows, C, rng):
    """int16 rows of the residual stream: a third full range (uniform over all 65536 values), the rest normal with a per-row sigma
    of 5 .. 6000 (log-uniform); one constant row (std = 0: the literal row of every kernel)"""
    sigma = np.exp(rng.uniform(np.log(5.0), np.log(6000.0), size=(rows, 1)))
    q = np.clip(np.rint(rng.normal(rng.normal(0, 50, size=(rows, 1)), sigma, size=(rows, C))), -32768, 32767)
    q[::3] = rng.integers(-32768, 32768, size=q[::3].shape)
    q[1] = 7
    return q.astype(np.int16)


@pytest.mark.parametrize("case", LN_CASES, ids=lambda c: "B{}_{}x{}_ws{}_shift{}_C{}".format(*c))
def test_window_order_equals_the_ex_entry_permuted(case):
    B, H, W, ws, shift, C = case
    rows = B * H * W
    q = stream_rows(rows, C, np.random.default_rng(sum(case)))
    sq = ((q.astype(np.int64) - q.astype(np.int64).mean(1, keepdims=True).round()) ** 2).sum(1)
    assert (sq >= 2 ** 24).sum() > rows // 4 and (sq < 2 ** 24).any() and sq[1] == 0      # variance sums on both sides of 2^24
    assert markstein_division_ok(S_POW2, 16) and S_NATURAL != 2.0 ** np.round(np.log2(S_NATURAL))
    x = dev(q)
    tabs = tables(C, C)[3]
    perm = torch.from_numpy(window_row_map(B, H, W, ws, shift)).to(DEV)
    assert sorted(perm.tolist()) == list(range(rows))
    for s_in, shift_pow2 in ((S_NATURAL, 1.0), (S_POW2, 4.0)):
        for flags in (0, 1, ISQ, 1 | ISQ):
            ref = torch.full((rows, C), 55, dtype=torch.int8, device=DEV)
            got = torch.full((rows, C), 66, dtype=torch.int8, device=DEV)
            run_ln(EX, x, C, rows, C, s_in, tabs, shift_pow2, ref, C, flags)
            run_ln(WIN, x, C, rows, C, s_in, tabs, shift_pow2, got, C, flags, (H, W, ws, shift))
            assert torch.equal(got[perm], ref), (float(s_in), flags, int((got[perm] != ref).sum()))
            assert len(torch.unique(ref)) > 100


def test_ws_zero_is_the_ex_entry():
    """ws == 0: rows in order; H, W and shift are not read"""
    rows, C = 98, 192
    x = dev(stream_rows(rows, C, np.random.default_rng(3)))
    tabs = tables(C, 5)[3]
    for flags in (1, ISQ):
        ref = torch.full((rows, C), 55, dtype=torch.int8, device=DEV)
        run_ln(EX, x, C, rows, C, S_POW2, tabs, 2.0, ref, C, flags)
        for geo in ((0, 0, 0, 0), (5, 3, 0, 9)):
            got = torch.full((rows, C), 66, dtype=torch.int8, device=DEV)
            run_ln(WIN, x, C, rows, C, S_POW2, tabs, 2.0, got, C, flags, geo)
            assert torch.equal(got, ref)


@pytest.mark.parametrize("C", [96, 192])
def test_window_order_against_the_oracle(C):
    """oracle/ibert.py's LayerNorm + the oracle's requant on rows whose sums stay below 2^24 (exact in any order), permuted by the host
    row map: the comparison above does not merely chain two kernels.  C = 96: the literal kernel, 192: the register kernel"""
    B, H, W, ws, shift = 2, 14, 14, 7, 3
    rows = B * H * W
    rng = np.random.default_rng(C)
    q = np.clip(np.rint(rng.normal(rng.normal(0, 5, size=(rows, 1)), 80.0, size=(rows, C))), -32768, 32767).astype(np.int16)
    gamma, beta, lp, tabs = tables(C, C + 1)
    y, s_ln, ninx = ib.layernorm(q.astype(np.int32), S_POW2, gamma, beta, shift=1.0)
    assert ninx == 0 and np.array_equal(s_ln, lp.s_ln)
    om, oe = orc.dyadic(s_ln, f32(3.1 / 127))
    ref = orc.requant(orc.roundtrip(y, s_ln), om, oe, 8)
    assert np.abs(ref).max() > 50
    want = np.empty_like(ref)
    want[window_row_map(B, H, W, ws, shift)] = ref
    for fd in (0, 1):
        got = torch.full((rows, C), 66, dtype=torch.int8, device=DEV)
        run_ln(WIN, dev(q), C, rows, C, S_POW2, tabs, 2.0, got, C, fd, (H, W, ws, shift))
        assert np.array_equal(got.cpu().numpy().astype(np.int32), want)


@pytest.mark.parametrize("C", [96, 192])
def test_window_order_strided_rows_fenced(C):
    """ldx = C + 8 between poisoned pads; ldo = _pad64(C) (128 at C = 96: the engine's `h` buffer) or C + 64: the pad columns, the
    guards and the slack keep their sentinel, every data row lands at its window-order position"""
    B, H, W, ws, shift = 1, 14, 14, 7, 3
    rows = B * H * W
    ldo = _pad64(C) if _pad64(C) > C else C + 64
    rng = np.random.default_rng(C + 16)
    s_in = f32(2.0 ** -9)
    q = np.clip(np.rint(rng.normal(rng.normal(0, 5, size=(rows, 1)), 80.0, size=(rows, C))), -32768, 32767).astype(np.int16)
    q[1] = q[1, 0]
    q[1, 3] += 9                                           # tiny variance
    assert (q.astype(np.int64) ** 2).sum(1).max() < 2 ** 24 and markstein_division_ok(s_in, 16)
    gamma = rng.uniform(0.5, 1.5, size=C).astype(f32)
    beta = rng.uniform(-1, 1, size=C).astype(f32)
    perm = window_row_map(B, H, W, ws, shift)
    for isq in (False, True):
        lp, orac = ibert_ln_oracle(gamma, beta, s_in, 1.0, isq)
        exp = orac(q)
        want = np.empty_like(exp)
        want[perm] = exp
        x = fenced.input(q, C + 8, fenced.POISON[q.dtype], oracle=orac, expected=exp, device=DEV)
        tabs = (p(dev(lp.bias_int)), p(dev(lp.s_ln)), 1.0, p(dev(lp.m.view(np.int32))), p(dev(lp.e)))
        for fd in (0, 1):
            o = fenced.output(rows, C, ldo, np.int8, expected=want, device=DEV)
            _lib.call("ivit_ibert_layernorm_i16_i8_win", x.ptr, x.ld, rows, C, float(s_in), *tabs, o.ptr, o.ld, fd | (ISQ if isq else 0),
                      H, W, ws, shift, st())
            fenced.check(o, want)
        fenced.check(x)


def test_error_codes():
    """a window description that does not match: IVIT_ERR_UNSUPPORTED (-2); a stray flag bit, a bad operand: IVIT_ERR_INVALID (-1);
    nothing is launched (the output keeps its fill)"""
    C, H, W, ws = 96, 14, 14, 7
    rows = 2 * H * W
    x = dev(np.zeros((rows, C), np.int16))
    out = torch.full((rows, C), 66, dtype=torch.int8, device=DEV)
    bias, s_ln, m, e = tables(C, 1)[3]
    L = _lib.lib()

    def rc(rows_=rows, flags=0, geo=(H, W, ws, 3), ldo=C):
        return L.ivit_ibert_layernorm_i16_i8_win(p(x), C, rows_, C, 2.0 ** -9, bias, s_ln, 1.0, m, e, p(out), ldo, flags, *geo, st())
    assert rc() == 0
    out.fill_(66)
    for bad in (dict(geo=(H, W, ws, ws)), dict(geo=(H, W, ws, -1)), dict(geo=(16, W, ws, 0)), dict(geo=(H, 15, ws, 0)),
                dict(rows_=rows - 1), dict(rows_=H * W + 7)):
        assert rc(**bad) == -2 and b"unsupported geometry" in L.ivit_last_error_string(), bad
    for bad in (dict(flags=2), dict(flags=ISQ | 4), dict(flags=ISQ << 1), dict(ldo=C - 1)):
        assert rc(**bad) == -1, bad
    torch.cuda.synchronize()
    assert bool((out == 66).all())


# =========================================================================================== the engine against the reference fixture
def traced(fn):
    """(result of fn(), the names of the launches it issued)"""
    names, real = [], _lib.call
    try:
        _lib.call = lambda name, *a: (names.append(name), real(name, *a))[1]
        return fn(), names
    finally:
        _lib.call = real


def fixture_engine():
    z = np.load(GOLDEN, allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    cfg = synth.SWIN_CONFIGS[meta["config"]]
    fs = synth.make_swin_float_state(meta["config"], meta["weight_seed"])
    ranges = {str(n): (float(lo), float(hi)) for n, (lo, hi) in zip(z["range_names"], z["ranges"])}
    for n, sh in zip([str(n) for n in z["shift_names"]], z["shifts"]):
        fs[n + ".shift"] = np.array([sh], f32)
    make = lambda: IntSwinEngine(fs, ranges, cfg["embed_dim"], cfg["depths"], cfg["num_heads"], cfg["window"], device=DEV,      # noqa: E731
                                 max_batch=4, img_size=meta["img_size"], family="ibert")
    return z, cfg, make


def test_engine_equals_the_reference_fixture():
    z, cfg, make = fixture_engine()
    eng, built_with = traced(make)
    x = torch.from_numpy(z["images"]).to(DEV)
    taps = {}
    li, _, top1 = eng.forward(x, taps=taps)
    assert np.array_equal(li.cpu().numpy(), z["logits_int32"]), int((li.cpu().numpy() != z["logits_int32"]).sum())
    assert np.array_equal(top1.cpu().numpy().astype(np.int64), z["top1"])
    gold = dict(zip([str(n) for n in z["tap_names"]], z["tap_crc32"]))
    assert set(taps) <= set(gold), sorted(set(taps) - set(gold))
    bad = [n for n in taps if zlib.crc32(np.ascontiguousarray(taps[n].cpu().numpy().astype(np.int32)).tobytes()) != int(gold[n])]
    # per block qact1, attn.qact1, attn.qact3, qact2, qact3, mlp.qact_gelu, mlp.qact1, mlp.qact2, qact4; per merging two; stem 3, tail 2
    assert not bad and len(taps) == 9 * sum(cfg["depths"]) + 2 * (len(cfg["depths"]) - 1) + 5, (len(taps), bad[:6])
    # without taps: attention output at its image rows in front of the one residual GEMM, GELU fused where fc1 takes the fragment copy
    (lf, _, t1), launched = traced(lambda: eng.forward(x))
    assert np.array_equal(lf.cpu().numpy(), z["logits_int32"]) and np.array_equal(t1.cpu().numpy().astype(np.int64), z["top1"])
    check_trace(built_with, launched, cfg["depths"])


def check_trace(built_with, launched, depths):
    nblk = sum(depths)
    both = built_with + launched
    assert launched.count("ivit_window_attention_i8_ibert") == nblk
    assert not [n for n in both if n.startswith("ivit_window_attention_i8") and n != "ivit_window_attention_i8_ibert"], sorted(set(both))
    assert not [n for n in both if n == "ivit_window_rows" or "shiftmax" in n or n.startswith("ivit_shiftgelu_build")], sorted(set(both))
    assert launched.count(WIN) == nblk                                               # every norm1
    assert launched.count(EX) == nblk + (len(depths) - 1) + 1                        # norm2, the mergings' norm, the final norm
    assert launched.count("ivit_ibert_layernorm_i8") == 1                            # patch norm
    assert not [n for n in launched if n.startswith("ivit_layernorm")], sorted(set(launched))
    assert launched.count("ivit_gemm_i8_requant_i16_residual_i16_ex") == nblk        # attn.proj + qact4 + the residual, in place
    assert built_with.count("ivit_ibert_gelu_build_lut") == nblk and built_with.count("ivit_ibert_softmax_build_table") == nblk
    assert launched.count("ivit_gemm_i8_requant_lut_ex") + launched.count("ivit_shiftgelu_lut_i8") == nblk


# =========================================================================================== the engine against the module path
ENGINE_TAPS_PER_BLOCK = 9


def engine_and_module(which, pow2, ops=None, max_batch=4):
    model, x = built(which, pow2, ops)
    return model, x, engine_from_model(model, max_batch=max_batch)


def assert_taps_equal(t_eng, t_mod):
    assert set(t_eng) <= set(t_mod), sorted(set(t_eng) - set(t_mod))
    for name, t in t_eng.items():
        a, b = t.reshape(-1).to(torch.int32), t_mod[name].reshape(-1)
        assert a.numel() == b.numel() and torch.equal(a, b), f"tap {name}: {int((a != b).sum())} of {a.numel()} differ"


def check_literal_tail(model, t_eng, lf):
    """an even token count at the pool at natural scales: the engine restates torch's CPU pooling order, the module path on the GPU pools
    with CUDA's mean, which can decide a .5 tie differently (tests/test_gpu_swin_384.py _check_tail).  The engine's
    qact3 against torch's CPU pooling (one thread) of its own qact2 tap + the oracle's requant, its logits against the module head on that"""
    s2 = f32(model.qact2.act_scaling_factor.reshape(-1)[0].item())
    s3t = model.qact3.act_scaling_factor
    s3 = f32(s3t.reshape(-1)[0].item())
    B = lf.shape[0]
    q2 = t_eng["qact2"].cpu().numpy().astype(f32).reshape(B, -1, model.num_features)
    prev = torch.get_num_threads()
    try:
        torch.set_num_threads(1)
        mean = torch.nn.AdaptiveAvgPool1d(1)(torch.from_numpy((q2 * s2).astype(f32)).transpose(1, 2))[:, :, 0].numpy()
    finally:
        torch.set_num_threads(prev)
    om, oe = orc.dyadic(np.array([s2], f32), s3)
    q3 = orc.requant(np.rint((mean / s2).astype(f32)).astype(np.int32), om, oe, 8)
    assert np.array_equal(t_eng["qact3"].cpu().numpy().astype(np.int32).reshape(B, -1), q3)
    yh, _ = model.head(torch.from_numpy((q3.astype(f32) * s3).astype(f32)).to(DEV), s3t)
    assert torch.equal(lf, yh)


@pytest.mark.parametrize("pow2", [False, True], ids=["natural", "pow2"])
@pytest.mark.parametrize("which", ["A", "B2"])
def test_engine_equals_the_module_path(which, pow2):
    model, x, eng = engine_and_module(which, pow2)
    assert eng.family == "ibert" and not eng.int_sqrt and "operator family" in model.engine_unsupported_reason()
    assert eng.pool_literal == ((which, pow2) == ("B2", False))
    t_mod, t_eng = {}, {}
    y = module_run(model, x, True, t_mod)
    assert len(torch.unique(y)) > x.shape[0]
    lf = eng.forward(x.contiguous(), taps=t_eng)[1].clone()
    depths = model.depths
    assert len(t_eng) == ENGINE_TAPS_PER_BLOCK * sum(depths) + 2 * (len(depths) - 1) + 5
    if eng.pool_literal:
        assert_taps_equal({n: t for n, t in t_eng.items() if n != "qact3"}, t_mod)      # through the pre-pool qact2
        with torch.no_grad():
            check_literal_tail(model, t_eng, lf)
    else:
        assert_taps_equal(t_eng, t_mod)
        assert torch.equal(lf, y)
    (_, lf2, _), launched = traced(lambda: eng.forward(x.contiguous()))
    assert torch.equal(lf2, lf)
    assert launched.count(WIN) == sum(depths) and "ivit_window_rows" not in launched
    assert all(b["attn"]["table"] is not None for s in eng.stages for b in s["blocks"])


@pytest.mark.parametrize("pow2", [False, True], ids=["natural", "pow2"])
def test_batches_on_both_sides_of_the_weight_layout_switches(pow2):
    """model A, stage-0 rows 588, 2156 and 8232: below 2048 rows (row-major weights), above (block / fragment copies; at 8232 rows
    stage 1 has 2058: fc1 + GELU in one launch), and above 8192 (the skinny-K form); an image's logits do not depend on its batch"""
    model, _ = built("A", pow2)
    eng = engine_from_model(model, max_batch=42)
    x = _images(42, 56, torch.Generator(device="cpu").manual_seed(97))
    y = module_run(model, x, True)
    assert len(torch.unique(y)) > 42
    fused_gelu = {}
    for B in (3, 11, 42):
        assert B * 14 * 14 == {3: 588, 11: 2156, 42: 8232}[B]
        (_, lf, _), launched = traced(lambda: eng.forward(x[:B].contiguous()))
        assert torch.equal(lf, y[:B]), (B, int((lf != y[:B]).sum()))
        fused_gelu[B] = launched.count("ivit_gemm_i8_requant_lut_ex")
        assert fused_gelu[B] + launched.count("ivit_shiftgelu_lut_i8") == sum(model.depths)
    assert fused_gelu == {3: 0, 11: 0, 42: 2}, fused_gelu
    t_mod, t_eng = {}, {}
    module_run(model, x[:11].contiguous(), True, t_mod)
    eng.forward(x[:11].contiguous(), taps=t_eng)
    assert_taps_equal(t_eng, t_mod)


def test_model_b_is_refused_for_its_classifier_width():
    model, _ = built("B", False)
    assert model.num_features == 96
    with pytest.raises(ValueError, match="96 features at the classifier"):
        engine_from_model(model, max_batch=4)


def test_int_sqrt_engine_equals_its_module_path():
    model, x, eng = engine_and_module("A", False, INT_SQRT_OPS)
    assert eng.int_sqrt and model.norm.use_int_sqrt
    t_mod, t_eng = {}, {}
    y = module_run(model, x, True, t_mod)
    _, lf, _ = eng.forward(x.contiguous(), taps=t_eng)
    assert torch.equal(lf, y)
    assert_taps_equal(t_eng, t_mod)
    assert torch.equal(eng.forward(x.contiguous())[1], y)
    plain = engine_from_model(built("A", False)[0], max_batch=4)
    assert all(b["ln1"]["flags"] == ISQ for s in eng.stages for b in s["blocks"]) and plain.stages[0]["blocks"][0]["ln1"]["flags"] == 0


def test_topk_graph_and_uint8_input():
    model, x, eng = engine_and_module("A", False)
    x = x.contiguous()
    li, lf, top1 = (t.clone() for t in eng.forward(x))
    ti, tf, tk = eng.forward_topk(x, k=3)
    assert torch.equal(ti, li) and torch.equal(tf, lf) and torch.equal(tk[:, 0], top1)
    assert torch.equal(tk.long(), torch.sort(lf, dim=1, descending=True, stable=True)[1][:, :3])
    for _ in range(2):                                     # capture, then a replay of the cached graph
        gi, gf, g1 = eng.forward_graph(x)
        assert torch.equal(gi, li) and torch.equal(gf, lf) and torch.equal(g1, top1)
    u8 = torch.from_numpy(np.random.default_rng(8).integers(0, 256, size=(3, 3, 56, 56), dtype=np.uint8)).to(DEV)
    xf = EvalTransform(resize=64, crop=56).to_float(u8).contiguous()
    want = eng.forward(xf)[0].clone()
    assert torch.equal(eng.forward(u8)[0], want) and len(torch.unique(want)) > 3
    eng.drop_graphs()


def test_mask_outside_the_precondition_is_refused_by_name():
    """attn.qact2 of the shifted block at s_attn = 0.5 (the edit of test_mask_beyond_the_precondition_runs_that_attention_core_literally):
    the engine has no literal attention core, so it does not build; with the range restored it does"""
    model, x = built("A", True)
    qa = model.layers[0].blocks[1].attn.qact2
    keep = (qa.x_min.clone(), qa.x_max.clone())
    try:
        qa.x_min.fill_(-127 * 0.5)
        qa.x_max.fill_(127 * 0.5)
        with pytest.raises(ValueError, match=r"layers\.0\.blocks\.1\b.*s_attn = 0\.5"):
            engine_from_model(model, max_batch=4)
    finally:
        qa.x_min.copy_(keep[0])
        qa.x_max.copy_(keep[1])
    eng = engine_from_model(model, max_batch=4)
    assert torch.equal(eng.forward(x.contiguous())[1], module_run(model, x, True))
