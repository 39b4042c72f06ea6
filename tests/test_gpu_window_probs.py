"""The Swin window probabilities (ivit_window_attention_probs_u8 / _ibert, csrc/swin_probs.hip) against the numpy specification of
tests/window_probs_ref.py, byte for byte: every Shiftmax form and both I-BERT table forms at 2, 49, 64, 65 and 144 tokens, rows whose
exponent sum reaches 2^24 (the reference's own outputs, tests/golden/shiftmax_bigsum_kat.npz), fenced outputs with three leading
dimensions, argument errors, and IntSwinEngine / SwinTransformer.attention_maps against the module path's forward hooks."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
from ivit_amd.prepare import window_shiftexp_band  # noqa: E402
from ivit_amd import swin_engine  # noqa: E402
from ivit_amd.swin_engine import (engine_from_model, key_pad, shift_mask_regions, window_attention_ibert_spec,  # noqa: E402
                                  window_attention_spec)
import fenced  # noqa: E402
import shiftmax_order_ref as smo  # noqa: E402
import window_probs_ref as wp  # noqa: E402
from test_gpu_shiftmax_bigsum import kat, natural, scales, window_problem  # noqa: E402
from test_gpu_swin_ibert_lazy import MODELS, _images, snap_pow2  # noqa: E402
from test_gpu_window_attention_ibert import SCALES as IBERT_SCALES, act_range  # noqa: E402

DEV = "cuda:0"
f32 = np.float32
HD = 32
FILL = 0xA5
MODELS.setdefault("B2", dict(img_size=96, window_size=12, depths=(2, 2), num_heads=(3, 6)))      # as tests/test_gpu_swin_ibert_engine.py
# (s_S, s_at, s_A = s_attn, s_tab): the scores' scale, qact_attn1, qact2, the bias table -> the Shiftmax form window_attention_spec reports
SHIFTMAX_SCALES = {"pow2": ((2.0 ** -12, 2.0 ** -2, 2.0 ** -3, 2.0 ** -5), None),
                   "band1": ((3.1e-4, 0.0731, 0.271, 0.0317), "band1x48"),
                   "band256": ((3.1e-4, 0.0731, 0.1173, 0.0317), "band256x96"),
                   "literal": ((3.1e-4, 0.0731, 0.031, 0.0317), "literal")}
# (heads, windows per image, images, shifted): heads 1 and 3, windows per image 1 and 4, one to three images, both mask states
COMBOS = [(1, 1, 3, False), (3, 4, 2, True), (3, 1, 1, True), (1, 4, 1, False)]
_KEEP = []


def upload(a):
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


def regions(N, nW, shifted, rng):
    if not shifted:
        return None
    ws = int(round(N ** 0.5))
    if ws * ws == N:
        side = ws * int(round(nW ** 0.5))
        return shift_mask_regions(side, side, ws, max(ws // 2, 1)).astype(np.uint8)
    reg = rng.integers(0, 3, size=(nW, N)).astype(np.uint8)          # no window geometry: any region table
    reg[0, :2] = (0, 1)                                               # ... with a masked key in window 0
    return reg


def run_case(family, N, make_spec, spec_probs):
    """the COMBOS of one (family, form, N): the spec's P, the properties every run must hold, the launch, the comparison"""
    masked_key = flat = one_hot = False
    top = 0
    for ci, (nH, nW, imgs, shifted) in enumerate(COMBOS):
        nwin = nW * imgs
        rng = np.random.default_rng(1000 * N + ci)
        qkv, bias = wp.problem(N, nH, nwin, 7 * N + ci)
        region = regions(N, nW, shifted, rng)
        want = spec_probs(qkv, bias, region, nW)
        m = wp.masked_pairs(region, nwin, nW)
        masked_key |= m is not None and bool(m.any())
        flat |= bool(wp.near_flat_rows(want).any())
        one_hot |= bool(wp.one_hot_rows(want).any())
        top = max(top, int(want.max()))
        spec = make_spec(bias, region, N, shifted)
        assert spec["bias"].shape[-1] == key_pad(N)
        got = torch.full((nwin, nH, N, N), FILL, dtype=torch.uint8, device=DEV)
        swin_engine.window_attention_probs(spec, family, upload(qkv), got, nwin, nW, nH, N, st())
        torch.cuda.synchronize()
        got = got.cpu().numpy().astype(np.int64)
        assert np.array_equal(got, want), (family, N, ci, int((got != want).sum()), got.size)
    assert masked_key and flat and one_hot, "the inputs must hold a masked key, a near-flat row and a one-hot row"
    return top


@pytest.mark.parametrize("form", list(SHIFTMAX_SCALES))
@pytest.mark.parametrize("N", [2, 49, 64, 65, 144])
def test_shiftmax_probabilities_equal_the_specification(N, form):
    (s_S, s_at, s_A, s_tab), reported = SHIFTMAX_SCALES[form]
    s_S, s_at, s_A, s_tab = f32(s_S), f32(s_at), f32(s_A), f32(s_tab)

    def make_spec(bias, region, N, shifted):
        spec, got_form = window_attention_spec(upload, bias, s_tab, s_S, s_at, s_A, f32(2.0 ** -11), f32(2.0 ** -5), region, N)
        # the one-row band is the form of a scale that is no power of two but has phi = identity (0.271): there only the shift
        # mask (-100 / s is no integer) takes the natural route, an unshifted block runs the integer table of distances at x0 = -4
        want_form = None if form == "band1" and not shifted else reported
        assert got_form == want_form, (got_form, want_form)
        assert (spec["band"] is not None) == str(got_form).startswith("band") and (spec["phi"] is not None) == (got_form is not None)
        return spec

    top = run_case("ivit", N, make_spec, lambda qkv, bias, region, nW: wp.probs("ivit", qkv, bias, region, nW, s_S, s_at, s_A, s_tab))
    assert 100 <= top <= 127


@pytest.mark.parametrize("form", ["table", "band"])
@pytest.mark.parametrize("N", [2, 49, 64, 65, 144])
def test_ibert_probabilities_equal_the_specification(N, form):
    """the calibrated ("natural") regime of tests/test_gpu_window_attention_ibert.py: its e_max = 32767 makes a one-hot row p = 128,
    the byte 0x80 (fl(e_max * floor(2^32 / e_max)) = 2^32)"""
    s_S, s_at, s_A, s_tab, _, _ = (f32(v) for v in IBERT_SCALES["natural"])
    rng_act = act_range(s_A, "natural")

    def make_spec(bias, region, N, shifted):
        spec = window_attention_ibert_spec(upload, DEV, st(), bias, s_tab, s_S, s_at, s_A, f32(2.0 ** -11), f32(2.0 ** -5), region, N,
                                           rng_act, form=form)
        assert spec is not None and (spec["band_w"] > 0) == (form == "band")
        return spec

    top = run_case("ibert", N, make_spec,
                   lambda qkv, bias, region, nW: wp.probs("ibert", qkv, bias, region, nW, s_S, s_at, s_A, s_tab, rng_act))
    assert top == 128


def test_shiftmax_rows_whose_sum_reaches_2_24():
    """144 tokens, the fixture rows of tests/test_gpu_shiftmax_bigsum.py as one window with a head per row: expected is the oracle's P,
    whose query-0 rows are the reference's own outputs.  On the class-(c) rows the exact sum rounded once gives other probabilities
    than the sum in torch's order (asserted): a kernel without the ordered sum fails on exactly those."""
    T, ran, seen_c = 144, 0, 0
    K = kat(T)
    for s in scales(T):
        pr = window_problem(T, s)
        if pr is None:
            continue
        c_rows = pr["rows"][pr["cls"] == smo.CLASS_C]
        assert all(np.any(K["exact"][r] != K["ref"][r]) for r in c_rows), "the ordered and the plain factor must differ on class (c)"
        seen_c += len(c_rows)
        H = pr["H"]
        qkv = np.ascontiguousarray(pr["qkv"][:, 0][:, None])                         # [3, 1 window, H, T, 32]
        exp = pr["P"].reshape(H * T, T)
        for form in (("literal", "band") if natural(s) else ("pow2",)):
            phi = (_lib.ptr(upload(pr["phi"])), _lib.ptr(upload(pr["phim"]))) if form == "literal" else (None, None)
            band = (None, 0, 0)
            if form == "band":
                bt, bw = window_shiftexp_band(pr["s"], False)
                assert bt is not None
                band = (_lib.ptr(upload(bt)), bw, bt.shape[0])
            o = fenced.output(H * T, T, T + 4, np.uint8, expected=exp)
            _lib.call("ivit_window_attention_probs_u8", _lib.ptr(upload(qkv)), o.ptr, o.ld, _lib.ptr(upload(pr["bias"])), None,
                      0 if form == "pow2" else -1, 1, 1, H, T, HD, int(pr["ms"][0]), int(pr["es"][0]), pr["mb"][0], pr["mb"][1],
                      float(pr["s"]), *phi, *band, st())
            torch.cuda.synchronize()
            got = o.rows2d(o.fetch())[:, :T].astype(np.int32).reshape(H, T, T)
            bad = np.any(got[:, 0] != pr["P"][:, 0], axis=1)
            assert not bad.any(), (s, form, {smo.CLASS_NAMES[c]: int((bad & (pr["cls"] == c)).sum()) for c in (0, 1, 2)})
            fenced.check(o, exp)
            ran += 1
    assert ran >= 4 and seen_c >= 4


# ----------------------------------------------------------------------------------- fenced outputs
@pytest.mark.parametrize("N,pad", [(49, 0), (49, 3), (64, 5)], ids=["bytes", "dwords", "odd_ld"])
def test_fenced_outputs_of_both_entries(N, pad):
    """ldp = N at 49 tokens (byte stores), N + 3 = 52 (dword stores and a byte tail), N + 5 at 64 tokens (no multiple of four):
    the pad bytes of every row and the guard rows keep their fill"""
    nH, nW, imgs = 3, 4, 2
    nwin = nW * imgs
    qkv, bias = wp.problem(N, nH, nwin, 3 * N + pad)
    ws = int(round(N ** 0.5))
    region = shift_mask_regions(2 * ws, 2 * ws, ws, ws // 2).astype(np.uint8)
    s_S, s_at, s_A, s_tab = (f32(v) for v in SHIFTMAX_SCALES["pow2"][0])
    a, form = window_attention_spec(upload, bias, s_tab, s_S, s_at, s_A, f32(2.0 ** -11), f32(2.0 ** -5), region, N)
    assert form is None
    exp = wp.probs("ivit", qkv, bias, region, nW, s_S, s_at, s_A, s_tab).reshape(nwin * nH * N, N)
    o = fenced.output(nwin * nH * N, N, N + pad, np.uint8, expected=exp)
    p = _lib.ptr
    _lib.call("ivit_window_attention_probs_u8", p(upload(qkv)), o.ptr, o.ld, p(a["bias"]), p(a["region"]), a["mask_value"], nwin, nW, nH,
              N, HD, *a["ms"], *a["mb"], a["s_attn"], None, None, None, 0, 0, st())
    torch.cuda.synchronize()
    fenced.check(o, exp)
    s_S, s_at, s_A, s_tab, _, _ = (f32(v) for v in IBERT_SCALES["natural"])
    rng_act = act_range(s_A, "natural")
    b = window_attention_ibert_spec(upload, DEV, st(), bias, s_tab, s_S, s_at, s_A, f32(2.0 ** -11), f32(2.0 ** -5), region, N, rng_act,
                                    form="band")
    exp = wp.probs("ibert", qkv, bias, region, nW, s_S, s_at, s_A, s_tab, rng_act).reshape(nwin * nH * N, N)
    assert exp.max() == 128
    o = fenced.output(nwin * nH * N, N, N + pad, np.uint8, expected=exp)
    _lib.call("ivit_window_attention_probs_u8_ibert", p(upload(qkv)), o.ptr, o.ld, p(b["bias"]), p(b["region"]), b["masked_exp"], nwin,
              nW, nH, N, HD, *b["ms"], *b["mb"], p(b["table"]), b["band_w"], st())
    torch.cuda.synchronize()
    fenced.check(o, exp)


# ----------------------------------------------------------------------------------- argument errors
GOOD = dict(qkv=True, probs=True, table=True, tokens=49, head_dim=32, ldp=49, band_off=0, band_w=48, band_rows=1)
INVALID, UNSUPPORTED = -1, -2
COMMON = [(dict(tokens=1), UNSUPPORTED), (dict(tokens=145), UNSUPPORTED), (dict(head_dim=64), UNSUPPORTED), (dict(ldp=48), INVALID),
          (dict(qkv=False), INVALID), (dict(probs=False), INVALID), (dict(band_w=8), INVALID)]
# the Shiftmax entry's band table is optional (NULL selects another form) but must be aligned and have 1 or 256 rows; the I-BERT
# entry's table is required
BAD = ([("ivit", c, rc) for c, rc in COMMON + [(dict(band_off=4), INVALID), (dict(band_rows=2), INVALID)]] +
       [("ibert", c, rc) for c, rc in COMMON + [(dict(table=False), INVALID)]])


def _entry_call(family, a):
    """one call with one window of one head; `table` stands for the Shiftmax band table and for the I-BERT table alike.
    -> (status, the output buffer)"""
    T = 144
    qkv = torch.zeros(3 * T * HD + 64, dtype=torch.int8, device=DEV)
    bias = torch.zeros(T * 144 + 64, dtype=torch.int16, device=DEV)
    tab = (torch.full((65536 + 64,), 1000, dtype=torch.int32, device=DEV) if family == "ivit"      # exp_int values / float32 exponents
           else torch.ones(65536 + 64, dtype=torch.float32, device=DEV))
    out = torch.full((T * T + 64,), FILL, dtype=torch.uint8, device=DEV)
    _KEEP.extend([qkv, bias, tab, out])
    p_qkv = qkv.data_ptr() if a["qkv"] else None
    p_out = out.data_ptr() if a["probs"] else None
    p_tab = tab.data_ptr() + a["band_off"] if a["table"] else None
    L = _lib.lib()
    if family == "ivit":
        rc = L.ivit_window_attention_probs_u8(p_qkv, p_out, a["ldp"], bias.data_ptr(), None, 0, 1, 1, 1, a["tokens"], a["head_dim"],
                                              1 << 20, 30, 1 << 30, 30, 0.271, None, None, p_tab, a["band_w"], a["band_rows"], st())
    else:
        rc = L.ivit_window_attention_probs_u8_ibert(p_qkv, p_out, a["ldp"], bias.data_ptr(), None, 0.0, 1, 1, 1, a["tokens"],
                                                    a["head_dim"], 1 << 20, 30, 1 << 30, 30, p_tab, a["band_w"], st())
    torch.cuda.synchronize()
    return rc, out, L


@pytest.mark.parametrize("family,change,status", BAD, ids=[f"{f}-" + "-".join(f"{k}={v}" for k, v in c.items()) for f, c, _ in BAD])
def test_argument_errors_write_nothing(family, change, status):
    """each error changes one thing in the call test_the_unchanged_arguments_are_accepted makes"""
    rc, out, L = _entry_call(family, {**GOOD, **change})
    assert rc == status and L.ivit_last_error_string(), (rc, L.ivit_last_error_string())
    assert bool((out == FILL).all()), "a rejected call wrote to its output"


@pytest.mark.parametrize("family", ["ivit", "ibert"])
def test_the_unchanged_arguments_are_accepted(family):
    rc, out, L = _entry_call(family, GOOD)
    assert rc == 0, L.ivit_last_error_string()
    T = GOOD["tokens"]
    assert bool((out[:T * T] != FILL).all()) and bool((out[T * T:] == FILL).all())


# ----------------------------------------------------------------------------------- engine and model
IVIT_OPS = ("ivit", "ivit", "ivit")
IBERT_OPS = ("ibert", "ibert", "ibert")
_BUILT = {}


def built(which, pow2, ops):
    """the calibrated, frozen model and a batch of three images for it, as tests/test_gpu_swin_ibert_lazy.py builds its models, with
    one difference: the qkv weights are twice as wide, the scores four times.  With that file's weights the 144 scores of a 12 x 12
    window are nearly equal and every probability of block (0, 0) is 128 / 144 rounded, at most 3: a map on which an error of the
    kernel could hide.  Built once per (model, regime, operators) and shared -- no test changes it."""
    key = (which, pow2, ops)
    if key not in _BUILT:
        cfg = MODELS[which]
        torch.manual_seed(11 + ord(which[0]) + pow2)
        names = dict(zip(("gelu_type", "softmax_type", "layernorm_type"), ops))
        model = ivit.SwinTransformer(patch_size=4, embed_dim=96, num_classes=10, **names, **cfg).to(DEV).eval()
        g = torch.Generator(device="cpu").manual_seed(5 + ord(which[0]))
        with torch.no_grad():
            for name, p in model.named_parameters():
                if p.dim() > 1:
                    p.mul_(6.0 if name.endswith("attn.qkv.weight") else 3.0)
                elif name.endswith("relative_position_bias_table"):
                    p.mul_(20.0)
            calib = _images(4, cfg["img_size"], g)
            model(calib)
            model(calib.flip(0) * 0.7)
        if pow2:
            snap_pow2(model)
        ivit.freeze_model(model)
        _BUILT[key] = (model, _images(3, cfg["img_size"], g))
    return _BUILT[key]


def _shapes(model, B):
    out = {}
    for li, (depth, nH) in enumerate(zip(model.depths, model.num_heads)):
        side = model.patch_grid[0] // 2 ** li
        win = min(model.window_size, side)
        for bi in range(depth):
            out[(li, bi)] = (B, (side // win) ** 2, nH, win * win, win * win)
    return out


def _hook_maps(model, x, blocks=None):
    model.use_engine = False
    try:
        return model.attention_maps(x, blocks)
    finally:
        model.use_engine = True


@pytest.mark.parametrize("pow2", [True, False], ids=["pow2", "natural"])
@pytest.mark.parametrize("which", ["A", "B2"])
def test_engine_maps_equal_the_module_paths_softmax_output(which, pow2):
    """a frozen two-stage Swin with the I-ViT operators: the maps of the engine call are, byte for byte, what forward hooks on the
    log_int_softmax modules of the same model see on the module path -- the reference's own tensor; the forward that produced them
    left the logits of model(x)"""
    model, x = built(which, pow2, IVIT_OPS)
    B = x.shape[0]
    shapes = _shapes(model, B)
    assert list(shapes.values())[0][1:] == ((4, 3, 49, 49) if which == "A" else (4, 3, 144, 144)) and shapes[(1, 0)][1] == 1
    with torch.no_grad():
        y = model(x)
        assert model.takes_engine(x)
        maps, scale = model.attention_maps(x)
        eng = model.engine(B)
        logits = eng.ws["logits_f"][:B, :eng.num_classes].clone()
        one, _ = model.attention_maps(x, blocks=[(1, 0)])
        ref, scale_r = _hook_maps(model, x)
    assert scale == scale_r == 2.0 ** -7
    assert list(maps) == list(ref) == sorted(shapes) and list(one) == [(1, 0)]
    assert torch.equal(logits, y)
    for key, shape in shapes.items():
        assert maps[key].dtype == ref[key].dtype == torch.uint8 and tuple(maps[key].shape) == tuple(ref[key].shape) == shape
        assert torch.equal(maps[key], ref[key]), f"block {key}: {int((maps[key] != ref[key]).sum())} of {maps[key].numel()} bytes differ"
        assert 8 < int(maps[key].max()) <= 128      # a live attention
    assert torch.equal(one[(1, 0)], maps[(1, 0)])
    with torch.no_grad():
        assert torch.equal(model(x), y)


@pytest.mark.parametrize("pow2", [True, False], ids=["pow2", "natural"])
@pytest.mark.parametrize("which", ["A", "B2"])
def test_ibert_engine_maps_equal_the_models_hooks(which, pow2):
    """all three operators 'ibert': model(x) does not dispatch that family, so model.attention_maps answers from the hooks;
    engine_from_model(model).attention_maps is the engine route"""
    model, x = built(which, pow2, IBERT_OPS)
    B = x.shape[0]
    shapes = _shapes(model, B)
    with torch.no_grad():
        assert not model.takes_engine(x)
        ref, scale_r = model.attention_maps(x)
        eng = engine_from_model(model, max_batch=4)
        maps, scale = eng.attention_maps(x.contiguous().float())
        one, _ = eng.attention_maps(x.contiguous().float(), blocks=[(0, 1)])
    assert scale == scale_r == 2.0 ** -7 and list(maps) == list(ref) == sorted(shapes)
    for key, shape in shapes.items():
        assert tuple(maps[key].shape) == tuple(ref[key].shape) == shape
        assert torch.equal(maps[key], ref[key]), f"block {key}: {int((maps[key] != ref[key]).sum())} of {maps[key].numel()} bytes differ"
        assert 8 < int(maps[key].max()) <= 128
    assert torch.equal(one[(0, 1)], maps[(0, 1)])


def test_a_16_bit_softmax_is_refused_on_both_paths():
    model, x = built("A", True, IVIT_OPS)
    sm = model.layers[0].blocks[1].attn.log_int_softmax
    sm.output_bit = 16
    try:
        with torch.no_grad():
            assert model.takes_engine(x)
            with pytest.raises(ValueError, match="16 bits"):
                model.attention_maps(x)
            with pytest.raises(ValueError, match="16 bits"):
                _hook_maps(model, x)
    finally:
        sm.output_bit = 8
