"""graph.ModuleGraph on the GPU: `forward_graph` of frozen models the fused engines decline against the eager `model(x)`, bit for
bit, for three different inputs through ONE captured graph (a baked-in input would pass one); no Python launch on a replay;
invalidation by an in-place range edit; a resident input; the engine case; the refusals; the `graph=` keyword of the evaluation
functions.  Small models: DeiT with embed_dim 128, depth 2, 2 heads, 10 classes at batch 2, and the small Swin of
tests/test_gpu_swin_ibert_lazy.py."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
import ivit_amd.quantization_utils as qu  # noqa: E402
from ivit_amd import _lib, inference  # noqa: E402

from test_gpu_mixed_families_lazy import build as build_deit_tiny  # noqa: E402
from test_gpu_swin_ibert_lazy import built as built_swin  # noqa: E402
from test_gpu_vit16_lazy import DEV, W8, W16, _Trace, _images  # noqa: E402
from test_gpu_w4_lazy import W4, _calibrated as calibrated_w4  # noqa: E402

IVIT = ("ivit", "ivit", "ivit")
_BUILT = {}


def _deit(img, ops=IVIT, widths=W8, peak=4.0):
    """a calibrated, frozen DeiT (ranges snapped to powers of two), built once per configuration and shared; tests that change a
    range restore it"""
    key = (img, ops, tuple(sorted(widths.items())), peak)
    if key not in _BUILT:
        torch.manual_seed(img + 16 + 128)
        model = ivit.VisionTransformer(img_size=img, patch_size=16, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4, qkv_bias=True,
                                       num_classes=10, gelu_type=ops[0], softmax_type=ops[1], layernorm_type=ops[2], **widths).to(DEV).eval()
        with torch.no_grad():
            for p in model.parameters():          # wider weights than the init's 0.02: activations that use their ranges
                if p.dim() > 1:
                    p.mul_(3.0)
            if 4 in widths.values():              # as tests/test_gpu_w4_lazy.py draws them: at the init's 0.02 the class row is all zeros
                model.cls_token.normal_(0.0, 2.0)
                model.pos_embed.normal_(0.0, 0.7)
            for blk in model.blocks:              # peaked attention (at 4 bits a row of 197 keys needs a sharp peak to hold 1/8 at all)
                blk.attn.qkv.weight.mul_(peak)
            g = torch.Generator(device="cpu").manual_seed(3)
            calib = _images(4, img, g)
            model(calib)
            model(calib.flip(0) * 0.7)
        for mod in model.modules():
            if isinstance(mod, qu.QuantAct):
                qmax = 2 ** (mod.activation_bit - 1) - 1
                a = max(-float(mod.x_min), float(mod.x_max)) / qmax
                assert a > 0, "a QuantAct of the test model saw nothing but zeros"
                p2 = 2.0 ** np.ceil(np.log2(a))
                mod.x_max.fill_(qmax * p2)
                mod.x_min.fill_(-qmax * p2)
        ivit.freeze_model(model)
        _BUILT[key] = (model, [_images(2, img, g) for _ in range(3)])
    return _BUILT[key]


def _eager(model, x):
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return model(x).clone()


def _replayed(model, x, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return model.forward_graph(x, **kw)


def _check(model, xs, distinct=True):
    """forward_graph == model(x) for every input of `xs` through one captured graph -> the launches of the capturing call"""
    assert not model.takes_engine(xs[0]), "the case must cover the module path"
    want = [_eager(model, x) for x in xs]         # (all eager calls first: a literal step's eager call moves published buffers)
    if distinct:
        assert not torch.equal(want[0], want[1]) and not torch.equal(want[1], want[2]), "the inputs must tell the results apart"
    model.drop_graphs()
    try:
        with _Trace() as tr:
            first = _replayed(model, xs[0]).clone()
        assert torch.equal(first, want[0])
        (key, entry), = model._graphs.items()
        assert key == (xs[0].shape[0], torch.float32)
        for x, w in zip(xs, want):
            y = _replayed(model, x)
            assert y.dtype == torch.float32 and tuple(y.shape) == tuple(w.shape) and torch.equal(y, w)
        assert list(model._graphs) == [key] and model._graphs[key] is entry, "the three inputs must go through one captured graph"
        model.graph_status()
    finally:
        model.drop_graphs()
    return tr.names


# ----------------------------------------------------------------------------------- 1 .. 4: configurations the engines decline
@pytest.mark.parametrize("ops", [("ibert", "ivit", "ivit"), ("ivit", "ibert", "ibert")], ids="-".join)
def test_deit_operator_mixtures(ops):
    model, xs = _deit(224, ops)
    assert "operator family" in model.engine_unsupported_reason()
    names = _check(model, xs)
    assert len([n for n in names if n.startswith("ivit_attention_fused")]) == 3 * 2      # two warm-up forwards and the capture


def test_deit_16_bit_stream_at_257_tokens():
    model, xs = _deit(256, widths=W16)
    assert "257 tokens" in model.engine_unsupported_reason()
    names = _check(model, xs)
    fused = [n for n in names if n.startswith("ivit_attention_fused")]
    assert len(fused) == 3 * 2 and all("long" in n for n in fused), sorted(set(names))


def test_deit_4_bit_softmax_alone():
    model, xs = _deit(224, widths=dict(W8, softmax_bw=4), peak=16.0)
    assert model.engine_unsupported_reason() is not None
    names = _check(model, xs)
    assert names.count("ivit_attention_fused_i8_wide") == 3 * 2, sorted(set(names))


def test_deit_all_zero_probabilities_keep_shiftmax_literal_inside_the_capture():
    """tests/test_gpu_w4_lazy.py's model whose attn.qact2 was calibrated on zeros: Shiftmax, the two QuantMatMuls and narrow_i8's
    overflow check (now the graph's status word) lie inside the capture.  (With no probability left the class row never sees a patch:
    this model's logits do not depend on the image, so this case cannot tell a baked-in input; the others do.)"""
    model, g = calibrated_w4(224, 16, 128, 2, 2, False, 3, "ivit", W4, peak=1.0)
    model.use_engine = False
    xs = [_images(2, 224, g) for _ in range(3)]
    names = _check(model, xs, distinct=False)
    assert any(n.startswith("ivit_shiftmax") for n in names) and "ivit_narrow_i32_i8" in names and "ivit_bgemm_pv_i32_i8" in names
    assert not [n for n in names if "attention_fused" in n]


@pytest.mark.parametrize("literal_mask", [False, True], ids=["fused", "literal_softmax_core"])
def test_swin_with_ibert_operators(literal_mask):
    """the small Swin, all three operators 'ibert', a shifted block included; then the same model with that block's attn.qact2 at
    +-127 * 0.5 (outside prepare.ibert_window_mask_ok): the literal softmax core -- torch float ops, IBERTIntSoftmax's literal kernel,
    two QuantMatMuls -- lies inside the capture"""
    model, x = built_swin("A", True)
    g = torch.Generator(device="cpu").manual_seed(19)
    xs = [x[:2].clone(), *(_images(2, 56, g) for _ in range(2))]
    blk = model.layers[0].blocks[1]
    assert blk.attn_mask is not None
    qa = blk.attn.qact2
    keep = (qa.x_min.clone(), qa.x_max.clone())
    try:
        if literal_mask:
            qa.x_min.fill_(-127 * 0.5)
            qa.x_max.fill_(127 * 0.5)
        names = _check(model, xs)
    finally:
        qa.x_min.copy_(keep[0])
        qa.x_max.copy_(keep[1])
    n_fused = sum(model.depths) - int(literal_mask)
    assert names.count("ivit_window_attention_i8_ibert") == 3 * n_fused
    assert ("ivit_ibert_softmax_f32_f32" in names) == literal_mask and ("ivit_bgemm_pv_i32_i8" in names) == literal_mask


# ----------------------------------------------------------------------------------- 5: no Python on the replay
def test_a_replay_launches_nothing_from_python():
    model, xs = _deit(224, ("ibert", "ivit", "ivit"))
    model.drop_graphs()
    calls = [0]
    real = _lib.call

    def counting(name, *args):
        calls[0] += 1
        return real(name, *args)
    try:
        _lib.call = counting
        _replayed(model, xs[0])
        assert calls[0] > 0
        calls[0] = 0
        y1 = _replayed(model, xs[1]).clone()
        assert calls[0] == 0
        y2 = _replayed(model, xs[2]).clone()
        assert calls[0] == 0
    finally:
        _lib.call = real
        model.drop_graphs()
    assert torch.equal(y1, _eager(model, xs[1])) and torch.equal(y2, _eager(model, xs[2]))


# ----------------------------------------------------------------------------------- 6: invalidation
def test_an_in_place_range_edit_drops_the_graphs():
    model, xs = _deit(224, ("ivit", "ibert", "ibert"))
    x = xs[0]
    y0 = _eager(model, x)
    model.drop_graphs()
    qa = model.blocks[1].attn.qact3
    keep = float(qa.x_max)
    try:
        assert torch.equal(_replayed(model, x), y0)
        graph = model._graphs[(2, torch.float32)][0]
        qa.x_max.fill_(keep * 0.25)
        qa.x_min.fill_(-keep * 0.25)
        y_graph = _replayed(model, x).clone()                 # the graph path first: it must notice by itself
        assert model._graphs[(2, torch.float32)][0] is not graph
        y_eager = _eager(model, x)
        assert not torch.equal(y_eager, y0), "the edit changed nothing: the test has no teeth"
        assert torch.equal(y_graph, y_eager)
    finally:
        qa.x_max.fill_(keep)
        qa.x_min.fill_(-keep)
    try:
        assert torch.equal(_replayed(model, x), y0)
    finally:
        model.drop_graphs()


# ----------------------------------------------------------------------------------- 7: resident input
def test_resident_input_is_read_in_place():
    model, xs = _deit(224, ("ibert", "ivit", "ivit"))
    want = [_eager(model, x) for x in xs]
    model.drop_graphs()
    buf = xs[0].clone()
    try:
        assert torch.equal(_replayed(model, buf, resident=True), want[0])
        (key, entry), = model._graphs.items()
        assert key == (2, torch.float32, buf.data_ptr()) and entry[1] is buf
        for x, w in zip(xs[1:], want[1:]):
            buf.copy_(x)
            assert torch.equal(_replayed(model, buf, resident=True), w)
        assert list(model._graphs) == [key]
    finally:
        model.drop_graphs()


# ----------------------------------------------------------------------------------- 8: a model the engine takes
def test_engine_models_go_to_the_engines_graph():
    from ivit_amd import synth
    model = build_deit_tiny(IVIT, True)
    xs = [torch.from_numpy(synth.make_images(2, seed)).to(DEV) for seed in (41, 42, 43)]
    assert model.takes_engine(xs[0])
    try:
        for x in xs:
            want = _eager(model, x)
            assert torch.equal(model.forward_graph(x), want)
        assert model._graphs == {} and len(model._engine[2]._graphs) == 1
    finally:
        model.drop_graphs()


# ----------------------------------------------------------------------------------- 9: refusals
def test_refusals():
    torch.manual_seed(2)
    raw = ivit.VisionTransformer(img_size=224, patch_size=16, embed_dim=128, depth=2, num_heads=2, num_classes=10,
                                 gelu_type="ibert").to(DEV).eval()
    x = _images(2, 224, torch.Generator(device="cpu").manual_seed(1))
    with pytest.raises(ValueError, match="not frozen"):
        raw.forward_graph(x)
    assert raw._graphs == {}
    model, xs = _deit(224, ("ibert", "ivit", "ivit"))
    model.drop_graphs()
    model.train()
    try:
        with pytest.raises(ValueError, match="training mode"):
            model.forward_graph(xs[0])
    finally:
        model.eval()
    h = model.blocks[0].attn.register_forward_hook(lambda m, i, o: None)
    try:
        with pytest.raises(ValueError, match=r"blocks\.0\.attn carries a forward hook"):
            model.forward_graph(xs[0])
    finally:
        h.remove()
    assert model._graphs == {}


# ----------------------------------------------------------------------------------- 10: evaluation
def test_evaluation_with_graph_replay_gives_the_same_percentages():
    model, xs = _deit(224, ("ibert", "ivit", "ivit"))
    g = torch.Generator(device="cpu").manual_seed(23)
    sizes = (4, 4, 4, 4, 3)                                   # five batches, the last one ragged
    loader = []
    for i, n in enumerate(sizes):
        imgs = _images(n, 224, g)
        top = _eager(model, imgs).topk(5, dim=1).indices.cpu()
        targets = torch.where(torch.arange(n) % 3 == 0, top[:, 0], torch.where(torch.arange(n) % 3 == 1, top[:, 2], (top[:, 0] + 5) % 10))
        loader.append((imgs.cpu(), targets))
    model.drop_graphs()
    try:
        eager = inference.evaluate_dataset(model, loader, DEV, print_batch_stats=False)
        replayed = inference.evaluate_dataset(model, loader, DEV, print_batch_stats=False, graph=True)
        assert sorted(k[0] for k in model._graphs) == [3, 4]
        assert replayed == eager and 0 < eager[0] < eager[1] <= eager[2] <= 100, (eager, replayed)
        eager_p = inference.evaluate_dataset_parallel(model, loader, DEV, print_batch_stats=False)
        replayed_p = inference.evaluate_dataset_parallel(model, loader, DEV, print_batch_stats=False, graph=True)
        assert replayed_p == eager_p and 0 < eager_p[0] < eager_p[1], (eager_p, replayed_p)
    finally:
        model.drop_graphs()
