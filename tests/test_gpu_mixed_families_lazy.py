"""DeiT-T with each of the six non-uniform 'ivit' / 'ibert' operator mixtures on the integer-carrying module path
(quantization_utils/lazy.py resolves every site by its own module): the logits equal the literal module path bit for bit, nothing
inside the blocks materialises, and the fused engine still declines the model for its operator family."""
import itertools
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
import ivit_amd.quantization_utils as qu  # noqa: E402
from ivit_amd import synth  # noqa: E402
from ivit_amd.quantization_utils import lazy  # noqa: E402

DEV = "cuda:0"
MIXTURES = [m for m in itertools.product(("ivit", "ibert"), repeat=3) if len(set(m)) == 2]


def build(mix, pow2):
    fs = synth.make_float_state("deit_tiny_patch16_224", 5)
    model = ivit.deit_tiny_patch16_224(gelu_type=mix[0], softmax_type=mix[1], layernorm_type=mix[2])
    model.load_state_dict({k: torch.from_numpy(v) for k, v in fs.items()}, strict=False)
    model.to(DEV).eval()
    with torch.no_grad():
        model(torch.from_numpy(synth.make_images(2, 3)).to(DEV))          # calibration forward (running min / max)
    if pow2:
        for mod in model.modules():
            if isinstance(mod, qu.QuantAct):
                qmax = 2 ** (mod.activation_bit - 1) - 1
                a = max(-float(mod.x_min), float(mod.x_max)) / qmax
                p = 2.0 ** np.ceil(np.log2(a))
                mod.x_max.fill_(qmax * p)
                mod.x_min.fill_(-qmax * p)
    ivit.freeze_model(model)
    return model


def run(model, x, lazy_on):
    old = lazy.ENABLED
    try:
        lazy.ENABLED = lazy_on
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return model(x)
    finally:
        lazy.ENABLED = old


@pytest.mark.parametrize("pow2", [True, False], ids=["pow2", "natural"])
@pytest.mark.parametrize("mix", MIXTURES, ids=["-".join(m) for m in MIXTURES])
def test_mixture_carries_integers_and_equals_the_literal_path(mix, pow2):
    assert len(MIXTURES) == 6
    model = build(mix, pow2)
    x = torch.from_numpy(synth.make_images(2, 41)).to(DEV)
    assert "operator family" in model.engine_unsupported_reason() and not model.takes_engine(x)
    y_plain = run(model, x, False)
    run(model, x, True)                                   # warm-up: constants and tables
    lazy.STATS.update(fused=0, materialised=0)
    y = run(model, x, True)
    stats = dict(lazy.STATS)
    assert torch.equal(y, y_plain) and len(torch.unique(y_plain)) > 2
    # the one materialisation of a forward is the logits handed to the caller; nothing inside the blocks
    assert stats["materialised"] == 1, stats
    # per block: norm1, qkv, attention, proj, residual, norm2, fc1, GELU, fc2, residual; patch embedding, position, final norm + class row
    assert stats["fused"] >= 10 * model.depth, stats
