"""The host side of the video segmentation scoring without a GPU: propagate.davis_measures on hand-written counts, the tolerance
rule, and the new names in the header, the ctypes table, the library and the package."""
import pytest
import torch

import ivit_amd
from ivit_amd import _lib, propagate

from test_abi_coverage_cpu import declared_names


def test_davis_measures_on_hand_written_counts():
    counts = torch.tensor([[[30, 40, 10, 20, 5, 15],       # ordinary: J = 3/4, P = 1/2, R = 3/4, F = 2 * 3/8 / (5/4) = 3/5
                            [0, 0, 0, 0, 0, 0],            # nothing anywhere: J = 1, P = R = 1
                            [0, 9, 0, 7, 0, 0],            # no predicted boundary: P = 1, R = 0
                            [0, 9, 7, 0, 0, 0],            # no true boundary: P = 0, R = 1
                            [0, 9, 7, 7, 0, 0]]])          # boundaries that never meet: P + R = 0
    J, F = propagate.davis_measures(counts)
    assert J.dtype == F.dtype == torch.float64 and J.shape == F.shape == (1, 5)
    assert J[0].tolist() == [0.75, 1.0, 0.0, 0.0, 0.0]
    assert F[0].tolist() == [pytest.approx(0.6, abs=1e-15), 1.0, 0.0, 0.0, 0.0]
    with pytest.raises(ValueError, match="n, O, 6"):
        propagate.davis_measures(torch.zeros(3, 5))


def test_bound_radius_rule():
    assert propagate.bound_radius(0.008, 480, 854) == 8 and propagate.bound_radius(3, 480, 854) == 3 and propagate.bound_radius(0, 9, 9) == 0


def test_new_names_are_declared_bound_and_exported():
    for name in ("ivit_upsample_argmax_u8", "ivit_mask_scores_u8"):
        assert name in declared_names() and name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert _lib.SIGNATURES["ivit_mask_scores_u8"] == [_lib.vp, _lib.vp] + [_lib.ci] * 5 + [_lib.vp, _lib.vp]
    assert ivit_amd.upsample_argmax is propagate.upsample_argmax and ivit_amd.mask_scores is propagate.mask_scores
    assert ivit_amd.davis_measures is propagate.davis_measures
    assert (propagate.R_MAX, propagate.OBJECTS_MAX, propagate.RADIUS_MAX) == (32, 255, 24)
