"""The dense linear probe on the CPU: tests/dense_ref.py (the exact integer specification the GPU tests compare with) is torch's
bilinear interpolation with align_corners=False wherever float64 can tell the two best classes apart, and dense.miou on
hand-computed matrices."""
import numpy as np
import pytest
import torch

from ivit_amd.dense import miou

import dense_ref


@pytest.mark.parametrize("B,gh,gw,r,classes,np_", dense_ref.CASES)
def test_reference_is_torch_bilinear_argmax(B, gh, gw, r, classes, np_):
    """the seeds of the GPU sweep: the reference's smallest top-2 relative margin stays above 1e-9, far above the error of torch's
    float64 interpolation (a few ulp of 2^-53), so both must name the same class at every pixel"""
    rng = np.random.default_rng(B + 10 * gh + 100 * gw + 1000 * r + classes)
    acc, s = dense_ref.random_case(rng.integers(1 << 30), B, gh, gw, classes, np_)
    assert dense_ref.margin(acc, s, classes, r) > 1e-9
    logits = torch.from_numpy(acc[..., :classes].astype(np.float64) * s[:classes].astype(np.float64)).permute(0, 3, 1, 2)
    up = torch.nn.functional.interpolate(logits, size=(gh * r, gw * r), mode="bilinear", align_corners=False)
    assert np.array_equal(up.argmax(1).numpy().astype(np.uint8), dense_ref.argmax(acc, s, classes, r))


def test_miou_on_hand_computed_matrices():
    m, pa, iou = miou(np.array([[3, 1, 0], [2, 4, 0], [0, 0, 0]]))      # class 2 absent from target and prediction
    assert np.allclose(iou[:2], [3 / 6, 4 / 7]) and np.isnan(iou[2])
    assert m == pytest.approx((3 / 6 + 4 / 7) / 2) and pa == pytest.approx(0.7)
    m, pa, iou = miou(torch.tensor([[0, 5], [0, 0]]))                   # predicted but never a target: IoU 0, in the mean
    assert (m, pa, iou.tolist()) == (0.0, 0.0, [0.0, 0.0])
    m, pa, iou = miou(np.zeros((2, 2), np.int64))
    assert np.isnan(m) and np.isnan(pa) and np.isnan(iou).all()
