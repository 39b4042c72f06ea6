"""Linear probe on the int8 feature bank, on the GPU: ivit_gram_i8_i64 (with ivit_gram_workspace_bytes) and ivit_group_sums_i8_i64
against tests/probe_ref.py, bit for bit -- the geometry sweep over every number of row segments, short and empty segments, the value
extremes, a sum beyond int32, accumulation, fenced operands, the refusals with sentinel-filled outputs -- then probe.BankStats /
LinearProbe against the reference's integers, and inference.evaluate_linear_probe and LinearProbe.load_into end to end on a
synthetic DeiT-Tiny-width model of depth 2."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
from ivit_amd.inference import evaluate_linear_probe, extract_features  # noqa: E402
from ivit_amd.knn import FeatureBank  # noqa: E402
from ivit_amd.probe import BankStats, LinearProbe  # noqa: E402

import fenced  # noqa: E402
import probe_ref  # noqa: E402

DEV = "cuda:0"
ROWS = (0, 1, 2, 63, 64, 65, 1000)
SPLITS = (0, 1, 2, 3, 64)
SENT = -0x5555555555555556      # 0xAAAA... in every byte of an int64 output


def st():
    return _lib.stream_ptr()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rand8(rng, rows, c):
    return rng.integers(-128, 128, size=(rows, c)).astype(np.int8)


def gram_workspace(rows, Cc, splits):
    need = C.c_int64(-1)
    _lib.call("ivit_gram_workspace_bytes", rows, Cc, splits, C.byref(need))
    assert need.value >= 0 and need.value % 4 == 0 and (need.value > 0) == (rows > 0)
    return torch.empty(max(need.value // 4, 1), dtype=torch.int32, device=DEV), need.value


def gram_gpu(xd, rows, Cc, splits, accumulate=0, start=None):
    """dense device rows -> the int64 Gram as numpy (on top of `start` with accumulate = 1)"""
    ws, need = gram_workspace(rows, Cc, splits)
    out = torch.full((Cc, Cc), SENT, dtype=torch.int64, device=DEV) if start is None else dev(start)
    _lib.call("ivit_gram_i8_i64", _lib.ptr(xd), xd.stride(0), rows, Cc, splits, accumulate, _lib.ptr(out), _lib.ptr(ws), need, st())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def sums_gpu(xd, rows, Cc, perm, ptr, accumulate=0, start=None):
    groups = len(ptr) - 1
    out = torch.full((groups, Cc), SENT, dtype=torch.int64, device=DEV) if start is None else dev(start)
    pd, gd = dev(np.asarray(perm, np.int32) if len(perm) else np.zeros(1, np.int32)), dev(np.asarray(ptr, np.int64))
    _lib.call("ivit_group_sums_i8_i64", _lib.ptr(xd), xd.stride(0), rows, Cc, _lib.ptr(pd), _lib.ptr(gd), groups, accumulate, _lib.ptr(out), st())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def as_dwords(a64):
    """an int64 matrix as the int32 matrix of twice the width that lies in the same memory (tests/fenced.py knows 1, 2 and 4 bytes)"""
    a64 = np.ascontiguousarray(a64, np.int64)
    return a64.view(np.int32).reshape(a64.shape[0], -1)


def guards_untouched(buf):
    raw = buf.fetch()
    fill = np.array([buf.fill]).astype(buf.dtype).view(np.uint8)
    for part in (raw[:buf.start], raw[buf.start + buf.body:]):
        assert (part.reshape(-1, fill.size) == fill).all(), "a guard of the workspace was written"


# =========================================================================================== Gram: geometry sweep
@pytest.mark.parametrize("Cc", [64, 128, 192, 1024])
def test_gram_geometry_sweep(Cc):
    rng = np.random.default_rng(Cc)
    x = rand8(rng, max(ROWS), Cc)
    x[0, 0], x[-1, -1] = -128, 127
    xd = dev(x)
    for rows in ROWS:
        exp = probe_ref.gram(x[:rows])
        for sp in (0, 1, 3, 64):                      # 64: more segments than 64-row tiles -- short and empty segments
            got = gram_gpu(xd, rows, Cc, sp)
            assert np.array_equal(got, exp), f"C={Cc} rows={rows} splits={sp}"
            assert np.array_equal(got, got.T)


def test_gram_70000_rows_every_split_and_accumulate():
    rng = np.random.default_rng(1)
    rows, Cc = 70000, 192
    x = rand8(rng, rows, Cc)
    xd = dev(x)
    exp = probe_ref.gram(x)
    for sp in SPLITS:
        got = gram_gpu(xd, rows, Cc, sp)
        assert np.array_equal(got, exp) and np.array_equal(got, got.T), f"splits={sp}"
    start = rng.integers(-2 ** 62, 2 ** 62, size=(Cc, Cc))
    assert np.array_equal(gram_gpu(xd, rows, Cc, 3, accumulate=1, start=start), start + exp)
    assert np.array_equal(gram_gpu(xd, 0, Cc, 0, accumulate=1, start=start), start)          # a sum over nothing, added
    assert not gram_gpu(xd, 0, Cc, 0).any()                                                  # ... and written


@pytest.mark.parametrize("Cc", [64, 1024])
def test_gram_value_extremes(Cc):
    rows = 1000
    low = np.full((rows, Cc), -128, np.int8)
    alt = low.copy()
    alt[:, 1::2] = 127
    for x in (low, alt):
        exp = probe_ref.gram(x)
        assert exp[0, 0] == rows * 2 ** 14 and exp.min() >= -rows * 128 * 127
        for sp in (1, 3):
            assert np.array_equal(gram_gpu(dev(x), rows, Cc, sp), exp)


def test_gram_beyond_int32_in_one_segment():
    rows = 140000                                     # every entry is 140000 * 2^14 > 2^31: an int32-only accumulation fails here
    x = torch.full((rows, 64), -128, dtype=torch.int8, device=DEV)
    got = gram_gpu(x, rows, 64, 1)
    assert (got == rows * 2 ** 14).all() and rows * 2 ** 14 > 2 ** 31


# =========================================================================================== Gram: fenced operands
@pytest.mark.parametrize("splits", [1, 3])
def test_gram_fenced_operands(splits):
    rng = np.random.default_rng(2)
    rows, Cc = 150, 128
    x = rand8(rng, rows, Cc)
    exp = probe_ref.gram(x)
    xf = fenced.input(x, Cc + 16, 127, oracle=lambda m: as_dwords(probe_ref.gram(m[:, 4:])), expected=as_dwords(exp))
    out = fenced.output(Cc, 2 * Cc, 2 * Cc, np.int32, expected=as_dwords(exp))
    need = C.c_int64()
    _lib.call("ivit_gram_workspace_bytes", rows, Cc, splits, C.byref(need))
    ws = fenced.output(1, need.value // 4, need.value // 4, np.int32, sentinel=fenced.SENTINELS[4][0])
    ldx = xf.ld
    _lib.call("ivit_gram_i8_i64", xf.ptr, ldx, rows, Cc, splits, 0, out.ptr, ws.ptr, need.value, st())
    torch.cuda.synchronize()
    fenced.check(out, as_dwords(exp))
    fenced.check(xf)
    guards_untouched(ws)


# =========================================================================================== Gram: refusals
def test_gram_refusals_leave_the_output_untouched():
    L = _lib.lib()
    rng = np.random.default_rng(3)
    rows, Cc = 300, 128
    wide = dev(rand8(rng, rows, 1104))                # rows wide enough for every C tried
    out = torch.full((1088 * 1088,), SENT, dtype=torch.int64, device=DEV)
    ws = torch.full((3 * 1088 * 1088 + 8,), -3, dtype=torch.int32, device=DEV)
    big = ws.numel() * 4

    def run(x=wide, ldx=1104, r=rows, Cn=Cc, splits=3, accumulate=0, o=out, w=ws, wb=big, xoff=0):
        xp = None if x is None else C.c_void_p(x.data_ptr() + xoff)
        return L.ivit_gram_i8_i64(xp, ldx, r, Cn, splits, accumulate, _lib.ptr(o), _lib.ptr(w), wb, st())

    assert run(x=None) == -1 and run(o=None) == -1 and run(w=None) == -1
    assert run(Cn=32) == -2 and run(Cn=96) == -2 and run(Cn=1088) == -2
    assert b"unsupported geometry" in L.ivit_last_error_string()
    assert run(ldx=64) == -1 and run(ldx=1104 + 8) == -1 and run(xoff=8) == -1
    assert run(splits=65) == -1 and run(splits=-1) == -1
    assert run(accumulate=2) == -1 and run(accumulate=-1) == -1
    assert run(r=-1) == -1 and run(r=2 ** 31) == -1
    need = C.c_int64()
    _lib.call("ivit_gram_workspace_bytes", rows, Cc, 3, C.byref(need))
    assert need.value == 3 * Cc * Cc * 4              # three segments of 128 rows, one int32 slab each
    assert run(wb=need.value - 8) == -1
    assert L.ivit_gram_workspace_bytes(rows, 96, 3, C.byref(need)) == -2 and L.ivit_gram_workspace_bytes(rows, Cc, 65, C.byref(need)) == -1
    assert L.ivit_gram_workspace_bytes(-1, Cc, 3, C.byref(need)) == -1 and L.ivit_gram_workspace_bytes(rows, Cc, 3, None) == -1
    torch.cuda.synchronize()
    assert (out == SENT).all() and (ws == -3).all()
    assert run(wb=3 * Cc * Cc * 4) == 0               # ... and the same call with the workspace it asked for runs
    torch.cuda.synchronize()
    assert np.array_equal(out[:Cc * Cc].view(Cc, Cc).cpu().numpy(), probe_ref.gram(wide.cpu().numpy()[:, :Cc]))
    assert (out[Cc * Cc:] == SENT).all() and (ws[3 * Cc * Cc:] == -3).all()


# =========================================================================================== group sums
@pytest.mark.parametrize("groups", [1, 2, 10, 1000])
@pytest.mark.parametrize("Cc", [64, 192, 1024])
def test_group_sums_sweep(Cc, groups):
    rng = np.random.default_rng(Cc + groups)
    x = rand8(rng, max(ROWS), Cc)
    x[0, 0], x[-1, -1] = -128, 127
    xd = dev(x)
    for rows in ROWS:
        labels = rng.integers(0, groups, size=rows)
        perm, ptr = probe_ref.csr(labels, groups)
        assert np.array_equal(sums_gpu(xd, rows, Cc, perm, ptr), probe_ref.group_sums(x, perm, ptr)), f"C={Cc} groups={groups} rows={rows}"


def test_group_sums_empty_groups_one_group_and_a_shuffled_perm():
    rng = np.random.default_rng(4)
    rows, Cc = 1000, 192
    x = rand8(rng, rows, Cc)
    xd = dev(x)
    labels = rng.choice([2, 3, 5, 6], size=rows)      # empty groups at the front (0, 1), in the middle (4) and at the end (7, 8)
    perm, ptr = probe_ref.csr(labels, 9)
    exp = probe_ref.group_sums(x, perm, ptr)
    got = sums_gpu(xd, rows, Cc, perm, ptr)
    assert np.array_equal(got, exp) and not got[[0, 1, 4, 7, 8]].any() and got[2].any()
    for g in range(9):                                # not the identity within a group: the sums do not depend on the order
        rng.shuffle(perm[ptr[g]:ptr[g + 1]])
    assert np.array_equal(sums_gpu(xd, rows, Cc, perm, ptr), exp)
    perm1, ptr1 = probe_ref.csr(np.zeros(rows, np.int64), 1)
    assert np.array_equal(sums_gpu(xd, rows, Cc, perm1, ptr1)[0], x.astype(np.int64).sum(axis=0))      # one group holding every row
    low = torch.full((rows, Cc), -128, dtype=torch.int8, device=DEV)
    assert (sums_gpu(low, rows, Cc, perm1, ptr1) == -128 * rows).all()
    start = rng.integers(-2 ** 62, 2 ** 62, size=(9, Cc))
    assert np.array_equal(sums_gpu(xd, rows, Cc, perm, ptr, accumulate=1, start=start), start + exp)


def test_group_sums_fenced_operands():
    rng = np.random.default_rng(5)
    rows, Cc, groups = 150, 128, 7
    x = rand8(rng, rows, Cc)
    perm, ptr = probe_ref.csr(rng.integers(0, groups, size=rows), groups)
    assert (np.diff(ptr) > 0).all()
    exp = probe_ref.group_sums(x, perm, ptr)
    xf = fenced.input(x, Cc + 16, 127, oracle=lambda m: as_dwords(probe_ref.group_sums(m[:, 4:], perm, ptr)), expected=as_dwords(exp))
    pf = fenced.input(perm[None, :], rows, 0)
    gf = fenced.input(as_dwords(ptr[None, :]), 2 * (groups + 1), 2 ** 30)
    out = fenced.output(groups, 2 * Cc, 2 * Cc, np.int32, expected=as_dwords(exp))
    ldx = xf.ld
    _lib.call("ivit_group_sums_i8_i64", xf.ptr, ldx, rows, Cc, pf.ptr, gf.ptr, groups, 0, out.ptr, st())
    torch.cuda.synchronize()
    fenced.check(out, as_dwords(exp))
    for b in (xf, pf, gf):
        fenced.check(b)


def test_group_sums_refusals_leave_the_output_untouched():
    L = _lib.lib()
    rng = np.random.default_rng(6)
    rows = 100
    wide = dev(rand8(rng, rows, 1104))
    perm, ptr = probe_ref.csr(rng.integers(0, 5, size=rows), 5)
    pd, gd = dev(perm), dev(ptr)
    out = torch.full((5 * 1088,), SENT, dtype=torch.int64, device=DEV)

    def run(x=wide, ldx=1104, r=rows, Cn=128, p=pd, g=gd, groups=5, accumulate=0, o=out, xoff=0):
        xp = None if x is None else C.c_void_p(x.data_ptr() + xoff)
        return L.ivit_group_sums_i8_i64(xp, ldx, r, Cn, _lib.ptr(p), _lib.ptr(g), groups, accumulate, _lib.ptr(o), st())

    assert run(x=None) == -1 and run(p=None) == -1 and run(g=None) == -1 and run(o=None) == -1
    assert run(Cn=32) == -2 and run(Cn=96) == -2 and run(Cn=1088) == -2
    assert run(ldx=64) == -1 and run(ldx=1104 + 8) == -1 and run(xoff=8) == -1
    assert run(groups=0) == -1 and run(groups=2 ** 20 + 1) == -1
    assert run(accumulate=2) == -1 and run(r=-1) == -1 and run(r=2 ** 31) == -1
    torch.cuda.synchronize()
    assert (out == SENT).all()
    assert run() == 0
    torch.cuda.synchronize()
    assert np.array_equal(out[:5 * 128].view(5, 128).cpu().numpy(), probe_ref.group_sums(wide.cpu().numpy()[:, :128], perm, ptr))


# =========================================================================================== the Python layer
def test_bank_stats_batches_from_bank_and_bad_labels():
    rng = np.random.default_rng(7)
    x, labels = rand8(rng, 500, 192), rng.integers(0, 10, size=500)
    store = dev(np.pad(x, ((0, 0), (0, 64))))         # the rows as a view of a wider buffer: used in place
    rows, lab = store[:, :192], torch.from_numpy(labels).to(DEV)
    G, S, n = probe_ref.stats(x, labels, 10)
    whole = BankStats(192, 10, DEV).update(rows, lab, 0.04)
    parts = BankStats(192, 10, DEV)
    for lo, hi in ((0, 7), (7, 300), (300, 500)):
        parts.update(rows[lo:hi], lab[lo:hi], 0.04)
    fb = FeatureBank(rows, lab, 0.04)
    for s in (whole, parts, BankStats.from_bank(fb, 10)):
        assert np.array_equal(s.gram.cpu().numpy(), G) and np.array_equal(s.sums.cpu().numpy(), S) and np.array_equal(s.counts.cpu().numpy(), n)
    merged = BankStats(192, 10, DEV).update(rows[:100], lab[:100], 0.04).merge(BankStats(192, 10, DEV).update(rows[100:], lab[100:], 0.04))
    assert torch.equal(merged.gram, whole.gram) and torch.equal(merged.sums, whole.sums) and torch.equal(merged.counts, whole.counts)
    names, orig = [], _lib.call
    _lib.call = lambda name, *a: (names.append(name), orig(name, *a))[1]
    try:
        for bad in (-1, 10):
            lb = lab.clone()
            lb[123] = bad
            with pytest.raises(ValueError, match=f"label {bad} "):
                whole.update(rows, lb, 0.04)
    finally:
        _lib.call = orig
    assert names == [] and np.array_equal(whole.gram.cpu().numpy(), G)


GEN = probe_ref.generator()


def test_linear_probe_logits_and_topk_equal_the_reference_integers():
    bank, labels, q, targets, scale = GEN
    stats = BankStats(192, 10, DEV).update(dev(bank), dev(labels), scale)
    G, S, n = probe_ref.stats(bank, labels, 10)
    assert np.array_equal(stats.gram.cpu().numpy(), G) and np.array_equal(stats.sums.cpu().numpy(), S)
    qd, td = dev(q), dev(targets.astype(np.int32))
    for probe in (stats.ridge(1e-3), stats.ridge(1.0), stats.ncm()):
        assert isinstance(probe, LinearProbe)
        racc, rlg = probe_ref.int_logits(q, probe.W, probe.b, probe.scale)
        acc, lg = probe.logits(qd)
        assert np.array_equal(acc.cpu().numpy(), racc) and np.array_equal(lg.cpu().numpy().view(np.int32), rlg.view(np.int32))
        hits = torch.zeros(5, dtype=torch.int64, device=DEV)
        top = probe.topk(qd, 5, td, hits)
        rtop = probe_ref.topk(rlg, 5)
        assert np.array_equal(top.cpu().numpy(), rtop) and np.array_equal(hits.cpu().numpy(), probe_ref.hits(rtop, targets))
        assert int(hits[0]) == 500                    # (what tests/test_probe_cpu.py shows of the reference on this data)


_MODEL = {}


def _model(K):
    """a calibrated, frozen DeiT-Tiny-width ViT of depth 2 with K classes, and 48 images for it"""
    if K not in _MODEL:
        from test_gpu_vit16_lazy import W8, _images
        torch.manual_seed(192 + K)
        model = ivit.VisionTransformer(img_size=224, patch_size=16, embed_dim=192, depth=2, num_heads=3, mlp_ratio=4, qkv_bias=True,
                                       num_classes=K, gelu_type="ivit", softmax_type="ivit", layernorm_type="ivit", **W8).to(DEV).eval()
        g = torch.Generator(device="cpu").manual_seed(13)
        imgs = _images(48, 224, g)
        with torch.no_grad():
            for p in model.parameters():
                if p.dim() > 1:
                    p.mul_(3.0)
            model(imgs[:4])
            model(imgs[4:8].flip(0) * 0.7)
        ivit.freeze_model(model)
        _MODEL[K] = (model, imgs)
    return _MODEL[K]


def test_evaluate_linear_probe_end_to_end_and_load_into():
    K = 6
    model, imgs = _model(K)
    labels = torch.arange(48) % K
    loader = [(imgs[i:i + 16], labels[i:i + 16]) for i in range(0, 48, 16)]
    rows, lab, scale = extract_features(model, loader, DEV, integers=True)
    assert rows.dtype == torch.int8 and rows.shape == (48, 192)
    x, y, s = rows.cpu().numpy(), lab.cpu().numpy(), float(torch.as_tensor(scale).reshape(-1)[0])
    G, S, n = probe_ref.stats(x, y, K)
    lams = (1e-2, 1.0)
    got = evaluate_linear_probe(model, loader, loader, DEV, K, lam=lams)
    for lam in lams:
        W, b, _ = probe_ref.ridge(G, S, n, lam, s)
        assert got[lam] == probe_ref.percentages(probe_ref.topk(probe_ref.int_logits(x, W, b, s)[1], 5), y)
    W, b = probe_ref.ncm(S, n, s)
    got = evaluate_linear_probe(model, loader, loader, DEV, K, kind="ncm")
    assert got == {None: probe_ref.percentages(probe_ref.topk(probe_ref.int_logits(x, W, b, s)[1], 5), y)}
    # the probe inside model(x): the head's weights replaced in place, the logits those of the probe on the model's own features
    probe = BankStats(192, K, DEV).update(rows, lab, scale).ridge(1e-2)
    before = model(imgs[:8])
    probe.load_into(model)
    with torch.no_grad():
        after = model(imgs[:8])
        feats = model.features(imgs[:8], integers=True)[0]
    _, lg = probe.logits(feats)
    assert after.shape == (8, K) and not torch.equal(after, before)
    assert torch.equal(after.view(torch.int32), lg.contiguous().view(torch.int32))
