"""Every kernel that computes a Shiftmax, on rows whose exponent sum reaches 2^24, against the reference's own outputs
(tests/golden/shiftmax_bigsum_kat.npz; tests/test_shiftmax_bigsum_cpu.py checks the fixture and the host side).  There the
reference's float32 sum depends on the order of torch's CPU kernel, and the exact sum rounded once gives other outputs on the
rows of class (c): a kernel that takes the wrong sum fails on exactly those, and the messages below say on how many.

A fixture row enters a fused entry as the construction of test_gpu_cls_tail._crafted: query 0 = 64 in every d, key j = a_j in every
d, score multiplier 2^-12 (2^-11 at head_dim 32), so query 0's requantised scores are the row a.  One crafted row per (image,
head); V and the other queries are random.  Expected: oracle P.V and requantisation, P of query 0 being the fixture's column.
The output multiplier (2^-5 at 8 bits, 2^-10 at 16) is chosen so that the other candidate's probabilities show in the output
bytes of every class-(c) row, which is asserted before anything is launched."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
from ivit_amd.prepare import dyadic, phi_table, window_shiftexp_band  # noqa: E402
import attention_ref as A  # noqa: E402
import fenced  # noqa: E402
import shiftmax_order_ref as smo  # noqa: E402
from attention_ref import DEV, dev, release, st  # noqa: E402,F401  (release: the autouse fixture)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHORT_T = (49, 144, 197, 208)
LONG_T = (208, 577, 1025)


@functools.lru_cache(maxsize=None)
def kat(T):
    z = np.load(os.path.join(GOLDEN, "shiftmax_bigsum_kat.npz"))
    ref = z[f"ref_{T}"].astype(np.int32)
    return dict(q=z[f"q_{T}"], s=z[f"s_{T}"], bits=z[f"bits_{T}"].astype(np.int32), cls=z[f"cls_{T}"].astype(np.int32), ref=ref,
                exact=ref + z[f"exact_minus_ref_{T}"].astype(np.int32))


def pick(T, s, bits):
    K = kat(T)
    return np.flatnonzero((K["s"] == np.float32(s)) & (K["bits"] == bits))


def scales(T):
    """the Shiftmax input scales the fixture has rows for at this length"""
    return [float(v) for v in np.unique(kat(T)["s"])]


def natural(s):
    return not orc.phi_is_identity(np.float32(s))


def forms(s):
    return ("band", "exp2d") if natural(s) else ("pow2",)


def rq(O, m, e):
    return orc.requant(np.ascontiguousarray(O).astype(np.int32), m.astype(np.float64), e, 8)


@functools.lru_cache(maxsize=None)
def problem(T, s, bits, hd=64):
    """The fixture rows of (T, s, bits) as one crafted attention problem, batch 1, one head per row -> dict, or None without rows.
    P [H, T, T]: the oracle's probabilities; its query-0 rows are the fixture's reference column (asserted)."""
    m = pick(T, s, bits)
    if not len(m):
        return None
    K, H = kat(T), len(m)
    s = np.float32(s)
    rng = np.random.default_rng(1000 * T + bits + hd)
    qkv = np.clip(np.rint(rng.normal(0, 40, size=(3, 1, H, T, hd))), -128, 127).astype(np.int8)
    qkv[0, 0, :, 0, :] = 64
    qkv[1, 0] = K["q"][m][:, :, None]
    ms, es = dyadic(np.float32(1.0 / (64 * hd)), np.float32(1.0))
    mo, eo = dyadic(np.float32(2.0 ** -10 if bits == 16 else 2.0 ** -5), np.float32(1.0))
    P = np.empty((H, T, T), np.int32)
    for h in range(H):
        ka = orc.requant(orc.gemm_i8(qkv[0, 0, h], qkv[1, 0, h]), ms.astype(np.float64), es, 8)
        assert np.array_equal(ka[0], K["q"][m[h]])
        P[h] = (orc.shiftmax_compat if natural(s) else orc.shiftmax)(ka, s, output_bit=bits)
    assert np.array_equal(P[:, 0], K["ref"][m]), "the oracle is not the reference on the fixture rows (test_shiftmax_bigsum_cpu.py)"
    V = qkv[2, 0].astype(np.int64)
    exp = np.stack([rq(P[h].astype(np.int64) @ V[h], mo, eo) for h in range(H)])                        # [H, T, hd]
    other = np.stack([rq(K["exact"][m[h]][None].astype(np.int64) @ V[h], mo, eo)[0] for h in range(H)])  # query 0, exact-sum candidate
    cls = K["cls"][m]
    shows = np.any(other != exp[:, 0], axis=1)
    assert np.all(shows[cls == smo.CLASS_C]), "a class-(c) row whose other candidate does not reach an output byte"
    return dict(qkv=qkv, s=s, ms=ms, es=es, mo=mo, eo=eo, P=P, exp=exp, cls=cls, H=H, rows=m, other=other)


def verdict(pr, got_q0, got_rest=None, exp_rest=None):
    """'' or what is wrong: crafted rows by class, which candidate the wrong ones took; got_q0 [H, width]"""
    bad = np.any(got_q0 != pr["exp"][:, 0], axis=1) if got_q0.shape[1] == pr["exp"].shape[2] else np.any(got_q0 != pr["P"][:, 0], axis=1)
    msg = []
    if bad.any():
        per = {smo.CLASS_NAMES[c]: f"{int((bad & (pr['cls'] == c)).sum())} of {int((pr['cls'] == c).sum())}" for c in (0, 1, 2)}
        took = ""
        if got_q0.shape[1] == pr["exp"].shape[2]:
            took = f"; {int(np.all(got_q0[bad] == pr['other'][bad], axis=1).sum())} of the wrong rows are the exact-sum candidate"
        msg.append(f"crafted rows wrong per class {per}{took}")
    if got_rest is not None and not np.array_equal(got_rest, exp_rest):
        msg.append(f"{int((got_rest != exp_rest).sum())} bytes of the other queries differ")
    return "; ".join(msg)


def fused(entry, pr, form, bits):
    """-> output [H, T, 64] of one fused ViT entry on the problem"""
    base = (int(pr["ms"][0]), int(pr["es"][0]), float(pr["s"]), int(pr["mo"][0]), int(pr["eo"][0]))
    if entry == "ivit_attention_fused_i8":
        out = A.launch(entry, pr["qkv"], base, 0)
    elif entry == "ivit_attention_fused_i8_compat":
        out = A.launch(entry, pr["qkv"], (*base, A.shiftmax_tables(pr["s"], "exp2d")[0]), 0)
    else:
        out = A.run(entry, pr["qkv"], pr["s"], pr["ms"], pr["es"], pr["mo"], pr["eo"], form, bits, 0)
    T = pr["qkv"].shape[3]
    return out.reshape(T, pr["H"], A.HD).transpose(1, 0, 2)


FUSED = [("ivit_attention_fused_i8", 8, SHORT_T), ("ivit_attention_fused_i8_compat", 8, SHORT_T),
         ("ivit_attention_fused_i8_compat_band", 8, SHORT_T), ("ivit_attention_fused_i8_wide", 8, SHORT_T),
         ("ivit_attention_fused_i8_wide", 16, SHORT_T), ("ivit_attention_fused_i8_long", 8, LONG_T),
         ("ivit_attention_fused_i8_wide_long", 8, LONG_T), ("ivit_attention_fused_i8_wide_long", 16, LONG_T)]


def entry_forms(entry, s):
    if entry == "ivit_attention_fused_i8":
        return () if natural(s) else ("pow2",)
    if entry == "ivit_attention_fused_i8_compat":
        return ("exp2d",) if natural(s) else ()
    return forms(s)


@pytest.mark.parametrize("entry,bits,T", [(e, b, T) for e, b, Ts in FUSED for T in Ts])
def test_fused_vit_entries(entry, bits, T):
    wrong, ran = [], 0
    for s in scales(T):
        pr = problem(T, s, bits)
        for form in entry_forms(entry, s) if pr else ():
            got = fused(entry, pr, form, bits)
            v = verdict(pr, got[:, 0], got[:, 1:], pr["exp"][:, 1:])
            ran += 1
            if v:
                wrong.append(f"s={s} {form}: {v}")
    assert ran, "no fixture row for this entry"
    assert not wrong, f"{entry} softmax_bits={bits} T={T}: " + " | ".join(wrong)


def cls_tail(pr, form):
    qkv, H, T = pr["qkv"], pr["H"], pr["qkv"].shape[3]
    d = dev(qkv)
    q0 = dev(np.ascontiguousarray(qkv[0, :, :, 0, :]).reshape(1, H * A.HD))
    exp = pr["exp"][:, 0].reshape(1, H * A.HD)
    o = fenced.output(1, H * A.HD, H * A.HD + 32, np.int8, expected=exp)
    _lib.call("ivit_attention_cls_i8", _lib.ptr(d[1]), _lib.ptr(d[2]), _lib.ptr(q0), o.ptr, o.ld, 1, H, T, A.HD, int(pr["ms"][0]),
              int(pr["es"][0]), float(pr["s"]), int(pr["mo"][0]), int(pr["eo"][0]), *A.shiftmax_tables(pr["s"], form), st())
    torch.cuda.synchronize()
    got = o.rows2d(o.fetch())[:, :H * A.HD].astype(np.int32).reshape(H, A.HD)
    v = verdict(pr, got)
    if not v:
        fenced.check(o, exp)
    return v


@pytest.mark.parametrize("T", SHORT_T)
def test_class_row_entry(T):
    wrong, ran = [], 0
    for s in scales(T):
        pr = problem(T, s, 8)
        for form in forms(s) if pr else ():
            v = cls_tail(pr, form)
            ran += 1
            if v:
                wrong.append(f"s={s} {form}: {v}")
    assert ran
    assert not wrong, f"ivit_attention_cls_i8 T={T}: " + " | ".join(wrong)


def probs(pr, form, q_rows=16):
    """ivit_attention_probs_u8 -> P [H, q_rows, T], fenced"""
    qkv, H, T = pr["qkv"], pr["H"], pr["qkv"].shape[3]
    exp = pr["P"][:, :q_rows].reshape(H * q_rows, T)
    o = fenced.output(H * q_rows, T, (T + 7) // 4 * 4, np.uint8, expected=exp)
    _lib.call("ivit_attention_probs_u8", _lib.ptr(dev(qkv)), o.ptr, o.ld, 1, H, T, A.HD, q_rows, int(pr["ms"][0]), int(pr["es"][0]),
              float(pr["s"]), *A.shiftmax_tables(pr["s"], form), st())
    torch.cuda.synchronize()
    return o, exp, o.rows2d(o.fetch())[:, :T].astype(np.int32).reshape(H, q_rows, T)


@pytest.mark.parametrize("T", SHORT_T + LONG_T[1:])
def test_probs_entry(T):
    wrong, ran = [], 0
    for s in scales(T):
        pr = problem(T, s, 8)
        for form in forms(s) if pr else ():
            o, exp, got = probs(pr, form)
            v = verdict(pr, got[:, 0], got[:, 1:], pr["P"][:, 1:16])
            ran += 1
            if v:
                wrong.append(f"s={s} {form}: {v}")
            else:
                fenced.check(o, exp)
    assert ran
    assert not wrong, f"ivit_attention_probs_u8 T={T}: " + " | ".join(wrong)


@pytest.mark.parametrize("T", SHORT_T + LONG_T[1:])
def test_probs_times_v_is_the_fused_output(T):
    """test_shiftmax_map_times_v_is_the_fused_output's property where the sum reaches 2^24: the probabilities the probs entry writes,
    multiplied with V and requantised on the host, are the fused entry's output -- on every crafted row, class (c) among them"""
    entry = "ivit_attention_fused_i8_compat_band" if T < 208 else "ivit_attention_fused_i8_long"
    seen_c = 0
    for s in scales(T):
        pr = problem(T, s, 8)
        for form in forms(s) if pr else ():
            _, _, P = probs(pr, form)
            out = fused(entry, pr, form, 8)
            V = pr["qkv"][2, 0].astype(np.int64)
            for h in range(pr["H"]):
                assert np.array_equal(rq(P[h].astype(np.int64) @ V[h], pr["mo"], pr["eo"]), out[h, :16]), (s, form, h)
            seen_c += int((pr["cls"] == smo.CLASS_C).sum())
    assert seen_c >= (4 if T >= 144 else 0)


def literal(x, s, bits):
    rows, L = x.shape
    o = fenced.output(rows, L, L + 5, np.int8 if bits == 8 else np.int16, sentinel=-86 if bits == 8 else -21846)
    xp = _lib.ptr(dev(x))
    if bits == 8:
        _lib.call("ivit_shiftmax_f32_i8", xp, L, rows, L, float(s), o.ptr, o.ld, st())
    else:
        _lib.call("ivit_shiftmax_f32_i16", xp, L, rows, L, float(s), bits, o.ptr, o.ld, st())
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("T", SHORT_T + LONG_T[1:])
def test_stand_alone_forms(T):
    """rows go in directly: the integer forms at the power-of-two scales, the literal forms (float view q * s) at every scale"""
    K = kat(T)
    wrong, ran = [], 0
    for s in scales(T):
        for bits in (8, 16):
            m = pick(T, s, bits)
            if not len(m):
                continue
            q, ref, cls = K["q"][m], K["ref"][m], K["cls"][m]
            runs = []
            x = (q.astype(np.float32) * np.float32(s)).astype(np.float32)
            runs.append(("ivit_shiftmax_f32_i8" if bits == 8 else "ivit_shiftmax_f32_i16", literal(x, s, bits)))
            if bits == 8 and not natural(s):
                for name, dt in (("ivit_shiftmax_i8", np.int8), ("ivit_shiftmax_i32_i8", np.int32)):
                    o = fenced.output(len(m), T, T + 5, np.int8, expected=ref)
                    _lib.call(name, _lib.ptr(dev(q.astype(dt))), T, len(m), T, float(s), o.ptr, o.ld, st())
                    torch.cuda.synchronize()
                    runs.append((name, o))
            for name, o in runs:
                got = o.rows2d(o.fetch())[:, :T].astype(np.int32)
                bad = np.any(got != ref, axis=1)
                ran += 1
                if bad.any():
                    per = {smo.CLASS_NAMES[c]: f"{int((bad & (cls == c)).sum())} of {int((cls == c).sum())}" for c in (0, 1, 2)}
                    exact = int(np.all(got[bad] == K["exact"][m][bad], axis=1).sum())
                    wrong.append(f"{name} s={s} bits={bits}: rows wrong per class {per}, {exact} of them the exact-sum candidate")
                else:
                    fenced.check(o, ref)
    assert ran
    assert not wrong, f"T={T}: " + " | ".join(wrong)


@pytest.mark.parametrize("T", SHORT_T + LONG_T[1:])
def test_literal_form_equals_probs_entry_at_natural_scales(T):
    """module path (ivit_shiftmax_f32_i8 on q * s) and fused path (the probs entry) on the same row"""
    ran = 0
    for s in scales(T):
        pr = problem(T, s, 8) if natural(s) else None
        if pr is None:
            continue
        q = kat(T)["q"][pr["rows"]]
        o = literal((q.astype(np.float32) * np.float32(s)).astype(np.float32), s, 8)
        lit = o.rows2d(o.fetch())[:, :T].astype(np.int32)
        for form in forms(s):
            _, _, P = probs(pr, form, q_rows=1)
            assert np.array_equal(P[:, 0], lit), (s, form, np.flatnonzero(np.any(P[:, 0] != lit, axis=1)).tolist())
            ran += 1
    assert ran


# ------------------------------------------------------------------------------------------------ Swin window attention
def window_problem(T, s):
    """problem() at head_dim 32 for one window: zero bias_add, identity (m_b, e_b), no mask"""
    pr = problem(T, s, 8, hd=32)
    if pr is None:
        return None
    kp = 64 if T <= 64 else (T + 15) // 16 * 16
    mb = dyadic(np.float32(s), np.float32(s))
    pr = dict(pr, bias=np.zeros((pr["H"], T, kp), np.int16), mb=(int(mb[0][0]), int(mb[1][0])))
    ph = phi_table(np.float32(s))
    pr["phi"] = ph
    pr["phim"] = ((((np.arange(-128, 128, dtype=np.float32) * pr["s"]).astype(np.float32) + np.float32(-100.0)).astype(np.float32)) / pr["s"]).astype(np.float32)
    return pr


def window(entry, pr, form):
    """-> output [H, T, 32] of one window-attention entry"""
    qkv, H, T = pr["qkv"][:, 0][:, None], pr["H"], pr["qkv"].shape[3]       # [3, 1 window, H, T, 32]
    hd, ws = 32, int(round(np.sqrt(T)))
    exp = pr["exp"].transpose(1, 0, 2).reshape(T, H * hd)
    o = fenced.output(T, H * hd, H * hd + 32, np.int8, expected=exp)
    head = (_lib.ptr(dev(qkv)), o.ptr, o.ld, _lib.ptr(dev(pr["bias"])), None)
    geo = (1, 1, H, T, hd, int(pr["ms"][0]), int(pr["es"][0]), pr["mb"][0], pr["mb"][1], float(pr["s"]), int(pr["mo"][0]), int(pr["eo"][0]))
    phi = (_lib.ptr(dev(pr["phi"])), _lib.ptr(dev(pr["phim"]))) if form == "literal" else (None, None)
    band = (None, 0, 0)
    if form == "band":
        bt, bw = window_shiftexp_band(pr["s"], False)
        assert bt is not None
        band = (_lib.ptr(dev(bt)), bw, bt.shape[0])
    if entry == "ivit_window_attention_i8":
        _lib.call(entry, *head, 0, *geo, st())
    elif entry == "ivit_window_attention_i8_compat":
        _lib.call(entry, *head, -1, *geo, *phi, st())
    elif entry == "ivit_window_attention_i8_band":
        _lib.call(entry, *head, *geo, *band, 0, 0, 0, 0, st())
    elif entry == "ivit_window_attention_i8_unwindow":      # one window per image, no shift: image order is window order
        _lib.call(entry, *head, 0 if form == "pow2" else -1, *geo, *phi, ws, ws, ws, 0, st())
    else:
        _lib.call(entry, *head, 0 if form == "pow2" else -1, *geo, *phi, *band, ws, ws, ws, 0, 0, st())
    torch.cuda.synchronize()
    got = o.rows2d(o.fetch())[:, :H * hd].astype(np.int32).reshape(T, H, hd).transpose(1, 0, 2)
    v = verdict(pr, got[:, 0], got[:, 1:], pr["exp"][:, 1:])
    if not v:
        fenced.check(o, exp)
    return v


WINDOW = {49: (("ivit_window_attention_i8", ("pow2",)), ("ivit_window_attention_i8_compat", ("literal",)),
               ("ivit_window_attention_i8_band", ("band",)), ("ivit_window_attention_i8_unwindow", ("pow2", "literal"))),
          144: (("ivit_window_attention_i8_long", ("pow2", "literal", "band")),)}


@pytest.mark.parametrize("T,entry,fms", [(T, e, f) for T, ef in WINDOW.items() for e, f in ef])
def test_window_entries(T, entry, fms):
    wrong, ran = [], 0
    for s in scales(T):
        pr = window_problem(T, s)
        if pr is None:
            continue
        for form in fms:
            if (form == "pow2") == natural(s):
                continue
            v = window(entry, pr, form)
            ran += 1
            if v:
                wrong.append(f"s={s} {form}: {v}")
    assert ran, "no fixture row for this entry"
    assert not wrong, f"{entry} T={T}: " + " | ".join(wrong)
