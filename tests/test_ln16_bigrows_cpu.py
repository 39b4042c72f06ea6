"""16-bit I-LayerNorm rows whose float32 sum reaches 2^24, whose int32 squares wrap, or whose variance lies at the edge of the Newton
shortcut (tests/golden/ln16_bigrows_kat.npz: the reference module's own outputs on crafted rows, oracle/gen_golden.py
gen_ln16_bigrows), on the host: the fixture holds what it must hold, the numpy restatement of tests/ln16_order_ref.py reproduces the
reference's bytes with torch's order and the wrapped square and tells the other candidates apart on exactly the rows of classes (c)
and (w), and the CPU oracles give the reference's bytes.  No GPU; the reference tree is not read."""
import importlib.util
import json
import os
import zlib

import numpy as np
import pytest

from oracle import oracle as orc
import ln16_order_ref as lno

WIDTHS = lno.TILED_C + lno.OTHER_C
GROUPS = [(C, si) for C in WIDTHS for si in (0, 1)]


@pytest.fixture(scope="module")
def kat(golden_dir):
    return np.load(os.path.join(golden_dir, "ln16_bigrows_kat.npz"))


def group(kat, C, si):
    """-> dict(q int16 [n, C], s, gamma, beta, hi, ref int8 [n, C], cls, vkind, edge, exact_crc, nowrap_crc)"""
    key = f"{C}_{si}"
    return dict(q=kat[f"q_{key}"], s=np.float32(kat["scales"][si]), gamma=kat[f"gamma_{C}"], beta=kat[f"beta_{C}"],
                hi=float(kat["ranges"][si]), ref=kat[f"ref_{key}"], cls=kat[f"cls_{key}"].astype(np.int64), vkind=kat[f"vkind_{key}"],
                edge=kat[f"edge_{key}"], exact_crc=kat[f"exact_crc_{key}"], nowrap_crc=kat[f"nowrap_crc_{key}"])


def crcs(a):
    return np.array([zlib.crc32(r.tobytes()) for r in np.ascontiguousarray(a, np.int8)], np.uint32)


def test_fixture_holds_the_required_rows(kat, golden_dir):
    from ivit_amd.prepare import markstein_division_ok
    assert os.path.getsize(os.path.join(golden_dir, "ln16_bigrows_kat.npz")) < 640 * 1024
    assert tuple(kat["widths"]) == WIDTHS and tuple(kat["scales"]) == lno.SCALES
    assert lno.S_POW2 == np.float32(2.0 ** -10) and markstein_division_ok(lno.S_NATURAL, 16)
    meta = json.loads(str(kat["meta"]))
    assert meta["classes"] == {"a": 0, "b": 1, "c": 2, "w": 3, "v": 4} and meta["torch"]
    total = 0
    for C, si in GROUPS:
        g = group(kat, C, si)
        q, cls = g["q"], g["cls"]
        assert q.dtype == np.int16 and q.shape[1] == C and g["ref"].dtype == np.int8 and g["ref"].shape == q.shape
        assert (cls == lno.CLASS_C).sum() == (8 if C in lno.TILED_C else 4) and (cls == lno.CLASS_W).sum() == 8      # what the generator writes
        assert (cls == lno.CLASS_A).sum() >= 1 and (cls == lno.CLASS_B).sum() >= 2 and g["edge"].sum() == 1
        sums = q.astype(np.int64).sum(axis=1)[cls == lno.CLASS_C]
        assert (sums > 0).any() and (sums < 0).any()                         # both signs
        # class (v): both sides of the band in every binade that +- pairs of 16-bit values reach at this width, and the 2^37 boundary
        var = lno.layernorm(q, g["s"], g["gamma"], g["beta"])["var"]
        assert (var > 0).all()
        v = cls == lno.CLASS_V
        ex = np.floor(np.log2(var.astype(np.float32).astype(np.float64))).astype(int)
        # (C = 772 / 2048: the kernels that take them have no shortcut; four binades, lno.V_BINADES_OTHER_C)
        for b in (range(24, 42) if C in lno.TILED_C else lno.V_BINADES_OTHER_C):
            if 2.0 ** b * 1.05 < C * 32767.0 ** 2 * 0.93:
                for kind in (lno.V_INSIDE, lno.V_OUTSIDE):
                    assert (v & (ex == b) & (g["vkind"] == kind)).any(), (C, si, b, kind)
            else:
                assert f"{C}_{si}_v{b}" in meta["notes"]
        vb = var[v & (g["vkind"] == lno.V_BOUNDARY)].astype(np.float32)
        assert np.float32(2.0 ** 37) in vb and np.nextafter(np.float32(2.0 ** 37), np.float32(0)) in vb
        total += len(q)
    assert 300 <= total <= 600


@pytest.mark.parametrize("C,si", GROUPS)
def test_restatement_reproduces_reference_and_classes(kat, C, si):
    g = group(kat, C, si)
    q, cls, ref = g["q"], g["cls"], g["ref"]
    got_cls, cand, r = lno.classify(q, g["s"], g["gamma"], g["beta"], -g["hi"], g["hi"])
    # torch's order + the wrapped square is the reference, on every row
    assert np.array_equal(cand[("torch", True)], ref), (C, si, "torch's order with int32 squares is not the reference's output")
    assert np.array_equal(got_cls, np.where(cls == lno.CLASS_V, lno.CLASS_A, cls))
    # the other candidates are the stored ones, and differ on exactly the rows of their class
    assert np.array_equal(crcs(cand[("exact", True)]), g["exact_crc"]) and np.array_equal(crcs(cand[("torch", False)]), g["nowrap_crc"])
    d_exact = np.any(cand[("exact", True)] != ref, axis=1)
    d_nowrap = np.any(cand[("torch", False)] != ref, axis=1)
    assert np.array_equal(d_exact, cls == lno.CLASS_C), (C, si)
    assert np.array_equal(d_nowrap, cls == lno.CLASS_W), (C, si)
    assert np.array_equal(np.any(cand[("exact", False)] != ref, axis=1), np.isin(cls, (lno.CLASS_C, lno.CLASS_W)))
    # what the classes say
    xf = lno.xint_of(q, g["s"])
    St, Se = lno.both_sums(xf)
    big = np.abs(xf.astype(np.float64).sum(axis=1)) >= 2.0 ** 24
    assert np.array_equal(St, np.array([orc.torch_rowsum(x) for x in xf], np.float32))      # the oracle's restatement of torch's kernel
    assert np.array_equal(big, np.isin(cls, (lno.CLASS_B, lno.CLASS_C)) | (big & (cls == lno.CLASS_W)))
    same_mean = lno.mean_int_of(St, C) == lno.mean_int_of(Se, C)
    assert np.array_equal(~same_mean, cls == lno.CLASS_C)
    assert np.array_equal(r["maxd"] >= lno.WRAP_FROM, cls == lno.CLASS_W)
    w = cls == lno.CLASS_W
    assert (r["maxd"][w] == lno.WRAP_FROM).any() and (r["maxd"][g["edge"] == 1] == lno.WRAP_FROM - 1).all()
    assert (r["var"] > 0).all() and (lno.layernorm(q, g["s"], g["gamma"], g["beta"], wrap=False)["var"][w] > r["var"][w]).all()
    # class (v): the rule of swin.hip's ln16_std10 says what the fixture says, and shortcut == literal steps on these rows
    v = cls == lno.CLASS_V
    varf = r["var"][v].astype(np.float32)
    slow, s = lno.std10_rule(varf)
    vk = g["vkind"][v]
    assert np.array_equal(slow[vk != lno.V_BOUNDARY], vk[vk != lno.V_BOUNDARY] == lno.V_INSIDE)
    assert np.array_equal(s[~slow], lno.newton10(varf)[~slow])


def quantised(y, s_ln, hi):
    return lno.quantact8(y, s_ln, -hi, hi)


@pytest.mark.parametrize("C,si", GROUPS)
def test_oracles_give_the_reference_bytes(kat, C, si):
    """oracle.layernorm (integers: the power-of-two scale) and oracle.layernorm_scaled (any scale) + the QuantAct against the reference's
    bytes.  oracle.layernorm_compat takes 8-bit rows only: see test_eight_bit_rows_reach_neither_case."""
    g = group(kat, C, si)
    q = g["q"].astype(np.int32)
    bad = {}
    y, s_ln, _ = orc.layernorm_scaled(q, g["s"], g["gamma"], g["beta"])
    bad["layernorm_scaled"] = np.any(quantised(y, s_ln, g["hi"]) != g["ref"], axis=1)
    if si == 0:
        y, s_ln, _ = orc.layernorm(q, g["gamma"], g["beta"])
        bad["layernorm"] = np.any(quantised(y, s_ln, g["hi"]) != g["ref"], axis=1)
    for name, b in bad.items():
        per_class = {lno.CLASS_NAMES[c]: f"{int(b[g['cls'] == c].sum())}/{int((g['cls'] == c).sum())}" for c in lno.CLASS_NAMES}
        print(f"oracle.{name} C={C} s={float(g['s']):.6g}: rows that differ from the reference, per class: {per_class}")
    for name, b in bad.items():
        assert not b.any(), (name, C, si, f"{int(b.sum())} rows differ, classes {sorted(set(g['cls'][b].tolist()))}")


def test_eight_bit_rows_reach_neither_case():
    """oracle.layernorm_compat (8-bit rows through the 256-entry phi table) cannot be fed the fixture, and needs neither step: |sum| <=
    C * 128 stays below 2^24 for every C the entries take (C <= 4096), |x - mean| <= 255.  It shares the C code of the other two; on
    8-bit rows the three agree."""
    assert 4096 * 128 < 1 << 24 and 255 < lno.WRAP_FROM
    rng = np.random.default_rng(3)
    q = rng.integers(-128, 128, size=(16, 768)).astype(np.int32)
    q[0], q[1] = 127, -128
    q[1, 5] = 127
    gamma, beta = rng.uniform(0.5, 1.5, size=768).astype(np.float32), rng.normal(0, 0.1, size=768).astype(np.float32)
    for s in lno.SCALES:
        a = orc.layernorm_compat(q, s, gamma, beta)[0]
        assert np.array_equal(a, orc.layernorm_scaled(q, s, gamma, beta)[0])
        assert np.array_equal(a[2:], lno.layernorm(q, s, gamma, beta)["y"][2:])           # (rows 0, 1: var = 0 and a lone element)


def test_oracle_swin_counter_counts_rows_at_2_24_and_more(kat):
    """OracleSwin.ln_big_sum_rows: the rows whose integer sum is 2^24 or more in magnitude -- classes (b), (c) and the (w) rows that
    reach it -- and its LayerNorm + QuantAct gives the reference's bytes on them"""
    C, si = 768, 0
    g = group(kat, C, si)
    om = orc.OracleSwin({"n.weight": g["gamma"], "n.bias": g["beta"]}, {})
    s_out = orc.sym_scale(-g["hi"], g["hi"], 8)
    got = om._ln_q(g["q"].astype(np.int32), "n", s_out)
    big = np.abs(g["q"].astype(np.int64).sum(axis=1)) >= 1 << 24
    assert om.ln_big_sum_rows == int(big.sum()) >= int(np.isin(g["cls"], (lno.CLASS_B, lno.CLASS_C)).sum()) >= 10
    assert np.array_equal(got, g["ref"])
    om._ln_q(g["q"][~big].astype(np.int32), "n", s_out)
    assert om.ln_big_sum_rows == int(big.sum())


BINADES = range(24, 42)


def test_std10_rule_against_the_literal_steps():
    """the rule of swin.hip's ln16_std10 (restated in ln16_order_ref.std10_rule) against the ten literal float32 steps: wherever the
    rule takes the shortcut, floor(sqrt(varf)) is what the steps give -- on the eight float32 below EVERY square of binades 24..41
    (2^(ex - 20) = 8 ulp; no square is sampled: 2.1 million roots), and on 200 000 seeded values per binade of the rest.  Binade 41
    covers the largest variance of a row without a wrapped square."""
    assert 1536 * 46340 ** 2 < 2 ** 42 and 2048 * 32768 ** 2 <= 2 ** 41
    rng = np.random.default_rng(41)
    below = 0
    for ex in BINADES:
        ulp = 2.0 ** (ex - 23)
        lo, hi = int(np.ceil(np.sqrt(2.0 ** ex))), int(np.sqrt(2.0 ** (ex + 1)))
        roots = np.arange(lo, hi + 1, dtype=np.float64)                        # every square of the binade (614 000 roots at 2^41)
        sq = roots * roots                                                    # exact: below 2^42
        top = sq.astype(np.float32)
        top = np.where(top.astype(np.float64) >= sq, np.nextafter(top, np.float32(0)), top)      # the largest float32 below the square
        k = np.arange(8, dtype=np.float64)                                    # 2^(ex - 20) = 8 ulp
        varf = (top.astype(np.float64)[:, None] - k[None, :] * ulp).astype(np.float32).reshape(-1)
        varf = varf[(varf >= np.float32(2.0 ** ex)) & (varf < np.float32(2.0 ** (ex + 1)))]
        assert np.array_equal(varf.astype(np.float64), np.rint(varf.astype(np.float64)))
        slow, s = lno.std10_rule(varf)
        t = lno.newton10(varf)
        assert np.array_equal(s[~slow], t[~slow]), (ex, "a shortcut value is not the ten steps' value")
        assert slow.any() and np.all((t[slow] == s[slow]) | (t[slow] == s[slow] + 1))
        below += len(roots)
        rest = (2.0 ** ex * (1.0 + rng.random(200000))).astype(np.float32)
        rest = np.floor(rest)
        slow, s = lno.std10_rule(rest)
        assert np.array_equal(s[~slow], lno.newton10(rest)[~slow]), ex
        # the band is varf * 2^-22 of the 2 sqrt(varf) between two squares: sqrt(varf) * 2^-23 of all values (a quarter at 2^42)
        assert slow.mean() < 2.0 ** ((ex + 1) / 2 - 23) * 1.1 + 0.001
    assert below >= 2 ** 21 - 2 ** 12 + 1      # every root 2^12 .. 2^21 (a root on a binade's edge counts in both)


def test_probe_walks_every_binade_the_kernel_reaches():
    """scripts/probes/ln16_newton_exhaustive.py names the binades it walks; the rule it checks is the one restated here"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "probes", "ln16_newton_exhaustive.py")
    spec = importlib.util.spec_from_file_location("ln16_newton_exhaustive", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert tuple(mod.BINADES) == tuple(BINADES)
    assert 2.0 ** mod.BINADES[-1] * 2 > 1536 * 46340 ** 2
    # its assertion on all 2^23 values of the top binade; the neighbourhood of every square of the other binades is
    # test_std10_rule_against_the_literal_steps, all their values the script itself
    assert mod.walk(BINADES[-1]) > 0
