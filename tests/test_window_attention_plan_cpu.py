"""CPU: the host side of the eight Swin window-attention entries (csrc/win_attn_host.h: descriptor, check, softmax form; the launchers
of csrc/swin.hip and csrc/swin_probs.hip) through the lab build's dry run (include/ivit_hip_debug.h
ivit_debug_window_attention_dry_run): the entries check their arguments, choose form and kernel, record the plan and return in front
of the launch.  Every call here passes made-up aligned addresses, so none may reach a launch: the dry run stays on for the whole file,
and the file does not run where a GPU is present.

Three things are held:
  rejections  one valid argument set per entry, one condition violated at a time, and pairs of violations that fix the order of the
              checks: return code and message
  selection   a sweep of accepted argument sets that reaches every slot of window_attention_kernel's table and every SM of the
              probability kernel: the sixteen numbers of the plan
  mirror      swin_engine.window_attention_spec's Python copy of the saturation rule (common.h shiftmax_ksat) against the launcher,
              and the fused and the probability entry of one spec against each other

Expected values: tests/golden/window_attention_checks.json, recorded with IVIT_WRITE_WINDOW_PLAN=1 from the commit BEFORE the host
side was unified (its launchers patched to record the same sixteen numbers immediately in front of their launch sites), so the file
is the old launchers' behaviour, not this code's."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib, swin_engine  # noqa: E402

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="made-up addresses: never beside a GPU")

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "window_attention_checks.json")
RECORD = os.environ.get("IVIT_WRITE_WINDOW_PLAN") == "1"
P = "ivit_window_attention_"
HEAD = "qkv out ldo bias region"
DIMS = "windows wpi heads tokens head_dim m_s e_s m_b e_b"
GEOM = "H W ws shift"
PARAMS = {      # the prototypes of include/ivit_hip.h (out / ldo: probs / ldp of the probability entries)
    P + "i8": f"{HEAD} mask_value {DIMS} s_attn m_o e_o stream",
    P + "i8_compat": f"{HEAD} mask_value {DIMS} s_attn m_o e_o phi phim stream",
    P + "i8_band": f"{HEAD} {DIMS} s_attn m_o e_o band band_w band_rows {GEOM} stream",
    P + "i8_unwindow": f"{HEAD} mask_value {DIMS} s_attn m_o e_o phi phim {GEOM} stream",
    P + "i8_long": f"{HEAD} mask_value {DIMS} s_attn m_o e_o phi phim band band_w band_rows {GEOM} image_order stream",
    P + "i8_ibert": f"{HEAD} masked_exp {DIMS} m_o e_o table band_w {GEOM} image_order stream",
    P + "probs_u8": f"{HEAD} mask_value {DIMS} s_attn phi phim band band_w band_rows stream",
    P + "probs_u8_ibert": f"{HEAD} masked_exp {DIMS} table band_w stream",
}
PARAMS = {k: v.split() for k, v in PARAMS.items()}
ENTRIES = list(PARAMS)
QKV, OUT, BIAS, REGION, PHI, PHIM, BAND, TABLE = (0x10000 * k for k in range(1, 9))      # made up, 64 KB apart, 16-byte aligned
PLAN_FIELDS = "sm rq32 long ord grid lds kp x0 ksat mask_value band_w tables omap_ws omap_inv dwords family".split()


def shape(tokens):
    """windows of `tokens` tokens on a map of 2 x 2 windows; no geometry (ws = 0) where tokens is no square"""
    ws = int(round(tokens ** 0.5))
    if ws * ws != tokens:
        ws = 0
    return dict(tokens=tokens, ws=ws, H=2 * ws, W=2 * ws, shift=ws // 2, wpi=4, windows=8)


def base(entry):
    """one valid argument set per entry: 49 tokens (144 for the long entry), a shift mask, x0 = -8"""
    a = dict(qkv=QKV, out=OUT, ldo=96, bias=BIAS, region=REGION, mask_value=-800, masked_exp=3.0, heads=3, head_dim=32, m_s=1, e_s=5,
             m_b=1, e_b=3, s_attn=0.125, m_o=3, e_o=9, phi=None, phim=None, band=None, band_w=0, band_rows=0, table=TABLE,
             image_order=0, stream=None, **shape(144 if entry == P + "i8_long" else 49))
    if entry == P + "i8_band":
        a.update(band=BAND, band_w=64, band_rows=256)
    if entry.startswith(P + "probs"):
        a["ldo"] = 52
    return a


def run(L, entry, args):
    """-> (rc, message, plan): the call under the dry run; plan None where it was refused"""
    rc = getattr(L, entry)(*[args[k] for k in PARAMS[entry]])
    if rc != 0:
        return rc, L.ivit_last_error_string().decode(), None
    out = (C.c_int32 * 16)()
    assert L.ivit_debug_window_attention_last_plan(out) == 0
    return 0, "", list(out)


@pytest.fixture(scope="module")
def lab():
    with _lib.lab_session() as L:
        L.ivit_debug_window_attention_dry_run(1)
        yield L


@pytest.fixture(scope="module")
def golden():
    if RECORD:
        store = json.load(open(FIXTURE)) if os.path.exists(FIXTURE) else {}
        yield store
        with open(FIXTURE, "w") as f:      # one case per line
            f.write("{\n" + ",\n".join(json.dumps(sec) + ": {\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(cases.items()))
                                       + "\n}" for sec, cases in sorted(store.items())) + "\n}\n")
    else:
        yield json.load(open(FIXTURE))


def hold(golden, section, got):
    """got: case id -> recorded value; equal to the fixture's section, case by case and as a set"""
    if RECORD:
        golden[section] = got
        return
    want = golden[section]
    assert sorted(want) == sorted(got), "the cases of the test and of the fixture differ"
    bad = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not bad, f"{len(bad)} of {len(got)} differ, e.g. {sorted(bad.items())[:3]}"


# ------------------------------------------------------------------------------------------ rejections
VIOLATIONS = {      # name -> overrides; applied to every entry that has all the arguments
    "null_qkv": dict(qkv=None), "null_out": dict(out=None), "null_bias": dict(bias=None), "null_table": dict(table=None),
    "null_band": dict(band=None), "no_region": dict(region=None),
    "qkv_8": dict(qkv=QKV + 8), "out_4": dict(out=OUT + 4), "out_1": dict(out=OUT + 1), "bias_4": dict(bias=BIAS + 4),
    "bias_8": dict(bias=BIAS + 8), "region_2": dict(region=REGION + 2), "table_8": dict(table=TABLE + 8), "table_2": dict(table=TABLE + 2),
    "phi_2": dict(phi=PHI + 2, phim=PHIM), "phim_2": dict(phi=PHI, phim=PHIM + 2), "band_8": dict(band=BAND + 8, band_w=64, band_rows=256),
    "ldo_100": dict(ldo=100), "ldo_88": dict(ldo=88), "ldo_48": dict(ldo=48), "ldo_53": dict(ldo=53),
    **{f"tokens_{t}": shape(t) for t in (1, 2, 64, 65, 144, 145)},
    "head_dim_64": dict(head_dim=64),
    "windows_0": dict(windows=0), "heads_0": dict(heads=0), "wpi_0": dict(wpi=0), "windows_6": dict(windows=6), "windows_big": dict(windows=1 << 30),
    "no_mask_windows_6": dict(windows=6, region=None),
    "H_15": dict(H=15), "W_0": dict(W=0), "ws_6": dict(ws=6), "ws_0": dict(ws=0), "ws_neg": dict(ws=-7), "wpi_3": dict(wpi=3),
    "shift_neg": dict(shift=-1), "shift_ws": dict(shift=7), "shift_12": dict(shift=12),
    "band_w_8": dict(band=BAND, band_w=8, band_rows=256), "band_w_200": dict(band=BAND, band_w=200, band_rows=256),
    "band_w_24": dict(band=BAND, band_w=24, band_rows=256), "band_w_192": dict(band=BAND, band_w=192, band_rows=256),
    "band_w_256": dict(band=BAND, band_w=256, band_rows=256), "band_w_272": dict(band=BAND, band_w=272, band_rows=256),
    "band_w_0": dict(band=BAND, band_w=0, band_rows=256), "band_w_without_band": dict(band=None, band_w=64, band_rows=256),
    **{f"width_{w}": dict(band_w=w) for w in (8, 24, 64, 200, 256, 272)},      # (the I-BERT entries take a width alone)
    "band_rows_2": dict(band=BAND, band_w=64, band_rows=2), "band_rows_1": dict(band=BAND, band_w=64, band_rows=1),
    "band_and_phi": dict(band=BAND, band_w=64, band_rows=256, phi=PHI, phim=PHIM),
    "phi_alone": dict(phi=PHI), "phim_alone": dict(phim=PHIM), "phi_pair": dict(phi=PHI, phim=PHIM),
    "mask_value_1": dict(mask_value=1), "mask_value_low": dict(mask_value=-32769), "mask_value_min": dict(mask_value=-32768),
    "scale_0": dict(s_attn=0.0), "scale_neg": dict(s_attn=-0.125), "x0_low": dict(s_attn=1.0 / 5000), "x0_4096": dict(s_attn=1.0 / 4096),
    "row_sum": dict(s_attn=1.0 / 3000), "scale_2": dict(s_attn=2.0),
    "Ms_bound": dict(m_s=2048, e_s=0), "Mb_bound": dict(m_b=1 << 20, e_b=0), "Mo_bound": dict(m_o=512, e_o=0),
    "Ms_below": dict(m_s=2047, e_s=0), "Mb_below": dict(m_b=(1 << 20) - 1, e_b=0), "Mo_below": dict(m_o=511, e_o=0),
    "masked_exp_neg": dict(masked_exp=-1.0), "masked_exp_high": dict(masked_exp=40000.0), "masked_exp_neg_no_mask": dict(masked_exp=-1.0, region=None),
    "image_order_2": dict(image_order=2), "image_order_1": dict(image_order=1), "image_order_1_no_geometry": dict(image_order=1, ws=0),
    "image_order_neg": dict(image_order=-1),
    "masked_scores": dict(s_attn=1.0 / 40), "masked_scores_no_mask": dict(s_attn=1.0 / 40, region=None),
    "masked_scores_phi": dict(s_attn=1.0 / 40, phi=PHI, phim=PHIM), "masked_scores_band": dict(s_attn=1.0 / 40, band=BAND, band_w=64, band_rows=1),
    "x0_24": dict(s_attn=1.0 / 24), "x0_25": dict(s_attn=1.0 / 25),
}
ORDER_PAIRS = [      # two violations at once: the message names the one the entry checks first
    ("null_qkv", "head_dim_64"), ("null_qkv", "windows_0"), ("windows_0", "tokens_65"), ("windows_0", "tokens_145"), ("tokens_145", "qkv_8"),
    ("head_dim_64", "ldo_100"), ("qkv_8", "bias_4"), ("bias_4", "mask_value_1"), ("region_2", "scale_0"), ("mask_value_1", "scale_0"),
    ("scale_0", "phi_alone"), ("phi_alone", "band_rows_2"), ("band_rows_2", "Ms_bound"), ("Ms_bound", "x0_low"), ("Mo_bound", "row_sum"),
    ("row_sum", "masked_scores"), ("H_15", "null_qkv"), ("H_15", "band_w_8"), ("shift_ws", "image_order_2"), ("band_w_8", "windows_0"),
    ("band_w_200", "image_order_2"), ("image_order_2", "null_bias"), ("masked_exp_neg", "null_out"), ("null_table", "tokens_145"),
    ("null_table", "null_qkv"), ("table_8", "image_order_2"), ("null_band", "H_15"), ("ldo_48", "qkv_8"), ("band_w_24", "phi_alone"),
    ("phi_2", "mask_value_1"), ("table_2", "band_w_272"), ("band_w_272", "masked_exp_neg"), ("windows_6", "ldo_48"), ("Mb_bound", "band_w_8"),
]


def rejection_cases():
    for entry in ENTRIES:
        have = set(PARAMS[entry])

        def over_of(name):      # a token count brings its geometry along for the entries that take one
            return {k: v for k, v in VIOLATIONS[name].items() if k in have or not name.startswith("tokens_")}

        yield f"{entry}/base", entry, {}
        for name in VIOLATIONS:
            if set(over_of(name)) <= have:
                yield f"{entry}/{name}", entry, over_of(name)
        for one, two in ORDER_PAIRS:
            over = {**over_of(one), **over_of(two)}
            if set(over) <= have:
                yield f"{entry}/{one}+{two}", entry, over


def test_rejections(lab, golden):
    """code and message of every rejection; an accepted set (the bases, the in-range ends) answers 0"""
    got = {}
    for cid, entry, over in rejection_cases():
        rc, msg, _ = run(lab, entry, {**base(entry), **over})
        assert rc in (0, -1, -2), (cid, rc, msg)
        got[cid] = [rc, msg]
    for entry in ENTRIES:
        assert got[f"{entry}/base"] == [0, ""], entry
        assert got[f"{entry}/null_qkv"][0] == -1 and got[f"{entry}/tokens_1"][0] != 0, entry
        # (the unwindow entry looks at its geometry first, and 145 tokens are no square)
        assert got[f"{entry}/tokens_145"][0] == (-1 if entry == P + "i8_unwindow" else -2), entry
    assert len(got) > 600 and sum(1 for rc, _ in got.values() if rc) > 400
    hold(golden, "rejections", got)


# ------------------------------------------------------------------------------------------ selection
FORMS = ("integer", "phi", "band256", "band1", "ibert_table", "ibert_band")
SCALES = {"x0_8": 0.125, "x0_10": 0.1, "x0_11": 1.0 / 11}
MULTS = {"pow2": dict(m_s=1, e_s=5, m_b=1, e_b=3), "ms3": dict(m_s=3, e_s=6, m_b=1, e_b=3), "mb3": dict(m_s=1, e_s=5, m_b=3, e_b=4)}


def fused_call(form, tokens, image_order):
    """the fused entry a caller takes for this form, as swin_engine.window_attention / window_attention_ibert choose, and its
    form arguments; None where there is none (image order needs the windows' geometry)"""
    g = shape(tokens)
    if image_order and not g["ws"]:
        return None
    table = {"phi": dict(phi=PHI, phim=PHIM), "band256": dict(band=BAND, band_w=64, band_rows=256),
             "band1": dict(band=BAND, band_w=48, band_rows=1), "ibert_band": dict(band_w=64)}.get(form, {})
    if form.startswith("ibert"):
        return P + "i8_ibert", {**g, **table, "image_order": image_order, **({} if image_order else dict(ws=0))}
    if tokens > 64:
        if not g["ws"]:
            return None
        return P + "i8_long", {**g, **table, "image_order": image_order}
    if form.startswith("band"):
        return P + "i8_band", {**g, **table, **({} if image_order else dict(ws=0))}
    return (P + "i8_unwindow" if image_order else P + "i8_compat"), {**g, **table}


def test_selection(lab, golden):
    """the plan of every accepted set of the sweep; the sweep reaches every kernel there is"""
    got, slots, probs_sm = {}, set(), set()
    for tokens in (2, 49, 64, 81, 144):
        for form in FORMS:
            for masked in (1, 0):
                for sname, s in SCALES.items():
                    for mname, mult in MULTS.items():
                        common = dict(s_attn=s, region=REGION if masked else None, ldo=96, **mult)
                        for image_order in (0, 1):
                            sel = fused_call(form, tokens, image_order)
                            if sel is None:
                                continue
                            entry, over = sel
                            cid = f"{entry}/{form}/t{tokens}/m{masked}/{sname}/{mname}/o{image_order}"
                            rc, msg, plan = run(lab, entry, {**base(entry), **common, **over})
                            assert rc == 0, (cid, rc, msg)
                            got[cid] = plan
                            slots.add(tuple(plan[:4]))
                        entry = P + ("probs_u8_ibert" if form.startswith("ibert") else "probs_u8")
                        over = fused_call(form, tokens, 0)[1] if shape(tokens)["ws"] or tokens <= 64 else None
                        if over is None or mname != "pow2":      # (the probability kernel has one score requantisation)
                            continue
                        for pname, pover in {"dw": dict(out=OUT, ldo=148), "odd_ptr": dict(out=OUT + 1, ldo=148), "odd_ld": dict(out=OUT, ldo=147)}.items():
                            cid = f"{entry}/{form}/t{tokens}/m{masked}/{sname}/{mname}/{pname}"
                            args = {**base(entry), **common, **{k: v for k, v in over.items() if k in PARAMS[entry]}, **pover}
                            rc, msg, plan = run(lab, entry, args)
                            assert rc == 0, (cid, rc, msg)
                            got[cid] = plan
                            probs_sm.add(plan[0])
                            assert plan[14] == (pname == "dw"), cid
    # the plain entry is the compat entry without tables
    for tokens in (2, 49, 64):
        rc, msg, plan = run(lab, P + "i8", {**base(P + "i8"), **shape(tokens)})
        assert rc == 0, msg
        got[f"{P}i8/t{tokens}"] = plan
    # every instantiation of window_attention_kernel<SM, RQ32, NKT, ORD>: the Shiftmax forms without the ordered-sum branch exist for
    # the short rows only, I-BERT has no such switch (ORD stays 1)
    want = {(sm, rq, lng, ord_) for sm in range(4) for rq in (0, 1) for lng in (0, 1) for ord_ in (0, 1) if ord_ or (sm != 3 and not lng)}
    assert len(want) == 22 and slots == want, sorted(want ^ slots)
    assert probs_sm == {0, 1, 2, 3}
    hold(golden, "selection", got)


def test_plan_numbers(lab):
    """a few plans by hand (independent of the fixture): Swin-T stage 0 at batch 128 and the 12 x 12 windows of 384 px"""
    a = {**base(P + "i8_compat"), "windows": 8192, "wpi": 64}
    plan = dict(zip(PLAN_FIELDS, run(lab, P + "i8_compat", a)[2]))
    assert plan == dict(sm=0, rq32=1, long=0, ord=0, grid=6144, lds=0, kp=64, x0=-8, ksat=84, mask_value=-800, band_w=0, tables=0,
                        omap_ws=0, omap_inv=0, dwords=0, family=0)
    a = {**base(P + "i8_long"), "band": BAND, "band_w": 48, "band_rows": 1, "image_order": 1, "windows": 4096, "wpi": 4, "heads": 4, "ldo": 128,
         "m_s": 3}
    plan = dict(zip(PLAN_FIELDS, run(lab, P + "i8_long", a)[2]))
    assert plan == dict(sm=0, rq32=0, long=1, ord=1, grid=4096, lds=0, kp=144, x0=-8, ksat=47, mask_value=-1024, band_w=48, tables=2,
                        omap_ws=12, omap_inv=65536 // 12 + 1, dwords=0, family=1)
    a = {**base(P + "i8_ibert"), **shape(144), "band_w": 64}
    plan = dict(zip(PLAN_FIELDS, run(lab, P + "i8_ibert", a)[2]))
    assert (plan["sm"], plan["long"], plan["ord"], plan["lds"], plan["tables"], plan["family"]) == (3, 1, 1, 4 * 16 * 145 * 4, 8, 2)


# ------------------------------------------------------------------------------------------ the Python mirror
class FakeTensor:
    """what _lib.ptr and the launch helpers of swin_engine read of a device tensor"""

    def __init__(self, addr, shape_):
        self.addr, self.shape = addr, tuple(shape_)

    def data_ptr(self):
        return self.addr

    def stride(self, i):
        return int(np.prod(self.shape[i + 1:])) if i != -1 else 1


def spec_for(s_A, N, masked):
    nW = 4
    region = swin_engine.shift_mask_regions(14, 14, 7, 3) if N == 49 else np.zeros((nW, N), np.int64) + (np.arange(N) % 3)[None]
    addr = iter(range(BIAS, BIAS + 0x100000, 0x10000))
    spec, form = swin_engine.window_attention_spec(lambda a: FakeTensor(next(addr), a.shape), np.zeros((3, N, N), np.int8), np.float32(0.01),
                                                   np.float32(0.002), np.float32(0.02), np.float32(s_A), np.float32(0.001),
                                                   np.float32(0.03), region if masked else None, N)
    return spec, form


MIRROR_SCALES = [1.0 / (k - 0.5) for k in range(1, 61)] + [2.0 ** -k for k in range(6)] + \
                [p / d for d in (64, 256, 512, 1024, 2048, 4096, 8192) for p in (5, 10, 20, 25, 40, 50, 80, 100, 125, 160, 200, 250, 320, 400)
                 if 1 <= d / p <= 60 and (100 * d) % p == 0]


def test_python_mirror_of_the_saturation_rule(lab):
    """window_attention_spec leaves the integer form of a masked window of at most 64 tokens exactly where the launcher refuses it
    with "cannot place masked scores": at 81 tokens the rule does not apply, so the form chosen there is what every other reason
    chooses.  The scales: x0 = -1 .. -60, the powers of two and the exact scales p / 2^k at which nothing else asks for the natural
    form (phi is the identity, -100 / s an integer), on both sides of x0 = -24 / -25."""
    x0s, refused_at, lone = set(), set(), 0
    for s in MIRROR_SCALES:
        s32 = np.float32(s)
        x0 = int(np.floor(np.float32(-1.0) / s32))
        short_form, other_form = spec_for(s32, 49, True)[1], spec_for(s32, 81, True)[1]
        args = {**base(P + "i8_compat"), "s_attn": float(s32), "mask_value": max(-32768, int(np.float32(-100.0) / s32))}
        rc, msg, plan = run(lab, P + "i8_compat", args)
        refused = rc != 0
        if refused:
            assert rc == -1 and "cannot place masked scores" in msg, (s, msg)
            refused_at.add(x0)
        else:
            assert plan[7] == x0
        assert (short_form is not None) == (other_form is not None or refused), (s, x0, short_form, other_form, refused)
        lone += other_form is None
        x0s.add(x0)
    assert x0s >= set(range(-60, 0)) and refused_at == {x for x in x0s if x <= -25}
    assert lone >= 12      # scales at which the rule alone decides, refused and accepted ones


@pytest.mark.parametrize("N", (49, 144))
def test_fused_and_probability_entries_choose_alike(lab, N):
    """for one spec, the entry swin_engine.window_attention calls and the one window_attention_probs calls report the same SM, x0,
    ksat, mask_value and tables"""
    ws = 7 if N == 49 else 12
    seen = set()
    for s in MIRROR_SCALES:
        for masked in (True, False):
            spec, form = spec_for(np.float32(s), N, masked)
            plans = []
            for fuse_proj in (False, True):
                swin_engine.window_attention(spec, FakeTensor(QKV, ()), FakeTensor(OUT, ()), 96, 8, 4, 3, N, 2 * ws, 2 * ws, ws, ws // 2,
                                             fuse_proj, None)
                out = (C.c_int32 * 16)()
                lab.ivit_debug_window_attention_last_plan(out)
                plans.append(list(out))
            swin_engine.window_attention_probs(spec, "ivit", FakeTensor(QKV, ()), FakeTensor(OUT, (8, 3, N, 148)), 8, 4, 3, N, None)
            out = (C.c_int32 * 16)()
            lab.ivit_debug_window_attention_last_plan(out)
            assert out[15] == 3 and [p[15] for p in plans] == [N > 64] * 2
            for p in plans:
                assert [p[i] for i in (0, 7, 8, 9, 11)] == [out[i] for i in (0, 7, 8, 9, 11)], (s, masked, form, p, list(out))
            seen.add((out[0], out[11]))
    # the integer form, the literal form and a band table (whichever of its two forms the scales of the sweep have)
    assert seen >= {(0, 0), (1, 4)} and seen & {(0, 2), (2, 1)}, seen
