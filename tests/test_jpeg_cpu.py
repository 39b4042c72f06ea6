"""CPU: the JPEG decoder's host side (i-vit_amd/csrc/jpeg.hip): ivit_jpeg_decode_host against Pillow's
Image.open(f).convert("RGB") on the fixture and on a few hundred seeded random files; the probe's verdicts and reasons (libjpeg-turbo's
colour-space guess included); corrupt and truncated streams; ImageFolderJPEG's indexing; the fixture against the installed Pillow;
the C prototypes against the ctypes table."""
import hashlib
import io
import os
import re

import numpy as np
import pytest

from ivit_amd import _lib
from ivit_amd.transforms import ImageFolderJPEG, ImageFolderU8, decode_jpeg_host, encode_images, probe_jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg_decode_pil.npz")


def _fixture():
    z = np.load(GOLDEN)
    cases = []
    for i, name in enumerate(z["names"]):
        data = z["data"][z["data_off"][i]:z["data_off"][i + 1]].tobytes()
        h, w = (int(v) for v in z["sizes"][i])
        p0, p1 = z["pix_off"][i], z["pix_off"][i + 1]
        px = z["pixels"][p0:p1].reshape(h, w, 3) if p1 > p0 else None
        cases.append(dict(name=str(name), data=data, h=h, w=w, supported=bool(z["supported"][i]), reason=str(z["reasons"][i]),
                          sha=z["sha256"][i].tobytes(), pixels=px))
    return cases


CASES = _fixture()


def _pil(data):
    Image = pytest.importorskip("PIL.Image")
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def test_fixture_reproduces_with_installed_pillow():
    for c in CASES:
        px = _pil(c["data"])
        assert px.shape == (c["h"], c["w"], 3), c["name"]
        assert hashlib.sha256(px.tobytes()).digest() == c["sha"], c["name"]
        if c["pixels"] is not None:
            assert np.array_equal(px, c["pixels"]), c["name"]


def test_fixture_covers_the_contract():
    names = {c["name"]: c for c in CASES}
    assert b"\xff\xc1" in names["37x53_420_qt16"]["data"]                        # 16-bit tables: an SOF1 frame
    assert b"\xff\xdd" in names["37x53_420_rst1"]["data"]                        # DRI
    big = names["1200x1600_420_q90"]["data"]
    assert 300_000 <= len(big) <= 600_000 and len(big) * 8 // 4096 > 500          # many hundreds of subsequences
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_host_decoder_equals_fixture():
    for c in CASES:
        ok, reason, info = probe_jpeg(c["data"])
        assert ok == c["supported"], (c["name"], reason)
        if not ok:
            assert c["reason"] in reason, (c["name"], reason)
            continue
        assert info[:2] == (c["h"], c["w"])
        px = decode_jpeg_host(c["data"])
        assert hashlib.sha256(px.tobytes()).digest() == c["sha"], c["name"]
        if c["pixels"] is not None:
            assert np.array_equal(px, c["pixels"]), c["name"]


def _random_jpeg(rng, Image):
    h, w = int(rng.integers(1, 90)), int(rng.integers(1, 90))
    if rng.random() < 0.1:
        h, w = int(rng.integers(100, 400)), int(rng.integers(100, 400))
    lo = rng.integers(0, 256, (max(h // 8, 2), max(w // 8, 2), 3), dtype=np.uint8)
    img = np.asarray(Image.fromarray(lo).resize((w, h), Image.BICUBIC)).astype(np.float32)
    img = np.clip(img + rng.normal(0, float(rng.choice([2, 10, 30])), img.shape), 0, 255).astype(np.uint8)
    gray = rng.random() < 0.2
    im = Image.fromarray(img[..., 0] if gray else img)
    kw = dict(quality=int(rng.choice([1, 5, 25, 50, 75, 90, 95, 100])), optimize=bool(rng.integers(0, 2)))
    if not gray:
        kw["subsampling"] = int(rng.integers(0, 3))
    r = int(rng.integers(0, 4))
    if r == 1:
        kw["restart_marker_blocks"] = int(rng.choice([1, 2, 3, 7]))
    elif r == 2:
        kw["restart_marker_rows"] = int(rng.choice([1, 2]))
    bio = io.BytesIO()
    try:
        im.save(bio, "JPEG", **kw)
    except OSError:     # libjpeg refuses some restart settings on tiny images
        return None, kw
    return bio.getvalue(), kw


def test_host_decoder_equals_pillow_on_random_files():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    n = 0
    while n < 300:
        data, kw = _random_jpeg(rng, Image)
        if data is None:
            continue
        n += 1
        ok, reason, _ = probe_jpeg(data)
        assert ok, (kw, reason)
        assert np.array_equal(decode_jpeg_host(data), _pil(data)), kw


def _segments(data):
    """(marker, start, end) of every marker segment before SOS"""
    out, p = [], 2
    while data[p + 1] != 0xDA:
        n = int.from_bytes(data[p + 2:p + 4], "big")
        out.append((data[p + 1], p, p + 2 + n))
        p += 2 + n
    return out


def _with_ids(data, ids, drop_app0=True, app14=None):
    """the file with its APP0 dropped, an Adobe APP14 inserted and the frame's / scan's component ids replaced"""
    b = bytearray(data)
    for m, s, e in _segments(bytes(b)):
        if m in (0xC0, 0xC1):
            for k in range(3):
                b[s + 4 + 6 + 3 * k] = ids[k]
    sos = bytes(b).index(b"\xff\xda")
    for k in range(3):
        b[sos + 5 + 2 * k] = ids[k]
    if drop_app0:
        for m, s, e in _segments(bytes(b)):
            if m == 0xE0:
                b = b[:s] + b[e:]
                break
    if app14 is not None:
        seg = b"\xff\xee" + (14).to_bytes(2, "big") + b"Adobe" + bytes([0, 100, 0, 0, 0, 0, app14])
        b = b[:2] + seg + b[2:]
    return bytes(b)


def test_probe_colour_space_guess():
    c = next(c for c in CASES if c["name"] == "37x53_444_q5")
    data = c["data"]
    assert probe_jpeg(data)[0]
    ok, reason, _ = probe_jpeg(_with_ids(data, (82, 71, 66)))               # no JFIF, ids 'R' 'G' 'B': RGB
    assert not ok and "R, G, B" in reason
    ok, reason, _ = probe_jpeg(_with_ids(data, (1, 2, 3), app14=0))         # Adobe transform 0: RGB
    assert not ok and "Adobe" in reason
    assert probe_jpeg(_with_ids(data, (1, 2, 3), app14=1))[0]               # Adobe transform 1: YCbCr
    assert probe_jpeg(_with_ids(data, (82, 71, 66), drop_app0=False))[0]    # JFIF wins over the ids
    assert probe_jpeg(_with_ids(data, (7, 8, 9)))[0]                        # unknown ids: YCbCr
    for variant in (_with_ids(data, (1, 2, 3), app14=1), _with_ids(data, (82, 71, 66), drop_app0=False), _with_ids(data, (7, 8, 9))):
        assert np.array_equal(decode_jpeg_host(variant), _pil(variant))


def test_probe_rejects_other_files_with_a_reason():
    c = next(c for c in CASES if c["name"] == "37x53_420_rst1")["data"]
    cases = {
        "truncated": c[:len(c) // 2],
        "no SOI": b"GIF89a" + bytes(40),
        "empty": b"",
        "12-bit": c.replace(b"\xff\xc0\x00\x11\x08", b"\xff\xc0\x00\x11\x0c", 1),
        "restart markers out of sequence": c.replace(b"\xff\xd1", b"\xff\xd2", 1),
    }
    for what, data in cases.items():
        ok, reason, _ = probe_jpeg(data)
        assert not ok and reason, what
        with pytest.raises(_lib.IvitError):
            decode_jpeg_host(data)
    assert "12-bit" in probe_jpeg(cases["12-bit"])[1]
    assert "out of sequence" in probe_jpeg(cases["restart markers out of sequence"])[1]


def test_corrupt_entropy_data_is_an_error_and_stays_in_bounds():
    rng = np.random.default_rng(3)
    c = next(c for c in CASES if c["name"] == "37x53_420_q100_opt")["data"]
    sos = c.index(b"\xff\xda")
    start = sos + 2 + int.from_bytes(c[sos + 2:sos + 4], "big")
    errors = 0
    for it in range(200):
        b = bytearray(c)
        if it % 2:
            for _ in range(8):   # random bytes (no 0xFF: the marker structure stays)
                b[int(rng.integers(start, len(c) - 2))] = int(rng.integers(0, 255))
        else:                    # the scan cut short, EOI kept
            cut = int(rng.integers(start + 1, len(c) - 2))
            b = b[:cut] + b"\xff\xd9"
        data = bytes(b)
        if not probe_jpeg(data)[0]:
            continue
        try:
            px = decode_jpeg_host(data)
            assert px.shape == (37, 53, 3)
        except _lib.IvitError as e:
            assert "corrupt" in str(e)
            errors += 1
    assert errors > 20


def test_encode_images_without_a_gpu():
    data = [c["data"] for c in CASES]
    enc = encode_images(data, pin=False)
    assert len(enc) == len(CASES) and enc.size(0) == len(CASES)
    for b, c in enumerate(CASES):
        assert tuple(enc.sizes[b]) == (c["h"], c["w"])
        assert (enc.sec_offsets[b] >= 0) == c["supported"]
        assert (b in enc.fallback) == (not c["supported"])
        if not c["supported"]:
            assert c["reason"] in enc.reasons[b]
            assert np.array_equal(enc.fallback[b], c["pixels"])
    g = enc.geometry(256, 224)
    assert g.shape == (len(CASES), 6) and tuple(g[0, :2]) == (1, 1)


def test_image_folder_jpeg_indexing(tmp_path):
    for k, c in enumerate(CASES[:9]):
        d = tmp_path / f"class{k % 3}"
        d.mkdir(exist_ok=True)
        (d / f"img{k}.{'png' if 'png' in c['name'] else 'jpg'}").write_bytes(c["data"])
    (tmp_path / "class0" / "notes.txt").write_text("not an image")
    a, b = ImageFolderJPEG(str(tmp_path)), ImageFolderU8(str(tmp_path))
    assert a.samples == b.samples and a.targets == b.targets and a.classes == b.classes
    data, target = a[0]
    assert isinstance(data, bytes) and data == open(a.samples[0][0], "rb").read() and target == a.targets[0]
    enc, t = ImageFolderJPEG.collate([a[i] for i in range(len(a))], pin=False)
    assert len(enc) == len(a) and t.tolist() == a.targets


def _prototypes():
    text = open(os.path.join(ROOT, "include", "ivit_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(ivit_jpeg_\w+)\s*\(([^)]*)\)\s*;", text):
        args = [a.strip() for a in m.group(2).split(",")]
        out[m.group(1)] = args
    return out


def test_jpeg_prototypes_match_ctypes_table():
    protos = _prototypes()
    assert set(protos) == {k for k in _lib.SIGNATURES if k.startswith("ivit_jpeg_")}
    import ctypes as C
    kind = {"int": C.c_int, "int64_t": C.c_int64}
    for name, args in protos.items():
        want = [C.c_void_p if "*" in a or a.startswith("ivit_stream_t") else kind[a.rsplit(" ", 1)[0]] for a in args]
        assert _lib.SIGNATURES[name] == want, name
