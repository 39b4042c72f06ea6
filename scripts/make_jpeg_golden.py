"""Writes tests/golden/jpeg_decode_pil.npz: seeded synthetic images encoded by Pillow (sizes from 1x1 to 1600x1200; 4:4:4, 4:2:2,
4:2:0 and grayscale; qualities 1 to 100; 16-bit quantisation tables; optimised Huffman tables; restart intervals; COM / APPn /
ICC segments), the JPEG bytes and Image.open(f).convert("RGB") of each: the pixels of the small images, SHA-256 of the pixels of
the large ones.  Fallback cases (progressive, CMYK, PNG) carry their pixels too.  Run on a machine with Pillow; the fixture is data
only, and the GPU tests compare the device decoder with it without Pillow.

    python scripts/make_jpeg_golden.py

A second entry point writes tests/golden/jpeg_batches_pil.npz, the files of the device decoder's batch tests (below):

    python scripts/make_jpeg_golden.py batches
"""
import hashlib
import io
import os

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIXELS_MAX = 64 * 64          # images up to this many pixels store their pixels, larger ones a hash


def textured(rng, h, w, sigma):
    """a smooth colour field plus Gaussian noise of the given sigma (uint8 H x W x 3)"""
    lo = rng.integers(0, 256, (max(h // 16, 2), max(w // 16, 2), 3), dtype=np.uint8)
    base = np.asarray(Image.fromarray(lo).resize((w, h), Image.BICUBIC)).astype(np.float32)
    return np.clip(base + rng.normal(0, sigma, base.shape), 0, 255).astype(np.uint8)


def qtable_16bit():
    """a quantisation table with entries above 255 (Pillow writes it as a 16-bit table in an SOF1 frame)"""
    return [[min(1 + 7 * i, 600) for i in range(64)], [min(2 + 9 * i, 700) for i in range(64)]]


# name, (h, w), mode, sigma, save arguments
CASES = [
    ("1x1_444_q90", (1, 1), "RGB", 4, dict(quality=90, subsampling=0)),
    ("7x9_420_q50", (7, 9), "RGB", 4, dict(quality=50, subsampling=2)),
    ("7x9_gray_q90", (7, 9), "L", 4, dict(quality=90)),
    ("17x31_422_q100", (17, 31), "RGB", 8, dict(quality=100, subsampling=1)),
    ("17x31_420_q1", (17, 31), "RGB", 8, dict(quality=1, subsampling=2)),
    ("37x53_444_q5", (37, 53), "RGB", 8, dict(quality=5, subsampling=0)),
    ("37x53_420_q100_opt", (37, 53), "RGB", 16, dict(quality=100, subsampling=2, optimize=True)),
    ("37x53_420_rst1", (37, 53), "RGB", 8, dict(quality=90, subsampling=2, restart_marker_blocks=1)),
    ("37x53_422_rst3_opt", (37, 53), "RGB", 8, dict(quality=75, subsampling=1, restart_marker_blocks=3, optimize=True)),
    ("37x53_444_rows1", (37, 53), "RGB", 8, dict(quality=90, subsampling=0, restart_marker_rows=1)),
    ("37x53_gray_rst1", (37, 53), "L", 8, dict(quality=90, restart_marker_blocks=1)),
    ("37x53_420_qt16", (37, 53), "RGB", 8, dict(qtables=qtable_16bit(), subsampling=2)),
    ("37x53_420_markers", (37, 53), "RGB", 8, dict(quality=90, subsampling=2, comment="a comment segment",
                                                     icc_profile=bytes(range(256)) * 3, exif=b"Exif\x00\x00" + bytes(64))),
    ("333x500_420_q90_opt", (333, 500), "RGB", 6, dict(quality=90, subsampling=2, optimize=True)),
    ("500x375_444_q75", (500, 375), "RGB", 4, dict(quality=75, subsampling=0)),
    ("500x375_gray_q90_rows1", (500, 375), "L", 6, dict(quality=90, restart_marker_rows=1)),
    ("375x500_422_q50_rst3", (375, 500), "RGB", 6, dict(quality=50, subsampling=1, restart_marker_blocks=3)),
    ("1200x1600_420_q90", (1200, 1600), "RGB", 5, dict(quality=90, subsampling=2)),
    # fallbacks
    ("37x53_progressive", (37, 53), "RGB", 8, dict(quality=90, progressive=True)),
    ("37x53_cmyk", (37, 53), "CMYK", 8, dict(quality=90)),
    ("37x53_png", (37, 53), "RGB", 8, dict(format="PNG")),
]
FALLBACK_REASON = {"37x53_progressive": "progressive", "37x53_cmyk": "4 components", "37x53_png": "not a JPEG"}


def encode(img, mode, kw):
    kw = dict(kw)
    fmt = kw.pop("format", "JPEG")
    im = Image.fromarray(img)
    if mode == "L":
        im = Image.fromarray(img[..., 0])
    elif mode == "CMYK":
        im = im.convert("CMYK")
    bio = io.BytesIO()
    im.save(bio, fmt, **kw)
    return bio.getvalue()


def main():
    rng = np.random.default_rng(20261016)
    names, blobs, sizes, supported, reasons, sha, pixels, pix_off = [], [], [], [], [], [], [], [0]
    for name, (h, w), mode, sigma, kw in CASES:
        data = encode(textured(rng, h, w, sigma), mode, kw)
        px = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        names.append(name)
        blobs.append(np.frombuffer(data, np.uint8))
        sizes.append(px.shape[:2])
        supported.append(name not in FALLBACK_REASON)
        reasons.append(FALLBACK_REASON.get(name, ""))
        sha.append(np.frombuffer(hashlib.sha256(px.tobytes()).digest(), np.uint8))
        if px.shape[0] * px.shape[1] <= PIXELS_MAX:
            pixels.append(px.reshape(-1))
        pix_off.append(pix_off[-1] + (px.size if px.shape[0] * px.shape[1] <= PIXELS_MAX else 0))
        print(f"{name:28s} {len(data):8d} bytes")
    data_off = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.int64)
    path = os.path.join(ROOT, "tests", "golden", "jpeg_decode_pil.npz")
    np.savez_compressed(path, names=np.array(names), data=np.concatenate(blobs), data_off=data_off,
                        sizes=np.array(sizes, np.int32), supported=np.array(supported), reasons=np.array(reasons),
                        sha256=np.stack(sha), pixels=np.concatenate(pixels), pix_off=np.array(pix_off, np.int64))
    print(path, os.path.getsize(path), "bytes")


# ------------------------------------------------------------------------------------------------------------------------------
# tests/golden/jpeg_batches_pil.npz: files for the device decoder's batch tests (tests/test_jpeg_batches_cpu.py says what each
# structured file has to be).  JPEG bytes, sizes and the SHA-256 of Pillow's pixels; no pixels: the host decoder supplies them
# and the CPU test ties it to the hash.  A seed of its own: the first fixture's random stream is untouched.

BATCHES_SEED = 20261019
BATCHES_DATA_MAX = 1_000_000      # JPEG bytes in the fixture; the file stays under 1 MiB

# name, (h, w), mode, sigma, save arguments
STRUCTURED = [
    # several restart segments of 8-40 subsequences, >= 150 in all
    ("rows_mid", (256, 384), "RGB", 10, dict(quality=92, subsampling=0, restart_marker_rows=2)),
    # two restart segments, the first longer than 256 subsequences (20 of the 28 MCU rows)
    ("two_long", (448, 448), "RGB", 22, dict(quality=97, subsampling=2, restart_marker_rows=20)),
    # noise at quality 100: long codewords, slow self-synchronisation; one segment of 100-300 subsequences
    ("noise_q100", (124, 124), "RGB", 60, dict(quality=100, subsampling=0)),
    # an interval that does not divide 256, segments of 2 and 3 subsequences
    ("blocks37_opt", (200, 300), "RGB", 6, dict(quality=85, subsampling=1, optimize=True, restart_marker_blocks=37)),
    # thin images: downsampled widths / heights of 1 and 2, where libjpeg-turbo replicates instead of interpolating
    ("thin_130x2_420", (130, 2), "RGB", 8, dict(quality=90, subsampling=2)),
    ("thin_2x130_420", (2, 130), "RGB", 8, dict(quality=90, subsampling=2)),
    ("thin_3x200_422", (3, 200), "RGB", 8, dict(quality=90, subsampling=1)),
    ("thin_200x3_422", (200, 3), "RGB", 8, dict(quality=90, subsampling=1)),
    ("thin_1x64_444", (1, 64), "RGB", 8, dict(quality=90, subsampling=0)),
    ("thin_64x1_444", (64, 1), "RGB", 8, dict(quality=90, subsampling=0)),
    ("thin_17x1_gray", (17, 1), "L", 8, dict(quality=90)),
]
RANDOM_MIN = 130
RANDOM_DRAWS = 400


def build_batches():
    """the arrays of jpeg_batches_pil.npz"""
    import sys
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from test_jpeg_cpu import _random_jpeg      # the CPU test's distribution, not a copy of it

    rng = np.random.default_rng(BATCHES_SEED)
    names, blobs = [], []
    for name, (h, w), mode, sigma, kw in STRUCTURED:
        names.append(name)
        blobs.append(encode(textured(rng, h, w, sigma), mode, kw))
    total = sum(len(b) for b in blobs)
    for _ in range(RANDOM_DRAWS):                 # as many small random files as the size cap allows
        data, kw = _random_jpeg(rng, Image)
        if data is None or total + len(data) > BATCHES_DATA_MAX:
            continue
        names.append(f"random_{len(names) - len(STRUCTURED):03d}")
        blobs.append(data)
        total += len(data)
    assert len(names) - len(STRUCTURED) >= RANDOM_MIN, len(names)
    sizes, sha = [], []
    for data in blobs:
        px = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        sizes.append(px.shape[:2])
        sha.append(np.frombuffer(hashlib.sha256(px.tobytes()).digest(), np.uint8))
    data_off = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.int64)
    return dict(names=np.array(names), data=np.concatenate([np.frombuffer(b, np.uint8) for b in blobs]), data_off=data_off,
                sizes=np.array(sizes, np.int32), sha256=np.stack(sha))


def main_batches():
    z = build_batches()
    for i, name in enumerate(z["names"][:len(STRUCTURED)]):
        print(f"{name:28s} {int(z['data_off'][i + 1] - z['data_off'][i]):8d} bytes")
    print(len(z["names"]) - len(STRUCTURED), "random files,", int(z["data_off"][-1]), "bytes of JPEG in all")
    path = os.path.join(ROOT, "tests", "golden", "jpeg_batches_pil.npz")
    np.savez_compressed(path, **z)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    import sys
    if sys.argv[1:] == ["batches"]:
        main_batches()
    else:
        main()
