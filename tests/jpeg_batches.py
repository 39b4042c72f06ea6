"""Shared by tests/test_jpeg_batches_cpu.py and tests/test_gpu_jpeg_batches.py: the files of tests/golden/jpeg_batches_pil.npz,
the batches that put a 256-multiple of the global subsequence index on a named spot of a named file (place, PLACEMENTS), the index
rows ivit_jpeg_workspace writes for a batch, and the seeded corrupt set.  Host code only: neither Pillow nor a GPU."""
import ctypes as C
import os

import numpy as np

from ivit_amd import _lib
from ivit_amd.transforms import decode_jpeg_host, encode_images, probe_jpeg

import jpeg_sync_ref as ref
from test_jpeg_cpu import CASES as OLD_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg_batches_pil.npz")
LANES = ref.LANES

INDEX = np.dtype([("sec", "<i8"), ("out", "<i8"), ("coef", "<i8"), ("plane", "<i8"), ("sub_first", "<i4"), ("nsub", "<i4")])
assert INDEX.itemsize == 40


def _load():
    z = np.load(GOLDEN)
    out = []
    for i, name in enumerate(z["names"]):
        data = z["data"][z["data_off"][i]:z["data_off"][i + 1]].tobytes()
        h, w = (int(v) for v in z["sizes"][i])
        out.append(dict(name=str(name), data=data, h=h, w=w, sha=z["sha256"][i].tobytes(), supported=True, pixels=None))
    return out


FILES = _load()
BY_NAME = {f["name"]: f for f in FILES}
RANDOM = [f for f in FILES if f["name"].startswith("random_")]
THIN = [f for f in FILES if f["name"].startswith("thin_")]
OLD = {c["name"]: c for c in OLD_CASES}
FALLBACKS = [c for c in OLD_CASES if not c["supported"]]       # progressive, CMYK, PNG: their pixels come with the old fixture
FILLER = BY_NAME["thin_1x64_444"]                               # one restart segment of one subsequence

_HOST = {}


def host_pixels(f):
    """ivit_jpeg_decode_host of a file, computed once (the fallback files: the pixels stored with them)"""
    if f["pixels"] is not None and not f["supported"]:
        return f["pixels"]
    px = _HOST.get(f["data"])
    if px is None:
        px = _HOST[f["data"]] = decode_jpeg_host(f["data"])
        px.setflags(write=False)
    return px


def encode(files, pin=None):
    """encode_images of a list of files; the fallback files' pixels are supplied, so Pillow is not needed"""
    return encode_images([f["data"] for f in files], decode_fallback=lambda b, data: files[b]["pixels"], pin=pin)


def index_rows(enc, lo=0, hi=None, out_offsets=None):
    """the index ivit_jpeg_workspace writes for images [lo, hi) of an EncodedImages -> (rows as an INDEX array, sizes4, plan slice,
    section offsets relative to the slice, output offsets); what decode_images does, on the host.  out_offsets: other
    output offsets than the packed ones"""
    hi = len(enc) if hi is None else hi
    n = hi - lo
    sec = enc.sec_offsets[lo:hi]
    dev = np.nonzero(sec >= 0)[0]
    p0 = int(sec[dev[0]])
    p1 = int(sec[dev[-1]] + enc.sec_bytes[lo + dev[-1]])
    plan = enc.plan[p0:p1]
    rel = np.ascontiguousarray(np.where(sec >= 0, sec - p0, -1).astype(np.int64))
    offs = np.ascontiguousarray((enc.offsets[lo:hi] - enc.offsets[lo] if out_offsets is None else out_offsets).astype(np.int64))
    assert offs.shape == (n,)
    index = np.zeros(n * INDEX.itemsize, np.uint8)
    sizes4 = (C.c_int64 * 4)()
    _lib.call("ivit_jpeg_workspace", C.c_void_p(plan.data_ptr()), p1 - p0, rel.ctypes.data_as(C.c_void_p),
              offs.ctypes.data_as(C.c_void_p), n, index.ctypes.data_as(C.c_void_p), sizes4)
    return index.view(INDEX), [int(v) for v in sizes4], plan, rel, offs


_NSUB = {}


def nsub(f):
    """subsequences per restart segment of a file, by the restatement"""
    s = _NSUB.get(f["data"])
    if s is None:
        s = _NSUB[f["data"]] = ref.subsequences(f["data"]) if f["supported"] else []
    return s


def seg_first(f, seg):
    """local index of the first subsequence of a restart segment"""
    return sum(nsub(f)[:seg])


def place(files, target, min_index=0):
    """Prepends one-subsequence files until a 256-multiple of the global subsequence index falls on subsequence target[1] of
    files[target[0]], and that image's index in the batch is at least min_index.  -> (the batch, the target's index in it)"""
    t, local = target
    assert 0 <= local < sum(nsub(files[t]))
    before = sum(sum(nsub(f)) for f in files[:t])
    k = -(before + local) % LANES
    while k + t < min_index:
        k += LANES
    return [FILLER] * k + list(files), k + t


def _placements():
    rows, two, noise, b37 = (BY_NAME[n] for n in ("rows_mid", "two_long", "noise_q100", "blocks37_opt"))
    thin = BY_NAME["thin_200x3_422"]
    prog = OLD["37x53_progressive"]
    last = sum(nsub(rows)) - 1
    # name -> (files, (position of the target file, local subsequence), least index of the target image, what lies there)
    return {
        "a_image_start": ([b37, rows, thin], (1, 0), 0, "the first subsequence of an image with index > 0"),
        "b_segment_start": ([thin, rows, b37], (1, seg_first(rows, 5)), 0, "the first subsequence of a non-first restart segment"),
        "c_segment_second": ([thin, rows, b37], (1, seg_first(rows, 5) + 1), 0, "the second subsequence of a non-first segment"),
        "d_segment_last": ([b37, rows, thin], (1, seg_first(rows, 7) - 1), 0, "the last subsequence of a non-last segment"),
        "e_image_last_then_device": ([thin, rows, b37], (1, last), 0, "the last subsequence of an image, a device image next"),
        "e_image_last_then_fallback": ([thin, rows, prog, b37], (1, last), 0, "the last subsequence of an image, a fallback next"),
        "f_two_in_long_segment": ([two, b37], (0, 5), 64, "two boundaries inside one long segment, image index >= 64"),
        "g_inside_noise": ([thin, noise, b37], (1, 60), 0, "a boundary inside noise at quality 100"),
    }


PLACEMENTS = _placements()


def placed(name):
    """-> (the batch's files, the target image's index, the target's local subsequence)"""
    files, target, min_index, _ = PLACEMENTS[name]
    batch, b = place(files, target, min_index)
    return batch, b, target[1]


# ------------------------------------------------------------------------------------------------------------------------------
# the corrupt set: seeded mutations of a 4:2:0 file and of a file with restart markers, made as
# test_jpeg_cpu.test_corrupt_entropy_data_is_an_error_and_stays_in_bounds makes them; only what the probe accepts is kept

CORRUPT_SEED = 11
CORRUPT_SOURCES = ("37x53_420_q100_opt", "37x53_444_rows1")
CORRUPT_MUTATIONS = 24


def _mutations():
    rng = np.random.default_rng(CORRUPT_SEED)
    out = []
    for it in range(CORRUPT_MUTATIONS):
        src = OLD[CORRUPT_SOURCES[(it // 2) % 2]]
        c = src["data"]
        sos = c.index(b"\xff\xda")
        start = sos + 2 + int.from_bytes(c[sos + 2:sos + 4], "big")
        b = bytearray(c)
        if it % 2:
            for _ in range(8):   # random bytes (no 0xFF: the marker structure stays)
                b[int(rng.integers(start, len(c) - 2))] = int(rng.integers(0, 255))
        else:                    # the scan cut short, EOI kept
            cut = int(rng.integers(start + 1, len(c) - 2))
            b = b[:cut] + b"\xff\xd9"
        out.append((src, bytes(b)))
    return out


def corrupt_set():
    """-> list of dict(name, data, h, w, source, refused, pixels): the mutations the probe accepts; refused: the host decoder
    raises "corrupt"; else pixels: what it decodes"""
    out = []
    for k, (src, data) in enumerate(_mutations()):
        if not probe_jpeg(data)[0]:
            continue
        f = dict(name=f"corrupt_{k:02d}_{src['name']}", data=data, h=src["h"], w=src["w"], source=src, supported=True)
        try:
            f["pixels"] = decode_jpeg_host(data)
            f["refused"] = False
        except _lib.IvitError as e:
            assert "corrupt" in str(e), str(e)
            f["pixels"] = None
            f["refused"] = True
        out.append(f)
    return out
