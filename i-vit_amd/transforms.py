"""The reference's evaluation transform on the device (scripts/inference.py:63-66, utils/data_utils.py:82-91):
Resize(s, BICUBIC) -> CenterCrop(c) -> ToTensor -> Normalize, without torchvision.

ImageFolderU8 decodes on the CPU; ImageFolderJPEG hands the compressed bytes on, and EvalTransform decodes baseline JPEGs on the
device (ivit_jpeg_decode_u8, byte-identical to Image.open(f).convert("RGB")), every other file in the loader worker with Pillow.
The resize and crop run in ivit_resize_crop_bicubic_u8 (h x w crops, an exact-size Resize((h, w)) and CenterCrop's zero padding:
ivit_resize_crop_bicubic_hw_u8) and are byte-identical to Pillow's resize plus torchvision's CenterCrop.  The fused engines take the uint8 crops as they are (their input table folds
ToTensor + Normalize + the input QuantAct); the module path takes EvalTransform.to_float(crops), the float32 tensor ToTensor +
Normalize would give.

    loader = torch.utils.data.DataLoader(ImageFolderU8(root), batch_size=256, collate_fn=ImageFolderU8.collate)
    inference.evaluate_dataset_parallel(model, loader, "cuda", transform=EvalTransform.for_input_size(224))

EvalTransform.for_model(model) is the transform of the model's own image size, square or h x w.

ImageFolderJPEG / ImageFolderJPEG.collate in place of ImageFolderU8 / ImageFolderU8.collate decode on the device instead.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib
from .prepare import IMAGENET_MEAN, IMAGENET_STD

# torchvision.datasets.folder.IMG_EXTENSIONS
IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")


def eval_geometry(h: int, w: int, resize: int, crop: int):
    """(new_h, new_w, top, left) of Resize([resize]) + CenterCrop(crop) for an h x w image (the library's ivit_eval_geometry, a host
    function: the rule exists once).  ValueError for what the library calls an unsupported geometry."""
    out = (C.c_int32 * 4)()
    L = _lib.lib()
    rc = L.ivit_eval_geometry(int(h), int(w), int(resize), int(crop), out)
    if rc != 0:
        raise ValueError(L.ivit_last_error_string().decode())
    return tuple(int(v) for v in out)


def _key(v, what):
    """an int or a pair (h, w) in the form a geometry cache key and an EvalTransform hold: a scalar becomes an int, a pair a tuple
    of two ints"""
    try:
        a, b = v
    except TypeError:
        return int(v)
    except ValueError:
        raise ValueError(f"{what} must be an int or a pair (h, w), got {v!r}") from None
    return int(a), int(b)


def _pair(v, what):
    """an int n -> (n, n); a pair -> (int, int)"""
    k = _key(v, what)
    return (k, k) if isinstance(k, int) else k


def eval_geometry_hw(h: int, w: int, resize, crop, pad: bool = False):
    """(new_h, new_w, top, left) of Resize(resize) + CenterCrop(crop) for an h x w image, the library's ivit_eval_geometry_hw (a host
    function: the rule exists once).  resize: an int (the short side goes to it) or a pair (exactly that size); crop: an int or a
    pair (h, w).  Where a crop side is longer than the resized image torchvision pads with zeros: with pad the offset on that axis
    is minus the zeros in front, -((c - n) // 2); without it the geometry is unsupported.  ValueError for an unsupported geometry."""
    resize = _key(resize, "resize")
    if isinstance(resize, int):
        rh, rw = resize, 0            # the library's spelling of the short-side rule
    else:
        rh, rw = resize
        if rw < 1:
            raise ValueError(f"unsupported geometry (resize {rh} x {rw})")
    ch, cw = _pair(crop, "crop")
    out = (C.c_int32 * 4)()
    L = _lib.lib()
    rc = L.ivit_eval_geometry_hw(int(h), int(w), rh, rw, ch, cw, int(bool(pad)), out)
    if rc != 0:
        raise ValueError(L.ivit_last_error_string().decode())
    return tuple(int(v) for v in out)


def _geometry_rows(sizes, cache, resize, crop, pad):
    """int32 [B, 6] rows (h, w, new_h, new_w, top, left) of a batch, cached under the full (resize, crop, pad) tuple.  Two ints
    without pad go through eval_geometry (the square rule and its refusals), everything else through eval_geometry_hw."""
    key = (_key(resize, "resize"), _key(crop, "crop"), bool(pad))
    g = cache.get(key)
    if g is None:
        square = isinstance(key[0], int) and isinstance(key[1], int) and not key[2]
        g = np.empty((len(sizes), 6), np.int32)
        for b, (h, w) in enumerate(sizes):
            g[b, :2] = (h, w)
            g[b, 2:] = eval_geometry(h, w, key[0], key[1]) if square else eval_geometry_hw(h, w, key[0], key[1], key[2])
        cache[key] = g
    return g


@dataclass
class PackedImages:
    """A batch of decoded RGB images in one flat uint8 buffer (HWC, image b at data[offsets[b]:]), their sizes, and the per-image
    geometry rows the device transform takes (cached per (resize, crop, pad))."""
    data: torch.Tensor          # uint8 [total bytes], pinned when a GPU is present
    offsets: np.ndarray         # int64 [B]
    sizes: np.ndarray           # int32 [B, 2]: (h, w)
    _geom: dict = field(default_factory=dict, repr=False)

    def __len__(self):
        return len(self.offsets)

    def size(self, dim=0):      # evaluate_dataset* read the batch size as imgs.size(0)
        if dim != 0:
            raise IndexError("PackedImages has one dimension: images")
        return len(self)

    def geometry(self, resize, crop, pad: bool = False) -> np.ndarray:
        """int32 [B, 6]: (h, w, new_h, new_w, top, left) per image; resize and crop an int or a pair (h, w), as eval_geometry_hw"""
        return _geometry_rows(self.sizes, self._geom, resize, crop, pad)


def pack_images(images, pin: bool | None = None) -> PackedImages:
    """list of uint8 H x W x 3 arrays -> PackedImages (the collate function of a loader).  pin=None pins the buffer when a GPU is
    present (pass pin=False in loader worker processes that must not touch the GPU)."""
    sizes = np.empty((len(images), 2), np.int32)
    offsets = np.empty(len(images), np.int64)
    total = 0
    for b, im in enumerate(images):
        a = np.asarray(im)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
            raise ValueError(f"image {b}: expected a non-empty uint8 H x W x 3 array, got {a.dtype} {a.shape}")
        sizes[b] = a.shape[:2]
        offsets[b] = total
        total += a.size
    if pin is None:
        pin = torch.cuda.is_available()
    data = torch.empty(total, dtype=torch.uint8, pin_memory=bool(pin))
    flat = data.numpy()
    for b, im in enumerate(images):
        a = np.asarray(im)
        flat[offsets[b]:offsets[b] + a.size] = a.reshape(-1)
    return PackedImages(data, offsets, sizes)


class EvalTransform:
    """Resize(resize, BICUBIC) -> CenterCrop(crop) on the device; mean / std are the Normalize the model was trained behind.
    transform(packed, lo, hi) -> device uint8 [hi - lo, 3, crop_h, crop_w] of images [lo, hi) of the packed batch.

    resize: an int (torchvision Resize([s]): the short side goes to s) or a pair (h, w) (Resize((h, w)): exactly that size, whatever
    the image's aspect ratio -- how Swin's 384 px checkpoints are evaluated).  crop: an int or a pair (h, w).  pad: torchvision's
    CenterCrop pads with zeros where the crop is longer than the resized image; that has to be asked for.  Without pad, a
    combination under which some image would be padded is refused here, before any image is seen.  .resize and .crop keep the
    form they were given in (ints stay ints); .crop_hw is always the pair."""

    def __init__(self, resize=256, crop=224, mean=IMAGENET_MEAN, std=IMAGENET_STD, pad: bool = False):
        self.resize, self.crop, self.pad = _key(resize, "resize"), _key(crop, "crop"), bool(pad)
        self.crop_hw = _pair(self.crop, "crop")
        # two ints without pad: ivit_resize_crop_bicubic_u8 and its rules, as before there were pairs
        self._square = isinstance(self.resize, int) and isinstance(self.crop, int) and not self.pad
        if min(self.crop_hw) <= 32:
            raise ValueError(f"crop {self.crop} <= 32: input sizes without a resize (CIFAR) are not supported")
        if not self.pad:
            # Resize([s]) leaves both sides >= s, and the short one at s; Resize((h, w)) leaves exactly (h, w)
            if isinstance(self.resize, int) and max(self.crop_hw) > self.resize:
                raise ValueError(f"crop {self.crop} > resize {self.resize}: torchvision would pad")
            if not isinstance(self.resize, int) and (self.crop_hw[0] > self.resize[0] or self.crop_hw[1] > self.resize[1]):
                raise ValueError(f"crop {self.crop} > resize {self.resize}: torchvision would pad (pass pad=True)")
        if min(_pair(self.resize, "resize")) < 1:
            raise ValueError(f"resize {self.resize} < 1")
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self._ws = {}
        self._tables = {}

    @classmethod
    def for_input_size(cls, n, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        """utils/data_utils.py build_transform: Resize(int(256 / 224 * n)) -> CenterCrop(n) (384 -> 438 / 384).

        n = (h, w): Resize(int(256 / 224 * max(h, w))) -> CenterCrop((h, w)).  The reference has no rule for h != w; max is chosen
        because (1) Resize([s]) leaves both sides of every image at least s, so s >= max(h, w) is the only choice of the reference's
        form under which no image is ever padded, whatever its aspect ratio (with min(h, w), a portrait image into a landscape crop
        would be), and (2) it is the reference's rule at h == w."""
        n = _key(n, "input size")
        if isinstance(n, int):
            if n <= 32:
                raise ValueError(f"input size {n} <= 32: the reference does not resize there (out of scope)")
            return cls(int((256 / 224) * n), n, mean, std)
        h, w = n
        if min(h, w) <= 32:
            raise ValueError(f"input size {h} x {w} <= 32: the reference does not resize there (out of scope)")
        return cls(int((256 / 224) * max(h, w)), (h, w), mean, std)

    @classmethod
    def for_model(cls, model, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        """for_input_size of the model's own image size (VisionTransformer, SwinTransformer: patch_embed.img_size); a square model
        gets the int form, the reference's transform"""
        try:
            h, w = (int(v) for v in model.patch_embed.img_size)
        except (AttributeError, TypeError, ValueError):
            raise TypeError(f"{type(model).__name__} has no patch_embed.img_size: pass the size to for_input_size") from None
        return cls.for_input_size(h if h == w else (h, w), mean, std)

    @property
    def default_normalisation(self) -> bool:
        return self.mean == tuple(IMAGENET_MEAN) and self.std == tuple(IMAGENET_STD)

    def __repr__(self):
        pad = ", pad=True" if self.pad else ""
        return f"EvalTransform(resize={self.resize}, crop={self.crop}, mean={self.mean}, std={self.std}{pad})"

    def _workspace(self, device, nbytes):
        ws = self._ws.get(device)
        if ws is None or ws.numel() < nbytes:
            ws = self._ws[device] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        return ws

    def __call__(self, packed, lo: int = 0, hi: int | None = None, device="cuda", out: torch.Tensor | None = None):
        """packed: a PackedImages, or an EncodedImages whose images [lo, hi) are decoded on the device first"""
        hi = len(packed) if hi is None else hi
        if not 0 <= lo <= hi <= len(packed):
            raise IndexError(f"shard [{lo}, {hi}) of a batch of {len(packed)}")
        if isinstance(packed, EncodedImages):
            packed = decode_images(packed, lo, hi, device)
            lo, hi = 0, len(packed)
        n, (ch, cw) = hi - lo, self.crop_hw
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if out is None:
            out = torch.empty(n, 3, ch, cw, dtype=torch.uint8, device=device)
        elif out.shape != (n, 3, ch, cw) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != device:
            raise ValueError(f"out must be a contiguous uint8 [{n}, 3, {ch}, {cw}] tensor on {device}")
        if n == 0:
            return out
        geom = np.ascontiguousarray(packed.geometry(self.resize, self.crop, self.pad)[lo:hi])
        plan = (C.c_int32 * 3)()
        nbytes = C.c_int64()
        L = _lib.lib()
        # two ints without pad: the square entries and their refusals; everything else: the h x w entries
        suffix, crop_args = ("", (ch,)) if self._square else ("_hw", (ch, cw))
        rc = getattr(L, "ivit_resize_crop_workspace" + suffix)(geom.ctypes.data_as(C.c_void_p), n, *crop_args, plan, C.byref(nbytes))
        if rc != 0:
            raise _lib.IvitError(f"ivit_resize_crop_workspace{suffix} failed ({rc}): {L.ivit_last_error_string().decode()}")
        start = int(packed.offsets[lo])
        end = int(packed.offsets[hi]) if hi < len(packed) else packed.data.numel()
        src = packed.data[start:end].to(device, non_blocking=True)
        offs = torch.from_numpy(packed.offsets[lo:hi] - start).to(device)
        g = torch.from_numpy(geom).to(device)
        ws = self._workspace(device, nbytes.value)
        with torch.cuda.device(device):
            _lib.call(f"ivit_resize_crop_bicubic{suffix}_u8", _lib.ptr(src), _lib.ptr(offs), _lib.ptr(g), n, *crop_args, plan[0], plan[1],
                      plan[2], _lib.ptr(ws), ws.numel(), _lib.ptr(out), _lib.stream_ptr())
        return out

    def table(self) -> np.ndarray:
        """float32 [3, 256]: ToTensor (v / 255) then Normalize ((x - mean) / std), in float32 in torchvision's order"""
        v = np.arange(256, dtype=np.float32) / np.float32(255.0)
        return np.stack([((v - np.float32(m)).astype(np.float32) / np.float32(s)).astype(np.float32)
                         for m, s in zip(self.mean, self.std)])

    def to_float(self, u8: torch.Tensor) -> torch.Tensor:
        """uint8 [B, 3, H, W] -> the float32 tensor ToTensor + Normalize produce (a gather from table())"""
        if u8.dtype != torch.uint8 or u8.dim() != 4 or u8.shape[1] != 3:
            raise ValueError(f"expected uint8 [B, 3, H, W], got {u8.dtype} {tuple(u8.shape)}")
        t = self._tables.get(u8.device)
        if t is None:
            t = self._tables[u8.device] = torch.from_numpy(self.table()).to(u8.device)
        out = torch.empty(u8.shape, dtype=torch.float32, device=u8.device)
        for ch in range(3):
            out[:, ch] = t[ch][u8[:, ch].long()]
        return out


def _pil_loader(path):
    try:
        from PIL import Image
    except ImportError as e:   # decoding is the one CPU step left; it needs Pillow
        raise ImportError("ImageFolderU8 decodes images with Pillow, which is not installed (pip install pillow)") from e
    with open(path, "rb") as f:
        img = Image.open(f)
        return np.asarray(img.convert("RGB"))


class ImageFolderU8:
    """torchvision.datasets.ImageFolder's indexing (sorted class folders, sorted walk, its extension list, RGB conversion) that
    returns decoded uint8 H x W x 3 arrays instead of transformed tensors.  collate -> (PackedImages, int64 targets)."""

    def __init__(self, root, extensions=IMG_EXTENSIONS):
        self.root = os.fspath(root)
        self.classes = sorted(e.name for e in os.scandir(self.root) if e.is_dir())
        if not self.classes:
            raise FileNotFoundError(f"no class folders in {self.root}")
        self.class_to_idx = {c: i for i, c in enumerate(self.classes)}
        exts = tuple(x.lower() for x in extensions)
        self.samples = []
        for cls in self.classes:
            for dirpath, _, fnames in sorted(os.walk(os.path.join(self.root, cls), followlinks=True)):
                for fname in sorted(fnames):
                    if fname.lower().endswith(exts):
                        self.samples.append((os.path.join(dirpath, fname), self.class_to_idx[cls]))
        self.targets = [t for _, t in self.samples]

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, i):
        path, target = self.samples[i]
        return _pil_loader(path), target

    @staticmethod
    def collate(batch, pin: bool | None = None):
        imgs, targets = zip(*batch)
        return pack_images(list(imgs), pin=pin), torch.tensor(targets, dtype=torch.int64)


# ---- JPEG decoding on the device ------------------------------------------------------------------------------------------

_INDEX_BYTES = 40          # ivit_jpeg_workspace's index row
_JPEG_WS = {}              # device -> workspace


def _pil_decode_bytes(data) -> np.ndarray:
    """Image.open(f).convert("RGB") of an encoded file held in memory (the reference's loader)"""
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("files the device decoder does not take are decoded with Pillow, which is not installed") from e
    import io
    with Image.open(io.BytesIO(bytes(data))) as img:
        return np.asarray(img.convert("RGB"))


def probe_jpeg(data) -> tuple:
    """(supported, reason, info): supported is True for a file ivit_jpeg_decode_u8 decodes; reason says why not; info = (h, w,
    components, sampling) as far as the header gives them (sampling 0 gray, 1 4:4:4, 2 4:2:2, 3 4:2:0, -1 unsupported)"""
    buf = bytes(data)
    info = (C.c_int32 * 4)()
    L = _lib.lib()
    rc = L.ivit_jpeg_probe(buf, len(buf), info)
    if rc == 0:
        return True, "", tuple(int(v) for v in info)
    return False, L.ivit_last_error_string().decode(), tuple(int(v) for v in info)


def decode_jpeg_host(data) -> np.ndarray:
    """ivit_jpeg_decode_host: one file decoded serially on the host with the device's primitives (uint8 H x W x 3).
    IvitError for a file the probe rejects or corrupt entropy data."""
    buf = bytes(data)
    ok, reason, info = probe_jpeg(buf)
    if not ok:
        raise _lib.IvitError(f"unsupported JPEG: {reason}")
    out = np.empty((info[0], info[1], 3), np.uint8)
    _lib.call("ivit_jpeg_decode_host", buf, len(buf), out.ctypes.data_as(C.c_void_p), out.size)
    return out


@dataclass
class EncodedImages:
    """A batch of compressed images with PackedImages' interface (len, size(0), geometry(resize, crop, pad) from the header sizes).
    The device images' plan sections (ivit_jpeg_plan_image) lie in one buffer, in image order; the other images carry Pillow's
    pixels (fallback) and the probe's reason (reasons)."""
    plan: torch.Tensor          # uint8 [plan bytes], pinned when a GPU is present
    sec_offsets: np.ndarray     # int64 [B]: section of image b in plan, -1 for a fallback image
    sec_bytes: np.ndarray       # int64 [B]: its size, 0 for a fallback image
    offsets: np.ndarray         # int64 [B]: HWC offset of image b in the decoded batch (pack_images' offsets)
    sizes: np.ndarray           # int32 [B, 2]: (h, w)
    fallback: dict = field(default_factory=dict)   # b -> uint8 H x W x 3
    reasons: dict = field(default_factory=dict)    # b -> why b is not decoded on the device
    _geom: dict = field(default_factory=dict, repr=False)

    def __len__(self):
        return len(self.offsets)

    def size(self, dim=0):
        if dim != 0:
            raise IndexError("EncodedImages has one dimension: images")
        return len(self)

    def geometry(self, resize, crop, pad: bool = False) -> np.ndarray:
        """int32 [B, 6]: (h, w, new_h, new_w, top, left) per image; resize and crop an int or a pair (h, w), as eval_geometry_hw"""
        return _geometry_rows(self.sizes, self._geom, resize, crop, pad)


def encode_images(files, decode_fallback=None, pin: bool | None = None) -> EncodedImages:
    """list of encoded files (bytes) -> EncodedImages: probe and plan every file; decode_fallback(b, data) -> uint8 H x W x 3
    decodes the others (default: Pillow's convert("RGB")).  Host code only: loader workers call it without touching the GPU
    (pass pin=False there)."""
    L = _lib.lib()
    n = len(files)
    bufs = [bytes(f) for f in files]
    sec_bytes = np.zeros(n, np.int64)
    sec_offsets = np.full(n, -1, np.int64)
    reasons = {}
    total = 0
    nb = C.c_int64()
    for b, buf in enumerate(bufs):
        if L.ivit_jpeg_plan_image(buf, len(buf), None, 0, C.byref(nb)) == 0:
            sec_offsets[b], sec_bytes[b] = total, nb.value
            total += nb.value
        else:
            reasons[b] = L.ivit_last_error_string().decode()
    if pin is None:
        pin = torch.cuda.is_available()
    plan = torch.empty(max(total, 16), dtype=torch.uint8, pin_memory=bool(pin))
    base = plan.data_ptr()
    sizes = np.empty((n, 2), np.int32)
    fallback = {}
    decode_fallback = decode_fallback or (lambda b, data: _pil_decode_bytes(data))
    for b, buf in enumerate(bufs):
        if sec_offsets[b] >= 0:
            rc = L.ivit_jpeg_plan_image(buf, len(buf), C.c_void_p(base + int(sec_offsets[b])), int(sec_bytes[b]), C.byref(nb))
            if rc != 0:
                raise _lib.IvitError(f"ivit_jpeg_plan_image failed ({rc}): {L.ivit_last_error_string().decode()}")
            hw = np.frombuffer(C.string_at(base + int(sec_offsets[b]) + 8, 8), np.int32)   # Sec: int64 bytes, then h, w
            sizes[b] = hw
        else:
            a = np.ascontiguousarray(decode_fallback(b, buf))
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
                raise ValueError(f"image {b}: fallback decode gave {a.dtype} {a.shape}, expected uint8 H x W x 3")
            fallback[b] = a
            sizes[b] = a.shape[:2]
    px = sizes[:, 0].astype(np.int64) * sizes[:, 1] * 3
    offsets = np.concatenate([[0], np.cumsum(px)[:-1]]).astype(np.int64) if n else np.zeros(0, np.int64)
    return EncodedImages(plan, sec_offsets, sec_bytes, offsets, sizes, fallback, reasons)


def _jpeg_workspace(device, nbytes):
    ws = _JPEG_WS.get(device)
    if ws is None or ws.numel() < nbytes:
        ws = _JPEG_WS[device] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
    return ws


def decode_images(encoded: EncodedImages, lo: int = 0, hi: int | None = None, device="cuda") -> PackedImages:
    """Images [lo, hi) of an EncodedImages -> a device-resident PackedImages: the device images decoded by ivit_jpeg_decode_u8
    (one copy of their plan sections), the fallback images' pixels copied in.  IvitError for corrupt entropy data."""
    hi = len(encoded) if hi is None else hi
    if not 0 <= lo <= hi <= len(encoded):
        raise IndexError(f"shard [{lo}, {hi}) of a batch of {len(encoded)}")
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    n = hi - lo
    start = int(encoded.offsets[lo]) if n else 0
    sizes = encoded.sizes[lo:hi].copy()
    offs = encoded.offsets[lo:hi] - start
    total = int((sizes[:, 0].astype(np.int64) * sizes[:, 1] * 3).sum())
    out = torch.empty(max(total, 1), dtype=torch.uint8, device=device)
    sec = encoded.sec_offsets[lo:hi]
    dev = np.nonzero(sec >= 0)[0]
    errors = None
    if len(dev):
        p0 = int(sec[dev[0]])
        p1 = int(sec[dev[-1]] + encoded.sec_bytes[lo + dev[-1]])
        host_plan = encoded.plan[p0:p1]
        rel = np.ascontiguousarray(np.where(sec >= 0, sec - p0, -1).astype(np.int64))
        offs_c = np.ascontiguousarray(offs.astype(np.int64))
        index = torch.empty(n * _INDEX_BYTES, dtype=torch.uint8, pin_memory=encoded.plan.is_pinned())
        sizes4 = (C.c_int64 * 4)()
        _lib.call("ivit_jpeg_workspace", C.c_void_p(host_plan.data_ptr()), p1 - p0, rel.ctypes.data_as(C.c_void_p),
                  offs_c.ctypes.data_as(C.c_void_p), n, C.c_void_p(index.data_ptr()), sizes4)
        plan_d = host_plan.to(device, non_blocking=True)
        index_d = index.to(device, non_blocking=True)
        errors = torch.empty(n, dtype=torch.int32, device=device)
        with torch.cuda.device(device):
            ws = _jpeg_workspace(device, int(sizes4[0]))
            _lib.call("ivit_jpeg_decode_u8", _lib.ptr(plan_d), _lib.ptr(index_d), n, sizes4[1], sizes4[2], sizes4[3], _lib.ptr(ws),
                      ws.numel(), _lib.ptr(out), _lib.ptr(errors), _lib.stream_ptr())
    for b in range(lo, hi):
        a = encoded.fallback.get(b)
        if a is not None:
            o = int(encoded.offsets[b]) - start
            out[o:o + a.size].copy_(torch.from_numpy(a.reshape(-1)).to(device))
    if errors is not None:
        bad = np.nonzero(errors.cpu().numpy())[0]
        if len(bad):
            raise _lib.IvitError(f"corrupt JPEG data in image(s) {[int(lo + b) for b in bad]} of the batch")
    return PackedImages(out, offs.astype(np.int64), sizes)


class ImageFolderJPEG(ImageFolderU8):
    """ImageFolderU8's indexing; items are the files' bytes, and collate -> (EncodedImages, int64 targets): it probes and plans
    every file and decodes the ones the device does not take with Pillow, in the loader worker."""

    def __getitem__(self, i):
        path, target = self.samples[i]
        with open(path, "rb") as f:
            return f.read(), target

    @staticmethod
    def collate(batch, pin: bool | None = None):
        files, targets = zip(*batch)
        return encode_images(list(files), pin=pin), torch.tensor(targets, dtype=torch.int64)
