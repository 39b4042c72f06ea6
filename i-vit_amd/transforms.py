"""The reference's evaluation transform on the device (scripts/inference.py:63-66, utils/data_utils.py:82-91):
Resize(s, BICUBIC) -> CenterCrop(c) -> ToTensor -> Normalize, without torchvision.

Decoding stays on the CPU (ImageFolderU8); the resize and crop run in ivit_resize_crop_bicubic_u8 and are byte-identical to
Pillow's resize plus torchvision's CenterCrop.  The fused engines take the uint8 crops as they are (their input table folds
ToTensor + Normalize + the input QuantAct); the module path takes EvalTransform.to_float(crops), the float32 tensor ToTensor +
Normalize would give.

    loader = torch.utils.data.DataLoader(ImageFolderU8(root), batch_size=256, collate_fn=ImageFolderU8.collate)
    inference.evaluate_dataset_parallel(model, loader, "cuda", transform=EvalTransform.for_input_size(224))
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


@dataclass
class PackedImages:
    """A batch of decoded RGB images in one flat uint8 buffer (HWC, image b at data[offsets[b]:]), their sizes, and the per-image
    geometry rows the device transform takes (cached per (resize, crop))."""
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

    def geometry(self, resize: int, crop: int) -> np.ndarray:
        """int32 [B, 6]: (h, w, new_h, new_w, top, left) per image"""
        key = (int(resize), int(crop))
        g = self._geom.get(key)
        if g is None:
            g = np.empty((len(self), 6), np.int32)
            for b, (h, w) in enumerate(self.sizes):
                g[b, :2] = (h, w)
                g[b, 2:] = eval_geometry(h, w, resize, crop)
            self._geom[key] = g
        return g


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
    transform(packed, lo, hi) -> device uint8 [hi - lo, 3, crop, crop] of images [lo, hi) of the packed batch."""

    def __init__(self, resize: int = 256, crop: int = 224, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        self.resize, self.crop = int(resize), int(crop)
        if self.crop <= 32:
            raise ValueError(f"crop {self.crop} <= 32: input sizes without a resize (CIFAR) are not supported")
        if self.crop > self.resize:
            raise ValueError(f"crop {self.crop} > resize {self.resize}: torchvision would pad")
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self._ws = {}
        self._tables = {}

    @classmethod
    def for_input_size(cls, n: int, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        """utils/data_utils.py build_transform: Resize(int(256 / 224 * n)) -> CenterCrop(n) (384 -> 438 / 384)"""
        if n <= 32:
            raise ValueError(f"input size {n} <= 32: the reference does not resize there (out of scope)")
        return cls(int((256 / 224) * n), n, mean, std)

    @property
    def default_normalisation(self) -> bool:
        return self.mean == tuple(IMAGENET_MEAN) and self.std == tuple(IMAGENET_STD)

    def __repr__(self):
        return f"EvalTransform(resize={self.resize}, crop={self.crop}, mean={self.mean}, std={self.std})"

    def _workspace(self, device, nbytes):
        ws = self._ws.get(device)
        if ws is None or ws.numel() < nbytes:
            ws = self._ws[device] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        return ws

    def __call__(self, packed: PackedImages, lo: int = 0, hi: int | None = None, device="cuda", out: torch.Tensor | None = None):
        hi = len(packed) if hi is None else hi
        if not 0 <= lo <= hi <= len(packed):
            raise IndexError(f"shard [{lo}, {hi}) of a batch of {len(packed)}")
        n, c = hi - lo, self.crop
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if out is None:
            out = torch.empty(n, 3, c, c, dtype=torch.uint8, device=device)
        elif out.shape != (n, 3, c, c) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != device:
            raise ValueError(f"out must be a contiguous uint8 [{n}, 3, {c}, {c}] tensor on {device}")
        if n == 0:
            return out
        geom = np.ascontiguousarray(packed.geometry(self.resize, c)[lo:hi])
        plan = (C.c_int32 * 3)()
        nbytes = C.c_int64()
        L = _lib.lib()
        rc = L.ivit_resize_crop_workspace(geom.ctypes.data_as(C.c_void_p), n, c, plan, C.byref(nbytes))
        if rc != 0:
            raise _lib.IvitError(f"ivit_resize_crop_workspace failed ({rc}): {L.ivit_last_error_string().decode()}")
        start = int(packed.offsets[lo])
        end = int(packed.offsets[hi]) if hi < len(packed) else packed.data.numel()
        src = packed.data[start:end].to(device, non_blocking=True)
        offs = torch.from_numpy(packed.offsets[lo:hi] - start).to(device)
        g = torch.from_numpy(geom).to(device)
        ws = self._workspace(device, nbytes.value)
        with torch.cuda.device(device):
            _lib.call("ivit_resize_crop_bicubic_u8", _lib.ptr(src), _lib.ptr(offs), _lib.ptr(g), n, c, plan[0], plan[1], plan[2],
                      _lib.ptr(ws), ws.numel(), _lib.ptr(out), _lib.stream_ptr())
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
