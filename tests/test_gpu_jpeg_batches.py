"""GPU: the device JPEG decoder's parallel orchestration (sync_kernel's neighbour rounds, fix_kernel's continuation across
256-lane workgroups, the two segmented scans' carries, find_image / find_seg, the workspace layout, errors[]) on the batches of
tests/jpeg_batches.py.  Every comparison is of bytes, against ivit_jpeg_decode_host; tests/test_jpeg_batches_cpu.py holds that
function to Pillow on the same files and asserts what each batch reaches.  Neither Pillow nor the restatement's state stepping is
needed here (place() only counts de-stuffed bytes)."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
from ivit_amd.transforms import decode_images  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_batches as jb  # noqa: E402

DEV = "cuda:0"
GAP = 64                       # bytes of 0xA5 before, between and after the images of a gapped output
GUARD = 4096                   # bytes of 0xA5 on both sides of the workspace
CANARY = 0x5AA55AA5


def _unpack(packed):
    data = packed.data.cpu().numpy()
    return [data[o:o + h * w * 3].reshape(h, w, 3) for o, (h, w) in zip(packed.offsets, packed.sizes)]


def _assert_equal_host(pixels, files, what=""):
    assert len(pixels) == len(files)
    for b, (px, f) in enumerate(zip(pixels, files)):
        want = jb.host_pixels(f)
        assert px.shape == want.shape and np.array_equal(px, want), (what, b, f["name"])


def test_many_small_images_one_batch():
    fb = jb.FALLBACKS
    files = [fb[0]] + jb.RANDOM[:62] + fb + jb.RANDOM[62:] + jb.THIN + [fb[1]]
    assert len(files) > 128 and [b for b, f in enumerate(files) if not f["supported"]] == [0, 63, 64, 65, len(files) - 1]
    enc = jb.encode(files)
    assert sorted(enc.fallback) == [0, 63, 64, 65, len(files) - 1]
    pixels = _unpack(decode_images(enc, device=DEV))
    _assert_equal_host(pixels, files)
    for px, f in zip(pixels, files):
        if f["supported"]:
            assert hashlib.sha256(np.ascontiguousarray(px).tobytes()).digest() == f["sha"], f["name"]
    # shards [lo, hi): offsets relative to lo, the same pixels
    for lo, hi in ((60, 70), (64, 65), (1, 129), (120, 140), (127, len(files)), (63, 66)):
        _assert_equal_host(_unpack(decode_images(enc, lo, hi, DEV)), files[lo:hi], (lo, hi))


@pytest.mark.parametrize("name", list(jb.PLACEMENTS))
def test_boundary_placements(name):
    batch, b, local = jb.placed(name)
    assert max(len(f["data"]) for f in batch) <= 300_000
    enc = jb.encode(batch)
    rows, _, _, _, _ = jb.index_rows(enc)
    assert (int(rows["sub_first"][b]) + local) % jb.LANES == 0 and rows["sub_first"][b] + local > 0
    _assert_equal_host(_unpack(decode_images(enc, device=DEV)), batch, name)


# --------------------------------------------------------------------------------------------------------- through the C ABI
class _Abi:
    """one batch laid out for ivit_jpeg_decode_u8: the plan and index on the device, a gapped output, errors between canaries"""

    def __init__(self, files):
        self.files = files
        enc = jb.encode(files)
        n = len(files)
        self.px = (enc.sizes[:, 0].astype(np.int64) * enc.sizes[:, 1] * 3)
        self.offs = GAP + np.concatenate([[0], np.cumsum(self.px + GAP)[:-1]]).astype(np.int64)
        self.total = int(self.offs[-1] + self.px[-1] + GAP)
        rows, self.sizes4, plan, _, _ = jb.index_rows(enc, out_offsets=self.offs)
        assert list(rows["out"]) == list(self.offs)
        self.plan_d = plan.to(DEV)
        self.index_d = torch.from_numpy(rows.view(np.uint8).copy()).to(DEV)
        self.n = n

    def decode(self, ws):
        """one call on a workspace of exactly sizes4[0] bytes -> (pixels per image, None for an image the call leaves alone or
        flags; errors)"""
        assert ws.numel() == self.sizes4[0] and ws.data_ptr() % 256 == 0
        out = torch.full((self.total,), 0xA5, dtype=torch.uint8, device=DEV)
        err = torch.full((self.n + 2,), CANARY, dtype=torch.int32, device=DEV)
        _lib.call("ivit_jpeg_decode_u8", _lib.ptr(self.plan_d), _lib.ptr(self.index_d), self.n, self.sizes4[1], self.sizes4[2],
                  self.sizes4[3], _lib.ptr(ws), ws.numel(), _lib.ptr(out), _lib.ptr(err[1:]), _lib.stream_ptr())
        torch.cuda.synchronize()
        err = err.cpu().numpy()
        assert err[0] == CANARY and err[-1] == CANARY
        out = out.cpu().numpy()
        gaps = np.ones(self.total, bool)
        pixels = []
        for f, o, p in zip(self.files, self.offs, self.px):
            if f["supported"]:
                gaps[o:o + p] = False
                pixels.append(out[o:o + p].reshape(f["h"], f["w"], 3))
            else:
                pixels.append(None)               # not decoded on the device: its bytes stay as they were
        assert (out[gaps] == 0xA5).all(), "a store outside the images"
        return pixels, err[1:-1]


def _guarded(nbytes, fill):
    """a workspace of exactly nbytes, filled with `fill`, inside a larger tensor with GUARD bytes of 0xA5 on both sides"""
    big = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = big[GUARD:GUARD + nbytes]
    ws.fill_(fill)
    return big, ws


def _guards_intact(big, nbytes):
    host = big.cpu().numpy()
    return (host[:GUARD] == 0xA5).all() and (host[GUARD + nbytes:] == 0xA5).all()


def _mixed_batch():
    old = jb.OLD
    return (jb.THIN[:4] + [jb.BY_NAME["blocks37_opt"]] + jb.RANDOM[:5] + [old["37x53_progressive"], old["37x53_420_rst1"]]
            + jb.RANDOM[5:9] + [jb.BY_NAME["noise_q100"]] + jb.THIN[4:] + [old["37x53_gray_rst1"]])


def test_exact_workspace_gapped_output_and_stale_contents():
    files = _mixed_batch()
    assert 18 <= len(files) <= 24
    a = _Abi(files)
    nbytes = a.sizes4[0]
    runs = []
    for fill in (0x00, 0xFF):
        big, ws = _guarded(nbytes, fill)
        runs.append(a.decode(ws))
        assert _guards_intact(big, nbytes), fill
    # straight after a larger, different batch has used the same workspace
    other = _Abi([jb.BY_NAME["rows_mid"], jb.BY_NAME["two_long"]] + jb.RANDOM[20:50])
    assert other.sizes4[0] > nbytes and other.sizes4[1] > a.sizes4[1]
    big, ws_other = _guarded(other.sizes4[0], 0x3C)
    pixels, err = other.decode(ws_other)
    assert not err.any() and _guards_intact(big, other.sizes4[0])
    _assert_equal_host(pixels, other.files, "the larger batch")
    big[GUARD + nbytes:].fill_(0xA5)
    runs.append(a.decode(big[GUARD:GUARD + nbytes]))
    assert _guards_intact(big, nbytes)
    for k, (pixels, err) in enumerate(runs):
        assert not err.any(), k
        for b, (px, f) in enumerate(zip(pixels, files)):
            if f["supported"]:
                assert np.array_equal(px, jb.host_pixels(f)), (k, b, f["name"])
                assert np.array_equal(px, runs[0][0][b]), (k, b, f["name"])


def test_corrupt_entropy_is_flagged_per_image():
    """The corrupt set interleaved with good files, one call.  The files pass the probe, so the marker structure, the tables and
    the geometry are sound; only the entropy bits are arbitrary, which is what every lane of sync_kernel already decodes when it
    starts from a guessed state.  The bound of every store that depends on those bits (write_kernel, run_sub):
      - coefficient stores C0[slot * 64 + pos]: the loop runs only while slot < limit, limit = (first_mcu + nmcu) * bpm <= the
        image's blocks, and slot starts at base[g] >= first_mcu * bpm (block counts are >= 0); a segment that decodes more blocks
        than its MCUs hold stores nothing past them;
      - pos = kNatural[z] with z <= 63 + 15 = 78 in the 80-entry natural order (a run past 63 lands on 63), so pos is 0..63;
      - peek32 reads byte + i only where byte + i < the segment's bytes and takes 0 beyond, and a codeword starts only at
        p < end <= 8 * bytes; every codeword advances p by at least one bit, so run_sub ends;
      - run_sub (sync_kernel, fix_kernel) stores only st_in / st_out / cnt of its own subsequence g < nsub.
    errors[b] is nonzero exactly where the host decoder refuses the file; all other images, the corrupt but decodable ones
    included, are the host decoder's bytes."""
    cs = jb.corrupt_set()
    good = jb.RANDOM[100:100 + len(cs)] + [jb.BY_NAME["blocks37_opt"]]
    files = []
    for k, f in enumerate(cs):
        files += [good[k], f]
    files.append(good[-1])
    refused = [b for b, f in enumerate(files) if f.get("refused")]
    assert len(refused) >= 6 and sum(1 for f in files if f.get("refused") is False) >= 6
    a = _Abi(files)
    big, ws = _guarded(a.sizes4[0], 0xFF)
    pixels, err = a.decode(ws)
    assert _guards_intact(big, a.sizes4[0])
    assert [int(b) for b in np.nonzero(err)[0]] == refused
    for b, (px, f) in enumerate(zip(pixels, files)):
        if b not in refused:
            assert np.array_equal(px, jb.host_pixels(f)), (b, f["name"])
    with pytest.raises(_lib.IvitError) as e:
        decode_images(jb.encode(files), device=DEV)
    assert str(refused) in str(e.value)
