"""CPU: what the device JPEG decoder's batch tests (tests/test_gpu_jpeg_batches.py) feed it, asserted here.  The fixture
tests/golden/jpeg_batches_pil.npz against the installed Pillow and the host decoder; the restatement of sync_kernel / fix_kernel
(tests/jpeg_sync_ref.py) against the library's own plan; the structure of the structured files; that noise at quality 100 needs
several neighbour rounds; that every placement batch puts a 256-lane workgroup boundary where its name says, and that the serial
continuation has work to do there; the split of the corrupt set."""
import hashlib
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_batches as jb  # noqa: E402
import jpeg_sync_ref as ref  # noqa: E402
from ivit_amd.transforms import probe_jpeg  # noqa: E402

STRUCTURED = ("rows_mid", "two_long", "noise_q100", "blocks37_opt")


# ---------------------------------------------------------------------------------------------------------------------- fixture
def test_fixture_reproduces_with_installed_pillow():
    Image = pytest.importorskip("PIL.Image")
    for f in jb.FILES:
        px = np.asarray(Image.open(io.BytesIO(f["data"])).convert("RGB"))
        assert px.shape == (f["h"], f["w"], 3), f["name"]
        assert hashlib.sha256(px.tobytes()).digest() == f["sha"], f["name"]
    # the generator gives the same files again
    sys.path.insert(0, os.path.join(jb.ROOT, "scripts"))
    import make_jpeg_golden as gen
    z, stored = gen.build_batches(), np.load(jb.GOLDEN)
    assert sorted(stored.files) == sorted(z) == ["data", "data_off", "names", "sha256", "sizes"]
    for key in z:
        assert np.array_equal(z[key], stored[key]), key


def test_fixture_size_and_contents():
    assert os.path.getsize(jb.GOLDEN) < 1 << 20
    assert len(jb.RANDOM) >= 130
    assert max(len(f["data"]) for f in jb.FILES) <= 300_000
    want = {"thin_130x2_420": (130, 2, 3), "thin_2x130_420": (2, 130, 3), "thin_3x200_422": (3, 200, 2), "thin_200x3_422": (200, 3, 2),
            "thin_1x64_444": (1, 64, 1), "thin_64x1_444": (64, 1, 1), "thin_17x1_gray": (17, 1, 0)}
    assert {f["name"] for f in jb.THIN} == set(want)
    for name, (h, w, sampling) in want.items():
        ok, reason, info = probe_jpeg(jb.BY_NAME[name]["data"])
        assert ok and info == (h, w, 1 if sampling == 0 else 3, sampling), (name, reason, info)


def test_host_decoder_hashes_to_the_fixture():
    for f in jb.FILES:
        ok, reason, info = probe_jpeg(f["data"])
        assert ok and info[:2] == (f["h"], f["w"]), (f["name"], reason)
        assert hashlib.sha256(jb.host_pixels(f).tobytes()).digest() == f["sha"], f["name"]


# ------------------------------------------------------------------------------------------------ restatement against the library
def test_segments_equal_the_library_plan():
    enc = jb.encode(jb.FILES, pin=False)
    rows, sizes4, _, _, _ = jb.index_rows(enc)
    total = 0
    for f, row in zip(jb.FILES, rows):
        lens = ref.segments(f["data"])
        subs = [max(-(-8 * n // ref.SUB_BITS), 1) for n in lens]
        assert subs == jb.nsub(f)
        assert sum(subs) == row["nsub"], f["name"]                    # the last int32 of the 40-byte row
        assert row["sub_first"] == total, f["name"]
        total += sum(subs)
    assert total == sizes4[1]


def test_restatement_decodes_the_frame_s_blocks():
    names = ("rows_mid", "noise_q100", "blocks37_opt", "thin_130x2_420", "thin_200x3_422", "thin_17x1_gray", "random_000", "random_001",
             "random_002", "random_003")
    for name in names:
        f = jb.BY_NAME[name]
        F = ref.parse(f["data"])
        assert (F.h, F.w) == (f["h"], f["w"])
        per = ref.decoded_blocks(f["data"])
        assert sum(want for _, want, _ in per) == F.nmcu * F.bpm, name      # the frame geometry's blocks
        for count, want, left in per:
            assert count == want and 0 <= left < 8, (name, count, want, left)
    # the library counts the same blocks: the next image's first block slot
    files = [jb.BY_NAME[n] for n in names]
    rows, sizes4, _, _, _ = jb.index_rows(jb.encode(files, pin=False))
    blocks = [sum(c for c, _, _ in ref.decoded_blocks(f["data"])) for f in files]
    assert list(rows["coef"]) == list(np.cumsum([0] + blocks[:-1])) and sizes4[2] == sum(blocks)


def test_restatement_states_are_consistent():
    """after the continuation every recorded entry state is the true one, at any alignment; without it they are not"""
    f = jb.BY_NAME["blocks37_opt"]
    for g0 in (0, 255, 250):
        s = ref.sync_states(f["data"], g0)
        assert s.final_in == s.true_in
        for j in range(len(s.true_in) - 1):
            if s.seg_of[j + 1] == s.seg_of[j]:
                assert s.final_out[j] == s.true_in[j + 1]


# -------------------------------------------------------------------------------------------------------------------- structure
def test_structured_files_have_the_structure():
    rows, two, noise, b37 = (jb.nsub(jb.BY_NAME[n]) for n in STRUCTURED)
    assert len(rows) >= 4 and all(8 <= n <= 40 for n in rows) and sum(rows) >= 150
    assert len(two) >= 2 and max(two) > ref.LANES
    assert len(noise) == 1 and 100 <= noise[0] <= 300
    F = ref.parse(jb.BY_NAME["blocks37_opt"]["data"])
    assert F.restart == 37 and ref.LANES % 37 and (F.ncomp, F.bpm) == (3, 4)     # 4:2:2
    assert {2, 3} <= set(b37) and len(b37) > 4
    assert b"\xff\xc4" in jb.BY_NAME["blocks37_opt"]["data"]
    for name in STRUCTURED:
        assert len(jb.BY_NAME[name]["data"]) <= 300_000


def test_noise_needs_several_neighbour_rounds():
    s = ref.sync_states(jb.BY_NAME["noise_q100"]["data"], 0)
    assert s.final_in == s.true_in
    worst = max(s.rounds)
    print("noise_q100: neighbour rounds per lane, maximum", worst, "; lanes with more than one:", sum(r > 1 for r in s.rounds), "of",
          len(s.rounds))
    assert worst > 1


# ------------------------------------------------------------------------------------------------------------------- placements
def _target_states(name):
    batch, b, local = jb.placed(name)
    rows, _, _, _, _ = jb.index_rows(jb.encode(batch, pin=False))
    g0 = int(rows["sub_first"][b])
    return batch, b, local, rows, ref.sync_states(batch[b]["data"], g0)


@pytest.mark.parametrize("name", list(jb.PLACEMENTS))
def test_placement_puts_a_boundary_on_the_spot(name):
    batch, b, local, rows, s = _target_states(name)
    f = batch[b]
    subs = jb.nsub(f)
    first = [sum(subs[:i]) for i in range(len(subs))]
    assert (int(rows["sub_first"][b]) + local) % ref.LANES == 0 and rows["sub_first"][b] + local > 0
    assert rows["nsub"][b] == sum(subs) and max(len(x["data"]) for x in batch) <= 300_000
    assert s.final_in == s.true_in
    seg = s.seg_of[local]
    hit = dict(s.boundaries)
    if name == "a_image_start":
        assert b > 0 and local == 0
        assert not hit or min(hit) >= ref.LANES       # the image's own first subsequence is no boundary of fix_kernel's
    elif name == "b_segment_start":
        assert f["name"] == "rows_mid" and seg > 0 and local == first[seg] and hit[local] == "first"
    elif name == "c_segment_second":
        assert f["name"] == "rows_mid" and seg > 0 and local == first[seg] + 1
        assert s.after_sync_in[local] != s.true_in[local] and hit[local] >= 1
        print(name, "continuation re-decodes", hit[local], "subsequence(s)")
    elif name == "d_segment_last":
        assert f["name"] == "rows_mid" and seg < len(subs) - 1 and local == first[seg] + subs[seg] - 1 and subs[seg] > 1
        assert hit[local] != "first"
    elif name.startswith("e_image_last"):
        assert local == sum(subs) - 1 and b + 1 < len(batch)
        assert batch[b + 1]["supported"] == (name == "e_image_last_then_device")
        assert rows["sec"][b + 1] >= 0 if batch[b + 1]["supported"] else rows["sec"][b + 1] == -1
        assert rows["sub_first"][b + 1] == rows["sub_first"][b] + rows["nsub"][b]
        if not batch[b + 1]["supported"]:              # the tie find_image has to break: the fallback and the next device image
            assert rows["nsub"][b + 1] == 0 and rows["sub_first"][b + 2] == rows["sub_first"][b + 1]
    elif name == "f_two_in_long_segment":
        assert f["name"] == "two_long" and b >= 64 and subs[seg] > ref.LANES
        inside = [x for x in (local, local + ref.LANES) if first[seg] < x < first[seg] + subs[seg]]
        assert len(inside) == 2
        for x in inside:
            assert s.after_sync_in[x] != s.true_in[x] and hit[x] >= 1
        print(name, "continuation re-decodes", [hit[x] for x in inside], "subsequence(s)")
    elif name == "g_inside_noise":
        assert f["name"] == "noise_q100" and 0 < local < subs[0] - 1 and hit[local] != "first"
        print(name, "continuation re-decodes", hit[local], "subsequence(s); neighbour rounds, maximum", max(s.rounds))
    # without the continuation the states after a boundary inside a segment are not the true ones
    if any(v != "first" and v >= 1 for v in hit.values()):
        assert ref.sync_states(f["data"], int(rows["sub_first"][b]), continuation=False).final_in != s.true_in


# ------------------------------------------------------------------------------------------------------------------- corrupt set
def test_corrupt_set_split():
    cs = jb.corrupt_set()
    refused = [f for f in cs if f["refused"]]
    differ = [f for f in cs if not f["refused"] and not np.array_equal(f["pixels"], jb.host_pixels(f["source"]))]
    print("corrupt set:", len(cs), "accepted by the probe,", len(refused), "refused by the host decoder,", len(differ),
          "decoded to other pixels")
    assert {f["source"]["name"] for f in cs} == set(jb.CORRUPT_SOURCES)
    assert len(refused) >= 6 and len(differ) >= 6
    for f in cs:
        if not f["refused"]:
            assert f["pixels"].shape == (f["h"], f["w"], 3)
