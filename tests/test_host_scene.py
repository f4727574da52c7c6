"""Host mirror of the reference's scene interface (rtiow_amd.scene) and of the
row sharding, checked against the oracle's own restatements and the fixtures."""
import os

import numpy as np
import pytest

import rtiow_amd as rt
from rtiow_amd.distributed import shard_row_map
from conftest import GOLDEN


def test_random_scene_matches_committed_fixture(book1_flat):
    flat = rt.random_scene(1).flatten()
    assert flat.tobytes() == book1_flat.tobytes()


def test_random_scene_structure():                  # main.rs:59-102
    world = rt.random_scene(1)
    flat = world.flatten()
    assert len(flat) <= 1 + 23 * 23 + 3 and len(flat) >= 520
    g = flat[0]
    assert g["center"].tolist() == [0, -1000, 0] and g["radius"] == 1000 and g["kind"] == 0
    assert flat[-3]["kind"] == 2 and flat[-3]["param"] == 1.5 and flat[-3]["center"].tolist() == [0, 1, 0]
    assert flat[-2]["kind"] == 0 and flat[-2]["albedo"].tolist() == [0.4, 0.2, 0.1]
    assert flat[-1]["kind"] == 1 and flat[-1]["param"] == 0.0 and flat[-1]["center"].tolist() == [4, 1, 0]
    small = flat[1:-3]
    assert (small["radius"] == 0.2).all() and (small["center"][:, 1] == 0.2).all()
    d = small["center"] - np.array([4, 0.2, 0])
    assert (np.sqrt((d * d).sum(1)) > 0.9).all()    # main.rs:72
    mix = np.bincount(small["kind"], minlength=3) / len(small)
    assert 0.72 < mix[0] < 0.88 and 0.08 < mix[1] < 0.22 and 0.01 < mix[2] < 0.10
    metal = small[small["kind"] == 1]
    assert (metal["albedo"] >= 0.5).all() and (metal["albedo"] < 1.0).all()
    assert (metal["param"] >= 0.0).all() and (metal["param"] < 0.5).all()
    assert (small[small["kind"] == 2]["param"] == 1.5).all()


def test_other_seeds_give_other_scenes():
    assert rt.random_scene(1).flatten().tobytes() != rt.random_scene(2).flatten().tobytes()


def test_tenk_scene_matches_fixture_head():
    fx = np.load(os.path.join(GOLDEN, "tenk_scene_seed1_head.npz"), allow_pickle=False)
    flat = rt.random_scene(1, grid=(-50, 49)).flatten()
    assert len(flat) == int(fx["count"]) and len(flat) > 9900
    assert flat[:8].tobytes() == fx["head"].tobytes() and flat[-8:].tobytes() == fx["tail"].tobytes()


@pytest.mark.parametrize("wh", [(400, 225), (1200, 800), (3840, 2160)])
def test_camera_new_equals_oracle_restatement(oracle_mod, wh):   # camera.rs:17-45
    w, h = wh
    host = rt.book1_camera(w, h)
    orc = oracle_mod.book1_camera(w, h)
    for name in ("origin", "lower_left_corner", "horizontal", "vertical", "u", "v"):
        assert list(getattr(orc, name)) == [float(x) for x in getattr(host, name)], name
    assert orc.lens_radius == host.lens_radius == 0.05
    c = host.to_rt_camera()
    assert list(c.horizontal) == list(orc.horizontal)


def test_hittable_list_keeps_push_order():
    w = rt.HittableList()
    w.push(rt.Sphere(rt.Point3(1, 2, 3), 0.5, rt.Metal(rt.Color(0.1, 0.2, 0.3), 0.25)))
    w.push(rt.Sphere(rt.Point3(4, 5, 6), 1.5, rt.Dialectric(1.5)))
    f = w.flatten()
    assert f["center"].tolist() == [[1, 2, 3], [4, 5, 6]] and f["kind"].tolist() == [1, 2]
    assert f["param"].tolist() == [0.25, 1.5] and f.dtype.itemsize == 72


@pytest.mark.parametrize("height,tile,count", [(675, 8, 8), (225, 8, 3), (18, 4, 2), (7, 3, 4), (5, 8, 2), (2160, 16, 8)])
def test_shard_rows_partition_the_image(height, tile, count):
    seen = []
    for k in range(count):
        rows = shard_row_map(height, tile, k, count)
        p = rt.make_params(64, height, 1, tile_rows=tile, shard_index=k, shard_count=count)
        assert rt.shard_rows(p) == len(rows)                        # C ABI (no GPU needed) agrees
        assert rt.shard_row_indices(p).tolist() == rows.tolist()
        assert (np.diff(rows) > 0).all() if len(rows) > 1 else True
        seen.extend(rows.tolist())
    assert sorted(seen) == list(range(height))


def test_ppm_roundtrip(tmp_path):
    rgba = (np.arange(5 * 7 * 4) % 251).astype(np.uint8).reshape(5, 7, 4)
    path = tmp_path / "x.ppm"
    rt.write_ppm(str(path), rgba)
    assert np.array_equal(rt.read_ppm(str(path)), rgba[:, :, :3])


def test_png_is_the_references_image_png(tmp_path):
    """main.rs:147,177: the reference saves an 8-bit RGBA PNG, rows top first.  write_png() writes that colour type, bit depth and pixel
    order; read_png() gets the pixels back, and so does an independent decoder (PIL, when the image has it)."""
    import struct
    rng = np.random.default_rng(3)
    rgba = rng.integers(0, 256, (41, 67, 4), dtype=np.uint8)
    rgba[:, :, 3] = 255
    path = str(tmp_path / "image.png")
    rt.write_png(path, rgba)
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[12:16] == b"IHDR"
    w, h, depth, ctype, comp, flt, lace = struct.unpack(">IIBBBBB", data[16:29])
    assert (w, h, depth, ctype, comp, flt, lace) == (67, 41, 8, 6, 0, 0, 0)          # RGBA8, non-interlaced
    assert np.array_equal(rt.read_png(path), rgba)
    try:
        from PIL import Image
    except ImportError:
        return
    assert np.array_equal(np.array(Image.open(path)), rgba)


def test_read_png_decodes_every_row_filter(tmp_path):
    """read_png() against files whose rows use the filters an encoder may choose (Sub, Up, Average, Paeth): built here by filtering
    by hand, so the decoder is checked on all five types without a third-party encoder."""
    import struct, zlib
    rng = np.random.default_rng(4)
    h, w, c = 9, 13, 4
    img = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    flat = img.reshape(h, w * c).astype(np.int32)
    raw = bytearray()
    for y in range(h):
        ft = y % 5
        prev = flat[y - 1] if y else np.zeros(w * c, dtype=np.int32)
        line = []
        for i in range(w * c):
            a = int(flat[y, i - c]) if i >= c else 0
            b = int(prev[i])
            cc = int(prev[i - c]) if i >= c else 0
            pa, pb, pc = abs(b - cc), abs(a - cc), abs(a + b - 2 * cc)
            pred = [0, a, b, (a + b) >> 1, a if (pa <= pb and pa <= pc) else (b if pb <= pc else cc)][ft]
            line.append((int(flat[y, i]) - pred) & 255)
        raw += bytes([ft]) + bytes(line)
    chunk = lambda t, d: struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)
    path = str(tmp_path / "f.png")
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(bytes(raw))) + chunk(b"IEND", b""))
    assert np.array_equal(rt.read_png(path), img)


def test_read_png_on_the_references_own_render():
    """The one image the reference ships (rtiow_part1_final.png, written by the `image` crate's encoder): read_png() must give the sky rows
    the committed fixture holds (tests/golden/ref_png_sky_rows.json, extracted with PIL).  The input is that render's top rows,
    tests/golden/ref_png_head.png (tests/golden/make_ref_png_head.py): the encoder's own filtered scanlines, every filter type it
    used among them, re-deflated."""
    import json
    import struct
    import zlib
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    src = os.path.join(golden, "ref_png_head.png")
    data = open(src, "rb").read()
    rows, = struct.unpack(">I", data[20:24])                          # IHDR height
    stride = 1 + 1200 * 4
    raw = zlib.decompress(data[8 + 25 + 8:-12 - 4])                    # the one IDAT chunk's payload
    assert sorted(set(raw[y * stride] for y in range(rows))) == [1, 2, 3, 4]   # Sub, Up, Average, Paeth: all undone by read_png
    im = rt.read_png(src)
    fx = json.load(open(os.path.join(golden, "ref_png_sky_rows.json")))
    assert rows <= fx["height"] and im.shape == (rows, fx["width"], 4) and (im[:, :, 3] == 255).all()
    for y, rgb in fx["constant_rows"].items():
        assert (im[int(y), :, :3] == np.array(rgb, dtype=np.uint8)).all()
    for pt in fx["points"]:
        assert im[pt["y"], pt["x"], :3].tolist() == pt["rgb"]


def test_scene_file_roundtrip(tmp_path, book1_flat):
    path = str(tmp_path / "scene.bin")
    rt.save_scene(path, rt.random_scene(1))
    got = rt.load_scene(path)
    assert got.tobytes() == book1_flat.tobytes()
    with open(path, "ab") as f:
        f.write(b"\0" * 5)
    with pytest.raises(ValueError):
        rt.load_scene(path)


def test_checkpoint_roundtrip(tmp_path):
    fix = (np.arange(4 * 5 * 3, dtype=np.uint64) * np.uint64(1 << 33)).reshape(4, 5, 3)
    path = str(tmp_path / "ck.npz")
    rt.save_checkpoint(path, fix, 37, 0xDEADBEEF12345678)
    f2, spp, seed = rt.load_checkpoint(path)
    assert np.array_equal(f2, fix) and spp == 37 and seed == 0xDEADBEEF12345678
