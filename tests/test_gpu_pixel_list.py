"""Pixel-list renders (rt_render_pixels / rt_render_pixels_device): spp samples of an arbitrary list of pixels of the frame.
Sample s of listed pixel g is the sample a dense render gives pixel g, so entry k of the compact output equals the dense
Oracle-B sums at pixels[k] -- bit for bit, on the small-grid kernel (the book scene) and on the general one (10 001 spheres),
with direct adds (1, 4 spp) and block sums (8 ... 100 spp; blocks that straddle list entries)."""
import numpy as np
import pytest
import torch

import rtiow_amd as rt

pytestmark = pytest.mark.gpu

SPPS = (1, 4, 8, 24, 40, 100)


def _lists(w, h, rng):
    npix = w * h
    ident = np.arange(npix, dtype=np.uint32)
    sub = rng.choice(npix, size=max(npix // 100, 8), replace=False).astype(np.uint32)
    sub = np.concatenate([sub, sub[:7], sub[3:5]])                        # duplicates
    rng.shuffle(sub)
    jj, ii = np.mgrid[h // 4:h // 4 + 13, w // 3:w // 3 + 21]
    rect = (jj * w + ii).astype(np.uint32).reshape(-1)
    corners = np.array([0, w - 1, (h - 1) * w, npix - 1], dtype=np.uint32)
    out = {"identity": ident, "random 1 % shuffled with duplicates": sub, "rectangle": rect, "one pixel": np.array([npix // 2 + 5], dtype=np.uint32),
           "corners": corners}
    perm = rng.permutation(npix).astype(np.uint32)
    for n in (1, 63, 64, 65, 257):
        out[f"n_pixels {n}"] = perm[1000:1000 + n].copy()
    return out


def _oracle_cumulative(oracle_mod, cam, flat, w, h, seed):
    """Oracle-B sums of samples [0, spp) for every spp of SPPS, from additive passes (one oracle render of 100 samples in all)."""
    ocam = oracle_mod.camera_from_host(cam)
    want, acc, lo = {}, np.zeros((h, w, 3), dtype=np.uint64), 0
    for spp in SPPS:
        f, _, _ = oracle_mod.render_b(ocam, flat, oracle_mod.make_params(w, h, spp - lo, sample_begin=lo, seed=seed))
        acc = acc + f
        want[spp], lo = acc.copy(), spp
    return want


def _check_scene(renderer, oracle_mod, flat, w, h, seed, want_variant_bit0):
    renderer.upload_scene(flat)
    cam = rt.book1_camera(w, h)
    want = _oracle_cumulative(oracle_mod, cam, flat, w, h, seed)
    lists = _lists(w, h, np.random.default_rng(11))
    for spp in SPPS:
        dense = want[spp].reshape(-1, 3)
        for name, px in lists.items():
            got, st = renderer.render_pixels(cam, rt.make_params(w, h, spp, seed=seed), px)
            assert np.array_equal(got, dense[px]), (spp, name)
            assert st["samples"] == len(px) * spp, (spp, name)
            assert st["kernel_variant"] & 8 and (st["kernel_variant"] & 1) == want_variant_bit0 and st["scan_mode"] == 5
            if spp < 5:
                assert st["direct_samples"] == len(px) * spp
        _, fix, _ = renderer.render(cam, rt.make_params(w, h, spp, seed=seed))                       # the identity list = rt_render's fix
        assert np.array_equal(fix, want[spp])
    return cam, want, lists


def test_pixel_lists_equal_the_oracle_on_the_book_scene(renderer, oracle_mod, book1_flat):
    _check_scene(renderer, oracle_mod, book1_flat, 160, 90, 3, 1)


def test_pixel_lists_equal_the_oracle_on_the_general_kernel(renderer, oracle_mod):
    flat = rt.random_scene(1, grid=(-50, 49)).flatten()
    assert len(flat) == 10001
    _check_scene(renderer, oracle_mod, flat, 192, 108, 2, 0)


def test_sample_begin_and_two_accumulating_passes_on_two_streams(renderer, oracle_mod, book1_flat):
    w, h, seed = 120, 67, 9
    renderer.upload_scene(book1_flat)
    cam = rt.book1_camera(w, h)
    ocam = oracle_mod.camera_from_host(cam)
    rng = np.random.default_rng(5)
    px = np.sort(rng.choice(w * h, size=900, replace=False)).astype(np.uint32)
    for spp, begin in ((24, 40), (3, 7), (100, 1000)):
        want, _, _ = oracle_mod.render_b(ocam, book1_flat, oracle_mod.make_params(w, h, spp, sample_begin=begin, seed=seed))
        got, st = renderer.render_pixels(cam, rt.make_params(w, h, spp, sample_begin=begin, seed=seed), px)
        assert np.array_equal(got, want.reshape(-1, 3)[px]) and st["samples"] == len(px) * spp
    # passes [0, 30) and [30, 41) of the same list, accumulated into one zeroed buffer from two streams
    want, _, _ = oracle_mod.render_b(ocam, book1_flat, oracle_mod.make_params(w, h, 41, seed=seed))
    d_px = torch.from_numpy(px.view(np.int32).copy()).cuda()
    d_fix = torch.zeros((len(px), 3), dtype=torch.int64, device="cuda")
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for k, (spp, begin) in enumerate(((30, 0), (11, 30))):
        p = rt.make_params(w, h, spp, sample_begin=begin, seed=seed, flags=rt.RT_FLAG_ACCUMULATE | rt.RT_FLAG_OVERLAPPED)
        renderer.render_pixels_device(cam, p, d_px.data_ptr(), len(px), d_fix.data_ptr(), streams[k].cuda_stream)
    torch.cuda.synchronize()
    assert renderer.last_stats()["samples"] == len(px) * 11
    assert np.array_equal(d_fix.cpu().numpy().view(np.uint64), want.reshape(-1, 3)[px])


def test_a_rejected_call_touches_nothing_and_an_empty_list_does_nothing(renderer, book1_flat):
    w, h = 64, 36
    renderer.upload_scene(book1_flat)
    cam = rt.book1_camera(w, h)
    px = np.arange(50, dtype=np.uint32)
    _, st0 = renderer.render_pixels(cam, rt.make_params(w, h, 6), px)
    before = renderer.last_stats()
    d_px = torch.from_numpy(px.view(np.int32).copy()).cuda()
    d_fix = torch.full((50, 3), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for kw in (dict(flags=rt.RT_FLAG_UNIFORM53), dict(flags=rt.RT_FLAG_DIAG_STATS), dict(flags=rt.RT_FLAG_NO_FILTER), dict(shard_count=2),
               dict(flags=0x20)):
        with pytest.raises(rt.RtiowHipError):
            renderer.render_pixels_device(cam, rt.make_params(w, h, 6, **kw), d_px.data_ptr(), 50, d_fix.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream)
    with pytest.raises(rt.RtiowHipError):                                                           # host form: a number outside the frame
        renderer.render_pixels(cam, rt.make_params(w, h, 6), np.array([w * h], dtype=np.uint32))
    renderer.render_pixels_device(cam, rt.make_params(w, h, 6), d_px.data_ptr(), 0, d_fix.data_ptr(), torch.cuda.current_stream().cuda_stream)
    got, st = renderer.render_pixels(cam, rt.make_params(w, h, 6), np.zeros(0, dtype=np.uint32))
    assert got.shape == (0, 3) and st is None
    torch.cuda.synchronize()
    assert (d_fix.cpu().numpy() == 0x5A5A5A5A).all()
    after = renderer.last_stats()
    assert after == before and after["samples"] == 50 * 6 == st0["samples"]
