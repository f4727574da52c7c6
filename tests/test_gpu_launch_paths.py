"""The three launch paths of the render kernel -- dense (rt_render_device), pixel list (rt_render_pixels_device) and frame batch
(rt_render_frames_device) -- share one plan, one parameter fill, one prologue and one tail (rt_launch.hpp).  Through the public API
only: the same frame through all three, launched back to back on one context and one stream, is the same bits (and Oracle B's), and
rt_last_stats reports per path what it always did -- the kernel variant, the scan mode (after a max_depth 0 call too: 0, 0 and 5),
the samples and the grid.  A rejected RT_FLAG_UNIFORM53 combination touches nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import rtiow_amd as rt
from rtiow_amd import _ffi

pytestmark = pytest.mark.gpu

W, H, SEED = 32, 18, 11


@pytest.fixture(scope="module")
def one_per_cu():
    """A context of its own, created under RTIOW_BLOCKS_PER_CU=1 (read by rt_create): the persistent grid is min(CUs, work blocks of 256)."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("RTIOW_BLOCKS_PER_CU", "1")
        r = rt.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def tenk_flat():
    flat = rt.random_scene(1, grid=(-50, 49)).flatten()
    assert len(flat) == 10001
    return flat


def _three_launches(r, cam, p, ask_stats):
    """Dense, then all pixels as a list, then two identical cameras as a batch: back to back on the current stream, nothing in between
    (ask_stats: rt_last_stats after each launch, which waits for that launch).  Returns the three results and the stats asked for."""
    w, h = p.width, p.height
    d_dense = torch.full((h, w, 3), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    d_list = torch.full((h * w, 3), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    d_batch = torch.full((2, h, w, 3), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    d_pixels = torch.arange(h * w, dtype=torch.int32, device="cuda")
    d_cams = torch.from_numpy(rt.cameras_to_array([cam, cam])).cuda()
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    stats = []
    r.render_device(cam, p, d_dense.data_ptr(), stream)
    if ask_stats: stats.append(r.last_stats())
    r.render_pixels_device(cam, p, d_pixels.data_ptr(), h * w, d_list.data_ptr(), stream)
    if ask_stats: stats.append(r.last_stats())
    r.render_frames_device(d_cams.data_ptr(), 2, 0, p, d_batch.data_ptr(), stream)
    if ask_stats: stats.append(r.last_stats())
    torch.cuda.synchronize()
    as_u64 = lambda t: t.cpu().numpy().view(np.uint64)
    return as_u64(d_dense), as_u64(d_list).reshape(h, w, 3), as_u64(d_batch), stats


def _check_paths(r, oracle_mod, flat, spp, variants, direct):
    r.upload_scene(flat)
    cam = rt.book1_camera(W, H)
    p = rt.make_params(W, H, spp, seed=SEED)
    want, _, ost = oracle_mod.render_b(oracle_mod.camera_from_host(cam), flat, oracle_mod.make_params(W, H, spp, seed=SEED))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for ask_stats in (False, True):
        dense, listed, batch, stats = _three_launches(r, cam, p, ask_stats)
        assert np.array_equal(dense, want), (spp, ask_stats)
        assert np.array_equal(listed, want), (spp, ask_stats)
        assert np.array_equal(batch[0], want) and np.array_equal(batch[1], want), (spp, ask_stats)
        if not ask_stats:
            stats = [None, None, r.last_stats()]                           # (the latest launch: the batch)
        for st, variant, frames in zip(stats, variants, (1, 1, 2)):
            if st is None:
                continue
            items = W * H * spp * frames
            assert st["samples"] == items, (spp, variant)
            assert st["rays_traced"] == ost["rays_traced"] * frames, (spp, variant)
            assert st["kernel_variant"] == variant and st["scan_mode"] == 5, (spp, st)
            assert st["grid_blocks"] == min(cus * 1, -(-items // 256)), (spp, variant, st["grid_blocks"])
            assert (st["direct_samples"] == items) == direct, (spp, variant, st["direct_samples"])


def test_the_book_scene_on_a_ring_of_blocks_of_64(one_per_cu, oracle_mod, book1_flat):
    _check_paths(one_per_cu, oracle_mod, book1_flat, 5, (1, 9, 17), direct=False)


def test_the_book_scene_with_every_sample_direct(one_per_cu, oracle_mod, book1_flat):
    _check_paths(one_per_cu, oracle_mod, book1_flat, 3, (1, 9, 17), direct=True)


def test_the_large_grid_kernel(one_per_cu, oracle_mod, tenk_flat):
    _check_paths(one_per_cu, oracle_mod, tenk_flat, 5, (0, 8, 16), direct=False)


def test_depth_zero_reports_what_it_always_did(one_per_cu, book1_flat):
    w, h, spp = 8, 8, 2
    one_per_cu.upload_scene(book1_flat)
    dense, listed, batch, stats = _three_launches(one_per_cu, rt.book1_camera(w, h), rt.make_params(w, h, spp, max_depth=0, seed=SEED), True)
    assert not dense.any() and not listed.any() and not batch.any()        # (black without tracing; the pattern was cleared)
    assert [st["samples"] for st in stats] == [w * h * spp, w * h * spp, 2 * w * h * spp]
    assert [st["rays_traced"] for st in stats] == [0, 0, 0]
    assert [st["scan_mode"] for st in stats] == [0, 0, 5]                   # (the frame batch says 5 where the other two say 0: kept as it is)


def test_a_rejected_uniform53_combination_touches_nothing(one_per_cu, oracle_mod, book1_flat):
    import bench
    one_per_cu.upload_scene(book1_flat)
    cam = rt.book1_camera(W, H)
    d_fix = torch.full((H, W, 3), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    bad = rt.make_params(W, H, 5, seed=SEED, flags=_ffi.RT_FLAG_UNIFORM53 | _ffi.RT_FLAG_DIAG_STATS)
    rc = _ffi.load().rt_render_device(one_per_cu._h, C.byref(cam.to_rt_camera()), C.byref(bad), C.c_void_p(d_fix.data_ptr()), C.c_void_p(stream))
    assert rc == -1                                                          # RT_ERR_INVALID_ARGUMENT
    assert _ffi.load().rt_last_error().decode() == ("RT_FLAG_UNIFORM53 runs with scan mode 5 (the default) or RT_FLAG_NO_FILTER, "
                                                    "without RT_FLAG_DIAG_STATS")
    torch.cuda.synchronize()
    # The check now comes before the launch takes a slot and queues the clear of the caller's buffer.  (A library of an earlier
    # revision, loaded through RTIOW_HIP_LIB, still cleared it: asserted on the library built from this tree.)
    if _ffi.load().rt_build_source_sha().decode() == bench.kernel_source_sha():
        assert (d_fix == 0x5A5A5A5A).all().item()
    good = rt.make_params(W, H, 5, seed=SEED, flags=_ffi.RT_FLAG_UNIFORM53)
    one_per_cu.render_device(cam, good, d_fix.data_ptr(), stream)
    st = one_per_cu.last_stats()
    want, _, ost = oracle_mod.render_b(oracle_mod.camera_from_host(cam), book1_flat, oracle_mod.make_params(W, H, 5, seed=SEED, uniform53=True))
    assert np.array_equal(d_fix.cpu().numpy().view(np.uint64), want)
    assert st["kernel_variant"] == 3 and st["samples"] == W * H * 5 and st["rays_traced"] == ost["rays_traced"]
