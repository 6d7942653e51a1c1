"""scnerf_amd.batching.RayBatcher on the MI355X: both modes against the numpy transcription (tests/batching_reference.py),
bit for bit, for fp32 and uint8 storage; no host wait in next(); rank slices; a side stream; the hand-off to
get_rays_kps_use_camera; the empty batch.  The shapes are those of tests/test_emu_batching.py."""
import numpy as np
import pytest
import torch

from tests import batching_reference as R

pytestmark = pytest.mark.gpu
HH, WW, IDS = 21, 25, [4, 0, 2]


def stack(dtype, channels=3, n=5, seed=0):
    rng = np.random.RandomState(seed)
    if dtype == np.uint8:
        return rng.randint(0, 256, (n, HH, WW, channels)).astype(np.uint8)
    return rng.rand(n, HH, WW, channels).astype(np.float32)


def same(batch, coords, select_inds, image_idx, target):
    assert batch.coords.dtype == batch.select_inds.dtype == batch.image_idx.dtype == torch.int64
    assert batch.target.dtype == torch.float32 and all(v.is_cuda for v in batch)
    assert np.array_equal(batch.coords.cpu().numpy(), coords) and np.array_equal(batch.select_inds.cpu().numpy(), select_inds)
    assert np.array_equal(batch.image_idx.cpu().numpy(), image_idx)
    assert batch.target.cpu().numpy().tobytes() == target.tobytes()


@pytest.mark.parametrize("storage", ["fp32", "u8x3", "u8x4", "u8x4_white"])
def test_both_modes_against_the_transcription(storage):
    from scnerf_amd.batching import RayBatcher
    images = stack(np.float32) if storage == "fp32" else stack(np.uint8, 3 if storage == "u8x3" else 4)
    white = storage == "u8x4_white"
    dev = torch.from_numpy(images).cuda()
    n = 65
    b = RayBatcher(dev, n, mode="all_images", image_ids=IDS, seed=77, white_bkgd=white)
    M = 3 * HH * WW
    flat = []
    for step in range(2 * M // n + 2):                                   # past two epoch ends
        got = b.next()
        coords, sel, idx = R.batch(R.ALL_IMAGES, 77, step, n, HH, WW, n_sel=3)
        same(got, coords, sel, idx, R.target(images, IDS, coords, idx, white))
        flat.append(idx * (HH * WW) + sel)
    flat = np.concatenate(flat)
    for epoch in range(2):
        assert np.array_equal(np.sort(flat[epoch * M:(epoch + 1) * M]), np.arange(M))
    for frac in (None, 0.5):
        window = (0, 0, WW, HH) if frac is None else R.precrop_window(HH, WW, frac)
        for n in (1, 65, window[2] * window[3]):
            one = RayBatcher(dev, n, mode="one_image", image_ids=IDS, seed=5, white_bkgd=white)
            for step, img_i in enumerate((0, 2)):
                got = one.next(img_i=img_i, precrop_frac=frac)
                coords, sel, idx = R.batch(R.ONE_IMAGE, 5, step, n, HH, WW, image_pos=IDS.index(img_i), window=window)
                same(got, coords, sel, idx, R.target(images, IDS, coords, idx, white))
                assert len(np.unique(sel)) == n
    with pytest.raises(ValueError):
        RayBatcher(dev, HH * WW + 1, mode="one_image").next(img_i=0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        RayBatcher(torch.from_numpy(images), n)


def test_next_does_not_make_the_host_wait():
    from scnerf_amd.batching import RayBatcher
    dev = torch.from_numpy(stack(np.uint8, 4)).cuda()
    ones = RayBatcher(dev, 65, mode="one_image", image_ids=IDS, seed=1, white_bkgd=True)
    alls = RayBatcher(dev, 65, mode="all_images", image_ids=IDS, seed=1)
    ones.next(img_i=0), alls.next()                                      # the library is loaded, the allocator is warm
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
    except Exception as e:                                               # pragma: no cover
        pytest.skip("this torch build has no sync debug mode: %s" % e)
    try:
        a = ones.next(img_i=2, precrop_frac=0.5)
        b = alls.next()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    coords, sel, idx = R.batch(R.ALL_IMAGES, 1, 1, 65, HH, WW, n_sel=3)
    assert np.array_equal(b.coords.cpu().numpy(), coords) and a.coords.shape == (65, 2)


@pytest.mark.parametrize("mode", ["one_image", "all_images"])
def test_rank_slices(mode):
    from scnerf_amd.batching import RayBatcher
    dev = torch.from_numpy(stack(np.float32)).cuda()
    n = 100
    kw = dict(img_i=2) if mode == "one_image" else {}
    whole = RayBatcher(dev, 2 * n, mode=mode, seed=9)
    ranks = [RayBatcher(dev, n, mode=mode, seed=9, rank=r, world_size=2) for r in range(2)]
    for _ in range(3):
        w = whole.next(**kw)
        parts = [r.next(**kw) for r in ranks]
        for k in range(4):
            assert torch.equal(torch.cat([p[k] for p in parts]), w[k])
        flat = torch.cat([p.image_idx * (HH * WW) + p.select_inds for p in parts])
        assert flat.unique().numel() == 2 * n


def test_side_stream():
    from scnerf_amd.batching import RayBatcher
    images = stack(np.float32)
    dev = torch.from_numpy(images).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = RayBatcher(dev, 65, mode="all_images", image_ids=IDS, seed=3).next()
        picked = dev[torch.tensor(IDS, device="cuda")[got.image_idx], got.coords[:, 1], got.coords[:, 0]]   # consumed there
        ok = torch.equal(picked, got.target)
    side.synchronize()
    coords, sel, idx = R.batch(R.ALL_IMAGES, 3, 0, 65, HH, WW, n_sel=3)
    same(got, coords, sel, idx, R.target(images, IDS, coords, idx))
    assert ok


def test_hand_off_to_the_camera_rays():
    """the batch goes into get_rays_kps_use_camera as it is and gives the rays of the same coordinates and indices built the
    reference's way on the host (NeRF/run_nerf.py:372-391)"""
    import types
    from test_gpu_camera import HH as CH, WW as CW, make_camera
    from scnerf_amd import camera_dict, get_rays
    from scnerf_amd.batching import RayBatcher
    M = types.SimpleNamespace(cd=camera_dict)
    cm, _, _ = make_camera(M, "pinhole_rot_noise_10k_rayo_rayd", False)
    dev = torch.zeros((5, CH, CW, 3), dtype=torch.uint8, device="cuda")
    batch = RayBatcher(dev, 257, mode="all_images", seed=13).next()
    ro, rd = get_rays.get_rays_kps_use_camera(CH, CW, cm, kps_list=batch.coords, idx_in_camera_param=batch.image_idx)
    coords, sel, idx = R.batch(R.ALL_IMAGES, 13, 0, 257, CH, CW, n_sel=5)
    ray_idx = idx * (CH * CW) + sel                                       # the reference's shuffled_ray_idx slice
    h_list, w_list = ray_idx % (CH * CW) // CW, ray_idx % (CH * CW) % CW
    kps = torch.from_numpy(np.stack([w_list, h_list], -1)).cuda()
    ro2, rd2 = get_rays.get_rays_kps_use_camera(CH, CW, cm, kps_list=kps,
                                                idx_in_camera_param=torch.from_numpy(ray_idx // (CH * CW)).cuda())
    assert ro.shape == (257, 3) and torch.equal(ro, ro2) and torch.equal(rd, rd2)
    one = RayBatcher(dev, 257, mode="one_image", seed=13).next(img_i=3)
    ro, rd = get_rays.get_rays_kps_use_camera(CH, CW, cm, kps_list=one.coords, idx_in_camera_param=one.image_idx)
    ro2, rd2 = get_rays.get_rays_kps_use_camera(CH, CW, cm, kps_list=one.coords, idx_in_camera_param=3)
    assert torch.equal(ro, ro2) and torch.equal(rd, rd2)


def test_empty_batch():
    from scnerf_amd.batching import RayBatcher
    dev = torch.from_numpy(stack(np.float32)).cuda()
    for mode, kw in (("one_image", dict(img_i=1)), ("all_images", {})):
        got = RayBatcher(dev, 0, mode=mode).next(**kw)
        assert got.coords.shape == (0, 2) and got.select_inds.shape == (0,) and got.image_idx.shape == (0,)
        assert got.target.shape == (0, 3)
        assert got.coords.dtype == got.select_inds.dtype == got.image_idx.dtype == torch.int64
        assert got.target.dtype == torch.float32
