"""scnerf_ray_batch (csrc/ray_batch.hip under the CPU SIMT interpreter) on numpy buffers: the permutation is a bijection
and equals the numpy transcription (tests/batching_reference.py) integer for integer; both modes, rank slices, the three
image storages bit for bit, optional and unwritten outputs, argument errors, uniformity against the chi-square quantile
that numpy's own sampler is held to, and the Python layer (scnerf_amd.batching) on top of the same library."""
import numpy as np
import pytest
import torch

from tests import batching_reference as R
from tests.emu import harness as H

pytestmark = pytest.mark.emu
EINVAL = R.EINVAL
SENTINEL = -7777
SIZES = (1, 2, 3, 5, 16, 17, 33, 480, 1025, 4097)
SEEDS = (0, 0x1234567, 0xFEDCBA9876543210)


def run(mode, seed, step, n, Hh, Ww, images=None, image_ids=None, n_sel=1, image_pos=0, window=None, rank=0, world=1,
        white_bkgd=False, want=(True, True, True, True), pad=0, status=False, n_images=None):
    """-> coords, select_inds, image_idx, target (None where not wanted); `pad` extra sentinel rows after n"""
    x0, y0, ww, wh = window if window is not None else (0, 0, Ww, Hh)
    rows = max(n, 0) + pad
    coords = np.full((rows, 2), SENTINEL, np.int64) if want[0] else None
    sel = np.full(rows, SENTINEL, np.int64) if want[1] else None
    idx = np.full(rows, SENTINEL, np.int64) if want[2] else None
    tgt = np.full((rows, 3), np.float32(SENTINEL), np.float32) if (want[3] and images is not None) else None
    u8, ch, ni = 0, 3, n_sel
    if images is not None:
        u8, ch, ni = int(images.dtype == np.uint8), images.shape[3], images.shape[0]
    ids = None if image_ids is None else np.ascontiguousarray(image_ids, np.int64)
    args = (mode, seed, step, images, u8, ch, ni if n_images is None else n_images, Hh, Ww, ids, n_sel, image_pos, x0, y0, ww,
            wh, n, rank, world, int(white_bkgd), coords, sel, idx, tgt, None)
    if status:
        return H.lib_call_status("scnerf_ray_batch", *args)
    H.call("scnerf_ray_batch", *args)
    return coords, sel, idx, tgt


def order(M, seed, epoch):
    """the M rays of one epoch of a 1 x M 'image stack' in all_images mode: pi_epoch(0 .. M-1)"""
    assert epoch * M < 2 ** 62
    return run(R.ALL_IMAGES, seed, epoch, M, 1, M)[1]


def test_the_transcription_is_the_published_philox():
    """the known answers of Random123's kat_vectors for philox4x32-10: the yardstick below is that generator"""
    for counter, key, want in (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                               ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                               ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
                                (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))):
        got = R.philox4x32_10(*[np.array([c], np.uint64) for c in counter], *key)
        assert tuple(int(v[0]) for v in got) == want


@pytest.mark.parametrize("M", SIZES)
def test_bijection_and_transcription(M):
    seen = {}
    for seed in SEEDS:
        for epoch in (0, 1):
            got = order(M, seed, epoch)
            assert np.array_equal(np.sort(got), np.arange(M)), (M, seed, epoch)
            want = R.permute(np.arange(M, dtype=np.uint64), M, seed, np.uint64(epoch), R.ALL_IMAGES).astype(np.int64)
            assert np.array_equal(got, want), (M, seed, epoch)
            seen[seed, epoch] = got.tobytes()
    if M >= 16:                              # 16! orders and more: two keys that agree would be a defect, not chance
        assert len(set(seen.values())) == len(seen)


def test_one_image_mode_uses_the_same_permutation_with_its_own_key():
    for M in SIZES:
        got = run(R.ONE_IMAGE, 5, 3, M, 1, M)[1]
        assert np.array_equal(np.sort(got), np.arange(M))
        assert np.array_equal(got, R.permute(np.arange(M, dtype=np.uint64), M, 5, np.uint64(3), R.ONE_IMAGE).astype(np.int64))
        if M >= 16:
            assert not np.array_equal(got, order(M, 5, 3))


@pytest.mark.parametrize("n_sel,Hh,Ww", [(100, 1080, 1920), (1, 1, 2 ** 39 + 7)], ids=["100x1080x1920", "2^39+7"])
def test_large_domains(n_sel, Hh, Ww):
    M, n = n_sel * Hh * Ww, 4096
    for step in (0, 12345):
        coords, sel, idx, _ = run(R.ALL_IMAGES, 99, step, n, Hh, Ww, n_sel=n_sel)
        flat = idx * (Hh * Ww) + sel
        assert flat.min() >= 0 and flat.max() < M and len(np.unique(flat)) == n
        wc, ws, wi = R.batch(R.ALL_IMAGES, 99, step, n, Hh, Ww, n_sel=n_sel)
        assert np.array_equal(coords, wc) and np.array_equal(sel, ws) and np.array_equal(idx, wi)


def test_large_window_in_one_image_mode():
    Hh, Ww, n = 1, 2 ** 39 + 7, 4096
    coords, sel, idx, _ = run(R.ONE_IMAGE, 3, 8, n, Hh, Ww, rank=1, world=2)
    assert sel.min() >= 0 and sel.max() < Ww and len(np.unique(sel)) == n
    wc, ws, wi = R.batch(R.ONE_IMAGE, 3, 8, n, Hh, Ww, rank=1, world=2)
    assert np.array_equal(coords, wc) and np.array_equal(sel, ws) and np.array_equal(idx, wi)


def stack(n, Hh, Ww, channels=3, dtype=np.float32, seed=0):
    rng = np.random.RandomState(seed)
    if dtype == np.uint8:
        return rng.randint(0, 256, (n, Hh, Ww, channels)).astype(np.uint8)
    return rng.rand(n, Hh, Ww, channels).astype(np.float32)


def test_all_images_epochs_straddle_and_gather():
    Hh, Ww, n, ids = 20, 24, 100, np.array([4, 0, 2])
    images = stack(5, Hh, Ww)
    M = 3 * Hh * Ww
    assert M == 1440 and M % n != 0
    flat, targets = [], []
    for step in range(30):
        coords, sel, idx, tgt = run(R.ALL_IMAGES, 11, step, n, Hh, Ww, images=images, image_ids=ids, n_sel=3)
        assert coords.shape == (n, 2) and np.isfinite(tgt).all()                       # every batch is full
        assert np.array_equal(sel, coords[:, 1] * Ww + coords[:, 0])
        assert (coords[:, 0] >= 0).all() and (coords[:, 0] < Ww).all() and (coords[:, 1] >= 0).all() and (coords[:, 1] < Hh).all()
        assert (idx >= 0).all() and (idx < 3).all()
        assert tgt.tobytes() == images[ids[idx], coords[:, 1], coords[:, 0]].tobytes()
        wc, ws, wi = R.batch(R.ALL_IMAGES, 11, step, n, Hh, Ww, n_sel=3)
        assert np.array_equal(coords, wc) and np.array_equal(sel, ws) and np.array_equal(idx, wi)
        flat.append(idx * (Hh * Ww) + sel)
    flat = np.concatenate(flat)
    assert len(flat) == 3000                                                            # two whole epochs and 120 rays
    for epoch in range(2):
        assert np.array_equal(np.sort(flat[epoch * M:(epoch + 1) * M]), np.arange(M)), epoch
    assert len(np.unique(flat[2 * M:])) == 120
    assert not np.array_equal(flat[:M], flat[M:2 * M])
    # step 14 holds rays 1400 .. 1499: the last 40 of epoch 0 and the first 60 of epoch 1
    assert np.array_equal(flat[1400:1500], np.concatenate([
        R.permute(np.arange(1400, 1440, dtype=np.uint64), M, 11, np.uint64(0), R.ALL_IMAGES),
        R.permute(np.arange(0, 60, dtype=np.uint64), M, 11, np.uint64(1), R.ALL_IMAGES)]).astype(np.int64))


@pytest.mark.parametrize("frac", [None, 0.5], ids=["full", "precrop"])
def test_one_image_windows(frac):
    Hh, Ww = 21, 25
    images = stack(4, Hh, Ww)
    window = (0, 0, Ww, Hh) if frac is None else R.precrop_window(Hh, Ww, frac)
    if frac is not None:
        assert window == (6, 5, 12, 10)                  # dW = int(12 * .5) = 6 about 12; dH = int(10 * .5) = 5 about 10
    x0, y0, ww, wh = window
    M = ww * wh
    for n in (1, 65, M):
        for step in (0, 1):
            coords, sel, idx, tgt = run(R.ONE_IMAGE, 21, step, n, Hh, Ww, images=images, image_ids=np.array([3, 1]), n_sel=2,
                                        image_pos=1, window=window)
            assert len(np.unique(sel)) == n and np.array_equal(sel, coords[:, 1] * Ww + coords[:, 0])
            assert (coords[:, 0] >= x0).all() and (coords[:, 0] < x0 + ww).all()
            assert (coords[:, 1] >= y0).all() and (coords[:, 1] < y0 + wh).all()
            assert (idx == 1).all()
            assert tgt.tobytes() == images[1, coords[:, 1], coords[:, 0]].tobytes()
            wc, ws, wi = R.batch(R.ONE_IMAGE, 21, step, n, Hh, Ww, image_pos=1, window=window)
            assert np.array_equal(coords, wc) and np.array_equal(sel, ws) and np.array_equal(idx, wi)
    assert run(R.ONE_IMAGE, 21, 0, M, Hh, Ww, window=window, status=True) == 0
    assert run(R.ONE_IMAGE, 21, 0, M + 1, Hh, Ww, window=window, status=True) == EINVAL
    assert run(R.ONE_IMAGE, 21, 0, M // 2 + 1, Hh, Ww, window=window, rank=1, world=2, status=True) == EINVAL


@pytest.mark.parametrize("mode", [R.ONE_IMAGE, R.ALL_IMAGES], ids=["one_image", "all_images"])
def test_rank_slices_are_disjoint_and_tile_the_global_batch(mode):
    Hh, Ww, n = 20, 24, 100
    images = stack(3, Hh, Ww)
    kw = dict(images=images, n_sel=3, image_pos=2)
    for step in (0, 2, 7):
        whole = run(mode, 42, step, 4 * n, Hh, Ww, **kw)
        parts = [run(mode, 42, step, n, Hh, Ww, rank=r, world=4, **kw) for r in range(4)]
        for k in range(4):
            assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k]), (step, k)
        flat = np.concatenate([p[2] * (Hh * Ww) + p[1] for p in parts])
        # all_images, step 7: rays 2800 .. 3199 of the sequence cross the epoch end at 2 x 1440, where a ray may come again
        if mode == R.ONE_IMAGE or step != 7:
            assert len(np.unique(flat)) == 4 * n


def test_uint8_storage_is_converted_as_the_loaders_do():
    Hh, Ww = 16, 16
    every = np.arange(256, dtype=np.uint8).reshape(Hh, Ww)
    rgb = np.stack([every, every[::-1], every.T], -1)[None].copy()
    coords, _, idx, tgt = run(R.ONE_IMAGE, 1, 0, 256, Hh, Ww, images=rgb)
    v = rgb[0, coords[:, 1], coords[:, 0]]
    assert set(v[:, 0].tolist()) == set(range(256))
    assert tgt.tobytes() == (v / 255.).astype(np.float32).tobytes()
    # 3 channels have nothing to composite: white_bkgd changes nothing
    assert run(R.ONE_IMAGE, 1, 0, 256, Hh, Ww, images=rgb, white_bkgd=True)[3].tobytes() == tgt.tobytes()
    rgba = np.concatenate([rgb, stack(1, Hh, Ww, 1, np.uint8, seed=3)], -1)
    rgba[0, :2, :, 3] = [[0], [255]]                          # fully transparent and fully opaque rows
    for white in (False, True):
        coords, _, idx, tgt = run(R.ALL_IMAGES, 1, 0, 256, Hh, Ww, images=rgba, white_bkgd=white)
        assert tgt.tobytes() == R.target(rgba, None, coords, idx, white).tobytes(), white
        f = (rgba[0, coords[:, 1], coords[:, 0]] / 255.).astype(np.float32)
        want = f[:, :3] * f[:, 3:] + (np.float32(1.) - f[:, 3:]) if white else f[:, :3]
        assert want.dtype == np.float32 and tgt.tobytes() == want.tobytes()


def test_a_row_outside_the_stack_is_not_read():
    images = stack(2, 4, 4)
    _, _, idx, tgt = run(R.ALL_IMAGES, 1, 0, 32, 4, 4, images=images, image_ids=np.array([1, 2]), n_sel=2)
    assert np.isnan(tgt[idx == 1]).all() and np.isfinite(tgt[idx == 0]).all()


def test_optional_outputs_and_the_tail():
    Hh, Ww, n = 20, 24, 65
    images = stack(2, Hh, Ww)
    full = run(R.ALL_IMAGES, 9, 2, n, Hh, Ww, images=images, n_sel=2, pad=5)
    for out in full:
        assert (out[:n] != SENTINEL).all() and (out[n:] == SENTINEL).all()
    for skip in range(4):
        want = tuple(k != skip for k in range(4))
        got = run(R.ALL_IMAGES, 9, 2, n, Hh, Ww, images=images, n_sel=2, pad=5, want=want)
        for k in range(4):
            if k == skip:
                assert got[k] is None
            else:
                assert got[k].tobytes() == full[k].tobytes(), (skip, k)
    # no image stack at all: the index outputs alone
    bare = run(R.ALL_IMAGES, 9, 2, n, Hh, Ww, n_sel=2, pad=5)
    assert bare[3] is None and all(bare[k].tobytes() == full[k].tobytes() for k in range(3))
    # a second call gives the same bits
    again = run(R.ALL_IMAGES, 9, 2, n, Hh, Ww, images=images, n_sel=2, pad=5)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, full))


def test_argument_errors_and_empty_batch():
    Hh, Ww = 20, 24
    images = stack(2, Hh, Ww)
    u8 = stack(2, Hh, Ww, 4, np.uint8)
    ok = lambda **k: dict(dict(mode=R.ONE_IMAGE, seed=1, step=0, n=10, Hh=Hh, Ww=Ww, images=images, n_sel=2), **k)
    assert run(status=True, **ok()) == 0
    assert run(status=True, **ok(mode=R.ALL_IMAGES)) == 0
    assert run(status=True, **ok(images=u8)) == 0
    for bad in (dict(mode=2), dict(mode=-1), dict(n=-1), dict(rank=1), dict(rank=-1), dict(rank=2, world=2), dict(world=0),
                dict(window=(0, 0, Ww + 1, Hh)), dict(window=(1, 0, Ww, Hh)), dict(window=(0, 1, Ww, Hh)),
                dict(window=(-1, 0, 4, 4)), dict(window=(0, 0, 0, 4)), dict(window=(0, 0, 4, 0)),
                dict(mode=R.ALL_IMAGES, window=(0, 0, Ww, Hh - 1)), dict(mode=R.ALL_IMAGES, window=(1, 1, 4, 4)),
                dict(image_pos=2), dict(image_pos=-1), dict(n_sel=0), dict(n_sel=3), dict(n=Hh * Ww + 1),
                dict(images=np.zeros((2, Hh, Ww, 4), np.float32)), dict(images=np.zeros((2, Hh, Ww, 2), np.uint8)),
                dict(images=np.zeros((2, Hh, Ww, 5), np.uint8)), dict(Hh=0), dict(Ww=0), dict(n_images=0),
                dict(mode=R.ALL_IMAGES, step=2 ** 62)):
        assert run(status=True, **ok(**bad)) == EINVAL, bad
    # M at the limit: 2^40 rays are one too many, in both modes
    assert run(R.ALL_IMAGES, 1, 0, 4, 1, 2 ** 20, n_sel=2 ** 20, status=True) == EINVAL
    assert run(R.ALL_IMAGES, 1, 0, 4, 2 ** 20, 2 ** 20, status=True) == EINVAL
    assert run(R.ONE_IMAGE, 1, 0, 4, 2 ** 20, 2 ** 20, window=(0, 0, 4, 4), status=True) == EINVAL
    assert run(R.ALL_IMAGES, 1, 0, 4, 1, 2 ** 20, n_sel=2 ** 20 - 1, status=True) == 0
    # a target without images
    tgt = np.zeros((10, 3), np.float32)
    assert H.lib_call_status("scnerf_ray_batch", 0, 1, 0, None, 0, 3, 2, Hh, Ww, None, 2, 0, 0, 0, Ww, Hh, 10, 0, 1, 0,
                             None, None, None, tgt, None) == EINVAL
    # n == 0: a successful no-op, whatever the mode
    for mode in (R.ONE_IMAGE, R.ALL_IMAGES):
        out = run(mode, 1, 0, 0, Hh, Ww, images=images, n_sel=2, pad=3)
        assert all((o == SENTINEL).all() for o in out)


def test_uniformity_against_the_chi_square_quantile():
    """Pearson's statistic of the per-pixel hit counts (M = 480 cells, K steps of N = 64 rays, expected K N / M each) must
    not exceed the chi-square(479) quantile at 1 - 1e-6 (Wilson-Hilferty at z = 4.753: 640.9); numpy's own sampler goes
    through the same statistic and is held to the same bound.  (Sampling without replacement within a step only lowers the
    variance of a count: the bound is on the safe side.)"""
    Hh, Ww, n, K = 20, 24, 64, 3000
    M = Hh * Ww
    bound = R.wilson_hilferty(M - 1, 4.753)
    assert abs(bound - 640.9) < 0.05
    for seed in (0, 2024):
        counts = np.zeros(M, np.int64)
        for step in range(K):
            counts += np.bincount(run(R.ONE_IMAGE, seed, step, n, Hh, Ww, want=(False, True, False, False))[1], minlength=M)
        stat = R.pearson(counts, K * n / M)
        print("seed %d: Pearson %.1f over %d cells (bound %.1f)" % (seed, stat, M, bound))
        assert counts.sum() == K * n and stat <= bound, (seed, stat, bound)
    rng = np.random.RandomState(0)
    counts = np.zeros(M, np.int64)
    for step in range(K):
        counts += np.bincount(rng.choice(M, size=[n], replace=False), minlength=M)
    stat = R.pearson(counts, K * n / M)
    print("numpy: Pearson %.1f (bound %.1f)" % (stat, bound))
    assert stat <= bound, (stat, bound)


def test_uniformity_of_the_first_element():
    Hh, Ww, K = 20, 24, 20000
    M = Hh * Ww
    bound = R.wilson_hilferty(M - 1, 4.753)
    first = np.array([run(R.ONE_IMAGE, 7, step, 1, Hh, Ww, want=(False, True, False, False))[1][0] for step in range(K)])
    stat = R.pearson(np.bincount(first, minlength=M), K / M)
    print("first element: Pearson %.1f (bound %.1f)" % (stat, bound))
    assert stat <= bound, (stat, bound)
    rng = np.random.RandomState(0)
    ref = np.array([rng.choice(M, size=[64], replace=False)[0] for _ in range(K)])
    stat = R.pearson(np.bincount(ref, minlength=M), K / M)
    print("numpy's first element: Pearson %.1f (bound %.1f)" % (stat, bound))
    assert stat <= bound, (stat, bound)


def test_python_layer_on_the_interpreter():
    """scnerf_amd.batching over the same library on CPU tensors: next() is the kernel-level sequence, state_dict resumes it"""
    from scnerf_amd import batching
    from tests.emu.host_on_emu import emulated_device
    Hh, Ww, n = 21, 25, 65
    images = stack(5, Hh, Ww)
    t_images = torch.from_numpy(images)
    ids = [4, 0, 2]
    with emulated_device():
        b = batching.RayBatcher(t_images, n, mode="all_images", image_ids=torch.tensor(ids), seed=77)
        seq = [b.next() for _ in range(3)]
        state = b.state_dict()
        assert state == {"seed": 77, "step": 3}
        later = [b.next() for _ in range(2)]
        for step, got in enumerate(seq + later):
            want = run(R.ALL_IMAGES, 77, step, n, Hh, Ww, images=images, image_ids=np.array(ids), n_sel=3)
            assert got.coords.dtype == torch.int64 and got.target.dtype == torch.float32
            for g, w in zip(got, want):
                assert g.numpy().tobytes() == w.tobytes(), step
        resumed = batching.RayBatcher(t_images, n, mode="all_images", image_ids=ids, seed=1)
        resumed.load_state_dict(state)
        for got, want in zip([resumed.next() for _ in range(2)], later):
            assert all(torch.equal(g, w) for g, w in zip(got, want))
        # one image, pre-crop, a rank slice, uint8 over white
        rgba = stack(5, Hh, Ww, 4, np.uint8)
        one = batching.RayBatcher(torch.from_numpy(rgba), 30, mode="one_image", image_ids=ids, seed=5, rank=1, world_size=2,
                                  white_bkgd=True)
        one.load_state_dict({"seed": 5, "step": 9})
        got = one.next(img_i=0, precrop_frac=0.5)
        want = run(R.ONE_IMAGE, 5, 9, 30, Hh, Ww, images=rgba, image_ids=np.array(ids), n_sel=3, image_pos=1,
                   window=R.precrop_window(Hh, Ww, 0.5), rank=1, world=2, white_bkgd=True)
        assert all(g.numpy().tobytes() == w.tobytes() for g, w in zip(got, want)) and (got.image_idx == 1).all()
        assert one.step == 10
        with pytest.raises(ValueError):
            one.next(img_i=3)                              # not among image_ids
        with pytest.raises(ValueError):
            one.next()
        with pytest.raises(ValueError):
            one.next(img_i=0, precrop_frac=0.1)            # a 2 x 2 window cannot give 2 x 30 rays
        with pytest.raises(ValueError):
            b.next(img_i=0)
        with pytest.raises(ValueError):
            b.next(precrop_frac=0.5)
        with pytest.raises(ValueError):
            batching.RayBatcher(t_images, n, mode="each_image")
        with pytest.raises(ValueError):
            batching.RayBatcher(t_images, n, image_ids=[5])
        with pytest.raises(ValueError):
            batching.RayBatcher(t_images, n, rank=2, world_size=2)
        with pytest.raises(TypeError):
            batching.RayBatcher(t_images.double(), n)
        torch.manual_seed(1234)
        assert batching.RayBatcher(t_images, n).seed == 1234
        empty = batching.RayBatcher(t_images, 0, mode="all_images").next()
        assert empty.coords.shape == (0, 2) and empty.target.shape == (0, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        batching.RayBatcher(t_images, n)                   # outside the context these are CPU tensors
