"""The occupancy grid on the MI355X (csrc/occupancy.hip, scnerf_amd/occupancy.py, ops.inference_occupancy): the kernels
through the C ABI against the transcriptions of tests/occupancy_reference.py -- the index list, the slot table, the live
rows and BOTH copies of the count, each launch twice for identical bytes --, and a forward-only render_rays call under the
switch against the oracle of tests/occupancy_cases.py, bit for bit in all twelve outputs: a ball-shaped grid at (24, 16,
8), (70, 16, 24) and (130, 64, 128) -- 64 coarse samples otherwise take the one-launch coarse stage --, every bit set
(the switch-off call's bits, on the resident, the fp32 and the one-product arithmetic), no bit set (no network launch),
N_importance = 0, with inference_skip_empty, with noise and with gradients (the switch is not noticed), stale and foreign
networks, a grid on the wrong device, and the baking.  Interpreter twin: tests/test_emu_occupancy.py."""
import numpy as np
import pytest
import torch

from tests import occupancy_cases as C
from tests import skip_empty_case as SE

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def _lib():
    from scnerf_amd import _capi
    return _capi.load(), _capi.current_stream()


class Gpu:
    @staticmethod
    def compact(pts, vd, vd_stride, spr, bits, R, lo, inv):
        lib, stream = _lib()
        P = pts.shape[0]
        pts_d, vd_d, bits_d = _dev(pts), _dev(vd), _dev(bits)
        live_idx = torch.full((P,), C.SENTINEL, dtype=torch.int32, device="cuda")
        slot_of = torch.full((P,), C.SENTINEL, dtype=torch.int32, device="cuda")
        pts_live, vd_live = (torch.full((P, 3), float("nan"), device="cuda") for _ in range(2))
        ws = torch.zeros(int(lib.scnerf_occ_compact_workspace_ints(P)), dtype=torch.int32, device="cuda")
        n_dev = torch.full((1,), C.SENTINEL, dtype=torch.int32, device="cuda")
        n_host = torch.full((1,), C.SENTINEL, dtype=torch.int32, device="cpu").pin_memory()
        st = lib.scnerf_occ_compact(_ptr(pts_d), P, _ptr(vd_d), vd_stride, spr, _ptr(bits_d), R, *[float(x) for x in lo],
                                    *[float(x) for x in inv], _ptr(ws), _ptr(live_idx), _ptr(slot_of), _ptr(pts_live),
                                    _ptr(vd_live), _ptr(n_dev), _ptr(n_host), stream)
        assert st == 0, st
        ev = torch.cuda.Event()
        ev.record()
        ev.synchronize()
        host_count = int(n_host[0])                      # behind the event alone: no copy, no device read
        return (live_idx.cpu().numpy(), slot_of.cpu().numpy(), pts_live.cpu().numpy(), vd_live.cpu().numpy(),
                int(n_dev.cpu()[0]), host_count)

    @staticmethod
    def expand(raw_live, slot_of, n_live):
        lib, stream = _lib()
        P = slot_of.shape[0]
        raw = torch.full((P, 4), float("nan"), device="cuda")
        raw_d, slot_d = _dev(raw_live), _dev(slot_of)
        st = lib.scnerf_occ_expand_raw(_ptr(raw_d), _ptr(slot_d), _ptr(raw), P, n_live, stream)
        assert st == 0, st
        return raw.cpu().numpy()

    @staticmethod
    def probe(first, n_cells, R, k, lo, cell):
        lib, stream = _lib()
        pts = torch.full((n_cells * k ** 3, 3), float("nan"), device="cuda")
        offs = [float(np.float32(np.float32(j + 0.5) / np.float32(k))) if j < k else 0.0 for j in range(3)]
        st = lib.scnerf_occ_probe_points(first, n_cells, R, k, *[float(x) for x in lo], *[float(x) for x in cell], *offs,
                                         _ptr(pts), stream)
        assert st == 0, st
        return pts.cpu().numpy()

    @staticmethod
    def accumulate(raw, sigma_min, first, n_cells, R, k, bits):
        lib, stream = _lib()
        raw_d, bits_d = _dev(raw), _dev(bits)
        st = lib.scnerf_occ_accumulate(_ptr(raw_d), float(sigma_min), first, n_cells, R, k, _ptr(bits_d), stream)
        assert st == 0, st
        return bits_d.cpu().numpy()

    @staticmethod
    def dilate(bits, R):
        lib, stream = _lib()
        bits_d = _dev(bits)
        out = torch.full_like(bits_d, C.SENTINEL)
        st = lib.scnerf_occ_dilate(_ptr(bits_d), _ptr(out), R, stream)
        assert st == 0, st
        return out.cpu().numpy()


@pytest.fixture
def ops():
    from scnerf_amd import ops as O
    before = (O.inference_arithmetic(), O.mlp_arithmetic(), O.resident_guard(), O.inference_skip_empty())
    O.mlp_arithmetic("resident")
    O.inference_arithmetic("same")
    O.resident_guard("off")
    O.inference_skip_empty("off")
    O.inference_occupancy("off")
    yield O
    O.inference_arithmetic(before[0])
    O.mlp_arithmetic(before[1])
    O.resident_guard(before[2])
    O.inference_skip_empty("off" if before[3] is None else before[3])
    O.inference_occupancy("off")


_shared = {}


def _nets():
    """(read only: one pair for the module)"""
    if "nets" not in _shared:
        _shared["nets"] = SE.networks("cuda")
    return _shared["nets"]


@pytest.mark.parametrize("kind", C.GRIDS)
@pytest.mark.parametrize("spr", [1, 16])
@pytest.mark.parametrize("P", C.SIZES)
def test_compaction_and_expansion_equal_the_transcription(P, spr, kind):
    C.check_compact_and_expand(Gpu, P, spr, kind)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_probe_points_and_accumulation_equal_the_transcription(k):
    C.check_probe_points(Gpu, k)
    C.check_accumulate(Gpu, k)


@pytest.mark.parametrize("R", [32, 64])
def test_dilation_of_single_cells_is_the_clipped_cube(R):
    C.check_dilate(Gpu, R)


def test_argument_errors_and_the_optional_pinned_word():
    lib, stream = _lib()
    bits, R, lo, inv = C.kernel_grid("ball")
    pts, vd = C.kernel_points(64, 16)
    pts_d, vd_d, bits_d = _dev(pts), _dev(vd), _dev(bits)
    i32 = torch.zeros((2, 64), dtype=torch.int32, device="cuda")
    f3 = torch.zeros((2, 64, 3), device="cuda")
    ws = torch.zeros(4, dtype=torch.int32, device="cuda")
    one = torch.zeros(1, dtype=torch.int32, device="cuda")
    box = [float(x) for x in lo] + [float(x) for x in inv]

    def compact(pts_=pts_d, P=64, R_=R, idx=i32[0], host=None):
        return lib.scnerf_occ_compact(_ptr(pts_), P, _ptr(vd_d), 5, 16, _ptr(bits_d), R_, *box, _ptr(ws), _ptr(idx), _ptr(i32[1]),
                                      _ptr(f3[0]), _ptr(f3[1]), _ptr(one), host, stream)
    assert compact() == 0
    assert int(one.cpu()[0]) == int((~C.REF.dead_mask(pts, bits, R, lo, inv)).sum())
    assert compact(pts_=None) == C.EINVAL and compact(idx=None) == C.EINVAL
    assert compact(R_=48) == C.EINVAL and compact(P=1 << 31) == C.EINVAL
    raw = torch.zeros((64, 4), device="cuda")
    assert lib.scnerf_occ_expand_raw(None, _ptr(i32[0]), _ptr(raw), 64, 64, stream) == C.EINVAL
    assert lib.scnerf_occ_expand_raw(_ptr(raw), _ptr(i32[0]), _ptr(raw.clone()), 1 << 31, 0, stream) == C.EINVAL
    geo = [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.5, 0.0, 0.0]
    assert lib.scnerf_occ_probe_points(32, 64, 32, 1, *geo, _ptr(f3[0]), stream) == C.EINVAL     # first cell not a multiple of 64
    assert lib.scnerf_occ_probe_points(64, 64, 48, 1, *geo, _ptr(f3[0]), stream) == C.EINVAL
    assert lib.scnerf_occ_probe_points(64, 64, 32, 1, *geo, None, stream) == C.EINVAL
    words = torch.zeros(32 ** 3 // 32, dtype=torch.int32, device="cuda")
    assert lib.scnerf_occ_accumulate(_ptr(raw), 0.0, 96, 64, 32, 1, _ptr(words), stream) == C.EINVAL
    assert lib.scnerf_occ_accumulate(None, 0.0, 64, 64, 32, 1, _ptr(words), stream) == C.EINVAL
    assert lib.scnerf_occ_dilate(_ptr(words), _ptr(words.clone()), 40, stream) == C.EINVAL
    assert lib.scnerf_occ_dilate(_ptr(words), None, 32, stream) == C.EINVAL
    torch.cuda.synchronize()


def test_wrappers_on_tensors(ops):
    """ops.occ_compact / occ_expand_raw: the same numbers through the typed wrappers, the view directions as a column
    slice of a ray batch"""
    P, spr = 70 * 16, 16
    bits, R, lo, inv = C.kernel_grid("ball")
    pts, vd = C.kernel_points(P, spr)
    grid = C.hand_grid(C.REF.mask_of_bits(bits, R), "cuda", lo=C.KLO, hi=C.KHI)
    assert grid.inv == tuple(float(x) for x in inv)
    live, slot_of, pts_live, vd_live = C.REF.compact(pts, vd, spr, bits, R, lo, inv)
    ops.occupancy_stats(reset=True)
    rays = _dev(vd)
    live_idx, slots, pts_l, vd_l, n_live = ops.occ_compact(_dev(pts), rays[:, 0:3], spr, grid)
    assert n_live == live.shape[0] and ops.occupancy_stats(reset=True) == {"samples": P, "skipped": P - n_live}
    assert np.array_equal(live_idx[:n_live].cpu().numpy(), live) and np.array_equal(slots.cpu().numpy(), slot_of)
    assert pts_l.cpu().numpy().tobytes() == pts_live.tobytes() and vd_l.cpu().numpy().tobytes() == vd_live.tobytes()
    raw_live = torch.randn(n_live, 4, device="cuda")
    assert ops.occ_expand_raw(raw_live, slots, n_live).cpu().numpy().tobytes() == C.REF.expand(raw_live.cpu().numpy(), slot_of).tobytes()
    with pytest.raises(ValueError):
        ops.occ_expand_raw(raw_live[:-1].contiguous(), slots, n_live)


@pytest.mark.parametrize("shape", [(24, 16, 8), (70, 16, 24), (130, 64, 128)])
def test_the_render_path_equals_the_oracle(ops, shape):
    C.mixed_case(ops, "cuda", _nets(), *shape)


@pytest.mark.parametrize("variant", ["white_bkgd", "lindisp", "injected_draws"])
def test_the_render_path_equals_the_oracle_in_every_variant(ops, variant):
    from scnerf_amd import synthetic as synth
    n, sc, sf = 130, 64, 128
    rnd = synth.render_randoms(n, sc, sf, seed=3) if variant == "injected_draws" else None
    C.mixed_case(ops, "cuda", _nets(), n, sc, sf, white_bkgd=variant == "white_bkgd", lindisp=variant == "lindisp",
                 randoms=None if rnd is None else {"t_rand": rnd["t_rand"].cuda(), "u": rnd["u"].cuda()})


@pytest.mark.parametrize("mode", ["resident", "fp32", "fast"])
def test_every_bit_set_returns_the_switch_off_bits(ops, mode):
    if mode == "fp32":
        ops.mlp_arithmetic("fp32")
    elif mode == "fast":
        ops.inference_arithmetic("fast")
    C.all_set_case(ops, "cuda", _nets(), 130, 64, 128, what=mode + ": ")
    C.all_set_case(ops, "cuda", _nets(), 70, 16, 24, what=mode + ": ")


def test_no_bit_set_launches_no_network(ops, monkeypatch):
    C.none_set_case(ops, "cuda", _nets(), 130, 64, 128, monkeypatch)


def test_no_importance_samples(ops):
    C.mixed_case(ops, "cuda", _nets(), 130, 64, 0)


def test_with_skip_empty_equals_the_composition_by_hand(ops):
    C.with_skip_empty_case(ops, "cuda", _nets(), 130, 64, 128)


def test_the_guard_in_fallback_mode(ops):
    ops.resident_guard("fallback")
    C.mixed_case(ops, "cuda", _nets(), 130, 64, 128, what="guard fallback: ")


def test_a_call_that_tracks_gradients_does_not_notice(ops):
    C.tracking_case(ops, "cuda", SE.networks("cuda"), 130, 64, 128)


def test_a_call_with_density_noise_does_not_notice(ops):
    C.noise_case(ops, "cuda", _nets(), 130, 64, 128)


def test_stale_and_foreign_networks_raise(ops):
    C.stale_and_foreign_case(ops, "cuda", SE.networks("cuda"))


def test_a_grid_on_the_wrong_device_is_a_value_error(ops):
    from scnerf_amd import synthetic as synth
    rays = synth.ray_batch(24, seed=1).cuda()
    grid = C.hand_grid(C.mixed_mask(), "cpu")
    with pytest.raises(ValueError):
        C.with_grid(ops, grid, lambda: C.node(rays, _nets(), 16, 8))
    assert C.node(rays, _nets(), 16, 8)["rgb_map"].shape == (24, 3)


@pytest.mark.parametrize("probes", [1, 2])
def test_baking_equals_the_transcription(ops, probes):
    nets = SE.networks("cuda")
    grid = C.bake_case(ops, "cuda", nets, probes)
    assert 0.0 < grid.occupied_fraction() <= 1.0
    moved = grid.to("cpu")
    assert moved.bits.device.type == "cpu" and torch.equal(moved.bits, grid.bits.cpu())
    # a baked grid serves its networks and refuses them once their weights have moved
    C.stale_and_foreign_case(ops, "cuda", nets, grid=grid)
