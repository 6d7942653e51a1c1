"""ops.inference_occupancy_nerfpp on the MI355X (pytest -m gpu): the kernels of csrc/npp_occupancy.hip through the C ABI
against the transcriptions of tests/npp_occupancy_reference.py -- the index list, the slot table, the live rows and BOTH
copies of the count, each launch twice for identical bytes --, and the NeRF++ node, the baking and render_single_image with
the switch on against the oracle of tests/npp_occupancy_cases.py, bit for bit in all eight outputs, in the fp32, resident
and one-product arithmetics.  Interpreter twin: tests/test_emu_npp_occupancy.py."""
import numpy as np
import pytest
import torch

from tests import npp_occupancy_cases as C

pytestmark = pytest.mark.gpu
MODES = ["fp32", "resident", "fast"]


class GpuRoute:
    """how the kernel cases hold buffers and call the C ABI on the device"""
    @staticmethod
    def inp(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()

    @staticmethod
    def out(shape, dtype=np.float32):
        full = (shape[0] + 2,) + tuple(shape[1:])
        if dtype == np.int32:
            buf = torch.full(full, C.SENTINEL, dtype=torch.int32, device="cuda")
        else:
            buf = torch.full(full, float("nan"), dtype=torch.float32, device="cuda")
        return buf, buf[1:-1]

    @staticmethod
    def pinned_word():
        return torch.full((1,), C.SENTINEL, dtype=torch.int32, device="cpu").pin_memory()

    @staticmethod
    def shifted(t):
        return t.reshape(-1)[1:]

    @staticmethod
    def size(name, n):
        from scnerf_amd import _capi
        return getattr(_capi.load(), name)(n)

    @staticmethod
    def status(name, *args):
        from scnerf_amd import _capi
        return getattr(_capi.load(), name)(*[a.data_ptr() if torch.is_tensor(a) else a for a in args], _capi.current_stream())

    @staticmethod
    def call(name, *args):
        from scnerf_amd import _capi
        _capi.check(GpuRoute.status(name, *args), name)

    @staticmethod
    def host(buf):
        return buf.cpu().numpy()

    @staticmethod
    def sync():
        # (the pinned word is read behind an event alone: no copy, no device read)
        ev = torch.cuda.Event()
        ev.record()
        ev.synchronize()


@pytest.fixture
def ops():
    assert torch.cuda.is_available()
    from scnerf_amd import ops as O
    before = (O.inference_arithmetic(), O.mlp_arithmetic(), O.resident_guard(), O.inference_skip_background())
    O.resident_guard("off")
    O.inference_skip_background("off")
    O.inference_occupancy("off")
    O.inference_occupancy_nerfpp("off")
    yield O
    O.inference_arithmetic(before[0])
    O.mlp_arithmetic(before[1])
    O.resident_guard(before[2])
    O.inference_skip_background("off" if before[3] is None else before[3])
    O.inference_occupancy("off")
    O.inference_occupancy_nerfpp("off")


def test_the_switch_the_spaces_and_the_state_dict(ops):
    C.validation(ops)


@pytest.mark.parametrize("kind", C.GRIDS)
@pytest.mark.parametrize("P", C.SIZES)
def test_compaction_and_expansion_equal_the_transcription(P, kind):
    C.check_compact4_and_expand(GpuRoute, P, kind)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_inverted_probe_points_equal_the_transcription(k):
    C.check_probe_points_inverted(GpuRoute, k)


def test_bad_arguments_are_status_codes():
    C.argument_checks(GpuRoute)


def test_wrappers_on_tensors(ops):
    """ops.occ_compact4 / occ_expand_raw: the same numbers through the typed wrappers, the view directions as a column slice"""
    P, spr = 70 * 16, 12
    bits, R, lo, inv = C.kernel_grid("halfball", C.BOXES[1])
    pts, vd = C.kernel_points(P, spr, C.BOXES[1])
    grid = C.hand_grid(C.REF.mask_of_bits(bits, R), "cuda", "inverted_sphere", C.BOXES[1])
    assert grid.inv == tuple(float(x) for x in inv)
    live, slot_of, pts_live, vd_live = C.REF4.compact4(pts, vd, spr, bits, R, lo, inv)
    before = (ops.occupancy_stats(), ops.occupancy_nerfpp_stats())
    rays = GpuRoute.inp(vd)
    live_idx, slots, pts_l, vd_l, n_live = ops.occ_compact4(GpuRoute.inp(pts), rays[:, 0:3], spr, grid)
    assert n_live == live.shape[0] and (ops.occupancy_stats(), ops.occupancy_nerfpp_stats()) == before
    assert np.array_equal(live_idx[:n_live].cpu().numpy(), live) and np.array_equal(slots.cpu().numpy(), slot_of)
    assert pts_l.cpu().numpy().tobytes() == pts_live.tobytes() and vd_l.cpu().numpy().tobytes() == vd_live.tobytes()
    raw_live = torch.randn(n_live, 4, device="cuda")
    assert ops.occ_expand_raw(raw_live, slots, n_live).cpu().numpy().tobytes() == C.REF.expand(raw_live.cpu().numpy(), slot_of).tobytes()


@pytest.mark.parametrize("mode", MODES)
def test_both_grids_mixed_equal_the_oracle(ops, mode):
    C.mixed_case(ops, "cuda", mode)


@pytest.mark.parametrize("which", ["fg", "bg"])
@pytest.mark.parametrize("mode", MODES)
def test_one_grid_alone_mixed_all_set_none_set(ops, mode, which, monkeypatch):
    C.one_grid_case(ops, "cuda", mode, which, monkeypatch)


@pytest.mark.parametrize("mode", MODES)
def test_nothing_live_launches_no_network(ops, mode, monkeypatch):
    C.nothing_live_case(ops, "cuda", mode, monkeypatch)


@pytest.mark.parametrize("mode", MODES)
def test_with_skip_background_equals_the_composition_by_hand(ops, mode):
    C.with_skip_background_case(ops, "cuda", mode)


@pytest.mark.parametrize("guard", ["fallback", "report"])
def test_with_the_scale_guard_on(ops, guard):
    C.mixed_case(ops, "cuda", "resident", guard=guard)


@pytest.mark.parametrize("mode", ["fp32", "resident"])
def test_a_call_that_tracks_gradients_does_not_notice(ops, mode):
    C.tracking_call_case(ops, "cuda", mode)


def test_the_euclidean_switch_is_still_ignored_by_the_node(ops):
    C.euclidean_switch_is_ignored_case(ops, "cuda", "resident")


def test_grids_on_the_wrong_device_are_a_value_error(ops):
    C.wrong_device_case(ops, "cuda")


@pytest.mark.parametrize("dilate", [0, 1])
@pytest.mark.parametrize("probes", [1, 2])
def test_baking_equals_the_transcription_in_both_spaces(ops, probes, dilate):
    nets, fg, bg = C.bake_case(ops, "cuda", probes, dilate)
    assert 0.0 < fg.occupied_fraction() <= 1.0 and 0.0 < bg.occupied_fraction() <= 1.0
    if (probes, dilate) == (2, 1):
        # baked grids serve their networks and refuse them once their weights have moved
        C.stale_and_foreign_case(ops, "cuda", nets[0], (fg, bg))


def test_stale_and_foreign_networks_raise(ops):
    C.stale_and_foreign_case(ops, "cuda")


@pytest.mark.parametrize("mode", MODES)
def test_render_single_image_level_by_level(ops, mode):
    C.render_single_image_case(ops, "cuda", mode, 0)
