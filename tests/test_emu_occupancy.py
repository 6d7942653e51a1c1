"""Interpreter twin of tests/test_gpu_occupancy.py: the occupancy grid (csrc/occupancy.hip, scnerf_amd/occupancy.py,
ops.inference_occupancy) under the CPU SIMT interpreter -- the kernels through the C ABI on numpy buffers against the
transcriptions of tests/occupancy_reference.py, the render path (the package's host layer on CPU tensors, fp32 kernels,
24 rays x (16 + 8) samples) against the oracle of tests/occupancy_cases.py.  Everything for equality of bits.  The
switch's own checks need no kernel."""
import numpy as np
import pytest

from tests import occupancy_cases as C
from tests import skip_empty_case as SE
from tests.emu import harness as H

N, SC, SF = 24, 16, 8


class Emu:
    @staticmethod
    def compact(pts, vd, vd_stride, spr, bits, R, lo, inv):
        P = pts.shape[0]
        live_idx, slot_of = np.full(P, C.SENTINEL, np.int32), np.full(P, C.SENTINEL, np.int32)
        pts_live, vd_live = np.full((P, 3), np.nan, np.float32), np.full((P, 3), np.nan, np.float32)
        ws = np.zeros(int(H.lib().scnerf_occ_compact_workspace_ints(P)), np.int32)
        n_dev, n_host = np.full(1, C.SENTINEL, np.int32), np.full(1, C.SENTINEL, np.int32)
        H.call("scnerf_occ_compact", pts, P, vd, vd_stride, spr, bits, R, *[float(x) for x in lo], *[float(x) for x in inv], ws,
               live_idx, slot_of, pts_live, vd_live, n_dev, n_host, None)
        return live_idx, slot_of, pts_live, vd_live, int(n_dev[0]), int(n_host[0])

    @staticmethod
    def expand(raw_live, slot_of, n_live):
        raw = np.full((slot_of.shape[0], 4), np.nan, np.float32)
        H.call("scnerf_occ_expand_raw", raw_live, slot_of, raw, slot_of.shape[0], n_live, None)
        return raw

    @staticmethod
    def probe(first, n_cells, R, k, lo, cell):
        pts = np.full((n_cells * k ** 3, 3), np.nan, np.float32)
        offs = [float(np.float32(np.float32(j + 0.5) / np.float32(k))) if j < k else 0.0 for j in range(3)]
        H.call("scnerf_occ_probe_points", first, n_cells, R, k, *[float(x) for x in lo], *[float(x) for x in cell], *offs, pts, None)
        return pts

    @staticmethod
    def accumulate(raw, sigma_min, first, n_cells, R, k, bits):
        bits = bits.copy()
        H.call("scnerf_occ_accumulate", np.ascontiguousarray(raw), float(sigma_min), first, n_cells, R, k, bits, None)
        return bits

    @staticmethod
    def dilate(bits, R):
        out = np.full_like(bits, C.SENTINEL)
        H.call("scnerf_occ_dilate", np.ascontiguousarray(bits), out, R, None)
        return out


@pytest.fixture(autouse=True)
def _blocks_on_the_calling_thread(monkeypatch):
    """The interpreter runs the blocks of a launch on threads of its own and keeps every thread's fiber stacks mapped for
    the life of the process; on the calling thread (one worker) the stacks are reused from launch to launch, and this
    file's many small launches leave a test worker's memory where it was."""
    monkeypatch.setenv("SIMT_EMU_THREADS", "1")


@pytest.fixture
def ops():
    from scnerf_amd import ops as O
    O.inference_occupancy("off")
    O.inference_skip_empty("off")
    yield O
    O.inference_occupancy("off")
    O.inference_skip_empty("off")


def test_the_switch_validates_its_argument(ops):
    C.switch_validation(ops)


def test_the_grid_validates_its_arguments():
    import torch
    from scnerf_amd.occupancy import OccupancyGrid, box_of_rays
    from scnerf_amd import synthetic as synth
    ok = torch.zeros((32, 32, 32), dtype=torch.bool)
    for mask, lo, hi in ((torch.zeros((48, 48, 48), dtype=torch.bool), (0, 0, 0), (1, 1, 1)), (ok, (0, 0, 0), (1, 0, 1)),
                         (ok.float(), (0, 0, 0), (1, 1, 1)), (ok, (0, 0, float("nan")), (1, 1, 1))):
        with pytest.raises(ValueError):
            OccupancyGrid.from_mask(mask, lo, hi)
    mask = torch.from_numpy(C.mixed_mask())
    grid = OccupancyGrid.from_mask(mask, C.BOX_LO, C.BOX_HI)
    assert grid.bits.numpy().tobytes() == C.REF.bits_of_mask(mask.numpy()).tobytes()
    assert grid.inv == (8.0, 8.0, 8.0) and grid.occupied_fraction() == float(mask.sum()) / 32 ** 3
    back = OccupancyGrid.from_state_dict(grid.state_dict())
    assert back.bits.numpy().tobytes() == grid.bits.numpy().tobytes() and back.inv == grid.inv
    rays = synth.ray_batch(50, seed=1)
    lo, hi = box_of_rays(rays, resolution=32)
    ends = torch.cat([rays[:, :3] + rays[:, 3:6] * rays[:, 6:7], rays[:, :3] + rays[:, 3:6] * rays[:, 7:8]])
    assert (ends > torch.tensor(lo)).all() and (ends < torch.tensor(hi)).all()


@pytest.mark.emu
@pytest.mark.parametrize("kind", C.GRIDS)
@pytest.mark.parametrize("spr", [1, 16])
@pytest.mark.parametrize("P", C.SIZES)
def test_compaction_and_expansion_equal_the_transcription(P, spr, kind):
    C.check_compact_and_expand(Emu, P, spr, kind)


@pytest.mark.emu
@pytest.mark.parametrize("k", [1, 2, 3])
def test_probe_points_and_accumulation_equal_the_transcription(k):
    C.check_probe_points(Emu, k)
    C.check_accumulate(Emu, k)


@pytest.mark.emu
@pytest.mark.parametrize("R", [32, 64])
def test_dilation_of_single_cells_is_the_clipped_cube(R):
    C.check_dilate(Emu, R)


@pytest.mark.emu
def test_argument_errors():
    st = H.lib_call_status
    bits, R, lo, inv = C.kernel_grid("ball")
    pts, vd = C.kernel_points(64, 16)
    i32, f3 = np.zeros(64, np.int32), np.zeros((64, 3), np.float32)
    one, ws = np.zeros(1, np.int32), np.zeros(4, np.int32)
    box = [float(x) for x in lo] + [float(x) for x in inv]

    def compact(pts_=pts, P=64, R_=R, idx=i32, bits_=bits):
        return st("scnerf_occ_compact", pts_, P, vd, 5, 16, bits_, R_, *box, ws, idx, i32.copy(), f3, f3.copy(), one, one.copy(), None)
    assert compact() == 0
    assert compact(pts_=None) == C.EINVAL and compact(idx=None) == C.EINVAL and compact(bits_=None) == C.EINVAL
    assert compact(R_=48) == C.EINVAL and compact(R_=0) == C.EINVAL
    assert compact(P=1 << 31) == C.EINVAL and compact(P=-1) == C.EINVAL
    # (the pinned word is optional)
    assert st("scnerf_occ_compact", pts, 64, vd, 5, 16, bits, R, *box, ws, i32, i32.copy(), f3, f3.copy(), one, None, None) == 0
    raw = np.zeros((64, 4), np.float32)
    assert st("scnerf_occ_expand_raw", raw, i32, raw.copy(), 64, 64, None) == 0
    assert st("scnerf_occ_expand_raw", None, i32, raw.copy(), 64, 64, None) == C.EINVAL
    assert st("scnerf_occ_expand_raw", raw, i32, None, 64, 0, None) == C.EINVAL
    assert st("scnerf_occ_expand_raw", raw, i32, raw.copy(), 64, 65, None) == C.EINVAL
    assert st("scnerf_occ_expand_raw", raw, i32, raw.copy(), 1 << 31, 0, None) == C.EINVAL
    p3 = np.zeros((64, 3), np.float32)
    geo = [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.5, 0.0, 0.0]
    assert st("scnerf_occ_probe_points", 64, 64, 32, 1, *geo, p3, None) == 0
    assert st("scnerf_occ_probe_points", 32, 64, 32, 1, *geo, p3, None) == C.EINVAL          # first cell not a multiple of 64
    assert st("scnerf_occ_probe_points", 64, 64, 48, 1, *geo, p3, None) == C.EINVAL
    assert st("scnerf_occ_probe_points", 64, 64, 32, 4, *geo, p3, None) == C.EINVAL
    assert st("scnerf_occ_probe_points", 64, 64, 32, 1, *geo, None, None) == C.EINVAL
    assert st("scnerf_occ_probe_points", 32 ** 3 - 64, 128, 32, 1, *geo, p3, None) == C.EINVAL    # past the grid
    words = np.zeros(32 ** 3 // 32, np.int32)
    assert st("scnerf_occ_accumulate", raw, 0.0, 64, 64, 32, 1, words, None) == 0
    assert st("scnerf_occ_accumulate", raw, 0.0, 96, 64, 32, 1, words, None) == C.EINVAL
    assert st("scnerf_occ_accumulate", raw, 0.0, 64, 64, 40, 1, words, None) == C.EINVAL
    assert st("scnerf_occ_accumulate", None, 0.0, 64, 64, 32, 1, words, None) == C.EINVAL
    assert st("scnerf_occ_accumulate", raw, 0.0, 64, 64, 32, 1, None, None) == C.EINVAL
    assert st("scnerf_occ_dilate", words, words.copy(), 32, None) == 0
    assert st("scnerf_occ_dilate", words, words.copy(), 33, None) == C.EINVAL
    assert st("scnerf_occ_dilate", None, words.copy(), 32, None) == C.EINVAL
    assert st("scnerf_occ_dilate", words, words, 32, None) == C.EINVAL                          # in place


@pytest.mark.emu
@pytest.mark.parametrize("variant", ["plain", "white_bkgd", "lindisp", "injected_draws"])
def test_the_render_path_equals_the_oracle(ops, variant):
    from scnerf_amd import synthetic as synth
    from tests.emu.host_on_emu import emulated_device
    with emulated_device("fp32"):
        rnd = synth.render_randoms(N, SC, SF, seed=3) if variant == "injected_draws" else None
        C.mixed_case(ops, "cpu", SE.networks("cpu"), N, SC, SF, white_bkgd=variant == "white_bkgd", lindisp=variant == "lindisp",
                     randoms=None if rnd is None else {"t_rand": rnd["t_rand"], "u": rnd["u"]})


@pytest.mark.emu
def test_all_set_none_set_and_no_importance(ops, monkeypatch):
    from tests.emu.host_on_emu import emulated_device
    with emulated_device("fp32"):
        nets = SE.networks("cpu")
        C.all_set_case(ops, "cpu", nets, N, SC, SF)
        C.none_set_case(ops, "cpu", nets, N, SC, SF, monkeypatch)
        C.mixed_case(ops, "cpu", nets, N, SC, 0, what="N_importance = 0: ")


@pytest.mark.emu
def test_with_skip_empty_equals_the_composition_by_hand(ops):
    from tests.emu.host_on_emu import emulated_device
    with emulated_device("fp32"):
        C.with_skip_empty_case(ops, "cpu", SE.networks("cpu"), N, SC, SF)


@pytest.mark.emu
def test_calls_with_noise_or_gradients_do_not_notice(ops):
    from tests.emu.host_on_emu import emulated_device
    with emulated_device("fp32"):
        nets = SE.networks("cpu")
        C.noise_case(ops, "cpu", nets, N, SC, SF)
        C.tracking_case(ops, "cpu", nets, 4, SC, SF)


@pytest.mark.emu
def test_stale_and_foreign_networks_and_one_baking_pass(ops):
    from tests.emu.host_on_emu import emulated_device
    with emulated_device("fp32"):
        nets = SE.networks("cpu")
        C.bake_case(ops, "cpu", nets, probes=1, first=64 * 250, n_cells=64)
        C.stale_and_foreign_case(ops, "cpu", nets)
