"""Interpreter twin of tests/test_gpu_early_stop.py: early ray termination (csrc/early_stop.hip, ops.inference_early_stop)
under the CPU SIMT interpreter -- the kernels through the C ABI on numpy buffers against the transcriptions of
tests/early_stop_reference.py, the render path (the package's host layer on CPU tensors, fp32 kernels, 24 rays x (16 + 8)
samples and 24 x 16 with the coarse stage final) against the oracle of tests/early_stop_cases.py.  The switch's own checks
need no kernel.

The interpreter's sizes are capped (a wave is 64 fibers): the compaction runs every (n, S) of the GPU file with n S <=
257 x 65, the transmittance -- whose reference factors come from n (S - 1) two-sample rays through the compositing kernel
-- those with n S <= 1300.

THE MIXED CASE (early_stop_cases.FINE_ALPHA_BIAS = 4.0, EPS = 1e-2; synthetic.ray_batch seed 1), measured here on the
fp64 recomputation: see test_the_render_path_equals_the_oracle's docstring."""
import numpy as np
import pytest

from tests import early_stop_cases as C
from tests.emu import harness as H

N, SC, SF = 24, 16, 8


class Emu:
    @staticmethod
    def compact(pts, vd, vd_stride, S, first, length, alive, grid):
        n = pts.shape[0] // S
        E = n * length
        live_idx, slot_of = np.full(E, C.SENTINEL, np.int32), np.full(E, C.SENTINEL, np.int32)
        pts_live, vd_live = np.full((E, 3), np.nan, np.float32), np.full((E, 3), np.nan, np.float32)
        ws = np.zeros(int(H.lib().scnerf_seg_compact_workspace_ints(E)), np.int32)
        c_dev, c_host = np.full(2, C.SENTINEL, np.int32), np.full(2, C.SENTINEL, np.int32)
        bits, R, lo, inv = grid if grid is not None else (None, 0, (0.0,) * 3, (0.0,) * 3)
        H.call("scnerf_seg_compact", pts, n, S, first, length, alive, vd, vd_stride, bits, R, *[float(x) for x in lo],
               *[float(x) for x in inv], ws, live_idx, slot_of, pts_live, vd_live, c_dev, c_host, None)
        return live_idx, slot_of, pts_live, vd_live, c_dev, c_host

    @staticmethod
    def expand(raw_live, slot_of, before, n, S, first, length, n_live):
        raw = before.copy()
        H.call("scnerf_seg_expand_raw", raw_live, slot_of, raw, n, S, first, length, n_live, None)
        return raw

    @staticmethod
    def transmittance(raw, z, rays, S, first, length, k, K, eps, T, alive, stop):
        T, alive, stop = T.copy(), alive.copy(), stop.copy()
        H.call("scnerf_seg_transmittance", np.ascontiguousarray(raw), z, rays, rays.shape[1], z.shape[0], S, first, length, k, K,
               float(eps), T, alive, stop, None)
        return T, alive, stop

    @staticmethod
    def weights(raw, z, rays):
        n, s = z.shape
        rgb, w = np.zeros((n, 3), np.float32), np.full((n, s), np.nan, np.float32)
        disp, acc, depth = (np.zeros(n, np.float32) for _ in range(3))
        H.call("scnerf_composite_fwd", np.ascontiguousarray(raw), np.ascontiguousarray(z), np.ascontiguousarray(rays),
               rays.shape[1], None, 0, rgb, disp, acc, depth, w, n, s, None)
        return w


@pytest.fixture(autouse=True)
def _blocks_on_the_calling_thread(monkeypatch):
    """as tests/test_emu_occupancy.py: this file's many small launches reuse one worker's fiber stacks"""
    monkeypatch.setenv("SIMT_EMU_THREADS", "1")


@pytest.fixture
def ops():
    from scnerf_amd import ops as O

    def off():
        O.inference_early_stop("off")
        O.inference_occupancy("off")
        O.inference_skip_empty("off")
    off()
    yield O
    off()


def test_the_switch_validates_its_arguments(ops, monkeypatch):
    C.switch_validation(ops, monkeypatch)


def test_the_transcriptions_agree_with_each_other():
    """bounds, the segment of a sample, and the fp64 decisions on a hand-made ray"""
    for S in C.SAMPLES:
        for K in C.SEGMENTS:
            if K <= S:
                b = C.REF.bounds(S, K)
                seg = C.REF.segment_of(S, K)
                assert b[0] == 0 and b[-1] == S and all(np.all(seg[b[k]:b[k + 1]] == k) for k in range(K))
    assert C.REF.bounds(5, 3) == [0, 1, 3, 5] and C.REF.bounds(2, 2) == [0, 1, 2]
    T = np.array([[0.5, 0.2, 0.05], [1e-4, 1e-9, 0.0], [0.9, 0.8, 0.7], [0.5, 1e-2, 1e-3]])
    assert C.REF.stop_segment_fp64(T, 1e-2).tolist() == [4, 1, 4, 2]
    assert C.REF.in_band(T, 1e-2).tolist() == [False, False, False, True]


SHAPES = [(n, S) for n in C.RAYS for S in C.SAMPLES]


@pytest.mark.emu
@pytest.mark.parametrize("n,S", [x for x in SHAPES if x[0] * x[1] <= 257 * 65])
def test_compaction_and_expansion_equal_the_transcription(n, S):
    C.check_compact_and_expand(Emu, n, S)


@pytest.mark.emu
@pytest.mark.parametrize("n,S", [x for x in SHAPES if x[0] * x[1] <= 1300])
def test_transmittance_and_decisions(n, S):
    C.check_transmittance(Emu, n, S)


@pytest.mark.emu
def test_argument_errors():
    st = H.lib_call_status
    bits, R, lo, inv = C.OC.kernel_grid("ball")
    n, S = 4, 16
    pts, vd = C.OC.kernel_points(n * S, S)
    i32, f3 = np.zeros(n * S, np.int32), np.zeros((n * S, 3), np.float32)
    two, ws = np.zeros(2, np.int32), np.zeros(8, np.int32)
    alive = np.ones(n, np.int32)
    box = [float(x) for x in lo] + [float(x) for x in inv]

    def compact(pts_=pts, n_=n, first=4, length=8, R_=R, idx=i32, bits_=bits, host=two.copy()):
        return st("scnerf_seg_compact", pts_, n_, S, first, length, alive, vd, 5, bits_, R_, *box, ws, idx, i32.copy(), f3, f3.copy(),
                  two, host, None)
    assert compact() == 0 and compact(bits_=None, R_=0) == 0 and compact(host=None) == 0
    assert compact(pts_=None) == C.EINVAL and compact(idx=None) == C.EINVAL
    assert compact(R_=48) == C.EINVAL and compact(n_=-1) == C.EINVAL and compact(n_=1 << 31) == C.EINVAL
    assert compact(first=12, length=8) == C.EINVAL and compact(length=0) == C.EINVAL and compact(first=-1) == C.EINVAL
    raw, rows = np.zeros((n * S, 4), np.float32), np.zeros((n * 8, 4), np.float32)
    slots = np.full(n * 8, -1, np.int32)
    assert st("scnerf_seg_expand_raw", rows, slots, raw, n, S, 4, 8, n * 8, None) == 0
    assert st("scnerf_seg_expand_raw", None, slots, raw, n, S, 4, 8, 1, None) == C.EINVAL
    assert st("scnerf_seg_expand_raw", rows, slots, None, n, S, 4, 8, 0, None) == C.EINVAL
    assert st("scnerf_seg_expand_raw", rows, slots, raw, n, S, 4, 8, n * 8 + 1, None) == C.EINVAL
    assert st("scnerf_seg_expand_raw", rows, slots, raw, n, S, 12, 8, 0, None) == C.EINVAL
    z, rays = np.ones((n, S), np.float32), np.ones((n, 11), np.float32)
    T, stop = np.zeros(n, np.float64), np.zeros(n, np.int32)

    def trans(eps=1e-3, k=0, K=2, first=0, length=8, T_=T, stride=11):
        return st("scnerf_seg_transmittance", raw, z, rays, stride, n, S, first, length, k, K, float(eps), T_, alive.copy(), stop, None)
    assert trans() == 0
    assert trans(eps=0.0) == C.EINVAL and trans(eps=1.0) == C.EINVAL and trans(eps=float("nan")) == C.EINVAL
    assert trans(k=2) == C.EINVAL and trans(k=-1) == C.EINVAL and trans(first=9, length=8) == C.EINVAL
    assert trans(T_=None) == C.EINVAL and trans(stride=5) == C.EINVAL


@pytest.mark.emu
@pytest.mark.parametrize("variant", ["plain", "white_bkgd K=2", "lindisp", "injected_draws", "coarse_final"])
def test_the_render_path_equals_the_oracle(ops, variant):
    """The mixed case at 24 x (16 + 8) and 24 x 16 (the coarse stage final), fp32 kernels, FINE_ALPHA_BIAS = 4.0, EPS =
    1e-2, synthetic.ray_batch seed 1 (the probe behind early_stop_cases.FINE_ALPHA_BIAS also ran seeds 2 and 3).  On the
    fp64 recomputation 16 of 24 rays stop before the last of K = 4 segments at 16 + 8 and 19 at 16 + 0 -- between 20 % and
    80 %, asserted below --, 6 at K = 2, 5 with lindisp; no ray of seed 1 (nor of 2 and 3) lies in the band eps (1 +- 1e-4)
    at any boundary, asserted as well.  Every run prints its counts."""
    from scnerf_amd import synthetic as synth
    from tests.emu.host_on_emu import emulated_device
    with emulated_device("fp32"):
        sf = 0 if variant == "coarse_final" else SF
        rnd = synth.render_randoms(N, SC, sf, seed=3) if variant == "injected_draws" else None
        randoms = None if rnd is None else {"t_rand": rnd["t_rand"], "u": rnd["u"]}
        white = variant == "white_bkgd K=2"
        res = C.stopped_case(ops, "cpu", C.networks("cpu"), N, SC, sf, 2 if white else 4, white_bkgd=white,
                             lindisp=variant == "lindisp", randoms=randoms, seed=1, what=variant + ": ")
        print(variant, res)
        assert res["band"] == 0, "choose another seed: a ray of the fp64 reference lies in the band"
        if variant in ("plain", "coarse_final"):
            assert 0.2 * N <= res["fp64_stopped"] <= 0.8 * N, res


@pytest.mark.emu
def test_nothing_stops_all_stop_and_too_many_segments(ops, monkeypatch):
    from tests.emu.host_on_emu import emulated_device
    with emulated_device("fp32"):
        C.nothing_stops_case(ops, "cpu", C.networks("cpu", fine_density_bias=-50.0), N, SC, SF, 4)
        C.all_stop_case(ops, "cpu", C.networks("cpu", fine_density_bias=200.0), N, SC, SF, 4, monkeypatch)
        C.all_stop_case(ops, "cpu", C.networks("cpu", fine_density_bias=200.0), N, SC, 0, 2, monkeypatch)
        C.too_many_segments_case(ops, "cpu", C.networks("cpu"))


@pytest.mark.emu
def test_with_skip_empty_and_with_the_occupancy_grid(ops):
    from tests.emu.host_on_emu import emulated_device
    with emulated_device("fp32"):
        nets = C.networks("cpu")
        C.with_skip_empty_case(ops, "cpu", nets, N, SC, SF, 4)
        C.with_grid_case(ops, "cpu", nets, N, SC, SF, 4)
        C.with_grid_case(ops, "cpu", nets, N, SC, SF, 4, skip_empty=True)


@pytest.mark.emu
def test_calls_with_noise_or_gradients_do_not_notice(ops):
    from tests.emu.host_on_emu import emulated_device
    with emulated_device("fp32"):
        nets = C.networks("cpu")
        C.noise_case(ops, "cpu", nets, N, SC, SF, 4)
        C.tracking_case(ops, "cpu", nets, 4, SC, SF, 4)
