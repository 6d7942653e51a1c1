"""Early ray termination on the MI355X (csrc/early_stop.hip, ops.inference_early_stop): the kernels through the C ABI
against the transcriptions of tests/early_stop_reference.py -- the index list, the per-segment slot table, the live rows
and BOTH copies of the two counts, the expansion into the dense raw, the fp64 transmittance and the decisions that follow
from it, each launch twice for identical bytes --, and a forward-only render_rays call under the switch against the oracle
of tests/early_stop_cases.py, bit for bit in all twelve outputs: (24, 16, 8), (70, 16, 24), (130, 64, 128) and (24, 16, 0)
-- the coarse stage final --, K = 2 and 4, white_bkgd, lindisp, the resident, the fp32 and the one-product arithmetic, the
guard in fallback mode; the stop decisions against an fp64 recomputation; the bound against the switch-off call; an eps
at which nothing stops (the switch-off call's bits), a density at which everything stops behind segment 0 (no further
network launch); with inference_skip_empty, with an occupancy grid, with both; with noise, with gradients and on the
NeRF++ node (the switch is not noticed).  Interpreter twin: tests/test_emu_early_stop.py."""
import numpy as np
import pytest
import torch

from tests import early_stop_cases as C

pytestmark = pytest.mark.gpu


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def _lib():
    from scnerf_amd import _capi
    return _capi.load(), _capi.current_stream()


class Gpu:
    @staticmethod
    def compact(pts, vd, vd_stride, S, first, length, alive, grid):
        lib, stream = _lib()
        n = pts.shape[0] // S
        E = n * length
        bits, R, lo, inv = grid if grid is not None else (None, 0, (0.0,) * 3, (0.0,) * 3)
        pts_d, vd_d, bits_d, alive_d = _dev(pts), _dev(vd), _dev(bits), _dev(alive)
        live_idx = torch.full((E,), C.SENTINEL, dtype=torch.int32, device="cuda")
        slot_of = torch.full((E,), C.SENTINEL, dtype=torch.int32, device="cuda")
        pts_live, vd_live = (torch.full((E, 3), float("nan"), device="cuda") for _ in range(2))
        ws = torch.zeros(int(lib.scnerf_seg_compact_workspace_ints(E)), dtype=torch.int32, device="cuda")
        c_dev = torch.full((2,), C.SENTINEL, dtype=torch.int32, device="cuda")
        c_host = torch.full((2,), C.SENTINEL, dtype=torch.int32, device="cpu").pin_memory()
        st = lib.scnerf_seg_compact(_ptr(pts_d), n, S, first, length, _ptr(alive_d), _ptr(vd_d), vd_stride, _ptr(bits_d), R,
                                    *[float(x) for x in lo], *[float(x) for x in inv], _ptr(ws), _ptr(live_idx), _ptr(slot_of),
                                    _ptr(pts_live), _ptr(vd_live), _ptr(c_dev), _ptr(c_host), stream)
        assert st == 0, st
        ev = torch.cuda.Event()
        ev.record()
        ev.synchronize()
        host_counts = c_host.numpy().copy()                  # behind the event alone: no copy, no device read
        return (live_idx.cpu().numpy(), slot_of.cpu().numpy(), pts_live.cpu().numpy(), vd_live.cpu().numpy(),
                c_dev.cpu().numpy(), host_counts)

    @staticmethod
    def expand(raw_live, slot_of, before, n, S, first, length, n_live):
        lib, stream = _lib()
        raw, raw_d, slot_d = _dev(before), _dev(raw_live), _dev(slot_of)
        st = lib.scnerf_seg_expand_raw(_ptr(raw_d), _ptr(slot_d), _ptr(raw), n, S, first, length, n_live, stream)
        assert st == 0, st
        return raw.cpu().numpy()

    @staticmethod
    def transmittance(raw, z, rays, S, first, length, k, K, eps, T, alive, stop):
        lib, stream = _lib()
        raw_d, z_d, rays_d, T_d, alive_d, stop_d = (_dev(a) for a in (raw, z, rays, T, alive, stop))
        st = lib.scnerf_seg_transmittance(_ptr(raw_d), _ptr(z_d), _ptr(rays_d), rays.shape[1], z.shape[0], S, first, length, k, K,
                                          float(eps), _ptr(T_d), _ptr(alive_d), _ptr(stop_d), stream)
        assert st == 0, st
        return T_d.cpu().numpy(), alive_d.cpu().numpy(), stop_d.cpu().numpy()

    @staticmethod
    def weights(raw, z, rays):
        lib, stream = _lib()
        n, s = z.shape
        raw_d, z_d, rays_d = _dev(raw), _dev(z), _dev(rays)
        rgb = torch.zeros((n, 3), device="cuda")
        disp, acc, depth = (torch.zeros(n, device="cuda") for _ in range(3))
        w = torch.full((n, s), float("nan"), device="cuda")
        st = lib.scnerf_composite_fwd(_ptr(raw_d), _ptr(z_d), _ptr(rays_d), rays.shape[1], None, 0, _ptr(rgb), _ptr(disp),
                                      _ptr(acc), _ptr(depth), _ptr(w), n, s, stream)
        assert st == 0, st
        return w.cpu().numpy()


@pytest.fixture
def ops():
    from scnerf_amd import ops as O
    before = (O.inference_arithmetic(), O.mlp_arithmetic(), O.resident_guard())

    def off():
        O.inference_early_stop("off")
        O.inference_skip_empty("off")
        O.inference_occupancy("off")
    O.mlp_arithmetic("resident")
    O.inference_arithmetic("same")
    O.resident_guard("off")
    off()
    yield O
    O.inference_arithmetic(before[0])
    O.mlp_arithmetic(before[1])
    O.resident_guard(before[2])
    off()


_shared = {}


def _nets(**kw):
    """(read only: one pair per density for the module)"""
    key = tuple(sorted(kw.items()))
    if key not in _shared:
        _shared[key] = C.networks("cuda", **kw)
    return _shared[key]


@pytest.mark.parametrize("S", C.SAMPLES)
@pytest.mark.parametrize("n", C.RAYS)
def test_compaction_and_expansion_equal_the_transcription(n, S):
    C.check_compact_and_expand(Gpu, n, S)


@pytest.mark.parametrize("S", C.SAMPLES)
@pytest.mark.parametrize("n", C.RAYS)
def test_transmittance_and_decisions(n, S):
    C.check_transmittance(Gpu, n, S)


def test_argument_errors_and_the_optional_pinned_words():
    lib, stream = _lib()
    n, S = 4, 16
    bits, R, lo, inv = C.OC.kernel_grid("ball")
    pts, vd = C.OC.kernel_points(n * S, S)
    pts_d, vd_d, bits_d = _dev(pts), _dev(vd), _dev(bits)
    i32 = torch.zeros((2, n * S), dtype=torch.int32, device="cuda")
    f3 = torch.zeros((2, n * S, 3), device="cuda")
    ws = torch.zeros(8, dtype=torch.int32, device="cuda")
    two = torch.zeros(2, dtype=torch.int32, device="cuda")
    alive = torch.ones(n, dtype=torch.int32, device="cuda")
    box = [float(x) for x in lo] + [float(x) for x in inv]

    def compact(pts_=pts_d, n_=n, first=4, length=8, R_=R, idx=i32[0], host=None):
        return lib.scnerf_seg_compact(_ptr(pts_), n_, S, first, length, _ptr(alive), _ptr(vd_d), 5, _ptr(bits_d), R_, *box, _ptr(ws),
                                      _ptr(idx), _ptr(i32[1]), _ptr(f3[0]), _ptr(f3[1]), _ptr(two), host, stream)
    assert compact() == 0
    want = C.REF.compact(pts, vd, S, 4, 8, None, (bits, R, lo, inv))
    assert two.cpu().tolist() == [want[0].shape[0], n]
    assert compact(pts_=None) == C.EINVAL and compact(idx=None) == C.EINVAL and compact(R_=48) == C.EINVAL
    assert compact(n_=1 << 31) == C.EINVAL and compact(first=12) == C.EINVAL and compact(length=0) == C.EINVAL
    pageable = np.zeros(2, np.int32)
    assert compact(host=pageable.ctypes.data) == C.EINVAL                       # not page-locked
    raw = torch.zeros((n * S, 4), device="cuda")
    assert lib.scnerf_seg_expand_raw(None, _ptr(i32[0]), _ptr(raw), n, S, 4, 8, 1, stream) == C.EINVAL
    assert lib.scnerf_seg_expand_raw(_ptr(raw), _ptr(i32[0]), _ptr(raw.clone()), n, S, 12, 8, 0, stream) == C.EINVAL
    z, rays = torch.ones((n, S), device="cuda"), torch.ones((n, 11), device="cuda")
    T = torch.zeros(n, dtype=torch.float64, device="cuda")

    def trans(eps=1e-3, k=0, K=2, T_=T):
        return lib.scnerf_seg_transmittance(_ptr(raw), _ptr(z), _ptr(rays), 11, n, S, 0, 8, k, K, float(eps), _ptr(T_), _ptr(alive),
                                            _ptr(i32[1]), stream)
    assert trans() == 0
    assert trans(eps=0.0) == C.EINVAL and trans(eps=1.0) == C.EINVAL and trans(k=2) == C.EINVAL and trans(T_=None) == C.EINVAL
    torch.cuda.synchronize()


def test_wrappers_on_tensors(ops):
    """ops.seg_compact / seg_expand_raw / seg_transmittance: the same numbers through the typed wrappers, the view
    directions as a column slice of a ray batch; the opening pass without flags and grid waits for nothing"""
    n, S, K = 70, 24, 4
    b = ops.segment_bounds(S, K)
    assert b == C.REF.bounds(S, K)
    first, length = b[1], b[2] - b[1]
    bits, R, lo, inv = C.OC.kernel_grid("ball")
    pts, vd = C.OC.kernel_points(n * S, S)
    grid = C.OC.hand_grid(C.OREF.mask_of_bits(bits, R), "cuda", lo=C.OC.KLO, hi=C.OC.KHI)
    alive = C.alive_pattern("alternating", n)
    live, slot_of, pts_live, vd_live, n_rays = C.REF.compact(pts, vd, S, first, length, alive, (bits, R, lo, inv))
    rays = _dev(vd)
    live_idx, slots, pts_l, vd_l, n_live, got_rays = ops.seg_compact(_dev(pts), rays[:, 0:3], S, first, length, _dev(alive), grid)
    assert (n_live, got_rays) == (live.shape[0], n_rays)
    assert np.array_equal(live_idx[:n_live].cpu().numpy(), live) and np.array_equal(slots.cpu().numpy(), slot_of)
    assert pts_l.cpu().numpy().tobytes() == pts_live.tobytes() and vd_l.cpu().numpy().tobytes() == vd_live.tobytes()
    _, slots0, pts0, _, n0, rays0 = ops.seg_compact(_dev(pts), rays[:, 0:3], S, 0, b[1], read=False)
    assert (n0, rays0) == (n * b[1], n) and pts0.shape == (n * b[1], 3)
    assert np.array_equal(slots0.cpu().numpy(), np.arange(n * b[1], dtype=np.int32))
    before = torch.full((n * S, 4), float("nan"), device="cuda")
    raw_live = torch.randn(n_live, 4, device="cuda")
    got = ops.seg_expand_raw(raw_live, slots, before.clone(), S, first, length, n_live)
    assert got.cpu().numpy().tobytes() == C.REF.expand(before.cpu().numpy(), raw_live.cpu().numpy(), slot_of, S, first, length).tobytes()
    with pytest.raises(ValueError):
        ops.seg_expand_raw(raw_live[:-1].contiguous(), slots, before.clone(), S, first, length, n_live)
    with pytest.raises(ValueError):
        ops.seg_compact(_dev(pts), rays[:, 0:3], S, first, length, _dev(alive), read=False)


@pytest.mark.parametrize("K", [2, 4])
@pytest.mark.parametrize("shape", [(24, 16, 8), (70, 16, 24), (130, 64, 128), (24, 16, 0)])
def test_the_render_path_equals_the_oracle(ops, shape, K):
    res = C.stopped_case(ops, "cuda", _nets(), *shape, K, what="%s K=%d: " % (shape, K))
    print(shape, K, res)


@pytest.mark.parametrize("variant", ["white_bkgd", "lindisp", "injected_draws"])
def test_the_render_path_equals_the_oracle_in_every_variant(ops, variant):
    from scnerf_amd import synthetic as synth
    n, sc, sf = 130, 64, 128
    rnd = synth.render_randoms(n, sc, sf, seed=3) if variant == "injected_draws" else None
    C.stopped_case(ops, "cuda", _nets(), n, sc, sf, 4, white_bkgd=variant == "white_bkgd", lindisp=variant == "lindisp",
                   randoms=None if rnd is None else {"t_rand": rnd["t_rand"].cuda(), "u": rnd["u"].cuda()}, what=variant + ": ")


@pytest.mark.parametrize("mode", ["fp32", "fast"])
def test_the_other_arithmetics(ops, mode):
    if mode == "fp32":
        ops.mlp_arithmetic("fp32")
    else:
        ops.inference_arithmetic("fast")
    C.stopped_case(ops, "cuda", _nets(), 130, 64, 128, 4, what=mode + ": ")
    C.stopped_case(ops, "cuda", _nets(), 70, 16, 24, 2, white_bkgd=True, what=mode + " white: ")


def test_the_guard_in_fallback_mode_takes_a_record_per_pass(ops):
    ops.resident_guard("fallback")
    K = 4
    C.stopped_case(ops, "cuda", _nets(), 130, 64, 128, K, what="guard fallback: ")
    margins = ops.resident_margins()
    assert all("fine/%d" % k in margins for k in range(K)), sorted(margins)
    assert all(margins["fine/%d" % k]["reran_blocks"] == 0 for k in range(K)), margins         # nothing trips: the bits above


def test_an_eps_at_which_nothing_stops_returns_the_switch_off_bits(ops):
    nets = _nets(fine_density_bias=-50.0)
    C.nothing_stops_case(ops, "cuda", nets, 130, 64, 128, 4)
    C.nothing_stops_case(ops, "cuda", nets, 24, 16, 0, 2)


def test_every_ray_stopped_behind_segment_0_launches_no_further_network(ops, monkeypatch):
    nets = _nets(fine_density_bias=200.0)
    C.all_stop_case(ops, "cuda", nets, 130, 64, 128, 4, monkeypatch)
    C.all_stop_case(ops, "cuda", nets, 24, 16, 0, 2, monkeypatch)


def test_with_skip_empty(ops):
    C.with_skip_empty_case(ops, "cuda", _nets(), 130, 64, 128, 4)


def test_with_the_occupancy_grid(ops):
    C.with_grid_case(ops, "cuda", _nets(), 130, 64, 128, 4)


def test_with_all_three_switches(ops):
    C.with_grid_case(ops, "cuda", _nets(), 130, 64, 128, 2, skip_empty=True)


def test_a_call_with_density_noise_does_not_notice(ops):
    C.noise_case(ops, "cuda", _nets(), 130, 64, 128, 4)


def test_a_call_that_tracks_gradients_does_not_notice(ops):
    C.tracking_case(ops, "cuda", C.networks("cuda"), 130, 64, 128, 4)


def test_the_nerfpp_node_does_not_notice(ops):
    C.nerfpp_case(ops, "cuda")


def test_more_segments_than_samples_is_a_value_error(ops):
    C.too_many_segments_case(ops, "cuda", _nets())
