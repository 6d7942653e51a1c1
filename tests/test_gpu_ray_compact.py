"""csrc/ray_compact.hip on the MI355X, through the C ABI: scnerf_ray_compact against np.flatnonzero(~(acc <= tau)) -- the
index list, the slot table and BOTH copies of the count, the one in device memory and the one the kernel stores to pinned
host memory --, scnerf_ray_rows_gather against fancy indexing, scnerf_ray_expand against a numpy scatter: all for equality,
twice for identical bytes (tests/ray_compact_cases.py), from no ray to 70 001 rays (sixteen uneven wave segments, four
tiles in flight, a last tile of 49 rays).  The interpreter twin is tests/test_emu_ray_compact.py."""
import numpy as np
import pytest
import torch

from tests import ray_compact_cases as C

pytestmark = pytest.mark.gpu
EINVAL = -22


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


class Gpu:
    @staticmethod
    def lib():
        from scnerf_amd import _capi
        return _capi.load(), _capi.current_stream()

    @staticmethod
    def compact(acc, tau):
        lib, stream = Gpu.lib()
        n = acc.shape[0]
        acc_d = _dev(acc)
        live_idx = torch.full((n,), C.SENTINEL, dtype=torch.int32, device="cuda")
        slot_of = torch.full((n,), C.SENTINEL, dtype=torch.int32, device="cuda")
        n_dev = torch.full((1,), C.SENTINEL, dtype=torch.int32, device="cuda")
        n_host = torch.full((1,), C.SENTINEL, dtype=torch.int32, device="cpu").pin_memory()
        st = lib.scnerf_ray_compact(_ptr(acc_d) if n else None, tau, _ptr(live_idx) if n else None, _ptr(slot_of) if n else None,
                                    _ptr(n_dev), _ptr(n_host), n, stream)
        assert st == 0, st
        ev = torch.cuda.Event()
        ev.record()
        ev.synchronize()
        host_count = int(n_host[0])                      # behind the event alone: no copy, no device read
        return live_idx.cpu().numpy(), slot_of.cpu().numpy(), int(n_dev.cpu()[0]), host_count

    @staticmethod
    def gather(src, live, w):
        lib, stream = Gpu.lib()
        nl = live.shape[0]
        dst = torch.full((nl, w), float("nan"), device="cuda")
        src_d, live_d = _dev(src), _dev(live)
        st = lib.scnerf_ray_rows_gather(_ptr(src_d) if src.size else None, _ptr(live_d) if nl else None, _ptr(dst) if nl else None,
                                        nl, w, src.shape[0], stream)
        assert st == 0, st
        return dst.cpu().numpy()

    @staticmethod
    def expand(slot_of, n_live, fine, coarse, s_tot, s_fine):
        lib, stream = Gpu.lib()
        n = slot_of.shape[0]
        outs = [torch.full(s, float("nan"), device="cuda")
                for s in [(n, 3), (n,), (n,), (n,), (n,), (n, s_tot, 4), (n, s_tot), (n, s_fine)]]
        ins = [_dev(a) for a in list(fine) + list(coarse)]
        slot_d = _dev(slot_of)
        st = lib.scnerf_ray_expand(_ptr(slot_d) if n else None, n, n_live, s_tot, s_fine,
                                   *[_ptr(t) if t.numel() else None for t in ins], *[_ptr(t) if t.numel() else None for t in outs],
                                   stream)
        assert st == 0, st
        return [t.cpu().numpy() for t in outs]


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("n", C.SIZES)
def test_compact_gather_expand_equal_numpy(n, kind):
    C.check_all(Gpu, n, kind)


def test_argument_errors_and_the_optional_pinned_word():
    lib, stream = Gpu.lib()
    acc = torch.rand(64, device="cuda")
    i32 = torch.zeros((2, 64), dtype=torch.int32, device="cuda")
    n_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
    for tau, n, count in ((1.0, 64, n_dev), (-0.1, 64, n_dev), (0.5, -1, n_dev), (0.5, 64, None)):
        assert lib.scnerf_ray_compact(_ptr(acc), tau, _ptr(i32[0]), _ptr(i32[1]), _ptr(count), None, n, stream) == EINVAL
    assert lib.scnerf_ray_compact(_ptr(acc), 0.5, _ptr(i32[0]), _ptr(i32[1]), _ptr(n_dev), None, 64, stream) == 0
    assert int(n_dev.cpu()[0]) == int((acc.cpu() > 0.5).sum())


def test_wrappers_on_tensors():
    """ops.ray_compact / ray_rows_gather / ray_expand: the same numbers through the typed wrappers"""
    from scnerf_amd import ops
    n, s_tot, s_fine = 1000, 40, 24
    acc, tau = C.make(n, "nan_and_ties")
    live, slot_of = C.reference(acc, tau)
    ops.skip_empty_stats(reset=True)
    live_idx, slots, n_live = ops.ray_compact(_dev(acc), tau)
    assert n_live == live.shape[0] and ops.skip_empty_stats(reset=True) == {"rays": n, "skipped": n - n_live}
    assert np.array_equal(live_idx[:n_live].cpu().numpy(), live) and np.array_equal(slots.cpu().numpy(), slot_of)
    src = torch.randn(n, 11, device="cuda")
    assert torch.equal(ops.ray_rows_gather(src, live_idx, n_live), src[torch.from_numpy(live).long().cuda()])
    g = torch.Generator().manual_seed(0)
    fine = [torch.randn(s, generator=g) for s in [(n_live, 3), (n_live,), (n_live,), (n_live,), (n_live,), (n_live, s_tot, 4),
                                                   (n_live, s_tot), (n_live, s_fine)]]
    coarse = [torch.randn(s, generator=g) for s in [(n, 3), (n,), (n,), (n,)]]
    got = ops.ray_expand(slots, n_live, [t.cuda() for t in fine], [t.cuda() for t in coarse], s_tot, s_fine)
    want = C.expand_reference(slot_of, live, [t.numpy() for t in fine], [t.numpy() for t in coarse], s_tot, s_fine)
    for a, b in zip(got, want):
        assert a.cpu().numpy().tobytes() == b.tobytes()
    with pytest.raises(ValueError):
        ops.ray_expand(slots, n_live, [t.cuda() for t in fine[:7]] + [fine[7][:, :-1].contiguous().cuda()],
                       [t.cuda() for t in coarse], s_tot, s_fine)
