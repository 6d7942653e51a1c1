"""csrc/ray_compact.hip under the CPU SIMT interpreter, through the C ABI on numpy buffers: scnerf_ray_compact against
np.flatnonzero(~(acc <= tau)), scnerf_ray_rows_gather against fancy indexing, scnerf_ray_expand against a numpy scatter --
all for equality, twice for identical bytes (tests/ray_compact_cases.py; the GPU twin is tests/test_gpu_ray_compact.py and
goes on to 70 001 rays).  Then the argument errors."""
import numpy as np
import pytest

from tests import ray_compact_cases as C
from tests.emu import harness as H

pytestmark = pytest.mark.emu
EINVAL = -22


class Emu:
    @staticmethod
    def compact(acc, tau):
        n = acc.shape[0]
        live_idx = np.full(n, C.SENTINEL, np.int32)
        slot_of = np.full(n, C.SENTINEL, np.int32)
        n_dev, n_host = np.full(1, C.SENTINEL, np.int32), np.full(1, C.SENTINEL, np.int32)
        H.call("scnerf_ray_compact", acc, tau, live_idx, slot_of, n_dev, n_host, n, None)
        return live_idx, slot_of, int(n_dev[0]), int(n_host[0])

    @staticmethod
    def gather(src, live, w):
        dst = np.full((live.shape[0], w), np.nan, np.float32)
        H.call("scnerf_ray_rows_gather", src, live, dst, live.shape[0], w, src.shape[0], None)
        return dst

    @staticmethod
    def expand(slot_of, n_live, fine, coarse, s_tot, s_fine):
        n = slot_of.shape[0]
        outs = [np.full(s, np.nan, np.float32) for s in [(n, 3), (n,), (n,), (n,), (n,), (n, s_tot, 4), (n, s_tot), (n, s_fine)]]
        H.call("scnerf_ray_expand", slot_of, n, n_live, s_tot, s_fine, *fine, *coarse, *outs, None)
        return outs


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("n", [n for n in C.SIZES if n <= 1025])
def test_compact_gather_expand_equal_numpy(n, kind):
    C.check_all(Emu, n, kind)


def test_argument_errors():
    acc, tau = C.make(64, "random")
    i32 = np.zeros(64, np.int32)
    one = np.zeros(1, np.int32)
    st = H.lib_call_status
    assert st("scnerf_ray_compact", acc, tau, i32, i32.copy(), one, one.copy(), -1, None) == EINVAL
    assert st("scnerf_ray_compact", acc, 1.0, i32, i32.copy(), one, one.copy(), 64, None) == EINVAL
    assert st("scnerf_ray_compact", acc, -0.1, i32, i32.copy(), one, one.copy(), 64, None) == EINVAL
    assert st("scnerf_ray_compact", acc, float("nan"), i32, i32.copy(), one, one.copy(), 64, None) == EINVAL
    assert st("scnerf_ray_compact", acc, tau, i32, i32.copy(), None, one, 64, None) == EINVAL
    assert st("scnerf_ray_compact", None, tau, i32, i32.copy(), one, one.copy(), 64, None) == EINVAL
    # (the pinned word is optional)
    assert st("scnerf_ray_compact", acc, tau, i32, i32.copy(), one, None, 64, None) == 0
    src, dst = np.zeros((64, 3), np.float32), np.zeros((64, 3), np.float32)
    assert st("scnerf_ray_rows_gather", src, i32, dst, 64, 0, 64, None) == EINVAL
    assert st("scnerf_ray_rows_gather", src, i32, dst, 65, 3, 64, None) == EINVAL
    assert st("scnerf_ray_rows_gather", None, i32, dst, 64, 3, 64, None) == EINVAL
    f = [np.zeros(s, np.float32) for s in [(4, 3), (4,), (4,), (4,), (4,), (4, 8, 4), (4, 8), (4, 3)]]
    c = [np.zeros(s, np.float32) for s in [(4, 3), (4,), (4,), (4,)]]
    o = [a.copy() for a in f]
    slot = np.arange(4, dtype=np.int32)
    assert st("scnerf_ray_expand", slot, 4, 5, 8, 3, *f, *c, *o, None) == EINVAL          # more live rays than rays
    assert st("scnerf_ray_expand", slot, 4, 4, 8, 9, *f, *c, *o, None) == EINVAL          # s_fine > s_tot
    assert st("scnerf_ray_expand", slot, 4, 4, 8, 3, *([None] + f[1:]), *c, *o, None) == EINVAL
    assert st("scnerf_ray_expand", slot, 4, 4, 8, 3, *f, *c, *(o[:7] + [None]), None) == EINVAL
    assert st("scnerf_ray_expand", slot, 4, 4, 8, 3, *f, *c, *o, None) == 0


def test_a_slot_outside_the_live_batch_is_a_skipped_ray():
    """the expansion follows no index it cannot check: slot_of >= n_live reads nothing of the live arrays"""
    f = [np.ones(s, np.float32) for s in [(1, 3), (1,), (1,), (1,), (1,), (1, 8, 4), (1, 8), (1, 3)]]
    c = [np.full(s, 2.0, np.float32) for s in [(3, 3), (3,), (3,), (3,)]]
    o = [np.full(s, np.nan, np.float32) for s in [(3, 3), (3,), (3,), (3,), (3,), (3, 8, 4), (3, 8), (3, 3)]]
    H.call("scnerf_ray_expand", np.array([0, 1, -1], np.int32), 3, 1, 8, 3, *f, *c, *o, None)
    assert (o[0][0] == 1).all() and (o[0][1:] == 2).all()
    assert (o[5][0] == 1).all() and (o[5][1:] == 0).all() and (o[4] == [1, 0, 0]).all()
