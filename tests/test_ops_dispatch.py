"""Which library entry the four resident launchers of scnerf_amd/ops.py call, and with which guard arguments and lean
flag: the launchers run on CPU tensors against a recording stand-in for the library (the three patches of
tests/emu/host_on_emu.py), so nothing is computed -- every device entry is written down as (name, args) and returns 0, the
host-only functions go to the real library.  Smallest legal shapes: 2 rays x 64 samples for the coarse stage, 2 x (64 + 64)
for the fine stage, P = 128 for mlp_fwd / mlp_bwd with 3-D and 4-D points."""
import ctypes
import os

import pytest
import torch

from scnerf_amd import _capi, ops
from scnerf_amd import mlp_layout as ML

HOST_ONLY = set(_capi.SIZE_FUNCS) | {"scnerf_wgrad256_chunks", "scnerf_wgrad_arithmetic", "scnerf_abi_version",
                                     "scnerf_mlp_layout_info"}
NULLS = (None, None, None)


class Recorder:
    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if name in HOST_ONLY:
            return getattr(self.real, name)
        if name not in _capi.PROTOTYPES:
            raise AttributeError(name)

        def entry(*args):
            assert len(args) == len(_capi.PROTOTYPES[name]), (name, len(args))
            self.calls.append((name, args))
            return 0
        return entry


@pytest.fixture(scope="module")
def real_lib():
    if not os.path.isfile(_capi.LIB_PATH):
        from scnerf_amd.csrc import build
        build.build(verbose=False)
    return _capi.bind(ctypes.CDLL(_capi.LIB_PATH))


@pytest.fixture
def rec(real_lib, monkeypatch):
    r = Recorder(real_lib)
    monkeypatch.setattr(_capi, "_lib", r)
    monkeypatch.setattr(_capi, "on_device", lambda t: True)
    monkeypatch.setattr(_capi, "current_stream", lambda: None)
    mode, last = ops.resident_guard(), dict(ops._GUARD_LAST)
    yield r
    ops.resident_guard(mode)
    ops._GUARD_LAST.clear()
    ops._GUARD_LAST.update(last)


def weights(pd, fast=False):
    """resident weights and packed tables of the right sizes (their contents are never read)"""
    rw = ops.ResidentWeights(torch.zeros(512, dtype=torch.int16), torch.zeros(512, dtype=torch.int16), torch.zeros(64), pd)
    rw.fast = fast
    lay = ML.layout(pd)
    return rw, torch.zeros(lay.fwd_total), torch.zeros(lay.bwd_total)


def record(P, mode="fallback"):
    """(forward record, data-gradient record) of one pass of P samples in guard mode `mode`"""
    ops.resident_guard(mode)
    g = ops.guard_records("cpu", [("pass", P)])
    return g["pass"], g["pass_bwd"]


# each launcher: (guard, lean, training, weights, n) -> the recorded calls; n = rays (the stages) or samples (mlp_*)
def run_mlp_fwd(pd):
    def run(guard, lean, train, rw_w, P=128):
        rw, wf, _ = rw_w
        save = ops.save_workspace(P, "cpu", pd) if train else None
        mx = ops.ChunkMaxima(P, "cpu") if train else None
        raw = ops.mlp_fwd_resident(torch.rand(P, pd), torch.rand(max(P // 64, 1), 3), 64, wf, rw, save, mx, guard, lean=lean)
        assert raw.shape == (P, 4)
    return run


def run_mlp_bwd(pd):
    def run(guard, lean, train, rw_w, P=128):
        rw, _, wb = rw_w
        mx = ops.ChunkMaxima(P, "cpu")
        grads, d_pts, d_views = ops.mlp_bwd_resident(torch.rand(P, 4), torch.rand(P, pd), torch.rand(max(P // 64, 1), 3), 64, wb, rw,
                                                     ops.save_workspace(P, "cpu", pd), mx, True, guard, lean=lean)
        assert d_pts.shape == (P, pd) and d_views.shape == (P, 3) and mx.scales is rw.scales
    return run


def run_coarse(guard, lean, train, rw_w, n=2):
    rw, wf, _ = rw_w
    save = ops.save_workspace(n * 64, "cpu") if train else None
    mx = ops.ChunkMaxima(n * 64, "cpu") if train else None
    out = ops.coarse_stage_fwd(torch.rand(n, 11), torch.linspace(0, 1, 64), None, False, wf, save, None, False, planes=rw,
                               maxima=mx, guard=guard, lean=lean)
    assert len(out) == 8 and out[2].shape == (n, 64, 4) and out[6].shape == (n, 64)


def run_fine(guard, lean, train, rw_w, n=2):
    assert guard is None                                  # (the fused fine stage takes no record)
    rw, wf, _ = rw_w
    save = ops.save_workspace(n * 128, "cpu") if train else None
    mx = ops.ChunkMaxima(n * 128, "cpu") if train else None
    out = ops.fine_stage_fwd(torch.rand(n, 11), torch.rand(n, 64), torch.rand(n, 64), torch.rand(n, 64), wf, save, None, False,
                             rw, maxima=mx, lean=lean)
    assert len(out) == 12 and out[6].shape == (n, 128, 4) and out[11] is None


# launcher id -> (runner, pd, entry, gated rerun entry, whether it leaves a forward record)
LAUNCHERS = {
    "mlp_fwd": (run_mlp_fwd(3), 3, "scnerf_mlp_fwd_h3_lean", "scnerf_mlp_fwd_gated", True),
    "mlp_fwd/pd4": (run_mlp_fwd(4), 4, "scnerf_mlp_fwd_h3_lean", "scnerf_mlp_fwd_gated", True),
    "coarse_stage_fwd": (run_coarse, 3, "scnerf_coarse_stage_fwd_h3_lean", "scnerf_coarse_stage_fwd_gated", True),
    "fine_stage_fwd": (run_fine, 3, "scnerf_fine_stage_fwd_h3_lean", None, True),
    "mlp_bwd": (run_mlp_bwd(3), 3, "scnerf_mlp_bwd_h3_lean", "scnerf_mlp_bwd_gated", False),
    "mlp_bwd/pd4": (run_mlp_bwd(4), 4, "scnerf_mlp_bwd_h3_lean", "scnerf_mlp_bwd_gated", False),
}
GUARDED = [k for k, v in LAUNCHERS.items() if v[3] is not None]        # (the fused fine stage takes no guard record)
FORWARD = [k for k, v in LAUNCHERS.items() if v[4]]


@pytest.mark.parametrize("lean", [False, True])
@pytest.mark.parametrize("launcher,guarded", [(k, False) for k in LAUNCHERS] + [(k, True) for k in GUARDED])
def test_one_entry_with_the_guard_arguments_and_the_lean_flag(rec, launcher, guarded, lean):
    run, pd, entry, gated, forward = LAUNCHERS[launcher]
    guard = record(128)[0 if forward else 1] if guarded else None
    run(guard, lean, True, weights(pd))
    name, args = rec.calls[0]
    assert name == entry
    # (flags, any, report: a "fallback" record has no report)
    assert args[-5:-2] == ((guard.flags.data_ptr(), guard.any.data_ptr(), None) if guarded else NULLS)
    assert args[-2] == int(lean) and type(args[-2]) is int and args[-1] is None
    # a "fallback" record with blocks: the gated exact-fp32 launch follows, on the record's flags, and nothing else
    assert [c[0] for c in rec.calls[1:]] == ([gated] if guarded else [])
    if guarded:
        assert rec.calls[1][1][-3:] == (guard.flags.data_ptr(), 0, None)
        assert ops._GUARD_LAST[guard.name] is guard


@pytest.mark.parametrize("launcher", FORWARD)
def test_forward_only_launch_is_not_lean_and_leaves_no_maxima(rec, launcher):
    run, pd, entry = LAUNCHERS[launcher][:3]
    run(None, False, False, weights(pd))
    (name, args), = rec.calls
    assert name == entry and args[-5:-2] == NULLS and args[-2] == 0
    assert args[-8:-5] == (None, 0, 0)                    # chunk maxima, chunks, chunk samples


@pytest.mark.parametrize("launcher,entry", [("mlp_fwd", "scnerf_mlp_fwd_h3_fast"), ("mlp_fwd/pd4", "scnerf_mlp_fwd_h3_fast"),
                                            ("coarse_stage_fwd", "scnerf_coarse_stage_fwd_h3_fast")])
def test_fast_packs_take_the_one_product_entry(rec, launcher, entry):
    run, pd = LAUNCHERS[launcher][:2]
    run(None, False, False, weights(pd, fast=True))
    (name, args), = rec.calls
    assert name == entry and args[-4:] == (None, 0, 0, None)          # no maxima, no guard arguments, no lean flag
    with pytest.raises(ValueError, match="forward-only and takes no guard record"):
        run(record(128)[0], False, False, weights(pd, fast=True))
    with pytest.raises(ValueError, match="forward-only and takes no guard record"):
        run(None, False, True, weights(pd, fast=True))
    assert len(rec.calls) == 1


def test_fast_packs_have_no_fused_fine_stage_and_no_lean_pass(rec):
    with pytest.raises(ValueError, match="no one-product instantiation"):
        run_fine(None, False, False, weights(3, fast=True))
    with pytest.raises(ValueError, match="lean workspace needs a training pass on three-product packs"):
        LAUNCHERS["mlp_bwd"][0](None, True, True, weights(3, fast=True))
    assert rec.calls == []


@pytest.mark.parametrize("n", [1, 0], ids=["blocks", "no_blocks"])
@pytest.mark.parametrize("mode", ["fallback", "strict"])
@pytest.mark.parametrize("launcher", GUARDED)
def test_gated_rerun_follows_exactly_when_the_record_has_blocks(rec, launcher, mode, n):
    run, pd, entry, gated, forward = LAUNCHERS[launcher]
    size = n * (128 if "mlp" in launcher else 2)          # samples for mlp_*, rays for the coarse stage
    guard = record(size if "mlp" in launcher else size * 64, mode)[0 if forward else 1]
    assert guard.mode == mode and (guard.blocks > 0) == (n > 0)
    run(guard, False, True, weights(pd), size)
    assert rec.calls[0][0] == entry and rec.calls[0][1][-5:-2] == guard.args() and rec.calls[0][1][-2] == 0
    assert (rec.calls[0][1][-3] is not None) == (mode == "strict")          # (the report: "report" and "strict" alone)
    # "fallback": the gated launch when there is a block to run again; "strict": never (it reads the record and raises)
    assert [c[0] for c in rec.calls[1:]] == ([gated] if (mode == "fallback" and n > 0) else [])
    assert ops._GUARD_LAST[guard.name] is guard


def test_strict_raises_on_a_tripped_record(rec):
    guard = record(128, "strict")[0]
    guard.any.fill_(1)
    guard.flags.fill_(1)
    with pytest.raises(ops.ResidentRangeError):
        LAUNCHERS["mlp_fwd"][0](guard, False, True, weights(3))
    assert [c[0] for c in rec.calls] == ["scnerf_mlp_fwd_h3_lean"]


@pytest.mark.parametrize("pd", [3, 4])
def test_public_wrappers_route_resident_weights_to_the_resident_launchers(rec, pd):
    rw, wf, wb = weights(pd)
    P = 128
    pts, vd, save = torch.rand(P, pd), torch.rand(2, 3), ops.save_workspace(P, "cpu", pd)
    ops.mlp_fwd(pts, vd, 64, wf, save, pd=pd, planes=rw)
    ops.mlp_bwd(torch.rand(P, 4), pts, vd, 64, wb, save, pd=pd, planes=rw)
    ops.mlp_fwd(pts, vd, 64, wf, save, pd=pd)
    ops.mlp_bwd(torch.rand(P, 4), pts, vd, 64, wb, save, pd=pd)
    assert [c[0] for c in rec.calls] == ["scnerf_mlp_fwd_h3_lean", "scnerf_mlp_bwd_h3_lean", "scnerf_mlp_fwd", "scnerf_mlp_bwd"]
    assert all(c[1][0] == pd for c in rec.calls)
    other = weights(7 - pd)[0]
    for call in (lambda: ops.mlp_fwd(pts, vd, 64, wf, save, pd=pd, planes=other),
                 lambda: ops.mlp_bwd(torch.rand(P, 4), pts, vd, 64, wb, save, pd=pd, planes=other)):
        with pytest.raises(ValueError, match="another network variant"):
            call()
    # the shared argument checks, with their messages
    for wrong, match in ((lambda: ops.mlp_fwd(pts, vd, 64, wf[1:], save, pd=pd, planes=rw), "wpacked has the wrong size"),
                         (lambda: ops.mlp_fwd(pts, vd, 64, wf, save[1:], pd=pd), "activation workspace too small"),
                         (lambda: ops.mlp_bwd(torch.rand(P, 4), pts, vd, 64, wb[1:], save, pd=pd, planes=rw),
                          "wpacked_bwd has the wrong size"),
                         (lambda: ops.mlp_bwd(torch.rand(P, 4), pts, vd, 64, wf, save, pd=pd), "wpacked_bwd has the wrong size")):
        with pytest.raises(ValueError, match=match):
            wrong()
    with pytest.raises(TypeError, match="viewdirs must be a CUDA fp32"):
        ops.mlp_fwd(pts, vd.double(), 64, wf, save, pd=pd, planes=rw)
    assert len(rec.calls) == 4
