"""The scale guard of the resident arithmetic (csrc/resident_guard.h) on the CPU SIMT interpreter: a guarded launch computes
bit for bit what the unguarded one does, its per-layer margins follow the host rule of tests/trained_weights.py, and it
trips on a network whose scale bound is too loose and on no other."""
import numpy as np
import pytest
import torch

from scnerf_amd import mlp_layout as ML
from tests import hostile_weights, trained_weights
from tests.emu import harness as H
from tests.emu_mlp_util import network_params, pack_backward, pack_forward, pack_h3

pytestmark = pytest.mark.emu

NL, SLOTS, BIAS = 10, 64, 256          # csrc/resident_guard.h


def _inputs(P, spr, pd, seed=3):
    g = torch.Generator().manual_seed(seed)
    pts = torch.rand(P, pd, generator=g) * 3 - 1.5
    vd = torch.randn(P // spr, 3, generator=g)
    vd = vd / vd.norm(dim=-1, keepdim=True)
    d_raw = torch.randn(P, 4, generator=g)
    return pts.numpy(), vd.numpy(), d_raw.numpy()


def _record(P):
    return np.zeros((P + 127) // 128, np.int32), np.zeros(1, np.int32), np.zeros(NL * (SLOTS + 2), np.float32)


def _margins(report):
    best = report[:NL * SLOTS].reshape(NL, SLOTS).max(1)
    counts = report[NL * SLOTS:].reshape(NL, 2)
    return [None if b == 0 else BIAS - int(b) for b in best], counts


def _run(p, pd, P, spr, guarded):
    """(raw, save, chunk maxima x, grads, d_pts, d_views, chunk maxima z, forward record, backward record)"""
    lay = ML.layout(pd)
    wpk, wbk = pack_forward(p, pd), pack_backward(p, pd)
    fwd, bwd, sc = pack_h3(p, pd)
    pts, vd, d_raw = _inputs(P, spr, pd)
    n_chunks, chunk = 2, 64
    raw = np.full((P, 4), np.nan, np.float32)
    save = np.full(lay.save_floats(P), np.nan, np.float32)
    amx = np.zeros((12, n_chunks), np.float32)
    rf = _record(P) if guarded else (None, None, None)
    head = (pd, pts, vd, 3, spr, wpk, fwd, sc, raw, save, P, amx, n_chunks, chunk)
    if guarded:
        H.call("scnerf_mlp_fwd_h3_guarded", *head, *rf, None)
    else:
        H.call("scnerf_mlp_fwd_h3", *head, None)
    grads = np.full(ML.grad_floats(P), np.nan, np.float32)
    d_pts = np.full((P, pd), np.nan, np.float32)
    d_views = np.full((P, 3), np.nan, np.float32)
    amz = np.zeros((12, n_chunks), np.float32)
    rb = _record(P) if guarded else (None, None, None)
    head = (pd, d_raw, pts, vd, 3, spr, wbk, bwd, sc, save, grads, d_pts, d_views, P, amz, n_chunks, chunk)
    if guarded:
        H.call("scnerf_mlp_bwd_h3_guarded", *head, *rb, None)
    else:
        H.call("scnerf_mlp_bwd_h3", *head, None)
    return dict(raw=raw, save=save, amx=amx, grads=grads, d_pts=d_pts, d_views=d_views, amz=amz, fwd=rf, bwd=rb, sc=sc, pts=pts)


@pytest.mark.parametrize("pd,n_rays,spr", [(3, 2, 70), (4, 3, 15)])
def test_guarded_launches_compute_the_same_numbers(pd, n_rays, spr):
    p = network_params(0 if pd == 3 else 777, pd)
    P = n_rays * spr
    a = _run(p, pd, P, spr, guarded=False)
    b = _run(p, pd, P, spr, guarded=True)
    for k in ("raw", "save", "amx", "grads", "d_pts", "d_views", "amz"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    # xavier weights, inputs of the suite's size: nothing trips, every layer reports a margin inside the range
    for rec in (b["fwd"], b["bwd"]):
        flags, any_, report = rec
        assert not flags.any() and any_[0] == 0
        mins, counts = _margins(report)
        assert not counts.any()
        assert all(m is not None and -3 <= m < 13 for m in mins), mins


def test_forward_margins_follow_the_host_rule():
    p = network_params(0)
    P, spr = 140, 70
    r = _run(p, 3, P, spr, guarded=True)
    mins, _ = _margins(r["fwd"][2])

    class Planes:
        scales = torch.from_numpy(r["sc"])
    host = trained_weights.scale_margins(None, Planes, torch.from_numpy(r["save"]), P, torch.from_numpy(r["pts"]))
    for l in range(8):
        assert mins[l] == int(np.floor(host["layer_%d" % l]["log2_min"])), (l, mins[l], host["layer_%d" % l])


def test_hostile_network_trips_every_block_at_layer_3():
    p = hostile_weights.weights(0)
    P, spr = 192, 64
    r = _run(p, 3, P, spr, guarded=True)
    flags, any_, report = r["fwd"]
    assert flags.tolist() == [1, 1] and any_[0] == 1
    mins, counts = _margins(report)
    assert mins[3] <= -6, mins
    assert counts[3, 0] == P and counts[3, 1] == 0          # every live sample under the range at layer 3
    # the outputs are still the unguarded kernel's
    q = _run(p, 3, P, spr, guarded=False)
    assert np.array_equal(q["raw"].view(np.uint32), r["raw"].view(np.uint32))


def test_guarded_launches_reject_half_a_record():
    p = network_params(0)
    P = 32
    wpk = pack_forward(p)
    fwd, _, sc = pack_h3(p, directions=("fwd",))
    pts, vd, _ = _inputs(P, 32, 3)
    raw = np.zeros((P, 4), np.float32)
    flags, _, report = _record(P)
    any_ = np.zeros(1, np.int32)
    for rec in ((flags, None, report), (None, any_, None), (None, None, report)):      # flags without any, and back; report alone
        st = H.lib_call_status("scnerf_mlp_fwd_h3_guarded", 3, pts, vd, 3, 32, wpk, fwd, sc, raw, None, P, None, 0, 0, *rec, None)
        assert st != 0, rec


# ---- the gated exact-fp32 re-run ----------------------------------------------------------------------------------------
def _fp32_forward(p, P, spr, flags=None, wgs=0):
    lay = ML.layout(3)
    wpk = pack_forward(p)
    pts, vd, _ = _inputs(P, spr, 3)
    raw = np.full((P, 4), np.nan, np.float32)
    save = np.full(lay.save_floats(P), np.nan, np.float32)
    if flags is None:
        H.call("scnerf_mlp_fwd", 3, pts, vd, 3, spr, wpk, raw, save, P, None)
    else:
        H.call("scnerf_mlp_fwd_gated", 3, pts, vd, 3, spr, wpk, raw, save, P, flags, wgs, None)
    return raw, save


def _only_flagged(got, ref, flags, rows_per_block):
    """rows of flagged blocks bit-identical to the ungated kernel's, every other row untouched (NaN)"""
    for b, f in enumerate(flags):
        sl = slice(b * rows_per_block, (b + 1) * rows_per_block)
        if f:
            assert np.array_equal(got[sl].view(np.uint32), ref[sl].view(np.uint32)), b
        else:
            assert np.isnan(got[sl]).all(), b


def test_gated_forward_with_no_flag_writes_nothing():
    p = network_params(0)
    raw, save = _fp32_forward(p, 300, 60, flags=np.zeros(3, np.int32), wgs=2)
    assert np.isnan(raw).all() and np.isnan(save).all()


def test_gated_forward_runs_exactly_the_flagged_blocks():
    p = network_params(0)
    P, spr = 300, 60
    ref_raw, ref_save = _fp32_forward(p, P, spr)
    flags = np.array([1, 0, 1], np.int32)
    raw, save = _fp32_forward(p, P, spr, flags=flags, wgs=1)            # one workgroup walks all three blocks
    _only_flagged(raw, ref_raw, flags, 128)
    done = ~np.isnan(save)
    assert done.any() and np.array_equal(save[done].view(np.uint32), ref_save[done].view(np.uint32))


def test_gated_data_gradients_run_exactly_the_flagged_blocks():
    p = network_params(2)
    P, spr = 300, 60
    wbk = pack_backward(p)
    _, save = _fp32_forward(p, P, spr)
    pts, vd, d_raw = _inputs(P, spr, 3)

    def run(flags):
        grads = np.full(ML.grad_floats(P), np.nan, np.float32)
        d_pts = np.full((P, 3), np.nan, np.float32)
        d_views = np.full((P, 3), np.nan, np.float32)
        if flags is None:
            H.call("scnerf_mlp_bwd", 3, d_raw, pts, vd, 3, spr, wbk, save, grads, d_pts, d_views, P, None)
        else:
            H.call("scnerf_mlp_bwd_gated", 3, d_raw, pts, vd, 3, spr, wbk, save, grads, d_pts, d_views, P, flags, 2, None)
        return grads, d_pts, d_views
    ref = run(None)
    flags = np.array([0, 1, 1], np.int32)
    got = run(flags)
    _only_flagged(got[1], ref[1], flags, 128)
    _only_flagged(got[2], ref[2], flags, 128)
    done = ~np.isnan(got[0])
    assert done.any() and np.array_equal(got[0][done].view(np.uint32), ref[0][done].view(np.uint32))
    none = run(np.zeros(3, np.int32))
    assert all(np.isnan(x).all() for x in none)


def test_gated_coarse_stage_runs_exactly_the_flagged_blocks():
    from scnerf_amd import synthetic as synth
    p = network_params(0)
    wpk = pack_forward(p)
    n = 6                                                   # 3 blocks of two rays
    rays = synth.ray_batch(n, seed=5).numpy()
    rnd = synth.render_randoms(n, 64, 8, seed=7)
    t_vals = np.linspace(0, 1, 64, dtype=np.float32)
    t_rand, noise = rnd["t_rand"].numpy(), rnd["noise_c"].numpy()

    def run(flags):
        out = dict(z=np.full((n, 64), np.nan, np.float32), pts=np.full((n, 64, 3), np.nan, np.float32),
                   raw=np.full((n, 64, 4), np.nan, np.float32), rgb=np.full((n, 3), np.nan, np.float32),
                   disp=np.full(n, np.nan, np.float32), acc=np.full(n, np.nan, np.float32),
                   depth=np.full(n, np.nan, np.float32), w=np.full((n, 64), np.nan, np.float32))
        args = (rays, rays.shape[1], t_vals, t_rand, 0, wpk, None, noise, 0, out["z"], out["pts"], out["raw"], out["rgb"],
                out["disp"], out["acc"], out["depth"], out["w"], n, 64)
        if flags is None:
            H.call("scnerf_coarse_stage_fwd", *args, None)
        else:
            H.call("scnerf_coarse_stage_fwd_gated", *args, flags, 1, None)
        return out
    ref = run(None)
    flags = np.array([0, 1, 0], np.int32)
    got = run(flags)
    for k in ref:
        _only_flagged(got[k], ref[k], flags, 2)
