"""The lean workspace (ops.lean_workspace, csrc/wgrad.hip) against the full one on the MI355X.

feature_linear has no activation, so with M = sum_p dZv_p act7_p^T and s = sum_p dZv_p the gradients of feature_linear and of
the feature columns of views_linears.0 follow from one views-layer GEMM; a lean pass stores neither `feature` nor `d feature`
and runs seven 256 x 256 weight-gradient GEMMs instead of eight.  Everything the lean pass still writes must be the full
pass's bits; the three derived tensors are judged against fp64 with the exact-fp32-MFMA group as the yardstick.

K = 4: lean error <= K x the fp32 group's error, per tensor, error = largest |difference to fp64| over the tensor's largest
entry.  Ratios measured on the MI355X over this file's cases (P = 300, P = 40 000, the step's fine and coarse pass):
feature_linear.weight 0.20 - 1.38, views_linears.0.weight[:, :256] 0.54 - 0.90, feature_linear.bias 1.51 - 3.07 (errors of
6e-8 .. 4.4e-7 on either side; the bias's yardstick is a plain fp32 sum, 4e-8 .. 1.3e-7).  Largest: 3.07; K is the next power
of two above it.  A ratio above 4 would have meant "do not make lean the default"."""
import numpy as np
import pytest
import torch

from scnerf_amd import mlp_layout as ML
from scnerf_amd import synthetic as synth

pytestmark = pytest.mark.gpu

K = 4.0                        # the next power of two above the largest measured ratio, 3.07 (see the docstring)

SC, SF = 64, 128
OFF = ML.PARAM_OFFSETS
DERIVED = ("feature_linear.weight", "feature_linear.bias", "views_linears.0.weight[:, :256]")
CASES = {300: (6, 50), 40000: (200, 200)}      # P -> (rays, samples per ray): a partial 128-block; several chunks per job


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from scnerf_amd import ops as _ops
    _ops.check_layout()
    return _ops


@pytest.fixture
def modes(ops):
    before = (ops.lean_workspace(), ops.wgrad_arithmetic(), ops.mlp_arithmetic())
    if before[2] != "resident":
        pytest.skip("the lean workspace is the resident arithmetic's")
    ops.wgrad_arithmetic("half")
    yield ops
    ops.lean_workspace(before[0])
    ops.wgrad_arithmetic(before[1])


def _words(t):
    return t.contiguous().view(torch.int32).cpu()


def _derived_mask():
    """True where the flat gradient holds one of the three derived tensors"""
    m = np.zeros(ML.layout(3).n_params, bool)
    m[OFF["feature_linear.weight"]:OFF["feature_linear.weight"] + 256 * 256] = True
    m[OFF["feature_linear.bias"]:OFF["feature_linear.bias"] + 256] = True
    m[OFF["views_linears.0.weight"]:OFF["views_linears.0.weight"] + 128 * 283].reshape(128, 283)[:, :256] = True
    return m


def _derived(flat):
    flat = np.asarray(flat)
    wv = flat[OFF["views_linears.0.weight"]:OFF["views_linears.0.weight"] + 128 * 283].reshape(128, 283)
    return {DERIVED[0]: flat[OFF["feature_linear.weight"]:OFF["feature_linear.weight"] + 256 * 256].reshape(256, 256),
            DERIVED[1]: flat[OFF["feature_linear.bias"]:OFF["feature_linear.bias"] + 256],
            DERIVED[2]: wv[:, :256]}


def _fp64_reference(save, grads, P):
    """the three derived gradients as direct fp64 sums over the samples, from a FULL pass's saved sections"""
    Pp = ML.padded_samples(P)
    so, _ = ML.section_offsets(ML.layout(3).save_sections, P)
    go, _ = ML.section_offsets(ML.GRAD_SECTIONS, P)

    def rows(buf, o, w):        # (only the four sections the sums need leave the device)
        return ML.untile(buf[o:o + w * Pp].cpu().numpy(), w, P).astype(np.float64)
    act7, feat = rows(save, so["act7"], 256), rows(save, so["feat"], 256)
    dzv, dfeat = rows(grads, go["dzv"], 128), rows(grads, go["dfeat"], 256)
    return {DERIVED[0]: dfeat.T @ act7, DERIVED[1]: dfeat.sum(0), DERIVED[2]: dzv.T @ feat}


def _errors(flat, ref):
    got = _derived(flat)
    return {k: float(np.abs(got[k] - ref[k]).max() / np.abs(ref[k]).max()) for k in DERIVED}


def _judge(what, lean_flat, yard_flat, ref):
    e_lean, e_yard = _errors(lean_flat, ref), _errors(yard_flat, ref)
    ratios = {k: e_lean[k] / e_yard[k] for k in DERIVED}
    for k in DERIVED:
        print("[lean] %s %s: lean %.3e fp32-MFMA %.3e ratio %.2f" % (what, k, e_lean[k], e_yard[k], ratios[k]))
    for k in DERIVED:
        assert e_lean[k] <= K * e_yard[k], (what, k, e_lean[k], e_yard[k])
    return ratios


# ---- the kernels and the weight-gradient group, lean against full -------------------------------------------------------
@pytest.fixture(scope="module")
def passes(ops):
    """per P: the forward, the data gradients (both input_grad settings) and the weight-gradient groups of a full and a
    lean pass on the same inputs, computed once"""
    from tests.emu_mlp_util import network_params
    if ops.mlp_arithmetic() != "resident":
        pytest.skip("the lean workspace is the resident arithmetic's")
    before = (ops.wgrad_arithmetic(),)
    ops.wgrad_arithmetic("half")
    lay = ML.layout(3)
    p = network_params(4, 3)
    flat = torch.cat([p[name].reshape(-1) for name, _ in lay.param_shapes]).contiguous().cuda()
    wf, wb, rw = ops.pack_weights(flat, "fwd"), ops.pack_weights(flat, "bwd"), ops.pack_resident(flat, 3)
    out = {}
    for P, (n_rays, spr) in CASES.items():
        g = torch.Generator().manual_seed(100 + P)
        pts = (torch.rand(P, 3, generator=g) * 2.4 - 1.2).contiguous().cuda()
        vd = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=g), dim=-1).contiguous().cuda()
        d_raw = torch.randn(P, 4, generator=g).contiguous().cuda()
        R = {"P": P, "flat": flat, "pts": pts, "vd": vd, "spr": spr, "wb": wb, "rw": rw}
        for lean in (False, True):
            save = torch.full((lay.save_floats(P),), float("nan"), device="cuda")
            mx = ops.ChunkMaxima(P, "cuda")
            raw = ops.mlp_fwd(pts, vd, spr, wf, save, planes=rw, maxima=mx, lean=lean)
            r = {"raw": raw, "save": save, "mx": mx, "x": mx.x.clone()}
            for ig in (True, False):
                mz = ops.ChunkMaxima(P, "cuda")
                grads, d_pts, d_views = ops.mlp_bwd(d_raw, pts, vd, spr, wb, save, planes=rw, maxima=mz, input_grad=ig, lean=lean)
                r["bwd", ig] = (grads, d_pts, d_views, mz.z.clone())
                if ig:
                    mx.z.copy_(mz.z)
                    mx.scales = mz.scales
                    r["grads"] = grads
            r["wgrad"] = ops.nerf_wgrad(save, r["grads"], d_raw, P, maxima=mx, lean=lean, flat_params=flat if lean else None)
            R[lean] = r
            R["d_raw"] = d_raw
        ops.wgrad_arithmetic("fp32")
        R["yardstick"] = ops.nerf_wgrad(R[False]["save"], R[False]["grads"], d_raw, P, maxima=R[False]["mx"])
        ops.wgrad_arithmetic("half")
        R["ref"] = _fp64_reference(R[False]["save"], R[False]["grads"], P)
        out[P] = R
    ops.wgrad_arithmetic(before[0])
    return out


@pytest.mark.parametrize("P", sorted(CASES))
def test_forward_writes_the_full_pass_bits_except_the_feature_section(passes, P):
    full, lean = passes[P][False], passes[P][True]
    lay = ML.layout(3)
    assert torch.equal(_words(full["raw"]), _words(lean["raw"]))
    assert torch.equal(_words(full["x"]), _words(lean["x"]))                       # the X maxima, row 7 = act7's among them
    off, total = ML.section_offsets(lay.save_sections, P)
    Pp = ML.padded_samples(P)
    sf, sl = _words(full["save"]), _words(lean["save"])
    for name, w in lay.save_sections:
        a, b = sf[off[name]:off[name] + w * Pp], sl[off[name]:off[name] + w * Pp]
        if name == "feat":
            assert bool(torch.isnan(lean["save"][off[name]:off[name] + w * Pp]).all()), "the lean pass wrote the feature section"
            assert not bool(torch.isnan(full["save"][off[name]:off[name] + w * Pp]).any())
        else:
            assert torch.equal(a, b), name
    assert torch.equal(sf[total:], sl[total:])                                      # the ReLU bit masks


@pytest.mark.parametrize("input_grad", [True, False])
@pytest.mark.parametrize("P", sorted(CASES))
def test_data_gradients_write_the_full_pass_bits_except_d_feature(passes, P, input_grad):
    gf, pf, vf, zf = passes[P][False]["bwd", input_grad]
    gl, pl, vl, zl = passes[P][True]["bwd", input_grad]
    off, _ = ML.section_offsets(ML.GRAD_SECTIONS, P)
    Pp = ML.padded_samples(P)
    a, b = _words(gf), _words(gl)
    for name, w in ML.GRAD_SECTIONS:
        if name != "dfeat":
            assert torch.equal(a[off[name]:off[name] + w * Pp], b[off[name]:off[name] + w * Pp]), name
    assert torch.equal(_words(zf), _words(zl))                                      # the Z maxima
    if input_grad:
        assert torch.equal(_words(pf), _words(pl)) and torch.equal(_words(vf), _words(vl))
    else:
        assert pf is None and pl is None and vf is None and vl is None


POISON = 0x7FC0BEEF                 # a quiet NaN no kernel produces: a word still holding it was not written


@pytest.mark.parametrize("input_grad", [True, False])
@pytest.mark.parametrize("P", sorted(CASES))
def test_data_gradients_leave_the_d_feature_section_unwritten(ops, passes, P, input_grad):
    """the data-gradient kernel through the C ABI into a prefilled workspace: with the flag every word of the d feature section
    still holds the fill (the shut store window drops the stores on the device, not only under the interpreter) and every other
    word is the ops-level run's; without it the section is written in full"""
    from scnerf_amd import _capi
    R = passes[P]
    off, _ = ML.section_offsets(ML.GRAD_SECTIONS, P)
    Pp = ML.padded_samples(P)
    lo, hi = off["dfeat"], off["dfeat"] + 256 * Pp
    vptr, vstride = ops._vd(R["vd"])
    for lean in (1, 0):
        grads = torch.full((ML.grad_floats(P),), POISON, dtype=torch.int32, device="cuda")
        d_pts = torch.empty((P, 3), device="cuda") if input_grad else None
        d_views = torch.empty((P, 3), device="cuda") if input_grad else None
        mz = ops.ChunkMaxima(P, "cuda")
        st = _capi.load().scnerf_mlp_bwd_h3_lean(3, ops._p(R["d_raw"]), ops._p(R["pts"]), vptr, vstride, R["spr"], ops._p(R["wb"]),
                                                 ops._p(R["rw"].bwd), ops._p(R["rw"].scales), ops._p(R[bool(lean)]["save"]),
                                                 ops._p(grads), ops._p(d_pts), ops._p(d_views), P, ops._p(mz.z), mz.chunks,
                                                 mz.chunk_samples, None, None, None, lean, ops._stream())
        _capi.check(st, "scnerf_mlp_bwd_h3_lean")
        words = grads.cpu()
        if lean:
            assert bool((words[lo:hi] == POISON).all()), int((words[lo:hi] != POISON).sum())
        else:
            assert not bool((words[lo:hi] == POISON).any())
        want = _words(R[bool(lean)]["bwd", input_grad][0])
        assert not bool((words[:lo] == POISON).any()) and not bool((words[hi:] == POISON).any())
        assert torch.equal(words[:lo], want[:lo]) and torch.equal(words[hi:], want[hi:])


@pytest.mark.parametrize("P", sorted(CASES))
def test_weight_gradients_outside_the_derived_tensors_are_the_full_groups_bits(passes, P):
    a, b = _words(passes[P][False]["wgrad"]).numpy(), _words(passes[P][True]["wgrad"]).numpy()
    keep = ~_derived_mask()
    np.testing.assert_array_equal(a[keep], b[keep])
    o = OFF["views_linears.0.bias"]                    # (the finishing kernel copies s: bit-identical, and inside `keep`)
    np.testing.assert_array_equal(a[o:o + 128], b[o:o + 128])
    assert np.isfinite(passes[P][True]["wgrad"].cpu().numpy()).all()


@pytest.mark.parametrize("P", sorted(CASES))
def test_derived_gradients_against_fp64_with_the_fp32_group_as_yardstick(passes, P):
    R = passes[P]
    _judge("P=%d" % P, R[True]["wgrad"].cpu().numpy(), R["yardstick"].cpu().numpy(), R["ref"])


def test_accumulation_equals_the_sum_of_two_calls(passes, modes):
    ops = modes
    A, B = passes[40000], passes[300]
    g = A[True]["wgrad"].clone()
    r = B[True]
    ops.nerf_wgrad(r["save"], r["grads"], B["d_raw"], B["P"], flat_grad=g, accumulate=True, maxima=r["mx"], lean=True,
                   flat_params=B["flat"])
    assert torch.equal(_words(g), _words(A[True]["wgrad"] + r["wgrad"]))


def test_a_lean_workspace_never_reaches_the_full_group(passes, modes):
    ops = modes
    R = passes[300]
    r = R[True]
    ops.wgrad_arithmetic("fp32")
    with pytest.raises(RuntimeError):
        ops.nerf_wgrad(r["save"], r["grads"], R["d_raw"], R["P"], maxima=r["mx"], lean=True, flat_params=R["flat"])
    ops.wgrad_arithmetic("half")
    with pytest.raises(ValueError):
        ops.nerf_wgrad(r["save"], r["grads"], R["d_raw"], R["P"], maxima=None, lean=True, flat_params=R["flat"])


# ---- one training step, lean on against lean off ------------------------------------------------------------------------
def _nets():
    from scnerf_amd import run_nerf_helpers as H
    out = []
    for seed in (0, 1):
        net = H.NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
        net.load_state_dict(synth.network_params(seed=seed))
        out.append(net.cuda())
    return out


def _step(nets, n, seed=5):
    from scnerf_amd import create_nerf, render, run_nerf_helpers as H
    query = create_nerf.FusedNetworkQuery(H.get_embedder(10, 0)[0], H.get_embedder(4, 0)[0])
    rays = synth.ray_batch(n, seed=seed).cuda().requires_grad_(True)
    rnd = {k: v.cuda() for k, v in synth.render_randoms(n, SC, SF, seed=seed + 1).items()}
    ret = render.render_rays(rays, nets[0], query, SC, retraw=True, perturb=1.0, N_importance=SF, network_fine=nets[1],
                             raw_noise_std=1.0, _randoms=rnd)
    loss = (ret["rgb_map"] ** 2).sum() + (ret["rgb0"] ** 2).sum() + ret["disp_map"].sum() + ret["acc0"].sum()
    params = [list(net.parameters()) for net in nets]
    got = torch.autograd.grad(loss, [rays] + params[0] + params[1])
    n0 = len(params[0])
    flat = [torch.cat([g.reshape(-1) for g in got[1:1 + n0]]), torch.cat([g.reshape(-1) for g in got[1 + n0:]])]
    keys = ("rgb_map", "disp_map", "acc_map", "rgb0", "disp0", "acc0", "raw")
    return {k: ret[k].detach() for k in keys}, flat, got[0].detach()


@pytest.fixture
def fine_stage_route(ops):
    before = ops.fused_fine_stage()
    yield ops.fused_fine_stage
    ops.fused_fine_stage(before)


@pytest.mark.parametrize("fused", [False, True], ids=["three_launches", "fused_fine_stage"])
def test_training_step_lean_on_against_lean_off(modes, monkeypatch, fine_stage_route, fused):
    """256 rays x (64 + 128): rendered outputs, d rays and both networks' flat gradients outside the three tensors bit for
    bit; the three tensors against fp64 sums over the lean-off step's own workspaces, the fp32 group on those workspaces
    as the yardstick.  The coarse pass is the coarse-stage instantiation, the fine pass the sample-list one or -- `fused` --
    the fused fine stage (ops.fine_stage_fwd)."""
    ops = modes
    fine_stage_route(fused)
    nets = _nets()
    captured = []
    real = ops.nerf_wgrad

    def spy(save, grads, d_raw, P, **kw):
        captured.append((save, grads, d_raw, P, kw.get("maxima"), bool(kw.get("lean"))))
        return real(save, grads, d_raw, P, **kw)
    monkeypatch.setattr(ops, "nerf_wgrad", spy)
    fused_calls = []
    real_fine = ops.fine_stage_fwd

    def spy_fine(*a, **kw):
        fused_calls.append(bool(kw.get("lean")))
        return real_fine(*a, **kw)
    monkeypatch.setattr(ops, "fine_stage_fwd", spy_fine)
    ops.lean_workspace(False)
    off = _step(nets, 256)
    assert [c[5] for c in captured] == [False, False]
    full_calls = list(captured)
    ops.lean_workspace(True)
    on = _step(nets, 256)
    assert [c[5] for c in captured[2:]] == [True, True]
    assert fused_calls == ([False, True] if fused else [])
    monkeypatch.setattr(ops, "nerf_wgrad", real)
    for k in off[0]:
        assert torch.equal(_words(off[0][k]), _words(on[0][k])), k
    assert torch.equal(_words(off[2]), _words(on[2])), "d rays"
    keep = ~_derived_mask()
    # (the fine pass's weight gradients come first in the backward: functional.py)
    for (save, grads, d_raw, P, mx, _), name in zip(full_calls, ("fine", "coarse")):
        i = 1 if name == "fine" else 0
        a, b = off[1][i].cpu().numpy(), on[1][i].cpu().numpy()
        np.testing.assert_array_equal(a.view(np.int32)[keep], b.view(np.int32)[keep], err_msg=name)
        ops.wgrad_arithmetic("fp32")
        yard = real(save, grads, d_raw, P, maxima=mx).cpu().numpy()
        ops.wgrad_arithmetic("half")
        _judge("step/%s P=%d" % (name, P), b, yard, _fp64_reference(save, grads, P))
