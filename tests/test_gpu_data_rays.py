"""The training step on rays that are data, on the MI355X: the resident data-gradient kernel without the input gradient
(scnerf_mlp_bwd_h3 with d_pts == d_views == NULL, csrc/mlp_bwd_h3_kernel.h IG = false), composite_bwd without d rays_d, no
ray reduction.  That kernel passes over three products (skip_units: the weight stream advances, no MFMA), runs unfilled the
epilogues those products hid, and writes chunk-maxima rows 9 - 11 from a branch of its own -- an LDS ring phase, accumulator
reads straight behind the MFMAs and raw write-through stores that the sequentially consistent CPU interpreter
(tests/test_emu_mlp_bwd_no_input_grad.py) cannot judge.

(a) the two instantiations write the same bits, (b) the one without the input gradient against fp64 on its own evidence,
(d) a render_rays step on data rays equals the step on differentiable rays bit for bit, (e) the fused network query in all
four requires_grad combinations of its inputs.  ((c), the weight gradients with the ReLU decisions aligned:
tests/test_gpu_kernels.py::test_relu_gate_flips_are_attributed[resident_no_input_grad].)"""
import numpy as np
import pytest
import torch

from scnerf_amd import mlp_layout as ML
from scnerf_amd import synthetic as synth
from tests import dgrad_reference, hostile_weights, trained_weights

pytestmark = pytest.mark.gpu

SC, SF = 64, 128
KEYS = ("rgb_map", "disp_map", "acc_map", "rgb0", "disp0", "acc0", "raw")
POISON = 0x7FC0BEEF                 # a quiet NaN no kernel produces: a word still holding it was not written


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from scnerf_amd import ops as _ops
    _ops.check_layout()
    return _ops


@pytest.fixture
def modes(ops):
    before = (ops.resident_guard(), ops.mlp_arithmetic(), ops.wgrad_arithmetic())
    if before[1] != "resident":
        pytest.skip("the data-ray kernels are the resident arithmetic's")
    yield ops
    ops.resident_guard(before[0])
    ops.mlp_arithmetic(before[1])
    ops.wgrad_arithmetic(before[2])


def _flat(p, pd=3):
    return torch.cat([p[name].reshape(-1) for name, _ in ML.layout(pd).param_shapes]).contiguous().cuda()


def _weights(pd, kind):
    if pd == 4:
        from tests.emu_mlp_util import network_params
        assert kind == "xavier"
        return network_params(779, 4)
    return hostile_weights.weights(0) if kind == "hostile" else trained_weights.weights(kind, 4)


def _wide_d_raw(P, g):
    """every sample's incoming gradient scaled by its own power of ten between 1e-30 and 1e+10, every 97th row zero"""
    d_raw = torch.randn(P, 4, generator=g) * 10.0 ** torch.randint(-30, 11, (P, 1), generator=g).float()
    d_raw[::97] = 0.0
    return d_raw


def _kernel_inputs(ops, pd, kind, n_rays, spr, seed=18, wide=True, guard=None):
    """packs, inputs and the activation workspace of a resident training forward"""
    p = _weights(pd, kind)
    flat = _flat(p, pd)
    P = n_rays * spr
    g = torch.Generator().manual_seed(seed)
    pts = (torch.rand(P, pd, generator=g) * 2.4 - 1.2).contiguous().cuda()
    vd = torch.randn(n_rays, 3, generator=g)
    vd = (vd / vd.norm(dim=-1, keepdim=True)).contiguous().cuda()
    d_raw = (_wide_d_raw(P, g) if wide else torch.randn(P, 4, generator=g)).contiguous().cuda()
    rw = ops.pack_resident(flat, pd)
    save = ops.save_workspace(P, "cuda", pd)
    ops.mlp_fwd(pts, vd, spr, ops.pack_weights(flat, "fwd", pd=pd), save, pd=pd, planes=rw, guard=guard)
    return dict(p=p, pd=pd, P=P, spr=spr, pts=pts, vd=vd, d_raw=d_raw, rw=rw, save=save, wb=ops.pack_weights(flat, "bwd", pd=pd))


def _launch(ops, S, vd, input_grad, with_maxima=True):
    """scnerf_mlp_bwd_h3 through the C ABI into a poisoned workspace -> (grads as int32 words, maxima [12, chunks] as int32
    words or None, d_pts, d_views)"""
    from scnerf_amd import _capi
    pd, P = S["pd"], S["P"]
    grads = torch.full((ML.grad_floats(P),), POISON, dtype=torch.int32, device="cuda")
    d_pts = torch.full((P, pd), float("nan"), device="cuda") if input_grad else None
    d_views = torch.full((P, 3), float("nan"), device="cuda") if input_grad else None
    mx = ops.ChunkMaxima(P, "cuda") if with_maxima else None
    vptr, vstride = ops._vd(vd)
    st = _capi.load().scnerf_mlp_bwd_h3(pd, ops._p(S["d_raw"]), ops._p(S["pts"]), vptr, vstride, S["spr"], ops._p(S["wb"]),
                                        ops._p(S["rw"].bwd), ops._p(S["rw"].scales), ops._p(S["save"]), ops._p(grads),
                                        ops._p(d_pts), ops._p(d_views), P, ops._p(mx.z) if mx else None,
                                        mx.chunks if mx else 0, mx.chunk_samples if mx else 0, ops._stream())
    _capi.check(st, "scnerf_mlp_bwd_h3")
    return grads, (mx.z.contiguous().view(torch.int32) if mx else None), d_pts, d_views


def _same_words(a, b, what):
    if not torch.equal(a, b):
        idx = torch.nonzero(a != b).reshape(-1) if a.dim() == 1 else torch.nonzero(a != b)
        Pp = a.numel() // ML.GRAD_FLOATS_PER_SAMPLE if a.dim() == 1 else 0
        raise AssertionError("%s: %d words differ, first at %s%s" % (
            what, idx.shape[0], idx[0].tolist(),
            " (section offsets in floats: %s)" % ML.section_offsets(ML.GRAD_SECTIONS, Pp)[0] if Pp else ""))


# ---- (a) the two instantiations write the same bits ---------------------------------------------------------------------
@pytest.mark.parametrize("vd_form", ["contiguous", "ray_batch_slice"])
@pytest.mark.parametrize("n_rays,spr", [(21, 50), (1, 45), (1024, 64), (4096, 192)])
@pytest.mark.parametrize("pd,kind", [(3, "xavier"), (3, "trained"), (3, "adversarial"), (4, "xavier")])
def test_both_instantiations_write_the_same_bits(ops, pd, kind, n_rays, spr, vd_form):
    """mlp_bwd_h3_kernel<pd, true> and <pd, false> on the same workspace, packs and chunk geometry: the whole gradient
    workspace (pre-filled with a NaN pattern: the same set of written words, the same values) and all twelve rows of chunk
    maxima equal as integer words; rows 8 - 11, which the narrow weight-gradient GEMMs scale by, positive in every chunk.
    (21, 50): a ragged last workgroup, samples_per_ray no multiple of the wave tile; (1, 45): less than one wave tile pair;
    (4096, 192): the headline fine pass, 6144 workgroups -- there the kernel without the input gradient runs twice: a race in
    the schedule of the passed-over units shows as a difference between two launches, not as a tolerance.  The view
    directions as a [n, 3] tensor and as columns 8 .. 10 of a ray batch (row stride 11: what render_rays passes, and what
    row 11 of the maxima reads in the branch of its own)."""
    S = _kernel_inputs(ops, pd, kind, n_rays, spr)
    vd = S["vd"]
    if vd_form == "ray_batch_slice":
        rays = torch.zeros(n_rays, 11, device="cuda")
        rays[:, 8:11] = vd
        vd = rays[:, 8:11]
        assert n_rays == 1 or ops._vd(vd)[1] == 11
    g_full, m_full, d_pts, d_views = _launch(ops, S, vd, True)
    assert bool(torch.isfinite(d_pts).all()) and bool(torch.isfinite(d_views).all())
    g_none, m_none, _, _ = _launch(ops, S, vd, False)
    assert not bool((g_full == POISON).any()), "the workspace has words no launch wrote"
    _same_words(g_full, g_none, "gradient workspace")
    _same_words(m_full, m_none, "chunk maxima")
    assert bool((m_none[8:].view(torch.float32) > 0).all()), m_none[8:].view(torch.float32).min(1)[0].tolist()
    if (n_rays, spr) == (4096, 192):
        del g_full, d_pts, d_views
        g_again, m_again, _, _ = _launch(ops, S, vd, False)
        _same_words(g_none, g_again, "gradient workspace, second launch")
        _same_words(m_none, m_again, "chunk maxima, second launch")


@pytest.mark.parametrize("pd", [3, 4])
def test_both_instantiations_run_without_a_maxima_table(ops, pd):
    """maxima == NULL (the fp32 weight-gradient arithmetic): neither instantiation touches a table, and the workspace is what
    it is with one"""
    S = _kernel_inputs(ops, pd, "xavier", 21, 50)
    g_full, m, _, _ = _launch(ops, S, S["vd"], True, with_maxima=False)
    assert m is None
    g_none, _, _, _ = _launch(ops, S, S["vd"], False, with_maxima=False)
    g_table, _, _, _ = _launch(ops, S, S["vd"], False, with_maxima=True)
    assert not bool((g_none == POISON).any())
    _same_words(g_full, g_none, "gradient workspace")
    _same_words(g_table, g_none, "gradient workspace, with and without a maxima table")


@pytest.mark.parametrize("kind", ["hostile", "xavier"])
def test_guarded_entry_is_the_same_with_and_without_the_input_gradient(ops, modes, monkeypatch, kind):
    """scnerf_mlp_bwd_h3_guarded (ops.mlp_bwd(..., guard=...)) with and without the input gradient, on a network that trips
    every block (tests/hostile_weights.py) and on one that trips none: block flags, the `any` word, the report and the
    gradient workspace identical -- straight after the resident launch, and after the gated exact-fp32 launch that runs the
    flagged blocks again (which always forms the input gradient: into scratch when the caller wants none)."""
    ops.resident_guard("report")
    n_rays, spr = 37, 64
    P = n_rays * spr
    fwd = ops.guard_records("cuda", [("pass", P)])
    S = _kernel_inputs(ops, 3, kind, n_rays, spr, wide=False, guard=fwd["pass"])
    flags_in = fwd["pass"].flags.clone()
    assert bool((flags_in != 0).all()) if kind == "hostile" else not bool(flags_in.any())

    def run(input_grad, rerun):
        rec = ops.guard_records("cuda", [("pass", P)])
        rec["pass"].flags.copy_(flags_in)                       # what the forward left: the data gradients share its flags
        with monkeypatch.context() as mp:
            if not rerun:
                mp.setattr(ops, "_guard_after", lambda guard, launch: None)
            grads, d_pts, d_views = ops.mlp_bwd(S["d_raw"], S["pts"], S["vd"], spr, S["wb"], S["save"], planes=S["rw"],
                                                maxima=ops.ChunkMaxima(P, "cuda"), input_grad=input_grad, guard=rec["pass_bwd"])
        assert (d_pts is None and d_views is None) == (not input_grad)
        b = rec["pass_bwd"]
        return grads.view(torch.int32), b.flags.clone(), b.any.clone(), b.report.clone().view(torch.int32)

    for rerun in (False, True):
        full, none = run(True, rerun), run(False, rerun)
        for a, b, what in zip(full, none, ("gradient workspace", "block flags", "any", "report")):
            _same_words(a, b, "%s (%s the fp32 launch)" % (what, "after" if rerun else "before"))
        if rerun:
            assert (not torch.equal(none[0], before[0])) == (kind == "hostile")   # the flagged blocks did run again
        before = none


# ---- (b) the kernel without the input gradient against fp64 -------------------------------------------------------------
@pytest.mark.parametrize("kind", ["xavier", "trained", "adversarial"])
def test_chain_without_input_gradient_is_fp32_grade_against_fp64(ops, kind):
    """The resident chain WITHOUT the input gradient against the chain in double precision on the same saved gates
    (tests/dgrad_reference.py), beside the fused fp32 chain judged the same way, 1024 x 192 samples, incoming gradients
    over forty orders of magnitude: per gradient section the resident kernel's worst row may be no further from fp64 than
    3 x the fp32 kernel's + 1e-7, its 99.9 % row no further than 2 x + 1e-7 (the bounds of
    test_resident_data_gradients_follow_the_fused_chain_row_by_row's fp64 branch), and zero rows stay exactly zero.  The
    yardsticks are fp64 and the fp32 kernel, never the resident kernel with the input gradient."""
    from tests import parity_attribution as PA
    S = _kernel_inputs(ops, 3, kind, 1024, 192)
    P, spr = S["P"], S["spr"]
    ga, _, _ = ops.mlp_bwd(S["d_raw"], S["pts"], S["vd"], spr, S["wb"], S["save"])
    gb, d_pts, d_views = ops.mlp_bwd(S["d_raw"], S["pts"], S["vd"], spr, S["wb"], S["save"], planes=S["rw"], input_grad=False)
    assert d_pts is None and d_views is None
    ref = dgrad_reference.fp64_chain(S["p"], S["save"], S["d_raw"], P)
    zero = S["d_raw"].abs().sum(1) == 0
    rep = {}
    for name, width in ML.GRAD_SECTIONS:
        b = dgrad_reference.grad_rows(gb, name, width, P)
        assert bool(torch.isfinite(b).all()), name
        ea = dgrad_reference.row_errors(ga, ref, name, width, P, ~zero)
        eb = dgrad_reference.row_errors(gb, ref, name, width, P, ~zero)
        rep[name] = {"fp32_max": float(ea.max()), "resident_max": float(eb.max()),
                     "fp32_q999": float(torch.quantile(ea[:1 << 20], 0.999)), "resident_q999": float(torch.quantile(eb[:1 << 20], 0.999))}
        print(kind, name, rep[name])
    PA.REPORT["resident_data_gradient_chain_no_input_grad_row_error_vs_fp64/" + kind] = rep
    for name, width in ML.GRAD_SECTIONS:
        assert rep[name]["resident_max"] <= 3.0 * rep[name]["fp32_max"] + 1e-7, (name, rep[name])
        assert rep[name]["resident_q999"] <= 2.0 * rep[name]["fp32_q999"] + 1e-7, (name, rep[name])
        assert bool((dgrad_reference.grad_rows(gb, name, width, P)[zero] == 0).all()), name


# ---- (d) the step on data rays equals the step on differentiable rays ---------------------------------------------------
def _nets(params):
    from scnerf_amd import run_nerf_helpers as H
    out = []
    for p in params:
        net = H.NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
        net.load_state_dict(p)
        out.append(net.cuda())
    return out


def _params(kind):
    if kind == "hostile":
        return [hostile_weights.weights(0), hostile_weights.weights(1)]
    if kind == "trained":
        return [trained_weights.weights("trained", which="coarse"), trained_weights.weights("trained", which="fine")]
    return [synth.network_params(seed=0), synth.network_params(seed=1)]


def _query():
    from scnerf_amd import create_nerf, run_nerf_helpers as H
    return create_nerf.FusedNetworkQuery(H.get_embedder(10, 0)[0], H.get_embedder(4, 0)[0])


def _loss(nets, n, rays_need_grad, seed=5):
    from scnerf_amd import render
    rays = synth.ray_batch(n, seed=seed).cuda().requires_grad_(rays_need_grad)
    rnd = {k: v.cuda() for k, v in synth.render_randoms(n, SC, SF, seed=seed + 1).items()}
    ret = render.render_rays(rays, nets[0], _query(), SC, retraw=True, perturb=1.0, N_importance=SF, network_fine=nets[1],
                             raw_noise_std=1.0, _randoms=rnd)
    loss = (ret["rgb_map"] ** 2).sum() + (ret["rgb0"] ** 2).sum() + ret["disp_map"].sum() + ret["acc0"].sum()
    return rays, ret, loss


def _step(nets, n, rays_need_grad, seed=5):
    """one render_rays training step -> (outputs, [flat gradient of each network], d rays or None)"""
    rays, ret, loss = _loss(nets, n, rays_need_grad, seed)
    params = [list(net.parameters()) for net in nets]
    got = torch.autograd.grad(loss, ([rays] if rays_need_grad else []) + params[0] + params[1])
    k = 1 if rays_need_grad else 0
    n0 = len(params[0])
    flat = [torch.cat([g.reshape(-1) for g in got[k:k + n0]]), torch.cat([g.reshape(-1) for g in got[k + n0:]])]
    return {key: ret[key].detach() for key in KEYS}, flat, (got[0].detach() if rays_need_grad else None)


def _same_step(a, b):
    for key in KEYS:
        assert torch.equal(a[0][key], b[0][key]), key
    for net, x, y in zip(("coarse", "fine"), a[1], b[1]):
        assert torch.equal(x, y), (net, "flat gradient", int((x != y).sum()), float((x - y).abs().max()))


@pytest.mark.parametrize("kind", ["xavier", "trained"])
@pytest.mark.parametrize("n", [4096, 1001])
def test_step_on_data_rays_equals_the_step_on_differentiable_rays(modes, n, kind):
    """render_rays -> loss -> gradients with a ray batch that is data (mlp_bwd_h3_kernel<3, false>, composite_bwd without
    d rays_d, no ray reduction) and with one that requires a gradient: every output and both networks' flat gradients bit
    for bit.  1001 rays: 1001 x 64 and 1001 x 192 samples both end mid-workgroup."""
    if kind == "trained" and not trained_weights.have_trained():
        pytest.skip("no trained weights")
    nets = _nets(_params(kind))
    full = _step(nets, n, True)
    data = _step(nets, n, False)
    assert full[2] is not None and bool(full[2].abs().sum() > 0) and data[2] is None
    _same_step(full, data)


def test_hostile_step_on_data_rays_under_the_fallback_guard(modes):
    """every block trips (tests/hostile_weights.py) and runs again on the exact-fp32 kernels -- forward and data gradients,
    both passes: the step on data rays is the step on differentiable rays bit for bit"""
    ops = modes
    nets = _nets(_params("hostile"))
    ops.resident_guard("fallback")
    full = _step(nets, 512, True)
    data = _step(nets, 512, False)
    m = ops.resident_margins()
    for name in ("coarse", "fine", "coarse_bwd", "fine_bwd"):
        assert m[name]["blocks"] > 0 and m[name]["reran_blocks"] == m[name]["blocks"], (name, m[name])
    _same_step(full, data)


def test_data_ray_step_accumulates_into_attached_flat_buffers(modes):
    """every .grad a view of one flat buffer (RenderRaysFunction._stage_wgrad's `into`): loss.backward() on data rays leaves
    in .grad what autograd.grad returns"""
    from scnerf_amd.parallel import FlatGradAllReduce
    n = 1001
    plain = _nets(_params("xavier"))
    want = _step(plain, n, False)
    nets = _nets(_params("xavier"))
    red = FlatGradAllReduce(nets, 1)
    assert all(net.attached_flat_grad() is not None for net in nets)
    red.flat.zero_()
    _, ret, loss = _loss(nets, n, False)
    loss.backward()
    assert all(net.attached_flat_grad() is not None for net in nets)            # still the one buffer
    for key in KEYS:
        assert torch.equal(ret[key].detach(), want[0][key]), key
    for net, flat in zip(nets, want[1]):
        got = torch.cat([p.grad.reshape(-1) for p in net.parameters()])
        assert torch.equal(got, flat), (int((got != flat).sum()), float((got - flat).abs().max()))


def test_fp32_step_on_data_rays_equals_the_step_on_differentiable_rays(modes):
    """mlp_arithmetic("fp32") + wgrad_arithmetic("fp32"): the fused fp32 kernel forms the input gradient whatever the flag
    says -- what differs between the two steps is host plumbing alone (no d rays_d, no ray reduction, no zero d rays)"""
    ops = modes
    ops.mlp_arithmetic("fp32")
    ops.wgrad_arithmetic("fp32")
    nets = _nets(_params("xavier"))
    _same_step(_step(nets, 1001, True), _step(nets, 1001, False))


# ---- (e) the fused network query ---------------------------------------------------------------------------------------
def test_network_query_in_all_four_requires_grad_combinations(modes):
    """create_nerf.FusedNetworkQuery on 64 x 70 samples: the kernel without the input gradient runs when NEITHER the points
    nor the directions need one.  raw and every parameter gradient bit-identical across the four combinations; the input
    gradients that were asked for equal those of the run that asked for both; the others are None."""
    net = _nets([synth.network_params(seed=2)])[0]
    g = torch.Generator().manual_seed(31)
    pts0 = (torch.rand(64, 70, 3, generator=g) * 2.4 - 1.2).cuda()
    vd0 = torch.nn.functional.normalize(torch.randn(64, 3, generator=g), dim=-1).cuda()
    gy = torch.randn(64, 70, 4, generator=g).cuda()
    runs = {}
    for need_p in (True, False):
        for need_v in (True, False):
            net.zero_grad(set_to_none=True)
            pts, vd = pts0.clone().requires_grad_(need_p), vd0.clone().requires_grad_(need_v)
            raw = _query()(pts, vd, net)
            (raw * gy).sum().backward()
            runs[need_p, need_v] = (raw.detach(), [p.grad.clone() for p in net.parameters()], pts.grad, vd.grad)
    ref = runs[True, True]
    assert ref[2] is not None and ref[3] is not None and bool(ref[2].abs().sum() > 0) and bool(ref[3].abs().sum() > 0)
    for (need_p, need_v), (raw, pg, d_p, d_v) in runs.items():
        assert torch.equal(raw, ref[0]), (need_p, need_v)
        for (name, _), a, b in zip(net.named_parameters(), pg, ref[1]):
            assert torch.equal(a, b), (need_p, need_v, name)
        for need, got, want, what in ((need_p, d_p, ref[2], "d pts"), (need_v, d_v, ref[3], "d viewdirs")):
            if need:
                assert torch.equal(got, want), (need_p, need_v, what)
            else:
                assert got is None, (need_p, need_v, what)
