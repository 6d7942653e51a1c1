"""GPU parity of the full render path (pytest -m gpu): scnerf_amd.render.{render_rays,
batchify_rays, raw2outputs, sample_pdf} through the C ABI vs (1) golden vectors of the unmodified
reference and (2) the CPU oracle on seeded inputs at the headline size.

Tolerances: north-star bar 1e-4 on rgb / disparity; gradients are compared relative to the
largest entry of the reference gradient (they span orders of magnitude)."""
import numpy as np
import pytest
import torch

import json
import os

from oracle import scnerf_oracle as O
from scnerf_amd import synthetic as synth
from conftest import t
from tests import parity_attribution as PA

pytestmark = pytest.mark.gpu

REPORT = PA.REPORT          # written by tests/conftest.py at the end of the session

CASES = ["c64_f0_det", "c64_f0_pert", "c64_f128_pert", "c64_f128_det", "c64_f64_lindisp"]


@pytest.fixture(scope="module")
def R():
    assert torch.cuda.is_available()
    from scnerf_amd import render, create_nerf, run_nerf_helpers, ops
    ops.check_layout()
    return dict(render=render, create_nerf=create_nerf, helpers=run_nerf_helpers, ops=ops)


from tests.render_step_case import make_net, make_query, net_params      # noqa: E402,F401  (shared with the interpreter twin)
from tests.render_step_case import kernel_gates as _kernel_gates, render_node as _render_node      # noqa: E402,F401


def rel_err(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return float(np.abs(a - b).max()) / (float(np.abs(b).max()) + 1e-30)


def grad_close(a, b, what, q=0.999, tol_q=1e-3, tol_max=5e-2):
    """Gradients of a ReLU network are discontinuous: a pre-activation within rounding of zero may
    be 'on' on one side and 'off' on the other, which changes that sample's gradient by O(1/width).
    So: the q-quantile of |err| / max|ref| must be tight, single outliers only bounded."""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    e = np.sort(np.abs(a - b).reshape(-1) / (float(np.abs(b).max()) + 1e-30))
    n_out = max(3, int(np.ceil((1 - q) * e.size)))          # entries allowed above tol_q (a few mask flips)
    eq = float(e[max(0, e.size - 1 - n_out)])
    assert eq <= tol_q, "%s: rel err %g beyond %d allowed outliers (max %g)" % (what, eq, n_out, float(e[-1]))
    assert float(e[-1]) <= tol_max, "%s: max rel err %g" % (what, float(e[-1]))


def rays_within(got, ref, tol):
    """fraction of rays whose every component is within tol"""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    e = np.abs(got - ref).reshape(ref.shape[0], -1).max(1)
    return float((e <= tol).mean()), float(e.max())


@pytest.fixture(params=["resident", "fp32"])
def arithmetic(request):
    """the golden render_rays cases run in both arithmetics of the training step (ops.mlp_arithmetic /
    ops.wgrad_arithmetic): the default resident kernels on three fp16 products and the all-fp32-MFMA yardstick"""
    from scnerf_amd import ops
    saved = (ops.mlp_arithmetic(), ops.wgrad_arithmetic())
    ops.mlp_arithmetic(request.param)
    ops.wgrad_arithmetic("fp32" if request.param == "fp32" else "half")
    yield request.param
    ops.mlp_arithmetic(saved[0])
    ops.wgrad_arithmetic(saved[1])


@pytest.mark.parametrize("tag", CASES)
def test_render_rays_vs_reference_golden(R, golden, tag, arithmetic):
    g = golden("render_rays")
    k = tag + "/"
    n, sc, sf, perturb, rns, lindisp, wb = g[k + "cfg"]
    n, sc, sf = int(n), int(sc), int(sf)
    net_c, net_f = make_net(R, 0), make_net(R, 1)
    rays = t(g[k + "rays"]).cuda().requires_grad_(True)
    rnd = {}
    if perturb > 0:
        rnd["t_rand"] = t(g[k + "rnd/t_rand"]).cuda()
        if sf > 0:
            rnd["u"] = t(g[k + "rnd/u"]).cuda()
    if rns > 0:
        rnd["noise_c"] = (t(g[k + "rnd/noise_c"]) * rns).cuda()
        if sf > 0:
            rnd["noise_f"] = (t(g[k + "rnd/noise_f"]) * rns).cuda()
    ret = R["render"].batchify_rays(
        rays, chunk=1 << 15, network_fn=net_c, network_query_fn=make_query(R), N_samples=sc, retraw=True,
        lindisp=bool(lindisp), perturb=float(perturb), N_importance=sf, network_fine=net_f if sf > 0 else None,
        white_bkgd=bool(wb), raw_noise_std=float(rns), _randoms=rnd)
    # Coarse outputs (and everything when there is no fine stage) meet the 1e-4 bar on every ray.
    # Outputs behind the hierarchical sampler inherit the reference algorithm's own discontinuity
    # (render.py:455-456: a bin whose mass crosses 1e-5 switches between "interpolate" and "snap to
    # the left edge", moving a sample by up to one bin for a 1e-8 change of the coarse weights), so
    # there a single ray may legitimately differ; the fine stage is pinned strictly in
    # test_fine_stage_strict (fed the oracle's samples).
    strict = [("rgb0", 1e-4), ("acc0", 1e-4)] if sf > 0 else [("rgb_map", 1e-4), ("acc_map", 1e-4)]
    for name, tol in strict:
        np.testing.assert_allclose(ret[name].detach().cpu().numpy(), g[k + name], rtol=0, atol=tol, err_msg=name)
    for name in (["disp0"] if sf > 0 else ["disp_map"]):
        np.testing.assert_allclose(ret[name].detach().cpu().numpy(), g[k + name], rtol=1e-4, atol=1e-4, err_msg=name)
    clean = np.ones(n, bool)
    if sf > 0:
        # every ray beyond the bar owns a sample the reference algorithm itself places discontinuously
        # (tests/parity_attribution.py): compared on the cdf / search indices both sides expose
        from scnerf_amd.functional import host_linspace
        u_dev = rnd["u"] if perturb > 0 else host_linspace(sf, "cuda").expand(n, sf).contiguous()
        st = PA.gpu_sampling_state(R["ops"], host_linspace, rays.detach(), net_c, rnd.get("t_rand"), u_dev,
                                   rnd.get("noise_c"), sc, bool(lindisp), bool(wb))
        same = torch.equal(torch.where(st["rgb0"] >= 1.0, torch.ones_like(st["rgb0"]), st["rgb0"]), ret["rgb0"].detach())
        z_c = st["z_c"].cpu()
        cls = PA.classify(u_dev.cpu(), 0.5 * (z_c[:, 1:] + z_c[:, :-1]), st["cdf"].cpu(), st["inds"].cpu(),
                          g[k + "cdf"], g[k + "inds"])
        clean = ~(cls["index"] | cls["branch"] | cls["illcond"])
        rep = {}
        for name, rel in (("rgb_map", False), ("acc_map", False), ("disp_map", True)):
            err = PA.per_ray_error(ret[name], g[k + name], relative=rel)
            rep[name] = PA.summary(err, cls)
            assert rep[name]["over_bar_unexplained"] == 0, (name, rep[name])
            assert rep[name]["max"] < 1e-2, (name, rep[name])
        rep["coarse_rerun_bit_identical"] = bool(same)      # the re-run IS the coarse stage inside render_rays
        REPORT["golden/" + tag + ("" if arithmetic == "resident" else "/all_fp32_mfma")] = rep
        zs = np.abs(ret["z_std"].cpu().numpy() - g[k + "z_std"])
        assert zs[clean].max(initial=0.0) <= 1e-5 + 1e-3 * np.abs(g[k + "z_std"]).max()
    else:
        np.testing.assert_allclose(ret["raw"].detach().cpu().numpy(), g[k + "raw"], rtol=0, atol=1e-4)
    target = t(g[k + "target"]).cuda()
    loss = torch.mean((ret["rgb_map"] - target) ** 2)
    if sf > 0:
        loss = loss + torch.mean((ret["rgb0"] - target) ** 2)
    np.testing.assert_allclose(float(loss.detach()), float(g[k + "loss"]), rtol=1e-4)
    loss.backward()
    cols = [0, 1, 2, 3, 4, 5, 8, 9, 10]
    tq = 2e-3 if sf > 0 else 1e-3
    ge = np.abs(rays.grad[:, cols].cpu().numpy() - g[k + "g_rays"][:, cols]).max(1) / np.abs(g[k + "g_rays"]).max()
    # rays whose samples sit where the reference places them: the ray gradient holds to 1e-3 of the largest entry
    # but for single ReLU-flip rays -- at most 3 of the 24, and those within 5e-3 (a flipped gate changes one
    # sample's contribution, not the ray); rays with a moved sample are only bounded
    REPORT.setdefault("golden/" + tag + ("" if arithmetic == "resident" else "/all_fp32_mfma"), {})["d_ray_batch"] = dict(
        clean_rays=int(clean.sum()), clean_within_1e3=float((ge[clean] < 1e-3).mean()), clean_max=float(ge[clean].max()),
        all_max=float(ge.max()))
    assert (ge[clean] >= 1e-3).sum() <= 3 and ge[clean].max(initial=0.0) < 5e-3 and ge.max() < 0.1, (
        "d ray_batch", int((ge[clean] >= 1e-3).sum()), float(ge[clean].max(initial=0.0)), float(ge.max()))
    assert float(rays.grad[:, 6:8].abs().max()) == 0.0
    nets = {"coarse": net_c, "fine": net_f}
    for key in g:
        if key.startswith(k + "g/"):
            _, _, net, pn = key.split("/")
            got = dict(nets[net].named_parameters())[pn].grad
            assert got is not None, key
            # behind the sampler one moved sample (see above) shifts every entry of a weight gradient a
            # little at this tiny batch (24 rays); the tight end-to-end statement is
            # test_training_gradients_with_both_discontinuities_aligned (4.5e-6), the network-only ones
            # test_run_network_* and tests/test_gpu_kernels.py::test_relu_gate_flips_are_attributed
            grad_close(got, g[key], key, q=0.99, tol_q=(2e-2 if sf > 0 else tq), tol_max=(0.1 if sf > 0 else 5e-2))
        elif key.startswith(k + "gnorm/"):
            _, _, net, pn = key.split("/")
            got = float(dict(nets[net].named_parameters())[pn].grad.double().norm())
            np.testing.assert_allclose(got, float(g[key]), rtol=(2e-2 if sf > 0 else 5e-3), err_msg=key)


def test_fine_stage_strict(R):
    """Fine network + compositing on the ORACLE's merged depths (so both sides see identical
    samples): every ray within 1e-4, as the staged-parity plan of SURVEY.md section 7 asks."""
    n, sc, sf = 256, 64, 128
    net_f = make_net(R, 1)
    pc, pf = synth.network_params(seed=0), synth.network_params(seed=1)
    rays = synth.ray_batch(n, seed=1)
    rnd = synth.render_randoms(n, sc, sf, seed=3)
    with torch.no_grad():
        o = O.render_rays(rays, pc, pf, sc, sf, rnd["t_rand"], rnd["u"], rnd["noise_c"], rnd["noise_f"], rowsum="aten")
    # our sampler on the oracle's coarse weights: bit-exact indices / samples / merged depths
    z_f, pts_f, z_s, z_std, inds, cdf = R["ops"].fine_sample(rays.cuda(), o["z_coarse"].cuda().contiguous(),
                                                            o["weights_coarse"].cuda().contiguous(),
                                                            rnd["u"].cuda(), True, True)
    np.testing.assert_array_equal(inds.cpu().numpy(), o["inds"].numpy())
    np.testing.assert_array_equal(z_s.cpu().numpy(), o["z_samples"].numpy())
    np.testing.assert_array_equal(z_f.cpu().numpy(), o["z_fine"].numpy())
    raw = make_query(R)(pts_f, rays[:, 8:11].cuda().contiguous(), net_f)
    raw = raw.detach()
    np.testing.assert_allclose(raw.cpu().numpy(), o["raw"].numpy(), rtol=0, atol=1e-4)
    rgb, disp, acc, w, depth = R["render"].raw2outputs(raw, z_f, rays[:, 3:6].cuda(), _noise=rnd["noise_f"].cuda())
    np.testing.assert_allclose(rgb.cpu().numpy(), o["rgb_map"].numpy(), rtol=0, atol=1e-4)
    np.testing.assert_allclose(acc.cpu().numpy(), o["acc_map"].numpy(), rtol=0, atol=1e-4)
    np.testing.assert_allclose(depth.cpu().numpy(), o["depth_map"].numpy(), rtol=0, atol=1e-4)
    np.testing.assert_allclose(disp.cpu().numpy(), o["disp_map"].numpy(), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("n,kind,mode,data_rays", [(256, "xavier", None, False), (4096, "xavier", None, False),
                                                   (4096, "trained", None, False), (4096, "trained", "fp32", False),
                                                   (256, "xavier", None, True), (4096, "trained", None, True)],
                         ids=["256rays", "4096rays", "4096rays_trained", "4096rays_trained_fp32_yardstick",
                              "256rays_data_rays", "4096rays_trained_data_rays"])
def test_training_gradients_with_both_discontinuities_aligned(R, n, kind, mode, data_rays):
    """(`kind`: the networks' weights -- the reference's initialisation, or both networks after 5000 training steps;
    `mode`: None = the arithmetic in force, "fp32" = the exact-fp32 MFMA kernels as the yardstick on the same case;
    `data_rays`: the GPU run's ray batch requires no gradient -- the benchmark's headline step: the data-gradient kernel
    without the input gradient, composite_bwd without d rays_d, no ray reduction -- and there is no ray gradient to compare.)
    The golden cases bound the gradients behind the hierarchical sampler only loosely: one sample the reference
    algorithm places discontinuously (render.py:444, :455-456) or one ReLU whose pre-activation is a rounding from
    zero shifts every entry of a weight gradient a little at 24 rays.  Here both discontinuities are taken out of the
    COMPARISON instead of out of the bound: the CPU oracle runs the whole `render_rays` -- coarse stage, fine stage,
    both losses -- on the GPU run's own new depths (detached in the reference, :274: same graph) and with the GPU
    run's own ReLU decisions (the bit masks its training forward leaves), and every parameter gradient of both
    networks and every ray's gradient is held to the bound of the network-only attribution test
    (tests/test_gpu_kernels.py::test_relu_gate_flips_are_attributed).  How many decisions differ from the oracle's
    own goes to the report."""
    from scnerf_amd.functional import host_linspace
    saved = (R["ops"].mlp_arithmetic(), R["ops"].wgrad_arithmetic())
    if mode is not None:
        R["ops"].mlp_arithmetic(mode)
        R["ops"].wgrad_arithmetic(mode)
    try:
        _aligned_gradients_case(R, n, kind, mode, host_linspace, data_rays)
    finally:
        R["ops"].mlp_arithmetic(saved[0])
        R["ops"].wgrad_arithmetic(saved[1])


def _aligned_gradients_case(R, n, kind, mode, host_linspace, data_rays=False, **options):
    """(the body: tests/render_step_case.py, shared with tests/test_emu_render_step.py; 4096 rays x (64 + 128): the headline
    batch -- 8.6e8 ReLU decisions taken from the bit masks)"""
    from tests.render_step_case import aligned_gradients_case
    return aligned_gradients_case(R, n, kind, mode, host_linspace, data_rays, **options)


# sc, sf, arithmetic (None: the one in force), rays, options
GENERAL_SIZE_CASES = [
    (16, 16, None, 37, {}),
    (40, 33, None, 37, {}),                                   # 73 samples per ray: rays straddle 128-sample blocks, odd P
    (40, 33, "fp32", 37, {}),
    (40, 33, None, 37, dict(data_rays=True)),
    (40, 33, None, 37, dict(lindisp=True, white_bkgd=True)),
    (40, 33, None, 37, dict(perturb=0.0)),                    # no t_rand, the shared deterministic u row
    (64, 200, None, 9, {}),                                   # 264: the fused coarse stage, the three-launch fine stage
    (96, 0, None, 37, {}),                                    # no fine stage
    (40, 33, None, 37, dict(shared_net=True)),
    (40, 33, None, 37, dict(shared_net=True, attached=True)),
    (64, 128, None, 37, dict(shared_net=True)),
]


def _general_case_id(c):
    sc, sf, mode, n, opt = c
    return "%dx(%d+%d)%s%s" % (n, sc, sf, "" if mode is None else "_" + mode,
                               "".join("_%s" % k if v is True else "_%s%g" % (k, v) for k, v in opt.items()))


@pytest.mark.parametrize("case", GENERAL_SIZE_CASES, ids=_general_case_id)
def test_training_gradients_aligned_at_general_sample_counts(R, case):
    """test_training_gradients_with_both_discontinuities_aligned -- the same body, the same bounds -- at sample counts that
    are no multiple of 64 (the three-launch coarse stage, rays that straddle the 128-sample blocks and the waves, an odd
    n * samples_per_ray for the chunk maxima, the half weight-gradient group and the lean workspace), without a fine stage,
    and with ONE network for both stages (network_fine=None, reference render.py:279: shared packs and backward tables, the
    summed gradient, the attached flat .grad buffer accumulated into twice).  37 / 9 rays, xavier weights; the report
    entry of each case is keyed by its sizes and options."""
    from scnerf_amd.functional import host_linspace
    sc, sf, mode, n, opt = case
    saved = (R["ops"].mlp_arithmetic(), R["ops"].wgrad_arithmetic())
    if mode is not None:
        R["ops"].mlp_arithmetic(mode)
        R["ops"].wgrad_arithmetic(mode)
    try:
        print("\n%s: %s" % (_general_case_id(case), json.dumps(
            _aligned_gradients_case(R, n, "xavier", mode, host_linspace, sc=sc, sf=sf, **opt))))
    finally:
        R["ops"].mlp_arithmetic(saved[0])
        R["ops"].wgrad_arithmetic(saved[1])


def test_general_sample_count_step_is_bit_identical_under_the_scale_guard(R):
    """37 rays x (40 + 33) -- ceil(P / 128) blocks with a ragged last one: a training step under ops.resident_guard("fallback")
    and one under "strict" return the outputs and gradients of the step with the guard off, bit for bit, and "strict" does
    not raise (xavier weights trip nothing; the guarded entry points promise identical outputs)."""
    ops = R["ops"]
    n, sc, sf = 37, 40, 33
    rays = synth.ray_batch(n, seed=11).cuda()
    rnd = {k: v.cuda() for k, v in synth.render_randoms(n, sc, sf, seed=12).items()}
    target = torch.rand(n, 3, generator=torch.Generator().manual_seed(13)).cuda()
    saved = (ops.resident_guard(), ops.mlp_arithmetic())
    results = {}
    try:
        ops.mlp_arithmetic("resident")
        for guard in ("off", "fallback", "strict"):
            ops.resident_guard(guard)
            net_c, net_f = make_net(R, 0), make_net(R, 1)
            rd = rays.clone().requires_grad_(True)
            ret = R["render"].render_rays(rd, net_c, make_query(R), sc, retraw=True, perturb=1.0, N_importance=sf,
                                          network_fine=net_f, raw_noise_std=1.0, _randoms=rnd)
            (torch.mean((ret["rgb_map"] - target) ** 2) + torch.mean((ret["rgb0"] - target) ** 2)).backward()
            results[guard] = ([ret[k].detach() for k in ("rgb_map", "disp_map", "acc_map", "raw", "rgb0", "disp0", "acc0", "z_std")]
                              + [p.grad.clone() for p in list(net_c.parameters()) + list(net_f.parameters())] + [rd.grad.clone()])
    finally:
        ops.resident_guard(saved[0])
        ops.mlp_arithmetic(saved[1])
    for guard in ("fallback", "strict"):
        for i, (a, b) in enumerate(zip(results["off"], results[guard])):
            assert torch.equal(a, b), (guard, i)


@pytest.mark.parametrize("rays_need_grad", [True, False], ids=["differentiable_rays", "data_rays"])
def test_training_step_is_bit_reproducible(R, arithmetic, rays_need_grad):
    """(`rays_need_grad` False: the ray batch is data -- the data-gradient kernel without the input gradient, whose schedule
    passes over three products and runs their epilogues unfilled: the argument below applies to it at least as much.)
    The same 4096-ray training step five times: every output, the ray gradients and every parameter gradient of both
    networks bit for bit the same.  All sums of the path run in a fixed order (per-GEMM partial slabs reduced by index,
    fp64 prefix products, maxima through integer atomicMax), so anything else is a race -- and the LDS schedules of the
    resident kernels and the weight-gradient GEMMs (two slab images, one barrier per slab; chunk rings behind one
    barrier per chunk) are exactly what the sequentially consistent CPU interpreter cannot check."""
    n, sc, sf = 4096, 64, 128
    net_c, net_f = make_net(R, 0), make_net(R, 1)
    rays = synth.ray_batch(n, seed=21).cuda()
    rnd = {k: v.cuda() for k, v in synth.render_randoms(n, sc, sf, seed=22).items()}
    target = torch.rand(n, 3, generator=torch.Generator().manual_seed(23)).cuda()
    params = list(net_c.parameters()) + list(net_f.parameters())

    def once():
        r = rays.clone().requires_grad_(rays_need_grad)
        ret = R["render"].render_rays(r, net_c, make_query(R), sc, retraw=True, perturb=1.0, N_importance=sf,
                                      network_fine=net_f, raw_noise_std=1.0, _randoms=rnd)
        loss = torch.mean((ret["rgb_map"] - target) ** 2) + torch.mean((ret["rgb0"] - target) ** 2)
        grads = torch.autograd.grad(loss, ([r] if rays_need_grad else []) + params)
        keys = ("rgb_map", "disp_map", "acc_map", "raw", "rgb0", "disp0", "acc0", "z_std")
        return [ret[k].detach().clone() for k in keys] + [g.detach().clone() for g in grads]

    first = once()
    for rep in range(4):
        again = once()
        for i, (a, b) in enumerate(zip(first, again)):
            assert torch.equal(a, b), ("run %d differs from run 0 in item %d" % (rep + 1, i), float((a - b).abs().max()))


def test_batchify_clamp_zeroes_gradient(R):
    """rgb >= 1 is overwritten with 1 in place and its gradient vanishes (reference render.py:404-406)."""
    net = make_net(R, 0)
    with torch.no_grad():
        net.rgb_linear.bias += 30.0            # saturate the colour head
    rays = synth.ray_batch(8, seed=3).cuda().requires_grad_(True)
    ret = R["render"].batchify_rays(rays, chunk=4, network_fn=net, network_query_fn=make_query(R), N_samples=64,
                                    retraw=True, white_bkgd=True)
    assert float(ret["rgb_map"].detach().max()) == 1.0 and ret["rgb_map"].shape == (8, 3)
    ret["rgb_map"].sum().backward()
    assert float(net.rgb_linear.bias.grad.abs().max()) == 0.0


def test_raw2outputs_and_sample_pdf_api(R, golden):
    g = golden("composite")
    raw = t(g["s64/raw"]).cuda().requires_grad_(True)
    d = t(g["s64/rays_d"]).cuda().requires_grad_(True)
    rgb, disp, acc, w, depth = R["render"].raw2outputs(raw, t(g["s64/z"]).cuda(), d, white_bkgd=True,
                                                       _noise=t(g["s64/noise"]).cuda())
    key = "s64/wb1_n1/"
    np.testing.assert_allclose(rgb.detach().cpu().numpy(), g[key + "rgb"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(w.cpu().numpy(), g[key + "weights"], rtol=2e-6, atol=1.5e-7)
    ((rgb * t(g["s64/g_rgb"]).cuda()).sum() + (disp * t(g["s64/g_disp"]).cuda()).sum()
     + (acc * t(g["s64/g_acc"]).cuda()).sum() + (depth * t(g["s64/g_depth"]).cuda()).sum()).backward()
    ref = g[key + "g_raw"]
    got = raw.grad.cpu().numpy()
    for r in range(ref.shape[0]):
        assert np.abs(got[r] - ref[r]).max() <= 2e-4 * (np.abs(ref[r]).max() + 1e-30)
    assert rel_err(d.grad, g[key + "g_rays_d"]) < 2e-4
    sp = golden("sample_pdf")
    s = R["render"].sample_pdf(t(sp["bins"]).cuda(), t(sp["weights"]).cuda(), 128, _u=t(sp["rand/u"]).cuda())
    np.testing.assert_array_equal(s.cpu().numpy(), sp["rand/samples"])
    s = R["render"].sample_pdf(t(sp["bins"]).cuda(), t(sp["weights"]).cuda(), 128, det=True)
    np.testing.assert_array_equal(s.cpu().numpy(), sp["det/samples"])


def test_run_network_matches_oracle_with_grads(R):
    net = make_net(R, 2)
    p = {k: v.clone().requires_grad_(True) for k, v in synth.network_params(seed=2).items()}
    g = torch.Generator().manual_seed(5)
    pts = torch.rand(9, 40, 3, generator=g) * 2 - 1
    vd = torch.nn.functional.normalize(torch.randn(9, 3, generator=g), dim=-1)
    gy = torch.randn(9, 40, 4, generator=g)
    pd, vdd = pts.cuda().requires_grad_(True), vd.cuda().requires_grad_(True)
    out = make_query(R)(pd, vdd, net)
    (out * gy.cuda()).sum().backward()
    pc, vc = pts.clone().requires_grad_(True), vd.clone().requires_grad_(True)
    ref = O.query_network(p, pc, vc)
    (ref * gy).sum().backward()
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), rtol=2e-5, atol=2e-5)
    grad_close(pd.grad, pc.grad.numpy(), "d pts", q=0.99, tol_q=1e-4)
    grad_close(vdd.grad, vc.grad.numpy(), "d viewdirs", q=0.9, tol_q=1e-3)
    for name, prm in net.named_parameters():
        grad_close(prm.grad, p[name].grad.numpy(), name, q=0.999, tol_q=1e-3)


_HEADLINE_ORACLE = {}


def _headline_oracle(n, sc, sf, kind="xavier"):
    """fp32 and fp64 runs of the CPU oracle on the headline inputs (shared by the arithmetics under test)"""
    if kind not in _HEADLINE_ORACLE:
        pc, pf = net_params(0, kind), net_params(1, kind)
        rays = synth.ray_batch(n, seed=1)
        rnd = synth.render_randoms(n, sc, sf, seed=3)
        torch.set_num_threads(max(1, min(64, torch.get_num_threads())))
        with torch.no_grad():
            o32 = O.render_rays(rays, pc, pf, sc, sf, rnd["t_rand"], rnd["u"], rnd["noise_c"], rnd["noise_f"], rowsum="aten")
            dd = lambda d_: {k: v.double() for k, v in d_.items()}
            o64 = O.render_rays(rays.double(), dd(pc), dd(pf), sc, sf, rnd["t_rand"].double(), rnd["u"].double(),
                                rnd["noise_c"].double(), rnd["noise_f"].double())
        _HEADLINE_ORACLE[kind] = (o32, o64)
    return _HEADLINE_ORACLE[kind]


@pytest.mark.parametrize("mode,kind", [("resident", "xavier"), ("fp32", "xavier"), ("resident", "trained"), ("fp32", "trained")])
def test_headline_size_against_oracle(R, mode, kind):
    """(`kind`: xavier weights or both networks after 5000 training steps, tests/trained_weights.py.)  4096 rays x (64 + 128): the BASELINE.json configuration, against the CPU oracle on the same seeded inputs, in
    every arithmetic of the training step (the report carries the moved-ray counts of each).

    Coarse outputs: every ray within 1e-4.  Fine outputs (rgb, acc absolute; disparity relative): every ray whose
    128 new samples sit where the oracle puts them is within 1e-4; each ray beyond the bar owns a sample the
    reference algorithm places discontinuously (search index or `denom < 1e-5` branch differs between the two
    fp32 sides, tests/parity_attribution.py) -- and re-rendering exactly those rays' fine stage on the GPU from the
    ORACLE's merged depths brings every one of them within 1e-4.  The distribution goes to profiles/parity_r02.json."""
    from scnerf_amd.functional import host_linspace
    saved_mode = R["ops"].mlp_arithmetic()
    R["ops"].mlp_arithmetic(mode)
    try:
        _headline_case(R, mode, host_linspace, kind)
    finally:
        R["ops"].mlp_arithmetic(saved_mode)


def _headline_case(R, mode, host_linspace, kind="xavier"):
    n, sc, sf = 4096, 64, 128
    net_c, net_f = make_net(R, 0, kind), make_net(R, 1, kind)
    rays = synth.ray_batch(n, seed=1)
    rnd = synth.render_randoms(n, sc, sf, seed=3)
    rnd_d = {k: v.cuda() for k, v in rnd.items()}
    ret = R["render"].render_rays(rays.cuda(), net_c, make_query(R), sc, retraw=True, perturb=1.0,
                                  N_importance=sf, network_fine=net_f, raw_noise_std=1.0, _randoms=rnd_d)
    o32, o64 = _headline_oracle(n, sc, sf, kind)
    st = PA.gpu_sampling_state(R["ops"], host_linspace, rays.cuda(), net_c, rnd_d["t_rand"], rnd_d["u"], rnd_d["noise_c"], sc)
    np.testing.assert_array_equal(st["z_c"].cpu().numpy(), o32["z_coarse"].numpy())          # stratified depths: bit-exact
    z_c = o32["z_coarse"]
    cls = PA.classify(rnd["u"], 0.5 * (z_c[:, 1:] + z_c[:, :-1]), st["cdf"].cpu(), st["inds"].cpu(), o32["cdf"], o32["inds"])
    moved = cls["index"] | cls["branch"] | cls["illcond"]
    report = {"rays_with_a_discontinuously_placed_sample": int(moved.sum()),
              "rays_index": int(cls["index"].sum()), "rays_branch": int(cls["branch"].sum()),
              "rays_illcond": int(cls["illcond"].sum()),
              "coarse_rerun_bit_identical": bool(torch.equal(st["rgb0"], ret["rgb0"])),
              "sample_indices_equal_fraction": float((st["inds"].cpu() == o32["inds"]).float().mean())}
    key = ("headline_4096x(64+128)" + ("" if kind == "xavier" else "_%s_weights" % kind)
           + ("" if mode == "resident" else "/" + mode))                            # (the default arithmetic: plain key)
    REPORT[key] = report                                     # filled in below; written even if an assertion trips
    for name in ("rgb0", "acc0"):                                                        # coarse: strict
        err = PA.per_ray_error(ret[name], o32[name])
        report[name] = PA.summary(err, cls)
        assert err.max() <= 1e-4, (name, report[name])
    err = PA.per_ray_error(ret["disp0"], o32["disp0"], relative=True)
    report["disp0"] = PA.summary(err, cls)
    assert err.max() <= 1e-4, ("disp0", report["disp0"])
    for name, rel in (("rgb_map", False), ("acc_map", False), ("disp_map", True)):        # fine: attributed
        err = PA.per_ray_error(ret[name], o32[name], relative=rel)
        rep = PA.summary(err, cls)
        rep["vs_fp64_max"] = float(PA.per_ray_error(ret[name], o64[name], relative=rel).max())
        rep["oracle32_vs_fp64_max"] = float(PA.per_ray_error(o32[name], o64[name], relative=rel).max())
        report[name] = rep
        assert rep["over_bar_unexplained"] == 0 and rep["max_among_clean_rays"] <= 1e-4, (name, rep)
        assert rep["over_bar"] <= 0.01 * n, (name, rep)                   # a few dozen rays of 4096, not a tail
        assert rep["vs_fp64_max"] <= max(1e-4, 3 * rep["oracle32_vs_fp64_max"]), (name, rep)   # no further from fp64 than fp32 is
    # the flagged rays, fine stage re-rendered on the GPU from the oracle's merged depths: within the bar, all of them
    idx = torch.from_numpy(np.nonzero(moved)[0])
    if idx.numel():
        sub = rays[idx].cuda().contiguous()
        z_f = o32["z_fine"][idx].cuda().contiguous()
        pts = (sub[:, None, 0:3] + sub[:, None, 3:6] * z_f[:, :, None]).contiguous()
        with torch.no_grad():
            raw = make_query(R)(pts, sub[:, 8:11].contiguous(), net_f)
            rgb, disp, acc, _, _ = R["render"].raw2outputs(raw, z_f, sub[:, 3:6], _noise=rnd["noise_f"][idx].cuda())
        redo = {}
        for name, got, rel in (("rgb_map", rgb, False), ("acc_map", acc, False), ("disp_map", disp, True)):
            e = PA.per_ray_error(got, o32[name][idx], relative=rel)
            redo[name] = float(e.max())
            assert e.max() <= 1e-4, ("re-rendered from the oracle's samples", name, float(e.max()))
        report["flagged_rays_rerendered_from_oracle_samples_max"] = redo
    assert float((ret["z_std"].cpu() - o32["z_std"]).abs()[~torch.from_numpy(moved)].max()) < 1e-5
    REPORT[key] = report
    print("\nheadline parity report (%s):" % mode, json.dumps(report))


def test_weight_gradients_accumulate_into_attached_flat_buffers(R):
    """With every .grad a view of one flat buffer (FusedAdam / FlatGradAllReduce attach them so) the backward
    adds the weight gradients straight into that buffer; the result equals the ordinary autograd
    accumulation, also over two backward passes (gradient accumulation) and with a pre-filled buffer."""
    from scnerf_amd.parallel import FlatGradAllReduce
    n, sc, sf = 64, 64, 128
    rays = synth.ray_batch(n, seed=1).cuda()
    target = synth.target_rgb(n, seed=2).cuda()
    rnd = {k: v.cuda() for k, v in synth.render_randoms(n, sc, sf, seed=3).items()}
    query = make_query(R)

    def run(attach):
        net_c, net_f = make_net(R, 0), make_net(R, 1)
        red = FlatGradAllReduce([net_c, net_f], 1) if attach else None
        if attach:
            assert net_c.attached_flat_grad() is not None and net_f.attached_flat_grad() is not None
            red.flat.fill_(0.25)                              # whatever is there must be added to, not replaced
        else:
            assert net_c.attached_flat_grad() is None
        for _ in range(2):
            ret = R["render"].batchify_rays(rays, chunk=1 << 15, network_fn=net_c, network_query_fn=query, N_samples=sc,
                                         perturb=1.0, N_importance=sf, network_fine=net_f, raw_noise_std=1.0, _randoms=rnd)
            loss = torch.mean((ret["rgb_map"] - target) ** 2) + torch.mean((ret["rgb0"] - target) ** 2)
            loss.backward()
        return [p.grad.clone() for m in (net_c, net_f) for p in m.parameters()]
    plain = run(False)
    attached = run(True)
    for a, b in zip(plain, attached):
        scale = float(a.abs().max()) + 1e-12
        assert float((b - 0.25 - a).abs().max()) <= 2e-6 * scale + 1e-7


def test_headline_size_invariants(R):
    """Size-independent properties at the BASELINE size (4096 x (64 + 128)), no oracle needed:
    sorted merged depths that contain the coarse depths, weights that partition at most unity, colours in
    [0, 1], ray independence (a permuted / split batch renders bit-identically), chunking invariance, and the
    gradient of a sum of per-ray losses being the sum of the per-half gradients."""
    from scnerf_amd import ops
    from scnerf_amd.functional import host_linspace
    n, sc, sf = 4096, 64, 128
    net_c, net_f = make_net(R, 0), make_net(R, 1)
    query = make_query(R)
    rays = synth.ray_batch(n, seed=11).cuda()
    rnd = {k: v.cuda() for k, v in synth.render_randoms(n, sc, sf, seed=13).items()}
    kw = dict(network_fn=net_c, network_query_fn=query, N_samples=sc, perturb=1.0, N_importance=sf,
              network_fine=net_f, raw_noise_std=1.0)
    with torch.no_grad():
        full = R["render"].batchify_rays(rays, chunk=1 << 15, retraw=True, _randoms=rnd, **kw)
        # sampling invariants straight from the kernels
        z_c, _ = ops.coarse_sample(rays, host_linspace(sc, rays.device), rnd["t_rand"], False)
        raw_c = torch.zeros(n, sc, 4, device="cuda")
        raw_c[..., 3] = torch.rand(n, sc, device="cuda") * 5
        _, _, acc_c, w_c, _ = ops.composite_fwd(raw_c, z_c, rays, None, False)
        z_f, pts_f, z_s, z_std, _, _ = ops.fine_sample(rays, z_c, w_c, rnd["u"])
    assert bool((z_c[:, 1:] >= z_c[:, :-1]).all()) and bool((z_f[:, 1:] >= z_f[:, :-1]).all())
    assert z_f.shape == (n, sc + sf)
    # every coarse depth and every new sample is in the merged set (sort of the concatenation)
    ref_sorted = torch.sort(torch.cat([z_c, z_s], -1), -1)[0]
    assert torch.equal(z_f, ref_sorted)
    assert bool((w_c >= 0).all()) and float(w_c.sum(-1).max()) <= 1.0 + 1e-5 and float(acc_c.max()) <= 1.0 + 1e-5
    for k in ("rgb_map", "rgb0"):
        assert float(full[k].min()) >= 0.0 and float(full[k].max()) <= 1.0
    assert torch.isfinite(full["disp_map"]).all() and torch.isfinite(full["raw"]).all()

    # ray independence: a permutation of the batch permutes the outputs, bit for bit; so does chunking
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(5)).cuda()
    with torch.no_grad():
        permuted = R["render"].batchify_rays(rays[perm], chunk=1 << 15, _randoms={k: v[perm] for k, v in rnd.items()}, **kw)
        chunked = torch.cat([R["render"].batchify_rays(rays[a:a + 1000], chunk=384,      # sub-batches AND chunks
                                                       _randoms={k: v[a:a + 1000] for k, v in rnd.items()}, **kw)["rgb_map"]
                             for a in range(0, n, 1000)], 0)
    assert torch.equal(permuted["rgb_map"], full["rgb_map"][perm])
    assert torch.equal(permuted["disp_map"], full["disp_map"][perm])
    assert torch.equal(chunked, full["rgb_map"])

    # additivity of the backward over rays: grad(sum over all rays) == grad(first half) + grad(second half)
    target = synth.target_rgb(n, seed=17).cuda()

    def grads(lo, hi):
        for m in (net_c, net_f):
            for p in m.parameters():
                p.grad = None
        ret = R["render"].batchify_rays(rays[lo:hi], chunk=1 << 15, _randoms={k: v[lo:hi] for k, v in rnd.items()}, **kw)
        (((ret["rgb_map"] - target[lo:hi]) ** 2).sum() + ((ret["rgb0"] - target[lo:hi]) ** 2).sum()).backward()
        return torch.cat([p.grad.reshape(-1) for m in (net_c, net_f) for p in m.parameters()])
    g_all, g_a, g_b = grads(0, n), grads(0, n // 2), grads(n // 2, n)
    scale = float(g_all.abs().max())
    assert float((g_all - (g_a + g_b)).abs().max()) <= 2e-5 * scale


def test_render_rays_with_the_fused_fine_stage_is_bit_identical(R):
    """ops.fused_fine_stage(True): render_rays takes the fine stage as one launch (scnerf_fine_stage_fwd_h3) instead of
    three -- the same device code on the same numbers: every output and every gradient bit for bit (odd ray count: the last
    workgroup's second ray is empty)."""
    n, sc, sf = 1025, 64, 128
    rays = synth.ray_batch(n, seed=1).cuda()
    rnd = {k: v.cuda() for k, v in synth.render_randoms(n, sc, sf, seed=3).items()}
    target = synth.target_rgb(n, seed=2).cuda()
    results = []
    saved = R["ops"].fused_fine_stage()
    try:
        for fused in (False, True):
            R["ops"].fused_fine_stage(fused)
            net_c, net_f = make_net(R, 0), make_net(R, 1)
            rd = rays.clone().requires_grad_(True)
            ret = R["render"].render_rays(rd, net_c, make_query(R), sc, retraw=True, perturb=1.0, N_importance=sf,
                                          network_fine=net_f, raw_noise_std=1.0, _randoms=rnd)
            (torch.mean((ret["rgb_map"] - target) ** 2) + torch.mean((ret["rgb0"] - target) ** 2)).backward()
            results.append(([ret[k].detach() for k in ("rgb_map", "disp_map", "acc_map", "raw", "rgb0", "z_std")],
                            [p.grad.clone() for p in list(net_c.parameters()) + list(net_f.parameters())] + [rd.grad.clone()]))
    finally:
        R["ops"].fused_fine_stage(saved)
    for a, b in zip(results[0][0] + results[0][1], results[1][0] + results[1][1]):
        assert torch.equal(a, b)
