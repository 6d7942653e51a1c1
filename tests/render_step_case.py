"""TEST INFRASTRUCTURE: the body of the gate- and sample-aligned training-step comparison, shared by the GPU tests
(tests/test_gpu_render.py) and their twin on the CPU SIMT interpreter (tests/test_emu_render_step.py): one `render_rays`
training step of the package against the CPU oracle running the whole step on the package's own new depths and with the
package's own ReLU decisions.  `device` is "cuda" on the GPU and "cpu" inside tests.emu.host_on_emu.emulated_device."""
import numpy as np
import torch

from oracle import scnerf_oracle as O
from scnerf_amd import synthetic as synth
from tests import parity_attribution as PA

REPORT = PA.REPORT


def modules():
    from scnerf_amd import render, create_nerf, run_nerf_helpers, ops
    return dict(render=render, create_nerf=create_nerf, helpers=run_nerf_helpers, ops=ops)


def net_params(seed, kind="xavier"):
    """`kind` (tests/trained_weights.py): "xavier" = the reference's initialisation; "trained" = the coarse (seed 0) / fine
    (seed 1) network after 5000 steps on the procedural scene"""
    from tests import trained_weights as TW
    return TW.weights(kind, seed, which="coarse" if seed == 0 else "fine")


def make_net(R, seed, kind="xavier", device="cuda"):
    net = R["helpers"].NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
    net.load_state_dict(net_params(seed, kind))
    return net.to(device)


def make_query(R):
    e, _ = R["helpers"].get_embedder(10, 0)
    ed, _ = R["helpers"].get_embedder(4, 0)
    return R["create_nerf"].FusedNetworkQuery(e, ed)


def render_node(tensor):
    """the RenderRaysFunction node behind an output of render_rays (its ctx: .coarse / .fine hold the activation workspaces)"""
    seen, todo = set(), [tensor.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if "RenderRaysFunction" in type(fn).__name__:
            return fn
        todo.extend(f for f, _ in fn.next_functions)
    raise AssertionError("no RenderRaysFunction node behind this tensor")


def kernel_gates(save, P, pd=3):
    """the ReLU decisions the training forward took, from the bit masks behind its activation workspace:
    -> 8 x bool [P, 256] (trunk) + bool [P, 128] (views layer)"""
    from scnerf_amd import mlp_layout as ML
    from tests.test_gpu_kernels import _gates_from_masks
    lay = ML.layout(pd)
    _, total = ML.section_offsets(lay.save_sections, P)
    masks = save[total:].cpu().numpy().view(np.uint32).reshape(9, ML.padded_samples(P) // 32, 64, 4)
    return [torch.from_numpy(_gates_from_masks(masks[l], P, 8 if l < 8 else 4)) for l in range(9)]


def report_key(n, kind, mode, data_rays, sc=64, sf=128, lindisp=False, white_bkgd=False, perturb=1.0, shared_net=False,
               attached=False):
    """(the six headline-size cases keep the keys they always had)"""
    return "training_gradients_discontinuities_aligned_%dx(%d+%d)%s%s%s%s%s%s%s%s" % (
        n, sc, sf, "" if kind == "xavier" else "_%s_weights" % kind, "" if mode is None else "/" + mode,
        "_data_rays" if data_rays else "", "_lindisp" if lindisp else "", "_white_bkgd" if white_bkgd else "",
        "" if perturb > 0 else "_no_perturb", "_shared_net" if shared_net else "", "_attached_flat_grad" if attached else "")


def aligned_gradients_case(R, n, kind, mode, host_linspace, data_rays=False, sc=64, sf=128, lindisp=False, white_bkgd=False,
                           perturb=1.0, shared_net=False, attached=False, device="cuda"):
    """`shared_net`: network_fine=None with N_importance > 0 -- one network serves both stages (reference render.py:279) and
    the oracle gets the same parameter dict for both, so autograd sums the two stages; `attached`: that network's .grad
    tensors are views of one flat buffer pre-filled with 0.25, which the backward adds to (0.25 is subtracted before the
    comparison); `perturb` 0: no t_rand, the shared deterministic u row; sf == 0: no fine stage -- only the coarse gates
    are imposed and rgb_map, acc_map, the loss, the coarse network's gradients and the ray gradient compared."""
    fine = sf > 0
    two_nets = fine and not shared_net
    net_c = make_net(R, 0, kind, device)
    net_f = make_net(R, 1, kind, device) if two_nets else None
    if attached:
        from scnerf_amd.parallel import FlatGradAllReduce
        red = FlatGradAllReduce([net_c] + ([net_f] if two_nets else []), 1)
        assert net_c.attached_flat_grad() is not None
        red.flat.fill_(0.25)                              # whatever is there must be added to, not replaced
    rays = synth.ray_batch(n, seed=11, lindisp=lindisp)
    rnd = synth.render_randoms(n, sc, sf, seed=12)
    if not perturb > 0:
        rnd = {k: v for k, v in rnd.items() if k.startswith("noise")}
    rnd_d = {k: v.to(device) for k, v in rnd.items()}
    t_rand, u, noise_c, noise_f = rnd.get("t_rand"), rnd.get("u"), rnd["noise_c"], rnd.get("noise_f")
    target = torch.rand(n, 3, generator=torch.Generator().manual_seed(13))
    rays_d = rays.clone().to(device).requires_grad_(not data_rays)     # (a copy on the CPU too: `rays` stays plain data)
    ret = R["render"].render_rays(rays_d, net_c, make_query(R), sc, retraw=True, lindisp=lindisp, perturb=float(perturb),
                                  N_importance=sf, network_fine=net_f, white_bkgd=white_bkgd, raw_noise_std=1.0,
                                  _randoms=rnd_d)
    node = render_node(ret["rgb_map"])
    gates_c = kernel_gates(node.coarse[4], n * sc)
    gates_f = kernel_gates(node.fine[4], n * (sc + sf)) if fine else None
    loss = torch.mean((ret["rgb_map"] - target.to(device)) ** 2)
    if fine:
        loss = loss + torch.mean((ret["rgb0"] - target.to(device)) ** 2)
    loss.backward()
    pc = {k: v.clone().requires_grad_(True) for k, v in net_params(0, kind).items()}
    pf = {k: v.clone().requires_grad_(True) for k, v in net_params(1, kind).items()} if two_nets else None
    rays_o = rays.clone().requires_grad_(True)
    kw = dict(rowsum="aten", lindisp=lindisp, white_bkgd=white_bkgd)
    if fine:
        u_dev = rnd_d["u"] if perturb > 0 else host_linspace(sf, device)
        st = PA.gpu_sampling_state(R["ops"], host_linspace, rays.to(device), net_c, rnd_d.get("t_rand"), u_dev, rnd_d["noise_c"],
                                   sc, lindisp, white_bkgd)
        assert torch.equal(st["rgb0"], ret["rgb0"].detach())            # the re-run IS the coarse stage of the run above
        kw["z_samples"] = st["z_s"].cpu()
    rec = {}
    with torch.no_grad():                                               # the oracle's own decisions, for the count
        own = O.render_rays(rays, pc, pf, sc, sf, t_rand, u, noise_c, noise_f, record_gates=rec, **kw)
    theirs, ours = rec["coarse"] + (rec["fine"] if fine else []), gates_c + (gates_f if fine else [])
    flips = sum(int((a != b).sum()) for a, b in zip(theirs, ours))
    n_gates = sum(a.numel() for a in theirs)
    assert flips <= 1e-5 * n_gates, (flips, n_gates)                    # a handful of 1e8 (measured: see the report)
    o = O.render_rays(rays_o, pc, pf, sc, sf, t_rand, u, noise_c, noise_f, gates_coarse=gates_c, gates_fine=gates_f, **kw)
    if fine:
        np.testing.assert_array_equal(o["z_fine"].detach().numpy(), st["z_f"].cpu().numpy())   # identical merged depths
    # imposing the gates moves nothing visible: a flipped unit's pre-activation is a rounding from zero
    assert float((o["raw"].detach() - own["raw"]).abs().max()) <= 1e-5
    loss_o = torch.mean((o["rgb_map"] - target) ** 2)
    if fine:
        loss_o = loss_o + torch.mean((o["rgb0"] - target) ** 2)
    loss_o.backward()
    for name in ("rgb_map", "acc_map") + (("rgb0", "acc0") if fine else ()):                # every ray, no attribution needed
        np.testing.assert_allclose(ret[name].detach().cpu().numpy(), o[name].detach().numpy(), rtol=0, atol=1e-4, err_msg=name)
    np.testing.assert_allclose(float(loss.detach()), float(loss_o.detach()), rtol=2e-6)
    rep = {}
    for tag, net, p in (("coarse", net_c, pc),) + ((("fine", net_f, pf),) if two_nets else ()):
        for pn, prm in net.named_parameters():
            ref = p[pn].grad.numpy()
            got = prm.grad.detach().cpu().numpy()
            if attached:
                got = got - np.float32(0.25)
            e = np.abs(got - ref).reshape(-1) / (np.abs(ref).max() + 1e-30)
            # (the 99.9 % quantile of a tensor with fewer than 2000 entries IS its largest entries: only the max bound applies)
            rep[tag + "/" + pn] = [float(np.quantile(e, 0.999)) if e.size >= 2000 else 0.0, float(e.max())]
    worst = max(rep, key=lambda k_: rep[k_][1])
    entry = dict(relu_decisions=n_gates, relu_decisions_differing_from_the_oracles_own=flips,
                 worst_q999=max(v[0] for v in rep.values()), worst_max=rep[worst][1], worst_parameter=worst)
    if data_rays:
        assert rays_d.grad is None
    else:
        cols = [0, 1, 2, 3, 4, 5, 8, 9, 10]
        ge = np.abs(rays_d.grad[:, cols].cpu().numpy() - rays_o.grad[:, cols].numpy()).max(1) / np.abs(rays_o.grad.numpy()).max()
        entry["d_ray_batch_worst_ray"] = float(ge.max())
    REPORT[report_key(n, kind, mode, data_rays, sc, sf, lindisp, white_bkgd, perturb, shared_net, attached)] = dict(entry)
    entry["loss_rel"] = abs(float(loss.detach()) - float(loss_o.detach())) / abs(float(loss_o.detach()))
    for key, (q999, mx) in rep.items():
        assert q999 <= 2e-5 and mx <= 1e-4, (key, q999, mx)
    if not data_rays:
        assert ge.max() <= 1e-4, float(ge.max())
    return entry
