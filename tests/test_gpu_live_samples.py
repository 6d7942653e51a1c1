"""The backward pass on the live samples alone (ops.live_samples, csrc/live_compact.hip) on the MI355X.

A sample whose d_raw row is all +-0 adds exact zeros to every gradient.  The compaction lists the others in ascending order;
the unchanged data-gradient kernel runs on that batch and the weight-gradient GEMMs on its dZ with X gathered from the dense
workspace.  Checked here at P = 300 (a ragged last workgroup) and P = 40 000: the compaction and the gathers word for word
against tests/live_samples_ref.py, the compact dZ rows bit for bit against the dense launch, the weight gradients against
fp64 sums over the dense workspaces with the dense half group as the yardstick, the remapped X maxima as bounds, and one
33-ray training step, live route against dense route.

K: every parameter's largest |difference to fp64| over its largest entry, live group <= K x dense half group.  Both run the
same arithmetic over differently cut chunks, so the ratio scatters around 1; K is the next power of two above the largest
ratio measured on the MI355X over this file's cases (profiles/r10_live_samples.txt has the table)."""
import numpy as np
import pytest
import torch

from scnerf_amd import mlp_layout as ML
from scnerf_amd import synthetic as synth
from tests import live_samples_ref as R

pytestmark = pytest.mark.gpu

K = 4.0                        # largest measured ratio 2.27 (profiles/r10_live_samples.txt)
SC, SF = 64, 128
OFF = ML.PARAM_OFFSETS
CASES = {300: (6, 50), 40000: (200, 200)}      # P -> (rays, samples per ray)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from scnerf_amd import ops as _ops
    _ops.check_layout()
    before = (_ops.wgrad_arithmetic(), _ops.live_samples(), _ops.mlp_arithmetic(), _ops.resident_guard())
    _ops.mlp_arithmetic("resident")                # the live route is the resident arithmetic's: forced, like "half"
    _ops.wgrad_arithmetic("half")
    _ops.resident_guard("off")
    yield _ops
    _ops.wgrad_arithmetic(before[0])
    _ops.live_samples(before[1], min_samples=_ops.LIVE_MIN_SAMPLES)
    _ops.mlp_arithmetic(before[2])
    _ops.resident_guard(before[3])


def _words(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


def _compact(ops, d_raw):
    L = ops.live_compact(d_raw)
    ops.live_counts(L)
    return L


# ---- compaction and gathers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", sorted(CASES))
def test_compaction_and_gathers_equal_the_numpy_restatement(ops, P):
    n_rays, spr = CASES[P]
    lay = ML.layout(3)
    Pp = ML.padded_samples(P)
    rng = np.random.default_rng(P)
    pts = rng.standard_normal((P, 3)).astype(np.float32)
    rays = rng.standard_normal((n_rays, 11)).astype(np.float32)
    save = np.zeros(lay.save_floats(P), np.float32)
    masks = rng.integers(0, 2 ** 32, ML.MASK_WORDS_PER_SAMPLE * Pp, dtype=np.uint32)
    save[lay.save_floats_per_sample * Pp:] = masks.view(np.float32)
    save_d, pts_d, rays_d = (torch.from_numpy(a).cuda() for a in (save.view(np.int32), pts, rays))
    save_d = save_d.view(torch.float32)
    for name, live in R.patterns(P).items():
        d_raw = R.d_raw_with(live)
        want = R.live_index(d_raw)
        L = _compact(ops, torch.from_numpy(d_raw).cuda())
        n, Pl = len(want), ML.padded_samples(len(want))
        assert L.n == n == int(L.count.item()), name
        np.testing.assert_array_equal(L.idx[:Pl].cpu().numpy(), R.padded_index(want, P), err_msg=name)
        np.testing.assert_array_equal(L.xoff[:Pl].cpu().numpy().view(np.uint32), R.xoff_table(want), err_msg=name)
        np.testing.assert_array_equal(_words(L.d_raw[:n]), d_raw[want].view(np.int32), err_msg=name)
        if n == 0:
            continue
        m_l, p_l, v_l = ops.live_gather(L, save_d, pts_d, rays_d[:, 8:11], spr)
        np.testing.assert_array_equal(m_l.cpu().numpy().view(np.uint32), R.gather_masks(masks, P, want), err_msg=name)
        np.testing.assert_array_equal(p_l.cpu().numpy(), pts[want], err_msg=name)
        np.testing.assert_array_equal(v_l.cpu().numpy(), rays[want // spr, 8:11], err_msg=name)
        back = ops.live_scatter_rows(L, p_l).cpu().numpy()
        ref = np.zeros((P, 3), np.float32)
        ref[want] = pts[want]
        np.testing.assert_array_equal(back, ref, err_msg=name)


# ---- one pass: dense against live ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def passes(ops):
    """per P: a full (not lean) forward, the dense data gradients (both instantiations) and the dense half group, then the
    same on the live samples; the fp64 sums over the dense workspaces.  Computed once."""
    from tests.emu_mlp_util import network_params
    lay = ML.layout(3)
    p = network_params(4, 3)
    flat = torch.cat([p[name].reshape(-1) for name, _ in lay.param_shapes]).contiguous().cuda()
    wf, wb, rw = ops.pack_weights(flat, "fwd"), ops.pack_weights(flat, "bwd"), ops.pack_resident(flat, 3)
    out = {}
    for P, (n_rays, spr) in CASES.items():
        g = torch.Generator().manual_seed(100 + P)
        pts = (torch.rand(P, 3, generator=g) * 2.4 - 1.2).contiguous().cuda()
        vd = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=g), dim=-1).contiguous().cuda()
        live = R.patterns(P, seed=P)["random"]
        live[40:75] = False                      # a whole wave tile without a live sample
        d_raw = torch.from_numpy(R.d_raw_with(live, seed=P + 1)).cuda()
        save = torch.full((lay.save_floats(P),), float("nan"), device="cuda")
        mx = ops.ChunkMaxima(P, "cuda")
        ops.mlp_fwd(pts, vd, spr, wf, save, planes=rw, maxima=mx)
        L = _compact(ops, d_raw)
        masks, pts_l, vd_l = ops.live_gather(L, save, pts, vd, spr)
        r = {"P": P, "live": live, "L": L, "mx": mx}
        for ig in (True, False):
            mz = ops.ChunkMaxima(P, "cuda")
            dense = ops.mlp_bwd(d_raw, pts, vd, spr, wb, save, planes=rw, maxima=mz, input_grad=ig)
            ml = ops.live_maxima(L, mx)
            got = ops.mlp_bwd_live(L, masks, pts_l, vd_l, wb, rw, ml, input_grad=ig)
            r["bwd", ig] = (dense, got)
            if ig:
                mx.z.copy_(mz.z)
                mx.scales = mz.scales
                r["mx_live"] = ml
        dense, got = r["bwd", True]
        r["dense"] = ops.nerf_wgrad(save, dense[0], d_raw, P, maxima=mx)
        r["got"] = ops.nerf_wgrad_live(L, save, got[0], d_raw, r["mx_live"])
        r["ref"] = _fp64_reference(save, dense[0], d_raw, P)
        r["save"] = save
        out[P] = r
    return out


def _rows(buf, off, w, P, tiled=True):
    Pp = ML.padded_samples(P)
    blk = buf[off:off + w * Pp]
    if tiled:
        blk = blk.view(Pp // 32, w // 4, 32, 4).permute(0, 2, 1, 3).reshape(Pp, w)
    else:
        blk = blk.view(Pp, w)
    return blk[:P].double()


LEAN_DERIVED = ("views_linears.0.weight", "feature_linear.weight", "feature_linear.bias")


def _fp64_reference(save, grads, d_raw, P, lean=False):
    """every parameter's gradient as a direct fp64 sum over the samples, from the dense workspaces (on the device);
    lean workspaces: without the three tensors whose operands they do not hold"""
    so, _ = ML.section_offsets(ML.layout(3).save_sections, P)
    go, _ = ML.section_offsets(ML.GRAD_SECTIONS, P)
    act = [_rows(save, so["act%d" % l], 256, P) for l in range(8)]
    epts = _rows(save, so["epts"], 64, P, tiled=False)[:, :63]
    eviews = _rows(save, so["eviews"], 32, P, tiled=False)[:, :27]
    feat, hv = _rows(save, so["feat"], 256, P), _rows(save, so["hv"], 128, P)
    dz = [_rows(grads, go["dz%d" % l], 256, P) for l in range(8)]
    dfeat, dzv = _rows(grads, go["dfeat"], 256, P), _rows(grads, go["dzv"], 128, P)
    dr = d_raw.reshape(P, 4).double()
    ref = {}
    for l in range(8):
        x = epts if l == 0 else (torch.cat([epts, act[4]], 1) if l == 5 else act[l - 1])
        ref["pts_linears.%d.weight" % l] = dz[l].T @ x
        ref["pts_linears.%d.bias" % l] = dz[l].sum(0)
    ref["views_linears.0.weight"] = dzv.T @ torch.cat([feat, eviews], 1)
    ref["views_linears.0.bias"] = dzv.sum(0)
    ref["feature_linear.weight"] = dfeat.T @ act[7]
    ref["feature_linear.bias"] = dfeat.sum(0)
    ref["alpha_linear.weight"] = dr[:, 3:4].T @ act[7]
    ref["alpha_linear.bias"] = dr[:, 3].sum(0, keepdim=True)
    ref["rgb_linear.weight"] = dr[:, :3].T @ hv
    ref["rgb_linear.bias"] = dr[:, :3].sum(0)
    return {k: v.cpu().numpy() for k, v in ref.items() if not (lean and k in LEAN_DERIVED)}


def _param(flat, name, shape):
    return np.asarray(flat)[OFF[name]:OFF[name] + int(np.prod(shape))].reshape(shape)


def judge(what, got_flat, yard_flat, ref):
    """-> {parameter: error ratio}; asserts the K bound for every parameter"""
    ratios = {}
    for name, shape in ML.PARAM_SHAPES:
        if name not in ref:
            continue
        scale = np.abs(ref[name]).max()
        e_got = float(np.abs(_param(got_flat, name, shape) - ref[name].reshape(shape)).max() / scale)
        e_yard = float(np.abs(_param(yard_flat, name, shape) - ref[name].reshape(shape)).max() / scale)
        ratios[name] = e_got / e_yard if e_yard > 0 else (0.0 if e_got == 0 else float("inf"))
        print("[live] %s %s: live %.3e dense %.3e ratio %.2f" % (what, name, e_got, e_yard, ratios[name]))
    for name in ratios:
        assert ratios[name] <= K, (what, name, ratios[name])
    return ratios


@pytest.mark.parametrize("input_grad", [True, False])
@pytest.mark.parametrize("P", sorted(CASES))
def test_data_gradients_on_the_compact_batch_are_the_dense_rows(passes, P, input_grad):
    r = passes[P]
    dense, got = r["bwd", input_grad]
    live, n = r["live"], r["L"].n
    idx = torch.from_numpy(np.flatnonzero(live)).cuda()
    dead = torch.from_numpy(np.flatnonzero(~live)).cuda()
    assert n == idx.numel()
    go, _ = ML.section_offsets(ML.GRAD_SECTIONS, P)
    gl, _ = ML.section_offsets(ML.GRAD_SECTIONS, n)
    for name, w in ML.GRAD_SECTIONS:
        a = _rows(dense[0], go[name], w, P).float()
        b = _rows(got[0], gl[name], w, n).float()
        assert torch.equal(a[idx].view(torch.int32), b.view(torch.int32)), name
        assert not a[dead].any(), name                          # the dead rows of the dense launch are all +-0
    if input_grad:
        for a, b in ((dense[1], got[1]), (dense[2], got[2])):
            assert torch.equal(a[idx].view(torch.int32), b.view(torch.int32))
            assert not a[dead].any()
    else:
        assert got[1] is None and got[2] is None


@pytest.mark.parametrize("P", sorted(CASES))
def test_weight_gradients_against_fp64_with_the_dense_half_group_as_yardstick(passes, P):
    r = passes[P]
    got, dense = r["got"].cpu().numpy(), r["dense"].cpu().numpy()
    assert np.isfinite(got).all(), [name for name, shape in ML.PARAM_SHAPES if not np.isfinite(_param(got, name, shape)).all()]
    judge("P=%d" % P, got, dense, r["ref"])
    for name, shape in ML.PARAM_SHAPES:
        if name.startswith(("alpha_linear", "rgb_linear")):     # vecmat / rows4 stay dense: the dense group's bits
            np.testing.assert_array_equal(_param(got, name, shape).view(np.int32), _param(dense, name, shape).view(np.int32), err_msg=name)


@pytest.mark.parametrize("P", sorted(CASES))
def test_remapped_x_maxima_bound_the_gathered_rows(passes, P):
    r = passes[P]
    L, ml = r["L"], r["mx_live"]
    so, _ = ML.section_offsets(ML.layout(3).save_sections, P)
    idx = L.idx[:L.n].long()
    bound = ml.x.cpu().numpy()
    for job in range(8):                                        # X of trunk layers 1 .. 7 and of feature_linear: act 0 .. 7
        dense_rows = _rows(r["save"], so["act%d" % job], 256, P).abs().max(dim=1).values
        rows, first = dense_rows[idx].cpu().numpy(), float(dense_rows[0])
        for c in range(ml.chunks):
            part = rows[c * ml.chunk_samples:(c + 1) * ml.chunk_samples]
            assert bound[job, c] >= (part.max() if len(part) else 0.0), (job, c)
            if c * ml.chunk_samples < ML.padded_samples(L.n) and (c + 1) * ml.chunk_samples > L.n:
                assert bound[job, c] >= first, (job, c)         # the padding entries of the chunk read sample 0


# ---- one training step, live route against dense route ------------------------------------------------------------------
def _nets(alpha_bias=None, params=None):
    from scnerf_amd import run_nerf_helpers as H
    out = []
    for seed in (0, 1):
        net = H.NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
        sd = synth.network_params(seed=seed) if params is None else params[seed]
        if alpha_bias is not None:
            sd["alpha_linear.bias"] = torch.full_like(sd["alpha_linear.bias"], alpha_bias)
        net.load_state_dict(sd)
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
def lean_setting(ops):
    before = ops.lean_workspace()
    yield ops.lean_workspace
    ops.lean_workspace(before)


@pytest.mark.parametrize("lean", [False, True])
def test_training_step_live_route_against_dense_route(ops, monkeypatch, lean_setting, lean):
    """lean off: every parameter against fp64 sums over the dense route's workspaces.  lean on: the workspaces hold neither
    feature nor d feature, so the three tensors derived from them (unchanged finishing kernel) are left to the lean-off
    case and the others are judged the same way."""
    lean_setting(lean)
    nets = _nets()
    n = 33
    ops.live_samples(False)
    caught = []
    real = ops.nerf_wgrad

    def spy(save, grads, d_raw, P, **kw):
        caught.append((save, grads, d_raw, P))
        return real(save, grads, d_raw, P, **kw)
    monkeypatch.setattr(ops, "nerf_wgrad", spy)
    out_d, flat_d, rays_d = _step(nets, n)
    monkeypatch.setattr(ops, "nerf_wgrad", real)
    assert len(caught) == 2
    ops.live_samples(True, min_samples=1)
    routed = []
    real_live = ops.nerf_wgrad_live
    monkeypatch.setattr(ops, "nerf_wgrad_live", lambda L, *a, **kw: (routed.append((L.n, L.P)), real_live(L, *a, **kw))[1])
    out_l, flat_l, rays_l = _step(nets, n)
    assert [P for _, P in routed] == [n * (SC + SF), n * SC] and all(0 < m < P for m, P in routed), routed
    for k in out_d:
        assert torch.equal(out_d[k], out_l[k]), k
    assert torch.equal(rays_d, rays_l)
    # the fine pass first, then the coarse pass (RenderRaysFunction.backward); flat[0] is the coarse network's
    for which, (save, grads, d_raw, P) in zip((1, 0), caught):
        ref = _fp64_reference(save, grads, d_raw, P, lean=lean)
        got, dense = flat_l[which].cpu().numpy(), flat_d[which].cpu().numpy()
        judge("step (lean %s), network %d" % (lean, which), got, dense, ref)
        if lean:
            # The three derived tensors, live against dense.  Both come from the views layer's narrow GEMM and the fp64
            # finishing kernel, and each is within K = 4 times the fp32 group's error of the fp64 sums -- at most 4.4e-7 of
            # the largest entry (tests/test_gpu_lean_workspace.py) -- so they differ by at most 2 x 4 x 4.4e-7 = 3.5e-6.
            for name, shape in ML.PARAM_SHAPES:
                if name in LEAN_DERIVED:
                    x, y = _param(got, name, shape), _param(dense, name, shape)
                    rel = float(np.abs(x - y).max() / np.abs(y).max())
                    print("[live] step (lean), network %d %s: live against dense %.3e" % (which, name, rel))
                    assert rel <= 3.5e-6, (which, name, rel)


def test_step_without_a_live_sample_gives_zero_gradients(ops, monkeypatch):
    nets = _nets(alpha_bias=-1e4)                  # every density far below zero: alpha = 0 everywhere
    ops.live_samples(True, min_samples=1)
    counted = []
    real = ops.live_counts
    monkeypatch.setattr(ops, "live_counts", lambda *b: (real(*b), counted.append([(L.n, L.P) for L in b]))[0])
    out, flat, d_rays = _step(nets, 33)
    assert counted == [[(0, 33 * (SC + SF)), (0, 33 * SC)]], counted          # the live route ran, on nothing
    assert not out["acc_map"].any() and not out["acc0"].any()
    for f in flat:
        assert not f.any()
    assert torch.isfinite(d_rays).all()


# ---- under the scale guard: a pass that trips goes back to the dense route ---------------------------------------------
def test_guarded_step_that_trips_takes_the_dense_route(ops, monkeypatch):
    """Hostile weights trip every block of both forwards at layer 3 (tests/test_gpu_resident_guard.py).  With the threshold
    forced down both passes compact, find their forward tripped and run the dense data gradients with the pass's own
    records, where the exact-fp32 rerun finds its workspace: the step is the live-off guarded step bit for bit, in the
    fallback and in the report mode, and the report counts every sample once."""
    from tests import hostile_weights
    nets = _nets(params=[hostile_weights.weights(0), hostile_weights.weights(1)])
    live_launches = []
    real = ops.mlp_bwd_live
    monkeypatch.setattr(ops, "mlp_bwd_live", lambda *a, **kw: (live_launches.append(1), real(*a, **kw))[1])
    trips = []
    real_tripped = ops.live_guard_tripped
    monkeypatch.setattr(ops, "live_guard_tripped", lambda g: (trips.append(real_tripped(g)), trips[-1])[1])
    for mode in ("fallback", "report"):
        ops.resident_guard(mode)
        ops.live_samples(False)
        out_d, flat_d, rays_d = _step(nets, 33)
        m_d = ops.resident_margins()
        ops.live_samples(True, min_samples=1)
        counted = []
        real_counts = ops.live_counts
        monkeypatch.setattr(ops, "live_counts", lambda *b: (real_counts(*b), counted.append([L.n for L in b]))[0])
        out_l, flat_l, rays_l = _step(nets, 33)
        monkeypatch.setattr(ops, "live_counts", real_counts)
        m_l = ops.resident_margins()
        assert len(counted) == 1 and all(n > 0 for n in counted[0]), counted        # both passes compacted ...
        assert not live_launches                                                      # ... and neither ran on its compact batch
        assert trips == [True, True], trips                                           # because its forward had tripped
        del trips[:]
        for k in out_d:
            assert torch.equal(out_d[k], out_l[k]), (mode, k)
        assert torch.equal(rays_d, rays_l), mode
        for a, b in zip(flat_d, flat_l):
            assert torch.equal(a, b), mode
        for name in ("coarse", "fine", "coarse_bwd", "fine_bwd"):
            assert m_l[name] == m_d[name], (mode, name, m_l[name], m_d[name])
            assert m_l[name]["reran_blocks"] == m_l[name]["blocks"] > 0, (mode, name)
    ops.resident_guard("off")
