"""The lean workspace for 4-D points (the NeRF++ background network) against the full one on the MI355X: the pt_dims = 4
twin of the kernel-level half of test_gpu_lean_workspace.py, at the same two sizes for the same reasons (P = 300: a partial
128-block; P = 40 000: several chunks per job).

Everything the lean pass still writes must be the full pass's bits; the feature / d feature sections stay unwritten; the
three derived tensors (feature_linear.weight, feature_linear.bias, views_linears.0.weight[:, :256]) are judged against
direct fp64 sums over the FULL pass's saved sections with the exact-fp32-MFMA group on those workspaces as the yardstick.

K = 4 as for 3-D points (test_gpu_lean_workspace.py): lean error <= K x the fp32 group's error, per tensor, error = largest
|difference to fp64| over the tensor's largest entry.  The algebra is the same for both variants, so K is not re-derived
here: a ratio above 4 at pt_dims = 4 would be a defect.  Ratios measured on the MI355X over this file's two cases:
feature_linear.weight 0.51 (P = 300), 1.06 (P = 40 000); views_linears.0.weight[:, :256] 0.37, 0.55; feature_linear.bias
1.79, 3.32 (errors of 1.9e-7 .. 5.9e-7 on the lean side, 1.7e-7 .. 8.1e-7 on the yardstick's; the bias's yardstick is a plain
fp32 sum).  Largest: 3.32, below K; at 3-D points the largest was 3.07, on the same tensor."""
import numpy as np
import pytest
import torch

from scnerf_amd import mlp_layout as ML

pytestmark = pytest.mark.gpu

K = 4.0                        # the project's acceptance factor (test_gpu_lean_workspace.py), unchanged

PD = 4
LAY = ML.layout(PD)
OFF = LAY.param_offsets
N = LAY.n_params
DERIVED = ("feature_linear.weight", "feature_linear.bias", "views_linears.0.weight[:, :256]")
CASES = {300: (6, 50), 40000: (200, 200)}      # P -> (rays, samples per ray): a partial 128-block; several chunks per job
POISON = 0x7FC0BEEF                 # a quiet NaN no kernel produces: a word still holding it was not written


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from scnerf_amd import ops as _ops
    _ops.check_layout()
    return _ops


@pytest.fixture
def modes(ops):
    before = (ops.lean_workspace_scope(), ops.wgrad_arithmetic())
    ops.wgrad_arithmetic("half")
    yield ops
    ops.lean_workspace_scope(before[0])
    ops.wgrad_arithmetic(before[1])


def _words(t):
    return t.contiguous().view(torch.int32).cpu()


def _derived_mask():
    """True where the 4-D layout's flat gradient holds one of the three derived tensors"""
    m = np.zeros(N, bool)
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
    so, _ = ML.section_offsets(LAY.save_sections, P)
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
        print("[lean pd4] %s %s: lean %.3e fp32-MFMA %.3e ratio %.2f" % (what, k, e_lean[k], e_yard[k], ratios[k]))
    for k in DERIVED:
        assert e_lean[k] <= K * e_yard[k], (what, k, e_lean[k], e_yard[k])
    return ratios


@pytest.fixture(scope="module")
def passes(ops):
    """per P: the forward, the data gradients (both input_grad settings) and the weight-gradient groups of a full and a
    lean pass on the same 4-D inputs, computed once (the resident kernels are called with their own packs: whatever
    ops.mlp_arithmetic says)"""
    from tests.emu_mlp_util import network_params
    before = (ops.wgrad_arithmetic(),)
    ops.wgrad_arithmetic("half")
    p = network_params(4, PD)
    flat = torch.cat([p[name].reshape(-1) for name, _ in LAY.param_shapes]).contiguous().cuda()
    wf, wb, rw = ops.pack_weights(flat, "fwd", pd=PD), ops.pack_weights(flat, "bwd", pd=PD), ops.pack_resident(flat, PD)
    out = {}
    for P, (n_rays, spr) in CASES.items():
        g = torch.Generator().manual_seed(100 + P)
        unit = torch.nn.functional.normalize(torch.randn(P, 3, generator=g), dim=-1)
        inv_r = 1.0 - torch.rand(P, 1, generator=g)                  # (0, 1]
        pts = torch.cat([unit, inv_r], -1).contiguous().cuda()
        vd = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=g), dim=-1).contiguous().cuda()
        d_raw = torch.randn(P, 4, generator=g).contiguous().cuda()
        R = {"P": P, "flat": flat, "pts": pts, "vd": vd, "spr": spr, "wb": wb, "rw": rw, "d_raw": d_raw}
        for lean in (False, True):
            save = torch.full((LAY.save_floats(P),), float("nan"), device="cuda")
            mx = ops.ChunkMaxima(P, "cuda")
            raw = ops.mlp_fwd(pts, vd, spr, wf, save, pd=PD, planes=rw, maxima=mx, lean=lean)
            r = {"raw": raw, "save": save, "mx": mx, "x": mx.x.clone()}
            for ig in (True, False):
                mz = ops.ChunkMaxima(P, "cuda")
                grads, d_pts, d_views = ops.mlp_bwd(d_raw, pts, vd, spr, wb, save, pd=PD, planes=rw, maxima=mz, input_grad=ig,
                                                    lean=lean)
                r["bwd", ig] = (grads, d_pts, d_views, mz.z.clone())
                if ig:
                    mx.z.copy_(mz.z)
                    mx.scales = mz.scales
                    r["grads"] = grads
            r["wgrad"] = ops.nerf_wgrad(save, r["grads"], d_raw, P, pd=PD, maxima=mx, lean=lean, flat_params=flat if lean else None)
            R[lean] = r
        ops.wgrad_arithmetic("fp32")
        R["yardstick"] = ops.nerf_wgrad(R[False]["save"], R[False]["grads"], d_raw, P, pd=PD, maxima=R[False]["mx"])
        ops.wgrad_arithmetic("half")
        R["ref"] = _fp64_reference(R[False]["save"], R[False]["grads"], P)
        out[P] = R
    ops.wgrad_arithmetic(before[0])
    return out


@pytest.mark.parametrize("P", sorted(CASES))
def test_forward_writes_the_full_pass_bits_except_the_feature_section(passes, P):
    full, lean = passes[P][False], passes[P][True]
    assert torch.equal(_words(full["raw"]), _words(lean["raw"]))
    assert torch.equal(_words(full["x"]), _words(lean["x"]))                       # the X maxima, row 7 = act7's among them
    off, total = ML.section_offsets(LAY.save_sections, P)
    Pp = ML.padded_samples(P)
    sf, sl = _words(full["save"]), _words(lean["save"])
    for name, w in LAY.save_sections:
        a, b = sf[off[name]:off[name] + w * Pp], sl[off[name]:off[name] + w * Pp]
        if name == "feat":
            assert bool(torch.isnan(lean["save"][off[name]:off[name] + w * Pp]).all()), "the lean pass wrote the feature section"
            assert not bool(torch.isnan(full["save"][off[name]:off[name] + w * Pp]).any())
        else:
            assert torch.equal(a, b), name
    assert torch.equal(sf[total:], sl[total:])                                      # the ReLU bit masks


@pytest.mark.parametrize("input_grad", [True, False])
@pytest.mark.parametrize("P", sorted(CASES))
def test_data_gradients_leave_d_feature_unwritten_and_write_the_full_pass_bits_elsewhere(ops, passes, P, input_grad):
    """the data-gradient kernel through the C ABI into a prefilled workspace: with the flag every word of the d feature section
    still holds the fill and every other word is written and is the ops-level run's -- which is the full pass's outside that
    section; without the flag the section is written in full"""
    from scnerf_amd import _capi
    R = passes[P]
    off, _ = ML.section_offsets(ML.GRAD_SECTIONS, P)
    Pp = ML.padded_samples(P)
    lo, hi = off["dfeat"], off["dfeat"] + 256 * Pp
    vptr, vstride = ops._vd(R["vd"])
    # the ops-level runs: lean against full
    gf, pf, vf, zf = R[False]["bwd", input_grad]
    gl, pl, vl, zl = R[True]["bwd", input_grad]
    a, b = _words(gf), _words(gl)
    assert torch.equal(a[:lo], b[:lo]) and torch.equal(a[hi:], b[hi:])
    assert torch.equal(_words(zf), _words(zl))                                      # the Z maxima
    if input_grad:
        assert pf.shape == (P, PD)
        assert torch.equal(_words(pf), _words(pl)) and torch.equal(_words(vf), _words(vl))
    else:
        assert pf is None and pl is None and vf is None and vl is None
    for lean in (1, 0):
        grads = torch.full((ML.grad_floats(P),), POISON, dtype=torch.int32, device="cuda")
        d_pts = torch.empty((P, PD), device="cuda") if input_grad else None
        d_views = torch.empty((P, 3), device="cuda") if input_grad else None
        mz = ops.ChunkMaxima(P, "cuda")
        st = _capi.load().scnerf_mlp_bwd_h3_lean(PD, ops._p(R["d_raw"]), ops._p(R["pts"]), vptr, vstride, R["spr"], ops._p(R["wb"]),
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
    assert a.shape == (N,)
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
    ops.nerf_wgrad(r["save"], r["grads"], B["d_raw"], B["P"], flat_grad=g, pd=PD, accumulate=True, maxima=r["mx"], lean=True,
                   flat_params=B["flat"])
    assert torch.equal(_words(g), _words(A[True]["wgrad"] + r["wgrad"]))


def test_a_lean_workspace_never_reaches_the_full_group(passes, modes):
    ops = modes
    R = passes[300]
    r = R[True]
    ops.wgrad_arithmetic("fp32")
    with pytest.raises(RuntimeError):
        ops.nerf_wgrad(r["save"], r["grads"], R["d_raw"], R["P"], pd=PD, maxima=r["mx"], lean=True, flat_params=R["flat"])
    ops.wgrad_arithmetic("half")
    with pytest.raises(ValueError):
        ops.nerf_wgrad(r["save"], r["grads"], R["d_raw"], R["P"], pd=PD, maxima=None, lean=True, flat_params=R["flat"])
    with pytest.raises(ValueError):                    # (the 3-D network's parameter buffer is not this network's)
        ops.nerf_wgrad(r["save"], r["grads"], R["d_raw"], R["P"], pd=PD, maxima=r["mx"], lean=True,
                       flat_params=R["flat"][:ML.layout(3).n_params].contiguous())
