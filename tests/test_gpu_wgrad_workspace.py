"""The weight-gradient group of a network pass stays inside its workspace on the MI355X (csrc/wgrad.hip).

Through the C ABI, into a workspace of scnerf_nerf_wgrad_workspace_floats(n_chunks) floats followed by 4096 guard words
the test owns: the guard words are unchanged, the flat gradient is finite and a second call gives the same words.
P = 300, 2400, 4100 samples are 1, 9 and 16 chunks (ops.wgrad_chunks): one workgroup per launch, a count the big launch
cannot divide by eight, and the first at which it runs at n_chunks / 8."""
import pytest
import torch

from scnerf_amd import mlp_layout as ML

pytestmark = pytest.mark.gpu

GUARD_WORDS = 4096
GUARD = 0x5AC35AC3                  # a finite float no sum of these inputs produces
NAN = 0x7FC00000
CASES = {300: (6, 50), 2400: (24, 100), 4100: (41, 100)}      # P -> (rays, samples per ray)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from scnerf_amd import ops as _ops
    _ops.check_layout()
    return _ops


@pytest.fixture
def half(ops):
    before = ops.wgrad_arithmetic()
    ops.wgrad_arithmetic("half")
    yield ops
    ops.wgrad_arithmetic(before)


@pytest.fixture(scope="module")
def passes(ops):
    """per (pd, P): the workspaces and chunk maxima of one resident forward and backward pass, computed once"""
    from tests.emu_mlp_util import network_params
    out = {}
    for pd in (3, 4):
        lay = ML.layout(pd)
        p = network_params(4, pd)
        flat = torch.cat([p[name].reshape(-1) for name, _ in lay.param_shapes]).contiguous().cuda()
        wf, wb, rw = ops.pack_weights(flat, "fwd", pd=pd), ops.pack_weights(flat, "bwd", pd=pd), ops.pack_resident(flat, pd)
        for P, (n_rays, spr) in CASES.items():
            g = torch.Generator().manual_seed(100 + P)
            if pd == 3:
                pts = (torch.rand(P, 3, generator=g) * 2.4 - 1.2).contiguous().cuda()
            else:
                unit = torch.nn.functional.normalize(torch.randn(P, 3, generator=g), dim=-1)
                pts = torch.cat([unit, 1.0 - torch.rand(P, 1, generator=g)], -1).contiguous().cuda()
            vd = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=g), dim=-1).contiguous().cuda()
            d_raw = torch.randn(P, 4, generator=g).contiguous().cuda()
            save = torch.full((lay.save_floats(P),), float("nan"), device="cuda")
            mx = ops.ChunkMaxima(P, "cuda")
            ops.mlp_fwd(pts, vd, spr, wf, save, pd=pd, planes=rw, maxima=mx)
            grads, _, _ = ops.mlp_bwd(d_raw, pts, vd, spr, wb, save, pd=pd, planes=rw, maxima=mx)
            assert mx.scales is not None
            out[pd, P] = dict(save=save, grads=grads, d_raw=d_raw, mx=mx, flat=flat)
    return out


def _call(ops, lean, pd, P, R, ws):
    from scnerf_amd import _capi
    lib, mx = _capi.load(), R["mx"]
    g = torch.full((ML.layout(pd).n_params,), float("nan"), device="cuda")
    a = (pd, ops._p(R["save"]), ops._p(R["grads"]), ops._p(R["d_raw"]), P, ops.wgrad_chunks(P), ops._p(ws), ops._p(g), 0,
         ops._p(mx.x), ops._p(mx.z), ops._p(mx.scales))
    if lean:
        _capi.check(lib.scnerf_nerf_wgrad_h3_lean(*a, ops._p(R["flat"]), None, None, ops._stream()), "scnerf_nerf_wgrad_h3_lean")
    else:
        _capi.check(lib.scnerf_nerf_wgrad_h3(*a, None, None, ops._stream()), "scnerf_nerf_wgrad_h3")
    return g


@pytest.mark.parametrize("P", sorted(CASES))
@pytest.mark.parametrize("lean", [False, True], ids=["h3", "h3_lean"])
@pytest.mark.parametrize("pd", [3, 4])
def test_the_group_stays_inside_its_workspace(half, passes, pd, lean, P):
    from scnerf_amd import _capi
    ops, R = half, passes[pd, P]
    chunks = ops.wgrad_chunks(P)
    assert chunks == {300: 1, 2400: 9, 4100: 16}[P]
    n = int(_capi.load().scnerf_nerf_wgrad_workspace_floats(chunks))

    def workspace():
        ws = torch.full((n + GUARD_WORDS,), NAN, dtype=torch.int32, device="cuda")
        ws[n:] = GUARD
        return ws
    ws = workspace()
    g = _call(ops, lean, pd, P, R, ws)
    guard = ws[n:].cpu()
    assert bool((guard == GUARD).all()), "%d guard words changed" % int((guard != GUARD).sum())
    assert bool(torch.isfinite(g).all())
    again = _call(ops, lean, pd, P, R, workspace())
    assert torch.equal(g.view(torch.int32).cpu(), again.view(torch.int32).cpu())
