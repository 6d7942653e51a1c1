"""Where a network pass's weight-gradient group writes in its workspace (csrc/wgrad.hip), under the CPU SIMT interpreter.

scnerf_nerf_wgrad_workspace_floats(n_chunks) is what a caller allocates; the partial slabs of every GEMM are laid out
from its start and the lean group's scratch (M [128][256], s [128]) fills its last 128 * 256 + 128 floats.  Behind a
workspace of exactly that size stand 4096 guard words: no entry, point dimension or chunking may change one of them, the
result must not depend on what lies behind the workspace, the slabs must end below the scratch, and only the lean
group may write the scratch."""
import functools

import numpy as np
import pytest
import torch

from scnerf_amd import mlp_layout as ML
from tests.emu import harness as H
from tests.emu_mlp_util import flat_params, network_params, pack_backward, pack_forward, pack_h3

pytestmark = pytest.mark.emu

GUARD_WORDS = 4096
GUARD = 0x5AC35AC3                  # a finite float no sum of these inputs produces
NAN = 0x7FC00000                    # the prefill (np.nan as fp32)
SCRATCH = 128 * 256 + 128
NO_GUARD = (None, None, None)
ENTRIES = ("nerf_wgrad", "h3", "h3_without_scales", "h3_fp32_arithmetic", "h3_lean")
# (P, n_chunks): a partial 128-block; n_chunks no multiple of 8 (the big launch keeps 3 chunks); trailing chunks own no samples
SHAPES = {(170, 2): (5, 34), (300, 3): (6, 50), (300, 16): (6, 50)}


@functools.lru_cache(maxsize=None)
def _operands(pd, P, chunks):
    """the workspaces and chunk maxima of one resident forward and backward pass (computed once per case, never modified)"""
    lib, lay = H.lib(), ML.layout(pd)
    n_rays, spr = SHAPES[P, chunks]
    p = network_params(3, pd)
    gen = torch.Generator().manual_seed(17)
    if pd == 3:
        pts = (torch.rand(P, 3, generator=gen) * 2.4 - 1.2).numpy()
    else:
        unit = torch.nn.functional.normalize(torch.randn(P, 3, generator=gen), dim=-1)
        pts = torch.cat([unit, 1.0 - torch.rand(P, 1, generator=gen)], -1).contiguous().numpy()
    vd = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=gen), dim=-1).numpy()
    d_raw = torch.randn(P, 4, generator=gen).numpy()
    fwd, bwd, sc = pack_h3(p, pd)
    nb = lib.scnerf_wgrad256_chunks(chunks)
    cs = lib.scnerf_wgrad_chunk_samples(P, nb)
    mx, mz = np.zeros((12, nb), np.float32), np.zeros((12, nb), np.float32)
    raw = np.zeros((P, 4), np.float32)
    save = np.full(lay.save_floats(P), np.nan, np.float32)
    H.call("scnerf_mlp_fwd_h3_lean", pd, pts, vd, 3, spr, pack_forward(p, pd), fwd, sc, raw, save, P, mx, nb, cs, *NO_GUARD, 0, None)
    grads = np.full(ML.grad_floats(P), np.nan, np.float32)
    d_pts, d_views = np.full((P, pd), np.nan, np.float32), np.full((P, 3), np.nan, np.float32)
    H.call("scnerf_mlp_bwd_h3_lean", pd, d_raw, pts, vd, 3, spr, pack_backward(p, pd), bwd, sc, save, grads, d_pts, d_views, P,
           mz, nb, cs, *NO_GUARD, 0, None)
    out = dict(save=save, grads=grads, d_raw=d_raw, mx=mx, mz=mz, sc=sc, params=flat_params(p, pd))
    for a in out.values():
        a.setflags(write=False)
    return out


def _call(entry, pd, P, chunks, ws):
    """one weight-gradient group into the float view of `ws` (uint32 words) -> the flat gradient's words"""
    o = _operands(pd, P, chunks)
    lib = H.lib()
    g = np.full(ML.layout(pd).n_params, np.nan, np.float32)
    a = (pd, o["save"], o["grads"], o["d_raw"], P, chunks, ws.view(np.float32), g, 0)
    if entry == "nerf_wgrad":
        H.call("scnerf_nerf_wgrad", *a, None)
    elif entry == "h3_lean":
        H.call("scnerf_nerf_wgrad_h3_lean", *a, o["mx"], o["mz"], o["sc"], o["params"], None, None, None)
    else:
        if entry == "h3_fp32_arithmetic":
            assert lib.scnerf_wgrad_arithmetic(0) == 0
        try:
            H.call("scnerf_nerf_wgrad_h3", *a, o["mx"], o["mz"], None if entry == "h3_without_scales" else o["sc"], None, None, None)
        finally:
            assert lib.scnerf_wgrad_arithmetic(1) == 1
    return g.view(np.uint32)


@pytest.mark.parametrize("P,chunks", sorted(SHAPES))
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("pd", [3, 4])
def test_the_group_stays_inside_its_workspace(pd, entry, P, chunks):
    n = H.lib().scnerf_nerf_wgrad_workspace_floats(chunks)
    ws = np.concatenate([np.full(n, NAN, np.uint32), np.full(GUARD_WORDS, GUARD, np.uint32)])
    g = _call(entry, pd, P, chunks, ws)
    assert (ws[n:] == GUARD).all(), "%d guard words changed, the first at +%d" % ((ws[n:] != GUARD).sum(), np.argmax(ws[n:] != GUARD))
    assert np.isfinite(g.view(np.float32)).all()
    exact = np.full(n, NAN, np.uint32)
    np.testing.assert_array_equal(g, _call(entry, pd, P, chunks, exact))
    np.testing.assert_array_equal(ws[:n], exact)                      # every slab where it was, whatever lies behind
    # the partial slabs end below the scratch: from the end of the last written slab up to the scratch the prefill is intact
    scratch = n - SCRATCH
    written = np.flatnonzero(ws[:scratch] != NAN)
    end = int(written[-1]) + 1
    assert 0 < end < scratch
    assert (ws[end:scratch] == NAN).all()
    if entry == "h3_lean":
        assert np.isfinite(ws[scratch:n].view(np.float32)).all()      # M and s
    else:
        assert (ws[scratch:n] == NAN).all()                           # only the lean group has a scratch
