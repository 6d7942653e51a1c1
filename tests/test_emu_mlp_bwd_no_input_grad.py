"""The resident data-gradient kernel without the input gradient (scnerf_mlp_bwd_h3 with d_pts == d_views == NULL,
csrc/mlp_bwd_h3_kernel.h IG = false) on the CPU SIMT interpreter: every dZ section of the gradient workspace and every
chunk maximum bit-identical to the full kernel's on the same inputs."""
import numpy as np
import pytest
import torch

from scnerf_amd import mlp_layout as ML
from tests.emu import harness as H
from tests.emu_mlp_util import network_params, pack_forward, pack_backward, pack_h3

pytestmark = pytest.mark.emu


def _inputs(pd, n_rays, spr, seed):
    lay = ML.layout(pd)
    p = network_params(seed, pd)
    wpk, wbk = pack_forward(p, pd), pack_backward(p, pd)
    fwd, bwd, sc = pack_h3(p, pd)
    P = n_rays * spr
    g = torch.Generator().manual_seed(seed + 1)
    pts = (torch.rand(P, pd, generator=g) * 2.4 - 1.2).numpy()
    vd = torch.randn(n_rays, 3, generator=g)
    vd = (vd / vd.norm(dim=-1, keepdim=True)).numpy()
    d_raw = torch.randn(P, 4, generator=g) * (10.0 ** torch.randint(-8, 3, (P, 1), generator=g).float())
    d_raw = d_raw.numpy()
    raw = np.zeros((P, 4), np.float32)
    save = np.full(lay.save_floats(P), np.nan, np.float32)
    H.call("scnerf_mlp_fwd_h3", pd, pts, vd, 3, spr, wpk, fwd, sc, raw, save, P, None, 0, 0, None)
    return P, pts, vd, d_raw, wbk, bwd, sc, save


def _bwd(pd, spr, P, pts, vd, d_raw, wbk, bwd, sc, save, chunks, chunk_samples, d_pts, d_views):
    grads = np.full(ML.grad_floats(P), np.nan, np.float32)
    amax = np.zeros((12, chunks), np.float32)
    H.call("scnerf_mlp_bwd_h3", pd, d_raw, pts, vd, 3, spr, wbk, bwd, sc, save, grads, d_pts, d_views, P, amax, chunks,
           chunk_samples, None)
    return grads, amax


@pytest.mark.parametrize("pd,n_rays,spr", [(3, 3, 64), (3, 2, 70), (3, 1, 45), (4, 1, 40)])
def test_no_input_grad_variant_is_bit_identical(pd, n_rays, spr):
    # P = 192, 140, 45, 40: whole and partial last waves, samples_per_ray not a multiple of the wave
    P, pts, vd, d_raw, wbk, bwd, sc, save = _inputs(pd, n_rays, spr, 3 + spr)
    chunk_samples = 64
    chunks = -(-P // chunk_samples)
    d_pts = np.full((P, pd), np.nan, np.float32)
    d_views = np.full((P, 3), np.nan, np.float32)
    g_full, m_full = _bwd(pd, spr, P, pts, vd, d_raw, wbk, bwd, sc, save, chunks, chunk_samples, d_pts, d_views)
    assert np.isfinite(d_pts).all() and np.isfinite(d_views).all()
    g_none, m_none = _bwd(pd, spr, P, pts, vd, d_raw, wbk, bwd, sc, save, chunks, chunk_samples, None, None)
    assert np.array_equal(g_full.view(np.uint32), g_none.view(np.uint32))
    assert np.array_equal(m_full.view(np.uint32), m_none.view(np.uint32))
    assert (m_full[8:] > 0).all()          # the rows the narrow weight-gradient GEMMs scale by were written


def test_exactly_one_input_gradient_buffer_is_an_error():
    pd, spr = 3, 32
    P, pts, vd, d_raw, wbk, bwd, sc, save = _inputs(pd, 1, spr, 11)
    grads = np.full(ML.grad_floats(P), np.nan, np.float32)
    d_pts = np.full((P, pd), np.nan, np.float32)
    d_views = np.full((P, 3), np.nan, np.float32)
    for a, b in ((d_pts, None), (None, d_views)):
        st = H.lib_call_status("scnerf_mlp_bwd_h3", pd, d_raw, pts, vd, 3, spr, wbk, bwd, sc, save, grads, a, b, P, None, 0, 0,
                               None)
        assert st != 0
    assert np.isnan(d_pts).all() and np.isnan(d_views).all()
