"""The resident data-gradient kernel without the input gradient (scnerf_mlp_bwd_h3 with d_pts == d_views == NULL,
csrc/mlp_bwd_h3_kernel.h IG = false) on the CPU SIMT interpreter: every dZ section of the gradient workspace and every
chunk maximum bit-identical to the full kernel's on the same inputs -- also through the guarded export
(scnerf_mlp_bwd_h3_guarded, csrc/resident_guard.h: block flags, the `any` word and the report as well; guarded against
unguarded WITH the input gradient is tests/test_emu_resident_guard.py's) and with the view directions read at the row stride
of a ray batch.  On the MI355X: tests/test_gpu_data_rays.py."""
import numpy as np
import pytest
import torch

from scnerf_amd import mlp_layout as ML
from tests import hostile_weights
from tests.emu import harness as H
from tests.emu_mlp_util import network_params, pack_forward, pack_backward, pack_h3

pytestmark = pytest.mark.emu


def _inputs(pd, n_rays, spr, seed, p=None):
    lay = ML.layout(pd)
    p = network_params(seed, pd) if p is None else p
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


def _bwd(pd, spr, P, pts, vd, d_raw, wbk, bwd, sc, save, chunks, chunk_samples, d_pts, d_views, vd_stride=3, record=None):
    grads = np.full(ML.grad_floats(P), np.nan, np.float32)
    amax = np.zeros((12, chunks), np.float32)
    head = (pd, d_raw, pts, vd, vd_stride, spr, wbk, bwd, sc, save, grads, d_pts, d_views, P, amax, chunks, chunk_samples)
    if record is None:
        H.call("scnerf_mlp_bwd_h3", *head, None)
    else:
        H.call("scnerf_mlp_bwd_h3_guarded", *head, *record, None)
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


def test_no_input_grad_variant_reads_directions_at_the_ray_batch_stride():
    """view directions as columns 8 .. 10 of a [n, 11] ray batch (what render_rays passes): row 11 of the maxima reads them in
    the branch of its own; directions far from unit length tell a wrong row or stride apart"""
    pd, n_rays, spr = 3, 3, 40
    P, pts, vd, d_raw, wbk, bwd, sc, save = _inputs(pd, n_rays, spr, 9)
    rays = np.zeros((n_rays, 11), np.float32)
    rays[:, 8:11] = vd * np.array([[3.0], [5.0], [7.0]], np.float32)
    rays[:, :8] = 1000.0                                    # a read at stride 3, or off by a column, finds these
    dirs = rays.reshape(-1)[8:]                             # the kernel's view: row r at dirs + 11 r
    chunk_samples = 32
    chunks = -(-P // chunk_samples)
    d_pts = np.full((P, pd), np.nan, np.float32)
    d_views = np.full((P, 3), np.nan, np.float32)
    g_full, m_full = _bwd(pd, spr, P, pts, dirs, d_raw, wbk, bwd, sc, save, chunks, chunk_samples, d_pts, d_views, vd_stride=11)
    g_none, m_none = _bwd(pd, spr, P, pts, dirs, d_raw, wbk, bwd, sc, save, chunks, chunk_samples, None, None, vd_stride=11)
    assert np.array_equal(g_full.view(np.uint32), g_none.view(np.uint32))
    assert np.array_equal(m_full.view(np.uint32), m_none.view(np.uint32))
    # row 11 = max(1, |direction|) over the chunk's samples: chunks of 32 samples against rays of 40
    ray_of = np.arange(P) // spr
    want = [max(1.0, float(np.abs(rays[ray_of[c * chunk_samples: (c + 1) * chunk_samples], 8:11]).max())) for c in range(chunks)]
    assert m_none[11].tolist() == want


def _record(P):
    return np.zeros((P + 127) // 128, np.int32), np.zeros(1, np.int32), np.zeros(10 * (64 + 2), np.float32)   # resident_guard.h


@pytest.mark.parametrize("kind", ["xavier", "hostile"])
def test_guarded_no_input_grad_variant_is_bit_identical(kind):
    """scnerf_mlp_bwd_h3_guarded with both input-gradient buffers NULL against both given: the gradient workspace, the chunk
    maxima, the block flags, the `any` word and the report word for word -- on a network that trips nothing and on one whose
    data gradients trip in every block.  (tests/hostile_weights.py is aimed at the forward: its cancellation row leaves dZ of
    layer 2 at the lower edge of the range, margin -3, inside; sixteen times that row -- its pre-activation is still exactly its
    bias -- puts W_3^T dZ_3 four octaves further below its scale.)"""
    pd, n_rays, spr = 3, 3, 50                              # 150 samples: two blocks, the second ragged
    p = None
    if kind == "hostile":
        p = hostile_weights.weights(0)
        p["pts_linears.3.weight"][7] *= 16.0
    P, pts, vd, d_raw, wbk, bwd, sc, save = _inputs(pd, n_rays, spr, 5, p=p)
    chunk_samples = 64
    chunks = -(-P // chunk_samples)
    d_pts = np.full((P, pd), np.nan, np.float32)
    d_views = np.full((P, 3), np.nan, np.float32)
    rec_full, rec_none = _record(P), _record(P)
    g_full, m_full = _bwd(pd, spr, P, pts, vd, d_raw, wbk, bwd, sc, save, chunks, chunk_samples, d_pts, d_views, record=rec_full)
    g_none, m_none = _bwd(pd, spr, P, pts, vd, d_raw, wbk, bwd, sc, save, chunks, chunk_samples, None, None, record=rec_none)
    assert np.isfinite(d_pts).all() and np.isfinite(d_views).all()
    assert np.array_equal(g_full.view(np.uint32), g_none.view(np.uint32))
    assert np.array_equal(m_full.view(np.uint32), m_none.view(np.uint32))
    for a, b, what in zip(rec_full, rec_none, ("flags", "any", "report")):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), what
    flags, any_, report = rec_none
    assert report[:10 * 64].max() > 0                       # the guard looked
    if kind == "hostile":
        assert flags.all() and any_[0] == 1
        assert report[10 * 64 + 2 * 2] > 0                  # samples under the range at dZ of layer 2
    else:
        assert not flags.any() and any_[0] == 0 and not report[10 * 64:].any()


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
