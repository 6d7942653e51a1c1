"""The occupancy grid of ops.inference_occupancy: a bit per cell of an R x R x R lattice over an axis-aligned box [lo, hi)
in the space the network sees (after the NDC warp where there is one), baked from the trained density; forward-only
render_rays calls skip the network on the samples whose cell it calls empty (csrc/occupancy.hip).

    grid = OccupancyGrid.bake((net_c, net_f), lo, hi, resolution=128, probes=2)
    ops.inference_occupancy(grid)          # ... render_path ...
    ops.inference_occupancy("off")

The NeRF++ node has a switch of its own with one grid per network: a euclidean grid over the
foreground network and an inverted-sphere grid (space = "inverted_sphere") over the background network's (x', y', z', 1 / r):

    fg_grid, bg_grid = bake_nerfpp(nerf_nets, resolution=128, probes=2)
    ops.inference_occupancy_nerfpp(fg_grid, bg_grid)          # ... render_single_image ...
    ops.inference_occupancy_nerfpp("off")

Bake after loading a checkpoint and bake again after training on: a baked grid remembers its networks and their weight
versions and refuses to serve others (OccupancyStaleError).  No arithmetic happens here: the lattice points, the threshold,
the bit words and the dilation are HIP launches (ops.occ_*), the densities are ops.mlp_fwd's."""
from __future__ import annotations

import weakref

import numpy as np
import torch

from . import ops

MAX_PASS_POINTS = 1 << 21           # probe points per baking pass: the workspace of a pass is bounded by it
SPACES = ("euclidean", "inverted_sphere")
_SPACE_OF_PD = {3: "euclidean", 4: "inverted_sphere"}       # the space that fits a network's points


class OccupancyStaleError(RuntimeError):
    """The grid was baked from other networks, or from these networks with other weights."""


def _triple(v, name):
    a = np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float32).reshape(-1)
    if a.shape[0] == 1:
        a = np.repeat(a, 3)
    if a.shape[0] != 3 or not np.isfinite(a).all():
        raise ValueError("%s is three finite numbers" % name)
    return a


def _weights_key(net):
    """what autograd knows about the identity of a network's weights: the flat buffer's address and version and every
    parameter's version (what ops.inference_packs keys its cache on)"""
    flat = net.flat_parameters()
    return (flat.data_ptr(), flat._version, tuple(p._version for p in net.parameters()))


class OccupancyGrid:
    """bits: int32 [R^3 / 32] on the device, cell (x, y, z) = bit c & 31 of word c >> 5, c = (z R + y) R + x.  lo, hi: the
    box, fp32; inv = R / (hi - lo), computed once here in fp32 -- a sample's cell is floor((p - lo) * inv).
    space: "euclidean" -- the box lies in the space of a network on 3-D points -- or "inverted_sphere" -- the grid of a
    NeRF++ background network on (x', y', z', w = 1 / r): the box lies in q = (x' w, y' w, z' w), the unit ball."""

    def __init__(self, bits, lo, hi, resolution, bound=(), space="euclidean"):
        if space not in SPACES:
            raise ValueError("space is one of %s, not %r" % (SPACES, space))
        self.space = space
        R = int(resolution)
        if R < 32 or R > 512 or R % 32:
            raise ValueError("resolution is a multiple of 32 from 32 to 512, not %r" % (resolution,))
        lo, hi = _triple(lo, "lo"), _triple(hi, "hi")
        if not (hi > lo).all():
            raise ValueError("the box needs lo < hi on every axis")
        if bits.dtype != torch.int32 or bits.numel() != R ** 3 // 32:
            raise ValueError("bits is int32 [R^3 / 32]")
        self.bits = bits.contiguous().view(-1)
        self.resolution = R
        self._lo, self._hi = lo, hi
        inv = np.float32(R) / (hi - lo)
        self.lo = tuple(float(x) for x in lo)
        self.hi = tuple(float(x) for x in hi)
        self.inv = tuple(float(x) for x in inv.astype(np.float32))
        self.cell = tuple(float(x) for x in ((hi - lo) / np.float32(R)).astype(np.float32))
        self._bound = tuple(bound)          # ((weak reference to a network, its weights' key), ...)

    # ---- construction ------------------------------------------------------------------------------------------------
    @classmethod
    def from_mask(cls, mask, lo, hi, space="euclidean"):
        """mask: a [R, R, R] bool tensor indexed [z, y, x].  A grid made by hand: bound to no network, checks nothing."""
        if mask.dim() != 3 or mask.dtype != torch.bool or not (mask.shape[0] == mask.shape[1] == mask.shape[2]):
            raise ValueError("mask is a [R, R, R] bool tensor")
        R = mask.shape[0]
        if R % 32:
            raise ValueError("resolution is a multiple of 32")
        w = mask.reshape(-1, 32).to(torch.int64) << torch.arange(32, dtype=torch.int64, device=mask.device)
        words = w.sum(1)
        words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)
        return cls(words, lo, hi, R, space=space)

    @classmethod
    def bake(cls, networks, lo, hi, resolution=128, probes=1, sigma_min=0.0, dilate=1, space="euclidean"):
        """networks: the NeRF modules whose density decides (the coarse and the fine one), all standard, on one device.
        A cell is set when the largest pre-activation density raw[..., 3] over its probes^3 lattice points (offsets
        (j + 0.5) / probes) and over all networks is > sigma_min -- with sigma_min = 0: relu(sigma) is non-zero somewhere we
        looked; a NaN density sets the cell.  Then `dilate` rounds of one-cell 26-neighbourhood dilation.  The density of
        the standard network does not depend on the view direction: a unit direction is passed.  Runs in passes of at most
        2^21 probe points through ops.mlp_fwd in the arithmetic in force.
        space "inverted_sphere": the networks take 4-D points (a NeRF++ background network); the lattice points q of the box
        become the probes (q / |q|, min(|q|, 1)) (ops.occ_probe_points_inverted) -- a lattice point outside the unit ball is
        probed on the sphere, which is conservative for the cells that straddle it.  A network whose points do not fit the
        space -- 3-D: euclidean, 4-D: inverted_sphere -- is refused."""
        if space not in SPACES:
            raise ValueError("space is one of %s, not %r" % (SPACES, space))
        nets =[n for n in (networks if isinstance(networks, (list, tuple)) else [networks]) if n is not None]
        if not nets:
            raise ValueError("bake needs a network")
        R, k = int(resolution), int(probes)
        if k not in (1, 2, 3):
            raise ValueError("probes is 1, 2 or 3")
        if int(dilate) < 0:
            raise ValueError("dilate is a number of rounds")
        packs = []
        for net in nets:
            net.require_standard()
            flat = net.flat_parameters()
            pd = int(getattr(net, "pt_dims", 3))
            if _SPACE_OF_PD.get(pd) != space:
                raise ValueError("a network on %d-D points does not fit an occupancy grid in the %s space" % (pd, space))
            packs.append((net, flat, pd, net.pack_remap() if hasattr(net, "pack_remap") else None))
        dev = packs[0][1].device
        grid = cls(torch.zeros(max(R, 32) ** 3 // 32, dtype=torch.int32, device=dev), lo, hi, R, space=space)
        probe = ops.occ_probe_points if space == "euclidean" else ops.occ_probe_points_inverted
        cells, k3 = R ** 3, k ** 3
        pass_cells = MAX_PASS_POINTS // k3 // 64 * 64
        direction = torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float32, device=dev)
        with torch.no_grad():
            for first in range(0, cells, pass_cells):
                n_cells = min(pass_cells, cells - first)
                pts = probe(first, n_cells, R, k, grid.lo, grid.cell, dev)
                for net, flat, pd, remap in packs:
                    wf, pl = ops.network_packs(net, flat, False, pts.shape[0], pd, remap=remap)
                    raw = ops.mlp_fwd(pts, direction, pts.shape[0], wf, None, pd=pd, planes=pl)
                    ops.occ_accumulate(raw, sigma_min, first, n_cells, R, k, grid.bits)
            for _ in range(int(dilate)):
                grid.bits = ops.occ_dilate(grid.bits, R)
        grid._bound = tuple((weakref.ref(p[0]), _weights_key(p[0])) for p in packs)
        return grid

    # ---- the networks it was baked from ---------------------------------------------------------------------------------
    def check(self, *networks):
        """Raises OccupancyStaleError unless every network given is one the grid was baked from, with the weights it was baked
        from.  A grid made by hand is bound to nothing and checks nothing."""
        if not self._bound:
            return
        for net in networks:
            if net is None:
                continue
            for ref, key in self._bound:
                if ref() is net:
                    if _weights_key(net) != key:
                        raise OccupancyStaleError("the weights have changed since the occupancy grid was baked: bake it again")
                    break
            else:
                raise OccupancyStaleError("the occupancy grid was baked from other networks")

    # ---- moving and saving ------------------------------------------------------------------------------------------------
    def to(self, device):
        g = OccupancyGrid(self.bits.to(device), self._lo, self._hi, self.resolution, self._bound, self.space)
        return g

    def state_dict(self):
        return {"bits": self.bits.detach().cpu().clone(), "lo": torch.from_numpy(self._lo.copy()),
                "hi": torch.from_numpy(self._hi.copy()), "resolution": self.resolution, "space": self.space}

    @classmethod
    def from_state_dict(cls, sd, networks=None):
        """`networks`: bind the grid to these networks as they are now (the caller vouches that it was baked from them)."""
        # (a dict written before the grid knew of spaces holds a euclidean grid)
        grid = cls(sd["bits"].clone(), sd["lo"], sd["hi"], int(sd["resolution"]), space=sd.get("space", "euclidean"))
        if networks is not None:
            nets = [n for n in (networks if isinstance(networks, (list, tuple)) else [networks]) if n is not None]
            grid._bound = tuple((weakref.ref(net), _weights_key(net)) for net in nets)
            if nets:
                grid = grid.to(nets[0].flat_parameters().device)
        return grid

    def occupied_fraction(self) -> float:
        """the share of set cells (one host read: the words)"""
        words = self.bits.detach().cpu().numpy().view(np.uint8)
        return float(np.unpackbits(words).sum()) / float(self.resolution ** 3)


def bake_nerfpp(nets, resolution=128, probes=2, sigma_min=0.0, dilate=1, fg_box=None, bg_box=None):
    """The two grids of ops.inference_occupancy_nerfpp -> (fg_grid, bg_grid).  nets: the NerfNet modules of every cascade
    level (one module or a list).  The foreground grid -- euclidean, over fg_box = (lo, hi), [-1, 1]^3 unless given: the
    foreground samples lie in the unit sphere -- is the OR over all levels' foreground networks; the background grid --
    inverted_sphere, over bg_box in q = (x' w, y' w, z' w), [-1, 1]^3 unless given -- the OR over their background
    networks.  Each is bound to its networks for check()."""
    nets = [n for n in (nets if isinstance(nets, (list, tuple)) else [nets]) if n is not None]
    if not nets:
        raise ValueError("bake_nerfpp needs a NerfNet")
    unit = ((-1.0,) * 3, (1.0,) * 3)
    fg_lo, fg_hi = fg_box if fg_box is not None else unit
    bg_lo, bg_hi = bg_box if bg_box is not None else unit
    fg = OccupancyGrid.bake([n.fg_net for n in nets], fg_lo, fg_hi, resolution, probes, sigma_min, dilate, space="euclidean")
    bg = OccupancyGrid.bake([n.bg_net for n in nets], bg_lo, bg_hi, resolution, probes, sigma_min, dilate,
                            space="inverted_sphere")
    return fg, bg


def box_of_rays(rays, resolution=128):
    """-> (lo, hi): the box of all o + d * near and o + d * far of a packed ray batch [n, >= 8], widened by one cell of an
    R = resolution grid on every side.  A convenience in plain torch."""
    o, d, near, far = rays[:, 0:3], rays[:, 3:6], rays[:, 6:7], rays[:, 7:8]
    ends = torch.cat([o + d * near, o + d * far], 0)
    lo, hi = ends.min(0)[0], ends.max(0)[0]
    pad = (hi - lo) / float(max(int(resolution) - 2, 1))
    return tuple(float(x) for x in (lo - pad)), tuple(float(x) for x in (hi + pad))
