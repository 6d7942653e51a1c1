"""TEST INFRASTRUCTURE: numpy transcriptions of csrc/npp_occupancy.hip -- the cell test of a 4-D sample in the inverted-sphere
space, the compaction of such samples and the probe points of an inverted-sphere grid.  fp32 with one rounding per operation
where the kernels round; the tests compare for EQUALITY.  The bit layout, the accumulation, the dilation and the raw expansion
serve both spaces: tests/occupancy_reference.py's."""
import numpy as np

from tests import occupancy_reference as REF

f32 = np.float32


def dead_mask4(pts, bits, R, lo, inv):
    """pts [P, 4] fp32 = (x', y', z', w) -> bool [P]: q_a = p_a * p_w, one rounding, then the euclidean test on q"""
    pts = np.asarray(pts, f32).reshape(-1, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        q = (pts[:, :3] * pts[:, 3:4]).astype(f32)
    return REF.dead_mask(q, bits, R, lo, inv)


def compact4(pts, viewdirs, samples_per_ray, bits, R, lo, inv):
    """-> (live_idx ascending, slot_of [P] with -1 on the dead, pts_live [n_live, 4], vd_live [n_live, 3])"""
    pts = np.asarray(pts, f32).reshape(-1, 4)
    live = np.flatnonzero(~dead_mask4(pts, bits, R, lo, inv)).astype(np.int32)
    slot_of = np.full(pts.shape[0], -1, np.int32)
    slot_of[live] = np.arange(live.shape[0], dtype=np.int32)
    return live, slot_of, pts[live], np.asarray(viewdirs, f32)[live // samples_per_ray, :3]


def probe_points_inverted(first, n_cells, R, k, lo, cell):
    """pts [n_cells k^3, 4]: the lattice point q of the euclidean probe, r2 = ((qx qx) + (qy qy)) + (qz qz), r = sqrt(r2),
    the row (q / r, min(r, 1)); (0, 0, 1, 0) where r == 0.  numpy's fp32 square root and division are correctly rounded."""
    q = REF.probe_points(first, n_cells, R, k, lo, cell)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        sq = (q * q).astype(f32)
        r2 = ((sq[:, 0] + sq[:, 1]).astype(f32) + sq[:, 2]).astype(f32)
        r = np.sqrt(r2).astype(f32)
        out = np.empty((q.shape[0], 4), f32)
        out[:, :3] = (q / r[:, None]).astype(f32)
        out[:, 3] = np.where(r < f32(1), r, f32(1))
    out[r == 0] = np.array([0, 0, 1, 0], f32)
    return out
