"""TEST INFRASTRUCTURE: numpy transcriptions of csrc/occupancy.hip -- the bit layout, the probe points, the accumulation,
the dilation, the cell lookup of a sample, the compaction and the raw expansion.  Every function states the kernels'
contract in array code, in fp32 with one rounding per operation where the kernels round; the tests compare for EQUALITY."""
import numpy as np

f32 = np.float32


def box(lo, hi, R):
    """-> (lo, hi, inv, cell) as fp32 triples: inv = R / (hi - lo), cell = (hi - lo) / R, one rounding each"""
    lo, hi = np.asarray(lo, f32), np.asarray(hi, f32)
    return lo, hi, (f32(R) / (hi - lo)).astype(f32), ((hi - lo) / f32(R)).astype(f32)


def bits_of_mask(mask):
    """mask bool [R, R, R] indexed [z, y, x] -> int32 words: cell c = (z R + y) R + x is bit c & 31 of word c >> 5"""
    flat = np.ascontiguousarray(mask, bool).reshape(-1, 32)
    words = (flat.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32)
    return words.view(np.int32)


def mask_of_bits(bits, R):
    words = np.ascontiguousarray(bits).view(np.uint32)
    return (((words[:, None] >> np.arange(32, dtype=np.uint32)) & 1) != 0).reshape(R, R, R)


def probe_points(first, n_cells, R, k, lo, cell):
    """pts [n_cells k^3, 3]: point (jz k + jy) k + jx of cell c = first + .. is lo + (i + (j + 0.5) / k) * cell per axis"""
    c = first + np.arange(n_cells, dtype=np.int64)
    idx = np.stack([c % R, (c // R) % R, c // (R * R)], 1)                       # [cells, (x, y, z)]
    q = np.arange(k ** 3)
    j = np.stack([q % k, (q // k) % k, q // (k * k)], 1)                         # [k^3, (jx, jy, jz)]
    off = ((j.astype(f32) + f32(0.5)) / f32(k)).astype(f32)
    t = (idx[:, None, :].astype(f32) + off[None, :, :]).astype(f32)
    return (lo[None, None, :] + (t * cell[None, None, :]).astype(f32)).astype(f32).reshape(-1, 3)


def accumulate(bits, raw, sigma_min, first, n_cells, R, k):
    """-> new words: the cells' bits OR "some probe has !(sigma <= sigma_min)" -- a NaN density sets the cell"""
    sigma = np.asarray(raw, f32).reshape(n_cells, k ** 3, 4)[:, :, 3]
    with np.errstate(invalid="ignore"):
        hit = (~(sigma <= f32(sigma_min))).any(1)
    mask = mask_of_bits(bits, R).reshape(-1).copy()
    mask[first:first + n_cells] |= hit
    return bits_of_mask(mask.reshape(R, R, R))


def dilate_mask(mask):
    """one round of 26-neighbourhood dilation of a bool [z, y, x] array; a grid edge has no neighbour"""
    R = mask.shape[0]
    pad = np.zeros((R + 2,) * 3, bool)
    pad[1:-1, 1:-1, 1:-1] = mask
    out = np.zeros_like(mask)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                out |= pad[dz:dz + R, dy:dy + R, dx:dx + R]
    return out


def dilate(bits, R):
    return bits_of_mask(dilate_mask(mask_of_bits(bits, R)))


def dead_mask(pts, bits, R, lo, inv):
    """pts [P, 3] fp32 -> bool [P]: dead = all three t = (p - lo) * inv in [0, R) and the bit of cell floor(t) is 0"""
    pts = np.asarray(pts, f32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        t = ((pts - lo[None, :]).astype(f32) * inv[None, :]).astype(f32)
        inside = ((t >= f32(0)) & (t < f32(R))).all(1)
    cell = np.where(inside[:, None], t, f32(0)).astype(np.int64)                  # truncation = floor on [0, R); -0.0 -> 0
    c = (cell[:, 2] * R + cell[:, 1]) * R + cell[:, 0]
    words = np.ascontiguousarray(bits).view(np.uint32)
    bit = (words[c >> 5] >> (c & 31).astype(np.uint32)) & 1
    return inside & (bit == 0)


def compact(pts, viewdirs, samples_per_ray, bits, R, lo, inv):
    """-> (live_idx ascending, slot_of [P] with -1 on the dead, pts_live, vd_live)"""
    pts = np.asarray(pts, f32).reshape(-1, 3)
    live = np.flatnonzero(~dead_mask(pts, bits, R, lo, inv)).astype(np.int32)
    slot_of = np.full(pts.shape[0], -1, np.int32)
    slot_of[live] = np.arange(live.shape[0], dtype=np.int32)
    return live, slot_of, pts[live], np.asarray(viewdirs, f32)[live // samples_per_ray, :3]


def expand(raw_live, slot_of):
    raw = np.zeros((slot_of.shape[0], 4), f32)
    raw[slot_of >= 0] = raw_live[slot_of[slot_of >= 0]]
    return raw
