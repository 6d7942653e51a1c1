"""TEST INFRASTRUCTURE: numpy transcriptions of csrc/early_stop.hip -- the depth segments, the compaction of a segment's
samples, the expansion into the dense raw, the transmittance behind a segment and the stop decision -- and an independent
fp64 recomputation of the stop decisions from a dense raw.  The compaction and the expansion state the kernels' contract
in array code and are compared for EQUALITY; the transmittance is an fp64 product of the fp32 q the backend's own
compositing computes (tests/early_stop_cases.py: device_q), compared to 1e-12 relative."""
import numpy as np

from tests import occupancy_reference as OREF

f32 = np.float32


def bounds(S, K):
    """b_0 .. b_K: segment k holds the sample indices [b_k, b_k+1), b_k = (k S) // K"""
    return [(k * S) // K for k in range(K + 1)]


def segment_of(S, K):
    """-> int [S]: the segment of every sample index"""
    b = bounds(S, K)
    seg = np.zeros(S, np.int64)
    for k in range(K):
        seg[b[k]:b[k + 1]] = k
    return seg


def compact(pts, viewdirs, S, first, length, alive=None, grid=None):
    """pts [n S, 3], viewdirs [n, >= 3], alive int [n] or None, grid = (bits, R, lo, inv) or None
    -> (live_idx: dense sample indices ascending, slot_of [n length] with -1 on a sample that does not run, pts_live, vd_live,
    the number of alive rays)"""
    pts = np.asarray(pts, f32).reshape(-1, 3)
    n = pts.shape[0] // S
    up = np.ones(n, bool) if alive is None else (np.asarray(alive) != 0)
    e = np.arange(n * length, dtype=np.int64)
    ray, j = e // length, e % length
    i = ray * S + first + j
    runs = up[ray] if n else np.zeros(0, bool)
    if grid is not None and n:
        runs = runs & ~OREF.dead_mask(pts[i], *grid)
    live = i[runs].astype(np.int32)
    slot_of = np.full(n * length, -1, np.int32)
    slot_of[runs] = np.arange(live.shape[0], dtype=np.int32)
    return live, slot_of, pts[live], np.asarray(viewdirs, f32)[live // S, :3], int(up.sum()) if n else 0


def expand(raw, raw_live, slot_of, S, first, length):
    """the dense raw [n S, 4] with the segment's rows replaced: raw_live's row, or zero; every other row as it was"""
    out = np.array(raw, f32).reshape(-1, 4).copy()
    n = out.shape[0] // S
    e = np.arange(n * length, dtype=np.int64)
    i = (e // length) * S + first + e % length
    rows = np.zeros((n * length, 4), f32)
    ok = slot_of >= 0
    rows[ok] = raw_live[slot_of[ok]]
    out.view(np.uint32)[i] = rows.view(np.uint32)               # (bits travel, whatever they are)
    return out


def q_of_alpha(alpha):
    """q = 1 - alpha + 1e-10 as ray::sample_terms rounds it: two fp32 operations"""
    return ((f32(1.0) - np.asarray(alpha, f32)).astype(f32) + f32(1e-10)).astype(f32)


def transmittance(q, first, length, k, K, eps, T, alive, stop_segment):
    """q fp32 [n, S]; the state BEFORE segment k (ignored for k == 0) -> (T, alive, stop_segment) behind it: an fp64 product,
    one factor after the other; alive = !(T <= eps); a stopped ray keeps what it has"""
    n = q.shape[0]
    prod = np.ones(n, np.float64)
    for i in range(first, first + length):
        prod = prod * q[:, i].astype(np.float64)
    if k == 0:
        T_new = prod
        with np.errstate(invalid="ignore"):
            up = ~(T_new <= eps)
        return T_new, up.astype(np.int32), np.where(up, K, 1).astype(np.int32)
    was = np.asarray(alive) != 0
    T_new = np.where(was, np.asarray(T, np.float64) * prod, T)
    with np.errstate(invalid="ignore"):
        up = was & ~(T_new <= eps)
    stop = np.where(was & ~up, k + 1, stop_segment).astype(np.int32)
    return T_new, up.astype(np.int32), stop


def decide(T_own, k, K, eps, alive, stop_segment):
    """the decision the kernel must take from ITS OWN transmittance T_own behind segment k -> (alive, stop_segment)"""
    with np.errstate(invalid="ignore"):
        not_opaque = ~(np.asarray(T_own, np.float64) <= eps)
    if k == 0:
        return not_opaque.astype(np.int32), np.where(not_opaque, K, 1).astype(np.int32)
    was = np.asarray(alive) != 0
    up = was & not_opaque
    return up.astype(np.int32), np.where(was & ~up, k + 1, stop_segment).astype(np.int32)


def boundary_transmittance_fp64(sigma, z, norm, K):
    """INDEPENDENT of the kernels: sigma [n, S] (raw[..., 3]), z [n, S], norm [n] = |d| -> T fp64 [n, K - 1]: the
    transmittance behind segments 0 .. K - 2 in fp64 throughout, exp included"""
    sigma, z, norm = np.asarray(sigma, np.float64), np.asarray(z, np.float64), np.asarray(norm, np.float64)
    n, S = sigma.shape
    dist = np.concatenate([z[:, 1:] - z[:, :-1], np.full((n, 1), 1e10)], 1) * norm[:, None]
    a = np.maximum(sigma, 0.0)
    a = np.where(np.isnan(sigma), 0.0, a)                      # fmaxf(NaN, 0) = 0
    q = np.exp(-a * dist) + 1e-10
    cum = np.cumprod(q, axis=1)
    b = bounds(S, K)
    return np.stack([cum[:, b[k + 1] - 1] for k in range(K - 1)], 1)


def stop_segment_fp64(T_bound, eps):
    """T [n, K - 1] -> stop_segment [n]: the first segment not run, K when the ray runs them all"""
    n, km1 = T_bound.shape
    stopped = T_bound <= eps
    first = np.where(stopped.any(1), stopped.argmax(1) + 1, km1 + 1)
    return first.astype(np.int32)


def in_band(T_bound, eps, rel=1e-4):
    """rays whose fp64 T lies within eps (1 +- rel) at some boundary: their decision may go either way in fp32"""
    return ((T_bound >= eps * (1 - rel)) & (T_bound <= eps * (1 + rel))).any(1)
