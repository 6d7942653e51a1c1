"""TEST SUPPORT: the training-batch construction of scnerf_ray_batch in numpy, transcribed from its documentation
(include/scnerf_hip.h) and not from the kernel.

  Philox4x32-10 (Salmon et al., SC'11): ten rounds of
      (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),  M0 = D2511F53, M1 = CD9E8D57,
      the key bumped by (9E3779B9, BB67AE85) after each round.
  F_round(R) = philox(counter = (R, 0x52420000 | mode << 8 | round, counter_lo, counter_hi), key = (seed_lo, seed_hi))[0] mod 2^h
  pi: x = L 2^h + R, four rounds (L, R) <- (R, L ^ F_round(R)); applied again while the value is >= M.
  h: the smallest integer >= 1 with 2^(2h) >= M.

  mode 0 (one image):  counter = step, position = rank n + j, y = y0 + index // win_w, x = x0 + index % win_w
  mode 1 (all images): g = step world n + rank n + j, counter = g // M, position = g % M,
                       image = index // (H W), y = index % (H W) // W, x = index % W"""
import numpy as np

U32 = np.uint64(0xFFFFFFFF)
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
TAG = 0x52420000
ONE_IMAGE, ALL_IMAGES = 0, 1
EINVAL = -22


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """counters: uint64 arrays holding 32-bit values; key: Python ints -> the four output words"""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & U32 for c in (c0, c1, c2, c3))
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                               # 32 x 32 bits: exact in 64
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & U32,
                          (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & U32)
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def half_bits(M):
    h = 1
    while (1 << (2 * h)) < M:
        h += 1
    return h


def feistel(x, h, seed, counter, mode):
    """one application of the 2h-bit network to the uint64 array x; counter: uint64 array (or scalar) of the same shape"""
    mask = np.uint64((1 << h) - 1)
    left, right = x >> np.uint64(h), x & mask
    counter = np.broadcast_to(np.asarray(counter, np.uint64), x.shape)
    c_lo, c_hi = counter & U32, counter >> np.uint64(32)
    for rnd in range(4):
        f = philox4x32_10(right, np.full(x.shape, TAG | (mode << 8) | rnd, np.uint64), c_lo, c_hi,
                          seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[0] & mask
        left, right = right, left ^ f
    return (left << np.uint64(h)) | right


def permute(pos, M, seed, counter, mode, count=None):
    """pi(pos) on [0, M), element-wise; `count` (a list) receives the largest number of applications any element needed"""
    pos = np.asarray(pos, np.uint64)
    assert pos.size == 0 or int(pos.max()) < M
    h = half_bits(M)
    counter = np.broadcast_to(np.asarray(counter, np.uint64), pos.shape)
    v = feistel(pos, h, seed, counter, mode)
    applications = 1
    while True:
        out = v >= np.uint64(M)
        if not out.any():
            break
        assert applications < (1 << (2 * h)) - M + 1, "the walk outran its bound"
        v = v.copy()
        v[out] = feistel(v[out], h, seed, counter[out], mode)
        applications += 1
    if count is not None:
        count.append(applications)
    return v


def precrop_window(H, W, frac):
    """the reference's centre crop -> (x0, y0, w, h)"""
    dH, dW = int(H // 2 * frac), int(W // 2 * frac)
    return W // 2 - dW, H // 2 - dH, 2 * dW, 2 * dH


def batch(mode, seed, step, n, H, W, n_sel=1, image_pos=0, window=None, rank=0, world=1):
    """-> coords int64 [n, 2] (x, y), select_inds int64 [n], image_idx int64 [n]"""
    x0, y0, ww, wh = window if window is not None else (0, 0, W, H)
    j = np.arange(n, dtype=np.uint64)
    if mode == ONE_IMAGE:
        M = ww * wh
        index = permute(np.uint64(rank * n) + j, M, seed, np.uint64(step), mode).astype(np.int64)
        image = np.full(n, image_pos, np.int64)
        y, x = y0 + index // ww, x0 + index % ww
    else:
        M = n_sel * H * W
        g = np.uint64(step * world * n + rank * n) + j
        index = permute(g % np.uint64(M), M, seed, g // np.uint64(M), mode).astype(np.int64)
        image, y, x = index // (H * W), index % (H * W) // W, index % W
    return np.stack([x, y], -1), y * W + x, image


def to_float(images, white_bkgd=False):
    """what the loaders make of a stack: fp32 as it is; uint8 through (v / 255.).astype(float32), 4 channels composited
    over white op by op in fp32 (NeRF/run_nerf.py:167-171) or cut to rgb"""
    if images.dtype == np.float32:
        return images
    f = (images / 255.).astype(np.float32)
    if f.shape[-1] == 4:
        return f[..., :3] * f[..., -1:] + (np.float32(1.) - f[..., -1:]) if white_bkgd else f[..., :3]
    return f


def target(images, image_ids, coords, image_idx, white_bkgd=False):
    rows = image_idx if image_ids is None else np.asarray(image_ids)[image_idx]
    return to_float(images, white_bkgd)[rows, coords[:, 1], coords[:, 0]]


def wilson_hilferty(dof, z):
    """the chi-square quantile at the normal deviate z"""
    return dof * (1. - 2. / (9. * dof) + z * (2. / (9. * dof)) ** 0.5) ** 3


def pearson(counts, expected):
    counts = np.asarray(counts, np.float64)
    return float(((counts - expected) ** 2 / expected).sum())
