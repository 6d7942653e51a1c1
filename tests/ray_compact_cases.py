"""TEST INFRASTRUCTURE shared by tests/test_emu_ray_compact.py and tests/test_gpu_ray_compact.py: the inputs, the numpy
references and the checks of the three kernels of csrc/ray_compact.hip, written against a `backend` that runs the C ABI
on numpy arrays -- the CPU SIMT interpreter build (host pointers) or the product library (device copies).  Everything is
compared for EQUALITY: the kernels move values and count, they compute nothing."""
import numpy as np

SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097, 70001)
KINDS = ("random", "all_live", "none_live", "nan_and_ties", "zeros_tau0")
WIDTHS = (1, 3, 11, 64, 192)
SENTINEL = -7


def make(n, kind, seed=0):
    """-> (acc float32 [n], tau)"""
    rng = np.random.default_rng(1000 * seed + n)
    acc = rng.random(n, dtype=np.float32)
    tau = np.float32(0.5)
    if kind == "all_live":
        acc = np.float32(0.5) + np.float32(0.5) * acc + np.float32(1e-3)
    elif kind == "none_live":
        acc = np.float32(0.5) * acc
        acc[::3] = tau                                    # a tie is skipped
    elif kind == "nan_and_ties":
        acc[rng.random(n) < 0.2] = np.nan                 # live: NaN <= tau is false
        acc[rng.random(n) < 0.2] = tau
    elif kind == "zeros_tau0":
        tau = np.float32(0.0)
        acc[rng.random(n) < 0.4] = 0.0
        acc[rng.random(n) < 0.1] = -0.0
    return np.ascontiguousarray(acc, np.float32), float(tau)


def reference(acc, tau):
    live = np.flatnonzero(~(acc <= np.float32(tau))).astype(np.int32)
    slot_of = np.full(acc.shape[0], -1, np.int32)
    slot_of[live] = np.arange(live.shape[0], dtype=np.int32)
    return live, slot_of


def check_compact(backend, n, kind):
    """-> (live, slot_of) after the equalities; the launch runs twice and must leave identical bytes"""
    acc, tau = make(n, kind)
    live, slot_of = reference(acc, tau)
    if kind == "all_live":
        assert live.shape[0] == n
    if kind == "none_live":
        assert live.shape[0] == 0
    if kind in ("random", "nan_and_ties", "zeros_tau0") and n >= 63:
        assert 0 < live.shape[0] < n
    runs = [backend.compact(acc, tau) for _ in range(2)]
    for got_idx, got_slot, n_dev, n_host in runs:
        assert n_dev == live.shape[0] and n_host == live.shape[0], (n_dev, n_host, live.shape[0])
        assert np.array_equal(got_idx[:n_dev], live)
        assert np.array_equal(got_slot, slot_of)
        assert (got_idx[n_dev:] == SENTINEL).all(), "live_idx written past n_live"
    assert all(a.tobytes() == b.tobytes() for a, b in zip(runs[0][:2], runs[1][:2]))
    return live, slot_of


def check_gather(backend, n, live):
    rng = np.random.default_rng(n)
    for w in WIDTHS:
        src = rng.standard_normal((n, w)).astype(np.float32)
        if n:
            src[rng.integers(0, n), rng.integers(0, w)] = np.nan          # bits travel, whatever they are
        got = backend.gather(src, live, w)
        assert got.shape == (live.shape[0], w)
        assert got.tobytes() == src[live].tobytes(), "row gather, w = %d" % w


def expand_reference(slot_of, live, fine, coarse, s_tot, s_fine):
    """the numpy scatter: -> [rgb_map, disp_map, acc_map, depth_map, z_std, raw, z_vals, z_samples]"""
    n = slot_of.shape[0]
    skipped = slot_of < 0
    out = []
    for k, shape in enumerate([(n, 3), (n,), (n,), (n,), (n,), (n, s_tot, 4), (n, s_tot), (n, s_fine)]):
        o = np.zeros(shape, np.float32)
        o[live] = fine[k]
        if k < 4:
            o[skipped] = coarse[k][skipped]
        out.append(o)
    return out


def check_expand(backend, n, live, slot_of, s_tot, s_fine):
    rng = np.random.default_rng(7 * n + s_tot)
    nl = live.shape[0]

    def draw(*shape):
        return rng.standard_normal(shape).astype(np.float32)

    fine = [draw(nl, 3), draw(nl), draw(nl), draw(nl), draw(nl), draw(nl, s_tot, 4), draw(nl, s_tot), draw(nl, s_fine)]
    coarse = [draw(n, 3), draw(n), draw(n), draw(n)]
    want = expand_reference(slot_of, live, fine, coarse, s_tot, s_fine)
    runs = [backend.expand(slot_of, nl, fine, coarse, s_tot, s_fine) for _ in range(2)]
    names = ("rgb_map", "disp_map", "acc_map", "depth_map", "z_std", "raw", "z_vals", "z_samples")
    for got in runs:
        for name, g, w_ in zip(names, got, want):
            assert g.shape == w_.shape and g.tobytes() == w_.tobytes(), "%s (n = %d, %d live)" % (name, n, nl)
    if n:
        assert (runs[0][4][slot_of < 0] == 0).all()


def expand_shapes(n):
    """(s_tot, s_fine): a row shorter than a wave with an odd length, and -- where the buffers stay small -- the 64 + 128 of
    the render path"""
    return [(7, 3)] + ([(192, 128)] if n <= 1025 else [])


def check_all(backend, n, kind):
    live, slot_of = check_compact(backend, n, kind)
    check_gather(backend, n, live)
    for s_tot, s_fine in expand_shapes(n):
        check_expand(backend, n, live, slot_of, s_tot, s_fine)
