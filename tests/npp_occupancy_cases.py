"""TEST INFRASTRUCTURE shared by tests/test_emu_npp_occupancy.py and tests/test_gpu_npp_occupancy.py: the case bodies of
ops.inference_occupancy_nerfpp (csrc/npp_occupancy.hip, scnerf_amd/occupancy.py, nerfplusplus/ddp_model.py).

The kernel cases run the C ABI through a `route` object (it holds buffers -- every output NaN- or sentinel-filled with a guard
row on either side -- and calls the library: the CPU SIMT interpreter build on numpy arrays or the product library on device
tensors) and compare with tests/npp_occupancy_reference.py for EQUALITY, every launch twice for identical bytes.  The node
cases compare a forward-only NerfNet.forward under the switch, bit for bit in all eight outputs, with an oracle built here
from stand-alone launches: scnerf_npp_points_fwd, a DENSE ops.mlp_fwd with samples_per_ray = 1 and expanded view
directions, the rows of the dead samples zeroed in torch by the transcription's mask, scnerf_npp_composite_fwd -- the
construction of tests/occupancy_cases.py."""
import contextlib

import numpy as np
import torch

from tests import npp_occupancy_reference as REF4
from tests import occupancy_reference as REF
from tests import skip_background_case as SB

SENTINEL = -7
EINVAL = -22
KEYS = SB.KEYS
N, SF, SB_ = SB.N, SB.SF, SB.SB

# ---- the kernels ---------------------------------------------------------------------------------------------------------
SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 70 * 16, 4 * 1024 + 49)
SPRS = (1, 12, 65)
GRIDS = ("all", "none", "halfball")
BOXES = (((-1.0,) * 3, (1.0,) * 3), ((-0.5,) * 3, (0.75,) * 3))
KR = 32


def kernel_grid(kind, box, R=KR):
    """-> (bits, R, lo, inv): every cell, no cell, the cells whose centre (in q) lies in the unit ball with q_z >= 0"""
    lo, hi, inv, cell = REF.box(box[0], box[1], R)
    if kind == "all":
        mask = np.ones((R, R, R), bool)
    elif kind == "none":
        mask = np.zeros((R, R, R), bool)
    else:
        c = [lo[a] + (np.arange(R) + 0.5) * cell[a] for a in range(3)]
        x, y, z = c[0][None, None, :], c[1][None, :, None], c[2][:, None, None]
        mask = (x * x + y * y + z * z <= 1.0) & (z >= 0.0)
    return REF.bits_of_mask(mask), R, lo, inv


N_PLANTED = 8


def kernel_points(P, spr, box, seed=0):
    """-> (pts [P, 4], viewdirs [rays, 5] with two unused columns: a row stride of 5).  Random unit directions and w in
    [0, 1): q fills the unit ball.  Rows 0 .. 7 (where P has them): w = 0 with products +0, -0, +0 (inside: dead under an
    empty grid); q_x exactly on lo (inside); q_x exactly on hi (outside: live); a NaN direction component (live); a NaN w
    (live); w = 1 on the y axis; a negative w (q = -x' |w|, inside); a huge w (the products overflow: live)."""
    rng = np.random.default_rng(100 * seed + P)
    d = rng.standard_normal((P, 3))
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-9)
    pts = np.concatenate([d, rng.random((P, 1))], 1).astype(np.float32)
    lo, hi = np.float32(box[0][0]), np.float32(box[1][0])
    special = [[0.6, -0.8, 0.0, 0.0], [-1.0, 0.0, 0.0, -lo], [1.0, 0.0, 0.0, hi], [np.nan, 0.0, 1.0, 0.5],
               [0.0, 0.0, 1.0, np.nan], [0.0, 1.0, 0.0, 1.0], [0.6, 0.0, 0.8, -0.5], [0.6, -0.8, 0.0, 3e38]]
    for i, row in enumerate(special[:P]):
        pts[i] = np.asarray(row, np.float32)
    rays = (P + spr - 1) // spr
    vd = rng.standard_normal((max(rays, 1), 5)).astype(np.float32)
    return pts, vd


def _guards_kept(route, buf, what):
    b = route.host(buf)
    for edge in (b[0], b[-1]):
        assert (np.isnan(edge).all() if b.dtype == np.float32 else (edge == SENTINEL).all()), what + ": written outside its rows"
    return b[1:-1].copy()


def run_compact4(route, pts, vd, spr, bits, R, lo, inv):
    P = pts.shape[0]
    ws_ints = int(route.size("scnerf_occ_compact4_workspace_ints", P))
    assert ws_ints == max(1, -(-P // 1024))
    bufs = {"live_idx": route.out((P,), np.int32), "slot_of": route.out((P,), np.int32), "pts_live": route.out((P, 4)),
            "vd_live": route.out((P, 3)), "ws": route.out((ws_ints,), np.int32), "n_dev": route.out((1,), np.int32)}
    n_host = route.pinned_word()
    route.call("scnerf_occ_compact4", route.inp(pts), P, route.inp(vd), 5, spr, route.inp(bits), R, *[float(x) for x in lo],
               *[float(x) for x in inv], bufs["ws"][1], bufs["live_idx"][1], bufs["slot_of"][1], bufs["pts_live"][1],
               bufs["vd_live"][1], bufs["n_dev"][1], n_host)
    route.sync()
    got = {k: _guards_kept(route, b[0], k) for k, b in bufs.items()}
    return got["live_idx"], got["slot_of"], got["pts_live"], got["vd_live"], int(got["n_dev"][0]), int(route.host(n_host)[0])


def run_expand(route, raw_live, slot_of, n_live):
    P = slot_of.shape[0]
    raw = route.out((P, 4))
    route.call("scnerf_occ_expand_raw", route.inp(raw_live) if n_live else None, route.inp(slot_of) if P else None, raw[1], P,
               n_live)
    route.sync()
    return _guards_kept(route, raw[0], "raw")


def check_compact4_and_expand(route, P, kind):
    """case 1: every samples_per_ray and both boxes at one size and grid"""
    for box in BOXES:
        bits, R, lo, inv = kernel_grid(kind, box)
        for spr in SPRS:
            pts, vd = kernel_points(P, spr, box)
            live, slot_of, pts_live, vd_live = REF4.compact4(pts, vd, spr, bits, R, lo, inv)
            nl = live.shape[0]
            dead = REF4.dead_mask4(pts, bits, R, lo, inv)
            if kind == "all":
                assert nl == P
            if kind == "none" and P >= N_PLANTED:
                assert list(dead[:N_PLANTED]) == [True, True, False, False, False, False, True, False], dead[:N_PLANTED]
                assert 0 < nl < P
            if kind == "halfball" and P >= 63:
                assert 0 < nl < P
            if box is BOXES[1] and P >= 63:
                q = pts[N_PLANTED:, :3] * pts[N_PLANTED:, 3:4]
                assert ((q < lo) | (q >= np.asarray(box[1], np.float32))).any(), "no sample outside the box"
            runs = [run_compact4(route, pts, vd, spr, bits, R, lo, inv) for _ in range(2)]
            for got_idx, got_slot, got_pts, got_vd, n_dev, n_host in runs:
                assert n_dev == nl and n_host == nl, (n_dev, n_host, nl)
                assert np.array_equal(got_idx[:nl], live) and (np.diff(got_idx[:nl]) > 0).all()
                assert (got_idx[nl:] == SENTINEL).all(), "live_idx written past n_live"
                assert np.array_equal(got_slot, slot_of) and (got_slot[dead] == -1).all()
                assert got_pts[:nl].tobytes() == pts_live.tobytes() and got_vd[:nl].tobytes() == vd_live.tobytes()
                assert np.isnan(got_pts[nl:]).all() and np.isnan(got_vd[nl:]).all(), "a live row written past n_live"
            assert all(a.tobytes() == b.tobytes() for a, b in zip(runs[0][:4], runs[1][:4]))
            rng = np.random.default_rng(P + 1)
            raw_live = rng.standard_normal((nl, 4)).astype(np.float32)
            if nl:
                raw_live[rng.integers(0, nl), 1] = np.nan                     # bits travel, whatever they are
            want = REF.expand(raw_live, slot_of)
            for got in [run_expand(route, raw_live, slot_of, nl) for _ in range(2)]:
                assert got.shape == (P, 4) and got.tobytes() == want.tobytes()
            assert (want[dead] == 0).all()


def probe_boxes(k, R=KR):
    """the unit box, and a box of the same width placed so that the lattice point of cell (R/2, R/2, R/2) with probe index
    j = (0 or 1) is exactly 0: lo = -(R/2 + off) * cell with cell = 1/16 (every number exact in fp32)"""
    off = 0.25 if k == 2 else 0.5
    lo0 = -(R // 2 + off) / 16.0
    return (BOXES[0], ((lo0,) * 3, (lo0 + 2.0,) * 3))


def check_probe_points_inverted(route, k):
    """case 2"""
    R = KR
    middle = ((R // 2 - 1) * R + R // 2 - 1) * R // 64 * 64           # a multiple of 64 below cell (R/2 - 1, R/2 - 1, R/2 - 1)
    centre = ((R // 2) * R + R // 2) * R + R // 2
    ranges = ((middle, centre - middle + 1 + 17), (0, 64), (R ** 3 - 64, 64))
    for b, box in enumerate(probe_boxes(k)):
        lo, hi, inv, cell = REF.box(box[0], box[1], R)
        for first, n_cells in ranges:
            want = REF4.probe_points_inverted(first, n_cells, R, k, lo, cell)
            if first in (0, R ** 3 - 64):
                assert (want[:, 3] == 1.0).all(), "the corner cells lie outside the ball: w clamps to 1"
            else:
                assert ((want[:, 3] > 0) & (want[:, 3] < 1)).any()
                zero_rows = (want == np.array([0, 0, 1, 0], np.float32)).all(1)
                assert bool(zero_rows.any()) == (b == 1), "the r == 0 branch belongs to the shifted box alone"
            norm = np.linalg.norm(want[:, :3].astype(np.float64), axis=1)
            assert np.allclose(norm, 1.0, atol=1e-6)
            runs = []
            for _ in range(2):
                buf = route.out((n_cells * k ** 3, 4))
                offs = [float(np.float32(np.float32(j + 0.5) / np.float32(k))) if j < k else 0.0 for j in range(3)]
                route.call("scnerf_occ_probe_points_inverted", first, n_cells, R, k, *[float(x) for x in lo],
                           *[float(x) for x in cell], *offs, buf[1])
                route.sync()
                runs.append(_guards_kept(route, buf[0], "pts"))
            for got in runs:
                assert got.shape == want.shape and got.tobytes() == want.tobytes(), (k, b, first)
            # a probe inside the ball lies in its own cell by the samples' lookup
            inside = want[:, 3] < 1.0
            q = (want[:, :3] * want[:, 3:4]).astype(np.float32)
            t = np.floor(((q - lo) * inv).astype(np.float32)).astype(np.int64)
            c = first + np.arange(n_cells).repeat(k ** 3)
            own = np.stack([c % R, (c // R) % R, c // (R * R)], 1)
            assert (np.abs(t - own)[inside] <= 1).all()
            assert ((t == own).all(1) | ~inside).mean() > 0.95


def argument_checks(route):
    """case 3"""
    bits, R, lo, inv = kernel_grid("halfball", BOXES[0])
    pts, vd = kernel_points(64, 16, BOXES[0])
    box = [float(x) for x in lo] + [float(x) for x in inv]
    keep = {"pts": route.inp(pts), "vd": route.inp(vd), "bits": route.inp(bits)}

    def compact(P=64, spr=16, R_=R, stride=5, null=None, shift=None):
        a = {"pts": keep["pts"], "vd": keep["vd"], "bits": keep["bits"], "ws": route.out((4,), np.int32)[1],
             "idx": route.out((64,), np.int32)[1], "slot": route.out((64,), np.int32)[1], "pl": route.out((64, 4))[1],
             "vl": route.out((64, 3))[1], "nd": route.out((1,), np.int32)[1]}
        if null:
            a[null] = None
        if shift:
            a[shift] = route.shifted(a[shift])                     # four bytes on: no longer 16-byte aligned
        return route.status("scnerf_occ_compact4", a["pts"], P, a["vd"], stride, spr, a["bits"], R_, *box, a["ws"], a["idx"],
                            a["slot"], a["pl"], a["vl"], a["nd"], None)
    assert compact() == 0
    for null in ("pts", "vd", "bits", "ws", "idx", "slot", "pl", "vl", "nd"):
        assert compact(null=null) == EINVAL, null
    assert compact(R_=48) == EINVAL and compact(R_=0) == EINVAL and compact(R_=2048) == EINVAL
    assert compact(P=1 << 31) == EINVAL and compact(P=-1) == EINVAL
    assert compact(spr=0) == EINVAL and compact(stride=2) == EINVAL
    assert compact(shift="pts") == EINVAL and compact(shift="pl") == EINVAL
    assert compact(P=0, null="pts") == 0                         # no sample: the arrays may be null
    assert route.size("scnerf_occ_compact4_workspace_ints", -1) == -1
    geo = [-1.0, -1.0, -1.0, 0.0625, 0.0625, 0.0625, 0.5, 0.0, 0.0]
    p4 = route.out((64, 4))[1]
    probe = lambda first=64, n=64, R_=32, k=1, out=p4: route.status("scnerf_occ_probe_points_inverted", first, n, R_, k, *geo, out)
    assert probe() == 0
    assert probe(first=32) == EINVAL                              # first cell not a multiple of 64
    assert probe(R_=48) == EINVAL and probe(k=4) == EINVAL and probe(k=0) == EINVAL and probe(out=None) == EINVAL
    assert probe(first=32 ** 3 - 64, n=128) == EINVAL             # past the grid
    assert probe(n=-1) == EINVAL and probe(n=0, out=None) == 0
    route.sync()


# ---- the node ----------------------------------------------------------------------------------------------------------------
BOX = ((-1.0,) * 3, (1.0,) * 3)
WIDE = ((-64.0,) * 3, (64.0,) * 3)
NODE_R = 32
make_net, node_inputs, arithmetic, forward, same_bits = SB.make_net, SB.node_inputs, SB.arithmetic, SB.forward, SB.same_bits


def centres(R=NODE_R, box=BOX):
    c = [box[0][a] + (np.arange(R, dtype=np.float64) + 0.5) * (box[1][a] - box[0][a]) / R for a in range(3)]
    return c[0][None, None, :], c[1][None, :, None], c[2][:, None, None]                # x, y, z of mask[z, y, x]


def fg_mask(R=NODE_R):
    """foreground, [-1, 1]^3: a half-space -- the cells whose centre has x + y + z <= 0.35 are set"""
    x, y, z = centres(R)
    return np.broadcast_to(x + y + z <= FG_PLANE, (R, R, R)).copy()


def bg_mask(R=NODE_R):
    """background, q in [-1, 1]^3: a half-ball in w -- the cells whose centre has |q| <= 0.5 (r >= 2) are set"""
    x, y, z = centres(R)
    return x * x + y * y + z * z <= BG_RADIUS ** 2


FG_PLANE, BG_RADIUS = 0.35, 0.5


def hand_grid(mask, device, space, box=BOX):
    from scnerf_amd.occupancy import OccupancyGrid
    return OccupancyGrid.from_mask(torch.from_numpy(np.ascontiguousarray(mask)), box[0], box[1], space=space).to(device)


def mixed_grids(device):
    return hand_grid(fg_mask(), device, "euclidean"), hand_grid(bg_mask(), device, "inverted_sphere")


def constant_grids(device, value):
    m = np.full((NODE_R,) * 3, value, bool)
    return hand_grid(m, device, "euclidean", WIDE), hand_grid(m, device, "inverted_sphere", WIDE)


def grid_arrays(grid):
    return (grid.bits.cpu().numpy(), grid.resolution, np.asarray(grid.lo, np.float32), np.asarray(grid.inv, np.float32))


@contextlib.contextmanager
def switched(ops, fg, bg):
    assert ops.inference_occupancy_nerfpp() is None
    ops.inference_occupancy_nerfpp(fg, bg)
    try:
        yield
    finally:
        ops.inference_occupancy_nerfpp("off")


def points(ops, inputs):
    """scnerf_npp_points_fwd stand-alone -> fg_pts [n sf, 3], bg_pts [n sb, 4], views [n, 3]"""
    from scnerf_amd import _capi
    o, d, far, fg_z, bg_z = (t.contiguous().float() for t in inputs)
    n, sf, sb = o.shape[0], fg_z.shape[1], bg_z.shape[1]
    fg_pts, bg_pts, views = (torch.empty(s, dtype=torch.float32, device=o.device) for s in ((n * sf, 3), (n * sb, 4), (n, 3)))
    P = ops._p
    _capi.check(_capi.load().scnerf_npp_points_fwd(P(o), P(d), P(fg_z), P(bg_z), P(fg_pts), P(bg_pts), P(views), None, n, sf, sb,
                                                   ops._stream()), "scnerf_npp_points_fwd")
    return fg_pts, bg_pts, views


def masked_raws(ops, net, inputs, grids):
    """the dense networks on every sample with one view direction per sample, the rows of the samples a grid calls dead zeroed
    -> (raw_fg [n sf, 4], raw_bg [n sb, 4], dead_fg [n, sf], dead_bg [n, sb])"""
    fg_pts, bg_pts, views = points(ops, inputs)
    n = views.shape[0]
    raws, deads = [], []
    for sub, pts, pd, grid in ((net.fg_net, fg_pts, 3, grids[0]), (net.bg_net, bg_pts, 4, grids[1])):
        s = pts.shape[0] // n
        wf, pl = ops.network_packs(sub, sub.flat_parameters(), False, n, pd, remap=sub.pack_remap())
        raw = ops.mlp_fwd(pts, views.repeat_interleave(s, 0).contiguous(), 1, wf, None, pd=pd, planes=pl)
        if grid is None:
            dead = torch.zeros(n * s, dtype=torch.bool, device=raw.device)
        else:
            fn = REF.dead_mask if pd == 3 else REF4.dead_mask4
            dead = torch.from_numpy(fn(pts.cpu().numpy(), *grid_arrays(grid))).to(raw.device)
        raws.append(torch.where(dead[:, None], torch.zeros_like(raw), raw))
        deads.append(dead.view(n, s))
    return raws[0], raws[1], deads[0], deads[1]


def composite(ops, raw_f, raw_b, inputs):
    from scnerf_amd import _capi
    o, d, far, fg_z, bg_z = (t.contiguous().float() for t in inputs)
    n, sf, sb = o.shape[0], fg_z.shape[1], bg_z.shape[1]
    sh = SB.NR.composite_shapes(n, sf, sb)
    t = {k: torch.empty(sh[k], dtype=torch.float32, device=o.device) for k in KEYS}
    P = ops._p
    _capi.check(_capi.load().scnerf_npp_composite_fwd(P(raw_f), P(raw_b), P(fg_z), P(far), P(bg_z), P(d), *[P(t[k]) for k in KEYS],
                                                      n, sf, sb, ops._stream()), "scnerf_npp_composite_fwd")
    return t


def oracle(ops, net, inputs, grids, eps=None):
    """the switch-off pipeline from stand-alone launches with the dead rows zeroed -> (the eight outputs, the expected
    occupancy_nerfpp_stats() of the call).  `eps`: None, a float or "median" -- with inference_skip_background, the raw_bg rows of
    the rays with bg_lambda <= eps are zeros too and the background grid sees the live rays alone; -> also (eps, live)"""
    assert ops.inference_occupancy_nerfpp() is None and ops.inference_skip_background() is None
    with torch.no_grad():
        raw_f, raw_b, dead_f, dead_b = masked_raws(ops, net, inputs, grids)
        out = composite(ops, raw_f, raw_b, inputs)
        n, sf, sb = dead_f.shape[0], dead_f.shape[1], dead_b.shape[1]
        live = torch.ones(n, dtype=torch.bool, device=raw_f.device)
        if eps is not None:
            lam = out["bg_lambda"]
            if eps == "median":
                eps = float(lam.median())
            live = SB.live_mask(lam, eps)
            raw_b = torch.where(live.repeat_interleave(sb)[:, None], raw_b, torch.zeros_like(raw_b))
            out = composite(ops, raw_f, raw_b, inputs)
        n_live = int(live.sum())
        stats = {"fg_samples": n * sf if grids[0] is not None else 0, "fg_skipped": int(dead_f.sum()),
                 "bg_samples": n_live * sb if grids[1] is not None else 0, "bg_skipped": int(dead_b[live].sum())}
    return out, stats, eps, live


def same_eight(got, want, what=""):
    assert list(got.keys()) == list(KEYS)
    for k in KEYS:
        same_bits(got[k].reshape(want[k].shape), want[k], what + k)


def share_is_mixed(stats, which):
    share = stats[which + "_skipped"] / float(stats[which + "_samples"])
    assert 0.2 <= share <= 0.8, (which, share)
    return share


def mixed_case(ops, device, mode, guard=None):
    """case 4 (and the guard half of case 6): both grids mixed, all eight outputs equal the oracle, the dead shares of both
    networks lie in [0.2, 0.8] by the switch's own counts, which equal the transcription's"""
    saved = ops.resident_guard()
    with arithmetic(ops, mode):
        net, inputs = make_net(device), node_inputs(device)
        grids = mixed_grids(device)
        want, stats, _, _ = oracle(ops, net, inputs, grids)
        before = ops.occupancy_stats()
        ops.occupancy_nerfpp_stats(reset=True)
        if guard is not None:
            ops.resident_guard(guard)
        try:
            with switched(ops, *grids):
                got = forward(net, inputs)
        finally:
            ops.resident_guard(saved)
        counted = ops.occupancy_nerfpp_stats(reset=True)
        print("nerfpp occupancy %s: dead share fg %.3f, bg %.3f" % (mode, share_is_mixed(counted, "fg"), share_is_mixed(counted, "bg")))
        assert counted == stats, (counted, stats)
        assert ops.occupancy_stats() == before, "occupancy_stats() moved"
        same_eight(got, want, "%s%s: " % (mode, "" if guard is None else ", guard " + guard))
        off = forward(net, inputs)
        assert any(SB.bits(got[k]).tobytes() != SB.bits(off[k]).tobytes() for k in KEYS), "the grids changed nothing"


def one_grid_case(ops, device, mode, which, monkeypatch):
    """case 5: a grid in one slot alone -- mixed: the oracle with the other network dense; every cell set: the switch-off call's
    bits; no cell set (a box that holds every sample): that network is never launched, the outputs are those of zero raws"""
    pick = lambda pair: (pair[0], None) if which == "fg" else (None, pair[1])
    pd_other = 4 if which == "fg" else 3
    with arithmetic(ops, mode):
        net, inputs = make_net(device), node_inputs(device)
        off = forward(net, inputs)
        samples = N * (SF if which == "fg" else SB_)
        zero = {"fg_samples": 0, "fg_skipped": 0, "bg_samples": 0, "bg_skipped": 0}
        # mixed
        grids = pick(mixed_grids(device))
        want, stats, _, _ = oracle(ops, net, inputs, grids)
        ops.occupancy_nerfpp_stats(reset=True)
        with switched(ops, *grids):
            got = forward(net, inputs)
        counted = ops.occupancy_nerfpp_stats(reset=True)
        assert counted == stats and counted[which + "_samples"] == samples, (counted, stats)
        share_is_mixed(counted, which)
        same_eight(got, want, "%s grid alone: " % which)
        # every cell set
        with switched(ops, *pick(constant_grids(device, True))):
            got = forward(net, inputs)
        assert ops.occupancy_nerfpp_stats(reset=True) == dict(zero, **{which + "_samples": samples})
        same_eight(got, off, "every cell set: ")
        # no cell set
        grids = pick(constant_grids(device, False))
        want, stats, _, _ = oracle(ops, net, inputs, grids)
        assert stats[which + "_skipped"] == samples
        launches = []
        real = ops.mlp_fwd
        monkeypatch.setattr(ops, "mlp_fwd", lambda *a, **kw: (launches.append(kw.get("pd", 3)), real(*a, **kw))[1])
        with switched(ops, *grids):
            got = forward(net, inputs)
        monkeypatch.setattr(ops, "mlp_fwd", real)
        assert launches == [pd_other], launches
        assert ops.occupancy_nerfpp_stats(reset=True) == stats
        same_eight(got, want, "no cell set: ")
        if which == "bg":
            assert not SB.bits(got["bg_weights"]).any() and not SB.bits(got["bg_rgb"]).any()
            same_bits(got["rgb"], got["fg_rgb"], "rgb == fg_rgb without a background")
        else:
            assert not SB.bits(got["fg_weights"]).any() and not SB.bits(got["fg_rgb"]).any()


def nothing_live_case(ops, device, mode, monkeypatch):
    """case 5, both slots: no cell set in either grid -- no network launch at all"""
    with arithmetic(ops, mode):
        net, inputs = make_net(device), node_inputs(device)
        grids = constant_grids(device, False)
        want, stats, _, _ = oracle(ops, net, inputs, grids)
        launches = []
        real = ops.mlp_fwd
        monkeypatch.setattr(ops, "mlp_fwd", lambda *a, **kw: (launches.append(kw.get("pd", 3)), real(*a, **kw))[1])
        ops.occupancy_nerfpp_stats(reset=True)
        with switched(ops, *grids):
            got = forward(net, inputs)
        monkeypatch.setattr(ops, "mlp_fwd", real)
        assert not launches, launches
        assert ops.occupancy_nerfpp_stats(reset=True) == stats == {"fg_samples": N * SF, "fg_skipped": N * SF,
                                                                   "bg_samples": N * SB_, "bg_skipped": N * SB_}
        same_eight(got, want, "nothing live: ")
        assert not SB.bits(got["rgb"]).any() and not SB.bits(got["fg_weights"]).any() and not SB.bits(got["bg_weights"]).any()


def with_skip_background_case(ops, device, mode, extremes=True):
    """case 6: with inference_skip_background(eps) -- the skip-background result with the dead rows zeroed: the foreground
    under its grid, bg_lambda from the expanded raw, the background grid on the points of the live rays"""
    with arithmetic(ops, mode):
        net, inputs = make_net(device), node_inputs(device)
        grids = mixed_grids(device)
        want, stats, eps, live = oracle(ops, net, inputs, grids, eps="median")
        k = int((~live).sum())
        assert 0.0 < eps < 1.0 and 0 < k < N, (eps, k)
        ops.occupancy_nerfpp_stats(reset=True)
        ops.skip_background_stats(reset=True)
        with SB.switched(ops, eps), switched(ops, *grids):
            got = forward(net, inputs)
        assert ops.skip_background_stats(reset=True) == {"rays": N, "skipped": k}
        assert ops.occupancy_nerfpp_stats(reset=True) == stats, stats
        same_eight(got, want, "with skip_background: ")
        dead = ~live
        same_bits(got["rgb"][dead], got["fg_rgb"][dead], "skipped rays: rgb == fg_rgb")
        assert not SB.bits(got["bg_weights"][dead]).any()
        # (nearly) every ray live and (nearly) no ray live: the same composition
        for e in ((0.0, 0.999999) if extremes else ()):
            want, stats, _, lv = oracle(ops, net, inputs, grids, eps=e)
            ops.occupancy_nerfpp_stats(reset=True)
            with SB.switched(ops, e), switched(ops, *grids):
                got = forward(net, inputs)
            assert ops.occupancy_nerfpp_stats(reset=True) == stats
            same_eight(got, want, "with skip_background(%g): " % e)


def tracking_call_case(ops, device, mode):
    """case 7: a call that tracks gradients does not notice the switch: outputs and gradients"""
    with arithmetic(ops, mode):
        net = make_net(device)
        o, d, far, fg_z, bg_z = node_inputs(device, n=4)

        def step():
            net.zero_grad()
            oo = o.clone().requires_grad_(True)
            ret = net(oo, d, far, fg_z, bg_z)
            (ret["rgb"].sum() + ret["bg_depth"].sum()).backward()
            return ({k: v.detach().clone() for k, v in ret.items()}, oo.grad.clone(),
                    [p.grad.detach().clone() for p in net.parameters()])

        a = step()
        ops.occupancy_nerfpp_stats(reset=True)
        with switched(ops, *mixed_grids(device)):
            b = step()
        assert not any(ops.occupancy_nerfpp_stats().values())                 # the compaction never ran
        for k in KEYS:
            same_bits(a[0][k], b[0][k], k)
        same_bits(a[1], b[1], "d ray_o")
        assert float(b[1].abs().max()) > 0 and len(a[2]) == len(b[2]) > 0
        for i, (ga, gb) in enumerate(zip(a[2], b[2])):
            same_bits(ga, gb, "gradient of parameter %d" % i)


def euclidean_switch_is_ignored_case(ops, device, mode):
    """case 8: ops.inference_occupancy(euclidean grid) is still ignored by the NeRF++ node"""
    with arithmetic(ops, mode):
        net, inputs = make_net(device), node_inputs(device)
        off = forward(net, inputs)
        ops.occupancy_stats(reset=True)
        ops.occupancy_nerfpp_stats(reset=True)
        ops.inference_occupancy(constant_grids(device, False)[0])
        try:
            on = forward(net, inputs)
        finally:
            ops.inference_occupancy("off")
        assert ops.occupancy_stats() == {"samples": 0, "skipped": 0} and not any(ops.occupancy_nerfpp_stats().values())
        same_eight(on, off)


def wrong_device_case(ops, device):
    import pytest
    """grids on the host, rays on the device: a ValueError from either slot"""
    net, inputs = make_net(device), node_inputs(device)
    fg, bg = mixed_grids("cpu")
    for pair in ((fg, None), (None, bg)):
        with pytest.raises(ValueError):
            with switched(ops, *pair):
                forward(net, inputs)
    assert forward(net, inputs)["rgb"].shape == (N, 3)


# ---- baking ----------------------------------------------------------------------------------------------------------------
def bake_reference(ops, device, subnets, space, probes, R, box, sigma_min, dilate, passes=None):
    """the transcription fed with the very raw ops.mlp_fwd returns for the probe points -> words"""
    from scnerf_amd.occupancy import MAX_PASS_POINTS
    lo, hi, inv, cell = REF.box(box[0], box[1], R)
    k = probes
    direction = torch.tensor([[0.0, 0.0, 1.0]], device=device)
    want = np.zeros(R ** 3 // 32, np.int32)
    per_pass = MAX_PASS_POINTS // k ** 3 // 64 * 64               # the passes the bake itself makes
    if passes is None:
        passes = [(f, min(per_pass, R ** 3 - f)) for f in range(0, R ** 3, per_pass)]
    pd = 3 if space == "euclidean" else 4
    with torch.no_grad():
        for f, nc in passes:
            args = (f, nc, R, k, [float(x) for x in lo], [float(x) for x in cell], device)
            if pd == 3:
                pts = ops.occ_probe_points(*args)
                assert pts.cpu().numpy().tobytes() == REF.probe_points(f, nc, R, k, lo, cell).tobytes()
            else:
                pts = ops.occ_probe_points_inverted(*args)
                assert pts.cpu().numpy().tobytes() == REF4.probe_points_inverted(f, nc, R, k, lo, cell).tobytes()
            for sub in subnets:
                wf, pl = ops.network_packs(sub, sub.flat_parameters(), False, pts.shape[0], pd, remap=sub.pack_remap())
                raw = ops.mlp_fwd(pts, direction, pts.shape[0], wf, None, pd=pd, planes=pl)
                want = REF.accumulate(want, raw.cpu().numpy(), sigma_min, f, nc, R, k)
    for _ in range(dilate):
        want = REF.dilate(want, R)
    return want


def bake_case(ops, device, probes, dilate, R=32):
    """case 9: bake_nerfpp over two cascade levels against the transcription, both spaces; the grids serve their networks"""
    from scnerf_amd import occupancy as OC
    nets = [make_net(device, 778), make_net(device, 781)]
    fg, bg = OC.bake_nerfpp(nets, resolution=R, probes=probes, sigma_min=0.0, dilate=dilate)
    assert (fg.space, bg.space) == ("euclidean", "inverted_sphere") and fg.resolution == bg.resolution == R
    assert fg.lo == bg.lo == (-1.0,) * 3 and fg.hi == bg.hi == (1.0,) * 3
    for grid, subs in ((fg, [n.fg_net for n in nets]), (bg, [n.bg_net for n in nets])):
        want = bake_reference(ops, device, subs, grid.space, probes, R, BOX, 0.0, dilate)
        assert grid.bits.cpu().numpy().tobytes() == want.tobytes(), grid.space
        assert grid.occupied_fraction() == int(REF.mask_of_bits(want, R).sum()) / float(R ** 3)
        grid.check(*subs)
        back = OC.OccupancyGrid.from_state_dict(grid.state_dict())
        assert back.space == grid.space and back.bits.numpy().tobytes() == want.tobytes()
        assert grid.to("cpu").space == grid.space
    return nets, fg, bg


def one_baking_pass_case(ops, device, probes=1, R=32):
    """the interpreter's share of case 9: one pass of 64 cells around q = 0 through the stand-alone ops, inverted space"""
    net = make_net(device)
    first, nc = ((R // 2) * R + R // 2) * R, 64
    want = bake_reference(ops, device, [net.bg_net], "inverted_sphere", probes, R, BOX, 0.0, 0, passes=[(first, nc)])
    lo, hi, inv, cell = REF.box(BOX[0], BOX[1], R)
    bits = torch.zeros(R ** 3 // 32, dtype=torch.int32, device=device)
    with torch.no_grad():
        pts = ops.occ_probe_points_inverted(first, nc, R, probes, [float(x) for x in lo], [float(x) for x in cell], device)
        sub = net.bg_net
        wf, pl = ops.network_packs(sub, sub.flat_parameters(), False, pts.shape[0], 4, remap=sub.pack_remap())
        raw = ops.mlp_fwd(pts, torch.tensor([[0.0, 0.0, 1.0]], device=device), pts.shape[0], wf, None, pd=4, planes=pl)
        ops.occ_accumulate(raw, 0.0, first, nc, R, probes, bits)
    assert bits.cpu().numpy().tobytes() == want.tobytes()


def stale_and_foreign_case(ops, device, net=None, grids=None):
    """case 9: a baked grid serves the networks it was baked from, with the weights it was baked from"""
    import pytest
    from scnerf_amd.occupancy import OccupancyGrid, OccupancyStaleError
    if net is None:
        net = make_net(device)
        # (bound by hand: what from_state_dict(sd, networks) does after a bake)
        fg, bg = mixed_grids(device)
        grids = (OccupancyGrid.from_state_dict(fg.state_dict(), networks=[net.fg_net]),
                 OccupancyGrid.from_state_dict(bg.state_dict(), networks=[net.bg_net]))
        assert grids[1].space == "inverted_sphere"
    inputs = node_inputs(device, n=4)
    with switched(ops, *grids):
        forward(net, inputs)
    other = make_net(device, 779)
    for pair in ((grids[0], None), (None, grids[1])):
        with pytest.raises(OccupancyStaleError):
            with switched(ops, *pair):
                forward(other, inputs)
    with torch.no_grad():
        net.bg_net.sigma_layers[0].bias.add_(0.0)               # an in-place write: the version moves, whatever the value
    with switched(ops, grids[0], None):
        forward(net, inputs)                                      # the foreground network is as it was
    with pytest.raises(OccupancyStaleError):
        with switched(ops, *grids):
            forward(net, inputs)
    # grids made by hand check nothing
    with switched(ops, *mixed_grids(device)):
        forward(other, inputs)


def validation(ops):
    """case 9, the checks that need no kernel: the switch, the spaces, the state dict"""
    import pytest
    from scnerf_amd.occupancy import OccupancyGrid
    assert ops.inference_occupancy_nerfpp() is None
    fg, bg = mixed_grids("cpu")
    assert (fg.space, bg.space) == ("euclidean", "inverted_sphere")
    for bad in ((bg, None), (None, fg), (bg, fg), (0.5, None), (None, "on"), ("off", bg), (True, None)):
        with pytest.raises(ValueError):
            ops.inference_occupancy_nerfpp(*bad)
        assert ops.inference_occupancy_nerfpp() is None
    assert ops.inference_occupancy_nerfpp(fg, bg) == (fg, bg) and ops.inference_occupancy_nerfpp() == (fg, bg)
    assert ops.inference_occupancy_nerfpp(None, bg) == (None, bg)
    assert ops.inference_occupancy_nerfpp(fg) == (fg, None)
    assert ops.inference_occupancy_nerfpp("off") is None and ops.inference_occupancy_nerfpp() is None
    assert ops.occupancy_nerfpp_stats(reset=True).keys() == {"fg_samples", "fg_skipped", "bg_samples", "bg_skipped"}
    assert not any(ops.occupancy_nerfpp_stats().values())
    # the render_rays switch refuses an inverted grid and keeps taking euclidean ones
    with pytest.raises(ValueError):
        ops.inference_occupancy(bg)
    assert ops.inference_occupancy() is None
    assert ops.inference_occupancy(fg) is fg and ops.inference_occupancy("off") is None
    for fn, grid in ((ops.occ_compact, bg), (ops.occ_compact4, fg)):
        with pytest.raises(ValueError):
            fn(torch.zeros(4, 4 if grid is fg else 3), torch.zeros(4, 3), 1, grid)
    # the space travels: to(), state_dict(); a dict without the key holds a euclidean grid
    with pytest.raises(ValueError):
        OccupancyGrid.from_mask(torch.zeros((32,) * 3, dtype=torch.bool), BOX[0], BOX[1], space="spherical")
    sd = bg.state_dict()
    assert sd["space"] == "inverted_sphere" and OccupancyGrid.from_state_dict(sd).space == "inverted_sphere"
    assert bg.to("cpu").space == "inverted_sphere" and fg.state_dict()["space"] == "euclidean"
    old = {k: v for k, v in sd.items() if k != "space"}
    assert OccupancyGrid.from_state_dict(old).space == "euclidean"
    # a network's points fit one space
    net = make_net("cpu")
    with pytest.raises(ValueError):
        OccupancyGrid.bake([net.fg_net], BOX[0], BOX[1], resolution=32, space="inverted_sphere")
    with pytest.raises(ValueError):
        OccupancyGrid.bake([net.bg_net], BOX[0], BOX[1], resolution=32)
    with pytest.raises(ValueError):
        OccupancyGrid.bake([net.fg_net], BOX[0], BOX[1], resolution=32, space="spherical")


# ---- render_single_image ---------------------------------------------------------------------------------------------------
def render_single_image_case(ops, device, mode, rank):
    """case 10: two cascade levels on a 6 x 4 image in chunks of 10 rays, world_size 1, level by level: every call of a
    level's node is recorded with the inputs the level gave it -- the finer level's depths come from the weights the coarser
    level returned -- and equals the oracle of case 4 on those inputs; the statistics are the calls' sums"""
    from collections import OrderedDict
    from scnerf_amd import synthetic as synth
    from scnerf_amd.nerfplusplus import ddp_train_nerf as TR
    Hh, Ww = 6, 4
    o, d, near = synth.nerfpp_rays(Hh * Ww, seed=41)

    class Sampler:
        H, W = Hh, Ww

        def get_all(self, camera_model, camera_idx, sampler, rank):
            return OrderedDict(ray_o=o, ray_d=d, depth=torch.zeros(Hh * Ww), rgb=None, mask=None, min_depth=near, img_name="x")

    with arithmetic(ops, mode):
        models = OrderedDict(cascade_level=2, cascade_samples=[10, 6], net_0=make_net(device, 781), net_1=make_net(device, 782))
        calls = []
        hooks = [models["net_%d" % m].register_forward_hook(
            lambda mod, args, out, m=m: calls.append((m, mod, tuple(a.detach().clone() for a in args),
                                                      {k: v.detach().clone() for k, v in out.items()}))) for m in range(2)]
        grids = mixed_grids(device)
        ops.occupancy_nerfpp_stats(reset=True)
        try:
            with switched(ops, *grids):
                image = TR.render_single_image(rank, 1, models, Sampler(), 10, None, camera_idx=None)
        finally:
            for h in hooks:
                h.remove()
        counted = ops.occupancy_nerfpp_stats(reset=True)
        assert [c[0] for c in calls] == [0, 1] * 3 and len(image) == 2
        total = {k: 0 for k in counted}
        for m, mod, args, got in calls:
            assert args[3].shape[-1] == (10, 16)[m] and args[4].shape[-1] == (10, 16)[m]
            want, stats, _, _ = oracle(ops, mod, args, grids)
            same_eight(got, want, "level %d: " % m)
            for k in total:
                total[k] += stats[k]
        assert counted == total, (counted, total)
        assert total["fg_samples"] == total["bg_samples"] == Hh * Ww * (10 + 16)
        assert 0 < total["fg_skipped"] < total["fg_samples"] and 0 < total["bg_skipped"] < total["bg_samples"]
        print("render_single_image %s: %s" % (mode, counted))
