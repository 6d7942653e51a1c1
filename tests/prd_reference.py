"""TEST INFRASTRUCTURE: cases, fp64 references and bounds of the stand-alone tests of the projected-ray-distance kernels
(csrc/prd_loss.hip: scnerf_prd_loss_fwd in both modes, scnerf_prd_loss_bwd, scnerf_prd_filter): tests/test_emu_prd_kernels.py
on the CPU SIMT interpreter and tests/test_gpu_prd_kernels.py on the GPU.  Both routes run the SAME launches (`run` below,
through a `route` object that only knows how to hold a buffer and call the C ABI), see the same float32 inputs, references
and bounds.

Inputs: two cameras of synthetic.camera_spec's rig (120 x 160, focal 140), synthetic.matched_keypoints (pixel noise, 25 %
unrelated pairs, points behind a camera; seed 8 + m, SEEDS where that seed holds a match whose fp32 error asks for a wider
DELTA), rays by the pinhole formula, about half of the directions scaled by a factor in [0.5, 2].  negate_fx = 0 runs on the
scene mirrored about cx.  The special-rows case plants PLANT's rows at m = 65, each a copy of a valid match changed in one way.
References: oracle.scnerf_oracle.prd_match_errors / prd_loss on float64 leaves, gradients by autograd; yardstick E32: the same
on float32 leaves.  The planted rows with a non-finite error or a zero direction (DROPPED) are left out of the differentiated
call -- autograd would spread 0 * NaN from them into every sum -- and their gradient rows must be exactly +-0.

Counts (sums6 slots 1, 3, 4, 5 in both modes, `keep`): the fp64 classification, exactly.  A match is borderline when an fp64
error lies within DELTA of the threshold (relative) or an fp64 t within DELTA of 0 relative to |o0 - o1|; a count may differ by
the number of borderline matches of its kind.  DELTA = 1e-3: 8 x the fp32 oracle's largest relative error in L over the
matches within a factor 2 of the threshold is 9.4e-4 over all cases (m = 4097; 8.5e-4 at m = 257, 8.1e-4 at m = 63), rounded up
to a power of ten; test_margin_of_the_borderline_rule_covers_the_fp32_oracle re-measures it.  Borderline share: 0 of m in every
case of either route, 1000 and 4097 included (the condition, asserted in `references`: none at m <= 257, at most 1 % beyond).
Exact statements: guards untouched (a NaN row before and after every float output, GUARD_BYTE around `keep`); gradient rows
of a match masked both ways +-0; rows 3 of dK and dE 0; per-match gradients and `keep` bit for bit between two launches; a
NaN or inf error alone in an eval-mode launch gives sums6 = (thr, 1, thr, 1, 0, 1) and loss = thr; m = 0 through all entries.
Metric: largest |x - fp64| over a tensor / largest |fp64| entry of that tensor (composite_reference.metric), for the loss of
either mode, the four per-match gradient tensors, dK and dE.  Not per row: rows whose residual happens to be tiny carry
almost pure rounding noise, and the fp32 oracle itself then sits at 1e-3 .. 3e-1 from fp64.
Bound: figure <= K * max(E32, 2^-23), K the smallest power of two >= twice the worst ratio measured on either route, never
under 4, never over 16 (the rule of tests/camera_reference.py).

Worst ratio figure / max(E32, 2^-23) measured over these cases, interpreter | MI355X (the fp32 oracle runs on the host of
either route, so E32 differs between the columns; the interpreter column covers its own, shorter case list):
  loss 1.77 | 1.41   eval_loss 1.77 | 1.44   g_rays0_o 1.75 | 1.80   g_rays0_d 1.69 | 1.71   g_rays1_o 1.97 | 2.20
  g_rays1_d 2.81 (2.4e-4, m = 65) | 3.37 (6.7e-4, m = 65, threshold 1, negate_fx 0)   g_K 1.58 | 1.44   g_E2 1.53 | 1.17
                                                                                     worst 3.37 -> K_PRD = 8
Mutations of prd_loss.hip that the interpreter route catches (tests failing of 36): no `if (a.negate_fx) gk[0] = -gk[0]` 3,
`f->t1 >= 0.f` 1 (the special rows: a zero direction on ray 1 alone), `bad0` without `!finite_f(f.L0)` 2,
`ge[.. + 9 + aa] += gp[aa]` 12, `i <= a.m` in the backward's write guard 15.
"""
import numpy as np
import torch

from oracle import scnerf_oracle as O
from scnerf_amd import synthetic
from tests import camera_reference as CR
from tests.camera_reference import _cached, bound_check, case_id, report, same_bits  # noqa: F401  (one WORST table, one report)
from tests.composite_reference import assert_guards, metric
from tests.nerfpp_reference import FLOOR, assert_finite

K_PRD = 8.0
CR.K["prd"] = K_PRD                      # camera_reference.bound_check looks its factor up by family
DELTA = 1e-3

H_IMG, W_IMG, FOCAL = 120, 160, 140.0
CAMS = (0, 1)                            # the two cameras of synthetic.camera_spec's rig
EPS, FILTER_EPS = 1e-10, 1e-6            # ray_dist_loss.proj_ray_dist_loss_single | prd_evaluation.filter_matches_with_gt
GUARD_BYTE, UNWRITTEN = 0xA5, -7.0       # guard of `keep` | what the slot of the loss holds before the launch
COUNTS_BOTH = (1, 63, 64, 65, 257)
COUNTS_GPU = (255, 256, 1000, 4097)      # 4097: 17 blocks on the 6 + 36 atomic accumulators
SEEDS = {257: 1001, 4097: 1016}          # seed of the key points where 8 + m has a match whose fp32 error needs a wider DELTA
RAYS = ("rays0_o", "rays0_d", "rays1_o", "rays1_d")
INPUTS = ("kps0", "kps1") + RAYS + ("K", "E2")
GRADS = tuple("g_" + k for k in RAYS)
NUMERIC = ("loss",) + GRADS + ("g_K", "g_E2")
# the special-rows case (m = 65): row -> what is planted there.  First and last row, both sides of the lane 63 | 64 edge.
PLANT = dict(same_origin=0, inf_kp=1, only1=2, parallel=31, zero_dir1=32, only0=62, zero_dir0=63, nan_kp=64)
DROPPED = ("inf_kp", "zero_dir0", "zero_dir1", "nan_kp")           # autograd would spread 0 * NaN from these into every sum
EXACT_T = ("same_origin", "zero_dir0", "zero_dir1", "parallel")    # chirality false in any arithmetic: a t = +-0, or t0 = -t1


def prd_case(m=65, thr=5.0, neg=1, g=1.0, kind="plain"):
    """neg: negate_fx (0: the NeRF++ axes, on the scene mirrored about cx);  g: the incoming loss gradient;
    kind: plain | special (PLANT) | empty0 (every kps0 far off: no match valid in direction 0)"""
    return dict(m=m, thr=thr, neg=neg, g=g, kind=kind)


VARIANTS = (dict(thr=1.0), dict(neg=0), dict(thr=1.0, neg=0), dict(g=-0.37))
SPECIAL, EMPTY0 = prd_case(kind="special"), prd_case(m=64, kind="empty0")
CASES_BOTH = [prd_case(m) for m in COUNTS_BOTH] + [prd_case(65, **v) for v in VARIANTS] + [SPECIAL]
CASES_GPU = [prd_case(m) for m in COUNTS_GPU] + [prd_case(257, **v) for v in VARIANTS]


def twin(case):
    return dict(case, neg=1)


def _f32(d):
    return {k: np.ascontiguousarray(v, np.float32) for k, v in d.items()}


# ---- inputs ------------------------------------------------------------------------------------------------------------
def pinhole(kps, Kmat, E):
    """rays of key points (x, y) through a pinhole camera with NeRF's axes (x right, y up, looking down -z), float64"""
    dirs = np.stack([(kps[:, 0] - Kmat[0, 2]) / Kmat[0, 0], -(kps[:, 1] - Kmat[1, 2]) / Kmat[1, 1], -np.ones(len(kps))], -1)
    return np.tile(E[:3, 3], (len(kps), 1)), dirs @ E[:3, :3].T


def scene(m):
    """negate_fx = 1 inputs of m matches: synthetic's rig and matches (pixel noise, 25 % unrelated pairs, points behind a
    camera), pinhole rays, about half the directions scaled by a factor in [0.5, 2]"""
    def make():
        spec = synthetic.camera_spec(H_IMG, W_IMG, seed=4, focal=FOCAL)
        poses = spec["poses"][list(CAMS)]
        Kmat, E2 = spec["K_init"].double().numpy(), poses.double().numpy()
        if m:
            k0, k1 = synthetic.matched_keypoints(H_IMG, W_IMG, spec["K_init"], poses[0], poses[1], m,
                                                 seed=SEEDS.get(m, 8 + m))
            k0, k1 = k0.numpy(), k1.numpy()                       # float32: the rays start from the values the kernel reads
        else:
            k0 = k1 = np.zeros((0, 2), np.float32)
        rng = np.random.default_rng(100 + m)
        (o0, d0), (o1, d1) = pinhole(k0.astype(np.float64), Kmat, E2[0]), pinhole(k1.astype(np.float64), Kmat, E2[1])
        d0 = d0 * np.where(rng.random(m) < 0.5, 0.5 * 4.0 ** rng.random(m), 1.0)[:, None]
        d1 = d1 * np.where(rng.random(m) < 0.5, 0.5 * 4.0 ** rng.random(m), 1.0)[:, None]
        return _f32(dict(kps0=k0, kps1=k1, rays0_o=o0, rays0_d=d0, rays1_o=o1, rays1_d=d1, K=Kmat, E2=E2))
    return _cached(("prd_scene", m), make)


def match_state(inp, thr, neg, eps=EPS, dtype=torch.float64):
    """per match in `dtype`: the oracle's errors and chirality, t0 / t1 restated (asserted to give that chirality), the
    length scale |o0 - o1| -> dict of numpy arrays, with ok0 / ok1 = error below thr and finite"""
    T = {k: torch.from_numpy(inp[k]).to(dtype) for k in INPUTS}
    with torch.no_grad():
        l0, l1, chir = O.prd_match_errors(*[T[k] for k in INPUTS], eps, bool(neg))
        unit = lambda v: v / (v.norm(dim=-1, keepdim=True) + eps)
        d0, d1, w = unit(T["rays0_d"]), unit(T["rays1_d"]), T["rays0_o"] - T["rays1_o"]
        r = (d0 * d1).sum(-1)
        den = r ** 2 - 1 + eps
        t0 = ((d0 * w).sum(-1) - r * (d1 * w).sum(-1)) / den
        t1 = ((d1 * -w).sum(-1) - r * (d0 * -w).sum(-1)) / den
        assert torch.equal(chir, (t0 > 0) & (t1 > 0))
    s = dict(l0=l0.numpy(), l1=l1.numpy(), chir=chir.numpy(), t0=t0.numpy(), t1=t1.numpy(), scale=w.norm(dim=-1).numpy())
    with np.errstate(invalid="ignore"):
        s["ok0"], s["ok1"] = (s["l0"] < thr) & np.isfinite(s["l0"]), (s["l1"] < thr) & np.isfinite(s["l1"])
    return s


def inputs(case):
    m, kind = case["m"], case["kind"]
    inp = {k: v.copy() for k, v in scene(m).items()}
    if kind == "empty0":
        inp["kps0"] += np.float32(40.0)
    if kind == "special":
        s = match_state(inp, 1.0, 1)                            # donors: valid both ways even at threshold 1
        donors = [i for i in np.flatnonzero(s["chir"] & s["ok0"] & s["ok1"]) if i not in PLANT.values()]
        assert len(donors) >= len(PLANT)
        for (what, row), donor in zip(PLANT.items(), donors):
            for k in INPUTS[:6]:
                inp[k][row] = inp[k][donor]
            if what == "same_origin":                           # w = 0: t0 = t1 = +-0, chirality false by the strict >
                inp["rays1_o"][row] = inp["rays0_o"][row]
            elif what in ("zero_dir0", "zero_dir1"):            # d = 0 / eps = 0: that ray's t = +-0, the other's > 0
                i = int(what[-1])
                inp["rays%d_d" % i][row] = 0.0
                w = (inp["rays0_o"][row] - inp["rays1_o"][row]) * np.float32(1 - 2 * i)
                if np.dot(inp["rays%d_d" % (1 - i)][row], w) <= 0:          # (the other ray's t, up to its length): swap the origins
                    inp["rays0_o"][row], inp["rays1_o"][row] = inp["rays1_o"][row].copy(), inp["rays0_o"][row].copy()
            elif what == "nan_kp":                              # both errors non-finite while chirality holds
                inp["kps0"][row, 0] = inp["kps1"][row, 1] = np.nan
            elif what == "inf_kp":
                inp["kps0"][row, 1] = inp["kps1"][row, 0] = np.inf
            elif what == "only0":                               # a few pixels off on one side
                inp["kps1"][row] += np.float32([2.5, -2.0])
            elif what == "only1":
                inp["kps0"][row] += np.float32([-2.0, 2.5])
            elif what == "parallel":                            # bit-identical directions: r = |d|^2, den = eps + rounding
                inp["rays1_d"][row] = inp["rays0_d"][row]
                inp["kps0"][row] += np.float32([300.0, -200.0])
                inp["kps1"][row] += np.float32([-250.0, 350.0])
    if not case["neg"]:                                         # the same geometry seen with NeRF++'s axes
        for k in ("kps0", "kps1"):
            inp[k][:, 0] = np.float32(2.0) * inp["K"][0, 2] - inp[k][:, 0]
    return inp


# ---- references --------------------------------------------------------------------------------------------------------
def planted(case, names):
    return [PLANT[k] for k in names] if case["kind"] == "special" else []


def classify(inp, case, eps=EPS):
    """the fp64 verdicts and who is borderline: an error within DELTA of the threshold (relative), a t within DELTA of 0
    relative to the distance of the two origins.  Rows whose chirality is false in any arithmetic (EXACT_T) are never
    borderline."""
    s = match_state(inp, case["thr"], case["neg"], eps)
    exact = np.zeros(case["m"], bool)
    exact[planted(case, EXACT_T)] = True
    with np.errstate(invalid="ignore"):
        s["bl_t"] = ((np.abs(s["t0"]) <= DELTA * s["scale"]) | (np.abs(s["t1"]) <= DELTA * s["scale"])) & ~exact
        s["bl_0"] = (np.abs(s["l0"] - case["thr"]) <= DELTA * case["thr"]) & s["chir"] | s["bl_t"]
        s["bl_1"] = (np.abs(s["l1"] - case["thr"]) <= DELTA * case["thr"]) & s["chir"] | s["bl_t"]
    s["bl"] = s["bl_0"] | s["bl_1"]
    return s


def oracle(inp, case, dtype):
    """loss and every gradient of oracle.scnerf_oracle.prd_loss on leaves of `dtype`, the DROPPED rows left out (their
    gradient rows are zero); eval_loss on all rows.  empty0: the loss is NaN, the gradients those of direction 1 alone"""
    m, thr, neg = case["m"], case["thr"], bool(case["neg"])
    T = {k: torch.from_numpy(inp[k]).to(dtype) for k in INPUTS}
    leaves = {k: T[k].clone().requires_grad_(True) for k in RAYS + ("K", "E2")}
    keep = np.ones(m, bool)
    keep[planted(case, DROPPED)] = False
    rows = torch.from_numpy(np.flatnonzero(keep))
    args = [T["kps0"][rows], T["kps1"][rows]] + [leaves[k][rows] for k in RAYS] + [leaves["K"], leaves["E2"]]
    if case["kind"] == "empty0":
        l0, l1, chir = O.prd_match_errors(*args, EPS, neg)
        assert not (chir & (l0 < thr)).any()
        l1 = l1[chir]
        loss, n_match = 0.5 * l1[(l1 < thr) & torch.isfinite(l1)].mean(), 0.0
    else:
        loss, n_match = O.prd_loss(*args, thr, EPS, neg)
    (case["g"] * loss).backward()
    with torch.no_grad():
        ev, _ = O.prd_loss(*[T[k] for k in INPUTS], thr, EPS, neg, eval_mode=True)
    out = dict(loss=loss.reshape(1), eval_loss=ev.reshape(1), g_K=leaves["K"].grad, g_E2=leaves["E2"].grad)
    if case["kind"] == "empty0":
        del out["loss"]
    out.update({"g_" + k: leaves[k].grad for k in RAYS})
    return {k: v.detach().double().numpy() for k, v in out.items()}, n_match


def measured_delta(inp, case):
    """8 x the fp32 oracle's largest relative error in L against fp64 over the matches within a factor 2 of the threshold"""
    a, b = match_state(inp, case["thr"], case["neg"]), match_state(inp, case["thr"], case["neg"], dtype=torch.float32)
    worst = 0.0
    for k in ("l0", "l1"):
        with np.errstate(invalid="ignore"):
            near = (a[k] > 0.5 * case["thr"]) & (a[k] < 2.0 * case["thr"])
        if near.any():
            worst = max(worst, float((np.abs(b[k][near] - a[k][near]) / a[k][near]).max()))
    return 8.0 * worst


def references(case):
    """-> (inputs, fp64 oracle, fp32 oracle, fp64 verdicts of the loss, of the filter), once per session.  Preconditions
    asserted here: the oracles are finite and agree on n_match; no borderline match at m <= 257, at most 1 % beyond; the
    planted rows are what they are named"""
    def make():
        inp = inputs(case)
        (o64, n64), (o32, n32) = oracle(inp, case, torch.float64), oracle(inp, case, torch.float32)
        if case["m"]:
            assert_finite("prd " + case_id(case), o64, o32)
            assert n64 == n32, "the fp32 oracle classifies a match of %s differently" % case_id(case)
        cls, flt = classify(inp, case), classify(inp, case, FILTER_EPS)
        for c in (cls, flt):
            assert c["bl"].sum() <= (0 if case["m"] <= 257 else 0.01 * case["m"]), (case_id(case), np.flatnonzero(c["bl"]))
        if case["kind"] == "special":
            P, both = PLANT, cls["chir"] & cls["ok0"] & cls["ok1"]
            c32 = match_state(inp, case["thr"], case["neg"], dtype=torch.float32)
            assert not cls["chir"][[P["same_origin"], P["zero_dir0"], P["zero_dir1"], P["parallel"]]].any()
            assert cls["t0"][P["zero_dir0"]] == 0 and cls["t1"][P["zero_dir0"]] > 0           # each strict > on its own
            assert cls["t1"][P["zero_dir1"]] == 0 and cls["t0"][P["zero_dir1"]] > 0
            assert not c32["chir"][P["parallel"]] or not (c32["ok0"][P["parallel"]] or c32["ok1"][P["parallel"]])
            assert cls["chir"][[P["nan_kp"], P["inf_kp"]]].all()
            assert np.isnan(cls["l0"][P["nan_kp"]]) and np.isnan(cls["l1"][P["nan_kp"]])
            assert np.isinf(cls["l0"][P["inf_kp"]]) and np.isinf(cls["l1"][P["inf_kp"]])
            assert cls["chir"][P["only0"]] and cls["ok0"][P["only0"]] and not cls["ok1"][P["only0"]]
            assert cls["chir"][P["only1"]] and cls["ok1"][P["only1"]] and not cls["ok0"][P["only1"]]
            assert both.sum() >= 20
        return inp, o64, o32, cls, flt
    return _cached(("prd", CR._key(case)), make)


# ---- launches ----------------------------------------------------------------------------------------------------------
def collect(route, bufs):
    """guards intact, everything inside written -> name -> array without its guard rows"""
    got = {}
    for k, (buf, _) in bufs.items():
        b = route.host(buf)
        if b.dtype == np.uint8:
            assert (b[0] == GUARD_BYTE) and (b[-1] == GUARD_BYTE), k + ": written outside its rows"
            assert (b[1:-1] <= 1).all(), k + ": not written everywhere inside"
        elif k.endswith("loss"):                                # NaN is a value of the loss: its slot starts as UNWRITTEN
            assert np.isnan(b[0]) and np.isnan(b[-1]), k + ": written outside its rows"
            assert b[1] != UNWRITTEN, k + ": not written"
        else:
            assert_guards(b, k)
        got[k] = b[1:-1].copy()
    return got


def run_fwd(route, inp, case, eval_mode, bufs=None, tag=""):
    """scnerf_prd_loss_fwd into NaN buffers with a guard on each side"""
    m = inp["kps0"].shape[0]
    own = bufs is None
    bufs = {} if own else bufs
    bufs.update({tag + "sums6": route.out((6,)), tag + "loss": route.out((1,)), tag + "n_match": route.out((1,))})
    bufs[tag + "loss"][1][...] = UNWRITTEN
    route.call("scnerf_prd_loss_fwd", *[route.inp(inp[k]) for k in INPUTS], EPS, case["thr"], case["neg"], eval_mode, m,
               bufs[tag + "sums6"][1], bufs[tag + "loss"][1], bufs[tag + "n_match"][1])
    return collect(route, bufs) if own else None


def run(route, inp, case):
    """the forward in both modes, the backward on the train forward's sums, the filter -> name -> array"""
    m = case["m"]
    common = [route.inp(inp[k]) for k in INPUTS]
    bufs = {}
    run_fwd(route, inp, case, 0, bufs)
    run_fwd(route, inp, case, 1, bufs, "eval_")
    bufs.update({k: route.out((m, 3)) for k in GRADS})
    bufs.update(g_K=route.out((4, 4)), g_E2=route.out((2, 4, 4)), workspace=route.out((36,)))
    route.call("scnerf_prd_loss_bwd", *common, EPS, case["thr"], case["neg"], m, bufs["sums6"][1],
               route.inp(np.array([case["g"]], np.float32)), *[bufs[k][1] for k in GRADS], bufs["g_K"][1], bufs["g_E2"][1],
               bufs["workspace"][1])
    bufs["keep"] = route.out((m,), np.uint8)
    route.call("scnerf_prd_filter", *common, FILTER_EPS, case["thr"], case["neg"], m, bufs["keep"][1])
    return collect(route, bufs)


# ---- checks ------------------------------------------------------------------------------------------------------------
def check_counts(case, got, cls, flt):
    """sums6 slots 1, 3, 4, 5 of both modes and `keep`: the fp64 classification, exactly, but for borderline matches"""
    ch, ok0, ok1 = cls["chir"], cls["chir"] & cls["ok0"], cls["chir"] & cls["ok1"]
    slack = {1: cls["bl_0"].sum(), 3: cls["bl_1"].sum(), 4: cls["bl"].sum(), 5: cls["bl_t"].sum()}
    want = {1: ok0.sum(), 3: ok1.sum(), 4: (ok0 & ok1).sum(), 5: ch.sum()}
    print("prd %s counts %s  kernel %s  borderline %s" % (case_id(case), want, got["sums6"][[1, 3, 4, 5]], slack))
    for k in want:
        assert abs(float(got["sums6"][k]) - want[k]) <= slack[k], ("sums6", k, got["sums6"], want)
    for k, w in ((1, ch.sum()), (3, ch.sum()), (4, 0), (5, ch.sum())):
        assert abs(float(got["eval_sums6"][k]) - w) <= (slack[5] if w else 0), ("eval sums6", k, got["eval_sums6"], w)
    assert got["n_match"][0] == got["sums6"][4] and got["eval_n_match"][0] == 0
    sure = ~flt["bl"]
    np.testing.assert_array_equal(got["keep"][sure], (flt["chir"] & flt["ok0"] & flt["ok1"])[sure].astype(np.uint8))


def check_exact(case, got, cls):
    """the gradient rows of a match masked both ways are +-0, the fourth rows of dK and dE are 0"""
    masked = ~(cls["chir"] & (cls["ok0"] | cls["ok1"])) & ~cls["bl"]
    for k in GRADS:
        assert not got[k][masked].any(), k + ": a masked match has a gradient"
    assert not got["g_K"][3].any() and not got["g_E2"][:, 3].any()
    if case["m"] and case["kind"] != "empty0":
        assert masked.any() or case["m"] == 1


def check(case, got):
    inp, o64, o32, cls, flt = references(case)
    check_counts(case, got, cls, flt)
    check_exact(case, got, cls)
    if case["kind"] == "empty0":
        assert np.isnan(got["loss"][0]) and got["sums6"][1] == 0 and got["sums6"][3] > 0
    return bound_check("prd", case_id(case), got, o64, o32, tuple(k for k in NUMERIC + ("eval_loss",) if k in o64))


def check_twin(case, got, got_twin):
    """negate_fx = 0 on the mirrored scene against negate_fx = 1 on the scene itself: the same counts and verdicts, the
    same loss -- each kernel figure is within the bound of its fp64 value, and those two agree to 1e-6 (the mirrored key
    points are rounded to float32 once more)"""
    _, o64, o32, _, _ = references(case)
    _, t64, t32, _, _ = references(twin(case))
    np.testing.assert_array_equal(got["sums6"][[1, 3, 4, 5]], got_twin["sums6"][[1, 3, 4, 5]])
    np.testing.assert_array_equal(got["eval_sums6"][[1, 3, 4, 5]], got_twin["eval_sums6"][[1, 3, 4, 5]])
    np.testing.assert_array_equal(got["keep"], got_twin["keep"])
    for k in ("loss", "eval_loss"):
        assert metric(o64[k], t64[k]) <= 1e-6, k
        room = K_PRD * (max(metric(o32[k], o64[k]), FLOOR) + max(metric(t32[k], t64[k]), FLOOR)) + 1e-6
        fig = metric(got[k], got_twin[k].astype(np.float64))
        print("prd twin %s %-9s kernel %.3g  room %.3g" % (case_id(case), k, fig, room))
        assert fig <= room, (k, fig, room)


def check_linear(case, got, got_one):
    """the gradients at g_loss = g against g x the gradients at g_loss = 1.  Both launches share the forward pass and its
    roundings; only the backward's products round apart.  Yardstick: the fp32 oracle's own figure between its two runs"""
    one = dict(case, g=1.0)
    _, _, o32, _, _ = references(case)
    _, _, one32, _, _ = references(one)
    for k in NUMERIC[1:]:
        room = K_PRD * max(metric(o32[k], case["g"] * one32[k]), FLOOR)
        fig = metric(got[k], case["g"] * got_one[k].astype(np.float64))
        print("prd linear %s %-9s kernel %.3g  fp32 oracle %.3g" % (case_id(case), k, fig, room / K_PRD))
        assert fig <= room, (k, fig, room)


def run_and_check_nonfinite_eval(route):
    """the NaN and the +inf match each alone in a launch: in eval mode either direction contributes exactly `threshold`,
    in train mode the match is left out (0 / 0)"""
    inp = references(SPECIAL)[0]
    thr = np.float32(SPECIAL["thr"])
    for what in ("nan_kp", "inf_kp"):
        row = PLANT[what]
        one = {k: (v[row:row + 1].copy() if k in INPUTS[:6] else v) for k, v in inp.items()}
        got = run_fwd(route, one, SPECIAL, 1)
        np.testing.assert_array_equal(got["sums6"], np.array([thr, 1, thr, 1, 0, 1], np.float32), err_msg=what)
        assert got["loss"][0] == thr, (what, got["loss"])
        got = run_fwd(route, one, SPECIAL, 0)
        np.testing.assert_array_equal(got["sums6"], np.array([0, 0, 0, 0, 0, 1], np.float32), err_msg=what)
        assert np.isnan(got["loss"][0]) and got["n_match"][0] == 0, (what, got["loss"])


def run_and_check_empty(route):
    """m = 0 through all three entries: loss NaN, n_match 0, dK and dE zero, nothing else written (collect asserts it)"""
    case = prd_case(m=0)
    got = run(route, inputs(case), case)
    for tag in ("", "eval_"):
        assert np.isnan(got[tag + "loss"][0]) and got[tag + "n_match"][0] == 0 and not got[tag + "sums6"].any()
    assert not got["g_K"].any() and not got["g_E2"].any() and not got["workspace"].any()
    assert got["keep"].shape == (0,) and all(got[k].shape == (0, 3) for k in GRADS)


def run_twice_and_compare(route, case):
    """what one thread writes per match repeats bit for bit; the atomically summed sums6, dK, dE only under the bound"""
    inp = references(case)[0]
    a, b = run(route, inp, case), run(route, inp, case)
    same_bits(a, b, GRADS)
    np.testing.assert_array_equal(a["keep"], b["keep"])
    np.testing.assert_array_equal(a["sums6"][[1, 3, 4, 5]], b["sums6"][[1, 3, 4, 5]])
    check(case, b)
