"""Typed wrappers over the C ABI (include/scnerf_hip.h): torch CUDA(ROCm) tensors in,
kernels enqueued on torch's current stream.  No computation happens in Python and there
is no CPU fallback: a missing library or a CPU tensor raises."""
from __future__ import annotations

import os
from typing import Optional

import numpy as np
import torch

from . import _capi
from . import mlp_layout as ML

Tensor = torch.Tensor


class _Profile:
    """HIP-event timers around the heavy launches (off unless bench.py switches it on).  Events are
    recorded on torch's current stream, which is the stream the kernels are enqueued on."""

    def __init__(self):
        self.enabled = False
        self.records = {}

    def reset(self, enabled=False):
        self.records = {}
        self.enabled = enabled

    class _Region:
        def __init__(self, prof, name, flop, group):
            self.prof, self.name, self.flop, self.group = prof, name, flop, group

        def __enter__(self):
            if self.prof.enabled:
                self.e0 = torch.cuda.Event(enable_timing=True)
                self.e1 = torch.cuda.Event(enable_timing=True)
                self.e0.record()
            return self

        def __exit__(self, *exc):
            if self.prof.enabled:
                self.e1.record()
                self.prof.records.setdefault(self.name, []).append((self.e0, self.e1, self.flop, self.group))
            return False

    def region(self, name, flop=0, group=False):
        return _Profile._Region(self, name, flop, group)

    def raw_pair(self, name, flop=0):
        """two events the C side records itself (their raw handles exist once recorded here)"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        e1.record()
        self.records.setdefault(name, []).append((e0, e1, flop, False))
        return e0, e1

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, recs in self.records.items():
            ms = [a.elapsed_time(b) for a, b, _, _ in recs]
            out[name] = {"launches": len(recs), "total_ms": sum(ms), "avg_ms": sum(ms) / len(ms),
                         "flop_per_launch": sum(r[2] for r in recs) / len(recs), "group": recs[0][3]}
        return out


PROFILE = _Profile()


def _p(t: Optional[Tensor]):
    return None if t is None else t.data_ptr()


def _stream():
    return _capi.current_stream()


def _chk(t: Tensor, dtype, name):
    if not _capi.on_device(t):
        raise RuntimeError("%s must live on the GPU (scnerf_amd has no CPU path)" % name)
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    return t


def _f(t, name):
    return _chk(t, torch.float32, name)


def searchsorted(a: Tensor, v: Tensor, side: str = "right") -> Tensor:
    """Batched search with broadcast rows, int64 result (torchsearchsorted.searchsorted
    semantics, NeRF/torchsearchsorted/src/torchsearchsorted/searchsorted.py:20-53)."""
    _f(a, "a"), _f(v, "v")
    nrow = max(a.shape[0], v.shape[0])
    out = torch.empty((nrow, v.shape[1]), dtype=torch.int64, device=a.device)
    st = _capi.load().scnerf_searchsorted(_p(a), _p(v), _p(out), nrow, a.shape[0], v.shape[0],
                                          a.shape[1], v.shape[1], int(side == "left"), _stream())
    _capi.check(st, "scnerf_searchsorted")
    return out


def sample_pdf(bins: Tensor, weights: Tensor, u: Tensor, want_inds=False, want_cdf=False):
    _f(bins, "bins"), _f(weights, "weights"), _f(u, "u")
    n, nb = bins.shape
    ns = u.shape[-1]
    stride = ns if u.dim() == 2 else 0
    samples = torch.empty((n, ns), dtype=torch.float32, device=bins.device)
    inds = torch.empty((n, ns), dtype=torch.int64, device=bins.device) if want_inds else None
    cdf = torch.empty((n, nb), dtype=torch.float32, device=bins.device) if want_cdf else None
    st = _capi.load().scnerf_sample_pdf(_p(bins), _p(weights), _p(u), stride, _p(samples), _p(inds),
                                        _p(cdf), n, nb, ns, _stream())
    _capi.check(st, "scnerf_sample_pdf")
    return samples, inds, cdf


_random_state = {"shard": None, "draw": None}
_MASK64 = 0xFFFFFFFFFFFFFFFF


def random_shard(shard: Optional[int] = None) -> int:
    """Which slice of the Philox counter space this PROCESS draws from.  Ray-parallel ranks share the seed and make the
    same sequence of calls: without it ray i of every rank would get the same jitter.  Default: torch.distributed's rank
    once a process group is up (else $RANK, else 0); `random_shard(k)` pins it."""
    if shard is not None:
        _random_state["shard"] = int(shard) & 0xFFFFFFFF
    if _random_state["shard"] is not None:
        return _random_state["shard"]
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return int(dist.get_rank())
    except Exception:
        pass
    return int(os.environ.get("RANK", "0") or 0)


def next_random_call(device) -> tuple:
    """-> (seed, call) of the next render_randoms launch.  There is no hidden counter: `call` is one 63-bit draw from
    torch's DEFAULT (CPU) generator (1.4 us on the host, no device work), so torch.manual_seed(s) -- at the start or in the
    middle of a process -- reproduces everything that follows, as it does for the reference's torch.rand calls; the
    process's shard (random_shard) is folded in so that ranks draw apart.  `seed` is torch.initial_seed(); where the device
    generator was seeded on its own (torch.cuda.manual_seed, which the reference's on-device torch.rand would honour) its
    seed is mixed in."""
    seed = torch.initial_seed() & _MASK64
    if torch.device(device).type == "cuda":
        cs = torch.cuda.initial_seed() & _MASK64
        if cs != seed:
            seed = (seed * 0x9E3779B97F4A7C15 + cs) & _MASK64
    if _random_state["draw"] is None:
        _random_state["draw"] = torch.empty((), dtype=torch.int64, device="cpu")
    call = int(_random_state["draw"].random_()) ^ ((random_shard() * 0x9E3779B97F4A7C15) & _MASK64)
    return seed, call


def render_randoms(n: int, n_samples: int, n_importance: int, raw_noise_std: float, device, want_t_rand=True, want_u=True):
    """The draws of one render_rays call in ONE launch (csrc/randoms.hip; reference NeRF/render.py:252-257, :329-330,
    :425-429): -> (t_rand [n, S] | None, u [n, N_importance] | None, noise_c [n, S] | None, noise_f [n, S + N_importance] |
    None), the noises already multiplied by raw_noise_std.  Philox4x32-10, key and call id from `next_random_call`:
    reproducible from torch.manual_seed, different on every rank."""
    S, F = int(n_samples), int(n_importance)
    sizes = [n * S if want_t_rand else 0, n * F if (want_u and F > 0) else 0,
             n * S if raw_noise_std > 0 else 0, n * (S + F) if (raw_noise_std > 0 and F > 0) else 0]
    padded = [(z + 3) // 4 * 4 for z in sizes]
    buf = torch.empty(sum(padded), dtype=torch.float32, device=device)
    outs, o = [], 0
    for z, pz in zip(sizes, padded):
        outs.append(buf[o:o + z] if z else None)
        o += pz
    if sum(sizes) == 0:
        return (None, None, None, None)
    seed, call = next_random_call(device)
    st = _capi.load().scnerf_render_randoms(seed, call, _p(outs[0]), sizes[0], _p(outs[1]), sizes[1], _p(outs[2]), sizes[2],
                                            _p(outs[3]), sizes[3], float(max(raw_noise_std, 0.0)), _stream())
    _capi.check(st, "scnerf_render_randoms")
    shapes = [(n, S), (n, F), (n, S), (n, S + F)]
    return tuple(None if t is None else t.view(sh) for t, sh in zip(outs, shapes))


def coarse_sample(rays: Tensor, t_vals: Tensor, t_rand: Optional[Tensor], lindisp: bool):
    _f(rays, "rays"), _f(t_vals, "t_vals")
    n, s = rays.shape[0], t_vals.shape[0]
    if t_rand is not None:
        _f(t_rand, "t_rand")
    z = torch.empty((n, s), dtype=torch.float32, device=rays.device)
    pts = torch.empty((n, s, 3), dtype=torch.float32, device=rays.device)
    st = _capi.load().scnerf_coarse_sample(_p(rays), rays.shape[1], _p(t_vals), _p(t_rand), _p(z),
                                           _p(pts), n, s, int(bool(lindisp)), _stream())
    _capi.check(st, "scnerf_coarse_sample")
    return z, pts


def fine_sample(rays: Tensor, z_c: Tensor, w_c: Tensor, u: Tensor, want_inds=False, want_cdf=False):
    _f(rays, "rays"), _f(z_c, "z_c"), _f(w_c, "w_c"), _f(u, "u")
    n, sc = z_c.shape
    sf = u.shape[-1]
    stride = sf if u.dim() == 2 else 0
    dev = rays.device
    z_f = torch.empty((n, sc + sf), dtype=torch.float32, device=dev)
    pts_f = torch.empty((n, sc + sf, 3), dtype=torch.float32, device=dev)
    z_s = torch.empty((n, sf), dtype=torch.float32, device=dev)
    z_std = torch.empty((n,), dtype=torch.float32, device=dev)
    inds = torch.empty((n, sf), dtype=torch.int64, device=dev) if want_inds else None
    cdf = torch.empty((n, sc - 1), dtype=torch.float32, device=dev) if want_cdf else None
    st = _capi.load().scnerf_fine_sample(_p(rays), rays.shape[1], _p(z_c), _p(w_c), _p(u), stride,
                                         _p(z_f), _p(pts_f), _p(z_s), _p(z_std), _p(inds), _p(cdf),
                                         n, sc, sf, _stream())
    _capi.check(st, "scnerf_fine_sample")
    return z_f, pts_f, z_s, z_std, inds, cdf


_index_cache = {}


def _device_index(kind: str, device, pd: int = 3, remap=None) -> Tensor:
    """int32 gather table (flat parameter buffer -> streaming order) of network variant `pd` on the
    device.  `remap` = (key, int64 array [n_params]) translates the table's canonical parameter offsets
    (mlp_layout.Layout order) into the offsets of a module that registers the same tensors in another
    order (NeRF++'s MLPNet)."""
    key = (kind, str(device), pd, None if remap is None else remap[0])
    if key not in _index_cache:
        lay = ML.layout(pd)
        idx = lay.forward_index() if kind == "fwd" else lay.backward_index()
        if remap is not None:
            table = np.asarray(remap[1], dtype=np.int64)
            idx = np.where(idx >= 0, table[np.maximum(idx, 0)], -1).astype(np.int32)
        _index_cache[key] = torch.from_numpy(idx).to(device)
    return _index_cache[key]


def check_layout():
    import ctypes
    lib = _capi.load()
    for pd in (3, 4):
        lay = ML.layout(pd)
        out = np.zeros(32, np.int32)
        st = lib.scnerf_mlp_layout_info(pd, out.ctypes.data_as(ctypes.c_void_p), 32)
        _capi.check(st, "scnerf_mlp_layout_info")
        exp = [lay.fwd_stream, lay.fwd_bias, lay.fwd_bias_f, lay.fwd_bias_v, lay.fwd_bias_rgb, lay.fwd_alpha_w,
               lay.fwd_alpha_b, lay.fwd_total, lay.bwd_stream, lay.bwd_alpha_w, lay.bwd_total,
               lay.save_floats_per_sample, ML.GRAD_FLOATS_PER_SAMPLE]
        for P in (1, 128, 4097):
            if lib.scnerf_mlp_save_floats(pd, P) != lay.save_floats(P) or lib.scnerf_mlp_grad_floats(P) != ML.grad_floats(P):
                raise RuntimeError("workspace size formulas disagree between the kernels and mlp_layout.py")
        if out[:len(exp)].tolist() != exp or int(out[20]) != lay.n_params or int(out[21]) != lay.e_width:
            raise RuntimeError("kernel / mlp_layout.py constants disagree (pd=%d): %s vs %s"
                               % (pd, out[:22].tolist(), exp))


def pack_weights(flat_params: Tensor, kind: str = "fwd", out: Optional[Tensor] = None, pd: int = 3,
                 remap=None) -> Tensor:
    """flat parameter buffer (595 844 floats for pd = 3, 606 596 for pd = 4) -> packed streaming buffer."""
    _f(flat_params, "flat_params")
    lay = ML.layout(pd)
    if flat_params.numel() != lay.n_params:
        raise ValueError("expected %d parameters, got %d" % (lay.n_params, flat_params.numel()))
    idx = _device_index(kind, flat_params.device, pd, remap)
    if out is None:
        out = torch.empty(idx.numel(), dtype=torch.float32, device=flat_params.device)
    st = _capi.load().scnerf_gather_f32(_p(flat_params), _p(idx), _p(out), idx.numel(), _stream())
    _capi.check(st, "scnerf_gather_f32")
    return out


class _Switch:
    """One process-wide switch behind a public set-or-get function: `value` is preset from the environment variable
    `env` at import -- `parse(os.environ.get(env))` where the preset is not the value itself, else `default` when unset --
    and a preset outside `values` raises there; `switch(v)` sets it (`set_error` for a `v` outside `values`), `switch()`
    reads it."""

    def __init__(self, values, env, default=None, set_error=None, parse=None):
        preset = os.environ.get(env)
        self.values, self.set_error = values, set_error
        self.value = parse(preset) if parse is not None else (default if preset is None else preset)
        if self.value not in values:
            raise ValueError("%s must be one of %s, not %r" % (env, "|".join(values), self.value))

    def __call__(self, value=None):
        if value is not None:
            if value not in self.values:
                raise ValueError(self.set_error)
            self.value = value
        return self.value


def _on_off(on: Optional[bool]) -> Optional[bool]:
    return None if on is None else bool(on)


MLP_ARITHMETICS = ("fp32", "resident")
_MLP_ARITHMETIC = _Switch(MLP_ARITHMETICS, "SCNERF_MLP_ARITHMETIC", "resident",
                          "mlp_arithmetic is one of " + ", ".join(MLP_ARITHMETICS))


def mlp_arithmetic(mode: Optional[str] = None) -> str:
    """How the network runs, training and inference, forward and data gradients: "resident" (the default) -- one launch
    per pass on three fp16 products per product with the activations register-resident as cut fp16 planes
    (csrc/mlp_h3.h): the activation workspace is only written, for the weight-gradient GEMMs; "fp32" -- the fused
    kernels on the exact-fp32 MFMA (csrc/mlp_fwd.hip, mlp_bwd.hip): the numerical yardstick.
    Without an argument: the mode in force.  Environment preset: SCNERF_MLP_ARITHMETIC."""
    return _MLP_ARITHMETIC(mode)


INFERENCE_ARITHMETICS = ("same", "fast")
_INFERENCE_ARITHMETIC = _Switch(INFERENCE_ARITHMETICS, "SCNERF_INFER_ARITHMETIC", "same",
                                "inference_arithmetic is one of " + ", ".join(INFERENCE_ARITHMETICS))


def inference_arithmetic(mode: Optional[str] = None) -> str:
    """How FORWARD-ONLY network passes run (render_path, render_path_sharded, NeRF++'s render_single_image, a network query
    under torch.no_grad()): "same" (the default) -- as every other pass, ops.mlp_arithmetic; "fast" -- where that is
    "resident", on ONE fp16 product per product instead of three (csrc/mlp_fwd_h3_kernel.h, PRODUCTS == 1): operands
    rounded to fp16 after their power-of-two scale, fp32 accumulation, a third of the matrix instructions, outputs within
    fp16 rounding of the default's instead of fp32 rounding.  A call that tracks gradients runs exactly as without the
    switch, and so does every call under mlp_arithmetic("fp32").  "fast" passes take no scale-guard record.
    Without an argument: the mode in force.  Environment preset: SCNERF_INFER_ARITHMETIC."""
    return _INFERENCE_ARITHMETIC(mode)


class _FloatSwitch:
    """_Switch's sibling for a threshold: a float in [lo, hi) -- kept as the fp32 value the kernels compare with -- or off
    (None).  `switch(x)` sets it, `switch("off")` switches it off, `switch()` reads it; the preset comes from the
    environment variable `env` ("off", empty or unset: off).  Anything else raises ValueError."""

    def __init__(self, env, lo, hi, what):
        self.lo, self.hi, self.what = lo, hi, what
        preset = os.environ.get(env)
        self.value = None if preset in (None, "", "off") else self._parse(preset, env)

    def _parse(self, value, what):
        try:
            x = float(np.float32(float(value))) if not isinstance(value, bool) else None
        except (TypeError, ValueError):
            x = None
        if x is None or not (self.lo <= x < self.hi):
            raise ValueError("%s is \"off\" or a number in [%g, %g), not %r" % (what, self.lo, self.hi, value))
        return x

    def __call__(self, value=None):
        if value is not None:
            self.value = None if (isinstance(value, str) and value == "off") else self._parse(value, self.what)
        return self.value


_INFERENCE_SKIP_EMPTY = _FloatSwitch("SCNERF_INFER_SKIP_EMPTY", 0.0, 1.0, "inference_skip_empty")
_SKIP_EMPTY_STATS = {"rays": 0, "skipped": 0}


def inference_skip_empty(threshold=None) -> Optional[float]:
    """Forward-only render_rays calls skip the fine pass of the rays the coarse pass found empty: a float tau in [0, 1)
    switches it on, "off" (the default) off.  After the coarse stage of a chunk a ray with acc0 <= tau is SKIPPED (a NaN
    acc0 is not); the live rays -- their rows of the ray batch, of the coarse depths and weights and of per-ray draws -- are
    compacted, in ray order, into a shorter batch, the fine sampler, the fine network and the compositing run on that
    batch in the arithmetic and guard mode in force (the three launches, also under fused_fine_stage), and the outputs
    are expanded to the full batch: a live ray's are those of a switch-off call on the live rays alone, bit for bit; a
    skipped ray returns the coarse stage's rgb_map = rgb0, disp_map = disp0, acc_map = acc0, depth_map = depth0, z_std = 0
    and zero rows of raw, z_vals and z_samples.  What the coarse network does not see -- thin structures -- is lost on a
    skipped ray: tau is the caller's trade-off.  Honoured by a forward-only render_rays call on the fused path with
    N_importance > 0 (render_path, render_path_sharded, anything under torch.no_grad()); ignored by calls that track
    gradients, the NeRF++ node, network queries and the opaque-callable path.
    THE ONE HOST WAIT of the feature: the number of live rays sizes the fine stage's launches, so every chunk the host waits
    on an event behind the compaction kernel and reads one 4-byte word from pinned memory -- the coarse stage of a chunk has
    finished before its fine stage is enqueued (skip_empty_stats() re-uses these reads).
    Without an argument: the threshold in force, None when off.  Environment preset: SCNERF_INFER_SKIP_EMPTY."""
    return _INFERENCE_SKIP_EMPTY(threshold)


def skip_empty_stats(reset: bool = False) -> dict:
    """{"rays": rays compacted so far, "skipped": those of them skipped}: host-side sums of the counts ray_compact has
    already read (no device access); `reset` zeroes them after the read."""
    out = dict(_SKIP_EMPTY_STATS)
    if reset:
        _SKIP_EMPTY_STATS["rays"] = _SKIP_EMPTY_STATS["skipped"] = 0
    return out


def ray_compact(acc: Tensor, tau: float):
    """acc [n] (the coarse stage's acc_map), tau -> (live_idx int32 [n], slot_of int32 [n], n_live): ray i is live unless
    acc[i] <= tau; live_idx[:n_live] are the live rays ascending, slot_of[i] a live ray's position among them, -1 for a
    skipped one (csrc/ray_compact.hip).  WAITS for the launch: n_live is read from a pinned word behind an event.
    Counted in skip_empty_stats()."""
    live_idx, slot_of, n_live = _ray_compact(acc, tau)
    _SKIP_EMPTY_STATS["rays"] += acc.numel()
    _SKIP_EMPTY_STATS["skipped"] += acc.numel() - n_live
    return live_idx, slot_of, n_live


def _ray_compact(acc: Tensor, tau: float):
    """ray_compact without a counter: the launch and the one host read, shared by inference_skip_empty (ray_compact) and
    inference_skip_background (background_compact)"""
    _f(acc, "acc")
    n = acc.numel()
    both = torch.empty((2, n), dtype=torch.int32, device=acc.device)
    count = torch.empty(1, dtype=torch.int32, device=acc.device)
    # (CPU tensors: the interpreter build of the kernels under test, which runs the launch to its end)
    host = torch.empty(1, dtype=torch.int32, device="cpu", pin_memory=acc.is_cuda)
    st = _capi.load().scnerf_ray_compact(_p(acc), float(tau), _p(both[0]), _p(both[1]), _p(count), _p(host), n, _stream())
    _capi.check(st, "scnerf_ray_compact")
    if acc.is_cuda:
        ev = torch.cuda.Event()
        ev.record()
        ev.synchronize()
    n_live = int(host[0])
    return both[0], both[1], n_live


def ray_rows_gather(src: Tensor, live_idx: Tensor, n_live: int) -> Tensor:
    """src [n, w] -> [n_live, w]: the rows live_idx[:n_live]"""
    _f(src, "src"), _chk(live_idx, torch.int32, "live_idx")
    n, w = src.shape
    if not 0 <= n_live <= live_idx.numel():
        raise ValueError("n_live outside the index list")
    dst = torch.empty((n_live, w), dtype=torch.float32, device=src.device)
    st = _capi.load().scnerf_ray_rows_gather(_p(src), _p(live_idx), _p(dst), int(n_live), w, n, _stream())
    _capi.check(st, "scnerf_ray_rows_gather")
    return dst


def ray_expand(slot_of: Tensor, n_live: int, live, coarse, s_tot: int, s_fine: int):
    """live = (rgb, disp, acc, depth, z_std, raw, z_vals, z_samples) of the fine stage on the n_live live rays (None when
    there is none), coarse = (rgb0, disp0, acc0, depth0) of all n rays -> the same eight tensors for n rays: a live ray's
    row from `live`, a skipped ray's per-ray values from `coarse`, z_std = 0 and zero rows (one launch, no memset)."""
    _chk(slot_of, torch.int32, "slot_of")
    n, dev = slot_of.numel(), slot_of.device
    if live is None:
        if n_live:
            raise ValueError("live rays without their fine-stage outputs")
        live = (None,) * 8
    sizes = [m * k for m in (int(n_live), n) for k in (3, 1, 1, 1, 1, 4 * s_tot, s_tot, s_fine)][:12]
    for t_, size in zip(tuple(live) + tuple(coarse), sizes):
        if t_ is not None and _f(t_, "ray_expand input").numel() != size:
            raise ValueError("ray_expand: an input of %d floats where %d belong" % (t_.numel(), size))
    rgb, disp, acc, depth, _ = _ray_outputs(n, 0, dev, want_weights=False)
    z_std = torch.empty((n,), dtype=torch.float32, device=dev)
    raw = torch.empty((n, s_tot, 4), dtype=torch.float32, device=dev)
    z_vals = torch.empty((n, s_tot), dtype=torch.float32, device=dev)
    z_samples = torch.empty((n, s_fine), dtype=torch.float32, device=dev)
    st = _capi.load().scnerf_ray_expand(_p(slot_of), n, int(n_live), int(s_tot), int(s_fine), *[_p(t_) for t_ in live],
                                        *[_p(t_) for t_ in coarse], _p(rgb), _p(disp), _p(acc), _p(depth), _p(z_std), _p(raw),
                                        _p(z_vals), _p(z_samples), _stream())
    _capi.check(st, "scnerf_ray_expand")
    return rgb, disp, acc, depth, z_std, raw, z_vals, z_samples


# ---- NeRF++: skipping the background behind an opaque foreground (csrc/nerfpp.hip, nerfplusplus/ddp_model.py) ----------------
_INFERENCE_SKIP_BACKGROUND = _FloatSwitch("SCNERF_INFER_SKIP_BACKGROUND", 0.0, 1.0, "inference_skip_background")
_SKIP_BACKGROUND_STATS = {"rays": 0, "skipped": 0}
NPP_OUT_KEYS = ("rgb", "fg_weights", "bg_weights", "fg_rgb", "fg_depth", "bg_rgb", "bg_depth", "bg_lambda")


def inference_skip_background(eps=None) -> Optional[float]:
    """Forward-only NerfNet.forward calls (NeRF++) skip the background network of the rays whose foreground is opaque: a
    float eps in [0, 1) switches it on, "off" (the default) off.  rgb = fg_rgb + bg_lambda * bg_rgb, and bg_lambda -- the
    foreground's final transmittance -- is known after the foreground network alone: npp_fg_lambda computes it (the
    compositing kernel's own foreground sweep, bit for bit its bg_lambda), a ray with bg_lambda <= eps is SKIPPED (a NaN
    bg_lambda is not), the live rays' rows of ray_o, ray_d and bg_z are compacted in ray order, the background points and
    the background network run on n_live * sb samples in the arithmetic and guard mode in force, and
    npp_composite_fwd_skip composites with the background read through slot_of.  The call returns, bit for bit, what it
    would return had the background network answered raw_bg = 0 on every sample of the skipped rays: there bg_weights is a
    row of zeros, bg_rgb = 0, bg_depth = 0 and rgb == fg_rgb; every foreground output (fg_weights, fg_rgb, fg_depth,
    bg_lambda) is unchanged on every ray.  A live ray's eight outputs are the switch-off call's: with resident_guard "off"
    bit for bit those of the full-batch call (fp32, resident and one-product arithmetic: the forward is per-sample
    independent), with a guard mode on those of a switch-off call on the live rays alone (the background guard record
    stays sized for the dense pass).  All rays live continues on the switch-off route; none live launches neither the
    background points nor the background network.
    Error against switch off, per channel of a skipped ray: |d rgb_c| = bg_rgb_c(off) <= eps * (1 + 1e-6)^sb -- bg_rgb_c
    = bg_lambda * sum_i w_i c_i with every colour a sigmoid <= 1 and the background weights summing to at most (1 + 1e-6)^sb
    (weights so far plus the transmittance left grow by the factor 1 + 1e-6 per sample at most: DESIGN.md 4.7.5).
    In a cascade (render_single_image) every level decides by its own bg_lambda; a ray skipped at the coarse level hands
    zero bg_weights to the background sample_pdf, which then places uniform samples should the ray be live again at the
    fine level.  The foreground chain is untouched: the fine foreground depths depend on fg_weights alone.
    Honoured by a forward-only NerfNet.forward with at least one ray (render_single_image, anything under
    torch.no_grad()); a call that tracks gradients runs exactly as without the switch.  Composes with
    inference_arithmetic("fast").
    THE ONE HOST WAIT of the feature: n_live sizes the background launches, so every call waits on an event behind the
    compaction kernel and reads one 4-byte word from pinned memory (skip_background_stats() re-uses these reads;
    skip_empty_stats() never sees them).
    Without an argument: the threshold in force, None when off.  Environment preset: SCNERF_INFER_SKIP_BACKGROUND."""
    return _INFERENCE_SKIP_BACKGROUND(eps)


def skip_background_stats(reset: bool = False) -> dict:
    """{"rays": rays compacted by inference_skip_background so far, "skipped": those of them whose background was
    skipped}: host-side sums of the counts background_compact has already read (no device access); `reset` zeroes them
    after the read."""
    out = dict(_SKIP_BACKGROUND_STATS)
    if reset:
        _SKIP_BACKGROUND_STATS["rays"] = _SKIP_BACKGROUND_STATS["skipped"] = 0
    return out


def background_compact(bg_lambda: Tensor, eps: float):
    """ray_compact's launch and host read on acc = bg_lambda, tau = eps (ray i is live unless bg_lambda[i] <= eps) ->
    (live_idx, slot_of, n_live); counted in skip_background_stats(), not in skip_empty_stats()."""
    live_idx, slot_of, n_live = _ray_compact(bg_lambda, eps)
    _SKIP_BACKGROUND_STATS["rays"] += bg_lambda.numel()
    _SKIP_BACKGROUND_STATS["skipped"] += bg_lambda.numel() - n_live
    return live_idx, slot_of, n_live


def npp_fg_lambda(raw_fg: Tensor, fg_z: Tensor, fg_z_max: Tensor, ray_d: Tensor) -> Tensor:
    """raw_fg [n * sf, 4], fg_z [n, sf], fg_z_max [n], ray_d [n, 3] -> bg_lambda [n], the foreground's final transmittance:
    npp_composite_fwd's value bit for bit, without the background (csrc/nerfpp.hip)"""
    n, sf = fg_z.shape
    for t_, size, name in ((raw_fg, n * sf * 4, "raw_fg"), (fg_z, n * sf, "fg_z"), (fg_z_max, n, "fg_z_max"), (ray_d, n * 3, "ray_d")):
        if _f(t_, name).numel() != size:
            raise ValueError("npp_fg_lambda: %s holds %d floats where %d belong" % (name, t_.numel(), size))
    lam = torch.empty((n,), dtype=torch.float32, device=fg_z.device)
    st = _capi.load().scnerf_npp_fg_lambda(_p(raw_fg), _p(fg_z), _p(fg_z_max), _p(ray_d), _p(lam), n, sf, _stream())
    _capi.check(st, "scnerf_npp_fg_lambda")
    return lam


def npp_composite_fwd_skip(raw_fg: Tensor, raw_bg_live: Optional[Tensor], fg_z: Tensor, fg_z_max: Tensor, bg_z: Tensor,
                           ray_d: Tensor, slot_of: Tensor, n_live: int) -> dict:
    """NerfNet.forward's compositing with the background of the live rays only: raw_bg_live [n_live * sb, 4] (None when
    n_live == 0), slot_of [n] int32 (background_compact's) -> the eight outputs (NPP_OUT_KEYS) for all n rays, every
    element written by the one launch; a skipped ray's are those of a zero raw_bg row."""
    n, sf = fg_z.shape
    sb = bg_z.shape[-1]
    n_live = int(n_live)
    if not 0 <= n_live <= n:
        raise ValueError("n_live outside [0, n]")
    _chk(slot_of, torch.int32, "slot_of")
    sizes = [(raw_fg, n * sf * 4, "raw_fg"), (fg_z, n * sf, "fg_z"), (fg_z_max, n, "fg_z_max"), (bg_z, n * sb, "bg_z"),
             (ray_d, n * 3, "ray_d"), (slot_of, n, "slot_of")]
    if n_live or raw_bg_live is not None:
        if raw_bg_live is None:
            raise ValueError("live rays without their background outputs")
        sizes.append((raw_bg_live, n_live * sb * 4, "raw_bg_live"))
    for t_, size, name in sizes:
        if t_ is not slot_of:
            _f(t_, name)
        if t_.numel() != size:
            raise ValueError("npp_composite_fwd_skip: %s holds %d elements where %d belong" % (name, t_.numel(), size))
    shapes = {"rgb": (n, 3), "fg_weights": (n, sf), "bg_weights": (n, sb), "fg_rgb": (n, 3), "fg_depth": (n,),
              "bg_rgb": (n, 3), "bg_depth": (n,), "bg_lambda": (n,)}
    out = {k: torch.empty(shapes[k], dtype=torch.float32, device=fg_z.device) for k in NPP_OUT_KEYS}
    st = _capi.load().scnerf_npp_composite_fwd_skip(_p(raw_fg), _p(raw_bg_live) if n_live else None, _p(fg_z), _p(fg_z_max),
                                                    _p(bg_z), _p(ray_d), _p(slot_of), *[_p(out[k]) for k in NPP_OUT_KEYS], n,
                                                    n_live, sf, sb, _stream())
    _capi.check(st, "scnerf_npp_composite_fwd_skip")
    return out


# ---- skipping samples in empty space: the occupancy grid (csrc/occupancy.hip, scnerf_amd/occupancy.py) ----------------------
_INFERENCE_OCCUPANCY = [None]
_OCCUPANCY_STATS = {"samples": 0, "skipped": 0}


def inference_occupancy(grid=None):
    """Forward-only render_rays calls skip the network on the samples an occupancy grid calls empty: an
    occupancy.OccupancyGrid switches it on, "off" (the default) off.  A sample is DEAD only when its point -- the fp32 point
    the sampler wrote, in the space the network sees (after the NDC warp where there is one) -- lies inside the grid's box
    and the bit of its cell is 0; a point outside the box and a NaN coordinate are live.  The call returns, bit for bit, what it
    would return had the network answered raw = (0, 0, 0, 0) for every dead sample, in both passes; the fine sampler sees
    the coarse weights that result.  Per stage: the sampler as it is, the live samples' points and view directions
    compacted in sample order (occ_compact), mlp_fwd on that list with samples_per_ray = 1 in the arithmetic and guard mode
    in force, the result expanded with zero rows (occ_expand_raw), the unchanged compositing -- never the one-launch
    coarse or fine stage.  Honoured by a forward-only call on the fused path with n > 0 and no density noise (zero raw plus
    noise would paint fog into empty space); ignored by calls that track gradients, the NeRF++ node, network queries and
    the opaque-callable path.  Composes with inference_skip_empty(tau): the coarse stage with the grid, ray compaction by
    acc0, the fine stage with the grid on the live rays.  A grid baked from networks checks them (OccupancyStaleError when
    the weights have changed); a grid on another device than the rays is a ValueError.
    ONE HOST WAIT PER STAGE AND CHUNK: the number of live samples sizes the network launch, so the host waits on an event
    behind the compaction and reads one 4-byte word from pinned memory, exactly as ray_compact does
    (occupancy_stats() re-uses these reads).
    Without an argument: the grid in force, None when off.  No environment preset: a grid is not a string."""
    if grid is not None:
        if isinstance(grid, str) and grid == "off":
            _INFERENCE_OCCUPANCY[0] = None
        else:
            from .occupancy import OccupancyGrid
            if not isinstance(grid, OccupancyGrid):
                raise ValueError("inference_occupancy is \"off\" or an OccupancyGrid, not %r" % (grid,))
            if grid.space != "euclidean":
                raise ValueError("inference_occupancy takes a euclidean grid; an inverted-sphere grid belongs to the "
                                 "background slot of inference_occupancy_nerfpp")
            _INFERENCE_OCCUPANCY[0] = grid
    return _INFERENCE_OCCUPANCY[0]


_INFERENCE_OCCUPANCY_NERFPP = [None]
_OCCUPANCY_NERFPP_STATS = {"fg_samples": 0, "fg_skipped": 0, "bg_samples": 0, "bg_skipped": 0}


def inference_occupancy_nerfpp(fg=None, bg=None):
    """Forward-only NerfNet.forward calls (NeRF++: render_single_image, anything under torch.no_grad()) skip both networks
    on the samples a baked grid calls empty: `fg`, a euclidean occupancy.OccupancyGrid over the foreground network (its
    samples o + z d lie in the unit sphere: the natural box is [-1, 1]^3), and `bg`, an inverted-sphere grid over the
    background network, switch it on -- either may be None --, "off" (the default) off.  occupancy.bake_nerfpp bakes both.
    A foreground sample is dead by inference_occupancy's cell test.  A background sample (x', y', z', w = 1 / r) is DEAD only
    when q = (x' w, y' w, z' w) -- one fp32 multiplication per axis, the bijection of the outside of the unit sphere onto the
    unit ball -- lies inside the grid's box and the bit of its cell is 0; a q outside the box and a NaN component are live.
    The call returns, bit for bit, what it would return had the network answered raw = (0, 0, 0, 0) for every dead sample;
    the live samples keep their bits in the fp32, resident and one-product arithmetics, and each cascade level's sampler
    sees the weights that result.  Per network with a grid: the points kernel as it is, the live samples compacted in sample
    order (occ_compact / occ_compact4), mlp_fwd on that list with samples_per_ray = 1 in the arithmetic and guard mode in
    force (the guard record stays the dense pass's), the result expanded with zero rows (occ_expand_raw), the unchanged
    compositing.  All samples live goes the same way; none live launches no network.  Composes with
    inference_skip_background(eps): the foreground under its grid, bg_lambda from the expanded raw, ray compaction, the
    background points of the live rays, the background grid on them.  A call that tracks gradients never sees the switch.
    A grid baked from networks checks them (OccupancyStaleError); a grid on another device than the rays, and a grid of the
    wrong space in either slot, is a ValueError.  inference_occupancy's grid stays ignored by the NeRF++ node.
    ONE HOST WAIT PER NETWORK WITH A GRID AND CALL: the count sizes the network launch (occupancy_nerfpp_stats() re-uses
    these reads; occupancy_stats() never sees them).
    Without arguments: (fg, bg) in force, None when off.  No environment preset: a grid is not a string."""
    if fg is None and bg is None:
        return _INFERENCE_OCCUPANCY_NERFPP[0]
    if isinstance(fg, str) and fg == "off" and bg is None:
        _INFERENCE_OCCUPANCY_NERFPP[0] = None
        return None
    from .occupancy import OccupancyGrid
    for grid, space, slot in ((fg, "euclidean", "fg"), (bg, "inverted_sphere", "bg")):
        if grid is None:
            continue
        if not isinstance(grid, OccupancyGrid):
            raise ValueError("inference_occupancy_nerfpp: %s is an OccupancyGrid or None, not %r" % (slot, grid))
        if grid.space != space:
            raise ValueError("inference_occupancy_nerfpp: the %s grid lies in the %s space, not in the %s space"
                             % (slot, space, grid.space))
    _INFERENCE_OCCUPANCY_NERFPP[0] = (fg, bg)
    return _INFERENCE_OCCUPANCY_NERFPP[0]


def occupancy_nerfpp_stats(reset: bool = False) -> dict:
    """{"fg_samples", "fg_skipped", "bg_samples", "bg_skipped"}: the samples inference_occupancy_nerfpp compacted so far per
    network and those of them dead -- host-side sums of the counts already read (no device access); `reset` zeroes them
    after the read."""
    out = dict(_OCCUPANCY_NERFPP_STATS)
    if reset:
        for k in _OCCUPANCY_NERFPP_STATS:
            _OCCUPANCY_NERFPP_STATS[k] = 0
    return out


def nerfpp_network_under_grid(which: str, grid, pts: Tensor, viewdirs: Tensor, samples_per_ray: int, wf: Tensor, planes,
                              guard=None) -> Tensor:
    """The network `which` ("fg": pts [P, 3], "bg": pts [P, 4]) of a forward-only NeRF++ call under its grid -> raw [P, 4]:
    compaction (one host read), mlp_fwd on the live samples with one view direction each, expansion with zero rows.
    Counted in occupancy_nerfpp_stats()."""
    pd = 3 if which == "fg" else 4
    _, slot_of, pts_l, vd_l, n_live = _occ_compact(pts, viewdirs, samples_per_ray, grid, pd)
    P = pts.numel() // pd
    _OCCUPANCY_NERFPP_STATS[which + "_samples"] += P
    _OCCUPANCY_NERFPP_STATS[which + "_skipped"] += P - n_live
    raw_l = mlp_fwd(pts_l, vd_l, 1, wf, None, pd=pd, planes=planes, guard=guard) if n_live > 0 else None
    return occ_expand_raw(raw_l, slot_of, n_live)


def occupancy_stats(reset: bool = False) -> dict:
    """{"samples": samples compacted so far, "skipped": those of them dead}: host-side sums of the counts occ_compact has
    already read (no device access); `reset` zeroes them after the read."""
    out = dict(_OCCUPANCY_STATS)
    if reset:
        _OCCUPANCY_STATS["samples"] = _OCCUPANCY_STATS["skipped"] = 0
    return out


def _occ_resolution(bits: Tensor, R: int) -> int:
    _chk(bits, torch.int32, "bits")
    R = int(R)
    if R < 32 or R % 32 or bits.numel() != R * R * R // 32:
        raise ValueError("an occupancy grid of resolution %d holds %d words, not %d" % (R, R * R * R // 32, bits.numel()))
    return R


def occ_compact(pts: Tensor, viewdirs: Tensor, samples_per_ray: int, grid):
    """pts [P, 3] (sample i belongs to ray i // samples_per_ray), viewdirs [n, 3], grid (bits int32 [R^3 / 32], R, lo, inv)
    -> (live_idx int32 [P], slot_of int32 [P], pts_live [n_live, 3], vd_live [n_live, 3], n_live): the samples the grid does
    not call dead, ascending; slot_of[i] a live sample's position among them, -1 for a dead one (csrc/occupancy.hip).
    WAITS for the launch: n_live is read from a pinned word behind an event.  Counted in occupancy_stats()."""
    if getattr(grid, "space", "euclidean") != "euclidean":
        raise ValueError("occ_compact takes a euclidean grid; an inverted-sphere grid belongs to occ_compact4")
    out = _occ_compact(pts, viewdirs, samples_per_ray, grid, 3)
    _OCCUPANCY_STATS["samples"] += pts.numel() // 3
    _OCCUPANCY_STATS["skipped"] += pts.numel() // 3 - out[4]
    return out


def occ_compact4(pts: Tensor, viewdirs: Tensor, samples_per_ray: int, grid):
    """occ_compact for the samples of a NeRF++ background network: pts [P, 4] = (x', y', z', w), grid an inverted-sphere
    grid over a box in q = (x' w, y' w, z' w) -> (live_idx, slot_of, pts_live [n_live, 4], vd_live [n_live, 3], n_live)
    (csrc/npp_occupancy.hip).  WAITS for the launch as occ_compact does; counted in no statistic."""
    if getattr(grid, "space", "euclidean") != "inverted_sphere":
        raise ValueError("occ_compact4 takes an inverted-sphere grid")
    return _occ_compact(pts, viewdirs, samples_per_ray, grid, 4)


def _occ_compact(pts: Tensor, viewdirs: Tensor, samples_per_ray: int, grid, pd: int):
    """occ_compact (pd = 3) and occ_compact4 (pd = 4) without a counter: the launch and the one host read, shared by
    inference_occupancy and inference_occupancy_nerfpp"""
    _f(pts, "pts")
    R = _occ_resolution(grid.bits, grid.resolution)
    if grid.bits.device != pts.device:
        raise ValueError("the occupancy grid lives on %s, the samples on %s" % (grid.bits.device, pts.device))
    P = pts.numel() // pd
    dev = pts.device
    vptr, vstride = _vd(viewdirs) if P > 0 else (None, 3)
    lib = _capi.load()
    name = "scnerf_occ_compact" if pd == 3 else "scnerf_occ_compact4"
    ints = torch.empty((2, P), dtype=torch.int32, device=dev)
    rows_p = torch.empty((P, pd), dtype=torch.float32, device=dev)
    rows_v = torch.empty((P, 3), dtype=torch.float32, device=dev)
    ws = torch.empty(int(getattr(lib, name + "_workspace_ints")(P)) + 1, dtype=torch.int32, device=dev)
    # (CPU tensors: the interpreter build of the kernels under test, which runs the launch to its end)
    host = torch.empty(1, dtype=torch.int32, device="cpu", pin_memory=pts.is_cuda)
    st = getattr(lib, name)(_p(pts) if P else None, P, vptr, vstride, int(samples_per_ray), _p(grid.bits), R, *grid.lo,
                            *grid.inv, _p(ws[1:]), _p(ints[0]) if P else None, _p(ints[1]) if P else None,
                            _p(rows_p) if P else None, _p(rows_v) if P else None, _p(ws[:1]), _p(host), _stream())
    _capi.check(st, name)
    if pts.is_cuda:
        ev = torch.cuda.Event()
        ev.record()
        ev.synchronize()
    n_live = int(host[0])
    return ints[0], ints[1], rows_p[:n_live], rows_v[:n_live], n_live


def occ_expand_raw(raw_live: Optional[Tensor], slot_of: Tensor, n_live: int) -> Tensor:
    """raw_live [n_live, 4] (None when there is none), slot_of [P] -> raw [P, 4]: row slot_of[i] of raw_live, a zero row for
    a dead sample (one launch, every row written, no memset)."""
    _chk(slot_of, torch.int32, "slot_of")
    P = slot_of.numel()
    n_live = int(n_live)
    if n_live and (raw_live is None or _f(raw_live, "raw_live").numel() != 4 * n_live):
        raise ValueError("occ_expand_raw: %d live samples without their [n_live, 4] outputs" % n_live)
    raw = torch.empty((P, 4), dtype=torch.float32, device=slot_of.device)
    st = _capi.load().scnerf_occ_expand_raw(_p(raw_live) if n_live else None, _p(slot_of) if P else None, _p(raw) if P else None,
                                            P, n_live, _stream())
    _capi.check(st, "scnerf_occ_expand_raw")
    return raw


def occ_probe_points(first_cell: int, n_cells: int, R: int, k: int, lo, cell, device) -> Tensor:
    """The k^3 lattice points of cells [first_cell, first_cell + n_cells) of an R^3 grid -> pts [n_cells k^3, 3]; lo and
    cell = (hi - lo) / R: three fp32 numbers each.  p = lo + (i + (j + 0.5) / k) * cell, rounded after every operation."""
    k = int(k)
    if k not in (1, 2, 3):
        raise ValueError("probes is 1, 2 or 3")
    offs = [float(np.float32(np.float32(j + 0.5) / np.float32(k))) if j < k else 0.0 for j in range(3)]
    pts = torch.empty((int(n_cells) * k ** 3, 3), dtype=torch.float32, device=device)
    st = _capi.load().scnerf_occ_probe_points(int(first_cell), int(n_cells), int(R), k, *lo, *cell, *offs, _p(pts), _stream())
    _capi.check(st, "scnerf_occ_probe_points")
    return pts


def occ_probe_points_inverted(first_cell: int, n_cells: int, R: int, k: int, lo, cell, device) -> Tensor:
    """occ_probe_points for an inverted-sphere grid -> pts [n_cells k^3, 4]: the lattice point q of every probe becomes
    (q / r, min(r, 1)) with r = sqrt(((qx qx) + (qy qy)) + (qz qz)), every operation fp32 and correctly rounded; r == 0
    gives (0, 0, 1, 0) (csrc/npp_occupancy.hip)."""
    k = int(k)
    if k not in (1, 2, 3):
        raise ValueError("probes is 1, 2 or 3")
    offs = [float(np.float32(np.float32(j + 0.5) / np.float32(k))) if j < k else 0.0 for j in range(3)]
    pts = torch.empty((int(n_cells) * k ** 3, 4), dtype=torch.float32, device=device)
    st = _capi.load().scnerf_occ_probe_points_inverted(int(first_cell), int(n_cells), int(R), k, *lo, *cell, *offs, _p(pts),
                                                       _stream())
    _capi.check(st, "scnerf_occ_probe_points_inverted")
    return pts


def occ_accumulate(raw: Tensor, sigma_min: float, first_cell: int, n_cells: int, R: int, k: int, bits: Tensor) -> None:
    """raw [n_cells k^3, 4] of occ_probe_points' points: bits |= "a probe of the cell has !(sigma <= sigma_min)" (a NaN
    density sets the cell), in place."""
    R = _occ_resolution(bits, R)
    if _f(raw, "raw").numel() != 4 * int(n_cells) * int(k) ** 3:
        raise ValueError("occ_accumulate: raw does not hold four floats per probe point")
    st = _capi.load().scnerf_occ_accumulate(_p(raw), float(sigma_min), int(first_cell), int(n_cells), R, int(k), _p(bits), _stream())
    _capi.check(st, "scnerf_occ_accumulate")


def occ_dilate(bits: Tensor, R: int) -> Tensor:
    """one round of 26-neighbourhood dilation of an R^3 grid's words -> new words"""
    R = _occ_resolution(bits, R)
    out = torch.empty_like(bits)
    _capi.check(_capi.load().scnerf_occ_dilate(_p(bits), _p(out), R, _stream()), "scnerf_occ_dilate")
    return out


# ---- stopping rays once they are opaque: early ray termination (csrc/early_stop.hip) -----------------------------------------
EARLY_STOP_SEGMENTS = (2, 8)                   # K, inclusive
EARLY_STOP_DEFAULT_SEGMENTS = 4


class _EarlyStopSwitch:
    """_FloatSwitch's sibling for a pair: (eps, K) -- eps a float in (0, 1), the double the kernels compare with, K the
    number of depth segments in 2 .. 8 -- or off (None).  The preset comes from the environment variable `env`: "off" (or
    empty, unset), "eps" or "eps:segments".  Anything else raises ValueError."""

    def __init__(self, env, what):
        self.what = what
        preset = os.environ.get(env)
        self.value = None
        if preset not in (None, "", "off"):
            eps, _, segments = preset.partition(":")
            self.value = self._parse(eps, self._int(segments, env) if segments or ":" in preset else None, env)

    @staticmethod
    def _int(text, what):
        try:
            return int(text)
        except ValueError:
            raise ValueError("%s is \"off\", eps or eps:segments, not %r" % (what, text)) from None

    def _parse(self, eps, segments, what):
        try:
            x = float(eps) if not isinstance(eps, bool) else None
        except (TypeError, ValueError):
            x = None
        if x is None or not (0.0 < x < 1.0):
            raise ValueError("%s: eps is \"off\" or a number in (0, 1), not %r" % (what, eps))
        k = EARLY_STOP_DEFAULT_SEGMENTS if segments is None else segments
        lo, hi = EARLY_STOP_SEGMENTS
        if isinstance(k, bool) or not isinstance(k, int) or not (lo <= k <= hi):
            raise ValueError("%s: segments is an integer in %d .. %d, not %r" % (what, lo, hi, segments))
        return x, k

    def __call__(self, eps=None, segments=None):
        if eps is None:
            if segments is not None:
                raise ValueError("%s: segments go with an eps" % self.what)
        elif isinstance(eps, str) and eps == "off":
            self.value = None
        else:
            self.value = self._parse(eps, segments, self.what)
        return self.value


_INFERENCE_EARLY_STOP = _EarlyStopSwitch("SCNERF_INFER_EARLY_STOP", "inference_early_stop")
_EARLY_STOP_STATS = {"samples": 0, "skipped": 0, "rays": 0, "stopped": 0}
_EARLY_STOP_LAST = [None]


def inference_early_stop(eps=None, segments=None):
    """Forward-only render_rays calls stop a ray once it is opaque: a float eps in (0, 1) switches it on, with `segments`
    = K in 2 .. 8 depth segments (4 when not given), "off" (the default) off.  The network of the call's FINAL stage -- the
    fine stage, or the coarse stage when N_importance == 0; S samples per ray, K <= S -- runs front to back in K passes:
    segment k holds the sample indices [b_k, b_k+1), b_k = (k S) // K.  After segment k the ray's transmittance T is the
    product of q_i over i < b_k+1, q exactly the compositing's (ray::sample_terms, noise 0), multiplied in fp64; a ray
    with T <= eps is STOPPED (a NaN T is not), and its samples in all later segments do not reach the network.  The call
    returns, bit for bit in all twelve outputs, what it would return had the network answered raw = (0, 0, 0, 0) for every
    skipped sample: raw carries those zero rows, the compositing is unchanged.  Colours lie in [0, 1] and the skipped weights
    sum to at most T, so every rgb_map channel and acc_map move by at most eps (in exact arithmetic), with and without
    white_bkgd.  With N_importance > 0 the coarse stage is never touched: its weights feed the sampler.
    Honoured by a forward-only call on the fused path with n > 0 and no density noise; ignored by calls that track gradients,
    the NeRF++ node, network queries and the opaque-callable path.  Composes with inference_skip_empty (ray compaction
    first, the segments on the live rays), inference_occupancy (a sample runs only if the grid calls it live AND its ray is
    alive), inference_arithmetic("fast") and resident_guard (one record per segment pass, "fine/0" .. "fine/K-1").
    HOST WAITS: every pass but the first (every pass, with a grid) sizes its network launch by a count the host reads from
    pinned memory behind an event (early_stop_stats() re-uses these reads).
    Without an argument: (eps, K) in force, None when off.  Environment preset: SCNERF_INFER_EARLY_STOP = off | eps |
    eps:segments."""
    return _INFERENCE_EARLY_STOP(eps, segments)


def early_stop_stats(reset: bool = False) -> dict:
    """{"samples": samples of the final stages run in segments so far, "skipped": those of them that did not reach the
    network (with an occupancy grid: for either reason), "rays": their rays, "stopped": those of them stopped before the
    last segment}: host-side sums of the counts seg_compact has already read (no device access); `reset` zeroes them after
    the read."""
    out = dict(_EARLY_STOP_STATS)
    if reset:
        for k in _EARLY_STOP_STATS:
            _EARLY_STOP_STATS[k] = 0
    return out


def early_stop_last() -> Optional[Tensor]:
    """stop_segment int32 [n] of the latest stage run in segments (the first segment not run, K for a ray that ran them all;
    with inference_skip_empty: of the live rays), None before the first; a device tensor, nothing waits here"""
    return _EARLY_STOP_LAST[0]


def segment_bounds(samples_per_ray: int, segments: int) -> list:
    """b_0 .. b_K of the K depth segments of a stage of S samples: b_k = (k S) // K"""
    S, K = int(samples_per_ray), int(segments)
    if not EARLY_STOP_SEGMENTS[0] <= K <= EARLY_STOP_SEGMENTS[1] or K > S:
        raise ValueError("%d depth segments for %d samples per ray: segments in 2 .. 8 and at most the samples" % (K, S))
    return [(k * S) // K for k in range(K + 1)]


def seg_compact(pts: Tensor, viewdirs: Tensor, samples_per_ray: int, first: int, length: int, alive: Optional[Tensor] = None,
                grid=None, read: bool = True):
    """pts [n S, 3], viewdirs [n, 3]; the samples [first, first + length) of every ray whose ray is alive (alive int32 [n],
    None: every ray) and which `grid` (an OccupancyGrid or None) does not call dead -> (live_idx int32 [n length] -- dense
    sample indices, ascending --, slot_of int32 [n length] by segment element, pts_live [n_live, 3], vd_live [n_live, 3],
    n_live, alive rays) (csrc/early_stop.hip).  `read`: WAITS for the launch and reads the two counts from pinned words
    behind an event; False -- for a pass without flags and grid, whose counts the host knows -- waits for nothing."""
    _f(pts, "pts")
    S, first, length = int(samples_per_ray), int(first), int(length)
    n = pts.numel() // (3 * S)
    if pts.numel() != 3 * S * n or not (0 <= first and 1 <= length <= S - first):
        raise ValueError("seg_compact: samples [%d, %d) of %d per ray, %d points" % (first, first + length, S, pts.numel() // 3))
    dev = pts.device
    if alive is not None and _chk(alive, torch.int32, "alive").numel() != n:
        raise ValueError("seg_compact: one alive flag per ray")
    if not read and (alive is not None or grid is not None):
        raise ValueError("seg_compact: only a pass without flags and grid knows its counts")
    bits, R, box = None, 0, (0.0,) * 6
    if grid is not None:
        R = _occ_resolution(grid.bits, grid.resolution)
        if grid.bits.device != dev:
            raise ValueError("the occupancy grid lives on %s, the samples on %s" % (grid.bits.device, dev))
        bits, box = grid.bits, tuple(grid.lo) + tuple(grid.inv)
    E = n * length
    vptr, vstride = _vd(viewdirs) if n > 0 else (None, 3)
    lib = _capi.load()
    ints = torch.empty((2, E), dtype=torch.int32, device=dev)
    rows = torch.empty((2, E, 3), dtype=torch.float32, device=dev)
    ws = torch.empty(int(lib.scnerf_seg_compact_workspace_ints(E)) + 2, dtype=torch.int32, device=dev)
    # (CPU tensors: the interpreter build of the kernels under test, which runs the launch to its end)
    host = torch.empty(2, dtype=torch.int32, device="cpu", pin_memory=pts.is_cuda) if read else None
    st = lib.scnerf_seg_compact(_p(pts) if n else None, n, S, first, length, _p(alive), vptr, vstride, _p(bits), R, *box,
                                _p(ws[2:]), _p(ints[0]) if E else None, _p(ints[1]) if E else None, _p(rows[0]) if E else None,
                                _p(rows[1]) if E else None, _p(ws[:2]), _p(host), _stream())
    _capi.check(st, "scnerf_seg_compact")
    if read:
        if pts.is_cuda:
            ev = torch.cuda.Event()
            ev.record()
            ev.synchronize()
        n_live, n_rays = int(host[0]), int(host[1])
    else:
        n_live, n_rays = E, n
    return ints[0], ints[1], rows[0, :n_live], rows[1, :n_live], n_live, n_rays


def seg_expand_raw(raw_live: Optional[Tensor], slot_of: Tensor, raw: Tensor, samples_per_ray: int, first: int, length: int,
                   n_live: int) -> Tensor:
    """raw_live [n_live, 4] (None when there is none), slot_of [n length] -> the rows [first, first + length) of every ray of
    the dense raw [n, S, 4], in place: row slot_of[e] of raw_live, a zero row for a sample that did not run (one launch,
    every row of the segment written, none outside it)."""
    _chk(slot_of, torch.int32, "slot_of"), _f(raw, "raw")
    S, first, length, n_live = int(samples_per_ray), int(first), int(length), int(n_live)
    n = raw.numel() // (4 * S)
    if raw.numel() != 4 * S * n or slot_of.numel() != n * length or slot_of.device != raw.device:
        raise ValueError("seg_expand_raw: raw [n, %d, 4] and one slot per sample of the segment" % S)
    if n_live and (raw_live is None or _f(raw_live, "raw_live").numel() != 4 * n_live):
        raise ValueError("seg_expand_raw: %d live samples without their [n_live, 4] outputs" % n_live)
    st = _capi.load().scnerf_seg_expand_raw(_p(raw_live) if n_live else None, _p(slot_of) if n else None, _p(raw) if n else None,
                                            n, S, first, length, n_live, _stream())
    _capi.check(st, "scnerf_seg_expand_raw")
    return raw


class StopState:
    """What the segments of one stage carry from pass to pass: T float64 [n], alive int32 [n], stop_segment int32 [n]
    (csrc/early_stop.hip); segment 0 writes all three, so nothing is filled here."""
    __slots__ = ("T", "alive", "stop_segment")

    def __init__(self, n: int, device):
        self.T = torch.empty((n,), dtype=torch.float64, device=device)
        both = torch.empty((2, n), dtype=torch.int32, device=device)
        self.alive, self.stop_segment = both[0], both[1]


def seg_transmittance(raw: Tensor, z: Tensor, rays: Tensor, first: int, length: int, k: int, segments: int, eps: float,
                      state: StopState) -> None:
    """The transmittance behind segment k = samples [first, first + length) of every ray, from the dense raw [n, S, 4], the
    depths z [n, S] and the ray batch: state.T *= prod q (fp64), state.alive = !(T <= eps), state.stop_segment = k + 1
    where a ray stops; k == 0 starts every ray at T = 1 and writes all three arrays, a later k leaves stopped rays as they
    are (one launch, one wave per ray)."""
    _f(raw, "raw"), _f(z, "z"), _f(rays, "rays")
    n, S = z.shape
    if raw.numel() != 4 * n * S or rays.shape[0] != n or state.T.numel() != n:
        raise ValueError("seg_transmittance: raw [n, S, 4], z [n, S], rays [n, .] and the state of n rays")
    st = _capi.load().scnerf_seg_transmittance(_p(raw), _p(z), _p(rays), int(rays.stride(0)), n, S, int(first), int(length),
                                               int(k), int(segments), float(eps), _p(state.T), _p(state.alive),
                                               _p(state.stop_segment), _stream())
    _capi.check(st, "scnerf_seg_transmittance")


def early_stop_count(n: int, samples_per_ray: int, ran: int, alive_last: int, stop_segment: Tensor) -> None:
    """one stage run in segments enters early_stop_stats(): `ran` of its n S samples reached the network, `alive_last` of
    its rays were alive in the last segment"""
    _EARLY_STOP_STATS["samples"] += n * samples_per_ray
    _EARLY_STOP_STATS["skipped"] += n * samples_per_ray - ran
    _EARLY_STOP_STATS["rays"] += n
    _EARLY_STOP_STATS["stopped"] += n - alive_last
    _EARLY_STOP_LAST[0] = stop_segment


RESIDENT_GUARDS = ("off", "fallback", "report", "strict")
# Off by default: on the headline step the fallback mode costs 1.4 - 1.5 % (medians of alternating runs in both orders,
# profiles/r07_resident_guard.txt) -- over the half per cent a default may cost.
_RESIDENT_GUARD = _Switch(RESIDENT_GUARDS, "SCNERF_RESIDENT_GUARD", "off",
                          "resident_guard is one of " + ", ".join(RESIDENT_GUARDS))


def resident_guard(mode: Optional[str] = None) -> str:
    """The run-time check of the resident arithmetic's per-sample scales (csrc/resident_guard.h): every layer output
    cut at a bound-derived scale S is checked for m = exponent(max|z|) + exponent(S) in [-3, 13), where the cut is fp32
    grade.  "fallback" -- the resident kernels flag the 128-sample blocks holding a sample outside, and the
    exact-fp32 kernels run those blocks again on the device (gated launches, no host synchronisation): a flagged block's
    outputs are the fp32 arithmetic's bit for bit, every other block's are unchanged; "report" -- the same, plus per-layer
    minimum margins and trip counts (resident_margins()); "strict" -- the margins, and a pass with a tripped sample raises
    ResidentRangeError instead of running again (one host read per pass: for debugging); "off" (the default) -- the
    launches without the check.  Without an argument: the mode in force.  Environment preset: SCNERF_RESIDENT_GUARD."""
    return _RESIDENT_GUARD(mode)


class ResidentRangeError(RuntimeError):
    """A resident pass cut a layer output at a scale outside the range where the arithmetic is fp32 grade."""


GUARD_LAYERS = tuple("layer_%d" % l for l in range(8)) + ("feature", "views")
GUARD_SLOTS, GUARD_BIAS, GUARD_RANGE = 64, 256, (-3, 13)         # csrc/resident_guard.h
GUARD_REPORT_FLOATS = len(GUARD_LAYERS) * (GUARD_SLOTS + 2)
_GUARD_LAST = {}


class GuardRecord:
    """What one guarded resident launch leaves (csrc/resident_guard.h): int flags [ceil(P / 128)], the `any` word and, in
    "report" / "strict", the report (per layer the largest 256 - m over 64 slots, then the samples under / over).  Views
    of the one buffer guard_records() allocates; read only when asked."""
    __slots__ = ("name", "blocks", "flags", "any", "report", "mode")

    def __init__(self, name, blocks, flags, any_, report, mode):
        self.name, self.blocks, self.flags, self.any, self.report, self.mode = name, blocks, flags, any_, report, mode

    @property
    def rerun(self) -> bool:
        return self.mode in ("fallback", "report")

    def args(self):
        return _p(self.flags) if self.blocks else _p(self.any), _p(self.any), _p(self.report)

    def margins(self) -> dict:
        """{"reran_blocks": n, "blocks": N} and, with a report, {layer: {"min_log2": m or None (no live sample),
        "under": k, "over": k}}"""
        out = {"reran_blocks": int((self.flags != 0).sum()) if self.rerun else 0, "blocks": self.blocks}
        if self.report is not None:
            rep = self.report.cpu()
            nl = len(GUARD_LAYERS)
            best = rep[:nl * GUARD_SLOTS].view(nl, GUARD_SLOTS).max(1)[0]
            counts = rep[nl * GUARD_SLOTS:].view(nl, 2)
            for i, name in enumerate(GUARD_LAYERS):
                out[name] = {"min_log2": GUARD_BIAS - int(best[i]) if best[i] > 0 else None,
                             "under": int(counts[i, 0]), "over": int(counts[i, 1])}
        return out

    def raise_if_tripped(self):
        if int(self.any.item()) == 0:
            return
        m = self.margins()
        lo, hi = GUARD_RANGE
        bad = [(n, m[n]) for n in GUARD_LAYERS if m[n]["under"] or m[n]["over"]]
        raise ResidentRangeError("resident pass %r: %s outside [%d, %d) (%d of %d blocks)" % (
            self.name, ", ".join("%s at min_log2 %s (%d under, %d over)" % (n, r["min_log2"], r["under"], r["over"]) for n, r in bad),
            lo, hi, int((self.flags != 0).sum()), m["blocks"]))


def guard_records(device, passes, fast: bool = False) -> dict:
    """Records for the network passes of one call in the guard mode in force, carved from ONE zero-filled buffer:
    passes = [(name, P), ...] -> {name: forward record, name + "_bwd": data-gradient record} ({} when "off", and for a
    call whose passes run on the one-product arithmetic -- `fast`, ResidentWeights.fast: the guard does not apply to
    them, and what earlier launches of these passes left no longer shows in resident_margins()).  The
    data-gradient record shares its pass's block flags: a block the forward ran again in fp32 runs again in the data
    gradients too.  resident_margins() reads the latest launched record of every pass."""
    mode = _RESIDENT_GUARD.value
    if fast:
        for name, _ in passes:
            _GUARD_LAST.pop(name, None)
            _GUARD_LAST.pop(name + "_bwd", None)
        return {}
    if mode == "off":
        return {}
    rep = GUARD_REPORT_FLOATS if mode in ("report", "strict") else 0
    layout, total = [], 0
    for name, P in passes:
        nb = (int(P) + 127) // 128
        layout.append((name, nb, total))
        total += nb + 2 + 2 * rep
    buf = torch.zeros(total, dtype=torch.float32, device=device)
    ints = buf.view(torch.int32)
    out = {}
    for name, nb, o in layout:
        flags = ints[o:o + nb]
        r = o + nb + 2
        out[name] = GuardRecord(name, nb, flags, ints[o + nb:o + nb + 1], buf[r:r + rep] if rep else None, mode)
        out[name + "_bwd"] = GuardRecord(name + "_bwd", nb, flags, ints[o + nb + 1:o + nb + 2],
                                         buf[r + rep:r + 2 * rep] if rep else None, mode)
    return out


def resident_margins() -> dict:
    """{pass: GuardRecord.margins()} of the latest guarded launch of every pass (reads the device)."""
    return {name: rec.margins() for name, rec in _GUARD_LAST.items()}


def _guard_args(guard: Optional[GuardRecord]):
    """the three guard arguments of a resident launch (csrc/resident_guard.h): the record's, or three nulls -- no check"""
    return guard.args() if guard is not None else (None, None, None)


def _guard_after(guard: Optional[GuardRecord], rerun):
    """after a guarded resident launch: strict -- raise on a trip; fallback / report -- rerun(flags, max_workgroups)
    enqueues the gated exact-fp32 launch"""
    if guard is None:
        return
    _GUARD_LAST[guard.name] = guard
    if guard.mode == "strict":
        guard.raise_if_tripped()
    elif guard.rerun and guard.blocks:
        rerun(_p(guard.flags), 0)


def pack_for_arithmetic(flat_params: Tensor, train: bool, pd: int = 3, remap=None):
    """What mlp_fwd / coarse_stage_fwd / mlp_bwd take as `planes` in the arithmetic in force: the ResidentWeights
    ("resident") or None ("fp32": the fused fp32-MFMA kernels read the packed fp32 tables only)."""
    if _MLP_ARITHMETIC.value == "resident":
        return pack_resident(flat_params, pd, remap=remap)
    return None


_PACK_CACHE = _Switch((False, True), "SCNERF_PACK_CACHE", parse=lambda preset: preset != "0")
PACK_CACHE_STATS = {"hits": 0, "packs": 0}


def weight_pack_cache(on: Optional[bool] = None) -> bool:
    """Inference keeps the packed weights of a network between calls (a version-keyed cache):
    render_path renders an image in ~24 chunks of rays with the SAME weights, and re-packing per chunk was 2 x 5 launches
    of nothing.  The key is everything autograd knows about the weights' identity: the flat buffer's address and version
    and every parameter's version (in-place optimizer steps, load_state_dict and FusedAdam.step all bump them).  Writes
    that by-pass version counting (`p.data.mul_(...)`) are invisible to it -- switch the cache off around them
    (`weight_pack_cache(False)`, SCNERF_PACK_CACHE=0) or call `forget_packs(net)`.  Training never uses it."""
    return _PACK_CACHE(_on_off(on))


def forget_packs(net) -> None:
    if hasattr(net, "_infer_packs"):
        net._infer_packs = None


def inference_packs(net, flat_params: Tensor, pd: int = 3, remap=None):
    """-> (packed fp32 forward tables, what the arithmetic in force needs besides them) for a forward-only call, packed
    once per weight version (weight_pack_cache)."""
    def build():
        PACK_CACHE_STATS["packs"] += 1
        planes = pack_for_arithmetic(flat_params, False, pd, remap=remap)
        if isinstance(planes, ResidentWeights):
            planes.fast = _INFERENCE_ARITHMETIC.value == "fast"
        return (pack_weights(flat_params, "fwd", pd=pd, remap=remap), planes)
    if not _PACK_CACHE.value:
        return build()
    key = (flat_params.data_ptr(), flat_params._version, tuple(p._version for p in net.parameters()), _MLP_ARITHMETIC.value,
           _INFERENCE_ARITHMETIC.value, pd, torch.cuda.current_stream(flat_params.device).cuda_stream if flat_params.is_cuda else 0)
    hit = getattr(net, "_infer_packs", None)
    if hit is not None and hit[0] == key:
        PACK_CACHE_STATS["hits"] += 1
        return hit[1]
    packs = build()
    # (a plain attribute, not a buffer: it must not travel in state_dict() or follow .to())
    object.__setattr__(net, "_infer_packs", (key, packs))
    return packs


def network_packs(net, flat_params: Tensor, train: bool, n: int, pd: int = 3, remap=None):
    """-> (packed fp32 forward tables, planes) for one call of an autograd node on `n` samples: the tables and what the
    arithmetic in force (mlp_arithmetic) needs besides them -- the resident kernels' streams, or None (the fused fp32-MFMA
    kernels).  Training packs per call (the weights change every step); a forward-only call takes both from the
    network's version-keyed cache (inference_packs).  An empty batch launches no network: tables and planes = None."""
    if train or n == 0:
        wpacked = pack_weights(flat_params, "fwd", pd=pd, remap=remap)
        return wpacked, (pack_for_arithmetic(flat_params, train, pd, remap=remap) if n > 0 else None)
    return inference_packs(net, flat_params, pd, remap=remap)


_canon_cache = {}


class ResidentWeights:
    """What the resident arithmetic reads besides the packed fp32 tables: the two fp16 fragment streams and the
    scale table (pack_resident)."""
    __slots__ = ("fwd", "bwd", "scales", "pd", "fast")

    def __init__(self, fwd, bwd, scales, pd):
        self.fwd, self.bwd, self.scales, self.pd = fwd, bwd, scales, pd
        # forward-only launches with these weights run on one fp16 product per product (inference_arithmetic "fast").
        # Set by inference_packs alone -- the packs of a forward-only call -- so no training pass ever sees it.
        self.fast = False


class ChunkMaxima:
    """Per weight-gradient workgroup chunk, the largest |value| of the operands of the eight 256 x 256 GEMMs of one
    network pass: `x` [8, chunks] left by the resident forward, `z` [8, chunks] by the resident data-gradient chain
    (one atomic max per wave and layer); with them the GEMMs run on three fp16 products (csrc/wgrad256_half.h)."""
    __slots__ = ("x", "z", "chunks", "chunk_samples", "scales")

    def __init__(self, P: int, device):
        self.chunks = int(_capi.load().scnerf_wgrad256_chunks(wgrad_chunks(P)))
        self.chunk_samples = int(_capi.load().scnerf_wgrad_chunk_samples(int(P), self.chunks))
        # rows 0 .. 7: the eight 256 x 256 GEMMs; rows 8 .. 11 of z: dZ of the views layer, dZ of layer 0, max(1, |point|),
        # max(1, |direction|) (left by the resident data-gradient kernel for the narrow GEMMs, csrc/wgrad_half_narrow.h)
        both = torch.zeros((2, 12, self.chunks), dtype=torch.float32, device=device)
        self.x, self.z = both[0], both[1]
        self.scales = None        # the scale table of the weights the data-gradient kernel ran with (mlp_bwd_resident)


_h3_tables = {}


def _h3_device_tables(pd: int, device):
    key = (pd, str(device))
    if key not in _h3_tables:
        t = {"jobs": torch.from_numpy(np.ascontiguousarray(ML.h3_scale_jobs(pd))).to(device)}
        for kind in ("fwd", "bwd"):
            idx, meta, _, _ = ML.h3_plan(pd, kind)
            t[kind] = (torch.from_numpy(idx).to(device), torch.from_numpy(meta).to(device), int(meta.shape[0]))
        _h3_tables[key] = t
    return _h3_tables[key]


def pack_resident(flat_params: Tensor, pd: int = 3, out: Optional[ResidentWeights] = None, remap=None) -> ResidentWeights:
    """flat parameter buffer (reference order) -> the fp16 fragment streams of the forward and the data-gradient chain
    and the per-layer scale table of the resident arithmetic (csrc/mlp_h3.h); once per optimizer step.  `remap` as in
    pack_weights."""
    _f(flat_params, "flat_params")
    lay = ML.layout(pd)
    if flat_params.numel() != lay.n_params:
        raise ValueError("expected %d parameters, got %d" % (lay.n_params, flat_params.numel()))
    lib = _capi.load()
    dev = flat_params.device
    if remap is not None:
        key = (remap[0], str(dev))
        if key not in _canon_cache:
            _canon_cache[key] = torch.from_numpy(np.asarray(remap[1], dtype=np.int32)).to(dev)
        idx = _canon_cache[key]
        canon = torch.empty(lay.n_params, dtype=torch.float32, device=dev)
        _capi.check(lib.scnerf_gather_f32(_p(flat_params), _p(idx), _p(canon), idx.numel(), _stream()), "scnerf_gather_f32")
        flat_params = canon
    t = _h3_device_tables(pd, dev)
    if out is None:
        out = ResidentWeights(torch.empty(t["fwd"][2] * 512, dtype=torch.int16, device=dev),
                              torch.empty(t["bwd"][2] * 512, dtype=torch.int16, device=dev),
                              torch.empty(lib.scnerf_h3_scale_floats(), dtype=torch.float32, device=dev), pd)
    st = lib.scnerf_h3_pack(_p(flat_params), _p(t["jobs"]), _p(t["fwd"][0]), _p(t["fwd"][1]), t["fwd"][2],
                            _p(t["bwd"][0]), _p(t["bwd"][1]), t["bwd"][2], _p(out.fwd), _p(out.bwd), _p(out.scales), _stream())
    _capi.check(st, "scnerf_h3_pack")
    return out


def _vd(viewdirs: Tensor):
    """(pointer, row stride) of a [n,3] fp32 view-direction tensor that may be a column slice
    of the packed ray batch (ray_batch[:, 8:11])."""
    if viewdirs.dtype != torch.float32 or not _capi.on_device(viewdirs) or viewdirs.dim() != 2 or viewdirs.shape[1] != 3:
        raise TypeError("viewdirs must be a CUDA fp32 [n,3] tensor")
    if viewdirs.stride(1) != 1:
        raise ValueError("viewdirs rows must be dense")
    return viewdirs.data_ptr(), int(viewdirs.stride(0)) if viewdirs.shape[0] > 1 else 3


def _network_args(pts: Tensor, viewdirs: Tensor, packed: Tensor, kind: str, pd: int, save: Optional[Tensor]):
    """What mlp_fwd / mlp_bwd and their resident twins check alike: the points, the view directions, the packed fp32
    tables of the pass (`kind` "fwd": wpacked, "bwd": wpacked_bwd) and the activation workspace, which a forward may go
    without and must find large enough.  -> (view-direction pointer, its row stride, the layout of variant `pd`, P)."""
    name = "wpacked" if kind == "fwd" else "wpacked_bwd"
    _f(pts, "pts"), _f(packed, name)
    if kind == "bwd":
        _f(save, "save")
    vptr, vstride = _vd(viewdirs)
    lay = ML.layout(pd)
    P = pts.numel() // pd
    if packed.numel() != (lay.fwd_total if kind == "fwd" else lay.bwd_total):
        raise ValueError(name + " has the wrong size")
    if kind == "fwd" and save is not None:
        _f(save, "save")
        if save.numel() < lay.save_floats(P):
            raise ValueError("activation workspace too small")
    return vptr, vstride, lay, P


def _ray_outputs(n: int, s: int, device, want_weights: bool = True):
    """-> (rgb [n,3], disp [n], acc [n], depth [n], weights [n,s] or None): the per-ray outputs of a compositing launch"""
    rgb = torch.empty((n, 3), dtype=torch.float32, device=device)
    disp, acc, depth = (torch.empty((n,), dtype=torch.float32, device=device) for _ in range(3))
    return rgb, disp, acc, depth, torch.empty((n, s), dtype=torch.float32, device=device) if want_weights else None


_MAC_PER_SAMPLE = {3: 593408, 4: 593408 + 2 * 256 * 21}       # layer 0 and the skip layer are 21 columns wider


def mlp_fwd(pts: Tensor, viewdirs: Tensor, samples_per_ray: int, wpacked: Tensor,
            save: Optional[Tensor] = None, pd: int = 3, planes: Optional[Tensor] = None,
            maxima: Optional["ChunkMaxima"] = None, guard: Optional[GuardRecord] = None, lean: bool = False) -> Tensor:
    """pts [P, pd] (pd = 3: x y z; pd = 4: x y z 1/r) -> raw [P, 4] (rgb logits, sigma pre-activation).
    `planes`: the ResidentWeights (pack_resident) -> the resident kernel; None -> the fused fp32-MFMA kernel.
    `guard`: a GuardRecord (guard_records) for the resident kernel's scale guard; None: no check.
    `lean` (resident training pass of the standard network): the feature section of `save` is not written
    (lean_workspace)."""
    if isinstance(planes, ResidentWeights):
        if planes.pd != pd:
            raise ValueError("resident weights of another network variant")
        return mlp_fwd_resident(pts, viewdirs, samples_per_ray, wpacked, planes, save, maxima, guard, lean=lean)
    vptr, vstride, _, P = _network_args(pts, viewdirs, wpacked, "fwd", pd, save)
    raw = torch.empty((P, 4), dtype=torch.float32, device=pts.device)
    tag = "" if pd == 3 else "/pd4"
    if planes is not None:
        raise TypeError("planes must be a ResidentWeights or None")
    if lean:
        raise ValueError("the lean workspace belongs to the resident arithmetic")
    with PROFILE.region("mlp_fwd_kernel%s/P=%d/%s" % (tag, P, "train" if save is not None else "infer"),
                        2 * _MAC_PER_SAMPLE[pd] * P):
        st = _capi.load().scnerf_mlp_fwd(pd, _p(pts), vptr, vstride, int(samples_per_ray), _p(wpacked), _p(raw),
                                         _p(save), P, _stream())
    _capi.check(st, "scnerf_mlp_fwd")
    return raw


def mlp_fwd_resident(pts: Tensor, viewdirs: Tensor, samples_per_ray: int, wpacked: Tensor, rw: ResidentWeights,
                     save: Optional[Tensor] = None, maxima: Optional[ChunkMaxima] = None,
                     guard: Optional[GuardRecord] = None, lean: bool = False) -> Tensor:
    """mlp_fwd in the resident arithmetic: one launch, three fp16 products per product, activations register-resident
    (csrc/mlp_fwd_h3.hip); save (training) receives the same workspace as mlp_fwd's."""
    pd = rw.pd
    vptr, vstride, _, P = _network_args(pts, viewdirs, wpacked, "fwd", pd, save)
    raw = torch.empty((P, 4), dtype=torch.float32, device=pts.device)
    _check_lean(lean, pd, save, maxima, rw)
    if rw.fast:
        if save is not None or guard is not None:
            raise ValueError("the one-product arithmetic is forward-only and takes no guard record")
        with PROFILE.region("mlp_fwd_h3_kernel%s/P=%d/infer fast" % ("" if pd == 3 else "/pd4", P), 2 * _MAC_PER_SAMPLE[pd] * P):
            st = _capi.load().scnerf_mlp_fwd_h3_fast(pd, _p(pts), vptr, vstride, int(samples_per_ray), _p(wpacked), _p(rw.fwd),
                                                     _p(rw.scales), _p(raw), P, None, 0, 0, _stream())
        _capi.check(st, "scnerf_mlp_fwd_h3_fast")
        return raw
    with PROFILE.region("mlp_fwd_h3_kernel%s/P=%d/%s" % ("" if pd == 3 else "/pd4", P, "train" if save is not None else "infer"),
                        2 * _MAC_PER_SAMPLE[pd] * P):
        mx = maxima if save is not None else None
        st = _capi.load().scnerf_mlp_fwd_h3_lean(
            pd, _p(pts), vptr, vstride, int(samples_per_ray), _p(wpacked), _p(rw.fwd), _p(rw.scales), _p(raw), _p(save), P,
            _p(mx.x) if mx else None, mx.chunks if mx else 0, mx.chunk_samples if mx else 0, *_guard_args(guard), int(lean),
            _stream())
    _capi.check(st, "scnerf_mlp_fwd_h3")

    def rerun(flags, wgs):
        _capi.check(_capi.load().scnerf_mlp_fwd_gated(pd, _p(pts), vptr, vstride, int(samples_per_ray), _p(wpacked), _p(raw),
                                                      _p(save), P, flags, wgs, _stream()), "scnerf_mlp_fwd_gated")
    _guard_after(guard, rerun)
    return raw


def _check_lean(lean, pd, save, maxima, rw):
    """a lean pass is a training pass (3-D or 4-D points) that leaves chunk maxima (lean_workspace)"""
    if lean and (pd not in (3, 4) or save is None or maxima is None or rw.fast):
        raise ValueError("the lean workspace needs a training pass on three-product packs with chunk maxima")


COARSE_STAGE_SAMPLES = 64        # the fused coarse stage exists for two wave tiles per ray (csrc/mlp_fwd.hip)


def coarse_stage_fwd(rays: Tensor, t_vals: Tensor, t_rand: Optional[Tensor], lindisp: bool, wpacked: Tensor,
                     save: Optional[Tensor], noise: Optional[Tensor], white_bkgd: bool, planes: Optional[Tensor] = None,
                     maxima: Optional["ChunkMaxima"] = None, guard: Optional[GuardRecord] = None, lean: bool = False):
    """coarse_sample + mlp_fwd + composite_fwd of the coarse stage as one launch (64 samples per ray; `lean`: as mlp_fwd):
    -> (z [n,64], pts [n,64,3], raw [n,64,4], rgb [n,3], disp [n], acc [n], weights [n,64], depth [n])."""
    _f(rays, "rays"), _f(t_vals, "t_vals"), _f(wpacked, "wpacked")
    for name, t_ in (("t_rand", t_rand), ("noise", noise), ("save", save)):
        if t_ is not None:
            _f(t_, name)
    n, s = rays.shape[0], t_vals.shape[0]
    if s != COARSE_STAGE_SAMPLES or rays.shape[1] < 11:
        raise ValueError("the fused coarse stage takes 64 samples per ray and an 11-column ray batch")
    lay = ML.layout(3)
    if wpacked.numel() != lay.fwd_total:
        raise ValueError("wpacked has the wrong size")
    if save is not None and save.numel() < lay.save_floats(n * s):
        raise ValueError("activation workspace too small")
    dev = rays.device
    z = torch.empty((n, s), dtype=torch.float32, device=dev)
    pts = torch.empty((n, s, 3), dtype=torch.float32, device=dev)
    raw = torch.empty((n, s, 4), dtype=torch.float32, device=dev)
    rgb, disp, acc, depth, w = _ray_outputs(n, s, dev)
    P = n * s
    if isinstance(planes, ResidentWeights):
        if planes.pd != 3:
            raise ValueError("the coarse stage samples 3-D points")
        _check_lean(lean, 3, save, maxima, planes)
        if planes.fast:
            if save is not None or guard is not None:
                raise ValueError("the one-product arithmetic is forward-only and takes no guard record")
            with PROFILE.region("mlp_fwd_h3_kernel<coarse stage>/P=%d/infer fast" % P, 2 * _MAC_PER_SAMPLE[3] * P):
                st = _capi.load().scnerf_coarse_stage_fwd_h3_fast(
                    _p(rays), rays.shape[1], _p(t_vals), _p(t_rand), int(bool(lindisp)), _p(wpacked), _p(planes.fwd),
                    _p(planes.scales), _p(noise), int(bool(white_bkgd)), _p(z), _p(pts), _p(raw), _p(rgb), _p(disp), _p(acc),
                    _p(depth), _p(w), n, s, None, 0, 0, _stream())
            _capi.check(st, "scnerf_coarse_stage_fwd_h3_fast")
            return z, pts, raw, rgb, disp, acc, w, depth
        with PROFILE.region("mlp_fwd_h3_kernel<coarse stage>/P=%d/%s" % (P, "train" if save is not None else "infer"),
                            2 * _MAC_PER_SAMPLE[3] * P):
            st = _capi.load().scnerf_coarse_stage_fwd_h3_lean(
                _p(rays), rays.shape[1], _p(t_vals), _p(t_rand), int(bool(lindisp)), _p(wpacked), _p(planes.fwd),
                _p(planes.scales), _p(save), _p(noise), int(bool(white_bkgd)), _p(z), _p(pts), _p(raw), _p(rgb), _p(disp),
                _p(acc), _p(depth), _p(w), n, s, _p(maxima.x) if (maxima and save is not None) else None,
                maxima.chunks if maxima else 0, maxima.chunk_samples if maxima else 0, *_guard_args(guard), int(lean),
                _stream())
        _capi.check(st, "scnerf_coarse_stage_fwd_h3")

        def rerun(flags, wgs):
            _capi.check(_capi.load().scnerf_coarse_stage_fwd_gated(
                _p(rays), rays.shape[1], _p(t_vals), _p(t_rand), int(bool(lindisp)), _p(wpacked), _p(save), _p(noise),
                int(bool(white_bkgd)), _p(z), _p(pts), _p(raw), _p(rgb), _p(disp), _p(acc), _p(depth), _p(w), n, s, flags, wgs,
                _stream()), "scnerf_coarse_stage_fwd_gated")
        _guard_after(guard, rerun)
        return z, pts, raw, rgb, disp, acc, w, depth
    if planes is not None:
        raise TypeError("planes must be a ResidentWeights or None")
    if lean:
        raise ValueError("the lean workspace belongs to the resident arithmetic")
    with PROFILE.region("mlp_fwd_kernel/P=%d/%s" % (P, "train" if save is not None else "infer"), 2 * _MAC_PER_SAMPLE[3] * P):
        st = _capi.load().scnerf_coarse_stage_fwd(_p(rays), rays.shape[1], _p(t_vals), _p(t_rand), int(bool(lindisp)),
                                                  _p(wpacked), _p(save), _p(noise), int(bool(white_bkgd)), _p(z), _p(pts),
                                                  _p(raw), _p(rgb), _p(disp), _p(acc), _p(depth), _p(w), n, s, _stream())
    _capi.check(st, "scnerf_coarse_stage_fwd")
    return z, pts, raw, rgb, disp, acc, w, depth


FINE_STAGE_IMPORTANCE = (64, 128, 192)       # the fused fine stage exists for 64 + N_importance = 128, 192, 256 samples per ray
# Whether render_rays takes the fine stage as ONE launch (fine_stage_fwd) or as three (fine_sample, mlp_fwd, composite_fwd).
# Both routes are the same device code on the same numbers (bit-identical outputs: tests).  Measured on the MI355X at
# 4096 x (64 + 128) (profiles/r04_fused_fine_stage.txt): one launch 3.14 ms, the three launches back to back 3.07 ms
# (3.45 against 3.20 ms before the samplers' serial sections were rewritten).  The sampler is ~8 us of one wave's work per
# workgroup; as a kernel of its own a CU overlaps sixteen rays of it (43 us for the batch), in front of the resident
# network -- one wave per SIMD, nothing else resident -- every microsecond of it is exposed, eight workgroups in a row per
# CU.  Off by default for that reason; SCNERF_FUSED_FINE_STAGE=1 switches it on.
_FUSED_FINE_STAGE = _Switch((False, True), "SCNERF_FUSED_FINE_STAGE", parse=lambda preset: preset not in (None, "", "0"))


def fused_fine_stage(on: Optional[bool] = None) -> bool:
    return _FUSED_FINE_STAGE(_on_off(on))


# The lean workspace of a training pass (csrc/wgrad.hip): feature_linear has no activation and feeds the
# views layer linearly, so its weight gradients and the views layer's feature columns follow from ONE views-layer GEMM on
# act7 -- the resident kernels store neither `feature` nor `d feature`, the big weight-gradient launch runs seven GEMMs
# instead of eight, a finishing kernel forms three small products in fp64.  Taken by RenderRaysFunction when the pass
# trains on the resident arithmetic with the half weight-gradient arithmetic and chunk maxima; SCNERF_LEAN_WORKSPACE=0
# keeps the full workspace and the twelve-GEMM group (one build can be A/B-ed).
# The switch has a scope: "off", "render" (the default: RenderRaysFunction alone) or "all" (SCNERF_LEAN_WORKSPACE=all:
# also the NeRF++ node, both networks, and the differentiable network query node, under the same conditions).
_LEAN_SCOPES = ("off", "render", "all")


def _lean_scope_from_env(value: Optional[str]) -> str:
    if value is None:
        return "render"
    if value in ("", "0"):
        return "off"
    return "all" if value == "all" else "render"


_LEAN_WORKSPACE = _Switch(_LEAN_SCOPES, "SCNERF_LEAN_WORKSPACE", set_error="lean workspace scope must be one of %s" % (_LEAN_SCOPES,),
                          parse=_lean_scope_from_env)


def lean_workspace_scope(scope: Optional[str] = None) -> str:
    """Which training nodes take the lean workspace: "off" none, "render" the render step, "all" the NeRF++ node and the
    network query node as well.  Without an argument: the scope in force."""
    return _LEAN_WORKSPACE(scope)


def lean_workspace(on: Optional[bool] = None) -> bool:
    """The render step's switch: True selects scope "render", False "off"; -> whether the render step runs lean."""
    if on is not None:
        _LEAN_WORKSPACE.value = "render" if on else "off"
    return _LEAN_WORKSPACE.value != "off"


def lean_decision(scopes, *maxima) -> bool:
    """Whether a training node runs its passes lean -- the one copy of the rule: the scope in force is one of `scopes`
    (the render step: ("render", "all"); the NeRF++ node and the query node: ("all",)), every pass of the node has its
    chunk maxima (the resident kernels train) and the weight-gradient arithmetic is "half".  A node asks ONCE, in
    forward: its data gradients and weight-gradient groups follow the answer whatever the switches say by then."""
    return bool(_LEAN_WORKSPACE.value in scopes and all(m is not None for m in maxima) and wgrad_arithmetic() == "half")


def fine_stage_fwd(rays: Tensor, z_c: Tensor, w_c: Tensor, u: Tensor, wpacked: Tensor, save: Optional[Tensor],
                   noise: Optional[Tensor], white_bkgd: bool, planes: "ResidentWeights", maxima: Optional["ChunkMaxima"] = None,
                   want_inds=False, want_cdf=False, want_weights=False, lean: bool = False):
    """fine_sample + mlp_fwd + composite_fwd of the fine stage as ONE launch (resident arithmetic; 64 coarse samples and
    N_importance in FINE_STAGE_IMPORTANCE; `lean`: as mlp_fwd): -> (z_f [n,tot], pts_f [n,tot,3], z_samples [n,sf], z_std [n], inds, cdf,
    raw [n,tot,4], rgb [n,3], disp [n], acc [n], depth [n], weights)."""
    _f(rays, "rays"), _f(z_c, "z_c"), _f(w_c, "w_c"), _f(u, "u"), _f(wpacked, "wpacked")
    for name, t_ in (("noise", noise), ("save", save)):
        if t_ is not None:
            _f(t_, name)
    if not isinstance(planes, ResidentWeights) or planes.pd != 3:
        raise TypeError("the fused fine stage runs on the resident arithmetic (3-D points)")
    if planes.fast:
        raise ValueError("the fused fine stage has no one-product instantiation: fine_sample, mlp_fwd, composite_fwd")
    n, sc = z_c.shape
    sf = u.shape[-1]
    if sc != COARSE_STAGE_SAMPLES or sf not in FINE_STAGE_IMPORTANCE or rays.shape[1] < 11:
        raise ValueError("the fused fine stage takes 64 coarse samples, N_importance in %s and an 11-column ray batch" % (FINE_STAGE_IMPORTANCE,))
    tot = sc + sf
    stride = sf if u.dim() == 2 else 0
    lay = ML.layout(3)
    if wpacked.numel() != lay.fwd_total:
        raise ValueError("wpacked has the wrong size")
    if save is not None and save.numel() < lay.save_floats(n * tot):
        raise ValueError("activation workspace too small")
    dev = rays.device
    z_f = torch.empty((n, tot), dtype=torch.float32, device=dev)
    pts_f = torch.empty((n, tot, 3), dtype=torch.float32, device=dev)
    z_s = torch.empty((n, sf), dtype=torch.float32, device=dev)
    z_std = torch.empty((n,), dtype=torch.float32, device=dev)
    inds = torch.empty((n, sf), dtype=torch.int64, device=dev) if want_inds else None
    cdf = torch.empty((n, sc - 1), dtype=torch.float32, device=dev) if want_cdf else None
    raw = torch.empty((n, tot, 4), dtype=torch.float32, device=dev)
    rgb, disp, acc, depth, w = _ray_outputs(n, tot, dev, want_weights)
    P = n * tot
    mx = maxima if save is not None else None
    _check_lean(lean, 3, save, maxima, planes)
    with PROFILE.region("mlp_fwd_h3_kernel<fine stage>/P=%d/%s" % (P, "train" if save is not None else "infer"),
                        2 * _MAC_PER_SAMPLE[3] * P):
        # (no guard record: with the guard on the fine stage runs as three launches)
        st = _capi.load().scnerf_fine_stage_fwd_h3_lean(
            _p(rays), rays.shape[1], _p(z_c), _p(w_c), _p(u), stride, _p(wpacked), _p(planes.fwd), _p(planes.scales), _p(save),
            _p(noise), int(bool(white_bkgd)), _p(z_f), _p(pts_f), _p(z_s), _p(z_std), _p(inds), _p(cdf), _p(raw), _p(rgb),
            _p(disp), _p(acc), _p(depth), _p(w), n, sc, sf, _p(mx.x) if mx else None, mx.chunks if mx else 0,
            mx.chunk_samples if mx else 0, *_guard_args(None), int(lean), _stream())
    _capi.check(st, "scnerf_fine_stage_fwd_h3")
    return z_f, pts_f, z_s, z_std, inds, cdf, raw, rgb, disp, acc, depth, w


def save_workspace(P: int, device, pd: int = 3) -> Tensor:
    return torch.empty(ML.layout(pd).save_floats(P), dtype=torch.float32, device=device)


def mlp_bwd(d_raw: Tensor, pts: Tensor, viewdirs: Tensor, samples_per_ray: int, wpacked_bwd: Tensor,
            save: Tensor, pd: int = 3, planes: Optional[Tensor] = None, maxima: Optional["ChunkMaxima"] = None,
            input_grad: bool = True, guard: Optional[GuardRecord] = None, lean: bool = False):
    """-> (grads workspace, d_pts [P,pd], d_views [P,3]).  `planes`, `guard`: as mlp_fwd.  input_grad=False: d_pts / d_views
    are not needed -- the resident kernel skips them and returns None for both (the fp32 kernel computes them anyway).
    `lean` (the pass whose forward ran lean): the d feature section of the grads workspace is not written."""
    if isinstance(planes, ResidentWeights):
        if planes.pd != pd:
            raise ValueError("resident weights of another network variant")
        return mlp_bwd_resident(d_raw, pts, viewdirs, samples_per_ray, wpacked_bwd, planes, save, maxima, input_grad, guard,
                                lean=lean)
    if lean:
        raise ValueError("the lean workspace belongs to the resident arithmetic")
    _f(d_raw, "d_raw")
    vptr, vstride, _, P = _network_args(pts, viewdirs, wpacked_bwd, "bwd", pd, save)
    dev = pts.device
    grads = torch.empty(ML.grad_floats(P), dtype=torch.float32, device=dev)
    d_pts = torch.empty((P, pd), dtype=torch.float32, device=dev)
    d_views = torch.empty((P, 3), dtype=torch.float32, device=dev)
    if planes is not None:
        raise TypeError("planes must be a ResidentWeights or None")
    with PROFILE.region("mlp_bwd_kernel%s/P=%d" % ("" if pd == 3 else "/pd4", P), 2 * _MAC_PER_SAMPLE[pd] * P):
        st = _capi.load().scnerf_mlp_bwd(pd, _p(d_raw), _p(pts), vptr, vstride, int(samples_per_ray),
                                         _p(wpacked_bwd), _p(save), _p(grads), _p(d_pts), _p(d_views), P, _stream())
    _capi.check(st, "scnerf_mlp_bwd")
    return grads, d_pts, d_views


def mlp_bwd_resident(d_raw: Tensor, pts: Tensor, viewdirs: Tensor, samples_per_ray: int, wpacked_bwd: Tensor,
                     rw: ResidentWeights, save: Tensor, maxima: Optional[ChunkMaxima] = None, input_grad: bool = True,
                     guard: Optional[GuardRecord] = None, lean: bool = False):
    """mlp_bwd in the resident arithmetic (csrc/mlp_bwd_h3.hip): one launch -> (grads workspace, d_pts, d_views);
    input_grad=False: the instantiation without the input gradient, d_pts = d_views = None."""
    _f(d_raw, "d_raw")
    pd = rw.pd
    vptr, vstride, _, P = _network_args(pts, viewdirs, wpacked_bwd, "bwd", pd, save)
    _check_lean(lean, pd, save, maxima, rw)
    dev = pts.device
    grads = torch.empty(ML.grad_floats(P), dtype=torch.float32, device=dev)
    d_pts = torch.empty((P, pd), dtype=torch.float32, device=dev) if input_grad else None
    d_views = torch.empty((P, 3), dtype=torch.float32, device=dev) if input_grad else None
    with PROFILE.region("mlp_bwd_h3_kernel%s/P=%d" % ("" if pd == 3 else "/pd4", P), 2 * _MAC_PER_SAMPLE[pd] * P):
        if maxima is not None:
            maxima.scales = rw.scales
        st = _capi.load().scnerf_mlp_bwd_h3_lean(
            pd, _p(d_raw), _p(pts), vptr, vstride, int(samples_per_ray), _p(wpacked_bwd), _p(rw.bwd), _p(rw.scales), _p(save),
            _p(grads), _p(d_pts), _p(d_views), P, _p(maxima.z) if maxima else None, maxima.chunks if maxima else 0,
            maxima.chunk_samples if maxima else 0, *_guard_args(guard), int(lean), _stream())
    _capi.check(st, "scnerf_mlp_bwd_h3")

    def rerun(flags, wgs):
        # (the fp32 kernel always forms the input gradient: scratch when the caller does not want it)
        dp = d_pts if input_grad else torch.empty((P, pd), dtype=torch.float32, device=dev)
        dv = d_views if input_grad else torch.empty((P, 3), dtype=torch.float32, device=dev)
        _capi.check(_capi.load().scnerf_mlp_bwd_gated(pd, _p(d_raw), _p(pts), vptr, vstride, int(samples_per_ray),
                                                      _p(wpacked_bwd), _p(save), _p(grads), _p(dp), _p(dv), P, flags, wgs,
                                                      _stream()), "scnerf_mlp_bwd_gated")
    _guard_after(guard, rerun)
    return grads, d_pts, d_views


def wgrad_chunks(P: int) -> int:
    """workgroups the sample axis is split into (one per CU at full size)."""
    return int(max(1, min(256, P // 256)))


_wgrad_ws = {}


def wgrad_arithmetic(mode: Optional[str] = None) -> str:
    """The 256 x 256 weight-gradient GEMMs and the narrow ones with a tile-native dZ: "half" (default) -- three fp16
    products per product with one power-of-two scale per operand and workgroup chunk, where the resident kernels left
    the chunk maxima (csrc/wgrad256_half.h, wgrad_half_narrow.h); "fp32", and wherever no maxima were left: the
    exact-fp32 MFMA.  Without an argument: the mode in force."""
    code = {None: -1, "fp32": 0, "half": 1}[mode]
    return ("fp32", "half")[_capi.load().scnerf_wgrad_arithmetic(code)]


def nerf_wgrad(save: Tensor, grads: Tensor, d_raw: Tensor, P: int, flat_grad: Optional[Tensor] = None,
               pd: int = 3, accumulate: bool = False, maxima: Optional[ChunkMaxima] = None, lean: bool = False,
               flat_params: Optional[Tensor] = None) -> Tensor:
    """All parameter gradients of one network -> flat buffer (mlp_layout.Layout parameter order);
    `accumulate`: add to `flat_grad` instead of overwriting it.
    `lean`: the workspaces come from lean passes (lean_workspace: no feature / d feature sections) -- the lean group, which
    needs `flat_params`, the flat parameter buffer (mlp_layout order, pd 3 or 4) of the network that ran the pass, the
    chunk maxima of both resident kernels and the half arithmetic; without any of them it raises (a lean workspace must
    never reach the full group)."""
    lib = _capi.load()
    chunks = wgrad_chunks(P)
    key = (chunks, str(save.device))
    if key not in _wgrad_ws:
        _wgrad_ws[key] = torch.empty(lib.scnerf_nerf_wgrad_workspace_floats(chunks), dtype=torch.float32,
                                     device=save.device)
    if flat_grad is None:
        flat_grad = torch.empty(ML.layout(pd).n_params, dtype=torch.float32, device=save.device)
    elif flat_grad.numel() != ML.layout(pd).n_params or flat_grad.dtype != torch.float32 or not flat_grad.is_contiguous():
        raise ValueError("flat_grad must be a contiguous fp32 buffer of %d elements" % ML.layout(pd).n_params)
    tag = "" if pd == 3 else "/pd4"
    # the maxima count only when BOTH resident kernels of this pass filled them (the data-gradient kernel leaves its mark
    # in `scales`): a half-filled table would scale one operand by 2^126
    if maxima is not None and maxima.scales is None:
        maxima = None
    if lean:
        if pd not in (3, 4) or maxima is None or flat_params is None:
            raise ValueError("the lean weight-gradient group needs 3-D or 4-D points, the chunk maxima of both resident "
                             "kernels and flat_params")
        if wgrad_arithmetic() != "half":
            raise RuntimeError("the weight-gradient arithmetic was switched away from \"half\" after a lean forward pass: its "
                               "workspace has no feature sections for the full group")
        _f(flat_params, "flat_params")
        if flat_params.numel() != ML.layout(pd).n_params:
            raise ValueError("flat_params of another network")
    group = "wgrad(11 GEMMs + reduces + finish, lean)" if lean else "wgrad(12 GEMMs + reduces)"
    with PROFILE.region("%s%s/P=%d" % (group, tag, P), 2 * _MAC_PER_SAMPLE[pd] * P, group=True):
        ev = (None, None)
        if PROFILE.enabled:
            # the dominant launch inside this C call -- the eight 256 x 256 GEMMs -- between two events the call records
            mode = wgrad_arithmetic()
            if mode == "half" and maxima is None:
                mode = "fp32"
            big = 7 if lean else 8
            inner = PROFILE.raw_pair("wgrad256_kernel<%d GEMMs, %s>%s/P=%d" % (big, mode, tag, P), big * 2 * 256 * 256 * P)
            ev = (inner[0].cuda_event, inner[1].cuda_event)
        if maxima is not None and maxima.chunks != lib.scnerf_wgrad256_chunks(chunks):
            raise ValueError("chunk maxima of another chunking")
        if lean:
            st = lib.scnerf_nerf_wgrad_h3_lean(pd, _p(save), _p(grads), _p(d_raw), P, chunks, _p(_wgrad_ws[key]),
                                               _p(flat_grad), int(bool(accumulate)), _p(maxima.x), _p(maxima.z),
                                               _p(maxima.scales), _p(flat_params), ev[0], ev[1], _stream())
        else:
            st = lib.scnerf_nerf_wgrad_h3(pd, _p(save), _p(grads), _p(d_raw), P, chunks, _p(_wgrad_ws[key]),
                                          _p(flat_grad), int(bool(accumulate)), _p(maxima.x) if maxima else None,
                                          _p(maxima.z) if maxima else None, _p(maxima.scales) if maxima else None, ev[0], ev[1],
                                          _stream())
    _capi.check(st, "scnerf_nerf_wgrad")
    return flat_grad


# ---- the backward pass on the live samples (csrc/live_compact.hip) ----------------------------------------------------
# A sample whose noisy density is not positive has alpha = 0, so its d_raw row is all +-0 and it adds exact zeros to every
# gradient of the network.  With the switch on, the render step's backward compacts the other samples (ascending: the
# result is a function of the inputs alone), runs the unchanged data-gradient kernel on that batch and the weight-gradient
# GEMMs on its dZ with X gathered from the dense workspace.  ONE host read per backward: the two counts size the launches.
LIVE_MIN_SAMPLES = 131072       # below this a pass stays dense (the break-even against the host read)
LIVE_MAX_SAMPLES = (1 << 22) - 128      # the gather offsets of a 256-wide section are 32 bits
# A pass with a larger live share than this stays dense: the route costs about 0.47 ms of the headline step (the bound of
# 1.74 ms against the 1.27 ms kept, profiles/r10_live_samples.txt) where the two dense calls take 7.1 ms, so it pays from
# about 7 % of dead samples on.  The count is on the host by then and depends on d_raw alone.
LIVE_MAX_SHARE = 0.9
_LIVE_SAMPLES = _Switch((False, True), "SCNERF_LIVE_SAMPLES", parse=lambda preset: preset not in ("", "0"))
_LIVE_MIN = [LIVE_MIN_SAMPLES]


def live_samples(on: Optional[bool] = None, min_samples: Optional[int] = None) -> bool:
    """Whether the render step's backward runs on the live samples alone (default on; SCNERF_LIVE_SAMPLES=0 presets it
    off).  `min_samples`: the smallest pass that compacts (LIVE_MIN_SAMPLES; tests force it down)."""
    if on is not None:
        _LIVE_SAMPLES.value = bool(on)
    if min_samples is not None:
        _LIVE_MIN[0] = int(min_samples)
    return _LIVE_SAMPLES.value


def live_decision(P: int, maxima) -> bool:
    """Whether a pass of P samples compacts -- the one copy of the rule: the switch, the resident arithmetic with its chunk
    maxima, the half weight-gradient arithmetic, LIVE_MIN_SAMPLES <= P <= LIVE_MAX_SAMPLES.  Never a question of whether the
    rays need a gradient: both kinds of step take the same route at the same P.  The scale guard does not enter either: a
    step whose passes trip nothing must be the guard-off step bit for bit (tests/test_gpu_resident_guard.py), so a guarded
    pass compacts too and goes back to the dense route only where the guard trips (live_guard_tripped)."""
    return bool(_LIVE_SAMPLES.value and maxima is not None and wgrad_arithmetic() == "half"
                and _LIVE_MIN[0] <= P <= LIVE_MAX_SAMPLES)


def live_guard_record(guard: GuardRecord, n: int) -> GuardRecord:
    """the data-gradient record of a pass for its compact batch of n samples: block flags of the compact batch (the pass's
    own are indexed by dense blocks) and an `any` word and a report of its own, all zero -- where the compact batch trips,
    the pass goes back to the dense route with its own record, which this launch must not have touched"""
    nb = (int(n) + 127) // 128
    rep = guard.report.numel() if guard.report is not None else 0
    buf = torch.zeros(max(nb, 1) + 1 + rep, dtype=torch.float32, device=guard.any.device)
    ints = buf.view(torch.int32)
    return GuardRecord(guard.name, nb, ints[:max(nb, 1)], ints[max(nb, 1):max(nb, 1) + 1], buf[max(nb, 1) + 1:] if rep else None,
                       guard.mode)


def live_guard_keep(guard: GuardRecord):
    """the compact batch tripped nothing: its record is the pass's latest (resident_margins)"""
    _GUARD_LAST[guard.name] = guard


def live_guard_tripped(guard: Optional[GuardRecord]) -> bool:
    """Whether a guarded launch tripped (reads one device word: the guard modes pay a host wait the default does not).
    The exact-fp32 rerun of a tripped block reads the DENSE workspace, so a pass with a tripped block -- in its forward, or
    in the data gradients of its compact batch -- takes the dense route with the pass's own records."""
    return guard is not None and int(guard.any.item()) != 0


class LiveSamples:
    """The compaction of one pass: idx int32 [padded P] (the live samples ascending, then zeros up to the padded count),
    xoff uint32 in the 256 x 256 weight-gradient kernel's load order, d_raw [P, 4] (the live rows first), the count on the
    device and in a pinned word; `n` once live_counts has read it."""
    __slots__ = ("P", "idx", "xoff", "d_raw", "count", "host", "n")


def live_compact(d_raw: Tensor) -> LiveSamples:
    """d_raw [.., 4] -> the compaction of its samples (two launches; nothing waits here: live_counts does)."""
    _f(d_raw, "d_raw")
    lib = _capi.load()
    L = LiveSamples()
    L.P = d_raw.numel() // 4
    dev = d_raw.device
    Pp = ML.padded_samples(L.P)
    both = torch.empty((2, Pp), dtype=torch.int32, device=dev)
    L.idx, L.xoff = both[0], both[1]
    L.d_raw = torch.empty((L.P, 4), dtype=torch.float32, device=dev)
    L.count = torch.empty(1, dtype=torch.int32, device=dev)
    L.host = torch.empty(1, dtype=torch.int32, device="cpu", pin_memory=d_raw.is_cuda)
    L.n = None
    ws = torch.empty(int(lib.scnerf_live_compact_workspace_ints(L.P)), dtype=torch.int32, device=dev)
    st = lib.scnerf_live_compact(_p(d_raw), L.P, _p(ws), _p(L.idx), _p(L.xoff), _p(L.d_raw), _p(L.count), _p(L.host), _stream())
    _capi.check(st, "scnerf_live_compact")
    return L


def live_counts(*batches: LiveSamples):
    """THE host wait of a backward: one event behind the last compaction, then the pinned words of all of them."""
    if batches and batches[0].d_raw.is_cuda:
        ev = torch.cuda.Event()
        ev.record()
        ev.synchronize()
    for L in batches:
        L.n = int(L.host[0])
    return [L.n for L in batches]


def live_gather(L: LiveSamples, save: Tensor, pts: Tensor, viewdirs: Tensor, samples_per_ray: int, pd: int = 3):
    """-> (masks int32, pts [n, pd], viewdirs [n, 3]) of the compact batch: what the data-gradient kernel reads"""
    vptr, vstride = _vd(viewdirs)
    lay = ML.layout(pd)
    Pp, Pl = ML.padded_samples(L.P), ML.padded_samples(L.n)
    if save.numel() < lay.save_floats(L.P):
        raise ValueError("activation workspace too small")
    masks = save[lay.save_floats_per_sample * Pp:]
    dev = pts.device
    masks_l = torch.empty(ML.MASK_WORDS_PER_SAMPLE * Pl, dtype=torch.int32, device=dev)
    pts_l = torch.empty((L.n, pd), dtype=torch.float32, device=dev)
    vd_l = torch.empty((L.n, 3), dtype=torch.float32, device=dev)
    st = _capi.load().scnerf_live_gather(_p(L.idx), L.n, L.P, _p(masks), _p(pts), pd, vptr, vstride, int(samples_per_ray),
                                         _p(masks_l), _p(pts_l), _p(vd_l), _stream())
    _capi.check(st, "scnerf_live_gather")
    return masks_l, pts_l, vd_l


def live_maxima(L: LiveSamples, maxima: ChunkMaxima) -> ChunkMaxima:
    """the chunk maxima of the compact batch: x remapped from the forward's (an upper bound per compact chunk), z left
    to the data-gradient kernel"""
    out = ChunkMaxima(L.n, maxima.x.device)
    st = _capi.load().scnerf_live_remap_maxima(_p(L.idx), L.n, _p(maxima.x), maxima.chunks, maxima.chunk_samples, _p(out.x),
                                               out.chunks, out.chunk_samples, 8, _stream())
    _capi.check(st, "scnerf_live_remap_maxima")
    return out


def mlp_bwd_live(L: LiveSamples, masks: Tensor, pts: Tensor, viewdirs: Tensor, wpacked_bwd: Tensor, rw: ResidentWeights,
                 maxima: ChunkMaxima, input_grad: bool = True, lean: bool = False, guard: Optional[GuardRecord] = None):
    """mlp_bwd_resident on the compact batch of live_gather (one view direction per sample, the masks by their own
    pointer): -> (grads workspace of L.n samples, d_pts [n, pd], d_views [n, 3]) in compact order.  `guard`: a record of
    live_guard_record; "strict" raises on a trip here, the other modes leave the trip to the caller (live_guard_tripped,
    live_guard_keep)."""
    pd = rw.pd
    n, dev = L.n, pts.device
    _f(pts, "pts"), _f(viewdirs, "viewdirs"), _f(wpacked_bwd, "wpacked_bwd")
    if pts.numel() != n * pd or viewdirs.numel() != n * 3 or masks.numel() != ML.MASK_WORDS_PER_SAMPLE * ML.padded_samples(n):
        raise ValueError("not the compact batch of this compaction")
    if wpacked_bwd.numel() != ML.layout(pd).bwd_total:
        raise ValueError("wpacked_bwd has the wrong size")
    grads = torch.empty(ML.grad_floats(n), dtype=torch.float32, device=dev)
    d_pts = torch.empty((n, pd), dtype=torch.float32, device=dev) if input_grad else None
    d_views = torch.empty((n, 3), dtype=torch.float32, device=dev) if input_grad else None
    with PROFILE.region("mlp_bwd_h3_kernel%s/P=%d live" % ("" if pd == 3 else "/pd4", n), 2 * _MAC_PER_SAMPLE[pd] * n):
        maxima.scales = rw.scales
        st = _capi.load().scnerf_mlp_bwd_h3_masks(
            pd, _p(L.d_raw), _p(pts), _p(viewdirs), 3, 1, _p(wpacked_bwd), _p(rw.bwd), _p(rw.scales), _p(masks), _p(grads),
            _p(d_pts), _p(d_views), n, _p(maxima.z), maxima.chunks, maxima.chunk_samples, *_guard_args(guard), int(lean),
            _stream())
    _capi.check(st, "scnerf_mlp_bwd_h3_masks")
    if guard is not None and guard.mode == "strict":
        _GUARD_LAST[guard.name] = guard
        guard.raise_if_tripped()
    return grads, d_pts, d_views


def live_scatter_rows(L: LiveSamples, rows: Tensor) -> Tensor:
    """rows [n, w] of the compact batch -> [P, w] in sample order, zero rows for the dead samples"""
    _f(rows, "rows")
    w = rows.shape[1]
    out = torch.empty((L.P, w), dtype=torch.float32, device=rows.device)
    st = _capi.load().scnerf_live_scatter_rows(_p(rows), _p(L.idx), _p(out), L.n, w, L.P, _stream())
    _capi.check(st, "scnerf_live_scatter_rows")
    return out


def nerf_wgrad_live(L: LiveSamples, save: Tensor, grads: Tensor, d_raw: Tensor, maxima: ChunkMaxima,
                    flat_grad: Optional[Tensor] = None, pd: int = 3, accumulate: bool = False, lean: bool = False,
                    flat_params: Optional[Tensor] = None) -> Tensor:
    """nerf_wgrad over the live samples: `grads` and `maxima` of the compact batch (mlp_bwd_live, live_maxima), `save` and
    `d_raw` the dense ones of the pass.  alpha_linear and rgb_linear are the dense group's, bit for bit."""
    lib = _capi.load()
    chunks_src, chunks = wgrad_chunks(L.P), wgrad_chunks(L.n)
    key = (chunks_src, str(save.device))
    if key not in _wgrad_ws:
        _wgrad_ws[key] = torch.empty(lib.scnerf_nerf_wgrad_workspace_floats(chunks_src), dtype=torch.float32, device=save.device)
    n_params = ML.layout(pd).n_params
    if flat_grad is None:
        flat_grad = torch.empty(n_params, dtype=torch.float32, device=save.device)
    elif flat_grad.numel() != n_params or flat_grad.dtype != torch.float32 or not flat_grad.is_contiguous():
        raise ValueError("flat_grad must be a contiguous fp32 buffer of %d elements" % n_params)
    if maxima is None or maxima.scales is None or maxima.chunks != lib.scnerf_wgrad256_chunks(chunks):
        raise ValueError("the live group needs the chunk maxima of the compact batch")
    if lean and (flat_params is None or flat_params.numel() != n_params):
        raise ValueError("the lean weight-gradient group needs flat_params")
    if wgrad_arithmetic() != "half":
        raise RuntimeError("the weight-gradient arithmetic was switched away from \"half\" after the compaction")
    group = "wgrad(11 GEMMs + reduces + finish, lean, live)" if lean else "wgrad(12 GEMMs + reduces, live)"
    with PROFILE.region("%s/P=%d of %d" % (group, L.n, L.P), 2 * _MAC_PER_SAMPLE[pd] * L.n, group=True):
        ev = (None, None)
        if PROFILE.enabled:
            big = 7 if lean else 8
            inner = PROFILE.raw_pair("wgrad256_kernel<%d GEMMs, half, live>/P=%d" % (big, L.n), big * 2 * 256 * 256 * L.n)
            ev = (inner[0].cuda_event, inner[1].cuda_event)
        st = lib.scnerf_nerf_wgrad_h3_live(pd, _p(save), L.P, chunks_src, _p(grads), _p(d_raw), _p(L.idx), _p(L.xoff), L.n,
                                           chunks, _p(_wgrad_ws[key]), _p(flat_grad), int(bool(accumulate)), _p(maxima.x),
                                           _p(maxima.z), _p(maxima.scales), _p(flat_params) if lean else None, ev[0], ev[1],
                                           _stream())
    _capi.check(st, "scnerf_nerf_wgrad_h3_live")
    return flat_grad


def composite_fwd(raw: Tensor, z: Tensor, rays: Tensor, noise: Optional[Tensor], white_bkgd: bool,
                  want_weights=True):
    _f(raw, "raw"), _f(z, "z"), _f(rays, "rays")
    if noise is not None:
        _f(noise, "noise")
    n, s = z.shape
    rgb, disp, acc, depth, w = _ray_outputs(n, s, z.device, want_weights)
    st = _capi.load().scnerf_composite_fwd(_p(raw), _p(z), _p(rays), rays.shape[1], _p(noise),
                                           int(bool(white_bkgd)), _p(rgb), _p(disp), _p(acc), _p(depth),
                                           _p(w), n, s, _stream())
    _capi.check(st, "scnerf_composite_fwd")
    return rgb, disp, acc, w, depth


def composite_bwd(raw, z, rays, noise, white_bkgd, g_rgb, g_disp, g_acc, g_depth, g_raw_in, want_d_rays_d=True):
    n, s = z.shape
    dev = z.device
    for name, t_ in (("g_rgb", g_rgb), ("g_disp", g_disp), ("g_acc", g_acc), ("g_depth", g_depth),
                     ("g_raw_in", g_raw_in)):
        if t_ is not None:
            _f(t_, name)
    d_raw = torch.empty((n, s, 4), dtype=torch.float32, device=dev)
    d_rd = torch.empty((n, 3), dtype=torch.float32, device=dev) if want_d_rays_d else None
    st = _capi.load().scnerf_composite_bwd(_p(raw), _p(z), _p(rays), rays.shape[1], _p(noise),
                                           int(bool(white_bkgd)), _p(g_rgb), _p(g_disp), _p(g_acc),
                                           _p(g_depth), _p(g_raw_in), _p(d_raw), _p(d_rd), n, s, _stream())
    _capi.check(st, "scnerf_composite_bwd")
    return d_raw, d_rd


def ray_reduce(d_pts, d_views, z, extra_d, d_rays, accumulate: bool):
    n, s = z.shape
    st = _capi.load().scnerf_ray_reduce(_p(d_pts), _p(d_views), _p(z), _p(extra_d), _p(d_rays),
                                        d_rays.shape[1], int(bool(accumulate)), n, s, _stream())
    _capi.check(st, "scnerf_ray_reduce")
    return d_rays


# ------------------------------------------------------------------------------ camera
def camera_matrices_fwd(intr_init, intr_noise, intr_scale, multiplicative, extr_init, extr_noise, extr_scale):
    """-> K [4,4], E [C,4,4] (scnerf_camera_matrices_fwd)"""
    for name, t_ in (("intr_init", intr_init), ("intr_noise", intr_noise), ("extr_init", extr_init), ("extr_noise", extr_noise)):
        _f(t_, name)
    C = extr_init.shape[0]
    if intr_init.numel() != 4 or intr_noise.numel() != 4 or extr_init.shape != (C, 9) or extr_noise.shape != (C, 9):
        raise ValueError("camera parameters: intrinsics [4], extrinsics [C, 9]")
    K = torch.empty((4, 4), dtype=torch.float32, device=intr_init.device)
    E = torch.empty((C, 4, 4), dtype=torch.float32, device=intr_init.device)
    st = _capi.load().scnerf_camera_matrices_fwd(_p(intr_init), _p(intr_noise), float(intr_scale), int(bool(multiplicative)),
                                                 _p(extr_init), _p(extr_noise), float(extr_scale), C, _p(K), _p(E), _stream())
    _capi.check(st, "scnerf_camera_matrices_fwd")
    return K, E


def camera_matrices_bwd(intr_init, intr_noise, intr_scale, multiplicative, extr_init, extr_noise, extr_scale, g_K, g_E,
                        want_intr=True, want_extr=True):
    """-> d intr_noise [4], d extr_noise [C,9] (None where not wanted); g_K / g_E may be None (= zero)"""
    C = extr_init.shape[0]
    for name, t_ in (("g_K", g_K), ("g_E", g_E)):
        if t_ is not None:
            _f(t_, name)
    if not (want_intr or want_extr):
        return None, None
    dev = intr_init.device
    d_in = torch.empty(4, dtype=torch.float32, device=dev) if want_intr else None
    d_ex = torch.empty((C, 9), dtype=torch.float32, device=dev) if want_extr else None
    st = _capi.load().scnerf_camera_matrices_bwd(_p(intr_init), float(intr_scale), int(bool(multiplicative)), _p(extr_init),
                                                 _p(extr_noise), float(extr_scale), C, _p(g_K), _p(g_E), _p(d_in), _p(d_ex),
                                                 _stream())
    _capi.check(st, "scnerf_camera_matrices_bwd")
    return d_in, d_ex


def _cam_common(cam: dict):
    """(ctypes argument tuple shared by camera fwd / bwd) from a dict of tensors / scalars."""
    import ctypes
    F = ctypes.c_float
    g_o, g_d = cam.get("grid_o"), cam.get("grid_d")
    grid = g_o if g_o is not None else g_d
    gh, gw = (int(grid.shape[0]), int(grid.shape[1])) if grid is not None else (0, 0)
    ext = cam.get("extrinsic")
    n_ext = 0 if ext is None else (1 if ext.dim() == 2 else int(ext.shape[0]))
    idx = cam.get("cam_idx")
    return (_p(cam.get("kps")), _p(idx), int(cam.get("single_idx", 0)), _p(ext), n_ext,
            _p(cam["intr_init"]), _p(cam["intr_noise"]), F(float(cam["intr_scale"])), int(bool(cam["multiplicative"])),
            _p(cam["extr_init"]), _p(cam["extr_noise"]), F(float(cam["extr_scale"])), int(cam["extr_init"].shape[0]),
            _p(g_o), F(float(cam.get("scale_o", 0.0))), _p(g_d), F(float(cam.get("scale_d", 0.0))), gh, gw,
            int(cam["H"]), int(cam["W"]))


def camera_rays_fwd(cam: dict, n: int):
    dev = cam["intr_init"].device
    ro = torch.empty((n, 3), dtype=torch.float32, device=dev)
    rd = torch.empty((n, 3), dtype=torch.float32, device=dev)
    if n == 0:                          # an empty tensor has no address to hand over; there is nothing to launch
        return ro, rd
    st = _capi.load().scnerf_camera_rays_fwd(*_cam_common(cam), _p(ro), _p(rd), n, _stream())
    _capi.check(st, "scnerf_camera_rays_fwd")
    return ro, rd


def camera_rays_bwd(cam: dict, n: int, g_o: Optional[Tensor], g_d: Optional[Tensor]):
    lib = _capi.load()
    dev = cam["intr_init"].device
    C = int(cam["extr_init"].shape[0])
    ext = cam.get("extrinsic")
    n_ext = 0 if ext is None else (1 if ext.dim() == 2 else int(ext.shape[0]))
    d_in = torch.empty(4, dtype=torch.float32, device=dev)
    d_ex = torch.empty((C, 9), dtype=torch.float32, device=dev) if ext is None else None
    d_go = torch.empty_like(cam["grid_o"]) if cam.get("grid_o") is not None else None
    d_gd = torch.empty_like(cam["grid_d"]) if cam.get("grid_d") is not None else None
    d_E = torch.empty((n_ext, 4, 4), dtype=torch.float32, device=dev) if ext is not None else None
    if n == 0:                          # the gradient of an empty batch: zeros, as the entry point would leave them
        return tuple(None if t is None else t.zero_() for t in (d_in, d_ex, d_go, d_gd, d_E))
    ws = torch.empty(lib.scnerf_camera_bwd_workspace_floats(max(C, n_ext)), dtype=torch.float32, device=dev)
    st = lib.scnerf_camera_rays_bwd(*_cam_common(cam), _p(g_o), _p(g_d), _p(d_in), _p(d_ex), _p(d_go), _p(d_gd),
                                    _p(d_E), _p(ws), n, _stream())
    _capi.check(st, "scnerf_camera_rays_bwd")
    return d_in, d_ex, d_go, d_gd, d_E


def pinhole_rays(kps: Optional[Tensor], c2w: Tensor, focal: float, H: int, W: int):
    import ctypes
    _f(c2w, "c2w")
    n = H * W if kps is None else kps.shape[0]
    ro = torch.empty((n, 3), dtype=torch.float32, device=c2w.device)
    rd = torch.empty((n, 3), dtype=torch.float32, device=c2w.device)
    if n == 0:
        return ro, rd
    st = _capi.load().scnerf_pinhole_rays(_p(kps), 0 if kps is None else int(kps.shape[1]), _p(c2w),
                                          ctypes.c_float(float(focal)), H, W, _p(ro), _p(rd), n, _stream())
    _capi.check(st, "scnerf_pinhole_rays")
    return ro, rd


def ndc_fwd(H, W, f2: Tensor, near: float, o: Tensor, d: Tensor):
    import ctypes
    no, nd = torch.empty_like(o), torch.empty_like(d)
    if o.shape[0] == 0:
        return no, nd
    st = _capi.load().scnerf_ndc_fwd(H, W, _p(f2), ctypes.c_float(float(near)), _p(o), _p(d), _p(no), _p(nd),
                                     o.shape[0], _stream())
    _capi.check(st, "scnerf_ndc_fwd")
    return no, nd


def ndc_bwd(H, W, f2, near, o, d, g_no, g_nd):
    import ctypes
    g_o, g_d = torch.empty_like(o), torch.empty_like(d)
    g_f = torch.empty(2, dtype=torch.float32, device=o.device)
    if o.shape[0] == 0:
        return g_o, g_d, g_f.zero_()
    st = _capi.load().scnerf_ndc_bwd(H, W, _p(f2), ctypes.c_float(float(near)), _p(o), _p(d), _p(g_no), _p(g_nd),
                                     _p(g_o), _p(g_d), _p(g_f), o.shape[0], _stream())
    _capi.check(st, "scnerf_ndc_bwd")
    return g_o, g_d, g_f


def upsample_grid_fwd(grid: Tensor, scale: float, H: int, W: int):
    import ctypes
    _f(grid, "grid")
    out = torch.empty((H * W, 3), dtype=torch.float32, device=grid.device)
    st = _capi.load().scnerf_upsample_grid_fwd(_p(grid), ctypes.c_float(float(scale)), grid.shape[0], grid.shape[1],
                                               H, W, _p(out), _stream())
    _capi.check(st, "scnerf_upsample_grid_fwd")
    return out


def upsample_grid_bwd(g_out: Tensor, scale: float, gh: int, gw: int, H: int, W: int):
    import ctypes
    d = torch.empty((gh, gw, 3), dtype=torch.float32, device=g_out.device)
    st = _capi.load().scnerf_upsample_grid_bwd(_p(g_out), ctypes.c_float(float(scale)), gh, gw, H, W, _p(d), _stream())
    _capi.check(st, "scnerf_upsample_grid_bwd")
    return d


def prd_loss_fwd(kps0, kps1, r0o, r0d, r1o, r1d, K, E2, eps: float, threshold: float, negate_fx: bool,
                 eval_mode: bool):
    """-> (loss [] , n_match [], sums [6]) device tensors; no host sync."""
    import ctypes
    for name, t in (("kps0", kps0), ("kps1", kps1), ("rays0_o", r0o), ("rays0_d", r0d), ("rays1_o", r1o),
                    ("rays1_d", r1d), ("K", K), ("E2", E2)):
        _f(t, name)
    m = kps0.shape[0]
    out = torch.empty(8, dtype=torch.float32, device=kps0.device)
    st = _capi.load().scnerf_prd_loss_fwd(_p(kps0), _p(kps1), _p(r0o), _p(r0d), _p(r1o), _p(r1d), _p(K), _p(E2),
                                          ctypes.c_float(eps), ctypes.c_float(threshold), int(negate_fx),
                                          int(eval_mode), m, _p(out), out[6:].data_ptr(), out[7:].data_ptr(),
                                          _stream())
    _capi.check(st, "scnerf_prd_loss_fwd")
    return out[6], out[7], out[:6]


def prd_loss_bwd(kps0, kps1, r0o, r0d, r1o, r1d, K, E2, eps: float, threshold: float, negate_fx: bool, sums,
                 g_loss: Tensor):
    """-> (g_rays0_o, g_rays0_d, g_rays1_o, g_rays1_d, g_K [4,4], g_E2 [2,4,4])"""
    import ctypes
    m = kps0.shape[0]
    dev = kps0.device
    g = torch.empty((4, m, 3), dtype=torch.float32, device=dev)
    small = torch.empty(16 + 32 + 36, dtype=torch.float32, device=dev)
    g_loss = _f(g_loss.reshape(1).contiguous(), "g_loss")
    st = _capi.load().scnerf_prd_loss_bwd(_p(kps0), _p(kps1), _p(r0o), _p(r0d), _p(r1o), _p(r1d), _p(K), _p(E2),
                                          ctypes.c_float(eps), ctypes.c_float(threshold), int(negate_fx), m,
                                          _p(sums), _p(g_loss), g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(),
                                          g[3].data_ptr(), small.data_ptr(), small[16:].data_ptr(),
                                          small[48:].data_ptr(), _stream())
    _capi.check(st, "scnerf_prd_loss_bwd")
    return g[0], g[1], g[2], g[3], small[:16].view(4, 4), small[16:48].view(2, 4, 4)


def prd_filter(kps0, kps1, r0o, r0d, r1o, r1d, K, E2, eps: float, threshold: float, negate_fx: bool) -> Tensor:
    """-> bool [M]: matches that re-project within `threshold` both ways and lie in front of both cameras."""
    import ctypes
    for name, t in (("kps0", kps0), ("kps1", kps1), ("rays0_o", r0o), ("rays0_d", r0d), ("rays1_o", r1o),
                    ("rays1_d", r1d), ("K", K), ("E2", E2)):
        _f(t, name)
    m = kps0.shape[0]
    keep = torch.empty(m, dtype=torch.uint8, device=kps0.device)
    st = _capi.load().scnerf_prd_filter(_p(kps0), _p(kps1), _p(r0o), _p(r0d), _p(r1o), _p(r1d), _p(K), _p(E2),
                                        ctypes.c_float(eps), ctypes.c_float(threshold), int(negate_fx), m,
                                        _p(keep), _stream())
    _capi.check(st, "scnerf_prd_filter")
    return keep.bool()


def embed_fwd(x: Tensor, freqs: Tensor, include_input: bool) -> Tensor:
    """x [n,d] -> [n, d (include_input + 2 F)] (Embedder.embed)."""
    _f(x, "x"), _f(freqs, "freqs")
    n, d = x.shape
    out = torch.empty((n, d * (int(include_input) + 2 * freqs.numel())), dtype=torch.float32, device=x.device)
    st = _capi.load().scnerf_embed_fwd(_p(x), n, d, _p(freqs), freqs.numel(), int(include_input), _p(out), _stream())
    _capi.check(st, "scnerf_embed_fwd")
    return out


def embed_bwd(x: Tensor, g_out: Tensor, freqs: Tensor, include_input: bool) -> Tensor:
    _f(x, "x"), _f(g_out, "g_out"), _f(freqs, "freqs")
    n, d = x.shape
    g_x = torch.empty_like(x)
    st = _capi.load().scnerf_embed_bwd(_p(x), _p(g_out), n, d, _p(freqs), freqs.numel(), int(include_input), _p(g_x),
                                       _stream())
    _capi.check(st, "scnerf_embed_bwd")
    return g_x


def pack_rays_fwd(H, W, f2: Optional[Tensor], ndc_near: float, o: Tensor, d: Tensor, near: float, far: float, cols: int):
    import ctypes
    _f(o, "rays_o"), _f(d, "rays_d")
    n = o.shape[0]
    out = torch.empty((n, cols), dtype=torch.float32, device=o.device)
    if n == 0:
        return out
    st = _capi.load().scnerf_pack_rays_fwd(int(H), int(W), _p(f2), ctypes.c_float(float(ndc_near)), _p(o), _p(d),
                                           ctypes.c_float(float(near)), ctypes.c_float(float(far)), int(cols), _p(out), n,
                                           _stream())
    _capi.check(st, "scnerf_pack_rays_fwd")
    return out


def pack_rays_bwd(H, W, f2: Optional[Tensor], ndc_near: float, o: Tensor, d: Tensor, cols: int, g: Tensor, want_f2: bool):
    import ctypes
    _f(g, "g_ray_batch")
    g_o, g_d = torch.empty_like(o), torch.empty_like(d)
    g_f = torch.empty(2, dtype=torch.float32, device=o.device) if (want_f2 and f2 is not None) else None
    if o.shape[0] == 0:
        return g_o, g_d, None if g_f is None else g_f.zero_()
    st = _capi.load().scnerf_pack_rays_bwd(int(H), int(W), _p(f2), ctypes.c_float(float(ndc_near)), _p(o), _p(d), int(cols),
                                           _p(g), _p(g_o), _p(g_d), _p(g_f), o.shape[0], _stream())
    _capi.check(st, "scnerf_pack_rays_bwd")
    return g_o, g_d, g_f


def image_metrics(x: Tensor, y: Tensor, taps: Tensor, c1: float, c2: float, value_range: float, clip_x: bool,
                  want_map: bool = False):
    """SSIM [N], MSE [N] and optionally the SSIM map [N, C, H-win+1, W-win+1] of x against y, both [N, C, H, W] fp32 with
    ANY strides (no copy is made), in one kernel pass plus a small fixed-order reduction (csrc/image_metrics.hip).  `taps`:
    the normalised 1-D window [win] on the device."""
    for t, name in ((x, "x"), (y, "y"), (taps, "taps")):
        if not _capi.on_device(t):
            raise RuntimeError("%s must live on the GPU (scnerf_amd has no CPU path)" % name)
        if t.dtype != torch.float32:
            raise TypeError("%s must be torch.float32, got %s" % (name, t.dtype))
    if x.dim() != 4 or x.shape != y.shape:
        raise ValueError("x and y must both be [N, C, H, W], got %s and %s" % (tuple(x.shape), tuple(y.shape)))
    if taps.dim() != 1 or not taps.is_contiguous():
        raise ValueError("taps must be a contiguous vector")
    n, c, h, w = x.shape
    win = taps.shape[0]
    if win % 2 == 0 or not 3 <= win <= 11:
        raise ValueError("the window must have an odd number of taps between 3 and 11, got %d" % win)
    if h < win or w < win:
        raise ValueError("images of %d x %d pixels are smaller than the %d-tap window" % (h, w, win))
    if c < 1:
        raise ValueError("x and y need at least one channel")
    ssim = torch.empty(n, dtype=torch.float32, device=x.device)
    mse = torch.empty(n, dtype=torch.float32, device=x.device)
    ss_map = torch.empty((n, c, h - win + 1, w - win + 1), dtype=torch.float32, device=x.device) if want_map else None
    lib = _capi.load()
    ws = torch.empty(max(int(lib.scnerf_image_metrics_workspace_floats(n, c, h, w, win)), 2), dtype=torch.float32,
                     device=x.device)
    st = lib.scnerf_image_metrics(_p(x), *x.stride(), _p(y), *y.stride(), n, c, h, w, _p(taps), win, c1, c2, value_range,
                                  int(bool(clip_x)), _p(ssim), _p(mse), _p(ss_map), _p(ws), _stream())
    _capi.check(st, "scnerf_image_metrics")
    return ssim, mse, ss_map


def ray_batch(mode: int, seed: int, step: int, images: Optional[Tensor], image_ids: Optional[Tensor], n_sel: int,
              image_pos: int, H: int, W: int, window, n: int, rank: int = 0, world: int = 1, white_bkgd: bool = False,
              want_coords=True, want_select_inds=True, want_image_idx=True, device=None):
    """One training batch in ONE launch (csrc/ray_batch.hip; reference NeRF/run_nerf.py:368-478): -> (coords int64 [n, 2] as
    (x, y), select_inds int64 [n] = y W + x, image_idx int64 [n], target fp32 [n, 3]), None where not wanted (target: where
    `images` is None).  mode 0: n pixels of the window (x0, y0, w, h) of selected image `image_pos`, without replacement;
    mode 1: the next n rays of a permutation of every ray of the n_sel selected images.  `images`: [n_images, H, W, 3] fp32
    or [n_images, H, W, 3 | 4] uint8, read in place; `image_ids`: int64 [n_sel] rows of it, or None.  Nothing here makes
    the host wait for the device."""
    u8, channels, n_images = 0, 3, max(int(n_sel), 1)
    if images is not None:
        if not _capi.on_device(images):
            raise RuntimeError("images must live on the GPU (scnerf_amd has no CPU path)")
        if images.dtype not in (torch.float32, torch.uint8):
            raise TypeError("images must be torch.float32 or torch.uint8, got %s" % images.dtype)
        if images.dim() != 4 or not images.is_contiguous() or tuple(images.shape[1:3]) != (int(H), int(W)):
            raise ValueError("images must be contiguous [n, %d, %d, C], got %s" % (H, W, tuple(images.shape)))
        u8, channels, n_images = int(images.dtype == torch.uint8), int(images.shape[3]), int(images.shape[0])
        device = images.device
    if image_ids is not None:
        _chk(image_ids, torch.int64, "image_ids")
        if image_ids.numel() != int(n_sel):
            raise ValueError("image_ids must have n_sel = %d entries, got %d" % (n_sel, image_ids.numel()))
        device = image_ids.device if device is None else device
    if device is None:
        raise ValueError("ray_batch needs `images`, `image_ids` or `device` to know where to put the batch")
    n = int(n)
    empty = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=device)
    coords = empty((n, 2), torch.int64) if want_coords else None
    select_inds = empty((n,), torch.int64) if want_select_inds else None
    image_idx = empty((n,), torch.int64) if want_image_idx else None
    target = empty((n, 3), torch.float32) if images is not None else None
    x0, y0, w, h = (int(v) for v in window)
    st = _capi.load().scnerf_ray_batch(int(mode), int(seed) & _MASK64, int(step), _p(images), u8, channels, n_images, int(H),
                                       int(W), _p(image_ids), int(n_sel), int(image_pos), x0, y0, w, h, n, int(rank),
                                       int(world), int(bool(white_bkgd)), _p(coords), _p(select_inds), _p(image_idx),
                                       _p(target), _stream())
    _capi.check(st, "scnerf_ray_batch")
    return coords, select_inds, image_idx, target
