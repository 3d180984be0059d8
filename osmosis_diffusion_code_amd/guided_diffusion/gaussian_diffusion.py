"""Samplers -- registry surface of the reference's guided_diffusion/gaussian_diffusion.py
(register_sampler/get_sampler/create_sampler :19-62, GaussianDiffusion :65-370, space_timesteps
:373-426, SpacedDiffusion :429-474, DDPM :492-502, DDIM :505-535, get_named_beta_schedule :542-566).

`p_sample_loop` keeps the reference signature and return values.  For the Osmosis configuration
(pretrain_model == 'osmosis', our UNetModel, the 'osmosis' conditioning method with
gradient_x_prev, any registered mean / variance processor pair, clip_denoised or not) every step runs as
ONE device-resident sequence with no host synchronisation:

    fetch_coefs -> UNet forward plan -> osm_posterior_c -> [osm_phys_reduce/finalize x n_iter ->
    osm_phys_grad] -> [osm_clamp_bwd] -> osm_posterior_bwd_c -> UNet data-gradient plan -> osm_guide_update_c

(the reference performs 4 + n_iter device->host copies per step: gaussian_diffusion.py:216,276,288,
condition_methods.py:130,224).  Per-timestep coefficients live in a device table indexed by a
device-side step counter, so the whole step can be replayed from a hipGraph.  The rgb-guidance
configuration (`rgb_guidance=True`: DDPM / DDIM `p_sample` + 'ps' conditioning on an identity operator,
gaussian noiser) runs through the same loop: osm_phys_* with the identity operator (kind 3) for
||y - x0[:, 0:3]|| and its gradient, osm_guide_update(_rng)_c or osm_ddim_update_c for the step.  The per-step
noise is drawn inside the update kernel (Philox-4x32-10) unless `noise="aten"` asks for torch's stream.
`dynamic_threshold` runs there too (osm_posterior_dynthr_c / osm_dynthr_bwd: an on-device exact quantile of the whole batch) when the
batch is one engine pass.  The PCGS inner alternation (`local_M > 1`: the step repeated at the same t inside [s_end, s_start],
:225-309) runs there as `alternate_len` sub-steps per index (`pcgs_schedule`).  Any other combination (third-party conditioners /
operators / processors, a chunked batch with dynamic_threshold) falls back to a generic loop that follows the reference control flow on
top of the HIP UNet operator through torch.autograd.
`p_sample_loop(tiling=)` runs ONE canvas larger than the network's grid as overlapping tiles of the network's size (`_tiled_loop`,
`tile_grid`; osm_tile_gather / osm_tile_blend move canvas <-> tiles): the network is tiled, every other part of the step acts on the canvas.
A sampler built with `solver="ddim" | "dpmpp_2m"` (few-step solvers; include/osmosis_solver.h) replaces the state update of all three
loops by x_next = A x_t + B0 x0 + B1 x0_prev + S z - scale clamp(grad) (`solver_table`; osm_solver_update(_rng)_c on the fused and
tiled loops); `create_sampler(timestep_spacing=)` picks the few indices (`select_timesteps`).  `solver=None`: nothing changes.
"""
import math

import numpy as np
import torch

from .. import ops
from ..osmosis_utils import utils as utilso
from .condition_methods import ConditioningMethod, PosteriorSamplingOsmosis
from .posterior_mean_variance import get_mean_processor, get_var_processor

__SAMPLER__ = {}
DYNAMIC_THRESHOLD_S = 0.98     # the quantile process_xstart asks dynamic_thresholding for (posterior_mean_variance.py:45)


def register_sampler(name: str):
    def wrapper(cls):
        if __SAMPLER__.get(name, None):
            raise NameError(f"Name {name} is already registered!")
        __SAMPLER__[name] = cls
        return cls
    return wrapper


def get_sampler(name: str):
    if __SAMPLER__.get(name, None) is None:
        raise NameError(f"Name {name} is not defined!")
    return __SAMPLER__[name]


def create_sampler(sampler, steps, noise_schedule, model_mean_type, model_var_type, dynamic_threshold,
                   clip_denoised, rescale_timesteps, timestep_respacing="", timestep_spacing="uniform", solver=None,
                   solver_eta=0.0, **kwargs):
    """timestep_spacing: 'uniform' = `space_timesteps(steps, timestep_respacing)`; 'quad' / 'logsnr' take ONE integer count in
    `timestep_respacing` and pick the indices with `select_timesteps` (the low-noise end resolved: few-step chains).
    solver / solver_eta: a few-step solver as the step rule (`SOLVERS`; None: the sampler class's own)."""
    cls = get_sampler(name=sampler)
    betas = get_named_beta_schedule(noise_schedule, steps)
    if timestep_spacing not in TIMESTEP_SPACINGS:
        raise ValueError(f"timestep_spacing must be one of {TIMESTEP_SPACINGS}, got {timestep_spacing!r}")
    extra = {}
    if solver is not None:            # (a sampler without one is built exactly as it always was)
        extra = dict(solver=solver, solver_eta=solver_eta)
    if timestep_spacing == "uniform":
        if not timestep_respacing:
            timestep_respacing = [steps]
        use = space_timesteps(steps, timestep_respacing)
    else:
        try:
            if isinstance(timestep_respacing, (bool, float, list, tuple)):
                raise ValueError
            count = int(timestep_respacing)
        except (TypeError, ValueError):
            raise ValueError(f"timestep_spacing={timestep_spacing!r} takes one integer count in timestep_respacing, got "
                             f"{timestep_respacing!r}") from None
        use = set(select_timesteps(np.cumprod(1.0 - betas, axis=0), count, timestep_spacing))
    return cls(use_timesteps=use, betas=betas,
               model_mean_type=model_mean_type, model_var_type=model_var_type,
               dynamic_threshold=dynamic_threshold, clip_denoised=clip_denoised,
               rescale_timesteps=rescale_timesteps, annealing_time=kwargs.get("annealing_time", False), **extra)


def get_named_beta_schedule(schedule_name, num_diffusion_timesteps):
    T = num_diffusion_timesteps
    if schedule_name == "linear":
        k = 1000 / T
        return np.linspace(k * 0.0001, k * 0.02, T, dtype=np.float64)
    if schedule_name == "cosine":
        return betas_for_alpha_bar(T, lambda u: math.cos((u + 0.008) / 1.008 * math.pi / 2) ** 2)
    raise NotImplementedError(f"unknown beta schedule: {schedule_name}")


def betas_for_alpha_bar(num_diffusion_timesteps, alpha_bar, max_beta=0.999):
    T = num_diffusion_timesteps
    return np.array([min(1 - alpha_bar((i + 1) / T) / alpha_bar(i / T), max_beta) for i in range(T)])


def space_timesteps(num_timesteps, section_counts):
    if isinstance(section_counts, str):
        if section_counts.startswith("ddim"):
            want = int(section_counts[len("ddim"):])
            for stride in range(1, num_timesteps):
                if len(range(0, num_timesteps, stride)) == want:
                    return set(range(0, num_timesteps, stride))
            raise ValueError(f"cannot create exactly {num_timesteps} steps with an integer stride")
        section_counts = [int(x) for x in section_counts.split(",")]
    elif isinstance(section_counts, int):
        section_counts = [section_counts]
    base, extra = divmod(num_timesteps, len(section_counts))
    start, picked = 0, []
    for i, count in enumerate(section_counts):
        size = base + (1 if i < extra else 0)
        if size < count:
            raise ValueError(f"cannot divide section of {size} steps into {count}")
        stride = 1 if count <= 1 else (size - 1) / (count - 1)
        pos = 0.0
        for _ in range(count):
            picked.append(start + round(pos))   # Python round (banker's), as the reference
            pos += stride
        start += size
    return set(picked)


SOLVERS = ("ddim", "dpmpp_2m")
TIMESTEP_SPACINGS = ("uniform", "quad", "logsnr")


def select_timesteps(base_alphas_cumprod, N, spacing):
    """N distinct indices of a T-step schedule for a few-step chain, ascending, always with 0 and T - 1.  Targets from the noisiest
    end, k = N - 1 .. 0: 'quad' (T - 1) (k / (N - 1))^2, nearest index floor(v + 1/2); 'logsnr' N values uniform in
    lambda = log(alpha / sigma) from lambda(T - 1) to lambda(0), nearest index argmin |lambda - v|.  Each target takes its nearest
    index clamped to [targets still to come, previous pick - 1]."""
    ac = np.asarray(base_alphas_cumprod, dtype=np.float64)
    T = int(ac.shape[0])
    if spacing not in ("quad", "logsnr"):
        raise ValueError(f"select_timesteps: spacing must be 'quad' or 'logsnr', got {spacing!r}")
    if isinstance(N, bool) or int(N) != N or not 2 <= int(N) <= T:
        raise ValueError(f"select_timesteps: the step count must be an integer in [2, {T}], got {N!r}")
    N = int(N)
    if spacing == "quad":
        near = [int(math.floor((T - 1) * (k / (N - 1)) ** 2 + 0.5)) for k in range(N - 1, -1, -1)]
    else:
        lam = 0.5 * (np.log(ac) - np.log1p(-ac))
        near = [int(np.argmin(np.abs(lam - v))) for v in np.linspace(lam[T - 1], lam[0], N)]
    picks, prev = [], T
    for j, i in enumerate(near):
        prev = min(max(i, N - 1 - j), prev - 1)
        picks.append(prev)
    return picks[::-1]


def solver_table(sampler, rule, eta=0.0, first=None):
    """float64 [T][4] = A, B0, B1, S of a few-step solver over the sampler's own (respaced) schedule: the deterministic part of the
    state after index i is A x_t + B0 x0 + B1 x0_prev, plus S z (include/osmosis_solver.h states the rules; 'ddim': Song et al.
    2021 eq. 12 with `eta`; 'dpmpp_2m': Lu et al. 2022, DPM-Solver++ multistep, data prediction, eta = 0).  first: the first
    executed index (default T - 1) -- history starts empty there, so its 2M row is first order.  The last index' row is
    (0, 1, 0, 0): the sample is x0."""
    rule, eta = check_solver(rule if rule is not None else "", eta)
    ab = np.asarray(sampler.alphas_cumprod, dtype=np.float64)
    abp = np.asarray(sampler.alphas_cumprod_prev, dtype=np.float64)
    T = int(ab.shape[0])
    first = T - 1 if first is None else int(first)
    if not 0 <= first <= T - 1:
        raise ValueError(f"first must be in [0, {T - 1}], got {first}")
    tab = np.zeros((T, 4), dtype=np.float64)
    for i in range(T):
        if abp[i] == 1.0:
            tab[i] = (0.0, 1.0, 0.0, 0.0)
            continue
        al, sg, alp, sgp = math.sqrt(ab[i]), math.sqrt(1.0 - ab[i]), math.sqrt(abp[i]), math.sqrt(1.0 - abp[i])
        if rule == "ddim":
            s = eta * math.sqrt((1.0 - abp[i]) / (1.0 - ab[i])) * math.sqrt(1.0 - ab[i] / abp[i])
            A = math.sqrt(1.0 - abp[i] - s * s) / sg
            tab[i] = (A, alp - A * al, 0.0, s)
            continue
        h = math.log(alp / sgp) - math.log(al / sg)
        beta = -alp * math.expm1(-h)
        if i == first or i == T - 1:
            tab[i] = (sgp / sg, beta, 0.0, 0.0)
        else:
            r = (math.log(al / sg) - math.log(math.sqrt(ab[i + 1]) / math.sqrt(1.0 - ab[i + 1]))) / h      # h_prev / h
            tab[i] = (sgp / sg, beta * (1.0 + 1.0 / (2.0 * r)), -beta / (2.0 * r), 0.0)
    return tab


def check_solver(solver, solver_eta):
    """The (name, eta) of a sampler's solver, validated; (None, 0.0): the sampler's own step rule."""
    if solver is None:
        return None, 0.0
    if solver not in SOLVERS:
        raise ValueError(f"unknown solver {solver!r}: one of {', '.join(SOLVERS)} (or None for the sampler's own step rule)")
    eta = float(solver_eta)
    if not eta >= 0.0:
        raise ValueError(f"solver_eta must be >= 0, got {solver_eta!r}")
    if solver == "dpmpp_2m" and eta != 0.0:
        raise ValueError(f"the dpmpp_2m solver is deterministic: solver_eta must be 0, got {solver_eta!r}")
    return solver, eta


def solver_refusals(diffusion, sample_pattern, mean_only):
    """What a chain with a solver does not carry, raised on the host: the PCGS inner alternation (a step repeated at one t has no
    multistep meaning) and the mean-only branch."""
    if diffusion.solver is None:
        return
    if mean_only:
        raise NotImplementedError(f"solver={diffusion.solver!r}: the mean-only branch (pretrain_model != 'osmosis' without "
                                  "rgb_guidance) has no solver step")
    if max(a for _, _, a in pcgs_schedule(sample_pattern, diffusion.num_timesteps)) > 1 or (
            sample_pattern is not None and sample_pattern.get("pattern") not in (None, "original")
            and int(sample_pattern.get("local_M", 1)) > 1):
        raise ValueError(f"solver={diffusion.solver!r} with local_M > 1: a step repeated at the same t has no multistep meaning")


def guidance_flag(sample_pattern, idx, T):
    """Whether index idx of a T-step chain is guided (gaussian_diffusion.py:214-218)."""
    if sample_pattern is None or sample_pattern["pattern"] == "original" or sample_pattern["pattern"] is None:
        return True
    return sample_pattern["start_guidance"] * T >= idx >= sample_pattern["stop_guidance"] * T


def pcgs_schedule(sample_pattern, T):
    """[(guided, freeze_phi, alternate_len)] for idx = T-1 .. 0 (entry T-1-idx): the per-index decisions of the reference's loop
    (gaussian_diffusion.py:214-225, osmosis_utils/utils.py:574-630).  alternate_len > 1 is the PCGS inner loop (local_M sub-steps at
    the same t inside [s_end, s_start]).  Raises the reference's AssertionError for an invalid pattern (update_start <= update_end,
    s_start <= s_end, or with local_M > 1 a sub-step window outside the update window)."""
    if sample_pattern is None:
        return [(True, False, 1)] * T
    return [(guidance_flag(sample_pattern, idx, T), bool(utilso.is_freeze_phi(sample_pattern, idx, T)),
             int(utilso.set_alternate_length(sample_pattern, idx, T))) for idx in range(T - 1, -1, -1)]


TILE_WINDOWS = ("uniform", "hann")
TILING_KEYS = ("tile", "stride", "window")


def tile_origins(L, t, s):
    """First pixels of the tiles of side t at stride s along an axis of length L: range(0, L - t, s) and the edge-aligned last
    tile L - t (so the last overlap may be ragged); L == t -> [0]."""
    L, t, s = int(L), int(t), int(s)
    if t < 1 or L < t:
        raise ValueError(f"a tile of side {t} does not fit a canvas side of {L}")
    if not 1 <= s <= t:
        raise ValueError(f"the stride must be in [1, tile side] = [1, {t}], got {s}")
    return list(range(0, L - t, s)) + [L - t]


def tile_window(t, window):
    """float64 [t]: 'uniform' = ones, 'hann' = sin^2(pi (i + 1/2) / t) (strictly positive: every covered pixel keeps weight)."""
    if window == "uniform":
        return np.ones(int(t), dtype=np.float64)
    if window == "hann":
        return np.sin(np.pi * (np.arange(int(t), dtype=np.float64) + 0.5) / int(t)) ** 2
    raise ValueError(f"window must be one of {TILE_WINDOWS}, got {window!r}")


def _pair(v, what):
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"{what} must be an integer or a (y, x) pair, got {v!r}")
        a, b = v
    else:
        a = b = v
    if isinstance(a, bool) or isinstance(b, bool) or int(a) != a or int(b) != b:
        raise ValueError(f"{what} must be an integer or a (y, x) pair of integers, got {v!r}")
    return int(a), int(b)


def parse_tiling(tiling):
    """`tiling = dict(tile=int | (th, tw), stride=int | (sy, sx), window='uniform' | 'hann')` -> (th, tw, sy, sx, window).
    `tile` is required; stride defaults to half the tile, window to 'hann' (parameters, not tuned values).  Unknown keys raise."""
    if not isinstance(tiling, dict):
        raise ValueError(f"tiling must be a mapping with the keys {TILING_KEYS}, got {type(tiling).__name__}")
    unknown = set(tiling) - set(TILING_KEYS)
    if unknown:
        raise ValueError(f"tiling: unknown key(s) {sorted(unknown)} (known: {', '.join(TILING_KEYS)})")
    if "tile" not in tiling:
        raise ValueError("tiling needs `tile` (the side the network sees)")
    th, tw = _pair(tiling["tile"], "tiling.tile")
    sy, sx = _pair(tiling["stride"], "tiling.stride") if tiling.get("stride") is not None else (max(1, th // 2), max(1, tw // 2))
    window = tiling.get("window", "hann")
    if window not in TILE_WINDOWS:
        raise ValueError(f"window must be one of {TILE_WINDOWS}, got {window!r}")
    return th, tw, sy, sx, window


def tile_grid(Hc, Wc, tile, stride, window="hann"):
    """The tiles of a Hc x Wc canvas (tiled sampling, MultiDiffusion): (origins int32 [n,2] in (y, x) order, row-major -- y outer,
    x inner --, wy fp32 [th], wx fp32 [tw], inv_norm fp32 [Hc,Wc]), CPU tensors.  The window is separable, w(y, x) = wy[y] wx[x];
    inv_norm = 1 / sum of the covering tiles' fp32 windows, formed in float64 and cast once, so the blend weights sum to one at
    every pixel (each pixel is covered: the last tile of an axis is edge-aligned)."""
    th, tw = _pair(tile, "tile")
    sy, sx = _pair(stride, "stride")
    oys, oxs = tile_origins(Hc, th, sy), tile_origins(Wc, tw, sx)
    wy = torch.from_numpy(tile_window(th, window)).to(torch.float32)
    wx = torch.from_numpy(tile_window(tw, window)).to(torch.float32)
    sum_y, sum_x = np.zeros(int(Hc), dtype=np.float64), np.zeros(int(Wc), dtype=np.float64)
    for oy in oys:
        sum_y[oy:oy + th] += wy.double().numpy()
    for ox in oxs:
        sum_x[ox:ox + tw] += wx.double().numpy()
    inv_norm = torch.from_numpy(1.0 / np.outer(sum_y, sum_x)).to(torch.float32)
    origins = torch.tensor([[oy, ox] for oy in oys for ox in oxs], dtype=torch.int32).reshape(-1, 2)
    return origins, wy, wx, inv_norm


def extract_and_expand(array, time, target):
    a = torch.from_numpy(np.asarray(array)).to(target.device)[time].float()
    while a.ndim < target.ndim:
        a = a.unsqueeze(-1)
    return a.expand_as(target)


class _Chain:
    """What `_fused_loop` and `_tiled_loop` do alike for one chain: the host-only plan (`__init__`), then on the device (`open`) the
    chunks and engines of the network's inputs, the coefficient table with its device step counter and the library-noise seed, and
    per sub-step the coefficient fetch, the state update of a row block and the trace record; at the end the snapshots and the
    returned values.  What a loop does on its own (which noise it draws when, the tiles, the grouped walk) stays in the loop."""

    def __init__(self, diffusion, sample_pattern, kwargs, HW, record, record_every, ddim=False, mean_only=False):
        """The host-only plan of a chain over images of HW pixels.  It touches no device and draws nothing: everything it refuses
        is refused before an engine is built, a seed drawn or a kernel launched."""
        import os
        self.diffusion, self.kwargs, self.record, self.record_every, self.ddim = diffusion, kwargs, record, record_every, ddim
        T = diffusion.num_timesteps
        # optional sub-range of the chain (benchmarks / resumed chains): idx = first .. last, descending
        self.first, self.last = kwargs.get("index_range", (T - 1, 0))
        if not (0 <= self.last <= self.first <= T - 1):
            raise ValueError(f"index_range must satisfy 0 <= last <= first <= {T - 1}, got ({self.first}, {self.last})")
        self.sched = pcgs_schedule(sample_pattern, T)     # (an invalid pattern raises here)
        self.solver = diffusion.solver                    # a few-step solver as the state update (None: the class's own rule)
        solver_refusals(diffusion, sample_pattern, mean_only)
        self.solver_noisy = self.solver == "ddim" and diffusion.solver_eta > 0.0      # (S can be non-zero)
        if T > 1 << 16 and max(a for _, _, a in self.sched) > 1:
            raise ValueError("sub-steps need a chain of at most 65536 indices (the step counter word holds step | sub << 16)")
        self.noise_fn = kwargs.get("noise_fn", None)      # (k, shape) -> tensor : injected noise (parity runs)
        source = "fn" if self.noise_fn is not None else str(kwargs.get("noise", os.environ.get("OSM_STEP_NOISE", "library"))).lower()
        if source not in ("fn", "library", "aten"):
            raise ValueError(f"noise must be 'library' or 'aten', got {source!r}")
        if source == "library" and HW % 4 != 0:
            source = "aten"                               # (one Philox counter covers four consecutive elements of an image)
        self.source = source
        # q_sample's unused draw (reference :241) and, for 'ps', p_sample's draw before it: only meaningful on torch's generator
        self.draw_measurement_noise = kwargs.get("reference_rng_order", source == "aten") and source == "aten"
        # the update kernel draws the step noise itself (DDIM at eta = 0 adds none and osm_ddim_update_c takes a tensor for eta > 0;
        # the mean-only step adds none)
        self.lib_rng = source == "library" and not ddim and not mean_only
        self.trace = kwargs.get("trace", None)            # list collecting per-step tensors (tests)
        self.records = kwargs.get("record_out", [] if record else None)   # (idx, pred_xstart cpu) snapshots
        self.have_loss = False

    def open(self, model, n, h, w, dev, scale, clip, state_shape=None):
        """The device side, for n network inputs of h x w (independent chains, SURVEY.md F1/F2: a batch whose kept activations would
        not fit the device -- ~8 GB per 256 x 256 image in fp32 -- is walked in chunks per step, contiguous row blocks).  scale, clip:
        the conditioner's per-channel guidance scale [C] and gradient clip, used at the guided indices.  state_shape: the state's
        [B,C,H,W] where it is not the network inputs' (the canvas of a tiled chain): a solver's history has that shape."""
        sizes = self.diffusion.chunk_sizes(n, model.images_in_flight(n, h, w))
        self.chunks, c0 = [], 0
        for sz in sizes:
            self.chunks.append((c0, c0 + sz))
            c0 += sz
        self.engs = {}
        for sz in sorted(set(sizes), reverse=True):       # at most two sizes; the second call keeps the first engine alive
            self.engs[sz] = model.engine(sz, h, w, keep=tuple(self.engs.values()))
        self.eng = self.engs[sizes[0]]
        self.single = len(self.chunks) == 1
        self.scale, self.clip = scale, clip
        table = self.diffusion.coef_table()
        self.table = torch.from_numpy(table).to(dev)
        self.step = torch.tensor([self.first], device=dev, dtype=torch.int32)
        self.coef = torch.zeros(8, device=dev, dtype=torch.float32)
        self.dtable = self.dcoef = None
        if self.ddim:
            self.dtable = torch.from_numpy(self.diffusion.ddim_table(float(self.kwargs.get("eta", 0.0)))).to(dev)
            self.dcoef = torch.zeros(8, device=dev, dtype=torch.float32)
        self.stable = self.scoef = self.hist = None
        if self.solver is not None:   # rows [A, B0, B1, S, noise_on, 0, 0, t_model]; history starts empty at `first`
            rows = np.zeros((self.diffusion.num_timesteps, 8), dtype=np.float32)
            rows[:, 0:4] = solver_table(self.diffusion, self.solver, self.diffusion.solver_eta, first=self.first)
            rows[:, 4] = rows[:, 3] != 0
            rows[:, 7] = table[:, 7]
            self.stable = torch.from_numpy(rows).to(dev)
            self.scoef = torch.zeros(8, device=dev, dtype=torch.float32)
            # the previous index' processed x0 of every image of the state (the canvas's, for a tiled chain)
            self.hist = torch.empty(*(state_shape or (n, model.in_channels, h, w)), device=dev, dtype=torch.float32)
        self.seed = 0
        if self.source == "library":
            self.seed = self.kwargs.get("noise_seed")
            if self.seed is None:  # one draw per CHAIN from the device's generator (what torch.manual_seed seeds, and only device ops consume)
                self.seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, device=dev).item())

    def fetch(self, final):
        """The coefficients of this sub-step.  Every engine's timestep vector is filled from the SAME step counter; the counter moves
        once per index, in the last fetch of its last sub-step, which always goes through the first engine (stream order: the delta-0
        fetches read it before it moves)."""
        eng = self.eng
        for e2 in self.engs.values():
            if e2 is not eng:
                ops.fetch_coefs(self.table, self.step, 0, self.coef, e2.t_dev, e2.B)
        if self.ddim:
            ops.fetch_coefs(self.dtable, self.step, 0, self.dcoef, eng.t_dev, eng.B)
        if self.solver is not None:
            ops.fetch_coefs(self.stable, self.step, 0, self.scoef, eng.t_dev, eng.B)
        ops.fetch_coefs(self.table, self.step, -1 if final else 0, self.coef, eng.t_dev, eng.B)

    def update(self, a, b, g, dxu, noise, x_next, grad_out, noise_out, sub, final, img0, img_stride, rows=None):
        """x_next [Bc,C,H,W] = the state of one row block after this sub-step, from (a, b) = its (mean, log variance) -- for DDIM its
        (pred_xstart, x_t).  g, dxu: the data term's gradient and the network's dx, None at an unguided index (no scale, no clip);
        noise: the step noise as a tensor, or None (drawn in the kernel into noise_out if given; the mean-only step: none added).
        With a solver (a, b) = (pred_xstart, x_t) as for DDIM and rows = the block's rows of the state (None: all of it), whose
        history the same launch reads and renews; the noise is drawn in the kernel when the source is the library's stream and
        the rule can add any."""
        Bc, C, H, W = x_next.shape
        HW = H * W
        sc, cl = (None, -1.0) if g is None else (self.scale, self.clip)
        if self.solver is not None:
            hist = self.hist if rows is None else self.hist[rows[0]:rows[1]]
            if self.lib_rng and self.solver_noisy:
                ops.solver_update_rng_c(a, b, hist, g, dxu, self.coef, self.scoef, sc, cl, x_next, grad_out, noise_out, Bc, C, HW,
                                        self.seed, self.step, step_offset=1 if final else 0, sub=sub, img0=img0, img_stride=img_stride)
            else:
                ops.solver_update_c(a, b, hist, g, dxu, noise, self.coef, self.scoef, sc, cl, x_next, grad_out, noise_out, Bc, C, HW)
        elif self.ddim:
            ops.ddim_update_c(a, b, g, dxu, noise, self.coef, self.dcoef, sc, cl, x_next, grad_out, Bc, C, HW)
        elif self.lib_rng:                                # (+1 after the last sub-step's fetch: it moved the counter)
            ops.guide_update_rng_c(a, b, g, dxu, self.coef, sc, cl, x_next, grad_out, noise_out, Bc, C, HW, self.seed, self.step,
                                   step_offset=1 if final else 0, sub=sub, img0=img0, img_stride=img_stride)
        else:
            ops.guide_update_c(a, b, g, dxu, noise, self.coef, sc, cl, x_next, grad_out, Bc, C, HW)

    def trace_record(self, idx, sub, x_in, x0, mean, x_out, model_out, loss_all, phi, noise=None, q=None, grad=None):
        """One sub-step's entry of `trace=`; x_in: the state's clone from before the sub-step, model_out / grad: tensors of its own."""
        rec = dict(idx=idx, sub=sub, x_in=x_in, x0=x0.clone(), mean=mean.clone(), x_out=x_out.clone(), model_out=model_out,
                   loss=loss_all.clone() if self.have_loss else None, phi=None if phi is None else phi.clone(),
                   step=self.step.clone())                # (the device step counter after this sub-step)
        for key, v in (("noise", noise), ("q", q)):
            if v is not None:
                rec[key] = v.clone()
        if grad is not None:
            rec["grad"] = grad
        self.trace.append(rec)

    def snapshot(self, idx, x0):
        """pred_xstart during the chain (reference :308-327): same steps, one D2H copy each, after the index's last sub-step."""
        if self.records is not None and ((idx % self.record_every == 0) or idx == 0 or idx == 999):
            self.records.append((idx, x0.detach().cpu()))

    def finish(self, x_state, x0, loss_all, operator):
        """What the loop returns: the sample -- and with an operator (the Osmosis configuration) its variables, the last losses and
        pred_xstart; the rgb-guidance branch returns the sample only (:339-340)."""
        img = x_state.clone()
        if self.record and self.records:
            self.diffusion._save_process_grid(self.records, self.kwargs.get("save_grids_path"), self.kwargs.get("original_file_name"))
        if operator is None:
            return img
        variables = operator.optimize(freeze_phi=True)
        loss_np = loss_all.detach().cpu().numpy() if self.have_loss else None
        return img, variables, loss_np, x0.detach().cpu()


def _depth_prior_extras(depth_prior, x_start):
    """`p_sample_loop(depth_prior=)`: the range map lives on the image's grid; the setter's further keyword arguments."""
    zt = torch.as_tensor(depth_prior["z"])
    if tuple(zt.shape[-2:]) != tuple(x_start.shape[2:]):
        raise ValueError(f"depth_prior z {tuple(zt.shape)} does not match the image grid {tuple(x_start.shape[2:])}")
    return dict(batch=x_start.shape[0], device=x_start.device)


# The data-term options of a chain, in the order `p_sample_loop` applies them.  keyword -> (the conditioner's setter, the keys it takes
# from a chain (declared beside the setter), a key that must be there, the TypeError without the setter, the ValueError for anything but
# such a dict, a further check that returns the setter's extra keyword arguments).  `measurement_mask` is a tensor and keeps its own lines.
CHAIN_OPTIONS = {
    "gain_field": ("set_gain_field", PosteriorSamplingOsmosis.GAIN_FIELD_CHAIN_KEYS, None,
                   "gain_field needs a conditioner with set_gain_field (the 'osmosis' conditioning method)",
                   "gain_field must be a dict (grid, eta, n_iter, smooth, g_min, init, learn)", None),
    "robust": ("set_robust", ConditioningMethod.ROBUST_CHAIN_KEYS, None,
               "robust needs a conditioner with set_robust (a ConditioningMethod)",
               "robust must be a dict (loss, c, scale, sigma_min, per_pixel)", None),
    "depth_prior": ("set_depth_prior", PosteriorSamplingOsmosis.DEPTH_PRIOR_CHAIN_KEYS, "z",
                    "depth_prior needs a conditioner with set_depth_prior (the 'osmosis' conditioning method)",
                    "depth_prior must be a dict with the range map `z` (and confidence, weight, align, loss, scale, scale_min)",
                    _depth_prior_extras),
}


class GaussianDiffusion:
    def __init__(self, betas, model_mean_type, model_var_type, dynamic_threshold, clip_denoised,
                 rescale_timesteps, solver=None, solver_eta=0.0, **kwargs):
        """solver: None (the class's own step rule; nothing changes) or one of `SOLVERS` -- a few-step solver replaces the state
        update of every loop (`solver_table`); solver_eta: DDIM's eta (0: deterministic), 0 for dpmpp_2m."""
        self.solver, self.solver_eta = check_solver(solver, solver_eta)
        betas = np.array(betas, dtype=np.float64)
        self.betas = betas
        assert betas.ndim == 1, "betas must be 1-D"
        assert (0 < betas).all() and (betas <= 1).all(), "betas must be in (0..1]"
        self.num_timesteps = int(betas.shape[0])
        self.rescale_timesteps = rescale_timesteps
        alphas = 1.0 - betas
        self.alphas_cumprod = np.cumprod(alphas, axis=0)
        self.alphas_cumprod_prev = np.append(1.0, self.alphas_cumprod[:-1])
        self.alphas_cumprod_next = np.append(self.alphas_cumprod[1:], 0.0)
        self.sqrt_alphas_cumprod = np.sqrt(self.alphas_cumprod)
        self.sqrt_one_minus_alphas_cumprod = np.sqrt(1.0 - self.alphas_cumprod)
        self.log_one_minus_alphas_cumprod = np.log(1.0 - self.alphas_cumprod)
        self.sqrt_recip_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod)
        self.sqrt_recipm1_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod - 1)
        self.posterior_variance = betas * (1.0 - self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_log_variance_clipped = np.log(np.append(self.posterior_variance[1], self.posterior_variance[1:]))
        self.posterior_mean_coef1 = betas * np.sqrt(self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_mean_coef2 = (1.0 - self.alphas_cumprod_prev) * np.sqrt(alphas) / (1.0 - self.alphas_cumprod)
        self.mean_processor = get_mean_processor(model_mean_type, betas=betas, dynamic_threshold=dynamic_threshold,
                                                 clip_denoised=clip_denoised)
        self.var_processor = get_var_processor(model_var_type, betas=betas)
        self._fast = None

    # ------------------------------------------------------------------ reference tensor API
    def q_mean_variance(self, x_start, t):
        return (extract_and_expand(self.sqrt_alphas_cumprod, t, x_start) * x_start,
                extract_and_expand(1.0 - self.alphas_cumprod, t, x_start),
                extract_and_expand(self.log_one_minus_alphas_cumprod, t, x_start))

    def q_sample(self, x_start, t):
        noise = torch.randn_like(x_start)
        return (extract_and_expand(self.sqrt_alphas_cumprod, t, x_start) * x_start
                + extract_and_expand(self.sqrt_one_minus_alphas_cumprod, t, x_start) * noise)

    def q_posterior_mean_variance(self, x_start, x_t, t):
        assert x_start.shape == x_t.shape
        mean = (extract_and_expand(self.posterior_mean_coef1, t, x_start) * x_start
                + extract_and_expand(self.posterior_mean_coef2, t, x_t) * x_t)
        return (mean, extract_and_expand(self.posterior_variance, t, x_t),
                extract_and_expand(self.posterior_log_variance_clipped, t, x_t))

    def _scale_timesteps(self, t):
        if self.rescale_timesteps:
            return t.float() * (1000.0 / self.num_timesteps)
        return t

    def _model_timesteps(self, idx: int) -> float:
        """What the network is fed for loop index idx (base class: no respacing)."""
        return float(idx) * (1000.0 / self.num_timesteps) if self.rescale_timesteps else float(idx)

    def p_mean_variance(self, model, x, t):
        model_output = model(x, self._scale_timesteps(t))
        if model_output.shape[1] == 2 * x.shape[1]:
            model_output, model_var_values = torch.split(model_output, x.shape[1], dim=1)
        else:
            model_var_values = model_output
        mean, x0 = self.mean_processor.get_mean_and_xstart(x, t, model_output)
        var, logvar = self.var_processor.get_variance(model_var_values, t)
        assert mean.shape == logvar.shape == x0.shape == x.shape
        return {"mean": mean, "variance": var, "log_variance": logvar, "pred_xstart": x0}

    def p_sample(self, model, x, t):
        raise NotImplementedError

    # ------------------------------------------------------------------ fused (HIP) loop
    def _fast_path_ok(self, model, cond_fn, pretrain_model, rgb_guidance, sample_pattern, shape=None):
        """The conditioner whose step the fused loop implements, or None (-> `_generic_loop`).  Three configurations:
        the Osmosis one (pretrain_model 'osmosis', a 4 -> 8 network, 'osmosis' conditioning with gradient_x_prev, a physical
        operator), the rgb-guidance one (`rgb_guidance=True`: `DDPM.p_sample` / `DDIM.p_sample` + 'ps' conditioning on an identity
        operator with the gaussian noiser; gaussian_diffusion.py:231-232,296-302, condition_methods.py:234-251) and, for a
        3-channel network, the mean-only one (`rgb_guidance=False`, pretrain_model != 'osmosis': p_mean_variance, sample = mean,
        'ps' conditioning, no noise; :235-238, :298-306).  Networks: C = 3 or 4 input channels and C or 2 C output channels
        (create_model's 4 -> 8, 3 -> 6, 3 -> 3; a C -> C network goes with any variance processor, which then reads the
        network output itself, :349-355); OSM_FUSED_RGB=0 keeps 3-channel chains on `_generic_loop`.  shape: x_start's
        [B, C, H, W] (`dynamic_threshold` needs it)."""
        import os
        from .condition_methods import PosteriorSampling, PosteriorSamplingOsmosis
        from .unet import UNetModel
        cond = getattr(cond_fn, "__self__", None)
        if not isinstance(model, UNetModel):
            return None
        C = model.in_channels
        if C not in (3, 4) or model.out_channels not in (C, 2 * C):
            return None       # the step kernels serve [B,C,HW] with C in {3, 4} and a network output of C or 2 C channels
        if C == 3 and os.environ.get("OSM_FUSED_RGB", "1") == "0":
            return None
        if self.mean_processor.hip_kernel != "osm_posterior" or self.var_processor.hip_kernel != "osm_posterior":
            return None
        if self.mean_processor.dynamic_threshold:
            # the reference's quantile is taken over the WHOLE batch (util/img_utils.py:8-15): fused only when the batch runs as ONE
            # engine pass and within torch.quantile's 2^24 elements (a larger one raises in `_generic_loop`, as the reference does);
            # OSM_FUSED_DYNTHR=0 keeps such chains on `_generic_loop`
            if os.environ.get("OSM_FUSED_DYNTHR", "1") == "0" or shape is None:
                return None
            B, C, H, W = shape
            if B * C * H * W > ops.QUANTILE_MAX_N or len(self.chunk_sizes(B, model.images_in_flight(B, H, W))) != 1:
                return None
        if sample_pattern is not None and sample_pattern.get("pattern") != "original" and sample_pattern.get("local_M", 1) != 1:
            # the PCGS inner alternation runs as sub-steps of the fused loop; OSM_FUSED_PCGS=0 keeps such chains on `_generic_loop`
            if os.environ.get("OSM_FUSED_PCGS", "1") == "0":
                return None
        mean_only = pretrain_model != "osmosis" and not rgb_guidance
        if mean_only and C != 3:
            return None       # the reference's mean-only step (:234-236: p_mean_variance, sample = mean, no p_sample) on a 4-channel
            #                   network: `_generic_loop`; fused for the RGB model family only
        if rgb_guidance or mean_only:
            # the 'ps' step: only the two registered step rules, un-overridden, and a chain that is guided at every index (the
            # reference calls the conditioner at every step of these branches: an unguided index raises in its autograd.grad)
            if type(cond) is not PosteriorSampling or not cond.hip_ok(C):
                return None
            if mean_only:     # (p_mean_variance, not p_sample, is the step rule of this branch)
                if getattr(type(self), "p_mean_variance", None) not in (SpacedDiffusion.p_mean_variance,
                                                                        GaussianDiffusion.p_mean_variance):
                    return None
            elif getattr(type(self), "p_sample", None) not in (DDPM.p_sample, DDIM.p_sample):
                return None
            if sample_pattern is not None and not all(self._guidance_flag(sample_pattern, i) for i in (0, self.num_timesteps - 1)):
                return None
            return cond
        if not isinstance(cond, PosteriorSamplingOsmosis) or (C, model.out_channels) != (4, 8):
            return None
        if not cond.gradient_x_prev or not cond.hip_ok():       # (a third-party operator / auxiliary loss: autograd conditioning)
            return None
        return cond

    def coef_table(self) -> np.ndarray:
        """[T][8] fp32: c0,c1,c2,c3 (mean processor's `kernel_coefs`: c0 = d x0/d x, c1 = -d x0/d out, posterior_mean_coef1 / 2),
        the variance processor's two (learned_range: min_log, max_log; fixed_*: log variance, -), noise_on, t_model."""
        T = self.num_timesteps
        tab = np.zeros((T, 8), dtype=np.float32)
        for i in range(T):
            tab[i, 0:4] = self.mean_processor.kernel_coefs(i)
            tab[i, 4:6] = self.var_processor.kernel_coefs(i)
            tab[i, 6] = 0.0 if i == 0 else 1.0
            tab[i, 7] = self._model_timesteps(i)
        return tab

    def ddim_table(self, eta: float = 0.0) -> np.ndarray:
        """[T][8] fp32 rows of `DDIM.p_sample` (gaussian_diffusion.py:505-528) for osm_ddim_update:
        alpha_bar, alpha_bar_prev, eta, noise_on, sqrt_recip_ac, sqrt_recipm1_ac (predict_eps_from_x_start :533-536: the sampler's
        own tables, whatever the mean processor), -, t_model."""
        T = self.num_timesteps
        tab = np.zeros((T, 8), dtype=np.float32)
        tab[:, 0] = self.alphas_cumprod
        tab[:, 1] = self.alphas_cumprod_prev
        tab[:, 2] = eta
        tab[1:, 3] = 1.0
        tab[:, 4] = self.sqrt_recip_alphas_cumprod
        tab[:, 5] = self.sqrt_recipm1_alphas_cumprod
        tab[:, 7] = [self._model_timesteps(i) for i in range(T)]
        return tab

    @staticmethod
    def chunk_sizes(B: int, cap: int):
        """How a batch of B independent images is walked when at most `cap` fit the device at once: the fewest chunks n such
        that either all are equal (B % n == 0, ONE engine of B / n images) or the two sizes ceil(B / n) and floor(B / n)
        together stay within the cap (an engine owns its activation buffers, and a ragged walk keeps two engines).
        B = 37, cap = 32 -> [13, 12, 12] (rounds 1-2 fell back to 37 chunks of one image)."""
        cap = max(1, int(cap))
        n = -(-B // cap)
        while True:
            hi, lo = -(-B // n), B // n
            if B % n == 0:
                return [hi] * n
            if hi + lo <= cap:
                return [hi] * (B % n) + [lo] * (n - B % n)
            n += 1

    def _guidance_flag(self, sample_pattern, idx):
        return guidance_flag(sample_pattern, idx, self.num_timesteps)

    def _fused_loop(self, model, cond, x_start, measurement, sample_pattern, kwargs, record=False, record_every=150,
                    mean_only=False):
        """One device-resident step per index, for the Osmosis configuration and for the rgb-guidance ('ps') one (`_fast_path_ok`).
        Per-step noise (gaussian_diffusion.py:266-268 / :497 / :522): by default drawn INSIDE osm_guide_update_rng_c from the
        library's Philox-4x32-10 stream (seed: `noise_seed=`, else one draw per chain from the device's torch generator, so
        `torch.manual_seed` still fixes the chain); `noise="aten"` (or OSM_STEP_NOISE=aten) draws it with torch on the device in the reference's
        call order instead (the reference's own realisation for the same seed); `noise_fn=` injects it (parity runs).
        PCGS (`pcgs_schedule`): index idx runs alternate_len sub-steps at the same t, each a full step (network, posterior, conditioning
        with its own n_iter phi steps, noise) on the previous sub-step's x_t.  Only the last sub-step's fetch moves the step counter;
        noise_fn's k, the library stream's `sub` counter word and the trace count sub-steps; `record` snapshots (and the returned loss,
        phi, x0) are those after the index's last sub-step (:274, :309).
        mean_only: the mean-only 'ps' step (:235-238, :298-306): x_next = mean - scale grad at every index, no noise drawn or added
        (`noise="aten"` with reference_rng_order draws q_sample's only; noise_fn is not called).
        Channels: x_start [B,C,H,W] with the network's C; every step kernel is called through its channel-generic entry point
        (osm_*_c) with the chain's own (C, Cout) -- at (4, 8) bit-identical to the [B,4,HW] entry points, which remain for C callers.
        Shared water parameters (the operator's `phi_groups`): the images of a group are no longer independent in phi, so a guided
        sub-step runs every chunk's forward + posterior, then ONE data term over the whole batch (one phi step per group and inner
        iteration, osm_phys_optimize_g), then every chunk's backward + update.  With one chunk that is the ungrouped launch order
        with the grouped call in the data term's place; with more, each chunk's forward is re-run before its backward (the engine
        keeps one pass's activations): ONE EXTRA FORWARD per chunk per guided sub-step.  Ungrouped chains keep their launch sequence.
        The 'ps' branch takes the same walk for an operator with `couples_batch` (`blind_blur`: the learnt PSF is shared by the batch,
        so its step pools every image's tap gradient -- ONE `loss_grad_x0` over [0, B))."""
        from .condition_methods import PosteriorSampling
        ps = isinstance(cond, PosteriorSampling)
        ddim = self.solver is None and ps and not mean_only and getattr(type(self), "p_sample", None) is DDIM.p_sample
        dev = x_start.device
        B, C, H, W = x_start.shape
        Cout = model.out_channels
        if C != model.in_channels:
            raise ValueError(f"expected x_start [B,{model.in_channels},H,W], got {tuple(x_start.shape)}")
        HW = H * W
        T = self.num_timesteps
        # the loop drives the engine's plans directly and calls the network as model(x, t) (gaussian_diffusion.py:243): a
        # class-conditional network has no labels here -- the reference's forward asserts (unet.py:713-716); so does this path,
        # instead of replaying the plans with zero / stale label rows
        assert getattr(model, "num_classes", None) is None, "must specify y if and only if the model is class-conditional"
        ch = _Chain(self, sample_pattern, kwargs, HW, record, record_every, ddim=ddim, mean_only=mean_only)
        # ---- everything above is host-side; from here on the device is used
        ch.open(model, B, H, W, dev, cond.scale4(dev, C) if ps else cond.scale4(dev), -1.0 if ps else cond.clip_value)
        chunks, engs, eng, single, coef = ch.chunks, ch.engs, ch.eng, ch.single, ch.coef
        source, lib_rng, noise_fn, trace = ch.source, ch.lib_rng, ch.noise_fn, ch.trace
        f32 = dict(device=dev, dtype=torch.float32)
        x0, mean, logvar = (torch.empty(B, C, H, W, **f32) for _ in range(3))
        # `clip_denoised: True` (configs/rgb_guidance_sample_config.yaml; posterior_mean_variance.py:43-50): x0 is clamped inside
        # osm_posterior_c, the unclamped prediction is kept for the clamp's backward (osm_clamp_bwd masks d loss / d x0)
        # `dynamic_threshold: True` (util/img_utils.py:8-15): x0 = clip(x0_raw * quantile(|x0_raw|, 0.98), -1, 1) over the whole batch
        # (osm_posterior_dynthr_c; q and its order statistics stay on the device for osm_dynthr_bwd); `_fast_path_ok` guarantees one chunk
        dyn = bool(self.mean_processor.dynamic_threshold)
        x0_raw = torch.empty(B, C, H, W, **f32) if (self.mean_processor.clip_denoised or dyn) else None
        q_dev = None
        if dyn:
            assert single, "dynamic_threshold couples every image: the fused loop takes it in one engine pass only"
            q_dev, q_idx = torch.zeros(1, **f32), torch.zeros(2, device=dev, dtype=torch.int32)
            q_ws = ops.quantile_workspace(B * C * HW, dev)
        g = torch.empty(B, C, H, W, **f32)
        loss_all = torch.zeros(B, **f32)
        y = measurement.detach().to(dev, torch.float32).contiguous()
        # the chain's batch: the mask rows [B,3,hw] on the measurement's grid (the image's, except for a downsampling operator of the
        # 'ps' branch) and the robust / depth-prior / gain-field state at its initial values; the data term takes chunks by `rows=`
        cond.open_batch(B, (H, W), tuple(y.shape[2:]) if y.dim() == 4 else (H, W), dev)
        phi = None if ps else cond.operator.phi
        # a data term that couples the images of the batch: shared water parameters, or on the 'ps' branch an operator with
        # `couples_batch` (`blind_blur`: one learnt PSF for all images)
        grouped = (not ps and getattr(cond.operator, "group_sizes", None) is not None) or \
            (ps and bool(getattr(cond.operator, "couples_batch", False)))
        x_state = eng.x_in if single else torch.empty(B, C, H, W, **f32)
        x_state.copy_(x_start.detach())
        shared = bool(kwargs.get("shared_noise", False)) and B > 1   # every image receives the SAME noise (separately seeded batch-1 runs)
        img_base, img_stride = int(kwargs.get("image_index0", 0)), 0 if shared else 1
        noise = None if (lib_rng or mean_only) else torch.zeros(B, C, H, W, **f32)
        noise1 = torch.zeros(1, C, H, W, **f32) if (shared and source == "aten" and not mean_only) else None
        noise_used = torch.empty(B, C, H, W, **f32) if (lib_rng and trace is not None) else None
        mk, vk = self.mean_processor.kernel_kind, self.var_processor.kernel_kind
        k = 0                                             # sub-step count (noise_fn's k)
        for idx in range(ch.first, ch.last - 1, -1):
            guided, freeze, alt = ch.sched[T - 1 - idx]
            if ps:
                guided, freeze = True, False
            for sub in range(alt):
                final = sub == alt - 1
                if mean_only:                             # no step noise; the reference's only draw per call is q_sample's (:241)
                    if ch.draw_measurement_noise:
                        torch.randn_like(y[:1] if shared else y)
                elif source == "fn":
                    noise.copy_(noise_fn(k, noise.shape))
                elif source == "aten":
                    if ps:                                # DDPM / DDIM.p_sample draw first (:497, :522), then q_sample (:241)
                        noise1.normal_() if noise1 is not None else noise.normal_()
                    if ch.draw_measurement_noise:
                        torch.randn_like(y[:1] if noise1 is not None else y)
                    if not ps:
                        noise1.normal_() if noise1 is not None else noise.normal_()
                    if noise1 is not None:
                        noise.copy_(noise1.expand_as(noise))
                elif not lib_rng:                         # library stream, DDIM: as a tensor (used only for eta > 0)
                    ops.randn_sub(noise, B, C * HW, ch.seed, step=ch.step, sub=sub, img0=img_base,
                                  img_stride=img_stride)  # (before the fetch: counter = idx)
                ch.fetch(final)
                if trace is not None:
                    x_in = x_state.clone()
                    grad_all = torch.empty_like(g) if guided else None
                    model_out = torch.empty(B, eng.out.shape[1], H, W, **f32)
                # what this sub-step does, in launch order.  Independent chains: chunk by chunk forward -> data term -> backward -> update.
                # Shared water parameters (the operator's `phi_groups`): a group's phi step pools its members, so (a) every chunk's forward
                # + posterior into the [B]-sized x0 / mean / logvar, (b) ONE data term over the whole batch, (c) per chunk backward +
                # update -- with more than one chunk after re-running its forward (the engine's activations are the last chunk's by then)
                if grouped and guided:
                    walk = [("fwd", c) for c in chunks] + [("data", (0, B))]
                    for c in chunks:
                        walk += ([] if single else [("refwd", c)]) + [("upd", c)]
                else:
                    walk = []
                    for c in chunks:
                        walk += [("fwd", c)] + ([("data", c)] if guided else []) + [("upd", c)]
                for act, (c0, c1) in walk:
                    if act == "data":
                        if ps:
                            cond.loss_grad_x0(x0[c0:c1], y[c0:c1], g_out=g[c0:c1], loss_out=loss_all[c0:c1], rows=(c0, c1))
                        else:
                            cond.loss_grad_x0(x0[c0:c1], y[c0:c1], freeze_phi=freeze, g_out=g[c0:c1], loss_out=loss_all[c0:c1],
                                              rows=(c0, c1))
                        ch.have_loss = True
                        continue
                    ce, Bc = engs[c1 - c0], c1 - c0        # this chunk's engine (`eng` stays the first one)
                    if act == "refwd":
                        ce.x_in.copy_(x_state[c0:c1])
                        ce.run_forward()
                        continue
                    if act == "fwd":
                        if not single:
                            ce.x_in.copy_(x_state[c0:c1])
                        ce.run_forward()
                        if dyn:
                            ops.posterior_dynthr_c(ce.out, ce.x_in, coef, x0, mean, logvar, x0_raw, q_dev, q_idx, q_ws, Bc, C, Cout, HW,
                                                   mk, vk, DYNAMIC_THRESHOLD_S)
                        else:
                            ops.posterior_c(ce.out, ce.x_in, coef, x0[c0:c1], mean[c0:c1], logvar[c0:c1], Bc, C, Cout, HW, mk, vk,
                                            None if x0_raw is None else x0_raw[c0:c1])
                        if trace is not None:
                            model_out[c0:c1].copy_(ce.out)
                        continue
                    gg = dxu = grad_out = None
                    if guided:
                        if dyn:                           # (a clip_denoised clamp after it masks nothing more)
                            ops.dynthr_bwd(g, x0_raw, q_dev, q_idx, q_ws, DYNAMIC_THRESHOLD_S)
                        elif x0_raw is not None:
                            ops.clamp_bwd(g[c0:c1], x0_raw[c0:c1])
                        ops.posterior_bwd_c(g[c0:c1], coef, ce.d_out, Bc, C, Cout, HW)
                        ce.run_backward()
                        gg, dxu = g[c0:c1], ce.dx
                        grad_out = grad_all[c0:c1] if trace is not None else None
                    a, b = (x0[c0:c1], ce.x_in) if (ddim or ch.solver is not None) else (mean[c0:c1], logvar[c0:c1])
                    ch.update(a, b, gg, dxu, None if noise is None else noise[c0:c1], x_state[c0:c1], grad_out,
                              None if noise_used is None else noise_used[c0:c1], sub, final,
                              img_base + (0 if shared else c0), img_stride, rows=(c0, c1))
                if trace is not None:
                    ch.trace_record(idx, sub, x_in, x0, mean, x_state, model_out, loss_all, phi, noise_used, q_dev, grad_all)
                k += 1
            ch.snapshot(idx, x0)
        return ch.finish(x_state, x0, loss_all, None if ps else cond.operator)

    def _tiled_loop(self, model, cond_fn, x_start, measurement, pretrain_model, rgb_guidance, sample_pattern, kwargs, tiling,
                    record=False, record_every=150):
        """Tiled sampling (MultiDiffusion) of ONE canvas x_start [1,4,Hc,Wc] larger than the network's grid, Osmosis configuration.
        At every sub-step the network sees the n overlapping tiles of `tile_grid` as engine batches (`chunk_sizes` of n); the
        per-tile outputs are blended per pixel (window weights / their sum) into one canvas-sized network output, and everything
        else -- posterior, the physical model with its ONE phi, the mask, the auxiliary losses, clip_denoised, the guidance update,
        the step noise -- acts on the canvas exactly as `_fused_loop` does on an image (B = 1, HW = Hc Wc).  The guidance gradient
        goes back through the blend: the canvas d_out is gathered with the same weights (the blend's adjoint) into every tile's
        data-gradient pass and the per-tile dx are summed into the canvas dx.  The engine keeps one pass's activations, so with
        more than one chunk the forward of a chunk is re-run before its data-gradient pass.
        Never `_generic_loop` (the network on the whole canvas is another computation): what this loop does not carry raises
        NotImplementedError naming the option; a bad tiling raises ValueError before anything launches."""
        from .condition_methods import PosteriorSamplingOsmosis
        from .unet import UNetModel
        th, tw, sy, sx, window = parse_tiling(tiling)
        if rgb_guidance:
            raise NotImplementedError("tiling: rgb_guidance (the 'ps' branch) is not tiled")
        if getattr(getattr(getattr(cond_fn, "__self__", None), "operator", None), "degradation", None) is not None:
            raise NotImplementedError("tiling: a degradation inside the physical operator is not tiled")
        if getattr(getattr(getattr(cond_fn, "__self__", None), "operator", None), "group_sizes", None) not in (None, (1,)):
            raise NotImplementedError("tiling: phi_groups (water parameters shared across photos) is not tiled -- a tiled chain is one "
                                      "canvas with its one phi")
        if pretrain_model != "osmosis":
            raise NotImplementedError(f"tiling: pretrain_model={pretrain_model!r} (the mean-only branch) is not tiled")
        if getattr(type(self), "p_sample", None) is DDIM.p_sample:
            raise NotImplementedError("tiling: the ddim sampler is not tiled")
        if self.mean_processor.dynamic_threshold:
            raise NotImplementedError("tiling: dynamic_threshold is not tiled (its quantile couples the whole canvas)")
        if x_start.dim() != 4 or x_start.shape[0] != 1:
            raise NotImplementedError(f"tiling: one canvas per call (batch {tuple(x_start.shape)[0]} > 1 is not tiled)")
        if not isinstance(model, UNetModel) or (model.in_channels, model.out_channels) != (4, 8):
            raise NotImplementedError("tiling: only the 4 -> 8 (RGBD, learned variance) network is tiled")
        _, C, Hc, Wc = x_start.shape
        if C != 4 or tuple(measurement.shape) != (1, 3, Hc, Wc):
            raise ValueError(f"tiling: expected x_start [1,4,Hc,Wc] and measurement [1,3,Hc,Wc], got {tuple(x_start.shape)} and "
                             f"{tuple(measurement.shape)}")
        origins, wy, wx, inv_norm = tile_grid(Hc, Wc, (th, tw), (sy, sx), window)      # (ValueError: tile > canvas, stride, window)
        div = 1 << (len(model.channel_mult) - 1)
        if th % div or tw % div:
            raise ValueError(f"tiling: the network needs tile sides divisible by {div}, got {th} x {tw}")
        cond = self._fast_path_ok(model, cond_fn, pretrain_model, rgb_guidance, sample_pattern, tuple(x_start.shape))
        if not isinstance(cond, PosteriorSamplingOsmosis):
            raise NotImplementedError("tiling: this configuration has no fused step (conditioner / operator / processors the HIP "
                                      "loop has no kernels for, or a fused path switched off), and the generic loop is not tiled")
        assert getattr(model, "num_classes", None) is None, "must specify y if and only if the model is class-conditional"
        dev = x_start.device
        HW, T, n = Hc * Wc, self.num_timesteps, origins.shape[0]
        ch = _Chain(self, sample_pattern, kwargs, HW, record, record_every)
        # ---- everything above is host-side; from here on the device is used
        ch.open(model, n, th, tw, dev, cond.scale4(dev), cond.clip_value, state_shape=(1, 4, Hc, Wc))
        chunks, engs, eng, single, coef, trace = ch.chunks, ch.engs, ch.eng, ch.single, ch.coef, ch.trace
        f32 = dict(device=dev, dtype=torch.float32)
        org, wy, wx, inv_norm = origins.to(dev), wy.to(dev), wx.to(dev), inv_norm.to(dev).contiguous()
        weights = (wy, wx, inv_norm)
        x_state = x_start.detach().to(**f32).clone().contiguous()
        x0, mean, logvar, g, dx = (torch.empty(1, 4, Hc, Wc, **f32) for _ in range(5))
        model_out = torch.empty(1, 8, Hc, Wc, **f32)
        d_out = torch.empty(1, 8, Hc, Wc, **f32)
        out_tiles = None if single else torch.empty(n, 8, th, tw, **f32)
        dx_tiles = None if single else torch.empty(n, 4, th, tw, **f32)
        x0_raw = torch.empty(1, 4, Hc, Wc, **f32) if self.mean_processor.clip_denoised else None
        loss_all = torch.zeros(1, **f32)
        y = measurement.detach().to(dev, torch.float32).contiguous()
        # a batch of ONE canvas: the mask, the robust weights (one sigma), the depth prior (one fit) and the gain field are over it
        cond.open_batch(1, (Hc, Wc), (Hc, Wc), dev)
        phi = cond.operator.phi
        img_base = int(kwargs.get("image_index0", 0))
        noise = None if ch.lib_rng else torch.zeros(1, 4, Hc, Wc, **f32)      # the noise belongs to the canvas
        noise_used = torch.empty(1, 4, Hc, Wc, **f32) if (ch.lib_rng and trace is not None) else None
        mk, vk = self.mean_processor.kernel_kind, self.var_processor.kernel_kind

        def forward_chunk(ce, a, b):
            ops.tile_gather(x_state, ce.x_in, org[a:b])
            ce.run_forward()
        k = 0
        for idx in range(ch.first, ch.last - 1, -1):
            guided, freeze, alt = ch.sched[T - 1 - idx]
            for sub in range(alt):
                final = sub == alt - 1
                if ch.source == "fn":
                    noise.copy_(ch.noise_fn(k, noise.shape))
                elif ch.source == "aten":
                    if ch.draw_measurement_noise:
                        torch.randn_like(y)
                    noise.normal_()
                ch.fetch(final)
                if trace is not None:
                    x_in = x_state.clone()
                for a, b in chunks:
                    ce = engs[b - a]
                    forward_chunk(ce, a, b)
                    if not single:
                        out_tiles[a:b].copy_(ce.out)
                ops.tile_blend(eng.out if single else out_tiles, model_out, org, *weights)
                ops.posterior_c(model_out, x_state, coef, x0, mean, logvar, 1, 4, 8, HW, mk, vk, x0_raw)
                gg = dxu = grad_out = None
                if guided:
                    cond.loss_grad_x0(x0, y, freeze_phi=freeze, g_out=g, loss_out=loss_all)
                    ch.have_loss = True
                    if x0_raw is not None:
                        ops.clamp_bwd(g, x0_raw)
                    ops.posterior_bwd_c(g, coef, d_out, 1, 4, 8, HW)
                    for a, b in chunks:
                        ce = engs[b - a]
                        if not single:                    # this engine's activations are another chunk's by now
                            forward_chunk(ce, a, b)
                        ops.tile_gather(d_out, ce.d_out, org[a:b], *weights)
                        ce.run_backward()
                        if not single:
                            dx_tiles[a:b].copy_(ce.dx)
                    ops.tile_blend(eng.dx if single else dx_tiles, dx, org)
                    gg, dxu = g, dx
                    grad_out = torch.empty_like(g) if trace is not None else None
                a, b = (mean, logvar) if ch.solver is None else (x0, x_state)
                ch.update(a, b, gg, dxu, noise, x_state, grad_out, noise_used, sub, final, img_base, 1)
                if trace is not None:
                    ch.trace_record(idx, sub, x_in, x0, mean, x_state, model_out.clone(), loss_all, phi, noise_used, grad=grad_out)
                k += 1
            ch.snapshot(idx, x0)
        return ch.finish(x_state, x0, loss_all, cond.operator)

    @staticmethod
    def _save_process_grid(records, save_grids_path, original_file_name):
        """`<name>_process.png` of the reference (:308-333): clipped RGB of image 0 on the first row, the
        percentile-normalised viridis depth on the second, one column per recorded step (2-pixel padding, as
        torchvision.utils.make_grid lays it out)."""
        if save_grids_path is None:
            return None
        import os

        from PIL import Image
        rgb = [torch.clamp(0.5 * (x0[0, 0:3] + 1), 0, 1) for _, x0 in records]
        dep = [utilso.depth_tensor_to_color_image(
            utilso.min_max_norm_range_percentile(x0[:, 3], percent_low=0.05, percent_high=0.99)) for _, x0 in records]
        dep = [d.reshape(3, *d.shape[-2:]) for d in dep]
        # torchvision.utils.make_grid(rgb + depth, nrow=len(rgb)) -> tvtf.to_pil_image (:330-333): the stack is float64 (the viridis
        # depth), the background 0, and to_pil_image TRUNCATES (pic.mul(255).byte())
        from .. import sampling
        arr = sampling._to_pil_u8(sampling.make_grid(rgb + dep, nrow=len(rgb)))
        path = os.path.join(save_grids_path, f"{original_file_name}_process.png")
        Image.fromarray(arr).save(path)
        return path

    # ------------------------------------------------------------------ public loop
    def p_sample_loop(self, model, x_start, measurement, measurement_cond_fn, record, save_root,
                      pretrain_model=None, image_idx=None, record_every=150, rgb_guidance=False,
                      sample_pattern=None, measurement_mask=None, tiling=None, depth_prior=None, robust=None, gain_field=None,
                      **kwargs):
        """measurement_mask: a per-pixel validity mask of the measurement ([B,3,H,W], [B,1,H,W], [1,3,H,W] or [1,1,H,W] in
        [0, 1]; `ConditioningMethod.set_measurement_mask`), handed to the conditioner for this chain -- the fused loop and
        `_generic_loop` alike; None: the conditioner keeps whatever mask it was given directly (none by default).
        tiling: `dict(tile=, stride=, window=)` (`parse_tiling`) runs ONE canvas larger than the network's grid as overlapping
        tiles of the network's size (`_tiled_loop`); None: nothing changes.
        depth_prior: `dict(z=, confidence=, weight=, align=, loss=, scale=, scale_min=)` sets a range-map depth prior on the
        conditioner for this chain (`PosteriorSamplingOsmosis.set_depth_prior`; z on the image's grid, the canvas's when tiled);
        None: the conditioner keeps whatever prior it was given directly (none by default).
        robust: `dict(loss=, c=, scale=, sigma_min=, per_pixel=)` makes the data term robust for this chain
        (`ConditioningMethod.set_robust`; on a tiled canvas the weights are over the whole canvas, with one sigma); None: the
        conditioner keeps whatever setting it was given directly (none by default).
        gain_field: `dict(grid=, eta=, n_iter=, smooth=, g_min=, init=, learn=)` puts a learnt vignetting gain field into the Osmosis
        data term for this chain (`PosteriorSamplingOsmosis.set_gain_field`; on a tiled canvas one field over the canvas), its state
        starting afresh; None: the conditioner keeps whatever setting it was given directly (none by default).
        The three dicts go through one walk over `CHAIN_OPTIONS` -- gain field (and the opening of its state), robust, depth prior,
        in that order, then the mask: a conditioner without the setter is a TypeError, anything but a dict of the keys declared
        beside the setter a ValueError, before the setter runs."""
        from .posterior_mean_variance import PreviousXMeanProcessor
        cond_obj = getattr(measurement_cond_fn, "__self__", None)
        for name, value in (("gain_field", gain_field), ("robust", robust), ("depth_prior", depth_prior)):
            if value is not None:
                setter, keys, required, needs, must_be, extras = CHAIN_OPTIONS[name]
                if not hasattr(cond_obj, setter):
                    raise TypeError(needs)
                if not isinstance(value, dict) or (required is not None and required not in value):
                    raise ValueError(must_be)
                unknown = set(value) - set(keys)
                if unknown:
                    raise ValueError(f"{name}: unknown keys {sorted(unknown)}")
                getattr(cond_obj, setter)(**value, **({} if extras is None else extras(value, x_start)))
            if name == "gain_field" and getattr(cond_obj, "_gain", None) is not None:
                # the per-batch state at its initial values (`gain_values` reads them until the first guided sub-step); refusals first
                phi_all = getattr(cond_obj.operator, "phi", None)       # (a third-party operator keeps its parameters elsewhere)
                cond_obj.gain_open(x_start.shape[0] if phi_all is None else phi_all.shape[0], x_start.shape[2], x_start.shape[3],
                                   x_start.device)
        if measurement_mask is not None:
            if not hasattr(cond_obj, "set_measurement_mask"):
                raise TypeError("measurement_mask needs a conditioner with set_measurement_mask (a ConditioningMethod)")
            if tuple(measurement_mask.shape[2:]) != tuple(measurement.shape[2:]):
                raise ValueError(f"measurement_mask {tuple(measurement_mask.shape)} does not match the measurement's grid "
                                 f"{tuple(measurement.shape[2:])} (the image grid, or a downsampling operator's own)")
            cond_obj.set_measurement_mask(measurement_mask, batch=x_start.shape[0], device=x_start.device)
        if isinstance(self.mean_processor, PreviousXMeanProcessor) and not (
                rgb_guidance and getattr(type(self), "p_sample", None) is DDIM.p_sample):
            # Error behaviour of the reference: `previous_x` hands the network's split output on AS the mean
            # (posterior_mean_variance.py:68-72), and every step rule except DDIM.p_sample then adds to it in place
            # (gaussian_diffusion.py:268 / :499, condition_methods.py:223 / :249) -- autograd refuses that on a multi-output view.
            raise RuntimeError("Output 0 of SplitBackward0 is a view and is being modified inplace: the 'previous_x' mean processor "
                               "only runs with the DDIM sampler on the rgb-guidance branch (as in the reference)")
        if record and x_start.shape[1] < 4:
            # the reference's record branch reads the depth channel of pred_xstart (gaussian_diffusion.py:319) and fails there
            raise IndexError(f"index 3 is out of bounds for dimension 1 with size {x_start.shape[1]}: record=True snapshots the "
                             "depth channel of pred_xstart, which a 3-channel (RGB) chain does not have (as in the reference)")
        if tiling is not None:
            return self._tiled_loop(model, measurement_cond_fn, x_start, measurement, pretrain_model, rgb_guidance, sample_pattern,
                                    kwargs, tiling, record=record, record_every=record_every)
        cond = self._fast_path_ok(model, measurement_cond_fn, pretrain_model, rgb_guidance, sample_pattern, tuple(x_start.shape))
        if cond is not None:
            return self._fused_loop(model, cond, x_start, measurement, sample_pattern, kwargs, record=record,
                                    record_every=record_every, mean_only=pretrain_model != "osmosis" and not rgb_guidance)
        return self._generic_loop(model, x_start, measurement, measurement_cond_fn, pretrain_model,
                                  rgb_guidance, sample_pattern, kwargs, record=record, record_every=record_every)

    def _generic_loop(self, model, x_start, measurement, cond_fn, pretrain_model, rgb_guidance, sample_pattern,
                      kwargs, record=False, record_every=150):
        """Third-party conditioners / operators / processors the fused loop has no kernels for: the reference's control flow
        (gaussian_diffusion.py:213-340) over `p_mean_variance` / `p_sample` with torch.autograd through the HIP UNet operator.
        `record=True` snapshots pred_xstart at the reference's indices (:308-327) here as well.
        With a solver the step rule is `solver_table`'s row applied to torch tensors: the sample handed to the conditioner is the
        deterministic part A x + B0 x0 + B1 x0_prev (the history lives in this loop), and S z is added where the ancestral
        noise was (Osmosis branch: after the conditioner; rgb-guidance branch: in `p_sample`'s place, z drawn there)."""
        solver_refusals(self, sample_pattern, pretrain_model != "osmosis" and not rgb_guidance)
        stab = None if self.solver is None else solver_table(self, self.solver, self.solver_eta).astype(np.float32)
        hist = None
        img = x_start
        device = x_start.device
        T = self.num_timesteps
        loss = variable_dict = out = None
        records = kwargs.get("record_out", [] if record else None)
        osmosis = pretrain_model == "osmosis" and not rgb_guidance
        for idx in range(T - 1, -1, -1):
            time = torch.tensor([idx] * img.shape[0], device=device)
            guided = self._guidance_flag(sample_pattern, idx) if sample_pattern is not None else True
            alt = utilso.set_alternate_length(sample_pattern, idx, T) if sample_pattern is not None else 1
            for _ in range(alt):
                img = img.detach().requires_grad_(bool(guided))
                if stab is not None:
                    A, B0, B1, S = (float(v) for v in stab[idx])
                    out = self.p_mean_variance(model=model, x=img, t=time)
                    det = A * img + B0 * out["pred_xstart"]
                    if B1 != 0.0:
                        det = det + B1 * hist
                    hist = out["pred_xstart"].detach()
                    if rgb_guidance:
                        z = torch.randn_like(img)          # drawn at every index, as `p_sample` does
                        det = det + S * z if S != 0.0 else det
                    out["sample"] = det
                elif rgb_guidance:
                    out = self.p_sample(x=img, t=time, model=model)
                else:
                    out = self.p_mean_variance(model=model, x=img, t=time)
                    out["sample"] = out["mean"]
                noisy_measurement = self.q_sample(measurement, t=time)
                if not osmosis:
                    img, loss = cond_fn(x_t=out["sample"], measurement=measurement, noisy_measurement=noisy_measurement,
                                        x_prev=img, x_0_hat=out["pred_xstart"])
                    img = img.detach()
                    continue
                if guided:
                    img, loss, variable_dict, _grads, _aux = cond_fn(
                        x_t=out["sample"], measurement=measurement, noisy_measurement=noisy_measurement, x_prev=img,
                        x_0_hat=out["pred_xstart"], freeze_phi=utilso.is_freeze_phi(sample_pattern, idx, T),
                        time_index=float(idx) / T)
                else:
                    img = out["sample"]
                noise = torch.randn_like(img)
                img = img.detach()
                if stab is not None:
                    if S != 0.0:
                        img = img + S * noise
                elif idx != 0:
                    img = img + torch.exp(0.5 * out["log_variance"].detach()) * noise
            if records is not None and ((idx % record_every == 0) or idx == 0 or idx == 999):
                records.append((idx, out["pred_xstart"].detach().cpu()))
        if record and records:
            self._save_process_grid(records, kwargs.get("save_grids_path"), kwargs.get("original_file_name"))
        if osmosis:
            return img, variable_dict, loss, out["pred_xstart"].detach().cpu()
        return img


class SpacedDiffusion(GaussianDiffusion):
    def __init__(self, use_timesteps, **kwargs):
        self.use_timesteps = set(use_timesteps)
        self.timestep_map = []
        self.original_num_steps = len(kwargs["betas"])
        base_ac = np.cumprod(1.0 - np.array(kwargs["betas"], dtype=np.float64), axis=0)
        last, new_betas = 1.0, []
        for i, ac in enumerate(base_ac):
            if i in self.use_timesteps:
                new_betas.append(1 - ac / last)
                last = ac
                self.timestep_map.append(i)
        kwargs["betas"] = np.array(new_betas)
        super().__init__(**kwargs)

    def _model_timesteps(self, idx: int) -> float:
        t = float(self.timestep_map[idx])
        return t * (1000.0 / self.original_num_steps) if self.rescale_timesteps else t

    def p_mean_variance(self, model, *args, **kwargs):
        return super().p_mean_variance(self._wrap_model(model), *args, **kwargs)

    def _wrap_model(self, model):
        if isinstance(model, _WrappedModel):
            return model
        return _WrappedModel(model, self.timestep_map, self.rescale_timesteps, self.original_num_steps)

    def _scale_timesteps(self, t):
        return t   # done by the wrapped model


class _WrappedModel:
    def __init__(self, model, timestep_map, rescale_timesteps, original_num_steps):
        self.model = model
        self.timestep_map = timestep_map
        self.rescale_timesteps = rescale_timesteps
        self.original_num_steps = original_num_steps

    def __call__(self, x, ts, **kwargs):
        map_tensor = torch.tensor(self.timestep_map, device=ts.device, dtype=ts.dtype)
        new_ts = map_tensor[ts]
        if self.rescale_timesteps:
            new_ts = new_ts.float() * (1000.0 / self.original_num_steps)
        return self.model(x, new_ts, **kwargs)


@register_sampler(name="ddpm")
class DDPM(SpacedDiffusion):
    """Ancestral step (reference :492-502).  In the fused loop it IS osm_guide_update_c / osm_guide_update_rng_c (the row's
    `noise_on` switches the noise off at index 0); `p_sample` is the same row applied to torch tensors, for conditioners the
    fused loop has no kernels for (`_generic_loop`, autograd through `pred_xstart`)."""

    def p_sample(self, model, x, t):
        out = self.p_mean_variance(model, x, t)
        z = torch.randn_like(x)                            # drawn at every index (the reference's RNG order), used when noise_on
        noise_on = int(t[0]) != 0
        sample = out["mean"] + torch.exp(0.5 * out["log_variance"]) * z if noise_on else out["mean"]
        return {"sample": sample, "pred_xstart": out["pred_xstart"]}


@register_sampler(name="ddim")
class DDIM(SpacedDiffusion):
    """DDIM step (reference :505-535, Song et al. eq. 12).  In the fused loop it IS osm_ddim_update_c fed by `ddim_table`;
    `p_sample` applies the same fp32 row scalars to torch tensors (`_generic_loop`)."""

    def step_scalars(self, idx: int, eta: float = 0.0):
        """fp32 scalars of index idx in the kernel's operation order: (sqrt_recip_ac, sqrt_recipm1_ac, sqrt(ab_prev),
        sqrt(1 - ab_prev - sigma^2), sigma)."""
        f = np.float32
        ab, abp = f(self.alphas_cumprod[idx]), f(self.alphas_cumprod_prev[idx])
        sigma = f(eta) * np.sqrt((f(1) - abp) / (f(1) - ab)) * np.sqrt(f(1) - ab / abp)
        return (f(self.sqrt_recip_alphas_cumprod[idx]), f(self.sqrt_recipm1_alphas_cumprod[idx]), np.sqrt(abp),
                np.sqrt(f(1) - abp - sigma * sigma), sigma)

    def p_sample(self, model, x, t, eta=0.0):
        out = self.p_mean_variance(model, x, t)
        idx = int(t[0])
        c0, c1, sa, sb, sigma = (float(v) for v in self.step_scalars(idx, eta))
        x0 = out["pred_xstart"]
        z = torch.randn_like(x)                            # drawn at every index (the reference's RNG order)
        sample = x0 * sa + sb * ((c0 * x - x0) / c1)
        if idx != 0:
            sample = sample + sigma * z
        return {"sample": sample, "pred_xstart": x0}

    def predict_eps_from_x_start(self, x_t, t, pred_xstart):
        c0, c1 = (float(v) for v in self.step_scalars(int(t[0]))[:2])
        return (c0 * x_t - pred_xstart) / c1
