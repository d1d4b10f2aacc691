"""Hot-path drivers (reference: CWFA.py): z sampling (:47-64), the forward pyramid + NLL evaluation
(``evaluate_INN_forward`` :134-196), the per-volume inverse loop (:865-924) and the training-time NLL (:966-978),
plus the batch-sharded multi-GPU NLL (new; the reference is single-device).

The evaluation block behind every reconstructed volume (CWFA.py:1032-1117) is at the end of this file: step metrics
(``compute_INN_step_performance`` :98-132, fused as ``evaluate_step``) and the neuron traces (``corr_coeff_3D`` :240-379).

Out of scope: experiment management of ``run_CWFA`` -- checkpoint discovery, optimisers,
TensorBoard, figures, TIFF export.
"""
import math
from collections import namedtuple

import torch

from . import ops
from .amp import amp_function, amp_region
from .XLFMDataset import _estimate, _reg_args, _register, _register_args, quantile_rank, taper_window

__all__ = ["sample_z_truncated", "check_empty_depths", "evaluate_INN_forward", "inverse_pass", "nll_step",
           "nll_terms", "allreduce_nll", "build_networks", "step_log_likelihoods", "allgather_scores", "detect_ood",
           "forward_nll_pass", "mean_volume_cache", "save_mean_volume_cache", "load_mean_volume_cache",
           "denormalise_prediction", "denormalise_ground_truth", "compute_INN_step_performance", "evaluate_step", "roi_boxes",
           "corr_coeff_3D", "truncated_normal_variance", "posterior_moments", "posterior_samples", "posterior_roi_means",
           "ActivityMap", "RegressionMap", "RegressionMaps", "calcium_regressors", "find_neurons", "read_neural_coordinates_from_file", "write_neural_coordinates_to_file",
           "NeuronFootprints", "Footprints", "extract_traces", "demix_plan", "demix_traces", "trace_baseline", "delta_f_over_f", "trace_noise", "infer_spikes",
           "estimate_volume_shifts", "shift_volumes", "register_volumes", "VolumeRegistration", "VolumeRegistrar", "valid_box",
           "block_grid", "BlockGrid", "estimate_block_shifts", "warp_volumes", "register_volumes_piecewise", "PiecewiseRegistration",
           "PiecewiseVolumeRegistrar", "fit_rigid_motion", "RigidFit", "rigid_move_volumes", "estimate_rigid_motion", "register_volumes_rigid",
           "RigidRegistration", "RigidVolumeRegistrar", "rigid_angles", "rigid_corner_shifts"]


def _no_grad_trunc_normal_(tensor, mean=0., std=1., a=-1., b=1.):
    """Truncated normal by inverse-CDF sampling (utils.py:42-82 semantics).  Only reached for temperature != 0, a path
    that raises NameError in the reference itself; provided for completeness and checked
    statistically only."""
    def norm_cdf(v):
        return (1. + math.erf(v / math.sqrt(2.))) / 2.
    with torch.no_grad():
        lo, up = norm_cdf((a - mean) / std), norm_cdf((b - mean) / std)
        tensor.uniform_(2 * lo - 1, 2 * up - 1)
        tensor.erfinv_()
        tensor.mul_(std * math.sqrt(2.))
        tensor.add_(mean)
        tensor.clamp_(min=a, max=b)
        return tensor


def sample_z_truncated(x, device="cpu", temperature=1, seed=None, stream=0, sample_offset=0):
    """Latent sample; ``temperature == 0`` (the default of main.py:109) returns zeros.  CWFA.py:47-64.
    The fused inverse treats ``None`` as an all-zero z and never reads it (``inverse_pass`` does that itself).
    With ``seed`` the draw is ONE launch of the counter-based generator (``ops.rand_trunc_normal``: the first axis is its sample
    axis; ``stream`` / ``sample_offset`` as there) on the HIP device instead of torch's five passes and global generator."""
    shape_like = torch.is_tensor(x)
    if temperature == 0:
        return torch.zeros_like(x, device=device) if shape_like else torch.zeros(x, device=device)
    if seed is not None:
        return ops.rand_trunc_normal(tuple(x.shape) if shape_like else tuple(x), temperature, seed, stream, sample_offset,
                                     device=torch.device(device))
    base = torch.zeros_like(x, device=device) if shape_like else torch.zeros(x, device=device)
    return _no_grad_trunc_normal_(base, a=-temperature, b=temperature)


def check_empty_depths(gt_volume):
    """Add tiny noise to depth columns that are constant over depth (avoids degenerate statistics).  CWFA.py:84-96.
    Bookkeeping on the input volume (torch ops), not part of the kernel path."""
    empty = gt_volume.std(dim=1) == 0
    n_depths = gt_volume.shape[1]
    empty = empty.view(gt_volume.shape[0], empty.shape[0] // gt_volume.shape[0], empty.shape[1], empty.shape[2])
    if empty.any():
        sel = empty.repeat(1, n_depths, 1, 1)
        gt_volume[sel] += torch.normal(0, 0.001, gt_volume[sel].size(), device=gt_volume.device)
    return gt_volume


def nll_terms(graph, x, c):
    """Forward one step and return the shard-local NLL sums: (Z tuple, logdet[B], sum ||Z0||^2 as float64[1] tensor).
    The sum of squares comes out of the fused chain kernel (no extra pass over Z)."""
    sumsq = torch.zeros(1, dtype=torch.float64, device=x.device)
    Z, logdet = graph(x, c=c, sumsq=sumsq) if getattr(graph, "_plan", None) is not None else graph(x, c=c)
    if getattr(graph, "_plan", None) is None:
        st = ops.sample_stats(Z[0].reshape(1, -1, 1, 1))
        sumsq = st[1:2]
    return Z, logdet, sumsq


def evaluate_INN_forward(conv_inn, cond_nets, args_general, args_nets, gt_volume, input_views, train_statistics,
                         extra_cond_in=None):
    """Forward pyramid with per-step likelihood terms.  CWFA.py:134-196.
    Returns (losses, gt_cache, prior_errors, log_jacobians) with the reference's normalisations."""
    device = gt_volume.device
    gt_volume = check_empty_depths(gt_volume)
    mean_imgs, std_imgs = train_statistics[0], train_statistics[1]
    losses, prior_errors, log_jacobians = [], [], []
    gt_cache = args_general.INN_max_down_steps * [None]
    gt_cache[0] = gt_volume
    cond_input = (input_views - mean_imgs) / std_imgs
    B = gt_volume.shape[0]
    for n_net in range(len(conv_inn)):
        g = conv_inn[n_net]
        is_last_step = n_net == args_general.INN_max_down_steps - 1
        if is_last_step:
            cond_in = [] if args_general.force_all_steps_NF else [cond_nets[n_net](cond_input)[-1]]
        else:
            cond_in = [torch.zeros((B,) + tuple(g.dims_c[0]), device=device)] if len(g.dims_c) > 0 else []
        if len(g.dims_c) > 1:
            if extra_cond_in is None:
                cond_in.append(torch.zeros((B,) + tuple(g.dims_c[1]), device=device))
            else:
                cond_in.append(extra_cond_in[n_net].clone())
        Z, log_jac_det, sumsq = nll_terms(g, gt_volume, cond_in)
        error_on_prior = sumsq[0].to(torch.float32)
        numel = Z[-1].numel()
        curr = (0.5 * error_on_prior - log_jac_det) / numel
        losses.append(curr.mean())
        prior_errors.append(0.5 * error_on_prior.mean() / numel)
        log_jacobians.append(log_jac_det.mean() / numel)
        if not is_last_step:
            gt_volume = Z[1]
            gt_cache[n_net + 1] = gt_volume
    return losses, gt_cache, prior_errors, log_jacobians


def step_log_likelihoods(conv_inn, cond_nets, args_general, gt_volume, input_views, train_statistics, extra_cond_in=None,
                         group=None):
    """Per-sample, per-step log-likelihoods of a batch under the flows: LL[b, n] = -(0.5*||z_b||^2 - logdet_b) / numel_b
    -- the per-volume form of ``evaluate_INN_forward``'s losses (CWFA.py:183-186; for a batch of one, LL[0, n] is
    exactly -losses[n]).  This is the score the reference thresholds for out-of-distribution detection
    (main.py:78-80: ``--step_LL_to_use``, ``--step_LL_ths_to_use``; its evaluator ``main_OOD`` is not part of the
    released sources, main.py:16,401).  One fused forward chain per step; the per-sample sums of squares are one
    extra read of Z0 (``sample_stats``).  With a process group every rank scores its shard and the [B_local, S] blocks
    are all-gathered in rank order (RCCL on MI355X): every rank returns the scores of the global batch.
    Returns a float64 tensor [B, len(conv_inn)]."""
    device = gt_volume.device
    gt_volume = check_empty_depths(gt_volume)
    cond_input = (input_views - train_statistics[0]) / train_statistics[1]
    B = gt_volume.shape[0]
    cols = []
    for n_net, g in enumerate(conv_inn):
        is_last_step = n_net == args_general.INN_max_down_steps - 1
        if is_last_step:
            cond_in = [] if args_general.force_all_steps_NF else [cond_nets[n_net](cond_input)[-1]]
        else:
            cond_in = [torch.zeros((B,) + tuple(g.dims_c[0]), device=device)] if len(g.dims_c) > 0 else []
        if len(g.dims_c) > 1:
            cond_in.append(torch.zeros((B,) + tuple(g.dims_c[1]), device=device) if extra_cond_in is None
                           else extra_cond_in[n_net].clone())
        Z, logdet = g(gt_volume, c=cond_in)
        sumsq = ops.sample_stats(Z[0]).view(B, 2)[:, 1]
        cols.append(-(0.5 * sumsq - logdet.to(torch.float64)) / Z[-1][0].numel())
        if not is_last_step:
            gt_volume = Z[1]
    return allgather_scores(torch.stack(cols, 1), group)


def allgather_scores(scores, group=None):
    """Concatenate the ranks' [B_local, S] score blocks in rank order (shards may differ in size); no-op without
    torch.distributed.  Two small all-gathers: the shard sizes, then the blocks padded to the largest shard."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1):
        return scores
    device, B = scores.device, scores.shape[0]
    counts = [torch.zeros(1, dtype=torch.int64, device=device) for _ in range(dist.get_world_size(group))]
    dist.all_gather(counts, torch.tensor([B], dtype=torch.int64, device=device), group=group)
    counts = [int(c_) for c_ in counts]
    padded = torch.zeros(max(counts), scores.shape[1], dtype=scores.dtype, device=device)
    padded[:B] = scores
    blocks = [torch.empty_like(padded) for _ in counts]
    dist.all_gather(blocks, padded, group=group)
    return torch.cat([blk[:c_] for blk, c_ in zip(blocks, counts)], 0)


def detect_ood(scores, step_LL_to_use=0, step_LL_ths_to_use=-1.33):
    """Out-of-distribution flags from ``step_log_likelihoods``: a sample is flagged when the log-likelihood of step
    ``step_LL_to_use`` falls below the threshold (defaults of main.py:79-80)."""
    return scores[:, step_LL_to_use] < step_LL_ths_to_use


def inverse_pass(conv_inn, cond_nets, cond_input, mean_vols_cache, low=None, temperature=0.0, n_samples=1,
                 keep_all=False):
    """The reconstruction loop for one batch of views.  CWFA.py:865-924.

    ``cond_nets`` has one condition net per flow step plus, if ``low`` is None, the LRNN encoder as its last entry
    (CWFA.py:495-496,882).  ``mean_vols_cache[n]`` is the mean-volume detail at step n (CWFA.py:655,899).
    Returns the full-resolution volume (or every level, coarse -> fine, with ``keep_all``)."""
    S1 = len(conv_inn)
    if low is None:
        up = cond_nets[S1](cond_input, mean_vols_cache[S1 - 1])[-1]
    else:
        up = low
    vols = [up]
    from .networks import omega_first_scope
    with omega_first_scope(list(cond_nets[:S1]), cond_input):      # the steps' condition nets share their input: first convs in one launch
        return _inverse_steps(conv_inn, cond_nets, cond_input, mean_vols_cache, up, vols, temperature, n_samples, keep_all)


def _inverse_steps(conv_inn, cond_nets, cond_input, mean_vols_cache, up, vols, temperature, n_samples, keep_all):
    S1 = len(conv_inn)
    for n in range(S1 - 1, -1, -1):
        g = conv_inn[n]
        cond_processed = [cond_nets[n](cond_input)[-1], mean_vols_cache[n]]
        if n_samples > 1:
            cond_processed = [cc.repeat(n_samples, 1, 1, 1) for cc in cond_processed]
            up = up.repeat(n_samples, 1, 1, 1)
        if temperature == 0 and getattr(g, "_plan", None) is not None:
            z = None                              # z == 0: the fused chain never reads it (CWFA.py:54-55)
        else:
            z = sample_z_truncated((up.shape[0],) + tuple(g.global_out_shapes[0]), device=up.device,
                                   temperature=temperature)
        up, _ = g([z, up], c=cond_processed, rev=True, jac=getattr(g, "_plan", None) is None)   # log-det is discarded
        if n_samples > 1:                         # CWFA.py:913-914: average the samples
            parts = up.view(n_samples, -1, *up.shape[1:])
            acc = ops.axpby(parts[0], 1.0 / n_samples)
            for i in range(1, n_samples):
                acc = ops.axpby(parts[i], 1.0 / n_samples, acc, 1.0)
            up = acc
        vols.append(up)
    return vols if keep_all else up


# ---------------------------------------------------------------------------------------------------------------------
# The posterior of a CAT pyramid.  In a ConditionalAffineTransform step every s,t depends on the
# conditions (the views and the mean-volume cache) only, so given the views the whole pyramid is an AFFINE map of the
# latents: its mean is the temperature-0 reconstruction, its per-voxel variance has a closed form in the s rows, and N
# samples need every network once.
# ---------------------------------------------------------------------------------------------------------------------
def truncated_normal_variance(temperature):
    """Variance of the latent ``sample_z_truncated`` draws: a STANDARD normal truncated to [-T, T] (T is the truncation
    bound, not a standard deviation; CWFA.py:47-64).  z_var(T) = 1 - 2 T phi(T) / (2 Phi(T) - 1); z_var(0) = 0,
    z_var(1) = 0.2911..., z_var(inf) = 1.  float64 on the host.  The closed form cancels for small T (z_var -> T^2/3); below
    T = 0.5 the quotient is evaluated as a ratio of two series in T^2, which keeps the relative error near 1e-15."""
    T = float(temperature)
    if not T >= 0.0:
        raise ValueError(f"temperature {temperature!r}: the truncation bound must be >= 0")
    if T == 0.0:
        return 0.0
    if math.isinf(T):
        return 1.0
    if T < 0.5:
        # with u = T^2/2:  2 Phi(T) - 1 = 2 T phi(T) * sum_n T^(2n) / (2n+1)!!  =: 2 T phi(T) * (1 + A), so that
        # z_var = A / (1 + A):  no cancellation, every term positive
        A, term, n = 0.0, 1.0, 0
        while True:
            n += 1
            term *= T * T / (2 * n + 1)
            A += term
            if term <= 1e-18 * A:
                break
        return A / (1.0 + A)
    phi = math.exp(-0.5 * T * T) / math.sqrt(2.0 * math.pi)
    return 1.0 - 2.0 * T * phi / math.erf(T / math.sqrt(2.0))


def _affine_plans(conv_inn, what):
    """The CAT plans of a pyramid, or NotImplementedError where a step is not an affine map of its latent."""
    from .FrEIA.framework import _CatStepPlan
    plans = []
    for n, g in enumerate(conv_inn):
        plan = getattr(g, "_plan", None)
        if plan is None:
            raise NotImplementedError(f"{what}: step {n} has no fused CAT plan (its graph is not the conditional wavelet-flow step)")
        if type(plan) is not _CatStepPlan:
            raise NotImplementedError(f"{what}: step {n} has data-dependent coupling blocks (GLOW / RNVP / GIN / AllInOne): its output "
                                      "is not affine in z, so there is no closed-form posterior and no shared coefficients")
        if plan.needs_walk():
            raise NotImplementedError(f"{what}: step {n} holds an ActNorm that still has to initialise itself from its first batch")
        plans.append(plan)
    return plans


def _coarsest(conv_inn, cond_nets, cond_input, mean_vols_cache, low):
    S1 = len(conv_inn)
    return cond_nets[S1](cond_input, mean_vols_cache[S1 - 1])[-1] if low is None else low


@amp_function
@torch.no_grad()          # inference only: the plans' stage lists are built without a tape
def posterior_moments(conv_inn, cond_nets, cond_input, mean_vols_cache, low=None, temperature=1.0, std_scale=1.0,
                      keep_all=False):
    """(mean, std) per voxel of the volumes ``inverse_pass`` would reconstruct with latents drawn at ``temperature`` (every
    step all-CAT; NotImplementedError otherwise).  The loop of ``inverse_pass``: per step the sub-networks run once, one
    ``ops.chain_inv`` with z = None gives the mean -- the launches of ``inverse_pass(..., temperature=0)``, so bit-identical
    to it: the truncated normal is symmetric -- and one ``ops.chain_inv_var`` carries the variance down:
    var_x[2c] = var_x[2c+1] = (var_low[c] + z_var * exp(-2 * sum of s along the voxel's path)) / 2, with var_low = 0 behind
    the (deterministic) LRNN or a given ``low``.  The shifts never enter; ``low`` and the detail band are independent because
    the latents of different steps are drawn independently.

    ``std_scale`` multiplies the finest level's std in its own launch.  For the de-normalised volume of CWFA.py:1041
    (``denormalise_prediction``: volume * std_vols * 2**len(batch)) pass ``std_scale = std_vols * 2**len(batch)``.
    With ``keep_all`` both results are lists, coarse -> fine; the stds of the levels below the finest are unscaled (and the
    coarsest level's std is zero)."""
    plans = _affine_plans(conv_inn, "posterior_moments")
    if not float(std_scale) > 0.0:
        raise ValueError(f"std_scale {std_scale!r} must be > 0")
    z_var = truncated_normal_variance(temperature)
    S1 = len(conv_inn)
    up = _coarsest(conv_inn, cond_nets, cond_input, mean_vols_cache, low)
    var = None                                       # None = 0: the coarsest volume is deterministic
    means, stds = [up], [torch.zeros_like(up)] if keep_all else None
    from .networks import omega_first_scope
    with omega_first_scope(list(cond_nets[:S1]), cond_input):
        for n in range(S1 - 1, -1, -1):
            c = [cond_nets[n](cond_input)[-1], mean_vols_cache[n]]
            stages, tabs = plans[n].inverse_stages(c, tuple(up.shape[1:]), up.device)
            shape = tuple(up.shape)
            up = ops.chain_inv(None, up, stages, tables=tabs)
            last = n == 0                            # the finest level: the launch returns std_scale * sqrt(variance)
            var = ops.chain_inv_var(var, stages, z_var, shape=shape, std_scale=float(std_scale) if last else 0.0, tables=tabs)
            if keep_all:
                stds.append(var if last else var.sqrt())
            means.append(up)
    return (means, stds) if keep_all else (up, var)


@amp_function
@torch.no_grad()
def posterior_samples(conv_inn, cond_nets, cond_input, mean_vols_cache, n_samples, low=None, temperature=1.0,
                      return_z=False, seed=None, sample_offset=0):
    """``n_samples`` genuine posterior samples [n_samples, B, D, H, W] of the reconstruction (every step all-CAT;
    NotImplementedError otherwise).  Every condition net and every sub-network runs ONCE per step; per sample only the
    latent draw (``sample_z_truncated``) and one ``ops.chain_inv`` follow.  Each sample carries its own coarser volume down
    the pyramid and nothing is averaged between the steps -- unlike ``inverse_pass(n_samples=...)``, which repeats the
    conditions, runs every network per sample and averages after every step (CWFA.py:913-914).  ``temperature = 0`` yields
    ``n_samples`` copies of the mean.  With ``return_z`` also the latents: a list over the steps in execution order (coarse
    -> fine) of [n_samples, B, C_n, H, W] tensors (None per step at temperature 0).

    With ``seed`` (and temperature > 0) the latents come from the counter-based generator inside ONE ``ops.chain_inv_samples``
    launch per step -- no separate draw, no ``torch.stack``; the step's execution index (0 = coarsest) is the generator's
    stream and sample i draws at counter ``sample_offset + i``, so the call is reproducible and samples [k, n) of one call are
    samples [0, n - k) of a call with ``sample_offset + k``.  Without ``seed`` the latents are torch's, as before."""
    plans = _affine_plans(conv_inn, "posterior_samples")
    n_samples = int(n_samples)
    if n_samples < 1:
        raise ValueError("posterior_samples: n_samples must be >= 1")
    if not float(temperature) >= 0.0:
        raise ValueError(f"temperature {temperature!r}: the truncation bound must be >= 0")
    S1 = len(conv_inn)
    if seed is not None and temperature != 0:
        up = _coarsest(conv_inn, cond_nets, cond_input, mean_vols_cache, low)
        steps = _inverse_stage_lists(plans, cond_nets, cond_input, mean_vols_cache, tuple(up.shape[1:]), up.device)
        return _seeded_samples(steps, up, n_samples, temperature, seed, sample_offset, return_z)
    ups = [_coarsest(conv_inn, cond_nets, cond_input, mean_vols_cache, low)] * n_samples
    latents = []
    from .networks import omega_first_scope
    with omega_first_scope(list(cond_nets[:S1]), cond_input):
        for n in range(S1 - 1, -1, -1):
            c = [cond_nets[n](cond_input)[-1], mean_vols_cache[n]]
            stages, tabs = plans[n].inverse_stages(c, tuple(ups[0].shape[1:]), ups[0].device)
            if temperature == 0:
                zs = None                             # z == 0: the chain never reads it; every sample is the mean
                out = ops.chain_inv(None, ups[0], stages, tables=tabs)
                ups = [out] * n_samples
            else:
                zs = torch.stack([sample_z_truncated(ups[0], device=ups[0].device, temperature=temperature) for _ in range(n_samples)])
                ups = [ops.chain_inv(zs[i], ups[i], stages, tables=tabs) for i in range(n_samples)]
            latents.append(zs)
    out = torch.stack(ups)
    return (out, latents) if return_z else out


def _inverse_stage_lists(plans, cond_nets, cond_input, mean_vols_cache, shape, device):
    """(stages, tables) of every step in execution order (coarse -> fine): every condition net and sub-network runs once.
    ``shape`` = (C, H, W) of the coarsest volume; each step doubles the channels.  The coefficient tensors of all steps are alive
    together while the list is (ten planes per detail channel)."""
    from .networks import omega_first_scope
    S1 = len(plans)
    C0, H, W = shape
    steps = []
    with omega_first_scope(list(cond_nets[:S1]), cond_input):
        for i, n in enumerate(range(S1 - 1, -1, -1)):
            c = [cond_nets[n](cond_input)[-1], mean_vols_cache[n]]
            steps.append(plans[n].inverse_stages(c, (C0 << i, H, W), device))
    return steps


def _seeded_samples(steps, up, n_samples, temperature, seed, sample_offset, return_z):
    """One ``ops.chain_inv_samples`` launch per step: ``up`` [B,C,H,W] is shared at the coarsest step, afterwards every sample
    carries its own volume."""
    latents = []
    for i, (stages, tabs) in enumerate(steps):
        res = ops.chain_inv_samples(up, stages, n_samples, temperature, seed, stream=i, sample_offset=sample_offset, tables=tabs,
                                    return_z=return_z)
        up, z = res if return_z else (res, None)
        latents.append(z)
    return (up, latents) if return_z else up


@amp_function
@torch.no_grad()
def posterior_roi_means(conv_inn, cond_nets, cond_input, mean_vols_cache, boxes, n_samples, low=None, temperature=1.0, seed=0,
                        chunk=16):
    """The ROI means (``corr_coeff_3D``'s traces, before its normalisation) of ``n_samples`` posterior samples: float64
    [n_samples, B, n_roi] -- the DISTRIBUTION behind the error bar of a neuron's trace (quantiles, tails, any non-linear
    statistic).  Its first two moments need no samples: the mean, the variance and the covariance of any two ROI means are exact
    in ``posterior_roi_moments`` (the two voxels of a Haar pair share a latent with opposite signs and coarse latents are shared by
    2^k depths, which the closed form there accounts for).  ``boxes``: the
    integer [n_roi, 6] table of ``roi_boxes``.  Every network and stage list is built ONCE; the samples are then drawn ``chunk``
    at a time (``posterior_samples(seed=seed, sample_offset=...)``: the same values whatever ``chunk`` is) and reduced by
    ``ops.roi_means``, so the samples' memory is bounded by ``chunk`` volumes per level.  The price of building the networks once is
    fixed: the s and t tensors of EVERY step stay alive for the whole call (ten planes per detail channel: about 1 GB at
    96 x 512 x 512), where the unseeded ``posterior_samples`` frees a step's coefficients before the next step.  Every step
    all-CAT; NotImplementedError otherwise."""
    plans = _affine_plans(conv_inn, "posterior_roi_means")
    n_samples, chunk = int(n_samples), int(chunk)
    if n_samples < 1 or chunk < 1:
        raise ValueError("posterior_roi_means: n_samples and chunk must be >= 1")
    if not float(temperature) >= 0.0:
        raise ValueError(f"temperature {temperature!r}: the truncation bound must be >= 0")
    up = _coarsest(conv_inn, cond_nets, cond_input, mean_vols_cache, low)
    steps = _inverse_stage_lists(plans, cond_nets, cond_input, mean_vols_cache, tuple(up.shape[1:]), up.device)
    B = up.shape[0]
    if temperature == 0:                             # every sample is the mean
        for stages, tabs in steps:
            up = ops.chain_inv(None, up, stages, tables=tabs)
        return ops.roi_means(up, boxes).t().unsqueeze(0).repeat(n_samples, 1, 1)
    out = []
    for k in range(0, n_samples, chunk):
        n = min(chunk, n_samples - k)
        xs = _seeded_samples(steps, up, n, temperature, seed, k, False)
        out.append(ops.roi_means(xs.view(n * B, *xs.shape[2:]), boxes).t().reshape(n, B, -1))
    return torch.cat(out)


@amp_function
@torch.no_grad()
def posterior_roi_moments(conv_inn, cond_nets, cond_input, mean_vols_cache, boxes, low=None, temperature=1.0, pairs=None,
                          std_scale=1.0, return_volume=False):
    """Exact first and second moments of the ROI means (``corr_coeff_3D``'s traces, before its normalisation) under the posterior
    ``posterior_samples`` draws from: ``(mean [B, R], std [B, R], cov [B, P] or None)``, float64, plus the mean volume with
    ``return_volume``.  ``boxes``: the integer [R, 6] table of ``roi_boxes``; ``pairs``: integer [P, 2] box indices whose covariance
    is wanted (None: ``cov`` is None).  Every step all-CAT; NotImplementedError otherwise (as ``posterior_moments``).

    The loop of ``posterior_moments``: per step the sub-networks run once, one ``ops.chain_inv`` with z = None carries the mean
    volume down (the mean of an ROI mean is the ROI mean of that volume: E z = 0) and one ``ops.chain_inv_roi_cov`` adds the step's
    term of
        Cov(mean_r1, mean_r2) = z_var / (cnt_r1 cnt_r2) * sum_m 2^-m sum_c q_r1,m(c) q_r2,m(c) sum_{(y,x) in both footprints} exp(a_m[c,y,x])
    where step m (1 = finest) spreads its detail v[c] over the 2^m depths of block c with opposite signs on the two halves,
    q_r,m(c) counts the box's depths in the first half minus those in the second, and z_var exp(a_m) is the variance of v.  Depths
    that cover a whole block cancel exactly: a box over all depths has variance 0.  A step's coefficients are free before the
    next step runs.  An empty box gives NaN, as in ``ops.roi_means``.

    ``std_scale`` as in ``posterior_moments`` (std_vols * 2**len(batch) for the de-normalised volume): it multiplies ``mean`` and
    ``std`` and its square multiplies ``cov``, in float64 on the results; the returned volume is unscaled."""
    import numpy as np
    plans = _affine_plans(conv_inn, "posterior_roi_moments")
    if not float(std_scale) > 0.0:
        raise ValueError(f"std_scale {std_scale!r} must be > 0")
    z_var = truncated_normal_variance(temperature)
    S1 = len(conv_inn)
    bx = np.asarray(boxes, dtype=np.int32).reshape(-1, 6)
    R = len(bx)
    diag = np.repeat(np.arange(R, dtype=np.int32)[:, None], 2, 1)
    pr = diag if pairs is None else np.concatenate([diag, np.asarray(pairs, dtype=np.int32).reshape(-1, 2)])
    up = _coarsest(conv_inn, cond_nets, cond_input, mean_vols_cache, low)
    table = ops.RoiPairs(bx, pr, up.device)          # the variances first, then the requested pairs: one launch per step
    acc = torch.zeros(up.shape[0], len(pr), dtype=torch.float64, device=up.device)
    from .networks import omega_first_scope
    with omega_first_scope(list(cond_nets[:S1]), cond_input):
        for n in range(S1 - 1, -1, -1):
            c = [cond_nets[n](cond_input)[-1], mean_vols_cache[n]]
            stages, tabs = plans[n].inverse_stages(c, tuple(up.shape[1:]), up.device)
            shape = tuple(up.shape)
            up = ops.chain_inv(None, up, stages, tables=tabs)
            ops.chain_inv_roi_cov(acc, stages, z_var, shape, n + 1, table)      # step n is level m = n + 1 (n = 0: the finest)
    scale = float(std_scale)
    mean = ops.roi_means(up, bx).t() * scale
    std = acc[:, :R].sqrt() * scale
    cov = None if pairs is None else acc[:, R:] * (scale * scale)
    return (mean, std, cov, up) if return_volume else (mean, std, cov)


@amp_function
@torch.no_grad()
def nll_maps(conv_inn, cond_nets, gt_volume, cond_input, mean_vols_cache, want_z=False):
    """WHERE a volume disagrees with the flow (every step all-CAT, NotImplementedError otherwise: only there
    does the density factorise over the coefficients).  With the conditions of ``forward_nll_pass`` every Haar detail coefficient
    of every step is an independent Gaussian g z + o, so its standardised residual z = (d - o) / g and its share
    nll = z^2 / 2 + log g of the step's negative log-likelihood are exact.  One ``ops.chain_nll_map`` launch per step, fine ->
    coarse, each fed by the previous step's low band, then one ``ops.nll_compose``.  Returns

        (volume_map [B,D,H,W], maps, z_maps, sums, low)

    ``maps[n]`` [B, D / 2^(n+1), H, W]: the step-n coefficients' shares, each at the coefficient's own position; a coefficient covers
    2^(n+1) adjacent depths at its pixel and ``volume_map`` spreads it evenly over them, so its total is the pyramid's NLL.
    ``z_maps``: the z-scores laid out likewise (None unless ``want_z``): for a volume drawn from the posterior they are the latents
    that were drawn -- see ``zscore_coverage``.  ``sums`` float64 [B, S]: per sample and step the sum of ``maps[n]``
    = 0.5 * sum z^2 - logdet, what ``nll_terms`` reduces.  ``low``: the coarsest low band, as ``forward_nll_pass`` returns it."""
    plans = _affine_plans(conv_inn, "nll_maps")
    S1 = len(conv_inn)
    B = gt_volume.shape[0]
    sums = [torch.zeros(B, dtype=torch.float64, device=gt_volume.device) for _ in range(S1)]
    maps, z_maps = [], [] if want_z else None
    gt = gt_volume
    from .networks import omega_first_scope
    with omega_first_scope(list(cond_nets[:S1]), cond_input):
        for n in range(S1):
            c = [cond_nets[n](cond_input)[-1], mean_vols_cache[n]]
            stages, tabs = plans[n].inverse_stages(c, (gt.shape[1] // 2,) + tuple(gt.shape[2:]), gt.device)
            nll, gt, z = ops.chain_nll_map(gt, stages, tables=tabs, want_low=True, want_z=want_z, want_nll=True, nll_sum=sums[n])
            maps.append(nll)
            if want_z:
                z_maps.append(z)
    return ops.nll_compose(maps), maps, z_maps, torch.stack(sums, dim=1), gt


def zscore_coverage(z_levels, ks=(1.0, 2.0, 3.0)):
    """The calibration readout of the posterior: per level of z-scores (``nll_maps(..., want_z=True)[2]``, or any tensors) the
    fraction of |z| <= k beside the standard normal's erf(k / sqrt 2).  Returns (observed float64 [levels, len(ks)] on the
    z-scores' device, expected float64 [len(ks)]); a posterior that is too narrow for the volumes it is shown covers less than
    expected, one that is too wide more.  Torch reductions on the device; nothing waits for it."""
    z_levels = list(z_levels)
    ks = [float(k) for k in ks]
    if not z_levels or not ks:
        raise ValueError("zscore_coverage: needs at least one level and one k")
    rows = [torch.stack([(z.abs() <= k).sum().to(torch.float64) / z.numel() for k in ks]) for z in z_levels]
    expected = torch.tensor([math.erf(k / math.sqrt(2.0)) for k in ks], dtype=torch.float64)
    return torch.stack(rows), expected


def nll_step(graph, x, c, group=None):
    """Training-time NLL of one step, CWFA.py:966-978:  (0.5*||Z0||^2 - mean_b logdet) / numel(batch volume),
    with the norm taken over the WHOLE (global) batch.  The divisor is ``upsampled_vol.numel()`` = B*D_n*H*W, the step's
    full-depth volume (CWFA.py:911,978) -- twice ``Z[-1].numel()``, which ``evaluate_INN_forward`` divides by (:186).  With a process group the three shard sums are all-reduced
    (RCCL over xGMI on MI355X: one float64[3] message) and every rank returns the identical global value."""
    Z, logdet, sumsq = nll_terms(graph, x, c)
    terms = torch.stack([sumsq[0], logdet.to(torch.float64).sum(),
                         torch.tensor(float(x.shape[0]), dtype=torch.float64, device=x.device)])
    terms = allreduce_nll(terms, group)
    numel_total = terms[2] * x[0].numel()      # `upsampled_vol.numel()`: the step's whole input volume (CWFA.py:911,978)
    nll = (0.5 * terms[0] - terms[1] / terms[2]) / numel_total
    return nll, Z, logdet


def forward_nll_pass(conv_inn, cond_nets, gt_volume, cond_input, mean_vols_cache, group=None):
    """The forward / NLL twin of ``inverse_pass`` over the whole pyramid for one (shard of a) batch -- BASELINE.json
    configs[3]: for n = 0 .. S-2: condition net Omega_n, ``Z, logdet = conv_inn[n](gt_n, c=[Omega_n(views), mean_n])``
    (CWFA.py:895-899,966), ``gt_{n+1} = Z[1]`` (the low band: what CWFA.py:821 caches), and
    ``NLL_n = (0.5 * ||Z0||^2 - mean_b logdet) / numel(batch volume)`` (CWFA.py:970-978) with the norm and the mean
    taken over the GLOBAL batch.  With a process group the S-1 triples {sum z^2, sum logdet, B_local} are summed over
    the ranks in ONE all-reduce of a float64[3(S-1)] vector (RCCL over xGMI on MI355X) and every rank returns the same
    values.  Returns (nll float64[S-1], low-resolution volume gt_{S-1})."""
    gt = gt_volume
    rows = []
    from .networks import omega_first_scope
    with omega_first_scope(list(cond_nets[:len(conv_inn)]), cond_input):
        for n, g in enumerate(conv_inn):
            Z, logdet, sumsq = nll_terms(g, gt, [cond_nets[n](cond_input)[-1], mean_vols_cache[n]])
            rows.append(torch.stack([sumsq[0], logdet.to(torch.float64).sum(),
                                     torch.tensor(float(gt.shape[0]), dtype=torch.float64, device=gt.device)]))
            gt = Z[1]
    terms = allreduce_nll(torch.stack(rows).reshape(-1), group).view(len(conv_inn), 3)
    numel = torch.tensor([float(gt_volume[0].numel()) / 2 ** n for n in range(len(conv_inn))], dtype=torch.float64,
                         device=gt_volume.device)                    # per-sample numel of the step's input volume
    nll = (0.5 * terms[:, 0] - terms[:, 1] / terms[:, 2]) / (terms[:, 2] * numel)
    return nll, gt


def allreduce_nll(terms, group=None):
    """Sum the [sum z^2, sum logdet, B] vector over the data-parallel ranks (no-op without torch.distributed)."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(terms, op=dist.ReduceOp.SUM, group=group)
    return terms


def build_networks(n_depths=96, side=512, max_down_steps=5, block_type="CAT", n_blocks=4, internal_chans=64,
                   cond_chans=32, use_perm=True, use_bias=True, with_lrnn=True, device="cuda"):
    """Build the model list the way run_CWFA does (CWFA.py:478-532): one (GraphINN, cond_network) per flow step and the
    LRNN Encoder as the last condition net.  Flow nets and condition nets in eval mode, the LRNN in train mode."""
    from . import networks as N
    conv_inn, cond_nets = [], []
    for ix in range(max_down_steps - 1):
        cn = n_depths // (2 ** (ix + 1))
        cond_net, inns = N.conditional_wavelet_flow(
            input_volume_shape=[n_depths, side, side], condition_shape=[1, 29, side, side],
            st_subnet=N.wavelet_flow_subnetwork2D,
            conditional_network=lambda: N.cond_network(29, cn, ix + 1, max_down_steps, [], cond_chans),
            n_internal_ch=internal_chans, n_down_steps=ix + 1, use_permutations=use_perm, block_type=block_type,
            n_blocks=n_blocks, device="cpu")
        conv_inn.append(inns[ix].eval().to(device))
        cond_nets.append(cond_net.eval().to(device))
    if with_lrnn:
        enc = N.Encoder(29, n_depths // (2 ** (max_down_steps - 1)), max_down_steps, internal_chans, use_bias).to(device)
        enc.train()                                     # CWFA.py:532: BatchNorm batch statistics, dropout, drop_path
        cond_nets.append(enc)
    return conv_inn, cond_nets


# ---------------------------------------------------------------------------------------------------------------------
# Mean-volume cache and output step
# ---------------------------------------------------------------------------------------------------------------------
def mean_volume_cache(gt_levels):
    """The per-step second condition of the flows: for every level of the forward pyramid of a (normalised) mean volume
    -- ``evaluate_INN_forward``'s gt_cache -- the difference of the even and odd depth planes of its FIRST sample,
    ``gt[0, ::2] - gt[0, 1::2]`` (CWFA.py:655).  One channel gather (even planes | odd planes) and one subtraction per
    level on the HIP kernels; returns tensors [D_n / 2, H, W] like the reference."""
    out = []
    for gt in gt_levels:
        if gt is None:
            continue
        D = gt.shape[1]
        order = torch.cat([torch.arange(0, D, 2), torch.arange(1, D, 2)]).to(gt.device)
        eo = ops.gather(gt[:1], order, 1)                                  # [1, D, H, W]: even planes, then odd planes
        out.append(ops.axpby(eo[:, :D // 2], 1.0, eo[:, D // 2:], -1.0)[0])
    return out


def save_mean_volume_cache(path, cache):
    """``torch.save({'mean_vol_gt_cache': [...cpu tensors...]}, path)`` -- the file main.py:377 writes (named
    ``mean_vol_{N}Imgs_ds_{id}_{split}`` there)."""
    torch.save({'mean_vol_gt_cache': [v.detach().cpu() for v in cache]}, path)


def load_mean_volume_cache(path_or_dir, device="cpu", dataset_id=None, split=None):
    """Read a mean-volume cache as CWFA.py:637-640 does: ``path_or_dir`` is the file, or with ``dataset_id`` and ``split`` the
    directory searched for ``mean_vol_*ds_{dataset_id}_{split}`` (first match).  The file holds plain tensors: it is read
    with ``weights_only=True`` (nothing in it is executed).  Returns the list moved to ``device``, or None if no file matches."""
    import glob
    import os
    path = path_or_dir
    if dataset_id is not None:
        hits = sorted(glob.glob(os.path.join(str(path_or_dir), f"mean_vol_*ds_{dataset_id}_{split}")))
        if not hits:
            return None
        path = hits[0]
    data = torch.load(path, map_location="cpu", weights_only=True)
    return [v.to(device) for v in data['mean_vol_gt_cache']]


def denormalise_prediction(stored_volume, std_vols, mean_vols):
    """The evaluation branch's predicted output volume, CWFA.py:1041:
    ``(stored_volumes[0][0] * 2**len(stored_volumes[0])) * std_vols + mean_vols`` -- first sample of the finest reconstruction;
    the factor is 2 to the power of the BATCH length of that tensor, exactly as the reference has it.  One per-channel
    affine launch (scale and shift are the same scalar for every depth; a power of two commutes with the rounding of the
    product, and the kernel multiplies, then adds, like the reference)."""
    x = stored_volume[:1]
    C_ = x.shape[1]
    scale = (torch.as_tensor(std_vols, dtype=torch.float32).reshape(()) * float(2 ** len(stored_volume))).to(x.device)
    shift = torch.as_tensor(mean_vols, dtype=torch.float32).reshape(()).to(x.device)
    return ops.channel_affine(x, scale.expand(C_).contiguous(), shift.expand(C_).contiguous())[0]


def denormalise_ground_truth(gt_volume, std_vols, mean_vols):
    """The ground-truth volume of the evaluation branch, CWFA.py:1037-1038: ``gt[0] * std + mean`` shifted so that its minimum
    is 0.  The affine is the HIP kernel; the minimum and its subtraction are two torch reductions / elementwise ops on the
    result (output bookkeeping after the path, like the metrics that follow it in the reference)."""
    x = gt_volume[:1]
    C_ = x.shape[1]
    scale = torch.as_tensor(std_vols, dtype=torch.float32).reshape(()).to(x.device)
    shift = torch.as_tensor(mean_vols, dtype=torch.float32).reshape(()).to(x.device)
    v = ops.channel_affine(x, scale.expand(C_).contiguous(), shift.expand(C_).contiguous())[0]
    return v - v.min()


# ---------------------------------------------------------------------------------------------------------------------
# Evaluation pass (CWFA.py:1032-1117): step metrics, projections, neuron traces.  Inputs are assumed finite.
# ---------------------------------------------------------------------------------------------------------------------
def _metric_scalars(sums, numel):
    """(PSNR in dB, masked MAE * 100) from the [B,4] float64 sums of ``ops.volume_metrics`` over the whole batch; PSNR with the
    ``mse == 0`` branches of utils.py:389-392."""
    sse, sg, sam, _ = sums.sum(0).tolist()
    if sse == 0:
        p = 0.0 if sg == 0 else 100.0
    else:
        p = 20.0 * math.log10(1.0 / math.sqrt(sse / numel))
    return p, sam / numel * 100.0


def _mask_threshold(max_abs_pred, ths):
    """``p.abs().max() * ths`` as the reference forms it (fp32 scalar times Python number, CWFA.py:126); ths == 0: no mask."""
    if ths == 0:
        return float("-inf")
    return float(torch.as_tensor(max_abs_pred, dtype=torch.float32).reshape(()).cpu() * ths)


def _raw_volume(x, step, mean, std, offset=None):
    """(x / 2**step) * std - mean as a tensor, bit for bit (one per-channel affine launch: the power of two commutes with the
    rounding of the product, the kernel multiplies, then adds)."""
    C_ = x.shape[1]
    scale = (torch.as_tensor(std, dtype=torch.float32).reshape(()).cpu() * (2.0 ** -int(step))).to(x.device)
    shift = (-torch.as_tensor(mean, dtype=torch.float32).reshape(()).cpu()).to(x.device)
    return ops.channel_affine(x, scale.expand(C_).contiguous(), shift.expand(C_).contiguous())


def _minus(x, value):
    """x - value (fp32 scalar) through the per-channel affine kernel: x * 1 + (-value) is exact in its first step."""
    C_ = x.shape[1]
    one = torch.ones(C_, dtype=torch.float32, device=x.device)
    return ops.channel_affine(x, one, torch.full((C_,), -float(value), dtype=torch.float32, device=x.device))


@amp_function
def compute_INN_step_performance(gt_volume_in, pred_volume_in, step, mean, std, normaliaze_before_metrics=False, ths=0.05):
    """PSNR and masked MAE ("MAPE") of one pyramid step; CWFA.py:98-132, same signature.  Returns
    ``(psnr, masked_mae * 100, gt_volume_raw, pred_volume_raw)``: the raw volumes are materialised because the signature returns
    them (``evaluate_step`` is the form that does not).  The sums are float64 device sums of one pass over both raw volumes.

    Not mirrored: the reference's bare ``except`` that returns the 5-tuple ``0, 0, 1, gt, pred``.  ``ths == 0``: the reference
    leaves ``masked_psnr`` unassigned and raises UnboundLocalError; here the mask is empty and the value is the plain MAE * 100."""
    gt_raw = _raw_volume(ops._dev(gt_volume_in, "gt_volume_in"), step, mean, std)
    pred_raw = _raw_volume(ops._dev(pred_volume_in, "pred_volume_in"), step, mean, std)
    ext = ops.volume_extrema(pred_raw, gt_raw).cpu()
    max_abs_pred = ext[:, 3].max()
    if normaliaze_before_metrics:
        gt_raw, pred_raw = _minus(gt_raw, ext[:, 4].min()), _minus(pred_raw, ext[:, 0].min())
        max_abs_pred = ops.volume_extrema(pred_raw).cpu()[:, 3].max()
    sums = ops.volume_metrics(pred_raw, gt_raw, _mask_threshold(max_abs_pred, ths))
    p, m = _metric_scalars(sums, gt_raw.numel())
    return p, m, gt_raw, pred_raw


@amp_function
def evaluate_step(gt, pred, step, mean, std, ths=0.05, projections=True, on_device=False):
    """What the body of the reference's evaluation loop (CWFA.py:1065-1085) amounts to for one pyramid step, without writing a raw
    volume: one extrema pass and one metrics pass over (pred, gt) with the de-normalisation applied on load, and one pass that
    forms the maximum projections of |pred|, |gt| and |pred - gt| together.  Returns ``(psnr, masked_mae * 100, img_pred, img_gt,
    img_diff)``: the scalars of ``compute_INN_step_performance`` and the composites ``volume_2_projections`` gives for the raw
    prediction, the raw ground truth and their absolute difference (CPU float32 [B,1,H',W'] like there; ``on_device=True`` keeps
    them on the GPU; ``projections=False``: None)."""
    from . import utils as U
    ops._dev(gt, "gt"), ops._dev(pred, "pred")
    aff = ops.eval_affine(step, mean, std)
    ext = ops.volume_extrema(pred, gt, aff).cpu()
    sums = ops.volume_metrics(pred, gt, _mask_threshold(ext[:, 3].max(), ths), aff)
    imgs = [None, None, None]
    if projections:
        U.check_layout(pred.shape, [1, 1, 2])
        zp, xp, yp, _ = ops.mip3(pred, gt, triple=True, affine=aff)
        imgs = [U.compose_projections(zp[q], xp[q], yp[q], [1, 1, 2], 2, False) for q in range(3)]
        if not on_device:
            imgs = [im.cpu() for im in imgs]
    p, m = _metric_scalars(sums, gt.numel())
    return (p, m, *imgs)


def roi_boxes(coords, shape, r12, r3, start_plane_offset=-25 // 2):
    """The index ranges of the reference's ROIs (CWFA.py:282-285) for a stack of ``shape`` [T,D,H,W]: int32 [N,6] rows
    (z0, z1, y0, y1, x0, x1), half-open, with z shifted by ``D // 2 + start_plane_offset`` (the coordinates come from the central
    25 planes of a stack).  An empty range is written as (0, 0).  Each range is clipped by the axis it indexes (the reference
    clips x by shape[2] and y by shape[3] but indexes the other way round: the same for H == W)."""
    import numpy as np
    _, D, H, W = shape
    out = np.zeros((len(coords), 6), dtype=np.int32)
    for ix, (x_coord, y_coord, z_coord) in enumerate(coords):
        z_coord = z_coord + D // 2 + start_plane_offset
        for k, (c, r, n) in enumerate(((z_coord, r3, D), (y_coord, r12, H), (x_coord, r12, W))):
            lo, hi = max(0, int(c) - r), min(n, int(c) + r)
            if hi > lo:
                out[ix, 2 * k], out[ix, 2 * k + 1] = lo, hi
    return out


def correlate_traces(coords, boxes, traces_gt, traces_pred, median_gt, depth_shift, n_time_steps, minmax_ths=50, filter_width=10):
    """The host part of ``corr_coeff_3D`` (CWFA.py:259-337) on the [N,T] ROI traces of the two max-normalised stacks and the
    median of the positive ground-truth voxels: ``norm_data``, the ``minmax < img_ths`` gate, the threshold-halving loop (the
    lists keep growing over its sweeps, as there), ``np.corrcoef``, the data frame.
    Not mirrored: the reference's bare ``try / except`` around an ROI (coefficient 0, the previous ROI's signals reused in the
    frame, a ``roi_outside`` print).  Nothing in it raises here: an empty box gives NaN traces in the reference too, which is
    what this returns."""
    import numpy as np
    from .utils import norm_data
    cols = ['patch_n', 'coord_x', 'coord_y', 'coord_z', 'corr_coeff', 'is_gt'] + [f't{t}' for t in range(n_time_steps)]
    all_corr_coeffs, rows, index = [], [], []
    required_coords = int(len(coords) * 0.2)
    n_divisions = 0
    while len(all_corr_coeffs) <= required_coords and n_divisions < 5:
        img_ths = np.float32(median_gt) * np.float32(minmax_ths)
        for ix, (x_coord, y_coord, z_coord) in enumerate(coords):
            z_coord = z_coord + depth_shift
            width = min(filter_width, int(boxes[ix, 1] - boxes[ix, 0]))          # min(filter_width, gt_data.shape[-1]): the z extent
            GT_signal, minmax = norm_data(traces_gt[ix], width)
            if minmax < img_ths:
                continue
            pred_signal, _ = norm_data(traces_pred[ix], width)
            if GT_signal.max() == 0 or pred_signal.max() == 0:
                corr_coeff = 0
            else:
                corr_coeff = np.corrcoef(GT_signal, pred_signal)[0][1]
            all_corr_coeffs.append(corr_coeff)
            for is_gt, sig in ((1, GT_signal), (0, pred_signal)):
                row = {'patch_n': ix, 'coord_x': x_coord, 'coord_y': y_coord, 'coord_z': z_coord, 'corr_coeff': corr_coeff, 'is_gt': is_gt}
                row.update({f't{t}': sig[t] for t in range(len(sig))})
                rows.append(row)
                index.append(ix)
        if len(all_corr_coeffs) <= required_coords:
            minmax_ths /= 2
            n_divisions += 1
    return all_corr_coeffs, _trace_frame(rows, index, cols)


def _trace_frame(rows, index, cols):
    import pandas as pd
    return pd.DataFrame(rows, index=index, columns=cols).astype(float)


@amp_function
def corr_coeff_3D(stack_gt, pred_3D, coords, r12, r3, n_time_steps=None, start_plane_offset=-25 // 2, output_path=None, n_show=20,
                  minmax_ths=50, filter_width=10):
    """Correlation coefficients between the ROI traces of a ground-truth and a predicted time series of volumes; CWFA.py:240-379,
    same signature, device tensors [T,D,H,W].  Returns ``(all_corr_coeffs, neural_activity_dataframe)``.

    On the GPU: the maximum of each stack, the median of the positive ground-truth voxels (exact radix selection) and the
    float64 mean of every ROI at every time step (one launch per stack and 128 ROIs).  On the host: ``correlate_traces``.
    Two departures, invisible in the results: the reference divides both stacks in place by their maxima -- here the inputs stay
    untouched and the traces and the median are scaled instead (division by a positive number is monotone, so the median of the
    scaled values is the scaled median, bit for bit); and the ROI ranges are clipped by the axis they index (see ``roi_boxes``).
    ``output_path is not None`` (the reference's figure) raises NotImplementedError.  The selection counts in 64 bits: a
    stack may hold up to 2^45 voxels per time step."""
    import numpy as np
    if output_path is not None:
        raise NotImplementedError("corr_coeff_3D: plotting (output_path) is the reference's business")
    ops._dev(stack_gt, "stack_gt"), ops._dev(pred_3D, "pred_3D")
    if stack_gt.dim() != 4 or tuple(stack_gt.shape) != tuple(pred_3D.shape):
        raise ValueError("corr_coeff_3D: two [T,D,H,W] stacks of one shape")
    if n_time_steps is None:
        n_time_steps = stack_gt.shape[0]
    coords = [tuple(c) for c in coords]
    boxes = roi_boxes(coords, stack_gt.shape, r12, r3, start_plane_offset)
    max_gt = ops.volume_extrema(stack_gt)[:, 1]
    max_pred = ops.volume_extrema(pred_3D)[:, 1]
    median, _ = ops.select_positive(stack_gt, -1)
    tr_gt, tr_pred = ops.roi_means(stack_gt, boxes), ops.roi_means(pred_3D, boxes)
    m_gt, m_pred = np.float32(max_gt.cpu().numpy().max()), np.float32(max_pred.cpu().numpy().max())
    median_scaled = np.float32(median.cpu().numpy()[0]) / m_gt                         # fp32 division: the median of stack / max
    return correlate_traces(coords, boxes, tr_gt.cpu().numpy() / np.float64(m_gt), tr_pred.cpu().numpy() / np.float64(m_pred),
                            median_scaled, stack_gt.shape[1] // 2 + start_plane_offset, n_time_steps, minmax_ths, filter_width)


# ---------------------------------------------------------------------------------------------------- neuron detection
# The producer of the ``coords`` that corr_coeff_3D, roi_boxes and the ROI posterior moments take.  The reference
# reads them from a hand-annotated file (``read_neural_coordinates_from_file``, CWFA.py:223-238) or falls back to thirteen fixed pixel
# pairs (CWFA.py:45); here they come from the recording itself: frames -> volumes -> activity map -> local maxima -> that file.
class ActivityMap:
    """Per-voxel temporal statistics of a series of [D,H,W] volumes, accumulated as the volumes are produced (by ``inverse_pass``
    or ``XLFMDeconv``), so the series never has to be resident: mean, unbiased std, maximum and minimum over time.  ``finish``'s
    mean and std are bit for bit ``ops.stack_mean_std`` of the whole series, for any chunking (the same float64 additions per voxel in
    the same order).  The state costs 28 bytes per voxel -- the first sample, two float64 sums, maximum, minimum: about 700 MB at
    96 x 512 x 512.

    ``neighbours`` = 6 (faces), 8 (the in-plane ring) or 26 (the cube) also accumulates the pair sums of the local correlation
    image: ``finish("corr")`` then scores a voxel by the mean correlation of its series with its neighbours',
    which tells a neuron (its voxels move together) from a voxel that merely fluctuates (a hot pixel, shot noise on a bright
    structure).  That adds one float64 per forward offset, K = 3, 4 or 13: the state costs 28 + 8 K bytes per voxel, 3.3 GB at
    96 x 512 x 512 for 26 neighbours.  ``neighbours=0``: no pair sums, the state and the launches above."""

    def __init__(self, shape, device, neighbours=0):
        self.shape = tuple(int(s) for s in shape)
        if len(self.shape) != 3 or min(self.shape) < 0:
            raise ValueError(f"ActivityMap: shape is (D, H, W), got {shape!r}")
        if neighbours not in (0, 6, 8, 26):
            raise ValueError(f"ActivityMap: neighbours is 0, 6, 8 or 26, got {neighbours!r}")
        self.neighbours = neighbours
        self.state = ops.activity_state(self.shape, device)
        self.cc = ops.correlation_state(self.shape, device, neighbours) if neighbours else None
        self.count = 0

    def update(self, volumes):
        """Add ``volumes``: [T',D,H,W] or one [D,H,W] volume, float32 on the device."""
        ops._dev(volumes, "volumes")
        if volumes.dim() == 3:
            volumes = volumes.unsqueeze(0)
        if volumes.dim() != 4 or tuple(volumes.shape[1:]) != self.shape:
            raise ValueError(f"ActivityMap.update: volumes of shape {self.shape} are expected, got {tuple(volumes.shape)}")
        if volumes.shape[0]:
            if self.neighbours:
                ops.activity_update_corr(volumes, self.state, self.cc, self.neighbours, first=self.count == 0)
            else:
                ops.activity_update(volumes, self.state, first=self.count == 0)
            self.count += volumes.shape[0]
        return self

    def finish(self, kind="std"):
        """(score, mean, std, vmax, vmin), float32 [D,H,W].  ``kind`` chooses the score: "std", "range" = vmax - vmin, "peak" =
        vmax - mean, "snr" = (vmax - mean) / std with 0 where std == 0, or "corr", the local correlation image over the object's
        ``neighbours`` (in [-1, 1], 0 for a pair with a constant or non-finite series; needs ``neighbours != 0``).  The state is kept:
        more volumes may follow (vmax and vmin are the state's own tensors, which a later ``update`` writes)."""
        if kind == "corr" and not self.neighbours:
            raise ValueError("ActivityMap.finish: kind 'corr' needs an ActivityMap(neighbours=6, 8 or 26)")
        if self.count < 1:
            raise ValueError("ActivityMap.finish: no volume has been added")
        score, mean, std = ops.activity_finish(self.state, self.count, "std" if kind == "corr" else kind)
        if kind == "corr":
            score = ops.correlation_finish(self.state, self.cc, self.count, self.neighbours)
        return score, mean, std, self.state[3], self.state[4]


RegressionMaps = namedtuple("RegressionMaps", ["corr", "beta", "t", "r2"])


class RegressionMap:
    """The per-voxel linear regression of a series of [D,H,W] volumes against ``n_regressors`` known time courses (1 .. 16, beside an
    implicit intercept), accumulated as the volumes are produced: which voxels follow the stimulus, the
    behaviour or a seed neuron.  A regressor is a stimulus or behaviour trace through the calcium kernel (``calcium_regressors``)
    or a neuron's own trace.  Beside the state of an ``ActivityMap`` -- kept by the same operations, so ``activity`` returns that
    object's maps from the same pass -- a voxel keeps one float64 sum per regressor: 28 + 8 K bytes per voxel, 2.3 GB at
    96 x 512 x 512 for K = 8.  Any chunking of the series gives the same bits."""

    def __init__(self, shape, device, n_regressors):
        self.shape = tuple(int(s) for s in shape)
        if len(self.shape) != 3 or min(self.shape) < 0:
            raise ValueError(f"RegressionMap: shape is (D, H, W), got {shape!r}")
        self.reg = ops.regression_state(self.shape, device, n_regressors)
        self.n_regressors = int(n_regressors)
        self.state = self.reg.plain
        self.count = 0

    def update(self, volumes, rows):
        """Add ``volumes``: [T',D,H,W] or one [D,H,W] volume, float32 on the device, with their regressor values ``rows``: float64
        [T',K] on the device ([K] for one volume)."""
        K = self.n_regressors
        if not torch.is_tensor(volumes) or not torch.is_tensor(rows):
            raise TypeError("RegressionMap.update: volumes and rows are torch tensors")
        if volumes.dim() == 3 and rows.dim() == 1:
            volumes, rows = volumes.unsqueeze(0), rows.unsqueeze(0)
        if volumes.dim() != 4 or tuple(volumes.shape[1:]) != self.shape:
            raise ValueError(f"RegressionMap.update: volumes of shape {self.shape} are expected, got {tuple(volumes.shape)}")
        if rows.dim() != 2 or rows.shape[1] != K or rows.dtype != torch.float64:
            raise ValueError(f"RegressionMap.update: rows is a float64 tensor [T', {K}], got {tuple(rows.shape)} {rows.dtype}")
        if rows.shape[0] != volumes.shape[0]:
            raise ValueError(f"RegressionMap.update: {rows.shape[0]} rows for {volumes.shape[0]} volumes")
        ops._dev(volumes, "volumes")
        if volumes.shape[0]:
            first = self.count == 0
            ops.activity_update_regress(volumes, rows, self.reg, first=first)
            ops.regress_rows(rows, self.reg, first=first)
            self.count += volumes.shape[0]
        return self

    def finish(self, want=("corr", "beta", "t", "r2"), rcond=1e-10):
        """``RegressionMaps(corr, beta, t, r2)``, float32: per regressor [K,D,H,W] the correlation of the series with it, its
        coefficient in the joint fit and that coefficient's t-statistic (N - K - 1 degrees of freedom, white residuals), and
        [D,H,W] the fit's R^2; ``None`` for what ``want`` does not name.  A voxel whose series is constant or holds NaN or inf is 0
        in every map.  Raises ``ValueError`` when a regressor is constant, a combination of the others (a Cholesky pivot not above
        ``rcond`` times its diagonal entry) or not finite.  The state is kept: more volumes may follow."""
        if self.count < 1:
            raise ValueError("RegressionMap.finish: no volume has been added")
        ops.regress_want(want, self.count, self.n_regressors, "RegressionMap.finish")
        design = ops.regress_design(self.reg, self.count, rcond)
        code, k = (int(v) for v in design.status.cpu())
        if code:
            raise ValueError(f"RegressionMap.finish: collinear or constant regressor {k} "
                             f"({ops._lib.REGRESS_STATUS.get(code, code)}; rcond = {rcond:g})")
        return RegressionMaps(*ops.regress_finish(self.reg, design, self.count, want))

    def activity(self, kind="std"):
        """What ``ActivityMap.finish(kind)`` returns from the same state: (score, mean, std, vmax, vmin)."""
        if kind == "corr":
            raise ValueError("RegressionMap.activity: the local correlation image is an ActivityMap(neighbours=...)'s")
        if self.count < 1:
            raise ValueError("RegressionMap.activity: no volume has been added")
        score, mean, std = ops.activity_finish(self.state, self.count, kind)
        return score, mean, std, self.state[3], self.state[4]


@amp_region
def calcium_regressors(events, gamma, device="cuda"):
    """The regressors of a ``RegressionMap`` from event or stimulus time courses: every column of ``events`` ([T,K], or [T] for one)
    through the AR(1) calcium kernel ``infer_spikes`` assumes, c[t] = gamma c[t-1] + e[t] in float64 from c[-1] = 0.  Returns the
    float64 [T,K] tensor on ``device`` whose row slices go to ``RegressionMap.update``.  A host helper: T K values need no kernel."""
    import numpy as np
    e = np.asarray(events.detach().cpu().numpy() if torch.is_tensor(events) else events, dtype=np.float64)
    if e.ndim == 1:
        e = e[:, None]
    if e.ndim != 2:
        raise ValueError(f"calcium_regressors: events is [T] or [T,K], got {e.shape}")
    g = float(gamma)
    if not 0.0 <= g < 1.0:
        raise ValueError(f"calcium_regressors: gamma is in [0, 1), got {gamma!r}")
    c = np.empty_like(e)
    prev = np.zeros(e.shape[1])
    for t in range(e.shape[0]):
        prev = g * prev + e[t]
        c[t] = prev
    return torch.from_numpy(c).to(device)


def find_neurons(score, r12=5, r3=3, n_max=None, thr=None, rel_thr=0.1, start_plane_offset=-25 // 2, margin=None, dist=None, kind="std",
                 *, regressor=None):
    """Neuron positions as the 3-D local maxima of an activity map: ``(coords, scores)``.

    ``score``: a float32 device map [D,H,W], or an ``ActivityMap``, which is finished with ``kind`` (used in that case only; "corr"
    for the local correlation image of an ``ActivityMap(neighbours=...)``), or a ``RegressionMap``: ``kind`` = "t", "corr" or "beta"
    then takes that map of regressor ``regressor`` (the neurons tuned to it; an absolute ``thr`` is the natural argument for "t"
    and "corr"), any other ``kind`` the activity map of the same state.  A voxel is kept when it is at
    least ``thr`` (default ``rel_thr`` times the map's maximum), at least ``margin`` (default ``(r3, r12, r12)``) from every face and
    the maximum of the box of half-widths ``dist`` (default ``(2 r3 - 1, 2 r12 - 1, 2 r12 - 1)``) around it, ties going to the
    lowest linear index (``ops.local_maxima``); the ``n_max`` highest are returned, by descending score.  With the default ``dist`` two
    detections differ by at least 2 r on one axis, so their ROIs [c - r, c + r) are disjoint.  On a correlation map ``rel_thr`` is
    relative to a maximum near 1 whatever the recording, so an absolute ``thr`` (0.5, say) is the natural argument there.

    ``coords`` is a list of ``[x, y, z - (D // 2 + start_plane_offset)]`` (x indexes W, y indexes H): the convention of the
    reference's coordinates file, which ``roi_boxes(coords, shape, r12, r3, start_plane_offset)``, ``corr_coeff_3D`` and
    ``posterior_roi_moments`` take as it is.  ``scores``: float32 numpy array, the map's values at the peaks."""
    r12, r3 = int(r12), int(r3)
    if r12 < 1 or r3 < 1:
        raise ValueError("find_neurons: r12 and r3 are positive ROI half-widths")
    dist = (2 * r3 - 1, 2 * r12 - 1, 2 * r12 - 1) if dist is None else dist
    margin = (r3, r12, r12) if margin is None else margin
    dist, margin, n_max, _ = ops.local_maxima_args(dist, margin, n_max, 0, "find_neurons")
    if thr is None and not 0.0 <= float(rel_thr) <= 1.0:
        raise ValueError(f"find_neurons: rel_thr = {rel_thr} is not in [0, 1]")
    if isinstance(score, RegressionMap):
        if kind in ("t", "corr", "beta"):
            if isinstance(regressor, bool) or not isinstance(regressor, int) or not 0 <= regressor < score.n_regressors:
                raise ValueError(f"find_neurons: regressor is 0 .. {score.n_regressors - 1} for kind {kind!r}, got {regressor!r}")
            score = getattr(score.finish(want=(kind,)), kind)[regressor]
        else:
            score = score.activity(kind)[0]
    elif regressor is not None:
        raise ValueError("find_neurons: regressor is for a RegressionMap")
    if isinstance(score, ActivityMap):
        score = score.finish(kind)[0]
    ops._dev(score, "score")
    if score.dim() != 3:
        raise ValueError(f"find_neurons: a [D,H,W] map is expected, got {tuple(score.shape)}")
    if thr is None:
        thr = float(rel_thr) * float(ops.volume_extrema(score.unsqueeze(0))[0, 1].cpu()) if score.numel() else 0.0
    zyx, scores, _ = ops.local_maxima(score, thr, dist, margin, n_max)
    shift = score.shape[0] // 2 + int(start_plane_offset)
    return [[int(x), int(y), int(z) - shift] for z, y, x in zyx], scores


# ---------------------------------------------------------------------------------------------------- registration of volumes
# In front of everything that works per voxel over time: the rigid registration of section 26 carried to
# [N,D,H,W] stacks -- for volumes whose frames are gone, for comparing two reconstructions of one frame, and for motion the fan model
# of section 29 does not hold.
VolumeRegistration = namedtuple("VolumeRegistration", ["volumes", "shifts", "peak", "template"])


def _vol_reg_args(volumes, template, max_shift, taper, smooth, eps, chunk, subpixel, what):
    """The checks of ``estimate_volume_shifts`` that need no device, those of ``XLFMDataset._reg_args`` and the refusal of the
    up-sampled DFT: ((mz, my, mx), (tz, ty, tx), chunk)."""
    args = _reg_args(volumes, template, max_shift, taper, smooth, eps, chunk, what, "volume")[:3]
    if isinstance(subpixel, str):
        if subpixel == "dft":
            raise ValueError(f"{what}: subpixel='dft' (the up-sampled DFT of section 26.5) is not built for volumes; True fits a parabola per axis")
        raise ValueError(f"{what}: subpixel is True or False, got {subpixel!r}")
    return args


@amp_region
def estimate_volume_shifts(volumes, template, max_shift=(2, 8, 8), taper=None, smooth=0.0, eps=1e-5, subpixel=True, chunk=1):
    """(shifts float32 [N,3] as (dz, dy, dx), peak float32 [N]) on the device: the rigid displacement of every volume of a contiguous
    [N,D,H,W] float32 device stack against the float32 ``template`` [D,H,W] by phase correlation, the steps of
    ``XLFMDataset.estimate_shifts`` over three axes.  A volume that is the template displaced by d (volume[p] = template[p - d])
    reports d; ``shift_volumes`` undoes it.  ``peak`` is the correlation value at the integer peak.  Nothing is read back.

    Both get a raised-cosine edge taper (``taper``: None for min(16, side / 8) per axis, an int, or (tz, ty, tx); 0: none); the
    spectra (``rfftn`` over the last three axes) are whitened separately, F / (|F| + ``eps``), multiplied, optionally low-passed by a
    Gaussian of ``smooth`` voxels, and transformed back; the peak is searched over |d| <= ``max_shift`` (an int or (mz, my, mx)) and,
    with ``subpixel``, refined by a parabola per axis.  ``subpixel="dft"`` is refused: it is not built for volumes.  The volumes go
    through in chunks of ``chunk`` (a chunk's spectra are chunk x D x H x (W/2+1) x 8 bytes: 101 MB per 96 x 512 x 512 volume)."""
    what = "estimate_volume_shifts"
    m, taper, chunk = _vol_reg_args(volumes, template, max_shift, taper, smooth, eps, chunk, subpixel, what)
    if template is None:
        raise ValueError(f"{what}: a template is needed")
    w = [taper_window(n, t).to(volumes.device) for n, t in zip(volumes.shape[1:], taper)]
    return _estimate(lambda s, e, out: ops.reg_window3d(volumes[s:e], *w, out=out), ops.reg_window3d(template.contiguous()[None], *w)[0],
                     int(volumes.shape[0]), tuple(int(n) for n in volumes.shape[1:]), m, smooth, eps, bool(subpixel), False, None, chunk)


def _shift_volume_args(volumes, shifts, mode, out, what):
    if not torch.is_tensor(volumes) or volumes.dim() != 4 or not volumes.is_contiguous():
        raise ValueError(f"{what}: a contiguous [N,D,H,W] stack is expected")
    if volumes.dtype != torch.float32:
        raise ValueError(f"{what}: a float32 stack is expected, got {volumes.dtype}")
    ops._shift_mode(mode, what, plain=True)
    if shifts is not None and (not torch.is_tensor(shifts) or tuple(shifts.shape) != (int(volumes.shape[0]), 3) or shifts.dtype != torch.float32):
        raise ValueError(f"{what}: shifts is a float32 [{int(volumes.shape[0])}, 3] tensor")
    if out is not None and (out is volumes or (torch.is_tensor(out) and ops._overlap(out, volumes))):
        raise ValueError(f"{what}: out must not alias volumes")


@amp_region
def shift_volumes(volumes, shifts, mode="bilinear", fill=0.0, out=None):
    """out[n,z,y,x] = volumes[n, z + dz, y + dy, x + dx] with (dz, dy, dx) = shifts[n] (float32 [N,3] on the device, as
    ``estimate_volume_shifts`` returns them): trilinear ("bilinear" in every plane, blended along z), or ``mode="nearest"``; voxels
    from outside the volume are ``fill``.  An integer shift copies bits.  ``out`` must not share memory with ``volumes``."""
    _shift_volume_args(volumes, shifts, mode, out, "shift_volumes")
    return ops.reg_shift3d(volumes, shifts, mode=mode, fill=fill, out=out)


def _volume_median(volumes):
    """The per-voxel lower temporal median of a contiguous [N,D,H,W] stack."""
    N = int(volumes.shape[0])
    return ops.temporal_select(volumes.view(N, -1), [quantile_rank(0.5, N)])[0].view(volumes.shape[1:])


@amp_region
def register_volumes(volumes, template=None, n_iter=1, max_shift=(2, 8, 8), subpixel=True, mode="bilinear", taper=None, smooth=0.0, eps=1e-5,
                     chunk=1, fill=0.0, out=None):
    """Rigid registration of a contiguous [N,D,H,W] float32 device stack:
    ``VolumeRegistration(volumes, shifts, peak, template)`` with volumes[n] = the input's volume n moved back by shifts[n].
    ``template`` None: the per-voxel lower temporal median of the stack (usable where most volumes rest: section 26.4).
    ``n_iter`` > 1: the template becomes the median of the registered stack and the shifts are estimated again FROM THE ORIGINAL
    VOLUMES, so interpolation never compounds.  The other arguments are those of ``estimate_volume_shifts`` and ``shift_volumes``.
    Nothing is read back."""
    what = "register_volumes"
    _vol_reg_args(volumes, template, max_shift, taper, smooth, eps, chunk, subpixel, what)
    _register_args(volumes, n_iter, mode, out, what, "volume")
    estimate = lambda tmpl: estimate_volume_shifts(volumes, tmpl, max_shift=max_shift, taper=taper, smooth=smooth, eps=eps, subpixel=subpixel, chunk=chunk)
    out, (shifts, peak), tmpl = _register(volumes, template, n_iter, _volume_median, estimate,
                                          lambda est, out: shift_volumes(volumes, est[0], mode=mode, fill=fill, out=out), out)
    return VolumeRegistration(out, shifts, peak, tmpl)


class _StreamingRegistrar:
    """What the streaming registrars share: the checks of the template, ``mode`` and the estimate's arguments on a probe of no volumes,
    the call on a chunk or on one [D,H,W] volume, and the accessors.  A subclass names its device lists (``_lists``: what its
    estimate returns, in that order; the first is what moves the volumes) and states ``_check``, ``_estimate`` and ``_move``."""

    def __init__(self, template, mode, fill, estimate_args):
        what = type(self).__name__
        ops._dev(template, "template")
        if template.dim() != 3:
            raise ValueError(f"{what}: the template is a float32 [D,H,W] tensor, got {tuple(template.shape)}")
        ops._shift_mode(mode, what, plain=True)
        self.template, self.mode, self.fill, self.estimate_args = template.contiguous(), mode, float(fill), dict(estimate_args)
        a = self.estimate_args.get
        probe = torch.empty((0,) + tuple(template.shape), dtype=torch.float32, device=template.device)
        self._check(probe, (a("max_shift", (2, 8, 8)), a("taper"), a("smooth", 0.0), a("eps", 1e-5), a("chunk", 1), a("subpixel", True)), a, what)
        for name in self._lists:
            setattr(self, name, [])

    def __call__(self, volumes, out=None):
        single = torch.is_tensor(volumes) and volumes.dim() == 3
        if single:
            volumes = volumes.unsqueeze(0)
        est = self._estimate(volumes)
        moved = self._move(volumes, est[0], out)
        for name, t in zip(self._lists, est):
            getattr(self, name).append(t)
        return moved[0] if single else moved

    def _all(self, name, tail, dtype=torch.float32):
        """The list ``name`` concatenated, or the empty [0, *tail] tensor of ``dtype`` where no volume has been seen."""
        got = getattr(self, name)
        return torch.cat(got) if got else torch.empty((0, *tail), dtype=dtype, device=self.template.device)


class VolumeRegistrar(_StreamingRegistrar):
    """Registration of a series that is never resident, against a fixed float32 ``template`` [D,H,W]: ``reg(chunk)`` returns the
    registered [T',D,H,W] chunk (or volume, for one [D,H,W] volume) and appends the chunk's shifts and peaks to the device lists
    ``reg.shifts`` and ``reg.peak``; nothing is read back inside the call.  ``all_shifts()`` / ``all_peaks()`` concatenate them
    ([N,3], [N]); pass the former to ``valid_box``.  ``estimate_args``: those of ``estimate_volume_shifts``; ``mode`` and ``fill``:
    those of ``shift_volumes``.  This is how ``ActivityMap`` and ``NeuronFootprints`` are fed::

        reg = VolumeRegistrar(template, max_shift=(2, 8, 8))
        for cond in batches:
            fp.update(reg(inverse_pass(conv_inn, cond_nets, cond, mean_vols_cache)[:, 0]))
        box = valid_box(reg.all_shifts(), template.shape)      # the one read-back, after the loop
    """

    _lists = ("shifts", "peak")

    def __init__(self, template, mode="bilinear", fill=0.0, **estimate_args):
        super().__init__(template, mode, fill, estimate_args)

    def _check(self, probe, common, a, what):
        _vol_reg_args(probe, self.template, *common, what)

    def _estimate(self, volumes):
        return estimate_volume_shifts(volumes, self.template, **self.estimate_args)

    def _move(self, volumes, shifts, out):
        return shift_volumes(volumes, shifts, mode=self.mode, fill=self.fill, out=out)

    def all_shifts(self):
        """float32 [N,3] on the device: the shifts of every volume seen so far."""
        return self._all("shifts", (3,))

    def all_peaks(self):
        """float32 [N] on the device: the correlation peaks of every volume seen so far."""
        return self._all("peak", ())


def valid_box(shifts, shape):
    """(z0, z1, y0, y1, x0, x1): the box of a volume of ``shape`` (D, H, W) in which every volume registered with ``shifts`` [N,3]
    holds data and no ``fill`` -- planes z0 .. z1 - 1, rows y0 .. y1 - 1, columns x0 .. x1 - 1 -- all 0 where a shift is not finite
    or nothing is left.  A host helper: it reads the shifts back.  A detection whose ROI leaves the box saw ``fill`` in some
    volume; ``find_neurons(score, r12, r3, margin=(max(r3, z0, D - z1), max(r12, y0, H - y1), max(r12, x0, W - x1)))`` keeps every
    ROI inside it."""
    dims = tuple(int(v) for v in shape)
    if len(dims) != 3:
        raise ValueError(f"valid_box: shape is (D, H, W), got {shape!r}")
    s = torch.as_tensor(shifts).detach().to("cpu", torch.float64).reshape(-1, 3)
    if s.numel() == 0:
        return 0, dims[0], 0, dims[1], 0, dims[2]
    if not bool(torch.isfinite(s).all()):
        return (0,) * 6
    lo, hi = torch.floor(s).amin(0), torch.ceil(s).amax(0)
    box = []
    for a, side in enumerate(dims):
        b0, b1 = max(0, int(-lo[a])), min(side, side - int(hi[a]))
        if b1 <= b0:
            return (0,) * 6
        box += [b0, b1]
    return tuple(box)


# ---------------------------------------------------------------------------------------------------- piecewise-rigid registration
# For a sample whose parts move differently: the volume is cut into a grid of blocks, every block is registered
# like a volume of section 30, the table of block shifts is cleaned once and interpolated between the block centres, and the volume
# is resampled once under a displacement per voxel.
PiecewiseRegistration = namedtuple("PiecewiseRegistration", ["volumes", "field", "peak", "inlier", "shifts", "template"])


class BlockGrid:
    """The geometry ``block_grid`` makes, on the host: ``shape`` (D, H, W), ``block`` (bz, by, bx), ``grid`` (gz, gy, gx), ``B`` their
    product, and per axis ``origins`` (int32 [g]), ``centers`` (float64 [g]) and the interpolation tables ``idx`` (int32 [S]) and
    ``t`` (float32 [S]).  ``tables(device)``: (idxz, tz, idxy, ty, idxx, tx) on the device, copied once per device."""

    def __init__(self, shape, block, grid, origins, centers, idx, t):
        self.shape, self.block, self.grid, self.origins, self.centers, self.idx, self.t = shape, block, grid, origins, centers, idx, t
        self.B = grid[0] * grid[1] * grid[2]
        self._dev = {}

    def tables(self, device):
        key = str(torch.device(device))
        if key not in self._dev:
            self._dev[key] = tuple(torch.from_numpy(a).to(device) for pair in zip(self.idx, self.t) for a in pair)
        return self._dev[key]

    def windows(self, taper, device):
        """The three raised-cosine tapers of a block on the device, copied once per (taper, device)."""
        key = (tuple(taper), str(torch.device(device)))
        if key not in self._dev:
            self._dev[key] = tuple(taper_window(n, t).to(device) for n, t in zip(self.block, taper))
        return self._dev[key]


def block_grid(shape, block=(32, 128, 128), grid=None, device=None):
    """The ``BlockGrid`` of a volume of ``shape`` (D, H, W) cut into ``grid`` = (gz, gy, gx) blocks of ``block`` = (bz, by, bx) voxels
    (clipped to the volume; ``grid`` None: ceil(S / b) per axis; at most 4096 blocks) -- DESIGN.md section 32, all on the host in
    integers and float64.  Along an axis of S voxels the origins are (i (S - b)) // (g - 1), i = 0 .. g - 1 (one block: (S - b) // 2),
    so the first and last block touch the faces and blocks overlap or leave gaps as the sizes ask; a centre is origin + (b - 1) / 2;
    coordinate p interpolates between the centres around it -- node idx[p], the last centre at or below p, and the fraction
    t[p] = float32((p - c[idx]) / (c[idx + 1] - c[idx])) -- and takes the end centre's vector beyond it (t = 0).  ``device``: copy the
    tables there now; otherwise they are copied at their first use."""
    import numpy as np
    what = "block_grid"
    if not isinstance(shape, (tuple, list, torch.Size)) or len(shape) != 3:
        raise ValueError(f"{what}: shape is (D, H, W), got {shape!r}")
    shape = tuple(ops._count(s, "shape", what) for s in shape)
    if not isinstance(block, (tuple, list, torch.Size)) or len(block) != 3:
        raise ValueError(f"{what}: block is (bz, by, bx), got {block!r}")
    block = tuple(min(ops._count(b, "block", what), s) for b, s in zip(block, shape))
    grid = ops._block_grid3(tuple(-(-s // b) for s, b in zip(shape, block)) if grid is None else grid, what)
    origins, centers, idx, t = [], [], [], []
    for S, b, g in zip(shape, block, grid):
        o = np.array([(i * (S - b)) // (g - 1) for i in range(g)] if g > 1 else [(S - b) // 2], dtype=np.int64)
        c = o.astype(np.float64) + (b - 1) / 2.0
        p = np.arange(S, dtype=np.float64)
        i = np.clip(np.searchsorted(c, p, side="right") - 1, 0, g - 1)
        inner = (p > c[0]) & (p < c[g - 1])
        nxt = np.minimum(i + 1, g - 1)
        with np.errstate(all="ignore"):
            frac = ((p - c[i]) / (c[nxt] - c[i])).astype(np.float32)
        origins.append(o.astype(np.int32))
        centers.append(c)
        idx.append(np.where(p <= c[0], 0, np.where(p >= c[g - 1], g - 1, i)).astype(np.int32))
        t.append(np.where(inner, frac, np.float32(0)).astype(np.float32))
    bg = BlockGrid(shape, block, grid, tuple(origins), tuple(centers), tuple(idx), tuple(t))
    if device is not None:
        bg.tables(device)
    return bg


def _grid_arg(grid, what, volumes=None):
    """``grid`` is a ``BlockGrid``, made for the shape of ``volumes`` [N,D,H,W] where they are given."""
    if not isinstance(grid, BlockGrid):
        raise ValueError(f"{what}: grid is the BlockGrid of block_grid")
    if volumes is not None and tuple(int(n) for n in volumes.shape[1:]) != grid.shape:
        raise ValueError(f"{what}: the grid was made for volumes of {grid.shape}, got {tuple(volumes.shape[1:])}")


def _block_reg_args(volumes, template, grid, max_shift, taper, smooth, eps, chunk, subpixel, what):
    """The checks of ``estimate_block_shifts`` that need no device: those of ``estimate_volume_shifts`` for the stack and the template,
    and max_shift and taper against the BLOCK's sides: ((mz, my, mx), (tz, ty, tx), chunk)."""
    _vol_reg_args(volumes, template, 0, 0, smooth, eps, chunk, subpixel, what)
    _grid_arg(grid, what, volumes)
    probe = torch.empty((0, *grid.block), dtype=torch.float32)
    try:
        return _reg_args(probe, None, max_shift, taper, smooth, eps, chunk, what, "volume")[:3]
    except ValueError as e:
        raise ValueError(f"{e} (the volume here is a block of the grid)") from None


def _min_peak_args(min_peak, max_dev, what):
    min_peak = float(min_peak)
    if min_peak != min_peak:
        raise ValueError(f"{what}: min_peak is NaN")
    if max_dev is not None:
        try:
            max_dev = tuple(float(v) for v in ((max_dev,) * 3 if isinstance(max_dev, (int, float)) else max_dev))
        except (TypeError, ValueError):
            max_dev = ()
        if len(max_dev) != 3 or not all(v >= 0.0 for v in max_dev):
            raise ValueError(f"{what}: max_dev is None, a number or (dz, dy, dx), not negative and not NaN")
    return min_peak, max_dev


def _block_table(volumes, template, grid, m, taper, smooth, eps, subpixel, chunk, chunk_of=None):
    """(shifts float32 [N B, 3], peak float32 [N B]): the table of block shifts as measured -- no clean-up, no whole-volume estimate.
    ``chunk_of(s, e)``: the volumes s .. e - 1 the blocks are cut from, where they are not ``volumes[s:e]`` themselves."""
    w = grid.windows(taper, volumes.device)
    source = (lambda s, e: volumes[s:e]) if chunk_of is None else chunk_of
    return _estimate(lambda s, e, out: ops.reg_window_blocks3d(source(s, e), grid.origins, grid.block, *w, out=out),
                     ops.reg_window_blocks3d(template.contiguous()[None], grid.origins, grid.block, *w)[0], int(volumes.shape[0]), grid.block, m, smooth,
                     eps, bool(subpixel), False, None, chunk)


def _block_estimate(volumes, template, grid, max_shift, taper, smooth, eps, subpixel, min_peak, max_dev, base, chunk, what):
    """(field, peak, inlier, raw shifts), [N,gz,gy,gx,..]: ``estimate_block_shifts`` and the table before its clean-up."""
    m, taper, chunk = _block_reg_args(volumes, template, grid, max_shift, taper, smooth, eps, chunk, subpixel, what)
    min_peak, max_dev = _min_peak_args(min_peak, max_dev, what)
    if template is None:
        raise ValueError(f"{what}: a template is needed")
    N = int(volumes.shape[0])
    if base is not None and (not torch.is_tensor(base) or tuple(base.shape) != (N, 3) or base.dtype != torch.float32):
        raise ValueError(f"{what}: base is a float32 [{N}, 3] tensor")
    ops._dev(volumes, "volumes")
    shifts, peak = _block_table(volumes, template, grid, m, taper, smooth, eps, subpixel, chunk)
    if base is None:
        base = estimate_volume_shifts(volumes, template, max_shift=m, taper=taper, smooth=smooth, eps=eps, subpixel=subpixel, chunk=chunk)[0]
    field, inlier = ops.reg_field_fill(shifts.view(N, grid.B, 3), peak.view(N, grid.B), base, grid.grid, min_peak, max_dev)
    g = grid.grid
    return field.view(N, *g, 3), peak.view(N, *g), inlier.view(N, *g), shifts.view(N, *g, 3)


@amp_region
def estimate_block_shifts(volumes, template, grid, max_shift=(2, 8, 8), taper=None, smooth=0.0, eps=1e-5, subpixel=True, min_peak=0.0, max_dev=None,
                          base=None, chunk=1):
    """(field float32 [N,gz,gy,gx,3], peak float32 [N,gz,gy,gx], inlier uint8 [N,gz,gy,gx]) on the device: the displacement (dz, dy,
    dx) of every block of ``grid`` (a ``BlockGrid``) of every volume of a contiguous [N,D,H,W] float32 device stack against the same
    block of the float32 ``template`` [D,H,W].  The blocks are cut and tapered in one read (``taper``: that of
    ``estimate_volume_shifts`` at the BLOCK's size) and go through the transforms, the whitening, the peak search over |d| <=
    ``max_shift`` and the parabola of ``estimate_volume_shifts`` as a batch, ``chunk`` volumes (chunk x B blocks) at a time;
    ``subpixel="dft"`` is refused as there.  The shifts are TOTAL displacements of the original volume, not residuals after a rigid
    pass, so ``warp_volumes`` interpolates a volume once.

    The table is then cleaned once: a block is an inlier when its peak is finite and >= ``min_peak``, its shift is finite and, with
    ``max_dev`` (a number or (dz, dy, dx)), within that of ``base`` per component; an outlier takes the mean of the inliers among
    its 26 grid neighbours, or ``base`` where it has none.  ``base`` float32 [N,3]: None is the whole-volume rigid estimate of
    ``estimate_volume_shifts`` under the same arguments.  Nothing is read back."""
    return _block_estimate(volumes, template, grid, max_shift, taper, smooth, eps, subpixel, min_peak, max_dev, base, chunk, "estimate_block_shifts")[:3]


def _field_arg(volumes, field, grid, what):
    _grid_arg(grid, what, volumes)
    N = int(volumes.shape[0])
    if not torch.is_tensor(field) or field.dtype != torch.float32 or tuple(field.shape) not in ((N, *grid.grid, 3), (N, grid.B, 3)):
        raise ValueError(f"{what}: field is a float32 {[N, *grid.grid, 3]} tensor")
    return field.reshape(N, grid.B, 3)


@amp_region
def warp_volumes(volumes, field, grid, mode="bilinear", fill=0.0, out=None):
    """out[n,z,y,x] = volumes[n, z + dz, y + dy, x + dx] with (dz, dy, dx) the trilinear interpolation of ``field`` (float32
    [N,gz,gy,gx,3] on the device, as ``estimate_block_shifts`` returns it) between the block centres of ``grid`` at that voxel, the
    end centre's vector beyond it; the resampling of a voxel is ``shift_volumes``' under its vector ("bilinear" or "nearest", ``fill``
    outside the volume, a non-finite vector fills the voxel), so a field of equal nodes gives ``shift_volumes`` bit for bit and a
    region of constant integer field copies bits.  ``out`` must not share memory with ``volumes``.

    The interpolated vector is a convex combination of node vectors (up to rounding), so ``valid_box(field.reshape(-1, 3), shape)``
    bounds the box that holds data in every volume."""
    _shift_volume_args(volumes, None, mode, out, "warp_volumes")
    return ops.reg_warp3d(volumes, _field_arg(volumes, field, grid, "warp_volumes"), grid.grid, grid.tables(volumes.device), mode=mode, fill=fill, out=out)


@amp_region
def register_volumes_piecewise(volumes, template=None, grid=None, block=(32, 128, 128), n_iter=1, max_shift=(2, 8, 8), subpixel=True, mode="bilinear",
                               taper=None, smooth=0.0, eps=1e-5, min_peak=0.0, max_dev=None, chunk=1, fill=0.0, out=None):
    """Piecewise-rigid registration of a contiguous [N,D,H,W] float32 device stack:
    ``PiecewiseRegistration(volumes, field, peak, inlier, shifts, template)`` with volumes[n] = the input's volume n moved back under
    the interpolated ``field`` [N,gz,gy,gx,3]; ``shifts`` is the table as measured, before the clean-up.  ``grid``: a ``BlockGrid``, or
    (gz, gy, gx) / None for ``block_grid(shape, block, grid)``.  ``template`` None: the per-voxel lower temporal median; ``n_iter`` > 1:
    the template becomes the median of the registered stack and the field is estimated again FROM THE ORIGINAL VOLUMES.  The other
    arguments are those of ``estimate_block_shifts`` and ``warp_volumes``; ``valid_box(field.reshape(-1, 3), shape)`` is the box that
    holds data in every volume.  Nothing is read back."""
    what = "register_volumes_piecewise"
    _vol_reg_args(volumes, template, 0, 0, smooth, eps, chunk, subpixel, what)
    if not isinstance(grid, BlockGrid):
        grid = block_grid(tuple(int(n) for n in volumes.shape[1:]), block, grid)
    _block_reg_args(volumes, template, grid, max_shift, taper, smooth, eps, chunk, subpixel, what)
    _min_peak_args(min_peak, max_dev, what)
    _register_args(volumes, n_iter, mode, out, what, "volume")
    estimate = lambda tmpl: _block_estimate(volumes, tmpl, grid, max_shift, taper, smooth, eps, subpixel, min_peak, max_dev, None, chunk, what)
    out, (field, peak, inlier, shifts), tmpl = _register(volumes, template, n_iter, _volume_median, estimate,
                                                         lambda est, out: warp_volumes(volumes, est[0], grid, mode=mode, fill=fill, out=out), out)
    return PiecewiseRegistration(out, field, peak, inlier, shifts, tmpl)


class PiecewiseVolumeRegistrar(_StreamingRegistrar):
    """The streaming twin of ``VolumeRegistrar`` for piecewise-rigid motion: ``reg(chunk)`` returns the registered [T',D,H,W] chunk (or
    volume, for one [D,H,W] volume) against the fixed float32 ``template`` [D,H,W] on the ``BlockGrid`` ``grid`` and appends the
    chunk's field, peaks and inlier map to the device lists ``reg.field``, ``reg.peak`` and ``reg.inlier``; nothing is read back inside
    the call.  ``all_fields()`` concatenates the fields ([N,gz,gy,gx,3]); ``estimate_args``: those of ``estimate_block_shifts``;
    ``mode`` and ``fill``: those of ``warp_volumes``::

        reg = PiecewiseVolumeRegistrar(template, block_grid(template.shape, (32, 128, 128)), max_shift=(2, 8, 8))
        for cond in batches:
            am.update(reg(inverse_pass(conv_inn, cond_nets, cond, mean_vols_cache)[:, 0]))
        box = valid_box(reg.all_fields().reshape(-1, 3), template.shape)      # the one read-back, after the loop
    """

    _lists = ("field", "peak", "inlier")

    def __init__(self, template, grid, mode="bilinear", fill=0.0, **estimate_args):
        self.grid = grid
        super().__init__(template, mode, fill, estimate_args)

    def _check(self, probe, common, a, what):
        _block_reg_args(probe, self.template, self.grid, *common, what)
        _min_peak_args(a("min_peak", 0.0), a("max_dev"), what)

    def _estimate(self, volumes):
        return estimate_block_shifts(volumes, self.template, self.grid, **self.estimate_args)

    def _move(self, volumes, field, out):
        return warp_volumes(volumes, field, self.grid, mode=self.mode, fill=self.fill, out=out)

    def all_fields(self):
        """float32 [N,gz,gy,gx,3] on the device: the field of every volume seen so far."""
        return self._all("field", (*self.grid.grid, 3))

    def all_peaks(self):
        """float32 [N,gz,gy,gx] on the device: the correlation peak of every block seen so far."""
        return self._all("peak", self.grid.grid)


# ---------------------------------------------------------------------------------------------------- rigid registration with rotation
# For a sample that turns about the optical axis: the table of block shifts of section 32 is fitted by
# "rotation about z + 3-D shift", five float64 numbers (dz, dy, dx, c, s) per volume, and the volume is resampled once under them.
RigidFit = namedtuple("RigidFit", ["params", "inlier"])
RigidRegistration = namedtuple("RigidRegistration", ["volumes", "params", "peak", "inlier", "shifts", "template"])


def _rigid_center(center, shape, what):
    """(cy, cx) as the resampling kernel takes them: two finite numbers rounded to float32, the centre of the plane where None."""
    cy, cx = ops._rigid_center(center, shape, what)
    c = torch.tensor([cy, cx], dtype=torch.float32)
    return float(c[0]), float(c[1])


def _rigid_arms(grid, center, device):
    """float64 [B,2] on the device: block centre minus rotation centre, (y, x), block b = (iz gy + iy) gx + ix."""
    gz, gy, gx = grid.grid
    ay = torch.from_numpy(grid.centers[1]).to(torch.float64) - center[0]
    ax = torch.from_numpy(grid.centers[2]).to(torch.float64) - center[1]
    arms = torch.stack((ay[None, :, None].expand(gz, gy, gx), ax[None, None, :].expand(gz, gy, gx)), dim=-1)
    return arms.reshape(grid.B, 2).contiguous().to(device)


def _rigid_fit_args(min_peak, reject, what):
    min_peak, reject = float(min_peak), float(reject)
    if not min_peak >= 0.0 or not reject >= 0.0:
        raise ValueError(f"{what}: min_peak and reject are not negative and not NaN, got {min_peak}, {reject}")
    return min_peak, reject


def _rigid_params_arg(params, N, what, name="params"):
    if not torch.is_tensor(params) or tuple(params.shape) != (N, 5) or params.dtype != torch.float64:
        raise ValueError(f"{what}: {name} is a float64 [{N}, 5] tensor of (dz, dy, dx, c, s)")


def fit_rigid_motion(shifts, peak, grid, center=None, min_peak=0.0, reject=1.0, prior=None):
    """``RigidFit(params, inlier)`` from a table of block shifts (float32 [N,gz,gy,gx,3] or [N,B,3], as measured on the ``BlockGrid``
    ``grid``) and its peaks: per volume the motion (dz, dy, dx, c, s) -- a rotation about z by the angle of cosine c and sine s around
    ``center`` (cy, cx; None: the centre of the plane) plus a 3-D shift -- that explains the table best, a Procrustes fit in float64
    over the blocks whose peak is finite and >= ``min_peak`` with one rejection pass at ``reject`` voxels.  All
    blocks of a grid with gz > 1 vote for one in-plane rotation and one dz.  ``params`` float64 [N,5]; ``inlier`` uint8 [N,gz,gy,gx].
    ``prior`` float64 [N,5]: the motion already applied to the volumes that were measured; the result is the total motion of the
    original.  Everything stays on the device."""
    what = "fit_rigid_motion"
    _grid_arg(grid, what)
    min_peak, reject = _rigid_fit_args(min_peak, reject, what)
    center = _rigid_center(center, grid.shape, what)
    if not torch.is_tensor(shifts) or shifts.dim() < 3 or tuple(shifts.shape[1:]) not in ((*grid.grid, 3), (grid.B, 3)) or shifts.dtype != torch.float32:
        raise ValueError(f"{what}: shifts is a float32 {['N', *grid.grid, 3]} tensor")
    N = int(shifts.shape[0])
    if not torch.is_tensor(peak) or peak.numel() != N * grid.B or peak.dtype != torch.float32:
        raise ValueError(f"{what}: peak is a float32 {['N', *grid.grid]} tensor")
    if prior is not None:
        _rigid_params_arg(prior, N, what, "prior")
    if not shifts.is_cuda:
        raise RuntimeError(f"{what}: cwfa_amd runs on MI355X only -- shifts must be a device tensor (no CPU fallback exists)")
    params, inlier = ops.reg_fit_rigid(shifts.reshape(N, grid.B, 3), peak.reshape(N, grid.B), _rigid_arms(grid, center, shifts.device), min_peak, reject,
                                       prior)
    return RigidFit(params, inlier.view(N, *grid.grid))


@amp_region
def rigid_move_volumes(volumes, params, center=None, mode="bilinear", fill=0.0, out=None):
    """out[n,z,y,x] = volumes[n, z + dz, c0 + R ((y, x) - c0) + (dy, dx)] with (dz, dy, dx, c, s) = params[n] (float64 [N,5] on the
    device, as ``fit_rigid_motion`` returns them), R = [[c, -s], [s, c]] and c0 = ``center`` (None: the centre of the plane): the
    sign convention of ``shift_volumes``, which it equals bit for bit at (c, s) = (1, 0).  Trilinear or ``mode="nearest"``; voxels
    from outside the volume are ``fill``.  ``out`` must not share memory with ``volumes``.
    ``valid_box(rigid_corner_shifts(params, shape, center), shape)`` bounds the box that holds data in every volume."""
    what = "rigid_move_volumes"
    _shift_volume_args(volumes, None, mode, out, what)
    _rigid_params_arg(params, int(volumes.shape[0]), what)
    return ops.reg_rigid3d(volumes, params, _rigid_center(center, tuple(volumes.shape[1:]), what), mode=mode, fill=fill, out=out)


def _rigid_estimate(volumes, template, grid, n_refine, center, max_shift, taper, smooth, eps, subpixel, min_peak, reject, chunk, what):
    """(params, peak, inlier, shifts) of ``estimate_rigid_motion``."""
    m, taper, chunk = _block_reg_args(volumes, template, grid, max_shift, taper, smooth, eps, chunk, subpixel, what)
    min_peak, reject = _rigid_fit_args(min_peak, reject, what)
    if int(n_refine) < 0:
        raise ValueError(f"{what}: n_refine is not negative, got {n_refine}")
    center = _rigid_center(center, grid.shape, what)
    if template is None:
        raise ValueError(f"{what}: a template is needed")
    ops._dev(volumes, "volumes")
    N, g = int(volumes.shape[0]), grid.grid
    arms = _rigid_arms(grid, center, volumes.device)

    def table(chunk_of=None):
        shifts, peak = _block_table(volumes, template, grid, m, taper, smooth, eps, subpixel, chunk, chunk_of)
        return shifts.view(N, grid.B, 3), peak.view(N, grid.B)

    shifts, peak = table()
    params, inlier = ops.reg_fit_rigid(shifts, peak, arms, min_peak, reject)
    if N and int(n_refine):
        scratch = torch.empty((min(chunk, N), *grid.shape), dtype=torch.float32, device=volumes.device)
        for _ in range(int(n_refine)):
            moved = lambda s, e, cur=params: ops.reg_rigid3d(volumes[s:e], cur[s:e], center, out=scratch[:e - s])
            shifts, peak = table(moved)
            params, inlier = ops.reg_fit_rigid(shifts, peak, arms, min_peak, reject, prior=params)
    return params, peak.view(N, *g), inlier.view(N, *g), shifts.view(N, *g, 3)


@amp_region
def estimate_rigid_motion(volumes, template, grid, n_refine=2, center=None, max_shift=(2, 8, 8), taper=None, smooth=0.0, eps=1e-5, subpixel=True,
                          min_peak=0.0, reject=1.0, chunk=1):
    """(params float64 [N,5], peak float32 [N,gz,gy,gx], inlier uint8 [N,gz,gy,gx], shifts float32 [N,gz,gy,gx,3]) on the device: the
    rigid motion (dz, dy, dx, c, s) of every volume of a contiguous [N,D,H,W] float32 device stack against the float32 ``template``
    [D,H,W] -- a rotation about the optical axis around ``center`` plus a 3-D shift.  Pass 0 measures the table
    of block shifts of the ``BlockGrid`` ``grid`` as ``estimate_block_shifts`` measures it (its arguments; no clean-up and no
    whole-volume estimate) and fits it (``fit_rigid_motion``: ``min_peak``, ``reject``).  A block that is still rotated against its
    template reports a biased shift, so each of the ``n_refine`` further passes moves the ORIGINAL chunk under the current motion
    into a scratch chunk, measures that, and fits with the current motion as ``prior``: the result stays the total motion of the
    original and a volume is never interpolated twice.  ``peak``, ``inlier`` and ``shifts`` are those of the last pass.  The angles
    must be small enough for a block to correlate with its template (a few degrees).  Nothing is read back."""
    return _rigid_estimate(volumes, template, grid, n_refine, center, max_shift, taper, smooth, eps, subpixel, min_peak, reject, chunk,
                           "estimate_rigid_motion")


@amp_region
def register_volumes_rigid(volumes, template=None, grid=None, block=(32, 128, 128), n_iter=1, n_refine=2, center=None, max_shift=(2, 8, 8),
                           subpixel=True, mode="bilinear", taper=None, smooth=0.0, eps=1e-5, min_peak=0.0, reject=1.0, chunk=1, fill=0.0, out=None):
    """Rigid registration with a rotation about the optical axis of a contiguous [N,D,H,W] float32 device stack:
    ``RigidRegistration(volumes, params, peak, inlier, shifts, template)`` with volumes[n] = the input's volume n moved back under
    params[n] = (dz, dy, dx, c, s).  ``grid``: a ``BlockGrid``, or (gz, gy, gx) / None for ``block_grid(shape, block, grid)``.
    ``template`` None: the per-voxel lower temporal median; ``n_iter`` > 1: the template becomes the median of the registered stack
    and the motion is estimated again FROM THE ORIGINAL VOLUMES.  The other arguments are those of ``estimate_rigid_motion`` and
    ``rigid_move_volumes``; ``valid_box(rigid_corner_shifts(params, shape, center), shape)`` is the box that holds data in every
    volume.  Nothing is read back."""
    what = "register_volumes_rigid"
    _vol_reg_args(volumes, template, 0, 0, smooth, eps, chunk, subpixel, what)
    if not isinstance(grid, BlockGrid):
        grid = block_grid(tuple(int(n) for n in volumes.shape[1:]), block, grid)
    _block_reg_args(volumes, template, grid, max_shift, taper, smooth, eps, chunk, subpixel, what)
    _rigid_fit_args(min_peak, reject, what)
    _rigid_center(center, grid.shape, what)
    if int(n_refine) < 0:
        raise ValueError(f"{what}: n_refine is not negative, got {n_refine}")
    _register_args(volumes, n_iter, mode, out, what, "volume")
    estimate = lambda tmpl: _rigid_estimate(volumes, tmpl, grid, n_refine, center, max_shift, taper, smooth, eps, subpixel, min_peak, reject, chunk, what)
    out, (params, peak, inlier, shifts), tmpl = _register(volumes, template, n_iter, _volume_median, estimate,
                                                          lambda est, out: rigid_move_volumes(volumes, est[0], center, mode=mode, fill=fill, out=out), out)
    return RigidRegistration(out, params, peak, inlier, shifts, tmpl)


class RigidVolumeRegistrar(_StreamingRegistrar):
    """The streaming twin of ``PiecewiseVolumeRegistrar`` for rigid motion with rotation: ``reg(chunk)`` returns the registered
    [T',D,H,W] chunk (or volume, for one [D,H,W] volume) against the fixed float32 ``template`` [D,H,W] on the ``BlockGrid`` ``grid``
    and appends the chunk's parameters, peaks and inlier map to the device lists ``reg.params``, ``reg.peak`` and ``reg.inlier``;
    nothing is read back inside the call.  ``all_params()`` concatenates the parameters (float64 [N,5]); ``estimate_args``: those of
    ``estimate_rigid_motion``; ``mode`` and ``fill``: those of ``rigid_move_volumes``::

        reg = RigidVolumeRegistrar(template, block_grid(template.shape, (32, 128, 128)), max_shift=(2, 8, 8))
        for cond in batches:
            am.update(reg(inverse_pass(conv_inn, cond_nets, cond, mean_vols_cache)[:, 0]))
        box = valid_box(rigid_corner_shifts(reg.all_params(), template.shape), template.shape)      # the one read-back, after the loop
    """

    _lists = ("params", "peak", "inlier")

    def __init__(self, template, grid, mode="bilinear", fill=0.0, **estimate_args):
        self.grid = grid
        super().__init__(template, mode, fill, estimate_args)

    def _check(self, probe, common, a, what):
        _block_reg_args(probe, self.template, self.grid, *common, what)
        _rigid_fit_args(a("min_peak", 0.0), a("reject", 1.0), what)
        self.center = _rigid_center(a("center"), self.grid.shape, what)
        if int(a("n_refine", 2)) < 0:
            raise ValueError(f"{what}: n_refine is not negative, got {a('n_refine')}")

    def _estimate(self, volumes):
        return estimate_rigid_motion(volumes, self.template, self.grid, **self.estimate_args)

    def _move(self, volumes, params, out):
        return rigid_move_volumes(volumes, params, self.center, mode=self.mode, fill=self.fill, out=out)

    def all_params(self):
        """float64 [N,5] on the device: the motion of every volume seen so far."""
        return self._all("params", (5,), torch.float64)

    def all_peaks(self):
        """float32 [N,gz,gy,gx] on the device: the correlation peak of every block seen so far (last pass)."""
        return self._all("peak", self.grid.grid)


def rigid_angles(params):
    """float64 [N]: the rotation angles of ``params`` (float64 [N,5]) in degrees, atan2(s, c), on the tensor's device."""
    if not torch.is_tensor(params) or params.dim() != 2 or params.shape[1] != 5:
        raise ValueError("rigid_angles: params is a [N, 5] tensor of (dz, dy, dx, c, s)")
    p = params.to(torch.float64)
    return torch.atan2(p[:, 4], p[:, 3]) * (180.0 / math.pi)


def rigid_corner_shifts(params, shape, center=None):
    """float32 [4 N, 3] on the host: the displacement (dz, vy, vx) that ``rigid_move_volumes`` applies at the four corners of the plane
    of a volume of ``shape`` (D, H, W), for every row of ``params`` (float64 [N,5]), in the resampling's own fp32 arithmetic.  The
    displacement is affine in the position and every rounded operation is monotone, so its extremes over the plane are at the
    corners: ``valid_box(rigid_corner_shifts(params, shape, center), shape)`` bounds the box in which every registered volume holds
    data and no ``fill`` -- the box to hand to ``find_neurons(margin=)``.  A host helper: it reads the parameters back."""
    what = "rigid_corner_shifts"
    dims = tuple(int(v) for v in shape)
    if len(dims) != 3:
        raise ValueError(f"{what}: shape is (D, H, W), got {shape!r}")
    if not torch.is_tensor(params) or params.dim() != 2 or params.shape[1] != 5:
        raise ValueError(f"{what}: params is a [N, 5] tensor of (dz, dy, dx, c, s)")
    cy, cx = _rigid_center(center, dims, what)
    p = params.detach().to("cpu", torch.float64)
    f32 = lambda t: t.to(torch.float32)
    dz, dy, dx, s = f32(p[:, 0]), f32(p[:, 1]), f32(p[:, 2]), f32(p[:, 4])
    cm1 = f32(-(p[:, 4] * p[:, 4]) / (1.0 + p[:, 3]))
    cm1 = torch.where(torch.isfinite(p[:, 3]), cm1, torch.full_like(cm1, float("nan")))
    rows = []
    for y in (0, dims[1] - 1):
        for x in (0, dims[2] - 1):
            py = torch.tensor(float(y), dtype=torch.float32) - torch.tensor(cy, dtype=torch.float32)
            px = torch.tensor(float(x), dtype=torch.float32) - torch.tensor(cx, dtype=torch.float32)
            # (dz + 0 cm1: a rotation that is not finite fills the volume, so it makes the row non-finite in every component)
            rows.append(torch.stack((dz + 0.0 * cm1, dy + (cm1 * py - s * px), dx + (s * py + cm1 * px)), dim=1))
    return torch.stack(rows, dim=1).reshape(-1, 3)


# ---------------------------------------------------------------------------------------------------- neuron footprints
# Behind ``find_neurons``: which voxels of a neuron's ROI box belong to it, and the traces weighted by that.
def footprint_cores(coords, boxes, shape, core=(1, 1, 1), start_plane_offset=-25 // 2):
    """int32 [N,6]: the seed region [c - core, c + core + 1) of every neuron clipped by its box (``roi_boxes``' row), c the centre
    ``coords`` names in volumes of ``shape`` (D, H, W).  A core that the box clips away is written as the empty range at the box's
    lower corner."""
    import numpy as np
    D = shape[0]
    out = np.zeros((len(coords), 6), dtype=np.int32)
    for ix, (x_coord, y_coord, z_coord) in enumerate(coords):
        centre = (int(z_coord) + D // 2 + start_plane_offset, int(y_coord), int(x_coord))
        rows = [(max(int(boxes[ix][2 * k]), c - core[k]), min(int(boxes[ix][2 * k + 1]), c + core[k] + 1)) for k, c in enumerate(centre)]
        empty = any(hi <= lo for lo, hi in rows)
        for k, (lo, hi) in enumerate(rows):
            out[ix, 2 * k], out[ix, 2 * k + 1] = (boxes[ix][2 * k], boxes[ix][2 * k]) if empty else (lo, hi)
    return out


class Footprints:
    """What ``NeuronFootprints.finish`` returns.  ``boxes`` int32 [N,6] and ``offsets`` int64 [N+1] on the host: box n's voxels lie at
    ``offsets[n]`` of the ragged device arrays ``weights`` and ``corr`` (float32 [V]) in the box's own (z, y, x) order; ``wsum``
    float64 [N]: the sum of a neuron's weights; ``sizes`` int32 [N]: the voxels of its footprint (0: the trace is NaN)."""

    def __init__(self, boxes, offsets, weights, wsum, sizes, corr):
        self.boxes, self.offsets, self.weights, self.wsum, self.sizes, self.corr = boxes, offsets, weights, wsum, sizes, corr

    def dense(self, n):
        """The weights of neuron ``n`` as a [bz,by,bx] view of ``weights``."""
        b = self.boxes[n]
        return self.weights[int(self.offsets[n]):int(self.offsets[n + 1])].view(int(b[1] - b[0]), int(b[3] - b[2]), int(b[5] - b[4]))


class NeuronFootprints:
    """The footprint of every neuron of ``coords`` (what ``find_neurons`` returns) in a series of [D,H,W] volumes of ``shape``,
    accumulated while the volumes stream by.  Per voxel of a neuron's ROI box (``roi_boxes`` with ``r12``, ``r3``,
    ``start_plane_offset``) the state holds the float64 sums of its correlation with the seed trace -- the sum over the box
    ``centre +- core`` -- and with the neuropil trace, the sum over the shell between ``gap`` and ``gap + annulus`` around the box that
    no neuron's box touches: 36 bytes per box voxel, 22 KB per neuron at the default 600 voxels.  ``finish(thr)`` thresholds the partial
    correlation of voxel and seed given the neuropil trace (the plain correlation for ``neuropil=False``) and keeps what is connected
    through faces to the core.  The state after any chunking is bit for bit that of the whole series."""

    def __init__(self, coords, shape, device, r12=5, r3=3, start_plane_offset=-25 // 2, core=(1, 1, 1), gap=(1, 2, 2), annulus=(2, 4, 4),
                 neuropil=True):
        self.shape = tuple(int(s) for s in shape)
        if len(self.shape) != 3 or min(self.shape) < 0:
            raise ValueError(f"NeuronFootprints: shape is (D, H, W), got {shape!r}")
        core = ops._nonneg_triple(core, "core", "NeuronFootprints")
        if int(r12) < 1 or int(r3) < 1:
            raise ValueError("NeuronFootprints: r12 and r3 are positive ROI half-widths")
        coords = [list(c) for c in coords]
        if any(len(c) != 3 for c in coords):
            raise ValueError("NeuronFootprints: coords are [x, y, z] rows (find_neurons)")
        boxes = roi_boxes(coords, (0, *self.shape), int(r12), int(r3), start_plane_offset)
        cores = footprint_cores(coords, boxes, self.shape, core, start_plane_offset)
        self.geometry = ops.footprint_geometry(boxes, cores, self.shape, gap, annulus, device)
        self.neuropil = bool(neuropil)
        self.state = ops.footprint_state(self.geometry, device)
        self.count = 0

    def update(self, volumes):
        """Add ``volumes``: [T',D,H,W] or one [D,H,W] volume, float32 on the device."""
        ops._dev(volumes, "volumes")
        if volumes.dim() == 3:
            volumes = volumes.unsqueeze(0)
        if volumes.dim() != 4 or tuple(volumes.shape[1:]) != self.shape:
            raise ValueError(f"NeuronFootprints.update: volumes of shape {self.shape} are expected, got {tuple(volumes.shape)}")
        if volumes.shape[0]:
            c = ops.roi_weighted_sums(volumes, self.geometry.cores)
            u = ops.roi_shell_sums(volumes, self.geometry)[0] if self.neuropil else None
            ops.footprint_update(volumes, self.geometry, c, u, self.state, first=self.count == 0)
            self.count += volumes.shape[0]
        return self

    def finish(self, thr=0.5):
        """The ``Footprints`` at threshold ``thr`` in (0, 1].  The state is kept: more volumes may follow."""
        thr = ops.footprint_threshold(thr, "NeuronFootprints.finish")
        if self.count < 1:
            raise ValueError("NeuronFootprints.finish: no volume has been added")
        corr = ops.footprint_corr(self.state, self.geometry, self.count, self.neuropil)
        weights, wsum, sizes = ops.footprint_select(corr, self.geometry, thr)
        return Footprints(self.geometry.boxes, self.geometry.offsets, weights, wsum, sizes, corr)


def extract_traces(volumes, footprints, geometry=None, alpha=0.7):
    """``(F, Fnp, Fc)``, float64 [N,T'] on the device, of ``volumes`` [T',D,H,W] (or one [D,H,W] volume): F = sum of w x / sum of w over
    a neuron's footprint (NaN for an empty one), Fnp the mean over its neuropil shell (NaN for an empty shell), Fc = F - alpha Fnp (F
    where the shell is empty).  ``geometry``: the ``FootprintGeometry`` whose shells to use (``NeuronFootprints.geometry``); None skips
    the neuropil: Fnp is NaN and Fc equals F.  alpha = 0.7 is the usual convention, not a measurement.  Nothing is read back."""
    if not isinstance(footprints, Footprints):
        raise ValueError("extract_traces: footprints is what NeuronFootprints.finish returns")
    if geometry is not None and not isinstance(geometry, ops.FootprintGeometry):
        raise ValueError("extract_traces: geometry is a FootprintGeometry or None")
    ops._dev(volumes, "volumes")
    if volumes.dim() == 3:
        volumes = volumes.unsqueeze(0)
    F = ops.roi_weighted_sums(volumes, footprints.boxes, footprints.weights, footprints.offsets) / footprints.wsum[:, None]
    if geometry is None:
        return F, torch.full_like(F, float("nan")), F.clone()
    sums, counts = ops.roi_shell_sums(volumes, geometry)
    Fnp = sums / counts.to(torch.float64)[:, None]
    return F, Fnp, torch.where(torch.isnan(Fnp), F, F - float(alpha) * Fnp)


# ---- demixing of overlapping footprints: F_n carries a share M_nm of every neighbour m whose light falls on
# voxels of footprint n; the shares follow from the footprints alone, and the traces are solved for per time step.
@amp_region
def demix_plan(footprints):
    """The ``ops.DemixPlan`` of ``footprints`` (what ``NeuronFootprints.finish`` returns): the pairs of boxes that intersect, the
    overlap sums G_nm = sum w_n w_m over the intersections and the mixing coefficients M_nm = (G_nm wsum_m) / (G_mm wsum_n).
    Computed once per recording; it allocates and waits for its tables to reach the device."""
    if not isinstance(footprints, Footprints):
        raise ValueError("demix_plan: footprints is what NeuronFootprints.finish returns")
    return ops.DemixPlan(footprints)


@amp_region
def demix_traces(F, footprints_or_plan, n_sweeps=64, tol=0.0, nonneg=True):
    """``(Fd, sweeps)``: the raw traces ``F`` of ``extract_traces`` (float64 [N,T'] on the device, any chunking of time, a row stride
    allowed) with the neighbours' shares taken out, and the sweeps every time step ran (int32 [T']).  The model is that the voxels of
    the footprints hold sum_m w_m(v) f_m(t), so F_n = f_n + sum_{m != n} M_nm f_m; it is solved per time step by projected
    Gauss-Seidel from f = F (``nonneg``: f >= 0), ending after the first sweep that changes nothing by more than ``tol`` or after
    ``n_sweeps``.  A neuron whose box meets no other footprint returns the bits of its F; an empty footprint's row is NaN and
    reaches nobody.  ``footprints_or_plan``: a ``DemixPlan`` (``demix_plan``, once per recording) or the ``Footprints``, for which
    the plan is made here, every call.

    Intended use: ``delta_f_over_f(Fd, Fnp)`` -- demix the raw trace, then correct for neuropil; the shells exclude every box, so
    ``Fnp`` needs no demixing.  Limits: light of a neighbour that falls on footprint n outside the neighbour's own thresholded
    footprint is not removed; under a strong common background (0.4 of a blob's amplitude in the tests' scene) the result is not
    reliably better and some neurons get worse; two identical footprints make the system singular."""
    what = "demix_traces"
    plan = footprints_or_plan
    if isinstance(plan, Footprints):
        plan = ops.DemixPlan(plan)
    if not isinstance(plan, ops.DemixPlan):
        raise ValueError(f"{what}: footprints_or_plan is a DemixPlan (demix_plan) or what NeuronFootprints.finish returns")
    try:
        sweeps_ok = int(n_sweeps) >= 1 and int(n_sweeps) == n_sweeps
    except (TypeError, ValueError):
        sweeps_ok = False
    try:
        tol_ok = float(tol) >= 0.0
    except (TypeError, ValueError):
        tol_ok = False
    if not sweeps_ok:
        raise ValueError(f"{what}: n_sweeps is a positive integer, got {n_sweeps!r}")
    if not tol_ok:
        raise ValueError(f"{what}: tol is a non-negative number, got {tol!r}")
    if not torch.is_tensor(F) or F.dtype != torch.float64 or F.dim() != 2 or F.shape[1] < 1:
        raise ValueError(f"{what}: F is a float64 [N, T] tensor on the HIP device with T >= 1 (extract_traces)")
    if F.shape[0] != plan.N:
        raise ValueError(f"{what}: F has {F.shape[0]} rows, the footprints {plan.N} neurons")
    if not F.is_cuda:
        raise ValueError(f"{what}: F is a float64 [N, T] tensor on the HIP device, got one on {F.device}")
    return ops.demix_solve(F, plan, int(n_sweeps), float(tol), bool(nonneg))


# ---- what a user reads from the traces: dF/F against a running-percentile baseline, a robust noise level
# and spikes by exact AR(1) deconvolution.  float64 [N,T] on the device throughout; nothing is read back.
def _window(half_window, percentile, what):
    import operator
    try:                                                                          # any integer type (numpy's too), no float, no bool
        h = None if isinstance(half_window, bool) else operator.index(half_window)
    except TypeError:
        h = None
    if h is None or h < 0:
        raise ValueError(f"{what}: half_window is a non-negative integer number of samples, got {half_window!r}")
    try:
        p = None if isinstance(percentile, bool) else operator.index(percentile)
    except TypeError:
        p = None
    if p is None or not 0 <= p <= 100:
        raise ValueError(f"{what}: percentile is an integer in 0 .. 100, got {percentile!r}")
    return h, p


def trace_baseline(traces, half_window, percentile=8):
    """The running-percentile baseline of ``traces`` (float64 device [N,T], or a view with a row stride): per sample the
    ``(percentile * (m - 1)) // 100``-th smallest of the m samples within ``half_window`` of it, an element of the trace bit for bit
    (no interpolation; NaN sorts last).  ``half_window >= T - 1`` gives the row's global quantile everywhere."""
    h, p = _window(half_window, percentile, "trace_baseline")
    return ops.sliding_quantile(ops._rows(traces, "trace_baseline")[0], h, p)


def delta_f_over_f(F, Fnp=None, alpha=0.7, half_window=300, percentile=8, floor=0.0):
    """``(dff, B, D)`` of the raw traces ``F`` and neuropil traces ``Fnp`` of ``extract_traces``: Fc = F - alpha Fnp (F where Fnp is
    NaN or None), B and D the ``trace_baseline`` of Fc and of F, dff = (Fc - B) / max(D, floor) where that denominator is positive,
    NaN elsewhere.  The denominator is the raw trace's baseline: the corrected one's can be zero or negative.  ``half_window`` is in
    samples; the default suits 10 Hz recordings (a minute), set it from the frame rate."""
    what = "delta_f_over_f"
    h, p = _window(half_window, percentile, what)
    floor = float(floor)
    if not floor >= 0.0:
        raise ValueError(f"{what}: floor = {floor} is negative")
    F = ops._rows(F, what, "F")[0]
    if Fnp is None:
        Fc = F
    else:
        Fnp = ops._rows(Fnp, what, "Fnp")[0]
        if Fnp.shape != F.shape:
            raise ValueError(f"{what}: Fnp {tuple(Fnp.shape)} does not match F {tuple(F.shape)}")
        Fc = torch.where(torch.isnan(Fnp), F, F - float(alpha) * Fnp)
    B = ops.sliding_quantile(Fc, h, p)
    D = B if Fnp is None else ops.sliding_quantile(F, h, p)
    den = torch.clamp_min(D, floor)
    return torch.where(den > 0, (Fc - B) / den, torch.full_like(den, float("nan"))), B, D


def trace_noise(traces):
    """float64 [N]: the noise level of every trace from its first differences d, sigma = 1.0483580825075305 * mad with
    mad = lmed(|d - lmed(d)|) and lmed the element of rank (len - 1) // 2 -- 1 / (0.6744897501960817 sqrt 2) turns the median
    absolute deviation of the difference of two samples into the standard deviation of one.  T < 2 gives NaN."""
    x, N, T, _ = ops._rows(traces, "trace_noise")
    if T < 2:
        return torch.full((N,), float("nan"), dtype=torch.float64, device=x.device)
    d = x[:, 1:] - x[:, :-1]
    r = [(T - 2) // 2]
    med = ops.trace_select(d, r)[0]
    mad = ops.trace_select((d - med[:, None]).abs(), r)[0]
    return mad * 1.0483580825075305


def infer_spikes(traces, gamma, lam=None, lam_sigma=None):
    """``(c, s, pools)``: the denoised calcium c and the spikes s >= 0 (float64 [N,T]) of every trace by exact non-negative AR(1)
    deconvolution -- the minimiser of 1/2 sum (y - c)^2 + lam sum s with s_0 = c_0, s_t = c_t - gamma c_{t-1} (OASIS) -- and the
    number of pools (int32 [N]).  ``gamma`` in [0, 1): the decay per sample, one for all rows.  Exactly one of ``lam`` (a float or a
    float64 device [N] tensor) and ``lam_sigma`` (lam = lam_sigma * ``trace_noise(traces)``, which stays on the device) is given."""
    what = "infer_spikes"
    if (lam is None) == (lam_sigma is None):
        raise ValueError(f"{what}: exactly one of lam and lam_sigma is given")
    gamma = float(gamma)
    if not 0.0 <= gamma < 1.0:
        raise ValueError(f"{what}: gamma = {gamma} is not in [0, 1)")
    x, N, T, _ = ops._rows(traces, what)
    if lam_sigma is not None:
        lam = float(lam_sigma) * trace_noise(x)
    elif torch.is_tensor(lam):
        if not lam.is_cuda or lam.dtype != torch.float64 or tuple(lam.shape) != (N,):
            raise ValueError(f"{what}: lam is a float or a float64 [{N}] tensor on the HIP device, got {tuple(lam.shape)} {lam.dtype} on {lam.device}")
    else:
        lam = torch.full((N,), float(lam), dtype=torch.float64, device=x.device)
    return ops.ar1_deconv(x, gamma, lam)


def read_neural_coordinates_from_file(filename):
    """CWFA.py:223-238, same signature: the ``[x, y, z]`` rows with ``is_gt == 1`` of a coordinates CSV, or of a list of them.
    One departure: for a list the reference drops the result of ``dataframe.append`` (and pandas 2 has no such method), so it returns
    the first file's rows only; here the rows of all files are returned, in order."""
    import pandas as pd
    if isinstance(filename, str):
        dataframe = pd.read_csv(filename)
    else:
        dataframe = pd.concat([pd.read_csv(F) for F in filename], ignore_index=True)
    rows = dataframe[dataframe['is_gt'] == 1]
    cols = [rows[axis].tolist() for axis in ('coord_x', 'coord_y', 'coord_z')]
    return [[cols[0][ix], cols[1][ix], cols[2][ix]] for ix in range(len(cols[0]))]


def write_neural_coordinates_to_file(coords, filename, scores=None):
    """Write ``coords`` (``[x, y, z]`` integer rows, as ``find_neurons`` returns them) as the CSV the reference's
    ``read_neural_coordinates_from_file`` reads back exactly: columns patch_n, coord_x, coord_y, coord_z, corr_coeff (0), is_gt (1),
    and ``score`` when ``scores`` are given."""
    import pandas as pd
    rows = [[int(v) for v in c] for c in coords]
    if any(len(r) != 3 for r in rows) or any(a != b for r, c in zip(rows, coords) for a, b in zip(r, c)):
        raise ValueError("write_neural_coordinates_to_file: coords are [x, y, z] integer rows")
    data = {'patch_n': list(range(len(rows))), 'coord_x': [r[0] for r in rows], 'coord_y': [r[1] for r in rows],
            'coord_z': [r[2] for r in rows], 'corr_coeff': [0] * len(rows), 'is_gt': [1] * len(rows)}
    if scores is not None:
        scores = [float(s) for s in scores]
        if len(scores) != len(rows):
            raise ValueError("write_neural_coordinates_to_file: one score per coordinate")
        data['score'] = scores
    pd.DataFrame(data).to_csv(filename, index=False)
    return filename
