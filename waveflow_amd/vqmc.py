"""waveflow.vqmc call surface on the HIP path (reference: vqmc.py:19-221): the VQMC trainer.

One step = sample a batch -> local energies -> gradient of loss_fn_efficient under its custom tangent rule -> Adam.
The device work (sampler, H psi, the vector-Jacobian product, the fp64 batch sums) is libwaveflow_hip; the optimiser
state lives on the host like the parameters do (wf_model_set_params takes the host vector), and with several ranks
the step's only collective is one SUM all-reduce of [gradient, sum E_L, sum E_L^2, n].

`adam` follows jax.example_libraries.optimizers.adam, which is what vqmc.py:136 builds:
    m <- (1 - b1) g + b1 m;  v <- (1 - b2) g^2 + b2 v;  x <- x - step_size * m_hat / (sqrt(v_hat) + eps)
with m_hat = m / (1 - b1^(i+1)), v_hat = v / (1 - b2^(i+1)) for the step index i passed to opt_update.
"""
import json
import os
from pathlib import Path
from types import SimpleNamespace

import numpy as np

from . import checkpoint
from .core import DeviceParams, flatten_params, unflatten_batched
from .model_factory import get_waveflow_model
from .utils import helpers, physics


class OptState:
    """Adam state over the flat parameter vector (reference leaf order); `template` restores the pytree.  x, m, v are numpy
    vectors (host state) or float32 cuda tensors (device state: parameters and optimiser never leave the GPU)."""

    def __init__(self, template, x, m, v, model=None):
        self.template, self.x, self.m, self.v, self.model = template, x, m, v, model
        self.version = 0

    @property
    def on_device(self):
        return self.model is not None


def _lr_at(step_size, i):
    """The step size of step i: a number, or a schedule called with i."""
    return float(step_size(i) if callable(step_size) else step_size)


def adam(step_size, b1=0.9, b2=0.999, eps=1e-8, model=None):
    """-> (opt_init, opt_update, get_params), the triple protocol of jax.example_libraries.optimizers.
    With `model` (a DeviceModel) the state lives on that model's GPU, opt_update runs wf_adam_step in place and get_params
    returns core.DeviceParams; otherwise everything is numpy on the host."""
    def opt_init(params):
        x = flatten_params(params).astype(np.float32)
        if model is None:
            return OptState(params, x, np.zeros_like(x), np.zeros_like(x))
        import torch
        dev = f"cuda:{model.device}"
        template = params.template if isinstance(params, DeviceParams) else params
        xd = torch.as_tensor(x).to(dev)
        return OptState(template, xd, torch.zeros_like(xd), torch.zeros_like(xd), model=model)

    def opt_update(i, grads, state):
        if state.on_device:
            import torch
            g = grads if hasattr(grads, "is_cuda") else torch.as_tensor(flatten_params(grads) if not isinstance(grads, np.ndarray) else grads)
            g = g.to(state.x.device, dtype=torch.float32).contiguous()
            state.model.adam_step(state.x, g, state.m, state.v, i, _lr_at(step_size, i), b1, b2, eps)
            state.version += 1
            return state
        g = grads if isinstance(grads, np.ndarray) and grads.ndim == 1 else flatten_params(grads)
        g = np.asarray(g, dtype=np.float32)
        one = np.float32(1.0)
        m = (one - np.float32(b1)) * g + np.float32(b1) * state.m
        v = (one - np.float32(b2)) * np.square(g) + np.float32(b2) * state.v
        mhat = m / (one - np.float32(b1) ** np.float32(i + 1))
        vhat = v / (one - np.float32(b2) ** np.float32(i + 1))
        x = state.x - np.float32(_lr_at(step_size, i)) * mhat / (np.sqrt(vhat) + np.float32(eps))
        return OptState(state.template, x.astype(np.float32), m, v)

    def get_params(state):
        if state.on_device:
            return DeviceParams(state.template, state.x, state.version)
        return checkpoint.unflatten_like(state.template, state.x)

    return opt_init, opt_update, get_params


def _model_init_fun(box_length, n_particle, xu_coord_type, spline_degree, num_knots, n_flow_layers):
    """The model of create_train_state: init_fun(rng, n_particle) -> (params, psi, log_pdf, sample) on a DeviceModel of its own."""
    return get_waveflow_model(n_particle, base_spline_degree=spline_degree, i_spline_degree=spline_degree,
                              n_prior_internal_knots=num_knots, n_i_internal_knots=num_knots,
                              i_spline_reg=0.05, i_spline_reverse_fun_tol=0.000001,
                              n_flow_layers=n_flow_layers, box_size=box_length, xu_coord_type=xu_coord_type)


def create_train_state(box_length, learning_rate, n_particle, rng=0, xu_coord_type='mean', spline_degree=6, num_knots=23,
                       n_flow_layers=3):
    """vqmc.py:123-139"""
    init_fun = _model_init_fun(box_length, n_particle, xu_coord_type, spline_degree, num_knots, n_flow_layers)
    params, psi, log_pdf, sample = init_fun(rng, n_particle)
    opt_init, opt_update, get_params = adam(step_size=learning_rate, model=psi.model)   # state on the model's GPU
    return psi, log_pdf, sample, opt_init(params), opt_update, get_params


def _protons_of(h_fn):
    """The proton positions a Hamiltonian closure of physics.construct_hamiltonian_function carries."""
    pos = getattr(h_fn, "protons", None)
    if pos is None:
        raise TypeError("h_fn must come from waveflow_amd.utils.physics.construct_hamiltonian_function")
    return pos


def loss_fn_efficient(params, psi, h_fn, batch, running_average):
    """vqmc.py:193-200 (value only): mean of H psi / (psi + 1e-8) over the batch."""
    p = helpers._np(psi(params, batch)).reshape(-1, 1)
    e = helpers._np(h_fn(params, batch)).reshape(-1, 1)
    return float((e / (p + 1e-8)).mean())


def loss_and_grad_efficient(params, psi, h_fn, batch, running_average, group=None):
    """value_and_grad(loss_fn_efficient) with the custom tangent rule (vqmc.py:198-212, 215-221) over the walkers of ALL ranks
    of `group` (each rank passes its own shard).  -> (loss, flat gradient [n_params] float32 cuda tensor, (mean, variance,
    stderr) of E_L)."""
    from .distributed import all_reduce_gradient_and_moments, global_count, moments_to_stats
    model = psi.model
    model.ensure_params(params)
    pos = _protons_of(h_fn)
    # the tangent rule's 1 / batch factor is applied on the device, so the global count is needed up front
    # `group=None` means NOT distributed in every function of this module (as in ModelTrainer): no collective is entered, whatever
    # process group happens to be initialised -- a rank that passes None must not wait in an all-reduce its peers never reach.
    # Sharded walkers: pass the group explicitly (torch.distributed.group.WORLD for the default one).
    n_global = global_count(int(batch.shape[0]), f"cuda:{model.device}", group) if group is not None else int(batch.shape[0])
    sums, grad = model.vqmc_loss_grad(batch, pos, float(np.asarray(running_average).reshape(-1)[0]), global_count=n_global)
    if group is not None:
        grad, sums = all_reduce_gradient_and_moments(grad, sums, group)   # one collective per step
    s = sums.cpu().tolist()
    return s[0] / s[2], grad, moments_to_stats(s)


def train_step_efficient(epoch, psi, h_fn, opt_update, opt_state, params, batch, running_average, group=None):
    """vqmc.py:215-221 -> (new opt_state, loss)"""
    loss_val, gradients, _ = loss_and_grad_efficient(params, psi, h_fn, batch, running_average, group=group)
    return opt_update(epoch, gradients, opt_state), loss_val


def _energy_terms(params, psi, h_fn, batch):
    """One forward sweep: (model, x on the device, H psi, psi, laplacian) as float32 cuda vectors."""
    model = psi.model
    model.ensure_params(params)
    pos = _protons_of(h_fn)
    x, _ = model._to_dev(batch)
    hpsi, ps, lap = model.hamiltonian(x, pos, return_psi=True, return_laplacian=True)
    return model, x, hpsi, ps, lap


def _reduce_scalars(values, device, group):
    """SUM all-reduce of a few python floats (fp64 on the wire) -> list of floats; the identity for group=None (see loss_and_grad_efficient)."""
    if group is None:
        return [float(v) for v in values]
    import torch
    from .distributed import all_reduce_moments
    t = torch.tensor([float(v) for v in values], dtype=torch.float64, device=device)
    return all_reduce_moments(t, group).cpu().tolist()


def _reduce_gradient(grad, group):
    if group is None:
        return grad
    import torch
    from .distributed import all_reduce_gradient_and_moments
    g, _ = all_reduce_gradient_and_moments(grad, torch.zeros(3, dtype=torch.float64, device=grad.device), group)
    return g


def loss_fn_uniform(params, psi, h_fn, batch):
    """vqmc.py:143-148: mean(psi * H psi) / mean(psi^2) over a uniformly drawn batch (value only; the gradient treats the
    denominator as a constant, see train_step_uniform)."""
    p = helpers._np(psi(params, batch)).reshape(-1, 1).astype(np.float64)
    e = helpers._np(h_fn(params, batch)).reshape(-1, 1).astype(np.float64)
    return float((p * e).mean() / (p * p).mean())


def loss_and_grad_uniform(params, psi, h_fn, batch, group=None):
    """value_and_grad(loss_fn_uniform) (vqmc.py:150-154) on the HIP path.  With H psi = -1/2 lap + V psi and the denominator
    Z = mean(psi^2) under stop_gradient,
        d loss = 1 / (n Z) * sum_b [ (H psi_b + V_b psi_b) d psi_b  -  1/2 psi_b d lap_b ],     V_b psi_b = H psi_b + 1/2 lap_b
    (no division by psi), which is one wf_psi_vjp.  Several ranks: n and Z are global (one small all-reduce), then the gradient."""
    model, x, hpsi, ps, lap = _energy_terms(params, psi, h_fn, batch)
    d = ps.double()
    num, den, n = _reduce_scalars([float((d * hpsi.double()).sum()), float((d * d).sum()), float(x.shape[0])], x.device, group)
    z = den / n
    scale = 1.0 / (n * z)
    w_psi = (2.0 * hpsi + 0.5 * lap) * scale
    w_lap = ps * (-0.5 * scale)
    grad = _reduce_gradient(model.psi_vjp(x, w_psi, w_lap), group)
    return (num / n) / z, grad


def train_step_uniform(epoch, psi, h_fn, opt_update, opt_state, get_params, batch, group=None):
    """vqmc.py:150-154 -> (new opt_state, loss)"""
    loss_val, gradients = loss_and_grad_uniform(get_params(opt_state), psi, h_fn, batch, group=group)
    return opt_update(epoch, gradients, opt_state), loss_val


def loss_fn(params, psi, h_fn, batch):
    """vqmc.py:157-161 -> (mean of H psi / psi, (H psi [B, 1], psi [B, 1]))"""
    p = helpers._np(psi(params, batch)).reshape(-1, 1)
    e = helpers._np(h_fn(params, batch)).reshape(-1, 1)
    return float((e / p).mean()), (e, p)


def train_step_gradients(params, psi, h_fn, log_pdf, batch, running_average, group=None, clip=10.0):
    """The gradient and loss of vqmc.train_step (vqmc.py:172-187) before the optimiser:
        energy part   grad of mean(H psi / psi) -- true derivative through psi and through the Laplacian:
                      d (E / psi) = -1/2 d lap / psi + (V / psi - E / psi^2) d psi = -1/(2 psi) d lap + lap / (2 psi^2) d psi
        density part  mean_b [ d log_pdf_b * (E_b / psi_b - running_average) ]   (the jacrev of the reference, contracted)
    summed, then clipped elementwise to [-clip, clip] (the reference's 10; None: unclipped, for tests); loss = mean of E / psi clipped to [-100, 100].
    -> (flat gradient float32 cuda [n_params], loss)"""
    import torch
    if getattr(log_pdf, "model", None) is not psi.model:
        raise ValueError("psi and log_pdf must be the two closures of one model (model_factory init_fun)")
    model, x, hpsi, ps, lap = _energy_terms(params, psi, h_fn, batch)
    ne = hpsi / ps
    loss_sum, n = _reduce_scalars([float(torch.clamp(ne, -100.0, 100.0).double().sum()), float(x.shape[0])], x.device, group)
    inv = 1.0 / n
    w_psi = 0.5 * lap / (ps * ps) * inv
    w_lap = -0.5 / ps * inv
    grad = model.psi_vjp(x, w_psi, w_lap)
    grad = grad + model.logpdf_vjp(x, (ne - float(np.asarray(running_average).reshape(-1)[0])) * inv)
    grad = _reduce_gradient(grad, group)
    return (torch.clamp(grad, -clip, clip) if clip is not None else grad), loss_sum / n


def train_step(epoch, psi, h_fn, log_pdf, opt_update, opt_state, get_params, batch, running_average, group=None):
    """vqmc.py:169-187 -> (new opt_state, loss)"""
    gradients, loss_val = train_step_gradients(get_params(opt_state), psi, h_fn, log_pdf, batch, running_average, group=group)
    return opt_update(epoch, gradients, opt_state), loss_val


def log_pdf_jacobian(log_pdf):
    """-> jac(params, batch): jax.jacrev(log_pdf, argnums=0)(params, batch) (vqmc.py:179), the pytree of `params` with a leading batch axis on
    every leaf (float32 cuda views of one [B, n_params] tensor).  train_step keeps its contracted path (logpdf_vjp)."""
    model = log_pdf.model

    def jac(params, batch):
        model.ensure_params(params)
        return unflatten_batched(params, model.logpdf_jacobian(batch))
    jac.model = model
    return jac


def log_psi_jacobian(psi):
    """-> jac(params, batch): O_k(x_b) = d ln psi_b / d theta_k as jacrev(psi) / (psi + 1e-8) -- the reference's regulariser (vqmc.py:196) --,
    the pytree of `params` with a leading batch axis: the rows stochastic reconfiguration and per-sample gradient statistics start from."""
    model = psi.model

    def jac(params, batch):
        model.ensure_params(params)
        x, _ = model._to_dev(batch)
        rows = model.psi_jacobian(x)
        rows /= (model.psi(x) + 1e-8)[:, None]
        return unflatten_batched(params, rows)
    jac.model = model
    return jac


def _check_lower_states(lower_states, overlap_penalty):
    """lower_states: a list of (psi closure, params), at most overlap.MAX_REFS; overlap_penalty: one number or one per state, >= 0
    -> (the list, float32 [K]); ([], None) for None or an empty list.  Before anything is launched (ValueError)."""
    if not lower_states:
        return [], None
    from . import overlap
    lower_states = list(lower_states)
    overlap._check_K(len(lower_states))
    for entry in lower_states:
        if not isinstance(entry, (tuple, list)) or len(entry) != 2 or getattr(entry[0], "model", None) is None:
            raise ValueError("lower_states must be a list of (psi closure of model_factory's init_fun, params)")
    return lower_states, overlap._check_penalty(overlap_penalty, len(lower_states))


def _penalised_energies(model, x, ps, e_loc, lower_states, penalty, overlap_record):
    """The local energies of the penalty method L = E + sum_k lambda_k S_k^2 on the walkers x of `model` (psi `ps` and local energies
    `e_loc` on them): every lower psi at x through its own model's psi (its parameters are uploaded when they are not the ones it holds:
    once), overlap.accumulate into a fresh accumulator, overlap.penalise -> e~ float32 cuda [B].  overlap_record, a list, receives S_k of
    the step (float64 numpy [K]; this waits for the device)."""
    import torch
    from . import overlap
    rows = []
    for lpsi, lparams in lower_states:
        lm = lpsi.model
        if lm is model:
            raise ValueError("a lower state must have a DeviceModel of its own: it shares the model being trained")
        if lm.D != model.D or lm.device != model.device:
            raise ValueError(f"a lower state has {lm.D} coordinates on device {lm.device}, the model {model.D} on device {model.device}")
        lm.ensure_params(lparams)
        rows.append(lm.psi(x))
    refs = torch.stack(rows)
    acc = overlap.Accumulator(len(rows), x.device)
    ratios = overlap.accumulate(ps, refs, acc=acc, ratios=torch.empty_like(refs))
    e_pen = overlap.penalise(e_loc, ratios, acc, penalty)
    if overlap_record is not None:
        overlap_record.append(acc.totals().result()["overlap"])
    return e_pen


def _sr_rows_and_energies(what, params, psi, h_fn, batch, damping, relative_damping, group, solver, tol, max_iter, lower_states, overlap_penalty,
                          overlap_record, spring=None):
    """What sr_natural_gradient and spring_direction share ahead of the solve: the checks (spring: (momentum, clip) for SPRING), then on the
    walkers of `batch` the rows O = d psi / d theta / (psi + 1e-8), the local energies e_loc = H psi / (psi + 1e-8) and the energies the solver
    receives (penalised when there are lower states, else e_loc itself) -> (rows, e_used, e_loc)."""
    from . import sr
    lower_states, penalty = _check_lower_states(lower_states, overlap_penalty)
    if group is not None:
        raise NotImplementedError(f"{what} over sharded walkers (group=...) is not implemented: pass all walkers on one GPU")
    sr._check_damping(damping, relative_damping)
    if spring is not None:
        sr._check_spring(spring[0], 0.0, spring[1])
    sr._check_solver(solver, tol, max_iter)
    model, x, hpsi, ps, _ = _energy_terms(params, psi, h_fn, batch)
    inv = 1.0 / (ps + 1e-8)
    e_loc = hpsi * inv
    rows = model.psi_jacobian(x, w_psi=inv)
    e_used = _penalised_energies(model, x, ps, e_loc, lower_states, penalty, overlap_record) if lower_states else e_loc
    return rows, e_used, e_loc


def sr_natural_gradient(params, psi, h_fn, batch, damping=0.0, relative_damping=1e-3, group=None, solver='cholesky', tol=1e-8, max_iter=2000, *,
                        lower_states=None, overlap_penalty=0.0, overlap_record=None):
    """Stochastic reconfiguration on the walkers of `batch`: d = (S + lambda I)^-1 g with O_k(x_b) = d ln psi_b / d theta_k (the rows of
    log_psi_jacobian, written once with the weight 1 / (psi + 1e-8)), S = O^T H O / B, g = (2 / B) O^T H e_loc, e_loc = H psi / (psi + 1e-8)
    and lambda = damping + relative_damping * trace(H O O^T H / B) / B, solved in its B x B form (waveflow_amd.sr).
    -> (d float32 cuda [n_params], loss = mean e_loc).  Sharded walkers (`group`) are not supported.  solver='cg' (with tol, max_iter): the
    matrix-free solve of sr.solve_cg, for batches beyond sr.MAX_WALKERS.

    Excited states.  lower_states: a list of (psi closure, params) of states to stay orthogonal to, each closure on a DeviceModel of its own
    (another init_fun call); overlap_penalty: lambda, one number or one per state, >= 0.  The solver then receives the local energies of
    L = E + sum_k lambda_k S_k^2 (overlap.penalise: e~_b = e_b + sum_k lambda_k a_k (r_kb - a_k) with r_k = psi_k / (psi + 1e-8) and a_k its
    batch mean) in the place of e_loc; the returned loss stays the mean of the unpenalised e_loc.  overlap_record: a list that receives S_k of
    this step's walkers (float64 numpy [K]) -- how every function of this module that takes lower_states reports the overlaps; the return
    values keep their shape.  With lower_states None or empty nothing of this is called and the result is bit for bit the one without."""
    from . import sr
    rows, e_used, e_loc = _sr_rows_and_energies("stochastic reconfiguration", params, psi, h_fn, batch, damping, relative_damping, group, solver, tol, max_iter,
                                                lower_states, overlap_penalty, overlap_record)
    d = sr.natural_gradient(rows, e_used, damping=damping, relative_damping=relative_damping, **_solver_args(solver, tol, max_iter))
    return d, float(e_loc.double().mean())


def _solver_args(solver, tol, max_iter):
    """The solver keywords for sr.natural_gradient / sr.spring_direction: none for the dense solve, whose call stays as it was."""
    return {} if solver == 'cholesky' else {"solver": solver, "tol": tol, "max_iter": max_iter}


def _overlap_args(lower_states, overlap_penalty, overlap_record):
    """The excited-state keywords for sr_natural_gradient / spring_direction: none without lower states, whose call stays as it was."""
    return {"lower_states": lower_states, "overlap_penalty": overlap_penalty, "overlap_record": overlap_record} if lower_states else {}


def _stepped(params, step, d):
    """params - step * d as a new pytree of the same shape (numpy leaves), or a new core.DeviceParams when `params` is one; `params` is left as it is."""
    if isinstance(params, DeviceParams):
        return DeviceParams(params.template, params.flat - step * d.to(params.flat.device), params.version + 1)
    flat = flatten_params(params).astype(np.float32)
    return checkpoint.unflatten_like(params, flat - np.float32(step) * d.cpu().numpy())


def train_step_sr(epoch, psi, h_fn, params, batch, learning_rate, group=None, *, lower_states=None, overlap_penalty=0.0, overlap_record=None, **damping):
    """One stochastic-reconfiguration step theta <- theta - lr d (sr_natural_gradient; `damping`: its damping / relative_damping, and solver / tol / max_iter;
    learning_rate: a number, or a schedule called with `epoch`) -> (new params, loss).  `params` is left as it is: the result is a new
    pytree of the same shape (numpy leaves), or a new core.DeviceParams when `params` is one.  lower_states, overlap_penalty, overlap_record:
    as in sr_natural_gradient."""
    d, loss_val = sr_natural_gradient(params, psi, h_fn, batch, group=group, **damping, **_overlap_args(lower_states, overlap_penalty, overlap_record))
    return _stepped(params, _lr_at(learning_rate, epoch), d), loss_val


def spring_direction(params, psi, h_fn, batch, prev, momentum, damping=0.0, relative_damping=1e-3, clip=0.0, group=None, solver='cholesky', tol=1e-8,
                     max_iter=2000, *, lower_states=None, overlap_penalty=0.0, overlap_record=None):
    """The SPRING direction on the walkers of `batch` (sr.spring_direction on the rows and local energies of sr_natural_gradient): stochastic
    reconfiguration pulled towards momentum * prev, local energies clamped `clip` mean absolute deviations around their median (0: not clamped).
    prev: the previous direction, float32 cuda [n_params] (zeros at the start).  -> (d float32 cuda [n_params], loss = mean of the unclipped e_loc).
    Sharded walkers (`group`) are not supported.  solver, tol, max_iter: as in sr_natural_gradient.  lower_states, overlap_penalty,
    overlap_record: as in sr_natural_gradient -- the clip then clamps the penalised energies around their median."""
    from . import sr
    rows, e_used, e_loc = _sr_rows_and_energies("SPRING", params, psi, h_fn, batch, damping, relative_damping, group, solver, tol, max_iter, lower_states,
                                                overlap_penalty, overlap_record, spring=(momentum, clip))
    d = sr.spring_direction(rows, e_used, prev.to(rows.device), momentum, damping=damping, relative_damping=relative_damping, clip=clip,
                            **_solver_args(solver, tol, max_iter))
    return d, float(e_loc.double().mean())


def spring_step_size(learning_rate, d, norm_constraint):
    """float32 min(lr, sqrt(C / |d|^2)) with |d|^2 in float64; lr itself when C == 0 or d == 0 (the device step's rule)."""
    norm2 = float((d.double() ** 2).sum())
    eff = float(learning_rate)
    if float(norm_constraint) != 0.0 and norm2 != 0.0:
        eff = min(eff, float(np.sqrt(float(norm_constraint) / norm2)))
    return float(np.float32(eff))


def train_step_spring(epoch, psi, h_fn, params, batch, learning_rate, prev, momentum, norm_constraint, clip, group=None, *, lower_states=None,
                      overlap_penalty=0.0, overlap_record=None, **damping):
    """One SPRING step theta <- theta - eff d with d = spring_direction(...) and eff = spring_step_size(lr, d, norm_constraint)
    -> (new params, d, loss); the caller passes d as `prev` of the next step.  `params` is left as it is, as in train_step_sr.  `damping` also
    carries solver / tol / max_iter to spring_direction.  lower_states, overlap_penalty, overlap_record: as in sr_natural_gradient."""
    from . import sr
    sr._check_spring(momentum, norm_constraint, clip)
    d, loss_val = spring_direction(params, psi, h_fn, batch, prev, momentum, clip=clip, group=group, **damping,
                                   **_overlap_args(lower_states, overlap_penalty, overlap_record))
    eff = spring_step_size(_lr_at(learning_rate, epoch), d, norm_constraint)
    return _stepped(params, eff, d), d, loss_val


def _save_spring_state(save_dir, phi, epoch):
    """SPRING's previous direction next to the checkpoints, as Adam's moments are: `spring_state.npz` {phi, epoch}."""
    tmp = f"{save_dir}/spring_state.tmp.npz"
    np.savez(tmp, phi=phi.detach().cpu().numpy(), epoch=np.int64(epoch))
    os.replace(tmp, f"{save_dir}/spring_state.npz")


def _load_spring_state(save_dir, phi, epoch):
    """-> True when the direction of exactly this checkpoint epoch was restored into phi."""
    path = f"{save_dir}/spring_state.npz"
    if not os.path.isfile(path):
        return False
    with np.load(path) as z:
        if int(z["epoch"]) != int(epoch) or z["phi"].shape != tuple(phi.shape):
            return False
        import torch
        phi.copy_(torch.as_tensor(z["phi"].astype(np.float32)))
    return True


def _save_optimizer_state(save_dir, opt_state, epoch):
    """Adam's moments next to the reference's artefacts (the reference checkpoints parameters only, vqmc.py:96-100, and a restart
    there begins with a fresh optimiser): `optimizer_state.npz` {m, v, epoch}, rewritten at every checkpoint."""
    m, v = (t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t) for t in (opt_state.m, opt_state.v))
    tmp = f"{save_dir}/optimizer_state.tmp.npz"
    np.savez(tmp, m=m, v=v, epoch=np.int64(epoch))
    os.replace(tmp, f"{save_dir}/optimizer_state.npz")


def _load_optimizer_state(save_dir, opt_state, epoch):
    """-> True when the moments of exactly this checkpoint epoch were restored."""
    path = f"{save_dir}/optimizer_state.npz"
    if not os.path.isfile(path):
        return False
    with np.load(path) as z:
        if int(z["epoch"]) != int(epoch) or z["m"].shape != tuple(opt_state.m.shape):
            return False
        m, v = z["m"].astype(np.float32), z["v"].astype(np.float32)
    if opt_state.on_device:
        import torch
        opt_state.m.copy_(torch.as_tensor(m))
        opt_state.v.copy_(torch.as_tensor(v))
    else:
        opt_state.m, opt_state.v = m, v
    return True


def capture_step(model, step, warm_up=None, error=None):
    """`step` (library calls on resident data, workspaces allocated beforehand) captured once in a hipGraph on a side stream -> the callable
    that replays it.  warm_up() runs on that stream first, outside the capture: what must have happened once before the sequence is recorded,
    with whatever undoes its effects.  A failed capture leaves the side stream in an undefined capture state, so there is no fallback to
    call-by-call: RuntimeError(error) from the cause (error=None: the cause as it is)."""
    import torch
    side = torch.cuda.Stream(device=model.device)
    side.wait_stream(torch.cuda.current_stream(model.device))
    try:
        with torch.cuda.stream(side):
            if warm_up is not None:
                warm_up()
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                step()
    except Exception as e:
        if error is None:
            raise
        raise RuntimeError(error) from e
    torch.cuda.current_stream(model.device).wait_stream(side)
    return graph.replay


def loss_ring_reader(model, st, first, sign=1.0, after=None):
    """-> fetch(upto): the losses (sign * sum / count of a ring slot) of the steps after the last one fetched -- at first those from `first` on --
    up to step `upto`, read from the train state's loss ring once the device has caught up.  The caller fetches at least every ring_len steps.
    after(upto), if given, runs behind every read (what else the host looks at while the device is idle)."""
    import torch
    fetched = [first - 1]   # losses of the steps up to here are on the host
    n = st["ring_len"]

    def fetch(upto):
        torch.cuda.synchronize(model.device)
        ring = st["ring"].cpu().numpy()
        new = [float(sign * ring[e % n, 0] / ring[e % n, 2]) for e in range(fetched[0] + 1, upto + 1)]
        fetched[0] = upto
        if after is not None:
            after(upto)
        return new
    return fetch


def run_device_loop(model, opt_state, get_params, replay, fetch, record, first, last, checkpoint_every, checkpoint, fetch_every, fetched,
                    report_every=0):
    """Epochs first .. last of a step that runs on the device without the host (`replay`: one graph launch or a few library calls; losses in a
    ring, read by `fetch`) -> the final parameters.  An epoch without a boundary costs the host its modulo tests and one call of `replay`.
    checkpoint(epoch, params): before epoch 1 and every checkpoint_every-th epoch, on the parameters after epoch - 1, the losses up to there
    recorded (record(new) appends them to the caller's lists); the model's images are refreshed behind it.  fetched(epoch, new): after every
    fetch_every-th (and report_every-th, if set) epoch, with the losses since the last fetch, which it records itself.  At the end every loss
    is recorded and every image of the model, evaluation tables included, holds the final parameters."""
    for epoch in range(first, last + 1):
        if epoch % checkpoint_every == 0 or epoch == 1:
            record(fetch(epoch - 1))
            opt_state.version += 1
            checkpoint(epoch, get_params(opt_state))
            model.set_params_device(opt_state.x)
        replay()
        if epoch % fetch_every == 0 or (report_every and epoch % report_every == 0):
            fetched(epoch, fetch(epoch))
    record(fetch(last))
    opt_state.version += 1
    model.set_params_device(opt_state.x)
    return get_params(opt_state)


class _Run(SimpleNamespace):
    """What every loop of start_training works on: the model's closures, the optimiser state, `loss` and `energies` (which grow in place), the
    host generator, rank and group."""

    def record(self, new):
        self.loss.extend(new)
        self.energies.extend([[v] for v in new])

    def checkpoint(self, seed, epoch, params, save_optimizer):
        """The reference's artefacts, and Adam's moments next to them, from rank 0 (every rank draws `seed`: the host streams stay aligned)."""
        if self.rank == 0:
            helpers.create_checkpoint_wavefunc(seed, self.save_dir, self.psi, self.sample, params, epoch, self.loss, self.energies, self.system_dict)
            if save_optimizer:
                _save_optimizer_state(self.save_dir, self.opt_state, epoch)
            if getattr(self, "save_extra", None) is not None:
                self.save_extra(epoch)


# optimizer='spring': the settings tests/test_gpu_sr_spring.py trains He with (learning rate 0.1 there), measured on the MI355X -- DESIGN 4.21.
# relative_damping is what an empty sr_damping means under 'spring' (under 'sr' it stays train_step_sr's 1e-3).
SPRING_DEFAULTS = {"momentum": 0.9, "norm_constraint": 0.1, "clip": 5.0, "relative_damping": 1e-2}


def _check_distinct_start(flat0, lower_flat, k):
    """An excited model must not start on the state it avoids: at psi = psi_k the ratio r is 1 on every walker, the penalty gradient
    2 lambda a (r - a) vanishes and the point is a saddle the optimiser only leaves by noise.  ValueError when the initial parameters equal
    lower state k bit for bit."""
    a, b = np.ascontiguousarray(flat0, dtype=np.float32).reshape(-1), np.ascontiguousarray(lower_flat, dtype=np.float32).reshape(-1)
    if a.size == b.size and np.array_equal(a.view(np.int32), b.view(np.int32)):
        raise ValueError(f"lower_states[{k}] equals this trainer's initial parameters bit for bit: the overlap penalty has no gradient there; "
                         "start the excited state from another seed")


class ModelTrainer:
    """vqmc.py:19-119, same constructor arguments, attributes and on-disk artefacts."""

    def __init__(self, system_name='He', learning_rate=1e-4, box_length=10, num_epochs=200000, batch_size=128, log_every=2000):
        self.system_name = system_name
        self.n_space_dimension = 1
        self.system, self.n_particle = physics.system_catalogue[self.n_space_dimension][self.system_name]
        self.box_length = box_length
        self.xu_coord_type = 'mean'
        self.spline_degree = 6
        self.num_knots = 23
        self.n_flow_layer = 3
        self.realtime_plots = False
        self.n_plotting = 200
        self.log_every = log_every
        self.window = 100
        self.learning_rate = learning_rate
        self.num_epochs = num_epochs
        self.batch_size = batch_size
        self.save_dir = f'./results/{self.system_name}_{self.n_space_dimension}d_L{self.box_length}box'
        self.use_graph = True  # single process: capture the whole step (wf_vqmc_train_step) in a hipGraph and replay it
        self.seed = 2          # vqmc.py:57: PRNGKey(2)
        self.exact_sampler = False   # False: the reference's sampler (made.py:88 quirk); True: draws from |psi|^2
        self.optimizer = 'adam'      # 'sr': stochastic reconfiguration steps (train_step_sr; eager unless sr_on_device), one process
        self.sr_damping = {}         # damping / relative_damping of train_step_sr (its defaults when empty)
        self.sr_on_device = False    # optimizer='sr' / 'spring': True runs the whole step on the device (wf_vqmc_sr_step / wf_vqmc_spring_step), captured once when use_graph
        self.sr_solver = 'cholesky'  # eager 'sr' / 'spring' steps: 'cg' solves matrix-free (sr.solve_cg), for batch_size beyond sr.MAX_WALKERS; the device-side steps are dense
        # optimizer='spring': train_step_spring (sr_on_device as for 'sr'; an empty sr_damping means SPRING_DEFAULTS['relative_damping']); DESIGN 4.21
        self.spring_momentum = SPRING_DEFAULTS["momentum"]
        self.spring_norm_constraint = SPRING_DEFAULTS["norm_constraint"]   # the step is capped at sqrt(this) in norm; 0: no cap
        self.spring_clip = SPRING_DEFAULTS["clip"]                         # local energies clamped this many mean absolute deviations around the median; 0: off
        # excited states (eager 'sr' / 'spring' loops): the states to stay orthogonal to -- result directories of earlier runs (their
        # `checkpoints` file) or flat parameter vectors, loaded into models built with this trainer's settings -- and the penalty lambda of
        # L = E + sum_k lambda_k S_k^2, one number or one per state (above the gap to the state avoided).  S_k per epoch: self.overlap_history
        self.lower_states = []
        self.overlap_penalty = 0.0

    def _check_lower_state_settings(self, optimizer):
        """What a non-empty lower_states excludes, before anything is built -> the penalties (float32 [K]), or None without lower states."""
        lower = getattr(self, "lower_states", None)
        if lower is None or len(lower) == 0:
            return None
        from . import overlap
        if optimizer == 'adam':
            raise ValueError("lower_states with optimizer='adam': the overlap penalty is built into the eager 'sr' and 'spring' steps only")
        if getattr(self, "sr_on_device", False):
            raise ValueError("lower_states with sr_on_device=True: the device-side steps have no overlap penalty; use sr_on_device=False")
        try:
            overlap._check_K(len(lower))
        except ValueError as e:
            raise ValueError(f"lower_states: {e}") from None
        return overlap._check_penalty(getattr(self, "overlap_penalty", 0.0), len(lower))

    def _load_lower_states(self, template, flat0):
        """-> [(psi closure, DeviceParams)], one model per entry of lower_states, built with this trainer's model settings; its parameters from
        the entry: a result directory (or its `checkpoints` file), or a flat vector.  ValueError for an entry of another size, and for one that
        equals the initial parameters flat0 bit for bit (_check_distinct_start)."""
        import torch
        out = []
        for k, entry in enumerate(self.lower_states):
            if isinstance(entry, (str, os.PathLike)):
                path = os.fspath(entry)
                tree, _ = checkpoint.load_reference_checkpoint(os.path.join(path, "checkpoints") if os.path.isdir(path) else path)
                flat = flatten_params(tree)
            else:
                flat = flatten_params(entry) if isinstance(entry, (DeviceParams, tuple, list)) else np.asarray(
                    entry.detach().cpu().numpy() if hasattr(entry, "detach") else entry, dtype=np.float32).reshape(-1)
            flat = np.ascontiguousarray(flat, dtype=np.float32)
            if flat.size != flat0.size:
                raise ValueError(f"lower_states[{k}] holds {flat.size} parameters, this trainer's model has {flat0.size}")
            _check_distinct_start(flat0, flat, k)
            init_fun = _model_init_fun(self.box_length, self.n_particle, self.xu_coord_type, self.spline_degree, self.num_knots, self.n_flow_layer)
            _, psi_k, _, _ = init_fun(0, self.n_particle)
            dev = torch.as_tensor(flat).to(f"cuda:{psi_k.model.device}")
            out.append((psi_k, DeviceParams(template, dev)))
        return out

    def start_training(self, restart=False, verbose=True, group=None):
        """Under torch.distributed (one process per GPU, `torchrun examples/run_vqmc.py`) the walkers of a step are split over
        the ranks: every rank builds the same model from the same seed, draws batch_size / world walkers with its own sampler
        stream, and the step's single all-reduce (gradient + energy moments) keeps the replicas identical; rank 0 writes."""
        import torch.distributed as dist
        optimizer = getattr(self, "optimizer", "adam")
        if optimizer not in ('adam', 'sr', 'spring'):
            raise ValueError(f"optimizer must be 'adam', 'sr' or 'spring', got {optimizer!r}")
        if optimizer in ('sr', 'spring'):
            self._sr_solver_args()
        penalties = self._check_lower_state_settings(optimizer)
        distributed = dist.is_available() and dist.is_initialized()
        if optimizer in ('sr', 'spring') and (distributed or group is not None):
            raise NotImplementedError(f"optimizer={optimizer!r} runs in one process: stochastic reconfiguration over sharded walkers is not implemented")
        if distributed and group is None:
            group = dist.group.WORLD   # (None would read as "not distributed" further down: the default group, explicitly)
        rank = dist.get_rank(group) if distributed else 0
        world = dist.get_world_size(group) if distributed else 1
        local_batch = (self.batch_size * (rank + 1)) // world - (self.batch_size * rank) // world
        verbose = verbose and rank == 0
        save_dir = self.save_dir
        rng = np.random.default_rng(self.seed)
        psi, log_pdf, sample, opt_state, opt_update, get_params = create_train_state(
            self.box_length, self.learning_rate, n_particle=self.n_particle, rng=int(rng.integers(1 << 31)),
            xu_coord_type=self.xu_coord_type, spline_degree=self.spline_degree, num_knots=self.num_knots, n_flow_layers=self.n_flow_layer)
        h_fn = physics.construct_hamiltonian_function(psi, protons=self.system, n_space_dimensions=self.n_space_dimension, eps=0.0)
        start_epoch = 0
        loss, energies = [0], []
        if Path(save_dir).is_dir() and restart:
            # unlike vqmc.py:68-71, which reloads the parameters but keeps stepping the freshly initialised optimiser state
            # (so the reloaded parameters are dropped after one step), a restart here continues from the checkpoint
            params, start_epoch = checkpoint.load_reference_checkpoint(f'{save_dir}/checkpoints')
            import torch
            opt_state.x.copy_(torch.as_tensor(flatten_params(params).astype(np.float32)))
            opt_state.version += 1
            if optimizer != 'spring' and not _load_optimizer_state(save_dir, opt_state, start_epoch):
                # (a directory written by the reference, or by an older run): the moments restart from zero while the step index
                # -- and with it Adam's bias correction -- continues, so the first ~10 steps are up to 3x the nominal size
                import warnings
                warnings.warn(f"{save_dir}/optimizer_state.npz does not match checkpoint epoch {start_epoch}: Adam moments restart from zero")
            loss = np.load(f'{save_dir}/loss.npy').tolist()
            energies = np.load(f'{save_dir}/energies.npy').tolist()
        system_dict = {"system_name": self.system_name, "box_length": self.box_length, "n_particle": self.n_particle,
                       "n_space_dimension": self.n_space_dimension, "window": self.window, "n_plotting": self.n_plotting}
        if rank == 0:
            helpers.make_result_dirs(save_dir)
            with open(f"{save_dir}/system_info.json", "w") as fout_sys:
                json.dump(system_dict, fout_sys, indent=4)
        if verbose:
            print("Start training...")
        run = _Run(psi=psi, sample=sample, h_fn=h_fn, opt_state=opt_state, opt_update=opt_update, get_params=get_params, start_epoch=start_epoch,
                   loss=loss, energies=energies, system_dict=system_dict, save_dir=save_dir, rng=rng, verbose=verbose,
                   group=group if distributed else None, rank=rank, local_batch=local_batch)
        self.overlap_history = []   # S_k of every epoch's walkers (float64 numpy [K] each), when lower_states is in use
        if penalties is not None:
            run.lower_states = self._load_lower_states(opt_state.template, opt_state.x.detach().cpu().numpy())
            run.overlap_penalty, run.overlap_record = penalties, self.overlap_history
            self.lower_state_models = run.lower_states   # [(psi closure, DeviceParams)]: for measurements against them afterwards
            run.log_extra = lambda: f" | max |S_k|: {float(np.abs(self.overlap_history[-1]).max()):.4f}" if self.overlap_history else ""
        # the whole step as one captured launch sequence, where the library has it (models the sweeps cover; the wave sampler: <= 131072 walkers
        # per step, no such limit where the staged large-batch sampler applies); otherwise the host-stepped loop (sampler, loss + gradient, Adam: three library calls per step)
        # Sharded over several processes: the same sequence in two halves around the step's one all-reduce.
        fused = optimizer == 'adam' and self.use_graph and local_batch >= 1
        if fused:
            from ._lib import WfError
            try:
                fused = psi.model.train_step_workspace_bytes(local_batch) > 0
            except WfError:   # (the library has no fused step for this model or batch)
                fused = False
        if optimizer == 'sr':
            params = (self._train_sr_device if getattr(self, "sr_on_device", False) else self._train_sr)(run)
        elif optimizer == 'spring':
            params = (self._train_spring_device if getattr(self, "sr_on_device", False) else self._train_spring)(run)
        elif fused:
            params = self._train_graphed(run)
        else:
            params = self._train_adam(run, group)
        self.params, self.loss, self.energies = params, loss, energies
        self.psi, self.log_pdf, self.sample, self.h_fn = psi, log_pdf, sample, h_fn
        return params, loss

    def _train_host(self, run, step, save_optimizer):
        """The host-stepped loop: per epoch two draws from the host stream (checkpoint seed, sampler seed: the same on every rank), a checkpoint
        from rank 0 at epoch 1 and every log_every epochs, this rank's walkers, and step(epoch, params, batch) -> loss, which moves run.opt_state."""
        params = run.get_params(run.opt_state)
        for epoch in range(run.start_epoch + 1, run.start_epoch + self.num_epochs + 1):
            ckpt_seed, step_seed = int(run.rng.integers(1 << 31)), int(run.rng.integers(1 << 31))
            if epoch % self.log_every == 0 or epoch == 1:
                run.checkpoint(ckpt_seed, epoch, params, save_optimizer)
            batch = run.sample(step_seed + 7919 * run.rank, params, run.local_batch, exact_inverse=self.exact_sampler)
            new_loss = step(epoch, params, batch)
            params = run.get_params(run.opt_state)
            if epoch % self.log_every == 0 and run.verbose:
                print(f"epoch {epoch} | Loss: {round(float(new_loss), 3)}" + (run.log_extra() if getattr(run, "log_extra", None) else ""))
            run.record([new_loss])
        return params

    @staticmethod
    def _run_overlap_args(run):
        """The excited-state keywords of the eager steps from what start_training loaded: none without lower states."""
        return _overlap_args(getattr(run, "lower_states", None), getattr(run, "overlap_penalty", 0.0), getattr(run, "overlap_record", None))

    def _train_adam(self, run, group):
        """The host-stepped loop with train_step_efficient (`group` as start_training received it: None means not distributed); the running
        average follows the losses every 100 epochs, before that epoch's loss joins them (vqmc.py:112-118)."""
        average = [np.zeros(1)]

        def step(epoch, params, batch):
            run.opt_state, new_loss = train_step_efficient(epoch, run.psi, run.h_fn, run.opt_update, run.opt_state, params, batch, average[0], group=group)
            if epoch % 100 == 0:
                average[0] = np.asarray(run.loss[-100:]).mean()
            return new_loss
        return self._train_host(run, step, save_optimizer=True)

    def _sr_solver_args(self):
        """{} for the dense solve, {"solver": 'cg'} for the matrix-free one; ValueError for a solver the steps do not know, and for 'cg' together
        with sr_on_device (wf_vqmc_sr_step and wf_vqmc_spring_step factorise the B x B matrix)."""
        from . import sr
        solver = getattr(self, "sr_solver", "cholesky")
        sr._check_solver(solver)
        if solver == 'cholesky':
            return {}
        if getattr(self, "sr_on_device", False):
            raise ValueError(f"sr_solver={solver!r} with sr_on_device=True: the device-side steps solve densely (at most {sr.MAX_WALKERS} walkers); "
                             "use sr_on_device=False for the matrix-free solve")
        return {"solver": solver}

    def _train_sr(self, run):
        return self._train_sr_eager(run, spring=False)

    def _train_sr_device(self, run):
        return self._train_sr_on_device(run, spring=False)

    def _train_spring(self, run):
        return self._train_sr_eager(run, spring=True)

    def _train_spring_device(self, run):
        return self._train_sr_on_device(run, spring=True)

    def _spring_damping(self):
        return getattr(self, "sr_damping", None) or {"relative_damping": SPRING_DEFAULTS["relative_damping"]}

    def _spring_settings(self):
        return (float(getattr(self, "spring_momentum", SPRING_DEFAULTS["momentum"])),
                float(getattr(self, "spring_norm_constraint", SPRING_DEFAULTS["norm_constraint"])),
                float(getattr(self, "spring_clip", SPRING_DEFAULTS["clip"])))

    def _spring_phi(self, run):
        """The previous direction on the device of the parameters: zeros, or on a restart what the checkpoint's epoch saved."""
        import torch
        import warnings
        phi = torch.zeros_like(run.opt_state.x)
        if run.start_epoch > 0 and not _load_spring_state(run.save_dir, phi, run.start_epoch):
            warnings.warn(f"{run.save_dir}/spring_state.npz does not match checkpoint epoch {run.start_epoch}: SPRING's momentum restarts from zero")
        run.save_extra = lambda epoch: _save_spring_state(run.save_dir, phi, epoch)
        return phi

    def _train_sr_eager(self, run, spring):
        """The host-stepped loop with train_step_sr, or with spring: train_step_spring, in the place of the Adam step: eager (the solver's status is
        read every step), parameters on the device in opt_state.x, no optimiser state to save.  SPRING carries the previous direction from step to
        step, saves it with every checkpoint and reports at the end the number of steps the norm cap bound (self.spring_capped_steps)."""
        if spring:
            momentum, cap, clip = self._spring_settings()
            phi = self._spring_phi(run)
        capped = [0]

        def step(epoch, params, batch):
            if spring:
                new_params, d, new_loss = train_step_spring(epoch, run.psi, run.h_fn, params, batch, self.learning_rate, phi, momentum, cap, clip,
                                                            **self._spring_damping(), **self._sr_solver_args(), **self._run_overlap_args(run))
                capped[0] += int(spring_step_size(_lr_at(self.learning_rate, epoch), d, cap) < float(np.float32(_lr_at(self.learning_rate, epoch))))
                phi.copy_(d)
            else:
                new_params, new_loss = train_step_sr(epoch, run.psi, run.h_fn, params, batch, self.learning_rate, **getattr(self, "sr_damping", {}),
                                                     **self._sr_solver_args(), **self._run_overlap_args(run))
            run.opt_state.x.copy_(new_params.flat)
            run.opt_state.version += 1
            return new_loss
        params = self._train_host(run, step, save_optimizer=False)
        if spring:
            self.spring_capped_steps, self.spring_skipped_steps = capped[0], 0
            if run.verbose:
                print(f"SPRING: the norm constraint bound {capped[0]} of {self.num_epochs} steps")
        return params

    def _train_sr_on_device(self, run, spring):
        """optimizer='sr' or, with spring, 'spring' under sr_on_device: run_device_loop around wf_vqmc_sr_step / wf_vqmc_spring_step.  Per epoch one
        graph launch (use_graph) or one library call; the learning rate is a device scalar, rewritten before the step when `learning_rate` is a
        schedule; the host looks at the loss ring every 100 epochs and at checkpoints, and at the step's status with it: steps the solver refused
        (a pivot that is not positive, a step that is not finite) leave the parameters as they are and are reported once, with their count.
        SPRING also reads the ring of applied step sizes there: the steps the norm cap bound are counted (self.spring_capped_steps) and reported
        at the end with the skipped ones."""
        import warnings
        model, opt_state, start_epoch = run.psi.model, run.opt_state, run.start_epoch
        lr = self.learning_rate
        batch = int(self.batch_size)
        name, step_name = ("SPRING", "SPRING") if spring else ("stochastic reconfiguration", "stochastic-reconfiguration")
        if spring:
            momentum, cap, clip = self._spring_settings()
            settings = dict(self._spring_damping(), momentum=momentum, norm_constraint=cap, clip=clip)
            phi = self._spring_phi(run)
            st = model.make_spring_train_state(opt_state.x, start_epoch + 1, 0.0, ring_len=128, defer_eval_tables=True, phi=phi)
            run_step, ws_bytes, rings = model.spring_step, model.spring_step_workspace_bytes, ("ring", "norm_ring", "eff_ring", "status")
        else:
            settings = getattr(self, "sr_damping", {})
            st = model.make_sr_train_state(opt_state.x, start_epoch + 1, 0.0, ring_len=128, defer_eval_tables=True)
            run_step, ws_bytes, rings = model.sr_step, model.sr_step_workspace_bytes, ("ring", "norm_ring", "status")
        model.set_params_device(opt_state.x)
        seed = int(run.rng.integers(1 << 62))

        def step():
            run_step(st, seed, batch, run.h_fn.protons, exact_sampler=self.exact_sampler, **settings)
        st["ws"] = model._workspace(ws_bytes(batch), opt_state.x.device)   # allocated here, outside the capture
        phi0 = phi.clone() if spring else None

        def warm_up():
            # one step outside the capture (every kernel of the sequence has run once before it is recorded) at learning rate 0: the
            # parameters come out bitwise as they went in; what it left in phi, the counter, the rings and the status is put back
            step()
            if spring:
                phi.copy_(phi0)
            st["counter"].fill_(start_epoch + 1)
            for ring in rings:
                st[ring].zero_()
        launch = capture_step(model, step, warm_up, f"hipGraph capture of the {step_name} step failed") if self.use_graph else step
        if callable(lr):   # a schedule: the rate of its epoch in front of every step
            epochs = iter(range(start_epoch + 1, start_epoch + self.num_epochs + 1))

            def replay():
                st["step_size"].fill_(_lr_at(lr, next(epochs)))
                launch()
        else:
            st["step_size"].fill_(float(lr))
            replay = launch
        warned, seen, capped = [False], [start_epoch], [0]

        def status(upto):
            info, skipped = (int(v) for v in st["status"].cpu().tolist())
            if spring:
                eff = st["eff_ring"].cpu().numpy()
                for e in range(seen[0] + 1, upto + 1):
                    capped[0] += int(0.0 < eff[e % st["ring_len"]] < float(np.float32(_lr_at(lr, e))))
                seen[0] = max(seen[0], upto)
                self.spring_capped_steps, self.spring_skipped_steps = capped[0], skipped
            if skipped and not warned[0]:
                warned[0] = True
                warnings.warn(f"{name}: {skipped} of the first {upto - start_epoch} steps were skipped (status of the last step: {info}; > 0: that pivot of "
                              f"the shifted B x B matrix is not positive, -1: the step is not finite) -- more damping")

        def fetched(epoch, new):
            run.record(new)
            if epoch % self.log_every == 0 and run.verbose:
                print(f"epoch {epoch} | Loss: {round(float(new[-1]), 3)}")
        params = run_device_loop(model, opt_state, run.get_params, replay, loss_ring_reader(model, st, start_epoch + 1, after=status), run.record,
                                 start_epoch + 1, start_epoch + self.num_epochs, self.log_every,
                                 lambda epoch, params: run.checkpoint(int(run.rng.integers(1 << 31)), epoch, params, False), 100, fetched)
        if spring and run.verbose:
            print(f"SPRING: the norm constraint bound {capped[0]} and the solver skipped {self.spring_skipped_steps} of {self.num_epochs} steps")
        return params

    def _train_graphed(self, run):
        """The training loop with the step captured once in a hipGraph (run_device_loop): per epoch one graph launch; the host looks at the
        losses every 100 epochs (to refresh the running average, vqmc.py:112-113) and at checkpoints.
        With run.group (one process per GPU) the step is wf_vqmc_train_step_local -> all-reduce of one packed fp64 buffer ->
        wf_vqmc_train_step_apply, issued call by call (WF_GRAPH_COLLECTIVE=1 captures it with the RCCL collective inside) -- either
        way without a host synchronisation per step."""
        import torch
        from .distributed import _all_reduce_sum
        model, opt_state, start_epoch, group, rank, local_batch = run.psi.model, run.opt_state, run.start_epoch, run.group, run.rank, run.local_batch
        # (the steps leave out the tables only the large-batch evaluation kernel reads; every evaluation below goes through
        # ensure_params / set_params_device first, and the loop ends with a full refresh)
        # Large batches are the exception: from WF_GRAD_TILE_MIN walkers per step on (default 16 384) the loss + gradient of the two-particle family runs
        # on the matrix cores (wf_kernels_etile.hip), which reads those tables -- the steps then refresh everything (tens of microseconds against
        # milliseconds of step)
        tile_min = int(os.environ.get("WF_GRAD_TILE_MIN", 16384))
        sample_min = int(os.environ.get("WF_SAMPLE_TILE_MIN", 16384))   # (the staged sampler of large batches reads them too)
        per_step = int(local_batch) if group is not None else int(self.batch_size)
        large = (tile_min > 0 and per_step >= tile_min) or (sample_min > 0 and per_step >= sample_min)
        st = model.make_train_state(opt_state.x, opt_state.m, opt_state.v, start_epoch + 1, ring_len=128, defer_eval_tables=not large)
        model.set_params_device(opt_state.x)
        seed = int(run.rng.integers(1 << 62))
        warm_up, capture = None, True
        if group is None:
            def step():
                model.train_step(st, seed, self.batch_size, run.h_fn.protons, self.learning_rate, exact_sampler=self.exact_sampler)
        else:
            import torch.distributed as dist
            red = torch.zeros(model.n_params + 3, dtype=torch.float64, device=opt_state.x.device)

            def step():   # every rank draws its own walkers (stream seed + 7919 rank); the tangent rule carries 1 / global batch
                model.train_step_local(st, seed + 7919 * rank, local_batch, run.h_fn.protons, 1.0 / float(self.batch_size), red, exact_sampler=self.exact_sampler)
                _all_reduce_sum(red, group)
                model.train_step_apply(st, red, self.learning_rate)

            def warm_up():   # RCCL sets up its communicator at the first collective: outside the capture
                _all_reduce_sum(torch.zeros(8, dtype=torch.float64, device=opt_state.x.device), group)
            # Capturing the collective in the graph measured no faster than issuing the three calls (4.91 vs 4.94 s per 20 000 steps, one
            # rank) and could not be tried on several GPUs here: opt-in.
            capture = dist.get_backend(group) == "nccl" and os.environ.get("WF_GRAPH_COLLECTIVE") == "1"
        st["ws"] = model._workspace(model.train_step_workspace_bytes(per_step), opt_state.x.device)   # allocated here, outside the capture
        replay = step if not capture else capture_step(model, step, warm_up, "hipGraph capture of the training step failed" + (
            " (WF_GRAPH_COLLECTIVE=1: the RCCL all-reduce inside the graph; unset it to issue the three calls per step instead)" if group is not None else ""))

        def fetched(epoch, new):
            run.record(new[:-1])
            st["running_average"].fill_(float(np.asarray(run.loss[-100:]).mean()))   # before this epoch's loss joins (vqmc.py:112-118)
            run.record(new[-1:])
            if epoch % self.log_every == 0 and run.verbose:
                print(f"epoch {epoch} | Loss: {round(float(new[-1]), 3)}")
        return run_device_loop(model, opt_state, run.get_params, replay, loss_ring_reader(model, st, start_epoch + 1), run.record,
                               start_epoch + 1, start_epoch + self.num_epochs, self.log_every,
                               lambda epoch, params: run.checkpoint(int(run.rng.integers(1 << 31)), epoch, params, True), 100, fetched)
