#!/usr/bin/env python3
"""From a wavefunction to its fixed-node DMC energy on MI355X, next to its variational energy.

psi comes from --checkpoint (a reference `checkpoints` pickle) or, without one, from a training run here (--train-epochs Adam steps of 512
walkers on 1-D He, as tests/test_gpu_grad.py::test_trained_energy_respects_the_variational_bound trains it; the shipped fixture
tests/golden/he_checkpoint.npz is kept for parity and is no ground state).  E_VMC is measured on --vmc-walkers walkers of the
exact sampler (observables.measure); E_DMC by dmc.run for every --tau given: --walkers walkers, equilibrated for --equil-time a.u. of
imaginary time (at least 30: the excited antisymmetric states of He decay with 5.7 a.u.), then --steps measured generations, one captured
step replayed, the host waits once at the end.  In one dimension the fixed-node energy is the exact eigenvalue (-1.8161 for He in the box
of 10, scratch/he1d_exact.py) up to the time-step error, which two values of --tau bracket.

--forward-walk SLOTS STRIDE adds forward walking (dmc_observables): V_en and V_ee per lag of 0, STRIDE, ..., SLOTS * STRIDE
generations, next to the VMC values and the extrapolated estimator 2 * mixed - VMC.  Exact for 1-D He, L = 10: -2.5942 and 0.40462
(scratch/he1d_exact_parts.py).

    python examples/run_vqmc_dmc.py [--checkpoint PATH] [--walkers 2048] [--tau 0.05 0.025] [--steps 1500] [--forward-walk 8 25]
"""
import argparse
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--checkpoint", default=None, help="reference `checkpoints` pickle; default: train here")
ap.add_argument("--train-epochs", type=int, default=20000)
ap.add_argument("--walkers", type=int, default=2048)
ap.add_argument("--tau", type=float, nargs="+", default=[0.05, 0.025])
ap.add_argument("--steps", type=int, default=1500, help="measured generations at the first tau; the others get the same imaginary time")
ap.add_argument("--equil-time", type=float, default=30.0, help="imaginary time that is discarded, in a.u.")
ap.add_argument("--vmc-walkers", type=int, default=1 << 20)
ap.add_argument("--limit-drift", action="store_true")
ap.add_argument("--e-cut", type=float, default=0.0)
ap.add_argument("--box-length", type=float, default=10)
ap.add_argument("--seed", type=int, default=1234)
ap.add_argument("--forward-walk", type=int, nargs=2, default=None, metavar=("SLOTS", "STRIDE"),
                help="forward walking with SLOTS tag slots (1 .. 16), measured and tagged every STRIDE generations")
ap.add_argument("--no-graph", action="store_true", help="call the step instead of replaying its capture")
args = ap.parse_args()

import torch
from waveflow_amd import checkpoint, dmc, dmc_observables, observables, vqmc
from waveflow_amd.core import flatten_params
from waveflow_amd.model_factory import get_waveflow_model
from waveflow_amd.utils import physics

protons, n_particle = physics.system_catalogue[1]["He"]
if args.checkpoint:
    # vqmc.ModelTrainer defaults (vqmc.py:26-34) + examples/run_vqmc.py:3-13
    init_fun = get_waveflow_model(n_particle, base_spline_degree=6, i_spline_degree=6, n_prior_internal_knots=23, n_i_internal_knots=23,
                                  i_spline_reg=0.05, i_spline_reverse_fun_tol=0.000001, n_flow_layers=3, box_size=args.box_length,
                                  xu_coord_type="mean")
    _, psi, _, _ = init_fun(2, n_particle)
    params, epoch = checkpoint.load_reference_checkpoint(args.checkpoint)
    model = psi.model
    flat = torch.as_tensor(np.asarray(flatten_params(params), dtype=np.float32)).cuda()
    model.set_params_device(flat)
    print(f"checkpoint {args.checkpoint}, epoch {epoch}")
else:
    t = vqmc.ModelTrainer(system_name="He", learning_rate=5e-4, box_length=args.box_length, num_epochs=args.train_epochs, batch_size=512,
                          log_every=10 ** 9)
    t.save_dir = tempfile.mkdtemp(prefix="run_vqmc_dmc_")
    t.exact_sampler = True
    params, _ = t.start_training(verbose=False)
    model = t.psi.model
    model.ensure_params(params)
    print(f"trained here: {args.train_epochs} Adam steps of 512 walkers")

vmc_totals = observables.measure(model, protons, args.vmc_walkers, min(args.vmc_walkers, 1 << 17), args.seed, use_graph=not args.no_graph)
r = vmc_totals.result()
print(f"E_VMC = {r['e_loc']:.5f} +- {r['e_loc_stderr']:.5f}   ({r['n']} walkers of |psi|^2, {r['n_skipped']} skipped)")
results = []
for tau in args.tau:
    n_equil = int(np.ceil(args.equil_time / tau - 1e-9))
    n_steps = int(round(args.steps * args.tau[0] / tau))
    # the same bins as observables.measure's default accumulator, so that the two sides can be subtracted
    fw = model.make_forward_walk(args.walkers, args.forward_walk[0], args.forward_walk[1], series_len=n_steps) if args.forward_walk else None
    d = dmc.run(model, protons, args.walkers, tau, n_steps, n_equil, args.seed, limit_drift=args.limit_drift, e_cut=args.e_cut,
                use_graph=not args.no_graph, forward_walk=fw)
    results.append(d)
    print(f"tau {tau:g}: E_DMC = {d['e_dmc']:.5f} +- {d['e_dmc_stderr']:.5f} (mixed), {d['e_growth_mean']:.5f} +- {d['e_growth_stderr']:.5f} (growth); "
          f"{n_equil} + {n_steps} generations of {args.walkers} walkers, acceptance {d['acceptance']:.4f}, left the domain {d['left_domain']}, "
          f"not finite {d['not_finite']}, status {d['status']}")
    if fw is not None:
        f = d["forward_walk"]
        print(f"  VMC:               V_en = {r['v_en']:.5f} +- {r['v_en_stderr']:.5f}   V_ee = {r['v_ee']:.5f} +- {r['v_ee_stderr']:.5f}")
        for j, lag in enumerate(f["lag"]):
            print(f"  lag {lag:5d} ({lag * tau:6.2f} a.u.): V_en = {f['v_en'][j]:.5f} +- {f['v_en_stderr'][j]:.5f}   V_ee = {f['v_ee'][j]:.5f} +- "
                  f"{f['v_ee_stderr'][j]:.5f}   surviving ancestors {f['distinct_fraction'][j]:.3f}" + ("   (mixed)" if j == 0 else ""))
        e = dmc_observables.extrapolated(f, vmc_totals)
        print(f"  2 mixed - VMC:     V_en = {e['v_en']:.5f}   V_ee = {e['v_ee']:.5f}")
if len(results) > 1:
    a, b = results[0], results[1]
    print(f"|E(tau = {args.tau[0]:g}) - E(tau = {args.tau[1]:g})| = {abs(a['e_dmc'] - b['e_dmc']):.5f} "
          f"(combined error {np.hypot(a['e_dmc_stderr'], b['e_dmc_stderr']):.5f})")
print("exact antisymmetric ground state of 1-D He, L = 10: -1.8161" + ("; <V_en> -2.5942, <V_ee> 0.40462" if args.forward_walk else ""))
