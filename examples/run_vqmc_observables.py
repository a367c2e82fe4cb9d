#!/usr/bin/env python3
"""Measurement counterpart of examples/run_vqmc_eval.py on MI355X: loads a checkpoint (reference pickle) or the shipped He parameters and
measures, over --walkers walkers drawn from |psi|^2 in steps of --batch on the device (observables.measure: one captured step, replayed; no
host round trip until the end), the local energy with its standard error, its split into T_lap, V_en and V_ee, the gradient-form kinetic
energy T_grad, the one-body density and the pair-distance distribution.  Under torch.distributed.run every rank measures --walkers walkers
of its own sampler stream and the totals are combined with two all-reduces (observables.Totals.all_reduce).

    python examples/run_vqmc_observables.py [--checkpoint PATH] [--walkers 16777216] [--batch 131072] [--bins 200] [--save-dir DIR]
    python -m torch.distributed.run --nproc-per-node 8 examples/run_vqmc_observables.py ...
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--checkpoint", default=None, help="reference `checkpoints` pickle; default: the shipped He parameters")
ap.add_argument("--walkers", type=int, default=1 << 24, help="walkers per GPU")
ap.add_argument("--batch", type=int, default=1 << 17, help="walkers per step")
ap.add_argument("--bins", type=int, default=200, help="bins of the density and of the pair-distance histogram")
ap.add_argument("--box-length", type=float, default=10)
ap.add_argument("--seed", type=int, default=1234)
ap.add_argument("--save-dir", default="./results/He_1d_observables", help="where observables.npz goes (rank 0)")
ap.add_argument("--reproduce-made-inverse", action="store_true", help="the sampler that reproduces made.py:88 instead of the exact one")
ap.add_argument("--no-graph", action="store_true", help="call the step instead of replaying its capture")
args = ap.parse_args()

import torch
import torch.distributed as dist
from waveflow_amd import checkpoint, observables
from waveflow_amd.core import flatten_params
from waveflow_amd.model_factory import get_waveflow_model
from waveflow_amd.utils import physics

rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", 0)))
if world > 1:
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("nccl")

# vqmc.ModelTrainer defaults (vqmc.py:26-34) + examples/run_vqmc.py:3-13
system_name, n_space_dimension = "He", 1
protons, n_particle = physics.system_catalogue[n_space_dimension][system_name]
spline_degree, num_knots, n_flow_layer = 6, 23, 3
init_fun = get_waveflow_model(n_particle, base_spline_degree=spline_degree, i_spline_degree=spline_degree, n_prior_internal_knots=num_knots,
                              n_i_internal_knots=num_knots, i_spline_reg=0.05, i_spline_reverse_fun_tol=0.000001,
                              n_flow_layers=n_flow_layer, box_size=args.box_length, xu_coord_type="mean")
params, psi, log_pdf, sample = init_fun(2, n_particle)
if args.checkpoint:
    params, epoch = checkpoint.load_reference_checkpoint(args.checkpoint)
    flat = flatten_params(params)
else:
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "he_checkpoint.npz"))
    flat, epoch = z["flat"], int(z["epoch"])
model = psi.model
model.set_params_device(torch.as_tensor(np.asarray(flat, dtype=np.float32)).cuda())

acc = observables.Accumulator(model.D, args.bins, args.bins, model=model)
totals = observables.measure(model, protons, args.walkers, args.batch, args.seed + 7919 * rank, exact_sampler=not args.reproduce_made_inverse,
                             acc=acc, use_graph=not args.no_graph)
if world > 1:
    totals.all_reduce()
if rank == 0:
    r = totals.result()
    print(f"epoch {epoch} | {r['n']} walkers on {world} GPU(s), {r['n_skipped']} skipped, {r['outside_density']} coordinates and "
          f"{r['outside_pair']} pairs outside the histograms")
    for name in observables.SCALARS:
        print(f"  <{name:6s}> = {r[name]: .6f} +- {r[name + '_stderr']:.6f}" + ("   (error bar indicative: infinite variance at the nodes)" if name == "t_grad" else ""))
    print(f"  <e_loc> - (<t_lap> + <v_en> + <v_ee>) = {r['e_loc'] - (r['t_lap'] + r['v_en'] + r['v_ee']): .3e}")
    print(f"  <t_lap> - <t_grad>                    = {r['t_lap'] - r['t_grad']: .3e}")
    os.makedirs(args.save_dir, exist_ok=True)
    path = os.path.join(args.save_dir, "observables.npz")
    np.savez(path, **totals.arrays(), **{k: np.asarray(v) for k, v in r.items()})
    print("wrote", path)
if world > 1:
    dist.destroy_process_group()
