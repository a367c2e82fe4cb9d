#!/usr/bin/env python3
"""The three lowest antisymmetric states of He in the L = 10 box on MI355X: the ground state with SPRING on the device, then the second and
the third state with eager SPRING steps penalised against the states before (ModelTrainer.lower_states / overlap_penalty: the local energies
of L = E + sum_k lambda_k S_k^2), each from a trainer seed of its own.  Prints the energies on fresh walkers next to the
finite-difference levels and the overlap matrix (overlap.overlap_matrix: every off-diagonal entry estimated from both sides).

    python examples/run_vqmc_excited.py [--ground-steps 300] [--steps 1500] [--penalty 1.0] [--walkers 131072] [--save-dir DIR]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--ground-steps", type=int, default=300)
ap.add_argument("--steps", type=int, default=1500, help="penalised steps per excited state")
ap.add_argument("--penalty", type=float, default=1.0, help="lambda: above the gap to every state avoided (0.176 and 0.261 here)")
ap.add_argument("--batch", type=int, default=512)
ap.add_argument("--learning-rate", type=float, default=0.1)
ap.add_argument("--walkers", type=int, default=1 << 17, help="fresh walkers per energy and per row of the overlap matrix")
ap.add_argument("--seed", type=int, default=2, help="trainer seed of the ground state; state k trains from seed + k")
ap.add_argument("--save-dir", default="./results/He_1d_excited")
args = ap.parse_args()

import torch  # noqa: E402,F401
from waveflow_amd import overlap, vqmc  # noqa: E402

EXACT = (-1.8161, -1.6400, -1.5550)   # finite differences, n = 400 (scratch/he1d_exact.py extended to three levels)


def train(k, lower):
    t = vqmc.ModelTrainer(system_name="He", learning_rate=args.learning_rate, box_length=10, num_epochs=args.steps if k else args.ground_steps,
                          batch_size=args.batch, log_every=100)
    t.save_dir = os.path.join(args.save_dir, f"state{k}")
    t.seed = args.seed + k
    t.exact_sampler = True
    t.optimizer = 'spring'
    t.sr_on_device = k == 0          # the penalised steps are eager
    t.lower_states = lower
    t.overlap_penalty = args.penalty
    params, _ = t.start_training(verbose=True)
    t.psi.model.ensure_params(params)
    return t, params


def energy(t):
    m, es = t.psi.model, []
    for s in range(-(-args.walkers // (1 << 15))):
        x = m.sample(500 + s, 1 << 15, exact=True)
        h, ps = m.hamiltonian(x, t.h_fn.protons, return_psi=True)
        es.append((h / (ps + 1e-8)).double().cpu().numpy())
    e = np.concatenate(es)
    e = e[np.isfinite(e)]
    return e.mean(), e.std() / np.sqrt(e.size), np.median(e)


trainers, flats = [], []
for k in range(3):
    t, params = train(k, list(flats))
    trainers.append(t)
    flats.append(params.flat.clone())
print()
for k, t in enumerate(trainers):
    e, sem, med = energy(t)
    print(f"state {k}: E = {e:.5f} +- {sem:.5f} (median {med:.5f})   finite differences {EXACT[k]:.4f}")
m = overlap.overlap_matrix([t.psi.model for t in trainers], args.walkers, min(args.walkers, 1 << 15), 99)
np.set_printoptions(precision=4, suppress=True)
print("overlaps <psi_j|psi_i> on the walkers of i (rows):")
print(m["raw"])
print("standard errors:")
print(m["raw_stderr"])
print("symmetrised:")
print(m["overlap"])
