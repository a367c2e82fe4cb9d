"""Does optimizer = 'spring' train He from a fresh initialisation, and with which settings?  The runs behind DESIGN 4.21 and
profiles/spring_training_runs.txt: ModelTrainer on the device path (He, box 10, exact sampler, 512 walkers, --steps steps), then the energy on
4 x 2^15 independent |psi|^2 walkers, as tests/test_gpu_sr_spring.py evaluates it.

  the search   Adam (lr 5e-4) and every setting of SEARCH at the first seed
  the table    Adam and the shipped setting (vqmc.SPRING_DEFAULTS at lr 0.1) at every seed of --seeds

Prints one JSON line per run: optimiser, seed, steps, the settings, mean, sem and median of the local energy, whether all parameters are
finite, skipped and capped steps, the last recorded loss, seconds of training and of evaluation.

    python examples/spring_training_runs.py [--steps 300] [--seeds 2 3 4 5] [--table-only]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveflow_amd import vqmc  # noqa: E402

D = vqmc.SPRING_DEFAULTS
# (lr, momentum, norm constraint, relative damping, clip): the SPRING paper's values as remembered first, the shipped ones among the rest
SEARCH = [(2e-2, 0.99, 1e-3, 1e-3, 5.0), (2e-2, 0.9, 1e-3, 1e-3, 5.0), (5e-2, 0.9, 1e-2, 1e-3, 5.0), (2e-2, 0.0, 1e-3, 1e-3, 5.0),
          (1e-1, 0.9, 1e-2, 1e-3, 5.0), (5e-2, 0.99, 1e-2, 1e-3, 5.0), (1e-1, D["momentum"], D["norm_constraint"], D["relative_damping"], D["clip"]),
          (2e-2, 0.9, 1e-3, 1e-3, 0.0), (1e-2, 0.9, 1e-4, 1e-3, 5.0), (1e-1, 0.95, 3e-2, 1e-3, 5.0)]
SHIPPED = SEARCH[6]


def run(optimizer, seed, steps, setting, save_dir):
    lr, mu, cap, lam, clip = setting
    t = vqmc.ModelTrainer(system_name="He", learning_rate=lr if optimizer == 'spring' else 5e-4, box_length=10, num_epochs=steps, batch_size=512,
                          log_every=10 ** 9)
    t.save_dir, t.seed, t.exact_sampler, t.optimizer, t.sr_on_device = save_dir, seed, True, optimizer, True
    t.spring_momentum, t.spring_norm_constraint, t.spring_clip, t.sr_damping = mu, cap, clip, {"relative_damping": lam}
    t0 = time.perf_counter()
    params, loss = t.start_training(verbose=False)
    t1 = time.perf_counter()
    m = t.psi.model
    m.ensure_params(params)
    es = []
    for s in range(4):
        x = m.sample(500 + s, 1 << 15, exact=True)
        h, ps = m.hamiltonian(x, t.h_fn.protons, return_psi=True)
        es.append((h / (ps + 1e-8)).double().cpu().numpy())
    e = np.concatenate(es)
    spring = optimizer == 'spring'
    if not spring:
        mu = cap = lam = clip = None   # (Adam reads none of them)
    return {"opt": optimizer, "seed": seed, "n": steps, "lr": t.learning_rate, "mu": mu, "cap": cap, "lam": lam, "clip": clip, "mean": float(e.mean()),
            "sem": float(e.std() / np.sqrt(e.size)), "median": float(np.median(e)), "finite": bool(np.isfinite(params.flat.cpu().numpy()).all()),
            "skipped": t.spring_skipped_steps if spring else None, "capped": t.spring_capped_steps if spring else None, "last_loss": float(loss[-1]),
            "train_s": round(t1 - t0, 2), "eval_s": round(time.perf_counter() - t1, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--seeds", type=int, nargs="+", default=[2, 3, 4, 5])
    ap.add_argument("--table-only", action="store_true", help="skip the search at the first seed")
    a = ap.parse_args()
    jobs = []
    if not a.table_only:
        jobs += [("adam", a.seeds[0], SHIPPED)] + [("spring", a.seeds[0], s) for s in SEARCH]
    for seed in a.seeds:
        jobs += [("adam", seed, SHIPPED), ("spring", seed, SHIPPED)]
    with tempfile.TemporaryDirectory() as tmp:
        for i, (optimizer, seed, setting) in enumerate(jobs):
            print(json.dumps(run(optimizer, seed, a.steps, setting, os.path.join(tmp, str(i)))), flush=True)


if __name__ == "__main__":
    main()
