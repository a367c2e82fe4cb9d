"""Per-step time of the SPRING step (wf_vqmc_spring_step) for He (32 588 parameters) at 128, 1024 and 4096 walkers per step against the
stochastic-reconfiguration step it extends (wf_vqmc_sr_step), all captured once in a hipGraph and replayed in the same process:

  sr           DeviceModel.sr_step -- the yardstick
  spring_off   DeviceModel.spring_step with momentum, norm constraint and clip off: the launches of `sr` (one sequence serves both entries)
               plus phi <- d in the update
  spring       DeviceModel.spring_step at --momentum / --norm-constraint / --clip: two launches more than `sr` (e_loc ahead of the rows,
               q = O phi: one more pass over the rows) and the one-workgroup sort of the local energies

and, on their own on the rows of the last step's size (random fp32 [B, n_params]): sr.matvec, sr.apply and sr.apply_add, the passes over the
rows the step's excess is measured against.  Learning rate 0 by default, as in bench_sr_step.py: the work per step does not drift.  A repeat
times --steps consecutive steps between two hipEvents; each variant first runs until --warmup-seconds have passed; then --repeats rounds in
which the variants alternate.  Prints one JSON line per batch size.

    python examples/bench_spring.py [--repeats 7] [--batches 128 1024 4096]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveflow_amd import core, model_factory, sr, vqmc  # noqa: E402
from waveflow_amd.utils import physics  # noqa: E402

SEED = 11


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 1024, 4096])
    ap.add_argument("--steps", type=int, nargs="+", default=None, help="steps per timed window, one per batch size (default: 200, 20, 5)")
    ap.add_argument("--warmup-seconds", type=float, default=2.0)
    ap.add_argument("--learning-rate", type=float, default=0.0)
    ap.add_argument("--momentum", type=float, default=vqmc.SPRING_DEFAULTS["momentum"])
    ap.add_argument("--norm-constraint", type=float, default=vqmc.SPRING_DEFAULTS["norm_constraint"])
    ap.add_argument("--clip", type=float, default=vqmc.SPRING_DEFAULTS["clip"])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_spring.py needs a GPU"
    assert a.repeats >= 5
    LR = a.learning_rate
    steps_of = dict(zip(a.batches, a.steps)) if a.steps else {}
    init_fun = model_factory.get_waveflow_model(2, base_spline_degree=6, i_spline_degree=6, n_prior_internal_knots=23, n_i_internal_knots=23,
                                                i_spline_reg=0.05, n_flow_layers=3, box_size=10.0)
    template, psi, _, _ = init_fun(42, 2)
    model = psi.model
    protons, _ = physics.system_catalogue[1]["He"]
    h_fn = physics.construct_hamiltonian_function(psi, protons=protons, n_space_dimensions=1, eps=0.0)
    flat0 = torch.as_tensor(core.flatten_params(template).astype(np.float32)).cuda()
    P = model.n_params

    def window(fn, n):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn(n)
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / n

    def measure(variants, n_steps):
        for fn in variants.values():
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < a.warmup_seconds:
                fn(n_steps)
                torch.cuda.synchronize()
        ts = {k: [] for k in variants}
        for _ in range(a.repeats):
            for k, fn in variants.items():
                ts[k].append(window(fn, n_steps))
        torch.cuda.synchronize()
        return {k: {"mean": float(f"{np.mean(v):.4g}"), "min": float(f"{np.min(v):.4g}"), "max": float(f"{np.max(v):.4g}")} for k, v in ts.items()}

    for B in a.batches:
        n_steps = steps_of.get(B, 200 if B <= 256 else 20 if B <= 2048 else 5)
        settings = {"sr": None, "spring_off": (0.0, 0.0, 0.0), "spring": (a.momentum, a.norm_constraint, a.clip)}
        states, variants = {}, {}
        for name, s in settings.items():
            x = flat0.clone()
            if s is None:
                st = model.make_sr_train_state(x, 1, LR, defer_eval_tables=True)
                st["ws"] = model._workspace(model.sr_step_workspace_bytes(B), x.device)
            else:
                st = model.make_spring_train_state(x, 1, LR, defer_eval_tables=True)
                st["ws"] = model._workspace(model.spring_step_workspace_bytes(B), x.device)
            states[name] = (x, st)

            def step(st=st, s=s):
                if s is None:
                    model.sr_step(st, SEED, B, h_fn.protons)
                else:
                    model.spring_step(st, SEED, B, h_fn.protons, momentum=s[0], norm_constraint=s[1], clip=s[2])
            model.set_params_device(x)
            replay = vqmc.capture_step(model, step, warm_up=step)

            def steps(n, x=x, replay=replay):
                model.set_params_device(x)   # (the model's images follow whichever parameter vector stepped last)
                for _ in range(n):
                    replay()
            variants[name] = steps
        r = {"model": "He", "batch": B, "n_params": P, "repeats": a.repeats, "learning_rate": LR, "steps_per_window": n_steps,
             "spring_settings": {"momentum": a.momentum, "norm_constraint": a.norm_constraint, "clip": a.clip},
             "ms_per_step": measure(variants, n_steps)}
        m = r["ms_per_step"]
        r["spring_minus_sr_ms"] = float(f"{m['spring']['mean'] - m['sr']['mean']:.4g}")
        r["skipped_steps"] = {k: int(states[k][1]["status"][1].item()) for k in states}
        # the passes over the rows on their own
        rows = torch.randn(B, P, device="cuda")
        v, y = torch.randn(P, device="cuda"), torch.randn(B, device="cuda", dtype=torch.float64)
        ws = sr._workspace(B, P, rows.device)
        out = torch.empty(P, device="cuda")
        passes = {"matvec": lambda n: [sr.matvec(rows, v) for _ in range(n)],
                  "apply": lambda n: [sr.apply(rows, y, 2.0 / B, workspace=ws) for _ in range(n)],
                  "apply_add": lambda n: [sr.apply_add(rows, y, 2.0 / B, prev=v, mu=a.momentum, out=out, workspace=ws) for _ in range(n)]}
        r["row_passes_ms"] = measure(passes, n_steps)
        r["rows_bytes"] = B * P * 4
        print(json.dumps(r), flush=True)
        del variants, states, rows
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
