"""Time of the overlap machinery for the shipped He model, each measurement beside the same run without the new work:

  step      DeviceModel.overlap_step with K references (sampler, K + 1 wf_psi_fwd calls, wf_overlap_accumulate), captured once in a hipGraph
            and replayed at --batch walkers
  parts     model.sample + K + 1 model.psi calls at the same batch in the same process: the walkers and the amplitudes without any
            measurement, with torch's allocations of their outputs as an eager caller pays them
  spring    vqmc.train_step_spring, eager, --train-batch walkers: plain, and penalised against K lower states (K = 1, 2)

A repeat times --steps consecutive steps between two hipEvents (the eager SPRING steps: wall clock around a device synchronisation, since
each step reads its loss on the host).  Each variant first runs until --warmup-seconds have passed; then --repeats rounds in which the
variants alternate.  Prints one JSON line per measurement: mean and min .. max in ms per step.

    python examples/bench_overlap.py [--repeats 7]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveflow_amd import checkpoint, model_factory, overlap, vqmc  # noqa: E402
from waveflow_amd.utils import physics  # noqa: E402

SEED = 11


def he(flat):
    init_fun = model_factory.get_waveflow_model(2, base_spline_degree=6, i_spline_degree=6, n_prior_internal_knots=23, n_i_internal_knots=23,
                                                i_spline_reg=0.05, n_flow_layers=3, box_size=10.0)
    params, psi, _, _ = init_fun(42, 2)
    psi.model.set_params(flat)
    return checkpoint.unflatten_like(params, flat), psi


def stats(v):
    return {"mean": float(f"{np.mean(v):.4g}"), "min": float(f"{np.min(v):.4g}"), "max": float(f"{np.max(v):.4g}")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=1 << 17)
    ap.add_argument("--train-batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed window")
    ap.add_argument("--warmup-seconds", type=float, default=2.0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_overlap.py needs a GPU"
    assert a.repeats >= 5
    pa = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "he_checkpoint.npz"))["flat"].astype(np.float32)
    g = np.random.default_rng(0)
    flats = [pa] + [(pa + 0.05 * g.standard_normal(pa.shape)).astype(np.float32) for _ in range(2)]
    states = [he(f) for f in flats]
    model = states[0][1].model

    def window(fn, n):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn(n)
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / n

    def wall(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(n)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    def run(variants, timer):
        warm = {}
        for k, fn in variants.items():
            t0, n = time.perf_counter(), 0
            while time.perf_counter() - t0 < a.warmup_seconds:
                fn(a.steps)
                torch.cuda.synchronize()
                n += a.steps
            warm[k] = n
        ts = {k: [] for k in variants}
        for _ in range(a.repeats):
            for k, fn in variants.items():
                ts[k].append(timer(fn, a.steps))
        torch.cuda.synchronize()
        return ts, warm

    # ---- the measurement step beside sampler + psi calls
    B = a.batch
    for K in (1, 2):
        refs = [s[1].model for s in states[1:1 + K]]
        acc = overlap.Accumulator(K, f"cuda:{model.device}")
        counter = torch.zeros(1, dtype=torch.int64, device=acc.device)
        acc.st["ws"] = model._workspace(model.overlap_step_workspace_bytes(B, K), acc.device)

        def step():
            model.overlap_step(refs, acc, counter, SEED, B, exact_sampler=True)
        launch = vqmc.capture_step(model, step, warm_up=step)
        drawn = [0]

        def step_steps(n):
            for _ in range(n):
                launch()

        def parts_steps(n):
            for _ in range(n):
                drawn[0] += 1
                x = model.sample(SEED + drawn[0], B, exact=True)
                model.psi(x)
                for r in refs:
                    r.psi(x)
        variants = {"step": step_steps, "parts": parts_steps}
        ts, warm = run(variants, window)
        res = acc.totals().result()
        r = {"what": "overlap_step", "model": "He", "batch": B, "K": K, "captured": True, "repeats": a.repeats, "steps_per_window": a.steps, "warmup_steps": warm,
             "workspace_bytes": int(acc.st["ws"].numel()), "step_ms": stats(ts["step"]), "parts_ms": stats(ts["parts"]),
             "step_over_parts": float(f"{np.mean(ts['step']) / np.mean(ts['parts']):.4g}"),
             "walkers_per_second": float(f"{B / (np.mean(ts['step']) * 1e-3):.4g}"),
             "measured": {"n": res["n"], "n_skipped": res["n_skipped"], "steps": int(counter.item()), "overlap": [float(f"{v:.5g}") for v in res["overlap"]],
                          "stderr": [float(f"{v:.3g}") for v in res["stderr"]]}}
        assert res["n"] + res["n_skipped"] == int(counter.item()) * B and res["n"] > 0
        print(json.dumps(r), flush=True)
        del launch, acc
        torch.cuda.empty_cache()

    # ---- the model-free kernels alone
    K = 2
    psi = torch.randn(B, device="cuda")
    rows = torch.randn(K, B, device="cuda")
    e = torch.randn(B, device="cuda")
    acc = overlap.Accumulator(K, "cuda")
    ratios = torch.empty_like(rows)
    ws = model._workspace(overlap.lib().wf_overlap_workspace_bytes(B, K), "cuda")
    out = torch.empty_like(e)

    def accumulate_steps(n):
        for _ in range(n):
            overlap.accumulate(psi, rows, acc=acc, ratios=ratios, workspace=ws)

    def penalise_steps(n):
        for _ in range(n):
            overlap.penalise(e, ratios, acc, 0.5, out=out)
    ts, warm = run({"accumulate": accumulate_steps, "penalise": penalise_steps}, window)
    print(json.dumps({"what": "kernels", "batch": B, "K": K, "accumulate_ms": stats(ts["accumulate"]), "penalise_ms": stats(ts["penalise"]),
                      "accumulate_bytes_per_second": float(f"{(1 + 2 * K) * 4 * B / (np.mean(ts['accumulate']) * 1e-3):.4g}")}),   # psi, K rows in, K rows out
          flush=True)

    # ---- an eager SPRING step: plain, and penalised against K lower states
    protons, _ = physics.system_catalogue[1]["He"]
    params, psi_fn = states[0]
    h_fn = physics.construct_hamiltonian_function(psi_fn, protons=protons, n_space_dimensions=1, eps=0.0)
    x = model.sample(SEED, a.train_batch, exact=True)
    prev = torch.zeros(model.n_params, device="cuda")
    lower = [(s[1], s[0]) for s in states[1:]]
    record = []

    def spring(K):
        def steps(n):
            for _ in range(n):
                vqmc.train_step_spring(1, psi_fn, h_fn, params, x, 0.1, prev, 0.9, 0.1, 5.0, relative_damping=1e-2, lower_states=lower[:K], overlap_penalty=1.0,
                                       overlap_record=record if K else None)
        return steps
    ts, warm = run({"plain": spring(0), "K1": spring(1), "K2": spring(2)}, wall)
    print(json.dumps({"what": "eager_spring_step", "model": "He", "batch": a.train_batch, "repeats": a.repeats, "steps_per_window": a.steps, "warmup_steps": warm,
                      "plain_ms": stats(ts["plain"]), "K1_ms": stats(ts["K1"]), "K2_ms": stats(ts["K2"]),
                      "K1_over_plain": float(f"{np.mean(ts['K1']) / np.mean(ts['plain']):.4g}"),
                      "K2_over_plain": float(f"{np.mean(ts['K2']) / np.mean(ts['plain']):.4g}"), "last_overlaps": [float(f"{v:.5g}") for v in record[-1]]}), flush=True)


if __name__ == "__main__":
    main()
