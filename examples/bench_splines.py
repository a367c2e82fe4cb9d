"""Timer of the spline closures' device entry points (wf_spline_*): hipEvents around each launch, 10 warm-up launches, >= 50 timed ones;
median and minimum, and bytes/s from the bytes the shapes imply (coefficients + inputs read, outputs written; the L2-resident tables are
not counted).  Prints one JSON line per shape.

    python examples/bench_splines.py [--iters 50] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveflow_amd.splines import BSpline_fun, ISpline_fun, MSpline_fun  # noqa: E402


def timed(fn, iters, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_splines.py needs a GPU"
    root = tempfile.mkdtemp()
    g = torch.Generator(device="cuda").manual_seed(0)
    lines = []

    def report(name, us, us_min, nbytes, **kw):
        r = {"shape": name, "median_us": round(us, 2), "min_us": round(us_min, 2), "bytes": nbytes,
             "TB_per_s_median": round(nbytes / us * 1e-6, 3), "TB_per_s_best": round(nbytes / us_min * 1e-6, 3), **kw}
        print(json.dumps(r), flush=True)
        lines.append(r)

    N = 1 << 22
    for kind, fun in (("I", ISpline_fun), ("B", BSpline_fun)):
        kw = {"zero_border": False} if kind == "I" else {}
        out = fun()(0, 6, 23, cached_bases_path_root=os.path.join(root, kind), **kw)
        dev = out[1].spline
        c = torch.rand((N, dev.nc), device="cuda", generator=g)
        c = c / c.sum(1, keepdim=True)
        x = torch.rand(N, device="cuda", generator=g)
        dev.apply(c[:1], x[:1])   # the handle
        y, dy = torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
        import ctypes
        h, L, st = dev.handle(), dev._L, dev._stream()
        fn = lambda: L.wf_spline_apply(h, c.data_ptr(), N, x.data_ptr(), 0, y.data_ptr(), dy.data_ptr(), st)
        med, mn = timed(fn, a.iters)
        report(f"apply+grad {kind} k=6 23 knots nb={dev.nb} N=2^22", med, mn, N * (dev.nc + 1 + 2) * 4)
        if kind == "I":
            M = 1 << 20
            yy = torch.rand(M, device="cuda", generator=g)
            xo = torch.empty(M, device="cuda")
            fn = lambda: L.wf_spline_reverse(h, c.data_ptr(), M, yy.data_ptr(), ctypes.c_float(1e-3), xo.data_ptr(), st)
            med, mn = timed(fn, a.iters)
            report(f"reverse I k=6 23 knots tol=1e-3 N=2^20", med, mn, M * (dev.nc + 2) * 4)
    for kind, fun in (("M", MSpline_fun), ("B", BSpline_fun)):
        out = fun()(0, 6, 23, cached_bases_path_root=os.path.join(root, "s" + kind))
        dev = out[1].spline
        rows, ns = 1 << 10, 1 << 10
        c = out[5](torch.rand((rows, dev.nc), device="cuda", generator=g) * (2 if kind == "M" else 1) - (0 if kind == "M" else 0.5))
        xs = torch.empty((rows, ns), device="cuda")
        h, L, st = dev.handle(), dev._L, dev._stream()
        fn = lambda: L.wf_spline_sample(h, 7, c.data_ptr(), rows, ns, 100000, xs.data_ptr(), st)
        med, mn = timed(fn, a.iters)
        assert bool(torch.isfinite(xs).all())
        report(f"sample {kind} k=6 23 knots 2^10 rows x 2^10 draws", med, mn, rows * ns * 4 + rows * dev.nc * 4,
               draws_per_s=round(rows * ns / med * 1e6, 1))
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
