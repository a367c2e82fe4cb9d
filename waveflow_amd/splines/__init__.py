"""waveflow.splines call surface on the HIP path: ISpline_fun, MSpline_fun, BSpline_fun (splines/isplines_jax.py, msplines_jax.py,
bsplines_jax.py).  Same init_fun keywords, defaults and return tuples as the reference; the closures take numpy arrays or torch.cuda
tensors shaped as the reference's vmap(in_axes=(0, 0)) (params [N, nc], x [N]) and return torch.cuda float32 tensors on torch's current
stream.  The device work runs in wf_spline_* (include/waveflow_hip.h, wf_kernels_spline.hip)."""
from .bsplines_jax import BSpline_fun  # noqa: F401
from .isplines_jax import ISpline_fun  # noqa: F401
from .msplines_jax import MSpline_fun  # noqa: F401
