"""Host-side handle on a wf_model (include/waveflow_hip.h) plus pytree helpers.

PyTorch is used only as plumbing: device buffers, the current HIP stream, torch.distributed.
"""
import ctypes
import os

import numpy as np

from . import _lib


def tree_leaves(tree, out=None):
    """Leaves in JAX pytree order for nested tuples / lists (depth first, left to right)."""
    if out is None:
        out = []
    if isinstance(tree, (tuple, list)):
        for t in tree:
            tree_leaves(t, out)
    elif tree is not None:
        out.append(tree)
    return out


class DeviceParams:
    """Parameters that live on the GPU: the flat float32 vector (reference leaf order) plus the pytree they unflatten to.
    Accepted wherever the closures take `params`; `tree()` downloads them as the reference's pytree of numpy arrays."""

    def __init__(self, template, flat, version=0):
        self.template, self.flat, self.version = template, flat, version

    def tree(self):
        from .checkpoint import unflatten_like
        return unflatten_like(self.template, self.flat.detach().cpu().numpy())


def flatten_params(tree):
    """-> contiguous float32 host vector in leaf order."""
    if isinstance(tree, DeviceParams):
        return np.ascontiguousarray(tree.flat.detach().cpu().numpy(), dtype=np.float32)
    leaves = tree_leaves(tree)
    parts = []
    for a in leaves:
        if hasattr(a, "detach"):  # torch tensor
            a = a.detach().to("cpu").numpy()
        parts.append(np.asarray(a, dtype=np.float32).reshape(-1))
    if not parts:
        return np.zeros(0, np.float32)
    return np.ascontiguousarray(np.concatenate(parts))


def unflatten_batched(template, jac):
    """[B, n_params] (numpy or torch, leaf order) -> the pytree of `template` with a leading batch axis on every leaf: what
    jax.jacrev(f, argnums=0)(params, batch) returns for a per-walker f (vqmc.py:179).  Leaves are views of `jac`."""
    if isinstance(template, DeviceParams):
        template = template.template
    if jac.ndim != 2:
        raise ValueError(f"expected a [B, n_params] array, got shape {tuple(jac.shape)}")
    B, n = int(jac.shape[0]), int(jac.shape[1])
    pos = [0]

    def rec(t):
        if isinstance(t, tuple):
            return tuple(rec(q) for q in t)
        if isinstance(t, list):
            return [rec(q) for q in t]
        if t is None:
            return None
        shape = tuple(np.shape(t))
        size = int(np.prod(shape, dtype=np.int64))
        out = jac[:, pos[0]:pos[0] + size].reshape((B,) + shape)
        pos[0] += size
        return out

    tree = rec(template)
    if pos[0] != n:
        raise ValueError(f"rows have {n} values, template needs {pos[0]}")
    return tree


def check_jacobian_bytes(B, n_params, free_bytes):
    """A [B, n_params] float32 Jacobian must fit the free device memory: the library never spills it to the host behind the caller's back."""
    need = int(B) * int(n_params) * 4
    if need > int(free_bytes):
        raise ValueError(f"a [{int(B)}, {int(n_params)}] float32 Jacobian needs {need} bytes, {int(free_bytes)} bytes of device memory are free: "
                         "pass the walkers in smaller batches")
    return need


def _torch():
    import torch
    return torch


class DeviceModel:
    """Owns one wf_model on one GPU."""

    def __init__(self, desc, device=None):
        torch = _torch()
        if not torch.cuda.is_available():
            raise _lib.WfError(_lib.ERR_NO_DEVICE, "wf_model_create")
        if device is None:
            device = torch.cuda.current_device()
        self.device = int(device)
        self.desc = desc
        h = ctypes.c_void_p()
        _lib.call("wf_model_create", ctypes.byref(desc), self.device, ctypes.byref(h))
        self._h = h
        self.n_params = int(_lib.call("wf_model_param_count", h))
        self.i_nb = int(_lib.call("wf_model_n_bases", h, 0))
        self.p_nb = int(_lib.call("wf_model_n_bases", h, 1))
        self._vjp_ws = None
        self._invalidate_host_copy()
        self.D = int(desc.n_dim)
        self.n_layers = int(desc.n_flow_layers)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                _lib.lib().wf_model_destroy(h)
            except Exception:
                pass
            self._h = None

    # ---- parameters
    def set_params(self, flat):
        flat = np.ascontiguousarray(flat, dtype=np.float32).reshape(-1)
        if flat.size != self.n_params:
            raise ValueError(f"expected {self.n_params} parameters, got {flat.size}")
        self._run("wf_model_set_params", flat.ctypes.data, flat.size)
        self._flat = flat.copy()

    def set_params_device(self, flat_dev):
        """Parameters from a float32 cuda vector: asynchronous, no host copy (wf_model_set_params_device)."""
        if flat_dev.numel() != self.n_params or str(flat_dev.dtype) != "torch.float32" or not flat_dev.is_cuda:
            raise ValueError(f"expected a float32 cuda vector of {self.n_params} parameters")
        flat_dev = flat_dev.contiguous()
        self._run("wf_model_set_params_device", self._p(flat_dev), flat_dev.numel())
        self._flat = None

    def ensure_params(self, tree):
        """Upload `tree` unless it equals what the device already holds."""
        if isinstance(tree, DeviceParams):
            key = (id(tree.flat), tree.version)
            if self._dev_key != key:
                self.set_params_device(tree.flat)
                self._dev_key = key
            return
        self._dev_key = None
        flat = flatten_params(tree)
        if self._flat is None or flat.size != self._flat.size or not np.array_equal(flat, self._flat):
            self.set_params(flat)

    def _invalidate_host_copy(self):
        """The device parameters are no longer what set_params / ensure_params last uploaded (a training step moved them)."""
        self._flat = None
        self._dev_key = None

    def set_kernel(self, kind):
        kind = {"auto": _lib.KERNEL_AUTO, "scalar": _lib.KERNEL_SCALAR, "mfma": _lib.KERNEL_MFMA, "wave": _lib.KERNEL_WAVE}.get(kind, kind)
        _lib.call("wf_model_set_kernel", self._h, int(kind))

    # ---- plumbing
    def _stream(self):
        return _lib.stream_ptr(self.device)

    def _run(self, name, *args):
        """wf_<name>(model, args..., stream), checked."""
        return _lib.call(name, self._h, *args, self._stream())

    def _to_dev(self, x):
        """-> (float32 contiguous cuda tensor [B, D], converter for outputs)"""
        torch = _torch()
        was_numpy = not hasattr(x, "detach")
        t = torch.as_tensor(np.asarray(x, dtype=np.float32)) if was_numpy else x
        squeeze = t.dim() == 1  # wavefunctions.py:35-36 promotes a single walker to [1, D]
        if squeeze:
            t = t[None]
        if t.dim() != 2 or t.shape[1] != self.D:
            raise ValueError(f"expected inputs of shape [B, {self.D}], got {tuple(t.shape)}")
        t = t.to(device=f"cuda:{self.device}", dtype=torch.float32).contiguous()
        back = (lambda o: o.cpu().numpy()) if was_numpy else (lambda o: o)
        return t, back

    def _new(self, shape, dtype=None):
        torch = _torch()
        return torch.empty(shape, device=f"cuda:{self.device}", dtype=dtype or torch.float32)

    _p = staticmethod(_lib.ptr)

    @staticmethod
    def _pick(back, *outs):
        """The outputs that were asked for (the others are None), converted: one value, or a tuple of them."""
        res = [back(o) for o in outs if o is not None]
        return res[0] if len(res) == 1 else tuple(res)

    @staticmethod
    def _protons(protons):
        """1-D proton positions -> (float32 host pointer or None, n); the pointer object keeps its array alive."""
        pr = np.ascontiguousarray(np.asarray(protons, dtype=np.float32).reshape(-1))
        return (pr.ctypes.data_as(ctypes.c_void_p) if pr.size else None), pr.size

    @staticmethod
    def _weights(w, B, device, message):
        """A per-walker weight as a float32 cuda vector of B entries, or ValueError(message)."""
        torch = _torch()
        t = torch.as_tensor(w, dtype=torch.float32).to(device).contiguous()
        if t.numel() != B:
            raise ValueError(message)
        return t

    @staticmethod
    def _workspace(nbytes, device):
        torch = _torch()
        ws = torch.empty(int(nbytes), device=device, dtype=torch.uint8)
        if os.environ.get("WF_POISON"):
            ws.fill_(0xFF)   # NaN patterns: see dev_alloc_bytes in wf_runtime.cpp
        return ws

    def _grad_ws(self, entry, B, device):
        """-> (pointer, bytes) of the one workspace all gradient and Jacobian entries share, holding at least what `entry`
        (a *_workspace_bytes function) asks for B walkers: grown when it is too small, never shrunk."""
        nbytes = _lib.call(entry, self._h, B)
        if self._vjp_ws is None or self._vjp_ws.numel() < nbytes:
            self._vjp_ws = self._workspace(nbytes, device)
        return self._p(self._vjp_ws), self._vjp_ws.numel()

    def _train_ws(self, st, nbytes):
        """-> (pointer, bytes) of the train state's workspace, allocated here unless the caller did (before a capture)."""
        if st.get("ws") is None or st["ws"].numel() < nbytes:
            st["ws"] = self._workspace(nbytes, st["x"].device)
        return self._p(st["ws"]), st["ws"].numel()

    # ---- hot path
    def _eval(self, name, x, return_sample, return_bin_idx):
        torch = _torch()
        t, back = self._to_dev(x)
        B = t.shape[0]
        out = self._new((B,))
        u = self._new((B, self.D)) if return_sample else None
        idx = self._new((B, self.n_layers + 1, self.D, 2), torch.int32) if return_bin_idx else None
        if idx is not None:
            idx.zero_()
        self._run(name, self._p(t), B, self._p(out), self._p(u), self._p(idx))
        return self._pick(back, out, u, idx)

    def log_pdf(self, x, return_sample=False, return_bin_idx=False):
        return self._eval("wf_logpdf_fwd", x, return_sample, return_bin_idx)

    def psi(self, x, return_sample=False, return_bin_idx=False):
        return self._eval("wf_psi_fwd", x, return_sample, return_bin_idx)

    def psi_antisym(self, x, return_inversions=False):
        """psi(sort(x)) * (-1)^inversions(x) for walkers in any particle order (helpers.py:55-58, coordinates.py:41-51): sort and sign on the device."""
        torch = _torch()
        t, back = self._to_dev(x)
        B = t.shape[0]
        out = self._new((B,))
        inv = self._new((B,), torch.int32) if return_inversions else None
        self._run("wf_psi_antisym_fwd", self._p(t), B, self._p(out), self._p(inv))
        return self._pick(back, out, inv)

    def log_pdf_unsorted(self, x):
        """log_pdf(sort(x)): rows in any particle order, sorted on the device."""
        t, back = self._to_dev(x)
        B = t.shape[0]
        out = self._new((B,))
        self._run("wf_logpdf_unsorted_fwd", self._p(t), B, self._p(out))
        return back(out)

    def flow(self, x):
        t, back = self._to_dev(x)
        B = t.shape[0]
        u, ld = self._new((B, self.D)), self._new((B,))
        self._run("wf_flow_fwd", self._p(t), B, self._p(u), self._p(ld))
        return back(u), back(ld)

    def layer(self, l, u_in, return_bin_idx=False):
        torch = _torch()
        t, back = self._to_dev(u_in)
        B = t.shape[0]
        y, ld = self._new((B, self.D)), self._new((B,))
        idx = self._new((B, self.D, 2), torch.int32) if return_bin_idx else None
        if idx is not None:
            idx.zero_()
        self._run("wf_layer_fwd", int(l), self._p(t), B, self._p(y), self._p(ld), self._p(idx))
        return self._pick(back, y, ld, idx)

    def inverse(self, u, exact=False):
        """Serial.inverse_fun; exact=False reproduces the reference's IMADE.inverse_fun (conditioner on its inputs)."""
        t, back = self._to_dev(u)
        B = t.shape[0]
        x = self._new((B, self.D))
        self._run("wf_inverse_fwd", self._p(t), B, self._p(x), int(bool(exact)))
        return back(x)

    def sample(self, seed, num_samples, return_latent=False, exact=False):
        """-> x [n, D] on the device (and the prior-space samples when return_latent)."""
        B = int(num_samples)
        x = self._new((B, self.D))
        lat = self._new((B, self.D)) if return_latent else None
        self._run("wf_sample", ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), B, self._p(x), self._p(lat), int(bool(exact)))
        return (x, lat) if return_latent else x

    def hamiltonian(self, x, protons, return_psi=False, return_laplacian=False):
        """H psi = -1/2 laplacian(psi) + V psi (physics.construct_hamiltonian_function); protons: 1-D positions."""
        t, back = self._to_dev(x)
        B = t.shape[0]
        h = self._new((B,))
        ps = self._new((B,)) if return_psi else None
        lap = self._new((B,)) if return_laplacian else None
        self._run("wf_hamiltonian_fwd", self._p(t), B, *self._protons(protons), self._p(h), self._p(ps), self._p(lap))
        return self._pick(back, h, ps, lap)

    def psi_derivatives(self, x, hessian_diag=False, return_psi=False):
        """d psi / d x_d -> [B, D] (jax.grad(psi, 1)); with hessian_diag also d^2 psi / d x_d^2 -> [B, D] (the diagonal of jax.hessian(psi, 1),
        whose row sums are the Laplacian of `hamiltonian`).  Returns grad, or (grad[, hdiag][, psi]); sorted walkers, numpy or torch like `hamiltonian`."""
        t, back = self._to_dev(x)
        B = t.shape[0]
        grad = self._new((B, self.D))
        hd = self._new((B, self.D)) if hessian_diag else None
        ps = self._new((B,)) if return_psi else None
        self._run("wf_psi_coord_derivs", self._p(t), B, self._p(ps), self._p(grad), self._p(hd))
        return self._pick(back, grad, hd, ps)

    def psi_vjp(self, x, w_psi, w_lap):
        """grad[p] = sum_b (w_psi[b] d psi_b/d theta_p + w_lap[b] d laplacian_b/d theta_p) -> torch.cuda float32 [n_params]."""
        t, _ = self._to_dev(x)
        B = t.shape[0]
        wp = self._weights(w_psi, B, t.device, "w_psi / w_lap must have one entry per walker")
        wl = self._weights(w_lap, B, t.device, "w_psi / w_lap must have one entry per walker")
        ws = self._grad_ws("wf_psi_vjp_workspace_bytes", B, t.device)
        grad = self._new((self.n_params,))
        self._run("wf_psi_vjp", self._p(t), B, self._p(wp), self._p(wl), self._p(grad), *ws)
        return grad

    def logpdf_vjp(self, x, w):
        """grad[p] = sum_b w[b] d log_pdf_b / d theta_p -> torch.cuda float32 [n_params]."""
        t, _ = self._to_dev(x)
        B = t.shape[0]
        wt = self._weights(w, B, t.device, "w must have one entry per row of x")
        ws = self._grad_ws("wf_logpdf_vjp_workspace_bytes", B, t.device)
        grad = self._new((self.n_params,))
        self._run("wf_logpdf_vjp", self._p(t), B, self._p(wt), self._p(grad), *ws)
        return grad

    def _jac_rows(self, x):
        """-> (x on the device, empty [B, n_params] float32 cuda); ValueError if the rows do not fit the free device memory."""
        torch = _torch()
        shape = tuple(np.shape(x))
        if len(shape) == 2:   # before anything is uploaded
            dev = f"cuda:{self.device}"
            free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
            check_jacobian_bytes(shape[0], self.n_params, free)
        t, _ = self._to_dev(x)
        return t, self._new((t.shape[0], self.n_params))

    def logpdf_jacobian(self, x, return_logp=False):
        """jac[b, p] = d log_pdf_b / d theta_p -> torch.cuda float32 [B, n_params] (jax.jacrev(log_pdf, argnums=0)(params, batch), vqmc.py:179, in
        flat leaf order: core.unflatten_batched gives the pytree); with return_logp also log_pdf [B] of the same sweep."""
        t, jac = self._jac_rows(x)
        B = t.shape[0]
        ws = self._grad_ws("wf_logpdf_jac_workspace_bytes", B, t.device)
        lp = self._new((B,)) if return_logp else None
        self._run("wf_logpdf_jac", self._p(t), B, self._p(jac), self._p(lp), *ws)
        return (jac, lp) if return_logp else jac

    def psi_jacobian(self, x, w_psi=None, w_lap=None):
        """jac[b, p] = w_psi[b] d psi_b / d theta_p + w_lap[b] d laplacian_b / d theta_p -> torch.cuda float32 [B, n_params]: the rows whose sum
        is psi_vjp.  Defaults w_psi = 1, w_lap = 0: jax.jacrev(psi, argnums=0)(params, batch)."""
        torch = _torch()
        t, jac = self._jac_rows(x)
        B = t.shape[0]
        message = "w_psi / w_lap must have one entry per walker"
        wp = torch.ones(B, dtype=torch.float32, device=t.device) if w_psi is None else self._weights(w_psi, B, t.device, message)
        wl = None if w_lap is None else self._weights(w_lap, B, t.device, message)
        ws = self._grad_ws("wf_psi_jac_workspace_bytes", B, t.device)
        self._run("wf_psi_jac", self._p(t), B, self._p(wp), self._p(wl), self._p(jac), *ws)
        return jac

    def logpdf_loss_grad(self, x, weight):
        """(log_pdf [B], weight * sum_b d log_pdf_b / d theta [n_params]) from one forward and one reverse sweep."""
        t, _ = self._to_dev(x)
        B = t.shape[0]
        ws = self._grad_ws("wf_logpdf_vjp_workspace_bytes", B, t.device)
        lp, grad = self._new((B,)), self._new((self.n_params,))
        self._run("wf_logpdf_loss_grad", self._p(t), B, float(weight), self._p(lp), self._p(grad), *ws)
        return lp, grad

    def vqmc_loss_grad(self, x, protons, running_average, global_count=None):
        """loss_fn_efficient and its gradient (vqmc.py:193-221) for the walkers x on this device, one fused pass.
        -> (sums fp64 [sum E_L, sum E_L^2, count] (torch.cuda), grad float32 [n_params] scaled by 1/global_count)."""
        t, _ = self._to_dev(x)
        B = t.shape[0]
        ws = self._grad_ws("wf_psi_vjp_workspace_bytes", B, t.device)
        el, grad = self._new((B,)), self._new((self.n_params,))
        inv = 1.0 / float(global_count if global_count else max(B, 1))
        self._run("wf_vqmc_loss_grad", self._p(t), B, *self._protons(protons), float(running_average), inv, self._p(el), self._p(grad), *ws)
        return self.block_sums(el), grad

    def adam_step(self, x, g, m, v, step, step_size, b1=0.9, b2=0.999, eps=1e-8):
        """In-place Adam update of the cuda vectors x, m, v with the gradient g (wf_adam_step)."""
        for t in (x, g, m, v):
            if not t.is_cuda or not t.is_contiguous() or t.numel() != x.numel() or str(t.dtype) != "torch.float32":
                raise ValueError("adam_step needs contiguous float32 cuda vectors of equal length")
        _lib.call("wf_adam_step", self._p(x), self._p(g), self._p(m), self._p(v), x.numel(), int(step), float(step_size), float(b1),
                  float(b2), float(eps), self._stream())

    def make_train_state(self, x, m, v, first_step, ring_len=128, defer_eval_tables=False):
        """Device-side state of wf_vqmc_train_step around the Adam vectors x, m, v (float32 cuda, updated in place).
        defer_eval_tables: the steps skip the tables only the large-batch evaluation kernel reads; the caller refreshes them with
        set_params_device(x) before evaluating (ensure_params does so for a DeviceParams of a new version)."""
        torch = _torch()
        dev = x.device
        st = {"x": x, "m": m, "v": v, "ring_len": int(ring_len),
              "counter": torch.tensor([int(first_step)], dtype=torch.int64, device=dev),
              "running_average": torch.zeros(1, dtype=torch.float32, device=dev),
              "ring": torch.zeros(int(ring_len), 3, dtype=torch.float64, device=dev)}
        st["c"] = _lib.TrainState(x.data_ptr(), m.data_ptr(), v.data_ptr(), st["counter"].data_ptr(), st["running_average"].data_ptr(),
                                  st["ring"].data_ptr(), int(ring_len), int(bool(defer_eval_tables)))
        return st

    def train_step_workspace_bytes(self, batch):
        """Workspace of train_step / train_step_local for `batch` walkers per step; WfError where the library has no fused step for them."""
        return _lib.call("wf_vqmc_train_step_workspace_bytes", self._h, int(batch))

    def mle_train_step_workspace_bytes(self, n):
        """Workspace of mle_train_step for n resident rows."""
        return _lib.call("wf_mle_train_step_workspace_bytes", self._h, int(n))

    def train_step(self, st, seed, batch, protons, step_size, b1=0.9, b2=0.999, eps=1e-8, exact_sampler=False):
        """One whole training step on the device (wf_vqmc_train_step): no host work, capturable in a hipGraph."""
        ws = self._train_ws(st, self.train_step_workspace_bytes(batch))
        self._run("wf_vqmc_train_step", ctypes.byref(st["c"]), int(seed), int(batch), *self._protons(protons), float(step_size), float(b1),
                  float(b2), float(eps), int(bool(exact_sampler)), *ws)
        self._invalidate_host_copy()

    def train_step_local(self, st, seed, batch_local, protons, inv_global_batch, red, exact_sampler=False):
        """First half of a sharded training step (wf_vqmc_train_step_local): this rank's walkers -> red[n_params + 3] (float64 cuda)
        = [gradient contribution, sum E_L, sum E_L^2, local walkers]; the caller all-reduces red and calls train_step_apply."""
        ws = self._train_ws(st, self.train_step_workspace_bytes(batch_local))
        if str(red.dtype) != "torch.float64" or red.numel() != self.n_params + 3 or not red.is_cuda or not red.is_contiguous():
            raise ValueError("red must be a contiguous float64 cuda vector of n_params + 3 entries")
        self._run("wf_vqmc_train_step_local", ctypes.byref(st["c"]), int(seed), int(batch_local), *self._protons(protons), float(inv_global_batch),
                  int(bool(exact_sampler)), self._p(red), *ws)

    def train_step_apply(self, st, red, step_size, b1=0.9, b2=0.999, eps=1e-8):
        """Second half (wf_vqmc_train_step_apply): Adam with the reduced gradient, image refill, loss ring, counter."""
        self._run("wf_vqmc_train_step_apply", ctypes.byref(st["c"]), self._p(red), float(step_size), float(b1), float(b2), float(eps))
        self._invalidate_host_copy()

    def mle_train_step(self, st, x, step_size, b1=0.9, b2=0.999, eps=1e-8):
        """One maximum-likelihood epoch on the device (wf_mle_train_step): no host work, capturable in a hipGraph."""
        n = int(x.shape[0])
        ws = self._train_ws(st, self.mle_train_step_workspace_bytes(n))
        self._run("wf_mle_train_step", ctypes.byref(st["c"]), self._p(x), n, float(step_size), float(b1), float(b2), float(eps), *ws)
        self._invalidate_host_copy()

    # ---- stochastic reconfiguration as a whole step on the device (include/waveflow_sr_step.h)
    def make_sr_train_state(self, x, first_step, learning_rate, ring_len=128, defer_eval_tables=False):
        """Device-side state of wf_vqmc_sr_step around the parameter vector x (float32 cuda, updated in place): the step counter, the learning
        rate ("step_size": one float32 on the device, rewritten between steps or graph replays with .fill_), the loss ring [ring_len, 3], the
        ring of |d|^2 ("norm_ring") and "status" = [the solver's info of the last step, steps skipped so far]."""
        torch = _torch()
        from . import sr
        if not x.is_cuda or str(x.dtype) != "torch.float32" or not x.is_contiguous() or x.numel() != self.n_params:
            raise ValueError(f"expected a contiguous float32 cuda vector of {self.n_params} parameters")
        if int(ring_len) < 1:
            raise ValueError("ring_len must be >= 1")
        dev = x.device
        st = {"x": x, "ring_len": int(ring_len),
              "counter": torch.tensor([int(first_step)], dtype=torch.int64, device=dev),
              "step_size": torch.tensor([float(learning_rate)], dtype=torch.float32, device=dev),
              "ring": torch.zeros(int(ring_len), 3, dtype=torch.float64, device=dev),
              "norm_ring": torch.zeros(int(ring_len), dtype=torch.float64, device=dev),
              "status": torch.zeros(2, dtype=torch.int32, device=dev)}
        st["c"] = sr.SrTrainState(x.data_ptr(), st["counter"].data_ptr(), st["step_size"].data_ptr(), st["ring"].data_ptr(),
                                  st["norm_ring"].data_ptr(), st["status"].data_ptr(), int(ring_len), int(bool(defer_eval_tables)))
        return st

    def sr_step_workspace_bytes(self, batch):
        """Workspace of sr_step for `batch` walkers per step; WfError where the library has no such step for this model or batch."""
        from . import sr
        return _lib.check(sr.lib().wf_vqmc_sr_step_workspace_bytes(self._h, int(batch)), "wf_vqmc_sr_step_workspace_bytes")

    def sr_step(self, st, seed, batch, protons, damping=0.0, relative_damping=1e-3, exact_sampler=False, walkers=None, out_walkers=None):
        """One whole stochastic-reconfiguration step on the device (wf_vqmc_sr_step): no host work, no wait, capturable in a hipGraph.
        The step draws its walkers (out_walkers [batch, D], if given, receives them) or reads them from `walkers` [batch, D]; the learning
        rate is st["step_size"].  Arguments are checked before anything is launched (ValueError)."""
        from . import sr
        damping, relative_damping = sr._check_step(batch, self.D, damping, relative_damping, walkers, out_walkers)
        ws = self._train_ws(st, self.sr_step_workspace_bytes(batch))
        x = walkers if walkers is not None else out_walkers
        _lib.check(sr.lib().wf_vqmc_sr_step(self._h, ctypes.byref(st["c"]), int(seed) & 0xFFFFFFFFFFFFFFFF, int(batch), *self._protons(protons),
                                            damping, relative_damping, int(bool(exact_sampler)), self._p(x), int(walkers is None), *ws,
                                            self._stream()), "wf_vqmc_sr_step")
        self._invalidate_host_copy()

    # ---- the SPRING optimiser as a whole step on the device (include/waveflow_sr_spring.h)
    def make_spring_train_state(self, x, first_step, learning_rate, ring_len=128, defer_eval_tables=False, phi=None):
        """Device-side state of wf_vqmc_spring_step: that of make_sr_train_state, plus "phi" (the previous direction: float32 cuda [n_params],
        zeros unless given; updated in place) and "eff_ring" (the step size each step applied after the norm cap; 0 for a skipped step)."""
        torch = _torch()
        from . import sr
        st = self.make_sr_train_state(x, first_step, learning_rate, ring_len=ring_len, defer_eval_tables=defer_eval_tables)
        if phi is None:
            phi = torch.zeros(self.n_params, dtype=torch.float32, device=x.device)
        elif not phi.is_cuda or phi.device != x.device or str(phi.dtype) != "torch.float32" or not phi.is_contiguous() or phi.numel() != self.n_params:
            raise ValueError(f"phi must be a contiguous float32 cuda vector of {self.n_params} entries on the device of the parameters")
        st["phi"] = phi
        st["eff_ring"] = torch.zeros(int(ring_len), dtype=torch.float64, device=x.device)
        st["c"] = sr.SpringTrainState(x.data_ptr(), st["counter"].data_ptr(), st["step_size"].data_ptr(), st["ring"].data_ptr(),
                                      st["norm_ring"].data_ptr(), st["status"].data_ptr(), int(ring_len), int(bool(defer_eval_tables)),
                                      phi.data_ptr(), st["eff_ring"].data_ptr())
        return st

    def spring_step_workspace_bytes(self, batch):
        """Workspace of spring_step for `batch` walkers per step; WfError where the library has no such step for this model or batch."""
        from . import sr
        return _lib.check(sr.lib().wf_vqmc_spring_step_workspace_bytes(self._h, int(batch)), "wf_vqmc_spring_step_workspace_bytes")

    def spring_step(self, st, seed, batch, protons, damping=0.0, relative_damping=1e-3, momentum=0.0, norm_constraint=0.0, clip=0.0,
                    exact_sampler=False, walkers=None, out_walkers=None):
        """One whole SPRING step on the device (wf_vqmc_spring_step): sr_step with momentum (st["phi"]), the step capped at
        sqrt(norm_constraint) in norm (0: no cap) and local energies clamped `clip` mean absolute deviations around their median (0: not clamped).
        No host work, no wait, capturable in a hipGraph.  Arguments are checked before anything is launched (ValueError)."""
        from . import sr
        damping, relative_damping = sr._check_step(batch, self.D, damping, relative_damping, walkers, out_walkers)
        momentum, norm_constraint, clip = sr._check_spring(momentum, norm_constraint, clip)
        ws = self._train_ws(st, self.spring_step_workspace_bytes(batch))
        x = walkers if walkers is not None else out_walkers
        _lib.check(sr.lib().wf_vqmc_spring_step(self._h, ctypes.byref(st["c"]), int(seed) & 0xFFFFFFFFFFFFFFFF, int(batch), *self._protons(protons),
                                                damping, relative_damping, momentum, norm_constraint, clip, int(bool(exact_sampler)), self._p(x),
                                                int(walkers is None), *ws, self._stream()), "wf_vqmc_spring_step")
        self._invalidate_host_copy()

    # ---- one measurement step on the device (include/waveflow_observe.h; observables.measure drives it)
    def observe_step_workspace_bytes(self, batch):
        """Workspace of observe_step for `batch` walkers per step; WfError where the library has no such step for this model or batch."""
        from . import observables
        return _lib.check(observables.lib().wf_vqmc_observe_step_workspace_bytes(self._h, int(batch)), "wf_vqmc_observe_step_workspace_bytes")

    def observe_step(self, acc, counter, seed, batch, protons, exact_sampler=False, walkers=None, out_walkers=None, values=None):
        """One measurement step on the device (wf_vqmc_observe_step): no host work, no wait, capturable in a hipGraph after one call outside the
        capture.  The step draws its walkers (stream `seed` advanced by `counter`, one int64 on the device, + 1 at the end; out_walkers [batch, D],
        if given, receives them) or reads them from `walkers` [batch, D]; it adds them to `acc` (an observables.Accumulator; None with `values`)
        and writes the per-walker values to `values` [batch, 5] if given.  Nothing of the model changes.  Arguments are checked before anything
        is launched (ValueError)."""
        from . import observables
        batch = observables._check_step(batch, self.D, walkers, out_walkers, values)
        if acc is None and values is None:
            raise ValueError("nothing to do: neither an accumulator nor values")
        if acc is not None and acc.D != self.D:
            raise ValueError(f"the accumulator holds {acc.D} columns, the model has {self.D}")
        if not hasattr(counter, "is_cuda") or counter.numel() != 1 or str(counter.dtype) != "torch.int64" or not counter.is_cuda:
            raise ValueError("counter must be one int64 on the device (no CPU fallback)")
        st = acc.st if acc is not None else {"x": counter, "ws": None}
        ws = self._train_ws(st, self.observe_step_workspace_bytes(batch))
        x = walkers if walkers is not None else out_walkers
        _lib.check(observables.lib().wf_vqmc_observe_step(self._h, ctypes.byref(acc.c) if acc is not None else None, self._p(counter),
                                                          int(seed) & 0xFFFFFFFFFFFFFFFF, batch, *self._protons(protons), int(bool(exact_sampler)),
                                                          self._p(x), int(walkers is None), self._p(values), *ws, self._stream()),
                   "wf_vqmc_observe_step")

    # ---- one overlap measurement step on the device (include/waveflow_overlap.h; overlap.measure drives it)
    def overlap_step_workspace_bytes(self, batch, K):
        """Workspace of overlap_step for `batch` walkers per step and K reference models; WfError where the library has no such step."""
        from . import overlap
        return _lib.check(overlap.lib().wf_vqmc_overlap_step_workspace_bytes(self._h, int(batch), int(K)), "wf_vqmc_overlap_step_workspace_bytes")

    def overlap_step(self, refs, acc, counter, seed, batch, exact_sampler=True, walkers=None, out_walkers=None, ratios=None):
        """One overlap measurement step on the device (wf_vqmc_overlap_step): no host work, no wait, capturable in a hipGraph after one call
        outside the capture.  The step draws its walkers from this model (stream `seed` advanced by `counter`, one int64 on the device, + 1 at
        the end; out_walkers [batch, D], if given, receives them) or reads them from `walkers` [batch, D]; it evaluates psi of this model and of
        every DeviceModel of `refs` (1 .. 8 of them, on this device, with this D, holding their parameters; this model may be among them) on
        them, adds r_k = psi_k / (psi + 1e-8) to `acc` (an overlap.Accumulator; None with `ratios`) and writes them to `ratios` [K, batch] if
        given.  No model changes.  Arguments are checked before anything is launched (ValueError)."""
        from . import overlap
        refs = list(refs)
        K = overlap._check_K(len(refs))
        batch = overlap._check_step(batch, self.D, K, walkers, out_walkers, ratios)
        for r in refs:
            if not isinstance(r, DeviceModel) or r.D != self.D or r.device != self.device:
                raise ValueError(f"every reference must be a DeviceModel of {self.D} coordinates on device {self.device}")
        if acc is None and ratios is None:
            raise ValueError("nothing to do: neither an accumulator nor ratios")
        if acc is not None and (not isinstance(acc, overlap.Accumulator) or acc.K != K):
            raise ValueError(f"the accumulator must be an overlap.Accumulator of {K} reference states")
        if not hasattr(counter, "is_cuda") or counter.numel() != 1 or str(counter.dtype) != "torch.int64" or not counter.is_cuda:
            raise ValueError("counter must be one int64 on the device (no CPU fallback)")
        st = acc.st if acc is not None else {"x": counter, "ws": None}
        ws = self._train_ws(st, self.overlap_step_workspace_bytes(batch, K))
        handles = (ctypes.c_void_p * K)(*[r._h.value for r in refs])
        x = walkers if walkers is not None else out_walkers
        _lib.check(overlap.lib().wf_vqmc_overlap_step(self._h, handles, K, ctypes.byref(acc.c) if acc is not None else None, self._p(counter),
                                                      int(seed) & 0xFFFFFFFFFFFFFFFF, batch, int(bool(exact_sampler)), self._p(x), int(walkers is None),
                                                      self._p(ratios), *ws, self._stream()), "wf_vqmc_overlap_step")

    # ---- fixed-node diffusion Monte Carlo on the device (include/waveflow_dmc.h; dmc.run drives it)
    def dmc_workspace_bytes(self, n_walkers):
        """Workspace of dmc_init and dmc_step for a population of n_walkers; WfError where the library has no such step for this model or size."""
        from . import dmc
        return _lib.check(dmc.lib().wf_vqmc_dmc_workspace_bytes(self._h, int(n_walkers)), "wf_vqmc_dmc_workspace_bytes")

    def make_dmc_state(self, n_walkers, ring_len=1024):
        """-> dmc.State: the device tensors of a population of n_walkers on this model's device (filled by dmc_init)."""
        from . import dmc
        return dmc.State(n_walkers, self.D, ring_len, f"cuda:{self.device}")

    def dmc_init(self, state, seed, protons, exact_sampler=True, walkers=None):
        """Fills `state` (wf_vqmc_dmc_init): its walkers from |psi|^2 (stream `seed`) or copied from `walkers` [n, D] (contiguous float32 cuda),
        psi, grad and e_loc on them, E_T their mean local energy, one comb that replaces walkers that are not finite, counter 0."""
        from . import dmc
        if walkers is not None:
            dmc._float_tensor(walkers, (state.n, self.D), "walkers", state.device)
        if state.D != self.D:
            raise ValueError(f"the state holds {state.D} columns, the model has {self.D}")
        ws = self._train_ws(state.st, self.dmc_workspace_bytes(state.n))
        _lib.check(dmc.lib().wf_vqmc_dmc_init(self._h, ctypes.byref(state.c), int(seed) & 0xFFFFFFFFFFFFFFFF, state.n, *self._protons(protons),
                                              int(bool(exact_sampler)), self._p(walkers), int(walkers is None), *ws, self._stream()),
                   "wf_vqmc_dmc_init")

    def dmc_step(self, state, seed, protons, tau, limit_drift=False, e_cut=0.0):
        """One DMC generation on the device (wf_vqmc_dmc_step): propose, wf_psi_coord_derivs at the proposals, accept, the comb, the ring record,
        E_T, counter + 1.  No host work, no wait, capturable in a hipGraph after one call outside the capture.  Nothing of the model changes.
        Arguments are checked before anything is launched (ValueError)."""
        from . import dmc
        tau, e_cut = dmc._check_tau(tau, e_cut)
        if state.D != self.D:
            raise ValueError(f"the state holds {state.D} columns, the model has {self.D}")
        ws = self._train_ws(state.st, self.dmc_workspace_bytes(state.n))
        _lib.check(dmc.lib().wf_vqmc_dmc_step(self._h, ctypes.byref(state.c), int(seed) & 0xFFFFFFFFFFFFFFFF, state.n, *self._protons(protons), tau,
                                              int(bool(limit_drift)), e_cut, *ws, self._stream()), "wf_vqmc_dmc_step")

    # ---- forward walking behind the comb (include/waveflow_dmc_observe.h; dmc.run(..., forward_walk=) drives it)
    def make_forward_walk(self, n_walkers, n_slots, stride, n_density_bins=200, n_pair_bins=200, lo=None, hi=None, series_len=4096):
        """-> dmc_observables.ForwardWalk for a population of n_walkers on this model's device; lo, hi default to the model's box."""
        from . import dmc_observables
        lo = -float(self.desc.box_size) if lo is None else lo
        hi = float(self.desc.box_size) if hi is None else hi
        return dmc_observables.ForwardWalk(n_walkers, self.D, n_slots, stride, n_density_bins, n_pair_bins, lo, hi, series_len, f"cuda:{self.device}")

    def dmc_fw_workspace_bytes(self, n_walkers, n_slots):
        """Workspace of dmc_fw_step for a population of n_walkers and a tracker of n_slots; WfError as dmc_workspace_bytes."""
        from . import dmc_observables
        return _lib.check(dmc_observables.lib().wf_vqmc_dmc_fw_workspace_bytes(self._h, int(n_walkers), int(n_slots)), "wf_vqmc_dmc_fw_workspace_bytes")

    def dmc_fw_step(self, state, fw, seed, protons, tau, limit_drift=False, e_cut=0.0):
        """One DMC generation with its forward-walking update (wf_vqmc_dmc_fw_step): the launches of dmc_step -- the state it leaves is bit for
        bit the one dmc_step leaves -- then the tracker `fw` (a ForwardWalk) composed with the comb's parent indices, measured and retagged as
        the state's counter says.  No host work, no wait, capturable like dmc_step.  Arguments are checked before anything is launched."""
        from . import dmc, dmc_observables
        tau, e_cut = dmc._check_tau(tau, e_cut)
        if state.D != self.D:
            raise ValueError(f"the state holds {state.D} columns, the model has {self.D}")
        if not isinstance(fw, dmc_observables.ForwardWalk) or (fw.n, fw.D) != (state.n, state.D) or fw.device != state.device:
            raise ValueError(f"the tracker must be a ForwardWalk of {state.n} walkers of {state.D} coordinates on {state.device}")
        ws = self._train_ws(state.st, self.dmc_fw_workspace_bytes(state.n, fw.n_slots))
        _lib.check(dmc_observables.lib().wf_vqmc_dmc_fw_step(self._h, ctypes.byref(state.c), ctypes.byref(fw.c), int(seed) & 0xFFFFFFFFFFFFFFFF, state.n,
                                                             *self._protons(protons), tau, int(bool(limit_drift)), e_cut, *ws, self._stream()),
                   "wf_vqmc_dmc_fw_step")

    def block_sums(self, v):
        """fp64 [sum v, sum v^2, count] on the device (deterministic order)."""
        torch = _torch()
        v = v.contiguous()
        ws = torch.empty(int(_lib.call("wf_block_sums_workspace_bytes", v.numel())), device=v.device, dtype=torch.uint8)
        out = torch.empty(3, device=v.device, dtype=torch.float64)
        _lib.call("wf_block_sums", self._p(v), v.numel(), self._p(out), self._p(ws), ws.numel(), self._stream())
        return out


def build_tables(kind, degree, n_internal_knots, n_mesh=2000):
    """Host-only: fp64 [4][n_bases][n_mesh] (+ (b_to_ob, ob_to_b) for kind == SPLINE_OB)."""
    nb = _lib.call("wf_tables_build", kind, degree, n_internal_knots, n_mesh, None, None, None)
    out = np.zeros((4, nb, n_mesh))
    if kind == _lib.SPLINE_OB:
        b2o, o2b = np.zeros((nb, nb)), np.zeros((nb, nb))
        _lib.call("wf_tables_build", kind, degree, n_internal_knots, n_mesh, out.ctypes.data, b2o.ctypes.data, o2b.ctypes.data)
        return out, b2o, o2b
    _lib.call("wf_tables_build", kind, degree, n_internal_knots, n_mesh, out.ctypes.data, None, None)
    return out
