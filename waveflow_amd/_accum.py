"""What the measurement modules (observables, overlap, dmc, dmc_observables, sr) share on the Python side of the device's fp64 accumulation
(csrc/wf_accum.h): `ordered_sum`, the order of the device's sums restated in numpy -- the bit-for-bit tests and overlap.reference_accumulate
rest on it --, the argument checks of a tensor and of a step's walkers, the device of an accumulator, the all-reduce of its totals and the
measurement loop.  The checks take the calling module's phrase ("the observables have no CPU fallback", ...) for their messages."""
import numpy as np

GRID_BLOCKS, BLOCK = 1024, 256   # the capped grid of an accumulation kernel (csrc/wf_accum.h: kObsMaxBlocks, kObsBlock)


def ordered_sum(v):
    """The fp64 sum of v [B] in the order of the device (csrc/wf_accum.h states it): lane sums in walker order over the grid-stride loop, the
    shuffle tree of a wave, the four waves of a block in order, then t = 0; t = t + block b, in block order.  A skipped walker enters as 0."""
    B = v.shape[0]
    blocks = min(-(-B // BLOCK), GRID_BLOCKS)
    stride = blocks * BLOCK
    passes = -(-B // stride)
    padded = np.zeros(passes * stride, np.float64)
    padded[:B] = v
    lanes = np.zeros(stride, np.float64)
    for p in range(passes):
        lanes = lanes + padded[p * stride:(p + 1) * stride]
    w = lanes.reshape(blocks, BLOCK // 64, 64)
    for half in (32, 16, 8, 4, 2, 1):
        w = w[..., :half] + w[..., half:2 * half]
    w = w[..., 0]
    per_block = w[:, 0]
    for k in range(1, BLOCK // 64):
        per_block = per_block + w[:, k]
    t = np.float64(0.0)
    for b in range(blocks):
        t = t + per_block[b]
    return t


def check_float_tensor(t, shape, what, phrase, device=None, on="", dtype=None):
    """`t` is a contiguous float32 (or `dtype`) cuda tensor of this shape, on `device` if one is given (`on`: how the message names that
    device, " on the device of the walkers"); ValueError otherwise, its texts those of the modules' checks."""
    import torch
    dtype = dtype or torch.float32
    if not hasattr(t, "is_cuda") or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what} must be a torch tensor of shape {list(shape)}")
    if t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous {str(dtype).replace('torch.', '')}, got {t.dtype}")
    if not t.is_cuda or (device is not None and t.device != device):
        raise ValueError(f"{what} must be a cuda tensor{on}: {phrase}")


def check_step_walkers(batch, n_dim, walkers, out_walkers, phrase, extra=()):
    """The walkers of one device-side step: `walkers` (read) and `out_walkers` (written) are contiguous float32 cuda tensors [batch, n_dim] or
    None, at most one of them given; `extra`: further (name, tensor or None, shape) of the same kind."""
    if walkers is not None and out_walkers is not None:
        raise ValueError("walkers (the step reads them) and out_walkers (the step writes what it drew) exclude each other")
    shape = (int(batch), int(n_dim))
    for what, t, s in (("walkers", walkers, shape), ("out_walkers", out_walkers, shape)) + tuple(extra):
        if t is not None:
            check_float_tensor(t, s, what, phrase)


def cuda_device(device, owner, phrase):
    """torch.device(device) with its index filled in; ValueError where it is no cuda device (`owner`: "an Accumulator")."""
    import torch
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"{owner} lives on a cuda device: {phrase}")
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


def all_reduce_totals(floats, ints, group=None):
    """SUM over the ranks of `group` of a float64 and an int64 numpy vector -> (floats, ints): one all-reduce each
    (distributed._all_reduce_sum).  The two buffers are host tensors under gloo; under any other backend (nccl: RCCL reduces device tensors
    only) they are moved to the current cuda device, reduced there and copied back."""
    import torch
    import torch.distributed as dist
    from .distributed import _all_reduce_sum
    f = torch.from_numpy(np.array(floats, dtype=np.float64).reshape(-1))
    i = torch.from_numpy(np.array(ints, dtype=np.int64).reshape(-1))
    if dist.get_backend(group) != "gloo":
        f, i = f.cuda(), i.cuda()
    _all_reduce_sum(f, group)
    _all_reduce_sum(i, group)
    return f.cpu().numpy().copy(), i.cpu().numpy().copy()


def measure_loop(model, acc, step, steps, workspace_bytes, restore, what, use_graph=True):
    """`steps` calls of step() into the accumulator `acc`, whose workspace is allocated here, outside a capture.  With use_graph the step is
    captured once (vqmc.capture_step) and replayed: its warm-up call outside the capture (the model entries grow their scratch there, not
    inside) is undone by putting back the tensors of `restore`.  The host waits once, at the end."""
    import torch
    acc.st["ws"] = model._workspace(workspace_bytes, acc.device)
    launch = step
    if use_graph:
        from . import vqmc
        kept = [t.clone() for t in restore]

        def warm_up():
            step()
            for t, k in zip(restore, kept):
                t.copy_(k)
        launch = vqmc.capture_step(model, step, warm_up, f"hipGraph capture of the {what} step failed")
    for _ in range(steps):
        launch()
    torch.cuda.synchronize(acc.device)
