"""Walkers in any particle order: the batch of tests/test_gpu_walker_order.py and its host reference (no GPU; pinned by
tests/test_walker_order_host.py).  Per D the batch holds EVERY one of the D! orders of each of n_base sorted base walkers -- a random row
almost never needs all D passes of an odd-even transposition network, the reversed order of every base walker does -- plus the rows where a
sort can go wrong without a number changing much: ties (adjacent, between non-adjacent arrivals, all coordinates equal) and +-0."""
import itertools
import math
from collections import namedtuple

import numpy as np

from conftest import sorted_walkers

BOX_L = 10.0
# (D, knots): one 32-row block per dimension at 23 knots (29 bases), two at 33 knots (39 bases)
SHAPES = ((2, 23), (3, 23), (4, 23), (5, 23), (6, 23), (7, 23), (8, 23), (2, 33), (3, 33), (4, 33), (5, 33))
KERNELS = ("mfma", "wave", "scalar", "auto")
# (kernel, shape) pairs wf_model_set_kernel refuses: k_mfma is built for D <= 4 at two row blocks (mfma_shape_built); the wave and the scalar
# kernels serve every shape (wave_ok)
REFUSED = frozenset({("mfma", (5, 33))})
RAGGED = (1, 31, 33, 63, 65, 257, 1000)

Batch = namedtuple("Batch", "x base kind")   # rows [N, D] fp32; base walker of each row (-1: a special row); name of a special row ("" otherwise)


def n_row_blocks(knots, degree=6):
    """32-row blocks per dimension of the conditioner outputs: knots + degree bases (the prior's, one fewer for the I-splines)"""
    return (knots + degree + 31) // 32


def mfma_shape_built(D, nbk):
    """wf_kernels_mfma.hip, restated"""
    return (nbk == 1 and 2 <= D <= 8) or (nbk == 2 and 2 <= D <= 4)


def n_base(D):
    return max(1, 4096 // math.factorial(D))


def base_walkers(D, extra=0):
    return sorted_walkers(n_base(D) + extra, D, BOX_L, 7000 + D)


def permutations(D):
    return np.array(list(itertools.permutations(range(D))), dtype=np.int64)


def special_rows(D):
    """[(name, row)]: inside the box, coordinates 1.7 apart where they differ"""
    asc = ((np.arange(D) - 0.5 * (D - 1)) * 1.7 + 0.3).astype(np.float32)
    adjacent = asc.copy()
    adjacent[1] = adjacent[0]
    rows = [("ascending", asc), ("descending", asc[::-1].copy()), ("adjacent tie", adjacent), ("all equal", np.full(D, 0.3, np.float32))]
    if D >= 3:
        apart = asc.copy()                       # (a, b, a, ...) with b > a: one inversion, the pair (b, a)
        apart[2] = apart[0]
        rows.append(("tie of non-adjacent arrivals", apart))
    if D == 2:
        rows += [("+0 -0", np.array([0.0, -0.0], np.float32)), ("-0 +0", np.array([-0.0, 0.0], np.float32))]
    return rows


SPECIAL_INVERSIONS = {"ascending": lambda D: 0, "descending": lambda D: D * (D - 1) // 2, "adjacent tie": lambda D: 0, "all equal": lambda D: 0,
                      "tie of non-adjacent arrivals": lambda D: 1, "+0 -0": lambda D: 0, "-0 +0": lambda D: 0}


def build_batch(D):
    """Every order of every base walker, the special rows, shuffled once: the orders of one walker land in different tiles and lanes."""
    special = special_rows(D)
    extra = 1 if (n_base(D) * math.factorial(D) + len(special)) % 32 == 0 else 0     # never a whole number of 32-walker tiles
    base = base_walkers(D, extra)
    perms = permutations(D)
    nb = n_base(D)
    rows = [base[:nb][:, perms].reshape(-1, D)]
    ids = [np.repeat(np.arange(nb), len(perms))]
    kinds = [""] * (nb * len(perms))
    if extra:
        rows.append(base[nb:])
        ids.append(np.array([-1]))
        kinds.append("ascending")
    rows.append(np.stack([r for _, r in special]))
    ids.append(np.full(len(special), -1))
    kinds += [k for k, _ in special]
    x, ids, kinds = np.concatenate(rows).astype(np.float32), np.concatenate(ids), np.array(kinds)
    order = np.random.default_rng(90 + D).permutation(len(x))
    return Batch(np.ascontiguousarray(x[order]), ids[order], kinds[order])


def host_reference(x):
    """(rows sorted ascending, inversion counts).  The stable sort leaves equal keys -- +0 and -0 included -- in arrival order, as the device's
    exchanges on `>` do; the inversions are the pairs i < j with x_i > x_j."""
    from waveflow_amd.utils.coordinates import get_num_inversion_count
    x = np.asarray(x)
    return np.sort(x, axis=-1, kind="stable"), get_num_inversion_count(x)


def tie_rows(x):
    """rows with two equal coordinates (+0 == -0)"""
    s = np.sort(x, axis=-1)
    return (s[:, 1:] == s[:, :-1]).any(axis=1)


def parity_by_cycles(perm):
    """parity of a permutation from its cycle decomposition: a cycle of length c is c - 1 transpositions"""
    seen, odd = [False] * len(perm), 0
    for i in range(len(perm)):
        c = 0
        while not seen[i]:
            seen[i] = True
            i = perm[i]
            c += 1
        odd ^= (c - 1) & 1 if c else 0
    return odd
