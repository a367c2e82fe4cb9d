"""wf_psi_antisym_fwd, wf_logpdf_unsorted_fwd and wf_inversion_count on walkers in ANY particle order, for every kernel shape that sorts or reads
sorted rows: every wf_mfma_inst_* unit with the presort bit (one and two row blocks, the two-tile own-walker kernel), the wave and the scalar
route (k_sort_rows -> scratch -> k_apply_sign) for every D, the automatic route of small batches (sorted rows behind the wave tails).

The batch (tests/walker_order.py, pinned on the host by tests/test_walker_order_host.py) holds all D! orders of every base walker -- the reversed
order needs every pass of the sorting network, which a random row almost never does -- and the tie / signed-zero rows.  Every property is exact:
integers, or bit equality with another call of the same library on host-sorted rows; plus the project's fp64 yardstick on a sample."""
import numpy as np
import pytest

import oracle
import walker_order as wo
from test_gpu_mfma_paired import _shape
from test_gpu_parity import as_accurate_as_fp32_reference

pytestmark = pytest.mark.gpu

SIGN = np.int32(-2 ** 31)
N_LAYERS = 2


def make_model(D, kn):
    from waveflow_amd import model_factory
    init_fun = model_factory.get_waveflow_model(D, base_spline_degree=6, i_spline_degree=6, n_prior_internal_knots=kn, n_i_internal_knots=kn,
                                                i_spline_reg=0.05, n_flow_layers=N_LAYERS, box_size=wo.BOX_L)
    params, psi, log_pdf, _ = init_fun(42, D)
    psi.model.ensure_params(params)
    return params, psi.model


_BATCH = {}


def batch(D):
    """the batch of D-particle walkers and its host reference, once: (Batch, host-sorted rows, host inversion counts)"""
    if D not in _BATCH:
        b = wo.build_batch(D)
        _BATCH[D] = (b,) + wo.host_reference(b.x)
    return _BATCH[D]


def bits(t):
    """a device or host float32 array as int32 bits on the host"""
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(np.int32)


def check_rows(m, x, xs, inv_host, tag):
    """Assertions 1 - 4 on rows x (any order) with their host-sorted rows xs and host inversion counts; -> (bits of psi_antisym, psi(xs))."""
    import torch
    from waveflow_amd.utils.coordinates import get_num_inversion_count
    xd, xsd = torch.from_numpy(x).cuda(), torch.from_numpy(xs).cuda()
    ps, inv = m.psi_antisym(xd, return_inversions=True)
    assert inv.dtype == torch.int32 and np.array_equal(inv.cpu().numpy(), inv_host), (tag, "inversions of psi_antisym")
    assert np.array_equal(get_num_inversion_count(xd).cpu().numpy(), inv_host), (tag, "wf_inversion_count")
    ref = m.psi(xsd)
    got, want = bits(ps), bits(ref) ^ np.where(inv_host & 1, SIGN, np.int32(0))
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (tag, "psi_antisym != psi(sorted) with the parity in the sign bit", bad.size, bad[:8].tolist(), x[bad[:2]].tolist())
    assert np.array_equal(bits(m.psi_antisym(xd)), got), (tag, "psi_antisym without the inversion output")
    lpu, lp = bits(m.log_pdf_unsorted(xd)), bits(m.log_pdf(xsd))
    bad = np.flatnonzero(lpu != lp)
    assert bad.size == 0, (tag, "log_pdf_unsorted != log_pdf(sorted)", bad.size, bad[:8].tolist(), x[bad[:2]].tolist())
    return got, ref.cpu().numpy()


def check_every_order(m, D, tag):
    """Assertions 1 - 8 under the kernel choice and environment the caller holds."""
    import torch
    b, xs, inv = batch(D)
    N = len(b.x)
    # 8. call order first, while this model's scratch is what model creation reserved: a big call grows it, a small one and the big one
    # again reuse it oversized
    big, small = torch.from_numpy(b.x).cuda(), torch.from_numpy(b.x[:33]).cuda()
    first = bits(m.psi_antisym(big))
    small_bits = bits(m.psi_antisym(small))
    assert np.array_equal(bits(m.psi_antisym(big)), first), (tag, "big, small, big: the third call differs from the first")
    # 1 - 4 on the whole batch
    got, ref = check_rows(m, b.x, xs, inv, tag)
    assert np.array_equal(got, first), tag
    # 5. the sorted rows of distinct coordinates have a finite psi
    ties = wo.tie_rows(b.x)
    assert np.isfinite(ref[~ties]).all() and (ref[~ties] != 0).any(), tag
    # 6. the D! orders of a base walker: the same magnitude bits, whichever lane and tile each landed on
    rows = b.base >= 0
    mag = got & np.int32(0x7fffffff)
    per_base = np.zeros(wo.n_base(D), np.int32)
    per_base[b.base[rows]] = mag[rows]
    bad = np.flatnonzero(rows & (mag != per_base[np.maximum(b.base, 0)]))
    assert bad.size == 0, (tag, "orders of one walker differ in magnitude bits", bad.size, bad[:8].tolist())
    # 7. ragged batches: the first B rows
    for B in wo.RAGGED:
        g, _ = check_rows(m, b.x[:B], xs[:B], inv[:B], (tag, B))
        if B == 33:
            assert np.array_equal(g, small_bits), (tag, "the small call between the two big ones")
        # a row's value does not depend on the batch it is in: same route at every B <= N for the forced kernels; under "auto" only where the
        # whole batch takes the small-batch route too
        if same_route_at_every_size(tag, N):
            assert np.array_equal(g, got[:B]), (tag, B, "first B rows differ from the same rows of the whole batch")


def same_route_at_every_size(tag, N):
    return tag[0] != "auto" or N <= 6144     # kWaveEvalMax: the automatic route changes kernel there


@pytest.mark.parametrize("shape", wo.SHAPES, ids=lambda s: f"D{s[0]}-{s[1]}knots")
@pytest.mark.parametrize("kernel", wo.KERNELS)
def test_every_order_of_every_walker(kernel, shape):
    from waveflow_amd import _lib
    D, kn = shape
    _, m = make_model(D, kn)
    if (kernel, shape) in wo.REFUSED:
        with pytest.raises(_lib.WfError) as e:
            m.set_kernel(kernel)
        assert e.value.status == _lib.ERR_UNSUPPORTED
        return
    m.set_kernel(kernel)
    check_every_order(m, D, (kernel, shape))


@pytest.mark.parametrize("waves,tiles", ((8, 2), (4, 2)))
def test_every_order_on_the_two_tile_kernel(waves, tiles):
    """k_mfma<2, 1, W, 2>: the own-walker layout sorts and signs in its own code (wf_mfma_impl.h), log_pdf_unsorted included"""
    _, m = make_model(2, 23)
    m.set_kernel("mfma")
    with _shape(waves, tiles):
        check_every_order(m, 2, ("mfma", (2, 23), waves, tiles))
    # the same bits as the one-tile kernel (tests/test_gpu_mfma_paired.py says so for sorted rows and every other row exchanged)
    import torch
    x = torch.from_numpy(batch(2)[0].x).cuda()
    with _shape(waves, tiles):
        two = bits(m.psi_antisym(x)), bits(m.log_pdf_unsorted(x))
    with _shape(16, 1):
        one = bits(m.psi_antisym(x)), bits(m.log_pdf_unsorted(x))
    assert np.array_equal(two[0], one[0]) and np.array_equal(two[1], one[1])


@pytest.mark.parametrize("shape", ((3, 23), (4, 23), (5, 23), (6, 23), (7, 23), (3, 33)), ids=lambda s: f"D{s[0]}-{s[1]}knots")
def test_signed_psi_of_every_16th_row_against_fp64(shape):
    """Assertion 9: "psi(sorted) and psi_antisym wrong alike" excluded, with the yardstick and tolerances of
    test_c4_antisymmetrised_psi_of_unsorted_walkers_on_the_device.  Tie rows are left out of the sample: two equal coordinates put a zero width
    into the box transform, where the fp32 and the fp64 oracle need not agree on finiteness -- their bits are pinned by assertion 3."""
    import torch
    from waveflow_amd import flatten_params
    D, kn = shape
    params, m = make_model(D, kn)
    m.set_kernel("mfma")
    b, xs, inv = batch(D)
    sel = np.arange(0, len(b.x), 16)
    sel = sel[~wo.tie_rows(b.x[sel])]
    om = oracle.Model(D=D, n_layers=N_LAYERS, box="mean", box_L=wo.BOX_L, i_k=6, i_knots=kn, i_reg=0.05, i_left={0: 0}, i_right={0: 1},
                      prior="waveflow", p_k=6, p_knots=kn, p_left={0: 0}, p_right={0: 0}, constr_left=tuple(range(D - 1)))
    flat = flatten_params(params)
    sign = (-1.0) ** inv[sel]
    o32 = om.psi(flat, xs[sel], threads=8)
    o64 = om.psi(flat, xs[sel], threads=8, f64=True)
    got = m.psi_antisym(torch.from_numpy(b.x).cuda())[torch.from_numpy(sel).cuda()].cpu().numpy()
    assert (inv[sel] & 1).any() and not (inv[sel] & 1).all()
    as_accurate_as_fp32_reference(got, o32 * sign, o64 * sign, atol=1e-6 * np.abs(o64).max(), what=f"psi_antisym D={D}, {kn} knots, every 16th row")
    nz = np.abs(o64) > 1e-6 * np.abs(o64).max()
    assert nz.sum() > len(sel) // 2
    assert np.array_equal(np.sign(got[nz]), np.sign((o64 * sign)[nz]))
