"""MSpline_fun (msplines_jax.py:67-196) on the HIP path."""
from .. import _lib
from ._device import build_closures

MAX_PROPOSALS = 100000   # per output slot; the reference's while_loop is unbounded


def MSpline_fun():

    def init_fun(rng, k, n_internal_knots, cardinal_splines=True, zero_border=False, use_cached_bases=True,
                 cached_bases_path_root='./cached_splines_bases/M/', n_mesh_points=1000,
                 constraints_dict_left={0: 0}, constraints_dict_right={0: 0}):
        """-> (initial_params, apply_fun_vec, apply_fun_vec_grad, sample_fun_vec, knots, enforce_boundary_conditions, remove_bias)"""
        initial_params, knots, dev = build_closures(_lib.SPLINE_M, rng, k, n_internal_knots, cardinal_splines, zero_border, use_cached_bases,
                                                    cached_bases_path_root, n_mesh_points, constraints_dict_left, constraints_dict_right)

        def apply_fun_vec(params, x):
            return dev.apply(params, x)

        def apply_fun_vec_grad(params, x):
            return dev.apply(params, x, grad=True)[1]

        def sample_fun_vec(rng_array, params, num_samples, max_proposals=MAX_PROPOSALS):
            """[N, num_samples] draws of density proportional to min(f, max(c) * len(knots)); a slot still without a draw after
            max_proposals proposals raises, naming its row."""
            return dev.sample(rng_array, params, num_samples, max_proposals)

        def enforce_boundary_conditions(weights):
            return dev.rowwise("wf_spline_enforce_bc", weights)

        def remove_bias(params):
            return dev.rowwise("wf_spline_remove_bias", params)

        apply_fun_vec.spline = dev
        return initial_params, apply_fun_vec, apply_fun_vec_grad, sample_fun_vec, knots, enforce_boundary_conditions, remove_bias

    return init_fun
