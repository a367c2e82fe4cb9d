"""ISpline_fun (isplines_jax.py:84-207) on the HIP path."""
from .. import _lib
from ._device import build_closures


def ISpline_fun():

    def init_fun(rng, k, n_internal_knots, cardinal_splines=True, zero_border=True, reverse_fun_tol=None,
                 use_cached_bases=True, cached_bases_path_root='./cached_splines_bases/I/', n_mesh_points=1000,
                 constraints_dict_left={0: 0.0}, constraints_dict_right={0: 1.0}):
        """-> (initial_params, apply_fun_vec, apply_fun_vec_grad, reverse_fun_vec, knots, enforce_boundary_conditions, remove_bias)"""
        if reverse_fun_tol is None:
            reverse_fun_tol = 1 / n_mesh_points
        initial_params, knots, dev = build_closures(_lib.SPLINE_I, rng, k, n_internal_knots, cardinal_splines, zero_border, use_cached_bases,
                                                    cached_bases_path_root, n_mesh_points, constraints_dict_left, constraints_dict_right)

        def apply_fun_vec(params, x):
            return dev.apply(params, x)

        def apply_fun_vec_grad(params, x):
            return dev.apply(params, x, grad=True)[1]

        def reverse_fun_vec(params, y):
            return dev.reverse(params, y, reverse_fun_tol)

        def enforce_boundary_conditions(weights):
            return dev.rowwise("wf_spline_enforce_bc", weights)

        def remove_bias(params):
            return dev.rowwise("wf_spline_remove_bias", params)

        apply_fun_vec.spline = dev
        return initial_params, apply_fun_vec, apply_fun_vec_grad, reverse_fun_vec, knots, enforce_boundary_conditions, remove_bias

    return init_fun
