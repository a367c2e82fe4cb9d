"""BSpline_fun (bsplines_jax.py:52-203) on the HIP path.  As in the reference, the closures map the coefficients to
normalised(c @ ob_to_b) and evaluate those against the orthogonalised tables; enforce_boundary_conditions reads the plain B tables."""
from .. import _lib
from ._device import build_closures
from .msplines_jax import MAX_PROPOSALS


def BSpline_fun():

    def init_fun(rng, k, n_internal_knots, cardinal_splines=True, use_cached_bases=True,
                 cached_bases_path_root='./cached_splines_bases/B/', n_mesh_points=1000,
                 constraints_dict_left={0: 0}, constraints_dict_right={0: 0}):
        """-> (initial_params, apply_fun_vec, apply_fun_vec_grad, sample_fun_vec, knots, enforce_boundary_conditions)"""
        initial_params, knots, dev = build_closures(_lib.SPLINE_B, rng, k, n_internal_knots, cardinal_splines, False, use_cached_bases,
                                                    cached_bases_path_root, n_mesh_points, constraints_dict_left, constraints_dict_right)

        def apply_fun_vec(params, x):
            return dev.apply(params, x)

        def apply_fun_vec_grad(params, x):
            return dev.apply(params, x, grad=True)[1]

        def sample_fun_vec(rng_array, params, num_samples, max_proposals=MAX_PROPOSALS):
            """[N, num_samples] draws of density proportional to min(f^2, ymax), ymax = max((normalised(c @ ob_to_b) @ b_to_ob)^2);
            a slot still without a draw after max_proposals proposals raises, naming its row."""
            return dev.sample(rng_array, params, num_samples, max_proposals)

        def enforce_boundary_conditions(weights):
            return dev.rowwise("wf_spline_enforce_bc", weights)

        apply_fun_vec.spline = dev
        return initial_params, apply_fun_vec, apply_fun_vec_grad, sample_fun_vec, knots, enforce_boundary_conditions

    return init_fun
