"""The forecast moments of DESIGN.md section 4 ("Forecast"), restated in numpy on tests/moments_ref.py's tree sum and weights
(modppl_amd/csrc/mp_forecast.h, k_forecast_mom, is the device's statement):

    mean[k][c] = TREE(a_i v_ic(k)) / A;   var[k][c] = TREE(a_i (v_ic(k) - mean[k][c])^2) / A

over the forecast states v_i(k) [dim_state] and, with the same two formulas, the forecast observations y_i(k) [dim_obs].  The paths
themselves are not restated here: they are held bit for bit against `simulate` and against the filter's own next steps.
"""
import numpy as np

from tests import moments_ref as R


def _columns(paths, a, A, var):
    paths = np.asarray(paths, dtype=np.float64)
    n, H, w = paths.shape
    mean, v = np.empty((H, w)), (np.empty((H, w)) if var else None)
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(H):
            for j in range(w):
                mean[k, j] = R.tree_sum(a * paths[:, k, j]) / A
                if var:
                    c = paths[:, k, j] - mean[k, j]
                    v[k, j] = R.tree_sum(a * (c * c)) / A
    return mean, v


def forecast_moments(states, obs, lw, var=True):
    """states [n, H, d], obs [n, H, dobs], lw [n]  ->  (state_mean [H, d], state_var or None, obs_mean [H, dobs], obs_var or None),
    bit for bit what mp_pf_forecast_moments returns (up to the sign of a zero)"""
    _, _, a = R.pf_weights(lw)
    A = R.tree_sum(a)
    sm, sv = _columns(states, a, A, var)
    om, ov = _columns(obs, a, A, var)
    return sm, sv, om, ov
