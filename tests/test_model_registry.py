"""CPU: every filter model kind goes through ONE registry of factories (csrc/mp_models_builtin.h for the eight built-in kinds,
MP_REGISTER_UNFOLD_MODEL for the rest).  A descriptor is judged before the first HIP call, so a rejected one needs no GPU: one
bad descriptor per built-in kind keeps its status code (callers tell MP_ERR_INVALID_ARG from MP_ERR_UNSUPPORTED) and leaves a
message for mp_last_error().  No kernel is launched."""
import numpy as np
import pytest


def _cases():
    import modppl_amd as mp
    from modppl_amd import capi

    U, bad, unsup = mp.UnfoldModel, capi.MP_ERR_INVALID_ARG, capi.MP_ERR_UNSUPPORTED
    eye16 = np.eye(16)
    return [
        ("lgssm1: four params", U(capi.MP_MODEL_LGSSM1, 1, 1, [0.0, 1.0, 0.9, 0.5], "bad"), bad, "MP_MODEL_LGSSM1"),
        ("lgssm1: sig_y = 0", mp.lgssm_model(0.0, 1.0, 0.9, 0.5, 0.0), bad, "standard deviations"),
        ("spiral: dim_state 3", U(capi.MP_MODEL_SPIRAL, 3, 2, [], "bad"), bad, "MP_MODEL_SPIRAL"),
        ("hmm: nine states", mp.hmm_model(np.full(9, 1 / 9), np.full((2, 9), 0.5), np.full((9, 9), 1 / 9)), unsup, "MP_MODEL_HMM"),
        ("hmm: prior sums to 1.1", mp.hmm_model([0.5, 0.6], np.eye(2), np.eye(2)), bad, "prior"),
        ("bearings: sig_theta < 0", mp.bearings_model(sig_theta=-0.02), bad, "MP_MODEL_BEARINGS"),
        ("band: D = 3", mp.lgssm_band_model(D=3), unsup, "D in {2, 4, 16}"),
        ("band: dim_state != D", U(capi.MP_MODEL_LGSSM_BAND, 4, 4, [16, 0.9, 0.05, 1.0, 0.5, 1.0], "bad"), bad, "dim_state = dim_obs = D"),
        ("pointed_2d: xmax < xmin", mp.pointed_2d_model(bounds=(5.0, -5.0, -5.0, 5.0)), bad, "xmax > xmin"),
        ("pointed_2d: no Cholesky factor", mp.pointed_2d_model(cov=((-1.0, 0.0), (0.0, -1.0))), unsup, "Cholesky"),
        ("line: five points", mp.line_model(xs=(0.0, 1.0, 2.0, 3.0, 4.0)), unsup, "MP_MODEL_LINE"),
        ("dense: D = 8", mp.lgssm_dense_model(np.eye(8), np.eye(8), np.eye(8)), unsup, "D = 16"),
        ("dense: sig0 = 0", mp.lgssm_dense_model(eye16, eye16, eye16, sig0=0.0), bad, "sig0"),
        ("stochastic volatility (registered): sigma = 0", mp.stochastic_volatility_model(sigma=0.0), bad, "stochastic volatility: standard deviations must be > 0"),
        ("unknown kind", U(9999, 1, 1, [0.0], "bad"), unsup, "model kind 9999 is not compiled into this library"),
    ]


def test_rejected_descriptors_keep_their_codes_and_messages():
    import modppl_amd as mp
    from modppl_amd import build, capi

    build.build()
    L = capi.load()
    for what, model, code, text in _cases():
        with pytest.raises(mp.ModpplError) as e:
            mp.ParticleSystem(model, 10, 1)
        assert e.value.code == code, (what, e.value.code, str(e.value))
        msg = L.mp_last_error().decode()
        assert msg and text in msg, (what, msg)
