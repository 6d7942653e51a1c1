"""The identities behind the lean weight-gradient group (csrc/wgrad.hip): feature_linear has no
activation and feeds the views layer linearly, so both weight gradients that touch `feature` follow from the one
sample-summed matrix M = sum_p dZv_p act7_p^T and s = sum_p dZv_p.  Checked in numpy fp64 against the direct sums."""
import numpy as np


def test_feature_layer_gradients_follow_from_one_views_layer_product():
    rng = np.random.default_rng(7)
    P = 200
    W_f = rng.standard_normal((256, 256)) / 16.0
    b_f = rng.standard_normal(256)
    W_vf = rng.standard_normal((128, 256)) / 16.0        # views_linears.0.weight[:, :256]
    act7 = np.maximum(rng.standard_normal((P, 256)), 0.0)
    dZv = rng.standard_normal((P, 128)) * (rng.random((P, 128)) < 0.5)

    feature = act7 @ W_f.T + b_f                          # [P, 256]
    dfeat = dZv @ W_vf                                    # [P, 256]
    direct_dWv = dZv.T @ feature                          # sum_p dZv_p feature_p^T
    direct_dWf = dfeat.T @ act7                           # sum_p dfeat_p act7_p^T
    direct_dbf = dfeat.sum(0)

    M = dZv.T @ act7                                      # [128, 256]
    s = dZv.sum(0)                                        # = d views bias
    lean_dWv = M @ W_f.T + np.outer(s, b_f)
    lean_dWf = W_vf.T @ M
    lean_dbf = W_vf.T @ s

    for lean, direct in ((lean_dWv, direct_dWv), (lean_dWf, direct_dWf), (lean_dbf, direct_dbf)):
        assert np.abs(lean - direct).max() <= 1e-12 * np.abs(direct).max()
