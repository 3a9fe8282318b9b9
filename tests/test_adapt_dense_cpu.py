"""CPU: adapt.warmup_with(mass="dense") driven by the CPU oracle on the two rotated targets of tests/dense_adapt_cases.py, the
accumulator on the covariance restatement of tests/cov_cases.py - held to the conditions the GPU test
(tests/test_gpu_adapt_dense.py) puts on the engines, so the reference side of that test stays inside them on its own."""
import numpy as np
import pytest

import adapt_cases as A
import dense_adapt_cases as DA


@pytest.mark.parametrize("t", [DA.GAUSS, DA.SECH], ids=["gauss", "sech"])
def test_dense_warmup_on_the_oracle(t):
    """the dense warm-up and its follow-up at L = 2 against the diagonal warm-up of the same seeds and its follow-up at L = 10."""
    D = t.scale.size
    r = DA.oracle_warmup(t, "dense")
    assert np.asarray(r.inv_mass).shape == (D, D) and np.asarray(r.inv_mass).dtype == np.float32
    wins = [h for h in r.history if h["kind"] == "window"]
    assert [h["n_draws"] for h in wins] == [45, 45, 90, 180]
    assert len([h for h in r.history if h["kind"] == "block"]) == 45
    draws, acc = DA.oracle_follow_up(t, r, DA.L_DENSE)
    rhat, ess = A.diagnostics(draws)
    diag = DA.oracle_warmup(t, "diag")
    assert np.asarray(diag.inv_mass).shape == (D,)
    rhat_d, ess_d = A.diagnostics(DA.oracle_follow_up(t, diag, DA.L)[0])
    print("step size dense %.4f diagonal %.4f | diagonal follow-up: rhat %.3f" % (r.step_size, diag.step_size, rhat_d))
    DA.check(t.name, [bool(h["accepted"]) for h in wins], DA.whitened_eigenvalues(t, r.inv_mass), acc, rhat, ess, ess_d)


def test_the_resonance_is_real():
    """what the L = 2 of the follow-up avoids: with the EXACT mass and the step size 1.17 (inside the range dense warm-ups end
    at), L = 10 turns every coordinate by 3.98 pi and the chains stop mixing, however good the mass; L = 2 mixes."""
    from hamiltorch_amd import adapt
    t = DA.GAUSS
    r = adapt.WarmupResult(DA.start(t), 1.17, DA.covariance(t).astype(np.float32), [])
    angle = DA.L * 2.0 * np.arcsin(r.step_size / 2.0) / np.pi
    rhat10, ess10 = A.diagnostics(DA.oracle_follow_up(t, r, DA.L)[0])
    rhat2, ess2 = A.diagnostics(DA.oracle_follow_up(t, r, DA.L_DENSE)[0])
    print("step size %.4f: L = 10 turns by %.3f pi: rhat %.3f ess %.0f; L = 2: rhat %.4f ess %.0f" % (r.step_size, angle, rhat10, ess10, rhat2, ess2))
    assert abs(angle - round(angle)) < 0.1 and ess10 < 0.05 * ess2
