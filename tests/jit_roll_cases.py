"""Likelihoods summed over data rows for the tests of the rolled callback route (hamiltorch_amd/jit/roll.py): plain closures over
tensors, synthetic data from a fixed generator.  Shared by tests/test_jit_roll_cpu.py and tests/test_gpu_jit_roll.py."""
import numpy as np
import torch


def _t(a, dtype, device):
    return torch.tensor(np.asarray(a), dtype=dtype, device=device)


def logistic(N=40, D=3, dtype=torch.float64, device="cpu", seed=0):
    """Case 1: Bayesian logistic regression, binary labels - (y log s(Xw) + (1 - y) log s(-Xw)).sum() - 0.5 |w|^2."""
    rng = np.random.default_rng(seed)
    X, y = _t(rng.standard_normal((N, D)), dtype, device), _t((rng.uniform(size=N) > 0.5).astype(np.float64), dtype, device)

    def f(w):
        z = X @ w
        return (y * torch.log(torch.sigmoid(z)) + (1 - y) * torch.log(torch.sigmoid(-z))).sum() - 0.5 * (w * w).sum()
    f.data = (X, y)
    return f


def hierarchical(N=24, D=4, dtype=torch.float64, device="cpu", seed=1):
    """Case 2: linear regression with a sampled noise scale - sigma = exp(th[D-1]), Normal(X b, sigma).log_prob(y).sum()."""
    rng = np.random.default_rng(seed)
    X, y = _t(rng.standard_normal((N, D - 1)), dtype, device), _t(rng.standard_normal(N), dtype, device)

    def f(th):
        sigma = torch.exp(th[D - 1])
        return torch.distributions.Normal(X @ th[:D - 1], sigma).log_prob(y).sum()
    f.data = (X, y)
    return f


def two_structures(n=16, D=3, dtype=torch.float64, device="cpu", seed=2):
    """Case 3: n Poisson rows (log rate Xp w) + n Gaussian rows (mean Xg w, unit scale) + a Gaussian prior; the LAST Poisson row has
    x = 0 features, folds to a constant of another shape and stays in the rest."""
    rng = np.random.default_rng(seed)
    Xp = rng.standard_normal((n + 1, D)) * 0.5
    Xp[n] = 0.0
    k = rng.poisson(2.0, n + 1).astype(np.float64)
    Xp, k = _t(Xp, dtype, device), _t(k, dtype, device)
    Xg, yg = _t(rng.standard_normal((n, D)), dtype, device), _t(rng.standard_normal(n), dtype, device)

    def f(w):
        eta = Xp @ w
        r = yg - Xg @ w
        return (k * eta - torch.exp(eta)).sum() - 0.5 * (r * r).sum() - 0.25 * (w * w).sum()
    f.data = (Xp, k, Xg, yg)
    return f


def big_logistic(N=1500, D=4, dtype=torch.float64, device="cpu", seed=3):
    """A data set beyond straight-line code (value + gradient: ~45 000 scalar operations, limit 6000): y z - softplus(z), prior."""
    rng = np.random.default_rng(seed)
    X, y = _t(rng.standard_normal((N, D)), dtype, device), _t((rng.uniform(size=N) > 0.5).astype(np.float64), dtype, device)

    def f(w):
        z = X @ w
        return (y * z - torch.nn.functional.softplus(z)).sum() - 0.5 * (w * w).sum()
    f.data = (X, y)
    return f
