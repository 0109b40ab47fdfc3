"""Mixing matrices for temporally correlated sampling in CEM / PI2 (Engine.set_sampling_correlation).

A candidate's standard draws z[0..H-1] become y = L @ z along the time axis; with L the lower-triangular Cholesky factor of
an autocovariance matrix with unit diagonal, y keeps unit variance per step and gets that autocovariance (exactly for normal
draws, to a good approximation for the engine's truncated ones).  Everything is computed in float64 and returned as float32.
"""
import numpy as np


def _cholesky_of_autocovariance(c):
    h = c.shape[0]
    idx = np.abs(np.arange(h)[:, None] - np.arange(h)[None, :])
    return np.linalg.cholesky(c[idx]).astype(np.float32)


def colored_noise_autocovariance(horizon, beta):
    """c[tau], tau = 0..H-1, of noise with the power-law spectrum S_k = (k / 2H)^(-beta), k = 1..H, sampled at the H
    planning steps: c[tau] = 0.5 S_1 + sum_{k=1}^{H-1} S_k cos(pi k tau / H) + 0.5 S_H (-1)^tau, normalised to c[0] = 1.
    beta = 0 is white noise (c = 1, 0, 0, ...), 1 pink, 2 red."""
    h = int(horizon)
    if h < 1:
        raise ValueError("horizon must be >= 1, got %r" % (horizon,))
    beta = float(beta)
    if not np.isfinite(beta) or beta < 0.0:
        raise ValueError("noise_beta must be finite and >= 0, got %r" % (beta,))
    k = np.arange(1, h + 1, dtype=np.float64)
    s = (k / (2.0 * h)) ** (-beta)
    tau = np.arange(h, dtype=np.float64)
    c = 0.5 * s[0] + 0.5 * s[-1] * np.where(np.arange(h) % 2 == 0, 1.0, -1.0)
    if h > 1:
        c = c + np.cos(np.pi * np.outer(tau, k[:-1]) / h) @ s[:-1]
    return c / c[0]


def colored_noise_mixing(horizon, beta):
    """[H, H] float32 lower-triangular factor L with L @ L.T = toeplitz(colored_noise_autocovariance(H, beta)): iCEM's
    colored noise as a mixing matrix.  beta = 0 gives the identity."""
    return _cholesky_of_autocovariance(colored_noise_autocovariance(horizon, beta))


def ar1_mixing(horizon, rho):
    """The same for the AR(1) / Ornstein-Uhlenbeck autocovariance c[tau] = rho^tau, |rho| < 1.  rho = 0 gives the identity."""
    h = int(horizon)
    if h < 1:
        raise ValueError("horizon must be >= 1, got %r" % (horizon,))
    rho = float(rho)
    if not np.isfinite(rho) or abs(rho) >= 1.0:
        raise ValueError("rho must satisfy |rho| < 1, got %r" % (rho,))
    return _cholesky_of_autocovariance(rho ** np.arange(h, dtype=np.float64))


def resolve_sampling_correlation(horizon, noise_beta=None, sampling_correlation=None):
    """What CEMOptimizer / PI2Optimizer hand to the engine: None, colored_noise_mixing(H, noise_beta), or the caller's own
    [H, H] matrix, checked."""
    if noise_beta is not None and sampling_correlation is not None:
        raise ValueError("pass noise_beta or sampling_correlation, not both")
    if noise_beta is not None:
        return colored_noise_mixing(horizon, noise_beta)
    if sampling_correlation is None:
        return None
    m = np.asarray(sampling_correlation, dtype=np.float32)
    h = int(horizon)
    if m.shape != (h, h):
        raise ValueError("sampling_correlation must be [planning_horizon, planning_horizon] = [%d, %d], got %s" % (h, h, m.shape))
    if not np.all(np.isfinite(m)):
        raise ValueError("sampling_correlation has a non-finite entry")
    return np.ascontiguousarray(m)
