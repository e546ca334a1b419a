"""Fixtures and ground truth of the device IACT tests (test_gpu_iact.py): AR(1) series, the extended-precision restatement of
the semantics (mean, centred lag sums, rho, the running T_k, the window rule), the host path's window from pmg_iact's own
autocorrelation, and the bounds -- which come from the input alone.  Needs no GPU."""
import ctypes as C

import numpy as np

U = 2.0 ** -53  # unit roundoff of float64
PHIS = (0.0, 0.5, 0.9, -0.5)
MARGIN = 1e-6  # every fixture keeps |i - 5 T_i| above this for i <= window: the window is a discrete decision


def ar1(n, phis, rng):
    """(n, len(phis)): x_t = phi x_{t-1} + sqrt(1 - phi^2) eps_t, x_0 = eps_0 (stationary, unit variance), one column per phi"""
    phis = np.asarray(phis, np.float64)
    eps = rng.standard_normal((n, len(phis)))
    x = np.empty_like(eps)
    x[0] = eps[0]
    g = np.sqrt(1.0 - phis * phis)
    for t in range(1, n):
        x[t] = phis * x[t - 1] + g * eps[t]
    return x


def ar1_cycle(n, S, seed):
    """case 1 of the issue: phi cycles over PHIS by series, default_rng(seed)"""
    return ar1(n, [PHIS[s % len(PHIS)] for s in range(S)], np.random.default_rng(seed))


def phi_for_window(w):
    """the AR(1) coefficient whose IACT (1 + phi) / (1 - phi) is w / 5"""
    return (w / 5.0 - 1.0) / (w / 5.0 + 1.0)


def host_iact(x):
    """pmg_iact on one series and its window: (tau, window, valid, T) with T the host's 2 cumsum(acf) - 1.  The window loop is
    pmg_diag.c:87-103 on the autocorrelation pmg_iact returns; T[window] is checked to be the tau it returned, bit for bit."""
    from parmgmc_amd.capi import lib

    x = np.ascontiguousarray(x, np.float64)
    n = len(x)
    acf = np.empty(n)
    tau, valid = C.c_double(), C.c_int()
    assert lib.pmg_iact(n, x.ctypes.data, C.byref(tau), acf.ctypes.data, C.byref(valid)) == 0
    T = 2 * np.cumsum(acf) - 1  # sequential in float64, as out[i] = out[i] + out[i - 1]
    k = np.arange(n, dtype=np.float64)
    if np.isnan(T).all():
        return tau.value, n - 1, bool(valid.value), T
    hits = np.nonzero(k >= 5 * T)[0]
    w = int(hits[0]) if len(hits) else 0
    assert T[w] == tau.value, (T[w], tau.value)
    return tau.value, w, bool(valid.value), T


def margin(T, w):
    """min over i <= w of |i - 5 T_i| on the host values"""
    i = np.arange(w + 1, dtype=np.float64)
    return float(np.abs(i - 5 * T[: w + 1]).min())


def truth(x, nlags):
    """(rho, T) of the lags 0 .. nlags - 1 in np.longdouble, straight from the definitions"""
    xl = np.asarray(x, np.longdouble)
    n = len(xl)
    z = xl - xl.sum() / n
    c = np.array([np.dot(z[: n - k], z[k:]) for k in range(nlags)], np.longdouble)
    rho = c / c[0]
    return rho, 2 * np.cumsum(rho) - 1


def rho_bound(x):
    """8 n u (1 + |mean| / rms(z)): the bound of a length-n sum of products of centred data, numerator and denominator, with
    the cancellation of the mean made explicit"""
    xl = np.asarray(x, np.longdouble)
    n = len(xl)
    m = xl.sum() / n
    rms = np.sqrt(((xl - m) ** 2).sum() / n)
    return float(8 * n * U * (1 + abs(m) / rms))


def tau_bound(x, window):
    return 2 * (window + 1) * rho_bound(x)


# series whose host window is exactly the key -- the edges of a 256-lag block: window -> (n, seed), found once by a search on the
# CPU over seed = 0, 1, ... with x = ar1(n, [phi_for_window(window)], default_rng(seed))[:, 0] and a margin above 1e-4 (n = 6000
# has no seed below 1500 for window 512; n = 9000 has)
EDGE_SEEDS = {255: (6000, 609), 256: (6000, 499), 257: (6000, 180), 512: (9000, 94)}
