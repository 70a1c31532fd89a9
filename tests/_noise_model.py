"""Correlated exploration noise in numpy fp32 (include/hirl4ucav.h "Exploration noise"): the AR(1) bank's rule with every product and sum rounded to fp32
in the kernel's order, the coefficient recipes of the three colours, the sigma ladder, the Philox counters with a float64 Box-Muller, and the analytic
autocorrelation and spectrum of a bank.  No GPU, no library."""
import numpy as np

from tests._upsample_model import philox4x32_10

MAX_POLES, MAX_STEPS = 8, 64
TAG_STEP, TAG_INIT = 0x4E4F4900, 0x4E4F4980
LADDER_MULT = 2654435761


# ---- the recipes: float64, stored as fp32 ------------------------------------------------------------------------------------------------------------
def recipe(kind, tau=16.0, octaves=6):
    """-> (a, b, w) fp32 [K]: white K = 1, a = 0; ou K = 1, a = exp(-1 / tau); pink K = octaves, a[k] = exp(-2^-k), w[k] = 1 / sqrt(K); b = sqrt(1 - a^2)"""
    if kind == "white":
        a, w = np.zeros(1), np.ones(1)
    elif kind == "ou":
        a, w = np.exp(-1.0 / np.array([float(tau)])), np.ones(1)
    elif kind == "pink":
        k = np.arange(int(octaves), dtype=np.float64)
        a, w = np.exp(-(2.0 ** -k)), np.full(int(octaves), 1.0 / np.sqrt(float(octaves)))
    else:
        raise ValueError(kind)
    return a.astype(np.float32), np.sqrt(1.0 - a * a).astype(np.float32), w.astype(np.float32)


def ladder(n_envs, sigma, sigma_max, env_id0=0):
    """sigma_i = sigma (sigma_max / sigma)^(u_i), u_i = ((env_id0 + i) 2654435761 mod 2^32) / 2^32: float64, stored as fp32 [n_envs]"""
    ids = np.arange(int(env_id0), int(env_id0) + int(n_envs), dtype=np.uint64)
    u = ((ids * np.uint64(LADDER_MULT)) & np.uint64(0xFFFFFFFF)).astype(np.float64) / 4294967296.0
    return (float(sigma) * (float(sigma_max) / float(sigma)) ** u).astype(np.float32)


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------------------
def fill(z, a, b, w, eps, sigma):
    """z [K, 4, n] fp32 (updated in place), eps [steps, K, n, 4] fp32, sigma a scalar or [n] -> out [steps, n, 4] fp32"""
    a, b, w = (np.asarray(v, np.float32) for v in (a, b, w))
    K, _, n = z.shape
    steps = eps.shape[0]
    s = np.broadcast_to(np.asarray(sigma, np.float32), (n,))[:, None]
    out = np.empty((steps, n, 4), np.float32)
    for t in range(steps):
        x = None
        for k in range(K):
            az = (a[k] * z[k]).astype(np.float32)
            be = (b[k] * eps[t, k].T).astype(np.float32)
            z[k] = (az + be).astype(np.float32)
            wz = (w[k] * z[k]).astype(np.float32)
            x = wz if x is None else (x + wz).astype(np.float32)
        out[t] = (s * x.T).astype(np.float32)
    return out


# ---- the draws ---------------------------------------------------------------------------------------------------------------------------------------
def normal4(counter, seed):
    """one Philox call -> four standard-normal draws: u01, then Box-Muller with cos / sin per pair, in float64"""
    u = [((int(v) >> 8) + 0.5) / 16777216.0 for v in philox4x32_10(counter, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))]
    out = []
    for p in (0, 2):
        rad, ang = np.sqrt(-2.0 * np.log(u[p])), 2.0 * np.pi * u[p + 1]
        out += [rad * np.cos(ang), rad * np.sin(ang)]
    return out


def step_counter(row, step, k):
    step = int(step) & 0xFFFFFFFFFFFFFFFF
    return ((int(row)) & 0xFFFFFFFF, step & 0xFFFFFFFF, step >> 32, TAG_STEP | int(k))


def philox_eps(seed, row0, n, poles, step0, steps):
    """the draws hx_noise_fill takes with eps_in = NULL, float64 [steps, poles, n, 4]"""
    out = np.empty((steps, poles, n, 4))
    for t in range(steps):
        for k in range(poles):
            for i in range(n):
                out[t, k, i] = normal4(step_counter(row0 + i, step0 + t, k), seed)
    return out


def philox_init(seed, row0, n, poles):
    """the state hx_noise_init writes, float64 [poles, 4, n]"""
    out = np.empty((poles, 4, n))
    for k in range(poles):
        for i in range(n):
            out[k, :, i] = normal4(((row0 + i) & 0xFFFFFFFF, 0, 0, TAG_INIT | k), seed)
    return out


# ---- what a bank is, analytically --------------------------------------------------------------------------------------------------------------------
def autocorr(a, w, lag):
    """sum_k w[k]^2 a[k]^lag: the autocorrelation of x at `lag` steps (unit variance)"""
    a, w = np.asarray(a, np.float64), np.asarray(w, np.float64)
    return float((w * w * a ** lag).sum())


def spectrum(a, w, f):
    """sum_k w^2 (1 - a^2) / (1 - 2 a cos 2 pi f + a^2) at the frequencies f (cycles per step)"""
    a, w, f = np.asarray(a, np.float64)[:, None], np.asarray(w, np.float64)[:, None], np.asarray(f, np.float64)[None, :]
    return (w * w * (1.0 - a * a) / (1.0 - 2.0 * a * np.cos(2.0 * np.pi * f) + a * a)).sum(0)


def band(poles):
    """the band an octave bank of `poles` poles covers: 1 / (2 pi 2^(poles - 1)) .. 1 / (2 pi) cycles per step"""
    return 1.0 / (2.0 * np.pi * 2.0 ** (poles - 1)), 1.0 / (2.0 * np.pi)


def loglog_slope(a, w, lo, hi, points=64):
    f = np.geomspace(lo, hi, points)
    return float(np.polyfit(np.log(f), np.log(spectrum(a, w, f)), 1)[0])
