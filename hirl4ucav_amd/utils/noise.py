"""Temporally correlated exploration noise (an extension: the reference's chooseAction draws white Gaussian noise, HIRL.py:192-212).

White noise on control-surface levels averages out within a few ticks of the 6-DoF integrator; the standard remedy for continuous control is noise that
is correlated in time — DDPG's Ornstein-Uhlenbeck process, or 1 / f ("pink") noise (Eberhard et al., ICLR 2023).  ColoredNoise owns the state of
hx_noise_fill (hx_noise.hip): per env and action component a bank of stationary AR(1) processes whose coefficients are the recipes below; one launch
fills `chunk` vector steps, next() hands out the [n, 4] slice of the current step — the tensor noise_mode 2 of the acting kernels and the Gaussian head's
eps take.  A ladder of noise scales over the population (sigma_max, after Ape-X) is fixed per env id.  The rule is stated in include/hirl4ucav.h
("Exploration noise"); the helpers in front of the class are host-only.  Whether coloured noise helps these agents learn has not been measured.
"""
import math

from .. import _lib

MAX_POLES, MAX_STEPS = (_lib.DEFINES[k] for k in ("HX_NOISE_MAX_POLES", "HX_NOISE_MAX_STEPS"))
KINDS = ("white", "ou", "pink")
LADDER_MULT = 2654435761  # Knuth's multiplicative hash: consecutive env ids land far apart in [0, 1)


# ---- host-only helpers (plain values: unit-tested without a GPU) ----------------------------------------------------------------------------
def coefficients(kind, tau=16.0, octaves=6):
    """-> (a, b, w), three lists of K floats computed in float64 (the caller stores them as fp32): white K = 1, a = 0; ou K = 1, a = exp(-1 / tau); pink
    K = octaves, a[k] = exp(-2^-k), w[k] = 1 / sqrt(K).  b = sqrt(1 - a^2) and sum w^2 = 1: unit variance for every pole and for their sum."""
    if kind == "white":
        a, w = [0.0], [1.0]
    elif kind == "ou":
        if not (math.isfinite(tau) and tau > 0):
            raise ValueError(f"tau {tau}: the correlation time of the OU process, in vector steps, > 0")
        a, w = [math.exp(-1.0 / tau)], [1.0]
    elif kind == "pink":
        if not 1 <= int(octaves) <= MAX_POLES:
            raise ValueError(f"octaves {octaves}: the poles of the 1 / f bank, 1..{MAX_POLES}")
        a, w = [math.exp(-(2.0 ** -k)) for k in range(int(octaves))], [1.0 / math.sqrt(int(octaves))] * int(octaves)
    else:
        raise ValueError(f"kind {kind!r}: one of {', '.join(KINDS)}")
    return a, [math.sqrt(1.0 - v * v) for v in a], w


def lag_autocorr(a, w, lag=1):
    """sum w[k]^2 a[k]^lag: the analytic autocorrelation of the bank's output at `lag` vector steps"""
    return sum(wk * wk * ak ** lag for ak, wk in zip(a, w))


def sigma_ladder(n_envs, sigma, sigma_max, env_id0=0):
    """sigma_i = sigma (sigma_max / sigma)^(u_i), u_i = ((env_id0 + i) 2654435761 mod 2^32) / 2^32 in float64 -> a list of n_envs floats: fixed per env
    id (a rank's envs get what they would get in one population) and uncorrelated with --env mixed's sorted thirds"""
    if not (math.isfinite(sigma) and math.isfinite(sigma_max) and 0 < sigma <= sigma_max):
        raise ValueError(f"sigma {sigma}, sigma_max {sigma_max}: the ladder runs from sigma > 0 up to sigma_max >= sigma")
    ratio = sigma_max / sigma
    return [sigma * ratio ** ((((env_id0 + i) * LADDER_MULT) & 0xFFFFFFFF) / 4294967296.0) for i in range(int(n_envs))]


class ColoredNoise:
    """next() -> the [n_envs, 4] noise of the current vector step, a view of the chunk (valid until the chunk is refilled: `chunk` calls later).  Every
    `chunk` calls one hx_noise_fill; the 64-bit step counter keys the Philox draws, so the process is a function of (seed, env id, step) and of nothing
    else: chunk size, env count and the split over ranks change no value.  Episodes do not reset the state (a stationary process continued across an
    auto-reset is a stationary draw for the new episode).  Everything only enqueues on the current torch stream."""

    def __init__(self, n_envs, kind, *, tau=16.0, octaves=6, sigma=0.1, sigma_max=None, seed, env_id0=0, chunk=16, device):
        import torch

        if not 1 <= int(n_envs) < 2 ** 31:
            raise ValueError(f"n_envs {n_envs}: 1 <= n_envs < 2^31")
        if not 1 <= int(chunk) <= MAX_STEPS:
            raise ValueError(f"chunk {chunk}: the vector steps of one fill, 1..{MAX_STEPS}")
        if not (math.isfinite(sigma) and sigma >= 0):
            raise ValueError(f"sigma {sigma}: the noise scale, >= 0")
        a, b, w = coefficients(kind, tau, octaves)
        self.params = {"kind": kind, "tau": float(tau), "octaves": int(octaves), "sigma": float(sigma), "sigma_max": None if sigma_max is None else float(sigma_max),
                       "seed": int(seed), "env_id0": int(env_id0), "chunk": int(chunk), "n_envs": int(n_envs)}
        self.n, self.poles, self.sigma, self.seed, self.env_id0, self.chunk = int(n_envs), len(a), float(sigma), int(seed), int(env_id0), int(chunk)
        self.a, self.b, self.w = a, b, w
        self.coef = torch.zeros((3, MAX_POLES), dtype=torch.float32)  # host: a | b | w as fp32
        for r, row in enumerate((a, b, w)):
            self.coef[r, :self.poles] = torch.tensor(row, dtype=torch.float64).to(torch.float32)
        self.device = torch.device(device)
        self.sigma_env = None
        if sigma_max is not None:
            self.sigma_env = torch.tensor(sigma_ladder(self.n, self.sigma, float(sigma_max), self.env_id0), dtype=torch.float64).to(torch.float32).to(self.device)
        words = int(_lib.load().hx_noise_workspace_floats(self.n, self.poles))
        if words != 4 * self.poles * self.n:
            raise _lib.HxError(f"ABI mismatch: the noise state is {4 * self.poles * self.n} floats here, {words} in {_lib.SO_PATH}")
        self.z = torch.zeros(words, dtype=torch.float32, device=self.device)
        self.out = torch.zeros((self.chunk, self.n, 4), dtype=torch.float32, device=self.device)
        self.step = 0              # vector steps handed out so far: the Philox counter of the next fill is the step its first slice belongs to
        self.cursor = self.chunk   # slice of `out` the next call returns; == chunk: refill first
        _lib.call("hx_noise_init", self.z.data_ptr(), self.n, self.poles, self.seed, self.env_id0, _lib.stream_ptr())

    def sigma_range(self):
        """(smallest, largest) per-env scale"""
        if self.sigma_env is None:
            return self.sigma, self.sigma
        return float(self.sigma_env.min()), float(self.sigma_env.max())

    def fill(self, step0, steps, out, eps_in=None, eps_out=None):
        """`steps` vector steps from step `step0` on into out [steps, n, 4] (one launch); z advances"""
        _lib.call("hx_noise_fill", self.z.data_ptr(), _lib.ptr(self.sigma_env), self.n, self.poles, self.sigma, self.coef.data_ptr(), self.seed, self.env_id0,
                  int(step0) & (2 ** 64 - 1), int(steps), out.data_ptr(), _lib.ptr(eps_in), _lib.ptr(eps_out), _lib.stream_ptr())

    def next(self):
        if self.cursor == self.chunk:
            self.fill(self.step, self.chunk, self.out)
            self.cursor = 0
        view = self.out[self.cursor]
        self.cursor += 1
        self.step += 1
        return view

    def state_dict(self):
        return {"params": dict(self.params), "z": self.z.cpu().clone(), "out": self.out.cpu().clone(), "cursor": self.cursor, "step": self.step}

    def load_state_dict(self, st):
        if st["params"] != self.params:
            diff = sorted(k for k in self.params if st["params"].get(k) != self.params[k])
            raise ValueError("snapshot's exploration noise was written under " + ", ".join(f"{k} {st['params'].get(k)}" for k in diff) + "; this generator has "
                             + ", ".join(f"{k} {self.params[k]}" for k in diff))
        self.z.copy_(st["z"])
        self.out.copy_(st["out"])
        self.cursor, self.step = int(st["cursor"]), int(st["step"])
