"""Float64 restatement of the tone map (Reinhard + gamma, simple_raytracer.cpp:391-398) and of the quantiser (:447-449), and the
inputs where an implementation of them goes wrong.  Shared by the device test (tests/test_gpu_modes.py) and the oracle's
(tests/test_oracle_golden.py)."""
import numpy as np

REINHARD = (0.2, 0.5, 4.0)
GAMMA = (0.4545, 1.0, 1.1, 2.0, 2.2, 64.0, 65.0)


def tone_ref(lin, reinhard, gamma):
    """c / (c + r) in float32 (as tone1), the power in float64, rounded once to float32."""
    c = np.asarray(lin, np.float32)
    with np.errstate(all="ignore"):
        ratio = c / (c + np.float32(reinhard))
        return np.power(ratio.astype(np.float64), np.float64(np.float32(gamma))).astype(np.float32)


def pow_device_ref(x, y):
    """The device's pow as the oracle's device mode restates it (simple_raytracer_amd/csrc/srt_device.h pow_like_host): x^e for an
    integer e in [1, 64] and x in (1e-30, 1e30) by square-and-multiply in float64 with one rounding, otherwise the float64 pow
    rounded once.  Elementwise over float32 arrays."""
    x = np.asarray(x, np.float32); y = np.broadcast_to(np.asarray(y, np.float32), x.shape)
    with np.errstate(all="ignore"):
        out = np.power(x.astype(np.float64), y.astype(np.float64)).astype(np.float32)
        small = (x > np.float32(1e-30)) & (x < np.float32(1e30)) & (y >= 1) & (y <= 64) & (y == np.trunc(y))
        r, b = np.ones(x.shape, np.float64), x.astype(np.float64)
        e = np.where(small, y, 0).astype(np.int64)
        while e.any():
            r = np.where(e & 1, r * b, r)
            b = b * b
            e >>= 1
        return np.where(small, r.astype(np.float32), out)


def quant_ref(tone):
    """int(c * 255) with the product in float32, clamped to [0, 255], NaN -> 0."""
    with np.errstate(all="ignore"):
        s = np.asarray(tone, np.float32) * np.float32(255.0)
        q = np.where(s > 0, s, 0).astype(np.float64)
    return np.floor(np.minimum(q, 255.0)).astype(np.int32)


def ulp_diff(a, b):
    """Distance in units in the last place between float32 arrays (NaN vs NaN = 0, NaN vs a number = a huge distance)."""
    def key(x):
        i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    na, nb = np.isnan(a), np.isnan(b)
    d = np.abs(key(a) - key(b))
    return np.where(na & nb, 0, np.where(na | nb, 1 << 40, d))


def inputs(reinhard, gamma, n_random=60000, seed=0):
    """Linear colours for one (reinhard, gamma): zeros and denormals, ratios c / (c + r) that straddle pow's 1e-30 cut-off, ratios
    whose gamma * log2 lands near -1000 and +1000 (c just below -r gives ratios far above 1), inf, NaN and negative values, and a
    spread of ordinary values."""
    r = np.float32(reinhard)
    g = float(np.float32(gamma))
    rng = np.random.default_rng(seed)
    special = [0.0, -0.0, 1e-45, -1e-45, 1e-40, 1.17e-38, 1e-38, 3e-39, np.inf, -np.inf, np.nan, -1.0, -0.1, -r, -2 * r, 1.0, 1e30, 3e38, -3e38]
    cut = np.float32(1e-30) * r * (1.0 + np.linspace(-1e-6, 1e-6, 41))                      # ratio ~ 1e-30
    z = []
    for target in (-1000.0, 1000.0):
        with np.errstate(all="ignore"):
            x = 2.0 ** (target / g * (1.0 + np.linspace(-2e-3, 2e-3, 41)))                # the ratio that makes g * log2(ratio) ~ target
            c = np.where(x < 1, x * r / (1 - x), -r * x / (x - 1))                          # c / (c + r) = x
        z.append(c[np.isfinite(c)])
    ordinary = np.concatenate([rng.uniform(0, 4, n_random), rng.exponential(0.3, n_random // 2), 10.0 ** rng.uniform(-30, 6, n_random // 2),
                               -rng.uniform(0, 2 * r, n_random // 4)])
    lin = np.concatenate([np.array(special, np.float64), cut, *z, ordinary]).astype(np.float32)
    pad = (-lin.shape[0]) % 3
    return np.concatenate([lin, np.zeros(pad, np.float32)]).reshape(-1, 3)
