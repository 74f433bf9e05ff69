"""fp64 numpy restatement of mapdit_amd.flow (rectified flow on a timestep grid), written from the mathematics and shared by
tests/test_flow_cpu.py and tests/test_flow_gpu.py.  Nothing here imports the package.

    x_s = (1 - s) x0 + s eps,   velocity eps - x0,   index k <-> s_k = shifted((k + 1) / T),   shifted(s) = shift s / (1 + (shift - 1) s)
"""
import numpy as np

C_DATA = 0.5                     # the exact-solution case: data ~ N(0, c^2 I)


def shifted(s, shift):
    return shift * s / (1.0 + (shift - 1.0) * s)


def sigmas(T, shift):
    s = shifted((np.arange(T, dtype=np.float64) + 1.0) / T, shift)
    s[-1] = 1.0
    return s


def schedule(sig, shift, num_steps, order):
    """-> (steps, h, t, coef, kind) in execution order.  Targets shifted(1 - j / K), j = 0 .. K - 1 (target K is exactly 0: no grid
    point), each replaced by the nearest grid point (np.argmin returns the first, i.e. lowest, index of a tie), duplicates dropped;
    step sizes are differences of the grid values used, the last step ends at 0.  Euler: one committing row (0, h) per step.  Heun: a
    predictor row (0, h) at k_a and a committing row (h / 2, h / 2) at k_b; its final step is an Euler row."""
    steps = []
    for j in range(num_steps):
        k = int(np.argmin(np.abs(sig - shifted(1.0 - j / num_steps, shift))))
        if not steps or k != steps[-1]:
            steps.append(k)
    s_a = [sig[k] for k in steps]
    h = [b - a for a, b in zip(s_a, s_a[1:] + [0.0])]
    t, coef, kind = [], [], []
    for i, k in enumerate(steps):
        if order == 1 or i == len(steps) - 1:
            t.append(k); coef.append((0.0, h[i])); kind.append(0)
        else:
            t.append(k); coef.append((0.0, h[i])); kind.append(1)
            t.append(steps[i + 1]); coef.append((h[i] / 2, h[i] / 2)); kind.append(0)
    return np.array(steps), np.array(h), np.array(t), np.array(coef).reshape(-1, 2), np.array(kind)


def step(base, hist, v, c_h, c_v, predictor):
    """One evaluation: -> (out, new base, new hist, magnitude of the terms)."""
    out = base + c_h * hist + c_v * v
    mag = np.abs(base) + np.abs(c_h * hist) + np.abs(c_v * v)
    return out, (base if predictor else out), (v if predictor else hist), mag


def sample_loop(model, noise, sig, shift, num_steps, order):
    """The whole loop in fp64; model(x, k) -> velocity at grid index k."""
    _, _, t, coef, kind = schedule(sig, shift, num_steps, order)
    x = base = noise.astype(np.float64)
    hist = np.zeros_like(base)
    for k, (c_h, c_v), pred in zip(t, coef, kind):
        x, base, hist, _ = step(base, hist, model(x, int(k)), c_h, c_v, bool(pred))
    return x


def q_sample(x0, eps, s):
    """s: [N] flow times -> (x_s, magnitude of the two terms)."""
    s = s.reshape(-1, *([1] * (x0.ndim - 1)))
    return (1 - s) * x0 + s * eps, np.abs((1 - s) * x0) + np.abs(s * eps)


def loss_and_grad(v_pred, x0, eps):
    """-> (loss [N], G of v_pred's shape = d loss / d v_pred)."""
    diff = v_pred - (eps - x0)
    per = x0[0].size
    return (diff ** 2).reshape(len(x0), -1).mean(axis=1), 2.0 * diff / per


def logit_normal_index(z, loc, scale, T):
    p = 1.0 / (1.0 + np.exp(-(loc + scale * z)))
    return np.minimum(np.floor(p * T), T - 1).astype(np.int64)


def exact_velocity_coef(s, c=C_DATA):
    """Data N(0, c^2 I): E[eps - x0 | x_s = x] = a(s) x with a(s) = (s - (1 - s) c^2) / ((1 - s)^2 c^2 + s^2).  The ODE dx/ds = a(s) x
    has x(s) = x(1) sqrt((1 - s)^2 c^2 + s^2), so x(0) = c x(1)."""
    return (s - (1 - s) * c * c) / ((1 - s) ** 2 * c * c + s * s)
