"""Models, inputs and checks shared by tests/test_rollout_host.py (CPU) and tests/test_gpu_rollout.py -- TEST INFRASTRUCTURE ONLY."""
import numpy as np

from optimal_control_problem_amd import models

from tests.support.advance_cases import pendulum

HORIZONS = (2, 3, 20)
BATCHES = (1, 63, 64, 65, 130)      # across the wave and the workgroup boundary of one thread per instance in 64-thread workgroups


class Blowup(models.StageOCP):
    """nx = nu = 1, F = s s 1e150 + u: from s_0 = 1 the second step leaves the finite numbers (1e150 squared), from s_0 = 0 nothing happens"""
    nx, nu, name = 1, 1, "blowup"

    def F(self, s, u):
        return np.stack([s[..., 0] * s[..., 0] * 1e150 + u[..., 0]], axis=-1)


def blowup(N=5):
    return Blowup(N, 0.1, Q=[1.0], R=[1.0])


def zoo(name, N):
    return {"double_integrator": models.DoubleIntegrator, "quadrotor": models.Quadrotor, "cartpole": models.CartPole}[name](N)


def model(name, N):
    return pendulum(N) if name == "pendulum" else zoo(name, N)


MODELS = ("double_integrator", "cartpole", "quadrotor", "pendulum")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def inputs(mdl, B, seed=0):
    """(x, lbx, ubx): a random iterate whose first frame and inputs partly lie outside the box (so the clip acts), the first frame of
    every third instance pinned through lbx = ubx, and the states of the frames k >= 1 NaN: the rule may not read them.
    The quadrotor's input box is drawn tight around hover (+-2 %, inputs spread 3 %) instead of the model's [0, 2 hover]: a rotor held at 0 or at
    twice hover for the whole horizon is 49 rad/s^2 of body acceleration, the pitch passes pi / 2 inside 20 frames, and F -- which divides by
    cos(pitch) -- is then so badly conditioned that no two libms agree to 1e-12 in one step.  The per-step bar belongs to the regime
    tests/test_gpu_advance.py draws (attitudes of a few tenths of a radian); with the tight box the held input tilts the vehicle by 0.2 rad."""
    rng = np.random.default_rng(1000 * mdl.N + 7 * B + seed + mdl.nx)
    X = rng.normal(0.0, 0.3, size=(B, mdl.N, mdl.f))
    tight = None
    if mdl.name == "quadrotor":
        X[:, :, mdl.nx:] = mdl.hover_thrust * (1.0 + rng.normal(0.0, 0.03, size=(B, mdl.N, mdl.nu)))      # about half outside hover +- 2 %
        tight = (0.98 * mdl.hover_thrust, 1.02 * mdl.hover_thrust)
    elif mdl.name == "cartpole":
        X[:, :, mdl.nx:] = rng.normal(0.0, 15.0, size=(B, mdl.N, mdl.nu))                                 # some outside +-20
        X[:, 0, 0] = rng.normal(0.0, 2.0, size=B)                                                         # some outside +-2.4
    else:
        X[:, :, mdl.nx:] = rng.normal(0.0, 1.5, size=(B, mdl.N, mdl.nu))
    frame0 = X[:, 0].copy()
    lbx, ubx, _, _ = mdl.stacked_bounds(frame0)
    lo, hi = mdl.frame_bounds()
    if tight is not None:
        lo, hi = lo.copy(), hi.copy()
        lo[mdl.nx:], hi[mdl.nx:] = tight
        lbx = np.tile(lo, (B, mdl.N)); ubx = np.tile(hi, (B, mdl.N))
        lbx[:, :mdl.f] = frame0; ubx[:, :mdl.f] = frame0
    free = np.arange(B) % 3 != 0
    lbx[free, :mdl.f] = lo; ubx[free, :mdl.f] = hi
    X[:, 1:, :mdl.nx] = np.nan
    return X.reshape(B, -1), lbx, ubx


def clip(v, lo, hi):
    v = np.where(v < lo, lo, v)
    return np.where(v > hi, hi, v)


def check_rule(mdl, x_in, lbx, ubx, mode, out, step_tol=0.0, rows=None):
    """the rule of mpcqp_stage_rollout on `out` = the x it produced: the first frame and the inputs bitwise the clip, every state within
    step_tol * max(1, |ref|) of F at out's own previous frame (0: bitwise).  rows: per-instance parameter rows, else the model's shared ones."""
    B, N, nx, f = x_in.shape[0], mdl.N, mdl.nx, mdl.f
    X = x_in.reshape(B, N, f); O = np.asarray(out).reshape(B, N, f)
    Lo = lbx.reshape(B, N, f); Hi = ubx.reshape(B, N, f)
    assert np.array_equal(bits(O[:, 0]), bits(clip(X[:, 0], Lo[:, 0], Hi[:, 0])))
    for k in range(1, N):
        u_in = O[:, 0, nx:] if mode == "hold" else X[:, k, nx:]
        assert np.array_equal(bits(O[:, k, nx:]), bits(clip(u_in, Lo[:, k, nx:], Hi[:, k, nx:]))), k
    for k in range(N - 1):
        if rows is None:
            ref = mdl.F(O[:, k, :nx], O[:, k, nx:])
        else:
            saved = np.array(mdl.theta, float)
            try:
                ref = np.empty((B, nx))
                for b in range(B):
                    mdl.theta = rows[b].copy()
                    ref[b] = mdl.F(O[b:b + 1, k, :nx], O[b:b + 1, k, nx:])[0]
            finally:
                mdl.theta = saved
        if step_tol == 0.0:
            assert np.array_equal(bits(O[:, k + 1, :nx]), bits(ref)), k
        else:
            err = np.abs(O[:, k + 1, :nx] - ref) / np.maximum(1.0, np.abs(ref))
            assert np.isfinite(O[:, k + 1, :nx]).all() and err.max() <= step_tol, (k, err.max())


def cartpole_rows(B):
    """per-instance cart-pole parameters {mc, mp, length, grav}: masses and lengths spread around the defaults"""
    rng = np.random.default_rng(5 + B)
    base = np.array([1.0, 0.1, 0.5, 9.81])
    return base * (1.0 + rng.uniform(-0.3, 0.3, size=(B, 4)) * np.array([1.0, 1.0, 1.0, 0.0]))


def recipe(batch=4):
    """cart-pole N = 100 hanging down, the workload's own seed: (model, meta) of models.make_workload"""
    mdl, _, meta = models.make_workload("cartpole", batch, N=100)
    return mdl, meta
