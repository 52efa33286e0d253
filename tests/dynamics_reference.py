"""Numpy yardstick of the transient response (test infrastructure, never imported by the package): the Newmark scheme
of include/trs_dynamics.h stated on the oracle's dense K_ff and the lumped masses of `tests/modes_reference.matrices`,
in any floating-point type - `numpy.float64`, or `numpy.longdouble` to measure what float64 itself loses.  The linear
system is solved by a plain elimination without pivoting (K_ff + sigma M is positive definite) written here, so both
types run the same algorithm.  Also the excitations that the CPU and the GPU tests share."""
import numpy as np

from oracle import truss_oracle as orc
from tests import modes_reference as mref


def constants(dt, beta, gamma, damp_mass, damp_stiff, dtype=np.float64):
    """a0 .. a5, s and sigma of the scheme, in `dtype`."""
    dt, beta, gamma, alpha, beta_r = (dtype(x) for x in (dt, beta, gamma, damp_mass, damp_stiff))
    one, two = dtype(1), dtype(2)
    c = {"a0": one / (beta * dt * dt), "a1": gamma / (beta * dt), "a2": one / (beta * dt), "a3": one / (two * beta) - one,
         "a4": gamma / beta - one, "a5": dt / two * (gamma / beta - two)}
    c["s"] = one + c["a1"] * beta_r
    c["sigma"] = (c["a0"] + c["a1"] * alpha) / c["s"]
    return c


class Eliminated:
    """A = L U by plain elimination (no pivoting), kept for any number of `solve` calls."""

    def __init__(self, A):
        self.U = np.array(A, copy=True)
        n = len(A)
        self.Lm = np.zeros_like(self.U)
        for k in range(n - 1):
            f = self.U[k + 1:, k] / self.U[k, k]
            self.Lm[k + 1:, k] = f
            self.U[k + 1:, k:] -= f[:, None] * self.U[k, k:][None, :]

    def solve(self, rhs):
        """x of A x = rhs; rhs [n, L]."""
        x = np.array(rhs, copy=True)
        n = len(x)
        for k in range(n - 1):
            x[k + 1:] -= self.Lm[k + 1:, k][:, None] * x[k][None, :]
        for k in range(n - 1, -1, -1):
            x[k] /= self.U[k, k]
            x[:k] -= self.U[:k, k][:, None] * x[k][None, :]
        return x


def member_forces(data, u, dtype=np.float64):
    """N [.., nM] = E A / len c . (u_j1 - u_j0) for displacements u [.., nJ, dim], tension positive."""
    p = orc.prepare(data)
    pos = np.asarray(p.pos, dtype=dtype)
    out = np.zeros(u.shape[:-2] + (len(p.members),), dtype=dtype)
    for m, (j0, j1, a, e, _rho) in enumerate(p.members):
        d = pos[j1] - pos[j0]
        length = np.sqrt((d * d).sum())
        out[..., m] = dtype(e) * dtype(a) / length * ((u[..., j1, :] - u[..., j0, :]) * (d / length)).sum(-1)
    return out


def newmark(data, pattern, dt, steps, scale=None, accel=None, beta=0.25, gamma=0.5, damp_mass=0.0, damp_stiff=0.0,
            joint_mass=None, mass_scale=1.0, dtype=np.float64):
    """The response of one truss to L excitations from rest.  pattern [L, nJ, dim], scale [L, steps + 1] or None,
    accel [L, steps + 1, dim] or None, in the JSON's joint numbering.  Returns a dict: the histories u, v, a
    [L, steps + 1, nJ, dim] (zero at held DOFs) and N [L, steps + 1, nM], and the envelopes of the device's definition -
    u_peak, u_step [L, nJ, dim], N_max, N_max_step, N_min, N_min_step [L, nM] (the first time point that attains an
    extreme)."""
    p = orc.prepare(data)
    K64, m64, mask = mref.matrices(data, joint_mass, mass_scale)
    K, m = K64.astype(dtype), m64.astype(dtype)
    nJ, dim, n = len(p.pos), p.dim, len(m64)
    pattern = np.asarray(pattern, dtype=dtype)
    L, T1 = pattern.shape[0], steps + 1
    P = pattern.reshape(L, nJ * dim)[:, mask].T                                   # [n, L]
    sc = np.ones([L, T1], dtype=dtype) if scale is None else np.asarray(scale, dtype=dtype)
    axis = (np.arange(nJ * dim) % dim)[mask]
    ag = None if accel is None else np.asarray(accel, dtype=dtype)[:, :, axis].transpose(2, 0, 1)   # [n, L, T1]
    c = constants(dt, beta, gamma, damp_mass, damp_stiff, dtype)
    dt, gamma, alpha, beta_r = dtype(dt), dtype(gamma), dtype(damp_mass), dtype(damp_stiff)
    A = K.copy()
    A[np.arange(n), np.arange(n)] += c["sigma"] * m
    fac = Eliminated(A)

    def load(k):
        f = sc[:, k][None, :] * P
        return f if ag is None else f - m[:, None] * ag[:, :, k]

    u = np.zeros([n, L], dtype=dtype)
    v = np.zeros([n, L], dtype=dtype)
    a = np.where(m[:, None] > 0, load(0) / np.where(m > 0, m, dtype(1))[:, None], dtype(0))
    hist = {k: np.zeros([L, T1, nJ * dim], dtype=dtype) for k in "uva"}
    for key, x in (("u", u), ("v", v), ("a", a)):
        hist[key][:, 0, mask] = x.T
    for k in range(1, T1):
        rhs = load(k) + m[:, None] * ((c["a0"] + alpha * c["a1"]) * u + (c["a2"] + alpha * c["a4"]) * v
                                      + (c["a3"] + alpha * c["a5"]) * a)
        if damp_stiff > 0:
            rhs = rhs + beta_r * (K @ (c["a1"] * u + c["a4"] * v + c["a5"] * a))
        u_new = fac.solve(rhs / c["s"])
        a_new = c["a0"] * (u_new - u) - c["a2"] * v - c["a3"] * a
        v = v + dt * ((dtype(1) - gamma) * a + gamma * a_new)
        u, a = u_new, a_new
        for key, x in (("u", u), ("v", v), ("a", a)):
            hist[key][:, k, mask] = x.T
    out = {k: x.reshape(L, T1, nJ, dim) for k, x in hist.items()}
    out["N"] = member_forces(data, out["u"], dtype)
    mag = np.abs(out["u"])
    out.update(u_peak=mag.max(1), u_step=mag.argmax(1).astype(np.int32), N_max=out["N"].max(1),
               N_max_step=out["N"].argmax(1).astype(np.int32), N_min=out["N"].min(1),
               N_min_step=out["N"].argmin(1).astype(np.int32))
    return out


def first_frequency(data):
    """omega_1 of the truss (lumped mass, every free DOF with mass)."""
    K_ff, m, _ = mref.matrices(data)
    return float(np.sqrt(mref.eigenvalues(K_ff, m)[0]))


COMPARED = ("u", "v", "a", "N")


def relative_difference(x, y):
    """The largest max-scaled difference between two `newmark` results over the histories of u, v, a and N."""
    worst = 0.0
    for key in COMPARED:
        scale = float(np.abs(y[key]).max())
        if scale > 0:
            worst = max(worst, float(np.abs(x[key].astype(np.longdouble) - y[key]).max()) / scale)
    return worst


def excitation(datas, L, steps, dt, omega, seed):
    """The excitations of the parity tests for a batch of trusses, L cases each, in the JSON's numbering, padded to the
    batch: pattern [B, L, nJ_max, 3], scale [B, L, steps + 1], accel [B, L, steps + 1, 3].  Case l cycles through three
    kinds: 0 a step load (a random pattern on every joint, scale 1), 1 the same kind of pattern under
    sin(sqrt 2 omega t + 0.3), 2 no load but a ground acceleration with components of three frequencies irrational to
    one another.  Patterns and amplitudes are drawn per (truss, case) from `seed`; z stays zero on a 2D truss."""
    B, nJ_max = len(datas), max(len(d["joint"]) for d in datas)
    t = dt * np.arange(steps + 1)
    pattern = np.zeros([B, L, nJ_max, 3])
    scale = np.ones([B, L, steps + 1])
    accel = np.zeros([B, L, steps + 1, 3])
    for b, data in enumerate(datas):
        nJ, dim = len(data["joint"]), orc.truss_dim(data)
        for l in range(L):
            rng = np.random.default_rng([seed, b, l])          # (case l of truss b does not depend on B or L)
            draw = rng.uniform(-1.0, 1.0, size=[nJ, 3])
            amp = rng.uniform(0.5, 1.5, size=3)
            kind = l % 3
            if kind < 2:
                pattern[b, l, :nJ, :dim] = 1000.0 * draw[:nJ, :dim]
            if kind == 1:
                scale[b, l] = np.sin(np.sqrt(2.0) * omega * t + 0.3)
            if kind == 2:
                waves = np.stack([np.sin(np.sqrt(3.0) * omega * t + 0.1), np.cos(np.sqrt(5.0) * omega * t),
                                  np.sin(np.sqrt(0.7) * omega * t + 1.0)], axis=-1)
                accel[b, l, :, :dim] = (100.0 * amp * waves)[:, :dim]
    return pattern, scale, accel


#: the ragged default batch of the GPU tests: 2D and 3D, padding joints and members, n_free no multiple of 64
BATCH = ("bar-10_input_0", "bar-25_input_0", "bar-47_input_0", "cube-7_case_3")
BIG = "bar-942_input_0"
SEED = 20260


def setting(datas, damped):
    """(dt, omega, damp_mass, damp_stiff) of the parity tests for a batch: omega the largest fundamental frequency of its
    trusses, 20 steps per period of it, and - `damped` - alpha = 0.05 omega, beta_R = 0.02 / omega."""
    omega = max(first_frequency(d) for d in datas)
    return 2.0 * np.pi / (20.0 * omega), omega, (0.05 * omega if damped else 0.0), (0.02 / omega if damped else 0.0)


def reference(datas, L, steps, damped, dtype=np.float64, seed=SEED):
    """The yardstick's results for every truss of a batch under `excitation` and `setting`: a list of `newmark` dicts."""
    dt, omega, alpha, beta_r = setting(datas, damped)
    pattern, scale, accel = excitation(datas, L, steps, dt, omega, seed)
    out = []
    for b, data in enumerate(datas):
        nJ, dim = len(data["joint"]), orc.truss_dim(data)
        out.append(newmark(data, pattern[b, :, :nJ, :dim], dt, steps, scale[b], accel[b, :, :, :dim], damp_mass=alpha,
                           damp_stiff=beta_r, dtype=dtype))
    return out
