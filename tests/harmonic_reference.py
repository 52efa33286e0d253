"""Numpy reference of the harmonic response analysis (test infrastructure, never imported by the package): a plain
restatement of include/trs_harmonic.h on the shapes and eigenvalues it is GIVEN, in float64 or longdouble, built on the
arrays and the system of `tests/mode_gradients_reference.py` / `tests/spectrum_reference.py`; the same on `eigh`'s pairs;
and the direct complex solve of the damped system, which needs no modes at all."""
import numpy as np

from tests import mode_gradients_reference as G
from tests import spectrum_reference as SR

KEYS = ("u", "N", "R")


def load(d, pattern=None, ag=None, mass_scale=1.0, dtype=np.float64):
    """f = P - M iota(ag) in joint layout [nJ, 3], zero at held DOFs: `pattern` [nJ, 3] or None, `ag` [3] or None."""
    nJ = len(d["xyz"])
    free = d["free"]
    f = np.zeros([nJ, 3], dtype)
    if pattern is not None:
        f += np.asarray(pattern, dtype=dtype)[:nJ]
    if ag is not None:
        m = np.zeros(3 * nJ, dtype)
        m[free.ravel()] = SR.system(d, mass_scale, dtype)[1]
        f -= m.reshape(nJ, 3) * np.asarray(ag, dtype=dtype)[None, :]
    f[~free] = 0
    return f


def _members(d, dtype):
    f = lambda x: np.asarray(x, dtype=dtype)
    xyz, conn = f(d["xyz"]), d["conn"]
    D = xyz[conn[:, 1]] - xyz[conn[:, 0]]
    length = np.sqrt((D * D).sum(1))
    return conn[:, 0], conn[:, 1], D / length[:, None], f(d["E"]) * f(d["A"]) / length


def forces(d, u, dtype=np.float64):
    """(N [..., nM], R [..., nJ, 3]) of displacement vectors u [..., nJ, 3] (real or complex): N = k c . (u_j1 - u_j0),
    R the sum of the member end forces in member-id order, zero at free DOFs."""
    j0, j1, c, k = _members(d, dtype)
    N = k * ((u[..., j1, :] - u[..., j0, :]) * c).sum(-1)
    R = np.zeros(u.shape, u.dtype)
    for mm in range(len(j0)):     # member-id order
        R[..., j1[mm], :] += N[..., mm, None] * c[mm]
        R[..., j0[mm], :] -= N[..., mm, None] * c[mm]
    R[..., d["free"]] = 0
    return N, R


def envelope(y):
    """(the largest modulus over the leading axis, the FIRST index that attains it) of complex y [S, ...]."""
    amp = np.sqrt(y.real * y.real + y.imag * y.imag)
    return amp.max(0), amp.argmax(0).astype(np.int32)


def _finish(out):
    for key in KEYS:
        out[key + "_amp"], out[key + "_at"] = envelope(out[key])
    return out


def response(d, phi, lam, omegas, f, zeta=0.02, damp_mass=0.0, damp_stiff=0.0, residual=True, mass_scale=1.0,
             dtype=np.float64):
    """include/trs_harmonic.h for the shapes `phi` [p, nJ, 3] (joint layout, M-orthonormal, zero at held DOFs) and the
    eigenvalues `lam` [p] as given (a NaN or non-positive one contributes nothing), the forcing frequencies `omegas`
    [S] and ONE load `f` [nJ, 3] (`load`), evaluated in `dtype`.  Returns a dict: the complex u, R [S, nJ, 3] and N
    [S, nM] at every frequency, their envelopes u_amp, N_amp, R_amp with the first indices u_at, N_at, R_at, the modal
    loads g [p] and u_res [nJ, 3]."""
    cplx = np.complex128 if dtype is np.float64 else np.clongdouble
    fl = lambda x: np.asarray(x, dtype=dtype)
    phi, lam, W, f = fl(phi), fl(lam), fl(omegas), fl(f)
    p, nJ = len(lam), len(d["xyz"])
    free = d["free"].ravel()
    K_ff, m = SR.system(d, mass_scale, dtype)
    X = phi.reshape(p, -1)[:, free]
    fr = f.reshape(-1)[free]
    live = np.isfinite(lam.astype(np.float64)) & (lam > 0)
    g = np.zeros(p, dtype)
    rest = fr.copy()
    for k in range(p):
        if live[k]:
            g[k] = (X[k] * fr).sum()
            rest = rest - g[k] * (m * X[k])
    u_res = np.zeros(3 * nJ, dtype)
    if residual:
        u_res[free] = SR.solve(K_ff, rest, dtype)
    u_res = u_res.reshape(nJ, 3)
    u = np.zeros([len(W), nJ, 3], cplx)
    u += u_res
    half, two = dtype(0.5), dtype(2)
    for k in range(p):
        if not live[k]:
            continue
        w = np.sqrt(lam[k])
        zk = dtype(zeta) + dtype(damp_mass) / (two * w) + dtype(damp_stiff) * w * half
        dr = lam[k] - W * W
        di = two * zk * w * W
        n2 = dr * dr + di * di
        c = (g[k] * (dr / n2)).astype(cplx) + cplx(1j) * (g[k] * (-di / n2)).astype(cplx)
        u += c[:, None, None] * phi[k].astype(cplx)
    N, R = forces(d, u, dtype)
    return _finish({"u": u, "N": N, "R": R, "g": g, "u_res": u_res})


def exact_response(d, p, omegas, f, mass_scale=1.0, **kw):
    """`response` with the p lowest pairs of `eigh` (fewer when the truss has fewer)."""
    lam, Phi = G.eigen_pairs(d, mass_scale, p)
    return response(d, Phi, lam[:len(Phi)], omegas, f, mass_scale=mass_scale, **kw)


def direct(d, omegas, f, damp_mass=0.0, damp_stiff=0.0, mass_scale=1.0):
    """The complex solve (K - W^2 M + i W (damp_mass M + damp_stiff K)) U = f at every frequency (float64): no modes."""
    K_ff, m = G.system(d, mass_scale)
    nJ = len(d["xyz"])
    free = d["free"].ravel()
    fr = np.asarray(f, dtype=float).reshape(-1)[free]
    u = np.zeros([len(omegas), 3 * nJ], np.complex128)
    for s, W in enumerate(np.asarray(omegas, dtype=float)):
        Z = K_ff - W * W * np.diag(m) + 1j * W * (damp_mass * np.diag(m) + damp_stiff * K_ff)
        u[s, free] = np.linalg.solve(Z, fr.astype(np.complex128))
    u = u.reshape(len(omegas), nJ, 3)
    N, R = forces(d, u)
    return _finish({"u": u, "N": N, "R": R})
