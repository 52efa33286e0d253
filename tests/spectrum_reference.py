"""Numpy reference of the response spectrum analysis (test infrastructure, never imported by the package): a plain
restatement of include/trs_spectrum.h on the shapes and eigenvalues it is GIVEN, in float64 or longdouble, built on the
arrays, the system and the eigenpairs of `tests/mode_gradients_reference.py`."""
import numpy as np

from tests import mode_gradients_reference as G

RULES = {"srss": 0, "cqc": 1, "abs": 2}
KEYS = ("gamma", "sa", "meff", "mtot", "base", "u", "N", "R", "modal_u", "modal_N", "modal_R")


def system(d, mass_scale=1.0, dtype=np.float64):
    """(K_ff, m) of `mode_gradients_reference.system`, the same operations in `dtype`."""
    if dtype is np.float64:
        return G.system(d, mass_scale)
    f = lambda x: np.asarray(x, dtype=dtype)
    xyz, conn = f(d["xyz"]), d["conn"]
    nJ = len(xyz)
    D = xyz[conn[:, 1]] - xyz[conn[:, 0]]
    length = np.sqrt((D * D).sum(1))
    c = D / length[:, None]
    k = f(d["E"]) * f(d["A"]) / length
    K = np.zeros([nJ, 3, nJ, 3], dtype)
    blocks = k[:, None, None] * c[:, :, None] * c[:, None, :]
    for (j0, j1), blk in zip(conn, blocks):
        K[j0, :, j0] += blk
        K[j1, :, j1] += blk
        K[j0, :, j1] -= blk
        K[j1, :, j0] -= blk
    half = dtype(0.5) * (f(d["A"]) * length * f(d["rho"]))
    mj = np.zeros(nJ, dtype)
    np.add.at(mj, conn[:, 0], half)
    np.add.at(mj, conn[:, 1], half)
    mj = dtype(mass_scale) * mj + f(d["joint_mass"])
    free = d["free"].ravel()
    K = K.reshape(3 * nJ, 3 * nJ)
    return K[free][:, free], np.repeat(mj, 3)[free]


def solve(K, f, dtype=np.float64):
    """inv(K) f; in longdouble by iterative refinement of the float64 solution with residuals formed in longdouble."""
    if dtype is np.float64:
        return np.linalg.solve(K, f)
    K64 = K.astype(np.float64)
    x = np.linalg.solve(K64, f.astype(np.float64)).astype(dtype)
    for _ in range(4):
        r = f - K @ x
        x = x + np.linalg.solve(K64, r.astype(np.float64)).astype(dtype)
    return x


def spectrum_at(T, Sa, Tk):
    """The table of one direction at period Tk: linear between the points, constant outside them."""
    K = len(T)
    if not Tk >= T[0]:
        return Sa[0]
    if Tk >= T[K - 1]:
        return Sa[K - 1]
    i = max(j for j in range(K - 1) if T[j] <= Tk)
    t = (Tk - T[i]) / (T[i + 1] - T[i])
    return t * (Sa[i + 1] - Sa[i]) + Sa[i]


def cqc_rho(wi, wj, zeta):
    b = wj / wi
    return 8 * zeta * zeta * (1 + b) * b ** 1.5 / ((1 - b * b) ** 2 + 4 * zeta * zeta * b * (1 + b) ** 2)


def correlations(omega, live, zeta, rule, dtype=np.float64):
    """rho [p + 1, p + 1]: the modes' block (identity for SRSS and ABS, 0 where a mode contributes nothing) and the
    missing-mass slot, correlated with itself alone."""
    p = len(omega)
    rho = np.zeros([p + 1, p + 1], dtype)
    for i in range(p):
        for j in range(p):
            if live[i] and live[j]:
                rho[i, j] = 1 if i == j else cqc_rho(omega[i], omega[j], dtype(zeta)) if rule == "cqc" else 0
    rho[p, p] = 1
    return rho


def combine(rho, r, rule):
    """sqrt(max(0, sum_ij rho_ij r_i r_j)) over the leading axis of r, or sum_i |r_i|."""
    if rule == "abs":
        return np.abs(r).sum(0)
    s = np.einsum("ij,i...,j...->...", rho, r, r)
    return np.sqrt(np.maximum(s, 0))


def response(d, phi, lam, dirs, T, Sa, zeta=0.05, rule="cqc", missing_mass=True, zpa=None, mass_scale=1.0,
             dtype=np.float64):
    """include/trs_spectrum.h for the shapes `phi` [p, nJ, 3] (joint layout, M-orthonormal, zero at held DOFs) and the
    eigenvalues `lam` [p] as given (a NaN or non-positive one contributes nothing), evaluated in `dtype`.  Returns a
    dict: gamma, sa, meff [G, p], mtot, base [G], u, R [G, nJ, 3], N [G, nM], modal_u, modal_R [G, p + 1, nJ, 3],
    modal_N [G, p + 1, nM], modal_base [G, p + 1] and the correlations rho [p + 1, p + 1]."""
    f = lambda x: np.asarray(x, dtype=dtype)
    dirs, T, Sa, phi, lam = f(dirs), f(T), f(Sa), f(phi), f(lam)
    dirs = dirs if dirs.shape[1] == 3 else np.concatenate([dirs, np.zeros([len(dirs), 1], dtype)], axis=1)
    zpa = Sa[:, 0].copy() if zpa is None else f(zpa)
    xyz, conn = f(d["xyz"]), d["conn"]
    G_, p, nJ, nM = len(dirs), len(lam), len(xyz), len(conn)
    j0, j1 = conn[:, 0], conn[:, 1]
    D = xyz[j1] - xyz[j0]
    length = np.sqrt((D * D).sum(1))
    c = D / length[:, None]
    k = f(d["E"]) * f(d["A"]) / length
    K_ff, m = system(d, mass_scale, dtype)
    free = d["free"].ravel()
    axis = np.tile(np.arange(3), nJ)[free]
    X = phi.reshape(p, -1)[:, free]
    live = np.isfinite(lam.astype(np.float64)) & (lam > 0)
    omega = np.where(live, np.sqrt(np.where(live, lam, 1)), 0)
    rho = correlations(omega, live, zeta, rule, dtype)
    two_pi = 2 * f(np.pi) if dtype is np.float64 else 2 * np.arctan(dtype(1)) * 4

    def forces(u):            # (N [nM], R [nJ, 3]) of a displacement vector in joint layout
        N = k * (c * (u[j1] - u[j0])).sum(1)
        R = np.zeros([nJ, 3], dtype)
        for mm in range(nM):     # member-id order
            R[j1[mm]] += N[mm] * c[mm]
            R[j0[mm]] -= N[mm] * c[mm]
        R[d["free"]] = 0
        return N, R

    out = {"gamma": np.zeros([G_, p], dtype), "sa": np.zeros([G_, p], dtype), "meff": np.zeros([G_, p], dtype),
           "mtot": np.zeros([G_], dtype), "base": np.zeros([G_], dtype), "u": np.zeros([G_, nJ, 3], dtype),
           "N": np.zeros([G_, nM], dtype), "R": np.zeros([G_, nJ, 3], dtype),
           "modal_u": np.zeros([G_, p + 1, nJ, 3], dtype), "modal_N": np.zeros([G_, p + 1, nM], dtype),
           "modal_R": np.zeros([G_, p + 1, nJ, 3], dtype), "modal_base": np.zeros([G_, p + 1], dtype), "rho": rho}
    axial = [forces(phi[kk]) if live[kk] else None for kk in range(p)]
    for g in range(G_):
        iota = dirs[g][axis]
        out["mtot"][g] = mtot = (m * iota * iota).sum()
        rest = iota.copy()
        for kk in range(p):
            if not live[kk]:
                continue
            ga = (m * X[kk] * iota).sum()
            sa = spectrum_at(T, Sa[g], two_pi / omega[kk])
            q = ga * sa / lam[kk]
            out["gamma"][g, kk], out["sa"][g, kk] = ga, sa
            out["meff"][g, kk] = ga * ga / mtot if mtot > 0 else 0
            out["modal_u"][g, kk] = q * phi[kk]
            out["modal_N"][g, kk] = q * axial[kk][0]
            out["modal_R"][g, kk] = q * axial[kk][1]
            out["modal_base"][g, kk] = ga * ga * sa
            rest = rest - ga * X[kk]
        if missing_mass:
            y = solve(K_ff, zpa[g] * (m * rest), dtype)
            u = np.zeros(3 * nJ, dtype)
            u[free] = y
            out["modal_u"][g, p] = u.reshape(nJ, 3)
            out["modal_N"][g, p], out["modal_R"][g, p] = forces(u.reshape(nJ, 3))
            out["modal_base"][g, p] = zpa[g] * (mtot - (out["gamma"][g] ** 2).sum())
        for key in ("u", "N", "R", "base"):
            out[key][g] = combine(rho, out["modal_" + key][g], rule)
    return out


def exact_response(d, p, dirs, T, Sa, mass_scale=1.0, **kw):
    """`response` with the p lowest pairs of `eigh` (fewer when the truss has fewer)."""
    lam, Phi = G.eigen_pairs(d, mass_scale, p)
    return response(d, Phi, lam[:len(Phi)], dirs, T, Sa, mass_scale=mass_scale, **kw)
