"""Numpy reference of the adjoint gradients (test infrastructure, never imported by the package): the formulas of
include/trs_solver.h "Adjoint gradients" restated on top of `oracle.solve` / `oracle.global_K`, and the central
finite differences of `oracle.solve` they are checked against.

For cotangents gu, gf [nJ, dim] and gN [nM] (the derivative of a scalar J with respect to u, f_ext and N) `vjp` returns
dJ/dA, dJ/dE [nM], dJ/dxyz, dJ/dloads [nJ, dim] of ONE load case."""
import copy

import numpy as np

from oracle import truss_oracle as orc


def dense_forces(data, loads):
    """`data` with EVERY joint in its "force" block (the oracle drops entries below 1e-10, so a dense block with
    exact zeros at supported joints is the same truss); `loads` [nJ, >= dim]."""
    dim = orc.truss_dim(data)
    return dict(data, force=[[j, [float(x) for x in loads[j, :dim]]] for j in range(len(data["joint"]))])


def dense_loads(data):
    dim = orc.truss_dim(data)
    out = np.zeros([len(data["joint"]), dim])
    for j, vec in data["force"]:
        out[j] = vec
    return out


def vjp(data, gu, gf, gN):
    p = orc.prepare(data)
    dim = p.dim
    r = orc.solve(p)
    K, mask = orc.global_K(p), r["mask"]
    nJ = len(p.pos)
    pos = np.array(p.pos)
    j0 = np.array([m[0] for m in p.members])
    j1 = np.array([m[1] for m in p.members])
    A = np.array([m[2] for m in p.members])
    E = np.array([m[3] for m in p.members])
    d = pos[j1] - pos[j0]
    length = np.sqrt((d * d).sum(1))
    k = E * A / length
    c = d / length[:, None]
    gu, gf, gN = (np.asarray(x, dtype=float) for x in (gu, gf, gN))
    # 1. reduced right-hand side: gu + K[:, constrained] gf_c + sum over member ends (+- k gN c)
    rhs = gu.ravel().copy()
    rhs += K[:, ~mask] @ gf.ravel()[~mask]
    ends = np.zeros([nJ, dim])
    np.add.at(ends, j1, (gN * k)[:, None] * c)
    np.add.at(ends, j0, -(gN * k)[:, None] * c)
    rhs += ends.ravel()
    # 2. K_ff lambda = r_f;  3. mu = lambda at free, -gf at constrained DOFs
    mu = np.zeros(nJ * dim)
    mu[mask] = np.linalg.solve(r["K_ff"], rhs[mask])
    mu[~mask] = -gf.ravel()[~mask]
    MU, U = mu.reshape(nJ, dim), r["u"]
    g_loads = np.zeros(nJ * dim)
    g_loads[mask] = mu[mask] + gf.ravel()[mask]
    dU, dMU = U[j1] - U[j0], MU[j1] - MU[j0]
    cu, cm = (c * dU).sum(1), (c * dMU).sum(1)
    N = k * cu
    gA, gE = N / A * (gN - cm), N / E * (gN - cm)
    EA = E * A
    du_, dm_ = (d * dU).sum(1), (d * dMU).sum(1)
    e = EA * dm_ * du_ / length ** 3
    de = (EA / length ** 3)[:, None] * (dMU * du_[:, None] + dU * dm_[:, None]) - (3 * e / length ** 2)[:, None] * d
    dN = (EA / length ** 2)[:, None] * dU - (2 * N / length ** 2)[:, None] * d
    gd = gN[:, None] * dN - de
    gx = np.zeros([nJ, dim])
    np.add.at(gx, j1, gd)
    np.add.at(gx, j0, -gd)
    return {"A": gA, "E": gE, "xyz": gx, "loads": g_loads.reshape(nJ, dim)}, r


def vjp_cases(data, loads, gu, gf, gN):
    """L load cases of one truss: `loads`, gu, gf [L, nJ, >= dim], gN [L, nM] (None = zero).  Returns (dA, dE [nM],
    dxyz [nJ, dim] summed over the cases, dloads [L, nJ, dim]) as a dict, and the list of forward results."""
    dim, nJ, nM = orc.truss_dim(data), len(data["joint"]), len(data["member"])
    out = {"A": np.zeros(nM), "E": np.zeros(nM), "xyz": np.zeros([nJ, dim]), "loads": np.zeros([len(loads), nJ, dim])}
    forward = []
    for k in range(len(loads)):
        z = np.zeros([nJ, dim])
        g, r = vjp(dense_forces(data, loads[k]), z if gu is None else gu[k][:nJ, :dim], z if gf is None else gf[k][:nJ, :dim],
                   np.zeros(nM) if gN is None else gN[k][:nM])
        for key in ("A", "E", "xyz"):
            out[key] += g[key]
        out["loads"][k] = g["loads"]
        forward.append(r)
    return out, forward


def objective(data, gu, gf, gN):
    r = orc.solve(data)
    return (gu * r["u"]).sum() + (gf * r["f_ext"]).sum() + (gN * r["N"]).sum()


def finite_differences(data, gu, gf, gN, h=1e-4, load_step=1e-2, coordinates=True):
    """Central differences of J = gu . u + gf . f_ext + gN . N through `oracle.solve`: relative step `h` for A, E and the
    coordinates (step `h` for a coordinate that is zero), `load_step` of the largest load for the loads.  `data` must
    carry dense forces (`dense_forces`)."""
    nJ, nM, dim = len(data["joint"]), len(data["member"]), orc.truss_dim(data)
    out = {"A": np.zeros(nM), "E": np.zeros(nM), "xyz": np.zeros([nJ, dim]), "loads": np.zeros([nJ, dim])}

    def diff(setter, x0, step):
        vals = []
        for s in (+1, -1):
            dd = copy.deepcopy(data)
            setter(dd, x0 + s * step)
            vals.append(objective(dd, gu, gf, gN))
        return (vals[0] - vals[1]) / (2 * step)

    for m in range(nM):
        a, e_, rho = (float(x) for x in data["member"][m][1])
        out["A"][m] = diff(lambda dd, v: dd["member"][m].__setitem__(1, [v, e_, rho]), a, h * abs(a))
        out["E"][m] = diff(lambda dd, v: dd["member"][m].__setitem__(1, [a, v, rho]), e_, h * abs(e_))
    full = dense_loads(data)
    largest = np.abs(full).max()
    free = orc.free_mask(data).reshape(nJ, dim)
    for j in range(nJ):
        for t in range(dim):
            if coordinates:
                x0 = float(data["joint"][j][0][t])

                def setx(dd, v):
                    dd["joint"][j][0] = list(dd["joint"][j][0])
                    dd["joint"][j][0][t] = v
                out["xyz"][j, t] = diff(setx, x0, h * abs(x0) if x0 != 0 else h)
            if free[j, t]:
                def setf(dd, v):
                    ff = full.copy()
                    ff[j, t] = v
                    dd["force"] = [[jj, [float(x) for x in ff[jj]]] for jj in range(nJ)]
                out["loads"][j, t] = diff(setf, float(full[j, t]), load_step * largest)
    return out
