"""NUMPY YARDSTICK OF THE MEMBER-SET SCENARIOS - TEST INFRASTRUCTURE ONLY.  Never imported by the product package.

A scenario is (members, factors): an ordered list of distinct member ids and the area factor gamma of each (0 removed,
below 1 damaged, above 1 strengthened).  Two routes to the state of a JSON truss in a scenario:

`resolve`      the definition.  Every member's area is scaled by its gamma, the members with gamma = 0 are deleted, K_ff
               of what is left is formed as the oracle forms it (`member_matK` blocks added in member-id order,
               `free_mask`); the scenario is UNSTABLE when `eigvalsh` gives lambda_min / lambda_max < 1e-12, and
               `first_unstable` is the first position j at which the scenario cut down to its members 0 .. j is; otherwise
               one `numpy.linalg.solve` per load case, N' = gamma k c . D u', the stresses |k c . D u'| / a (which do not
               depend on gamma; removed members excluded) and the joint displacement norms.
`closed_form`  the rank-k update of include/trs_sets.h: the columns z_j = inv(K_ff) b_j,f, W_ij = k_i b_i,f . z_j,
               A = I + W diag(gamma - 1) eliminated without pivoting in the set's order, the pivots, and
               a = diag(theta) inv(A) n, u' = u - sum_j a_j z_j, N'_m = gamma_m (N_m - sum_j a_j W_mj).

The discrepancy between the two is what the GPU tests scale their tolerance with.
"""
import functools

import numpy as np

from oracle import truss_oracle as orc
from tests import helpers as H
from tests import member_loss_reference as M

UNSTABLE_EIG_RATIO = M.CRITICAL_EIG_RATIO
FACTORS = (0.0, 0.0, 0.5, 2.0)
SMALL_MEMBERS = 130      # a fixture with at most this many members is "small": its scenario list holds every singleton removal


def scenarios(name, seed, S):
    """A seeded list of S random scenarios of fixture `name`, sizes 1 .. 8 and factors drawn from {0, 0, 0.5, 2},
    then an empty set, then - for a small fixture - every singleton removal."""
    nM = len(H.load_json(name)["member"])
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(S):
        k = int(rng.integers(1, min(8, nM) + 1))
        members = [int(m) for m in rng.choice(nM, size=k, replace=False)]
        out.append((members, [float(FACTORS[i]) for i in rng.integers(0, len(FACTORS), size=k)]))
    out.append(([], []))
    if nM <= SMALL_MEMBERS:
        out += [([e], [0.0]) for e in range(nM)]
    return out


def _gamma(nM, members, factors):
    g = np.ones([nM])
    g[list(members)] = factors
    return g


def _blocks(data):
    p, dim = orc.prepare(data), orc.truss_dim(data)
    return [(j0 * dim, j1 * dim, p.pos[j0], p.pos[j1], a, e_mod, length)
            for (j0, j1, a, e_mod, _rho), length in zip(p.members, p.lengths)]


def stiffness_scaled(blocks, gamma, ndof, dim):
    """`oracle.global_K` of the truss whose member areas are scaled by `gamma`, the members with gamma = 0 deleted."""
    K = np.zeros([ndof, ndof])
    for (x0, x1, p0, p1, a, e_mod, length), g in zip(blocks, gamma):
        if g == 0.0:
            continue
        Ke = orc.member_matK(p0, p1, a * g, e_mod, length)
        for i, x in ((0, x0), (dim, x1)):
            for j, y in ((0, x0), (dim, x1)):
                K[x: x + dim, y: y + dim] += Ke[i: i + dim, j: j + dim]
    return K


def peaks(stress, removed, U_after):
    """(stress, member, gap to the second best, displacement, joint, gap): `peaks` of the member-loss yardstick with
    the removed members (bool [nM]) left out."""
    stress = np.where(removed, -1.0, stress)
    norm = np.sqrt((U_after ** 2).sum(axis=1))
    out = []
    for v in (stress, norm):
        order = np.argsort(-v, kind="stable")
        best = v[order[0]]
        second = v[order[1]] if len(v) > 1 else -np.inf
        out += [max(float(best), 0.0), int(order[0]) if best >= 0.0 else -1, float(best - second)]
    return out


def _pack(S, L, nM, nJ, dim):
    return {"unstable": np.zeros([S], dtype=bool), "first_unstable": np.full([S], -1),
            "N_after": np.full([L, S, nM], np.nan), "U_after": np.full([L, S, nJ, dim], np.nan),
            "peak_stress": np.full([L, S], np.inf), "peak_member": np.full([L, S], -1), "stress_gap": np.zeros([L, S]),
            "peak_displace": np.full([L, S], np.inf), "peak_joint": np.full([L, S], -1), "displace_gap": np.zeros([L, S])}


def _fill(out, l, s, N_after, stress, removed, U_after):
    out["N_after"][l, s], out["U_after"][l, s] = N_after, U_after
    (out["peak_stress"][l, s], out["peak_member"][l, s], out["stress_gap"][l, s], out["peak_displace"][l, s],
     out["peak_joint"][l, s], out["displace_gap"][l, s]) = peaks(stress, removed, U_after)


def resolve(data, scen, loads=None):
    """Every scenario by scaling and deleting the members and solving again.  Also eig_ratio [S]."""
    dim, nJ, nM = orc.truss_dim(data), len(data["joint"]), len(data["member"])
    F = M.load_matrix(data, loads)
    free = orc.free_mask(data)
    Bm, k, area = M.member_rows(data)
    blocks = _blocks(data)
    out = _pack(len(scen), len(F), nM, nJ, dim)
    out["eig_ratio"] = np.ones([len(scen)])

    def ratio(gamma):
        Kff = stiffness_scaled(blocks, gamma, nJ * dim, dim)[free][:, free]
        lam = np.linalg.eigvalsh(Kff)
        return Kff, lam[0] / lam[-1]

    for s, (members, factors) in enumerate(scen):
        gamma = _gamma(nM, members, factors)
        Kff, out["eig_ratio"][s] = ratio(gamma)
        if out["eig_ratio"][s] < UNSTABLE_EIG_RATIO:
            out["unstable"][s] = True
            for j in range(len(members)):
                if j == len(members) - 1 or ratio(_gamma(nM, members[:j + 1], factors[:j + 1]))[1] < UNSTABLE_EIG_RATIO:
                    out["first_unstable"][s] = j
                    break
            continue
        X = np.linalg.solve(Kff, F.reshape(len(F), -1)[:, free].T)      # [n, L]
        for l in range(len(F)):
            u = np.zeros([nJ * dim])
            u[free] = X[:, l]
            n = k * (Bm @ u)
            _fill(out, l, s, gamma * n, np.abs(n) / area, gamma == 0.0, u.reshape(nJ, dim))
    return out


def closed_form(data, scen, loads=None, r_tol=1e-8):
    """Every scenario by the rank-k update.  Also pivot [S, 8] (NaN beyond the set and after a failing position), and
    the intact u [L, nJ, dim] and N [L, nM]."""
    dim, nJ, nM = orc.truss_dim(data), len(data["joint"]), len(data["member"])
    F = M.load_matrix(data, loads)
    free = orc.free_mask(data)
    Bm, k, area = M.member_rows(data)
    Kff = orc.global_K(data)[free][:, free]
    Bf = Bm[:, free]
    used = sorted({m for members, _f in scen for m in members})
    col = {m: i for i, m in enumerate(used)}
    Zf = np.linalg.solve(Kff, Bf[used].T) if used else np.zeros([int(free.sum()), 0])      # [n, used]
    U = np.zeros([len(F), nJ * dim])
    U[:, free] = np.linalg.solve(Kff, F.reshape(len(F), -1)[:, free].T).T
    N = (Bm @ U.T).T * k                                                 # [L, nM]
    out = _pack(len(scen), len(F), nM, nJ, dim)
    out.update(pivot=np.full([len(scen), 8], np.nan), u=U.reshape(len(F), nJ, dim), N=N)
    for s, (members, factors) in enumerate(scen):
        kk = len(members)
        theta = np.asarray(factors, dtype=float) - 1.0
        Z = np.zeros([nJ * dim, kk])
        Z[free] = Zf[:, [col[m] for m in members]]
        Wall = k[:, None] * (Bm @ Z)                                     # [nM, kk]
        A = np.eye(kk) + Wall[list(members)] * theta[None, :]
        lower = np.eye(kk)
        for p in range(kk):                                              # Gauss without pivoting, in the set's order
            out["pivot"][s, p] = A[p, p]
            if A[p, p] <= r_tol:
                out["unstable"][s], out["first_unstable"][s] = True, p
                break
            for i in range(p + 1, kk):
                lower[i, p] = A[i, p] / A[p, p]
                A[i, p:] -= lower[i, p] * A[p, p:]
        if out["unstable"][s]:
            continue
        gamma = _gamma(nM, members, factors)
        for l in range(len(F)):
            x = np.linalg.solve(np.triu(A), np.linalg.solve(lower, N[l, list(members)])) if kk else np.zeros([0])
            a = theta * x
            n = N[l] - Wall @ a                                          # k c . D u' of every member
            _fill(out, l, s, gamma * n, np.abs(n) / area, gamma == 0.0, (U[l] - Z @ a).reshape(nJ, dim))
    return out


def discrepancy(a, b):
    """The largest difference between two routes over N_after and U_after of the scenarios neither calls unstable,
    each relative to the largest magnitude of the compared array."""
    keep = ~(a["unstable"] | b["unstable"])
    worst = 0.0
    for key in ("N_after", "U_after"):
        x, y = a[key][:, keep], b[key][:, keep]
        if x.size:
            worst = max(worst, H.max_scaled_err(x, y))
    return worst


@functools.lru_cache(maxsize=None)
def fixture(name, seed=7, S=40, load_seed=None, cases=1):
    """(data, scenarios, loads [L, nJ, 3] or None, resolve, closed_form, d) of a shipped JSON truss, computed once per
    process: `load_seed` None = the truss's own forces, else `cases` seeded load cases."""
    data = H.load_json(name)
    loads = None
    if load_seed is not None:
        dim, nJ = orc.truss_dim(data), len(data["joint"])
        loads = np.zeros([cases, nJ, 3])
        loads[:, :, :dim] = np.random.default_rng(load_seed).uniform(-3e4, 3e4, size=(cases, nJ, dim))
    scen = scenarios(name, seed, S)
    a, b = resolve(data, scen, loads), closed_form(data, scen, loads)
    return data, scen, loads, a, b, discrepancy(a, b)
