"""NUMPY YARDSTICK OF THE MEMBER-LOSS ANALYSIS - TEST INFRASTRUCTURE ONLY.  Never imported by the product package.

Two routes to the state of a truss after the removal of one member e, for every member of a JSON truss:

`resolve`      the definition.  Member e is deleted, K_ff of what is left is formed as the oracle forms it (`global_K`
               of the data without e - `stiffness_without` gives the same bits faster - and `free_mask`); e is CRITICAL
               when `eigvalsh` gives lambda_min / lambda_max < 1e-12 (over the
               shipped fixtures the critical members sit at <= 1e-16 and the others at >= 1e-7); otherwise one
               `numpy.linalg.solve` per load case, and N, the stresses |N| / a and the joint displacement norms formed
               member by member as `effects_reference.solve` forms them.
`closed_form`  the rank-one update of include/trs_loss.h: z_e = inv(K_ff) b_e,f, r_e = 1 - k_e b_e,f . z_e,
               alpha = N_e / r_e, u' = u + alpha z_e, N'_m = N_m + alpha k_m b_m,f . z_e.

The discrepancy between the two is what the GPU tests scale their tolerance with.
"""
import contextlib
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import truss_oracle as orc
from tests import effects_reference as R
from tests import helpers as H

CRITICAL_EIG_RATIO = 1e-12


def load_matrix(data, loads=None):
    """[L, nJ, dim]: the given dense cases [L, nJ, >= dim], or the truss's own forces as one case."""
    dim, nJ = orc.truss_dim(data), len(data["joint"])
    if loads is None:
        return orc.force_vector(data).reshape(1, nJ, dim)
    return np.asarray(loads, dtype=float)[:, :nJ, :dim]


def member_rows(data):
    """(Bm [nM, nJ * dim], k [nM], a [nM]): b_m over ALL DOFs, the stiffnesses and the areas."""
    dim, nJ = orc.truss_dim(data), len(data["joint"])
    members = R.members_of(data)
    Bm, k = np.zeros([len(members), nJ * dim]), np.zeros([len(members)])
    for m, (j0, j1, _EA, km, c, _half) in enumerate(members):
        Bm[m, j1 * dim:(j1 + 1) * dim] += c
        Bm[m, j0 * dim:(j0 + 1) * dim] -= c
        k[m] = km
    return Bm, k, np.array([float(a) for _ends, (a, _e, _rho) in data["member"]])


def peaks(N_after, U_after, area, e):
    """Peak stress and displacement of one removal: (stress, member, gap to the second best, displacement, joint,
    gap to the second best); the gaps are absolute differences (inf where there is no second)."""
    stress = np.abs(N_after) / area
    stress[e] = -1.0
    norm = np.sqrt((U_after ** 2).sum(axis=1))
    out = []
    for v in (stress, norm):
        order = np.argsort(-v, kind="stable")
        best = v[order[0]]
        second = v[order[1]] if len(v) > 1 else -np.inf
        out += [max(float(best), 0.0), int(order[0]), float(best - second)]
    return out


def stiffness_without(blocks, e, ndof, dim):
    """`oracle.global_K` of the truss with member e deleted, bit for bit: the oracle's member matrices
    (`member_matK`, formed once per member instead of once per removal) added block by block in member-ID order."""
    K = np.zeros([ndof, ndof])
    for m, (x0, x1, Ke) in enumerate(blocks):
        if m == e:
            continue
        for i, x in ((0, x0), (dim, x1)):
            for j, y in ((0, x0), (dim, x1)):
                K[x: x + dim, y: y + dim] += Ke[i: i + dim, j: j + dim]
    return K


def _pack(nM, L, nJ, dim):
    return {"critical": np.zeros([nM], dtype=bool), "N_after": np.full([L, nM, nM], np.nan),
            "U_after": np.full([L, nM, nJ, dim], np.nan), "peak_stress": np.full([L, nM], np.inf),
            "peak_member": np.full([L, nM], -1), "stress_gap": np.zeros([L, nM]),
            "peak_displace": np.full([L, nM], np.inf), "peak_joint": np.full([L, nM], -1),
            "displace_gap": np.zeros([L, nM])}


def _fill(out, l, e, N_after, U_after, area):
    out["N_after"][l, e], out["U_after"][l, e] = N_after, U_after
    (out["peak_stress"][l, e], out["peak_member"][l, e], out["stress_gap"][l, e], out["peak_displace"][l, e],
     out["peak_joint"][l, e], out["displace_gap"][l, e]) = peaks(N_after, U_after, area, e)


def resolve(data, loads=None):
    """Every single-member removal by deleting the member and solving again."""
    dim, nJ, nM = orc.truss_dim(data), len(data["joint"]), len(data["member"])
    F = load_matrix(data, loads)
    free = orc.free_mask(data)
    Bm, k, area = member_rows(data)
    out = _pack(nM, len(F), nJ, dim)
    out["eig_ratio"] = np.zeros([nM])

    p = orc.prepare(data)
    blocks = [(j0 * dim, j1 * dim, orc.member_matK(p.pos[j0], p.pos[j1], a, e_mod, length))
              for (j0, j1, a, e_mod, _rho), length in zip(p.members, p.lengths)]

    def one(e):
        Kff = stiffness_without(blocks, e, nJ * dim, dim)[free][:, free]
        lam = np.linalg.eigvalsh(Kff)
        out["eig_ratio"][e] = lam[0] / lam[-1]
        if out["eig_ratio"][e] < CRITICAL_EIG_RATIO:
            out["critical"][e] = True
            return
        X = np.linalg.solve(Kff, F.reshape(len(F), -1)[:, free].T)      # [n, L]
        for l in range(len(F)):
            u = np.zeros([nJ * dim])
            u[free] = X[:, l]
            N_after = k * (Bm @ u)
            N_after[e] = 0.0
            _fill(out, l, e, N_after, u.reshape(nJ, dim), area)

    # every removal writes its own rows of `out`; LAPACK runs outside the interpreter lock, so a few threads cut
    # bar-942's 942 eigenvalue problems of order 696 from a minute to seconds - with LAPACK's own threads held at one
    # per worker, so that the pool never asks for more than eight cores (without threadpoolctl: two workers)
    try:
        from threadpoolctl import threadpool_limits
        workers, limit = min(8, os.cpu_count() or 1), threadpool_limits(limits=1)
    except ImportError:
        workers, limit = 2, contextlib.nullcontext()
    with limit, ThreadPoolExecutor(max_workers=workers) as pool:
        list(pool.map(one, range(nM)))
    return out


def closed_form(data, loads=None, r_tol=1e-8):
    """Every single-member removal by the rank-one update; also r [nM], and the intact u [L, nJ, dim] and N [L, nM]."""
    dim, nJ, nM = orc.truss_dim(data), len(data["joint"]), len(data["member"])
    F = load_matrix(data, loads)
    free = orc.free_mask(data)
    Bm, k, area = member_rows(data)
    Kff = orc.global_K(data)[free][:, free]
    Bf = Bm[:, free]
    Z = np.linalg.solve(Kff, Bf.T)                                       # [n, nM]
    r = 1.0 - k * np.einsum("mi,im->m", Bf, Z)
    U = np.zeros([len(F), nJ * dim])
    U[:, free] = np.linalg.solve(Kff, F.reshape(len(F), -1)[:, free].T).T
    N = (Bm @ U.T).T * k                                                 # [L, nM]
    out = _pack(nM, len(F), nJ, dim)
    out.update(r=r, u=U.reshape(len(F), nJ, dim), N=N, n_free=int(free.sum()))
    out["critical"] = r <= r_tol
    for e in np.flatnonzero(~out["critical"]):
        z = np.zeros([nJ * dim])
        z[free] = Z[:, e]
        q = k * (Bm @ z)
        for l in range(len(F)):
            alpha = N[l, e] / r[e]
            N_after = N[l] + alpha * q
            N_after[e] = 0.0
            _fill(out, l, e, N_after, (U[l] + alpha * z).reshape(nJ, dim), area)
    return out


def discrepancy(a, b):
    """The largest difference between two routes over N_after and U_after of the members neither calls critical,
    each relative to the largest magnitude of the compared array."""
    keep = ~(a["critical"] | b["critical"])
    worst = 0.0
    for key in ("N_after", "U_after"):
        x, y = a[key][:, keep], b[key][:, keep]
        if x.size:
            worst = max(worst, H.max_scaled_err(x, y))
    return worst


@functools.lru_cache(maxsize=None)
def fixture(name, seed=None, cases=1):
    """(data, loads [L, nJ, 3] or None, resolve, closed_form, d) of a shipped JSON truss, computed once per process:
    `seed` None = the truss's own forces, else `cases` seeded load cases."""
    data = H.load_json(name)
    loads = None
    if seed is not None:
        dim, nJ = orc.truss_dim(data), len(data["joint"])
        loads = np.zeros([cases, nJ, 3])
        loads[:, :, :dim] = np.random.default_rng(seed).uniform(-3e4, 3e4, size=(cases, nJ, dim))
    a, b = resolve(data, loads), closed_form(data, loads)
    return data, loads, a, b, discrepancy(a, b)
