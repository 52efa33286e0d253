"""NUMPY YARDSTICK OF THE EFFECT LOAD CASES - TEST INFRASTRUCTURE ONLY.  Never imported by the product package.

A dense restatement of the definitions of include/trs_effects.h, written from the formulas: the global stiffness
matrix of the oracle (`oracle.truss_oracle.global_K`), the partition into free and constrained DOFs, one
`numpy.linalg.solve`, and the member forces, support forces and body loads formed member by member.

Member m from joint j0 to j1, len its length, c = (x_j1 - x_j0) / len, k = E A / len, tension positive.  With the case's
joint forces `loads`, initial strains `eps0`, settlements `ubar` (constrained DOFs) and body-force vector `g`:
    body_j  = sum over the member ends at j of 1/2 (a len density) g
    P0_j    = sum over the member ends at j of (+ at j1, - at j0) E A eps0_m c              (equivalent pre-strain loads)
    K_ff u_f = (loads + body + P0)_f - K_fc ubar_c,   u_c = ubar_c
    N_m     = k c . (u_j1 - u_j0) - E A eps0_m
    f_ext   = loads at the free DOFs;  sum over the ends (+ at j1, - at j0) of N_m c  -  body  at the constrained DOFs
"""
import numpy as np

from oracle import truss_oracle as orc


def members_of(data):
    """[(j0, j1, EA, k, c [dim], half weight)] per member, lengths and cosines as the oracle forms them."""
    p = orc.prepare(data)
    out = []
    for (j0, j1, a, e, rho), length in zip(p.members, p.lengths):
        c = np.array(orc.member_cosines(p.pos[j0], p.pos[j1], length))
        out.append((j0, j1, e * a, e * a / length, c, 0.5 * (a * length * rho)))
    return out


def body_loads(data, accel):
    """[nJ, dim]: half the weight of every member times `accel` on each of its end joints."""
    dim, nJ = orc.truss_dim(data), len(data["joint"])
    body = np.zeros([nJ, dim])
    if accel is not None:
        g = np.asarray(accel, dtype=float)[:dim]
        for j0, j1, _EA, _k, _c, half in members_of(data):
            body[j0] += half * g
            body[j1] += half * g
    return body


def equivalent_loads(data, prestrain):
    """[nJ, dim]: the joint loads a member initial strain is equivalent to - E A eps0 c pushes joint1 away from joint0."""
    dim, nJ = orc.truss_dim(data), len(data["joint"])
    P0 = np.zeros([nJ, dim])
    if prestrain is not None:
        for m, (j0, j1, EA, _k, c, _half) in enumerate(members_of(data)):
            P0[j1] += EA * prestrain[m] * c
            P0[j0] -= EA * prestrain[m] * c
    return P0


def solve(data, loads=None, prestrain=None, settlement=None, accel=None):
    """One case of one truss.  `loads`, `settlement`: [nJ, >= dim] or None; `prestrain`: [nM] or None; `accel`: [>= dim]
    or None.  Returns dict u, f_ext, body [nJ, dim], N [nM], mask (free DOFs)."""
    dim, nJ = orc.truss_dim(data), len(data["joint"])
    K = orc.global_K(data)
    free = orc.free_mask(data)
    held = ~free
    f = np.zeros([nJ, dim]) if loads is None else np.asarray(loads, dtype=float)[:nJ, :dim].copy()
    ubar = np.zeros([nJ * dim])
    if settlement is not None:
        ubar[held] = np.asarray(settlement, dtype=float)[:nJ, :dim].reshape(-1)[held]
    body = body_loads(data, accel)
    rhs = (f + body + equivalent_loads(data, prestrain)).reshape(-1)[free] - K[free][:, held] @ ubar[held]
    u = ubar.copy()
    u[free] = np.linalg.solve(K[free][:, free], rhs)
    U = u.reshape(nJ, dim)
    members = members_of(data)
    N = np.zeros([len(members)])
    pull = np.zeros([nJ, dim])      # sum over the ends of (+-) N c
    for m, (j0, j1, EA, k, c, _half) in enumerate(members):
        N[m] = k * (c @ (U[j1] - U[j0])) - (EA * prestrain[m] if prestrain is not None else 0.0)
        pull[j1] += N[m] * c
        pull[j0] -= N[m] * c
    f_ext = np.where(free.reshape(nJ, dim), f, pull - body)
    return {"u": U, "f_ext": f_ext, "N": N, "body": body, "mask": free}
