"""NUMPY YARDSTICK OF THE INFLUENCE LINES AND MOVING-LOAD ENVELOPES - TEST INFRASTRUCTURE ONLY.  Never imported by the
product package.

The definitions of include/trs_influence.h, written from the formulas.  Two routes to the influence ordinates
eta[m][p] of the member forces of a JSON truss along a path of joints, for a load vector d:

`by_definition`  for every path joint one dense solve (`effects_reference.solve`) with the load d at that joint: the N of
                 that solve are the ordinates.  The envelope of a load train and the two areas are then formed from the
                 definitions with plain Python loops over the candidates, the axles and the segments.
`by_column`      k_m inv(K_ff) b_m,f read along the path (Maxwell / Mueller-Breslau).

The discrepancy between the two is what the GPU tests scale their tolerance with.
"""
import numpy as np

from oracle import truss_oracle as orc
from tests import effects_reference as R
from tests.member_loss_reference import member_rows

EPS = 1e-12     # an axle within EPS * S of an end of the path stands on the end joint


def arc_lengths(data, path):
    """s [P]: s_0 = 0, s_p = s_{p-1} + |x_path[p] - x_path[p-1]|."""
    s = np.zeros([len(path)])
    if not len(path):
        return s
    pos = np.array([orc.prepare(data).pos[j] for j in path], dtype=float)
    for p in range(1, len(path)):
        s[p] = s[p - 1] + float(np.sqrt(((pos[p] - pos[p - 1]) ** 2).sum()))
    return s


def ordinates_by_definition(data, path, d):
    """eta [nM, P]: column p holds the member forces under the load d at joint path[p] alone."""
    dim, nJ, nM = orc.truss_dim(data), len(data["joint"]), len(data["member"])
    eta, solved = np.zeros([nM, len(path)]), {}
    for p, j in enumerate(path):
        if j not in solved:
            loads = np.zeros([nJ, dim])
            loads[j] = np.asarray(d, dtype=float)[:dim]
            solved[j] = R.solve(data, loads)["N"]
        eta[:, p] = solved[j]
    return eta


def ordinates_by_column(data, path, d):
    """eta [nM, P] = k_m (d . z_m at path[p]), z_m = inv(K_ff) b_m,f spread over the joints, zero at held DOFs."""
    dim, nJ, nM = orc.truss_dim(data), len(data["joint"]), len(data["member"])
    free = orc.free_mask(data)
    Bm, k, _area = member_rows(data)
    Z = np.zeros([nM, nJ * dim])
    Z[:, free] = np.linalg.solve(orc.global_K(data)[free][:, free], Bm[:, free].T).T
    Z = Z.reshape(nM, nJ, dim)
    dv = np.asarray(d, dtype=float)[:dim]
    return np.stack([k * (Z[:, j] @ dv) for j in path], axis=1) if len(path) else np.zeros([nM, 0])


def line_at(s, eta, t):
    """eta_m(t) of every member [nM]: piecewise linear through (s_p, eta[:, p]) by the lever rule, 0 off the path, the
    ends taken within EPS * S."""
    P, S = len(s), float(s[-1])
    if t < -EPS * S or t > S + EPS * S:
        return np.zeros([eta.shape[0]])
    if P == 1:
        return eta[:, 0].copy()
    t = min(max(t, 0.0), S)
    q = min(int(np.searchsorted(s, t, side="right")) - 1, P - 2)
    lam = (t - s[q]) / (s[q + 1] - s[q])
    return (1.0 - lam) * eta[:, q] + lam * eta[:, q + 1]


def response(s, eta, train, x):
    """N_m(x) [nM] = sum_a w_a eta_m(x - o_a): the member forces with the lead axle at arc position x."""
    N = np.zeros([eta.shape[0]])
    for w, o in train:
        N += w * line_at(s, eta, x - o)
    return N


def candidates(s, eta, train):
    """(values [P * A, nM], x [P * A]) in p-major order: at candidate (p, a) axle a stands on path joint p, axle a' at
    s_p + (o_a - o_a')."""
    values, xs = [], []
    for p in range(len(s)):
        for _wa, oa in train:
            N = np.zeros([eta.shape[0]])
            for w2, o2 in train:
                N += w2 * line_at(s, eta, s[p] + (oa - o2))
            values.append(N)
            xs.append(s[p] + oa)
    return np.array(values).reshape(len(xs), eta.shape[0]), np.array(xs)


def areas(s, eta):
    """(area_pos, area_neg) [nM]: the integrals of max(eta_m, 0) and min(eta_m, 0) over the path, segment by segment, a
    segment whose ends differ in sign split at the crossing."""
    nM = eta.shape[0]
    pos, neg = np.zeros([nM]), np.zeros([nM])
    for m in range(nM):
        for p in range(len(s) - 1):
            h, u, v = s[p + 1] - s[p], eta[m, p], eta[m, p + 1]
            if u >= 0 and v >= 0:
                pos[m] += 0.5 * h * (u + v)
            elif u <= 0 and v <= 0:
                neg[m] += 0.5 * h * (u + v)
            else:
                cut = h * u / (u - v)
                au, av = 0.5 * u * cut, 0.5 * v * (h - cut)
                pos[m] += au if u > 0 else av
                neg[m] += av if u > 0 else au
    return pos, neg


def by_definition(data, path, d, train=None):
    """Everything the analysis returns for one truss, from the definitions.  `train`: [(weight, offset)], None = one unit
    axle.  Returns dict s [P], eta [nM, P], N_max, N_min, x_max, x_min, area_pos, area_neg [nM], values [P A, nM] and
    x [P A] (the candidates), and d_routes, the discrepancy between the two routes to eta relative to the largest |eta|."""
    train = [(1.0, 0.0)] if train is None else [(float(w), float(o)) for w, o in train]
    path = [int(j) for j in path]
    nM = len(data["member"])
    s = arc_lengths(data, path)
    eta = ordinates_by_definition(data, path, d)
    out = {"s": s, "eta": eta, "train": train}
    if len(path) == 0:
        nan = np.full([nM], np.nan)
        out.update(N_max=np.zeros([nM]), N_min=np.zeros([nM]), x_max=nan, x_min=nan.copy(), area_pos=np.zeros([nM]),
                   area_neg=np.zeros([nM]), values=np.zeros([0, nM]), x=np.zeros([0]), d_routes=0.0)
        return out
    values, xs = candidates(s, eta, train)
    hi, lo = values.argmax(axis=0), values.argmin(axis=0)       # (the first of equal values: the lowest candidate)
    pos, neg = areas(s, eta)
    column = ordinates_by_column(data, path, d)
    scale = np.abs(eta).max()
    out.update(N_max=values.max(axis=0), N_min=values.min(axis=0), x_max=xs[hi], x_min=xs[lo], area_pos=pos,
               area_neg=neg, values=values, x=xs,
               d_routes=float(np.abs(eta - column).max() / scale) if scale > 0 else float(np.abs(column).max()))
    return out
