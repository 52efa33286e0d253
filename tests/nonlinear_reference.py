"""Numpy yardstick of the geometrically nonlinear statics (test infrastructure, never imported by the package): a
dense Newton iteration in the formulation of include/trs_nonlinear.h, in any floating-point type - `numpy.float64`, or
`numpy.longdouble` to measure what float64 itself loses.  The linear systems are solved by the plain elimination of
`tests/dynamics_reference.Eliminated`, so both types run the same algorithm.

The formulation, per member m with ends j0, j1, undeformed coordinates X and displacement u:
    D = X_j1 - X_j0, L0 = |D|, dl = u_j1 - u_j0, d = D + dl, l = |d|, n = d / l
    e = (2 D.dl + dl.dl) / (L0 (l + L0))   (= (l - L0) / L0 exactly, without subtracting two lengths),  N = E A e
    internal force +N n at j1, -N n at j0
    k_t = (EA / L0) n n^T + (N / l)(I - n n^T), + on the two diagonal blocks of K_t, - on the two off-diagonal ones
Residual on the free DOFs r = lambda P - f_int; held DOFs stay at zero.  Converged when |r|_inf <= tol |lambda P|_inf;
for lambda P = 0 the answer is u unchanged."""
import numpy as np

from oracle import truss_oracle as orc
from tests.dynamics_reference import Eliminated

ACTIVE, CONVERGED, ITER_LIMIT, NOT_PD, NOT_ATTEMPTED = -1, 0, 1, 2, 3


def state(data, u, dtype=np.float64, tangent=False):
    """(N [nM], f_int [nJ * dim], K_t [nJ * dim, nJ * dim] or None) at displacements u [nJ, dim]."""
    p = orc.prepare(data)
    dim = p.dim
    X = np.asarray(p.pos, dtype=dtype)
    u = np.asarray(u, dtype=dtype).reshape(len(X), dim)
    N = np.zeros(len(p.members), dtype=dtype)
    f = np.zeros(len(X) * dim, dtype=dtype)
    K = np.zeros([len(X) * dim] * 2, dtype=dtype) if tangent else None
    eye = np.eye(dim, dtype=dtype)
    for m, (j0, j1, a, e, _rho) in enumerate(p.members):
        D = X[j1] - X[j0]
        L0 = np.sqrt((D * D).sum())
        dl = u[j1] - u[j0]
        d = D + dl
        l = np.sqrt((d * d).sum())
        n = d / l
        EA = dtype(e) * dtype(a)
        strain = (dtype(2) * (D * dl).sum() + (dl * dl).sum()) / (L0 * (l + L0))
        N[m] = EA * strain
        s0, s1 = slice(j0 * dim, (j0 + 1) * dim), slice(j1 * dim, (j1 + 1) * dim)
        f[s1] += N[m] * n
        f[s0] -= N[m] * n
        if tangent:
            nn = np.outer(n, n)
            kt = (EA / L0) * nn + (N[m] / l) * (eye - nn)
            K[s0, s0] += kt
            K[s1, s1] += kt
            K[s0, s1] -= kt
            K[s1, s0] -= kt
    return N, f, K


def residual(data, u, lam, dtype=np.float64, pattern=None):
    """(|r|_inf, |lambda P|_inf) over the free DOFs at displacements u [nJ, dim]."""
    mask = orc.free_mask(data)
    P = np.asarray(orc.force_vector(data) if pattern is None else pattern, dtype=dtype).ravel()
    _, f, _ = state(data, u, dtype)
    lp = dtype(lam) * P[mask]
    r = lp - f[mask]
    return (np.abs(r).max() if r.size else dtype(0)), (np.abs(lp).max() if lp.size else dtype(0))


def positive_definite(A):
    """Whether the plain Cholesky factorisation of A meets positive pivots only."""
    try:
        np.linalg.cholesky(np.asarray(A, dtype=np.float64))
        return True
    except np.linalg.LinAlgError:
        return False


def newton(data, load_factors, tol=1e-9, max_iters=25, dtype=np.float64, pattern=None, keep_tangents=False, solve=None):
    """The load steps of one truss, each started from the previous step's u.  Returns a dict over the S steps:
    u [S, nJ, dim], N [S, nM], f_ext [S, nJ, dim] (lambda P at free DOFs, f_int at held ones), iters, status [S] (int32),
    residual [S] (|r|_inf at the u returned) and - `keep_tangents` - "tangents": per step the list of the reduced
    tangents that were factored.  Status as include/trs_nonlinear.h: 0 converged, 1 iteration limit, 2 tangent not
    positive definite (u is the last accepted iterate, iters the number of accepted updates), 3 not attempted because
    an earlier step failed.  `solve(K_t, r)` (None: the plain elimination) is what solves an iteration's system: a
    float64 test of a large truss may pass `numpy.linalg.solve` for speed - Newton's method corrects itself, the
    converged u is set by the residual, not by how the steps towards it were solved."""
    p = orc.prepare(data)
    dim, nJ = p.dim, len(p.pos)
    mask = orc.free_mask(p)
    P = np.asarray(orc.force_vector(p) if pattern is None else pattern, dtype=dtype).ravel()
    S = len(load_factors)
    out = {"u": np.zeros([S, nJ, dim], dtype=dtype), "N": np.zeros([S, len(p.members)], dtype=dtype),
           "f_ext": np.zeros([S, nJ, dim], dtype=dtype), "iters": np.zeros([S], dtype=np.int32),
           "status": np.zeros([S], dtype=np.int32), "residual": np.zeros([S], dtype=dtype), "tangents": []}
    u = np.zeros(nJ * dim, dtype=dtype)
    failed = False
    for s, lam in enumerate(load_factors):
        lp = dtype(lam) * P
        status, its, tangents = (NOT_ATTEMPTED if failed else ACTIVE), 0, []
        while True:
            N, f, K = state(p, u.reshape(nJ, dim), dtype, tangent=status == ACTIVE)
            r = lp[mask] - f[mask]
            rn = np.abs(r).max() if r.size else dtype(0)
            pn = np.abs(lp[mask]).max() if r.size else dtype(0)
            if status != ACTIVE:
                break
            if pn == 0 or rn <= dtype(tol) * pn:
                status = CONVERGED
                break
            if its == max_iters:
                status = ITER_LIMIT
                break
            Kt = K[mask][:, mask]
            tangents.append(Kt)
            if not positive_definite(Kt):
                status = NOT_PD
                break
            u[mask] += Eliminated(Kt).solve(r[:, None])[:, 0] if solve is None else solve(Kt, r)
            its += 1
        failed = failed or status != CONVERGED
        f_ext = np.where(mask, lp, f)
        out["u"][s], out["N"][s], out["f_ext"][s] = u.reshape(nJ, dim), N, f_ext.reshape(nJ, dim)
        out["iters"][s], out["status"][s], out["residual"][s] = its, status, rn
        out["tangents"].append(tangents)
    if not keep_tangents:
        del out["tangents"]
    return out


COMPARED = ("u", "N", "f_ext")


def relative_difference(x, y):
    """The largest max-scaled difference between two `newton` results over u, N and f_ext."""
    worst = 0.0
    for key in COMPARED:
        scale = float(np.abs(y[key]).max())
        if scale > 0:
            worst = max(worst, float(np.abs(x[key].astype(np.longdouble) - y[key]).max()) / scale)
    return worst


#: the ragged batch of the GPU tests (n_free 5, 8, 18, 40, 48, 111) and its load steps
BATCH = ("bar-6_input_0", "bar-10_input_0", "bar-25_input_0", "bar-47_input_0", "bar-72_input_0", "bar-120_input_0")
STEPS = (1.0, 2.0, 3.0)
BIG = "bar-942_input_0"
BIG_STEPS = (0.004,)
