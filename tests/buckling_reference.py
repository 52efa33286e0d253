"""Numpy yardstick of the linear buckling analysis (test infrastructure, never imported by the package), in the words
of include/trs_buckling.h.

Reference state: N_m the linear member force under the truss's own loads (the oracle's `solve`), g_m = N_m / L0_m, n_m the
undeformed direction.  Geometric stiffness: per member g_m (I - n n^T), + on the two diagonal joint blocks, - on the two
off-diagonal ones.  Problem: K_ff phi = lambda H phi with H = -Kg; a positive lambda scales the load as applied, a
negative one means buckling under the reversed load.

Shift: for theta >= 0 with Kbar = K_ff + theta Kg positive definite, iterate on H phi = nu Kbar phi; then
lambda = theta + 1 / nu, and the largest |nu| is the eigenvalue nearest theta.  One iteration on a block F of 16 vectors:
    Y = inv(Kbar) F,  G = H Y,  A_r = Y^T G,  B_r = Y^T F (= Y^T Kbar Y)
    deflation: B_r = V D V^T (cyclic Jacobi); the directions with D_k <= 2^-40 max D are dropped, r are left
    T = V_r D_r^-1/2,  C = T^T A_r T = W diag(nu) W^T (cyclic Jacobi),  |nu| descending,  Q = T W
    X <- Y Q,  F_new <- G Q;  residual of pair i = |(G Q)_i - nu_i (F Q)_i|_2 / |nu_i (F Q)_i|_2
The first block F is `modes_reference.start_block`.

Search for the smallest positive factor: see `search`."""
import numpy as np

from oracle import truss_oracle as orc
from tests import modes_reference as mref

BLOCK = mref.BLOCK
DEFLATE = 2.0 ** -40
FOUND, NONE, SHIFT_LIMIT, ITER_LIMIT, NOT_PD = 0, 1, 2, 3, 4


def reversed_loads(data):
    """The same truss with every load negated."""
    return dict(data, force=[[j, [-float(v) for v in vec]] for j, vec in data["force"]])


def matrices(data, dtype=np.float64):
    """(K_ff, H = -Kg_ff, the free mask) of one truss in the oracle's numbering, Kg from the oracle's own member forces."""
    p = orc.prepare(data)
    dim = p.dim
    ref = orc.solve(p, check_stable=False)
    mask = ref["mask"]
    Kg = np.zeros([len(p.pos) * dim] * 2, dtype=dtype)
    eye = np.eye(dim, dtype=dtype)
    for (j0, j1, _a, _e, _rho), length, N in zip(p.members, p.lengths, ref["N"]):
        n = (np.asarray(p.pos[j1], dtype=dtype) - np.asarray(p.pos[j0], dtype=dtype)) / dtype(length)
        kg = (dtype(N) / dtype(length)) * (eye - np.outer(n, n))
        s0, s1 = slice(j0 * dim, (j0 + 1) * dim), slice(j1 * dim, (j1 + 1) * dim)
        Kg[s0, s0] += kg
        Kg[s1, s1] += kg
        Kg[s0, s1] -= kg
        Kg[s1, s0] -= kg
    return np.asarray(ref["K_ff"], dtype=dtype), -Kg[mask][:, mask], mask


def exact_factors(K_ff, H):
    """Every finite eigenvalue lambda of K_ff phi = lambda H phi, ascending: reciprocals of the eigenvalues mu of
    inv(L) H inv(L)^T (K_ff = L L^T) that are not zero to rounding (|mu| > 1e-13 max |mu|)."""
    L = np.linalg.cholesky(K_ff)
    M = np.linalg.solve(L, np.linalg.solve(L, H).T).T
    mu = np.linalg.eigvalsh(0.5 * (M + M.T))
    if not mu.size or not np.abs(mu).max() > 0:
        return np.zeros(0)
    return np.sort(1.0 / mu[np.abs(mu) > 1e-13 * np.abs(mu).max()])


def smallest_positive(lams):
    pos = lams[lams > 0]
    return float(pos.min()) if pos.size else float("nan")


def nearest(lams, theta, p):
    """The p eigenvalues nearest theta, nearest first."""
    return lams[np.argsort(np.abs(lams - theta), kind="stable")[:p]]


def jacobi(C, sweeps=30):
    """`modes_reference.jacobi` (cyclic Jacobi in the round-robin order: (eigenvalues, eigenvectors), unsorted) for
    float64; the same sweeps in the matrix's own type for any other (`numpy.longdouble`: the float64 floor)."""
    if C.dtype == np.float64:
        return mref.jacobi(C, sweeps)
    dtype, q = C.dtype.type, len(C)
    A, W = C.copy(), np.eye(q, dtype=dtype)
    for _ in range(sweeps):
        rotated = False
        for rnd in range(BLOCK - 1):
            pairs = [(BLOCK - 1, rnd)] + [((rnd + k) % (BLOCK - 1), (rnd - k) % (BLOCK - 1)) for k in range(1, 8)]
            J = np.eye(q, dtype=dtype)
            for a, c in pairs:
                if a >= q or c >= q:
                    continue
                apq = A[a, c]
                if abs(apq) > np.finfo(dtype).eps / 2 * np.sqrt(abs(A[a, a] * A[c, c])) and apq != 0:
                    tau = (A[c, c] - A[a, a]) / (2 * apq)
                    t = (1 if tau >= 0 else -1) / (abs(tau) + np.sqrt(1 + tau * tau))
                    cs = 1 / np.sqrt(1 + t * t)
                    J[a, a] = J[c, c] = cs
                    J[a, c], J[c, a] = t * cs, -t * cs
                    rotated = True
            A, W = J.T @ A @ J, W @ J
        if not rotated:
            break
    return np.diag(A).copy(), W


def reduced_problem(Ar, Br):
    """(nu [16] with NaN beyond r, Q [16, 16] with zero columns beyond r, r) of A_r Q = B_r Q diag(nu) with deflation."""
    Ar, Br = 0.5 * (Ar + Ar.T), 0.5 * (Br + Br.T)
    d, V = jacobi(Br)
    keep = [k for k in range(BLOCK) if d[k] > DEFLATE * d.max()]
    r = len(keep)
    nu, Q = np.full(BLOCK, np.nan, dtype=Ar.dtype), np.zeros([BLOCK, BLOCK], dtype=Ar.dtype)
    if r:
        T = V[:, keep] / np.sqrt(d[keep])[None, :]
        C = T.T @ Ar @ T
        th, W = jacobi(0.5 * (C + C.T))
        order = np.argsort(-np.abs(th), kind="stable")
        nu[:r] = th[order]
        Q[:, :r] = T @ W[:, order]
    return nu, Q, r


def block_iteration(K_ff, H, theta=0.0, p=4, tol=1e-10, max_iters=256, check_every=4, dtype=np.float64):
    """The device's iteration at one shift.  Returns a dict: lam [p] (theta + 1 / nu, nearest theta first, NaN beyond
    n_modes), X [n, p], resid [p], n_modes = min(p, r), iters (0: the first n_modes residuals never all fell to tol at
    a check point) and pd (whether K_ff - theta H is positive definite; nothing else is set when it is not)."""
    n = len(K_ff)
    H = H.astype(dtype)
    Kbar = K_ff.astype(dtype) - dtype(theta) * H
    out = {"lam": np.full(p, np.nan), "X": np.zeros([n, p]), "resid": np.full(p, np.nan), "n_modes": 0, "iters": 0,
           "pd": True}
    try:
        np.linalg.cholesky(Kbar.astype(np.float64))
    except np.linalg.LinAlgError:
        out["pd"] = False
        return out
    if dtype is np.float64:
        solve = lambda F: np.linalg.solve(Kbar, F)
    else:   # (the plain elimination of the dynamics yardstick, in the type asked for)
        from tests.dynamics_reference import Eliminated
        solve = Eliminated(Kbar).solve
    F = mref.start_block(n, min(BLOCK, n)).astype(dtype)
    X = np.zeros([n, BLOCK], dtype=dtype)
    nu, resid = np.full(BLOCK, np.nan, dtype=dtype), np.full(BLOCK, np.nan, dtype=dtype)
    r = 0
    for it in range(1, max_iters + 1):
        Y = solve(F)
        G = H @ Y
        nu, Q, r = reduced_problem(Y.T @ G, Y.T @ F)
        X, GQ, FQ = Y @ Q, G @ Q, F @ Q
        n_modes = min(p, r)
        if it % check_every == 0 or it == max_iters:
            resid[:] = np.nan
            lp = nu[None, :r] * FQ[:, :r]
            with np.errstate(divide="ignore", invalid="ignore"):
                resid[:r] = np.sqrt(((GQ[:, :r] - lp) ** 2).sum(0) / (lp ** 2).sum(0))
            if np.all(resid[:n_modes] <= tol):
                out["iters"] = it
                break
        F = GQ
    n_modes = min(p, r)
    with np.errstate(divide="ignore"):
        out["lam"] = np.full(p, np.nan, dtype=dtype)
        out["lam"][:n_modes] = dtype(theta) + 1 / nu[:n_modes]
    out["X"][:, :n_modes] = X[:, :n_modes]
    out["resid"][:n_modes] = resid[:n_modes]
    out["n_modes"] = n_modes
    return out


def search(K_ff, H, p=4, shift=0.0, max_shifts=6, tol=1e-10, max_iters=256, check_every=4, dtype=np.float64):
    """The host's search for the smallest positive factor.  Round 0 runs at theta = `shift`.  After a round:
      - Kbar not positive definite: status NOT_PD, the outputs of the previous round are kept;
      - the round did not converge within max_iters: status ITER_LIMIT, bound = theta (Kbar is positive definite, so no
        positive factor lies at or below theta);
      - a positive lambda among the n_modes converged pairs: critical = the smallest of them, bound = critical, FOUND;
      - n_modes < p: the whole spectrum has been seen and holds no positive factor: critical NaN, bound +inf, NONE;
      - otherwise all p pairs are negative: no eigenvalue lies within d = max |lambda_i - theta| of theta, bound =
        theta + d; it is the next round's theta, or the search ends with SHIFT_LIMIT after max_shifts rounds.
    Returns a dict: factor [p], critical, critical_mode, bound, shift (of the last round), rounds, iters, resid [p],
    n_modes, X [n, p], status."""
    theta = float(shift)
    out = {"factor": np.full(p, np.nan), "critical": np.nan, "critical_mode": -1, "bound": 0.0, "shift": theta,
           "rounds": 0, "iters": 0, "resid": np.full(p, np.nan), "n_modes": 0, "X": np.zeros([len(K_ff), p]),
           "status": SHIFT_LIMIT}
    for rnd in range(max_shifts):
        res = block_iteration(K_ff, H, theta, p, tol, max_iters, check_every, dtype)
        out["rounds"] = rnd + 1
        if not res["pd"]:
            out["status"] = NOT_PD
            return out
        out.update(factor=res["lam"], resid=res["resid"], n_modes=res["n_modes"], X=res["X"], iters=res["iters"],
                   shift=theta, bound=theta)
        lam = res["lam"][:res["n_modes"]]
        if res["iters"] == 0:
            out["status"] = ITER_LIMIT
            return out
        if (lam > 0).any():
            k = int(np.where(lam > 0, lam, np.inf).argmin())
            out.update(critical=float(lam[k]), critical_mode=k, bound=float(lam[k]), status=FOUND)
            return out
        if res["n_modes"] < p:
            out.update(bound=np.inf, status=NONE)
            return out
        theta = theta + float(np.abs(lam - theta).max())
        out["bound"] = theta
    out["status"] = SHIFT_LIMIT
    return out
