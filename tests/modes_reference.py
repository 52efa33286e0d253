"""Numpy reference of the natural frequencies (test infrastructure, never imported by the package): the lumped mass
matrix of include/trs_modes.h built from the JSON, the generalised eigenproblem K_ff phi = lambda M phi through
`numpy.linalg.eigvalsh` on the oracle's own matrices, and a plain restatement of the block inverse iteration the device
runs (Cholesky of M_r, cyclic Jacobi on the reduced matrix, residual without a stiffness product, check points)."""
import numpy as np

from oracle import truss_oracle as orc

BLOCK = 16


def joint_masses(data, joint_mass=None, mass_scale=1.0):
    """m_j = mass_scale * sum over the member ends at j of 1/2 (a * length * density) + joint_mass_j, members in id order."""
    p = orc.prepare(data)
    m = np.zeros(len(p.pos))
    for (j0, j1, a, _e, rho), length in zip(p.members, p.lengths):
        half = 0.5 * (a * length * rho)
        m[j0] += half
        m[j1] += half
    m = mass_scale * m
    if joint_mass is not None:
        m = m + np.asarray(joint_mass, dtype=float)[:len(m)]
    return m


def matrices(data, joint_mass=None, mass_scale=1.0):
    """(K_ff, the diagonal of M over the free DOFs, the free mask) of one truss, in the oracle's numbering."""
    p = orc.prepare(data)
    mask = orc.free_mask(p)
    K = orc.global_K(p)
    K_ff = K[mask, :][:, mask]
    m = np.repeat(joint_masses(data, joint_mass, mass_scale), p.dim)[mask]
    return K_ff, m, mask


def eigenvalues(K_ff, m):
    """Ascending eigenvalues of K_ff phi = lambda M phi for a positive diagonal M: eigvalsh(M^-1/2 K_ff M^-1/2)."""
    s = 1.0 / np.sqrt(m)
    return np.linalg.eigvalsh(K_ff * s[:, None] * s[None, :])


def eigenvalues_semidefinite(K_ff, m):
    """The finite eigenvalues when some masses are zero: reciprocals of the non-zero eigenvalues of
    M^1/2 inv(K_ff) M^1/2, ascending."""
    s = np.sqrt(m)
    mu = np.linalg.eigvalsh(np.linalg.inv(K_ff) * s[:, None] * s[None, :])
    mu = mu[mu > 1e-12 * mu.max()]
    return np.sort(1.0 / mu)


def start_block(n, q):
    """X[c][k] = one splitmix64 step of 16 c + k + 1, mapped into (-1, 1); the columns k >= q are zero."""
    c, k = np.meshgrid(np.arange(n, dtype=np.uint64), np.arange(BLOCK, dtype=np.uint64), indexing="ij")
    with np.errstate(over="ignore"):
        z = (c * np.uint64(BLOCK) + k + np.uint64(1)) * np.uint64(0x9e3779b97f4a7c15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
        z = z ^ (z >> np.uint64(31))
    X = ((z >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 4503599627370496.0) - 1.0
    X[:, q:] = 0.0
    return X


def jacobi(C, sweeps=30):
    """Cyclic Jacobi in the round-robin order on a symmetric matrix: (eigenvalues, eigenvectors), unsorted."""
    q = len(C)
    A, W = C.copy(), np.eye(q)
    for _ in range(sweeps):
        rotated = False
        for rnd in range(BLOCK - 1):
            pairs = [(BLOCK - 1, rnd)] + [((rnd + k) % (BLOCK - 1), (rnd - k) % (BLOCK - 1)) for k in range(1, 8)]
            J = np.eye(q)
            for a, c in pairs:
                if a >= q or c >= q:
                    continue
                apq = A[a, c]
                if abs(apq) > 2.0 ** -53 * np.sqrt(abs(A[a, a] * A[c, c])) and apq != 0.0:
                    tau = (A[c, c] - A[a, a]) / (2.0 * apq)
                    t = (1.0 if tau >= 0 else -1.0) / (abs(tau) + np.sqrt(1.0 + tau * tau))
                    cs = 1.0 / np.sqrt(1.0 + t * t)
                    J[a, a] = J[c, c] = cs
                    J[a, c], J[c, a] = t * cs, -t * cs
                    rotated = True
            A, W = J.T @ A @ J, W @ J
        if not rotated:
            break
    return np.diag(A).copy(), W


def block_iteration(K_ff, m, p=8, tol=1e-10, max_iters=256, check_every=8):
    """The device's iteration in numpy: returns (lam [p] with NaN beyond n_modes, Phi [n, p], resid [p], n_modes,
    iters - 0 when the first n_modes residuals never all fell to tol at a check point)."""
    n = len(m)
    n_mass = int((m > 0).sum())
    q, n_modes = min(BLOCK, n_mass), min(p, n_mass)
    X = start_block(n, q)
    lam, resid = np.full(BLOCK, np.nan), np.full(BLOCK, np.nan)
    iters = 0
    for it in range(1, max_iters + 1):
        Y = np.linalg.solve(K_ff, m[:, None] * X)
        Kr = Y[:, :q].T @ (m[:, None] * X[:, :q])
        Mr = Y[:, :q].T @ (m[:, None] * Y[:, :q])
        Kr, Mr = 0.5 * (Kr + Kr.T), 0.5 * (Mr + Mr.T)
        Lc = np.linalg.cholesky(Mr)
        C = np.linalg.solve(Lc, np.linalg.solve(Lc, Kr).T).T
        theta, W = jacobi(0.5 * (C + C.T))
        order = np.argsort(theta, kind="stable")
        Q = np.zeros([BLOCK, BLOCK])
        Q[:q, :q] = np.linalg.solve(Lc.T, W[:, order])
        lam[:q] = theta[order]
        Phi, XQ = Y @ Q, X @ Q
        if it % check_every == 0 or it == max_iters:
            lp = lam[None, :q] * Phi[:, :q]
            resid[:q] = np.sqrt((m[:, None] * (XQ[:, :q] - lp) ** 2).sum(0) / (m[:, None] * lp ** 2).sum(0))
        X = Phi
        if it % check_every == 0 and np.all(resid[:n_modes] <= tol):
            iters = it
            break
    out_lam = np.full(p, np.nan)
    out_lam[:n_modes] = lam[:n_modes]
    Phi = X[:, :p].copy()
    Phi[:, n_modes:] = 0.0
    return out_lam, Phi, resid[:p].copy(), n_modes, iters
