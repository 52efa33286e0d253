"""Numpy reference of the eigenvalue gradients (test infrastructure, never imported by the package): a plain restatement
of the formulas of include/trs_modegrad.h on the shapes and eigenvalues it is GIVEN, in float64 or longdouble, an exact
variant that takes its pairs from `numpy.linalg.eigh` of M^-1/2 K_ff M^-1/2, and the eigenvalues of a perturbed design
for central differences."""
import numpy as np

from oracle import truss_oracle as orc

KEYS = ("A", "E", "rho", "xyz", "joint_mass")


def arrays(data, joint_mass=None):
    """A JSON truss as arrays: xyz [nJ, 3] (z = 0 for a 2D truss), conn [nM, 2], A, E, rho [nM], free [nJ, 3] (bool),
    joint_mass [nJ] (zeros when None)."""
    p = orc.prepare(data)
    nJ, dim = len(p.pos), p.dim
    xyz = np.zeros([nJ, 3])
    xyz[:, :dim] = np.asarray(p.pos, dtype=float)
    free = np.zeros([nJ, 3], dtype=bool)
    free[:, :dim] = orc.free_mask(p).reshape(nJ, dim)
    mem = np.asarray(p.members, dtype=float).reshape(-1, 5)
    jm = np.zeros(nJ) if joint_mass is None else np.asarray(joint_mass, dtype=float)[:nJ].copy()
    return {"xyz": xyz, "conn": mem[:, :2].astype(np.int64), "A": mem[:, 2].copy(), "E": mem[:, 3].copy(),
            "rho": mem[:, 4].copy(), "free": free, "joint_mass": jm}


def system(d, mass_scale=1.0):
    """(K_ff, m) over the free DOFs of the arrays `d`: the stiffness matrix and the lumped mass of include/trs_modes.h."""
    xyz, conn = d["xyz"], d["conn"]
    nJ = len(xyz)
    D = xyz[conn[:, 1]] - xyz[conn[:, 0]]
    length = np.sqrt((D * D).sum(1))
    c = D / length[:, None]
    k = d["E"] * d["A"] / length
    K = np.zeros([nJ, 3, nJ, 3])
    blocks = k[:, None, None] * c[:, :, None] * c[:, None, :]
    for (j0, j1), blk in zip(conn, blocks):
        K[j0, :, j0] += blk
        K[j1, :, j1] += blk
        K[j0, :, j1] -= blk
        K[j1, :, j0] -= blk
    half = 0.5 * (d["A"] * length * d["rho"])
    mj = np.zeros(nJ)
    np.add.at(mj, conn[:, 0], half)
    np.add.at(mj, conn[:, 1], half)
    mj = mass_scale * mj + d["joint_mass"]
    free = d["free"].ravel()
    K = K.reshape(3 * nJ, 3 * nJ)
    return K[free][:, free], np.repeat(mj, 3)[free]


def eigen_pairs(d, mass_scale=1.0, p=None):
    """(lam [n] ascending, Phi [p, nJ, 3] M-orthonormal in joint layout, zero at held DOFs) from `eigh` of
    M^-1/2 K_ff M^-1/2 (positive masses).  `p` None: every pair."""
    K_ff, m = system(d, mass_scale)
    s = 1.0 / np.sqrt(m)
    lam, V = np.linalg.eigh(K_ff * s[:, None] * s[None, :])
    p = len(lam) if p is None else min(p, len(lam))
    Phi = np.zeros([p, d["free"].size])
    Phi[:, d["free"].ravel()] = (V[:, :p] * s[:, None]).T
    return lam, Phi.reshape(p, -1, 3)


def eigenvalues(d, mass_scale=1.0):
    K_ff, m = system(d, mass_scale)
    s = 1.0 / np.sqrt(m)
    return np.linalg.eigvalsh(K_ff * s[:, None] * s[None, :])


def gaps(lam, count=None):
    """gap_k = min over i != k, i < count, of |lam_i - lam_k| / |lam_k| (inf where there is no other)."""
    lam = np.asarray(lam, dtype=float)[:count]
    out = np.full(len(lam), np.inf)
    for k in range(len(lam)):
        other = np.delete(lam, k)
        if len(other):
            out[k] = np.abs(other - lam[k]).min() / abs(lam[k])
    return out


def gradients(d, phi, lam, mass_scale=1.0, dtype=np.float64):
    """The formulas of include/trs_modegrad.h for the shapes `phi` [p, nJ, 3] (joint layout, M-orthonormal, zero at held
    DOFs) and eigenvalues `lam` [p] as given, evaluated in `dtype`: a dict A, E, rho [p, nM], xyz [p, nJ, 3],
    joint_mass [p, nJ].  Rows whose `lam` is NaN are zero."""
    f = lambda x: np.asarray(x, dtype=dtype)
    xyz, conn, A, E, rho = f(d["xyz"]), d["conn"], f(d["A"]), f(d["E"]), f(d["rho"])
    phi, lam, mu = f(phi), f(lam), dtype(mass_scale)
    p, nJ, nM = len(lam), len(xyz), len(conn)
    j0, j1 = conn[:, 0], conn[:, 1]
    D = xyz[j1] - xyz[j0]
    length = np.sqrt((D * D).sum(1))
    c = D / length[:, None]
    k = E * A / length
    half = dtype(0.5)
    out = {"A": np.zeros([p, nM], dtype), "E": np.zeros([p, nM], dtype), "rho": np.zeros([p, nM], dtype),
           "xyz": np.zeros([p, nJ, 3], dtype), "joint_mass": np.zeros([p, nJ], dtype)}
    for r in range(p):
        if np.isnan(lam[r]):
            continue
        ph, l = phi[r], lam[r]
        Dphi = ph[j1] - ph[j0]
        s = (c * Dphi).sum(1)
        h = (ph[j0] * ph[j0]).sum(1) + (ph[j1] * ph[j1]).sum(1)
        out["A"][r] = (E / length) * s * s - l * mu * half * length * rho * h
        out["E"][r] = (A / length) * s * s
        out["rho"][r] = -l * mu * half * A * length * h
        out["joint_mass"][r] = -l * (ph * ph).sum(1)
        g = (k / length * s)[:, None] * (2 * Dphi - 3 * s[:, None] * c) - (l * mu * half * A * rho * h)[:, None] * c
        for m in range(nM):     # member-id order
            out["xyz"][r, j1[m]] += g[m]
            out["xyz"][r, j0[m]] -= g[m]
    return out


def exact_gradients(d, p, mass_scale=1.0, dtype=np.float64):
    """(lam [p], gaps [p] against the whole spectrum, gradients) with the pairs of `eigen_pairs`."""
    lam, Phi = eigen_pairs(d, mass_scale, p)
    return lam[:len(Phi)], np.array([gaps(lam)[k] for k in range(len(Phi))]), gradients(d, Phi, lam[:len(Phi)], mass_scale, dtype)


def scaled_difference(got, want):
    """max |got - want| / max |want| (0 when both are all zero)."""
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    scale = np.abs(want).max() if want.size else 0.0
    diff = np.abs(got - want).max() if want.size else 0.0
    return float(diff / scale) if scale > 0 else float(diff)


def central_differences(d, key, fn, mass_scale=1.0, rel=1e-5):
    """d fn(eigenvalues) / d (every entry of d[key]) by central differences, step `rel` times the entry (coordinates:
    times the truss's largest coordinate; joint masses: times the largest lumped mass).  `fn` maps the ascending
    eigenvalues to a vector; returns an array of shape fn(.).shape + d[key].shape."""
    base = d[key]
    if key == "xyz":
        scale = np.full(base.shape, np.abs(base).max())
    elif key == "joint_mass":
        scale = np.full(base.shape, system(d, mass_scale)[1].max())
    else:
        scale = np.abs(base)
    out = None
    for idx in np.ndindex(base.shape):
        step = rel * scale[idx]
        vals = []
        for sign in (1.0, -1.0):
            x = base.copy()
            x[idx] += sign * step
            vals.append(np.asarray(fn(eigenvalues(dict(d, **{key: x}), mass_scale))))
        col = (vals[0] - vals[1]) / (2.0 * step)
        if out is None:
            out = np.zeros(col.shape + base.shape)
        out[(Ellipsis,) + idx] = col
    return out
