"""Numpy yardstick of the member sizing (test infrastructure, never imported by the package): fully stressed design
with a displacement envelope, the stress-ratio method of include/trs_sizing.h stated on a dense stiffness matrix, in any
floating-point type - `numpy.float64`, or `numpy.longdouble` to measure what float64 itself loses.  The linear systems
are solved by the plain elimination of `tests/dynamics_reference.Eliminated`, so both types run the same algorithm.

The method (the header, the kernel and this file state it in the same words).  Inputs: L load cases (joint forces), the
scalars allow_tension > 0, allow_compression > 0, allow_displace (0 = no limit), euler_kappa >= 0 (the member's second
moment of area as I = kappa A^2, 1/(4 pi) for a solid round bar, 0 = no member buckling check), relax in (0, 1],
tol >= 0, max_iters >= 0, and per member a_min > 0 and a_max >= a_min.  The initial design is the truss's own A (> 0).
Analysis k (k = 0, 1, ...) of design A_k:
  - for each case l, N_ml = (E A_k / L0) c.(u_j1 - u_j0);
  - the required area in case l is N / allow_tension for N > 0; for P = -N > 0 it is
    max(P / allow_compression, sqrt(P L0^2 / (pi^2 E kappa))), the second term only when kappa > 0;
  - req_m is the maximum over the cases, taken in ascending l; on a tie the lowest l governs;
  - d = max over cases and the truss's joints of |u_j| / allow_displace; 0 without a limit;
  - r_m = max(req_m / A_m, d);
  - A'_m = clamp(A_m ((1 - relax) + relax r_m), a_min_m, a_max_m);
  - change = max_m |A'_m - A_m| / A_m over the truss's live members;
  - if change <= tol the truss is converged (status 0) and keeps A_k;
  - otherwise, if k = max_iters, the truss gets status 1 and keeps A_k;
  - otherwise A_{k+1} = A' and the truss's `iterations` becomes k + 1;
  - if the factorisation of A_k reports info != 0 the truss gets status 2, its design goes back to A_{k-1}, and its
    outputs (iterations among them) stay those of analysis k - 1; for k = 0 the outputs are zero (governing -1: nothing
    was analysed), the areas are the initial ones and `iterations` is 0.
No thresholds on small forces: a zero-force member has r = d and ends on its lower bound.  `governing` is the case l
whose requirement governs r_m, or -1 where the displacement ratio does (d > req_m / A_m)."""
import numpy as np

from oracle import truss_oracle as orc
from tests.dynamics_reference import Eliminated
from tests.nonlinear_reference import positive_definite

ACTIVE, CONVERGED, ITER_LIMIT, NOT_PD = -1, 0, 1, 2
#: two candidates for r_m closer than this (times the truss's largest r) leave `governing` to the rounding
AMBIGUOUS = 1e-9
COMPARED = ("areas", "weight", "weight_history", "utilisation", "disp_ratio")


class Geometry:
    """What does not change with the areas: end joints, direction cosines, lengths, moduli, densities, in `dtype`."""

    def __init__(self, data, dtype):
        p = orc.prepare(data)
        self.p, self.dim, self.nJ, self.dtype = p, p.dim, len(p.pos), dtype
        X = np.asarray(p.pos, dtype=dtype)
        self.j0 = np.array([m[0] for m in p.members], dtype=np.int64)
        self.j1 = np.array([m[1] for m in p.members], dtype=np.int64)
        D = X[self.j1] - X[self.j0]
        self.L02 = (D * D).sum(axis=1)
        self.L0 = np.sqrt(self.L02)
        self.c = D / self.L0[:, None]
        self.A0 = np.array([m[2] for m in p.members], dtype=dtype)
        self.E = np.array([m[3] for m in p.members], dtype=dtype)
        self.rho = np.array([m[4] for m in p.members], dtype=dtype)
        self.mask = orc.free_mask(p)

    def stiffness(self, A):
        """The reduced stiffness matrix of the design A: sum over the members of (E A / L0) c c^T blocks."""
        dim, n = self.dim, self.nJ * self.dim
        K = np.zeros([n, n], dtype=self.dtype)
        k = self.E * A / self.L0
        for m in range(len(A)):
            kcc = k[m] * np.outer(self.c[m], self.c[m])
            s0 = slice(self.j0[m] * dim, (self.j0[m] + 1) * dim)
            s1 = slice(self.j1[m] * dim, (self.j1[m] + 1) * dim)
            K[s0, s0] += kcc
            K[s1, s1] += kcc
            K[s0, s1] -= kcc
            K[s1, s0] -= kcc
        return K[self.mask][:, self.mask]

    def forces(self, A, u):
        """N [L, nM] of the design A under displacements u [L, nJ, dim]."""
        proj = ((u[:, self.j1] - u[:, self.j0]) * self.c[None]).sum(axis=2)
        return (self.E * A / self.L0)[None] * proj

    def weight(self, A):
        return (A * self.L0 * self.rho).sum()


def analyse(geo, A, loads, allow_tension, allow_compression, allow_displace=0.0, euler_kappa=0.0, solve=None):
    """One analysis of the design A under `loads` [L, nJ, dim]: None when the reduced stiffness matrix is not positive
    definite, else a dict with u [L, nJ, dim], N [L, nM], required [L, nM] (the required area per case), req, case [nM]
    (the maximum and the first case that attains it), utilisation [nM], disp_ratio, r [nM], governing [nM], weight and
    ambiguous [nM] (bool: the two largest candidates for r_m lie within AMBIGUOUS of the truss's largest r)."""
    dtype = geo.dtype
    K = geo.stiffness(A)
    if not positive_definite(K):
        return None
    L = len(loads)
    P = np.asarray(loads, dtype=dtype).reshape(L, -1)[:, geo.mask].T
    x = Eliminated(K).solve(P) if solve is None else np.asarray(solve(K.astype(np.float64), P.astype(np.float64)), dtype=dtype)
    u = np.zeros([L, geo.nJ * geo.dim], dtype=dtype)
    u[:, geo.mask] = x.T
    u = u.reshape(L, geo.nJ, geo.dim)
    N = geo.forces(A, u)
    at, ac, kappa = dtype(allow_tension), dtype(allow_compression), dtype(euler_kappa)
    comp = np.maximum(-N, 0)
    required = np.where(N > 0, N / at, comp / ac)
    if euler_kappa > 0:
        pi = dtype(np.pi) if dtype is np.float64 else np.arctan(dtype(1)) * 4
        euler = np.sqrt(comp * ((geo.L0 * geo.L0) / ((pi * pi * geo.E) * kappa))[None])
        required = np.where(N < 0, np.maximum(required, euler), required)
    case = required.argmax(axis=0)          # (the first of equal maxima: the lowest l)
    req = required.max(axis=0)
    util = req / A
    d = dtype(0)
    if allow_displace > 0:
        d = np.sqrt((u * u).sum(axis=2)).max() / dtype(allow_displace)
    r = np.maximum(util, d)
    governing = np.where(d > util, -1, case).astype(np.int32)
    cand = required / A[None]
    if allow_displace > 0:
        cand = np.concatenate([cand, np.full([1, len(A)], d, dtype=dtype)], axis=0)
    top = np.sort(cand, axis=0)[::-1]
    second = top[1] if len(top) > 1 else np.full(len(A), -np.inf)
    ambiguous = (top[0] - second) <= dtype(AMBIGUOUS) * r.max()
    return {"u": u, "N": N, "required": required, "req": req, "case": case, "utilisation": util, "disp_ratio": d, "r": r,
            "governing": governing, "weight": geo.weight(A), "ambiguous": ambiguous}


def snap(A, catalog):
    """(areas, index): every area to the smallest catalogue entry >= it, the largest where there is none."""
    cat = np.asarray(catalog, dtype=A.dtype)
    idx = np.minimum(np.searchsorted(cat, A, side="left"), len(cat) - 1)
    return cat[idx], idx.astype(np.uint8)


def size(data, loads, allow_tension, allow_compression, allow_displace=0.0, euler_kappa=0.0, area_min=None, area_max=None,
         relax=1.0, tol=1e-4, max_iters=40, catalog=None, dtype=np.float64, solve=None, areas=None):
    """The sizing of one truss.  loads [L, nJ, dim]; area_min, area_max scalars or [nM]; `areas`: another initial design
    than the truss's own.  Returns a dict: areas, utilisation [nM], governing (int32 [nM]), weight, disp_ratio,
    iterations, status, info (0, or 1 for a design that could not be factored), weight_history [max_iters + 1],
    catalog_index (uint8 [nM], with `catalog`), and per analysis of the loop: changes (list), ambiguous (list of bool
    [nM]); `ambiguous_last` is that of the analysis the outputs describe."""
    geo = Geometry(data, dtype)
    nM = len(geo.A0)
    lo = np.broadcast_to(np.asarray(area_min, dtype=dtype), [nM])
    hi = np.broadcast_to(np.asarray(area_max, dtype=dtype), [nM])
    A = geo.A0.copy() if areas is None else np.asarray(areas, dtype=dtype).copy()
    kw = dict(allow_tension=allow_tension, allow_compression=allow_compression, allow_displace=allow_displace,
              euler_kappa=euler_kappa, solve=solve)
    out = {"areas": A.copy(), "utilisation": np.zeros(nM, dtype=dtype), "governing": np.full(nM, -1, dtype=np.int32),
           "weight": dtype(0), "disp_ratio": dtype(0), "iterations": 0, "status": ACTIVE, "info": 0,
           "weight_history": np.zeros(max_iters + 1, dtype=dtype), "changes": [], "ambiguous": [],
           "ambiguous_last": np.zeros(nM, dtype=bool)}

    def report(an, design):
        out.update(areas=design.copy(), utilisation=an["utilisation"], governing=an["governing"], weight=an["weight"],
                   disp_ratio=an["disp_ratio"], ambiguous_last=an["ambiguous"])

    one, rx = dtype(1), dtype(relax)
    k = 0
    while True:
        an = analyse(geo, A, loads, **kw)
        if an is None:                      # the outputs stay those of analysis k - 1
            out["status"], out["info"] = NOT_PD, 1
            out["iterations"] = max(k - 1, 0)
            break
        report(an, A)
        out["weight_history"][k] = an["weight"]
        out["ambiguous"].append(an["ambiguous"])
        new = np.minimum(np.maximum(A * ((one - rx) + rx * an["r"]), lo), hi)
        change = (np.abs(new - A) / A).max() if nM else dtype(0)
        out["changes"].append(change)
        if change <= dtype(tol):
            out["status"] = CONVERGED
            break
        if k == max_iters:
            out["status"] = ITER_LIMIT
            break
        A = new
        k += 1
        out["iterations"] = k
    if catalog is not None and out["status"] in (CONVERGED, ITER_LIMIT):
        snapped, idx = snap(out["areas"], catalog)
        an = analyse(geo, snapped, loads, **kw)
        out["catalog_index"] = idx
        if an is not None:
            report(an, snapped)
        else:
            out["areas"], out["info"] = snapped, 1
    return out


def relative_difference(x, y):
    """The largest max-scaled difference between two `size` results over COMPARED."""
    worst = 0.0
    for key in COMPARED:
        a, b = np.asarray(x[key], dtype=np.longdouble), np.asarray(y[key], dtype=np.longdouble)
        scale = float(np.abs(b).max())
        if scale > 0:
            worst = max(worst, float(np.abs(a - b).max()) / scale)
    return worst


# ---- the inputs that the CPU and the GPU tests share -------------------------------------------------------------------
#: the ragged batch of the GPU tests, and the large truss
BATCH = ("bar-6_input_0", "bar-10_input_0", "bar-25_input_0", "bar-47_input_0", "bar-72_input_0", "bar-120_input_0")
BIG = "bar-942_input_0"
CONFIGS = ("stress", "disp", "euler")
DEPTH = 6              # the parity at a fixed depth: tol = 0, max_iters = DEPTH
FULL = {"tol": 1e-4, "max_iters": 40}
#: what a throwaway prototype of the method gave for (status, iterations) under FULL; the yardstick is the authority
TABLE = {"stress": {"bar-6": (0, 3), "bar-10": (0, 9), "bar-25": (1, 40), "bar-47": (1, 40), "bar-72": (0, 23),
                    "bar-120": (0, 27), "bar-942": (1, 40)},
         "disp": {"bar-6": (0, 12), "bar-10": (0, 20), "bar-25": (0, 7), "bar-47": (0, 8), "bar-72": (0, 8),
                  "bar-120": (0, 9), "bar-942": (0, 5)}}


def cases(data):
    """[2, nJ, dim]: case 0 the fixture's own forces f0, case 1 [j, a] = 0.3 f0[j, a] - 0.5 f0[j, dim - 1 - a]."""
    p = orc.prepare(data)
    f0 = orc.force_vector(p).reshape(len(p.pos), p.dim)
    return np.stack([f0, 0.3 * f0 - 0.5 * f0[:, ::-1]])


def config(data, which, solve=None):
    """The keyword arguments of `size` (and, renamed, of the device) for one of CONFIGS on a fixture: the allowables from
    s0 and d0, the largest |N| / A and the largest joint displacement norm of the initial design over both cases."""
    geo = Geometry(data, np.float64)
    loads = cases(data)
    an = analyse(geo, geo.A0, loads, 1.0, 1.0, solve=solve)
    s0 = float((np.abs(an["N"]) / geo.A0[None]).max())
    d0 = float(np.sqrt((an["u"] ** 2).sum(axis=2)).max())
    kw = {"loads": loads, "allow_tension": 0.5 * s0, "allow_compression": 0.4 * s0, "allow_displace": 0.0,
          "euler_kappa": 0.0, "area_min": 0.1 * float(geo.A0.min()), "area_max": 1000.0 * float(geo.A0.max()), "relax": 1.0}
    if which == "disp":
        kw["allow_displace"] = 0.5 * d0
    elif which == "euler":
        kw.update(euler_kappa=1.0 / (4.0 * np.pi), relax=0.7)
    elif which != "stress":
        raise ValueError(which)
    return kw


def ladder(datas, count=16):
    """A geometric ladder of `count` catalogue areas for a batch: from the smallest area_min of its trusses to 30 x the
    largest initial area."""
    areas = np.concatenate([Geometry(data, np.float64).A0 for data in datas])
    return np.geomspace(0.1 * float(areas.min()), 30.0 * float(areas.max()), count)
