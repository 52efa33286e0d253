"""`torch.autograd` entry point of the solver: a batch of trusses whose topology, supports and joint order are fixed,
solved as a differentiable function of the joint coordinates, the member areas and moduli and the loads.

    dt = DifferentiableTruss(packed, "cuda:0")
    A = dt.A.clone().requires_grad_()
    u, f_ext, N = dt.solve(dt.xyz, A, dt.E, loads)        # loads [B, L, nJ_max, 3]
    (u * loads).sum().backward()                           # A.grad: one substitution against the factor

The forward pass is `DeviceBatch.factor()` + `solve_cases()`, the backward pass `DeviceBatch.adjoint_cases()`
(HIP kernels of csrc/adjoint.hip): no finite differences and no second factorisation.  The factor and the forward
solution stay resident in the object between the two passes, so a backward pass belongs to the LAST forward pass of
its object: after another `solve()` the earlier graph can no longer be differentiated (ValueError).

    lam = dt.eigenvalues(dt.xyz, A, dt.E, p=4)              # [B, p], lambda = omega^2 of K phi = lambda M phi
    lam[:, 0].sqrt().sum().backward()                       # A.grad: one pass over the members, no solve

is the second differentiable function: forward `factor()` + `modes()`, backward `DeviceBatch.mode_gradients()`
(csrc/modegrad.hip) with the cotangent of lambda as the weights.  The same rule holds: a backward pass belongs to the
last forward pass of the object, whichever of the two functions that was."""
import torch

from .batch import DeviceBatch, PackedBatch, pack_trusses


class _Solve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, owner, xyz, A, E, loads):
        db = owner.batch
        owner._write_inputs(xyz, A, E)
        db.factor()
        out = db.solve_cases(loads.detach().contiguous())
        ctx.owner, ctx.generation = owner, db.generation
        ctx.set_materialize_grads(False)   # an unused result has NO cotangent: a NULL pointer, not a tensor of zeros
        return out["u"], out["f_ext"], out["N"]

    @staticmethod
    def backward(ctx, grad_u, grad_f_ext, grad_N):
        owner = ctx.owner
        needs = dict(zip(("xyz", "A", "E", "loads"), ctx.needs_input_grad[1:]))
        want = tuple(k for k in DeviceBatch.GRADIENTS if needs[k])
        owner.last_want = want
        if not want:
            return None, None, None, None, None
        if grad_u is None and grad_f_ext is None and grad_N is None:
            g = {k: None for k in want}
        else:
            g = owner.batch.adjoint_cases(grad_u, grad_f_ext, grad_N, want=want, generation=ctx.generation)
        return None, g.get("xyz"), g.get("A"), g.get("E"), g.get("loads")


class _Eigenvalues(torch.autograd.Function):
    @staticmethod
    def forward(ctx, owner, xyz, A, E, rho, joint_mass, p, mass_scale, tol, max_iters):
        db = owner.batch
        owner._write_inputs(xyz, A, E, rho)
        db.factor()
        out = db.modes(p, tol=tol, max_iters=max_iters, mass_scale=mass_scale,
                       joint_mass=None if joint_mass is None else joint_mass.detach().contiguous())
        ctx.owner, ctx.generation = owner, db.generation
        ctx.set_materialize_grads(False)
        owner.last_modes = out
        return out["lam"].clone()

    @staticmethod
    def backward(ctx, grad_lam):
        owner = ctx.owner
        needs = dict(zip(("xyz", "A", "E", "rho", "joint_mass"), ctx.needs_input_grad[1:6]))
        want = tuple(k for k in DeviceBatch.MODE_GRADIENTS if needs[k])
        owner.last_want = want
        if not want or grad_lam is None:
            return (None,) * 10
        # (the NaN tail of lambda gets no gradient: the kernel reads no weight beyond a truss's n_modes)
        g = owner.batch.mode_gradients(weights=grad_lam.contiguous(), want=want, generation=ctx.generation)
        g = {k: v[:, 0] for k, v in g.items() if k != "gap"}
        return (None, g.get("xyz"), g.get("A"), g.get("E"), g.get("rho"), g.get("joint_mass"), None, None, None, None)


class DifferentiableTruss:
    """A resident general-form `DeviceBatch` (staged pipeline, `use_small=False`) behind a `torch.autograd.Function`.
    `packed_or_trusses`: a `PackedBatch` or a list of `Truss`; `reorder` as `DeviceBatch` (the joint order is found
    once, here; tensors go in and come out in the caller's numbering).  `xyz`, `A`, `E` are the batch's own values as
    float64 device tensors [B, nJ_max, 3] / [B, nM_max] (caller's numbering) - starting points for the caller."""

    def __init__(self, packed_or_trusses, device=None, reorder=False, options=None):
        packed = packed_or_trusses if isinstance(packed_or_trusses, PackedBatch) else pack_trusses(list(packed_or_trusses))
        packed = packed.general()
        self.packed = packed
        self.batch = DeviceBatch(packed, device, use_small=False, reorder=reorder, options=options)
        dev = self.batch.device
        up = lambda a: torch.from_numpy(a.copy()).to(dev)
        self.xyz, self.A, self.E, self.rho = up(packed.xyz), up(packed.A), up(packed.E), up(packed.rho)
        #: the gradients the last backward pass asked `adjoint_cases` / `mode_gradients` for (the others got a NULL
        #: output pointer)
        self.last_want = None
        #: the dict the last `eigenvalues()` got from `DeviceBatch.modes` (phi, resid, n_modes, iters beside lam)
        self.last_modes = None

    @property
    def device(self):
        return self.batch.device

    def _write_inputs(self, xyz, A, E, rho=None):
        db = self.batch
        xyz = xyz.detach()
        if db.joint_out is not None:   # resident joint j is the caller's joint joint_out[j]
            xyz = torch.gather(xyz, 1, db.joint_out.long()[:, :, None].expand(-1, -1, 3))
        db.xyz.copy_(xyz)
        db.A.copy_(A.detach())
        db.E.copy_(E.detach())
        if rho is not None:
            db.rho.copy_(rho.detach())

    def solve(self, xyz, A, E, loads):
        """(u, f_ext, N) of every load case: u, f_ext [B, L, nJ_max, 3], N [B, L, nM_max], differentiable with respect
        to `xyz` [B, nJ_max, 3], `A`, `E` [B, nM_max] and `loads` [B, L, nJ_max, 3] (float64 tensors on this object's
        device).  `self.batch.info` holds the factorisation's status per truss."""
        db = self.batch
        shapes = {"xyz": (db.B, db.nJ_max, 3), "A": (db.B, db.nM_max), "E": (db.B, db.nM_max)}
        for name, x in (("xyz", xyz), ("A", A), ("E", E), ("loads", loads)):
            ok = x.dim() == 4 and (int(x.shape[0]), int(x.shape[2]), int(x.shape[3])) == (db.B, db.nJ_max, 3) \
                if name == "loads" else tuple(x.shape) == shapes[name]
            if not ok or x.dtype != torch.float64 or x.device != db.device:
                want = f"[{db.B}, L, {db.nJ_max}, 3]" if name == "loads" else list(shapes[name])
                raise ValueError(f"DifferentiableTruss.solve: {name} must be float64 {want} on {db.device}, "
                                 f"got {x.dtype} {list(x.shape)} on {x.device}")
        return _Solve.apply(self, xyz, A, E, loads)

    def eigenvalues(self, xyz, A, E, rho=None, joint_mass=None, p=6, mass_scale=1.0, tol=1e-10, max_iters=256):
        """lambda [B, p] = omega^2 of K phi = lambda M phi (lumped mass, `DeviceBatch.modes`; NaN beyond a truss's
        n_modes), differentiable with respect to `xyz` [B, nJ_max, 3], `A`, `E`, `rho` [B, nM_max] (None: the batch's
        own densities) and `joint_mass` [B, nJ_max] (caller's numbering, or None) - float64 tensors on this object's
        device.  Omega and f are the caller's `lam.sqrt()` and `lam.sqrt() / (2 pi)` in torch: d omega = d lambda /
        (2 omega).  The derivative is that of a SIMPLE eigenvalue; for a repeated one (symmetric trusses) differentiate
        the sum over the cluster (`DeviceBatch.mode_gradients` gives the gaps).  The NaN tail gets no gradient.
        `self.last_modes` keeps residuals, iteration counts and shapes of the forward pass."""
        db = self.batch
        rho = self.rho if rho is None else rho
        shapes = {"xyz": (db.B, db.nJ_max, 3), "A": (db.B, db.nM_max), "E": (db.B, db.nM_max), "rho": (db.B, db.nM_max),
                  "joint_mass": (db.B, db.nJ_max)}
        for name, x in (("xyz", xyz), ("A", A), ("E", E), ("rho", rho), ("joint_mass", joint_mass)):
            if x is None and name == "joint_mass":
                continue
            if tuple(x.shape) != shapes[name] or x.dtype != torch.float64 or x.device != db.device:
                raise ValueError(f"DifferentiableTruss.eigenvalues: {name} must be float64 {list(shapes[name])} on "
                                 f"{db.device}, got {x.dtype} {list(x.shape)} on {x.device}")
        return _Eigenvalues.apply(self, xyz, A, E, rho, joint_mass, int(p), float(mass_scale), float(tol), int(max_iters))
