"""`Member` and `Truss`: the Python model whose `Truss.Solve()` is the drop-in boundary.

Public names, argument meaning, result shapes (sparse dicts with the 1e-10 threshold)
and exceptions follow the reference's `slientruss3d/truss.py:10-466`.  What differs is
what happens inside `Solve()`: the reference assembles and solves one truss in Python
and numpy (`truss.py:329-364`); here `Solve()` is a batch-of-one call into the batched
HIP solver (`batch.solve_batch`), which needs a GPU and the in-tree C-ABI library and
raises `HipExtensionError` otherwise - there is no CPU fallback.
"""
import copy
import json
import math
from pprint import pformat

import numpy as np

from .type import MemberType, SupportType
from .utils import (CheckDim, DimensionError, GetLength, InvaildJointError, IsZero,
                    IsZeroVector, NotAllBeSetError, TrussNotSolvedError,
                    TrussNotStableError, ZERO_EPS)


def _distance(p, q):
    """sqrt of the sum of the squared differences - the squares as `x ** 2.0`, summed left to right, exactly as
    the generic form `sqrt(sum((b - a) ** 2.0 ...))` rounds (unrolled: this runs once per member of every truss
    object that is built)."""
    if len(p) == 3:
        return math.sqrt((q[0] - p[0]) ** 2.0 + (q[1] - p[1]) ** 2.0 + (q[2] - p[2]) ** 2.0)
    if len(p) == 2:
        return math.sqrt((q[0] - p[0]) ** 2.0 + (q[1] - p[1]) ** 2.0)
    return math.sqrt(sum((b - a) ** 2.0 for a, b in zip(p, q)))


class Member:
    """One bar between two joint positions (reference `truss.py:10-106`)."""

    def __init__(self, joint0, joint1, dim=3, memberType=None):
        self._dim = CheckDim(dim)
        if len(joint0) != dim or len(joint1) != dim:
            raise DimensionError(
                f"Dimension of each joint must be {dim}, but got dim(joint0) = {len(joint0)} "
                f"and dim(joint1) = {len(joint1)}.")
        self._ends = [joint0, joint1]
        # The instance is kept, not copied: two members given the same MemberType object
        # stay aliased through `memberType = ...` exactly as in the reference
        # (`truss.py:16-18,44-46`).
        self._type = MemberType() if memberType is None else memberType
        self._length = _distance(joint0, joint1)

    def __repr__(self):
        return f"Member[{self._ends[0]}, {self._ends[1]}, k={self.k :.4f}]"

    dim = property(lambda self: self._dim)
    e = property(lambda self: self._type.e)
    a = property(lambda self: self._type.a)
    density = property(lambda self: self._type.density)
    length = property(lambda self: self._length)

    @property
    def memberType(self):
        return self._type.Copy()

    @memberType.setter
    def memberType(self, other):
        self._type.Set(other)

    @property
    def weight(self):
        return self.a * self._length * self.density

    @property
    def k(self):
        """Axial stiffness E*A/L (`truss.py:56-58`)."""
        return self.e * self.a / self._length

    @property
    def cosines(self):
        p, q = self._ends
        return [(q[i] - p[i]) / self._length for i in range(self._dim)]

    @property
    def matK(self):
        """2*dim x 2*dim local stiffness k*[[cc^T, -cc^T], [-cc^T, cc^T]] (`truss.py:65-86`)."""
        c = np.asarray(self.cosines, dtype=float)
        block = np.outer(c, c)
        return self.k * np.block([[block, -block], [-block, block]])

    def IsTension(self, forceVec):
        """True when the force on joint1 points away from joint0 (`truss.py:89-91`)."""
        axis = np.asarray(self._ends[1], dtype=float) - np.asarray(self._ends[0], dtype=float)
        return bool(np.dot(axis, forceVec) > 0)

    def SetPosition(self, jointID_0or1, position):
        if jointID_0or1 not in (0, 1):
            raise KeyError("[jointID_0or1] must be 0 or 1.")
        self._ends[jointID_0or1] = position
        self._length = _distance(self._ends[0], self._ends[1])

    def Serialize(self):
        return {"joint0": list(self._ends[0]), "joint1": list(self._ends[1]),
                "memberType": self._type.Serialize()}

    def Copy(self):
        return Member(tuple(self._ends[0]), tuple(self._ends[1]), self._dim, self._type.Copy())


class Truss:
    """A 2D/3D pin-jointed truss (reference `truss.py:109-466`).

    Joint and member IDs are consecutive integers in insertion order (`truss.py:175,185`);
    the DOF of (joint j, axis a) is j*dim + a (`truss.py:312-314,324`).
    """

    def __init__(self, dim):
        self._dim = CheckDim(dim)
        self._pos = []        # jointID -> tuple of dim floats
        self._sup = []        # jointID -> SupportType value
        self._loads = {}      # jointID -> tuple of dim floats, insertion ordered
        self._ends = []       # memberID -> (jointID0, jointID1)
        self._bars = []       # memberID -> Member
        self._clear_results()

    def _clear_results(self):
        self._displace = None
        self._external = None
        self._internal = None
        self._solved = False

    def __repr__(self):
        bar = "-" * 30

        def section(title, body):
            return f"{bar}\n{title}\n{bar}\n{body}\n\n"

        solved = self._solved
        return (object.__repr__(self) + "\n"
                + section("Joints :", pformat(self.GetJoints()))
                + section("Forces :", pformat(self._loads))
                + section("Members :", pformat(self.GetMembers(False)))
                + section("Displaces:", pformat(self._displace) if solved else "(Not Solved)")
                + section("Internals:", pformat(self._internal) if solved else "(Not Solved)")
                + section("Externals:", pformat(self._external) if solved else "(Not Solved)"))

    # ------------------------------------------------------------------ counts
    dim = property(lambda self: self._dim)
    nJoint = property(lambda self: len(self._pos))
    nMember = property(lambda self: len(self._bars))
    nForce = property(lambda self: len(self._loads))
    isSolved = property(lambda self: self._solved)

    @property
    def nSupport(self):
        return sum(1 for s in self._sup if s != SupportType.NO)

    @property
    def nResistance(self):
        return sum(SupportType.GetResistanceNumber(s, self._dim) for s in self._sup)

    @property
    def isStable(self):
        """Necessary-only counting test of the reference (`truss.py:158-164`)."""
        nRes = self.nResistance
        enough = self.nMember + nRes >= self.nJoint * self._dim
        return enough if self._dim == 2 else (nRes >= 6 and enough)

    @property
    def weight(self):
        return sum(bar.weight for bar in self._bars)

    # ---------------------------------------------------------------- builders
    def AddNewJoint(self, vector, supportType=SupportType.NO):
        self._pos.append(tuple(float(vector[i]) for i in range(self._dim)))
        self._sup.append(supportType)

    def AddExternalForce(self, jointID, vector):
        if not (isinstance(jointID, (int, np.integer)) and 0 <= jointID < len(self._pos)):
            raise InvaildJointError(f"No such joint [{jointID}], can't add force on it.")
        if not IsZeroVector(vector):  # zero loads are dropped (`truss.py:181-182`)
            self._loads[int(jointID)] = tuple(float(vector[i]) for i in range(self._dim))

    def AddNewMember(self, jointID0, jointID1, memberType):
        self._ends.append((jointID0, jointID1))
        self._bars.append(Member(self._pos[jointID0], self._pos[jointID1], self._dim, memberType))

    # ----------------------------------------------------------------- setters
    def SetJointPosition(self, jointID, position):
        self._pos[jointID] = position
        for (j0, j1), bar in zip(self._ends, self._bars):
            if j0 == jointID:
                bar.SetPosition(0, position)
            if j1 == jointID:
                bar.SetPosition(1, position)

    def SetJointPositions(self, jointPositionDict):
        for jointID, position in jointPositionDict.items():
            self.SetJointPosition(jointID, position)

    def SetSupportType(self, jointID, supportType):
        # The reference assigns into a tuple here and raises TypeError (`truss.py:198-203`);
        # this implementation performs the documented intent.  See INTEGRATION.md.
        self._sup[jointID] = supportType

    def SetSupportTypes(self, supportTypeDict):
        for jointID, supportType in supportTypeDict.items():
            self.SetSupportType(jointID, supportType)

    def SetMemberType(self, memberID, memberType):
        self._bars[memberID].memberType = memberType

    def SetMemberTypes(self, memberTypeDict, isCheckAllSet=False):
        if isCheckAllSet and set(range(len(self._bars))) - set(memberTypeDict):
            raise NotAllBeSetError("Didn't set member types to all members.")
        for memberID, memberType in memberTypeDict.items():
            self._bars[memberID].memberType = memberType

    def SetMemberConnect(self, memberID, connect):
        bar = self._bars[memberID]
        bar.SetPosition(0, self._pos[connect[0]])
        bar.SetPosition(1, self._pos[connect[1]])
        self._ends[memberID] = (connect[0], connect[1])

    def SetMemberConnects(self, memberConnectDict):
        for memberID, connect in memberConnectDict.items():
            self.SetMemberConnect(memberID, connect)

    # ----------------------------------------------------------------- getters
    def GetJointPosition(self, jointID):
        return self._pos[jointID]

    def GetJointPositions(self):
        return dict(enumerate(self._pos))

    def GetSupportType(self, jointID):
        return self._sup[jointID]

    def GetSupportTypes(self):
        return dict(enumerate(self._sup))

    def GetMemberType(self, memberID):
        return self._bars[memberID].memberType

    def GetMemberTypes(self):
        return {i: bar.memberType for i, bar in enumerate(self._bars)}

    def GetMemberConnect(self, memberID):
        return self._ends[memberID]

    def GetMemberFromConnect(self, connect):
        for ends, bar in zip(self._ends, self._bars):
            if ends[0] == connect[0] and ends[1] == connect[1]:
                return bar
        return None

    def GetForce(self, jointID):
        return self._loads[jointID]

    def GetJoints(self, isProtect=True):
        return {i: (p, s) for i, (p, s) in enumerate(zip(self._pos, self._sup))}

    def GetMembers(self, isProtect=True):
        bars = [bar.Copy() for bar in self._bars] if isProtect else self._bars
        return {i: (j0, j1, bar) for i, ((j0, j1), bar) in enumerate(zip(self._ends, bars))}

    def GetForces(self, isProtect=True):
        return dict(self._loads) if isProtect else self._loads

    def GetDisplacements(self, isProtect=True):
        return copy.deepcopy(self._displace) if isProtect else self._displace

    def GetExternalForces(self, isProtect=True):
        return copy.deepcopy(self._external) if isProtect else self._external

    def GetInternalForces(self, isProtect=True):
        return copy.deepcopy(self._internal) if isProtect else self._internal

    def GetInternalStresses(self):
        if self._internal is None:
            return None
        return {m: force / self._bars[m].a for m, force in self._internal.items()}

    def GetResistances(self):
        """External force minus applied load at every supported joint (`truss.py:279-291`)."""
        if not self._solved:
            return None
        out = {}
        for jointID, sup in enumerate(self._sup):
            if sup == SupportType.NO:
                continue
            total = self._external.get(jointID, np.zeros([self._dim]))
            out[jointID] = total - self._loads[jointID] if jointID in self._loads else total
        return out

    def GetJointIDs(self):
        return list(range(len(self._pos)))

    def GetMemberIDs(self):
        return list(range(len(self._bars)))

    def GetUsedMemberTypes(self):
        return {bar.memberType for bar in self._bars}

    # ------------------------------------------- dense views used by the packer
    def GetExternalForceVector(self):
        """Dense load vector of length nJoint*dim (`truss.py:303-304`)."""
        f = np.zeros([len(self._pos), self._dim])
        for jointID, vec in self._loads.items():
            f[jointID] = vec
        return f.ravel()

    def PackedArrays(self):
        """This truss as the arrays the batched solver packs (`batch.pack_trusses`): positions [nJ, dim], member
        end joints [nM, 2] int32, sections [nM, 3] = (a, e, density), support types (list), loads [nJ, dim] -
        straight from the model's own lists, no per-joint getter calls."""
        nJ, dim = len(self._pos), self._dim
        xyz = np.array(self._pos, dtype=float).reshape(nJ, dim)
        conn = np.array(self._ends, dtype=np.int32).reshape(len(self._bars), 2)
        sections = np.array([(t.a, t.e, t.density) for t in (bar._type for bar in self._bars)],
                            dtype=float).reshape(len(self._bars), 3)
        return xyz, conn, sections, self._sup, self.GetExternalForceVector().reshape(nJ, dim)

    def GetKMatrix(self):
        """The dense global stiffness matrix, `[nJoint * dim, nJoint * dim]` (`truss.py:307-316`): every
        member's four dim x dim blocks `+- k c c^T` added at its joints' DOFs (DOF = joint * dim + axis),
        supports NOT eliminated.  Assembled on the GPU by the solve's own assembly kernel
        (`batch.global_stiffness`); no CPU fallback."""
        from .batch import global_stiffness  # late import: keeps the model importable without torch
        return global_stiffness([self])[0]

    def GetDisplacementUnknownMask(self):
        """True where the DOF is free (`truss.py:319-326`)."""
        mask = np.ones([len(self._pos) * self._dim], dtype=np.bool_)
        for jointID, sup in enumerate(self._sup):
            lo = jointID * self._dim
            mask[lo: lo + self._dim] = ~SupportType.GetResistanceMask(sup, self._dim)
        return mask

    # -------------------------------------------------------------------- solve
    def Solve(self):
        """Direct-stiffness analysis of this truss on the GPU (reference `truss.py:329-364`).

        Raises `TrussNotStableError` before any arithmetic when the counting test fails
        and `numpy.linalg.LinAlgError` when the reduced stiffness matrix is not positive
        definite (the reference's LU raises it for an exactly singular matrix).
        """
        if not self.isStable:
            raise TrussNotStableError("The truss is not stable !")
        from .batch import solve_batch  # late import: keeps the model importable without torch
        result = solve_batch([self])
        if int(result.info[0]) != 0:
            raise np.linalg.LinAlgError("Singular matrix")
        self.AdoptDenseResults(result.displace[0], result.external[0], result.internal[0])

    def SolveLoadCases(self, cases):
        """Solve this truss under several load cases with ONE factorisation of its stiffness matrix: `cases` is a list
        of `{jointID: vector}` dicts.  Returns one solved copy of the truss per case, carrying that case's forces and
        results (its `Serialize()` has the shape of the reference's output files); this truss stays as it is.
        Raises `TrussNotStableError` before any arithmetic when the counting test fails and
        `numpy.linalg.LinAlgError` when the reduced stiffness matrix is not positive definite."""
        if not self.isStable:
            raise TrussNotStableError("The truss is not stable !")
        from .batch import pack_trusses, solve_load_cases  # late import: keeps the model importable without torch
        packed = pack_trusses([self])
        copies = []
        for case in cases:
            t = Truss(self._dim).LoadFromJSON(data=self.Serialize())
            t._loads = {}
            for jointID, vector in case.items():
                t.AddExternalForce(jointID, vector)
            copies.append(t)
        loads = np.zeros([1, len(copies), packed.nJ_max, 3])
        for k, t in enumerate(copies):
            for j, v in t._loads.items():
                loads[0, k, j, :self._dim] = v
        if not copies:
            return []
        result = solve_load_cases(packed, loads)
        if int(result.info[0]) != 0:
            raise np.linalg.LinAlgError("Singular matrix")
        for k, t in enumerate(copies):
            t.AdoptDenseResults(result.displace[0, k], result.external[0, k], result.internal[0, k])
        return copies

    def SolveEffectCases(self, cases):
        """Solve this truss under several `LoadCase`s - joint forces, support settlements, member pre-strains
        (temperature, lack of fit) and self-weight, in any mix - with ONE factorisation of its stiffness matrix: all of
        them change the right-hand side only (`batch.solve_effect_cases`).  Returns one solved copy of the truss per
        case, carrying that case's forces and results: `GetDisplacements` shows the settlements at the supports,
        `GetInternalForces` is k c . (u1 - u0) - E A eps0, and `GetExternalForces` / `GetResistances` hold what the
        supports and the applied forces supply - the self-weight is in neither (it is `copy.bodyForces`,
        {jointID: vector}).  This truss stays as it is.  Raises `TrussNotStableError` before any arithmetic when the
        counting test fails, ValueError for a settlement along a free axis, and `numpy.linalg.LinAlgError` when the
        reduced stiffness matrix is not positive definite."""
        if not self.isStable:
            raise TrussNotStableError("The truss is not stable !")
        from .batch import pack_trusses, solve_effect_cases  # late import: keeps the model importable without torch
        cases = list(cases)
        if not cases:
            return []
        nJ, nM, dim = len(self._pos), len(self._bars), self._dim
        dense = pack_load_cases(cases, nJ, nM, dim)
        if dense["loads"] is None:
            dense["loads"] = np.zeros([1, len(cases), nJ, 3])
        copies = []
        for case in cases:
            t = Truss(dim).LoadFromJSON(data=self.Serialize())
            t._loads = {}
            for jointID, vector in case.forces.items():
                t.AddExternalForce(jointID, vector)
            copies.append(t)
        result = solve_effect_cases(pack_trusses([self]), **dense)
        if int(result.info[0]) != 0:
            raise np.linalg.LinAlgError("Singular matrix")
        for k, t in enumerate(copies):
            t.AdoptDenseResults(result.displace[0, k], result.external[0, k], result.internal[0, k])
            body = result.body[0, k, :nJ, :dim]
            t.bodyForces = {j: body[j].copy() for j in np.flatnonzero((np.abs(body) >= ZERO_EPS).any(axis=1)).tolist()}
        return copies

    def NaturalFrequencies(self, nModes=6, jointMasses=None, massScale=1.0, returnShapes=False):
        """The `nModes` (1 .. 8) lowest natural circular frequencies omega of this truss, ascending, with a lumped mass
        matrix: every member gives half of `a * length * density` (times `massScale`: 1 / g for weight densities) to
        each end joint, `jointMasses` ({jointID: mass}) adds non-structural mass.  A truss with fewer than `nModes` free
        DOFs of positive mass returns as many values as it has.  `returnShapes=True`: also a list of
        `{jointID: vector}` dicts, one per frequency (mass-orthonormal, largest component positive).
        One factorisation on the GPU and inverse iteration against it (`batch.solve_modes`); the truss's loads, its
        solved state and its results stay as they are.  Raises `TrussNotStableError` when the counting test fails and
        `numpy.linalg.LinAlgError` when the reduced stiffness matrix is not positive definite, as `Solve()` does."""
        if not self.isStable:
            raise TrussNotStableError("The truss is not stable !")
        from .batch import pack_trusses, solve_modes  # late import: keeps the model importable without torch
        packed = pack_trusses([self])
        masses = None
        if jointMasses:
            masses = np.zeros([1, packed.nJ_max])
            for jointID, mass in jointMasses.items():
                masses[0, jointID] = mass
        result = solve_modes(packed, p=nModes, joint_mass=masses, mass_scale=massScale)
        if int(result.info[0]) != 0:
            raise np.linalg.LinAlgError("Singular matrix")
        count = int(result.n_modes[0])
        omega = result.omega[0, :count].copy()
        if not returnShapes:
            return omega
        nJ, dim = len(self._pos), self._dim
        shapes = [dict(zip(range(nJ), result.shape[0, k, :nJ, :dim].copy())) for k in range(count)]
        return omega, shapes

    def FrequencyGradients(self, nModes=6, jointMasses=None, massScale=1.0):
        """The derivatives of the `nModes` (1 .. 8) lowest eigenvalues lambda = omega^2 of `NaturalFrequencies` (the same
        lumped mass, `jointMasses`, `massScale`) with respect to this truss's design, from one factorisation and one
        pass over the members with the converged mode shapes (`batch.solve_mode_gradients`).  Returns a dict of numpy
        arrays in the truss's own joint and member ids, n the number of values the truss has: "eigenvalue", "omega",
        "gap" [n]; "dA", "dE", "drho" [n, members] (area, modulus, density of every member); "dxyz" [n, joints, dim]
        (every joint, supports included); "djoint_mass" [n, joints] when `jointMasses` is given.
        d omega = d lambda / (2 omega).  "gap" is the relative distance to the nearest other eigenvalue: a row with a
        tiny gap belongs to a repeated eigenvalue (symmetric trusses have them) and means nothing alone - the sum of
        the rows of the whole cluster is the derivative of the sum of its eigenvalues.  The truss's loads, its solved
        state and its results stay as they are; errors as `NaturalFrequencies`."""
        if not self.isStable:
            raise TrussNotStableError("The truss is not stable !")
        from .batch import pack_trusses, solve_mode_gradients  # late import: keeps the model importable without torch
        packed = pack_trusses([self])
        masses = None
        if jointMasses:
            masses = np.zeros([1, packed.nJ_max])
            for jointID, mass in jointMasses.items():
                masses[0, jointID] = mass
        result = solve_mode_gradients(packed, p=nModes, joint_mass=masses, mass_scale=massScale)
        if int(result.info[0]) != 0:
            raise np.linalg.LinAlgError("Singular matrix")
        n, nJ, nM, dim = int(result.n_modes[0]), len(self._pos), int(packed.nM[0]), self._dim
        out = {"eigenvalue": result.eigenvalue[0, :n].copy(), "omega": result.omega[0, :n].copy(),
               "gap": result.gap[0, :n].copy(), "dA": result.dA[0, :n, :nM].copy(), "dE": result.dE[0, :n, :nM].copy(),
               "drho": result.drho[0, :n, :nM].copy(), "dxyz": result.dxyz[0, :n, :nJ, :dim].copy()}
        if masses is not None:
            out["djoint_mass"] = result.djoint_mass[0, :n, :nJ].copy()
        return out

    def ResponseSpectrum(self, directions, periods, accelerations, nModes=6, damping=0.05, rule="cqc", missingMass=True,
                         jointMasses=None, massScale=1.0):
        """The seismic response spectrum analysis of this truss with its `nModes` (1 .. 8) lowest modes (the lumped mass,
        `jointMasses` and `massScale` of `NaturalFrequencies`): `directions` [G, dim] ground directions (1 <= G <= 3;
        the length is a scale), the spectrum table `periods` [K] (ascending) and `accelerations` [G, K]
        (pseudo-accelerations, linear between the points and constant outside them), the modal `damping` ratio and the
        combination `rule` ("srss", "cqc" or "abs"); `missingMass`: the mass the truncated modes leave out responds
        statically at accelerations[:, 0] (`batch.solve_response_spectrum`).  Returns a dict of numpy arrays in the
        truss's own joint and member ids, n the number of modes the truss has: "eigenvalue", "omega" [n]; "gamma", "sa",
        "meff" [G, n] (participation factor, spectral ordinate, effective-mass fraction); "mtot", "base" [G] (the mass
        taking part and the combined base shear); the peaks per direction "displace", "reaction" [G, joints, dim] and
        "force" [G, members]; and their SRSS over the directions "displace_all", "reaction_all" [joints, dim] and
        "force_all" [members].  The truss's loads, its solved state and its results stay as they are; errors as
        `NaturalFrequencies`."""
        if not self.isStable:
            raise TrussNotStableError("The truss is not stable !")
        from .batch import pack_trusses, solve_response_spectrum  # late import: keeps the model importable without torch
        packed = pack_trusses([self])
        masses = None
        if jointMasses:
            masses = np.zeros([1, packed.nJ_max])
            for jointID, mass in jointMasses.items():
                masses[0, jointID] = mass
        result = solve_response_spectrum(packed, directions, periods, accelerations, p=nModes, damping=damping, rule=rule,
                                         missing_mass=missingMass, joint_mass=masses, mass_scale=massScale)
        if int(result.info[0]) != 0:
            raise np.linalg.LinAlgError("Singular matrix")
        n, nJ, nM, dim = int(result.n_modes[0]), len(self._pos), int(packed.nM[0]), self._dim
        return {"eigenvalue": result.eigenvalue[0, :n].copy(), "omega": result.omega[0, :n].copy(),
                "gamma": result.gamma[0, :, :n].copy(), "sa": result.sa[0, :, :n].copy(),
                "meff": result.meff[0, :, :n].copy(), "mtot": result.mtot[0].copy(), "base": result.base[0].copy(),
                "displace": result.displace[0, :, :nJ, :dim].copy(), "force": result.force[0, :, :nM].copy(),
                "reaction": result.reaction[0, :, :nJ, :dim].copy(),
                "displace_all": result.displace_all[0, :nJ, :dim].copy(), "force_all": result.force_all[0, :nM].copy(),
                "reaction_all": result.reaction_all[0, :nJ, :dim].copy()}

    def HarmonicResponse(self, omegas, loads=None, accel=None, nModes=6, damping=0.02, dampMass=0.0, dampStiff=0.0,
                         residual=True, monitorJoints=None, monitorMembers=None, jointMasses=None, massScale=1.0):
        """The steady-state response of this truss to harmonic excitation over the circular forcing frequencies
        `omegas` [S], by superposition of its `nModes` (1 .. 8) lowest modes (the lumped mass, `jointMasses` and
        `massScale` of `NaturalFrequencies`).  `loads`: a list of `{jointID: vector}` dicts, the load amplitudes of one
        case each (None: the truss's own joint forces as one case, unless only `accel` is given); `accel` [L, dim]:
        ground-acceleration amplitudes per case (the results are then relative to the ground); up to 16 cases.  Damping
        of mode k: `damping` + `dampMass` / (2 omega_k) + `dampStiff` omega_k / 2, at least one of them positive.
        `residual`: the modes beyond `nModes` respond statically (`batch.solve_harmonic`) - good well below the first
        frequency left out, not near or above it.  Returns a dict of numpy arrays in the truss's own joint and member
        ids, n the number of modes the truss has: "eigenvalue", "omega" [n]; the largest amplitudes over the sweep
        "displace", "reaction" [L, joints, dim] and "force" [L, members], the index into `omegas` where each occurs
        ("displace_at", ...) and that frequency ("displace_omega", ...); with `monitorJoints` / `monitorMembers` (lists of
        ids) the complex responses "frf_displace" [L, S, len(monitorJoints), dim] and "frf_force"
        [L, S, len(monitorMembers)].  The truss's loads, its solved state and its results stay as they are; errors as
        `NaturalFrequencies`."""
        if not self.isStable:
            raise TrussNotStableError("The truss is not stable !")
        from .batch import pack_trusses, solve_harmonic  # late import: keeps the model importable without torch
        packed = pack_trusses([self])
        nJ, dim = len(self._pos), self._dim
        masses = None
        if jointMasses:
            masses = np.zeros([1, packed.nJ_max])
            for jointID, mass in jointMasses.items():
                masses[0, jointID] = mass
        if loads is None and accel is None:
            loads = [self._loads]
        pattern = None
        if loads is not None:
            pattern = np.zeros([1, len(loads), packed.nJ_max, 3])
            for k, case in enumerate(loads):
                for jointID, vector in case.items():
                    pattern[0, k, jointID, :dim] = np.asarray(vector, dtype=float)[:dim]
        monitors = {}
        for name, ids in (("monitor_joints", monitorJoints), ("monitor_members", monitorMembers)):
            monitors[name] = None if ids is None or not len(ids) else np.asarray(ids, dtype=np.int32).reshape(1, -1)
        result = solve_harmonic(packed, omegas, pattern=pattern, accel=accel, p=nModes, damping=damping,
                                damp_mass=dampMass, damp_stiff=dampStiff, residual=residual, joint_mass=masses,
                                mass_scale=massScale, **monitors)
        if int(result.info[0]) != 0:
            raise np.linalg.LinAlgError("Singular matrix")
        n, nM = int(result.n_modes[0]), int(packed.nM[0])
        out = {"eigenvalue": result.eigenvalue[0, :n].copy(), "omega": result.omega[0, :n].copy()}
        for tail in ("", "_at", "_omega"):
            out["displace" + tail] = getattr(result, "displace" + tail)[0, :, :nJ, :dim].copy()
            out["reaction" + tail] = getattr(result, "reaction" + tail)[0, :, :nJ, :dim].copy()
            out["force" + tail] = getattr(result, "force" + tail)[0, :, :nM].copy()
        if monitors["monitor_joints"] is not None:
            out["frf_displace"] = result.frf_displace[0, ..., :dim].copy()
        if monitors["monitor_members"] is not None:
            out["frf_force"] = result.frf_force[0].copy()
        return out

    def BucklingFactors(self, nModes=4, returnShapes=False, maxShifts=6):
        """By what factor can this truss's loads grow before it buckles (linear buckling, `batch.solve_buckling`)?
        Returns `(critical, factors)`: `critical` the smallest positive load factor (NaN when none was found within
        `maxShifts` shift rounds, or when the truss has none - under pure tension, or without loads) and `factors` the
        up to `nModes` (1 .. 8) signed factors nearest the last shift, nearest first (a negative factor means buckling
        under the reversed loads).  `returnShapes=True`: also a list of `{jointID: vector}` dicts, one per factor
        (largest component +1).  Buckling of single members between their joints (Euler) is not part of it.  The
        truss's loads, its solved state and its results stay as they are.  Raises `TrussNotStableError` when the
        counting test fails and `numpy.linalg.LinAlgError` when the reduced stiffness matrix is not positive definite,
        as `Solve()` does."""
        if not self.isStable:
            raise TrussNotStableError("The truss is not stable !")
        from .batch import pack_trusses, solve_buckling  # late import: keeps the model importable without torch
        result = solve_buckling(pack_trusses([self]), p=nModes, max_shifts=maxShifts)
        if int(result.info[0]) != 0:
            raise np.linalg.LinAlgError("Singular matrix")
        count = int(result.n_modes[0])
        critical, factors = float(result.critical[0]), result.factor[0, :count].copy()
        if not returnShapes:
            return critical, factors
        nJ, dim = len(self._pos), self._dim
        shapes = [dict(zip(range(nJ), result.shape[0, k, :nJ, :dim].copy())) for k in range(count)]
        return critical, factors, shapes

    def TransientResponse(self, dt, steps, cases=None, scale=None, groundAcceleration=None, beta=0.25, gamma=0.5,
                          dampMass=0.0, dampStiff=0.0, jointMasses=None, massScale=1.0, monitorJoints=(),
                          monitorMembers=()):
        """What this truss does under a load history or a ground motion: `steps` Newmark steps of size `dt` (`beta`,
        `gamma`; the defaults are the average-acceleration rule) of M u'' + C u' + K u = scale(t) P - M iota(ag(t)) from
        rest, with the lumped mass of `NaturalFrequencies` (`jointMasses`, `massScale`) and Rayleigh damping
        C = dampMass M + dampStiff K, from ONE factorisation (`batch.solve_transient`).  `cases`: a list of
        `{jointID: vector}` load patterns P as `SolveLoadCases` takes them (None: the truss's own forces as one case);
        `scale`: [L, steps + 1] or [steps + 1] (the same for every case), None = 1; `groundAcceleration`:
        [L, steps + 1, dim] or [steps + 1, dim], None = none (the displacements are then relative to the ground).
        Returns a dict of numpy arrays, L the number of cases, T = steps:
          "displace", "velocity", "acceleration"   [L, nJ, dim]   the state at the last time point,
          "peakDisplace", "peakDisplaceStep"       [L, nJ, dim]   max |u| over the points 0 .. T and the first point there,
          "forceMax", "forceMaxStep", "forceMin", "forceMinStep"  [L, nM]   the signed extremes of the member forces,
          "historyDisplace" [L, T + 1, len(monitorJoints), dim], "historyForce" [L, T + 1, len(monitorMembers)].
        The truss's loads, its solved state and its results stay as they are.  Raises ValueError for bad arguments (as
        `batch.solve_transient`), `TrussNotStableError` when the counting test fails and `numpy.linalg.LinAlgError`
        when K + sigma M is not positive definite."""
        if not self.isStable:
            raise TrussNotStableError("The truss is not stable !")
        from .batch import pack_trusses, solve_transient  # late import: keeps the model importable without torch
        packed = pack_trusses([self])
        nJ, nM, dim = len(self._pos), len(self._bars), self._dim
        pattern = np.asarray(packed.loads, dtype=np.float64)[:, None] if cases is None \
            else self._case_loads(list(cases), packed.nJ_max)
        L = pattern.shape[1]
        spread = lambda x, nd: None if x is None else \
            np.array(np.broadcast_to(np.asarray(x, dtype=np.float64), (L,) + np.shape(x)[-nd:]))[None]
        masses = None
        if jointMasses:
            masses = np.zeros([1, packed.nJ_max])
            for jointID, mass in jointMasses.items():
                masses[0, jointID] = mass
        result = solve_transient(packed, pattern, dt, steps, scale=spread(scale, 1), accel=spread(groundAcceleration, 2),
                                 beta=beta, gamma=gamma, damp_mass=dampMass, damp_stiff=dampStiff, joint_mass=masses,
                                 mass_scale=massScale,
                                 monitor_joints=np.asarray(list(monitorJoints), dtype=np.int64).reshape(1, -1),
                                 monitor_members=np.asarray(list(monitorMembers), dtype=np.int64).reshape(1, -1))
        if int(result.info[0]) != 0:
            raise np.linalg.LinAlgError("Singular matrix")
        return {"displace": result.displace[0, :, :nJ, :dim].copy(), "velocity": result.velocity[0, :, :nJ, :dim].copy(),
                "acceleration": result.acceleration[0, :, :nJ, :dim].copy(),
                "peakDisplace": result.peak_displace[0, :, :nJ, :dim].copy(),
                "peakDisplaceStep": result.peak_displace_step[0, :, :nJ, :dim].copy(),
                "forceMax": result.force_max[0, :, :nM].copy(), "forceMaxStep": result.force_max_step[0, :, :nM].copy(),
                "forceMin": result.force_min[0, :, :nM].copy(), "forceMinStep": result.force_min_step[0, :, :nM].copy(),
                "historyDisplace": result.history_displace[0, ..., :dim].copy(),
                "historyForce": result.history_force[0].copy()}

    def SolveNonlinear(self, load_factors=(1.0,), tol=1e-9, maxIters=25):
        """Geometrically nonlinear statics of this truss (large displacements, small strains) under `load_factors`
        times its own forces, one load step per factor in the given order, each started from the previous step's
        displacements: Newton's method on the tangent stiffness (`batch.solve_nonlinear`).  Returns a dict of numpy
        arrays, S the number of load steps:
          "displace" [S, nJ, dim], "internal" [S, nM] (member forces, tension positive), "external" [S, nJ, dim] (the
          applied force at free DOFs, the reaction at held ones), "iterations", "status" [S] (0 converged, 1 iteration
          limit, 2 tangent not positive definite - the truss has passed a limit point; "displace" is then the last
          accepted iterate -, 3 not attempted because an earlier step failed) and "residual" [S].
        The truss's loads, its solved state and its linear results stay as they are.  Raises ValueError for bad
        arguments (as `batch.solve_nonlinear`) and `TrussNotStableError` when the counting test fails."""
        if not self.isStable:
            raise TrussNotStableError("The truss is not stable !")
        from .batch import pack_trusses, solve_nonlinear  # late import: keeps the model importable without torch
        nJ, nM, dim = len(self._pos), len(self._bars), self._dim
        result = solve_nonlinear(pack_trusses([self]), load_factors, tol=tol, max_iters=maxIters)
        return {"displace": result.displace[0, :, :nJ, :dim].copy(), "internal": result.internal[0, :, :nM].copy(),
                "external": result.external[0, :, :nJ, :dim].copy(), "iterations": result.iterations[0].copy(),
                "status": result.status[0].copy(), "residual": result.residual[0].copy()}

    def SizeMembers(self, cases=None, allowTension=None, allowCompression=None, allowDisplacement=None, eulerKappa=0.0,
                    areaMin=None, areaMax=None, relax=1.0, tol=1e-4, maxIters=40, catalog=None):
        """Size this truss's members by the stress-ratio method - fully stressed design with a displacement envelope
        (`batch.solve_sizing`): starting from the members' own areas, the design is analysed under all load cases and
        every member resized to what its worst case demands, until the areas stop moving.  `cases` is a list of
        `{jointID: vector}` dicts as `SolveLoadCases` takes them (None: the truss's own forces as one case);
        `allowTension`, `allowCompression`: allowable stresses (> 0); `allowDisplacement`: the largest joint
        displacement allowed (None: no limit); `eulerKappa`: the member's second moment of area as I = kappa A^2
        (1 / (4 pi) for a solid round bar; 0: no member buckling check); `areaMin` > 0, `areaMax` >= `areaMin`: scalars or
        one value per member; `relax` in (0, 1], `tol`, `maxIters` as `batch.solve_sizing`; `catalog`: a list of
        `MemberType` whose areas (sorted, duplicates dropped) the final design is rounded up to.  Returns a dict of numpy
        arrays and scalars:
          "areas", "utilisation" [nM] (required area / area; <= 1 is feasible), "governing" [nM] (the governing case,
          -1: the displacement limit), "weight", "disp_ratio", "iterations", "status" (0 converged, 1 iteration limit,
          2 a design could not be factored), "weight_history" [maxIters + 1] and - with `catalog` - "catalog_index" [nM]
          (into the sorted areas).
        The truss's own members, loads and solved state stay as they are.  Raises ValueError for bad arguments (as
        `batch.solve_sizing`) and `TrussNotStableError` when the counting test fails."""
        if not self.isStable:
            raise TrussNotStableError("The truss is not stable !")
        from .batch import pack_trusses, solve_sizing  # late import: keeps the model importable without torch
        packed = pack_trusses([self])
        nM = len(self._bars)
        loads = None
        if cases is not None:
            cases = list(cases)
            if not cases:
                raise ValueError("SizeMembers: cases must hold at least one load case")
            loads = self._case_loads(cases, packed.nJ_max)

        def bound(x):
            if x is None or np.ndim(x) == 0:
                return x
            row = np.zeros([1, packed.nM_max])
            row[0, :nM] = np.asarray(x, dtype=np.float64).reshape(nM)
            return row
        areas = None if catalog is None else sorted({float(t.a) for t in catalog})
        result = solve_sizing(packed, loads, allow_tension=allowTension, allow_compression=allowCompression,
                              allow_displace=0.0 if allowDisplacement is None else allowDisplacement,
                              euler_kappa=eulerKappa, area_min=bound(areaMin), area_max=bound(areaMax), relax=relax, tol=tol,
                              max_iters=maxIters, catalog=areas)
        out = {"areas": result.areas[0, :nM].copy(), "utilisation": result.utilisation[0, :nM].copy(),
               "governing": result.governing[0, :nM].copy(), "weight": float(result.weight[0]),
               "disp_ratio": float(result.disp_ratio[0]), "iterations": int(result.iterations[0]),
               "status": int(result.status[0]), "weight_history": result.weight_history[0].copy()}
        if catalog is not None:
            out["catalog_index"] = result.catalog_index[0, :nM].copy()
        return out

    def MinimizeCompliance(self, cases=None, alpha=None, target=None, measure="weight", eta=0.5, move=0.2, areaMin=None,
                           areaMax=None, tol=1e-4, maxIters=60):
        """The areas that make this truss stiffest at a given weight (or volume): compliance sizing by the
        optimality-criteria method (`batch.solve_min_compliance`), starting from the members' own areas.  `cases` is a
        list of `{jointID: vector}` dicts as `SolveLoadCases` takes them (None: the truss's own forces as one case);
        `alpha`: one weight >= 0 per case (None: ones); `target`: the weight (`measure` "weight": sum rho L A) or volume
        ("volume": sum L A) of the design (None: that of the members' own areas); `areaMin` > 0, `areaMax` >= `areaMin`:
        scalars or one value per member; `eta`, `move`, `tol`, `maxIters` as `batch.solve_min_compliance`.  Returns a
        dict of numpy arrays and scalars:
          "areas", "sensitivity" [nM] (-dJ/dA), "measure", "objective", "multiplier", "compliance" [L], "iterations",
          "status" (0 converged, 1 iteration limit, 2 a design could not be factored), "objective_history"
          [maxIters + 1].
        The truss's own members, loads and solved state stay as they are.  Raises ValueError for bad arguments (as
        `batch.solve_min_compliance`) and `TrussNotStableError` when the counting test fails."""
        if not self.isStable:
            raise TrussNotStableError("The truss is not stable !")
        from .batch import pack_trusses, solve_min_compliance  # late import: keeps the model importable without torch
        packed = pack_trusses([self])
        nM = len(self._bars)
        loads = None
        if cases is not None:
            cases = list(cases)
            if not cases:
                raise ValueError("MinimizeCompliance: cases must hold at least one load case")
            loads = self._case_loads(cases, packed.nJ_max)

        def bound(x):
            if x is None or np.ndim(x) == 0:
                return x
            row = np.zeros([1, packed.nM_max])
            row[0, :nM] = np.asarray(x, dtype=np.float64).reshape(nM)
            return row
        result = solve_min_compliance(packed, loads, alpha=alpha, target=target, measure=measure, eta=eta, move=move,
                                      area_min=bound(areaMin), area_max=bound(areaMax), tol=tol, max_iters=maxIters)
        return {"areas": result.areas[0, :nM].copy(), "sensitivity": result.sensitivity[0, :nM].copy(),
                "measure": float(result.measure[0]), "objective": float(result.objective[0]),
                "multiplier": float(result.multiplier[0]), "compliance": result.compliance[0].copy(),
                "iterations": int(result.iterations[0]), "status": int(result.status[0]),
                "objective_history": result.objective_history[0].copy()}

    def MinimizeWeight(self, loadCases=None, limits=None, measure="weight", move=0.2, areaMin=None, areaMax=None, tol=1e-4,
                       maxIters=60, sweeps=2, limitTol=1e-2, returnSensitivity=False, allowTension=None,
                       allowCompression=None, eulerKappa=0.0):
        """The lightest areas of this truss whose named joint displacements stay within named limits: minimum-weight
        sizing by the optimality-criteria method with one multiplier per limit (`batch.solve_min_weight`), starting from
        the members' own areas.  `loadCases` is a list of `{jointID: vector}` dicts as `SolveLoadCases` takes them (None:
        the truss's own forces as one case); `limits` is a list of up to 8 `(case, jointID, direction, value)`: under
        load case `case` the displacement of joint `jointID` along `direction` (any length but zero) must not exceed
        `value` > 0 - a two-sided limit is two limits with opposite directions; `measure`: what is minimised, the weight
        (sum rho L A) or the "volume" (sum L A); `areaMin` > 0, `areaMax` >= `areaMin`: scalars or one value per member;
        `move`, `tol`, `maxIters`, `sweeps`, `limitTol` as `batch.solve_min_weight`.  Returns a dict of numpy arrays and
        scalars:
          "areas" [nM], "measure", "displacement", "ratio" (displacement / value; <= 1 is feasible), "multipliers" [J],
          "iterations", "status" (0 converged within its limits, 1 iteration limit, 2 a design could not be factored, 3
          converged on its bounds without meeting a limit), "measure_history", "worst_history" [maxIters + 1] and - with
          `returnSensitivity` - "sensitivity" [J, nM] (minus the derivative of every limited displacement by every area).
        `allowTension`, `allowCompression` (both or neither, > 0; +inf switches a side off) and `eulerKappa` >= 0 (I =
        kappa A^2; 0: no member buckling term) add stress limits to the same run, as `SizeMembers` takes them: the dict
        then also holds "utilisation" [nM] (required area / area; <= 1 is feasible), "governing" [nM] (the load case
        that sets a member's requirement, -1: none) and "stress_history" [maxIters + 1], and status 0 asks the
        utilisation too for <= 1 + `limitTol`.
        The truss's own members, loads and solved state stay as they are.  Raises ValueError for bad arguments (as
        `batch.solve_min_weight`) and `TrussNotStableError` when the counting test fails."""
        if not self.isStable:
            raise TrussNotStableError("The truss is not stable !")
        from .batch import pack_trusses, solve_min_weight  # late import: keeps the model importable without torch
        packed = pack_trusses([self])
        nM = len(self._bars)
        loads = None
        if loadCases is not None:
            loadCases = list(loadCases)
            if not loadCases:
                raise ValueError("MinimizeWeight: loadCases must hold at least one load case")
            loads = self._case_loads(loadCases, packed.nJ_max)
        try:
            limits = [tuple(one) for one in limits]
            rows = [(case, jointID, [float(x) for x in direction], value) for case, jointID, direction, value in limits]
        except (TypeError, ValueError):
            raise ValueError("MinimizeWeight: limits must be a list of (case, jointID, direction, value)") from None
        if not rows or any(len(d) != self._dim for _, _, d, _ in rows):
            raise ValueError(f"MinimizeWeight: limits must hold at least one limit, every direction with {self._dim} "
                             "components")

        def bound(x):
            if x is None or np.ndim(x) == 0:
                return x
            row = np.zeros([1, packed.nM_max])
            row[0, :nM] = np.asarray(x, dtype=np.float64).reshape(nM)
            return row
        result = solve_min_weight(packed, loads, limit_case=[r[0] for r in rows], limit_joint=[r[1] for r in rows],
                                  limit_direction=[r[2] for r in rows], limit_value=[r[3] for r in rows], measure=measure,
                                  move=move, area_min=bound(areaMin), area_max=bound(areaMax), tol=tol, max_iters=maxIters,
                                  sweeps=sweeps, limit_tol=limitTol, want_sensitivity=returnSensitivity,
                                  allow_tension=allowTension, allow_compression=allowCompression, euler_kappa=eulerKappa)
        out = {"areas": result.areas[0, :nM].copy(), "measure": float(result.measure[0]),
               "displacement": result.displacement[0].copy(), "ratio": result.ratio[0].copy(),
               "multipliers": result.multipliers[0].copy(), "iterations": int(result.iterations[0]),
               "status": int(result.status[0]), "measure_history": result.measure_history[0].copy(),
               "worst_history": result.worst_history[0].copy()}
        if returnSensitivity:
            out["sensitivity"] = result.sensitivity[0, :, :nM].copy()
        if result.utilisation is not None:
            out.update(utilisation=result.utilisation[0, :nM].copy(), governing=result.governing[0, :nM].copy(),
                       stress_history=result.stress_history[0].copy())
        return out

    def SolveUnilateral(self, kinds, cases=None, slackFactor=0.0, maxIters=20):
        """Solve this truss with members that carry tension only or compression only - cables, tie rods, counter-bracing,
        struts that bear against a seat - by the active-set iteration (`batch.solve_unilateral`): every case is analysed,
        the unilateral members that are strained the wrong way are switched off, those that would be strained the right
        way are switched on, until nothing changes.  `kinds`: {memberID: "tension" | "compression"} (the others are
        ordinary members), or one value per member of 0, 1 (tension-only), -1 (compression-only); `cases`: a list of
        `{jointID: vector}` dicts as `SolveLoadCases` takes them, or of `LoadCase`s with forces and prestrains
        (pretension is a negative pre-strain; settlements and gravity are not taken) - None: the truss's own forces as
        one case; `slackFactor` >= 0: the fraction of its area a slack member keeps (0 removes it); `maxIters`: rounds of
        flips at most.  Returns a list, one dict per case:
          "displacements" [nJ, dim], "forces" [nM] (member forces, tension positive), "reactions" [nJ, dim] (what the
          supports supply; zero rows at free joints), "slack" (the IDs of the slack members), "status" (0 converged, 1
          iteration limit, 2 a structure could not be factored), "iterations", "violations".
        The linear small-displacement answer: no cable sag, no geometric stiffness.  The truss itself, its JSON format
        and `MemberType` stay as they are.  Raises ValueError for bad arguments (as `batch.solve_unilateral`) and
        `TrussNotStableError` when the counting test fails."""
        if not self.isStable:
            raise TrussNotStableError("The truss is not stable !")
        from .batch import pack_trusses, solve_unilateral  # late import: keeps the model importable without torch
        packed = pack_trusses([self])
        nJ, nM, dim = len(self._pos), len(self._bars), self._dim
        kind = np.zeros([1, packed.nM_max])
        if isinstance(kinds, dict):
            words = {"tension": 1, "compression": -1}
            for memberID, word in kinds.items():
                if not (isinstance(memberID, (int, np.integer)) and 0 <= memberID < nM):
                    raise ValueError(f"SolveUnilateral: no such member [{memberID}] in kinds")
                if word not in words:
                    raise ValueError(f"SolveUnilateral: kinds[{memberID}] must be 'tension' or 'compression', got {word!r}")
                kind[0, memberID] = words[word]
        else:
            row = np.asarray(kinds, dtype=np.float64)
            if row.shape != (nM,):
                raise ValueError(f"SolveUnilateral: kinds must be a dict or hold one value per member ({nM}), got "
                                 f"{row.shape}")
            kind[0, :nM] = row
        loads, prestrain = None, None
        if cases is not None:
            cases = list(cases)
            if not cases:
                return []
            if any(isinstance(c, LoadCase) for c in cases):
                cases = [c if isinstance(c, LoadCase) else LoadCase(forces=c) for c in cases]
                if any(c.settlements or c.gravity is not None for c in cases):
                    raise ValueError("SolveUnilateral: a case may carry forces and prestrains only - pass self-weight as "
                                     "joint forces")
                dense = pack_load_cases(cases, nJ, nM, dim)
                loads = self._case_loads([c.forces for c in cases], packed.nJ_max)
                if dense["prestrain"] is not None:
                    prestrain = np.zeros([1, len(cases), packed.nM_max])
                    prestrain[0, :, :nM] = dense["prestrain"][0]
            else:
                loads = self._case_loads(cases, packed.nJ_max)
        result = solve_unilateral(packed, kind, loads, prestrain, slack_factor=slackFactor, max_iters=maxIters)
        held = packed.constrained()[0, :nJ, :dim]
        out = []
        for k in range(result.status.shape[1]):
            slack = np.flatnonzero((kind[0, :nM] != 0) & (result.state[0, k, :nM] == 0))
            out.append({"displacements": result.displace[0, k, :nJ, :dim].copy(),
                        "forces": result.internal[0, k, :nM].copy(),
                        "reactions": np.where(held, result.external[0, k, :nJ, :dim], 0.0),
                        "slack": [int(m) for m in slack], "status": int(result.status[0, k]),
                        "iterations": int(result.iterations[0, k]), "violations": int(result.violations[0, k])})
        return out

    def CollapseLoad(self, capacities, cases=None, hardening=0.0, lambdaMax=1.0, dispLimit=0.0, maxEvents=64,
                     collapseRatio=1e8, tieTol=1e-9):
        """How much of a load pattern this truss carries before it collapses, and in which order its members give way:
        the event-to-event elastic-plastic analysis (`batch.solve_plastic`).  A member that reaches its capacity goes on
        carrying it while the rest of a redundant truss picks up the difference, until the truss is a mechanism.
        `capacities`: the member capacities as forces - one positive number, one per member, or
        {"tension": .., "compression": ..} of either; `cases`: a list of `{jointID: vector}` dicts as `SolveLoadCases`
        takes them, each a load pattern that the load factor scales - None: the truss's own forces as one case;
        `hardening` >= 0: the fraction of its stiffness a yielded member keeps; `lambdaMax` > 0 and `dispLimit` >= 0 (0:
        none) end a run; `maxEvents`: events at most.  Returns a list, one dict per case:
          "loadFactor", "status" (0 lambdaMax reached, 1 event limit, 2 mechanism: loadFactor is the collapse load, 3
          displacement limit), "events", "yielded" ({memberID: +1 tension | -1 compression}), "sequence" (the events in
          order as (loadFactor, memberID) pairs; memberID -1: members unloaded and returned to elastic), "forces" [nM],
          "displacements" [nJ, dim], "reactions" [nJ, dim] (zero rows at free joints), "curve" (the pushover curve as
          (loadFactor, largest |u|) pairs, one per analysis).
        Small displacements, one proportional load pattern, a compression capacity is a plateau.  The truss itself stays
        unsolved and unchanged.  Raises ValueError for bad arguments (as `batch.solve_plastic`) and
        `TrussNotStableError` when the counting test fails."""
        if not self.isStable:
            raise TrussNotStableError("The truss is not stable !")
        from .batch import pack_trusses, solve_plastic  # late import: keeps the model importable without torch
        packed = pack_trusses([self])
        nJ, nM, dim = len(self._pos), len(self._bars), self._dim
        if isinstance(capacities, dict):
            if set(capacities) != {"tension", "compression"}:
                raise ValueError("CollapseLoad: capacities must be a number, one per member, or a dict with the keys "
                                 "'tension' and 'compression'")
            pair = (capacities["tension"], capacities["compression"])
        else:
            pair = (capacities, capacities)
        caps = []
        for x in pair:
            try:
                row = np.asarray(x, dtype=np.float64)
            except (TypeError, ValueError):
                row = None
            if isinstance(x, bool) or row is None or row.shape not in ((), (nM,)):
                raise ValueError(f"CollapseLoad: a capacity must be one number or one per member ({nM}), got {x!r}")
            full = np.ones([1, packed.nM_max])
            full[0, :nM] = row
            caps.append(full)
        loads = None
        if cases is not None:
            cases = list(cases)
            if not cases:
                return []
            loads = self._case_loads(cases, packed.nJ_max)
        result = solve_plastic(packed, caps[0], caps[1], loads, hardening=hardening, lambda_max=lambdaMax,
                               disp_limit=dispLimit, collapse_ratio=collapseRatio, tie_tol=tieTol, max_events=maxEvents)
        held = packed.constrained()[0, :nJ, :dim]
        out = []
        for k in range(result.status.shape[1]):
            events = int(result.events[0, k])
            lam, member = result.lambda_history[0, k], result.member_history[0, k]
            state = result.state[0, k, :nM]
            out.append({"loadFactor": float(result.load_factor[0, k]), "status": int(result.status[0, k]), "events": events,
                        "yielded": {int(m): int(state[m]) for m in np.flatnonzero(state)},
                        "sequence": [(float(lam[i]), int(member[i])) for i in range(events)],
                        "forces": result.internal[0, k, :nM].copy(),
                        "displacements": result.displace[0, k, :nJ, :dim].copy(),
                        "reactions": np.where(held, result.external[0, k, :nJ, :dim], 0.0),
                        "curve": [(float(lam[i]), float(result.umax_history[0, k, i])) for i in range(events + 1)]})
        return out

    def MemberLoss(self, cases=None, rTol=None, returnForces=False):
        """What the loss of any ONE member does to this truss, for every member and every load case, from ONE
        factorisation (`batch.solve_member_loss`): `cases` is a list of `{jointID: vector}` dicts as `SolveLoadCases`
        takes them (None: the truss's own forces as one case).  Returns a list, one entry per case, of
        `{memberID: record}`; a record holds
          "redundancy"   r_e in [0, 1] (the same in every case; over the truss they sum to its degree of indeterminacy),
          "critical"     True when r_e <= `rTol` (default `batch.MEMBER_LOSS_R_TOL`): without the member the truss is a
                         mechanism - the peaks are then inf and their ids None,
          "peakStress", "peakStressMember"           the largest |N| / a among the surviving members, and where,
          "peakDisplacement", "peakDisplacementJoint"  the largest joint displacement, and where,
          "forces"       (`returnForces`) {memberID: N} after the removal, entries below 1e-10 dropped like the other
                         results (None for a critical member).
        The truss's loads, its solved state and its results stay as they are.  Raises `TrussNotStableError` when the
        counting test fails and `numpy.linalg.LinAlgError` when the reduced stiffness matrix is not positive definite,
        as `Solve()` does."""
        if not self.isStable:
            raise TrussNotStableError("The truss is not stable !")
        from .batch import MEMBER_LOSS_R_TOL, pack_trusses, solve_member_loss  # late import, as the other solvers
        packed = pack_trusses([self])
        nM = len(self._bars)
        loads = None
        if cases is not None:
            cases = list(cases)
            if not cases:
                return []
            loads = self._case_loads(cases, packed.nJ_max)
        result = solve_member_loss(packed, loads, r_tol=MEMBER_LOSS_R_TOL if rTol is None else rTol,
                                   want_forces=returnForces)
        if int(result.info[0]) != 0:
            raise np.linalg.LinAlgError("Singular matrix")
        out = []
        for k in range(result.peak_stress.shape[1]):
            records = {}
            for e in range(nM):
                critical = bool(result.critical[0, e])
                rec = {"redundancy": float(result.redundancy[0, e]), "critical": critical,
                       "peakStress": float(result.peak_stress[0, k, e]),
                       "peakStressMember": None if result.peak_member[0, k, e] < 0 else int(result.peak_member[0, k, e]),
                       "peakDisplacement": float(result.peak_displace[0, k, e]),
                       "peakDisplacementJoint": None if result.peak_joint[0, k, e] < 0 else int(result.peak_joint[0, k, e])}
                if returnForces:
                    n = result.internal_after[0, k, e, :nM]
                    rec["forces"] = None if critical else \
                        {int(m): float(n[m]) for m in np.flatnonzero(np.abs(n) >= ZERO_EPS)}
                records[e] = rec
            out.append(records)
        return out

    def _case_loads(self, cases, nJ_max):
        """[1, L, nJ_max, 3]: `{jointID: vector}` load cases as the dense array the batched analyses take, every vector
        checked as `AddExternalForce` checks it."""
        loads = np.zeros([1, len(cases), nJ_max, 3])
        for k, case in enumerate(cases):
            probe = Truss(self._dim).LoadFromJSON(data=dict(self.Serialize(), force=[]))
            for jointID, vector in case.items():
                probe.AddExternalForce(jointID, vector)
            for j, v in probe._loads.items():
                loads[0, k, j, :self._dim] = v
        return loads

    def MemberSets(self, sets, factors=None, cases=None, rTol=None, returnForces=False):
        """What removing, damaging or strengthening SEVERAL members at once does to this truss, for every scenario and
        every load case, from ONE factorisation (`batch.solve_member_sets`): `sets` is a list of scenarios, each a list
        of up to 8 distinct member IDs; `factors` a list of the same shape with the area factor of every named member
        (0 removed, below 1 damaged, above 1 strengthened; None: every member removed); `cases` a list of
        `{jointID: vector}` dicts as `SolveLoadCases` takes them (None: the truss's own forces as one case).  Returns a
        list, one entry per case, of lists with one record per scenario; a record holds
          "members", "factors"   the scenario as given,
          "pivots"        one per member, in the set's order: for removals the redundancy of the member once the members
                          before it are gone (None after a failing position),
          "unstable"      True when a pivot is <= `rTol` (default `batch.MEMBER_LOSS_R_TOL`): the truss is a mechanism -
                          the peaks are then inf and their ids None,
          "firstUnstable" the member ID at which the set makes the truss a mechanism (None: it stays stable),
          "peakStress", "peakStressMember"           the largest |N| / a among the members that are not removed, and where,
          "peakDisplacement", "peakDisplacementJoint"  the largest joint displacement, and where,
          "forces"        (`returnForces`) {memberID: N} in the scenario, entries below 1e-10 dropped like the other
                          results (None for an unstable scenario).
        The truss's loads, its solved state and its results stay as they are.  Raises ValueError for a bad scenario (as
        `batch.solve_member_sets`), `TrussNotStableError` when the counting test fails and `numpy.linalg.LinAlgError`
        when the reduced stiffness matrix is not positive definite, as `Solve()` does."""
        if not self.isStable:
            raise TrussNotStableError("The truss is not stable !")
        from .batch import MEMBER_LOSS_R_TOL, pack_trusses, solve_member_sets  # late import, as the other solvers
        packed = pack_trusses([self])
        nM = len(self._bars)
        sets = [list(x) for x in sets]
        if factors is not None:
            factors = [[list(g) for g in factors]]
        loads = None
        if cases is not None:
            cases = list(cases)
            if not cases:
                return []
            loads = self._case_loads(cases, packed.nJ_max)
        result = solve_member_sets(packed, [sets], factors, loads, r_tol=MEMBER_LOSS_R_TOL if rTol is None else rTol,
                                   want_forces=returnForces)
        if int(result.info[0]) != 0:
            raise np.linalg.LinAlgError("Singular matrix")
        out = []
        for k in range(result.peak_stress.shape[1]):
            records = []
            for s, members in enumerate(sets):
                unstable, first = bool(result.unstable[0, s]), int(result.first_unstable[0, s])
                pivots = [float(p) for p in result.pivot[0, s, :len(members)]]
                rec = {"members": [int(m) for m in members],
                       "factors": [0.0] * len(members) if factors is None else [float(g) for g in factors[0][s]],
                       "pivots": [None if p != p else p for p in pivots], "unstable": unstable,
                       "firstUnstable": int(members[first]) if unstable else None,
                       "peakStress": float(result.peak_stress[0, k, s]),
                       "peakStressMember": None if result.peak_member[0, k, s] < 0 else int(result.peak_member[0, k, s]),
                       "peakDisplacement": float(result.peak_displace[0, k, s]),
                       "peakDisplacementJoint": None if result.peak_joint[0, k, s] < 0 else int(result.peak_joint[0, k, s])}
                if returnForces:
                    n = result.internal_after[0, k, s, :nM]
                    rec["forces"] = None if unstable else \
                        {int(m): float(n[m]) for m in np.flatnonzero(np.abs(n) >= ZERO_EPS)}
                records.append(rec)
            out.append(records)
        return out

    def InfluenceLines(self, path, direction, train=None, returnLines=False):
        """Moving loads: the influence lines of every member force along `path` (a list of joint IDs, consecutive ones at
        distinct positions) for a load `direction` (a vector per unit axle weight), and the envelope of a load `train`
        - a list of (weight, offset) pairs, the offsets behind the lead axle ascending from 0; None: one unit axle -
        that crosses the path, from ONE factorisation (`batch.solve_influence`).  Returns `{memberID: record}`; a record
        holds
          "max", "maxAt"   the largest member force any position of the train gives, and the arc position of the lead
                           axle (measured along the path from its first joint) that gives it,
          "min", "minAt"   the smallest, and where (the positions are None for an empty path),
          "areaPositive", "areaNegative"   the integrals of the positive and of the negative part of the influence line
                           along the path (times a line load: the extremes under a uniform live load),
          "ordinates"      (`returnLines`) the influence ordinates at the path joints, a list over `path`.
        The truss's loads, its solved state and its results stay as they are.  Raises `TrussNotStableError` when the
        counting test fails and `numpy.linalg.LinAlgError` when the reduced stiffness matrix is not positive definite,
        as `Solve()` does."""
        if not self.isStable:
            raise TrussNotStableError("The truss is not stable !")
        from .batch import pack_trusses, solve_influence  # late import, as the other solvers
        path = [int(j) for j in path]
        result = solve_influence(pack_trusses([self]), [path], np.asarray(direction, dtype=float), train=train,
                                 want_lines=returnLines)
        if int(result.info[0]) != 0:
            raise np.linalg.LinAlgError("Singular matrix")
        at = lambda x: None if math.isnan(x) else float(x)
        records = {}
        for m in range(len(self._bars)):
            rec = {"max": float(result.N_max[0, m]), "maxAt": at(result.x_max[0, m]),
                   "min": float(result.N_min[0, m]), "minAt": at(result.x_min[0, m]),
                   "areaPositive": float(result.area_pos[0, m]), "areaNegative": float(result.area_neg[0, m])}
            if returnLines:
                rec["ordinates"] = [float(v) for v in result.lines[0, m, :len(path)]]
            records[m] = rec
        return records

    def AdoptDenseResults(self, displace, external, internal):
        """Install dense results (`[nJoint, dim]`, `[nJoint, dim]`, `[nMember]`) as the
        sparse result dicts of the reference: entries below 1e-10 in every component are
        dropped (`truss.py:344-345,350-351,358-359`).  Used by `Solve()` and by the
        batched callers, which solve many trusses in one launch."""
        nJ, nM, dim = len(self._pos), len(self._bars), self._dim
        u = np.asarray(displace, dtype=float)[:nJ, :dim]
        f = np.asarray(external, dtype=float)[:nJ, :dim]
        n = np.asarray(internal, dtype=float)[:nM]
        keep_u = (np.abs(u) >= ZERO_EPS).any(axis=1)
        keep_f = (np.abs(f) >= ZERO_EPS).any(axis=1)
        ju, jf, jm = np.flatnonzero(keep_u), np.flatnonzero(keep_f), np.flatnonzero(np.abs(n) >= ZERO_EPS)
        # (one copy per array, its rows handed out as the dict values: they do not alias the caller's arrays)
        self._displace = dict(zip(ju.tolist(), u[ju]))
        self._external = dict(zip(jf.tolist(), f[jf]))
        self._internal = dict(zip(jm.tolist(), n[jm].tolist()))
        self._solved = True

    # --------------------------------------------------------------------- JSON
    def Serialize(self):
        """The JSON-ready dict of `detail/combine_with_JSON.md:71-163` (`truss.py:367-398`)."""
        data = {
            "joint": [[list(p), SupportType.GetFromType(s)] for p, s in zip(self._pos, self._sup)],
            "force": [[j, list(v)] for j, v in self._loads.items()],
            "member": [[[j0, j1], bar._type.Serialize()]
                       for (j0, j1), bar in zip(self._ends, self._bars)],
        }
        if self._solved:
            data["displace"] = [[j, list(v)] for j, v in self._displace.items()]
            data["external"] = [[j, list(v)] for j, v in self._external.items()]
            data["internal"] = [[m, float(v)] for m, v in self._internal.items()]
            data["weight"] = self.weight
        return data

    def LoadFromJSON(self, path=None, isOutputFile=False, data=None):
        if data is None:
            with open(path, "r", encoding="utf-8") as f:
                data = json.load(f)
        for vector, supportName in data["joint"]:
            self.AddNewJoint(vector, SupportType.GetFromString(supportName))
        for jointID, vector in data["force"]:
            self.AddExternalForce(jointID, vector)
        for (jointID0, jointID1), typeList in data["member"]:
            self.AddNewMember(jointID0, jointID1, MemberType(*typeList))
        if isOutputFile:
            self._displace = {j: np.array(v) for j, v in data["displace"]}
            self._external = {j: np.array(v) for j, v in data["external"]}
            self._internal = {m: float(v) for m, v in data["internal"]}
            self._solved = True
        return self

    def DumpIntoJSON(self, path):
        with open(path, "w", encoding="utf-8") as f:
            json.dump(self.Serialize(), f, ensure_ascii=False)

    def Copy(self):
        return Truss(self._dim).LoadFromJSON(data=self.Serialize(), isOutputFile=self._solved)

    # ------------------------------------------------------- constraint checks
    def _excess(self, values, limit, isGetSumViolation, isGetSumNonViolation):
        """Shared body of the two `Is...Allowed` checks (`truss.py:429-462`).
        `values` is an iterable of (key, magnitude)."""
        values = list(values)
        if isGetSumViolation:
            violation = sum(v - limit for _, v in values if v > limit)
            ok = bool(IsZero(violation))
        else:
            violation = {key: v - limit for key, v in values if v > limit}
            ok = len(violation) == 0
        if isGetSumNonViolation:
            return ok, violation, sum(limit - v for _, v in values if v <= limit)
        return ok, violation

    def IsInternalStressAllowed(self, limit, isGetSumViolation=False, isGetSumNonViolation=False):
        if not self._solved:
            raise TrussNotSolvedError("Haven't done structural analysis yet.")
        stresses = ((m, abs(force) / self._bars[m].a) for m, force in self._internal.items())
        return self._excess(stresses, limit, isGetSumViolation, isGetSumNonViolation)

    def IsDisplacementAllowed(self, limit, isGetSumViolation=False, isGetSumNonViolation=False):
        if not self._solved:
            raise TrussNotSolvedError("Haven't done structural analysis yet.")
        lengths = ((j, GetLength(d)) for j, d in self._displace.items())
        return self._excess(lengths, limit, isGetSumViolation, isGetSumNonViolation)


class LoadCase:
    """One load case of `Truss.SolveEffectCases`: what acts on the structure beside (or in place of) joint forces.

    `forces`      {jointID: vector}   joint forces, as `AddExternalForce` takes them;
    `settlements` {jointID: vector}   prescribed displacements of a SUPPORTED joint - the components along its free
                                      axes must be zero;
    `prestrains`  {memberID: eps0}    member initial strain: alpha * dT for a temperature change, dL / L for a member
                                      fabricated too long (positive: the member wants to be longer);
    `gravity`     vector or None      body-force vector per unit weight: every member loads each of its end joints with
                                      half of a * length * density times it, e.g. (0, 0, -1) for weight densities."""

    def __init__(self, forces=None, settlements=None, prestrains=None, gravity=None):
        self.forces = dict(forces or {})
        self.settlements = dict(settlements or {})
        self.prestrains = dict(prestrains or {})
        self.gravity = None if gravity is None else tuple(float(x) for x in gravity)

    def __repr__(self):
        return (f"LoadCase(forces={self.forces!r}, settlements={self.settlements!r}, prestrains={self.prestrains!r}, "
                f"gravity={self.gravity!r})")


def pack_load_cases(cases, nJoint, nMember, dim):
    """A list of `LoadCase` as the dense arrays of `batch.solve_effect_cases` for ONE truss: a dict with `loads`,
    `settlement` [1, L, nJoint, 3], `prestrain` [1, L, nMember] and `accel` [1, L, 3]; an effect that no case carries is
    None (the cases that lack one the others carry get zeros).  Raises `InvaildJointError` / KeyError for an id the
    truss does not have and `DimensionError` for a vector that is not `dim` long."""
    cases = list(cases)
    L = len(cases)

    def vector(v):
        if len(v) != dim:
            raise DimensionError(f"Dimension of each vector of a load case must be {dim}, but got {len(v)}.")
        return [float(x) for x in v]

    def joints(field):
        if not any(getattr(c, field) for c in cases):
            return None
        out = np.zeros([1, L, nJoint, 3])
        for k, c in enumerate(cases):
            for jointID, v in getattr(c, field).items():
                if not (isinstance(jointID, (int, np.integer)) and 0 <= jointID < nJoint):
                    raise InvaildJointError(f"No such joint [{jointID}] in load case {k}.")
                out[0, k, jointID, :dim] = vector(v)
        return out

    prestrain = None
    if any(c.prestrains for c in cases):
        prestrain = np.zeros([1, L, nMember])
        for k, c in enumerate(cases):
            for memberID, eps0 in c.prestrains.items():
                if not (isinstance(memberID, (int, np.integer)) and 0 <= memberID < nMember):
                    raise KeyError(f"No such member [{memberID}] in load case {k}.")
                prestrain[0, k, memberID] = float(eps0)
    accel = None
    if any(c.gravity is not None for c in cases):
        accel = np.zeros([1, L, 3])
        for k, c in enumerate(cases):
            if c.gravity is not None:
                accel[0, k, :dim] = vector(c.gravity)
    return {"loads": joints("forces"), "settlement": joints("settlements"), "prestrain": prestrain, "accel": accel}


def load_cases_from_json(paths):
    """Several input files of ONE structure (the reference ships its examples so: `bar-47_input_{0,1,2}.json`) as
    `(Truss, cases)`: the truss of the first file (with that file's forces) and one `{jointID: vector}` dict of forces
    per file, for `Truss.SolveLoadCases`.  Raises ValueError naming the first file whose `joint` or `member` block
    differs from the first file's."""
    paths = list(paths)
    if not paths:
        raise ValueError("load_cases_from_json: no files")
    datas = []
    for path in paths:
        with open(path, "r", encoding="utf-8") as fh:
            datas.append(json.load(fh))
    first = datas[0]
    for path, data in zip(paths[1:], datas[1:]):
        for block in ("joint", "member"):
            if data[block] != first[block]:
                raise ValueError(f"load_cases_from_json: the {block!r} block of {path} differs from {paths[0]}'s: "
                                 "load cases must share one structure")
    dim = len(first["joint"][0][0]) if first["joint"] else 3
    truss = Truss(dim).LoadFromJSON(data={k: first[k] for k in ("joint", "force", "member")})
    cases = [{int(j): tuple(float(x) for x in v) for j, v in data["force"]} for data in datas]
    return truss, cases
