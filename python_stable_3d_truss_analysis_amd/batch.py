"""Batched `Truss.Solve()`: packing of many trusses into SoA tensors, the device pipeline
(dofmap -> assemble -> potrf -> potrs -> recover through the C ABI), and the dense results.

This is the layer the reference does not have: its `Solve()` (`slientruss3d/truss.py:329-364`)
handles one truss per call.  `Truss.Solve()` here is `solve_batch([truss])`.

All device work is enqueued on the current PyTorch-ROCm stream; tensors are only the memory
the kernels run on (plumbing).  No CPU fallback: without a GPU or the built library the calls
raise `HipExtensionError`.
"""
import os
from dataclasses import dataclass

import numpy as np

from . import _capi, _hostapi
from ._capi import (ASM_ALL_NARROW, ASM_ALL_TILES, ASM_ALL_WIDE, ASM_COMPACT, ASM_FULL_SYMMETRIC,   # noqa: F401
                    HINT_ALL_TILES, HINT_ALL_WIDE, HINT_COMPACT, HINT_NO_SMALL, HINT_NO_WIDE, HINT_RECOVER_SCAN,
                    HINT_RECOVER_UNSTAGED, HINT_SEPARATE_STAGES, HINT_SUBSTITUTED, MODES_BLOCK, NARROW_MAX_BELOW, ORDER_RCM_BELOW)
from .type import SupportType
from .utils import HipExtensionError


@dataclass
class PackedBatch:
    """B trusses as padded host arrays (numpy), ready to be uploaded.

    xyz [B,nJ_max,3] f64 | conn [B,nM_max,2] i32 | E, A, rho [B,nM_max] f64 |
    cbits [B,nJ_max] u8 (constrained-axis bits x=1,y=2,z=4) | loads [B,nJ_max,3] f64 |
    nJ, nM [B] i32 | dim [B] (2 or 3; 2D trusses are embedded with z fixed) | n_free [B] i32.

    TABLE member form (`table()`; ABI 10, `include/trs_solver.h` "Member forms"): the members' sections as one uint8
    `type_idx` [B,nM_max] into a table `types` [T,3] = (a, e, density), T <= 256 - the reference's own description of
    a member, `[[j0, j1], [a, e, density]]` with the triple drawn from a short list (`MemberType`, type.py:5-27) -
    and `conn` as uint16 pairs; E, A, rho are then None.  5 instead of 32 bytes per member in host memory, over PCIe
    and in HBM; the solvers take either form and give the same bits."""
    xyz: np.ndarray
    conn: np.ndarray
    E: np.ndarray
    A: np.ndarray
    rho: np.ndarray
    cbits: np.ndarray
    loads: np.ndarray
    nJ: np.ndarray
    nM: np.ndarray
    dim: np.ndarray
    n_free: np.ndarray
    type_idx: np.ndarray = None
    types: np.ndarray = None

    #: fields that are per batch, not per truss (never indexed, tiled or trimmed)
    _SHARED = ("types",)

    @property
    def B(self):
        return int(self.nJ.shape[0])

    @property
    def nJ_max(self):
        return int(self.xyz.shape[1])

    @property
    def nM_max(self):
        return int(self.conn.shape[1])

    @property
    def n_max(self):
        return int(self.n_free.max()) if self.B else 0

    @property
    def is_table(self):
        return self.type_idx is not None

    def constrained(self):
        """bool [B, nJ_max, 3]: the DOF is held by a support (the bits of `cbits`; False on padding joints)."""
        bits = np.asarray(self.cbits, dtype=np.uint8)
        live = np.arange(self.nJ_max)[None, :] < np.asarray(self.nJ)[:, None]
        return (((bits[:, :, None] >> np.arange(3, dtype=np.uint8)) & 1) != 0) & live[:, :, None]

    def _map(self, fn):
        """A batch whose per-truss arrays are `fn(field name, array)` (absent fields stay absent, the type table is shared)."""
        vals = {}
        for f in self.__dataclass_fields__:
            a = getattr(self, f)
            vals[f] = a if a is None or f in self._SHARED else fn(f, a)
        return PackedBatch(**vals)

    def replicate(self, times):
        """The same trusses `times` times over, as independent problems (no sharing on device)."""
        return self._map(lambda f, a: np.ascontiguousarray(np.tile(a, (times,) + (1,) * (a.ndim - 1))))

    def take(self, index):
        """Sub-batch (rows `index`, any numpy index) - used to shard a batch over ranks."""
        return self._map(lambda f, a: np.ascontiguousarray(a[index]))

    def pinned(self):
        """The same batch in page-locked host memory (one copy; needs the GPU runtime): `solve_batch`
        then uploads it by DMA at the full PCIe rate instead of through the driver's bounce buffers.
        The arrays are numpy views of pinned torch tensors, which they keep alive."""
        import torch

        def pin(f, a):
            a = np.ascontiguousarray(a)
            t = torch.empty(a.shape, dtype=torch.from_numpy(a[:0].copy()).dtype, pin_memory=True)
            v = t.numpy()
            v[...] = a
            return v
        return self._map(pin)

    def trimmed(self):
        """The same batch with the joint / member padding cut to this batch's own maxima."""
        jm = max(1, int(self.nJ.max(initial=1)))
        mm = max(1, int(self.nM.max(initial=1)))
        cut = {"xyz": jm, "loads": jm, "cbits": jm, "conn": mm, "E": mm, "A": mm, "rho": mm, "type_idx": mm}
        return self._map(lambda f, a: np.ascontiguousarray(a[:, :cut[f]]) if f in cut else a)

    def table(self):
        """The same batch in the TABLE member form (see the class): raises ValueError when the members use more than
        256 distinct (a, e, density) triples.  A batch already in that form is returned as it is."""
        if self.is_table:
            return self
        if self.nJ_max > 65535:
            raise ValueError("table member form: end joints are uint16 (at most 65 535 joints per truss)")
        live = np.arange(self.nM_max)[None, :] < np.asarray(self.nM)[:, None]
        # distinct BIT patterns (the table must give back exactly the doubles the batch holds), found without sorting
        # tens of millions of members: a 64-bit hash per member, the distinct hashes block by block, the hash's index in
        # their sorted list by binary search, and then the check that every member's triple IS its table row's
        bits = [np.ascontiguousarray(a, dtype=np.float64).view(np.uint64) for a in (self.A, self.E, self.rho)]
        with np.errstate(over="ignore"):
            h = (bits[0] * np.uint64(0x9E3779B97F4A7C15)) ^ (bits[1] * np.uint64(0xC2B2AE3D27D4EB4F) + np.uint64(0x165667B19E3779F9)) \
                ^ (bits[2] * np.uint64(0xD6E8FEB86659FD93) + np.uint64(0x27D4EB2F165667C5))
        h = np.where(live, h, h[0, 0] if h.size else 0).ravel()    # (padding members take the first member's type)
        seen = np.zeros([0], dtype=np.uint64)
        for k in range(0, h.size, 1 << 22):
            seen = np.union1d(seen, np.unique(h[k: k + (1 << 22)]))
            if len(seen) > 256:
                raise ValueError(f"table member form: more than 256 distinct (a, e, density) triples")
        idx = np.searchsorted(seen, h)
        rep = np.zeros([max(1, len(seen))], dtype=np.int64)
        rep[idx[::-1]] = np.arange(h.size - 1, -1, -1)                 # first member of every hash value
        flat = [b.ravel() for b in bits]
        types_bits = np.stack([f[rep] for f in flat], axis=-1)
        if not all(np.array_equal(np.where(live.ravel(), flat[c], types_bits[idx, c]), types_bits[idx, c]) for c in range(3)):
            raise ValueError("table member form: hash collision between member types (use the general form)")
        order = np.lexsort((types_bits[:, 2].view(np.float64), types_bits[:, 1].view(np.float64), types_bits[:, 0].view(np.float64)))
        rank = np.empty_like(order)
        rank[order] = np.arange(len(order))
        types = np.ascontiguousarray(types_bits[order].view(np.float64)) if h.size else np.zeros([1, 3])
        type_idx = (rank[idx].astype(np.uint8).reshape(self.B, self.nM_max) * live).astype(np.uint8)
        vals = {f: getattr(self, f) for f in self.__dataclass_fields__}
        vals.update(conn=np.ascontiguousarray(self.conn, dtype=np.uint16), E=None, A=None, rho=None, type_idx=type_idx,
                    types=types)
        return PackedBatch(**vals)

    def general(self):
        """The same batch in the GENERAL member form (int32 end joints, E / A / rho per member; padding members get
        the sections of type 0, which no kernel reads)."""
        if not self.is_table:
            return self
        t = np.asarray(self.types, dtype=np.float64)[self.type_idx.astype(np.int64)]
        vals = {f: getattr(self, f) for f in self.__dataclass_fields__}
        vals.update(conn=np.ascontiguousarray(self.conn, dtype=np.int32), A=np.ascontiguousarray(t[..., 0]),
                    E=np.ascontiguousarray(t[..., 1]), rho=np.ascontiguousarray(t[..., 2]), type_idx=None, types=None)
        return PackedBatch(**vals)


@dataclass
class BatchSizes:
    """What the host needs to know about a batch whose arrays live on the DEVICE (`generate.generate_cube_batch_device`):
    the per-truss counts (they decide the size buckets and the slab shapes) and the padded widths.  Accepted
    wherever a `PackedBatch` is only asked for its sizes (`RaggedSolver(..., tensors=)`, `solve_batch(...,
    device_inputs=)`, `size_buckets`); `to_packed(tensors)` downloads the arrays."""
    nJ: np.ndarray
    nM: np.ndarray
    n_free: np.ndarray
    nJ_max: int
    nM_max: int

    @property
    def B(self):
        return int(self.nJ.shape[0])

    @property
    def n_max(self):
        return int(self.n_free.max()) if self.B else 0

    @property
    def dim(self):
        return np.full([self.B], 3, dtype=np.int32)

    def to_packed(self, tensors):
        """The same batch as host arrays (`PackedBatch`), downloaded from its device tensors."""
        host = {f: tensors[f].cpu().numpy() for f in ("xyz", "conn", "E", "A", "rho", "cbits", "loads")}
        return PackedBatch(host["xyz"], host["conn"], host["E"], host["A"], host["rho"], host["cbits"], host["loads"],
                           self.nJ.copy(), self.nM.copy(), self.dim, self.n_free.copy())


def count_free(cbits, nJ):
    """n_free[b] from the constraint bits (host copy of what trs_dofmap computes)."""
    bits = np.asarray(cbits, dtype=np.uint8)
    valid = np.arange(bits.shape[1])[None, :] < np.asarray(nJ)[:, None]
    constrained = ((bits & 1) + ((bits >> 1) & 1) + ((bits >> 2) & 1)) * valid
    return (3 * np.asarray(nJ) - constrained.sum(axis=1)).astype(np.int32)


def pack_arrays(xyz_list, conn_list, mtype_list, support_list, loads_list, dims):
    """Pack per-truss arrays: xyz [nJ,dim], conn [nM,2], mtype [nM,3]=(a,e,density),
    support [nJ] SupportType values, loads [nJ,dim]."""
    B = len(xyz_list)
    nJ = np.array([len(x) for x in xyz_list], dtype=np.int32)
    nM = np.array([len(c) for c in conn_list], dtype=np.int32)
    nJ_max, nM_max = max(1, int(nJ.max(initial=1))), max(1, int(nM.max(initial=1)))
    xyz = np.zeros([B, nJ_max, 3])
    loads = np.zeros([B, nJ_max, 3])
    cbits = np.zeros([B, nJ_max], dtype=np.uint8)
    conn = np.zeros([B, nM_max, 2], dtype=np.int32)
    E = np.ones([B, nM_max])
    A = np.ones([B, nM_max])
    rho = np.zeros([B, nM_max])
    for b in range(B):
        dim = dims[b]
        x = np.asarray(xyz_list[b], dtype=float).reshape(-1, dim)
        xyz[b, :nJ[b], :dim] = x
        loads[b, :nJ[b], :dim] = np.asarray(loads_list[b], dtype=float).reshape(-1, dim)
        table = SupportType._BITS3 if dim == 3 else SupportType._BITS2
        try:    # (one dict look-up per joint; an unknown type takes the slow road to the reference's exception)
            bits = np.array([table[s] for s in support_list[b]], dtype=np.uint8)
        except (KeyError, TypeError):
            bits = np.array([SupportType.ConstraintBits(s, dim) for s in support_list[b]], dtype=np.uint8)
        cbits[b, :nJ[b]] = bits | (4 if dim == 2 else 0)  # a 2D truss never moves in z
        if nM[b]:
            conn[b, :nM[b]] = np.asarray(conn_list[b], dtype=np.int32).reshape(-1, 2)
            mt = np.asarray(mtype_list[b], dtype=float).reshape(-1, 3)
            A[b, :nM[b]], E[b, :nM[b]], rho[b, :nM[b]] = mt[:, 0], mt[:, 1], mt[:, 2]
    dims = np.asarray(dims, dtype=np.int32)
    return PackedBatch(xyz, conn, E, A, rho, cbits, loads, nJ, nM, dims, count_free(cbits, nJ))


def pack_trusses(trusses):
    """`list[Truss]` -> `PackedBatch` (DOF order joint*dim + axis, reference `truss.py:312-314`)."""
    xyz, conn, mtype, sup, loads, dims = [], [], [], [], [], []
    for t in trusses:
        x, c, sections, supports, f = t.PackedArrays()
        xyz.append(x); conn.append(c); mtype.append(sections); sup.append(supports); loads.append(f)
        dims.append(t.dim)
    return pack_arrays(xyz, conn, mtype, sup, loads, dims)


def _member_form(packed, members):
    """`members`: "general" (E, A, rho per member), "table" (uint16 end joints, uint8 type index, type table; an
    error beyond 256 distinct triples) or "auto" (the table form whenever the batch allows it)."""
    if members == "general":
        return packed
    if members == "table":
        return packed.table()
    if members == "auto":
        try:
            return packed.table()
        except ValueError:
            return packed
    raise ValueError(f"members must be 'general', 'table' or 'auto', not {members!r}")


def pack_json(data_list, members="general"):
    """List of reference-format JSON dicts (`detail/combine_with_JSON.md:71-163`) -> PackedBatch,
    without building `Truss` objects (bulk path).  `members` = "auto": the table member form (`PackedBatch.table`)
    when the documents' `[a, e, density]` triples are at most 256 distinct ones."""
    xyz, conn, mtype, sup, loads, dims = [], [], [], [], [], []
    for data in data_list:
        dim = len(data["joint"][0][0])
        nJ = len(data["joint"])
        xyz.append(np.array([p for p, _ in data["joint"]], dtype=float))
        sup.append([SupportType.GetFromString(s) for _, s in data["joint"]])
        f = np.zeros([nJ, dim])
        for j, v in data["force"]:
            if np.any(np.abs(np.asarray(v, dtype=float)) >= 1e-10):  # zero loads are dropped (truss.py:181)
                f[j] = v
        loads.append(f)
        conn.append(np.array([c for c, _ in data["member"]], dtype=np.int32).reshape(-1, 2))
        mtype.append(np.array([t for _, t in data["member"]], dtype=float).reshape(-1, 3))
        dims.append(dim)
    return _member_form(pack_arrays(xyz, conn, mtype, sup, loads, dims), members)


_JSON_ERRORS = {1: "JSON syntax", 2: "inconsistent coordinate / load dimension", 3: "unknown or invalid support type",
                4: "joint id out of range", 5: "does not fit the padding", 6: "file cannot be read"}


def _pack_json_native(count, call):
    """Two passes through the native reader (`csrc/jsonpack.c`): sizes, then the padded arrays."""
    nJ = np.zeros([count], dtype=np.int32); nM = np.zeros([count], dtype=np.int32)
    dim = np.full([count], 3, dtype=np.int32)
    ptr = _hostapi.ptr

    def run(nJ_max, nM_max, arrays):
        rc = call(nJ_max, nM_max, *(ptr(a) for a in arrays), ptr(nJ), ptr(nM), ptr(dim))
        if rc != 0:
            index, code = (-rc) // 1000 - 1, (-rc) % 1000
            raise ValueError(f"truss JSON #{index}: {_JSON_ERRORS.get(code, code)}")

    run(0, 0, [None] * 7)
    jm, mm = max(1, int(nJ.max(initial=1))), max(1, int(nM.max(initial=1)))
    xyz = np.empty([count, jm, 3]); loads = np.empty([count, jm, 3])
    conn = np.empty([count, mm, 2], dtype=np.int32)
    E = np.empty([count, mm]); A = np.empty([count, mm]); rho = np.empty([count, mm])
    cbits = np.empty([count, jm], dtype=np.uint8)
    run(jm, mm, [xyz, conn, E, A, rho, cbits, loads])
    return PackedBatch(xyz, conn, E, A, rho, cbits, loads, nJ, nM, dim, count_free(cbits, nJ))


def pack_json_texts(texts, members="general"):
    """Reference-format JSON documents (`bytes` or `str`, one truss each) -> `PackedBatch` through the
    native bulk reader (`csrc/jsonpack.c`, OpenMP over the documents): no Python objects per joint or
    member.  Same arrays as `pack_json([json.loads(t) for t in texts])`; `members` as there."""
    import ctypes
    lib = _hostapi.load()
    raw = [t.encode("utf-8") if isinstance(t, str) else bytes(t) for t in texts]
    B = len(raw)
    arr = (ctypes.c_char_p * B)(*raw)
    lens = np.array([len(r) for r in raw], dtype=np.int64)
    return _member_form(_pack_json_native(B, lambda jm, mm, *rest: lib.trs_json_pack(
        B, arr, _hostapi.ptr(lens), jm, mm, *rest)), members)


def pack_json_files(paths, members="general"):
    """Truss JSON FILES -> `PackedBatch`; the files are read (once) and parsed natively, in parallel
    (the bulk form of `Truss.LoadFromJSON`, reference `truss.py:401-421`)."""
    import ctypes
    lib = _hostapi.load()
    raw = [os.fsencode(p) for p in paths]
    B = len(raw)
    arr = (ctypes.c_char_p * B)(*raw)
    bufs = (ctypes.c_void_p * B)()
    lens = np.zeros([B], dtype=np.int64)
    rc = lib.trs_json_read_files(B, arr, bufs, _hostapi.ptr(lens))
    try:
        if rc != 0:
            raise ValueError(f"truss JSON #{(-rc) // 1000 - 1}: {_JSON_ERRORS[6]}")
        return _member_form(_pack_json_native(B, lambda jm, mm, *rest: lib.trs_json_pack(
            B, bufs, _hostapi.ptr(lens), jm, mm, *rest)), members)
    finally:
        lib.trs_json_free_files(B, bufs)


@dataclass
class BatchResult:
    """Dense host results of a batched solve: displace/external [B,nJ_max,3], internal [B,nM_max],
    info [B] (0 ok, k>0: pivot k of the reduced stiffness matrix is not positive)."""
    displace: np.ndarray
    external: np.ndarray
    internal: np.ndarray
    info: np.ndarray


def _require_gpu(device):
    try:
        import torch
    except ImportError as exc:  # pragma: no cover
        raise HipExtensionError("PyTorch-ROCm is required for device memory and streams") from exc
    if not torch.cuda.is_available():
        raise HipExtensionError("no GPU visible: the truss solver has no CPU fallback")
    return torch, torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")


#: per-batch switches of the pipeline and their defaults.  None of them changes a result; they select
#: between kernels that compute the same thing (A/B runs, tests).  They travel as flags / hints of every C
#: call (include/trs_solver.h) - the library has no process-wide state - and are attributes of a
#: `DeviceBatch` (`dev.options["compact"] = True`, or `DeviceBatch(..., options={...})`).
#:   compact             K_ff leaves the assembly as compact entry lists, tiles formed in the factorisation
#:   fused_substitution  the wave that factors a narrow-envelope matrix substitutes it as well
#:   recover_unstaged    force trs_recover's path for trusses whose tables exceed a CU's LDS
#:   recover_scan        with recover_unstaged: also that path's fall-back without member-end lists (tests)
#:   all_wide            every matrix to the work-group factorisation (four waves per matrix), whatever its envelope:
#:                       for batches of few, large systems, which leave most SIMDs idle under the wave-per-matrix kernel
DEFAULT_OPTIONS = {"compact": False, "fused_substitution": True, "recover_unstaged": False, "recover_scan": False,
                   "all_wide": False}


def default_options():
    """`DEFAULT_OPTIONS`, overridden by the environment variable TRS_OPTIONS="name=value,name=value" (A/B runs
    of the tools without touching code); an unknown name is an error."""
    opts = dict(DEFAULT_OPTIONS)
    for item in filter(None, os.environ.get("TRS_OPTIONS", "").split(",")):
        name, _, value = item.partition("=")
        if name.strip() not in opts:
            raise ValueError(f"TRS_OPTIONS: unknown option {name.strip()!r} (known: {sorted(opts)})")
        opts[name.strip()] = bool(int(value))
    return opts


def order_plan(reorder, nJ_max, nM_max):
    """How a `reorder=` argument is carried out: None (no renumbering), ("given", perm array), ("device", effort)
    - `trs_joint_order` on the GPU, no host pass - or ("host", name) - `joint_order` on the host.

    True / "auto" = every coordinate sweep, plus reverse Cuthill-McKee and its reverse for small trusses (fewer than
    128 free joints) or where no sweep is possible - effort 3: on larger lattice-like trusses a sweep wins, and
    Cuthill-McKee is 40 % of the device kernel's time; "profile" = every candidate for every truss (effort 2);
    "fast" = RCM, its reverse and one sweep: on the device whenever the batch shape fits its kernel
    (`trs_joint_order_fits`), else on the host.  "rcm" = plain reverse Cuthill-McKee (host).  "host-auto" /
    "host-profile" / "host-fast" force the host versions (comparisons, tests); "device" insists on the device
    version (effort 3) and raises when the shape does not fit."""
    if reorder is False or reorder is None:
        return None
    if isinstance(reorder, np.ndarray):
        return ("given", reorder)
    if reorder in ("host-auto", "host-profile", "host-fast", "rcm"):
        return ("host", {"host-auto": "auto", "host-profile": "profile", "host-fast": "fast"}.get(reorder, reorder))
    if reorder is True or reorder in ("auto", "profile", "fast", "device"):
        fits = bool(_capi.load().trs_joint_order_fits(int(nJ_max), int(nM_max)))
        if fits:
            return ("device", {"fast": 1, "profile": 2}.get(reorder, 3))
        if reorder == "device":
            raise ValueError(f"joint order on the device: batch shape ({nJ_max} joints, {nM_max} members) does not "
                             "fit trs_joint_order (see trs_joint_order_fits)")
        return ("host", reorder if reorder in ("fast", "profile") else "auto")
    raise ValueError(f"unknown joint order {reorder!r} (True, 'auto', 'profile', 'fast', 'rcm', 'device', 'host-auto', "
                     "'host-profile', 'host-fast' or a permutation array)")


def joint_order_device(torch, tensors, effort=2, apply=True, want_choice=False, out=None):
    """`trs_joint_order` on resident inputs (`tensors`: xyz, conn, cbits, loads, nJ, nM on one device, padded
    shapes of `PackedBatch`): the cheapest joint order of every truss found ON THE GPU, asynchronously on the
    current stream.  Returns a dict: `perm` int32 [B, nJ_max] (old id of the joint that becomes joint k = the
    `joint_out` of the recovery), `reach` int32 [B] (envelope reach of the chosen order, the launch hint),
    `choice` (if asked) and, with `apply`, the renumbered `xyz`, `conn`, `cbits`, `loads`.  `out` = the dict
    of an earlier call with the same shapes: its tensors are written again (no allocation)."""
    lib = _capi.load()
    xyz, conn, cbits, loads = (tensors[k].contiguous() for k in ("xyz", "conn", "cbits", "loads"))
    # (uint16 end joints = the table member form: the _tab twin reads and writes them)
    order_fn, what = (lib.trs_joint_order_tab, "trs_joint_order_tab") if conn.dtype == torch.uint16 \
        else (lib.trs_joint_order, "trs_joint_order")
    dev = xyz.device
    B, nJ_max, nM_max = int(xyz.shape[0]), int(xyz.shape[1]), int(conn.shape[1])
    if out is None:
        out = {"perm": torch.empty([B, nJ_max], dtype=torch.int32, device=dev),
               "reach": torch.empty([B], dtype=torch.int32, device=dev)}
        if want_choice:
            out["choice"] = torch.empty([B], dtype=torch.int32, device=dev)
        if apply:
            out.update(xyz=torch.empty_like(xyz), conn=torch.empty_like(conn), cbits=torch.empty_like(cbits),
                       loads=torch.empty_like(loads))
    ptr = lambda k: out[k].data_ptr() if k in out else None
    with torch.cuda.device(dev):
        _capi.check(order_fn(
            B, nJ_max, nM_max, xyz.data_ptr(), conn.data_ptr(), cbits.data_ptr(), loads.data_ptr(),
            tensors["nJ"].data_ptr(), tensors["nM"].data_ptr(), out["perm"].data_ptr(), ptr("choice"),
            out["reach"].data_ptr(), ptr("xyz"), ptr("conn"), ptr("cbits"), ptr("loads"), int(effort),
            torch.cuda.current_stream(dev).cuda_stream), what)
    return out


#: `r_tol` of the member-loss analysis: a member whose redundancy r_e is at most this is critical.  Over the shipped
#: fixtures the critical members have |r| <= a few 1e-15 and the others r >= 3.8e-4 (EXPERIMENTS R14).
MEMBER_LOSS_R_TOL = 1e-8
#: members per scenario of `member_sets` at most (TRS_SETS_MAX of include/trs_sets.h)
MEMBER_SETS_MAX = _capi.SETS_MAX


def _round_up16(x):
    return -(-int(x) // 16) * 16


def _chunk_columns(chunk, nM_max=None):
    """The columns C of one substitution of the column analyses: `chunk` rounded up to a multiple of 16 (one case group),
    and no more than `nM_max` rounded up, when given."""
    C = _round_up16(chunk)
    return C if nM_max is None else max(16, min(C, _round_up16(nM_max)))


def plan_member_sets(sets, chunk, nM_max=None):
    """The ranges `DeviceBatch.member_sets` takes the scenario axis in.  `sets`: int array [B, S, K] of member ids, -1
    padding at the end of a set; `chunk`: columns per substitution, rounded up to C, a multiple of 16 (and no more than
    `nM_max` rounded up, when given).  The scenarios are taken in order into consecutive ranges [s0, s1), each as long
    as every truss's DISTINCT members of the range number at most C - a member that several scenarios of a range share
    costs one column - and a scenario is never split (it has at most C members: K <= C is required).  Returns a list of
    (s0, s1, cols, slot): cols int32 [B, C], the members of the range in order of first appearance, -1 beyond them;
    slot int32 [B, s1 - s0, K], the place in cols[b] of every member of every scenario, -1 where `sets` has -1.  Pure
    numpy: no device is needed."""
    sets = np.asarray(sets)
    B, S, K = sets.shape
    C = _chunk_columns(chunk, nM_max)
    if K > C:
        raise ValueError(f"plan_member_sets: a set of {K} members does not fit {C} columns")
    width = int(sets.max(initial=-1)) + 1 if nM_max is None else int(nM_max)
    rows = np.arange(B)[:, None]
    valid = sets >= 0
    safe = np.where(valid, sets, 0)
    place = np.full([B, max(width, 1)], -1, dtype=np.int32)   # member -> its column in the open range
    count = np.zeros([B], dtype=np.int64)
    cols = np.full([B, C], -1, dtype=np.int32)
    slot = np.full([B, S, K], -1, dtype=np.int32)
    out, s0 = [], 0
    for s in range(S):
        fresh = valid[:, s] & (place[rows, safe[:, s]] < 0)
        if s > s0 and (count + fresh.sum(axis=1) > C).any():
            out.append((s0, s, cols, slot[:, s0:s]))
            place[:], count[:], s0 = -1, 0, s
            cols = np.full([B, C], -1, dtype=np.int32)
            fresh = valid[:, s].copy()
        where = (count[:, None] + np.cumsum(fresh, axis=1) - 1).astype(np.int32)
        b_new, k_new = np.nonzero(fresh)
        place[b_new, safe[b_new, s, k_new]] = where[b_new, k_new]
        cols[b_new, where[b_new, k_new]] = safe[b_new, s, k_new]
        count += fresh.sum(axis=1)
        slot[:, s] = np.where(valid[:, s], place[rows, safe[:, s]], -1)
    if S:
        out.append((s0, S, cols, slot[:, s0:S]))
    return out


def _member_set_arrays(who, sets, gamma, B, nM, nM_max):
    """`sets` and `gamma` of a member-set analysis as host arrays int32 / float64 [B, S, 8] (gamma None stays None), or
    ValueError.  `sets`: an integer array [B, S, K <= 8] with -1 padding at the end of every set, or a list (per truss)
    of lists (per scenario) of member ids - trusses with fewer scenarios get empty sets; `gamma` in the same form as
    `sets`, entry for entry (its entries at the padding are ignored).  `nM` [B]: the member counts the ids are checked
    against (None: `nM_max` for every truss)."""
    nested = isinstance(sets, (list, tuple))
    if nested:
        if len(sets) != B or not all(isinstance(row, (list, tuple)) and all(isinstance(x, (list, tuple, np.ndarray))
                                                                             for x in row) for row in sets):
            raise ValueError(f"{who}: sets must hold one list of scenarios (lists of member ids) per truss (B={B})")
        S = max([len(row) for row in sets], default=0)
        if any(len(x) > MEMBER_SETS_MAX for row in sets for x in row):
            raise ValueError(f"{who}: a set holds more than {MEMBER_SETS_MAX} members")
        dense = np.full([B, S, MEMBER_SETS_MAX], -1, dtype=np.int64)
        for b, row in enumerate(sets):
            for i, x in enumerate(row):
                x = np.asarray(x)
                if x.size and x.dtype.kind not in "iu":
                    raise ValueError(f"{who}: member ids must be integers")
                if (x.astype(np.int64) < 0).any():
                    raise ValueError(f"{who}: scenario {i} of truss {b} names a member out of range")
                dense[b, i, :x.size] = x
    else:
        raw = _host_array(sets, None)
        if raw.ndim != 3 or raw.shape[0] != B or raw.dtype.kind not in "iu":
            raise ValueError(f"{who}: sets must be a list of lists of member-id lists or an integer array [B={B}, S, K]")
        if raw.shape[2] > MEMBER_SETS_MAX:
            raise ValueError(f"{who}: a set holds more than {MEMBER_SETS_MAX} members (K = {raw.shape[2]})")
        dense = np.full(raw.shape[:2] + (MEMBER_SETS_MAX,), -1, dtype=np.int64)
        dense[:, :, :raw.shape[2]] = raw
    S = dense.shape[1]
    valid = dense >= 0
    limit = np.full([B], nM_max, dtype=np.int64) if nM is None else np.asarray(nM, dtype=np.int64)
    if (dense < -1).any() or (dense >= limit[:, None, None]).any():
        b, i = [int(v[0]) for v in np.nonzero((dense < -1) | (dense >= limit[:, None, None]))[:2]]
        raise ValueError(f"{who}: scenario {i} of truss {b} names a member out of range (members 0 .. {int(limit[b]) - 1})")
    if (valid[:, :, 1:] & ~valid[:, :, :-1]).any():
        raise ValueError(f"{who}: -1 pads the END of a set only")
    ordered = np.sort(dense, axis=2)
    if ((ordered[:, :, 1:] == ordered[:, :, :-1]) & (ordered[:, :, 1:] >= 0)).any():
        b, i = [int(v[0]) for v in np.nonzero((ordered[:, :, 1:] == ordered[:, :, :-1]) & (ordered[:, :, 1:] >= 0))[:2]]
        raise ValueError(f"{who}: scenario {i} of truss {b} names a member twice")
    if gamma is None:
        return dense.astype(np.int32), None
    g = np.zeros([B, S, MEMBER_SETS_MAX])
    if isinstance(gamma, (list, tuple)) and nested:
        if len(gamma) != B or any(len(grow) != len(row) or any(len(gx) != len(x) for gx, x in zip(grow, row))
                                  for grow, row in zip(gamma, sets)):
            raise ValueError(f"{who}: the factors must match the sets entry for entry")
        for b, grow in enumerate(gamma):
            for i, gx in enumerate(grow):
                g[b, i, :len(gx)] = np.asarray(gx, dtype=np.float64)
    else:
        raw = _host_array(gamma, np.float64)
        if nested or raw.ndim != 3 or raw.shape[:2] != (B, S) or raw.shape[2] > MEMBER_SETS_MAX \
                or raw.shape[2] < int(valid.sum(axis=2).max(initial=0)):
            raise ValueError(f"{who}: the factors must match the sets entry for entry ([B={B}, S={S}, K])")
        g[:, :, :raw.shape[2]] = raw
    g = np.where(valid, g, 0.0)
    if not np.isfinite(g).all() or (g < 0.0).any():
        raise ValueError(f"{who}: a factor is negative or not finite")
    return dense.astype(np.int32), np.ascontiguousarray(g)


# -- what the analyses' host layers share: the scalar rules, the `sections=` refusal, the output table --------
#: the types of "a number"; a site that takes no numpy integer (a `tol`, an `r_tol`) passes _REAL_NO_NPINT
_REAL = (int, float, np.integer, np.floating)
_REAL_NO_NPINT = (int, float, np.floating)


def _check_number(who, name, x, must="be a finite number", above=None, least=None, below=None, types=_REAL):
    """`x` as a float: a finite number of `types` (never a bool) with x > `above`, x >= `least` and x < `below` where
    they are given (positive: above=0; non-negative: least=0; an interval: two of them); else ValueError
    "`who`: `name` must `must`, got ..."."""
    if isinstance(x, bool) or not isinstance(x, types) or not np.isfinite(x) or (above is not None and not x > above) \
            or (least is not None and not x >= least) or (below is not None and not x < below):
        raise ValueError(f"{who}: {name} must {must}, got {x!r}")
    return float(x)


def _check_integer(who, name, x, least=1):
    """`x` as an int: a Python or numpy integer (never a bool) of at least `least`; else ValueError."""
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or x < least:
        raise ValueError(f"{who}: {name} must be an integer of at least {least}, got {x!r}")
    return int(x)


def _refuse_sections(who, what, sections):
    """`sections=` variants are for `solve_batch` alone: every analysis refuses them in its own words (`what`)."""
    if sections is not None:
        raise ValueError(f"{who}: sections= variants cannot be combined with {what}")


def _refuse_variants(who, what, sections, options, cases="load cases"):
    """What the iterated analyses refuse before any device work: `sections=` variants, in their own words (`what`), and
    `options["compact"]`, which keeps no slab that their `cases` could be solved against."""
    _refuse_sections(who, what, sections)
    if options and options.get("compact"):
        raise ValueError(f"{who}: options['compact'] writes no slab that the {cases} could be solved against")


def _check_case_loads(who, loads, B, nJ_max):
    """`loads` of an iterated analysis on the host: [B, L >= 1, nJ_max, 2 or 3] (numpy, torch or nested lists), finite.
    Returns them as a contiguous float64 array [B, L, nJ_max, 3] (two components get z = 0), or None for None: the
    batch's own loads."""
    if loads is None:
        return None
    try:
        x = _host_array(loads, np.float64)
    except (TypeError, ValueError):
        x = None
    shape = None if x is None else tuple(x.shape)
    if x is None or len(shape) != 4 or shape[0] != B or shape[1] < 1 or shape[2] != nJ_max or shape[3] not in (2, 3):
        raise ValueError(f"{who}: loads must be [B={B}, L >= 1, nJ_max={nJ_max}, 2 or 3], got {shape}")
    if not np.isfinite(x).all():
        raise ValueError(f"{who}: loads must be finite")
    return np.ascontiguousarray(np.pad(x, [(0, 0)] * 3 + [(0, 3 - shape[3])]))


#: how the device holds a `FIELDS` dtype that it has no kernel type for: (device dtype, trailing axes)
_DEVICE_DTYPES = {"bool": ("int32", ()), "complex128": ("float64", (2,))}


def _field_shapes(fields, B, sizes, keys=None):
    """{device key: (shape, torch dtype)} - what `DeviceBatch._out_tensors` takes - from a result class's `FIELDS`
    (field -> (device key, fill, dtype, shape after B)) for the device keys named in `keys` (None: all of them).  A name
    in a shape ("L", "S", "P", "G", "V", "R", "H", "T1", "Pj", "Pm", "nJ", "nM") is looked up in `sizes`; one that
    `sizes` lacks is a KeyError that names the field.  `_DEVICE_DTYPES`: a "bool" is int32 on the device, a "complex128"
    float64 with a trailing axis of 2."""
    import torch
    by_key = {key: (field, dtype, shape) for field, (key, fill, dtype, shape) in fields.items()}
    shapes = {}
    for key in by_key if keys is None else keys:
        field, dtype, shape = by_key[key]
        dtype, tail = _DEVICE_DTYPES.get(dtype, (dtype, ()))
        missing = [n for n in shape if isinstance(n, str) and n not in sizes]
        if missing:
            raise KeyError(f"field {field!r}: no size {missing[0]!r} among {sorted(sizes)}")
        shapes[key] = ([B] + [sizes[n] if isinstance(n, str) else n for n in shape] + list(tail), getattr(torch, dtype))
    return shapes


def newmark_constants(dt, beta=0.25, gamma=0.5, damp_mass=0.0, damp_stiff=0.0):
    """The constants of the Newmark scheme of include/trs_dynamics.h as plain Python floats (the library forms the same
    ones in the same order): a0 .. a5, s = 1 + a1 damp_stiff and sigma = (a0 + a1 damp_mass) / s, the multiple of the mass
    that `DeviceBatch.factor_dynamic` adds to the stiffness.  ValueError for dt <= 0, beta <= 0, gamma < 1/2 and negative
    or non-finite damping."""
    dt, beta, gamma, damp_mass, damp_stiff = (_check_number("transient", name, x) for name, x in (
        ("dt", dt), ("beta", beta), ("gamma", gamma), ("damp_mass", damp_mass), ("damp_stiff", damp_stiff)))
    if not dt > 0.0:
        raise ValueError(f"transient: dt must be positive, got {dt!r}")
    if not beta > 0.0:
        raise ValueError(f"transient: beta must be positive, got {beta!r}")
    if not gamma >= 0.5:
        raise ValueError(f"transient: gamma must be at least 1/2, got {gamma!r}")
    if damp_mass < 0.0 or damp_stiff < 0.0:
        raise ValueError(f"transient: damp_mass and damp_stiff must be non-negative, got {damp_mass!r}, {damp_stiff!r}")
    a0, a1, a2 = 1.0 / (beta * dt * dt), gamma / (beta * dt), 1.0 / (beta * dt)
    a3, a4, a5 = 1.0 / (2.0 * beta) - 1.0, gamma / beta - 1.0, 0.5 * dt * (gamma / beta - 2.0)
    s = 1.0 + a1 * damp_stiff
    return {"dt": dt, "beta": beta, "gamma": gamma, "damp_mass": damp_mass, "damp_stiff": damp_stiff, "a0": a0, "a1": a1,
            "a2": a2, "a3": a3, "a4": a4, "a5": a5, "s": s, "sigma": (a0 + a1 * damp_mass) / s}


def _check_newton_args(who, load_factors, tol=1e-9, max_iters=25, check_every=1):
    """The Newton arguments of the nonlinear analysis (ValueError): `load_factors` a non-empty sequence of finite
    numbers, `tol` finite and positive, `max_iters` and `check_every` integers of at least 1.  Returns the load factors
    as a list of floats."""
    try:
        lams = [float(x) for x in np.asarray(load_factors, dtype=np.float64).reshape(-1)] \
            if np.ndim(load_factors) == 1 else None
    except (TypeError, ValueError):
        lams = None
    if not lams or not np.isfinite(lams).all():
        raise ValueError(f"{who}: load_factors must be a non-empty sequence of finite numbers, got {load_factors!r}")
    _check_number(who, "tol", tol, "be a finite positive number", above=0, types=_REAL_NO_NPINT)
    _check_integer(who, "max_iters", max_iters)
    _check_integer(who, "check_every", check_every)
    return lams


def _check_sizing_scalars(who, allow_tension, allow_compression, allow_displace=0.0, euler_kappa=0.0, relax=1.0, tol=1e-4,
                          max_iters=40, check_every=1, catalog=None, B=None):
    """The scalar arguments of the member sizing (ValueError): the two allowables finite and positive, `allow_displace`,
    `euler_kappa` and `tol` finite and >= 0, `relax` in (0, 1], `max_iters` an integer >= 0, `check_every` an integer
    >= 1, `catalog` (or None) 1 to 256 finite positive areas in strictly ascending order.  With `B` each of the three
    allowables may also be one value per truss (an array [B], numpy or torch).  Returns them as a dict of floats and
    ints, an allowable per truss and the catalogue as float64 arrays (or None)."""
    def number(name, x):
        if B is not None and name.startswith("allow_") and (np.ndim(x) == 1 or hasattr(x, "detach")):
            try:
                arr = np.array(_host_array(x, np.float64), dtype=np.float64)
            except (TypeError, ValueError):
                arr = None
            if arr is None or arr.shape != (B,) or not np.isfinite(arr).all():
                raise ValueError(f"{who}: {name} must be a finite number or {B} finite numbers, one per truss")
            return arr
        return _check_number(who, name, x)
    val = {}
    for name, x in (("allow_tension", allow_tension), ("allow_compression", allow_compression)):
        val[name] = number(name, x)
        if not np.all(val[name] > 0):
            raise ValueError(f"{who}: {name} must be positive, got {x!r}")
    for name, x in (("allow_displace", allow_displace), ("euler_kappa", euler_kappa), ("tol", tol)):
        val[name] = number(name, x)
        if np.any(val[name] < 0):
            raise ValueError(f"{who}: {name} must be >= 0, got {x!r}")
    val["relax"] = number("relax", relax)
    if not 0 < val["relax"] <= 1:
        raise ValueError(f"{who}: relax must lie in (0, 1], got {relax!r}")
    val["max_iters"] = _check_integer(who, "max_iters", max_iters, least=0)
    val["check_every"] = _check_integer(who, "check_every", check_every)
    val["catalog"] = None
    if catalog is not None:
        try:
            cat = np.array(_host_array(catalog, np.float64), dtype=np.float64)
        except (TypeError, ValueError):
            cat = None
        if cat is None or cat.ndim != 1 or not 1 <= cat.size <= _capi.SZ_MAX_CATALOG or not np.isfinite(cat).all() \
                or not (cat > 0).all() or not (np.diff(cat) > 0).all():
            raise ValueError(f"{who}: catalog must hold 1 to {_capi.SZ_MAX_CATALOG} finite positive areas in strictly "
                             f"ascending order, got {catalog!r}")
        val["catalog"] = cat
    return val


def _check_area_bounds(who, area_min, area_max, B, nM, nM_max):
    """`area_min` / `area_max` of the member sizing: each a scalar or an array [B, nM_max] (numpy or torch), finite, with
    area_min > 0 and area_max >= area_min on every live member (`nM` [B]: the member counts on the host, or None when
    they are not at hand - then every entry is checked).  Returns ((scalar or None, array or None), the same for max)."""
    out = []
    for name, x in (("area_min", area_min), ("area_max", area_max)):
        if x is None:
            raise ValueError(f"{who}: {name} must be given: a scalar or an array [B, nM_max]")
        if np.ndim(x) == 0 and not hasattr(x, "detach"):
            out.append((_check_number(who, name, x, "be a finite number or an array [B, nM_max]"), None))
            continue
        try:
            arr = _host_array(x, np.float64)
        except (TypeError, ValueError):
            arr = None
        if arr is None or arr.shape != (B, nM_max) or not np.isfinite(arr).all():
            raise ValueError(f"{who}: {name} must be a finite number or a finite array [B={B}, nM_max={nM_max}]")
        out.append((None, arr))
    live = np.ones([B, nM_max], dtype=bool) if nM is None else np.arange(nM_max)[None, :] < np.asarray(nM)[:, None]
    lo = np.broadcast_to(out[0][0] if out[0][1] is None else out[0][1], [B, nM_max])
    hi = np.broadcast_to(out[1][0] if out[1][1] is None else out[1][1], [B, nM_max])
    if not (lo[live] > 0).all():
        raise ValueError(f"{who}: area_min must be positive on every member")
    if not (hi[live] >= lo[live]).all():
        raise ValueError(f"{who}: area_max must be >= area_min on every member")
    return tuple(out)


def _check_min_compliance_scalars(who, alpha=None, measure="weight", eta=0.5, move=0.2, tol=1e-4, max_iters=60,
                                  check_every=1, L=1):
    """The scalar arguments of the compliance sizing (ValueError): `alpha` L finite weights >= 0, not all zero (None:
    ones), `measure` "weight" or "volume", `eta` and `move` in (0, 1], `tol` finite and >= 0, `max_iters` an integer
    >= 0, `check_every` an integer >= 1.  Returns them as a dict; alpha as a float64 array [L]."""
    val = {}
    if alpha is None:
        val["alpha"] = np.ones([L], dtype=np.float64)
    else:
        try:
            arr = np.array(_host_array(alpha, np.float64), dtype=np.float64)
        except (TypeError, ValueError):
            arr = None
        if arr is None or arr.shape != (L,) or not np.isfinite(arr).all() or (arr < 0).any() or not (arr > 0).any():
            raise ValueError(f"{who}: alpha must hold {L} finite weights >= 0, one per load case and not all zero, "
                             f"got {alpha!r}")
        val["alpha"] = arr
    if not isinstance(measure, str) or measure not in _capi.CM_MEASURES:
        raise ValueError(f"{who}: measure must be one of {sorted(_capi.CM_MEASURES)}, got {measure!r}")
    val["measure"] = measure
    for name, x in (("eta", eta), ("move", move)):
        val[name] = _check_number(who, name, x, "lie in (0, 1]", above=0)
        if val[name] > 1:
            raise ValueError(f"{who}: {name} must lie in (0, 1], got {x!r}")
    val["tol"] = _check_number(who, "tol", tol, "be a finite number >= 0", least=0)
    val["max_iters"] = _check_integer(who, "max_iters", max_iters, least=0)
    val["check_every"] = _check_integer(who, "check_every", check_every)
    return val


def _check_target(who, target, B):
    """`target` of the compliance sizing as a float64 array [B]: a finite positive number, or B of them."""
    if np.ndim(target) == 0 and not hasattr(target, "detach"):
        return np.full([B], _check_number(who, "target", target, "be a finite positive number or one per truss", above=0))
    try:
        arr = np.array(_host_array(target, np.float64), dtype=np.float64)
    except (TypeError, ValueError):
        arr = None
    if arr is None or arr.shape != (B,) or not np.isfinite(arr).all() or not (arr > 0).all():
        raise ValueError(f"{who}: target must be a finite positive number or {B} of them, one per truss")
    return arr


def _check_min_weight_scalars(who, measure="weight", move=0.2, tol=1e-4, max_iters=60, sweeps=2, limit_tol=1e-2,
                              check_every=1):
    """The scalar arguments of the minimum-weight sizing (ValueError): `measure` "weight" or "volume", `move` in (0, 1],
    `tol` and `limit_tol` finite and >= 0, `max_iters` an integer >= 0, `sweeps` and `check_every` integers >= 1.
    Returns them as a dict."""
    val = {}
    if not isinstance(measure, str) or measure not in _capi.MW_MEASURES:
        raise ValueError(f"{who}: measure must be one of {sorted(_capi.MW_MEASURES)}, got {measure!r}")
    val["measure"] = measure
    val["move"] = _check_number(who, "move", move, "lie in (0, 1]", above=0)
    if val["move"] > 1:
        raise ValueError(f"{who}: move must lie in (0, 1], got {move!r}")
    val["tol"] = _check_number(who, "tol", tol, "be a finite number >= 0", least=0)
    val["limit_tol"] = _check_number(who, "limit_tol", limit_tol, "be a finite number >= 0", least=0)
    val["max_iters"] = _check_integer(who, "max_iters", max_iters, least=0)
    val["sweeps"] = _check_integer(who, "sweeps", sweeps)
    val["check_every"] = _check_integer(who, "check_every", check_every)
    return val


#: the results that `min_weight` has only with stress limits
_MW_STRESS_KEYS = ("utilisation", "governing", "stress_history")


def _check_stress_limits(who, allow_tension, allow_compression, euler_kappa, B):
    """The stress limits of the minimum-weight sizing (ValueError), by the rules of `_check_sizing_scalars`: both
    allowables None - no stress limits, `euler_kappa` must then be 0 - returns None; one None is refused; else each is a
    positive number or one per truss (an array [B], numpy or torch), and `euler_kappa` finite and >= 0.  +inf switches a
    side off: it goes through the check as a positive number and comes back as it was.  Returns {"allow_tension",
    "allow_compression": a float or a float64 array [B], "euler_kappa": a float}."""
    if allow_tension is None and allow_compression is None:
        if _check_number(who, "euler_kappa", euler_kappa) != 0.0:
            raise ValueError(f"{who}: euler_kappa needs allow_tension and allow_compression (+inf: no stress limit)")
        return None
    if allow_tension is None or allow_compression is None:
        raise ValueError(f"{who}: allow_tension and allow_compression must be given together (+inf switches one off)")

    def raw(x):
        if np.ndim(x) == 1 or hasattr(x, "detach"):
            try:
                return np.array(_host_array(x, np.float64), dtype=np.float64)
            except (TypeError, ValueError):
                return x
        return x

    def finite(x):
        if isinstance(x, np.ndarray):
            return np.where(x == np.inf, 1.0, x)
        return 1.0 if isinstance(x, _REAL) and not isinstance(x, bool) and x == np.inf else x
    given = {"allow_tension": raw(allow_tension), "allow_compression": raw(allow_compression)}
    val = _check_sizing_scalars(who, finite(given["allow_tension"]), finite(given["allow_compression"]), 0.0, euler_kappa,
                                B=B)
    out = {"euler_kappa": val["euler_kappa"]}
    for name, x in given.items():
        off = x == np.inf
        out[name] = np.where(off, np.inf, val[name]) if isinstance(val[name], np.ndarray) else (np.inf if off else val[name])
    return out


def _check_limits(who, limit_case, limit_joint, limit_direction, limit_value, B, nJ_max, L, nJ=None):
    """The displacement limits of the minimum-weight sizing (ValueError), J of them, 1 <= J <= 8: `limit_case` J integers
    in [0, L), shared by the batch; `limit_joint` integers [J] or [B, J] in the caller's joint numbering, -1 (switched
    off) to the truss's last joint (`nJ` [B]: the joint counts, or None: nJ_max for every truss); `limit_direction`
    [J, 2 or 3] or [B, J, 2 or 3], finite and not zero where the limit is switched on; `limit_value` a number, [J] or
    [B, J]: > 0, +inf switches a limit off.  Returns {"case": int32 [J], "joint": int32 [B, J], "direction": float64
    [B, J, 3] of unit length (zero where switched off), "value": float64 [B, J], "given": the directions as given,
    float64 [B, J, 3] - what `solve_min_weight` hands to its buckets, so that a direction is normalised once}."""
    def array(x, dtype):
        try:
            return np.array(_host_array(x, None))
        except (TypeError, ValueError):
            return None
    case = array(limit_case, None)
    most = _capi.MW_MAX_LIMITS
    if case is None or case.ndim != 1 or not 1 <= case.size <= most or case.dtype.kind not in "iu" \
            or (case < 0).any() or (case >= L).any():
        raise ValueError(f"{who}: limit_case must hold 1 to {most} integers in [0, L={L}), one per limit, got {limit_case!r}")
    J = int(case.size)
    joint = array(limit_joint, None)
    if joint is None or joint.dtype.kind not in "iu" or joint.shape not in ((J,), (B, J)):
        raise ValueError(f"{who}: limit_joint must be integers [J={J}] or [B={B}, J={J}]")
    joint = np.broadcast_to(joint, [B, J]).astype(np.int64)
    top = np.full([B], nJ_max) if nJ is None else np.asarray(nJ).reshape(B)
    if (joint < -1).any() or (joint >= top[:, None]).any():
        raise ValueError(f"{who}: limit_joint must name a joint of its truss, or -1 for a limit that is switched off")
    value = array(limit_value, None)
    if value is None or value.dtype.kind not in "iuf" or value.shape not in ((), (J,), (B, J)):
        raise ValueError(f"{who}: limit_value must be a number, [J={J}] or [B={B}, J={J}]")
    value = np.broadcast_to(value.astype(np.float64), [B, J]).copy()
    if np.isnan(value).any() or not (value > 0).all():
        raise ValueError(f"{who}: limit_value must be positive (+inf switches a limit off)")
    d = array(limit_direction, None)
    if d is None or d.dtype.kind not in "iuf" or d.shape[:-1] not in ((J,), (B, J)) or d.shape[-1] not in (2, 3) \
            or not np.isfinite(d).all():
        raise ValueError(f"{who}: limit_direction must be finite, [J={J}, 2 or 3] or [B={B}, J={J}, 2 or 3]")
    d = np.broadcast_to(d.astype(np.float64), [B, J, d.shape[-1]])
    d = np.concatenate([d, np.zeros([B, J, 3 - d.shape[-1]])], axis=2)
    on = (joint >= 0) & np.isfinite(value)
    norm = np.sqrt((d * d).sum(axis=2))
    if not (norm[on] > 0).all():
        raise ValueError(f"{who}: limit_direction must not be zero where the limit is switched on")
    unit = np.where(on[..., None], d / np.where(on, norm, 1.0)[..., None], 0.0)
    return {"case": case.astype(np.int32), "joint": joint.astype(np.int32), "direction": np.ascontiguousarray(unit),
            "value": value, "given": np.ascontiguousarray(d)}


def _check_mass_args(who, B, nJ_max, joint_mass_shape, mass_scale, joint_mass_min=None):
    """The mass arguments that the transient analysis shares with `modes` (`_check_mode_args`), refused in `who`'s name."""
    try:
        _check_mode_args(B, nJ_max, 1, joint_mass_shape, mass_scale, 1.0, 1, joint_mass_min=joint_mass_min)
    except ValueError as exc:
        raise ValueError(str(exc).replace("modes:", who + ":", 1)) from None


#: `status` of `DeviceBatch.buckling` / `solve_buckling`: the critical factor was found; the truss has no positive factor;
#: `max_shifts` rounds ended with negative factors only; the last round did not converge within `max_iters`; the
#: factorisation of K + theta Kg failed
BK_FOUND, BK_NONE, BK_SHIFT_LIMIT, BK_ITER_LIMIT, BK_NOT_PD = 0, 1, 2, 3, 4


def _ptr(x):
    """The device address of an optional tensor argument of a C call."""
    return None if x is None else x.data_ptr()


class DeviceBatch:
    """A packed batch resident in HBM plus the workspace of the pipeline.

    Build once, call `solve()` any number of times (e.g. after `set_sections`).  Every tensor
    lives on one device; kernels run on the current stream of that device.
    """
    INPUT_FIELDS = ("xyz", "conn", "E", "A", "rho", "cbits", "loads", "nJ", "nM")
    #: the inputs of a batch in the TABLE member form (`PackedBatch.table`): uint16 end joints, a uint8 type index per
    #: member and - shared by the batch - the type table `types` [T, 3] = (a, e, density)
    TABLE_FIELDS = ("xyz", "conn", "type_idx", "cbits", "loads", "nJ", "nM")

    def __init__(self, packed: PackedBatch, device=None, use_envelope=True, use_small=True, reorder=False,
                 options=None):
        """`use_envelope=False` treats every reduced stiffness matrix as dense (no tile skipping);
        `use_small=False` keeps a batch of small trusses off the fused single-kernel path
        (`trs_solve_small`) and sends it through the staged pipeline; `reorder` (see `joint_order`) uploads
        the trusses with their joints renumbered for a narrower envelope - the results still arrive in the
        caller's numbering (`trs_recover` writes them through `joint_out`), so nothing else changes."""
        torch, dev = _require_gpu(device)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.packed = packed
        plan = order_plan(reorder, packed.nJ_max, packed.nM_max)
        if plan is not None and use_small and _capi.load().trs_solve_small_fits(packed.nJ_max, packed.nM_max, packed.n_max):
            plan = None   # the fused small-system kernel keeps its matrix in LDS: nothing to gain from an order
        perm, resident, ordered = None, packed, None
        if plan is not None and plan[0] != "device":
            perm = joint_order(packed.general(), plan[1])   # found once, on the host
            resident = permute_joints(packed.general(), perm)
            if packed.is_table:   # (members keep their order: the type indices stay, the end joints are renumbered)
                import dataclasses
                resident = dataclasses.replace(packed, xyz=resident.xyz, cbits=resident.cbits, loads=resident.loads,
                                               conn=np.ascontiguousarray(resident.conn, dtype=np.uint16))
        tensors = {f: up(getattr(resident, f)) for f in (self.TABLE_FIELDS if packed.is_table else self.INPUT_FIELDS)}
        if packed.is_table:
            tensors["types"] = up(np.asarray(packed.types, dtype=np.float64))
        if plan is not None and plan[0] == "device" and packed.B:
            # found, applied and priced on the GPU (trs_joint_order): no host pass over the batch
            ordered = joint_order_device(torch, tensors, effort=plan[1])
            tensors.update({k: ordered[k] for k in ("xyz", "conn", "cbits", "loads")})
        self._setup(torch, dev, tensors, packed.B, packed.nJ_max, packed.nM_max, packed.n_max, use_envelope, use_small)
        self.options.update(options or {})
        if perm is not None:
            self.joint_out = up(perm)
        # what the launches may be told about this batch (see `all_narrow`): the reach of its envelopes - from
        # the device order's own pricing, else from the host's envelope analysis
        if use_envelope and not self.small and packed.B:
            if ordered is not None:
                self.joint_out = ordered["perm"]
                self.all_narrow = bool(int(ordered["reach"].max().item()) <= NARROW_MAX_BELOW)
            else:
                self.all_narrow = bool(envelope_reach(resident.general()).max() <= NARROW_MAX_BELOW)
        elif ordered is not None:
            self.joint_out = ordered["perm"]

    @classmethod
    def from_device(cls, tensors, n_max, use_envelope=True, use_small=True, joint_out=None, all_narrow=False):
        """A batch whose inputs already live on the device: `tensors` maps INPUT_FIELDS (or, table member form,
        TABLE_FIELDS + "types") to contiguous
        device tensors of the padded shapes (see PackedBatch); `n_max` bounds the free DOFs per truss
        (host-known, it sizes the slab); `joint_out` (int32 [B, nJ_max] on the device, or None): the
        results of joint j go to row joint_out[b, j] (the joint order the caller applied to the inputs)."""
        torch, dev = _require_gpu(tensors["xyz"].device)
        self = cls.__new__(cls)
        self.packed = None
        self._setup(torch, dev, tensors, int(tensors["xyz"].shape[0]), int(tensors["xyz"].shape[1]),
                    int(tensors["conn"].shape[1]), int(n_max), use_envelope, use_small)
        if joint_out is not None:
            if self.small:
                raise ValueError("a batch on the fused small-system path takes no joint order")
            if tuple(joint_out.shape) != (self.B, self.nJ_max) or joint_out.dtype != torch.int32:
                raise ValueError("joint_out must be int32 [B, nJ_max]")
            self.joint_out = joint_out.contiguous()
        self.all_narrow = bool(all_narrow and use_envelope and not self.small)
        return self

    def _setup(self, torch, dev, tensors, B, nJ_max, nM_max, n_max, use_envelope, use_small=True):
        self.torch, self.device = torch, dev
        self.lib = _capi.load()
        self.B, self.nJ_max, self.nM_max, self.n_max = B, nJ_max, nM_max, n_max
        #: table member form: conn uint16, `type_idx` + `types` in place of E / A / rho (which are then None)
        self.table = tensors.get("type_idx") is not None
        for f in self.INPUT_FIELDS + ("type_idx", "types"):
            setattr(self, f, tensors.get(f))
        if self.table and (self.conn.dtype != torch.uint16 or self.type_idx.dtype != torch.uint8 or self.types is None):
            raise ValueError("table member form: conn uint16 [B, nM_max, 2], type_idx uint8 [B, nM_max], types float64 [T, 3]")
        self.ld = self.lib.trs_slab_ld(self.n_max)
        self.rows = self.lib.trs_slab_rows(self.n_max)
        #: the whole batch goes through the fused small-system kernel (n_free <= 128, tables fit the LDS)
        self.small = bool(use_small and self.lib.trs_solve_small_fits(nJ_max, nM_max, n_max))
        self.use_envelope = use_envelope
        self.free_index = torch.empty([B, self.nJ_max * 3], dtype=torch.int32, device=dev)
        self.n_free = torch.empty([B], dtype=torch.int32, device=dev)
        self.u = torch.empty([B, self.nJ_max, 3], dtype=torch.float64, device=dev)
        self.f_ext = torch.empty([B, self.nJ_max, 3], dtype=torch.float64, device=dev)
        self.N = torch.empty([B, self.nM_max], dtype=torch.float64, device=dev)
        self.info = torch.empty([B], dtype=torch.int32, device=dev)
        self._slab = None   # (S, uf, work, env): the staged pipeline's workspace, allocated on first use
        self.joint_out = None   # int32 [B, nJ_max]: where the results of (resident) joint j go, or None
        #: the host knows that no envelope of this batch reaches further than NARROW_MAX_BELOW chunks below its
        #: diagonal blocks (`envelope_reach`): every matrix is then routed to the wave-per-matrix kernels
        #: (TRS_ASM_ALL_NARROW) and the work-group kernels, which would find nothing, are not launched.  Safe
        #: either way - with the flag the device routes so regardless - it only must not outlive the topology.
        self.all_narrow = False
        #: the host has SEEN (`adopt_tile_hint`) that no matrix of this resident batch leaves tiles of its envelope
        #: unwritten (trs_common.h `kmask`: a tower-like truss has too few tiles without an entry of K_ff for the
        #: skipping to pay): the assembly is then told not to form the masks again (TRS_ASM_ALL_TILES).  Like
        #: `all_narrow` it must not outlive the topology (`upload` resets it); a wrong value costs time, never a result.
        self.all_tiles = False
        self._potrf_fused = False
        self.options = default_options()

    def _workspace(self):
        """Stiffness slab, reduced solution, assembly workspace and envelope metadata of the staged
        pipeline; a batch on the fused small path never allocates them."""
        if self._slab is None:
            torch, dev, B = self.torch, self.device, self.B
            S = torch.empty([B, self.rows, self.ld], dtype=torch.float64, device=dev)
            if os.environ.get("TRS_DEBUG_POISON"):   # tests: any read of a never-written slab entry shows
                S.fill_(float("nan"))
            uf = torch.empty([B, self.rows], dtype=torch.float64, device=dev)
            work_bytes = self.lib.trs_assemble_work_bytes(self.nJ_max, self.nM_max, self.n_max)
            work = torch.empty([B, work_bytes], dtype=torch.uint8, device=dev)
            env = torch.zeros([B, self.lib.trs_env_ints(self.n_max)], dtype=torch.int32, device=dev) \
                if self.use_envelope else None
            self._slab = (S, uf, work, env)
        return self._slab

    S = property(lambda self: self._workspace()[0])
    uf = property(lambda self: self._workspace()[1])
    work = property(lambda self: self._workspace()[2])
    env = property(lambda self: self._workspace()[3])

    # -- individual stages (used by the parity tests and the benchmark) ------------------
    def _stream(self):
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def _env_ptr(self):
        return self.env.data_ptr() if self.env is not None else None

    def _members(self, types=None):
        """The three member arguments of a C call: (conn, E, A), or - table form - (conn16, type_idx, types)."""
        if self.table:
            return self.conn.data_ptr(), self.type_idx.data_ptr(), (self.types if types is None else types).data_ptr()
        return self.conn.data_ptr(), self.E.data_ptr(), self.A.data_ptr()

    def _fn(self, name):
        """The entry point `name`, or its `_tab` twin for a batch in the table member form."""
        return getattr(self.lib, name + "_tab" if self.table else name), name + ("_tab" if self.table else "")

    def dofmap(self):
        _capi.check(self.lib.trs_dofmap(self.B, self.nJ_max, self.cbits.data_ptr(), self.nJ.data_ptr(),
                                        self.free_index.data_ptr(), self.n_free.data_ptr(),
                                        self._stream()), "trs_dofmap")

    # -- the flag words of the C calls: one method per kind of call, composed nowhere else -------------
    def _enveloped(self):
        """There is envelope metadata and `all_wide` does not overrule it: what the narrow routing and the compact
        form need."""
        return self.env is not None and not self.options["all_wide"]

    def _assemble_flags(self):
        has_env = self.env is not None
        return (ASM_ALL_NARROW if self.all_narrow and self._enveloped() else 0) | \
               (ASM_COMPACT if self.options["compact"] and self._enveloped() else 0) | \
               (ASM_ALL_WIDE if self.options["all_wide"] and has_env else 0) | \
               (ASM_ALL_TILES if self.all_tiles and has_env else 0)

    def _form_hints(self):
        """How the matrices are stored and whether the factorising wave goes on to the substitution."""
        return (HINT_COMPACT if self.options["compact"] and self._enveloped() else 0) | \
               (0 if self.options["fused_substitution"] else HINT_SEPARATE_STAGES)

    def _potrf_hints(self):
        return (HINT_NO_WIDE if self.all_narrow and self._enveloped() else 0) | self._form_hints()

    def _potrs_hints(self):
        if not (self.all_narrow and self._enveloped()):
            return 0
        # (whether THIS batch's last factorisation ran with the substitution fused in, not the option's value now)
        fused = self.rows <= 1024 and self._potrf_fused
        return HINT_NO_WIDE | (HINT_SUBSTITUTED if fused else 0)

    def _recover_hints(self):
        return (HINT_RECOVER_UNSTAGED if self.options["recover_unstaged"] else 0) | \
               (HINT_RECOVER_SCAN if self.options["recover_scan"] else 0)

    def _solve_hints(self, rows=False):
        """`trs_solve` (never the fused small-system kernel: `solve` takes that path itself, by shape or by request), or
        `trs_solve_rows`.  TRS_HINT_NO_WIDE goes out whatever `all_wide` says: TRS_HINT_ALL_WIDE overrides it in C."""
        has_env = self.env is not None
        return (0 if rows else HINT_NO_SMALL) | self._form_hints() | self._recover_hints() | \
               (HINT_NO_WIDE if self.all_narrow and has_env else 0) | \
               (HINT_ALL_TILES if self.all_tiles and has_env else 0) | \
               (HINT_ALL_WIDE if self.options["all_wide"] and has_env else 0)

    def assemble(self, flags=0, xyz=None, loads=None):
        """`trs_assemble` of the resident batch; `xyz`, `loads` (float64 [B, nJ_max, 3] device tensors in the batch's own
        joint numbering): other coordinates and loads than the batch's own (`nonlinear`: the deformed coordinates and
        the residual)."""
        flags |= self._assemble_flags()
        fn, what = self._fn("trs_assemble")
        _capi.check(fn(
            self.B, self.nJ_max, self.nM_max, (self.xyz if xyz is None else xyz).data_ptr(), *self._members(),
            (self.loads if loads is None else loads).data_ptr(), self.free_index.data_ptr(),
            self.n_free.data_ptr(), self.nJ.data_ptr(), self.nM.data_ptr(), self.ld, self.rows,
            self.S.data_ptr(), flags, self.work.data_ptr(), self._env_ptr(), self.uf.data_ptr(), self.rows,
            self._stream()), what)

    def potrf(self):
        self._potrf_fused = bool(self.options["fused_substitution"])
        _capi.check(self.lib.trs_potrf_batched(self.B, self.n_free.data_ptr(), self.ld, self.rows,
                                               self.S.data_ptr(), self.info.data_ptr(), self._env_ptr(),
                                               self.work.data_ptr(), self.uf.data_ptr(), self.rows,
                                               self._potrf_hints(), self._stream()), "trs_potrf_batched")

    def potrs(self):
        _capi.check(self.lib.trs_potrs_batched(self.B, self.n_free.data_ptr(), self.ld, self.rows,
                                               self.S.data_ptr(), self.uf.data_ptr(), self.rows,
                                               self._env_ptr(), self._potrs_hints(), self._stream()),
                    "trs_potrs_batched")

    def recover(self):
        fn, what = self._fn("trs_recover")
        _capi.check(fn(
            self.B, self.nJ_max, self.nM_max, self.xyz.data_ptr(), *self._members(),
            self.loads.data_ptr(), self.free_index.data_ptr(),
            self.nJ.data_ptr(), self.nM.data_ptr(), self.uf.data_ptr(), self.rows, self.u.data_ptr(),
            self.f_ext.data_ptr(), self.N.data_ptr(),
            self.joint_out.data_ptr() if self.joint_out is not None else None,
            self._recover_hints(), self._stream()), what)

    def recover_rows(self, rows, out, nJ_out_max, nM_out_max):
        """`trs_recover_rows`: the recovery with a ragged batch's bucket scatter folded in - the results of truss b go
        to row rows[b] (int64 device tensor) of `out["u"]`, `out["f_ext"]` [*, nJ_out_max, 3], `out["N"]`
        [*, nM_out_max] and `out["info"]`."""
        fn, what = self._fn("trs_recover_rows")
        _capi.check(fn(
            self.B, self.nJ_max, self.nM_max, self.xyz.data_ptr(), *self._members(),
            self.loads.data_ptr(), self.free_index.data_ptr(),
            self.nJ.data_ptr(), self.nM.data_ptr(), self.uf.data_ptr(), self.rows,
            self.joint_out.data_ptr() if self.joint_out is not None else None, self.info.data_ptr(),
            rows.data_ptr(), int(nJ_out_max), int(nM_out_max), out["u"].data_ptr(), out["f_ext"].data_ptr(),
            out["N"].data_ptr(), out["info"].data_ptr(), self._recover_hints(), self._stream()), what)

    def solve_rows(self, rows, out, nJ_out_max, nM_out_max, types=None):
        """`trs_solve_rows`: the staged pipeline in one C call with `recover_rows` as its last stage.  `types` (table
        member form only): another type table for this solve (e.g. every row the same fixed section)."""
        fn, what = self._fn("trs_solve_rows")
        with self.torch.cuda.device(self.device):
            _capi.check(fn(
                self.B, self.nJ_max, self.nM_max, self.n_max, self.xyz.data_ptr(), *self._members(types),
                self.cbits.data_ptr(), self.loads.data_ptr(),
                self.nJ.data_ptr(), self.nM.data_ptr(), self.free_index.data_ptr(),
                self.n_free.data_ptr(), self.ld, self.rows, self.S.data_ptr(), self.uf.data_ptr(),
                self.rows, out["u"].data_ptr(), out["f_ext"].data_ptr(), out["N"].data_ptr(),
                self.info.data_ptr(), self.work.data_ptr(), self._env_ptr(),
                self.joint_out.data_ptr() if self.joint_out is not None else None, rows.data_ptr(),
                int(nJ_out_max), int(nM_out_max), out["info"].data_ptr(),
                self._solve_hints(rows=True), self._stream()), what)

    def _solve_small(self, fitness=None, out=None, types=None):
        """`trs_solve_small`: the whole of `Truss.Solve()` in one kernel (optionally with the GA
        reductions); returns the three reduction tensors (`out`, three float64 [B] device tensors, or new ones) or
        None."""
        t = self.torch
        if fitness is None:
            out = [None, None, None]
        elif out is None:
            out = [t.empty([self.B], dtype=t.float64, device=self.device) for _ in range(3)]
        ptr = lambda x: None if x is None else x.data_ptr()
        fn, what = self._fn("trs_solve_small")
        # (general form: the densities of the fitness reductions are an argument; table form: they are in the table)
        rho = () if self.table else (self.rho.data_ptr() if fitness is not None else None,)
        with t.cuda.device(self.device):
            _capi.check(fn(
                self.B, self.nJ_max, self.nM_max, self.n_max, self.xyz.data_ptr(), *self._members(types),
                self.cbits.data_ptr(), self.loads.data_ptr(),
                self.nJ.data_ptr(), self.nM.data_ptr(), self.u.data_ptr(), self.f_ext.data_ptr(),
                self.N.data_ptr(), self.info.data_ptr(), self.free_index.data_ptr(), self.n_free.data_ptr(), *rho,
                float(fitness[0]) if fitness else 0.0, float(fitness[1]) if fitness else 0.0,
                ptr(out[0]), ptr(out[1]), ptr(out[2]), self._stream()), what)
        return out if fitness is not None else None

    def solve_fitness(self, allow_stress, allow_displace, out=None):
        """Solve and reduce to (weight, stress_violation, displacement_violation) per truss - one kernel
        on the fused small path, `solve()` + `fitness()` otherwise (GA generation, ga.py:139-160).  `out`: three
        float64 [B] device tensors to write into (e.g. the rows of one [3, B] tensor: one download)."""
        if self.small:
            return self._solve_small((allow_stress, allow_displace), out)
        self.solve()
        return self.fitness(allow_stress, allow_displace, out)

    def set_sections_from_genes(self, genes, count, n_member, type_table):
        """`trs_ga_sections`: A, E, rho of the resident batch from a GA population's gene matrix (uint8 device tensor
        [count, n_member]) and its type table (float64 device tensor [n_type, 3] = a, e, density)."""
        if self.table:
            raise ValueError("set_sections_from_genes needs the general member form")
        _capi.check(self.lib.trs_ga_sections(self.B, self.nM_max, int(count), int(n_member), int(type_table.shape[0]),
                                             genes.data_ptr(), type_table.data_ptr(), self.A.data_ptr(),
                                             self.E.data_ptr(), self.rho.data_ptr(), self._stream()), "trs_ga_sections")

    def solve(self, types=None):
        """The whole pipeline, asynchronous on the current stream: one kernel for a batch of small
        trusses (`trs_solve_small`), otherwise one C call that enqueues the five stages.  `types` as `solve_rows`."""
        if self.small:
            self._solve_small(types=types)
            return
        fn, what = self._fn("trs_solve")
        with self.torch.cuda.device(self.device):
            _capi.check(fn(
                self.B, self.nJ_max, self.nM_max, self.n_max, self.xyz.data_ptr(), *self._members(types),
                self.cbits.data_ptr(), self.loads.data_ptr(),
                self.nJ.data_ptr(), self.nM.data_ptr(), self.free_index.data_ptr(),
                self.n_free.data_ptr(), self.ld, self.rows, self.S.data_ptr(), self.uf.data_ptr(),
                self.rows, self.u.data_ptr(), self.f_ext.data_ptr(), self.N.data_ptr(),
                self.info.data_ptr(), self.work.data_ptr(), self._env_ptr(),
                self.joint_out.data_ptr() if self.joint_out is not None else None,
                self._solve_hints(), self._stream()), what)

    # -- several load cases from one factorisation (include/trs_solver.h "Load cases") ------------------
    def factor(self):
        """dofmap, assembly and Cholesky factorisation of the resident batch, asynchronous on the current stream: the
        factor stays in the slab for any number of `solve_cases` calls (the batch's own `loads` ride along and are not
        needed by them).  A batch on the fused small-system path keeps no factor: build it with `use_small=False`."""
        self._need_slab("factor")
        with self.torch.cuda.device(self.device):
            self.dofmap()
            self.assemble()
            self.potrf()
        self._factored = True
        self._dynamic = None   # (the slab holds a factor of K_ff again: `transient` refuses until `factor_dynamic`)
        self._bump_generation()

    # what the analyses on the resident factor share (solve_cases, solve_effect_cases, adjoint_cases, modes)
    def _need_factor(self, what):
        if not getattr(self, "_factored", False):
            raise ValueError(f"{what}(): no factor - call factor() first")

    def _need_slab(self, what, compact=None):
        """The refusals of a method that keeps or amends a factor in the slab, in `what`'s name: a batch on the fused
        small-system path, and - with `compact`, the method's reason - the compact member form of the assembly."""
        if self.small:
            raise ValueError(f"{what}(): this batch takes the fused small-system kernel, which keeps no factor - "
                             "build the DeviceBatch with use_small=False")
        if compact is not None and self.options["compact"]:
            raise ValueError(f"{what}(): options['compact'] {compact}")

    def _need_fit(self, what, fits, kernel):
        """`fits`: what the `trs_*_fits` call of `what`'s kernel (`kernel`: its phrase) said of this batch's sizes."""
        if not fits:
            raise HipExtensionError(f"{what}(): a truss of {self.nJ_max} joints / {self.nM_max} members exceeds the LDS "
                                    f"of {kernel}")

    def _gather_cases(self, loads, L, into, own=False):
        """`trs_gather_cases`: the L cases `loads` [B, L, nJ_max, 3] reduced into the case block `into`.  `own`: they
        are the batch's own loads, already in the batch's joint order (gathered without `joint_out`)."""
        jo, stream, _ = self._case_launch()
        _capi.check(self.lib.trs_gather_cases(self.B, L, self.nJ_max, loads.data_ptr(), self.free_index.data_ptr(),
                                              self.n_free.data_ptr(), self.nJ.data_ptr(), None if own else jo,
                                              into.data_ptr(), self.rows, stream), "trs_gather_cases")

    def _out_tensors(self, what, shapes, out):
        """The result dict of `what`: exactly the keys of `shapes` (key -> (shape, dtype), as `_field_shapes` makes
        them), taken from `out` where it has them - they must be contiguous device tensors of that shape and type -
        and allocated (into `out` too, if one was given) where it has not."""
        t = self.torch
        out = {} if out is None else out
        for k, (shape, dtype) in shapes.items():
            if k not in out:
                out[k] = t.zeros(shape, dtype=dtype, device=self.device)
            elif list(out[k].shape) != shape or out[k].dtype != dtype or out[k].device != self.device \
                    or not out[k].is_contiguous():
                raise ValueError(f"{what}(): out[{k!r}] must be a contiguous {'float64' if dtype is t.float64 else dtype} "
                                 f"{shape} tensor on {self.device}")
        return {k: out[k] for k in shapes}

    def _case_block(self, attr, L):
        """The buffer `attr` (cases_F, cases_Lam) if it holds L cases, else a new one: right-hand sides and solutions,
        case-major [B][L][ld_f], ld_f = self.rows.  The caller keeps it in `attr`."""
        X = getattr(self, attr, None)
        if X is None or int(X.shape[1]) != L:
            X = self.torch.empty([self.B, L, self.rows], dtype=self.torch.float64, device=self.device)
        return X

    def _check_loads(self, what, loads):
        """`loads` of `what`(), contiguous: a float64 tensor [B, L, nJ_max, 3] on this batch's device, or ValueError."""
        if loads.dim() != 4 or tuple(loads.shape[:1]) + tuple(loads.shape[2:]) != (self.B, self.nJ_max, 3) \
                or loads.dtype != self.torch.float64 or loads.device != self.device:
            raise ValueError(f"{what}(): loads must be float64 [B={self.B}, L, nJ_max={self.nJ_max}, 3] on {self.device}")
        return loads.contiguous()

    def _sizes(self, **sizes):
        """The sizes a `FIELDS` shape may name: this batch's "nJ" and "nM" and the call's own."""
        return dict(sizes, nJ=self.nJ_max, nM=self.nM_max)

    def _case_launch(self):
        """What every launch of these methods is given: joint_out's pointer (or None), the current stream, and the infix
        of the entry points of this batch's member form."""
        return _ptr(self.joint_out), self._stream(), "_tab" if self.table else ""

    def _potrs_cases(self, X, L):
        """L y = f, U x = y for the L columns of X against the resident factor, in place."""
        _capi.check(self.lib.trs_potrs_cases(self.B, L, self.n_free.data_ptr(), self.ld, self.rows, self.S.data_ptr(),
                                             X.data_ptr(), self.rows, self._env_ptr(), self._stream()), "trs_potrs_cases")

    def solve_cases(self, loads, out=None):
        """Gather, multi-case substitution and recovery on the resident factor (`factor()` first).  `loads`: float64
        device tensor [B, L, nJ_max, 3] in the CALLER's joint numbering (a joint order applied to the batch is undone
        on the device).  Returns a dict of device tensors u, f_ext [B, L, nJ_max, 3] and N [B, L, nM_max] (`out`: such
        a dict to write into - its tensors are checked as the other analyses check theirs, and the dict returned holds
        exactly u, f_ext and N, not the caller's dict object); `self.info` holds the factorisation's status per truss."""
        t = self.torch
        self._need_factor("solve_cases")
        loads = self._check_loads("solve_cases", loads)
        L = int(loads.shape[1])
        out = self._out_tensors("solve_cases", _field_shapes(LoadCaseResult.FIELDS, self.B, self._sizes(L=L)), out)
        if self.B == 0 or L == 0:
            return out
        self._need_fit("solve_cases", self.lib.trs_recover_cases_fits(self.nJ_max, self.nM_max),
                       "the multi-case recovery (trs_recover_cases_fits)")
        F = self._case_block("cases_F", L)
        jo, stream, tab = self._case_launch()
        with t.cuda.device(self.device):
            self._gather_cases(loads, L, F)
            self._potrs_cases(F, L)
            _capi.check(getattr(self.lib, f"trs_recover{tab}_cases")(
                self.B, L, self.nJ_max, self.nM_max, self.xyz.data_ptr(), *self._members(), loads.data_ptr(),
                self.free_index.data_ptr(), self.nJ.data_ptr(), self.nM.data_ptr(), F.data_ptr(), self.rows,
                out["u"].data_ptr(), out["f_ext"].data_ptr(), out["N"].data_ptr(), jo, stream), f"trs_recover{tab}_cases")
        self.cases_F = F   # (kept: the reduced displacements of the last call, and the buffer of the next)
        self._bump_generation()
        self._forward = (self.generation, L)   # what `adjoint_cases` may differentiate
        return out

    # -- load cases with settlements, pre-strain and self-weight (include/trs_effects.h) ------------------
    def solve_effect_cases(self, loads=None, prestrain=None, settlement=None, accel=None, want_body=False, out=None):
        """`solve_cases` for cases that carry more than joint forces, on the resident factor (`factor()` first): `loads`
        [B, L, nJ_max, 3] joint forces, `prestrain` [B, L, nM_max] member initial strains (alpha dT, dL / L),
        `settlement` [B, L, nJ_max, 3] prescribed displacements (read at constrained DOFs only) and `accel` [B, L, 3]
        body-force vectors per unit weight (a member loads each end joint with half of a * length * density times it) -
        float64 device tensors, joint arrays in the CALLER's numbering; any may be None, at least one must be given, and
        all agree on L.  The effects change the right-hand side only (`trs_effects_rhs`), the substitution is
        `trs_potrs_cases` as it is, and the recovery (`trs_effects_recover`) gives u with the settlements at the
        supports, N = k c . (u1 - u0) - E A eps0 and f_ext without the self-weight (include/trs_effects.h).  Returns a
        dict of device tensors u, f_ext [B, L, nJ_max, 3], N [B, L, nM_max] and - `want_body` - body [B, L, nJ_max, 3],
        the self-weight load of every joint (`out`: such a dict to write into).  With only `loads` given the results are
        those of `solve_cases(loads)` bit for bit.
        `generation` is bumped and the forward state of `adjoint_cases` is dropped: the equivalent loads depend on A, E
        and xyz, which the adjoint of `solve_cases` does not know, so gradients of these cases are refused."""
        t = self.torch
        self._need_factor("solve_effect_cases")
        given = {"loads": loads, "prestrain": prestrain, "settlement": settlement, "accel": accel}
        tails = {"loads": (self.nJ_max, 3), "prestrain": (self.nM_max,), "settlement": (self.nJ_max, 3), "accel": (3,)}
        names = {"loads": "nJ_max, 3", "prestrain": "nM_max", "settlement": "nJ_max, 3", "accel": "3"}
        L = None
        for name, x in given.items():
            if x is None:
                continue
            shape = tuple(int(v) for v in x.shape)
            if len(shape) != 2 + len(tails[name]) or shape[:1] + shape[2:] != (self.B,) + tails[name] \
                    or x.dtype != t.float64 or x.device != self.device:
                raise ValueError(f"solve_effect_cases(): {name} must be float64 [B={self.B}, L, {names[name]}] "
                                 f"(nJ_max={self.nJ_max}, nM_max={self.nM_max}) on {self.device}")
            if L is not None and shape[1] != L:
                raise ValueError(f"solve_effect_cases(): {name} has L = {shape[1]}, the arguments before it L = {L}")
            L = shape[1]
            given[name] = x.contiguous()
        if L is None:
            raise ValueError("solve_effect_cases(): give at least one of loads, prestrain, settlement, accel")
        keys = ("u", "f_ext", "N") + (("body",) if want_body else ())
        out = self._out_tensors("solve_effect_cases", _field_shapes(EffectCaseResult.FIELDS, self.B, self._sizes(L=L), keys),
                                out)
        if self.B == 0 or L == 0:
            return out
        self._need_fit("solve_effect_cases", self.lib.trs_effects_fits(self.nJ_max, self.nM_max),
                       "the effect kernels (trs_effects_fits)")
        F = self._case_block("cases_F", L)
        jo, stream, tab = self._case_launch()
        members = self._members() if self.table else self._members() + (_ptr(self.rho),)
        effects = tuple(_ptr(given[k]) for k in ("loads", "prestrain", "settlement", "accel"))
        self._forward = None                 # (F is about to be overwritten; see the docstring)
        self._bump_generation()
        with t.cuda.device(self.device):
            _capi.check(getattr(self.lib, f"trs_effects{tab}_rhs")(
                self.B, L, self.nJ_max, self.nM_max, self.xyz.data_ptr(), *members, *effects,
                self.free_index.data_ptr(), self.n_free.data_ptr(), self.nJ.data_ptr(), self.nM.data_ptr(), jo,
                F.data_ptr(), self.rows, stream), f"trs_effects{tab}_rhs")
            self._potrs_cases(F, L)
            _capi.check(getattr(self.lib, f"trs_effects{tab}_recover")(
                self.B, L, self.nJ_max, self.nM_max, self.xyz.data_ptr(), *members, *effects,
                self.free_index.data_ptr(), self.nJ.data_ptr(), self.nM.data_ptr(), F.data_ptr(), self.rows,
                out["u"].data_ptr(), out["f_ext"].data_ptr(), out["N"].data_ptr(), _ptr(out.get("body")), jo, stream),
                f"trs_effects{tab}_recover")
        self.cases_F = F
        return out

    # -- adjoint gradients of the solved cases (include/trs_solver.h "Adjoint gradients") ------------------
    #: the gradients `adjoint_cases` can give, and their shapes' trailing dimensions
    GRADIENTS = ("A", "E", "xyz", "loads")

    @property
    def generation(self):
        """Counts the `factor()`, `factor_dynamic()`, `solve_cases()` (also the one inside `member_loss()`), `solve_effect_cases()` and `modes()` calls of this batch: a forward state is identified by the value
        after its `solve_cases()`, and `adjoint_cases` refuses any other."""
        return getattr(self, "_generation", 0)

    def _bump_generation(self):
        self._generation = self.generation + 1

    def adjoint_cases(self, grad_u=None, grad_f_ext=None, grad_N=None, want=GRADIENTS, out=None, generation=None):
        """The vector-Jacobian product of the last `solve_cases(loads)`: for cotangents `grad_u`, `grad_f_ext`
        [B, L, nJ_max, 3] and `grad_N` [B, L, nM_max] (float64 device tensors in the CALLER's joint numbering, the
        derivative of some scalar J with respect to the results; None = zero) the gradients dJ/dA, dJ/dE [B, nM_max],
        dJ/dxyz [B, nJ_max, 3] (summed over the L cases) and dJ/dloads [B, L, nJ_max, 3], as a dict of device tensors
        with the keys named in `want` (`out`: such a dict to write into).  Three launches on the current stream,
        asynchronous: the reduced right-hand sides, one substitution against the resident factor (no factorisation;
        the forward solutions in `cases_F` are only read), and the contraction with the forward field.  In the table
        member form dA / dE are per member too.
        The forward state must be current: `factor()` and `solve_cases()` bump `generation`, and a gradient of anything
        but the last `solve_cases()` of the last `factor()` raises ValueError (`generation`: the value the caller saw
        after ITS `solve_cases()`, checked as well)."""
        t = self.torch
        forward = getattr(self, "_forward", None)
        if not getattr(self, "_factored", False) or forward is None:
            raise ValueError("adjoint_cases(): no forward solution - call factor() and solve_cases(loads) first")
        if forward[0] != self.generation or (generation is not None and generation != self.generation):
            raise ValueError("adjoint_cases(): the forward solution is stale - factor() or solve_cases() ran since "
                             "the solve these gradients belong to")
        L = forward[1]
        want = tuple(want)
        if any(k not in self.GRADIENTS for k in want):
            raise ValueError(f"adjoint_cases(): want must name some of {self.GRADIENTS}, got {want}")
        shapes = {"grad_u": (self.B, L, self.nJ_max, 3), "grad_f_ext": (self.B, L, self.nJ_max, 3),
                  "grad_N": (self.B, L, self.nM_max)}
        cot = {"grad_u": grad_u, "grad_f_ext": grad_f_ext, "grad_N": grad_N}
        for name, g in cot.items():
            if g is None:
                continue
            if tuple(g.shape) != shapes[name] or g.dtype != t.float64 or g.device != self.device:
                raise ValueError(f"adjoint_cases(): {name} must be float64 {list(shapes[name])} on {self.device} "
                                 f"(the last solve_cases() had L = {L}), got {g.dtype} {list(g.shape)} on {g.device}")
            cot[name] = g.contiguous()
        out = self._out_tensors("adjoint_cases", _field_shapes(GradientResult.FIELDS, self.B, self._sizes(L=L), want), out)
        if self.B == 0 or L == 0:
            return out
        self._need_fit("adjoint_cases", self.lib.trs_adjoint_fits(self.nJ_max, self.nM_max),
                       "the adjoint kernels (trs_adjoint_fits)")
        Lam = self._case_block("cases_Lam", L)   # the adjoint systems: a buffer of their own, the forward F survives
        jo, stream, tab = self._case_launch()
        with t.cuda.device(self.device):
            _capi.check(getattr(self.lib, f"trs_adjoint{tab}_rhs")(
                self.B, L, self.nJ_max, self.nM_max, self.xyz.data_ptr(), *self._members(), _ptr(cot["grad_u"]),
                _ptr(cot["grad_f_ext"]), _ptr(cot["grad_N"]), self.free_index.data_ptr(), self.n_free.data_ptr(),
                self.nJ.data_ptr(), self.nM.data_ptr(), jo, Lam.data_ptr(), self.rows, stream), f"trs_adjoint{tab}_rhs")
            self._potrs_cases(Lam, L)
            _capi.check(getattr(self.lib, f"trs_adjoint{tab}_grad")(
                self.B, L, self.nJ_max, self.nM_max, self.xyz.data_ptr(), *self._members(), _ptr(cot["grad_f_ext"]),
                _ptr(cot["grad_N"]), self.free_index.data_ptr(), self.nJ.data_ptr(), self.nM.data_ptr(),
                self.cases_F.data_ptr(), Lam.data_ptr(), self.rows, _ptr(out.get("A")), _ptr(out.get("E")),
                _ptr(out.get("xyz")), _ptr(out.get("loads")), jo, stream), f"trs_adjoint{tab}_grad")
        self.cases_Lam = Lam
        return out

    # -- the analyses on the columns z_e = inv(K_ff) b_e,f: member_loss, member_sets, influence ------------------
    def _check_columns(self, what, chunk, r_tol=None):
        """The `chunk` (and `r_tol`) errors of a column analysis, under the calling method's name."""
        if r_tol is not None and not 0.0 < float(r_tol) < 1.0:
            raise ValueError(f"{what}(): r_tol must lie in (0, 1), got {r_tol!r}")
        if int(chunk) < 1:
            raise ValueError(f"{what}(): chunk must be at least 1, got {chunk!r}")

    def _columns(self, C, ranges, cols=None):
        """The loop of the column analyses, as a generator.  For every range of `ranges` the rows b_e,f of up to C members
        go into Z [B, C, rows] - the members range .. range + C - 1 (`trs_loss_rhs`), or with `cols` those that the device
        id list `cols(range)` [B, C] names (`trs_sets_rhs`) -, one `trs_potrs_cases` turns them into the columns
        z_e = inv(K_ff) b_e,f, and (Z, range) is yielded to the analysis's own kernel.  The caller iterates with this batch's
        device current (`torch.cuda.device`): the launches here run inside its loop."""
        t = self.torch
        # the range's columns: B * C * rows doubles (1.5 GB for bar-942 x 4096 at chunk 64) beside the slab, not counted
        # in `max_slab_bytes`, and released when the analysis returns
        Z = t.empty([self.B, C, self.rows], dtype=t.float64, device=self.device)
        stream, tab = self._case_launch()[1:]
        for rng in ranges:
            if cols is None:
                name, first, last = f"trs_loss{tab}_rhs", (rng, C), ()
            else:
                name, first, last = f"trs_sets{tab}_rhs", (C,), (cols(rng).data_ptr(),)
            _capi.check(getattr(self.lib, name)(
                self.B, *first, self.nJ_max, self.nM_max, self.xyz.data_ptr(), *self._members(), self.free_index.data_ptr(),
                self.n_free.data_ptr(), self.nM.data_ptr(), *last, Z.data_ptr(), self.rows, stream), name)
            self._potrs_cases(Z, C)
            yield Z, rng

    # -- member-loss analysis: every single-member removal from the resident factor (include/trs_loss.h) ------------------
    def member_loss(self, loads, r_tol=MEMBER_LOSS_R_TOL, want_forces=False, chunk=64, out=None,
                    max_result_bytes=4 << 30):
        """What the loss of any ONE member does to every truss, for every member, on the resident factor (`factor()`
        first): a removal is a rank-one change of K_ff, so per member one substitution column against the factor and
        one pass of `trs_loss_apply` replace a factorisation (include/trs_loss.h).  `loads`: float64 device tensor
        [B, L, nJ_max, 3] in the CALLER's joint numbering, as `solve_cases` takes it.  The intact state comes from
        `solve_cases(loads)`; then the members are taken `chunk` at a time (rounded up to a multiple of 16, one case
        group of the substitution): `trs_loss_rhs`, `trs_potrs_cases`, `trs_loss_apply`, on a buffer [B, chunk, rows] of
        this method's own (allocated per call, beside the slab) - `cases_F` keeps the intact displacements.  Returns a dict of device tensors: u, f_ext
        [B, L, nJ_max, 3] and N [B, L, nM_max] of the intact truss, r [B, nM_max] (the redundancy 1 - k_e b_e . z_e; the
        r of a truss sum to nM - n_free), critical [B, nM_max] (int32: r <= `r_tol`, the truss is a mechanism without
        that member), peak_stress, peak_displace [B, L, nM_max] (max |N'| / A over the surviving members, max |u'| over
        the joints; +inf for a critical member) with peak_member, peak_joint (int32; caller's joint numbering, the
        lowest id on a tie, -1 where there is none) and - `want_forces` - N_after [B, L, nM_max, nM_max], row e the
        member forces without member e (NaN for a critical member); refused with ValueError when it would exceed
        `max_result_bytes`.  `out`: such a dict to write into.  `generation` is bumped by the `solve_cases` inside and
        the forward state is that call's: `adjoint_cases` differentiates the intact state afterwards."""
        self._need_factor("member_loss")
        loads = self._check_loads("member_loss", loads)
        self._check_columns("member_loss", chunk, r_tol)
        B, L, nJ_max, nM_max = self.B, int(loads.shape[1]), self.nJ_max, self.nM_max
        if want_forces and B * L * nM_max * nM_max * 8 > max_result_bytes:
            raise ValueError(f"member_loss(): N_after [B={B}, L={L}, {nM_max}, {nM_max}] takes {B * L * nM_max * nM_max * 8} "
                             f"bytes, more than max_result_bytes = {max_result_bytes}")
        keys = [k for k, *_ in MemberLossResult.FIELDS.values() if k != "N_after" or want_forces]
        out = self._out_tensors("member_loss", _field_shapes(MemberLossResult.FIELDS, B, self._sizes(L=L), keys), out)
        self._need_fit("member_loss", not (B and L) or self.lib.trs_loss_fits(nJ_max, nM_max, L),
                       "the apply kernel (trs_loss_fits)")
        self.solve_cases(loads, out={k: out[k] for k in ("u", "f_ext", "N")})
        if B == 0 or L == 0 or nM_max == 0:
            return out
        C = _chunk_columns(chunk, nM_max)
        jo, stream, tab = self._case_launch()
        results = [out[k].data_ptr() for k in ("r", "critical", "peak_stress", "peak_member", "peak_displace", "peak_joint")]
        with self.torch.cuda.device(self.device):
            for Z, e0 in self._columns(C, range(0, nM_max, C)):
                _capi.check(getattr(self.lib, f"trs_loss{tab}_apply")(
                    B, L, e0, C, nJ_max, nM_max, self.xyz.data_ptr(), *self._members(), self.free_index.data_ptr(),
                    self.nJ.data_ptr(), self.nM.data_ptr(), Z.data_ptr(), self.cases_F.data_ptr(), self.rows, float(r_tol),
                    *results, _ptr(out.get("N_after")), jo, stream), f"trs_loss{tab}_apply")
        return out

    # -- member-set scenarios: up to eight members removed or resized at once (include/trs_sets.h) ------------------
    def member_sets(self, loads, sets, gamma=None, r_tol=MEMBER_LOSS_R_TOL, want_forces=False, want_displace=False,
                    chunk=64, out=None, max_result_bytes=4 << 30):
        """What removing, damaging or strengthening up to eight members AT ONCE does to every truss, for S scenarios per
        truss, on the resident factor (`factor()` first): a scenario changes K_ff by a term of rank k <= 8, so one
        substitution column per DISTINCT member of a range of scenarios and one k x k elimination per scenario replace a
        factorisation per scenario (include/trs_sets.h).  `loads`: float64 device tensor [B, L, nJ_max, 3] in the
        CALLER's joint numbering, as `solve_cases` takes it.  `sets`: HOST integer array [B, S, K <= 8] of member ids,
        -1 padding at the end of a set (an empty set gives the intact state), or the nested lists `solve_member_sets`
        takes; `gamma`: HOST array of the same shape, the area factor of every named member (0 removed, below 1
        damaged, above 1 strengthened, 1 unchanged), or None - every member removed.  They are host arrays because the
        plan is made on the host (`plan_member_sets`): the scenario axis is cut into ranges whose distinct members per
        truss fit `chunk` columns (rounded up to a multiple of 16, one case group of the substitution), and per range
        `trs_sets_rhs`, `trs_potrs_cases` and `trs_sets_apply` run on a buffer [B, chunk, rows] of this method's own
        (allocated per call, beside the slab).  The intact state comes from `solve_cases(loads)`.  Returns a dict of
        device tensors: u, f_ext [B, L, nJ_max, 3] and N [B, L, nM_max] of the intact truss; pivot [B, S, 8] (the pivots
        of the elimination in the set's order - for removals the redundancy of member j once the members before it are
        gone; NaN beyond the set and after a failing position), unstable, first_unstable [B, S] (int32: some pivot
        <= `r_tol` - the truss is a mechanism from that member of the set on - and its position, else -1); peak_stress,
        peak_displace [B, L, S] (max |N'| / (gamma A) over the members that are not removed, max |u'| over the joints;
        +inf for an unstable scenario) with peak_member, peak_joint (int32; caller's joint numbering, the lowest id on
        a tie, -1 where there is none) and - `want_forces`, `want_displace` - N_after [B, L, S, nM_max] and u_after
        [B, L, S, nJ_max, 3] (caller's joint numbering; NaN for an unstable scenario), together refused with ValueError
        above `max_result_bytes`.  `out`: such a dict to write into.  `generation` is bumped by the `solve_cases`
        inside and the forward state is that call's, exactly as after `member_loss`."""
        self._need_factor("member_sets")
        loads = self._check_loads("member_sets", loads)
        self._check_columns("member_sets", chunk, r_tol)
        B, L, nJ_max, nM_max = self.B, int(loads.shape[1]), self.nJ_max, self.nM_max
        sets, gamma = _member_set_arrays("member_sets()", sets, gamma, B, None, nM_max)
        S = int(sets.shape[1])
        extra = 8 * B * L * S * (nM_max * bool(want_forces) + 3 * nJ_max * bool(want_displace))
        if extra > max_result_bytes:
            raise ValueError(f"member_sets(): N_after / u_after of [B={B}, L={L}, S={S}] scenarios take {extra} bytes, "
                             f"more than max_result_bytes = {max_result_bytes}")
        keys = [k for k, *_ in MemberSetResult.FIELDS.values()
                if (k != "N_after" or want_forces) and (k != "u_after" or want_displace)]
        out = self._out_tensors("member_sets", _field_shapes(MemberSetResult.FIELDS, B, self._sizes(L=L, S=S), keys), out)
        self._need_fit("member_sets", not (B and L) or self.lib.trs_sets_fits(nJ_max, nM_max, L),
                       "the apply kernel (trs_sets_fits)")
        self.solve_cases(loads, out={k: out[k] for k in ("u", "f_ext", "N")})
        if B == 0 or L == 0 or S == 0:
            return out
        plan = plan_member_sets(sets, chunk, nM_max)
        C = int(plan[0][2].shape[1])
        jo, stream, tab = self._case_launch()
        results = [out[k].data_ptr() for k in ("pivot", "unstable", "first_unstable", "peak_stress", "peak_member",
                                               "peak_displace", "peak_joint")]
        up = lambda a: None if a is None else self.torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        uploaded = ((s0, s1, up(cols), up(slot), up(None if gamma is None else gamma[:, s0:s1]))
                    for s0, s1, cols, slot in plan)   # (a generator: one range at a time, as the loop comes to it)
        with self.torch.cuda.device(self.device):
            for Z, (s0, s1, cols, slot, factors) in self._columns(C, uploaded, cols=lambda rng: rng[2]):
                _capi.check(getattr(self.lib, f"trs_sets{tab}_apply")(
                    B, L, S, s0, s1 - s0, C, nJ_max, nM_max, self.xyz.data_ptr(), *self._members(),
                    self.free_index.data_ptr(), self.nJ.data_ptr(), self.nM.data_ptr(), cols.data_ptr(), slot.data_ptr(),
                    _ptr(factors), Z.data_ptr(), self.cases_F.data_ptr(), self.rows, float(r_tol), *results,
                    _ptr(out.get("N_after")), _ptr(out.get("u_after")), jo, stream), f"trs_sets{tab}_apply")
        return out

    # -- influence lines and moving-load envelopes from the resident factor (include/trs_influence.h) ------------------
    def influence(self, path, path_len, direction, train_w, train_o, want_lines=False, chunk=64, out=None):
        """The influence lines of every member force along a path of joints, and the envelope of a load train that
        crosses it, on the resident factor (`factor()` first): k_m inv(K_ff) b_m,f - the column the member-loss analysis
        forms - is the influence line of N_m for a unit load at every joint at once (include/trs_influence.h).  `path`:
        int32 device tensor [B, P_max] of joint ids in the CALLER's numbering, `path_len` int32 [B] (entries of `path`
        at or beyond it are ignored), `direction` float64 [B, 3] (the load vector per unit axle weight), `train_w`,
        `train_o` float64 [A] (axle weights, and offsets behind the lead axle ascending from 0) - the caller validates
        them (`solve_influence` does).  The members are taken `chunk` at a time (rounded up to a multiple of 16, one case
        group of the substitution): `trs_loss_rhs`, `trs_potrs_cases`, `trs_influence_apply`, on a buffer
        [B, chunk, rows] of this method's own (allocated per call, beside the slab).  Returns a dict of device tensors
        [B, nM_max]: N_max, N_min (the extremes of the train's response), x_max, x_min (the lead axle's arc positions
        that attain them; NaN for a padding member or an empty path), area_pos, area_neg (the integrals of the positive
        and the negative part of the line) and - `want_lines` - eta [B, nM_max, P_max], the ordinates at the path joints.
        `out`: such a dict to write into.  Nothing else of the batch changes: `cases_F`, `generation` and the forward
        state that `adjoint_cases` differentiates stay as they are."""
        t = self.torch
        self._need_factor("influence")
        B, nJ_max, nM_max = self.B, self.nJ_max, self.nM_max

        def need(x, name, shape, dtype):
            if x.dim() != len(shape) or any(s is not None and int(x.shape[i]) != s for i, s in enumerate(shape)) \
                    or x.dtype != dtype or x.device != self.device:
                raise ValueError(f"influence(): {name} must be {dtype} {['any' if s is None else s for s in shape]} "
                                 f"on {self.device}")
            return x.contiguous()

        path = need(path, "path", [B, None], t.int32)
        path_len = need(path_len, "path_len", [B], t.int32)
        direction = need(direction, "direction", [B, 3], t.float64)
        train_w = need(train_w, "train_w", [None], t.float64)
        train_o = need(train_o, "train_o", [int(train_w.shape[0])], t.float64)
        P_max, A = int(path.shape[1]), int(train_w.shape[0])
        if A < 1:
            raise ValueError("influence(): the train has no axle")
        self._check_columns("influence", chunk)
        keys = [k for k, *_ in InfluenceResult.FIELDS.values() if k != "eta" or want_lines]
        out = self._out_tensors("influence", _field_shapes(InfluenceResult.FIELDS, B, self._sizes(P=P_max), keys), out)
        if not self.lib.trs_influence_fits(nJ_max, P_max, A):
            raise HipExtensionError(f"influence(): a path of {P_max} joints with {A} axles on a truss of {nJ_max} joints "
                                    "exceeds the LDS of the apply kernel (trs_influence_fits)")
        if B == 0 or nM_max == 0:
            return out
        C = _chunk_columns(chunk, nM_max)
        jo, stream, tab = self._case_launch()
        results = [out[k].data_ptr() for k in ("N_max", "N_min", "x_max", "x_min", "area_pos", "area_neg")]
        with self.torch.cuda.device(self.device):
            for Z, e0 in self._columns(C, range(0, nM_max, C)):
                _capi.check(getattr(self.lib, f"trs_influence{tab}_apply")(
                    B, e0, C, nJ_max, nM_max, P_max, A, self.xyz.data_ptr(), *self._members(), self.free_index.data_ptr(),
                    self.nJ.data_ptr(), self.nM.data_ptr(), path.data_ptr(), path_len.data_ptr(), direction.data_ptr(),
                    train_w.data_ptr(), train_o.data_ptr(), Z.data_ptr(), self.rows, _ptr(out.get("eta")), *results, jo,
                    stream), f"trs_influence{tab}_apply")
        return out

    # -- natural frequencies and mode shapes from the resident factor (include/trs_modes.h) ------------------
    def modes(self, p, tol=1e-10, max_iters=256, check_every=8, joint_mass=None, mass_scale=1.0, out=None):
        """The `p` lowest pairs of K_ff phi = lambda M phi of every truss (M: lumped mass, include/trs_modes.h) by block
        inverse iteration against the resident factor (`factor()` first): per iteration one `trs_potrs_cases` launch
        on a block of 16 vectors and one `trs_modes_step` launch; every `check_every` iterations the residuals are
        formed, the trusses whose first n_modes pairs are below `tol` freeze, and ONE small read-back (is any truss still
        iterating?) decides whether to go on, up to `max_iters`.  `joint_mass`: float64 device tensor [B, nJ_max] in the
        CALLER's joint numbering (non-structural mass), or None; `mass_scale` multiplies the members' mass.
        Returns a dict of device tensors lam [B, p] (NaN beyond n_modes), phi [B, p, nJ_max, 3] (caller's numbering,
        M-orthonormal, largest component positive), resid [B, p], n_modes [B] = min(p, DOFs with mass) and iters [B]
        (0: not converged within `max_iters` - the last iterate and its residual are returned all the same).
        The block shares the buffer of `solve_cases`' right-hand sides, so a forward solution kept for
        `adjoint_cases` is invalidated (`generation` is bumped); the factor is only read."""
        t = self.torch
        self._need_factor("modes")
        _check_mode_args(self.B, self.nJ_max, p, None if joint_mass is None else tuple(joint_mass.shape), mass_scale, tol,
                         max_iters, check_every)
        p, max_iters, check_every = int(p), int(max_iters), int(check_every)
        if joint_mass is not None:
            if joint_mass.dtype != t.float64 or joint_mass.device != self.device:
                raise ValueError(f"modes(): joint_mass must be float64 [B={self.B}, nJ_max={self.nJ_max}] on {self.device}")
            joint_mass = joint_mass.contiguous()
        keys = ("lam", "phi", "resid", "n_modes", "iters")   # (no "omega": `ModeResult.FIELDS`)
        out = self._out_tensors("modes", _field_shapes(ModeResult.FIELDS, self.B, self._sizes(P=p), keys), out)
        if self.B == 0:
            return out
        self._need_fit("modes", self.lib.trs_modes_fits(self.nJ_max, self.nM_max), "the mass kernel (trs_modes_fits)")
        Q = MODES_BLOCK
        F = self.cases_F = self._case_block("cases_F", Q)   # the block's right-hand sides / solutions
        self._bump_generation()              # (whatever `solve_cases` left there is gone: `adjoint_cases` refuses it)
        ws = getattr(self, "_modes_ws", None)
        if ws is None:
            f64 = lambda *shape: t.empty(list(shape), dtype=t.float64, device=self.device)
            i32 = lambda *shape: t.empty(list(shape), dtype=t.int32, device=self.device)
            ws = self._modes_ws = {"X": f64(self.B, Q, self.rows), "Mf": f64(self.B, self.rows), "lam": f64(self.B, Q),
                                   "resid": f64(self.B, Q), "n_mass": i32(self.B), "state": i32(self.B)}
        jo, stream, tab = self._case_launch()

        def step(first, check, it):
            _capi.check(self.lib.trs_modes_step(
                self.B, p, self.n_free.data_ptr(), ws["n_mass"].data_ptr(), ws["Mf"].data_ptr(), F.data_ptr(),
                ws["X"].data_ptr(), self.rows, ws["lam"].data_ptr(), ws["resid"].data_ptr(), ws["state"].data_ptr(),
                first, check, it, float(tol), stream), "trs_modes_step")

        with t.cuda.device(self.device):
            self._lumped_mass(joint_mass, mass_scale, into=(ws["Mf"], ws["n_mass"]))
            self._block_iteration(F, step, ws["state"], max_iters, check_every)
            _capi.check(self.lib.trs_modes_shapes(self.B, p, self.nJ_max, ws["X"].data_ptr(), self.rows,
                                                  self.free_index.data_ptr(), self.nJ.data_ptr(), jo,
                                                  out["phi"].data_ptr(), stream), "trs_modes_shapes")
        out["lam"].copy_(ws["lam"][:, :p])
        out["resid"].copy_(ws["resid"][:, :p])
        out["n_modes"].copy_(ws["n_mass"].clamp(max=p))
        out["iters"].copy_(ws["state"])
        # what `mode_gradients` differentiates: the block stays in the workspace until the generation moves on
        self._modes_state = {"p": p, "mass_scale": float(mass_scale), "joint_mass": joint_mass,
                             "generation": self.generation}
        return out

    # -- what the analyses on the converged block share (mode_gradients, response_spectrum, harmonic) ------------------
    def _current_modes(self, who, generation):
        """The state that `modes()` left, if it is current; else ValueError (`mode_gradients` speaks of its forward
        solution, the others of the modes)."""
        what, stale, whose = ("forward solution", "is stale", "these gradients belong") if who == "mode_gradients" else \
            ("modes", "are stale", "this analysis belongs")
        state = getattr(self, "_modes_state", None)
        if not getattr(self, "_factored", False) or state is None:
            raise ValueError(f"{who}(): no {what} - call factor() and modes(p) first")
        if state["generation"] != self.generation or (generation is not None and generation != self.generation):
            raise ValueError(f"{who}(): the {what} {stale} - factor(), solve_cases() or another analysis ran since the "
                             f"modes() {whose} to")
        return state

    def _to_device(self, x):
        """A host array as a contiguous float64 tensor on the batch's device."""
        return self.torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(self.device)

    def _residual_block(self, on, modal):
        """`modal(F)` launches a modal kernel, which with the correction `on` leaves right-hand sides in the case block
        F (else None); `trs_potrs_cases` then solves them in place.  Returns F for the second kernel."""
        F = None
        if on:
            F = self.cases_F = self._case_block("cases_F", MODES_BLOCK)
        modal(F)
        if on:
            self._potrs_cases(F, MODES_BLOCK)
        return F

    # -- gradients of the eigenvalues from the converged block (include/trs_modegrad.h) ------------------
    #: the gradients `mode_gradients` can give
    MODE_GRADIENTS = ("A", "E", "rho", "xyz", "joint_mass")

    def mode_gradients(self, weights=None, want=None, out=None, generation=None):
        """The derivatives of the eigenvalues of the last `modes()` with respect to the member areas, moduli and
        densities [B, R, nM_max], the joint coordinates [B, R, nJ_max, 3] (every joint, held ones included; z = 0 for a
        2D truss) and the caller's `joint_mass` [B, R, nJ_max] (caller's joint numbering), as a dict of device tensors
        with the keys named in `want` plus `gap` (`want` None: all of `MODE_GRADIENTS`, "joint_mass" only when `modes()`
        was given masses - asked for by name without them it is refused; `out`: such a dict to write into).  `weights` None: R = p, row k is
        the gradient of lambda_k; `weights` [B, p] (float64 device tensor): R = 1, the row is sum_k w_k d lambda_k
        (a weight beyond the truss's n_modes is ignored, whatever it holds).  One launch on the current stream
        (`trs_mg_grad`: one pass over the members with the block X that `modes()` left resident - no solve, no
        factorisation); rows beyond n_modes, padding members and joints and members of zero length get zeros.
        d omega = d lambda / (2 omega).
        `gap` [B, p]: min over the other Ritz values of the block (i < min(16, DOFs with mass), i != k) of
        |lam_i - lam_k| / |lam_k|, +inf where there is no other, NaN beyond n_modes.  The formula holds for a SIMPLE
        eigenvalue: a row of a repeated one (gap of the order of the residual - symmetric trusses have them) is the
        formula on whichever vector of the invariant subspace came out and means nothing alone, while equal weights
        over a closed cluster always give the derivative of the cluster's sum.
        The `modes()` state must be current: any call that bumps `generation` since (`factor()`, `solve_cases()`, a later
        `modes()`, `buckling()`, ...) makes this raise ValueError (`generation`: the value the caller saw after ITS
        `modes()`, checked as well).  Nothing is bumped or overwritten here: the call can be repeated."""
        t = self.torch
        state = self._current_modes("mode_gradients", generation)
        p = state["p"]
        if want is None:
            want = tuple(k for k in self.MODE_GRADIENTS if k != "joint_mass" or state["joint_mass"] is not None)
        want = tuple(want)
        if any(k not in self.MODE_GRADIENTS for k in want):
            raise ValueError(f"mode_gradients(): want must name some of {self.MODE_GRADIENTS}, got {want}")
        if "joint_mass" in want and state["joint_mass"] is None:
            raise ValueError("mode_gradients(): 'joint_mass' is wanted, but modes() was given no joint_mass")
        if weights is not None:
            if tuple(weights.shape) != (self.B, p) or weights.dtype != t.float64 or weights.device != self.device:
                raise ValueError(f"mode_gradients(): weights must be float64 [B={self.B}, p={p}] on {self.device} (the "
                                 f"last modes() had p = {p}), got {weights.dtype} {list(weights.shape)} on "
                                 f"{weights.device}")
            weights = weights.contiguous()
        R = p if weights is None else 1
        out = self._out_tensors("mode_gradients", _field_shapes(ModeGradientResult.FIELDS, self.B, self._sizes(P=p, R=R),
                                                                want + ("gap",)), out)
        if self.B == 0:
            return out
        self._need_fit("mode_gradients", self.lib.trs_mg_fits(self.nJ_max, self.nM_max, p),
                       "the gradient kernel (trs_mg_fits)")
        ws = self._modes_ws
        jo, stream, tab = self._case_launch()
        members = self._members() if self.table else \
            (self.conn.data_ptr(), self.E.data_ptr(), self.A.data_ptr(), self.rho.data_ptr())
        with t.cuda.device(self.device):
            _capi.check(getattr(self.lib, f"trs_mg{tab}_grad")(
                self.B, self.nJ_max, self.nM_max, self.xyz.data_ptr(), *members, self.free_index.data_ptr(),
                self.n_free.data_ptr(), self.nJ.data_ptr(), self.nM.data_ptr(), jo, ws["X"].data_ptr(), self.rows,
                ws["lam"].data_ptr(), ws["n_mass"].data_ptr(), p, state["mass_scale"], _ptr(weights), _ptr(out.get("A")),
                _ptr(out.get("E")), _ptr(out.get("rho")), _ptr(out.get("xyz")), _ptr(out.get("joint_mass")), stream),
                f"trs_mg{tab}_grad")
            # the gaps, from the block's 16 Ritz values
            lam = ws["lam"]
            other = t.arange(MODES_BLOCK, device=self.device)
            valid = other[None, None, :] < ws["n_mass"].clamp(max=MODES_BLOCK)[:, None, None]
            valid = valid & (other[None, None, :] != other[None, :p, None])
            mine = lam[:, :p, None]
            dist = (lam[:, None, :] - mine).abs() / mine.abs()
            gap = t.where(valid, dist, t.full_like(dist, float("inf"))).amin(dim=2)
            out["gap"].copy_(t.where(mine[:, :, 0].isnan(), mine[:, :, 0], gap))
        return out

    # -- response spectrum analysis from the converged block (include/trs_spectrum.h) ------------------
    #: the combined results `response_spectrum` can give, and where their axes lie after [B, G]
    SPECTRUM_RESULTS = ("u", "N", "R")

    def response_spectrum(self, directions, periods, accel, damping=0.05, rule="cqc", missing_mass=True, zpa=None,
                          want=SPECTRUM_RESULTS, want_modal=False, out=None, generation=None):
        """The seismic response spectrum analysis of every truss with the modes of the last `modes()`: participation
        factors and effective modal masses per ground direction, the spectral ordinate of every mode, and the peak
        displacements `u` [B, G, nJ_max, 3], member forces `N` [B, G, nM_max] and support reactions `R`
        [B, G, nJ_max, 3] combined over the modes by `rule` ("srss", "cqc" - Der Kiureghian, needs `damping` > 0 -
        or "abs"), include/trs_spectrum.h.  Shared by the batch (numpy, torch or lists): `directions` [G, 3] (or
        [G, 2]; 1 <= G <= 3, the length is a scale), the spectrum table `periods` [K] (strictly ascending, >= 0,
        2 <= K <= 64) and `accel` [G, K] (pseudo-accelerations, >= 0; linear between the points, constant outside
        them), `zpa` [G] (the zero-period acceleration of the missing-mass correction; None: accel[:, 0]).
        `missing_mass`: the mass the truncated modes leave out responds statically - one more substitution against
        the resident factor (`trs_potrs_cases`), one more response vector per direction in slot p, uncorrelated with
        the modes.  Returns a dict of device tensors: gamma, sa, meff [B, G, p] (zeros beyond n_modes), mtot, base
        [B, G] (the mass that takes part and the combined base shear), n_modes [B], the results named in `want` (caller's
        joint numbering; u zero at held DOFs, R zero at free ones) and, with `want_modal`, their signed modal values
        modal_u, modal_R [B, G, p + 1, nJ_max, 3], modal_N [B, G, p + 1, nM_max] (slot p: the missing mass, zeros
        without it).  `out`: such a dict to write into.
        Guarded by `_current_modes`: the `modes()` state must be current (ValueError when `factor()`,
        `solve_cases()`, ... ran since; `generation`: the value the caller saw after ITS `modes()`, checked as well).
        Nothing is bumped here: `modes()` already invalidated what `adjoint_cases` differentiates, the case block is
        only scratch, and X, lam and n_mass are only read - `mode_gradients` works afterwards with the same bits, and
        the call can be repeated."""
        t = self.torch
        p = self._current_modes("response_spectrum", generation)["p"]
        dirs, T, Sa, zpa, code, want = _check_spectrum_args(p, directions, periods, accel, damping, rule, zpa, want)
        G, K = int(Sa.shape[0]), int(Sa.shape[1])
        if self.B and not self.lib.trs_rs_fits(self.nJ_max, self.nM_max, p):     # (before any output is allocated)
            raise HipExtensionError(f"response_spectrum(): the response vectors of a truss of {self.nJ_max} joints / "
                                    f"{self.nM_max} members exceed the LDS of the combine kernel (trs_rs_fits)")
        keys = ("gamma", "sa", "meff", "mtot", "base", "n_modes") + \
            tuple(pre + k for k in want for pre in (("", "modal_") if want_modal else ("",)))
        out = self._out_tensors("response_spectrum", _field_shapes(SpectrumResult.FIELDS, self.B,
                                                                   self._sizes(P=p, G=G, V=p + 1), keys), out)
        if self.B == 0:
            return out
        ws = self._modes_ws
        sc = getattr(self, "_rs_ws", None)
        if sc is None or tuple(sc["q"].shape) != (self.B, G, p):
            sc = self._rs_ws = {"q": t.empty([self.B, G, p], dtype=t.float64, device=self.device),
                                "rho": t.empty([self.B, 8, 8], dtype=t.float64, device=self.device)}
        jo, stream, tab = self._case_launch()
        with t.cuda.device(self.device):
            dirs_d, T_d, Sa_d, zpa_d = (self._to_device(x) for x in (dirs, T, Sa, zpa))
            F = self._residual_block(missing_mass, lambda F: _capi.check(self.lib.trs_rs_modal(
                self.B, self.nJ_max, self.free_index.data_ptr(), self.n_free.data_ptr(), self.nJ.data_ptr(),
                ws["X"].data_ptr(), self.rows, ws["lam"].data_ptr(), ws["Mf"].data_ptr(), ws["n_mass"].data_ptr(), p, G,
                dirs_d.data_ptr(), K, T_d.data_ptr(), Sa_d.data_ptr(), zpa_d.data_ptr(), float(damping), code,
                int(bool(missing_mass)), out["gamma"].data_ptr(), out["sa"].data_ptr(), out["meff"].data_ptr(),
                out["mtot"].data_ptr(), out["base"].data_ptr(), sc["q"].data_ptr(), sc["rho"].data_ptr(), _ptr(F), stream),
                "trs_rs_modal"))
            if want:
                modal = lambda k: _ptr(out.get("modal_" + k))
                _capi.check(getattr(self.lib, f"trs_rs_combine{tab}")(
                    self.B, self.nJ_max, self.nM_max, self.xyz.data_ptr(), *self._members(), self.free_index.data_ptr(),
                    self.n_free.data_ptr(), self.nJ.data_ptr(), self.nM.data_ptr(), jo, ws["X"].data_ptr(), self.rows,
                    ws["n_mass"].data_ptr(), p, G, sc["q"].data_ptr(), sc["rho"].data_ptr(), code, int(bool(missing_mass)),
                    _ptr(F), _ptr(out.get("u")), _ptr(out.get("R")), _ptr(out.get("N")), modal("u"), modal("R"),
                    modal("N"), stream), f"trs_rs_combine{tab}")
            out["n_modes"].copy_(ws["n_mass"].clamp(max=p))
        return out

    # -- harmonic response over a frequency sweep from the converged block (include/trs_harmonic.h) -----
    #: the envelopes `harmonic` can give, and where their axes lie after [B, L]
    HARMONIC_RESULTS = ("u", "N", "R")

    def harmonic(self, omegas, pattern=None, accel=None, damping=0.02, damp_mass=0.0, damp_stiff=0.0, residual=True,
                 monitor_joints=None, monitor_members=None, want=HARMONIC_RESULTS, out=None, generation=None,
                 max_result_bytes=4 << 30):
        """The steady-state response of every truss to L harmonic excitations Re(f_l e^(i W t)) over the circular
        forcing frequencies `omegas` [S] (>= 0, finite, any order; shared by the batch), by superposition of the modes
        of the last `modes()`, include/trs_harmonic.h.  f_l = P_l - M iota(ag_l): `pattern` a float64 device tensor
        [B, L, nJ_max, 3], the load patterns in the CALLER's joint numbering (reduced once by `trs_gather_cases`), and /
        or `accel` [L, 3] or [B, L, 3], ground-acceleration amplitudes (the results are then relative to the ground);
        1 <= L <= 16.  Damping per mode: zeta_k = `damping` + `damp_mass` / (2 w_k) + `damp_stiff` w_k / 2 (a modal
        ratio and Rayleigh's two constants of `factor_dynamic`; all >= 0, at least one > 0).  `residual`: the truncated
        modes respond STATICALLY (residual flexibility: one more substitution against the resident factor) - their
        damping and inertia are ignored, so the answer is the standard mode-acceleration one, good for W well below the
        frequency of the first mode left out and not beyond it; without it they are dropped altogether.
        `monitor_joints` [B, Pj], `monitor_members` [B, Pm]: int32 device tensors of caller's joint ids / member ids
        (-1: none) whose complex response at every frequency is wanted.  Returns a dict of device tensors: for the
        names in `want` the envelopes u_amp, R_amp [B, L, nJ_max, 3], N_amp [B, L, nM_max] (the largest amplitude over
        the sweep; caller's joint numbering; u zero at held DOFs, R zero at free ones) with u_at, R_at, N_at (int32: the
        FIRST index of `omegas` that attains it); frf_u [B, L, S, Pj, 3] and frf_N [B, L, S, Pm] (complex128) when
        monitors are given; g [B, L, p] (the modal loads, zeros beyond n_modes) and n_modes [B].  `out`: such a dict to
        write into.  The frf outputs are refused above `max_result_bytes`.
        Guarded by `_current_modes`: the `modes()` state must be current (ValueError when `factor()`,
        `solve_cases()`, ... ran since; `generation`: the value the caller saw after ITS `modes()`, checked as well).
        Nothing is bumped here: the case block is only scratch, and X, lam and n_mass are only read - `mode_gradients`
        and `response_spectrum` work afterwards with the same bits, and the call can be repeated."""
        t = self.torch
        p = self._current_modes("harmonic", generation)["p"]
        if pattern is not None:
            pattern = self._check_loads("harmonic", pattern)
        mon_j = self._monitor_ids("monitor_joints", monitor_joints, True)
        mon_m = self._monitor_ids("monitor_members", monitor_members, False)
        Pj, Pm = int(mon_j.shape[1]), int(mon_m.shape[1])
        W, ag, L, want = _check_harmonic_args(self.B, self.nJ_max, p, omegas, None if pattern is None else pattern.shape,
                                              accel, damping, damp_mass, damp_stiff, want, Pj, Pm, max_result_bytes)
        S = int(W.size)
        if self.B and not self.lib.trs_hr_fits(self.nJ_max, self.nM_max, p):     # (before any output is allocated)
            raise HipExtensionError(f"harmonic(): the response vectors of a truss of {self.nJ_max} joints / "
                                    f"{self.nM_max} members exceed the LDS of the sweep kernel (trs_hr_fits)")
        if out is not None:   # (what an earlier call returned: the complex views of its frf tensors)
            out = {k: t.view_as_real(x) if k in ("frf_u", "frf_N") and x.is_complex() else x for k, x in out.items()}
        keys = ("n_modes",) + tuple(k + end for k in want for end in ("_amp", "_at")) + \
            (("frf_u",) if Pj else ()) + (("frf_N",) if Pm else ())
        shapes = {"g": ([self.B, L, p], t.float64)}   # (the modal loads: no field of `HarmonicResult`)
        shapes.update(_field_shapes(HarmonicResult.FIELDS, self.B, self._sizes(P=p, L=L, S=S, Pj=Pj, Pm=Pm), keys))
        out = self._out_tensors("harmonic", shapes, out)
        if self.B:
            ws = self._modes_ws
            jo, stream, tab = self._case_launch()
            Pr = None
            with t.cuda.device(self.device):
                W_d, ag_d = self._to_device(W), None if ag is None else self._to_device(ag)
                if pattern is not None:
                    Pr = self._hr_Pr = self._case_block("_hr_Pr", L)
                    self._gather_cases(pattern, L, Pr)
                F = self._residual_block(residual, lambda F: _capi.check(self.lib.trs_hr_modal(
                    self.B, L, self.nJ_max, self.free_index.data_ptr(), self.n_free.data_ptr(), self.nJ.data_ptr(),
                    ws["X"].data_ptr(), self.rows, ws["lam"].data_ptr(), ws["Mf"].data_ptr(), ws["n_mass"].data_ptr(), p,
                    _ptr(Pr), _ptr(ag_d), int(bool(residual)), out["g"].data_ptr(), _ptr(F), stream), "trs_hr_modal"))
                if want or Pj or Pm:
                    get = lambda k: _ptr(out.get(k))
                    _capi.check(getattr(self.lib, f"trs_hr_sweep{tab}")(
                        self.B, L, self.nJ_max, self.nM_max, self.xyz.data_ptr(), *self._members(),
                        self.free_index.data_ptr(), self.n_free.data_ptr(), self.nJ.data_ptr(), self.nM.data_ptr(), jo,
                        ws["X"].data_ptr(), self.rows, ws["lam"].data_ptr(), ws["n_mass"].data_ptr(), p,
                        out["g"].data_ptr(), _ptr(F), S, W_d.data_ptr(), float(damping), float(damp_mass),
                        float(damp_stiff), get("u_amp"), get("u_at"), get("R_amp"), get("R_at"), get("N_amp"),
                        get("N_at"), mon_j.data_ptr() if Pj else None, Pj, mon_m.data_ptr() if Pm else None, Pm,
                        get("frf_u"), get("frf_N"), stream), f"trs_hr_sweep{tab}")
                out["n_modes"].copy_(ws["n_mass"].clamp(max=p))
        for k in ("frf_u", "frf_N"):
            if k in out:
                out[k] = t.view_as_complex(out[k])
        return out

    # -- transient response: Newmark time stepping on a factor of K + sigma M (include/trs_dynamics.h) ------------------
    def factor_dynamic(self, dt, beta=0.25, gamma=0.5, damp_mass=0.0, damp_stiff=0.0, joint_mass=None, mass_scale=1.0):
        """`factor()` for the time domain: dofmap, assembly, the lumped mass of `modes` (`trs_modes_mass`, the same
        `joint_mass` and `mass_scale`), the diagonal shift S[c][c] += sigma Mf[c] (`trs_dyn_shift`) and the Cholesky
        factorisation - the slab then holds a factor of K_ff + sigma M, sigma = (a0 + a1 damp_mass) / (1 + a1 damp_stiff)
        of the Newmark scheme (`beta`, `gamma`, step `dt`) with Rayleigh damping C = damp_mass M + damp_stiff K_ff, for
        any number of `transient` calls.  The static analyses (`solve_cases`, `modes`, `member_loss`, ...) refuse with
        their "no factor" error until a plain `factor()`, which in turn ends the dynamic state; `generation` is bumped;
        `self.info` keeps its meaning.  The compact member form of the assembly (`options["compact"]`) has no slab to
        shift and is refused, as is a batch on the fused small-system path."""
        t = self.torch
        self._need_slab("factor_dynamic", "leaves no slab whose diagonal could be shifted")
        const = newmark_constants(dt, beta, gamma, damp_mass, damp_stiff)
        _check_mass_args("factor_dynamic()", self.B, self.nJ_max, None if joint_mass is None else tuple(joint_mass.shape),
                         mass_scale)
        if joint_mass is not None:
            if joint_mass.dtype != t.float64 or joint_mass.device != self.device:
                raise ValueError(f"factor_dynamic(): joint_mass must be float64 [B={self.B}, nJ_max={self.nJ_max}] on "
                                 f"{self.device}")
            joint_mass = joint_mass.contiguous()
        self._need_fit("factor_dynamic", not self.B or self.lib.trs_modes_fits(self.nJ_max, self.nM_max),
                       "the mass kernel (trs_modes_fits)")
        self._factored = False
        self._dynamic = None
        with t.cuda.device(self.device):
            self.dofmap()
            self.assemble()
            Mf, n_mass = self._lumped_mass(joint_mass, mass_scale)
            if self.B:
                _capi.check(self.lib.trs_dyn_shift(self.B, self.n_free.data_ptr(), self.ld, self.rows, self.S.data_ptr(),
                                                   Mf.data_ptr(), self.rows, const["sigma"], self._stream()),
                            "trs_dyn_shift")
            self.potrf()
        self._bump_generation()
        self._forward = None
        self._dynamic = dict(const, Mf=Mf, n_mass=n_mass, generation=self.generation)

    def _block_iteration(self, F, step, state, max_iters, check_every, between=None):
        """The loop of `modes` and of a round of `buckling` on the block `F` of 16 vectors: `step(1, 0, 0)` starts it; an
        iteration is `trs_potrs_cases` on F, `between()` if given, and `step(0, check, it)` with the residuals on every
        `check_every`-th iteration and on the last, where ONE small read-back (any `state` still 0?) ends the loop."""
        step(1, 0, 0)
        for it in range(1, max_iters + 1):
            check = it % check_every == 0 or it == max_iters
            self._potrs_cases(F, MODES_BLOCK)
            if between is not None:
                between()
            step(0, int(check), it)
            if check and not bool((state == 0).any().item()):   # the one read-back per check point
                break

    def _lumped_mass(self, joint_mass, mass_scale, into=None):
        """(Mf [B, rows], n_mass [B]) of `trs_modes_mass` for the resident batch (`dofmap()` first): the lumped mass of
        every free DOF in the reduced numbering, zero on the padding.  `into`: (Mf, n_mass) to fill, not new ones."""
        t = self.torch
        Mf, n_mass = into or (t.zeros([self.B, self.rows], dtype=t.float64, device=self.device),
                              t.zeros([self.B], dtype=t.int32, device=self.device))
        if self.B:
            jo, stream, tab = self._case_launch()
            members = self._members() if self.table else (self.conn.data_ptr(), self.A.data_ptr(), self.rho.data_ptr())
            _capi.check(getattr(self.lib, f"trs_modes{tab}_mass")(
                self.B, self.nJ_max, self.nM_max, self.xyz.data_ptr(), *members, _ptr(joint_mass), jo,
                float(mass_scale), self.free_index.data_ptr(), self.n_free.data_ptr(), self.nJ.data_ptr(),
                self.nM.data_ptr(), Mf.data_ptr(), self.rows, n_mass.data_ptr(), stream), f"trs_modes{tab}_mass")
        return Mf, n_mass

    def _monitor_ids(self, what, ids, device_order):
        """A monitor list of `transient`: int32 [B, P] on this device (None: P = 0), -1 = none; `device_order`: caller's
        joint ids are translated into the batch's joint order."""
        t = self.torch
        if ids is None:
            return t.zeros([self.B, 0], dtype=t.int32, device=self.device)
        if ids.dim() != 2 or int(ids.shape[0]) != self.B or ids.dtype != t.int32 or ids.device != self.device:
            raise ValueError(f"transient(): {what} must be int32 [B={self.B}, P] on {self.device}")
        ids = ids.contiguous()
        if device_order and self.joint_out is not None and int(ids.shape[1]):
            where = t.empty_like(self.joint_out)   # where[b, caller's id] = the joint's place in the batch's order
            where.scatter_(1, self.joint_out.long(), t.arange(self.nJ_max, dtype=t.int32, device=self.device)
                           .expand(self.B, -1).contiguous())
            inside = (ids >= 0) & (ids < self.nJ_max)
            ids = t.where(inside, where.gather(1, ids.clamp(0, self.nJ_max - 1).long()), t.full_like(ids, -1)).contiguous()
        return ids

    def transient(self, pattern, steps, scale=None, accel=None, monitor_joints=None, monitor_members=None, state=None,
                  out=None):
        """`steps` Newmark steps of M u'' + C u' + K_ff u = scale(t) P - M iota(accel(t)) for L excitations per truss on
        the factor that `factor_dynamic` left: per step one `trs_potrs_cases` launch and one `trs_dyn_step` launch.
        `pattern`: float64 device tensor [B, L, nJ_max, 3], the load pattern P in the CALLER's joint numbering (reduced
        once by `trs_gather_cases`); `scale` [B, L, steps + 1] (None: 1) and `accel` [B, L, steps + 1, 3] (ground
        acceleration, None: 0; the displacements are then relative to the ground) at the time points 0 .. steps of this
        call; `monitor_joints` [B, Pj], `monitor_members` [B, Pm]: int32 device tensors of caller's joint ids / member ids
        (-1: none) whose histories are wanted.  Starts from rest (u = v = 0, a = f_0 / M) or, with `state` = the
        "state" of an earlier call on this batch, from where that call ended (its time point `steps` is this call's time
        point 0; the state's tensors are advanced in place).  Returns a dict of device tensors: the envelopes over this
        call's time points - u_peak [B, L, nJ_max, 3] = max |u| with u_step (int32, the FIRST point that attains it),
        N_max, N_min [B, L, nM_max] with N_max_step, N_min_step -, the histories hist_u [B, L, steps + 1, Pj, 3] and
        hist_N [B, L, steps + 1, Pm], the last u, v, a [B, L, nJ_max, 3] (caller's numbering), and "state".  A state of
        another batch, another `factor_dynamic` or another L is refused."""
        t = self.torch
        dyn = getattr(self, "_dynamic", None)
        if dyn is None:
            raise ValueError("transient(): no dynamic factor - call factor_dynamic() first")
        pattern = self._check_loads("transient", pattern)
        L = int(pattern.shape[1])
        if isinstance(steps, bool) or int(steps) != steps or int(steps) < 1:
            raise ValueError(f"transient(): steps must be an integer of at least 1, got {steps!r}")
        T1 = int(steps) + 1
        for name, x, tail in (("scale", scale, ()), ("accel", accel, (3,))):
            if x is not None and (tuple(int(v) for v in x.shape) != (self.B, L, T1) + tail or x.dtype != t.float64
                                  or x.device != self.device):
                raise ValueError(f"transient(): {name} must be float64 {[self.B, L, T1] + list(tail)} on {self.device}")
        scale = None if scale is None else scale.contiguous()
        accel = None if accel is None else accel.contiguous()
        mon_j = self._monitor_ids("monitor_joints", monitor_joints, True)
        mon_m = self._monitor_ids("monitor_members", monitor_members, False)
        Pj, Pm = int(mon_j.shape[1]), int(mon_m.shape[1])
        if state is not None:
            if state.get("batch") is not self or state.get("generation") != dyn["generation"] or state.get("L") != L:
                raise ValueError("transient(): state belongs to another batch, another factor_dynamic() or another L")
        out = self._out_tensors("transient", _field_shapes(TransientResult.FIELDS, self.B,
                                                           self._sizes(L=L, T1=T1, Pj=Pj, Pm=Pm)), out)
        if state is None:
            f64 = lambda: t.empty([self.B, L, self.rows], dtype=t.float64, device=self.device)
            state = {"U": f64(), "V": f64(), "Acc": f64(), "step": 0, "batch": self, "generation": dyn["generation"], "L": L}
            first = 1
        else:
            first = 2
        out["state"] = state
        if self.B == 0 or L == 0:
            return out
        damped = dyn["damp_stiff"] > 0.0
        self._need_fit("transient", self.lib.trs_dyn_fits(self.nJ_max, self.nM_max, int(damped)),
                       "the step kernel (trs_dyn_fits)")
        Pr = self._dyn_Pr = self._case_block("_dyn_Pr", L)
        F = self._dyn_F = self._case_block("_dyn_F", L)
        jo, stream, tab = self._case_launch()
        fn = getattr(self.lib, f"trs_dyn{tab}_step")

        def step(first, n):
            _capi.check(fn(
                self.B, L, self.nJ_max, self.nM_max, self.xyz.data_ptr(), *self._members(), self.free_index.data_ptr(),
                self.n_free.data_ptr(), self.nJ.data_ptr(), self.nM.data_ptr(), dyn["Mf"].data_ptr(), Pr.data_ptr(),
                _ptr(scale), _ptr(accel), T1, n, first, dyn["dt"], dyn["beta"], dyn["gamma"], dyn["damp_mass"],
                dyn["damp_stiff"], F.data_ptr(), state["U"].data_ptr(), state["V"].data_ptr(), state["Acc"].data_ptr(),
                self.rows, out["u_peak"].data_ptr(), out["u_step"].data_ptr(), out["N_max"].data_ptr(),
                out["N_max_step"].data_ptr(), out["N_min"].data_ptr(), out["N_min_step"].data_ptr(),
                mon_j.data_ptr() if Pj else None, Pj, mon_m.data_ptr() if Pm else None, Pm,
                out["hist_u"].data_ptr() if Pj else None, out["hist_N"].data_ptr() if Pm else None, jo, stream),
                f"trs_dyn{tab}_step")

        with t.cuda.device(self.device):
            self._gather_cases(pattern, L, Pr)
            step(first, 0)
            for n in range(1, T1):
                self._potrs_cases(F, L)
                step(0, n)
            _capi.check(self.lib.trs_dyn_collect(
                self.B, L, self.nJ_max, state["U"].data_ptr(), state["V"].data_ptr(), state["Acc"].data_ptr(), self.rows,
                self.free_index.data_ptr(), self.nJ.data_ptr(), jo, out["u"].data_ptr(), out["v"].data_ptr(),
                out["a"].data_ptr(), stream), "trs_dyn_collect")
        state["step"] += T1 - 1
        return out

    def nonlinear(self, load_factors, tol=1e-9, max_iters=25, check_every=1, out=None):
        """Geometrically nonlinear statics of the resident batch under `load_factors` times its own loads
        (include/trs_nonlinear.h: corotational bars, Newton's method on the tangent factor).  The load steps run in the
        given order, each from the previous step's converged u (the first from u = 0).  Per Newton iteration six
        launches: `trs_nl_state` (member forces, residual, convergence test), `trs_assemble` at the deformed
        coordinates with the residual as load, `trs_nl_tangent` (the slab then holds K_t), `trs_potrf_batched` and
        `trs_potrs_batched` as they are, `trs_nl_update`.  A truss is converged when |r|_inf <= `tol` |lambda P|_inf;
        it is then frozen, as is one whose tangent is not positive definite (`info != 0`: it keeps its last accepted u),
        so a truss's results depend neither on the others nor on `check_every` nor on `max_iters` beyond its own count.
        Every `check_every` iterations one int32 - the number of trusses still iterating - is downloaded to end a step
        early.  Returns a dict of device tensors over the S load steps, in the caller's joint numbering: u, f_ext
        [B, S, nJ_max, 3] (f_ext: the applied load at free DOFs, the reaction at held ones), N [B, S, nM_max], iters,
        status (int32 [B, S]: 0 converged, 1 iteration limit, 2 tangent not positive definite - u is the last accepted
        iterate, iters the number of accepted updates -, 3 not attempted because an earlier step failed) and residual
        [B, S] = |r|_inf at the u returned.  Afterwards the slab holds a tangent factor: the static analyses and
        `transient` refuse with their "no factor" errors until `factor()` / `factor_dynamic()`; `generation` is bumped;
        `self.xyz` and `self.loads` are untouched.  The compact member form of the assembly (`options["compact"]`) has
        no slab to amend and is refused, as is a batch on the fused small-system path."""
        t = self.torch
        self._need_slab("nonlinear", "leaves no slab that could be amended to the tangent")
        lams = _check_newton_args("nonlinear()", load_factors, tol, max_iters, check_every)
        S = len(lams)
        out = self._out_tensors("nonlinear", _field_shapes(NonlinearResult.FIELDS, self.B, self._sizes(S=S)), out)
        if self.B == 0:
            return out
        self._need_fit("nonlinear", self.lib.trs_nl_fits(self.nJ_max, self.nM_max), "the state kernel (trs_nl_fits)")
        self._factored = False
        self._dynamic = None
        self._forward = None
        ws = self._nl_workspace(max_iters, out)
        with t.cuda.device(self.device):
            self.dofmap()
            for step, lam in enumerate(lams):
                ws["active"].zero_()
                it = 0
                while True:
                    last = it == max_iters
                    self._nl_state(ws, lam, tol, it, last, step, S, it)
                    if last:
                        break
                    if it % check_every == 0 and int(ws["active"][it].item()) == 0:
                        self._nl_state(ws, lam, tol, it, 2, step, S, max_iters + 1)   # (no truss is active: outputs only)
                        break
                    self.assemble(xyz=ws["Xc"], loads=ws["R"])
                    self._nl_tangent(ws)
                    self.potrf()
                    self.potrs()
                    it += 1
                    self._nl_update(ws, it)
            # (what the factorisation reported for the tangent that ended a truss with status 2; 0 for every other truss)
            self.info.copy_(ws["st"][:, 2])
        self._bump_generation()
        return out

    # the stages of `nonlinear` (tools/bench_nonlinear.py times them one by one)
    def _nl_workspace(self, max_iters, out):
        """The state of a `nonlinear` run: U [B, nJ_max, 3] (joint layout, the batch's numbering) and the status words
        st [B, 4], zeroed; Xc, R (the inputs of the assembly), the member table W and the `active` counters - one per
        iteration of a load step, plus one for the call that only writes the outputs."""
        t, dev = self.torch, self.device
        U = t.zeros([self.B, self.nJ_max, 3], dtype=t.float64, device=dev)
        return {"U": U, "st": t.zeros([self.B, 4], dtype=t.int32, device=dev), "Xc": t.empty_like(U), "R": t.empty_like(U),
                "W": t.empty([self.B, max(self.nM_max, 1), 6], dtype=t.float64, device=dev),
                "active": t.zeros([max_iters + 2], dtype=t.int32, device=dev), "out": out}

    def _nl_state(self, ws, lam, tol, it, last, step, S, slot):
        jo, stream, tab = self._case_launch()
        out = ws["out"]
        _capi.check(getattr(self.lib, "trs_nl_state" + tab)(
            self.B, self.nJ_max, self.nM_max, self.xyz.data_ptr(), *self._members(), self.loads.data_ptr(),
            self.free_index.data_ptr(), self.n_free.data_ptr(), self.nJ.data_ptr(), self.nM.data_ptr(), self.rows,
            float(lam), float(tol), it, int(last), step, S, ws["U"].data_ptr(), ws["st"].data_ptr(), ws["Xc"].data_ptr(),
            ws["R"].data_ptr(), ws["W"].data_ptr(), ws["active"][slot:].data_ptr(), out["u"].data_ptr(),
            out["N"].data_ptr(), out["f_ext"].data_ptr(), out["iters"].data_ptr(), out["status"].data_ptr(),
            out["residual"].data_ptr(), jo, stream), "trs_nl_state" + tab)

    def _nl_tangent(self, ws, flags=0):
        """`flags`: what the assembly before it was given beside the batch's own flags (tests: ASM_FULL_SYMMETRIC)."""
        _, stream, tab = self._case_launch()
        _capi.check(getattr(self.lib, "trs_nl_tangent" + tab)(
            self.B, self.nJ_max, self.nM_max, *self._members(), self.free_index.data_ptr(), self.n_free.data_ptr(),
            self.nJ.data_ptr(), self.nM.data_ptr(), self.ld, self.rows, self.S.data_ptr(), self._env_ptr(),
            flags | self._assemble_flags(), ws["W"].data_ptr(), stream), "trs_nl_tangent" + tab)

    def _nl_update(self, ws, it):
        _capi.check(self.lib.trs_nl_update(
            self.B, self.nJ_max, self.free_index.data_ptr(), self.n_free.data_ptr(), self.nJ.data_ptr(),
            self.uf.data_ptr(), self.rows, self.info.data_ptr(), it, ws["U"].data_ptr(), ws["st"].data_ptr(),
            self._stream()), "trs_nl_update")

    # -- the iterated analyses - sizing, min_compliance, min_weight, unilateral, plastic - share one driver and one run protocol
    # (csrc/trs_iterate.h): analyse, one step kernel, one look at one counter ------------------------------
    def _refuse_iterated(self, name, what="load cases"):
        """What none of the five runs on: the fused small-system path, `options["compact"]` and the table form."""
        self._need_slab(name, f"writes no slab that the {what} could be solved against")
        if self.table:
            raise ValueError(f"{name}(): the table member form cannot hold one area per member - use the general form "
                             "(PackedBatch.general())")

    def _begin_iterated(self, name, *fits):
        """`fits`: (trs_*_fits, what it speaks for) of every kernel with LDS tables of the truss's shape.  The run
        factors designs of its own: what the batch held of a factor, a dynamic factor or a forward solve is void."""
        for fits_fn, what in fits:
            self._need_fit(name, fits_fn(self.nJ_max, self.nM_max), what)
        self._factored = False
        self._dynamic = None
        self._forward = None

    def _run_state(self, limit, L, loads, own=False, **more):
        """The state every run has: the status words st [B, 4] (status, count, the latched info, spare) and the `active`
        counters (one per analysis), zeroed; the case block of L cases; `loads` as `_analyse_cases` gathers them (`own`:
        the batch's own, already in the batch's joint order).  `more`: what the analysis adds."""
        t, dev = self.torch, self.device
        return dict(more, st=t.zeros([self.B, 4], dtype=t.int32, device=dev),
                    active=t.zeros([limit + 1], dtype=t.int32, device=dev), F=self._case_block("cases_F", L), L=L,
                    loads=loads, own=own, limit=limit)

    def _active(self, ws, it):
        """The counter that analysis `it` adds to (a report behind the last analysis: the last one's)."""
        return ws["active"][min(it, ws["limit"]):].data_ptr()

    def _iterate(self, ws, check_every, analyse, step):
        """analyse(ws), step(ws, it, mode) - mode 1 at the limit, else 0 - until the limit or until, at every
        `check_every`-th analysis, the one int32 read back says that no truss is still iterating.  Returns the last
        `it`."""
        it = 0
        while True:
            last = it == ws["limit"]
            analyse(ws)
            step(ws, it, 1 if last else 0)
            if last or (it % check_every == 0 and int(ws["active"][it].item()) == 0):
                return it
            it += 1

    def _end_iterated(self, ws, out, count="iterations"):
        """status and the count from st; `self.info`: what the factorisation reported for the design that ended a truss
        with the failed status, latched, 0 for every other truss; the slab holds the factor of the final design."""
        out["status"].copy_(ws["st"][:, 0])
        out[count].copy_(ws["st"][:, 1])
        self.info.copy_(ws["st"][:, 2])
        self.cases_F = ws["F"]
        self._factored = True
        self._bump_generation()

    def _area_bounds(self, who, area_min, area_max):
        """[(tensor or None, number)] of `area_min`, `area_max`: each a number or a float64 [B, nM_max] device tensor."""
        t, bounds = self.torch, []
        for name, x in (("area_min", area_min), ("area_max", area_max)):
            if hasattr(x, "data_ptr"):
                if list(x.shape) != [self.B, self.nM_max] or x.dtype != t.float64 or x.device != self.device:
                    raise ValueError(f"{who}: {name} must be a number or a float64 [B={self.B}, nM_max={self.nM_max}] "
                                     f"tensor on {self.device}")
                bounds.append((x.contiguous(), 0.0))
            else:
                bounds.append((None, _check_number(who, name, x, "be a finite number or a float64 [B, nM_max] tensor")))
        if bounds[0][0] is None and not bounds[0][1] > 0:
            raise ValueError(f"{who}: area_min must be positive, got {area_min!r}")
        if bounds[0][0] is None and bounds[1][0] is None and bounds[1][1] < bounds[0][1]:
            raise ValueError(f"{who}: area_max must be >= area_min, got {area_max!r} < {area_min!r}")
        return bounds

    def _own_loads(self):
        """The batch's own loads [B, nJ_max, 3] in the CALLER's joint numbering (carried there through `joint_out`)."""
        if self.joint_out is None:
            return self.loads
        index = self.joint_out.long().unsqueeze(-1).expand(-1, -1, 3)
        return self.torch.zeros_like(self.loads).scatter_(1, index, self.loads)

    def _analyse_cases(self, ws):
        """Assembly and factorisation of the design `self.A`, gather and substitution of the L cases of the run."""
        self.assemble()
        self.potrf()
        self._gather_cases(ws["loads"], ws["L"], ws["F"], own=ws["own"])
        self._potrs_cases(ws["F"], ws["L"])

    # -- member sizing: fully stressed design iterated on the device (include/trs_sizing.h) ------------------------------
    def sizing(self, loads=None, *, allow_tension, allow_compression, allow_displace=0.0, euler_kappa=0.0, area_min,
               area_max, relax=1.0, tol=1e-4, max_iters=40, check_every=1, catalog=None, out=None):
        """Member sizing of the resident batch by the stress-ratio method (include/trs_sizing.h: fully stressed design
        with a displacement envelope): every design is analysed under all L load cases, every member is resized to what
        its worst case demands - N / `allow_tension` in tension, the larger of P / `allow_compression` and the Euler
        area sqrt(P L0^2 / (pi^2 E `euler_kappa`)) in compression (I = kappa A^2; 0: no member buckling check), or the
        displacement ratio max |u_j| / `allow_displace` (0: no limit) where that is larger -, damped by `relax` in
        (0, 1] and clamped to [`area_min`, `area_max`] (scalars or float64 device tensors [B, nM_max]; equal bounds fix
        a member), until no area moves by more than `tol` (relative) or `max_iters` resizings are done.  `loads`:
        float64 device tensor [B, L, nJ_max, 3] as `solve_cases` takes them (None: the batch's own loads as one case).
        Each of the three allowables is one number for the batch or one per truss (an array [B]).
        The initial design is the batch's own A.  Per iteration five launches: `trs_assemble`, `trs_potrf_batched`,
        `trs_gather_cases`, `trs_potrs_cases` and `trs_sz_step`, which reads the L reduced solutions from the case block
        and writes the next design - neither u nor N of a case goes to HBM.  A converged truss is frozen, as is one whose
        design cannot be factored (`info != 0`: it goes back to the design before), so a truss's results depend neither
        on the others nor on `check_every` nor on `max_iters` beyond its own count.  Every `check_every` iterations one
        int32 - the number of trusses still iterating - is downloaded to stop early.  `catalog` (ascending areas, 1 to
        256): afterwards every member of a truss of status 0 or 1 goes to the smallest catalogue area >= its area (the
        largest where there is none) and ONE more analysis rewrites that truss's outputs; status and iterations stay.
        Returns a dict of device tensors, in the caller's member order: areas, utilisation [B, nM_max] (req / A: stress and
        member buckling only, <= 1 is feasible), governing (int32 [B, nM_max]: the governing case, -1 where the
        displacement ratio governs and on the padding), weight, disp_ratio [B], iterations, status (int32 [B]: 0
        converged, 1 iteration limit, 2 a design could not be factored), weight_history [B, max_iters + 1] (zero beyond
        the truss's own count) and - with `catalog` - catalog_index (uint8 [B, nM_max]).  `self.info` holds 0, or for a
        truss of status 2 what the factorisation reported, latched.  Afterwards `self.A` holds the returned areas and
        the slab the factor of the returned design for every truss of status 0 or 1: `solve_cases`, `solve_effect_cases`
        and `member_loss` may follow without another `factor()`; `generation` is bumped.  A batch on the fused
        small-system path, `options["compact"]` and the table member form (the step writes one area per member, which a
        type table cannot hold: `PackedBatch.general()` first) are refused."""
        t = self.torch
        self._refuse_iterated("sizing")
        val = _check_sizing_scalars("sizing()", allow_tension, allow_compression, allow_displace, euler_kappa, relax, tol,
                                    max_iters, check_every, catalog, B=self.B)
        bounds = self._area_bounds("sizing()", area_min, area_max)
        own = loads is None   # (the batch's own loads are already in the batch's joint order: gathered without joint_in)
        loads = self._check_loads("sizing", self.loads.unsqueeze(1) if own else loads)
        L, H = int(loads.shape[1]), val["max_iters"] + 1
        if L < 1:
            raise ValueError("sizing(): loads must hold at least one case")
        keys = [k for k, *_ in SizingResult.FIELDS.values() if k != "catalog_index" or val["catalog"] is not None]
        out = self._out_tensors("sizing", _field_shapes(SizingResult.FIELDS, self.B, self._sizes(H=H), keys), out)
        if self.B == 0:
            return out
        self._begin_iterated("sizing", (self.lib.trs_sz_fits, "the step kernel (trs_sz_fits)"))
        ws = self._sz_workspace(val, bounds, loads, out, own)
        with t.cuda.device(self.device):
            self.dofmap()
            out["weight_history"].zero_()
            it = self._iterate(ws, val["check_every"], self._analyse_cases, self._sz_step)
            if val["catalog"] is not None:
                cat = t.from_numpy(val["catalog"]).to(self.device)
                _capi.check(self.lib.trs_sz_snap(self.B, self.nM_max, self.nM.data_ptr(), ws["st"].data_ptr(), cat.data_ptr(),
                                                 int(cat.shape[0]), self.A.data_ptr(), out["catalog_index"].data_ptr(),
                                                 self._stream()), "trs_sz_snap")
                self._analyse_cases(ws)
                self._sz_step(ws, it, 2)
            self._end_iterated(ws, out)   # (the factor: of the returned design, for every truss of status 0 or 1)
        return out

    # the stages of `sizing` (tools/bench_sizing.py times them one by one)
    def _sz_workspace(self, val, bounds, loads, out, own=False):
        """The state of a `sizing` run: the design before the last resizing, the status words st [B, 4] and the `active`
        counters (one per analysis), zeroed; the case block; the arguments (`own`: `loads` are the batch's own, in the
        batch's joint order); `allow` [B, 3] when an allowable is given per truss."""
        t, dev = self.torch, self.device
        L = int(loads.shape[1])
        names = ("allow_tension", "allow_compression", "allow_displace")
        allow = None
        if any(isinstance(val[k], np.ndarray) for k in names):
            allow = t.from_numpy(np.stack([np.broadcast_to(val[k], [self.B]) for k in names], axis=1).copy()).to(dev)
            val = dict(val, **{k: float(np.max(val[k])) for k in names})   # (scalars that pass the library's own check)
        prev = t.zeros([self.B, max(self.nM_max, 1)], dtype=t.float64, device=dev)
        return self._run_state(val["max_iters"], L, loads, own, prev=prev, val=val, bounds=bounds, allow=allow, out=out)

    def _sz_step(self, ws, it, mode):
        val, out, (lo, hi) = ws["val"], ws["out"], ws["bounds"]
        _capi.check(self.lib.trs_sz_step(
            self.B, ws["L"], self.nJ_max, self.nM_max, self.xyz.data_ptr(), self.conn.data_ptr(), self.E.data_ptr(),
            self.A.data_ptr(), self.rho.data_ptr(), self.free_index.data_ptr(), self.n_free.data_ptr(), self.nJ.data_ptr(),
            self.nM.data_ptr(), ws["F"].data_ptr(), self.rows, self.info.data_ptr(), val["allow_tension"],
            val["allow_compression"], val["allow_displace"], _ptr(ws["allow"]), val["euler_kappa"], val["relax"],
            val["tol"], _ptr(lo[0]),
            lo[1], _ptr(hi[0]), hi[1], it, mode, ws["prev"].data_ptr(), ws["st"].data_ptr(),
            self._active(ws, it), out["areas"].data_ptr(), out["weight"].data_ptr(),
            out["utilisation"].data_ptr(), out["governing"].data_ptr(), out["disp_ratio"].data_ptr(),
            out["weight_history"].data_ptr(), val["max_iters"] + 1, self._stream()), "trs_sz_step")

    # -- compliance sizing: the stiffest design at a given weight, iterated on the device (include/trs_compliance.h) -----
    def min_compliance(self, loads=None, *, alpha=None, target=None, measure="weight", eta=0.5, move=0.2, area_min,
                       area_max, tol=1e-4, max_iters=60, check_every=1, out=None, levels=0):
        """Compliance sizing of the resident batch (include/trs_compliance.h: the optimality-criteria method): the areas
        that make every truss stiffest - the smallest J = sum_l `alpha`_l C_l, C_l = f_l.u_l the compliance of load case
        l - at the measure `target` = sum w A, w = rho L0 (`measure` "weight") or L0 ("volume").  Every design is
        analysed under all L load cases; the sensitivities -dJ/dA_m = s_m are the members' own strain energies per area
        (no adjoint solve); every member goes to A_m (s_m / (x w_m))^`eta`, held within `move` (relative) of A_m and
        within [`area_min`, `area_max`] (scalars or float64 device tensors [B, nM_max]; equal bounds fix a member), the
        multiplier x found by 64 bisections so that the new design meets the target; until no area moves by more than
        `tol` (relative) or `max_iters` resizings are done.  `loads`: float64 device tensor [B, L, nJ_max, 3] as
        `solve_cases` takes them (None: the batch's own loads as one case); `alpha`: L weights >= 0, not all zero (None:
        ones); `target`: a number > 0, one per truss (an array or float64 device tensor [B]) or None: the measure of
        the initial design, the batch's own A.  Per iteration five launches: `trs_assemble`, `trs_potrf_batched`,
        `trs_gather_cases`, `trs_potrs_cases` and `trs_cm_step`, which reads the L reduced solutions from the case block
        and writes the next design - neither u nor N of a case goes to HBM.  A converged truss is frozen, as is one whose
        design cannot be factored (`info != 0`: it goes back to the design before), so a truss's results depend neither
        on the others nor on `check_every` nor on `max_iters` beyond its own count.  `levels`: how many levels of the
        bisection the kernel evaluates per round (1, 2, 3; 0: the library's choice) - the same bits either way.
        Returns a dict of device tensors, in the caller's member order: areas, sensitivity [B, nM_max], measure,
        objective, multiplier [B], compliance [B, L], objective_history [B, max_iters + 1] (zero beyond the truss's own
        count), iterations, status (int32 [B]: 0 converged, 1 iteration limit, 2 a design could not be factored).
        `self.info` holds 0, or for a truss of status 2 what the factorisation reported, latched.  Afterwards `self.A`
        holds the returned areas and the slab the factor of the returned design for every truss of status 0 or 1:
        `solve_cases` may follow without another `factor()`; `generation` is bumped.  A batch on the fused small-system
        path, `options["compact"]` and the table member form are refused, as in `sizing()`."""
        t = self.torch
        who = "min_compliance()"
        self._refuse_iterated("min_compliance")
        own = loads is None   # (the batch's own loads are already in the batch's joint order: gathered without joint_in)
        loads = self._check_loads("min_compliance", self.loads.unsqueeze(1) if own else loads)
        L = int(loads.shape[1])
        if L < 1:
            raise ValueError(f"{who}: loads must hold at least one case")
        val = _check_min_compliance_scalars(who, alpha, measure, eta, move, tol, max_iters, check_every, L)
        if levels not in (0, 1, 2, 3):
            raise ValueError(f"{who}: levels must be 0, 1, 2 or 3, got {levels!r}")
        bounds = self._area_bounds(who, area_min, area_max)
        if target is None:
            W = t.zeros([self.B], dtype=t.float64, device=self.device)   # (the step fills in the initial measure)
        elif hasattr(target, "data_ptr"):
            if list(target.shape) != [self.B] or target.dtype != t.float64 or target.device != self.device:
                raise ValueError(f"{who}: target must be a positive number or a float64 [B={self.B}] tensor on {self.device}")
            W = target.clone()
        else:
            W = t.from_numpy(_check_target(who, target, self.B)).to(self.device)
        H = val["max_iters"] + 1
        out = self._out_tensors("min_compliance", _field_shapes(MinComplianceResult.FIELDS, self.B, self._sizes(H=H, L=L)),
                                out)
        if self.B == 0:
            return out
        self._begin_iterated("min_compliance", (self.lib.trs_cm_fits, "the step kernel (trs_cm_fits)"))
        ws = self._cm_workspace(val, bounds, loads, W, out, own, levels)
        with t.cuda.device(self.device):
            self.dofmap()
            out["objective_history"].zero_()
            self._iterate(ws, val["check_every"], self._analyse_cases, self._cm_step)
            self._end_iterated(ws, out)   # (the factor: of the returned design, for every truss of status 0 or 1)
        return out

    # the stages of `min_compliance` (tools/bench_compliance.py times them one by one; the analysis is `_analyse_cases`)
    def _cm_workspace(self, val, bounds, loads, target, out, own=False, levels=0):
        """The state of a `min_compliance` run: the design before the last resizing, the status words st [B, 4] and the
        `active` counters (one per analysis), zeroed; the case block; the weights and the targets on the device."""
        t, dev = self.torch, self.device
        L = int(loads.shape[1])
        prev = t.zeros([self.B, max(self.nM_max, 1)], dtype=t.float64, device=dev)
        return self._run_state(val["max_iters"], L, loads, own, prev=prev, alpha=t.from_numpy(val["alpha"]).to(dev),
                               target=target, levels=levels, val=val, bounds=bounds, out=out)

    def _cm_step(self, ws, it, mode):
        val, out, (lo, hi) = ws["val"], ws["out"], ws["bounds"]
        _capi.check(self.lib.trs_cm_step(
            self.B, ws["L"], self.nJ_max, self.nM_max, self.xyz.data_ptr(), self.conn.data_ptr(), self.E.data_ptr(),
            self.A.data_ptr(), self.rho.data_ptr(), self.free_index.data_ptr(), self.n_free.data_ptr(), self.nJ.data_ptr(),
            self.nM.data_ptr(), ws["F"].data_ptr(), self.rows, self.info.data_ptr(), ws["alpha"].data_ptr(),
            _capi.CM_MEASURES[val["measure"]], ws["target"].data_ptr(), val["eta"], val["move"], val["tol"], _ptr(lo[0]),
            lo[1], _ptr(hi[0]), hi[1], it, mode, ws["levels"], ws["prev"].data_ptr(), ws["st"].data_ptr(),
            self._active(ws, it), out["areas"].data_ptr(), out["measure"].data_ptr(),
            out["compliance"].data_ptr(), out["objective"].data_ptr(), out["objective_history"].data_ptr(),
            val["max_iters"] + 1, out["sensitivity"].data_ptr(), out["multiplier"].data_ptr(), self._stream()),
            "trs_cm_step")

    # -- minimum weight under displacement limits, iterated on the device (include/trs_minweight.h) ---------------------
    def min_weight(self, loads=None, *, limit_case, limit_joint, limit_direction, limit_value, measure="weight", move=0.2,
                   area_min, area_max, tol=1e-4, max_iters=60, sweeps=2, limit_tol=1e-2, check_every=1,
                   want_sensitivity=False, out=None, allow_tension=None, allow_compression=None, euler_kappa=0.0):
        """Minimum-weight sizing of the resident batch under displacement limits (include/trs_minweight.h: the
        optimality-criteria method with one multiplier per limit): the lightest design - the smallest sum w A, w = rho L0
        (`measure` "weight") or L0 ("volume") - with d_j.u_{l_j}(joint_j) <= `limit_value`_j for each of the J <= 8
        limits.  `limit_case`: J case numbers, shared by the batch; `limit_joint`: integers [J] or [B, J] in the CALLER's
        joint numbering (-1 switches a limit off for that truss); `limit_direction`: [J, 3] or [B, J, 3], normalised
        here; `limit_value`: a number, [J] or [B, J], > 0 (+inf switches a limit off); a two-sided limit is two limits
        with +-d.  Every design is analysed under the L load cases and the J unit loads of the limits, which are just
        more columns of the case block; the sensitivities are c_mj = (E / L0) proj_m(v_j) proj_m(u_{l_j}); the
        multipliers are found per truss by `sweeps` passes of one geometric bisection per limit inside the step kernel;
        every member goes to sqrt(sum_j mu_j q_mj / (w_m + sum_j mu_j n_mj)), held within `move` (relative) of A_m and
        within [`area_min`, `area_max`] (scalars or float64 device tensors [B, nM_max]; equal bounds fix a member), until
        no area moves by more than `tol` (relative) or `max_iters` resizings are done.  `loads`: float64 device tensor
        [B, L, nJ_max, 3] as `solve_cases` takes them (None: the batch's own loads as one case).  Per iteration five
        launches: `trs_assemble`, `trs_potrf_batched`, `trs_gather_cases`, `trs_potrs_cases` and `trs_mw_step`.  A truss
        that has left the run is frozen, as in `min_compliance()`: its results depend neither on the others nor on
        `check_every` nor on `max_iters` beyond its own count.
        Returns a dict of device tensors, in the caller's member order: areas [B, nM_max], measure [B], measure_history,
        worst_history [B, max_iters + 1] (zero beyond the truss's own count), displacement, ratio, multipliers [B, J]
        (g_j, g_j / limit_value_j - 0 for a limit that is switched off - and mu_j), iterations, status (int32 [B]: 0
        converged within `limit_tol` of its limits, 1 iteration limit, 2 a design could not be factored, 3 converged on
        its bounds without meeting a limit) and - with `want_sensitivity` - sensitivity [B, J, nM_max] = c_mj.
        `self.info` holds 0, or for a truss of status 2 what the factorisation reported, latched.  Afterwards `self.A`
        holds the returned areas and the slab the factor of the returned design for every truss of status 0, 1 or 3:
        `solve_cases` may follow without another `factor()`; `generation` is bumped.  A batch on the fused small-system
        path, `options["compact"]` and the table member form are refused, as in `sizing()`.
        Stress limits in the same run: `allow_tension` and `allow_compression` (both or neither; each a number > 0 or one
        per truss, an array [B], as `sizing()` takes them; +inf switches a side off) and `euler_kappa` >= 0 (I = kappa A^2;
        0: no member buckling term).  Every analysis gives every member the area its worst case demands - the stress-ratio
        area of `sizing()`, Euler term included - and uses it as the member's LOWER bound in the resizing, within the move
        limit and the area bounds: members governed by stress sit on that floor, members governed by a displacement limit
        are sized by the multipliers (`trs_mw_step_stress`: the same kernel with three more words per member in LDS).  The
        dict then also holds utilisation [B, nM_max] (req / A; <= 1 is feasible), governing (int32 [B, nM_max]: the case
        that sets a member's requirement, -1 where there is none and on the padding) and stress_history
        [B, max_iters + 1] (the largest utilisation of every design analysed); worst_history stays the displacement
        figure, and status 0 asks both for <= 1 + `limit_tol`, else 3.  With both None the call is the one without stress
        limits exactly: `trs_mw_step`, and none of the three keys."""
        t = self.torch
        who = "min_weight()"
        self._refuse_iterated("min_weight")
        # (the unit loads are in the caller's numbering, so the batch's own loads are carried there too)
        loads = self._check_loads("min_weight", self._own_loads().unsqueeze(1) if loads is None else loads)
        L = int(loads.shape[1])
        if L < 1:
            raise ValueError(f"{who}: loads must hold at least one case")
        val = _check_min_weight_scalars(who, measure, move, tol, max_iters, sweeps, limit_tol, check_every)
        stress = _check_stress_limits(who, allow_tension, allow_compression, euler_kappa, self.B)
        lim = _check_limits(who, limit_case, limit_joint, limit_direction, limit_value, self.B, self.nJ_max, L)
        J = int(lim["case"].size)
        bounds = self._area_bounds(who, area_min, area_max)
        H = val["max_iters"] + 1
        keys = [k for k, *_ in MinWeightResult.FIELDS.values()
                if (k != "sensitivity" or want_sensitivity) and (k not in _MW_STRESS_KEYS or stress is not None)]
        out = self._out_tensors("min_weight", _field_shapes(MinWeightResult.FIELDS, self.B, self._sizes(H=H, G=J), keys), out)
        if self.B == 0:
            return out
        fits, name = (self.lib.trs_mw_fits, "trs_mw_fits") if stress is None else \
            (self.lib.trs_mw_fits_stress, "trs_mw_fits_stress")
        self._begin_iterated("min_weight", (lambda nJ, nM: fits(nJ, nM, J), f"the step kernel ({name})"))
        ws = self._mw_workspace(val, bounds, loads, lim, out, stress)
        with t.cuda.device(self.device):
            self.dofmap()
            out["measure_history"].zero_()
            out["worst_history"].zero_()
            if stress is not None:
                out["stress_history"].zero_()
            self._iterate(ws, val["check_every"], self._analyse_cases, self._mw_step)
            self._end_iterated(ws, out)   # (the factor: of the returned design, for every truss of status 0, 1 or 3)
        return out

    # the stages of `min_weight` (tools/bench_minweight.py times them one by one; the analysis is `_analyse_cases`)
    def _mw_workspace(self, val, bounds, loads, lim, out, stress=None):
        """The state of a `min_weight` run: the design before the last resizing, the multipliers mu [B, J], the status
        words and the `active` counters, zeroed; the case block of L + J columns and its loads - the real cases, then
        the unit load d_j at every limit's joint (zero where the limit is switched off), in the caller's numbering; the
        limits on the device, their joints mapped through the batch's joint order into the device's numbering.
        `stress`: the dict of `_check_stress_limits` or None; an allowable given per truss makes `allow` [B, 2]."""
        t, dev = self.torch, self.device
        allow = None
        if stress is not None:
            names = ("allow_tension", "allow_compression")
            if any(isinstance(stress[k], np.ndarray) for k in names):
                allow = t.from_numpy(np.stack([np.broadcast_to(stress[k], [self.B]) for k in names], axis=1).copy()).to(dev)
                stress = dict(stress, **dict.fromkeys(names, 1.0))   # (not read beside `allow`)
        B, L, J = self.B, int(loads.shape[1]), int(lim["case"].size)
        joint = t.from_numpy(lim["joint"].astype(np.int64)).to(dev)                 # [B, J], the caller's numbering
        direction = t.from_numpy(lim["direction"]).to(dev)
        value = t.from_numpy(lim["value"]).to(dev)
        on = (joint >= 0) & t.isfinite(value)
        place = joint.clamp(min=0)
        unit = t.zeros([B, J, self.nJ_max, 3], dtype=t.float64, device=dev)
        unit.scatter_(2, place.view(B, J, 1, 1).expand(B, J, 1, 3), (direction * on.unsqueeze(-1)).unsqueeze(2))
        device_joint = place
        if self.joint_out is not None:   # joint_out[b, i] = the caller's id of the device's joint i: inverted here
            inverse = t.empty_like(self.joint_out, dtype=t.int64)
            inverse.scatter_(1, self.joint_out.long(), t.arange(self.nJ_max, device=dev).expand(B, -1))
            device_joint = inverse.gather(1, place)
        device_joint = t.where(on, device_joint, t.full_like(device_joint, -1)).to(t.int32).contiguous()
        prev = t.zeros([B, max(self.nM_max, 1)], dtype=t.float64, device=dev)
        return self._run_state(val["max_iters"], L + J, t.cat([loads, unit], dim=1).contiguous(), False, prev=prev,
                               mu=t.zeros([B, J], dtype=t.float64, device=dev), cases=L, J=J,
                               limit_case=t.from_numpy(lim["case"]).to(dev), limit_joint=device_joint,
                               limit_dir=direction.contiguous(), limit_value=value.contiguous(), val=val, bounds=bounds,
                               out=out, stress=stress, allow=allow)

    def _mw_step(self, ws, it, mode):
        val, out, (lo, hi) = ws["val"], ws["out"], ws["bounds"]
        stress = ws.get("stress")
        if stress is not None:
            _capi.check(self.lib.trs_mw_step_stress(
                self.B, ws["cases"], ws["J"], self.nJ_max, self.nM_max, self.xyz.data_ptr(), self.conn.data_ptr(),
                self.E.data_ptr(), self.A.data_ptr(), self.rho.data_ptr(), self.free_index.data_ptr(),
                self.n_free.data_ptr(), self.nJ.data_ptr(), self.nM.data_ptr(), ws["F"].data_ptr(), self.rows,
                self.info.data_ptr(), ws["limit_case"].data_ptr(), ws["limit_joint"].data_ptr(), ws["limit_dir"].data_ptr(),
                ws["limit_value"].data_ptr(), _capi.MW_MEASURES[val["measure"]], val["move"], val["tol"], val["limit_tol"],
                val["sweeps"], _ptr(lo[0]), lo[1], _ptr(hi[0]), hi[1], stress["allow_tension"], stress["allow_compression"],
                _ptr(ws["allow"]), stress["euler_kappa"], it, mode, ws["prev"].data_ptr(), ws["mu"].data_ptr(),
                ws["st"].data_ptr(), self._active(ws, it), out["areas"].data_ptr(), out["measure"].data_ptr(),
                out["measure_history"].data_ptr(), out["worst_history"].data_ptr(), val["max_iters"] + 1,
                out["displacement"].data_ptr(), out["ratio"].data_ptr(), out["multipliers"].data_ptr(),
                _ptr(out.get("sensitivity")), out["utilisation"].data_ptr(), out["governing"].data_ptr(),
                out["stress_history"].data_ptr(), self._stream()), "trs_mw_step_stress")
            return
        _capi.check(self.lib.trs_mw_step(
            self.B, ws["cases"], ws["J"], self.nJ_max, self.nM_max, self.xyz.data_ptr(), self.conn.data_ptr(),
            self.E.data_ptr(), self.A.data_ptr(), self.rho.data_ptr(), self.free_index.data_ptr(), self.n_free.data_ptr(),
            self.nJ.data_ptr(), self.nM.data_ptr(), ws["F"].data_ptr(), self.rows, self.info.data_ptr(),
            ws["limit_case"].data_ptr(), ws["limit_joint"].data_ptr(), ws["limit_dir"].data_ptr(),
            ws["limit_value"].data_ptr(), _capi.MW_MEASURES[val["measure"]], val["move"], val["tol"], val["limit_tol"],
            val["sweeps"], _ptr(lo[0]), lo[1], _ptr(hi[0]), hi[1], it, mode, ws["prev"].data_ptr(), ws["mu"].data_ptr(),
            ws["st"].data_ptr(), self._active(ws, it), out["areas"].data_ptr(), out["measure"].data_ptr(),
            out["measure_history"].data_ptr(), out["worst_history"].data_ptr(), val["max_iters"] + 1,
            out["displacement"].data_ptr(), out["ratio"].data_ptr(), out["multipliers"].data_ptr(),
            _ptr(out.get("sensitivity")), self._stream()), "trs_mw_step")

    # -- tension-only and compression-only members: the active-set iteration on the device (include/trs_unilateral.h) ----
    def unilateral(self, kind, loads=None, prestrain=None, slack_factor=0.0, max_iters=20, check_every=1, state=None,
                   out=None):
        """One load case of the resident batch with members that carry tension only or compression only (cables, tie
        rods, counter-bracing, struts that bear against a seat), by the active-set iteration of include/trs_unilateral.h:
        analyse, switch off every unilateral member that is strained the wrong way, switch on every one that would be
        strained the right way, repeat until nothing changes.  `kind`: int8 device tensor [B, nM_max] of 0 (bilateral),
        +1 (tension-only) and -1 (compression-only); `loads`: float64 device tensor [B, nJ_max, 3] in the CALLER's joint
        numbering (None: the batch's own loads); `prestrain`: float64 [B, nM_max] member initial strains eps0 as
        `solve_effect_cases` takes them - pretension goes in as a negative eps0 -, or None; `slack_factor` >= 0: the
        fraction of its area a slack member keeps (0 removes it exactly); `max_iters` >= 0 rounds of flips at most;
        `state`: int8 [B, nM_max] initial state (1 active, 0 slack; None: all active; bilateral members are always
        active).  The nominal areas are the batch's own A at the call.  A member is active where kind e > 0 for
        e = c.(u_j1 - u_j0) - eps0 L0, the elongation beyond its stress-free length; the test is strict and has no
        threshold, and all flips of an analysis are made at once.  Per analysis five launches: `trs_assemble` and
        `trs_potrf_batched` of the effective areas, `trs_effects_rhs`, `trs_potrs_cases` and `trs_un_step`, which reads
        the reduced solution from the case block and writes the next state and the next effective areas.  A converged
        truss is frozen, as is one whose structure cannot be factored (`info != 0`: it goes back to the state before),
        so a truss's results depend neither on the others nor on `check_every` nor on `max_iters` beyond its own count.
        Every `check_every` analyses one int32 - the number of trusses still iterating - is downloaded to stop early.
        Where a truss ended with status 2 the final states are analysed once more (its slab held a failed factor);
        `trs_effects_recover` with the effective areas then gives the results.
        Returns a dict of device tensors: u, f_ext [B, nJ_max, 3] in the caller's numbering, N [B, nM_max], state (int8
        [B, nM_max]: 1 active, 0 slack and on the padding), status (int32 [B]: 0 converged, 1 iteration limit - the
        simultaneous flips can cycle -, 2 a structure could not be factored - with `slack_factor` 0 a joint can lose its
        last support), iterations, violations (int32 [B]: the members that still want to flip in the returned state; 0
        when converged), flips_history (int32 [B, max_iters + 1]: the flips of every analysis, zero beyond the truss's
        own count) and areas_effective [B, nM_max].  `self.info` holds 0, or for a truss of status 2 what the
        factorisation reported, latched.  Afterwards `self.A` holds the effective areas and the slab the factor of the
        final structure: `solve_cases`, `modes()` and the others may follow on "the structure with its slack cables
        off" without another `factor()`; `generation` is bumped.  To get the nominal areas back, keep a copy and hand it
        to `set_sections(A, E, rho)` - or read them from the packed batch.  A batch on the fused small-system path,
        `options["compact"]` and the table member form are refused, as in `sizing()`."""
        t = self.torch
        who = "unilateral()"
        self._refuse_iterated("unilateral")
        slack = _check_number(who, "slack_factor", slack_factor, "be a finite number >= 0", least=0)
        max_iters = _check_integer(who, "max_iters", max_iters, least=0)
        check_every = _check_integer(who, "check_every", check_every)
        given = {"kind": (kind, t.int8, "int8", [self.B, self.nM_max]), "state": (state, t.int8, "int8", [self.B, self.nM_max]),
                 "prestrain": (prestrain, t.float64, "float64", [self.B, self.nM_max]),
                 "loads": (loads, t.float64, "float64", [self.B, self.nJ_max, 3])}
        on = {}
        for name, (x, dtype, word, shape) in given.items():
            if x is None and name != "kind":
                on[name] = None
                continue
            if not hasattr(x, "data_ptr") or list(x.shape) != shape or x.dtype != dtype or x.device != self.device:
                raise ValueError(f"{who}: {name} must be {word} {shape} on {self.device}")
            on[name] = x.contiguous()
        if bool(((on["kind"] < -1) | (on["kind"] > 1)).any().item()):
            raise ValueError(f"{who}: kind must hold 0 (bilateral), 1 (tension-only) or -1 (compression-only)")
        H = max_iters + 1
        out = self._out_tensors("unilateral", _field_shapes(UnilateralResult.CASE_FIELDS, self.B, self._sizes(H=H)), out)
        if self.B == 0:
            return out
        if on["state"] is not None and on["state"].data_ptr() == out["state"].data_ptr():
            on["state"] = on["state"].clone()   # (the state written is zeroed first)
        self._begin_iterated("unilateral", (self.lib.trs_un_fits, "the step kernel (trs_un_fits)"),
                             (self.lib.trs_effects_fits, "the effect kernels (trs_effects_fits)"))
        ws = self._un_workspace(on, slack, max_iters, out)
        with t.cuda.device(self.device):
            self.dofmap()
            for key in ("state", "violations", "flips_history"):
                out[key].zero_()
            if on["state"] is not None:   # the structure of analysis 0 (all active: the nominal areas as they are)
                self.A.copy_(t.where((on["kind"] == 0) | (on["state"] != 0), ws["A_nom"], slack * ws["A_nom"]))
            it = self._iterate(ws, check_every, self._un_analyse, self._un_step)
            if bool((ws["st"][:, 0] == _capi.UN_NOT_PD).any().item()):
                # (that truss's slab holds the failed factor of a state it no longer has; the others get the same bits)
                self._un_analyse(ws)
                self._un_step(ws, it, 2)
            jo, stream, _ = self._case_launch()
            _capi.check(self.lib.trs_effects_recover(
                self.B, 1, self.nJ_max, self.nM_max, self.xyz.data_ptr(), *self._members(), self.rho.data_ptr(),
                ws["loads"].data_ptr(), _ptr(on["prestrain"]), None, None, self.free_index.data_ptr(), self.nJ.data_ptr(),
                self.nM.data_ptr(), ws["F"].data_ptr(), self.rows, out["u"].data_ptr(), out["f_ext"].data_ptr(),
                out["N"].data_ptr(), None, jo, stream), "trs_effects_recover")
            live = t.arange(self.nM_max, device=self.device)[None, :] < self.nM[:, None]
            out["areas_effective"].copy_(t.where(live, self.A, t.zeros_like(self.A)))
            self._end_iterated(ws, out)   # (the factor: of the final structure)
        return out

    # the stages of `unilateral` (tools/bench_unilateral.py times them one by one)
    def _un_workspace(self, on, slack, max_iters, out):
        """The state of a `unilateral` run: the nominal areas (a copy), the state before the last flips, the status words
        st [B, 4] and the `active` counters (one per analysis), zeroed; the case block; the loads in the caller's joint
        numbering (the batch's own are carried there through `joint_out`)."""
        t, dev = self.torch, self.device
        loads = self._own_loads() if on["loads"] is None else on["loads"]
        return self._run_state(max_iters, 1, loads.contiguous(), A_nom=self.A.clone(),
                               prev=t.zeros([self.B, max(self.nM_max, 1)], dtype=t.int8, device=dev), on=on, slack=slack,
                               out=out)

    def _un_analyse(self, ws):
        """Assembly and factorisation of the structure `self.A`, right-hand side (with the pre-strain loads of these
        areas) and substitution of the one case."""
        jo, stream, _ = self._case_launch()
        self.assemble()
        self.potrf()
        _capi.check(self.lib.trs_effects_rhs(
            self.B, 1, self.nJ_max, self.nM_max, self.xyz.data_ptr(), *self._members(), self.rho.data_ptr(),
            ws["loads"].data_ptr(), _ptr(ws["on"]["prestrain"]), None, None, self.free_index.data_ptr(),
            self.n_free.data_ptr(), self.nJ.data_ptr(), self.nM.data_ptr(), jo, ws["F"].data_ptr(), self.rows, stream),
            "trs_effects_rhs")
        self._potrs_cases(ws["F"], 1)

    def _un_step(self, ws, it, mode):
        on, out = ws["on"], ws["out"]
        _capi.check(self.lib.trs_un_step(
            self.B, self.nJ_max, self.nM_max, self.xyz.data_ptr(), self.conn.data_ptr(), self.A.data_ptr(),
            self.free_index.data_ptr(), self.n_free.data_ptr(), self.nJ.data_ptr(), self.nM.data_ptr(), ws["F"].data_ptr(),
            self.rows, self.info.data_ptr(), _ptr(on["prestrain"]), on["kind"].data_ptr(), ws["A_nom"].data_ptr(),
            ws["slack"], _ptr(on["state"]), it, mode, out["state"].data_ptr(), ws["prev"].data_ptr(), ws["st"].data_ptr(),
            self._active(ws, it), out["violations"].data_ptr(), out["flips_history"].data_ptr(), ws["limit"] + 1,
            self._stream()), "trs_un_step")

    # -- collapse load: elastic-plastic members, event to event on the device (include/trs_plastic.h) -------------------
    def plastic(self, cap_tension, cap_compression, loads=None, hardening=0.0, lambda_max=1.0, disp_limit=0.0,
                collapse_ratio=1e8, tie_tol=1e-9, max_events=64, check_every=1, out=None):
        """How much of one load pattern the trusses of the resident batch carry before they collapse, and in which order
        their members give way: the event-to-event elastic-plastic analysis of include/trs_plastic.h.  The pattern
        `loads` (float64 device tensor [B, nJ_max, 3] in the CALLER's joint numbering; None: the batch's own loads) is
        scaled by the load factor lambda; `cap_tension`, `cap_compression`: float64 device tensors [B, nM_max] of
        positive member capacities (forces; the padding is not looked at); `hardening` >= 0: the fraction of its
        stiffness a yielded member keeps (0: perfectly plastic, the member's area is scaled to exactly 0);
        `lambda_max` > 0 and `disp_limit` >= 0 (the largest |u_d| of a DOF; 0: none) end a run with status 0 and 3;
        `collapse_ratio` > 1: a tangent structure that moves more than this many times what the elastic one does per
        unit load is a mechanism that the factorisation let through on rounding noise (status 2 with info 0);
        `tie_tol` >= 0: members within this relative distance of the governing step yield with it in one event;
        `max_events` >= 0 events at most (status 1).  The nominal areas are the batch's own A at the call.  Every
        analysis finds the load increment at which the next elastic member reaches its capacity, advances the
        accumulated forces, displacements and load factor by it and lets that member yield: it goes on carrying its
        capacity while the rest picks up the difference.  A yielded member that would unload returns to elastic (an
        event of its own).  Per analysis five launches: `trs_assemble` and `trs_potrf_batched` of the effective areas,
        `trs_gather_cases`, `trs_potrs_cases` and `trs_pl_step`.  A truss that has ended is frozen, so a truss's results
        depend neither on the others nor on `check_every` nor on a larger `max_events`.  Every `check_every` analyses
        one int32 - the number of trusses still going - is downloaded to stop early.  `trs_pl_finish` then writes the
        results from the accumulated state; nothing is analysed again.
        Returns a dict of device tensors: u, f_ext [B, nJ_max, 3] in the caller's numbering (f_ext: lambda P at the free
        DOFs, the reactions at the held ones), N [B, nM_max], state (int8 [B, nM_max]: 0 elastic and on the padding, +1
        yielded in tension, -1 in compression), status (int32 [B]: 0 lambda_max reached, 1 event limit, 2 mechanism -
        the collapse load is `load_factor` -, 3 displacement limit), events (int32 [B]), load_factor [B], and per
        analysis k < max_events + 1 lambda_history, umax_history (the pushover curve), member_history (int32: the
        governing member, -1 a release, -2 the terminal analysis) and count_history (members yielded or released), zero
        beyond the truss's own count; areas_effective [B, nM_max].  `self.info` holds 0, or for a truss that ended as a
        mechanism because its tangent could not be factored what the factorisation reported, latched; the slab holds no
        valid factor of such a truss.  For every other truss `self.A` holds the effective areas and the slab their
        factor: `solve_cases` and the others may follow on the tangent structure without another `factor()`;
        `generation` is bumped.  A batch on the fused small-system path, `options["compact"]` and the table member form
        are refused, as in `sizing()`."""
        t = self.torch
        who = "plastic()"
        self._refuse_iterated("plastic", "load pattern")
        val = _check_plastic_scalars(who, hardening, lambda_max, disp_limit, collapse_ratio, tie_tol, max_events, check_every)
        given = {"cap_tension": (cap_tension, [self.B, self.nM_max]), "cap_compression": (cap_compression, [self.B, self.nM_max]),
                 "loads": (loads, [self.B, self.nJ_max, 3])}
        on = {}
        for name, (x, shape) in given.items():
            if x is None and name == "loads":
                on[name] = None
                continue
            if not hasattr(x, "data_ptr") or list(x.shape) != shape or x.dtype != t.float64 or x.device != self.device:
                raise ValueError(f"{who}: {name} must be float64 {shape} on {self.device}")
            on[name] = x.contiguous()
        live = t.arange(self.nM_max, device=self.device)[None, :] < self.nM[:, None]
        for name in ("cap_tension", "cap_compression"):
            if bool((live & ~((on[name] > 0) & t.isfinite(on[name]))).any().item()):
                raise ValueError(f"{who}: {name} must be positive and finite")
        H = val["max_events"] + 1
        out = self._out_tensors("plastic", _field_shapes(PlasticResult.CASE_FIELDS, self.B, self._sizes(H=H)), out)
        if self.B == 0:
            return out
        self._begin_iterated("plastic", (self.lib.trs_pl_fits, "the step kernel (trs_pl_fits)"))
        ws = self._pl_workspace(on, val, out)
        with t.cuda.device(self.device):
            self.dofmap()
            for key in ("N", "state", "lambda_history", "umax_history", "member_history", "count_history"):
                out[key].zero_()
            self._iterate(ws, val["check_every"], self._analyse_cases, self._pl_step)
            jo, stream, _ = self._case_launch()
            _capi.check(self.lib.trs_pl_finish(
                self.B, self.nJ_max, self.nM_max, self.xyz.data_ptr(), self.conn.data_ptr(), self.free_index.data_ptr(),
                self.n_free.data_ptr(), self.nJ.data_ptr(), self.nM.data_ptr(), self.rows, ws["loads"].data_ptr(),
                out["N"].data_ptr(), ws["U"].data_ptr(), ws["acc"].data_ptr(), jo, out["u"].data_ptr(),
                out["f_ext"].data_ptr(), stream), "trs_pl_finish")
            out["load_factor"].copy_(ws["acc"][:, 0])
            out["areas_effective"].copy_(t.where(live, self.A, t.zeros_like(self.A)))
            self._end_iterated(ws, out, count="events")   # (the factor: of the final tangent structure, where info is 0)
        return out

    # the stages of `plastic` (tools/bench_plastic.py times them one by one)
    def _pl_workspace(self, on, val, out):
        """The state of a `plastic` run: the nominal areas (a copy), the accumulated displacements U [B, 3 nJ_max] in the
        batch's joint order, acc [B, 4] (lambda, r_0, the largest |u_d|), the status words st [B, 4] and the `active`
        counters (one per analysis), zeroed; the case block; the load pattern in the caller's joint numbering (the
        batch's own is carried there through `joint_out`)."""
        t, dev = self.torch, self.device
        loads = self._own_loads() if on["loads"] is None else on["loads"]
        # (own=False: the pattern is in the caller's numbering either way; `_analyse_cases` gathers it through joint_in)
        return self._run_state(val["max_events"], 1, loads.contiguous(), A_nom=self.A.clone(),
                               U=t.zeros([self.B, 3 * self.nJ_max], dtype=t.float64, device=dev),
                               acc=t.zeros([self.B, 4], dtype=t.float64, device=dev), on=on, val=val, out=out)

    def _pl_step(self, ws, it, mode):
        on, val, out = ws["on"], ws["val"], ws["out"]
        _capi.check(self.lib.trs_pl_step(
            self.B, self.nJ_max, self.nM_max, self.xyz.data_ptr(), self.conn.data_ptr(), self.E.data_ptr(),
            self.A.data_ptr(), self.free_index.data_ptr(), self.n_free.data_ptr(), self.nJ.data_ptr(), self.nM.data_ptr(),
            ws["F"].data_ptr(), self.rows, self.info.data_ptr(), on["cap_tension"].data_ptr(),
            on["cap_compression"].data_ptr(), ws["A_nom"].data_ptr(), val["hardening"], val["lambda_max"],
            val["disp_limit"], val["collapse_ratio"], val["tie_tol"], it, mode, out["state"].data_ptr(),
            out["N"].data_ptr(), ws["U"].data_ptr(), ws["acc"].data_ptr(), ws["st"].data_ptr(),
            self._active(ws, it), out["lambda_history"].data_ptr(),
            out["member_history"].data_ptr(), out["count_history"].data_ptr(), out["umax_history"].data_ptr(),
            val["max_events"] + 1, self._stream()), "trs_pl_step")

    # -- linear buckling: critical load factors from shifted factors of K + theta Kg (include/trs_buckling.h) ------------
    def buckling(self, p, shift=0.0, max_shifts=6, tol=1e-10, max_iters=256, check_every=4, out=None):
        """Linear buckling of the resident batch under its own loads (`factor()` first; include/trs_buckling.h): the
        load factors lambda of K_ff phi = lambda H phi, H = -Kg the geometric stiffness of the linear member forces, and
        per truss the smallest positive one.  The linear solution comes from one substitution against the resident
        factor, `trs_bk_members` makes the member tables.  A round at the per-truss shift theta (round 0: `shift`) is
        `assemble` -> `trs_nl_tangent` with W(theta) -> `potrf` (the slab then holds a factor of K + theta Kg; round 0 at
        shift 0 takes the resident factor as it is) and the block iteration: per iteration `trs_potrs_cases` on 16
        vectors, `trs_bk_product`, `trs_bk_step`; every `check_every` iterations the residuals are formed, the trusses
        whose n_modes = min(p, rank) pairs nearest theta are below `tol` freeze, and one small read-back decides whether
        to go on, up to `max_iters`.  After a round a truss is done with its critical factor if its pairs hold a positive
        lambda, done without one if rank < p (the whole spectrum has been seen); otherwise all p pairs are negative, no
        eigenvalue lies within d = max |lambda_i - theta| of theta, and the next round runs at theta + d, `max_shifts`
        rounds at most.  The rounds' outputs are merged per truss on the device; one read-back per round.
        Returns a dict of device tensors: factor [B, p] (signed, nearest the final shift first, NaN beyond n_modes),
        critical [B] (NaN: none found), critical_mode [B] (int32, -1: none), bound [B] (every positive factor is >= bound;
        +inf: there is none; the critical factor where one was found), shift [B] (of the truss's last round), rounds [B],
        iters [B] (the iteration at which the last round converged, 0: it did not), residual [B, p], n_modes [B],
        shape [B, p, nJ_max, 3] (caller's numbering, largest component +1), status [B] (BK_FOUND 0, BK_NONE 1 no positive
        factor exists, BK_SHIFT_LIMIT 2, BK_ITER_LIMIT 3 the last round did not converge, BK_NOT_PD 4 the factorisation
        of K + theta Kg failed: the outputs of the previous round are kept) and info [B] (what the last factorisation of
        the truss reported; also left in `self.info`).  `max_shifts=1` with a caller's `shift` is the plain signed
        analysis at that shift.  Afterwards the batch is WITHOUT a static factor (the slab may hold a factor of
        K + theta Kg): the static analyses refuse with their "no factor" error until `factor()`; `generation` is bumped
        and the buffer of `solve_cases`' right-hand sides is reused, as `modes` does.  The compact member form of the
        assembly (`options["compact"]`) has no slab to amend and is refused, as is a batch on the fused small path."""
        t = self.torch
        self._need_slab("buckling", "leaves no slab that could be amended to K + theta Kg")
        _check_buckling_args(p, shift, max_shifts, tol, max_iters, check_every)
        self._need_factor("buckling")
        p, shift = int(p), float(shift)
        B, Q, dev = self.B, MODES_BLOCK, self.device
        shapes = _field_shapes(BucklingResult.FIELDS, B, self._sizes(P=p))
        shapes["info"] = ([B], t.int32)   # (what the truss's last factorisation reported: no field of the table)
        out = self._out_tensors("buckling", shapes, out)
        if B == 0:
            return out
        self._need_fit("buckling", self.lib.trs_bk_fits(self.nJ_max, self.nM_max)
                       and self.lib.trs_nl_fits(self.nJ_max, self.nM_max),
                       "the product or the amend kernel (trs_bk_fits, trs_nl_fits)")
        F = self.cases_F = self._case_block("cases_F", Q)   # the block's right-hand sides / solutions
        self._bump_generation()
        self._factored = False
        self._forward = None
        f64 = lambda *shape, fill=0.0: t.full(list(shape), fill, dtype=t.float64, device=dev)
        i32 = lambda *shape, fill=0: t.full(list(shape), fill, dtype=t.int32, device=dev)
        nM = max(self.nM_max, 1)
        nan, inf = float("nan"), float("inf")
        # (kept on the batch as `modes` keeps its own: tools/buckling_speed.py times the launches on it one by one)
        ws = self._bk_ws = {
              "X": f64(B, Q, self.rows), "G": f64(B, Q, self.rows), "Fk": f64(B, Q, self.rows), "lam": f64(B, Q, fill=nan),
              "resid": f64(B, Q, fill=nan), "rank": i32(B), "state": i32(B), "theta": f64(B, fill=shift),
              "u0": f64(B, 1, self.rows), "N": f64(B, nM), "ends": i32(B, nM, 2), "Mt": f64(B, nM, 4), "W": f64(B, nM, 6)}
        for key, fill, dtype, shape in BucklingResult.FIELDS.values():
            out[key].fill_(fill)
        out["shift"].fill_(shift)
        jo, stream, tab = self._case_launch()
        theta, state, rank = ws["theta"], ws["state"], ws["rank"]

        def step(first, check, it):
            _capi.check(self.lib.trs_bk_step(
                B, p, self.n_free.data_ptr(), theta.data_ptr(), F.data_ptr(), ws["G"].data_ptr(), ws["Fk"].data_ptr(),
                ws["X"].data_ptr(), self.rows, ws["lam"].data_ptr(), ws["resid"].data_ptr(), rank.data_ptr(),
                state.data_ptr(), first, check, it, float(tol), stream), "trs_bk_step")

        def product():
            _capi.check(self.lib.trs_bk_product(
                B, self.nJ_max, self.nM_max, ws["ends"].data_ptr(), ws["Mt"].data_ptr(), self.free_index.data_ptr(),
                self.n_free.data_ptr(), self.nJ.data_ptr(), self.nM.data_ptr(), F.data_ptr(), ws["G"].data_ptr(),
                self.rows, stream), "trs_bk_product")

        with t.cuda.device(dev):
            # the linear solution under the batch's own loads (already in the batch's joint order: no joint_in)
            self._gather_cases(self.loads, 1, ws["u0"], own=True)
            self._potrs_cases(ws["u0"], 1)
            active = t.ones([B], dtype=t.bool, device=dev)
            col = t.arange(p, device=dev)[None, :]
            for rnd in range(int(max_shifts)):
                _capi.check(getattr(self.lib, "trs_bk_members" + tab)(
                    B, self.nJ_max, self.nM_max, self.xyz.data_ptr(), *self._members(), self.free_index.data_ptr(),
                    self.n_free.data_ptr(), self.nJ.data_ptr(), self.nM.data_ptr(), ws["u0"].data_ptr(), self.rows,
                    theta.data_ptr(), ws["N"].data_ptr(), ws["ends"].data_ptr(), ws["Mt"].data_ptr(), ws["W"].data_ptr(),
                    stream), "trs_bk_members" + tab)
                if rnd > 0 or shift != 0.0:   # (round 0 at shift 0: the resident factor, no amend)
                    self.assemble()
                    self._nl_tangent(ws)
                    self.potrf()
                info = self.info.clone()
                took = active & (info == 0)
                state.copy_(t.where(took, 0, -1))
                self._block_iteration(F, step, state, int(max_iters), int(check_every), between=product)
                # the round's verdict per truss, merged into the outputs on the device
                conv = took & (state > 0)
                n_modes = rank.clamp(max=p)
                lam = ws["lam"][:, :p]
                valid = col < n_modes[:, None]
                pos = valid & (lam > 0) & conv[:, None]
                found = pos.any(1)
                crit, mode = t.where(pos, lam, inf).min(1)
                none = conv & ~found & (n_modes < p)
                negative = conv & ~found & ~none
                reach = t.where(valid, (lam - theta[:, None]).abs(), 0.0).max(1).values
                status = t.where(found, BK_FOUND, t.where(none, BK_NONE, t.where(negative, BK_SHIFT_LIMIT, BK_ITER_LIMIT)))
                status = t.where(took, status, BK_NOT_PD).to(t.int32)
                bound = t.where(found, crit, t.where(none, inf, t.where(negative, theta + reach, theta)))
                out["status"].copy_(t.where(active, status, out["status"]))
                out["rounds"].add_(active.to(t.int32))
                out["info"].copy_(t.where(active, info, out["info"]))
                out["shift"].copy_(t.where(took, theta, out["shift"]))
                out["bound"].copy_(t.where(took, bound, out["bound"]))
                out["critical"].copy_(t.where(found, crit, out["critical"]))
                out["critical_mode"].copy_(t.where(found, mode.to(t.int32), out["critical_mode"]))
                out["iters"].copy_(t.where(took, state.clamp(min=0), out["iters"]))
                active = negative
                theta.copy_(t.where(negative, theta + reach, theta))
                if rnd + 1 == max_shifts or not bool(active.any().item()):   # the one read-back per round
                    break
            _capi.check(self.lib.trs_bk_shapes(B, p, self.nJ_max, ws["X"].data_ptr(), self.rows,
                                               self.free_index.data_ptr(), self.n_free.data_ptr(), self.nJ.data_ptr(),
                                               rank.data_ptr(), jo, out["shape"].data_ptr(), stream), "trs_bk_shapes")
            n_modes = rank.clamp(max=p)
            valid = col < n_modes[:, None]
            out["factor"].copy_(t.where(valid, ws["lam"][:, :p], nan))
            out["residual"].copy_(t.where(valid, ws["resid"][:, :p], nan))
            out["n_modes"].copy_(n_modes)
            self.info.copy_(out["info"])
        return out

    def fitness(self, allow_stress, allow_displace, out=None):
        """(weight, stress_violation, displacement_violation) per truss, on device."""
        t = self.torch
        if self.table:
            raise ValueError("trs_fitness exists in the general member form only (the fused small-system kernel takes either)")
        if out is None:
            out = [t.empty([self.B], dtype=t.float64, device=self.device) for _ in range(3)]
        _capi.check(self.lib.trs_fitness(
            self.B, self.nJ_max, self.nM_max, self.xyz.data_ptr(), self.conn.data_ptr(),
            self.A.data_ptr(), self.rho.data_ptr(), self.nJ.data_ptr(), self.nM.data_ptr(),
            self.u.data_ptr(), self.N.data_ptr(), float(allow_stress), float(allow_displace),
            out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), self._stream()), "trs_fitness")
        return out

    def adopt_tile_hint(self):
        """After a solve (or an assembly) of the resident batch: read back whether ANY matrix left tiles of its
        envelope unwritten (one int per truss of the envelope metadata) and, if none did, tell the later assemblies
        of this topology not to form the tile masks again (`all_tiles`).  Synchronises.  Returns `all_tiles`."""
        if self.small or self.env is None or self.B == 0:
            return False
        off = 2 * (self.rows // 16) + self.rows // 64 + 8       # kmask[0] of every truss (csrc/trs_common.h)
        self.all_tiles = bool((self.env[:, off] == -1).all().item())
        return self.all_tiles

    @property
    def fields(self):
        """Names of this batch's per-truss input tensors (its member form's)."""
        return self.TABLE_FIELDS if self.table else self.INPUT_FIELDS

    def pinned_inputs(self, packed: PackedBatch):
        """Page-locked host copies of a batch's inputs (same padded shapes and member form as this device batch)."""
        t = self.torch
        if packed.is_table != self.table:
            raise ValueError("pinned_inputs: the batch's member form differs from the resident batch's")
        return {f: t.from_numpy(np.ascontiguousarray(getattr(packed, f))).pin_memory() for f in self.fields}

    def upload(self, host_inputs):
        """Replace the resident inputs by another batch of the same padded shapes (asynchronous on
        the current stream when `host_inputs` come from `pinned_inputs`)."""
        self.all_narrow = False   # another topology: the host's knowledge of the envelopes is gone
        self.all_tiles = False
        for f in self.fields:
            getattr(self, f).copy_(host_inputs[f], non_blocking=True)

    def download(self, out=None):
        """Copy the dense results to (pinned) host tensors, asynchronously; returns the dict."""
        t = self.torch
        if out is None:
            out = {k: t.empty(v.shape, dtype=v.dtype).pin_memory()
                   for k, v in (("u", self.u), ("f_ext", self.f_ext), ("N", self.N), ("info", self.info))}
        for k in out:
            out[k].copy_(getattr(self, k), non_blocking=True)
        return out

    def set_sections(self, A, E, rho):
        """Replace the member sections (host arrays [B,nM_max]); geometry stays resident."""
        if self.table:
            raise ValueError("set_sections: a batch in the table member form changes its sections through `types` / `type_idx`")
        for dst, src in ((self.A, A), (self.E, E), (self.rho, rho)):
            dst.copy_(self.torch.from_numpy(np.ascontiguousarray(src, dtype=np.float64)))

    def result(self):
        """Synchronise and download the dense results."""
        self.torch.cuda.synchronize(self.device)
        return BatchResult(self.u.cpu().numpy(), self.f_ext.cpu().numpy(), self.N.cpu().numpy(),
                           self.info.cpu().numpy())


class StreamedSolver:
    """Host -> device -> host pipeline for a stream of equally shaped batches (the feed of a resident
    solver over PCIe): the upload of batch k+1, the solve of batch k and the download of batch k-1 overlap
    on three HIP streams, with `slots` resident `DeviceBatch`es and page-locked staging buffers.

        pipe = StreamedSolver(template_packed)
        for packed in batches:                     # same padded shapes as the template
            done = pipe.submit(pipe.stage(packed)) # the results of the batch submitted `slots` calls ago, or None
            ...consume `done` here...
        for done in pipe.drain(): ...

    Results are views of page-locked output buffers (a ring of slots + 1): what `submit` returns stays
    valid until the NEXT call of `submit`; `drain` results until the pipe is used again.  Only what the
    solve reads is uploaded (`fields`; the densities are not part of `Truss.Solve()`)."""

    def __init__(self, template: PackedBatch, device=None, slots=2, use_envelope=True,
                 fields=("xyz", "conn", "E", "A", "cbits", "loads", "nJ", "nM"), same_topology=False):
        """`same_topology=True`: every batch of the stream has the template's connectivity and supports (only
        coordinates, sections and loads vary - a parameter study, a GA, a replicated benchmark batch), so the
        launch hints the host derived from the template's envelopes hold for all of them."""
        torch, dev = _require_gpu(device)
        self.torch, self.device, self.fields = torch, dev, tuple(fields)
        self.dev = [DeviceBatch(template, dev, use_envelope=use_envelope) for _ in range(slots)]
        if not same_topology:   # the batches that follow need not share the template's envelopes: no launch hints
            for d in self.dev:
                d.all_narrow = False

        # Every slot's uploaded fields live in ONE device buffer and ONE page-locked host buffer of the same
        # layout (likewise the four result fields), so that a batch crosses PCIe as one DMA per direction
        # instead of eight + four copies; the DeviceBatch tensors and the host dicts are views of them.
        def flat(like, pinned):
            offs, total = {}, 0
            for k, v in like.items():
                offs[k] = total
                total += (v.numel() * v.element_size() + 255) // 256 * 256
            buf = torch.empty([total], dtype=torch.uint8, pin_memory=True) if pinned else \
                torch.empty([total], dtype=torch.uint8, device=dev)
            views = {k: buf[offs[k]: offs[k] + v.numel() * v.element_size()].view(v.dtype).view(v.shape)
                     for k, v in like.items()}
            return buf, views

        self.host_in, self._host_in_flat, self._dev_in_flat = [], [], []
        self.host_out, self._host_out_flat, self._dev_out_flat = [], [], []
        for d in self.dev:
            ins = {f: getattr(d, f) for f in self.fields}
            dbuf, dviews = flat(ins, pinned=False)
            hbuf, hviews = flat(ins, pinned=True)
            for f in self.fields:
                dviews[f].copy_(ins[f])
                hviews[f].copy_(ins[f])
                setattr(d, f, dviews[f])
            outs = {k: getattr(d, k) for k in ("u", "f_ext", "N", "info")}
            obuf, oviews = flat(outs, pinned=False)
            for k in outs:
                setattr(d, k, oviews[k])
            self._dev_in_flat.append(dbuf); self._host_in_flat.append(hbuf); self.host_in.append(hviews)
            self._dev_out_flat.append(obuf)
        torch.cuda.synchronize(dev)
        like_out = {k: getattr(self.dev[0], k) for k in ("u", "f_ext", "N", "info")}
        for _ in range(slots + 1):
            hbuf, hviews = flat(like_out, pinned=True)
            self._host_out_flat.append(hbuf); self.host_out.append(hviews)
        self.s_up, self.s_run, self.s_down = (torch.cuda.Stream(dev) for _ in range(3))
        self.ev_up = [torch.cuda.Event() for _ in range(slots)]       # upload into device slot finished
        self.ev_run = [torch.cuda.Event() for _ in range(slots)]      # solve on device slot finished
        self.ev_down = [torch.cuda.Event() for _ in range(slots)]     # device slot's results downloaded
        self.count = 0
        self.pending = []   # (device slot, host buffer) of the downloads in flight, oldest first

    def stage(self, packed: PackedBatch):
        """Copy a batch's host arrays into the next slot's page-locked staging buffers."""
        slot = self.count % len(self.dev)
        self.ev_up[slot].synchronize()   # the previous upload out of this staging buffer has finished
        for f in self.fields:
            self.host_in[slot][f].numpy()[...] = getattr(packed, f)
        return self.host_in[slot]

    def submit(self, host_inputs=None):
        """Enqueue upload -> solve -> download of one batch (`host_inputs`: pinned tensors by field name,
        default: the slot's staging buffers).  Returns the `BatchResult` of the batch submitted `slots`
        calls ago (its download has finished), else None."""
        t = self.torch
        n = len(self.dev)
        slot, hbuf = self.count % n, self.count % (n + 1)
        self.count += 1
        done = self._take(self.pending.pop(0)) if len(self.pending) == n else None
        dev, src = self.dev[slot], host_inputs if host_inputs is not None else self.host_in[slot]
        own = [i for i, h in enumerate(self.host_in) if h is src]   # one of this pipe's own staging buffers?
        with t.cuda.stream(self.s_up):
            self.s_up.wait_event(self.ev_run[slot])     # the slot's previous solve no longer reads its inputs
            if own:   # one DMA for all fields
                self._dev_in_flat[slot].copy_(self._host_in_flat[own[0]], non_blocking=True)
            else:
                for f in self.fields:
                    getattr(dev, f).copy_(src[f], non_blocking=True)
            self.ev_up[slot].record(self.s_up)
        with t.cuda.stream(self.s_run):
            self.s_run.wait_event(self.ev_up[slot])
            self.s_run.wait_event(self.ev_down[slot])   # the slot's previous results have been downloaded
            dev.solve()
            self.ev_run[slot].record(self.s_run)
        with t.cuda.stream(self.s_down):
            self.s_down.wait_event(self.ev_run[slot])
            self._host_out_flat[hbuf].copy_(self._dev_out_flat[slot], non_blocking=True)   # one DMA for the four results
            self.ev_down[slot].record(self.s_down)
        self.pending.append((slot, hbuf))
        return done

    def _take(self, entry):
        slot, hbuf = entry
        self.ev_down[slot].synchronize()
        o = self.host_out[hbuf]
        return BatchResult(o["u"].numpy(), o["f_ext"].numpy(), o["N"].numpy(), o["info"].numpy())

    def drain(self):
        """Wait for everything in flight; the results of the batches not yet handed out, oldest first."""
        out = [self._take(e) for e in self.pending]
        self.pending = []
        return out


def rcm_permutation(packed: PackedBatch):
    """Reverse Cuthill-McKee joint order of every truss (native, `csrc/reorder.c`):
    perm[b, k] = old id of the joint that becomes joint k.  Shrinks the envelope of the reduced
    stiffness matrix of trusses that are not numbered along their long axis (cube trusses)."""
    perm = np.empty([packed.B, packed.nJ_max], dtype=np.int32)
    ptr = _hostapi.ptr
    conn, cbits, nJ, nM = (np.ascontiguousarray(a) for a in (packed.conn, packed.cbits, packed.nJ, packed.nM))
    _hostapi.check(_hostapi.load().trs_rcm_order(packed.B, packed.nJ_max, packed.nM_max,
                                                 ptr(conn), ptr(cbits), ptr(nJ), ptr(nM), ptr(perm)), "trs_rcm_order")
    return perm


def profile_permutation(packed: PackedBatch, return_choice=False, effort=2):
    """The cheapest of several candidate joint orders per truss (native, `csrc/reorder.c`
    `trs_profile_order`): reverse Cuthill-McKee, its reverse and twelve binned coordinate sweeps, priced
    by the 16x16-tile envelope the factorisation works in.  Never worse than `rcm_permutation` (efforts 0-2); on
    the reference's cube trusses 25-35 % less factorisation work.  perm[b, k] = old id of the joint that
    becomes joint k; `return_choice` adds the winning candidate's id per truss (0 = RCM).  `effort`: 0 RCM and
    its reverse, 1 + one sweep, 2 everything, 3 every sweep and the RCM pair only for trusses below 128 free joints."""
    perm = np.empty([packed.B, packed.nJ_max], dtype=np.int32)
    choice = np.empty([packed.B], dtype=np.int32)
    ptr = _hostapi.ptr
    xyz = np.ascontiguousarray(packed.xyz, dtype=np.float64)
    conn, nJ, nM = (np.ascontiguousarray(a, dtype=np.int32) for a in (packed.conn, packed.nJ, packed.nM))
    cbits = np.ascontiguousarray(packed.cbits, dtype=np.uint8)
    _hostapi.check(_hostapi.load().trs_profile_order(
        packed.B, packed.nJ_max, packed.nM_max, ptr(xyz), ptr(conn), ptr(cbits), ptr(nJ), ptr(nM), ptr(perm), ptr(choice),
        effort), "trs_profile_order")
    return (perm, choice) if return_choice else perm


def envelope_reach(packed: PackedBatch, perm=None):
    """Per truss, how many 16-row chunks the row envelope of K_ff reaches below its 64 x 64 diagonal blocks in
    the numbering given, or after the renumbering `perm` (native, `csrc/reorder.c`; the metadata `trs_assemble`
    derives on the device).  A batch that stays at or below `NARROW_MAX_BELOW` holds no matrix for the
    work-group kernels."""
    reach = np.empty([packed.B], dtype=np.int32)
    ptr = _hostapi.ptr
    conn, nJ, nM = (np.ascontiguousarray(a, dtype=np.int32) for a in (packed.conn, packed.nJ, packed.nM))
    cbits = np.ascontiguousarray(packed.cbits, dtype=np.uint8)
    pm = None if perm is None else np.ascontiguousarray(perm, dtype=np.int32)
    _hostapi.check(_hostapi.load().trs_envelope_reach(
        packed.B, packed.nJ_max, packed.nM_max, ptr(conn), ptr(cbits), ptr(nJ), ptr(nM), ptr(pm), ptr(reach)),
        "trs_envelope_reach")
    return reach


def joint_order(packed: PackedBatch, reorder):
    """The HOST-side permutation for a `reorder=` argument, with the same meaning of the names as `order_plan`:
    True / "auto" = `profile_permutation(effort=3)` (every sweep; Cuthill-McKee for small trusses), "profile" = every
    candidate for every truss, "fast" = one coordinate sweep instead of six (80 % of the gain for half the host
    time: what a host-in / host-out call wants when the order has to be found on the host, where it is the longest
    step), "rcm" = `rcm_permutation`; an int32 array [B, nJ_max] found earlier (e.g. on another thread) passes
    through."""
    if isinstance(reorder, np.ndarray):
        if reorder.shape != (packed.B, packed.nJ_max):
            raise ValueError(f"joint order of shape {reorder.shape}, expected {(packed.B, packed.nJ_max)}")
        return np.ascontiguousarray(reorder, dtype=np.int32)
    if reorder == "fast":
        return profile_permutation(packed, effort=1)
    if reorder == "rcm":
        return rcm_permutation(packed)
    if reorder is True or reorder == "auto":
        return profile_permutation(packed, effort=3)
    if reorder == "profile":
        return profile_permutation(packed)
    raise ValueError(f"unknown joint order {reorder!r} (True, 'auto', 'profile', 'fast', 'rcm' or a permutation array)")


def permute_joints(packed: PackedBatch, perm):
    """The same trusses with joint k := old joint perm[b, k] (members keep their order).
    Native (`csrc/reorder.c`, OpenMP over the batch)."""
    B, nJ_max, nM_max = packed.B, packed.nJ_max, packed.nM_max
    src = [np.ascontiguousarray(a, dtype=t) for a, t in (
        (perm, np.int32), (packed.nM, np.int32), (packed.xyz, np.float64), (packed.conn, np.int32),
        (packed.cbits, np.uint8), (packed.loads, np.float64))]
    xyz, conn = np.empty_like(src[2]), np.empty_like(src[3])
    cbits, loads = np.empty_like(src[4]), np.empty_like(src[5])
    ptr = _hostapi.ptr
    _hostapi.check(_hostapi.load().trs_apply_joint_order(
        B, nJ_max, nM_max, *(ptr(a) for a in src), ptr(xyz), ptr(conn), ptr(cbits), ptr(loads)), "trs_apply_joint_order")
    return PackedBatch(xyz, conn, packed.E, packed.A, packed.rho, cbits, loads, packed.nJ, packed.nM,
                       packed.dim, packed.n_free)


def global_stiffness(trusses_or_packed, device=None):
    """The FULL global stiffness matrix of every truss, `Truss.GetKMatrix()` of the reference
    (`truss.py:307-316`: zero-initialised nDOF x nDOF, four dim x dim blocks added per member, DOF = joint * dim
    + axis, parallel members accumulate), assembled on the GPU by the same kernel as the solve: `trs_dofmap`
    on a batch with NO constraint frees every DOF (reduced index = DOF index) and `trs_assemble` with
    TRS_ASM_FULL_SYMMETRIC and no envelope writes the whole symmetric matrix.  Returns a list of B dense
    `np.ndarray`s of shape `[nJoint * dim, nJoint * dim]` (a 2D truss drops the embedded z axis)."""
    if not isinstance(trusses_or_packed, PackedBatch) and len(trusses_or_packed) == 0:
        return []
    packed = trusses_or_packed if isinstance(trusses_or_packed, PackedBatch) \
        else pack_trusses(list(trusses_or_packed))
    if packed.B == 0:
        return []
    torch, dev = _require_gpu(device)
    import dataclasses
    free = dataclasses.replace(packed, cbits=np.zeros_like(packed.cbits), n_free=(3 * packed.nJ).astype(np.int32))
    out = []
    # one slab per truss is nDOF^2 doubles: a few trusses at a time keep the workspace below ~1 GiB
    per = max(1, int((1 << 30) // max(1, (3 * packed.nJ_max + 80) ** 2 * 8)))
    with torch.cuda.device(dev):
        for lo in range(0, packed.B, per):
            part = free.take(np.arange(lo, min(packed.B, lo + per)))
            db = DeviceBatch(part, dev, use_envelope=False, use_small=False)
            db.dofmap()
            db.assemble(flags=ASM_FULL_SYMMETRIC)
            torch.cuda.synchronize(dev)
            S = db.S.cpu().numpy()
            for b in range(part.B):
                nJ, dim = int(part.nJ[b]), int(part.dim[b])
                K = S[b, :3 * nJ, :3 * nJ]
                if dim == 2:
                    keep = (np.arange(3 * nJ) % 3) < 2
                    K = K[keep][:, keep]
                out.append(np.ascontiguousarray(K))
            del db
    return out


SMALL_N = 128  # largest reduced system of the fused small-system kernel (csrc/small.hip)


def size_buckets(packed: PackedBatch, max_slab_bytes=64 << 30, granularity=64, quantum=0, span=2):
    """Group the trusses of a ragged batch for launching.  Returns a list of index arrays (their union
    is range(B)).

    * Every truss with at most SMALL_N free DOFs goes into ONE group when that group qualifies for the
      fused small-system kernel (`trs_solve_small_fits` on the group's own maxima): that kernel sizes
      its work per truss, so nothing is gained by splitting it.
    * The others are grouped by system size rounded up to `granularity` (a multiple of 64, the padded
      size n_pad: the slab and every work-group of a launch are then uniform), at most `max_slab_bytes`
      of stiffness slab per launch.
    * `quantum` > 0 (resident solvers: the matrices the factorisation kernel holds in flight, 12 per CU): the
      groups are cut at WHOLE ROUNDS of that kernel instead - the trusses in descending size, a group takes
      trusses of up to `span` further size classes below its largest and, where it can, a multiple of `quantum`
      of them.  A class of 3176 matrices runs 104 of them in a second round of their own; 65 536 cube trusses
      take 47.4 instead of 48.6 ms per step in ten groups instead of fourteen (`tools/round_buckets.py`).  The
      kernels work on every truss by its own size, so the results do not depend on the grouping."""
    g = max(64, int(granularity) // 64 * 64)
    n_pad = (packed.n_free.astype(np.int64) + g - 1) // g * g
    groups = []
    small = np.flatnonzero(packed.n_free <= SMALL_N)
    taken = np.zeros(packed.B, dtype=bool)
    # (with `quantum` also when they are of one size class: a bucket that spans further classes would take them through
    # the staged kernels, whose rounding differs from the small-system kernel's in the last bit - which kernel solves a
    # truss must not depend on how the batch is grouped, `tools/fuzz_streamed.py`)
    if len(small) and (quantum > 0 or len(np.unique(n_pad[small])) > 1):
        try:
            fits = _capi.load().trs_solve_small_fits(int(packed.nJ[small].max()), int(packed.nM[small].max()),
                                                     int(packed.n_free[small].max()))
        except HipExtensionError:
            fits = 0
        if fits:
            groups.append(small)
            taken[small] = True
    slab_bytes = lambda size: max(1, int(size) * (int(size) + 16) * 8)
    if quantum > 0:
        rest = np.flatnonzero(~taken)
        rest = rest[np.argsort(-n_pad[rest], kind="stable")]
        i = 0
        while i < len(rest):
            top = int(n_pad[rest[i]])
            cap = max(1, max_slab_bytes // slab_bytes(top))
            in_span = int(np.searchsorted(-n_pad[rest[i:]], -(top - g * max(0, int(span))), side="right"))
            take = min(cap, in_span)
            if take >= quantum:
                take = take // quantum * quantum
            # inside a group by ascending size: the factorisation takes its matrices from the last to the first, so
            # the largest start first and the chip empties over the smallest (47.2 against 48.5 ms per cube step)
            sl = np.sort(rest[i:i + take])
            sl = sl[np.argsort(packed.n_free[sl], kind="stable")]
            groups.append(sl)
            i += take
        return groups
    for size in np.unique(n_pad[~taken]):
        idx = np.flatnonzero((n_pad == size) & ~taken)
        step = max(1, max_slab_bytes // slab_bytes(size))
        groups.extend(idx[i: i + step] for i in range(0, len(idx), step))
    return groups


class SolverWorkspace:
    """Grow-only device buffers for the bucket pipelines of `RaggedSolver`s that run one after the other on one
    stream (slab, reduced vectors, assembly tables, envelope metadata, gathered un-ordered inputs): several
    solvers - the pieces of `solve_batch_streamed` - share one instead of allocating their own."""

    KINDS = {"S": "float64", "uf": "float64", "work": "uint8", "env": "int32", "raw_xyz": "float64",
             "raw_loads": "float64", "raw_cbits": "uint8", "raw_conn": "int32"}

    def __init__(self, torch, device):
        self.torch, self.device, self.buf = torch, device, {}
        self._lanes = {}

    def lane(self, index):
        """The workspace of lane `index` of a `RaggedSolver` that deals its buckets onto several streams (lane 0 is
        this workspace; the others are created on first use and live as long as it does)."""
        if index == 0:
            return self
        if index not in self._lanes:
            self._lanes[index] = SolverWorkspace(self.torch, self.device)
        return self._lanes[index]

    def nbytes(self):
        """Bytes this workspace and its lanes hold now."""
        own = sum(int(b.numel() * b.element_size()) for b in self.buf.values() if b is not None)
        return own + sum(ws.nbytes() for ws in self._lanes.values())

    def get(self, need):
        """Flat tensors of at least `need[kind]` elements each (zero-filled for the envelope metadata)."""
        t = self.torch
        grow = {kind: int(count) for kind, count in need.items()
                if self.buf.get(kind) is None or self.buf[kind].numel() < count}
        regrown = [kind for kind in grow if self.buf.get(kind) is not None]
        if regrown:
            # buffers that have to grow are dropped first and come back with headroom: a stream of batches of
            # slightly different shapes settles after a few steps.  The caching allocator keeps the dropped
            # blocks for other tensors; they go back to the driver only when the device is short of memory
            # (`empty_cache` costs a second with a hundred GB cached - never on the ordinary path)
            for kind in regrown:
                self.buf[kind] = None
                grow[kind] += grow[kind] // 8
            wanted = sum(grow[k] * t.empty((), dtype=getattr(t, self.KINDS[k])).element_size() for k in grow)
            free, _ = t.cuda.mem_get_info(self.device)
            reusable = t.cuda.memory_reserved(self.device) - t.cuda.memory_allocated(self.device)
            if free + reusable // 2 < wanted:
                t.cuda.empty_cache()
        for kind, count in grow.items():
            make = t.zeros if kind == "env" else t.empty
            self.buf[kind] = make([max(1, count)], dtype=getattr(t, self.KINDS[kind]), device=self.device)
            if kind == "S" and os.environ.get("TRS_DEBUG_POISON"):
                self.buf[kind].fill_(float("nan"))
        return self.buf


def default_slab_budget(torch, device, n_lanes, workspace=None):
    """Slab bytes a resident `RaggedSolver` may spread over its lanes when the caller names no budget:
    `LANE_SLAB_BYTES` per lane, but never more than 60 % of the device's memory and never more than 85 % of what is
    FREE now plus what the solver's own workspace (and this process's cached, unused blocks) already holds - a
    co-tenant of the device, e.g. the network being trained on the samples, keeps its memory; at least 2 GiB, so that a
    crowded device gives small buckets rather than none."""
    total = int(torch.cuda.get_device_properties(device).total_memory)
    free, _ = torch.cuda.mem_get_info(device)
    reusable = int(torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device))
    held = workspace.nbytes() if workspace is not None else 0
    roomy = int(0.85 * (int(free) + reusable + held))
    return max(2 << 30, min(n_lanes * LANE_SLAB_BYTES, int(0.6 * total), roomy))


_SHARED_WORKSPACES = {}
_LANE_STREAMS = {}
#: streams a resident `RaggedSolver` deals its buckets onto unless told otherwise (`lanes=`), and the slab budget per lane
DEFAULT_LANES = 4
LANE_SLAB_BYTES = 36 << 30
#: run streams of the host-fed pipeline (`RaggedSolver(host_io=...)`, `solve_batch_streamed`).  ONE: with two to four the
#: call is no shorter (67.2 / 67.9 / 67.8 ms per 65 536 cube trusses, EXPERIMENTS R6.4) - the run stream is busy from
#: the first pull to the last solve either way, and what bounds the call is that device work on the 232 CUs the copy
#: kernels leave it; `lanes=` stays for other shapes of batch
HOSTFED_LANES = int(os.environ.get("TRS_HOSTFED_LANES", "1"))


def lane_streams(torch, device, count):
    """`count` side streams of `device` for the extra lanes of `RaggedSolver`s (made once per process and device:
    every solver's step forks from and joins the caller's stream, so sharing them only serialises what two callers
    put on the same lane)."""
    have = _LANE_STREAMS.setdefault(str(device), [])
    while len(have) < count:
        have.append(torch.cuda.Stream(device=device))
    return have[:count]


def shared_workspace(torch, device):
    """The process's `SolverWorkspace` of (`device`, CURRENT STREAM) for bucket pipelines that run one after the
    other on that stream (the chunks of `data.dataset_chunks`): one slab for all of them instead of one per call.
    The buffers are re-used without any synchronisation of their own - stream order is the only thing that keeps
    one call's factorisation from the next call's assembly -, hence one workspace per stream: calls issued on
    different streams of a device (or from threads with different current streams) get different buffers.  Two
    threads that drive the SAME stream must serialise their calls themselves, as for any other stream-ordered
    resource.

    The cache is BOUNDED: at most `MAX_SHARED_WORKSPACES` (4; a workspace is up to tens of GB) live at a time PER DEVICE,
    the device's least recently used one is dropped when a further stream of it asks (its buffers go back to the caching allocator once
    the solvers built on it are gone; kernels still queued on them keep them alive through the allocator's
    stream-ordered reuse, as for any freed tensor).  A stream handle value that comes back after its stream was
    destroyed inherits the old entry - harmless: a destroyed stream has no work left, and the buffers carry no state
    between calls."""
    key = (str(device), int(torch.cuda.current_stream(device).cuda_stream))
    ws = _SHARED_WORKSPACES.pop(key, None)
    if ws is None:
        ws = SolverWorkspace(torch, device)
        # The bound is PER DEVICE (a process that drives eight devices in turn keeps every device's workspaces).
        # Dropping a workspace also drops its lanes' buffers, which were allocated on the caller's stream and used on
        # the side streams of the lanes: that is safe only because `RaggedSolver.step` always JOINS its lanes back into
        # the caller's stream before it returns - every use of a lane buffer is ordered before whatever the caller's
        # stream does next, the allocator's stream-ordered reuse included.
        mine = [k for k in _SHARED_WORKSPACES if k[0] == key[0]]       # (dicts keep insertion order: oldest use first)
        for old_key in mine[:max(0, len(mine) - MAX_SHARED_WORKSPACES + 1)]:
            _SHARED_WORKSPACES.pop(old_key)
    _SHARED_WORKSPACES[key] = ws                                       # most recently used last
    return ws


MAX_SHARED_WORKSPACES = 4


def release_workspaces():
    """Drop the shared workspaces of every device and stream (they hold the largest slabs a call needed - up to
    `default_slab_budget`, i.e. up to 60 % of a device's memory over the lanes - for the life of the process) and hand
    the cached blocks back to the driver."""
    import torch
    _SHARED_WORKSPACES.clear()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


class _MaskedStreams:
    """The three streams of the host-fed pipeline with their compute units set apart (`trs_stream_create_masked`):
    pull and push get CUs of their own - consecutive mask bits go round the XCDs, so eight are one CU of every
    XCD - and the solver kernels the rest."""

    def __init__(self, torch, dev, lib, pull_cus, push_cus):
        import ctypes
        n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
        if not (pull_cus > 0 and push_cus > 0 and pull_cus + push_cus < n_cu):
            raise ValueError(f"cannot set {pull_cus} + {push_cus} copy CUs apart on a device with {n_cu}")
        words = (n_cu + 31) // 32
        sets = (range(0, pull_cus), range(pull_cus + push_cus, n_cu), range(pull_cus, pull_cus + push_cus))   # pull, run, push
        self.lib, self.handles, self.streams = lib, [], []
        self.torch, self.dev = torch, dev
        with torch.cuda.device(dev):
            try:
                for k, cus in enumerate(sets):
                    mask = (ctypes.c_uint32 * words)()
                    for c in cus:
                        mask[c // 32] |= 1 << (c % 32)
                    if k == 1:
                        self.run_mask = mask
                    handle = ctypes.c_void_p()
                    _capi.check(lib.trs_stream_create_masked(mask, words, ctypes.byref(handle)), "trs_stream_create_masked")
                    self.handles.append(handle)
                    self.streams.append(torch.cuda.ExternalStream(handle.value, device=dev))
                self.runs = [self.streams[1]]
            except Exception:
                self.close()   # (a runtime that refuses the 2nd or 3rd mask must not leak the streams made so far)
                raise

    def __iter__(self):
        return iter(self.streams[:3])

    def run_streams(self, count):
        """`count` run streams on the solver kernels' CU set (the first is the pipeline's own; more are made on demand
        and kept): the run lanes of a host-fed `RaggedSolver`."""
        import ctypes
        while len(self.runs) < count:
            handle = ctypes.c_void_p()
            with self.torch.cuda.device(self.dev):
                _capi.check(self.lib.trs_stream_create_masked(self.run_mask, len(self.run_mask), ctypes.byref(handle)),
                            "trs_stream_create_masked")
            self.handles.append(handle)
            self.runs.append(self.torch.cuda.ExternalStream(handle.value, device=self.dev))
        return self.runs[:count]

    def close(self):
        """Destroy the streams (after the work queued on them has finished).  The pipeline's own set is created
        once per process and device and lives as long as the process."""
        self.torch.cuda.synchronize(self.dev)
        for handle in self.handles:
            _capi.check(self.lib.trs_stream_destroy(handle), "trs_stream_destroy")
        self.handles, self.streams, self.runs = [], [], []


def _flow_shop_order(groups, packed, n_pad_of, rule="johnson"):
    """Order of the buckets in the host-fed pipeline.  Every bucket is pulled over PCIe, then solved; the link and
    the chip each take the buckets one after the other - a two-machine flow shop, for which Johnson's rule gives the
    shortest makespan: first the buckets that take longer to solve than to pull, by increasing pull time (the chip
    starts early and never runs dry), then the others by decreasing solve time (what is left exposed at the end
    is the smallest solve).  The two times are estimates - live input bytes at the rate a pull reaches beside the
    solves, and count x n_pad^2 at the rate the factorisation of cube trusses runs at - and only their ratio
    matters.  Small buckets are link-bound, large ones chip-bound; smallest-first (`rule="small"`) leaves the chip
    waiting in the first third of the step and the link idle in the last."""
    if rule == "small":
        return sorted(groups, key=lambda idx: len(idx) * n_pad_of(idx) ** 2), 0
    if rule == "large":
        return sorted(groups, key=lambda idx: -len(idx) * n_pad_of(idx) ** 2), len(groups)
    nJ, nM = packed.nJ.astype(np.int64), packed.nM.astype(np.int64)
    pull = lambda idx: float((nJ[idx] * 49 + nM[idx] * 24).sum()) / 45e9
    solve = lambda idx: len(idx) * float(n_pad_of(idx)) ** 2 * 2.0e-12
    chip_bound = sorted((g for g in groups if pull(g) < solve(g)), key=pull)
    link_bound = sorted((g for g in groups if pull(g) >= solve(g)), key=lambda g: -solve(g))
    return chip_bound + link_bound, len(chip_bound)


def _pipeline_streams(torch, dev, lib):
    """(pull, run, push) streams of `RaggedSolver`'s host-fed pipeline.  By default the copy kernels get compute units
    of their own through CU-masked streams (`TRS_PCIE_CUS="pull,push"`, default "16,8" = two CUs per XCD for the pull,
    one for the push: the row copies reach the link's rate on those, `tools/masked_pipeline_check.py`) and the solver
    kernels the rest - 73 instead of 91 ms per host-fed call of the 65 536-truss cube batch, because the copies no
    longer compete with the factorisation for registers on every CU.  `TRS_PCIE_CUS=0` = three ordinary streams.
    (Round 4 had to make the masks opt-in: processes using them died of memory access faults or hung once in five
    runs of the host-fed tests.  That was the joint-order kernel's race, which any concurrent kernel could bring out -
    EXPERIMENTS R5.1; with it fixed, 36 of 36 runs of those tests with the masks passed.)"""
    spec = os.environ.get("TRS_PCIE_CUS", "16,8")
    key = (str(dev), spec)
    if key not in _PIPELINE_STREAMS:   # (a queue with a CU mask takes ~20 ms to create: once per process and device)
        pull_cus, push_cus = int(spec.split(",")[0]), int(spec.split(",")[-1])
        n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
        if pull_cus <= 0 or 2 * (pull_cus + push_cus) > n_cu:   # (a partitioned or small device: no CUs to spare)
            _PIPELINE_STREAMS[key] = (torch.cuda.Stream(dev), torch.cuda.Stream(dev), torch.cuda.Stream(dev))
        else:
            try:
                _PIPELINE_STREAMS[key] = _MaskedStreams(torch, dev, lib, pull_cus, push_cus)
            except HipExtensionError as exc:   # (a runtime that refuses CU masks: the pipeline still works, slower)
                import warnings
                warnings.warn(f"CU-masked streams are not available ({exc}); the host-fed pipeline uses ordinary streams")
                _PIPELINE_STREAMS[key] = (torch.cuda.Stream(dev), torch.cuda.Stream(dev), torch.cuda.Stream(dev))
    return _PIPELINE_STREAMS[key]


_PIPELINE_STREAMS = {}


class RaggedSolver:
    """A RAGGED batch (trusses of very different sizes: the reference's `GenerateRandomCubeTrusses` loop,
    `generate.py:342-374`, BASELINE config 3) resident on one device in the caller's order and numbering, set
    up once and solved any number of times with everything on the GPU.  Per size bucket (`size_buckets`):

        gather the bucket's rows, trimmed to its own maxima (`trs_copy_rows`)
        -> joint order of the bucket (`trs_joint_order`: found, applied and priced on the device; its LDS tables
           are sized by the BUCKET's maxima, so buckets of small trusses run more work-groups per CU)
        -> `trs_solve`
        -> scatter u / f_ext / N / info back to the caller's rows (`trs_copy_rows`)

    The buckets share ONE workspace (slab, reduced vectors, assembly tables, envelope metadata, the gathered
    un-ordered inputs) sized for the largest of them; their launches follow each other on the current stream.
    Results stay resident (`u`, `f_ext`, `N`, `info`: full-batch tensors in the caller's numbering) until
    `result()` downloads them.  `reorder` as `order_plan`; a host-side plan is carried out once, at set-up."""

    GATHER = ("xyz", "conn", "E", "A", "cbits", "loads", "nJ", "nM")
    GATHER_TABLE = ("xyz", "conn", "type_idx", "cbits", "loads", "nJ", "nM")   # table member form (`PackedBatch.table`)
    JOINT_ORDERED = ("xyz", "conn", "cbits", "loads")

    def __init__(self, packed, device=None, reorder=True, max_slab_bytes=None, granularity=64,
                 options=None, tensors=None, workspace=None, host_io=None, n_variants=1, lanes=None):
        """`packed`: a `PackedBatch` (uploaded here) or, with `tensors` = the batch's device tensors by field name
        (e.g. from `generate.generate_cube_batch_device`), just its `BatchSizes`.  `workspace`: a
        `SolverWorkspace` shared with other solvers that run on the same stream one after the other.

        `lanes` (default `DEFAULT_LANES` = 4; resident batches only): the buckets are dealt onto that many streams -
        lane 0 is the caller's stream, the others fork from it at the start of `step()` and join it at the end, so
        a step still is ONE stream-ordered operation for the caller -, each lane with a workspace of its own, so that
        one bucket's kernels fill the emptying-chip tails and the latency-bound phases of another's: 46.7 -> 43.8 ms
        per step of the 65 536-truss cube batch.  Results are bit for bit those of one lane (asserted step by step:
        `tests/test_gpu_streams.py`).  Rounds 3-4 had to keep this switched off - stalls and bursts of corrupted
        trusses once in a few dozen steps; the cause was a race in `trs_joint_order`'s kernel that only concurrent
        kernels brought out, found with the torch-free reproducer `tools/repro_streams.cpp` (EXPERIMENTS R5.1).
        `max_slab_bytes` (default `default_slab_budget`: `LANE_SLAB_BYTES` = 36 GiB per lane, at most 60 % of the
        device's memory and 85 % of what is free on it now) is the budget of all lanes together.

        `host_io=(inputs, outputs)`: the batch STAYS in page-locked host memory - `inputs` / `outputs` are dicts of
        pinned CPU tensors (the padded arrays of a `PackedBatch.pinned()`; `u`, `f_ext`, `N`, `info` of a
        `ResultPool`).  Page-locked memory is mapped into the device's address space, so every bucket's gather
        PULLS its rows straight out of the host batch and its scatter PUSHES the results into the host arrays
        (full rows, zero padding included); `step()` then runs the buckets as a three-stream pipeline - pull of
        bucket k + 1, device work of bucket k, push of bucket k - 1 at the same time (`solve_batch_streamed`).

        `n_variants` > 1: every step solves the batch that many times with different member sections
        (`step(sections=[...])`, as `solve_batch(sections=...)`): gather and joint order once per bucket, one result
        set per variant in `outs` (`u` / `f_ext` / `N` / `info` are the first variant's)."""
        torch, dev = _require_gpu(device if tensors is None else tensors["xyz"].device)
        self.torch, self.device, self.packed, self.lib = torch, dev, packed, _capi.load()
        B, nJ_max, nM_max = packed.B, packed.nJ_max, packed.nM_max
        self.B = B
        self.host_io = host_io is not None
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        #: table member form (uint16 end joints, a uint8 type index per member, one type table for the batch): the
        #: batch's own form - a `PackedBatch.table()`, host_io inputs or device tensors that carry `type_idx`
        source = host_io[0] if self.host_io else tensors
        self.table = (source.get("type_idx") is not None) if source is not None else bool(getattr(packed, "is_table", False))
        gather = self.GATHER_TABLE if self.table else self.GATHER
        self.types = None
        self._fixed_types = {}   # type tables of fixed-section variants (`_section_types`), by (a, e, density)
        if self.table:
            types = source.get("types") if source is not None and source.get("types") is not None else getattr(packed, "types", None)
            if types is None:
                raise ValueError("table member form: the type table `types` [T, 3] is missing")
            self.types = (types if torch.is_tensor(types) else torch.from_numpy(np.ascontiguousarray(types, dtype=np.float64))).to(dev)
        if self.host_io:
            # (the sizes nJ / nM come from `packed` and go up once, with the bucket index lists: they tell the copy
            # kernels how much of a row is live, so that nothing but live bytes crosses the link)
            self.gather_fields = tuple(f for f in gather if f not in ("nJ", "nM"))
            self.inputs = {f: host_io[0][f] for f in self.gather_fields}
            if not all(t.is_pinned() and t.is_contiguous() for t in self.inputs.values()):
                raise ValueError("host_io inputs must be contiguous page-locked tensors (PackedBatch.pinned())")
        else:
            self.gather_fields = gather
            self.inputs = {f: (tensors[f].contiguous() if tensors is not None else up(getattr(packed, f))) for f in gather}
        plan = order_plan(reorder, nJ_max, nM_max) if B else None
        self.plan = plan
        # A batch whose LARGEST truss does not fit `trs_joint_order` gets a host plan - but its buckets are ordered
        # one by one with tables sized by the bucket, so every bucket that fits is still ordered on the device
        # (unless the caller forced a host order or gave a permutation).
        self.device_effort = plan[1] if plan is not None and plan[0] == "device" else None
        if plan is not None and plan[0] == "host" and (reorder is True or reorder in ("auto", "profile", "fast")):
            self.device_effort = {"fast": 1, "profile": 2}.get(reorder, 3)
        self.ordered = None        # host plan: renumbered xyz / conn / cbits / loads + perm of the FULL batch
        if plan is not None and plan[0] != "device":
            # (found for the whole batch: the buckets that do not fit the device kernel take their rows from it)
            host = (packed if isinstance(packed, PackedBatch) else packed.to_packed(tensors)).general()
            perm = joint_order(host, plan[1])
            renum = permute_joints(host, perm)
            self.ordered = {k: up(getattr(renum, k)) for k in self.JOINT_ORDERED}
            if self.table:
                self.ordered["conn"] = up(np.ascontiguousarray(renum.conn, dtype=np.uint16))
            self.ordered["perm"] = up(perm)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)   # padding beyond a bucket's width stays 0
        if self.host_io:
            out = host_io[1]
            self.u, self.f_ext, self.N, self.info = out["u"], out["f_ext"], out["N"], out["info"]
            want = {"u": (B, nJ_max, 3), "f_ext": (B, nJ_max, 3), "N": (B, nM_max), "info": (B,)}
            if not all(out[k].is_pinned() and out[k].is_contiguous() and tuple(out[k].shape) == want[k] for k in want):
                raise ValueError("host_io outputs must be contiguous page-locked tensors of the padded result shapes")
            # `live` (optional): per result array a device int32 [B] "row r is zero behind byte live[r]"
            # (`ResultPool.take_tracked`); without it every push zero-fills its rows to their full width
            self.live = dict(out.get("live") or {})
            if any(t.device != dev or t.dtype != torch.int32 or tuple(t.shape) != (B,) for t in self.live.values()):
                raise ValueError("host_io live extents must be int32 [B] tensors on the solver's device")
            if n_variants != 1:
                raise ValueError("the host-fed pipeline solves one set of sections per step")
            self.outs = [{"u": self.u, "f_ext": self.f_ext, "N": self.N, "info": self.info}]
        else:
            self.outs = [{"u": z([B, nJ_max, 3], torch.float64), "f_ext": z([B, nJ_max, 3], torch.float64),
                          "N": z([B, nM_max], torch.float64), "info": z([B], torch.int32)}
                         for _ in range(max(1, int(n_variants)))]
            first = self.outs[0]
            self.u, self.f_ext, self.N, self.info = first["u"], first["f_ext"], first["N"], first["info"]
        # (host-fed: `lanes` = RUN streams of the pull / run / push pipeline - bucket k is ordered and solved on run
        # stream k mod lanes with that lane's workspace, so that one bucket's latency-bound phases and emptying-chip
        # tails are filled by the next bucket's kernels, as in the resident step)
        n_lanes = max(1, int(lanes if lanes is not None else (HOSTFED_LANES if self.host_io else DEFAULT_LANES)))
        if max_slab_bytes is None:
            max_slab_bytes = default_slab_budget(torch, dev, n_lanes, workspace)
        # resident batches: groups cut at whole rounds of the factorisation kernel (3 waves x 4 SIMDs per CU in flight)
        quantum = 0 if self.host_io else 12 * int(torch.cuda.get_device_properties(dev).multi_processor_count)
        groups = size_buckets(packed, max_slab_bytes // n_lanes, granularity, quantum=quantum) if B else []
        n_pad_of = lambda idx: (int(packed.n_free[idx].max()) + 63) // 64 * 64
        slab_of = lambda idx: len(idx) * n_pad_of(idx) * (n_pad_of(idx) + 16)
        # largest slab first (the shared workspace is sized once) - in the host-fed pipeline SMALLEST first: the
        # device starts after a short pull, and what is exposed at the end is a small bucket's push
        groups.sort(key=lambda idx: -slab_of(idx))
        if self.host_io:
            groups, self._chip_bound_buckets = _flow_shop_order(groups, packed, n_pad_of,
                                                                os.environ.get("TRS_HOSTFED_ORDER", "johnson"))
        self.buckets = []
        self.lanes = max(1, min(n_lanes, len(groups)))
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        for idx in groups:
            need = {"S": 0, "uf": 0, "work": 0, "env": 0, "raw_j": 0, "raw_m": 0}
            nJ_b, nM_b = max(1, int(packed.nJ[idx].max())), max(1, int(packed.nM[idx].max()))
            n_b, Bb = int(packed.n_free[idx].max()), len(idx)
            sub = {"xyz": e([Bb, nJ_b, 3], torch.float64), "loads": e([Bb, nJ_b, 3], torch.float64),
                   "cbits": e([Bb, nJ_b], torch.uint8), "nJ": e([Bb], torch.int32), "nM": e([Bb], torch.int32)}
            if self.table:
                sub.update(conn=e([Bb, nM_b, 2], torch.uint16), type_idx=e([Bb, nM_b], torch.uint8), types=self.types)
            else:
                sub.update(conn=e([Bb, nM_b, 2], torch.int32), E=e([Bb, nM_b], torch.float64), A=e([Bb, nM_b], torch.float64))
                sub["rho"] = sub["A"]   # placeholder of the right shape: no kernel of the solve reads the densities
            if self.host_io:
                sub["nJ"], sub["nM"] = up(packed.nJ[idx].astype(np.int32)), up(packed.nM[idx].astype(np.int32))
            small = bool(self.lib.trs_solve_small_fits(nJ_b, nM_b, n_b))
            renumbered = plan is not None and not small   # the fused small-system kernel gains nothing from an order
            jout = e([Bb, nJ_b], torch.int32) if renumbered else None
            db = DeviceBatch.from_device(sub, n_b, joint_out=jout)
            opts = dict(options or {})
            compact_rows = opts.pop("compact_rows", None)   # (lo, hi): the compact form for the buckets of lo <= rows < hi
            db.options.update(opts)
            if compact_rows is not None:
                db.options["compact"] = bool(compact_rows[0] <= db.rows < compact_rows[1])
            if not db.small:
                need["S"], need["uf"] = Bb * db.rows * db.ld, Bb * db.rows
                need["work"] = Bb * self.lib.trs_assemble_work_bytes(nJ_b, nM_b, n_b)
                need["env"] = Bb * self.lib.trs_env_ints(n_b)
            on_device = renumbered and self.device_effort is not None and \
                (plan[0] == "device" or bool(self.lib.trs_joint_order_fits(nJ_b, nM_b)))
            # A resident bucket that is ordered on the device needs neither a gather nor a scatter launch: its
            # trs_joint_order_rows reads the trusses' rows straight out of the full batch and its trs_recover_rows
            # writes the results straight into the caller's rows (`fused_io`).
            fused = on_device and not self.host_io and os.environ.get("TRS_RAGGED_FUSED_IO", "1") != "0"
            if on_device and not self.host_io and not fused:   # the bucket's rows in the caller's numbering: input of its trs_joint_order
                need["raw_j"], need["raw_m"] = Bb * nJ_b, Bb * nM_b
            self.buckets.append({"rows": up(np.ascontiguousarray(idx, dtype=np.int64)), "dev": db, "count": Bb,
                                 "renumbered": renumbered, "order_on_device": on_device, "idx": idx, "fused_io": fused,
                                 "reach": e([Bb], torch.int32) if on_device else None, "lane": 0, "need": need,
                                 # microseconds, roughly: what a bucket of the cube batch takes alone on the chip, per
                                 # truss 0.1 + 1.3e-6 rows^2 (EXPERIMENTS R5.6) - the lanes are dealt by it
                                 "cost": Bb * (0.1 + 1.3e-6 * float(db.rows) ** 2)})
        self.workspace = workspace if workspace is not None else SolverWorkspace(torch, dev)
        self._side_streams = lane_streams(torch, dev, self.lanes - 1) if self.lanes > 1 and not self.host_io else []
        self._deal_lanes()
        if self.host_io:
            self._streams = _pipeline_streams(torch, dev, self.lib)
            if isinstance(self._streams, _MaskedStreams):
                self._run_streams = self._streams.run_streams(self.lanes)
            else:
                self._run_streams = [tuple(self._streams)[1]] + list(lane_streams(torch, dev, self.lanes - 1))

    def _deal_lanes(self):
        """Deal the buckets onto the lanes - longest processing time first on `bk["cost"]` (a size model; dealing by MEASURED
        times, and evening out the lanes' ends move by move, were tried: the lanes then end together and the step is
        no shorter - the chip is busy either way, EXPERIMENTS R5.6) -, give every lane a workspace that holds the largest of ITS
        buckets (they run one after the other on its stream) and point the buckets at it.  The buckets are launched in
        the order of `self.buckets`; resident batches keep them by descending cost, so every lane starts with its
        longest bucket and the step ends over the short ones.  Nothing of this solver may be in flight."""
        if self.host_io:   # (the host-fed pipeline has its own order - the flow shop's -: the run lanes take turns)
            for k, bk in enumerate(self.buckets):
                bk["lane"] = k % self.lanes
            self._bind_lanes()
            return
        self.buckets.sort(key=lambda bk: -bk["cost"])
        load = [0.0] * self.lanes
        for bk in self.buckets:
            lane = min(range(self.lanes), key=lambda l: load[l])
            load[lane] += bk["cost"]
            bk["lane"] = lane
        self._bind_lanes()

    def _bind_lanes(self):
        """Workspaces for the lanes as the buckets are dealt now (`bk["lane"]`), the buckets pointed at them."""
        torch, dev = self.torch, self.device
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        needs = [{"S": 0, "uf": 0, "work": 0, "env": 0, "raw_j": 0, "raw_m": 0} for _ in range(self.lanes)]
        for bk in self.buckets:
            for k, v in bk["need"].items():
                needs[bk["lane"]][k] = max(needs[bk["lane"]][k], v)
        lane_bufs = []
        for lane, need in enumerate(needs):
            lane_bufs.append(self.workspace.lane(lane).get(
                {"S": need["S"], "uf": need["uf"], "work": need["work"], "env": need["env"],
                 "raw_xyz": need["raw_j"] * 3, "raw_loads": need["raw_j"] * 3, "raw_cbits": need["raw_j"],
                 "raw_conn": need["raw_m"] * 2}))
        for bk in self.buckets:
            db, Bb = bk["dev"], bk["count"]
            bufs = lane_bufs[bk["lane"]]
            raw = {"xyz": bufs["raw_xyz"], "loads": bufs["raw_loads"], "cbits": bufs["raw_cbits"], "conn": bufs["raw_conn"]}
            if not db.small:
                wb = self.lib.trs_assemble_work_bytes(db.nJ_max, db.nM_max, db.n_max)
                ei = self.lib.trs_env_ints(db.n_max)
                db._slab = (bufs["S"][:Bb * db.rows * db.ld].view(Bb, db.rows, db.ld),
                            bufs["uf"][:Bb * db.rows].view(Bb, db.rows), bufs["work"][:Bb * wb].view(Bb, wb),
                            bufs["env"][:Bb * ei].view(Bb, ei))
            if bk["fused_io"]:
                pass
            elif bk["order_on_device"] and self.host_io:
                # (the pull of bucket k + 1 runs while bucket k is being ordered: every bucket its own buffers)
                if "raw" not in bk:
                    nJ_b, nM_b = db.nJ_max, db.nM_max
                    bk["raw"] = {"xyz": e([Bb, nJ_b, 3], torch.float64), "loads": e([Bb, nJ_b, 3], torch.float64),
                                 "cbits": e([Bb, nJ_b], torch.uint8),
                                 "conn": e([Bb, nM_b, 2], torch.uint16 if self.table else torch.int32),
                                 "nJ": db.nJ, "nM": db.nM}
            elif bk["order_on_device"]:
                nJ_b, nM_b = db.nJ_max, db.nM_max
                bk["raw"] = {"xyz": raw["xyz"][:Bb * nJ_b * 3].view(Bb, nJ_b, 3),
                             "loads": raw["loads"][:Bb * nJ_b * 3].view(Bb, nJ_b, 3),
                             "cbits": raw["cbits"][:Bb * nJ_b].view(Bb, nJ_b),
                             "conn": (raw["conn"][:Bb * nM_b * 2].view(Bb, nM_b, 2) if not self.table else
                                      raw["conn"][:Bb * nM_b].view(torch.uint16).view(Bb, nM_b, 2)),
                             "nJ": db.nJ, "nM": db.nM}
            if bk["order_on_device"]:
                # trs_joint_order writes the renumbered bucket straight into the solver's input tensors
                bk["ordered"] = {"perm": db.joint_out, "reach": bk["reach"], "xyz": db.xyz, "conn": db.conn,
                                 "cbits": db.cbits, "loads": db.loads}
        self._tables = self._copy_tables()

    def _copy_tables(self):
        """ctypes argument arrays of the gather / scatter launches of every bucket (all device pointers are
        fixed at set-up)."""
        import ctypes
        P, Z = ctypes.c_void_p, ctypes.c_size_t
        row_bytes = lambda t: int(t[0].numel() * t.element_size()) if t.dim() > 1 else int(t.element_size())
        tables = []
        for bk in self.buckets:
            db = bk["dev"]
            pairs = []
            for f in (() if bk["fused_io"] else self.gather_fields):
                if bk["order_on_device"] and f in self.JOINT_ORDERED:
                    pairs.append((f, self.inputs[f], bk["raw"][f]))       # caller's numbering -> input of the order
                elif bk["renumbered"] and f in self.JOINT_ORDERED:
                    pairs.append((f, self.ordered[f], getattr(db, f)))     # host plan: renumbered at set-up
                else:
                    pairs.append((f, self.inputs[f], getattr(db, f)))
            if bk["renumbered"] and not bk["order_on_device"]:
                pairs.append(("perm", self.ordered["perm"], db.joint_out))
            outs = [[("u", db.u, o["u"]), ("f_ext", db.f_ext, o["f_ext"]), ("N", db.N, o["N"]), ("info", db.info, o["info"])]
                    for o in self.outs]
            # host-fed: only the live part of a row crosses the link - (count array, bytes per element) by field
            per_joint = {"xyz": 24, "loads": 24, "cbits": 1, "u": 24, "f_ext": 24}
            per_member = {"conn": 4 if self.table else 8, "E": 8, "A": 8, "type_idx": 1, "N": 8}

            def pack(pairs, trimmed_is_dst):
                n = len(pairs)
                src, dst = (P * n)(*[a.data_ptr() for _, a, _ in pairs]), (P * n)(*[b.data_ptr() for _, _, b in pairs])
                sp, dp = (Z * n)(*[row_bytes(a) for _, a, _ in pairs]), (Z * n)(*[row_bytes(b) for _, _, b in pairs])
                width = (Z * n)(*[row_bytes(b if trimmed_is_dst else a) for _, a, b in pairs])
                if not self.host_io:
                    return n, src, sp, dst, dp, width, None, None, None, None
                counts = (P * n)(*[db.nJ.data_ptr() if f in per_joint else (db.nM.data_ptr() if f in per_member else None)
                                   for f, _, _ in pairs])
                elem = (Z * n)(*[per_joint.get(f, per_member.get(f, 0)) for f, _, _ in pairs])
                # pulled rows are zeroed behind their live part on the device; pushed rows up to the full row of the
                # host array, or - where the array's live extents are tracked - only over what the last writer left
                fill = (Z * n)(*[row_bytes(b) for _, _, b in pairs])
                live = None if trimmed_is_dst else (P * n)(*[self.live[f].data_ptr() if f in self.live else None
                                                             for f, _, _ in pairs])
                return n, src, sp, dst, dp, width, fill, counts, elem, live
            tables.append((pack(pairs, True) if pairs else None, [pack(o, False) for o in outs]))
        return tables

    def step(self, record=None, sections=None):
        """One pass of the whole path over the batch, asynchronous on the current stream.  `record` (a list):
        instrumented step - (stage name, start event, end event) of every bucket's gather, order, solve and
        scatter are appended.  `sections`: one entry per variant of the solver (`n_variants`) - None = the
        members' own sections, (A, E, density) = every member set to that type; results in `outs[slot]`."""
        torch = self.torch
        if self.B == 0:
            return
        sections = [None] * len(self.outs) if sections is None else list(sections)
        if len(sections) != len(self.outs):
            raise ValueError(f"{len(sections)} section variants for a solver built for {len(self.outs)}")
        # the variants with the members' own sections first: they need what the gather brought
        slots = sorted(range(len(sections)), key=lambda k: sections[k] is not None)

        def timed(name, call):   # (events go onto the CURRENT stream: the bucket's lane)
            if record is None:
                return call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = call()
            e1.record()
            record.append((name, e0, e1))
            return out

        # work-groups of a copy kernel whose other side is host memory (it needs bytes in flight, not CUs)
        # (the pushes are kept to a handful of work-groups: stores to host memory are fire-and-forget, and beyond
        # ~35 GB/s they back up in the queues the solver's own stores stand in - its step beside a saturating
        # push takes 89 instead of 60 ms, beside one of four work-groups 64, `tools/masked_pipeline_check.py`; three
        # work-groups while the chip-bound buckets are being solved, eight for the small ones at the end, is where
        # the pushes still keep up with the solves of the cube batch)
        masked = self.host_io and isinstance(self._streams, _MaskedStreams)
        PCIE_BLOCKS = int(os.environ.get("TRS_PCIE_BLOCKS", "64" if masked else "32"))
        push_spec = os.environ.get("TRS_PCIE_PUSH_BLOCKS", "3,8" if masked else str(PCIE_BLOCKS)).split(",")
        n_chip = getattr(self, "_chip_bound_buckets", 0)   # "a,b": a for the chip-bound buckets, b for the others
        push_blocks = lambda k: int(push_spec[0] if (k < n_chip or len(push_spec) == 1) else push_spec[1])
        with torch.cuda.device(self.device):
            if not self.host_io:
                caller = torch.cuda.current_stream(self.device)
                lanes = [caller] + list(self._side_streams)
                self._lane_events = []   # (kept until the next step: none is destroyed while a stream may still wait on it)
                if len(lanes) > 1:   # fork: the side lanes start behind everything queued on the caller's stream
                    fork = torch.cuda.Event()
                    fork.record(caller)
                    self._lane_events.append(fork)
                    for side in lanes[1:]:
                        side.wait_event(fork)
                try:
                    self._step_resident(lanes, sections, slots, timed)
                finally:
                    for side in lanes[1:]:   # join: what follows on the caller's stream sees every lane's results
                        done = torch.cuda.Event()
                        done.record(side)
                        caller.wait_event(done)
                        self._lane_events.append(done)
                return
            if sections[0] is not None:
                raise ValueError("the host-fed pipeline solves the members' own sections")
            # host-fed pipeline: pull of bucket k + 1 | order + solve of bucket k | push of bucket k - 1
            s_up, _, s_down = tuple(self._streams)
            runs = self._run_streams
            caller = torch.cuda.current_stream(self.device)
            timing = record is not None
            begin = torch.cuda.Event(enable_timing=timing)
            begin.record(caller)
            for st in [s_up, s_down] + list(runs):
                st.wait_event(begin)
            mark = lambda name, stream: record.append((name, begin, self._marked(stream))) if timing else None
            for k, (bk, (gather, scatters)) in enumerate(zip(self.buckets, self._tables)):
                scatter = scatters[0]
                with torch.cuda.stream(s_up):
                    mark(f"bucket {k} pull begins", s_up)
                    _capi.check(self.lib.trs_copy_rows(*gather, bk["count"], bk["rows"].data_ptr(), 0, PCIE_BLOCKS,
                                                       s_up.cuda_stream), "trs_copy_rows (pull)")
                    pulled = torch.cuda.Event()
                    pulled.record(s_up)
                    mark(f"bucket {k} pulled", s_up)
                s_run = runs[bk["lane"]]
                with torch.cuda.stream(s_run):
                    s_run.wait_event(pulled)
                    mark(f"bucket {k} run begins", s_run)
                    if bk["order_on_device"]:
                        joint_order_device(torch, bk["raw"], effort=self.device_effort, out=bk["ordered"])
                    bk["dev"].solve()
                    solved = torch.cuda.Event()
                    solved.record(s_run)
                    mark(f"bucket {k} solved", s_run)
                with torch.cuda.stream(s_down):
                    s_down.wait_event(solved)
                    mark(f"bucket {k} push begins", s_down)
                    _capi.check(self.lib.trs_copy_rows(*scatter, bk["count"], bk["rows"].data_ptr(), 1, push_blocks(k),
                                                       s_down.cuda_stream), "trs_copy_rows (push)")
                    mark(f"bucket {k} pushed", s_down)
            done = torch.cuda.Event()
            done.record(s_down)
            caller.wait_event(done)   # work queued on the caller's stream after step() sees the results

    def _step_resident(self, lanes, sections, slots, timed):
        """The buckets of a resident batch, each on the stream of its lane (`lanes[0]` = the caller's)."""
        torch = self.torch
        nJ_full, nM_full = int(self.u.shape[1]), int(self.N.shape[1])
        for bk, (gather, scatters) in zip(self.buckets, self._tables):
            with torch.cuda.stream(lanes[bk["lane"]]):
                stream = lanes[bk["lane"]].cuda_stream
                if bk["fused_io"]:
                    db, inp, ordr = bk["dev"], self.inputs, bk["ordered"]
                    if self.table:
                        sec_in, sec_out = (inp["type_idx"].data_ptr(),), (db.type_idx.data_ptr(),)
                        order_rows, what = self.lib.trs_joint_order_rows_tab, "trs_joint_order_rows_tab"
                    else:
                        sec_in, sec_out = (inp["E"].data_ptr(), inp["A"].data_ptr()), (db.E.data_ptr(), db.A.data_ptr())
                        order_rows, what = self.lib.trs_joint_order_rows, "trs_joint_order_rows"
                    timed("order", lambda: _capi.check(order_rows(
                        bk["count"], db.nJ_max, db.nM_max, bk["rows"].data_ptr(), int(inp["xyz"].shape[1]),
                        int(inp["conn"].shape[1]), inp["xyz"].data_ptr(), inp["conn"].data_ptr(),
                        inp["cbits"].data_ptr(), inp["loads"].data_ptr(), *sec_in,
                        inp["nJ"].data_ptr(), inp["nM"].data_ptr(), ordr["perm"].data_ptr(), ordr["reach"].data_ptr(),
                        db.xyz.data_ptr(), db.conn.data_ptr(), db.cbits.data_ptr(), db.loads.data_ptr(),
                        *sec_out, db.nJ.data_ptr(), db.nM.data_ptr(),
                        int(self.device_effort), stream), what))
                    for slot in slots:
                        types = self._section_types(db, sections[slot])
                        timed("solve", lambda: db.solve_rows(bk["rows"], self.outs[slot], nJ_full, nM_full, types=types))
                    continue
                timed("gather", lambda: _capi.check(self.lib.trs_copy_rows(
                    *gather, bk["count"], bk["rows"].data_ptr(), 0, 0, stream), "trs_copy_rows (gather)"))
                if bk["order_on_device"]:
                    timed("order", lambda: joint_order_device(torch, bk["raw"], effort=self.device_effort, out=bk["ordered"]))
                for slot in slots:
                    types = self._section_types(bk["dev"], sections[slot])
                    timed("solve", lambda: bk["dev"].solve(types=types))
                    timed("scatter", lambda: _capi.check(self.lib.trs_copy_rows(
                        *scatters[slot], bk["count"], bk["rows"].data_ptr(), 1, 0, stream), "trs_copy_rows (scatter)"))

    def _section_types(self, db, section):
        """A section variant of a step (`section` = None: the members' own, or (a, e, density) for every member): the
        general form overwrites the bucket's A and E, the table form solves with another type table - every row the
        fixed triple - and leaves the bucket's type indices alone.  Returns the table to pass on, or None."""
        if section is None:
            return None
        if not db.table:
            db.A.fill_(float(section[0]))
            db.E.fill_(float(section[1]))
            return None
        key = tuple(float(v) for v in section[:3]) + (0.0,) * (3 - len(section[:3]))
        cache = self._fixed_types
        if key not in cache:
            row = self.torch.tensor(key, dtype=self.torch.float64, device=self.device)
            cache[key] = row.expand(max(1, int(self.types.shape[0])), 3).contiguous()
        return cache[key]

    def _marked(self, stream):
        ev = self.torch.cuda.Event(enable_timing=True)
        ev.record(stream)
        return ev

    def adopt_launch_hints(self):
        """After a step: read back the largest envelope reach the device order reported per bucket (one scalar
        each) and tell every bucket whose envelopes all stay within the wave-per-matrix kernels' range to skip the
        launches that would find no matrix (`DeviceBatch.all_narrow`).  The order is a function of the resident
        inputs, so the hint holds for every later step; it is safe in any case (a hinted batch is routed narrow
        on the device regardless).  Returns the number of buckets hinted."""
        hinted = 0
        for bk in self.buckets:
            db = bk["dev"]
            if bk["order_on_device"] and not db.small and db.use_envelope:
                db.all_narrow = bool(int(bk["reach"].max().item()) <= NARROW_MAX_BELOW)
                hinted += int(db.all_narrow)
        return hinted

    def result(self):
        """Synchronise and download the dense results (caller's order and numbering); in the host-fed mode they
        are in the caller's page-locked arrays already."""
        self.torch.cuda.synchronize(self.device)
        if self.host_io:
            return BatchResult(self.u.numpy(), self.f_ext.numpy(), self.N.numpy(), self.info.numpy())
        return BatchResult(self.u.cpu().numpy(), self.f_ext.cpu().numpy(), self.N.cpu().numpy(),
                           self.info.cpu().numpy())


@dataclass
class DeviceResult:
    """Dense results of a batched solve left on the device (torch tensors, caller's joint order):
    displace / external [B,nJ_max,3] f64, internal [B,nM_max] f64, info [B] i32; `inputs` maps
    DeviceBatch.INPUT_FIELDS to the resident input tensors (shared by the results of one call)."""
    displace: object
    external: object
    internal: object
    info: object
    inputs: dict


def _solve_small_host(packed: PackedBatch, torch, dev, variants, on_device=False):
    """Host arrays in -> host results out for a batch that qualifies for the fused small-system kernel
    as a whole: ONE upload (every input packed into one byte buffer), one `trs_solve_small` launch per
    section variant, ONE download.  This is what `Truss.Solve()` of a small truss costs: two copies and
    a kernel.  Returns a list of `BatchResult`, one per variant (`on_device`: of `DeviceResult`, nothing
    is downloaded)."""
    lib = _capi.load()
    B, nJm, nMm = packed.B, packed.nJ_max, packed.nM_max
    ins = [("xyz", packed.xyz, np.float64), ("loads", packed.loads, np.float64), ("E", packed.E, np.float64),
           ("A", packed.A, np.float64), ("rho", packed.rho, np.float64), ("conn", packed.conn, np.int32),
           ("nJ", packed.nJ, np.int32), ("nM", packed.nM, np.int32), ("cbits", packed.cbits, np.uint8)]
    off, total = {}, 0
    for name, arr, dt in ins:
        off[name] = total
        total += (arr.size * np.dtype(dt).itemsize + 15) // 16 * 16
    own = len(variants) > 1 or variants[0] is not None
    if own:   # the solves read A_var / E_var; the batch's own sections stay in A / E
        off["A_var"], off["E_var"] = total, total + (packed.A.size * 8 + 15) // 16 * 16
        total = off["E_var"] + (packed.A.size * 8 + 15) // 16 * 16
    host = np.empty([total], dtype=np.uint8)
    for name, arr, dt in ins:
        host[off[name]: off[name] + arr.size * np.dtype(dt).itemsize].view(dt)[:] = arr.reshape(-1)
    din = torch.from_numpy(host).to(dev)
    nu, nn = B * nJm * 3 * 8, B * nMm * 8
    per = 2 * nu + nn + (B * 4 + 15) // 16 * 16
    dout = torch.empty([len(variants) * per], dtype=torch.uint8, device=dev)
    pin, pout = din.data_ptr(), dout.data_ptr()
    stream = torch.cuda.current_stream(dev).cuda_stream
    nsec = B * nMm * 8
    with torch.cuda.device(dev):
        for slot, sec in enumerate(variants):
            a_ptr, e_ptr = pin + off["A"], pin + off["E"]
            if own:
                va = din[off["A_var"]: off["A_var"] + nsec].view(torch.float64)
                ve = din[off["E_var"]: off["E_var"] + nsec].view(torch.float64)
                if sec is None:
                    va.copy_(din[off["A"]: off["A"] + nsec].view(torch.float64))
                    ve.copy_(din[off["E"]: off["E"] + nsec].view(torch.float64))
                else:
                    va.fill_(float(sec[0])); ve.fill_(float(sec[1]))
                a_ptr, e_ptr = pin + off["A_var"], pin + off["E_var"]
            o = pout + slot * per
            _capi.check(lib.trs_solve_small(
                B, nJm, nMm, packed.n_max, pin + off["xyz"], pin + off["conn"], e_ptr, a_ptr,
                pin + off["cbits"], pin + off["loads"], pin + off["nJ"], pin + off["nM"], o, o + nu,
                o + 2 * nu, o + 2 * nu + nn, None, None, None, 0.0, 0.0, None, None, None, stream),
                "trs_solve_small")
    if on_device:
        tdt = {np.float64: torch.float64, np.int32: torch.int32, np.uint8: torch.uint8}
        inputs = {name: din[off[name]: off[name] + arr.size * np.dtype(dt).itemsize].view(tdt[dt]).view(arr.shape)
                  for name, arr, dt in ins}
        out = []
        for slot in range(len(variants)):
            d = dout[slot * per: (slot + 1) * per]
            out.append(DeviceResult(d[:nu].view(torch.float64).view(B, nJm, 3),
                                    d[nu: 2 * nu].view(torch.float64).view(B, nJm, 3),
                                    d[2 * nu: 2 * nu + nn].view(torch.float64).view(B, nMm),
                                    d[2 * nu + nn: 2 * nu + nn + 4 * B].view(torch.int32), inputs))
        return out
    hout = dout.cpu().numpy()
    results = []
    for slot in range(len(variants)):
        h = hout[slot * per: (slot + 1) * per]
        results.append(BatchResult(h[:nu].view(np.float64).reshape(B, nJm, 3),
                                   h[nu: 2 * nu].view(np.float64).reshape(B, nJm, 3),
                                   h[2 * nu: 2 * nu + nn].view(np.float64).reshape(B, nMm),
                                   h[2 * nu + nn: 2 * nu + nn + 4 * B].view(np.int32).copy()))
    return results


class ResultPool:
    """Page-locked host buffers for the results of `solve_batch(..., pool=...)`, reused from call to call:
    the download is one DMA per array instead of a copy into freshly page-faulted memory.  The arrays of a
    returned `BatchResult` are views of the pool and stay valid until the pool serves another call.

    `tracked=True` (opt-in): the host-fed pipeline (`solve_batch_streamed`) keeps LIVE EXTENTS of the result arrays
    (`take_tracked`) and pushes only live bytes - the zero padding crosses the link once, when the arrays are made.
    The contract that comes with it: the returned arrays are READ-ONLY views; a caller who writes into them (say
    `res.displace += x`) must call `invalidate()` before the pool's next use, or later results carry stale bytes in
    their padding.  Without it every push zero-fills its rows to their full width (more bytes over PCIe, no
    contract)."""

    def __init__(self, tracked=False):
        self._bufs = {}
        self._live = {}
        self.tracked = bool(tracked)

    def take(self, torch, key, shape, dtype):
        self._live.pop(key, None)   # whoever takes the plain buffer may write anything anywhere in it
        buf = self._bufs.get(key)
        if buf is None or tuple(buf.shape) != tuple(shape) or buf.dtype != dtype:
            buf = torch.empty(tuple(shape), dtype=dtype, pin_memory=True)
            self._bufs[key] = buf
        return buf

    def take_tracked(self, torch, key, shape, dtype, device):
        """The buffer together with its LIVE EXTENTS: a device int32 tensor, one entry per row, that states "row r
        is zero behind byte live[r]".  `trs_copy_rows` keeps the statement true while it pushes results into the
        rows (it zeroes only what the previous writer of a row left and records the new extent), so the zero
        padding of the padded result arrays is paid for once - the buffer is created zeroed - instead of crossing
        the link with every call.  Anyone else who writes into the buffer must take it with `take` (or call
        `invalidate`): the next tracked use then starts from "nothing known" and zero-fills whole rows once."""
        shape = tuple(shape)
        row_bytes = int(np.prod(shape[1:], dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
        buf, live = self._bufs.get(key), self._live.get(key)
        if buf is None or tuple(buf.shape) != shape or buf.dtype != dtype:
            buf = torch.zeros(shape, dtype=dtype, pin_memory=True)
            self._bufs[key] = buf
            live = torch.zeros([shape[0]], dtype=torch.int32, device=device)
        elif live is None or live.device != torch.device(device) or live.shape[0] != shape[0]:
            live = torch.full([shape[0]], row_bytes, dtype=torch.int32, device=device)
        self._live[key] = live
        return buf, live

    def invalidate(self):
        """Forget the live extents (after writing into pool buffers by hand)."""
        self._live.clear()


def host_result_arrays(torch, pool, B, nJ_max, nM_max, device):
    """The page-locked result arrays of a host-fed `RaggedSolver` (`host_io=(inputs, THIS)`) out of a
    `ResultPool`, with their live extents."""
    out, live = {}, {}
    for name, shape in (("u", [B, nJ_max, 3]), ("f_ext", [B, nJ_max, 3]), ("N", [B, nM_max])):
        if pool.tracked:   # (the caller opted into the read-only contract of tracked extents)
            out[name], live[name] = pool.take_tracked(torch, (0, name), shape, torch.float64, device)
        else:
            out[name] = pool.take(torch, (0, name), shape, torch.float64)
    out["info"] = pool.take(torch, (0, "info"), [B], torch.int32)
    out["live"] = live
    return out


def solve_batch_streamed(packed: PackedBatch, device=None, reorder=True, pool=None, max_slab_bytes=48 << 30, lanes=None):
    """Host arrays in -> host results out for a LARGE ragged batch held in page-locked memory
    (`PackedBatch.pinned()`), as a pipeline over PCIe with NO staging copy: the batch stays where it is, every
    size bucket's gather pulls its rows straight out of the host arrays (page-locked memory is mapped into the
    device's address space; only the bucket-trimmed prefix of every row crosses the link - for cube trusses
    about 60 % of the padded bytes), the device orders and solves the bucket, and its scatter pushes the results
    into the (page-locked) result arrays - pull of bucket k + 1, device work of bucket k and push of bucket k - 1
    at the same time on three streams (`RaggedSolver(host_io=...)`; `lanes` = run streams, default `HOSTFED_LANES`: the
    buckets' device work alternates between them).  Same results, bit for bit, as `solve_batch(packed, reorder=...)`.  `solve_batch(..., pool=...)` routes big pinned batches here by itself."""
    torch, dev = _require_gpu(device)
    B, nJ_max, nM_max = packed.B, packed.nJ_max, packed.nM_max
    if B == 0:
        return BatchResult(np.zeros([0, nJ_max, 3]), np.zeros([0, nJ_max, 3]), np.zeros([0, nM_max]),
                           np.zeros([0], dtype=np.int32))
    pool = pool if pool is not None else ResultPool()
    host_out = host_result_arrays(torch, pool, B, nJ_max, nM_max, dev)
    host_in = {f: torch.from_numpy(getattr(packed, f)) for f in (RaggedSolver.GATHER_TABLE if packed.is_table else RaggedSolver.GATHER)}
    if packed.is_table:   # (5 instead of 24 bytes per member cross the link: conn uint16 + one type index)
        host_in["types"] = torch.from_numpy(np.ascontiguousarray(packed.types, dtype=np.float64))
    solver = RaggedSolver(packed, dev, reorder=reorder, max_slab_bytes=max_slab_bytes, host_io=(host_in, host_out),
                          lanes=lanes)
    solver.step()
    return solver.result()


def _as_packed(trusses_or_packed):
    return trusses_or_packed if isinstance(trusses_or_packed, PackedBatch) else pack_trusses(list(trusses_or_packed))


def _device_f64(torch, dev, x, vectors=False):
    """An array argument (numpy or torch; None stays None) as a contiguous float64 tensor on `dev`; `vectors`: the last
    axis holds 2 or 3 components, and two get z = 0."""
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    x = x.to(device=dev, dtype=torch.float64)
    if vectors and int(x.shape[-1]) == 2:
        x = torch.nn.functional.pad(x, (0, 1))
    return x.contiguous()


def _host_result(torch, dev, res):
    """A result dataclass of device tensors as the same dataclass of numpy arrays (None stays None)."""
    torch.cuda.synchronize(dev)
    return type(res)(**{k: None if v is None else v.cpu().numpy() for k, v in vars(res).items()})


def _host_array(x, dtype):
    """An array argument (numpy, torch or nested lists) as a host array of `dtype` (None: its own)."""
    if not isinstance(x, np.ndarray) and hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=dtype)


def _peak_fields(*shape):
    """The `FIELDS` entries that `MemberLossResult` and `MemberSetResult` share: the two peaks and where they occur."""
    return {"peak_stress": ("peak_stress", 0.0, "float64", shape), "peak_member": ("peak_member", -1, "int32", shape),
            "peak_displace": ("peak_displace", 0.0, "float64", shape), "peak_joint": ("peak_joint", -1, "int32", shape)}


def _new_result(torch, dev, cls, B, sizes, without=()):
    """A result dataclass of an analysis on the resident factor on `dev`, from its table `cls.FIELDS`: field -> (key of the
    `DeviceBatch` method's dict, fill value, dtype, shape after B).  Shapes and types are the device's (`_field_shapes`):
    a "bool" is kept as int32 until `_finish_result`, a "complex128" is viewed as complex at once, as the methods return
    it.  Fields named in `without` (optional results that were not asked for) are None; `info` [B] is int32 zeros."""
    shapes = _field_shapes(cls.FIELDS, B, sizes, [v[0] for field, v in cls.FIELDS.items() if field not in without])
    made = dict.fromkeys(cls.FIELDS)
    for field, (key, fill, dtype, shape) in cls.FIELDS.items():
        if field not in without:
            x = torch.full(shapes[key][0], fill, dtype=shapes[key][1], device=dev)
            made[field] = torch.view_as_complex(x) if dtype == "complex128" else x
    return cls(**made, info=torch.zeros([B], dtype=torch.int32, device=dev))


def _upload_design_args(torch, dev, val):
    """(`on`, `bound`) of the two sizing analyses: "loads", "area_min" and "area_max" of `val` on `dev` - an array is
    uploaded, a number or None stays -, and bound(part, x): a bound [B, nM_max] cut to the bucket `part`, a number as it
    is."""
    on = {k: _device_f64(torch, dev, val[k]) if isinstance(val[k], np.ndarray) else val[k]
          for k in ("loads", "area_min", "area_max")}
    return on, lambda part, x: part.cut(x, nM=1) if hasattr(x, "data_ptr") else x


def _per_case_runs(torch, db, part, out, L, run):
    """The L cases of an analysis whose run writes the areas, on the resident bucket `db`: run(l) -> the dict of the
    `DeviceBatch` method, each an independent run from the nominal areas, into `out`[:, l] by `CASE_FIELDS`.  `db.info`
    ends as what the first case with a nonzero info left, per truss."""
    nominal = db.A.clone()
    info = torch.zeros_like(db.info)
    for l in range(L):
        db.A.copy_(nominal)
        res = run(l)
        for field, (key, fill, dtype, shape) in type(out).CASE_FIELDS.items():
            part.put(getattr(out, field)[:, l], res[key], nJ=1 if "nJ" in shape else None,
                     nM=1 if "nM" in shape else None)
        info = torch.where(info != 0, info, db.info)
    db.info.copy_(info)


def _put_result(part, out, res):
    """A bucket's results `res` (the dict of the `DeviceBatch` method) into the full-batch dataclass `out`: the "nJ" and
    "nM" places of a field's shape are the axes `_Bucket.put` narrows; a key that `res` lacks keeps its fill value."""
    for field, (key, fill, dtype, shape) in type(out).FIELDS.items():
        if getattr(out, field) is not None and key in res:
            part.put(getattr(out, field), res[key], nJ=shape.index("nJ") + 1 if "nJ" in shape else None,
                     nM=tuple(i + 1 for i, n in enumerate(shape) if n == "nM"))


def _finish_result(torch, dev, out, on_device):
    """The flags of `out` as bool, and the whole on the host unless `on_device`."""
    for field, (key, fill, dtype, shape) in type(out).FIELDS.items():
        if dtype == "bool":
            setattr(out, field, getattr(out, field) != 0)
    return out if on_device else _host_result(torch, dev, out)


class _Bucket:
    """One size bucket of `_factored_buckets`: `rows`, its trusses' places in the full batch, and the bucket's own padded
    sizes.  `cut` and `put` name the axis that runs over joints (`nJ=`) or members (`nM=`; `put` takes a tuple of them
    too), if the tensor has one."""

    def __init__(self, rows, nJ_max, nM_max):
        self.rows, self.nJ_max, self.nM_max = rows, nJ_max, nM_max

    def cut(self, x, nJ=None, nM=None):
        """The bucket's part of a full-batch device tensor, contiguous (None stays None)."""
        if x is None:
            return None
        x = x.index_select(0, self.rows)
        if nJ is not None:
            x = x.narrow(nJ, 0, self.nJ_max)
        if nM is not None:
            x = x.narrow(nM, 0, self.nM_max)
        return x.contiguous()

    def put(self, dst, src, nJ=None, nM=None):
        """Write a result of the bucket into the full-batch tensor `dst`."""
        index = [self.rows] + [slice(None)] * (src.dim() - 1)
        if nJ is not None:
            index[nJ] = slice(0, self.nJ_max)
        for axis in (() if nM is None else nM if isinstance(nM, tuple) else (nM,)):
            index[axis] = slice(0, self.nM_max)
        dst[tuple(index)] = src


def _factored_buckets(packed, dev, info, max_slab_bytes, reorder, options, use_envelope, cases=1, factor=None):
    """The loop that the analyses on a resident factor share: per size bucket (`size_buckets`) the trusses are uploaded,
    ordered and factored on the staged pipeline, and (DeviceBatch, _Bucket) is yielded for the analysis; afterwards the
    factorisation's status goes to the bucket's rows of `info`.  Nothing is factored for an empty batch or for
    `cases` = 0 load cases.  `factor(db, part)` (None: `db.factor()`) is what factors a bucket."""
    import torch
    if not packed.B or not cases:
        return
    for idx in size_buckets(packed, max_slab_bytes):
        sub = packed.take(idx).trimmed()
        part = _Bucket(torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(dev), sub.nJ_max, sub.nM_max)
        part.index = np.asarray(idx, dtype=np.int64)   # (the same places on the host: `solve_member_sets` plans there)
        db = DeviceBatch(sub, dev, use_envelope=use_envelope, use_small=False, reorder=reorder, options=options)
        if factor is None:
            db.factor()
        else:
            factor(db, part)
        yield db, part
        info[part.rows] = db.info


@dataclass
class LoadCaseResult:
    """Dense host results of `solve_load_cases`: displace/external [B, L, nJ_max, 3], internal [B, L, nM_max],
    info [B] (0 ok, k>0: pivot k of the reduced stiffness matrix is not positive - the cases of that truss are
    meaningless, the other trusses are unaffected)."""
    displace: np.ndarray
    external: np.ndarray
    internal: np.ndarray
    info: np.ndarray

    FIELDS = {"displace": ("u", 0.0, "float64", ("L", "nJ", 3)), "external": ("f_ext", 0.0, "float64", ("L", "nJ", 3)),
              "internal": ("N", 0.0, "float64", ("L", "nM"))}


def _load_cases_on_device(torch, dev, packed, loads, max_slab_bytes, reorder, options, use_envelope, after=None):
    """The forward pass of `solve_load_cases` and `solve_gradients`: `loads` float64 [B, L, nJ_max, 3] on `dev`, the
    buckets as `_factored_buckets` makes them; `after(db, part, res)` runs per bucket on the solved cases.  Returns a
    `LoadCaseResult` of device tensors."""
    L = int(loads.shape[1])
    out = _new_result(torch, dev, LoadCaseResult, packed.B, {"L": L, "nJ": packed.nJ_max, "nM": packed.nM_max})
    for db, part in _factored_buckets(packed, dev, out.info, max_slab_bytes, reorder, options, use_envelope, cases=L):
        res = db.solve_cases(part.cut(loads, nJ=2))
        _put_result(part, out, res)
        if after is not None:
            after(db, part, res)
    return out


def solve_load_cases(trusses_or_packed, loads, device=None, reorder=False, options=None, max_slab_bytes=64 << 30,
                     on_device=False, sections=None, use_envelope=True):
    """Solve every truss of a batch under L load cases, factoring each truss ONCE: `loads` is [B, L, nJ_max, dim]
    (numpy or torch; dim 2 or 3, a 2D load gets z = 0) in the caller's joint numbering; the packed batch's own `loads`
    field is ignored.  Per size bucket (`size_buckets`, as `solve_batch`'s generic route) the trusses are uploaded,
    ordered (`reorder`, any `order_plan`), assembled and factored once (`DeviceBatch.factor`), then all L cases are
    gathered, substituted against the factor and recovered (`DeviceBatch.solve_cases`).  Returns a `LoadCaseResult`
    (host arrays, or torch tensors on the device with `on_device=True`).  Either member form.  Batches of small
    trusses go through the staged pipeline too (the fused small-system kernel keeps no factor).  `sections=` variants
    are not combined with load cases (ValueError).  `use_envelope=False`: the dense mode (`DeviceBatch`)."""
    _refuse_sections("solve_load_cases", "load cases", sections)
    packed = _as_packed(trusses_or_packed)
    torch, dev = _require_gpu(device)
    B, nJ_max = packed.B, packed.nJ_max
    shape = tuple(int(x) for x in loads.shape)
    if len(shape) != 4 or shape[0] != B or shape[2] != nJ_max or shape[3] not in (2, 3):
        raise ValueError(f"solve_load_cases: loads must be [B={B}, L, nJ_max={nJ_max}, 2 or 3], got {shape}")
    out = _load_cases_on_device(torch, dev, packed, _device_f64(torch, dev, loads, vectors=True), max_slab_bytes,
                                reorder, options, use_envelope)
    return out if on_device else _host_result(torch, dev, out)


@dataclass
class EffectCaseResult:
    """Dense results of `solve_effect_cases`: displace/external/body [B, L, nJ_max, 3], internal [B, L, nM_max], info [B]
    (as `LoadCaseResult`).  `displace` holds the settlements at the constrained DOFs, `internal` is
    k c . (u1 - u0) - E A eps0, `external` never contains the self-weight - that is `body`, and over all DOFs of a truss
    `external + body` sums to zero."""
    displace: np.ndarray
    external: np.ndarray
    internal: np.ndarray
    body: np.ndarray
    info: np.ndarray

    FIELDS = dict(LoadCaseResult.FIELDS, body=("body", 0.0, "float64", ("L", "nJ", 3)))


def _check_effect_args(packed, loads, prestrain, settlement, accel, sections):
    """The argument errors of `solve_effect_cases` that need no device.  Returns (L, arrays): the given arguments as
    contiguous float64 host arrays, vectors padded to three components."""
    _refuse_sections("solve_effect_cases", "load cases", sections)
    B, nJ_max, nM_max = packed.B, packed.nJ_max, packed.nM_max
    # every argument is [B, L] + inner + last: the dimensions after L, and the allowed sizes of the vector axis (if any)
    inner = {"loads": (nJ_max,), "prestrain": (nM_max,), "settlement": (nJ_max,), "accel": ()}
    arrays, L = {}, None
    for name, x in (("loads", loads), ("prestrain", prestrain), ("settlement", settlement), ("accel", accel)):
        if x is None:
            continue
        x = _host_array(x, np.float64)
        vector = name != "prestrain"
        shape = tuple(x.shape)
        if vector:
            ok = len(shape) >= 3 and shape[-1] in (2, 3)
            shape = shape[:-1]
        else:
            ok = True
        ok = ok and len(shape) == 2 + len(inner[name]) and shape[0] == B and shape[2:] == inner[name]
        if not ok:
            tail = "".join(f", {v}" for v in inner[name]) + (", 2 or 3" if vector else "")
            raise ValueError(f"solve_effect_cases: {name} must be [B={B}, L{tail}], got {tuple(x.shape)}")
        if L is not None and x.shape[1] != L:
            raise ValueError(f"solve_effect_cases: {name} has L = {x.shape[1]}, the arguments before it L = {L}")
        L = int(x.shape[1])
        if not np.isfinite(x).all():
            raise ValueError(f"solve_effect_cases: {name} has a non-finite entry")
        if vector and x.shape[-1] == 2:
            x = np.concatenate([x, np.zeros(x.shape[:-1] + (1,))], axis=-1)
        arrays[name] = np.ascontiguousarray(x)
    if L is None:
        raise ValueError("solve_effect_cases: give at least one of loads, prestrain, settlement, accel")
    flat = np.asarray(packed.dim).reshape(-1) == 2
    if "accel" in arrays and arrays["accel"][flat][..., 2].any():
        raise ValueError("solve_effect_cases: accel has a z component on a 2D truss")
    if "settlement" in arrays:
        ubar = arrays["settlement"]
        if ubar[flat][..., 2].any():
            raise ValueError("solve_effect_cases: settlement has a z component on a 2D truss")
        held = packed.constrained()
        if (ubar != 0)[np.broadcast_to(~held[:, None], ubar.shape)].any():
            raise ValueError("solve_effect_cases: settlement is non-zero at a free DOF (a displacement can be "
                             "prescribed at constrained DOFs only)")
    return L, arrays


def solve_effect_cases(trusses_or_packed, loads=None, prestrain=None, settlement=None, accel=None, device=None,
                       reorder=False, options=None, max_slab_bytes=64 << 30, on_device=False, sections=None,
                       use_envelope=True):
    """`solve_load_cases` for cases that carry support settlements, member pre-strain and self-weight beside (or in
    place of) joint forces - every truss is still factored ONCE, because all three only change the right-hand side.
    Per case k of truss b (numpy or torch, caller's joint numbering; any may be None, at least one is given, all agree
    on L; vectors of a 2D truss may have two components):
      `loads`      [B, L, nJ_max, dim]  joint forces;
      `prestrain`  [B, L, nM_max]       member initial strain eps0: alpha * dT for a temperature change, dL / L for a
                                        member fabricated too long; N = k c . (u1 - u0) - E A eps0;
      `settlement` [B, L, nJ_max, dim]  prescribed displacements of the CONSTRAINED DOFs (zero elsewhere - a non-zero
                                        entry at a free DOF is a ValueError);
      `accel`      [B, L, dim]          body-force vector per unit weight, e.g. (0, 0, -1) for densities that are weight
                                        densities: a member loads each end joint with half of a * length * density
                                        times it.
    Returns an `EffectCaseResult` (host arrays, or torch tensors on the device with `on_device=True`): `displace` shows
    the settlements at the supports, `external` is the applied load at free DOFs and the support's force at constrained
    DOFs - never the self-weight, which is `body`.  Buckets, member forms, `reorder` plans, `options` and `use_envelope`
    as `solve_load_cases`; `sections=` variants, non-finite entries and z components on a 2D truss raise ValueError
    before any device work."""
    packed = _as_packed(trusses_or_packed)
    L, arrays = _check_effect_args(packed, loads, prestrain, settlement, accel, sections)
    torch, dev = _require_gpu(device)
    given = {k: _device_f64(torch, dev, v) for k, v in arrays.items()}
    out = _new_result(torch, dev, EffectCaseResult, packed.B, {"L": L, "nJ": packed.nJ_max, "nM": packed.nM_max})
    axis = {"loads": dict(nJ=2), "prestrain": dict(nM=2), "settlement": dict(nJ=2), "accel": {}}
    for db, part in _factored_buckets(packed, dev, out.info, max_slab_bytes, reorder, options, use_envelope, cases=L):
        _put_result(part, out, db.solve_effect_cases(**{k: part.cut(given.get(k), **axis[k]) for k in axis},
                                                     want_body=True))
    return out if on_device else _host_result(torch, dev, out)


@dataclass
class GradientResult:
    """Gradients of `solve_gradients`: dA, dE [B, nM_max] (per member, also in the table member form), dxyz
    [B, nJ_max, 3] (summed over the load cases; z = 0 for a 2D truss), dloads [B, L, nJ_max, 3] (per case, zero at
    constrained DOFs), info [B] (the factorisation's status: the gradients of a truss with info != 0 are meaningless)."""
    dA: np.ndarray
    dE: np.ndarray
    dxyz: np.ndarray
    dloads: np.ndarray
    info: np.ndarray

    FIELDS = {"dA": ("A", 0.0, "float64", ("nM",)), "dE": ("E", 0.0, "float64", ("nM",)),
              "dxyz": ("xyz", 0.0, "float64", ("nJ", 3)), "dloads": ("loads", 0.0, "float64", ("L", "nJ", 3))}


def _check_gradient_args(B, nJ_max, nM_max, loads, cotangents, loss, sections):
    """The argument errors of `solve_gradients` that need no device.  Returns L."""
    _refuse_sections("solve_gradients", "gradients", sections)
    shape = tuple(int(x) for x in loads.shape)
    if len(shape) != 4 or shape[0] != B or shape[2] != nJ_max or shape[3] not in (2, 3):
        raise ValueError(f"solve_gradients: loads must be [B={B}, L, nJ_max={nJ_max}, 2 or 3], got {shape}")
    L = shape[1]
    given = {k: g for k, g in cotangents.items() if g is not None}
    if loss is not None and given:
        raise ValueError("solve_gradients: give either loss= or fixed cotangents (grad_u / grad_f_ext / grad_N), not both")
    if loss is None and not given:
        raise ValueError("solve_gradients: nothing to differentiate - give grad_u, grad_f_ext, grad_N or loss=")
    for name, g in given.items():
        got = tuple(int(x) for x in g.shape)
        ok = got == (B, L, nM_max) if name == "grad_N" else \
            (len(got) == 4 and got[:3] == (B, L, nJ_max) and got[3] in (2, 3))
        if not ok:
            want = f"[B={B}, L={L}, nM_max={nM_max}]" if name == "grad_N" else f"[B={B}, L={L}, nJ_max={nJ_max}, 2 or 3]"
            raise ValueError(f"solve_gradients: {name} must be {want}, got {got}")
    return L


def solve_gradients(trusses_or_packed, loads, grad_u=None, grad_f_ext=None, grad_N=None, loss=None,
                    want=DeviceBatch.GRADIENTS, device=None, reorder=False, options=None, max_slab_bytes=64 << 30,
                    on_device=False, sections=None, use_envelope=True):
    """`solve_load_cases` plus the adjoint gradients of its results: every truss is factored ONCE, its L load cases
    are solved, and one more substitution against the same factor gives the derivative of a scalar J with respect to
    the member areas and moduli, the joint coordinates and the loads (`DeviceBatch.adjoint_cases`; no finite
    differences, no second factorisation).  J enters either as fixed cotangents `grad_u`, `grad_f_ext`
    [B, L, nJ_max, dim] and `grad_N` [B, L, nM_max] (numpy or torch, caller's joint numbering; a missing one is zero),
    or as `loss=`, a callable `(u, f_ext, N) -> (grad_u, grad_f_ext, grad_N)` on device tensors (entries may be None),
    called once per size bucket between the forward and the adjoint pass with that bucket's results
    [b, L, nJ_bucket, 3] / [b, L, nM_bucket] - for objectives that depend on the results (stress limits, displacement
    norms).  Buckets, member forms, `reorder` plans, `on_device` and `use_envelope` as `solve_load_cases`.
    Returns (`LoadCaseResult`, `GradientResult`); gradients not named in `want` come back as zeros."""
    packed = _as_packed(trusses_or_packed)
    B, nJ_max, nM_max = packed.B, packed.nJ_max, packed.nM_max
    cots = {"grad_u": grad_u, "grad_f_ext": grad_f_ext, "grad_N": grad_N}
    L = _check_gradient_args(B, nJ_max, nM_max, loads, cots, loss, sections)
    want = tuple(want)
    if any(k not in DeviceBatch.GRADIENTS for k in want):
        raise ValueError(f"solve_gradients: want must name some of {DeviceBatch.GRADIENTS}, got {want}")
    torch, dev = _require_gpu(device)
    cots = {k: _device_f64(torch, dev, g, vectors=k != "grad_N") for k, g in cots.items()}
    grads = _new_result(torch, dev, GradientResult, B, {"L": L, "nJ": nJ_max, "nM": nM_max})

    def adjoint(db, part, res):
        if loss is not None:
            gu, gf, gN = loss(res["u"], res["f_ext"], res["N"])
        else:
            gu, gf = part.cut(cots["grad_u"], nJ=2), part.cut(cots["grad_f_ext"], nJ=2)
            gN = part.cut(cots["grad_N"], nM=2)
        _put_result(part, grads, db.adjoint_cases(gu, gf, gN, want=want))   # (the gradients named in `want`)

    out = _load_cases_on_device(torch, dev, packed, _device_f64(torch, dev, loads, vectors=True), max_slab_bytes,
                                reorder, options, use_envelope, after=adjoint)
    grads.info = out.info
    return (out, grads) if on_device else (_host_result(torch, dev, out), _host_result(torch, dev, grads))


@dataclass
class ModeResult:
    """Results of `solve_modes`: eigenvalue [B, p] (lambda = omega^2 of K phi = lambda M phi, ascending; NaN beyond
    n_modes), omega [B, p] = sqrt(eigenvalue), shape [B, p, nJ_max, 3] (caller's joint numbering, M-orthonormal, zero at
    constrained DOFs, largest component positive; z = 0 for a 2D truss), residual [B, p] (relative, in the M-norm),
    n_modes [B] = min(p, free DOFs with mass), iters [B] (the iteration at which the truss's pairs were all below the
    tolerance; 0 = not within max_iters), info [B] (the factorisation's status: a truss with info != 0 has meaningless
    modes, the others are unaffected)."""
    eigenvalue: np.ndarray
    omega: np.ndarray
    shape: np.ndarray
    residual: np.ndarray
    n_modes: np.ndarray
    iters: np.ndarray
    info: np.ndarray

    # (`modes` returns no "omega": the field keeps its fill until `solve_modes` takes the root of the eigenvalues)
    FIELDS = {"eigenvalue": ("lam", float("nan"), "float64", ("P",)), "omega": ("omega", float("nan"), "float64", ("P",)),
              "shape": ("phi", 0.0, "float64", ("P", "nJ", 3)), "residual": ("resid", float("nan"), "float64", ("P",)),
              "n_modes": ("n_modes", 0, "int32", ()), "iters": ("iters", 0, "int32", ())}


def _check_p(who, p, note=""):
    if isinstance(p, bool) or int(p) != p or not 1 <= int(p) <= 8:
        raise ValueError(f"{who}: p must be an integer in 1 .. 8{note}, got {p!r}")


def _check_want(who, want, names):
    """`want` as a tuple of some of `names`."""
    if isinstance(want, str):
        raise ValueError(f"{who}: want must be a sequence of names out of {names}")
    want = tuple(want)
    if any(k not in names for k in want):
        raise ValueError(f"{who}: want must name some of {names}, got {want}")
    return want


def _check_damping(who, name, x):
    if isinstance(x, (bool, str)) or not isinstance(x, (int, float, np.integer, np.floating)) \
            or not (np.isfinite(x) and x >= 0):
        raise ValueError(f"{who}: {name} must be a non-negative finite number, got {x!r}")


def _mass_summary(joint_mass):
    """(shape, smallest entry - NaN when one is not finite) of a `joint_mass` (numpy or torch), (None, None) of None:
    what `_check_mode_args` is given."""
    if joint_mass is None:
        return None, None
    jm = _host_array(joint_mass, np.float64)
    return tuple(int(x) for x in joint_mass.shape), \
        (float(jm.min()) if jm.size else 0.0) if np.isfinite(jm).all() else float("nan")


def _mode_buckets(packed, dev, out, p, joint_mass, mass_scale, tol, max_iters, max_slab_bytes, reorder, options,
                  use_envelope):
    """The loop of the analyses on the mode block: `_factored_buckets`, `db.modes(p, ...)` per bucket, and
    (DeviceBatch, _Bucket, res) is yielded; the analysis adds its own results to the dict `res`, which then goes into
    `out` (`_put_result`).  At the end `out.omega` is the root of the eigenvalues."""
    for db, part in _factored_buckets(packed, dev, out.info, max_slab_bytes, reorder, options, use_envelope):
        res = db.modes(p, tol=tol, max_iters=max_iters, joint_mass=part.cut(joint_mass, nJ=1), mass_scale=mass_scale)
        yield db, part, res
        _put_result(part, out, res)
    out.omega = out.eigenvalue.sqrt()


def _check_mode_args(B, nJ_max, p, joint_mass_shape, mass_scale, tol, max_iters, check_every=8, joint_mass_min=None):
    """The argument errors of `solve_modes` / `DeviceBatch.modes` that need no device."""
    _check_p("modes", p, f" (one block of {MODES_BLOCK} vectors delivers at most 8 pairs)")
    if joint_mass_shape is not None and tuple(int(x) for x in joint_mass_shape) != (B, nJ_max):
        raise ValueError(f"modes: joint_mass must be [B={B}, nJ_max={nJ_max}], got {tuple(joint_mass_shape)}")
    if joint_mass_min is not None and not joint_mass_min >= 0:
        raise ValueError("modes: joint_mass must be non-negative and finite")
    if not (np.isfinite(mass_scale) and mass_scale >= 0):
        raise ValueError(f"modes: mass_scale must be non-negative and finite, got {mass_scale!r}")
    if not tol > 0:
        raise ValueError(f"modes: tol must be positive, got {tol!r}")
    if int(max_iters) < 1 or int(check_every) < 1:
        raise ValueError("modes: max_iters and check_every must be at least 1")


def solve_modes(trusses_or_packed, p=6, joint_mass=None, mass_scale=1.0, tol=1e-10, max_iters=256, device=None,
                reorder=False, options=None, max_slab_bytes=64 << 30, on_device=False, use_envelope=True):
    """The `p` (1 .. 8) lowest natural frequencies and mode shapes of every truss of a batch, from ONE factorisation per
    truss: lumped mass m_j = mass_scale * (half the mass a * length * density of every member at joint j) +
    joint_mass[b, j] on the three DOFs of a joint, block inverse iteration against the resident Cholesky factor
    (`DeviceBatch.factor` / `DeviceBatch.modes`, include/trs_modes.h).  `joint_mass`: [B, nJ_max] (numpy or torch,
    caller's joint numbering, non-negative) or None; `mass_scale`: 1 / g for densities given as weight densities.
    Buckets, member forms, `reorder` plans, `on_device` and `use_envelope` as `solve_load_cases`.  Returns a
    `ModeResult`."""
    packed = _as_packed(trusses_or_packed)
    B, nJ_max = packed.B, packed.nJ_max
    jm_shape, jm_min = _mass_summary(joint_mass)
    _check_mode_args(B, nJ_max, p, jm_shape, mass_scale, tol, max_iters, joint_mass_min=jm_min)
    p = int(p)
    torch, dev = _require_gpu(device)
    joint_mass = _device_f64(torch, dev, joint_mass)
    out = _new_result(torch, dev, ModeResult, B, {"P": p, "nJ": nJ_max})
    for _ in _mode_buckets(packed, dev, out, p, joint_mass, mass_scale, tol, max_iters, max_slab_bytes, reorder, options,
                           use_envelope):
        pass   # (the modes alone)
    return _finish_result(torch, dev, out, on_device)


@dataclass
class ModeGradientResult:
    """Results of `solve_mode_gradients`: eigenvalue, omega, gap, residual [B, p], n_modes, iters, info [B] as
    `ModeResult` (gap: the relative distance of eigenvalue k to the nearest other Ritz value of the truss's block, +inf
    where there is none, NaN beyond n_modes), and the gradients dA, dE, drho [B, R, nM_max] (per member, also in the
    table member form), dxyz [B, R, nJ_max, 3] (every joint, held ones included; z = 0 for a 2D truss) and djoint_mass
    [B, R, nJ_max] (caller's joint numbering).  R = p without weights (row k: the gradient of eigenvalue k; zeros
    beyond n_modes), R = 1 with weights (sum_k w_k row k).  d omega = d eigenvalue / (2 omega).  A row of a repeated
    eigenvalue (a gap of the order of the residual) means nothing alone; equal weights over a closed cluster always give
    the derivative of the cluster's sum.  A gradient that was not wanted is zeros."""
    eigenvalue: np.ndarray
    omega: np.ndarray
    gap: np.ndarray
    residual: np.ndarray
    n_modes: np.ndarray
    iters: np.ndarray
    dA: np.ndarray
    dE: np.ndarray
    drho: np.ndarray
    dxyz: np.ndarray
    djoint_mass: np.ndarray
    info: np.ndarray

    # (`modes` returns no "omega": the field keeps its fill until `solve_mode_gradients` takes the root)
    FIELDS = {"eigenvalue": ("lam", float("nan"), "float64", ("P",)), "omega": ("omega", float("nan"), "float64", ("P",)),
              "gap": ("gap", float("nan"), "float64", ("P",)), "residual": ("resid", float("nan"), "float64", ("P",)),
              "n_modes": ("n_modes", 0, "int32", ()), "iters": ("iters", 0, "int32", ()),
              "dA": ("A", 0.0, "float64", ("R", "nM")), "dE": ("E", 0.0, "float64", ("R", "nM")),
              "drho": ("rho", 0.0, "float64", ("R", "nM")), "dxyz": ("xyz", 0.0, "float64", ("R", "nJ", 3)),
              "djoint_mass": ("joint_mass", 0.0, "float64", ("R", "nJ"))}


def _check_mode_gradient_args(B, nJ_max, p, joint_mass_shape, mass_scale, tol, max_iters, weights=None, want=None,
                              sections=None, joint_mass_min=None):
    """The argument errors of `solve_mode_gradients` that need no device: those of `solve_modes`, and weights of the wrong
    shape or not finite (`weights`: a host array or None), unknown names in `want`, "joint_mass" wanted without masses,
    and `sections=`.  Returns `want` as a tuple (None: every gradient, "joint_mass" only when there are masses)."""
    _refuse_sections("solve_mode_gradients", "gradients", sections)
    _check_mode_args(B, nJ_max, p, joint_mass_shape, mass_scale, tol, max_iters, joint_mass_min=joint_mass_min)
    if want is None:
        want = tuple(k for k in DeviceBatch.MODE_GRADIENTS if k != "joint_mass" or joint_mass_shape is not None)
    want = _check_want("solve_mode_gradients", want, DeviceBatch.MODE_GRADIENTS)
    if "joint_mass" in want and joint_mass_shape is None:
        raise ValueError("solve_mode_gradients: 'joint_mass' is wanted, but no joint_mass was given")
    if weights is not None:
        got = tuple(int(x) for x in weights.shape)
        if got != (B, int(p)):
            raise ValueError(f"solve_mode_gradients: weights must be [B={B}, p={int(p)}], got {got}")
        if not np.isfinite(weights).all():
            raise ValueError("solve_mode_gradients: weights must be finite")
    return want


def solve_mode_gradients(trusses_or_packed, p=6, weights=None, joint_mass=None, mass_scale=1.0, want=None, tol=1e-10,
                         max_iters=256, device=None, reorder=False, options=None, max_slab_bytes=64 << 30,
                         on_device=False, use_envelope=True, sections=None):
    """`solve_modes` plus the derivatives of the eigenvalues lambda = omega^2 with respect to the member areas, moduli and
    densities, the joint coordinates and the non-structural joint masses: every truss is factored ONCE, its `p` lowest
    pairs are iterated, and one pass over the members with the converged block gives the gradients
    (`DeviceBatch.mode_gradients`, include/trs_modegrad.h; no finite differences, no further solve).  `weights` None:
    the Jacobian, one row per eigenvalue; `weights` [B, p] (numpy or torch, finite): the one row sum_k w_k d lambda_k.
    `want`: some of `DeviceBatch.MODE_GRADIENTS` (default: all, "joint_mass" only when `joint_mass` is given).  The other
    arguments as `solve_modes`.  Returns a `ModeGradientResult`; read its `gap` before trusting a single row."""
    packed = _as_packed(trusses_or_packed)
    B, nJ_max, nM_max = packed.B, packed.nJ_max, packed.nM_max
    jm_shape, jm_min = _mass_summary(joint_mass)
    want = _check_mode_gradient_args(B, nJ_max, p, jm_shape, mass_scale, tol, max_iters,
                                     weights=None if weights is None else _host_array(weights, np.float64), want=want,
                                     sections=sections, joint_mass_min=jm_min)
    p = int(p)
    torch, dev = _require_gpu(device)
    joint_mass, weights = _device_f64(torch, dev, joint_mass), _device_f64(torch, dev, weights)
    out = _new_result(torch, dev, ModeGradientResult, B,
                      {"P": p, "R": p if weights is None else 1, "nJ": nJ_max, "nM": nM_max})
    for db, part, res in _mode_buckets(packed, dev, out, p, joint_mass, mass_scale, tol, max_iters, max_slab_bytes,
                                       reorder, options, use_envelope):
        res.update(db.mode_gradients(weights=part.cut(weights), want=want))
    return _finish_result(torch, dev, out, on_device)


@dataclass
class SpectrumResult:
    """Results of `solve_response_spectrum`: eigenvalue, omega, residual [B, p], n_modes, iters, info [B] as `ModeResult`;
    gamma, sa, meff [B, G, p] (participation factor, spectral ordinate and effective-mass fraction of every mode per
    ground direction; zeros beyond n_modes), mtot, base [B, G] (the mass on free DOFs weighted by the direction, and the
    combined base shear); displace, reaction [B, G, nJ_max, 3] and force [B, G, nM_max] (the peaks per direction,
    combined over the modes: non-negative; displace zero at held DOFs, reaction zero at free ones); displace_all,
    reaction_all [B, nJ_max, 3] and force_all [B, nM_max] (SRSS over the G directions); with `want_modal` the signed
    modal values modal_displace, modal_reaction [B, G, p + 1, nJ_max, 3] and modal_force [B, G, p + 1, nM_max] (slot
    p: the missing-mass response), else None."""
    eigenvalue: np.ndarray
    omega: np.ndarray
    residual: np.ndarray
    n_modes: np.ndarray
    iters: np.ndarray
    gamma: np.ndarray
    sa: np.ndarray
    meff: np.ndarray
    mtot: np.ndarray
    base: np.ndarray
    displace: np.ndarray
    force: np.ndarray
    reaction: np.ndarray
    displace_all: np.ndarray
    force_all: np.ndarray
    reaction_all: np.ndarray
    modal_displace: np.ndarray
    modal_force: np.ndarray
    modal_reaction: np.ndarray
    info: np.ndarray

    # (`modes` returns no "omega" and `response_spectrum` no "*_all": `solve_response_spectrum` forms them with torch)
    FIELDS = {"eigenvalue": ("lam", float("nan"), "float64", ("P",)), "omega": ("omega", float("nan"), "float64", ("P",)),
              "residual": ("resid", float("nan"), "float64", ("P",)), "n_modes": ("n_modes", 0, "int32", ()),
              "iters": ("iters", 0, "int32", ()), "gamma": ("gamma", 0.0, "float64", ("G", "P")),
              "sa": ("sa", 0.0, "float64", ("G", "P")), "meff": ("meff", 0.0, "float64", ("G", "P")),
              "mtot": ("mtot", 0.0, "float64", ("G",)), "base": ("base", 0.0, "float64", ("G",)),
              "displace": ("u", 0.0, "float64", ("G", "nJ", 3)), "force": ("N", 0.0, "float64", ("G", "nM")),
              "reaction": ("R", 0.0, "float64", ("G", "nJ", 3)), "displace_all": ("u_all", 0.0, "float64", ("nJ", 3)),
              "force_all": ("N_all", 0.0, "float64", ("nM",)), "reaction_all": ("R_all", 0.0, "float64", ("nJ", 3)),
              "modal_displace": ("modal_u", 0.0, "float64", ("G", "V", "nJ", 3)),
              "modal_force": ("modal_N", 0.0, "float64", ("G", "V", "nM")),
              "modal_reaction": ("modal_R", 0.0, "float64", ("G", "V", "nJ", 3))}


def _check_spectrum_args(p, directions, periods, accel, damping=0.05, rule="cqc", zpa=None,
                         want=DeviceBatch.SPECTRUM_RESULTS):
    """The argument errors of `DeviceBatch.response_spectrum` / `solve_response_spectrum` that need no device.  Returns
    (directions [G, 3], periods [K], accel [G, K], zpa [G]) as host float64 arrays, the rule's code and `want` as a
    tuple."""
    who = "response_spectrum"
    _check_p(who, p)
    dirs = _host_array(directions, np.float64)
    if dirs.ndim != 2 or not 1 <= dirs.shape[0] <= 3 or dirs.shape[1] not in (2, 3):
        raise ValueError(f"{who}: directions must be [G, 3] (or [G, 2]) with 1 <= G <= 3, got {dirs.shape}")
    if dirs.shape[1] == 2:
        dirs = np.concatenate([dirs, np.zeros([len(dirs), 1])], axis=1)
    if not np.isfinite(dirs).all():
        raise ValueError(f"{who}: directions must be finite")
    G = len(dirs)
    T = _host_array(periods, np.float64)
    if T.ndim != 1 or not 2 <= T.size <= 64:
        raise ValueError(f"{who}: periods must be [K] with 2 <= K <= 64, got {T.shape}")
    if not (np.isfinite(T).all() and T[0] >= 0 and (np.diff(T) > 0).all()):
        raise ValueError(f"{who}: periods must be finite, non-negative and strictly ascending")
    Sa = _host_array(accel, np.float64)
    if Sa.shape != (G, T.size):
        raise ValueError(f"{who}: accel must be [G={G}, K={T.size}], got {Sa.shape}")
    if not (np.isfinite(Sa).all() and (Sa >= 0).all()):
        raise ValueError(f"{who}: accel must be finite and non-negative")
    if zpa is None:
        zpa = Sa[:, 0].copy()
    zpa = _host_array(zpa, np.float64)
    if zpa.shape != (G,) or not (np.isfinite(zpa).all() and (zpa >= 0).all()):
        raise ValueError(f"{who}: zpa must be [G={G}], finite and non-negative")
    if not isinstance(rule, str) or rule.lower() not in _capi.RS_RULES:
        raise ValueError(f"{who}: rule must be one of {sorted(_capi.RS_RULES)}, got {rule!r}")
    _check_damping(who, "damping", damping)
    if rule.lower() == "cqc" and not damping > 0:
        raise ValueError(f"{who}: rule 'cqc' needs damping > 0, got {damping!r}")
    want = _check_want(who, want, DeviceBatch.SPECTRUM_RESULTS)
    return dirs, T, Sa, zpa, _capi.RS_RULES[rule.lower()], want


def solve_response_spectrum(trusses_or_packed, directions, periods, accel, p=6, damping=0.05, rule="cqc",
                            missing_mass=True, zpa=None, joint_mass=None, mass_scale=1.0, want_modal=False, tol=1e-10,
                            max_iters=256, device=None, reorder=False, options=None, max_slab_bytes=64 << 30,
                            on_device=False, use_envelope=True):
    """The seismic response spectrum analysis of every truss of a batch, from ONE factorisation per truss: the `p`
    (1 .. 8) lowest modes (`solve_modes`: the same lumped mass, `joint_mass`, `mass_scale`), then per ground direction
    the participation factors, the spectral ordinates and the peak displacements, member forces and support reactions
    combined over the modes by `rule` ("srss", "cqc", "abs"), with the missing-mass correction by one more
    substitution against the resident factor (`DeviceBatch.response_spectrum`, include/trs_spectrum.h, where
    `directions`, `periods`, `accel`, `zpa` and `damping` are described; they are shared by the batch).  The G
    directions are combined by SRSS into displace_all, force_all and reaction_all.  The other arguments as
    `solve_modes`.  Returns a `SpectrumResult`."""
    packed = _as_packed(trusses_or_packed)
    B, nJ_max, nM_max = packed.B, packed.nJ_max, packed.nM_max
    jm_shape, jm_min = _mass_summary(joint_mass)
    _check_mode_args(B, nJ_max, p, jm_shape, mass_scale, tol, max_iters, joint_mass_min=jm_min)
    dirs, T, Sa, zpa, _, want = _check_spectrum_args(p, directions, periods, accel, damping, rule, zpa)
    p, G = int(p), len(dirs)
    torch, dev = _require_gpu(device)
    joint_mass = _device_f64(torch, dev, joint_mass)
    modal = ("modal_displace", "modal_force", "modal_reaction")
    out = _new_result(torch, dev, SpectrumResult, B, {"P": p, "G": G, "V": p + 1, "nJ": nJ_max, "nM": nM_max},
                      without=() if want_modal else modal)
    for db, part, res in _mode_buckets(packed, dev, out, p, joint_mass, mass_scale, tol, max_iters, max_slab_bytes,
                                       reorder, options, use_envelope):
        res.update(db.response_spectrum(dirs, T, Sa, damping=damping, rule=rule, missing_mass=missing_mass, zpa=zpa,
                                        want=want, want_modal=want_modal))
    out.displace_all = out.displace.square().sum(1).sqrt()
    out.force_all = out.force.square().sum(1).sqrt()
    out.reaction_all = out.reaction.square().sum(1).sqrt()
    return _finish_result(torch, dev, out, on_device)


@dataclass
class HarmonicResult:
    """Results of `solve_harmonic` for L harmonic excitations per truss over S forcing frequencies: eigenvalue, omega
    [B, p], n_modes, iters, info [B] as `ModeResult`; the envelopes displace, reaction [B, L, nJ_max, 3] and force
    [B, L, nM_max] (the largest steady-state amplitude over the sweep: non-negative; displace zero at held DOFs, reaction
    zero at free ones; relative to the ground when a ground acceleration was given), displace_at, force_at, reaction_at
    (int32: the first index of `omegas` that attains it) and displace_omega, force_omega, reaction_omega (the forcing
    frequency at that index); frf_displace [B, L, S, Pj, 3] and frf_force [B, L, S, Pm] (complex128: the response of the
    monitored joints and members at every frequency, u(t) = Re(frf e^(i W t)); zeros for a monitor id of -1).  The modes
    that were truncated respond statically (or not at all with residual=False): see `DeviceBatch.harmonic`."""
    eigenvalue: np.ndarray
    omega: np.ndarray
    n_modes: np.ndarray
    iters: np.ndarray
    displace: np.ndarray
    force: np.ndarray
    reaction: np.ndarray
    displace_at: np.ndarray
    force_at: np.ndarray
    reaction_at: np.ndarray
    displace_omega: np.ndarray
    force_omega: np.ndarray
    reaction_omega: np.ndarray
    frf_displace: np.ndarray
    frf_force: np.ndarray
    info: np.ndarray

    # (`modes` returns no "omega" and `harmonic` no "*_omega": `solve_harmonic` forms them with torch)
    FIELDS = {"eigenvalue": ("lam", float("nan"), "float64", ("P",)), "omega": ("omega", float("nan"), "float64", ("P",)),
              "n_modes": ("n_modes", 0, "int32", ()), "iters": ("iters", 0, "int32", ()),
              "displace": ("u_amp", 0.0, "float64", ("L", "nJ", 3)), "force": ("N_amp", 0.0, "float64", ("L", "nM")),
              "reaction": ("R_amp", 0.0, "float64", ("L", "nJ", 3)), "displace_at": ("u_at", 0, "int32", ("L", "nJ", 3)),
              "force_at": ("N_at", 0, "int32", ("L", "nM")), "reaction_at": ("R_at", 0, "int32", ("L", "nJ", 3)),
              "displace_omega": ("u_omega", 0.0, "float64", ("L", "nJ", 3)),
              "force_omega": ("N_omega", 0.0, "float64", ("L", "nM")),
              "reaction_omega": ("R_omega", 0.0, "float64", ("L", "nJ", 3)),
              "frf_displace": ("frf_u", 0.0, "complex128", ("L", "S", "Pj", 3)),
              "frf_force": ("frf_N", 0.0, "complex128", ("L", "S", "Pm"))}


def _check_harmonic_args(B, nJ_max, p, omegas, pattern_shape=None, accel=None, damping=0.02, damp_mass=0.0,
                         damp_stiff=0.0, want=DeviceBatch.HARMONIC_RESULTS, Pj=0, Pm=0, max_result_bytes=4 << 30):
    """The argument errors of `DeviceBatch.harmonic` / `solve_harmonic` that need no device (ValueError).
    `pattern_shape`: the shape of the load patterns ([B, L, nJ_max, 2 or 3]) or None.  Returns (omegas [S] as a host
    float64 array, accel [B, L, 3] as one or None, L, `want` as a tuple)."""
    who = "harmonic"
    _check_p(who, p)
    W = _host_array(omegas, np.float64)
    if W.ndim != 1 or W.size < 1:
        raise ValueError(f"{who}: omegas must be [S] with S >= 1, got {list(W.shape)}")
    if not (np.isfinite(W).all() and (W >= 0).all()):
        raise ValueError(f"{who}: omegas must be finite and non-negative")
    if pattern_shape is None and accel is None:
        raise ValueError(f"{who}: at least one of pattern and accel must be given")
    L = None
    if pattern_shape is not None:
        shape = tuple(int(v) for v in pattern_shape)
        if len(shape) != 4 or shape[0] != B or shape[2] != nJ_max or shape[3] not in (2, 3):
            raise ValueError(f"{who}: pattern must be [B={B}, L, nJ_max={nJ_max}, 2 or 3], got {list(shape)}")
        L = shape[1]
    ag = None
    if accel is not None:
        ag = _host_array(accel, np.float64)
        if ag.ndim not in (2, 3) or ag.shape[-1] not in (2, 3) or (ag.ndim == 3 and ag.shape[0] != B) \
                or (L is not None and ag.shape[-2] != L):
            raise ValueError(f"{who}: accel must be [L, 3] or [B={B}, L, 3] (or 2 components)"
                             + (f" with L={L} as pattern" if L is not None else "") + f", got {list(ag.shape)}")
        if not np.isfinite(ag).all():
            raise ValueError(f"{who}: accel must be finite")
        if ag.shape[-1] == 2:
            ag = np.concatenate([ag, np.zeros(ag.shape[:-1] + (1,))], axis=-1)
        if ag.ndim == 2:
            ag = np.broadcast_to(ag, (B,) + ag.shape)
        ag = np.array(ag, dtype=np.float64, order="C")   # (a copy: a broadcast view is not writable)
        L = int(ag.shape[1])
    if not 1 <= L <= MODES_BLOCK:
        raise ValueError(f"{who}: the number of cases L must be in 1 .. {MODES_BLOCK} (pattern or accel), got {L}")
    for name, x in (("damping", damping), ("damp_mass", damp_mass), ("damp_stiff", damp_stiff)):
        _check_damping(who, name, x)
    if not (damping > 0 or damp_mass > 0 or damp_stiff > 0):
        raise ValueError(f"{who}: at least one of damping, damp_mass and damp_stiff must be positive - an undamped mode "
                         "has no steady state at its own frequency")
    want = _check_want(who, want, DeviceBatch.HARMONIC_RESULTS)
    if Pj < 0 or Pm < 0:
        raise ValueError(f"{who}: monitor counts must not be negative")
    nbytes = 16 * B * L * int(W.size) * (3 * Pj + Pm)
    if nbytes > max_result_bytes:
        raise ValueError(f"{who}: the responses of {Pj} monitored joints and {Pm} members of B={B} trusses, L={L} cases "
                         f"at S={W.size} frequencies take {nbytes} bytes, more than max_result_bytes = {max_result_bytes}")
    return np.ascontiguousarray(W), ag, L, want


def solve_harmonic(trusses_or_packed, omegas, pattern=None, accel=None, p=6, damping=0.02, damp_mass=0.0, damp_stiff=0.0,
                   residual=True, monitor_joints=None, monitor_members=None, joint_mass=None, mass_scale=1.0, tol=1e-10,
                   max_iters=256, device=None, reorder=False, options=None, max_slab_bytes=64 << 30, on_device=False,
                   use_envelope=True, max_result_bytes=4 << 30):
    """The steady-state harmonic response of every truss of a batch over the forcing frequencies `omegas` [S], from ONE
    factorisation per truss: the `p` (1 .. 8) lowest modes (`solve_modes`: the same lumped mass, `joint_mass`,
    `mass_scale`), then per case the modal loads, the static correction for the truncated modes by one more substitution
    against the resident factor, and the sweep (`DeviceBatch.harmonic`, include/trs_harmonic.h, where `pattern`
    [B, L, nJ_max, dim], `accel` [L, dim] or [B, L, dim], the three dampings and `residual` are described, and what the
    static correction does NOT cover: frequencies near or above the first mode left out).  `monitor_joints` [B, Pj],
    `monitor_members` [B, Pm]: joint / member ids (-1: none) whose complex response at every frequency is returned.
    The other arguments as `solve_modes`.  Returns a `HarmonicResult`."""
    packed = _as_packed(trusses_or_packed)
    B, nJ_max, nM_max = packed.B, packed.nJ_max, packed.nM_max
    jm_shape, jm_min = _mass_summary(joint_mass)
    _check_mode_args(B, nJ_max, p, jm_shape, mass_scale, tol, max_iters, joint_mass_min=jm_min)
    mon = {}
    for name, ids, counts in (("monitor_joints", monitor_joints, packed.nJ), ("monitor_members", monitor_members, packed.nM)):
        x = np.zeros([B, 0], dtype=np.int32) if ids is None else _host_array(ids, None)
        if x.ndim != 2 or x.shape[0] != B or (x.size and not np.issubdtype(x.dtype, np.integer)):
            raise ValueError(f"harmonic: {name} must be an integer array [B={B}, P], got {x.dtype} {list(x.shape)}")
        if x.size and (np.any(x < -1) or np.any(x >= np.asarray(counts).reshape(-1, 1))):
            raise ValueError(f"harmonic: {name} has an id outside its truss (-1 = none)")
        mon[name] = np.ascontiguousarray(x, dtype=np.int32)
    Pj, Pm = mon["monitor_joints"].shape[1], mon["monitor_members"].shape[1]
    W, ag, L, want = _check_harmonic_args(B, nJ_max, p, omegas, None if pattern is None else np.shape(pattern), accel,
                                          damping, damp_mass, damp_stiff, Pj=Pj, Pm=Pm, max_result_bytes=max_result_bytes)
    p = int(p)
    torch, dev = _require_gpu(device)
    joint_mass = _device_f64(torch, dev, joint_mass)
    pattern, ag = _device_f64(torch, dev, pattern, vectors=True), _device_f64(torch, dev, ag)
    mon = {k: torch.from_numpy(x).to(dev) for k, x in mon.items()}
    out = _new_result(torch, dev, HarmonicResult, B,
                      {"P": p, "L": L, "S": int(W.size), "Pj": Pj, "Pm": Pm, "nJ": nJ_max, "nM": nM_max})
    for db, part, res in _mode_buckets(packed, dev, out, p, joint_mass, mass_scale, tol, max_iters, max_slab_bytes,
                                       reorder, options, use_envelope):
        res.update(db.harmonic(W, pattern=part.cut(pattern, nJ=2), accel=part.cut(ag), damping=damping,
                               damp_mass=damp_mass, damp_stiff=damp_stiff, residual=residual,
                               monitor_joints=part.cut(mon["monitor_joints"]) if Pj else None,
                               monitor_members=part.cut(mon["monitor_members"]) if Pm else None, want=want,
                               max_result_bytes=max_result_bytes))
    W_d = torch.from_numpy(W).to(dev)
    out.displace_omega = W_d[out.displace_at.long()]
    out.force_omega = W_d[out.force_at.long()]
    out.reaction_omega = W_d[out.reaction_at.long()]
    return _finish_result(torch, dev, out, on_device)


@dataclass
class TransientResult:
    """Results of `solve_transient` for L excitations per truss over the time points 0 .. T (T = `steps`).  The state at
    the last point: displace, velocity, acceleration [B, L, nJ_max, 3] (caller's joint numbering, zero at held DOFs;
    relative to the ground when a ground acceleration was given).  The envelopes over all points: peak_displace
    [B, L, nJ_max, 3] = max |u| per DOF with peak_displace_step (int32: the first point that attains it), force_max and
    force_min [B, L, nM_max] (signed member forces, tension positive) with force_max_step, force_min_step.  The
    histories of the monitored joints and members: history_displace [B, L, T + 1, Pj, 3], history_force
    [B, L, T + 1, Pm] (zeros for a monitor id of -1).  info [B]: the status of the factorisation of K + sigma M - a truss
    with info != 0 has meaningless numbers, the others are unaffected."""
    displace: np.ndarray
    velocity: np.ndarray
    acceleration: np.ndarray
    peak_displace: np.ndarray
    peak_displace_step: np.ndarray
    force_max: np.ndarray
    force_max_step: np.ndarray
    force_min: np.ndarray
    force_min_step: np.ndarray
    history_displace: np.ndarray
    history_force: np.ndarray
    info: np.ndarray

    FIELDS = {"displace": ("u", 0.0, "float64", ("L", "nJ", 3)), "velocity": ("v", 0.0, "float64", ("L", "nJ", 3)),
              "acceleration": ("a", 0.0, "float64", ("L", "nJ", 3)),
              "peak_displace": ("u_peak", 0.0, "float64", ("L", "nJ", 3)),
              "peak_displace_step": ("u_step", 0, "int32", ("L", "nJ", 3)),
              "force_max": ("N_max", 0.0, "float64", ("L", "nM")), "force_max_step": ("N_max_step", 0, "int32", ("L", "nM")),
              "force_min": ("N_min", 0.0, "float64", ("L", "nM")), "force_min_step": ("N_min_step", 0, "int32", ("L", "nM")),
              "history_displace": ("hist_u", 0.0, "float64", ("L", "T1", "Pj", 3)),
              "history_force": ("hist_N", 0.0, "float64", ("L", "T1", "Pm"))}


def _check_transient_args(packed, pattern, dt, steps, beta=0.25, gamma=0.5, damp_mass=0.0, damp_stiff=0.0, scale=None,
                          accel=None, monitor_joints=None, monitor_members=None, joint_mass=None, mass_scale=1.0,
                          sections=None, max_result_bytes=4 << 30):
    """The argument errors of `solve_transient` that need no device (ValueError).  Returns the arguments as contiguous
    host arrays: {"pattern" [B, L, nJ_max, 3], "scale" [B, L, T + 1] or None, "accel" [B, L, T + 1, 3] or None,
    "monitor_joints" [B, Pj], "monitor_members" [B, Pm] (int32), "joint_mass" [B, nJ_max] or None}."""
    who = "solve_transient"
    _refuse_sections(who, "the transient analysis", sections)
    newmark_constants(dt, beta, gamma, damp_mass, damp_stiff)
    _check_integer(who, "steps", steps)
    B, nJ_max, nM_max, T1 = packed.B, packed.nJ_max, packed.nM_max, int(steps) + 1
    flat = np.asarray(packed.dim).reshape(-1) == 2   # trusses embedded with z fixed

    def vectors(name, x, lead):
        x = _host_array(x, np.float64)
        if x.ndim != len(lead) + 1 or x.shape[:-1] != lead or x.shape[-1] not in (2, 3):
            raise ValueError(f"{who}: {name} must be {list(lead)} + [2 or 3], got {list(x.shape)}")
        if not np.isfinite(x).all():
            raise ValueError(f"{who}: {name} has a non-finite entry")
        if x.shape[-1] == 2:
            x = np.concatenate([x, np.zeros(x.shape[:-1] + (1,))], axis=-1)
        elif flat.any() and np.any(x[flat][..., 2] != 0.0):
            raise ValueError(f"{who}: {name} has a z component on a 2D truss")
        return np.ascontiguousarray(x)

    shape = tuple(np.shape(pattern)) if not hasattr(pattern, "shape") else tuple(int(v) for v in pattern.shape)
    if len(shape) != 4 or shape[0] != B or shape[1] < 1 or shape[2] != nJ_max:
        raise ValueError(f"{who}: pattern must be [B={B}, L >= 1, nJ_max={nJ_max}, 2 or 3], got {list(shape)}")
    L = shape[1]
    given = {"pattern": vectors("pattern", pattern, (B, L, nJ_max)), "scale": None, "accel": None, "joint_mass": None}
    if scale is not None:
        x = _host_array(scale, np.float64)
        if x.shape != (B, L, T1):
            raise ValueError(f"{who}: scale must be [B={B}, L={L}, steps + 1 = {T1}], got {list(x.shape)}")
        if not np.isfinite(x).all():
            raise ValueError(f"{who}: scale has a non-finite entry")
        given["scale"] = np.ascontiguousarray(x)
    if accel is not None:
        given["accel"] = vectors("accel", accel, (B, L, T1))
    for name, ids, counts in (("monitor_joints", monitor_joints, packed.nJ), ("monitor_members", monitor_members, packed.nM)):
        x = np.zeros([B, 0], dtype=np.int32) if ids is None else _host_array(ids, None)
        if x.ndim != 2 or x.shape[0] != B or (x.size and not np.issubdtype(x.dtype, np.integer)):
            raise ValueError(f"{who}: {name} must be an integer array [B={B}, P], got {x.dtype} {list(x.shape)}")
        if x.size and (np.any(x < -1) or np.any(x >= np.asarray(counts).reshape(-1, 1))):
            raise ValueError(f"{who}: {name} has an id outside its truss (-1 = none)")
        given[name] = np.ascontiguousarray(x, dtype=np.int32)
    if joint_mass is not None:
        x = _host_array(joint_mass, np.float64)
        finite = bool(np.isfinite(x).all())
        _check_mass_args(who, B, nJ_max, x.shape, mass_scale,
                         joint_mass_min=(float(x.min()) if x.size else 0.0) if finite else float("nan"))
        given["joint_mass"] = np.ascontiguousarray(x)
    else:
        _check_mass_args(who, B, nJ_max, None, mass_scale)
    Pj, Pm = given["monitor_joints"].shape[1], given["monitor_members"].shape[1]
    nbytes = B * L * (8 * (4 * 3 * nJ_max + 2 * nM_max + T1 * (3 * Pj + Pm)) + 4 * (3 * nJ_max + 2 * nM_max))
    if nbytes > max_result_bytes:
        raise ValueError(f"{who}: the results of B={B} trusses, L={L} cases and {T1} time points take {nbytes} bytes, more "
                         f"than max_result_bytes = {max_result_bytes}")
    return given


def solve_transient(trusses_or_packed, pattern, dt, steps, scale=None, accel=None, beta=0.25, gamma=0.5, damp_mass=0.0,
                    damp_stiff=0.0, joint_mass=None, mass_scale=1.0, monitor_joints=None, monitor_members=None,
                    device=None, reorder=False, options=None, on_device=False, sections=None, use_envelope=True,
                    max_slab_bytes=64 << 30, max_result_bytes=4 << 30):
    """The transient response of every truss of a batch to L excitations each, by Newmark time stepping
    (`beta`, `gamma`; the defaults are the unconditionally stable average acceleration) with step `dt` over `steps`
    steps, from ONE factorisation per truss (of K + sigma M; `DeviceBatch.factor_dynamic` / `DeviceBatch.transient`,
    include/trs_dynamics.h).  M u'' + C u' + K u = scale(t) P - M iota(accel(t)): lumped mass as `solve_modes`
    (`joint_mass` [B, nJ_max], `mass_scale`), Rayleigh damping C = damp_mass M + damp_stiff K, `pattern`
    [B, L, nJ_max, dim] the load pattern of every case (caller's joint numbering; dim 2 or 3), `scale` [B, L, steps + 1]
    its time function (None: 1, a step load), `accel` [B, L, steps + 1, dim] a ground acceleration (None: none; the
    displacements are then relative to the ground).  The start is at rest: u = v = 0, a = f(0) / M.
    `monitor_joints` [B, Pj], `monitor_members` [B, Pm]: joint / member ids (-1: none) whose histories are returned; the
    envelopes cover every DOF and member.  Buckets, member forms, `reorder` plans, `options`, `on_device` and
    `use_envelope` as `solve_load_cases`.  Bad arguments (`_check_transient_args`) raise ValueError before any device
    work; there is no continuation at this level (`DeviceBatch.transient` carries a state).  Returns a `TransientResult`."""
    packed = _as_packed(trusses_or_packed)
    given = _check_transient_args(packed, pattern, dt, steps, beta, gamma, damp_mass, damp_stiff, scale, accel,
                                  monitor_joints, monitor_members, joint_mass, mass_scale, sections, max_result_bytes)
    torch, dev = _require_gpu(device)
    L, T1 = int(given["pattern"].shape[1]), int(steps) + 1
    on = {k: _device_f64(torch, dev, given[k]) for k in ("pattern", "scale", "accel", "joint_mass")}
    mon = {k: torch.from_numpy(given[k]).to(dev) for k in ("monitor_joints", "monitor_members")}
    out = _new_result(torch, dev, TransientResult, packed.B,
                      {"L": L, "nJ": packed.nJ_max, "nM": packed.nM_max, "T1": T1,
                       "Pj": int(mon["monitor_joints"].shape[1]), "Pm": int(mon["monitor_members"].shape[1])})
    factor = lambda db, part: db.factor_dynamic(dt, beta, gamma, damp_mass, damp_stiff,
                                                joint_mass=part.cut(on["joint_mass"], nJ=1), mass_scale=mass_scale)
    for db, part in _factored_buckets(packed, dev, out.info, max_slab_bytes, reorder, options, use_envelope, factor=factor):
        _put_result(part, out, db.transient(part.cut(on["pattern"], nJ=2), int(steps), scale=part.cut(on["scale"]),
                                            accel=part.cut(on["accel"]), monitor_joints=part.cut(mon["monitor_joints"]),
                                            monitor_members=part.cut(mon["monitor_members"])))
    return _finish_result(torch, dev, out, on_device)


@dataclass
class NonlinearResult:
    """Results of `solve_nonlinear` over the S load steps, in the caller's joint numbering: displace, external
    [B, S, nJ_max, 3] (external: the applied load at free DOFs, the reaction at held ones), internal [B, S, nM_max]
    (member forces, tension positive), iterations and status (int32 [B, S]: 0 converged, 1 iteration limit, 2 tangent not
    positive definite - displace is then the last accepted iterate and iterations the number of accepted updates -, 3 not
    attempted because an earlier step failed), residual [B, S] = |lambda P - f_int|_inf over the free DOFs at the
    displacements returned.  info [B]: 0, or for a truss that ended with status 2 what the factorisation reported for the tangent
    that was not positive definite (k > 0: its pivot k), latched when the status was set."""
    displace: np.ndarray
    internal: np.ndarray
    external: np.ndarray
    iterations: np.ndarray
    status: np.ndarray
    residual: np.ndarray
    info: np.ndarray

    FIELDS = {"displace": ("u", 0.0, "float64", ("S", "nJ", 3)), "internal": ("N", 0.0, "float64", ("S", "nM")),
              "external": ("f_ext", 0.0, "float64", ("S", "nJ", 3)), "iterations": ("iters", 0, "int32", ("S",)),
              "status": ("status", 0, "int32", ("S",)), "residual": ("residual", 0.0, "float64", ("S",))}


def _check_nonlinear_args(packed, load_factors, tol=1e-9, max_iters=25, check_every=1, options=None, sections=None,
                          max_result_bytes=4 << 30):
    """The argument errors of `solve_nonlinear` that need no device (ValueError).  Returns the load factors as a list
    of floats."""
    who = "solve_nonlinear"
    _refuse_sections(who, "the nonlinear analysis", sections)
    if options and options.get("compact"):
        raise ValueError(f"{who}: options['compact'] leaves no slab that could be amended to the tangent")
    lams = _check_newton_args(who, load_factors, tol, max_iters, check_every)
    nbytes = packed.B * len(lams) * (8 * (6 * packed.nJ_max + packed.nM_max + 1) + 8)
    if nbytes > max_result_bytes:
        raise ValueError(f"{who}: the results of B={packed.B} trusses and {len(lams)} load steps take {nbytes} bytes, "
                         f"more than max_result_bytes = {max_result_bytes}")
    return lams


def solve_nonlinear(trusses_or_packed, load_factors=(1.0,), tol=1e-9, max_iters=25, check_every=1, device=None,
                    reorder=False, options=None, on_device=False, sections=None, use_envelope=True,
                    max_slab_bytes=64 << 30, max_result_bytes=4 << 30):
    """Geometrically nonlinear statics of every truss of a batch (large displacements, small strains; corotational
    bars, include/trs_nonlinear.h) under `load_factors` times its own loads, one load step per factor in the given order,
    each started from the previous step's displacements: Newton's method on the tangent stiffness, which has the
    sparsity of K and is factored in the batch's slab (`DeviceBatch.nonlinear`).  `tol`: a truss is converged when
    |lambda P - f_int|_inf <= tol |lambda P|_inf over its free DOFs; `max_iters` Newton iterations per step at most;
    `check_every`: how often the host looks whether every truss is done.  A truss whose tangent is not positive definite
    at an iterate (a limit point was passed: no path following here) stops with status 2 and its later steps get
    status 3; the other trusses are unaffected.  Buckets, member forms, `reorder` plans, `options`, `on_device` and
    `use_envelope` as `solve_load_cases`.  Bad arguments (`_check_nonlinear_args`) raise ValueError before any device
    work.  Returns a `NonlinearResult`."""
    packed = _as_packed(trusses_or_packed)
    lams = _check_nonlinear_args(packed, load_factors, tol, max_iters, check_every, options, sections, max_result_bytes)
    torch, dev = _require_gpu(device)
    out = _new_result(torch, dev, NonlinearResult, packed.B, {"S": len(lams), "nJ": packed.nJ_max, "nM": packed.nM_max})
    # (nothing to factor ahead: every Newton iteration assembles and factors its own tangent)
    for db, part in _factored_buckets(packed, dev, out.info, max_slab_bytes, reorder, options, use_envelope,
                                      factor=lambda db, part: None):
        _put_result(part, out, db.nonlinear(lams, tol=tol, max_iters=max_iters, check_every=check_every))
    return _finish_result(torch, dev, out, on_device)


@dataclass
class SizingResult:
    """Results of `solve_sizing`, in the caller's member order, all describing the last design of a truss that could be
    factored: areas, utilisation [B, nM_max] (required area / area: stress and member buckling only; <= 1 is feasible),
    governing (int32 [B, nM_max]: the load case whose requirement governs the member, -1 where the displacement ratio
    does and on the padding), weight [B] (sum of A L rho), disp_ratio [B] (largest joint displacement / allow_displace; 0
    without a limit), iterations [B] (resizings behind the returned design), status (int32 [B]: 0 converged, 1
    iteration limit, 2 a design could not be factored - the truss went back to the design before; with iterations 0 its
    areas are the initial ones and the other results zero), weight_history [B, max_iters + 1] (the weight of every design
    the truss analysed, zero beyond its own count), catalog_index (uint8 [B, nM_max], or None without a catalogue).
    info [B]: 0, or what the factorisation reported for the design that ended a truss with status 2."""
    areas: np.ndarray
    weight: np.ndarray
    utilisation: np.ndarray
    governing: np.ndarray
    disp_ratio: np.ndarray
    iterations: np.ndarray
    status: np.ndarray
    weight_history: np.ndarray
    catalog_index: np.ndarray
    info: np.ndarray

    FIELDS = {"areas": ("areas", 0.0, "float64", ("nM",)), "weight": ("weight", 0.0, "float64", ()),
              "utilisation": ("utilisation", 0.0, "float64", ("nM",)), "governing": ("governing", -1, "int32", ("nM",)),
              "disp_ratio": ("disp_ratio", 0.0, "float64", ()), "iterations": ("iterations", 0, "int32", ()),
              "status": ("status", 0, "int32", ()), "weight_history": ("weight_history", 0.0, "float64", ("H",)),
              "catalog_index": ("catalog_index", 0, "uint8", ("nM",))}


def _check_sizing_args(packed, loads=None, allow_tension=None, allow_compression=None, allow_displace=0.0, euler_kappa=0.0,
                       area_min=None, area_max=None, relax=1.0, tol=1e-4, max_iters=40, check_every=1, catalog=None,
                       options=None, sections=None, max_result_bytes=4 << 30):
    """The argument errors of `solve_sizing` that need no device (ValueError).  Returns the arguments checked: the dict
    of `_check_sizing_scalars` plus "loads" (a float64 host array [B, L, nJ_max, 3], or None for the batch's own loads)
    and "area_min" / "area_max" (each a float, or a float64 host array [B, nM_max])."""
    who = "solve_sizing"
    _refuse_variants(who, "the member sizing (it writes the sections)", sections, options)
    for name, x in (("allow_tension", allow_tension), ("allow_compression", allow_compression)):
        if x is None:
            raise ValueError(f"{who}: {name} must be given")
    B, nJ_max, nM_max = packed.B, packed.nJ_max, packed.nM_max
    val = _check_sizing_scalars(who, allow_tension, allow_compression, allow_displace, euler_kappa, relax, tol, max_iters,
                                check_every, catalog, B=B)
    val["loads"] = _check_case_loads(who, loads, B, nJ_max)
    (lo, lo_arr), (hi, hi_arr) = _check_area_bounds(who, area_min, area_max, B, packed.nM, nM_max)
    val["area_min"], val["area_max"] = (lo if lo_arr is None else lo_arr), (hi if hi_arr is None else hi_arr)
    live = np.arange(nM_max)[None, :] < np.asarray(packed.nM)[:, None]
    if B and not (np.asarray(packed.general().A if packed.is_table else packed.A)[live] > 0).all():
        raise ValueError(f"{who}: the initial design must be positive: every member's area > 0")
    nbytes = B * (nM_max * (8 + 8 + 4 + 1) + 8 * (val["max_iters"] + 1) + 32)
    if nbytes > max_result_bytes:
        raise ValueError(f"{who}: the results of B={B} trusses take {nbytes} bytes, more than max_result_bytes = "
                         f"{max_result_bytes}")
    return val


def solve_sizing(trusses_or_packed, loads=None, allow_tension=None, allow_compression=None, allow_displace=0.0,
                 euler_kappa=0.0, area_min=None, area_max=None, relax=1.0, tol=1e-4, max_iters=40, check_every=1,
                 catalog=None, device=None, reorder=False, options=None, on_device=False, sections=None, use_envelope=True,
                 max_slab_bytes=64 << 30, max_result_bytes=4 << 30):
    """Size the members of every truss of a batch by the stress-ratio method - fully stressed design with a displacement
    envelope (include/trs_sizing.h, `DeviceBatch.sizing`): analyse the design under all load cases, resize every member
    to what its worst case demands, repeat until the areas stop moving.  `loads`: [B, L, nJ_max, dim] (numpy or torch;
    the caller's joint numbering; dim 2 or 3) or None for the batch's own loads as one case; `allow_tension`,
    `allow_compression` (stresses, > 0), `allow_displace` (a joint displacement norm, 0: no limit) - each one number or
    one per truss, [B] -, `euler_kappa` (the
    member's second moment of area as I = kappa A^2: 1 / (4 pi) for a solid round bar, 0: no member buckling check);
    `area_min` > 0 and `area_max` >= `area_min`: scalars or [B, nM_max] (equal bounds fix a member); `relax` in (0, 1]
    damps the resizing, `tol` is the relative area change at which a truss is converged, `max_iters` the number of
    resizings at most, `check_every` how often the host looks whether every truss is done; `catalog`: ascending areas
    (1 to 256) to which the final design is rounded up, followed by one more analysis.  The initial design is the
    batch's own areas.  What the method is not: where the displacement limit governs, the design is feasible but not
    weight-optimal (every member is scaled alike), and on redundant trusses the convergence is linear.
    Every iteration factors its own design (`_factored_buckets` factors nothing ahead).  A table-form batch is converted
    with `.general()`: the sizing writes one area per member.  Buckets, `reorder` plans, `options`, `on_device` and
    `use_envelope` as `solve_load_cases`.  Bad arguments (`_check_sizing_args`) raise ValueError before any device work.
    Returns a `SizingResult`."""
    packed = _as_packed(trusses_or_packed)
    val = _check_sizing_args(packed, loads, allow_tension, allow_compression, allow_displace, euler_kappa, area_min,
                             area_max, relax, tol, max_iters, check_every, catalog, options, sections, max_result_bytes)
    if packed.is_table:
        packed = packed.general()
    torch, dev = _require_gpu(device)
    out = _new_result(torch, dev, SizingResult, packed.B, {"nM": packed.nM_max, "H": val["max_iters"] + 1},
                      without=() if val["catalog"] is not None else ("catalog_index",))
    on, bound = _upload_design_args(torch, dev, val)
    per_truss = lambda part, x: x[part.index] if isinstance(x, np.ndarray) else x
    for db, part in _factored_buckets(packed, dev, out.info, max_slab_bytes, reorder, options, use_envelope,
                                      factor=lambda db, part: None):
        _put_result(part, out, db.sizing(
            part.cut(on["loads"], nJ=2), allow_tension=per_truss(part, val["allow_tension"]),
            allow_compression=per_truss(part, val["allow_compression"]),
            allow_displace=per_truss(part, val["allow_displace"]), euler_kappa=val["euler_kappa"],
            area_min=bound(part, on["area_min"]),
            area_max=bound(part, on["area_max"]), relax=val["relax"], tol=val["tol"], max_iters=val["max_iters"],
            check_every=val["check_every"], catalog=val["catalog"]))
    return _finish_result(torch, dev, out, on_device)


@dataclass
class MinComplianceResult:
    """Results of `solve_min_compliance`, in the caller's member order, all describing the last design of a truss that
    could be factored: areas [B, nM_max], measure [B] (sum w A of the returned design: the target, from the first
    resizing on), compliance [B, L] (C_l = f_l.u_l), objective [B] (J = sum alpha_l C_l), objective_history
    [B, max_iters + 1] (J of every design the truss analysed, zero beyond its own count), sensitivity [B, nM_max]
    (s_m = -dJ/dA_m), multiplier [B] (of the last resizing computed: at the optimum s_m = multiplier w_m on every member
    strictly inside its bounds; 0 where the bounds alone decide), iterations [B] (resizings behind the returned design),
    status (int32 [B]: 0 converged, 1 iteration limit, 2 a design could not be factored - the truss went back to the
    design before; with iterations 0 its areas are the initial ones and the other results zero).
    info [B]: 0, or what the factorisation reported for the design that ended a truss with status 2."""
    areas: np.ndarray
    measure: np.ndarray
    compliance: np.ndarray
    objective: np.ndarray
    objective_history: np.ndarray
    sensitivity: np.ndarray
    multiplier: np.ndarray
    iterations: np.ndarray
    status: np.ndarray
    info: np.ndarray

    FIELDS = {"areas": ("areas", 0.0, "float64", ("nM",)), "measure": ("measure", 0.0, "float64", ()),
              "compliance": ("compliance", 0.0, "float64", ("L",)), "objective": ("objective", 0.0, "float64", ()),
              "objective_history": ("objective_history", 0.0, "float64", ("H",)),
              "sensitivity": ("sensitivity", 0.0, "float64", ("nM",)), "multiplier": ("multiplier", 0.0, "float64", ()),
              "iterations": ("iterations", 0, "int32", ()), "status": ("status", 0, "int32", ())}


def _check_min_compliance_args(packed, loads=None, alpha=None, target=None, measure="weight", eta=0.5, move=0.2,
                               area_min=None, area_max=None, tol=1e-4, max_iters=60, check_every=1, options=None,
                               sections=None, max_result_bytes=4 << 30):
    """The argument errors of `solve_min_compliance` that need no device (ValueError).  Returns the arguments checked:
    the dict of `_check_min_compliance_scalars` plus "loads" (a float64 host array [B, L, nJ_max, 3], or None for the
    batch's own loads), "target" (None, or a float64 array [B]) and "area_min" / "area_max" (each a float, or a float64
    host array [B, nM_max])."""
    who = "solve_min_compliance"
    _refuse_variants(who, "the compliance sizing (it writes the sections)", sections, options)
    B, nJ_max, nM_max = packed.B, packed.nJ_max, packed.nM_max
    host_loads = _check_case_loads(who, loads, B, nJ_max)
    L = 1 if host_loads is None else host_loads.shape[1]
    val = _check_min_compliance_scalars(who, alpha, measure, eta, move, tol, max_iters, check_every, L)
    val["loads"] = host_loads
    val["target"] = None if target is None else _check_target(who, target, B)
    (lo, lo_arr), (hi, hi_arr) = _check_area_bounds(who, area_min, area_max, B, packed.nM, nM_max)
    val["area_min"], val["area_max"] = (lo if lo_arr is None else lo_arr), (hi if hi_arr is None else hi_arr)
    live = np.arange(nM_max)[None, :] < np.asarray(packed.nM)[:, None]
    general = packed.general() if packed.is_table else packed
    if B and not (np.asarray(general.A)[live] > 0).all():
        raise ValueError(f"{who}: the initial design must be positive: every member's area > 0")
    if B and measure == "weight" and not (np.asarray(general.rho)[live] > 0).all():
        raise ValueError(f"{who}: measure='weight' needs a positive density rho on every member - a member with rho <= 0 "
                         "weighs nothing; use measure='volume'")
    nbytes = B * (nM_max * 16 + 8 * (val["max_iters"] + 1) + 8 * L + 40)
    if nbytes > max_result_bytes:
        raise ValueError(f"{who}: the results of B={B} trusses take {nbytes} bytes, more than max_result_bytes = "
                         f"{max_result_bytes}")
    return val


def solve_min_compliance(trusses_or_packed, loads=None, alpha=None, target=None, measure="weight", eta=0.5, move=0.2,
                         area_min=None, area_max=None, tol=1e-4, max_iters=60, check_every=1, device=None, reorder=False,
                         options=None, on_device=False, sections=None, use_envelope=True, max_slab_bytes=64 << 30,
                         max_result_bytes=4 << 30):
    """The stiffest design of every truss of a batch at a given weight (or volume): compliance sizing by the
    optimality-criteria method (include/trs_compliance.h, `DeviceBatch.min_compliance`).  The objective is
    J = sum_l `alpha`_l f_l.u_l over the load cases `loads` [B, L, nJ_max, dim] (numpy or torch; the caller's joint
    numbering; dim 2 or 3; None: the batch's own loads as one case); `alpha`: L weights >= 0, not all zero (None: ones);
    the constraint is sum w A = `target` with w = rho L0 (`measure` "weight") or L0 ("volume"); `target`: one number, one
    per truss [B], or None for the measure of the initial design, the batch's own areas.  `eta` in (0, 1] damps the
    resizing, `move` in (0, 1] limits the relative change of an area per resizing, `area_min` > 0 and `area_max` >=
    `area_min`: scalars or [B, nM_max] (equal bounds fix a member); `tol` is the relative area change at which a truss
    is converged, `max_iters` the number of resizings at most, `check_every` how often the host looks whether every
    truss is done.  What the method is not: there are no stress or displacement constraints (that is `solve_sizing`),
    members end on `area_min` rather than being removed, and with several weighted cases the fixed point can be
    approached slowly.  Every iteration factors its own design (`_factored_buckets` factors nothing
    ahead).  A table-form batch is converted with `.general()`.  `measure="weight"` is refused when a member has
    rho <= 0.  Buckets, `reorder` plans, `options`, `on_device` and `use_envelope` as `solve_load_cases`.  Bad arguments
    (`_check_min_compliance_args`) raise ValueError before any device work.  Returns a `MinComplianceResult`."""
    packed = _as_packed(trusses_or_packed)
    val = _check_min_compliance_args(packed, loads, alpha, target, measure, eta, move, area_min, area_max, tol, max_iters,
                                     check_every, options, sections, max_result_bytes)
    if packed.is_table:
        packed = packed.general()
    torch, dev = _require_gpu(device)
    L = 1 if val["loads"] is None else int(val["loads"].shape[1])
    out = _new_result(torch, dev, MinComplianceResult, packed.B, {"nM": packed.nM_max, "H": val["max_iters"] + 1, "L": L})
    on, bound = _upload_design_args(torch, dev, val)
    for db, part in _factored_buckets(packed, dev, out.info, max_slab_bytes, reorder, options, use_envelope,
                                      factor=lambda db, part: None):
        _put_result(part, out, db.min_compliance(
            part.cut(on["loads"], nJ=2), alpha=val["alpha"], target=None if val["target"] is None else val["target"][part.index],
            measure=val["measure"], eta=val["eta"], move=val["move"], area_min=bound(part, on["area_min"]),
            area_max=bound(part, on["area_max"]), tol=val["tol"], max_iters=val["max_iters"],
            check_every=val["check_every"]))
    return _finish_result(torch, dev, out, on_device)


@dataclass
class MinWeightResult:
    """Results of `solve_min_weight`, in the caller's member order, all describing the last design of a truss that could
    be factored: areas [B, nM_max], measure [B] (sum w A of the returned design), measure_history, worst_history
    [B, max_iters + 1] (the measure and the largest g_j / limit_value_j of every design the truss analysed, zero beyond
    its own count), displacement [B, J] (g_j = d_j.u_{l_j}(joint_j)), ratio [B, J] (g_j / limit_value_j; 0 for a limit that
    is switched off), multipliers [B, J] (of the last dual solve: at the optimum sum_j mu_j c_mj = w_m on every member
    strictly inside its bounds and move limits, and mu_j = 0 for a limit with slack), sensitivity [B, J, nM_max]
    (c_mj = -dg_j/dA_m; None unless asked for), iterations [B] (resizings behind the returned design), status (int32 [B]:
    0 converged within limit_tol of its limits, 1 iteration limit, 2 a design could not be factored - the truss went back
    to the design before; with iterations 0 its areas are the initial ones and the other results zero -, 3 converged on
    its bounds without meeting a limit).  info [B]: 0, or what the factorisation reported for the design that ended a
    truss with status 2.  With stress limits (None without): utilisation [B, nM_max] (req / A of the returned design: the
    stress-ratio area of its worst case over its area; <= 1 is feasible), governing (int32 [B, nM_max]: that case, -1
    where no case asks for any area and on the padding), stress_history [B, max_iters + 1] (the largest utilisation of
    every design the truss analysed); status 0 then asks the utilisation too for <= 1 + limit_tol."""
    areas: np.ndarray
    measure: np.ndarray
    measure_history: np.ndarray
    worst_history: np.ndarray
    displacement: np.ndarray
    ratio: np.ndarray
    multipliers: np.ndarray
    sensitivity: np.ndarray
    utilisation: np.ndarray
    governing: np.ndarray
    stress_history: np.ndarray
    iterations: np.ndarray
    status: np.ndarray
    info: np.ndarray

    #: ("G": the number of limits g_j, J of the header)
    FIELDS = {"areas": ("areas", 0.0, "float64", ("nM",)), "measure": ("measure", 0.0, "float64", ()),
              "measure_history": ("measure_history", 0.0, "float64", ("H",)),
              "worst_history": ("worst_history", 0.0, "float64", ("H",)),
              "displacement": ("displacement", 0.0, "float64", ("G",)), "ratio": ("ratio", 0.0, "float64", ("G",)),
              "multipliers": ("multipliers", 0.0, "float64", ("G",)),
              "sensitivity": ("sensitivity", 0.0, "float64", ("G", "nM")),
              "utilisation": ("utilisation", 0.0, "float64", ("nM",)), "governing": ("governing", -1, "int32", ("nM",)),
              "stress_history": ("stress_history", 0.0, "float64", ("H",)),
              "iterations": ("iterations", 0, "int32", ()), "status": ("status", 0, "int32", ())}


def _check_min_weight_args(packed, loads=None, limit_case=None, limit_joint=None, limit_direction=None, limit_value=None,
                           measure="weight", move=0.2, area_min=None, area_max=None, tol=1e-4, max_iters=60, sweeps=2,
                           limit_tol=1e-2, check_every=1, want_sensitivity=False, options=None, sections=None,
                           max_result_bytes=4 << 30, allow_tension=None, allow_compression=None, euler_kappa=0.0):
    """The argument errors of `solve_min_weight` that need no device (ValueError).  Returns the arguments checked: the
    dict of `_check_min_weight_scalars` plus "loads" (a float64 host array [B, L, nJ_max, 3], or None for the batch's own
    loads), "limits" (the dict of `_check_limits`), "want_sensitivity" and "area_min" / "area_max" (each a float, or a
    float64 host array [B, nM_max]) and "stress" (the dict of `_check_stress_limits`, or None)."""
    who = "solve_min_weight"
    _refuse_variants(who, "the minimum-weight sizing (it writes the sections)", sections, options)
    B, nJ_max, nM_max = packed.B, packed.nJ_max, packed.nM_max
    host_loads = _check_case_loads(who, loads, B, nJ_max)
    L = 1 if host_loads is None else host_loads.shape[1]
    val = _check_min_weight_scalars(who, measure, move, tol, max_iters, sweeps, limit_tol, check_every)
    if not isinstance(want_sensitivity, (bool, np.bool_)):
        raise ValueError(f"{who}: want_sensitivity must be True or False, got {want_sensitivity!r}")
    val["want_sensitivity"] = bool(want_sensitivity)
    val["stress"] = _check_stress_limits(who, allow_tension, allow_compression, euler_kappa, B)
    val["loads"] = host_loads
    if limit_case is None or limit_joint is None or limit_direction is None or limit_value is None:
        raise ValueError(f"{who}: limit_case, limit_joint, limit_direction and limit_value must be given")
    val["limits"] = _check_limits(who, limit_case, limit_joint, limit_direction, limit_value, B, nJ_max, L, packed.nJ)
    J = int(val["limits"]["case"].size)
    (lo, lo_arr), (hi, hi_arr) = _check_area_bounds(who, area_min, area_max, B, packed.nM, nM_max)
    val["area_min"], val["area_max"] = (lo if lo_arr is None else lo_arr), (hi if hi_arr is None else hi_arr)
    live = np.arange(nM_max)[None, :] < np.asarray(packed.nM)[:, None]
    general = packed.general() if packed.is_table else packed
    if B and not (np.asarray(general.A)[live] > 0).all():
        raise ValueError(f"{who}: the initial design must be positive: every member's area > 0")
    if B and measure == "weight" and not (np.asarray(general.rho)[live] > 0).all():
        raise ValueError(f"{who}: measure='weight' needs a positive density rho on every member - a member with rho <= 0 "
                         "weighs nothing; use measure='volume'")
    nbytes = B * (8 * nM_max * (1 + J * val["want_sensitivity"]) + 16 * (val["max_iters"] + 1) + 24 * J + 24)
    if val["stress"] is not None:
        nbytes += B * (12 * nM_max + 8 * (val["max_iters"] + 1))
    if nbytes > max_result_bytes:
        raise ValueError(f"{who}: the results of B={B} trusses take {nbytes} bytes, more than max_result_bytes = "
                         f"{max_result_bytes}")
    return val


def solve_min_weight(trusses_or_packed, loads=None, limit_case=None, limit_joint=None, limit_direction=None,
                     limit_value=None, measure="weight", move=0.2, area_min=None, area_max=None, tol=1e-4, max_iters=60,
                     sweeps=2, limit_tol=1e-2, check_every=1, want_sensitivity=False, device=None, reorder=False,
                     options=None, on_device=False, sections=None, use_envelope=True, max_slab_bytes=64 << 30,
                     max_result_bytes=4 << 30, allow_tension=None, allow_compression=None, euler_kappa=0.0):
    """The lightest design of every truss of a batch whose named joint displacements stay within named limits: the
    optimality-criteria method with one multiplier per limit (include/trs_minweight.h, `DeviceBatch.min_weight`).  The
    objective is sum w A with w = rho L0 (`measure` "weight") or L0 ("volume"); limit j means
    d_j.u_{l_j}(joint_j) <= `limit_value`_j under load case l_j = `limit_case`[j] of `loads` [B, L, nJ_max, dim] (numpy or
    torch; the caller's joint numbering; dim 2 or 3; None: the batch's own loads as one case); `limit_joint`: integers
    [J] or [B, J] (-1 switches a limit off for that truss), `limit_direction`: [J, dim] or [B, J, dim] (normalised here),
    `limit_value`: a number, [J] or [B, J], > 0 (+inf switches a limit off); 1 <= J <= 8; a two-sided limit is two limits
    with +-d.  `move` in (0, 1] limits the relative change of an area per resizing, `area_min` > 0 and `area_max` >=
    `area_min`: scalars or [B, nM_max] (equal bounds fix a member); `tol` is the relative area change at which a truss is
    converged, `limit_tol` how far above its limits a converged truss may lie and still get status 0 (else 3),
    `max_iters` the number of resizings at most, `sweeps` the passes of the dual solve over the limits, `check_every` how
    often the host looks whether every truss is done.  Stress limits in the same run: `allow_tension` and
    `allow_compression` (both or neither; each a number > 0 or one per truss [B]; +inf switches a side off) and
    `euler_kappa` >= 0, as `solve_sizing` takes them - every analysis makes the stress-ratio area of a member's worst
    case the member's lower bound in the resizing, and the result gains utilisation, governing and stress_history
    (`DeviceBatch.min_weight`); without them the three are None.  What the method is not: the stress floor
    is the stress-ratio estimate, exact only where the member forces do not depend on the areas; there are at most 8
    named displacement limits, not an envelope over all joints; a large `move` can stall on small members, and a truss
    with many members on the floor converges slowly; no linked member groups, no limits on reactions, and with several
    limits that compete for the same members the resizing can approach its fixed point slowly or cycle inside its move
    limits.  Every
    iteration factors its own design (`_factored_buckets` factors nothing ahead).  A table-form batch is converted with
    `.general()`.  `measure="weight"` is refused when a member has rho <= 0.  Buckets, `reorder` plans, `options`,
    `on_device` and `use_envelope` as `solve_load_cases`.  Bad arguments (`_check_min_weight_args`) raise ValueError
    before any device work.  Returns a `MinWeightResult`."""
    packed = _as_packed(trusses_or_packed)
    val = _check_min_weight_args(packed, loads, limit_case, limit_joint, limit_direction, limit_value, measure, move,
                                 area_min, area_max, tol, max_iters, sweeps, limit_tol, check_every, want_sensitivity,
                                 options, sections, max_result_bytes, allow_tension, allow_compression, euler_kappa)
    if packed.is_table:
        packed = packed.general()
    torch, dev = _require_gpu(device)
    lim = val["limits"]
    sizes = {"nM": packed.nM_max, "H": val["max_iters"] + 1, "G": int(lim["case"].size)}
    stress = val["stress"]
    out = _new_result(torch, dev, MinWeightResult, packed.B, sizes,
                      without=(() if val["want_sensitivity"] else ("sensitivity",)) + (_MW_STRESS_KEYS if stress is None else ()))
    cut = lambda part, x: x[part.index] if isinstance(x, np.ndarray) else x   # (an allowable per truss: the bucket's)
    on, bound = _upload_design_args(torch, dev, val)
    for db, part in _factored_buckets(packed, dev, out.info, max_slab_bytes, reorder, options, use_envelope,
                                      factor=lambda db, part: None):
        _put_result(part, out, db.min_weight(
            part.cut(on["loads"], nJ=2), limit_case=lim["case"], limit_joint=lim["joint"][part.index],
            limit_direction=lim["given"][part.index], limit_value=lim["value"][part.index], measure=val["measure"],
            move=val["move"], area_min=bound(part, on["area_min"]), area_max=bound(part, on["area_max"]), tol=val["tol"],
            max_iters=val["max_iters"], sweeps=val["sweeps"], limit_tol=val["limit_tol"],
            check_every=val["check_every"], want_sensitivity=val["want_sensitivity"],
            **({} if stress is None else {"allow_tension": cut(part, stress["allow_tension"]),
                                          "allow_compression": cut(part, stress["allow_compression"]),
                                          "euler_kappa": stress["euler_kappa"]})))
    return _finish_result(torch, dev, out, on_device)


@dataclass
class UnilateralResult:
    """Results of `solve_unilateral`, per truss and load case, all describing the state the truss ended with: displace,
    external [B, L, nJ_max, 3] (the caller's joint numbering), internal [B, L, nM_max] (0 in a member removed exactly),
    state (int8 [B, L, nM_max]: 1 active, 0 slack and on the padding; bilateral members are always 1), status (int32
    [B, L]: 0 converged, 1 iteration limit, 2 a structure could not be factored - the truss went back to the state
    before), iterations [B, L] (rounds of flips behind the returned state), violations (int32 [B, L]: the members that
    still want to flip in the returned state; 0 when converged), flips_history (int32 [B, L, max_iters + 1]: the flips
    of every analysis, zero beyond the truss's own count), areas_effective [B, L, nM_max].  info [B]: 0, or what the
    factorisation reported in the first case that ended the truss with status 2."""
    displace: np.ndarray
    external: np.ndarray
    internal: np.ndarray
    state: np.ndarray
    status: np.ndarray
    iterations: np.ndarray
    violations: np.ndarray
    flips_history: np.ndarray
    areas_effective: np.ndarray
    info: np.ndarray

    #: one load case, as `DeviceBatch.unilateral` returns it; FIELDS puts the case axis in front
    CASE_FIELDS = {"displace": ("u", 0.0, "float64", ("nJ", 3)), "external": ("f_ext", 0.0, "float64", ("nJ", 3)),
                   "internal": ("N", 0.0, "float64", ("nM",)), "state": ("state", 0, "int8", ("nM",)),
                   "status": ("status", 0, "int32", ()), "iterations": ("iterations", 0, "int32", ()),
                   "violations": ("violations", 0, "int32", ()), "flips_history": ("flips_history", 0, "int32", ("H",)),
                   "areas_effective": ("areas_effective", 0.0, "float64", ("nM",))}
    FIELDS = {field: (key, fill, dtype, ("L",) + shape) for field, (key, fill, dtype, shape) in CASE_FIELDS.items()}


def _check_unilateral_args(packed, kind, loads=None, prestrain=None, slack_factor=0.0, max_iters=20, check_every=1,
                           state=None, options=None, sections=None, max_result_bytes=4 << 30):
    """The argument errors of `solve_unilateral` that need no device (ValueError).  Returns the arguments checked:
    "kind" (int8 [B, nM_max], zero on the padding), "loads" (float64 [B, L, nJ_max, 3] or None for the batch's own
    loads), "prestrain" (float64 [B, L, nM_max] or None), "state" (int8 [B, nM_max] of 0 / 1, or None), "L",
    "slack_factor", "max_iters", "check_every"."""
    who = "solve_unilateral"
    _refuse_variants(who, "unilateral members (the iteration writes the areas)", sections, options)
    B, nJ_max, nM_max = packed.B, packed.nJ_max, packed.nM_max
    val = {"slack_factor": _check_number(who, "slack_factor", slack_factor, "be a finite number >= 0", least=0),
           "max_iters": _check_integer(who, "max_iters", max_iters, least=0),
           "check_every": _check_integer(who, "check_every", check_every)}
    live = np.arange(nM_max)[None, :] < np.asarray(packed.nM).reshape(B, 1)

    def members(name, x, what):
        try:
            x = _host_array(x, np.float64)
        except (TypeError, ValueError):
            x = None
        if x is None or x.shape != (B, nM_max) or not np.isfinite(x).all():
            raise ValueError(f"{who}: {name} must be [B={B}, nM_max={nM_max}] of {what}, got "
                             f"{None if x is None else x.shape}")
        return np.where(live, x, 0.0)
    if kind is None:
        raise ValueError(f"{who}: kind must be given")
    k = members("kind", kind, "0 (bilateral), 1 (tension-only) and -1 (compression-only)")
    if not np.isin(k, (-1.0, 0.0, 1.0)).all():
        raise ValueError(f"{who}: kind must hold 0 (bilateral), 1 (tension-only) or -1 (compression-only)")
    val["kind"] = np.ascontiguousarray(k.astype(np.int8))
    val["state"] = None
    if state is not None:
        val["state"] = np.ascontiguousarray((members("state", state, "1 (active) and 0 (slack)") != 0).astype(np.int8))
    val["loads"], val["prestrain"] = _check_case_loads(who, loads, B, nJ_max), None
    L = None if val["loads"] is None else val["loads"].shape[1]
    if prestrain is not None:
        try:
            x = _host_array(prestrain, np.float64)
        except (TypeError, ValueError):
            x = None
        shape = None if x is None else tuple(x.shape)
        if x is None or len(shape) != 3 or shape[0] != B or shape[1] < 1 or shape[2] != nM_max or not np.isfinite(x).all():
            raise ValueError(f"{who}: prestrain must be finite [B={B}, L >= 1, nM_max={nM_max}], got {shape}")
        if L is not None and shape[1] != L:
            raise ValueError(f"{who}: prestrain has L = {shape[1]}, loads L = {L}")
        val["prestrain"], L = np.ascontiguousarray(x), shape[1]
    val["L"] = 1 if L is None else L
    nbytes = B * val["L"] * (8 * 6 * nJ_max + (8 + 8 + 1) * nM_max + 4 * (val["max_iters"] + 1) + 12)
    if nbytes > max_result_bytes:
        raise ValueError(f"{who}: the results of B={B} trusses take {nbytes} bytes, more than max_result_bytes = "
                         f"{max_result_bytes}")
    return val


def solve_unilateral(trusses_or_packed, kind, loads=None, prestrain=None, slack_factor=0.0, max_iters=20, check_every=1,
                     state=None, device=None, reorder=False, options=None, on_device=False, sections=None,
                     use_envelope=True, max_slab_bytes=64 << 30, max_result_bytes=4 << 30):
    """Analyse every truss of a batch with members that carry tension only or compression only - cables, tie rods,
    slender counter-bracing, struts that bear against a seat - by the active-set iteration (include/trs_unilateral.h,
    `DeviceBatch.unilateral`): analyse, switch off every unilateral member that is strained the wrong way, switch on
    every one that would be strained the right way, repeat until nothing changes.  `kind`: [B, nM_max] of 0 (bilateral),
    1 (tension-only), -1 (compression-only); `loads`: [B, L, nJ_max, dim] (numpy or torch; the caller's joint numbering;
    dim 2 or 3) or None for the batch's own loads; `prestrain`: [B, L, nM_max] member initial strains as
    `solve_effect_cases` takes them (pretension is a negative eps0) or None; both given agree on L.  Every case is an
    independent run from the nominal areas - the active set differs per case, so the cases share the upload and nothing
    else - looped on the resident bucket.  `slack_factor` >= 0: the fraction of its area a slack member keeps (0 removes
    it exactly; a small positive value lets the iteration walk through states in which a joint has lost its last
    support); `max_iters`: rounds of flips at most; `check_every`: how often the host looks whether every truss is
    done; `state`: [B, nM_max] initial state of every case (1 active, 0 slack; None: all active).  What the method is
    not: the answer is the linear small-displacement one - no cable sag, no geometric stiffness -, all flips are made at
    once, which can cycle (status 1 with `violations` > 0), and self-weight is not re-formed with the effective areas:
    pass it as joint loads.  A table-form batch is converted with `.general()`.  Buckets, `reorder` plans,
    `options`, `on_device` and `use_envelope` as `solve_load_cases`.  Bad arguments (`_check_unilateral_args`) raise
    ValueError before any device work.  Returns a `UnilateralResult`."""
    packed = _as_packed(trusses_or_packed)
    val = _check_unilateral_args(packed, kind, loads, prestrain, slack_factor, max_iters, check_every, state, options,
                                 sections, max_result_bytes)
    if packed.is_table:
        packed = packed.general()
    torch, dev = _require_gpu(device)
    L = val["L"]
    out = _new_result(torch, dev, UnilateralResult, packed.B,
                      {"L": L, "nJ": packed.nJ_max, "nM": packed.nM_max, "H": val["max_iters"] + 1})
    up = lambda x: None if x is None else torch.from_numpy(x).to(dev)
    on = {k: up(val[k]) for k in ("kind", "state", "loads", "prestrain")}
    case = lambda x, l: None if x is None else x[:, l].contiguous()
    for db, part in _factored_buckets(packed, dev, out.info, max_slab_bytes, reorder, options, use_envelope,
                                      factor=lambda db, part: None):
        kinds, states = part.cut(on["kind"], nM=1), part.cut(on["state"], nM=1)
        forces, strains = part.cut(on["loads"], nJ=2), part.cut(on["prestrain"], nM=2)
        _per_case_runs(torch, db, part, out, L, lambda l: db.unilateral(
            kinds, case(forces, l), case(strains, l), slack_factor=val["slack_factor"], max_iters=val["max_iters"],
            check_every=val["check_every"], state=states))
    return _finish_result(torch, dev, out, on_device)


@dataclass
class PlasticResult:
    """Results of `solve_plastic`, per truss and load case, all describing the equilibrium state of the truss's last
    completed event: displace, external [B, L, nJ_max, 3] (the caller's joint numbering; external is lambda P at the free
    DOFs and the reactions at the held ones), internal [B, L, nM_max], state (int8 [B, L, nM_max]: 0 elastic and on the
    padding, +1 yielded in tension, -1 in compression), status (int32 [B, L]: 0 lambda_max reached, 1 event limit, 2
    mechanism - load_factor is the collapse load -, 3 displacement limit), events [B, L], load_factor [B, L], and per
    analysis k lambda_history, umax_history [B, L, max_events + 1] (the pushover curve), member_history (int32: the
    governing member, -1 a release, -2 the terminal analysis), count_history (the members yielded or released), zero
    beyond the truss's own count; areas_effective [B, L, nM_max].  info [B]: 0, or what the factorisation reported in the
    first case that ended the truss as a mechanism its tangent could not be factored for."""
    displace: np.ndarray
    external: np.ndarray
    internal: np.ndarray
    state: np.ndarray
    status: np.ndarray
    events: np.ndarray
    load_factor: np.ndarray
    lambda_history: np.ndarray
    umax_history: np.ndarray
    member_history: np.ndarray
    count_history: np.ndarray
    areas_effective: np.ndarray
    info: np.ndarray

    #: one load case, as `DeviceBatch.plastic` returns it; FIELDS puts the case axis in front
    CASE_FIELDS = {"displace": ("u", 0.0, "float64", ("nJ", 3)), "external": ("f_ext", 0.0, "float64", ("nJ", 3)),
                   "internal": ("N", 0.0, "float64", ("nM",)), "state": ("state", 0, "int8", ("nM",)),
                   "status": ("status", 0, "int32", ()), "events": ("events", 0, "int32", ()),
                   "load_factor": ("load_factor", 0.0, "float64", ()),
                   "lambda_history": ("lambda_history", 0.0, "float64", ("H",)),
                   "umax_history": ("umax_history", 0.0, "float64", ("H",)),
                   "member_history": ("member_history", 0, "int32", ("H",)),
                   "count_history": ("count_history", 0, "int32", ("H",)),
                   "areas_effective": ("areas_effective", 0.0, "float64", ("nM",))}
    FIELDS = {field: (key, fill, dtype, ("L",) + shape) for field, (key, fill, dtype, shape) in CASE_FIELDS.items()}


def _check_plastic_scalars(who, hardening, lambda_max, disp_limit, collapse_ratio, tie_tol, max_events, check_every):
    """The scalar rules of the collapse-load analysis (ValueError), for `DeviceBatch.plastic` and `solve_plastic`."""
    return {"hardening": _check_number(who, "hardening", hardening, "be a finite number >= 0", least=0),
            "lambda_max": _check_number(who, "lambda_max", lambda_max, "be a finite number > 0", above=0),
            "disp_limit": _check_number(who, "disp_limit", disp_limit, "be a finite number >= 0 (0: no limit)", least=0),
            "collapse_ratio": _check_number(who, "collapse_ratio", collapse_ratio, "be a finite number > 1", above=1),
            "tie_tol": _check_number(who, "tie_tol", tie_tol, "be a finite number >= 0", least=0),
            "max_events": _check_integer(who, "max_events", max_events, least=0),
            "check_every": _check_integer(who, "check_every", check_every)}


def _check_plastic_args(packed, cap_tension, cap_compression, loads=None, hardening=0.0, lambda_max=1.0, disp_limit=0.0,
                        collapse_ratio=1e8, tie_tol=1e-9, max_events=64, check_every=1, options=None, sections=None,
                        max_result_bytes=4 << 30):
    """The argument errors of `solve_plastic` that need no device (ValueError).  Returns the arguments checked:
    "cap_tension", "cap_compression" (float64 [B, nM_max], 1 on the padding), "loads" (float64 [B, L, nJ_max, 3] or None
    for the batch's own loads), "L" and the scalars."""
    who = "solve_plastic"
    _refuse_variants(who, "the collapse-load analysis (the iteration writes the areas)", sections, options,
                     "load pattern")
    B, nJ_max, nM_max = packed.B, packed.nJ_max, packed.nM_max
    val = _check_plastic_scalars(who, hardening, lambda_max, disp_limit, collapse_ratio, tie_tol, max_events, check_every)
    live = np.arange(nM_max)[None, :] < np.asarray(packed.nM).reshape(B, 1)
    for name, x in (("cap_tension", cap_tension), ("cap_compression", cap_compression)):
        try:
            x = None if x is None else _host_array(x, np.float64)
        except (TypeError, ValueError):
            x = None
        if x is None or x.shape != (B, nM_max):
            raise ValueError(f"{who}: {name} must be [B={B}, nM_max={nM_max}] of positive forces, got "
                             f"{None if x is None else x.shape}")
        x = np.where(live, x, 1.0)
        if not (np.isfinite(x) & (x > 0)).all():
            raise ValueError(f"{who}: {name} must be positive and finite")
        val[name] = np.ascontiguousarray(x)
    val["loads"] = _check_case_loads(who, loads, B, nJ_max)
    val["L"] = L = 1 if val["loads"] is None else val["loads"].shape[1]
    nbytes = B * L * (8 * 6 * nJ_max + (8 + 8 + 1) * nM_max + 24 * (val["max_events"] + 1) + 16)
    if nbytes > max_result_bytes:
        raise ValueError(f"{who}: the results of B={B} trusses take {nbytes} bytes, more than max_result_bytes = "
                         f"{max_result_bytes}")
    return val


def solve_plastic(trusses_or_packed, cap_tension, cap_compression, loads=None, hardening=0.0, lambda_max=1.0,
                  disp_limit=0.0, collapse_ratio=1e8, tie_tol=1e-9, max_events=64, check_every=1, device=None,
                  reorder=False, options=None, on_device=False, sections=None, use_envelope=True,
                  max_slab_bytes=64 << 30, max_result_bytes=4 << 30):
    """The collapse load of every truss of a batch - how much of a load pattern it carries before it becomes a mechanism,
    and in which order its members give way - by the event-to-event elastic-plastic analysis (include/trs_plastic.h,
    `DeviceBatch.plastic`): a member that reaches its capacity goes on carrying it while the rest of a redundant truss
    picks up the difference.  `cap_tension`, `cap_compression`: [B, nM_max] positive member capacities (forces);
    `loads`: [B, L, nJ_max, dim] load patterns (numpy or torch; the caller's joint numbering; dim 2 or 3) or None for
    the batch's own loads.  Every case is an independent run from the nominal areas, looped on the resident bucket.
    `hardening` >= 0: the fraction of its stiffness a yielded member keeps (0: perfectly plastic); `lambda_max` > 0 and
    `disp_limit` >= 0 (0: none) end a run; `collapse_ratio` > 1, `tie_tol` >= 0, `max_events` and `check_every` as
    `DeviceBatch.plastic`.  What the method is not: one proportional load pattern with no constant dead
    load beside it, no pre-strain, small displacements, and a compression capacity is a plateau, not a post-buckling
    drop; release and re-yield can cycle at a degenerate point, which ends as status 1.  A table-form batch is converted
    with `.general()`.  Buckets, `reorder` plans, `options`, `on_device` and `use_envelope` as `solve_load_cases`.  Bad
    arguments (`_check_plastic_args`) raise ValueError before any device work.  Returns a `PlasticResult`."""
    packed = _as_packed(trusses_or_packed)
    val = _check_plastic_args(packed, cap_tension, cap_compression, loads, hardening, lambda_max, disp_limit,
                              collapse_ratio, tie_tol, max_events, check_every, options, sections, max_result_bytes)
    if packed.is_table:
        packed = packed.general()
    torch, dev = _require_gpu(device)
    L = val["L"]
    out = _new_result(torch, dev, PlasticResult, packed.B,
                      {"L": L, "nJ": packed.nJ_max, "nM": packed.nM_max, "H": val["max_events"] + 1})
    up = lambda x: None if x is None else torch.from_numpy(x).to(dev)
    on = {k: up(val[k]) for k in ("cap_tension", "cap_compression", "loads")}
    case = lambda x, l: None if x is None else x[:, l].contiguous()
    scalars = {k: val[k] for k in ("hardening", "lambda_max", "disp_limit", "collapse_ratio", "tie_tol", "max_events",
                                   "check_every")}
    for db, part in _factored_buckets(packed, dev, out.info, max_slab_bytes, reorder, options, use_envelope,
                                      factor=lambda db, part: None):
        tension, compression = part.cut(on["cap_tension"], nM=1), part.cut(on["cap_compression"], nM=1)
        # (the padding of a bucket narrower or wider than the batch: a capacity that passes the check)
        live = torch.arange(db.nM_max, device=dev)[None, :] < db.nM[:, None]
        tension, compression = (torch.where(live, x, torch.ones_like(x)) for x in (tension, compression))
        forces = part.cut(on["loads"], nJ=2)
        _per_case_runs(torch, db, part, out, L, lambda l: db.plastic(tension, compression, case(forces, l), **scalars))
    return _finish_result(torch, dev, out, on_device)


@dataclass
class BucklingResult:
    """Results of `solve_buckling`: factor [B, p] (the load factors lambda of K phi = lambda H phi nearest the truss's
    final shift, nearest first, signed: a positive one scales the loads as applied, a negative one the reversed loads;
    NaN beyond n_modes), critical [B] (the smallest positive factor; NaN where none was found), critical_mode [B] (its
    place in `factor`, -1: none), bound [B] (every positive factor is >= bound: the critical factor where one was found,
    +inf where the truss has none, else the last proven value), shift, rounds [B] (the truss's last shift and how many
    rounds it took part in), iters [B] (the iteration at which its last round converged, 0: it did not), residual [B, p]
    (|H phi - nu Kbar phi|_2 / |nu Kbar phi|_2), n_modes [B], shape [B, p, nJ_max, 3] (caller's joint numbering, largest
    component +1, zero at held DOFs and beyond n_modes), status [B] (`BK_FOUND` 0, `BK_NONE` 1, `BK_SHIFT_LIMIT` 2,
    `BK_ITER_LIMIT` 3, `BK_NOT_PD` 4) and info [B] (the status of the truss's last factorisation: for info != 0 in round 0
    the truss has NaN factors, the others are unaffected)."""
    factor: np.ndarray
    critical: np.ndarray
    critical_mode: np.ndarray
    bound: np.ndarray
    shift: np.ndarray
    rounds: np.ndarray
    iters: np.ndarray
    residual: np.ndarray
    n_modes: np.ndarray
    shape: np.ndarray
    status: np.ndarray
    info: np.ndarray

    FIELDS = {"factor": ("factor", float("nan"), "float64", ("P",)), "critical": ("critical", float("nan"), "float64", ()),
              "critical_mode": ("critical_mode", -1, "int32", ()), "bound": ("bound", 0.0, "float64", ()),
              "shift": ("shift", 0.0, "float64", ()), "rounds": ("rounds", 0, "int32", ()), "iters": ("iters", 0, "int32", ()),
              "residual": ("residual", float("nan"), "float64", ("P",)), "n_modes": ("n_modes", 0, "int32", ()),
              "shape": ("shape", 0.0, "float64", ("P", "nJ", 3)), "status": ("status", BK_SHIFT_LIMIT, "int32", ())}


def _check_buckling_args(p, shift=0.0, max_shifts=6, tol=1e-10, max_iters=256, check_every=4, options=None):
    """The argument errors of `solve_buckling` / `DeviceBatch.buckling` that need no device (ValueError)."""
    who = "buckling"
    if isinstance(p, bool) or not isinstance(p, (int, np.integer)) or not 1 <= int(p) <= 8:
        raise ValueError(f"{who}: p must be an integer in 1 .. 8 (one block of {MODES_BLOCK} vectors delivers at most 8 "
                         f"pairs), got {p!r}")
    _check_number(who, "shift", shift, "be a finite number >= 0", least=0)
    _check_number(who, "tol", tol, "be a finite positive number", above=0, types=_REAL_NO_NPINT)
    for name, x in (("max_shifts", max_shifts), ("max_iters", max_iters), ("check_every", check_every)):
        _check_integer(who, name, x)
    if options and options.get("compact"):
        raise ValueError(f"{who}: options['compact'] leaves no slab that could be amended to K + theta Kg")


def solve_buckling(trusses_or_packed, p=4, shift=0.0, max_shifts=6, tol=1e-10, max_iters=256, check_every=4, device=None,
                   reorder=False, options=None, max_slab_bytes=64 << 30, on_device=False, use_envelope=True):
    """Linear buckling of every truss of a batch under its own loads: by what factor can the load grow before the truss
    buckles?  Per truss the `p` (1 .. 8) load factors nearest its final shift, signed, and `critical`, the smallest
    positive one, found by block inverse iteration on factors of K + theta Kg with a sequence of provably safe shifts
    (`DeviceBatch.buckling`, include/trs_buckling.h).  `shift`, `max_shifts`: the first shift and the number of rounds at
    most (`max_shifts=1`: the plain signed analysis at `shift`).  Buckles of single members (Euler) are not part of it.
    Buckets, member forms, `reorder` plans, `options`, `on_device` and `use_envelope` as `solve_load_cases`.  Bad
    arguments raise ValueError before any device work.  Returns a `BucklingResult`."""
    packed = _as_packed(trusses_or_packed)
    _check_buckling_args(p, shift, max_shifts, tol, max_iters, check_every, options)
    torch, dev = _require_gpu(device)
    out = _new_result(torch, dev, BucklingResult, packed.B, {"P": int(p), "nJ": packed.nJ_max})
    for db, part in _factored_buckets(packed, dev, out.info, max_slab_bytes, reorder, options, use_envelope):
        _put_result(part, out, db.buckling(p, shift=shift, max_shifts=max_shifts, tol=tol, max_iters=max_iters,
                                           check_every=check_every))
    return _finish_result(torch, dev, out, on_device)


@dataclass
class MemberLossResult:
    """Results of `solve_member_loss`.  The intact truss: displace/external [B, L, nJ_max, 3], internal [B, L, nM_max] (as
    `LoadCaseResult`).  Per removed member e: redundancy [B, nM_max] (r_e in [0, 1]; the r of a truss sum to its degree
    of statical indeterminacy nM - n_free), critical [B, nM_max] (bool: r_e <= r_tol - without e the truss is a
    mechanism), and per load case peak_stress, peak_displace [B, L, nM_max] (the largest |N'| / A among the surviving
    members and the largest joint displacement after the removal; +inf for a critical member) with peak_member,
    peak_joint [B, L, nM_max] (where: member id, caller's joint id; -1 where there is none), internal_after
    [B, L, nM_max, nM_max] (`want_forces`, else None: row e the member forces without e, NaN for a critical member).
    Padding members: zeros, ids -1.  info [B]: the factorisation's status - a truss with info != 0 has meaningless
    numbers, the others are unaffected."""
    displace: np.ndarray
    external: np.ndarray
    internal: np.ndarray
    redundancy: np.ndarray
    critical: np.ndarray
    peak_stress: np.ndarray
    peak_member: np.ndarray
    peak_displace: np.ndarray
    peak_joint: np.ndarray
    internal_after: np.ndarray
    info: np.ndarray

    FIELDS = dict(LoadCaseResult.FIELDS, redundancy=("r", 0.0, "float64", ("nM",)), critical=("critical", 0, "bool", ("nM",)),
                  **_peak_fields("L", "nM"), internal_after=("N_after", 0.0, "float64", ("L", "nM", "nM")))


def _check_column_args(who, what, packed, loads, r_tol, sections, chunk):
    """The argument errors that `solve_member_loss` and `solve_member_sets` (`who`) share.  Returns the loads as a
    contiguous float64 host array [B, L, nJ_max, 3] (`loads=None`: the batch's own loads as one case)."""
    _refuse_sections(who, f"the {what} analysis", sections)
    _check_number(who, "r_tol", r_tol, "lie in (0, 1)", above=0, below=1, types=_REAL_NO_NPINT)
    _check_integer(who, "chunk", chunk)
    B, nJ_max = packed.B, packed.nJ_max
    x = np.asarray(packed.loads, dtype=np.float64)[:, None] if loads is None else _host_array(loads, np.float64)
    shape = tuple(x.shape)
    if len(shape) != 4 or shape[0] != B or shape[2] != nJ_max or shape[3] not in (2, 3):
        raise ValueError(f"{who}: loads must be [B={B}, L, nJ_max={nJ_max}, 2 or 3], got {shape}")
    if not np.isfinite(x).all():
        raise ValueError(f"{who}: loads has a non-finite entry")
    if shape[3] == 2:
        x = np.concatenate([x, np.zeros(shape[:3] + (1,))], axis=-1)
    return np.ascontiguousarray(x)


def _check_member_loss_args(packed, loads, r_tol, sections, want_forces=False, max_result_bytes=4 << 30, chunk=64):
    """The argument errors of `solve_member_loss` that need no device.  Returns the loads as a contiguous float64 host
    array [B, L, nJ_max, 3] (`loads=None`: the batch's own loads as one case)."""
    x = _check_column_args("solve_member_loss", "member-loss", packed, loads, r_tol, sections, chunk)
    B, nM_max, shape = packed.B, packed.nM_max, x.shape
    if want_forces and B * shape[1] * nM_max * nM_max * 8 > max_result_bytes:
        raise ValueError(f"solve_member_loss: internal_after [B={B}, L={shape[1]}, {nM_max}, {nM_max}] takes "
                         f"{B * shape[1] * nM_max * nM_max * 8} bytes, more than max_result_bytes = {max_result_bytes}")
    return x


def solve_member_loss(trusses_or_packed, loads=None, r_tol=MEMBER_LOSS_R_TOL, want_forces=False, device=None,
                      reorder=False, options=None, max_slab_bytes=64 << 30, on_device=False, sections=None,
                      use_envelope=True, chunk=64, max_result_bytes=4 << 30):
    """Robustness screening: what the loss of any ONE member does to every truss of a batch - whether it is still stable,
    and the worst member stress and joint displacement afterwards under each of L load cases - from ONE factorisation
    per truss.  Removing member e changes K_ff by the rank-one term k_e b_e b_e^T, so one more substitution column
    z_e = inv(K_ff) b_e per member gives everything exactly: the redundancy r_e = 1 - k_e b_e . z_e (r_e <= `r_tol`: the
    member is critical), and with alpha = N_e / r_e the state u + alpha z_e, N_m + alpha k_m b_m . z_e after the removal
    (`DeviceBatch.member_loss`, include/trs_loss.h).  `loads`: [B, L, nJ_max, dim] (numpy or torch, caller's joint
    numbering; dim 2 or 3), or None for the batch's own loads as one case.  `want_forces`: also the member forces after
    every removal, [B, L, nM_max, nM_max] - refused above `max_result_bytes`.  Buckets, member forms, `reorder` plans,
    `options`, `on_device` and `use_envelope` as `solve_load_cases`; `chunk`: members per substitution (`member_loss`; its
    buffer of B * chunk * rows doubles per bucket comes on top of `max_slab_bytes`).  `sections=` variants, non-finite
    loads, an `r_tol` outside (0, 1) and a `chunk` below 1 raise ValueError before any device work.  Returns a `MemberLossResult`."""
    packed = _as_packed(trusses_or_packed)
    loads = _check_member_loss_args(packed, loads, r_tol, sections, want_forces, max_result_bytes, chunk)
    torch, dev = _require_gpu(device)
    L = int(loads.shape[1])
    loads = _device_f64(torch, dev, loads)
    out = _new_result(torch, dev, MemberLossResult, packed.B, {"L": L, "nJ": packed.nJ_max, "nM": packed.nM_max},
                      without=() if want_forces else ("internal_after",))
    for db, part in _factored_buckets(packed, dev, out.info, max_slab_bytes, reorder, options, use_envelope, cases=L):
        _put_result(part, out, db.member_loss(part.cut(loads, nJ=2), r_tol=r_tol, want_forces=want_forces, chunk=chunk,
                                              max_result_bytes=max_result_bytes))
    return _finish_result(torch, dev, out, on_device)


@dataclass
class MemberSetResult:
    """Results of `solve_member_sets`.  The intact truss: displace/external [B, L, nJ_max, 3], internal [B, L, nM_max] (as
    `LoadCaseResult`).  Per scenario s: pivot [B, S, 8] (the pivots of the elimination in the set's order - for removals
    the redundancy of member j once the members before it are gone; NaN beyond the set and after a failing position),
    unstable [B, S] (bool: some pivot <= r_tol), first_unstable [B, S] (the position in the set from which the truss is a
    mechanism, else -1), and per load case peak_stress, peak_displace [B, L, S] (the largest |N'| / (gamma A) among the
    members that are not removed and the largest joint displacement; +inf for an unstable scenario) with peak_member,
    peak_joint [B, L, S] (member id, caller's joint id; -1 where there is none), internal_after [B, L, S, nM_max]
    (`want_forces`, else None) and displace_after [B, L, S, nJ_max, 3] (`want_displace`, else None; NaN for an unstable
    scenario).  info [B]: the factorisation's status - a truss with info != 0 has meaningless numbers, the others are
    unaffected."""
    displace: np.ndarray
    external: np.ndarray
    internal: np.ndarray
    pivot: np.ndarray
    unstable: np.ndarray
    first_unstable: np.ndarray
    peak_stress: np.ndarray
    peak_member: np.ndarray
    peak_displace: np.ndarray
    peak_joint: np.ndarray
    internal_after: np.ndarray
    displace_after: np.ndarray
    info: np.ndarray

    FIELDS = dict(LoadCaseResult.FIELDS, pivot=("pivot", float("nan"), "float64", ("S", MEMBER_SETS_MAX)),
                  unstable=("unstable", 0, "bool", ("S",)), first_unstable=("first_unstable", -1, "int32", ("S",)),
                  **_peak_fields("L", "S"), internal_after=("N_after", 0.0, "float64", ("L", "S", "nM")),
                  displace_after=("u_after", 0.0, "float64", ("L", "S", "nJ", 3)))


def _check_member_sets_args(packed, sets, factors, loads, r_tol, sections, want_forces=False, want_displace=False,
                            max_result_bytes=4 << 30, chunk=64):
    """The argument errors of `solve_member_sets` that need no device.  Returns host arrays: sets int32 [B, S, 8],
    factors float64 [B, S, 8] or None, loads float64 [B, L, nJ_max, 3]."""
    loads = _check_column_args("solve_member_sets", "member-set", packed, loads, r_tol, sections, chunk)
    B, nJ_max, nM_max = packed.B, packed.nJ_max, packed.nM_max
    sets, factors = _member_set_arrays("solve_member_sets", sets, factors, B, packed.nM, nM_max)
    extra = 8 * B * int(loads.shape[1]) * int(sets.shape[1]) * (nM_max * bool(want_forces) + 3 * nJ_max * bool(want_displace))
    if extra > max_result_bytes:
        raise ValueError(f"solve_member_sets: internal_after / displace_after of [B={B}, L={loads.shape[1]}, "
                         f"S={sets.shape[1]}] scenarios take {extra} bytes, more than max_result_bytes = {max_result_bytes}")
    return sets, factors, loads


def solve_member_sets(trusses_or_packed, sets, factors=None, loads=None, r_tol=MEMBER_LOSS_R_TOL, want_forces=False,
                      want_displace=False, device=None, reorder=False, options=None, max_slab_bytes=64 << 30,
                      on_device=False, sections=None, use_envelope=True, chunk=64, max_result_bytes=4 << 30):
    """Scenario screening: what happens to every truss of a batch when up to eight of its members are removed, damaged
    or strengthened AT ONCE - "these two diagonals and that chord go together", "this bay corrodes to half its section",
    "double those four members" - for S scenarios per truss, from ONE factorisation per truss.  A scenario changes K_ff
    by sum_j (gamma_j - 1) k_j b_j b_j^T, of rank k <= 8: the columns z_j = inv(K_ff) b_j of its members and one k x k
    elimination in the set's order give the state exactly (`DeviceBatch.member_sets`, include/trs_sets.h); the pivots of
    that elimination tell whether - and from which member of the set on - the truss is a mechanism.  `sets`: a list (per
    truss) of lists (per scenario) of member-id lists, or an integer array [B, S, K <= 8] with -1 padding at the end of
    a set; an empty set gives the intact state (trusses with fewer scenarios are padded with it).  `factors`: the area
    factor gamma of every named member in the same form (0 removed, below 1 damaged, above 1 strengthened, 1 unchanged),
    or None: every member removed.  `loads`: [B, L, nJ_max, dim] (numpy or torch, caller's joint numbering; dim 2 or 3),
    or None for the batch's own loads as one case.  `want_forces`, `want_displace`: also the member forces and the
    joint displacements of every scenario - together refused above `max_result_bytes`.  Buckets, member forms, `reorder`
    plans, `options`, `on_device`, `use_envelope` and `chunk` as `solve_member_loss`.  An id outside [0, nM[b]), an id
    twice in a set, more than 8 members in a set, a negative or non-finite factor, `sections=` variants, non-finite
    loads, an `r_tol` outside (0, 1) and a `chunk` below 1 raise ValueError before any device work.  Returns a
    `MemberSetResult`."""
    packed = _as_packed(trusses_or_packed)
    sets, factors, loads = _check_member_sets_args(packed, sets, factors, loads, r_tol, sections, want_forces,
                                                   want_displace, max_result_bytes, chunk)
    torch, dev = _require_gpu(device)
    L = int(loads.shape[1])
    loads = _device_f64(torch, dev, loads)
    out = _new_result(torch, dev, MemberSetResult, packed.B,
                      {"L": L, "S": int(sets.shape[1]), "nJ": packed.nJ_max, "nM": packed.nM_max},
                      without=(() if want_forces else ("internal_after",)) + (() if want_displace else ("displace_after",)))
    for db, part in _factored_buckets(packed, dev, out.info, max_slab_bytes, reorder, options, use_envelope, cases=L):
        _put_result(part, out, db.member_sets(
            part.cut(loads, nJ=2), sets[part.index], None if factors is None else factors[part.index], r_tol=r_tol,
            want_forces=want_forces, want_displace=want_displace, chunk=chunk, max_result_bytes=max_result_bytes))
    return _finish_result(torch, dev, out, on_device)


@dataclass
class InfluenceResult:
    """Results of `solve_influence`, per member [B, nM_max]: N_max, N_min (the largest and the smallest force the load
    train puts into the member as it crosses the path), x_max, x_min (the arc positions of the lead axle that attain
    them; NaN for a padding member or an empty path), area_pos, area_neg (the integrals of the positive and the negative
    part of the influence line over the path: times a line load, the extremes under a uniform live load); lines
    [B, nM_max, P_max] (`want_lines`, else None: the influence ordinates at the path joints, zero past a truss's path).
    Padding members: zeros.  info [B]: the factorisation's status - a truss with info != 0 has meaningless numbers, the
    others are unaffected."""
    N_max: np.ndarray
    N_min: np.ndarray
    x_max: np.ndarray
    x_min: np.ndarray
    area_pos: np.ndarray
    area_neg: np.ndarray
    lines: np.ndarray
    info: np.ndarray

    FIELDS = {"N_max": ("N_max", 0.0, "float64", ("nM",)), "N_min": ("N_min", 0.0, "float64", ("nM",)),
              "x_max": ("x_max", float("nan"), "float64", ("nM",)), "x_min": ("x_min", float("nan"), "float64", ("nM",)),
              "area_pos": ("area_pos", 0.0, "float64", ("nM",)), "area_neg": ("area_neg", 0.0, "float64", ("nM",)),
              "lines": ("eta", 0.0, "float64", ("nM", "P"))}


def _check_influence_args(packed, path, direction, train, sections, want_lines=False, max_result_bytes=4 << 30, chunk=64):
    """The argument errors of `solve_influence` that need no device (the last one needs the library).  Returns host
    arrays: path int32 [B, P_max] (-1 padding), path_len int32 [B], direction float64 [B, 3], train_w, train_o [A]."""
    _refuse_sections("solve_influence", "the influence analysis", sections)
    _check_integer("solve_influence", "chunk", chunk)
    B, nJ_max, nM_max = packed.B, packed.nJ_max, packed.nM_max
    # the path: a list of joint-id lists, or [B, P_max] with -1 padding
    if isinstance(path, (list, tuple)) and all(isinstance(row, (list, tuple)) for row in path):
        rows = [[int(j) for j in row] for row in path]
        if len(rows) != B:
            raise ValueError(f"solve_influence: path must hold one list of joints per truss (B={B}), got {len(rows)}")
        dense = np.full([B, max([len(r) for r in rows], default=0)], -1, dtype=np.int64)
        for b, row in enumerate(rows):
            if any(j < 0 for j in row):
                raise ValueError(f"solve_influence: path of truss {b} names a joint out of range")
            dense[b, :len(row)] = row
    else:
        raw = _host_array(path, None)
        if raw.ndim != 2 or raw.shape[0] != B or raw.dtype.kind not in "iu":
            raise ValueError(f"solve_influence: path must be a list of joint-id lists or an integer array [B={B}, P_max]")
        dense = raw.astype(np.int64)
    P_max = int(dense.shape[1])
    path_len = (dense >= 0).sum(axis=1).astype(np.int32)
    nJ = np.asarray(packed.nJ, dtype=np.int64)
    for b in range(B):
        row = dense[b, :path_len[b]]
        if (dense[b, path_len[b]:] != -1).any() or (row < 0).any() or (row >= nJ[b]).any():
            raise ValueError(f"solve_influence: path of truss {b} names a joint out of range (joints 0 .. {int(nJ[b]) - 1}, "
                             "-1 padding at the end only)")
        pos = np.asarray(packed.xyz, dtype=np.float64)[b, row]
        if len(row) > 1 and (pos[1:] == pos[:-1]).all(axis=1).any():
            raise ValueError(f"solve_influence: two consecutive path joints of truss {b} lie at the same position")
    # the load vector
    d = _host_array(direction, np.float64)
    if d.shape not in ((2,), (3,), (B, 2), (B, 3)):
        raise ValueError(f"solve_influence: direction must be [3], [2], [B={B}, 3] or [B, 2], got {d.shape}")
    if not np.isfinite(d).all():
        raise ValueError("solve_influence: direction has a non-finite entry")
    d = np.broadcast_to(d, (B, d.shape[-1]))
    d = np.ascontiguousarray(np.concatenate([d, np.zeros([B, 3 - d.shape[-1]])], axis=1))
    # the train
    pairs = [(1.0, 0.0)] if train is None else [tuple(ax) for ax in train]
    if not pairs:
        raise ValueError("solve_influence: the train has no axle")
    if any(len(ax) != 2 for ax in pairs):
        raise ValueError("solve_influence: train must be a list of (weight, offset) pairs")
    w = np.array([float(ax[0]) for ax in pairs])
    o = np.array([float(ax[1]) for ax in pairs])
    if not (np.isfinite(w).all() and np.isfinite(o).all()):
        raise ValueError("solve_influence: train has a non-finite entry")
    if o[0] != 0.0 or (np.diff(o) < 0.0).any():
        raise ValueError("solve_influence: the axle offsets must ascend from 0 (the lead axle first)")
    if want_lines and B * nM_max * P_max * 8 > max_result_bytes:
        raise ValueError(f"solve_influence: lines [B={B}, {nM_max}, {P_max}] takes {B * nM_max * P_max * 8} bytes, more "
                         f"than max_result_bytes = {max_result_bytes}")
    if not _capi.load().trs_influence_fits(nJ_max, P_max, len(w)):
        raise ValueError(f"solve_influence: a path of {P_max} joints with {len(w)} axles on trusses of up to {nJ_max} "
                         "joints exceeds the LDS of the apply kernel (trs_influence_fits)")
    return np.ascontiguousarray(dense, dtype=np.int32), path_len, d, w, o


def solve_influence(trusses_or_packed, path, direction, train=None, want_lines=False, device=None, reorder=False,
                    options=None, max_slab_bytes=64 << 30, on_device=False, sections=None, use_envelope=True, chunk=64,
                    max_result_bytes=4 << 30):
    """Moving loads: the worst force a load train can put into every member of every truss of a batch as it crosses a
    path of joints - a vehicle on a bridge deck, a crane on a runway girder - from ONE factorisation per truss.  For
    member m the column z_m = inv(K_ff) b_m,f (the one the member-loss analysis forms) gives N_m = k_m z_m . f for ANY
    load f, so k_m z_m read along the path IS the influence line of N_m; the train is swept over it exactly - the
    extremes of a piecewise linear response lie where some axle stands on a path joint (`DeviceBatch.influence`,
    include/trs_influence.h).  `path`: a list of joint-id lists, one per truss, or [B, P_max] with -1 padding
    (caller's numbering; consecutive joints at distinct positions, a joint may recur); `direction`: the load vector per
    unit axle weight, [3], [2], [B, 3] or [B, 2]; `train`: a list of (weight, offset) pairs, the offsets behind the lead
    axle ascending from 0 (None: one unit axle - the envelope is then the extreme ordinate).  An axle between two path
    joints is shared between them by the lever rule; an axle off the path loads nothing.  `want_lines`: also the
    ordinates at the path joints, [B, nM_max, P_max] - refused above `max_result_bytes`.  Buckets, member forms,
    `reorder` plans, `options`, `on_device`, `use_envelope` and `chunk` as `solve_member_loss`.  `sections=` variants, a
    path joint out of range, two consecutive path joints at one position, a non-finite value, offsets that do not ascend
    from 0, an empty train and a shape `trs_influence_fits` refuses raise ValueError before any device work.  Returns an
    `InfluenceResult`."""
    packed = _as_packed(trusses_or_packed)
    path, path_len, d, w, o = _check_influence_args(packed, path, direction, train, sections, want_lines,
                                                    max_result_bytes, chunk)
    torch, dev = _require_gpu(device)
    up = lambda a: torch.from_numpy(a).to(dev)
    path, path_len, d, w, o = up(path), up(path_len), up(d), up(w), up(o)
    out = _new_result(torch, dev, InfluenceResult, packed.B, {"nM": packed.nM_max, "P": int(path.shape[1])},
                      without=() if want_lines else ("lines",))
    for db, part in _factored_buckets(packed, dev, out.info, max_slab_bytes, reorder, options, use_envelope, cases=1):
        _put_result(part, out, db.influence(part.cut(path), part.cut(path_len), part.cut(d), w, o,
                                            want_lines=want_lines, chunk=chunk))
    return _finish_result(torch, dev, out, on_device)


def _is_pinned(packed):
    """Every solver input of a `PackedBatch` is a contiguous array in page-locked memory."""
    import torch
    try:
        return all(getattr(packed, f).flags["C_CONTIGUOUS"] and torch.from_numpy(getattr(packed, f)).is_pinned()
                   for f in (RaggedSolver.GATHER_TABLE if packed.is_table else RaggedSolver.GATHER))
    except (RuntimeError, TypeError, ValueError):
        return False


#: `solve_batch(..., pool=...)` hands batches of at least this many trusses to `solve_batch_streamed`
STREAMED_FROM = 16384


def solve_batch(trusses_or_packed, device=None, max_slab_bytes=64 << 30, reorder=False, sections=None,
                on_device=False, pool=None, options=None, device_inputs=None):
    """Solve many trusses in device pipelines.  Accepts `list[Truss]` or a `PackedBatch`.

    The packed inputs go up once; a ragged batch is bucketed by padded system size
    (`size_buckets`) and every bucket is gathered, solved and scattered back ON THE DEVICE
    (`index_select` / `index_copy_`), inputs trimmed to the bucket's own maxima; the dense results come
    down once.  `reorder=True` renumbers the joints of every truss first, by the cheapest of reverse
    Cuthill-McKee and coordinate sweeps (`order_plan`: True / "profile", "fast", "rcm", ...): found, applied
    and undone (`trs_recover`'s `joint_out`) ON THE DEVICE by `trs_joint_order` whenever the batch shape fits
    that kernel, otherwise found on the host (natively, while the inputs go up).  Worth it when the trusses
    are not numbered along their long axis, e.g. generated cube trusses.

    `sections=[None, (a, e, density), ...]` solves the same trusses several times - `None` with their
    own member sections, a triple with every member set to it (the "fixed member type" prior of the
    reference's dataset path, `data.py:107-114`) - and returns a list of results: the geometry is
    uploaded, reordered and bucketed once, only A and E change between the solves.

    `on_device=True` leaves the results on the GPU (`DeviceResult`, torch tensors in the caller's joint
    order, plus the resident inputs) for device-side consumers such as the graph-feature kernel.  With
    `device_inputs` such a call runs in the `shared_workspace` of (device, current stream): its kernels - and
    the tensors it returns - are ordered by THAT stream only; a consumer on another stream must wait for it
    (`stream.wait_stream`), and callers that drive one stream from several threads must serialise their calls.

    Host side of a large batch: the joint order is found on a worker thread while the inputs go up; a
    `PackedBatch.pinned()` uploads by DMA; `pool=ResultPool()` downloads into reused page-locked buffers
    (the returned arrays are then views of the pool, valid until its next use).  `options`: per-call switches
    of the pipeline (`DEFAULT_OPTIONS`), for A/B runs and tests.  `device_inputs`: the batch's arrays already
    live on the device (dict by field name, e.g. `generate.generate_cube_batch_device`) - nothing is uploaded and
    the first argument only carries the sizes (`BatchSizes` or a `PackedBatch`).

    A `PackedBatch` in the TABLE member form (`PackedBatch.table()`, `pack_json(..., members="auto")`: uint16 end joints,
    a uint8 type index per member, one type table) goes up as it is - 5 instead of 24 bytes per member - and is solved
    by the resident bucket pipeline (`RaggedSolver`) through the `_tab` entry points: the same bits as the general form."""
    packed = trusses_or_packed if isinstance(trusses_or_packed, (PackedBatch, BatchSizes)) \
        else pack_trusses(list(trusses_or_packed))
    torch, dev = _require_gpu(device if device_inputs is None else device_inputs["xyz"].device)
    B, nJ_max, nM_max = packed.B, packed.nJ_max, packed.nM_max
    variants = [None] if sections is None else list(sections)
    if isinstance(packed, PackedBatch) and packed.is_table:
        if on_device or device_inputs is not None:
            packed = packed.general()   # (device-side consumers - graph features, fitness - read the general form)
        elif not (pool is not None and B >= STREAMED_FROM and sections is None and options is None and _is_pinned(packed)
                  and not _capi.load().trs_solve_small_fits(nJ_max, nM_max, packed.n_max)):
            # the table member form goes through the resident bucket pipeline as it is: 5 bytes per member up,
            # every kernel reads the table (same bits as the general form)
            if B == 0:
                empty = BatchResult(np.zeros([0, nJ_max, 3]), np.zeros([0, nJ_max, 3]), np.zeros([0, nM_max]),
                                    np.zeros([0], dtype=np.int32))
                return empty if sections is None else [empty for _ in variants]
            solver = RaggedSolver(packed, dev, reorder=reorder if reorder is not False else None,
                                  max_slab_bytes=None if max_slab_bytes >= 64 << 30 else max_slab_bytes,
                                  options=options, n_variants=len(variants))
            solver.step(sections=variants)
            torch.cuda.synchronize(dev)
            results = [BatchResult(o["u"].cpu().numpy(), o["f_ext"].cpu().numpy(), o["N"].cpu().numpy(),
                                   o["info"].cpu().numpy()) for o in solver.outs]
            return results[0] if sections is None else results
    if (pool is not None and B >= STREAMED_FROM and sections is None and not on_device and device_inputs is None
            and isinstance(packed, PackedBatch) and options is None and _is_pinned(packed)
            and not _capi.load().trs_solve_small_fits(nJ_max, nM_max, packed.n_max)):
        return solve_batch_streamed(packed, dev, reorder=reorder, pool=pool, max_slab_bytes=min(max_slab_bytes, 48 << 30))
    if B and device_inputs is None and _capi.load().trs_solve_small_fits(nJ_max, nM_max, packed.n_max):
        # every truss is small: the fused kernel, no bucketing, no reordering (nothing to gain from it)
        out = _solve_small_host(packed, torch, dev, variants, on_device)
        return out[0] if sections is None else out
    if device_inputs is not None and on_device and B and options is None:
        groups = size_buckets(packed, min(max_slab_bytes, 48 << 30))
        if len(groups) > 1:
            # a ragged batch that is on the device already and stays there: the resident bucket pipeline
            # (one-launch gathers and scatters, joint order per bucket, one workspace shared by all buckets and by
            # all calls on this device), one result set per section variant
            solver = RaggedSolver(packed, dev, reorder=reorder, tensors=device_inputs,
                                  max_slab_bytes=None if max_slab_bytes >= 64 << 30 else max_slab_bytes,
                                  workspace=shared_workspace(torch, dev), n_variants=len(variants))
            solver.step(sections=variants)
            inputs = {f: device_inputs[f] for f in DeviceBatch.INPUT_FIELDS if f in device_inputs}
            results = [DeviceResult(o["u"], o["f_ext"], o["N"], o["info"], inputs) for o in solver.outs]
            return results[0] if sections is None else results
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, non_blocking=True)
    plan = order_plan(reorder, nJ_max, nM_max) if B else None
    ordering = None
    if plan is not None and plan[0] == "host" and B >= 1024 and isinstance(packed, PackedBatch) and device_inputs is None:
        # native code (the GIL is released): the order is found while the inputs go up
        from concurrent.futures import ThreadPoolExecutor
        worker = ThreadPoolExecutor(max_workers=1)
        ordering = worker.submit(joint_order, packed, plan[1])
    # the densities play no part in the solve (weights and graph features only): they go up for on-device
    # consumers; otherwise the field is not transferred at all (a fifth of the upload of a cube-truss batch)
    needs_rho = on_device
    if device_inputs is not None:
        full = {f: device_inputs[f].contiguous() for f in DeviceBatch.INPUT_FIELDS if f in device_inputs}
        if plan is not None and plan[0] == "host" and not isinstance(packed, PackedBatch):
            packed_host = packed.to_packed(device_inputs)   # a host-side order needs the arrays on the host
            ordering = None
            plan = ("given", joint_order(packed_host, plan[1]))
    else:
        full = {f: up(getattr(packed, f)) for f in DeviceBatch.INPUT_FIELDS if f != "rho" or needs_rho}
    original = dict(full)   # the caller's joint order (the reordering below makes new tensors)
    perm32 = None
    if plan is not None and plan[0] == "device":
        # found and applied on the GPU, behind the upload on the same stream: no host pass over the batch
        ordered = joint_order_device(torch, full, effort=plan[1])
        perm32 = ordered["perm"]                                             # [B, nJ_max] int32, joint k := old perm[k]
        full.update({k: ordered[k] for k in ("xyz", "conn", "cbits", "loads")})
    elif plan is not None:
        if ordering is not None:
            host_perm = ordering.result()
            worker.shutdown(wait=False)
        else:
            host_perm = joint_order(packed, plan[1])
        perm32 = up(host_perm)
        perm = perm32.long()
        inverse = torch.empty_like(perm)
        inverse.scatter_(1, perm, torch.arange(nJ_max, device=dev).expand(B, -1))
        by_joint = perm[:, :, None].expand(-1, -1, 3)
        full["xyz"] = full["xyz"].gather(1, by_joint)
        full["loads"] = full["loads"].gather(1, by_joint)
        full["cbits"] = full["cbits"].gather(1, perm)
        conn = inverse.gather(1, full["conn"].long().reshape(B, -1)).reshape(B, nM_max, 2)
        live = torch.arange(nM_max, device=dev)[None, :, None] < full["nM"].long()[:, None, None]
        full["conn"] = (conn * live).to(torch.int32)
    groups = size_buckets(packed, max_slab_bytes)
    # largest slab first: the caching allocator then serves every later bucket from the first
    # bucket's block instead of growing the pool bucket by bucket
    n_pad_of = lambda idx: (int(packed.n_free[idx].max()) + 63) // 64 * 64
    groups.sort(key=lambda idx: -len(idx) * n_pad_of(idx) * (n_pad_of(idx) + 16))
    whole = len(groups) == 1 and len(groups[0]) == B
    outs = []
    for _ in variants:
        z = torch.zeros if not whole else torch.empty
        outs.append({"u": z([B, nJ_max, 3], dtype=torch.float64, device=dev),
                     "f_ext": z([B, nJ_max, 3], dtype=torch.float64, device=dev),
                     "N": z([B, nM_max], dtype=torch.float64, device=dev),
                     "info": z([B], dtype=torch.int32, device=dev)})
    joint_fields = ("xyz", "cbits", "loads")
    lib = _capi.load()
    for idx in groups:
        n_b = int(packed.n_free[idx].max()) if not whole else packed.n_max
        if whole:
            rows, nJ_b, nM_b = None, nJ_max, nM_max
        else:
            rows = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).to(dev)
            nJ_b = max(1, int(packed.nJ[idx].max()))
            nM_b = max(1, int(packed.nM[idx].max()))
        # a bucket of small trusses runs on the fused kernel, which takes no joint order (and gains
        # nothing from one): it reads the caller's numbering
        renumbered = perm32 is not None and not lib.trs_solve_small_fits(nJ_b, nM_b, n_b)
        source = full if renumbered else original
        if whole:
            sub = dict(source)
        else:
            sub = {}
            for f in DeviceBatch.INPUT_FIELDS:
                if f not in source:
                    continue
                t = source[f].index_select(0, rows)
                if f in ("nJ", "nM"):
                    sub[f] = t
                else:  # trimmed to the bucket's own maxima
                    sub[f] = t[:, :(nJ_b if f in joint_fields else nM_b)].contiguous()
        if "rho" not in sub:
            sub["rho"] = sub["A"]   # placeholder of the right shape: no kernel of the solve reads it
        own = (sub["A"], sub["E"]) if len(variants) > 1 else None
        if own is not None:   # the bucket's own sections survive the fixed-section solves
            sub["A"], sub["E"] = own[0].clone(), own[1].clone()
        # the bucket's kernels see the renumbered joints; trs_recover writes the results of joint k to the
        # caller's row perm[k] (a real joint's target is a real joint, so the trimmed width holds it)
        jout = None
        if renumbered:
            jout = perm32 if whole else perm32.index_select(0, rows)[:, :nJ_b].contiguous()
        # (no launch hints here: finding the envelopes' reach on the host costs a one-shot call more than
        # the handful of empty launches it would save; a resident DeviceBatch does it once and keeps it)
        bucket = DeviceBatch.from_device(sub, n_b, joint_out=jout)
        bucket.options.update(options or {})
        for slot, sec in enumerate(variants):
            if sec is not None:
                bucket.A.fill_(float(sec[0]))
                bucket.E.fill_(float(sec[1]))
            elif own is not None:
                bucket.A.copy_(own[0])
                bucket.E.copy_(own[1])
            bucket.solve()
            o = outs[slot]
            if whole:
                o["u"].copy_(bucket.u); o["f_ext"].copy_(bucket.f_ext); o["N"].copy_(bucket.N)
                o["info"].copy_(bucket.info)
            else:
                o["u"][:, :nJ_b].index_copy_(0, rows, bucket.u)
                o["f_ext"][:, :nJ_b].index_copy_(0, rows, bucket.f_ext)
                o["N"][:, :nM_b].index_copy_(0, rows, bucket.N)
                o["info"].index_copy_(0, rows, bucket.info)
        del bucket
    results = []
    if on_device:
        results = [DeviceResult(o["u"], o["f_ext"], o["N"], o["info"], original) for o in outs]
        return results[0] if sections is None else results
    if pool is not None:   # one DMA per array into the pool's page-locked buffers
        host = []
        for slot, o in enumerate(outs):
            h = {k: pool.take(torch, (slot, k), v.shape, v.dtype) for k, v in o.items()}
            for k, v in o.items():
                h[k].copy_(v, non_blocking=True)
            host.append(h)
        torch.cuda.synchronize(dev)
        for h in host:
            results.append(BatchResult(h["u"].numpy(), h["f_ext"].numpy(), h["N"].numpy(), h["info"].numpy()))
        return results[0] if sections is None else results
    torch.cuda.synchronize(dev)
    for o in outs:
        results.append(BatchResult(o["u"].cpu().numpy(), o["f_ext"].cpu().numpy(), o["N"].cpu().numpy(),
                                   o["info"].cpu().numpy()))
    return results[0] if sections is None else results
