"""The joint-parallel walk of `trs_joint_order` (csrc/order.hip, phase B1-B3) - `-m gpu`.

A truss whose six coordinate sweeps are priced alone (effort 3 from 128 free joints on) and whose keys a wave sorts in
registers (up to 256 free joints) is priced by the whole work-group in one walk over the neighbour lists; every other
truss keeps the per-wave pricing.  Both forms must give what the host gives (`trs_profile_order`,
`trs_apply_joint_order`, `trs_envelope_reach` of csrc/reorder.c): the same permutation, choice and reach, and the
renumbered inputs bit for bit.  The shapes are the smallest at which the forms differ or can go wrong: free-joint
counts around the keys per lane (64, 128, 256), the Cuthill-McKee rule (128) and the register sort's limit (256), list
lengths around the four neighbours a step of the walk reads, joints whose rows straddle a 16-row chunk, ties between
sweeps, ragged batches in all three calling forms, every effort, and two streams at once.
"""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FREE_COUNTS = (1, 2, 63, 64, 65, 128, 129, 255, 256, 257)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from python_stable_3d_truss_analysis_amd import batch
    return batch


# ---- trusses ---------------------------------------------------------------------------------------------------
def _finish(rng, xyz, conn, cbits):
    xyz, cbits = np.asarray(xyz, dtype=np.float64), np.asarray(cbits, dtype=np.uint8)
    loads = np.where((cbits != 7)[:, None], np.round(rng.uniform(-5, 5, size=xyz.shape), 2), 0.0)
    return {"xyz": xyz, "conn": np.asarray(conn, dtype=np.int32).reshape(-1, 2), "cbits": cbits, "loads": loads}


def _lattice(rng, n_free, n_fixed=4, partial=(0, 0), shuffle=True, shape=None, fixed=None, origin=(0.0, 0.0, 0.0)):
    """n_free + n_fixed joints on the first points of a unit lattice (x fastest), ids shuffled, members along the
    axes and two face diagonals (degrees up to ten); `partial` = (joints with one free DOF, joints with two) among the
    free ones; `shape` = an exact nx x ny x nz block instead; `fixed` = the fully constrained lattice points."""
    total = n_free + n_fixed
    if shape is None:
        side = max(2, int(np.ceil(total ** (1.0 / 3.0))))
        shape = (side, side, -(-total // (side * side)))
    pts = [(x, y, z) for z, y, x in itertools.product(range(shape[2]), range(shape[1]), range(shape[0]))][:total]
    ident = rng.permutation(total) if shuffle else np.arange(total)
    at = {p: int(ident[k]) for k, p in enumerate(pts)}
    xyz = np.zeros([total, 3])
    for p, j in at.items():
        xyz[j] = np.asarray(p, dtype=float) + np.asarray(origin)
    conn = []
    for p in pts:
        for d in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, -1, 0)):
            q = (p[0] + d[0], p[1] + d[1], p[2] + d[2])
            if q in at:
                conn.append((at[p], at[q]) if rng.integers(2) else (at[q], at[p]))
    cbits = np.zeros([total], dtype=np.uint8)
    held = rng.choice(total, size=n_fixed, replace=False) if fixed is None else [at[p] for p in fixed]
    cbits[held] = 7
    free = np.flatnonzero(cbits == 0)
    some = rng.choice(free, size=min(len(free), partial[0] + partial[1]), replace=False)
    cbits[some[:partial[0]]] = rng.choice([3, 5, 6], size=len(some[:partial[0]]))      # one free DOF
    cbits[some[partial[0]:]] = rng.choice([1, 2, 4], size=len(some[partial[0]:]))      # two
    return _finish(rng, xyz, conn, cbits)


def _hubs(rng, ring=150, degrees=(0, 3, 4, 5, 8, 9), parallel=False):
    """A ring of free joints (two neighbours each) and one hub per entry of `degrees` with exactly that many list
    entries: spokes to distinct ring joints, or - `parallel` - some of them doubled (parallel members between the same
    two joints, in both directions).  Two pinned joints with members to the hubs, which couple nothing."""
    n = ring + len(degrees) + 2
    xyz = np.round(rng.uniform(0, 10, size=[n, 3]), 1)
    conn = [(i, (i + 1) % ring) for i in range(ring)]
    for h, d in enumerate(degrees):
        hub = ring + h
        ends = rng.choice(ring, size=d, replace=False)
        if parallel and d >= 3:
            ends[1] = ends[0]
            ends[d - 1] = ends[d - 2]
        conn += [(hub, int(e)) if k % 2 else (int(e), hub) for k, e in enumerate(ends)]
        conn.append((hub, n - 1 - h % 2))
    cbits = np.zeros([n], dtype=np.uint8)
    cbits[n - 2:] = 7
    order = rng.permutation(len(conn))
    return _finish(rng, xyz, [conn[k] for k in order], cbits)


def _pack(gpu, trusses, pad_joints=0, pad_members=0):
    """A `PackedBatch` of trusses of `_finish`, every section 1 (one member type), padded beyond the largest truss."""
    B = len(trusses)
    nJ = np.array([len(t["xyz"]) for t in trusses], dtype=np.int32)
    nM = np.array([len(t["conn"]) for t in trusses], dtype=np.int32)
    jm, mm = max(1, int(nJ.max())) + pad_joints, max(1, int(nM.max())) + pad_members
    xyz, loads = np.zeros([B, jm, 3]), np.zeros([B, jm, 3])
    cbits, conn = np.zeros([B, jm], dtype=np.uint8), np.zeros([B, mm, 2], dtype=np.int32)
    for b, t in enumerate(trusses):
        xyz[b, :nJ[b]], loads[b, :nJ[b]], cbits[b, :nJ[b]], conn[b, :nM[b]] = t["xyz"], t["loads"], t["cbits"], t["conn"]
    ones = np.ones([B, mm])
    return gpu.PackedBatch(xyz, conn, ones.copy(), ones.copy(), ones.copy(), cbits, loads, nJ, nM,
                           np.full([B], 3, dtype=np.int32), gpu.count_free(cbits, nJ))


def _free_joints(packed):
    return ((packed.cbits != 7) & (np.arange(packed.nJ_max)[None, :] < packed.nJ[:, None])).sum(axis=1)


# ---- device against host -----------------------------------------------------------------------------------------
def _upload(torch, packed, fields=("xyz", "conn", "cbits", "loads", "nJ", "nM")):
    return {f: torch.from_numpy(np.ascontiguousarray(getattr(packed, f))).cuda() for f in fields}


def _device(gpu, packed, effort):
    import torch
    out = gpu.joint_order_device(torch, _upload(torch, packed), effort=effort, want_choice=True)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


_HOST = {}


def _host(gpu, key, packed, effort):
    """The host's answer for a batch (general form), computed once per (batch, effort) and shared."""
    if (key, effort) not in _HOST:
        perm, choice = gpu.profile_permutation(packed, return_choice=True, effort=effort)
        want = gpu.permute_joints(packed, perm)
        for a in (perm, choice):
            a.setflags(write=False)
        _HOST[key, effort] = (perm, choice, gpu.envelope_reach(packed, perm), want)
    return _HOST[key, effort]


def _assert_equals_host(gpu, key, packed, effort, got, tag=""):
    perm, choice, reach, want = _host(gpu, key, packed, effort)
    tag = f"{key} effort {effort} {tag}"
    for b in range(packed.B):
        assert sorted(got["perm"][b, :packed.nJ[b]].tolist()) == list(range(packed.nJ[b])), (tag, b)   # a permutation
    if "choice" in got:
        np.testing.assert_array_equal(got["choice"], choice, err_msg=tag)
    np.testing.assert_array_equal(got["perm"], perm, err_msg=tag)
    np.testing.assert_array_equal(got["reach"], reach, err_msg=tag)
    for field in ("xyz", "cbits", "loads"):
        np.testing.assert_array_equal(got[field].view(np.uint8), getattr(want, field).view(np.uint8), err_msg=f"{tag} {field}")
    np.testing.assert_array_equal(got["conn"].astype(np.int32), want.conn, err_msg=f"{tag} conn")


def _count_batch(gpu):
    rng = np.random.default_rng(101)
    return _pack(gpu, [_lattice(rng, n, partial=(n // 9, n // 7)) for n in FREE_COUNTS])


@pytest.mark.parametrize("effort", [3, 2])
def test_free_joint_counts_around_every_boundary(gpu, effort):
    """1 .. 257 free joints: one, two and four keys per lane, the Cuthill-McKee rule at 128 (effort 3: the walk from
    128 on, the per-wave form below; effort 2: the per-wave form throughout), the rank sort beyond 256."""
    packed = _count_batch(gpu)
    np.testing.assert_array_equal(_free_joints(packed), FREE_COUNTS)
    _assert_equals_host(gpu, "counts", packed, effort, _device(gpu, packed, effort))


@pytest.mark.parametrize("parallel", [False, True], ids=["distinct spokes", "parallel members"])
def test_list_lengths_around_the_four_look_ups_of_a_step(gpu, parallel):
    """Joints with 0, 3, 4, 5, 8 and 9 list entries among 150 ring joints (the walk reads four neighbours per step and
    takes the joint itself for the slack behind a list), with and without parallel members."""
    rng = np.random.default_rng(7 + parallel)
    packed = _pack(gpu, [_hubs(rng, parallel=parallel) for _ in range(6)])
    assert (_free_joints(packed) == 156).all()
    for effort in (3, 2):
        _assert_equals_host(gpu, f"hubs {parallel}", packed, effort, _device(gpu, packed, effort))


def test_partly_constrained_joints_straddle_row_chunks(gpu):
    """Joints with one and two free DOFs among free ones (a joint's rows then straddle 16-row chunks, forwards and
    backwards: checked on the winner), a truss with every joint constrained, one with two disconnected components."""
    rng = np.random.default_rng(33)
    mixed = [_lattice(rng, n, partial=(n // 4, n // 3)) for n in (130, 200, 256)]
    held = _lattice(rng, 0, n_fixed=20)
    a, b = _lattice(rng, 70, n_fixed=2), _lattice(rng, 75, n_fixed=2, origin=(100.0, 0.0, 0.0))
    two = {"xyz": np.concatenate([a["xyz"], b["xyz"]]), "conn": np.concatenate([a["conn"], b["conn"] + len(a["xyz"])]),
           "cbits": np.concatenate([a["cbits"], b["cbits"]]), "loads": np.concatenate([a["loads"], b["loads"]])}
    small_two = {k: v.copy() for k, v in two.items()}
    small_two["cbits"][40:72] = 7      # the same below 128 free joints: Cuthill-McKee beside the sweeps
    small_two["cbits"][100:] = 7
    small_two["loads"][small_two["cbits"] == 7] = 0.0
    packed = _pack(gpu, mixed + [held, two, small_two])
    got = _device(gpu, packed, 3)
    _assert_equals_host(gpu, "partial", packed, 3, got)
    assert got["choice"][3] == 0 and (got["choice"][:3] >= 2).all()
    for b_ in range(3):    # the case is there: some joint of the chosen order has rows in two chunks
        rows = 3 - np.unpackbits(packed.cbits[b_, got["perm"][b_, :packed.nJ[b_]], None], axis=1)[:, 5:].sum(axis=1)
        first = np.cumsum(rows) - rows
        assert ((first // 16 != (first + rows - 1) // 16) & (rows > 0)).any()


def test_ties_between_sweeps_on_an_exactly_cubic_lattice(gpu):
    """6 x 6 x 6 joints, the eight corners held, ids in lattice order and shuffled: the structure is the same along
    every axis, so sweeps cost the same and the evaluation rank decides, forwards before backwards - as on the host."""
    corners = list(itertools.product((0, 5), repeat=3))
    rng = np.random.default_rng(9)
    cubes = [_lattice(rng, 208, n_fixed=8, shuffle=s, shape=(6, 6, 6), fixed=corners) for s in (False, True, True)]
    stretched = _lattice(rng, 208, n_fixed=8, shuffle=True, shape=(6, 6, 6), fixed=corners)
    stretched["xyz"][:, 1] *= 1.5      # a longest extent: another sweep is evaluated first
    packed = _pack(gpu, cubes + [stretched])
    for effort in (3, 2):
        _assert_equals_host(gpu, "cubic", packed, effort, _device(gpu, packed, effort))
    assert (_host(gpu, "cubic", packed, 3)[1] >= 2).all()


def _ragged(gpu):
    rng = np.random.default_rng(55)
    trusses = [_lattice(rng, n, partial=(n // 8, n // 8)) for n in (129, 2, 256, 64, 1, 200, 257, 128, 63, 255, 65)]
    trusses += [_lattice(rng, 0, n_fixed=9), _hubs(rng, parallel=True)]
    return _pack(gpu, trusses, pad_joints=5, pad_members=3)


@pytest.mark.parametrize("form", ["general", "table"])
def test_ragged_batch_in_one_launch(gpu, form):
    """Every size class in one launch, rows padded beyond the largest truss, end joints as int32 and as uint16."""
    packed = _ragged(gpu)
    shaped = packed.table() if form == "table" else packed
    for effort in (3, 2):
        _assert_equals_host(gpu, "ragged", packed, effort, _device(gpu, shaped, effort), form)


@pytest.mark.parametrize("form", ["general", "table"])
def test_ragged_batch_in_the_gather_form(gpu, form):
    """`trs_joint_order_rows(_tab)`: rows of the ragged batch in another order into rows of their own width, the
    member sections and the counts copied along."""
    import torch
    lib = gpu._capi.load()
    packed = _ragged(gpu)
    pick = np.array([12, 0, 7, 2, 11, 9, 4, 5], dtype=np.int64)
    sub = packed.take(pick).trimmed()
    shaped = packed.table() if form == "table" else packed
    sections = ("type_idx",) if form == "table" else ("E", "A")
    inp = _upload(torch, shaped, ("xyz", "conn", "cbits", "loads", "nJ", "nM") + sections)
    rows = torch.from_numpy(pick).cuda()
    count, nJ_max, nM_max = len(pick), sub.nJ_max, sub.nM_max
    new = lambda shape, like: torch.full(shape, 77, dtype=like.dtype, device="cuda")
    out = {"perm": new([count, nJ_max], inp["nJ"]), "reach": new([count], inp["nJ"]),
           "xyz": new([count, nJ_max, 3], inp["xyz"]), "conn": new([count, nM_max, 2], inp["conn"]),
           "cbits": new([count, nJ_max], inp["cbits"]), "loads": new([count, nJ_max, 3], inp["loads"]),
           "nJ": new([count], inp["nJ"]), "nM": new([count], inp["nM"])}
    for s in sections:
        out[s] = new([count, nM_max], inp[s])
    fn = lib.trs_joint_order_rows_tab if form == "table" else lib.trs_joint_order_rows
    gpu._capi.check(fn(
        count, nJ_max, nM_max, rows.data_ptr(), packed.nJ_max, packed.nM_max,
        inp["xyz"].data_ptr(), inp["conn"].data_ptr(), inp["cbits"].data_ptr(), inp["loads"].data_ptr(),
        *(inp[s].data_ptr() for s in sections), inp["nJ"].data_ptr(), inp["nM"].data_ptr(), out["perm"].data_ptr(),
        out["reach"].data_ptr(), out["xyz"].data_ptr(), out["conn"].data_ptr(), out["cbits"].data_ptr(),
        out["loads"].data_ptr(), *(out[s].data_ptr() for s in sections), out["nJ"].data_ptr(), out["nM"].data_ptr(),
        3, torch.cuda.current_stream().cuda_stream), "trs_joint_order_rows")
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    _assert_equals_host(gpu, "ragged rows", sub, 3, got, form)
    np.testing.assert_array_equal(got["nJ"], sub.nJ)
    np.testing.assert_array_equal(got["nM"], sub.nM)
    live = np.arange(nM_max)[None, :] < sub.nM[:, None]
    for s in sections:
        want = getattr(shaped.take(pick).trimmed(), s)
        np.testing.assert_array_equal(got[s], np.where(live, want, 0), err_msg=s)


@pytest.mark.parametrize("effort", [0, 1, 2, 3])
def test_every_effort_on_one_mid_size_truss(gpu, effort):
    rng = np.random.default_rng(77)
    packed = _pack(gpu, [_lattice(rng, 200, n_fixed=6, partial=(10, 20))])
    _assert_equals_host(gpu, "efforts", packed, effort, _device(gpu, packed, effort))


@pytest.mark.timeout(120)
def test_two_streams_at_once_repeat_the_one_stream_bits(gpu):
    """The ragged batch, 160 copies of it, ordered on two streams at the same time (buffers of their own), ten times:
    every output of either stream equals, bit for bit, the launch that ran alone - work-groups of both launches share
    the CUs, which pulls the waves of a work-group apart (the shape of the race of EXPERIMENTS R5.1)."""
    import torch
    one = _ragged(gpu)
    packed = one.replicate(160)
    tensors = [_upload(torch, packed) for _ in range(2)]
    alone = gpu.joint_order_device(torch, tensors[0], effort=3, want_choice=True)
    torch.cuda.synchronize()
    alone = {k: v.clone() for k, v in alone.items()}
    host = {k: v.cpu().numpy() for k, v in alone.items()}
    _assert_equals_host(gpu, "ragged", one, 3, {k: a[:one.B] for k, a in host.items()})
    for k, a in host.items():      # ... and every copy is the first
        assert (a.reshape((160, one.B) + a.shape[1:]) == a[None, :one.B]).all(), k
    streams = [torch.cuda.Stream() for _ in range(2)]
    outs = [None, None]
    for rnd in range(10):
        for s in (0, 1):
            if outs[s] is not None:
                for v in outs[s].values():
                    v.fill_(-1 if v.dtype != torch.uint8 else 255)
        torch.cuda.synchronize()
        for s in ((0, 1) if rnd % 2 == 0 else (1, 0)):
            with torch.cuda.stream(streams[s]):
                outs[s] = gpu.joint_order_device(torch, tensors[s], effort=3, want_choice=True, out=outs[s])
        torch.cuda.synchronize()
        for s in (0, 1):
            for k, v in alone.items():
                assert torch.equal(outs[s][k].view(torch.uint8), v.view(torch.uint8)), (rnd, s, k)
