"""The sort of the sweep keys inside `trs_joint_order_kernel` (csrc/order.hip, csrc/trs_wavesort.h) - `-m gpu`.

A coordinate sweep sorts the free joints by (bin, bin, bin, position in the id list).  32-bit keys of up to 256 free
joints are sorted in a wave's registers by a bitonic network with R = 1, 2, 4 keys per lane (64, 128, 256 keys after
padding); beyond 256 free joints, and for keys that need more than 32 bits, the rank sort over LDS does it.  Whatever
sorts, the device must return the permutation, the choice and the reach of the host's `trs_profile_order`
(csrc/reorder.c), bit for bit.  The trusses are synthetic: shuffled lattices with a chosen number of free joints and a few
fully constrained joints among the ids, at every size where the sort changes its shape.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MT = [1.0, 1e7, 0.1]
#: every R, every padding boundary of the network, and both sides of the hand-over to the rank sort (256 | 257);
#: 511 .. 513 would be the boundary of eight keys per lane, which the kernel does not use
SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513)
WAVESORT_MAX = 256   # csrc/order.hip TRS_ORDER_WAVESORT_MAX


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from python_stable_3d_truss_analysis_amd import batch
    return batch


def _with_supports(points, members, rng, n_pin=3):
    """`points` [nf, 3] become free joints; `n_pin` fully constrained joints are inserted at spread positions of the id
    list, each tied to one free joint.  Returns the JSON form."""
    nf, n = len(points), len(points) + n_pin
    pins = sorted(set(int(s) for s in np.linspace(0, n - 1, n_pin + 2)[1:-1]))        # ids the supports take
    assert len(pins) == n_pin
    new_id, joints = {}, []
    for j in range(n):
        k = len(new_id)                                                              # free joints placed so far
        if j in pins:
            joints.append([(np.asarray(points[min(k, nf - 1)], dtype=float) + [0.5, 0.25, -0.5]).tolist(), "PIN"])
        else:
            new_id[k] = j
            joints.append([np.asarray(points[k], dtype=float).tolist(), "NO"])
    assert len(new_id) == nf
    mem = [[[new_id[a], new_id[b]], MT] for a, b in members]
    mem += [[[p, new_id[int(rng.integers(nf))]], MT] for p in pins]
    return {"joint": joints, "force": [[new_id[0], [0.0, 0.0, -1.0]]], "member": mem}


#: sparsely filled long boxes on which a coordinate sweep beats both Cuthill-McKee orders at effort 2 although they
#: have fewer than 128 free joints (found with the host function; asserted below): nf -> (box, seed)
STRIPS = {63: ((1, 4, 40), 3), 64: ((1, 4, 40), 3), 65: ((1, 4, 40), 3), 127: ((2, 3, 30), 1)}


def _lattice(nf, rng, box=None):
    """nf points of a small 3D lattice in shuffled id order, unit members between lattice neighbours that are present."""
    side = max(2, int(np.ceil(nf ** (1.0 / 3.0))))
    sx, sy, sz = box if box is not None else (side, side + 1, side + 2)
    cells = np.array([(x, y, z) for x in range(sx) for y in range(sy) for z in range(sz)])
    pts = cells[rng.permutation(len(cells))[:nf]]
    at = {tuple(p): i for i, p in enumerate(pts)}
    members = [(i, at[tuple(p + d)]) for i, p in enumerate(pts) for d in np.eye(3, dtype=int) if tuple(p + d) in at]
    if not members and nf > 1:
        members = [(0, 1)]
    return _with_supports(pts.astype(float), members, rng)


def _line(nf, rng):
    """A chain along x in shuffled id order: one bin on the y and z axes, the keys differ in one bin field and x."""
    order = rng.permutation(nf)
    pts = np.zeros([nf, 3])
    pts[:, 0] = order
    where = np.argsort(order)
    truss = _with_supports(pts, [(int(where[i]), int(where[i + 1])) for i in range(nf - 1)], rng)
    for j in truss["joint"]:                       # the supports on the line too
        j[0][1] = j[0][2] = 0.0
    return truss


def _cluster(nf, rng):
    """Free joints within 1e-3 of one point, long members to two far supports: every free joint falls into the same bin
    on every axis and the order of a sweep is decided by the position in the id list alone."""
    pts = 50.0 + 1e-3 * rng.random([nf, 3])
    joints = [[[0.0, 0.0, 0.0], "PIN"]] + [[p.tolist(), "NO"] for p in pts[:nf // 2]] + [[[100.0, 100.0, 100.0], "PIN"]] \
        + [[p.tolist(), "NO"] for p in pts[nf // 2:]]
    free = [j for j, (_, s) in enumerate(joints) if s == "NO"]
    mem = [[[free[i], free[(i * 7 + 3) % nf]], MT] for i in range(nf) if free[i] != free[(i * 7 + 3) % nf]]
    mem += [[[0 if i % 2 else nf // 2 + 1, f], MT] for i, f in enumerate(free)]
    return {"joint": joints, "force": [[free[0], [1.0, 0.0, 0.0]]], "member": mem}


def _far_joint(nf, rng):
    """A lattice plus one free joint 300 member lengths away along every axis: more than 1024 bins (quarter lengths)
    in use on all three axes, while the lattice's joints still spread over dozens of them - the three bin fields
    alone take 33 bits."""
    truss = _lattice(nf - 1, rng)
    truss["joint"].append([[300.0, 300.0, 300.0], "NO"])
    return truss


def _key_bits(packed, b):
    """Bits of a sweep key of truss b as the kernel counts them (bins per axis from the binning rule, plus the
    position field)."""
    bits_for = lambda count: max(1, int(np.ceil(np.log2(max(count, 1)))))
    nJ, nM = int(packed.nJ[b]), int(packed.nM[b])
    xyz, conn = packed.xyz[b, :nJ], packed.conn[b, :nM]
    d2 = ((xyz[conn[:, 1]] - xyz[conn[:, 0]]) ** 2).sum(axis=1)
    d2 = d2[d2 > 0]
    h = float(np.float32(0.25 * np.sqrt(d2.sum() / len(d2))))
    cap = 4 * packed.nJ_max + 64
    nf = int(((packed.cbits[b, :nJ] & 7) != 7).sum())
    total = bits_for(max(nf, 2))
    for a in range(3):
        lo, hi = xyz[:, a].min(), xyz[:, a].max()
        ha = h if (hi - lo) / h < cap - 2 else (hi - lo) / (cap - 2)
        q = np.minimum(np.floor((xyz[:, a] - lo) / ha + 0.5), cap - 1)
        total += bits_for(int(q.max()) + 1)
    return total


@pytest.fixture(scope="module")
def cases(gpu):
    return _build_cases(gpu)


def _build_cases(gpu):
    """ONE mixed batch (neighbouring work-groups differ in size and path) and the host's answers for it, per effort."""
    rng = np.random.default_rng(20)
    named = [(f"lattice nf={nf}", _lattice(nf, rng)) for nf in SIZES]
    named += [(f"strip nf={nf}", _lattice(nf, np.random.default_rng(seed), box)) for nf, (box, seed) in STRIPS.items()]
    named += [(f"line nf={nf}", _line(nf, rng)) for nf in (3, 64, 200, 256, 300)]
    named += [(f"cluster nf={nf}", _cluster(nf, rng)) for nf in (2, 65, 129, 256)]
    named += [(f"far joint nf={nf}", _far_joint(nf, rng)) for nf in (40, 129, 256, 300)]
    order = rng.permutation(len(named))
    named = [named[i] for i in order]
    packed = gpu.pack_json([d for _, d in named])
    names = [n for n, _ in named]
    assert gpu._capi.load().trs_joint_order_fits(packed.nJ_max, packed.nM_max) == 1
    free = [int(((packed.cbits[b, :packed.nJ[b]] & 7) != 7).sum()) for b in range(packed.B)]
    for name, nf in zip(names, free):
        assert int(name.split("=")[1]) == int(nf), name
    host = {}
    for effort in (2, 3):
        perm, choice = gpu.profile_permutation(packed, return_choice=True, effort=effort)
        host[effort] = (perm, choice, gpu.envelope_reach(packed, perm))
    return names, packed, host


def _device_order(gpu, packed, effort):
    import torch
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    tensors = {f: up(getattr(packed, f)) for f in ("xyz", "conn", "cbits", "loads", "nJ", "nM")}
    out = gpu.joint_order_device(torch, tensors, effort=effort, want_choice=True)
    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy() for k in ("perm", "choice", "reach")}


def test_the_batch_reaches_every_path_of_the_sort(cases):
    """No GPU work: the far-joint trusses, and only they, need more than 32 key bits; the others stand on both sides of
    the register sort's cap; the line and cluster trusses have the ties they are named for."""
    names, packed, host = cases
    bits = {n: _key_bits(packed, b) for b, n in enumerate(names)}
    assert all((bits[n] > 32) == n.startswith("far joint") for n in names), bits
    narrow = [int(n.split("=")[1]) for n in names if not n.startswith("far joint")]
    assert {WAVESORT_MAX, WAVESORT_MAX + 1} <= set(narrow)
    for b, n in enumerate(names):
        nJ = int(packed.nJ[b])
        freexyz = packed.xyz[b, :nJ][(packed.cbits[b, :nJ] & 7) != 7]
        if n.startswith("line"):
            assert np.ptp(freexyz[:, 1]) == 0 and np.ptp(freexyz[:, 2]) == 0
        if n.startswith("cluster"):
            assert np.ptp(freexyz, axis=0).max() <= 1e-3
    # the sort's result is what is compared only where a sweep (choice >= 2) wins: at effort 3 on every truss from 128
    # free joints up, at effort 2 on the strips, which cover R = 1 and R = 2 with and without padding
    for b, n in enumerate(names):
        if int(n.split("=")[1]) >= 128:
            assert host[3][1][b] >= 2, n
        if n.startswith("strip"):
            assert host[2][1][b] >= 2, n


@pytest.mark.parametrize("effort", [3, 2])
def test_device_sort_gives_the_hosts_order(gpu, cases, effort):
    names, packed, host = cases
    got = _device_order(gpu, packed, effort)
    perm, choice, reach = host[effort]
    for b, name in enumerate(names):       # truss by truss first, so that a failure names the size and the path
        assert np.array_equal(got["perm"][b], perm[b]), (name, effort)
        assert got["choice"][b] == choice[b] and got["reach"][b] == reach[b], (name, effort)
    assert np.array_equal(got["perm"], perm)
    assert np.array_equal(got["choice"], choice)
    assert np.array_equal(got["reach"], reach)


def test_device_sort_repeats_itself(gpu, cases):
    names, packed, host = cases
    first, second = _device_order(gpu, packed, 3), _device_order(gpu, packed, 3)
    for k in ("perm", "choice", "reach"):
        assert np.array_equal(first[k], second[k]), k
