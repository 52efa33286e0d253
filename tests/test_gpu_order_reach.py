"""The envelope reach the joint-order kernel reports (`trs_joint_order*`, csrc/order.hip) - `-m gpu`.

The kernel takes the reach of the winning order from the wave that priced it (no second pricing of the winner), so
the value must equal what the host derives from the permutation (`batch.envelope_reach`, csrc/reorder.c
`trs_envelope_reach`) for every truss: bar-942, the bundled data cases, a sample of cube trusses, in the general and
in the table member form, in the plain and in the gather form (`trs_joint_order_rows`, `trs_joint_order_rows_tab`);
and the permutation must be the host's (`trs_profile_order`) at efforts 1, 2, 3 and under the name "profile".
"""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from python_stable_3d_truss_analysis_amd import batch
    return batch


@pytest.fixture(scope="module")
def batches(gpu):
    from python_stable_3d_truss_analysis_amd import generate as gen
    rng = np.random.default_rng(17)
    return {
        "bar-942 x 64": gpu.pack_json([H.load_json("bar-942_input_0")]).replicate(64),
        "data cases": gpu.pack_json([H.load_json(n) for n in H.data_case_names()]),
        "cube sample": gen.generate_cube_batch(rng.integers(1, 191, size=384), gridRange=(6, 6, 6), seed=23),
    }


def _efforts(gpu, packed, effort):
    """(device effort, host permutation and choice) for an effort number or the name "profile"."""
    if effort == "profile":
        plan = gpu.order_plan("profile", packed.nJ_max, packed.nM_max)
        assert plan[0] == "device"
        return plan[1], gpu.joint_order(packed.general(), "profile")
    return effort, gpu.profile_permutation(packed.general(), effort=effort)


def _upload(torch, packed, fields):
    return {f: torch.from_numpy(np.ascontiguousarray(getattr(packed, f))).cuda() for f in fields}


@pytest.mark.parametrize("effort", [1, 2, 3, "profile"])
@pytest.mark.parametrize("form", ["general", "table"])
def test_plain_form_reports_the_hosts_reach_and_permutation(gpu, batches, form, effort):
    import torch
    for name, packed in batches.items():
        dev_effort, perm = _efforts(gpu, packed, effort)
        shaped = packed.table() if form == "table" else packed.general()
        tensors = _upload(torch, shaped, ("xyz", "conn", "cbits", "loads", "nJ", "nM"))
        assert tensors["conn"].dtype == (torch.uint16 if form == "table" else torch.int32)
        for apply in (True, False):     # (with and without the renumbered inputs: the reach does not depend on them)
            out = gpu.joint_order_device(torch, tensors, effort=dev_effort, apply=apply)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(out["perm"].cpu().numpy(), perm, err_msg=f"{name} {form} {effort}")
            np.testing.assert_array_equal(out["reach"].cpu().numpy(), gpu.envelope_reach(packed.general(), perm),
                                          err_msg=f"{name} {form} {effort}")


@pytest.mark.parametrize("effort", [1, 2, 3, "profile"])
@pytest.mark.parametrize("form", ["general", "table"])
def test_gather_form_reports_the_hosts_reach_and_permutation(gpu, batches, form, effort):
    """`trs_joint_order_rows(_tab)`: some rows of a wider batch, in another order, into rows of their own width."""
    import torch
    lib = gpu._capi.load()
    stream = torch.cuda.current_stream().cuda_stream
    for name, packed in batches.items():
        rng = np.random.default_rng(5)
        pick = np.sort(rng.permutation(packed.B)[:max(1, packed.B // 3)])[::-1].copy()
        sub = packed.take(pick).trimmed()
        dev_effort, perm = _efforts(gpu, sub, effort)
        shaped = packed.table() if form == "table" else packed.general()
        fields = ("xyz", "conn", "cbits", "loads", "nJ", "nM") + (("type_idx",) if form == "table" else ("E", "A"))
        inp = _upload(torch, shaped, fields)
        rows = torch.from_numpy(pick.astype(np.int64)).cuda()
        count, nJ_max, nM_max = len(pick), sub.nJ_max, sub.nM_max
        new = lambda shape, like: torch.full(shape, 77, dtype=like.dtype, device="cuda")
        out = {"perm": torch.full([count, nJ_max], -1, dtype=torch.int32, device="cuda"),
               "reach": torch.full([count], -1, dtype=torch.int32, device="cuda"),
               "xyz": new([count, nJ_max, 3], inp["xyz"]), "conn": new([count, nM_max, 2], inp["conn"]),
               "cbits": new([count, nJ_max], inp["cbits"]), "loads": new([count, nJ_max, 3], inp["loads"]),
               "nJ": new([count], inp["nJ"]), "nM": new([count], inp["nM"])}
        if form == "table":
            out["type_idx"] = new([count, nM_max], inp["type_idx"])
            fn, sec_in, sec_out = lib.trs_joint_order_rows_tab, (inp["type_idx"],), (out["type_idx"],)
        else:
            out["E"], out["A"] = new([count, nM_max], inp["E"]), new([count, nM_max], inp["A"])
            fn, sec_in, sec_out = lib.trs_joint_order_rows, (inp["E"], inp["A"]), (out["E"], out["A"])
        gpu._capi.check(fn(
            count, nJ_max, nM_max, rows.data_ptr(), int(inp["xyz"].shape[1]), int(inp["conn"].shape[1]),
            inp["xyz"].data_ptr(), inp["conn"].data_ptr(), inp["cbits"].data_ptr(), inp["loads"].data_ptr(),
            *(s.data_ptr() for s in sec_in), inp["nJ"].data_ptr(), inp["nM"].data_ptr(), out["perm"].data_ptr(),
            out["reach"].data_ptr(), out["xyz"].data_ptr(), out["conn"].data_ptr(), out["cbits"].data_ptr(),
            out["loads"].data_ptr(), *(s.data_ptr() for s in sec_out), out["nJ"].data_ptr(), out["nM"].data_ptr(),
            int(dev_effort), stream), "trs_joint_order_rows")
        torch.cuda.synchronize()
        tag = f"{name} {form} {effort}"
        np.testing.assert_array_equal(out["perm"].cpu().numpy(), perm, err_msg=tag)
        np.testing.assert_array_equal(out["reach"].cpu().numpy(), gpu.envelope_reach(sub.general(), perm), err_msg=tag)
        np.testing.assert_array_equal(out["nJ"].cpu().numpy(), sub.nJ, err_msg=tag)
        np.testing.assert_array_equal(out["nM"].cpu().numpy(), sub.nM, err_msg=tag)
