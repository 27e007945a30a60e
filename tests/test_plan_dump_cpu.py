"""CPU test of tools/plan_dump.py: the dump of a dry-run executor's bound call plan names every device pointer by
its allocation and depends on no address, so two builds of the same plan print the same text."""
import importlib.util
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("plan_dump", os.path.join(REPO, "tools", "plan_dump.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("graph", ["small_resnet20", "small_resnet_int8"])
def test_dump_is_address_free(graph):
    pd = _tool()
    symf, shp = pd.SMALL[graph]

    def dump():
        ex = pd.Executor(pd.Plan(symf(), [("data", shp)], [("softmax_label", (shp[0],))]), "cpu")
        return ex, list(pd.Dump(ex).lines())
    ex1, a = dump()  # (kept alive: the second build's buffers lie at other addresses)
    ex2, b = dump()
    assert ex1.master.data_ptr() != ex2.master.data_ptr()
    assert a == b
    assert not [ln for ln in a if "RAW:" in ln]
    heads = {ln.split()[0] for ln in a}
    assert {"_fwd_train", "_fwd_infer", "_bwd", "wpack_calls", "param_done_at", "buckets"} <= heads
    assert sum(ln.count("A0+") for ln in a) > 0 and any("S0" in ln for ln in a)
    # a descriptor the backward edits after the forward bound it prints in its final state in both lists
    if graph == "small_resnet_int8":
        assert any(ln.startswith("_fwd_train") and "clip=A" in ln for ln in a)
