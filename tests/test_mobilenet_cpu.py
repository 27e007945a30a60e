"""MobileNet-v1 (symbol/mobilenet.py) without a GPU: the graph builder against a restatement on the numpy
oracle, one step on mx.cpu() against the fp64 oracle, and the depthwise descriptors' host-side layout
(rn_conv_desc_init / rn_conv_pack_numel, rn_set_tuning 28)."""
import ctypes as C

import numpy as np
import pytest

import mxnet as mx
from mobilenet_util import oracle_mobilenet
from oracle import net as onet
from rn import graphs, lib as L
from rn.executor import Plan
from step_util import max_rel, oracle_step
from test_cpu_context import _check_grads, _module_step


def _plan(sym, batch, res, **kw):
    return Plan(sym, [("data", (batch, 3, res, res))], [("softmax_label", (batch,))], **kw)


def test_mobilenet_plan_summary_and_flops():
    p = _plan(graphs.mobilenet_1_0(), 256, 224)
    assert p.summary() == {"stem": 1, "bn": 27, "conv": 26, "pool": 1, "fc": 1, "softmax": 1}
    dw = [op for op in p.ops if op.kind == "conv" and op.groups > 1]
    assert len(dw) == 13 and all(op.groups == op.x.c == op.y.c and tuple(op.kernel) == (3, 3) for op in dw)
    assert abs(p.train_flops() / 1e9 - 868.036) < 0.01


def test_mobilenet_parameters_match_the_restated_graph():
    sym = graphs.mobilenet_1_0()
    g = oracle_mobilenet(1000)
    names = [n for n in sym.list_arguments() if n not in ("data", "softmax_label")]
    assert names == list(g.params)
    assert sym.list_auxiliary_states() == list(g.aux)
    assert len(names) == 83 and len(g.aux) == 54
    p = _plan(sym, 2, 224)
    assert {n: tuple(p.param_shape(n)) for n in names} == g.params
    assert sum(int(np.prod(s)) for s in g.params.values()) == 4231976
    assert graphs.get_symbol_compact(1000).list_arguments() == sym.list_arguments()
    internals = sym.get_internals().list_outputs()
    for node in ("conv_1_conv2d", "conv_2_dw_conv2d", "conv_14_dw_conv2d", "conv_14_batchnorm", "global_pool",
                 "flatten", "fc", "softmax"):
        assert node + "_output" in internals, node


def test_mobilenet_alpha_and_resolution():
    p = _plan(graphs.mobilenet(10, alpha=0.75, resolution=96), 2, 96)
    dw = [op for op in p.ops if op.kind == "conv" and op.groups > 1]
    assert [op.groups for op in dw] == [24 * m for m in (1, 2, 4, 4, 8, 8, 16, 16, 16, 16, 16, 16, 32)]
    with pytest.raises(AssertionError):
        graphs.mobilenet(10, alpha=0.3)
    with pytest.raises(AssertionError):
        graphs.mobilenet(10, resolution=100)
    with pytest.raises(AssertionError):
        graphs.get_symbol_compact(10, alpha=0.3)


def test_mobilenet_one_step_on_cpu():
    """alpha 0.25, 8 classes, batch 4, 64x64 on mx.cpu() against the fp64 oracle; bars of test_cpu_context."""
    g = oracle_mobilenet(8, 0.25)
    args, aux = onet.init_params(g)
    data, label = onet.synthetic_batch(4, (3, 64, 64), 8)
    res = _module_step(graphs.mobilenet(8, alpha=0.25, resolution=64), args, aux, data, label)
    assert type(res["mod"].executor).__name__ == "CPUExecutor"
    ref = oracle_step(g, args, aux, data, label)
    ref32 = oracle_step(g, args, aux, data, label, dtype=np.float32)
    assert max_rel(res["prob"][0], ref["prob"][0]) < 1e-4
    _check_grads(res, ref, ref32)


def _desc(lib, dtype=L.RN_BF16, c=64, r=3, pad=1, stride=1):
    d = L.ConvDesc(dtype=dtype, n=2, h=14, w=14, c=c, c_real=c, k=c, k_pad=c, r=r, s=r, stride_h=stride,
                   stride_w=stride, pad_h=pad, pad_w=pad, groups=c)
    assert lib.rn_conv_desc_init(C.byref(d)) == 0, lib.rn_last_error()
    return d


def test_depthwise_layout_is_fixed_at_descriptor_init():
    lib = L.load()
    d = _desc(lib)
    assert d.grouped_direct == 2
    assert lib.rn_conv_pack_numel(C.byref(d), 0) == lib.rn_conv_pack_numel(C.byref(d), 1) == 9 * 64
    assert lib.rn_conv_tile(C.byref(d), 0) == 0 and lib.rn_conv_tile(C.byref(d), 1) == 0
    assert _desc(lib, stride=2).grouped_direct == 2 and _desc(lib, c=24).grouped_direct == 2
    assert _desc(lib, c=1024).grouped_direct == 2
    try:
        assert lib.rn_set_tuning(28, 1) == 0
        d2 = _desc(lib)
        assert d2.grouped_direct == 0
        assert lib.rn_conv_pack_numel(C.byref(d2), 0) == lib.rn_conv_pack_numel(C.byref(d2), 1) == 64 * 9 * 64
        assert lib.rn_conv_pack_numel(C.byref(d), 0) == 9 * 64  # the first descriptor keeps its layout
    finally:
        lib.rn_set_tuning(28, 0)
    assert _desc(lib, dtype=L.RN_F32).grouped_direct == 0
    assert _desc(lib, c=2048).grouped_direct == 0
    assert _desc(lib, r=5, pad=2).grouped_direct == 0
    # the slab workspace the weight gradient needs: whole [c][9] fp32 partials, one per workgroup
    ws = lib.rn_conv_wgrad_ws_bytes(C.byref(d))
    assert ws > 0 and ws % (64 * 9 * 4) == 0
