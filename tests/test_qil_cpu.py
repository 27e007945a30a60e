"""QIL (quantization-interval learning: a learned pruning point and clipping point per tensor) without a GPU: the
symbol surface of mx.sym.Custom(op_type="QIL_PY"), the plan's lowering and routing rule, the bind-time errors, a
training step on mx.cpu() against the fp64 restatement, the lr_mult / wd_mult the thresholds are created with, and
checkpoints."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import mxnet as mx
import qil_util as U
from graph_passes import shape_dict
from rn import graphs
from rn.executor import Executor, Plan, PlanError
from rn.plan import multipliers

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (2, 3, 16, 16)
f32 = np.float32


def _plan(sym, shape=SHAPE):
    return Plan(sym, [("data", shape)], [("softmax_label", (shape[0],))], dtype="float32")


def _head(x, name="fc"):
    pool = mx.sym.Pooling(data=x, global_pool=True, kernel=(1, 1), pool_type="avg")
    return mx.sym.SoftmaxOutput(mx.sym.FullyConnected(mx.sym.Flatten(pool), num_hidden=4, name=name), name="softmax")


def _qil(name, data, prune=None, clip=None, gamma=None, **attrs):
    var = lambda suffix, init: mx.sym.var(name=name + suffix, init=U.get_constant(init))  # noqa: E731
    attrs = {"nbits": "4", "is_weight": "False", "fix_gamma": "True", **attrs}
    return mx.sym.Custom(name=name, data=data, pruning_point=prune if prune is not None else var("_pruning_point", 0),
                         clipping_point=clip if clip is not None else var("_clipping_point", 1.0),
                         gamma=gamma if gamma is not None else var("_gamma", 1.0), op_type="QIL_PY", **attrs)


def _act(channels=16):
    x = mx.sym.Convolution(data=mx.sym.Variable("data"), num_filter=channels, kernel=(3, 3), pad=(1, 1),
                           no_bias=True, name="conv0")
    return mx.sym.Activation(mx.sym.BatchNorm(x, name="bn0"), act_type="relu", name="relu0")


# ----------------------------------------------------------------------------- 1. symbol API
def test_symbol_lists_three_trainable_scalars():
    s = _qil("q", mx.sym.Variable("data"))
    assert s.list_arguments() == ["data", "q_pruning_point", "q_clipping_point", "q_gamma"]
    assert s.list_auxiliary_states() == []
    args, outs, aux = s.infer_shape(data=(2, 8, 4, 4))
    assert args == [(2, 8, 4, 4), (1,), (1,), (1,)] and outs == [(2, 8, 4, 4)] and aux == []
    again = mx.sym.load_json(s.tojson())
    assert json.loads(again.tojson()) == json.loads(s.tojson())
    assert "QIL_PY" in mx.operator.get_registry()

    @mx.operator.register("QIL_PY")  # the reference's own registration (core/operator/QIL.py:154) is accepted
    class Prop(mx.operator.CustomOpProp):
        def __init__(self, is_weight="False", fix_gamma="True", nbits="4"):
            super().__init__(True)

        def list_arguments(self):
            return ["data", "pruning_point", "clipping_point", "gamma"]

        def infer_shape(self, in_shape):
            return [in_shape[0], [1], [1], [1]], [in_shape[0]], []
    assert mx.operator.get_registry()["QIL_PY"] is Prop
    assert _qil("q", mx.sym.Variable("data")).list_arguments() == s.list_arguments()


def test_graph_builders_name_and_attribute_the_variables_as_the_reference():
    sym = U.qil_unit_net()
    attrs = sym.attr_dict()
    for base in ("unit1_conv1_weight", "unit1_conv1_data", "fc1_weight", "fc1_data"):
        p, c, g = (attrs[base + s] for s in ("_pruning_point", "_clipping_point", "_gamma"))
        assert (p["__lr_mult__"], p["__wd_mult__"]) == ("0.01", "0") and json.loads(p["__init__"])[1]["value"] == 0
        assert (c["__lr_mult__"], c["__wd_mult__"]) == ("0.01", "0") and json.loads(c["__init__"])[1]["value"] == 1.0
        assert "__lr_mult__" not in g and "__wd_mult__" not in g and json.loads(g["__init__"])[1]["value"] == 1.0
    # the same variables and attributes as core/graph_optimize.py's create_quant_node writes
    v = mx.sym.Variable("w_weight", shape=(8, 8, 1, 1))
    ref = U.create_quant_node(v, U.qil_settings()[0]).attr_dict()
    mine = graphs._qil("w_weight", v, 4, True, 1.0).attr_dict()
    assert {k: ref[k] for k in ref if k != "w_weight"} == {k: mine[k] for k in mine if k != "w_weight"}
    big = graphs.resnet50_qil()
    assert sum(1 for k in big.list_arguments() if k.endswith("_pruning_point")) == 2 * 53
    assert not any(k.startswith("conv0") and "point" in k for k in big.list_arguments())  # conv0: Quantization_int8


# ----------------------------------------------------------------------------- 2. lowering and routing
def test_lowering_and_routing(monkeypatch):
    monkeypatch.delenv("RN_INT8_MFMA", raising=False)
    plan = _plan(U.qil_unit_net(abits=4, wbits=4))
    assert plan.summary()["qil"] == 5 and plan.summary()["conv"] == 4
    convs = [op for op in plan.ops if op.kind == "conv"]
    qils = [op for op in plan.ops if op.kind == "qil"]
    assert all(op.int8 and op.qsrc.kind == "qil" and op.qweight["family"] == "qil" for op in convs)
    assert [op.emit_codes for op in qils] == [op.name != "fc1_data" for op in qils]
    assert not any(op.codes_wgrad for op in qils)
    assert sorted(plan.param_names) == sorted(n for n in plan.arg_names if n not in ("data", "softmax_label"))
    assert sum(1 for n in plan.param_names if n.endswith(("_pruning_point", "_clipping_point"))) == 20
    assert not plan.aux_names or not any("point" in n for n in plan.aux_names)
    for kw in (dict(abits=7, wbits=7), dict(abits=1, wbits=1)):
        assert all(op.int8 for op in _plan(U.qil_unit_net(**kw)).ops if op.kind == "conv")
    for kw in (dict(abits=8, wbits=4), dict(abits=4, wbits=8)):  # codes up to 255 do not fit a signed byte
        p8 = _plan(U.qil_unit_net(**kw))
        assert not any(op.int8 for op in p8.ops if op.kind == "conv")
        assert not any(op.emit_codes for op in p8.ops if op.kind == "qil")
    monkeypatch.setenv("RN_INT8_MFMA", "0")
    assert not any(op.int8 for op in _plan(U.qil_unit_net()).ops if op.kind == "conv")


@pytest.mark.parametrize("act_op,weight_op", [("QIL", "Quantization_int8"), ("QIL", "GDRQ"), ("PACT", "QIL"),
                                              ("GDRQ", "QIL"), ("Quantization_int8", "QIL")])
def test_mixed_pairs_qualify_side_by_side(monkeypatch, act_op, weight_op):
    monkeypatch.delenv("RN_INT8_MFMA", raising=False)
    q = graphs.quant_conv("q1", _act(), 16, (1, 1), (1, 1), in_channels=16, act_op=act_op, weight_op=weight_op,
                          abits=4, wbits=4)
    plan = _plan(_head(mx.sym.Activation(mx.sym.BatchNorm(q, name="bn1"), act_type="relu")))
    (conv,) = [op for op in plan.ops if op.kind == "conv" and op.name == "q1"]
    assert conv.int8 and conv.qsrc.emit_codes
    assert conv.qsrc.kind == {"QIL": "qil", "PACT": "pact", "GDRQ": "gdrq", "Quantization_int8": "quant"}[act_op]


# ----------------------------------------------------------------------------- 3. bind-time errors
def test_plan_errors_name_the_offender():
    def net(q):
        conv = mx.sym.Convolution(data=q, num_filter=16, kernel=(1, 1), no_bias=True, name="conv1")
        return _head(mx.sym.Activation(mx.sym.BatchNorm(conv, name="bn1"), act_type="relu"))
    with pytest.raises(PlanError, match="qbad.*fix_gamma"):
        _plan(net(_qil("qbad", _act(), fix_gamma="False")))
    for nbits in ("0", "17"):
        with pytest.raises(PlanError, match="qbits.*nbits %s" % nbits):
            _plan(net(_qil("qbits", _act(), nbits=nbits)))
    # a pruning point shared by two quantizers
    shared = mx.sym.var(name="shared_point", init=U.get_constant(0))
    a = _act()
    x1 = mx.sym.Convolution(data=_qil("qa", a, prune=shared), num_filter=16, kernel=(1, 1), no_bias=True, name="c1")
    x2 = mx.sym.Convolution(data=_qil("qb", a, prune=shared), num_filter=16, kernel=(1, 1), no_bias=True, name="c2")
    with pytest.raises(PlanError, match="qb.*shared_point.*shared.*qa"):
        _plan(_head(mx.sym.Activation(mx.sym.BatchNorm(x1 + x2, name="bn1"), act_type="relu")))
    # one variable as both points of one quantizer
    with pytest.raises(PlanError, match="qsame.*shared_point.*shared"):
        _plan(net(_qil("qsame", _act(), prune=shared, clip=shared)))
    # a threshold that is no parameter Variable: a computed tensor
    with pytest.raises(PlanError, match="qcomp.*clipping_point.*parameter Variable"):
        _plan(net(_qil("qcomp", _act(), clip=mx.sym.identity(mx.sym.var("some_point", shape=(1,))))))
    # a weight quantizer over a computed tensor
    w = mx.sym.identity(mx.sym.Variable("conv1_weight", shape=(16, 16, 1, 1)))
    wq = _qil("conv1_weight_q", w, is_weight="True")
    bad = mx.sym.Convolution(data=_act(), weight=wq, num_filter=16, kernel=(1, 1), no_bias=True, name="conv1")
    with pytest.raises(PlanError, match="conv1_weight_q.*computed tensor"):
        _plan(_head(mx.sym.Activation(mx.sym.BatchNorm(bad, name="bn1"), act_type="relu")))
    # an activation quantizer over something that is no activation tensor: the raw data input
    with pytest.raises(PlanError, match="qdata.*non-activation"):
        _plan(net(_qil("qdata", mx.sym.Variable("data"))))
    # any other Custom op_type still fails with its name
    with pytest.raises(PlanError, match="other.*QIL_V2_PY"):
        _plan(net(mx.sym.Custom(data=_act(), op_type="QIL_V2_PY", name="other")))


# ----------------------------------------------------------------------------- 4. the kernels' restatement
@pytest.mark.parametrize("pc", [(0.25, 0.75), (0.0, 1.0), (-0.5, 1.5)])
@pytest.mark.parametrize("nbits", [1, 4, 8])
def test_float32_restatement_against_the_operator_in_fp64(pc, nbits):
    """qil_fwd_ref / qil_bwd_ref (the kernels' operation order, float32) against core/operator/QIL.py restated in
    fp64: the codes agree except where t * L falls within float32 rounding of a tie, dx up to alpha's rounding."""
    pp, cc = pc
    x = U.edge_inputs(4160, False, max(pp, 0.0), min(cc, 1.0), seed=nbits)
    dy = np.random.RandomState(1).randn(x.size).astype(np.float32)
    v, q, unit, p1, c1 = U.qil_fwd_ref(x, pp, cc, nbits)
    assert (p1, c1) == (f32(max(pp, 0.0)), f32(min(cc, 1.0)))
    ref = U.qil_fp64(x, pp, cc, nbits, dy=dy)
    assert np.array_equal(q, ref["codes"]) and np.abs(v - ref["out"]).max() <= 2.0 ** -24
    dx, dp, dc, _, _ = U.qil_bwd_ref(x, dy, pp, cc)
    assert np.abs(dx - ref["dx"]).max() <= 2.0 ** -22 * np.abs(ref["dx"]).max()
    assert dp == pytest.approx(ref["dp"], rel=1e-12) and dc == pytest.approx(ref["dc"], rel=1e-12)
    assert not dx[x == 0].any()


# ----------------------------------------------------------------------------- 5. a step on mx.cpu()
@pytest.fixture(scope="module")
def unit_case():
    sym = U.qil_unit_net(abits=4, wbits=4)
    params = U.init_qil_net(sym, SHAPE, seed=0)
    data, label = U.batch(SHAPE, 8, seed=1)
    return sym, params, data, label, U.module_step(sym, params, data, label, mx.cpu(), steps=2)


def test_cpu_context_step_against_fp64(unit_case):
    sym, params, data, label, res = unit_case
    U.check_step(res, sym, params, data, label, step=0)
    dec = res["decisions"][0]["qil"]
    assert len(dec) == 10
    for k, d in dec.items():  # elements below, inside and above every interval (the pooled fc input: none below)
        assert 0 < d["flag"].mean() < 1 and d["above"].any(), k
        assert (~d["flag"] & ~d["above"]).any() or k == "fc1_data_pruning_point", k
    points = [k for k in params if k.endswith(("_pruning_point", "_clipping_point"))]
    assert len(points) == 20 and all(res["grads"][0][k][0] != 0 for k in points)
    assert all(not res["grads"][0][k].any() for k in params if k.endswith(("_data_gamma", "_weight_gamma")))


def test_thresholds_train_at_their_own_rate_and_are_not_decayed(unit_case):
    """lr_mult 0.01 and wd_mult 0 (core/graph_optimize.py:171-172) reach the update: after the first step, from a
    zero momentum buffer, a pruning point has moved by exactly f32(f32(lr) * f32(0.01)) * f32(g * rescale) in
    float32, with no decay term; gamma, whose gradient is zero, is decayed by its name (MXNet's rule)."""
    sym, params, data, label, res = unit_case
    lr, wd, rescale = 0.1, 1e-4, 1.0 / SHAPE[0]
    o = res["mod"]._optimizer
    assert o.lr_mult["fc1_data_pruning_point"] == 0.01 and o.wd_mult["fc1_data_pruning_point"] == 0.0
    assert "fc1_weight" not in o.lr_mult and "fc1_weight" not in o.wd_mult and o.wd_mult["fc1_bias"] == 0.0
    lre = f32(f32(lr) * f32(0.01))
    for k in params:
        g = res["grads"][0][k].astype(np.float32)
        w0 = params[k].astype(np.float32)
        if k.endswith(("_pruning_point", "_clipping_point")):
            want = (w0 - (lre * (g * f32(rescale)).astype(np.float32)).astype(np.float32)).astype(np.float32)
            assert np.array_equal(res["args"][0][k], want), (k, res["args"][0][k], want)
            assert res["args"][0][k][0] != w0[0]
            plain = (w0 - (f32(lr) * (g * f32(rescale)).astype(np.float32)).astype(np.float32)).astype(np.float32)
            assert not np.array_equal(want, plain)
        elif k.endswith(("_data_gamma", "_weight_gamma")):
            want = (w0 - f32(f32(lr) * f32(wd))).astype(np.float32)
            assert not g.any() and np.array_equal(res["args"][0][k], want) and want[0] < 1.0


def test_checkpoint_keeps_the_three_scalars(unit_case, tmp_path):
    sym, params, _, _, res = unit_case
    mod = res["mod"]
    prefix = str(tmp_path / "qil")
    mod.save_checkpoint(prefix, 2)
    sym2, arg, aux = mx.model.load_checkpoint(prefix, 2)
    now = {k: v.asnumpy() for k, v in mod.get_params()[0].items()}
    names = [k for k in arg if k.endswith(("_pruning_point", "_clipping_point", "_weight_gamma", "_data_gamma"))]
    assert len(names) == 30 and not any("point" in k for k in aux)
    assert all(np.array_equal(arg[k].asnumpy(), now[k]) for k in names)
    assert sym2.attr_dict()["fc1_data_pruning_point"]["__lr_mult__"] == "0.01"
    again = mx.mod.Module(sym2, context=mx.cpu())
    again.bind([("data", SHAPE)], [("softmax_label", (SHAPE[0],))])
    again.set_params(arg, aux)
    back = {k: v.asnumpy() for k, v in again.get_params()[0].items()}
    assert all(np.array_equal(back[k], now[k]) for k in names)


def test_reference_route_binds_and_trains_on_cpu():
    base = graphs.resnet20_cifar()
    shapes = shape_dict(base, (4, 3, 32, 32), (4,))
    w, a = U.qil_settings()
    sym = U.attach_quantize_node(base, shapes, w, a, skip_quantize_counts={"Convolution": 1})
    mod = mx.mod.Module(sym, context=mx.cpu())
    mod.bind([("data", (4, 3, 32, 32))], [("softmax_label", (4,))])
    mx.random.seed(3)
    mod.init_params(mx.init.Xavier(rnd_type="gaussian", factor_type="in", magnitude=2))
    mod.init_optimizer(optimizer="sgd", optimizer_params={"learning_rate": 0.1, "wd": 1e-4, "momentum": 0.9})
    data, label = U.batch((4, 3, 32, 32), 10, seed=5)
    b = mx.io.DataBatch(data=[mx.nd.array(data)], label=[mx.nd.array(label)])
    for _ in range(2):
        mod.forward(b, is_train=True)
        mod.backward()
        mod.update()
    assert np.isfinite(mod.get_outputs()[0].asnumpy()).all()
    plan = mod.executor.plan
    # (one quantizer per quantized tensor: 19 activations feed the 20 quantized convolutions and the fc)
    assert plan.summary()["qil"] == 19 and sum(1 for op in plan.ops if op.qweight) == 21
    arg = mod.get_params()[0]
    act_c = [k for k in arg if k.endswith("_clipping_point") and "_weight_" not in k]
    assert len(act_c) == 19 and all(arg[k].asnumpy()[0] != 1.0 for k in act_c)  # each has a gradient and moved
    mod.forward(b, is_train=True)  # the next forward clamps what the update pushed outside [0, 1]
    arg = mod.get_params()[0]
    assert all(0 < arg[k].asnumpy()[0] <= 1.0 for k in arg if k.endswith("_clipping_point"))
    assert all(0 <= arg[k].asnumpy()[0] < 1.0 for k in arg if k.endswith("_pruning_point"))


# ----------------------------------------------------------------------------- 6. graphs without multipliers
def _dump(ex):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import plan_dump
    return "\n".join(plan_dump.Dump(ex).lines())


@pytest.mark.parametrize("graph", ["small_resnet_int8", "small_resnet20"])
def test_a_graph_without_multipliers_binds_the_same_plan(graph):
    """Without __lr_mult__ / __wd_mult__ attributes the multipliers are the name rule's, the learning-rate table
    stays away and the plan dump is the same text before and after they are set."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import plan_dump
    symf, shp = plan_dump.SMALL[graph]
    sym = symf()
    ex = Executor(Plan(sym, [("data", shp)], [("softmax_label", (shp[0],))]), "cpu")
    before = _dump(ex)
    assert "multipliers" not in before and "_lrm" not in before
    wd0 = ex.wd_mult.copy()
    lr_mult, wd_mult = multipliers(sym, ex.plan.param_names)
    assert lr_mult == {} and all(v == 0.0 for v in wd_mult.values())
    ex.set_multipliers(lr_mult, wd_mult)
    assert ex.opt_lrms is None and np.array_equal(ex.wd_mult, wd0) and (ex.lr_mult == 1).all()
    assert hashlib.sha256(_dump(ex).encode()).hexdigest() == hashlib.sha256(before.encode()).hexdigest()
    # a QIL graph's dump names the entry point with the table and every moved multiplier
    q = Executor(_plan(U.qil_unit_net()), "cpu")
    text = _dump(q)
    assert "update rn_sgd_mom_update" in text and "_lrm" in text
    assert text.count("multipliers ") == 20 and "rn_weight_qil_pack" in text and "rn_weight_qil_bwd" in text
