"""PACT (activation quantization with a learned clipping threshold) without a GPU: the symbol surface
(mx.sym.contrib.PACT and mx.sym.Custom(op_type="PACT_PY")), the variables' own initialisers, the plan's routing
rule, the bind-time errors, a training step on mx.cpu() against the fp64 restatement, and checkpoints."""
import json
import os

import numpy as np
import pytest

import mxnet as mx
import pact_util as U
from graph_passes import _rebuild, shape_dict
from rn import graphs
from rn.executor import Plan, PlanError

SHAPE = (2, 3, 16, 16)


def _both_forms(nbits="4"):
    x = mx.sym.Activation(data=mx.sym.Variable("data"), act_type="relu", name="act")
    return [mx.sym.contrib.PACT(data=x, nbits=nbits, name="q"),
            mx.sym.Custom(data=x, nbits=nbits, op_type="PACT_PY", name="q"),
            mx.sym.Custom(data=x, gamma=mx.sym.var("q_gamma", init=U.get_constant(8.0)), nbits=nbits,
                          op_type="PACT_PY", name="q")]


# ----------------------------------------------------------------------------- 1. symbol API
def test_symbol_lists_gamma_and_infers_its_shape():
    for s in _both_forms():
        assert s.list_arguments() == ["data", "q_gamma"]
        assert s.list_auxiliary_states() == []
        args, outs, aux = s.infer_shape(data=(2, 8, 4, 4))
        assert args == [(2, 8, 4, 4), (1,)] and outs == [(2, 8, 4, 4)] and aux == []


def test_json_round_trip_and_positional_rebuild():
    for s in _both_forms():
        again = mx.sym.load_json(s.tojson())
        assert json.loads(again.tojson()) == json.loads(s.tojson())
        # core/graph_optimize.py's reconstruction: positional children, string attrs
        rebuilt = _rebuild(s, lambda node, kids, attrs, op_of: None)
        assert json.loads(rebuilt.tojson())["nodes"] == json.loads(s.tojson())["nodes"]
        assert rebuilt.list_arguments() == ["data", "q_gamma"]
        assert rebuilt.infer_shape(data=(2, 8, 4, 4))[0][1] == (1,)


def test_unregistered_custom_keeps_one_input():
    s = mx.sym.Custom(data=mx.sym.Variable("data"), op_type="NOT_REGISTERED_ANYWHERE", name="c")
    assert s.list_arguments() == ["data"]
    assert s.infer_shape(data=(2, 8, 4, 4))[1] == [(2, 8, 4, 4)]


@pytest.mark.parametrize("op_name", ["PACT", "PACT_CXX"])
def test_attach_puts_one_pact_per_quantized_tensor(op_name):
    sym = graphs.resnet20_cifar()
    shapes = shape_dict(sym, (2, 3, 32, 32), (2,))
    w, a = U.pact_settings(op_name, abits=4, init_value=6.0)
    q = U.attach_quantize_node(sym, shapes, w, a)
    nodes = json.loads(q.tojson())["nodes"]
    is_pact = lambda n: n["op"] == "_contrib_PACT" or (n["op"] == "Custom" and n["attrs"]["op_type"] == "PACT_PY")
    pacts = [n for n in nodes if is_pact(n)]
    convs = [n for n in nodes if n["op"] in ("Convolution", "FullyConnected")]
    # every conv / fc reads a PACT; the tensors read by two convolutions (a stage's first unit: conv1 and the
    # projection shortcut read the same ReLU output) get one node
    read = [nodes[c["inputs"][0][0]] for c in convs]
    assert all(is_pact(n) for n in read)
    sources = {n["inputs"][0][0] for n in pacts}
    assert len(sources) == len(pacts) == len({id(n) for n in read}) < len(convs)
    assert len(convs) - len(pacts) == 2  # stage2_unit1 and stage3_unit1
    gam = [n for n in q.list_arguments() if n.endswith("_gamma") and q.attr_dict()[n].get("__init__")]
    assert len(gam) == len(pacts)
    assert all(json.loads(q.attr_dict()[n]["__init__"]) == ["constant", {"value": 6.0}] for n in gam)
    assert not any(n.endswith("_gamma") for n in q.list_auxiliary_states())


# ----------------------------------------------------------------------------- 2. initialisation
def test_variables_own_initialisers_are_honoured():
    sym = U.pact_unit_net(pact_init=8.0)
    for init_value, s in ((8.0, sym), (3.5, U.pact_unit_net(pact_init=3.5))):
        mod = mx.mod.Module(s, context=mx.cpu())
        mod.bind([("data", SHAPE)], [("softmax_label", (SHAPE[0],))])
        mod.init_params(mx.init.Xavier(rnd_type="gaussian", factor_type="in", magnitude=2))
        arg, aux = mod.get_params()
        pact = [k for k in arg if k.endswith("_data_gamma")]
        assert len(pact) == 5
        for k, v in arg.items():
            v = v.asnumpy()
            if k in pact:
                assert v.shape == (1,) and v[0] == np.float32(init_value), k
            elif k.endswith("_gamma"):
                assert (v == 1).all(), k
            elif k.endswith("_beta") or k.endswith("_bias"):
                assert (v == 0).all(), k
            else:
                assert k.endswith("_weight") and v.std() > 0, k
        assert all((v.asnumpy() == 0).all() for k, v in aux.items() if k.endswith("_minmax"))
    # a *_weight variable with init=Constant(0.25) gets 0.25, not the global initializer's draw
    x = mx.sym.Convolution(data=mx.sym.Variable("data"), weight=mx.sym.var("c_weight", init=mx.init.Constant(0.25)),
                           num_filter=8, kernel=(3, 3), no_bias=True, name="c")
    x = mx.sym.Pooling(data=mx.sym.Activation(mx.sym.BatchNorm(x, name="b"), act_type="relu"), global_pool=True,
                       kernel=(1, 1), pool_type="avg")
    s = mx.sym.SoftmaxOutput(mx.sym.FullyConnected(mx.sym.Flatten(x), num_hidden=4, name="fc"), name="softmax")
    mod = mx.mod.Module(s, context=mx.cpu())
    mod.bind([("data", SHAPE)], [("softmax_label", (SHAPE[0],))])
    mod.init_params(mx.init.Xavier())
    arg, _ = mod.get_params()
    assert (arg["c_weight"].asnumpy() == np.float32(0.25)).all()
    assert arg["fc_weight"].asnumpy().std() > 0 and (arg["b_gamma"].asnumpy() == 1).all()
    # by name: constant, zero, one
    for init, want in ((mx.init.Zero(), 0.0), (mx.init.One(), 1.0), ('["zero", {}]', 0.0), ('["one", {}]', 1.0)):
        arr = mx.nd.zeros((3,)) + 7
        mx.init.Xavier()(mx.init.InitDesc("v_weight", {"__init__": init if isinstance(init, str) else init.dumps()}),
                         arr)
        assert (arr.asnumpy() == want).all()


# ----------------------------------------------------------------------------- 3. errors, routing
def test_other_custom_op_types_fail_at_bind_by_name():
    x = mx.sym.Convolution(data=mx.sym.Variable("data"), num_filter=16, kernel=(3, 3), no_bias=True, name="c")
    x = mx.sym.Custom(data=mx.sym.Activation(mx.sym.BatchNorm(x, name="b"), act_type="relu"),
                      op_type="SOMETHING_ELSE", name="cu")
    x = mx.sym.Pooling(data=x, global_pool=True, kernel=(1, 1), pool_type="avg")
    s = mx.sym.SoftmaxOutput(mx.sym.FullyConnected(mx.sym.Flatten(x), num_hidden=4, name="fc"), name="softmax")
    mod = mx.mod.Module(s, context=mx.cpu())
    with pytest.raises(PlanError, match="SOMETHING_ELSE"):
        mod.bind([("data", SHAPE)], [("softmax_label", (SHAPE[0],))])
    with pytest.raises(mx.MXNetError, match="DoReFa"):
        mx.sym.contrib.DoReFa(data=mx.sym.Variable("data"))


def _plan(sym, monkeypatch=None, **env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return Plan(sym, [("data", SHAPE)], [("softmax_label", (SHAPE[0],))], dtype="float32")


def test_plan_routes_pact_convolutions_to_the_int8_forward(monkeypatch):
    monkeypatch.delenv("RN_INT8_MFMA", raising=False)
    p = _plan(U.pact_unit_net(abits=4))
    assert p.summary()["pact"] == 5
    convs = [op for op in p.ops if op.kind == "conv"]
    pacts = [op for op in p.ops if op.kind == "pact"]
    assert len(convs) == 4 and all(op.int8 and op.qsrc.kind == "pact" for op in convs)
    # (the fc's PACT feeds no convolution: values only)
    assert [op.emit_codes for op in pacts] == [op.name != "fc1_data" for op in pacts]
    assert all(op.nbits == 4 and not op.codes_wgrad for op in pacts)
    # seven bits still fit a signed byte; eight do not
    assert all(op.int8 for op in _plan(U.pact_unit_net(abits=7)).ops if op.kind == "conv")
    for q in (_plan(U.pact_unit_net(abits=8)), _plan(U.pact_unit_net(abits=4), monkeypatch, RN_INT8_MFMA="0")):
        assert not any(op.int8 for op in q.ops if op.kind == "conv")
        assert not any(op.emit_codes for op in q.ops if op.kind == "pact")


def test_pact_of_a_tensor_that_may_be_negative_keeps_the_values_path(monkeypatch):
    monkeypatch.delenv("RN_INT8_MFMA", raising=False)
    data = mx.sym.Variable("data")
    x = mx.sym.Convolution(data=data, num_filter=64, kernel=(3, 3), pad=(1, 1), no_bias=True, name="conv0")
    bn = mx.sym.BatchNorm(x, fix_gamma=False, name="bn")  # no ReLU: the PACT's input has both signs
    neg = graphs.quant_conv("qneg", bn, 64, (1, 1), (1, 1), in_channels=64, act_op="PACT", abits=4)
    pos = graphs.quant_conv("qpos", mx.sym.Activation(bn, act_type="relu", name="relu"), 64, (1, 1), (1, 1),
                            in_channels=64, act_op="PACT", abits=4)
    pooled = mx.sym.Pooling(data=mx.sym.Activation(neg + pos, act_type="relu", name="relu2"), kernel=(2, 2),
                            stride=(2, 2), pool_type="max", name="pool")
    qpool = graphs.quant_conv("qpool", pooled, 64, (1, 1), (1, 1), in_channels=64, act_op="PACT", abits=4)
    head = mx.sym.Pooling(data=mx.sym.Activation(mx.sym.BatchNorm(qpool, name="bn1"), act_type="relu"),
                          global_pool=True, kernel=(1, 1), pool_type="avg")
    s = mx.sym.SoftmaxOutput(mx.sym.FullyConnected(mx.sym.Flatten(head), num_hidden=4, name="fc"), name="softmax")
    p = _plan(s)
    int8 = {op.name: op.int8 for op in p.ops if op.kind == "conv"}
    assert int8 == {"qneg": False, "qpos": True, "qpool": True}
    codes = {op.name: op.emit_codes for op in p.ops if op.kind == "pact"}
    assert codes == {"qneg_data": False, "qpos_data": True, "qpool_data": True}


def test_no_batchnorm_fusion_crosses_a_pact(monkeypatch):
    """The BatchNorm+ReLU feeding a PACT writes its output, and a convolution reading a PACT output neither
    applies a BatchNorm on load nor reduces / applies one in its data gradient -- with the int8 forward and, where
    the plain predicates would otherwise fire (1x1, unquantized-looking shapes), without it."""
    for env in ({}, {"RN_INT8_MFMA": "0"}):
        for k in ("RN_INT8_MFMA",):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        monkeypatch.setenv("RN_DRY_RUN", "1")
        monkeypatch.setenv("RN_BN_BWD_RECOMPUTE", "1")  # (whatever the size: the predicate itself must decline)
        mod = mx.mod.Module(U.pact_unit_net(), context=[mx.gpu(0)], precision="bfloat16")
        mod.bind([("data", SHAPE)], [("softmax_label", (SHAPE[0],))])
        ex = mod.executor
        pact_in = {id(op.x) for op in ex.plan.ops if op.kind == "pact"}
        fed = [op for op in ex.plan.ops if op.kind == "bn" and id(op.y) in pact_in]
        assert [op.name for op in fed] == ["unit1_bn1", "unit1_bn2", "unit1_bn3"]
        for op in ex.plan.ops:
            if op in fed:
                assert not op.apply_fused and not op.apply_in_quant and not op.recomputed, op.name
                assert not getattr(op.y, "virtual", False)
            if op.kind == "conv":
                assert op.xf is None, op.name
        names = [c[0] for c in ex._bwd]
        assert names.count("rn_pact_bwd") == 5
        assert not any(n.startswith("rn_conv_bwd_data_bn") for n in names), names
        # bn1 / bn2 / bn3 of the unit feed PACTs: each runs its own full backward
        assert names.count("rn_bn_bwd") >= 3
        fwd = [c[0] for c in ex._fwd_train]
        assert fwd.count("rn_pact_fwd") == 5
        assert ("rn_conv_fwd_i8" in fwd) == (not env)
        # every PACT gamma has its place in the flat buffers and closes its gradient bucket
        for op in ex.plan.ops:
            if op.kind == "pact":
                assert op.gamma in ex.param_off and ex.param_done_at[op.gamma] > 0
                assert ex.wd_mult[ex.param_order.index(op.gamma)] == 1.0


# ----------------------------------------------------------------------------- 3b. the two restatements agree
@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("nbits", [4, 7, 8])
@pytest.mark.parametrize("to_bf16", [False, True], ids=["fp32", "bf16"])
def test_layerwise_restatement_equals_the_kernel_tests(to_bf16, nbits, with_add):
    """tests/layerwise.py restates rn_pact_fwd / rn_pact_bwd in torch (pact_fwd_torch / pact_bwd_torch, what the
    layer-by-layer checker holds the device to); the kernel tests hold the device to pact_util.pact_fwd_ref /
    pact_bwd_ref in numpy. The two must not drift apart: equal element for element on the kernel tests' edge
    inputs (negatives, values above gamma, elements equal to gamma, exact ties of both signs), with a gamma whose
    4-bit unit is exact (7.5) and one whose unit is rounded (1.25), and for a non-positive gamma."""
    import torch
    from layerwise import pact_bwd_torch, pact_fwd_torch
    n = 1001 * 48 + 3
    for gamma in (np.float32(7.5), np.float32(1.25)):
        unit = np.float32(gamma / np.float32(2 ** nbits - 1))
        x = U.edge_inputs(n, to_bf16, gamma, unit, seed=n + nbits)
        assert (x < 0).any() and (x > gamma).any() and (x == gamma).any()
        a = x[x < gamma] / unit
        ties = np.abs(a - np.trunc(a)) == 0.5
        if nbits == 4 and gamma == np.float32(7.5):
            assert (ties & (a > 0)).sum() >= 2 and (ties & (a < 0)).sum() >= 2  # (exact ties of both signs are in)
        want, wcodes, wunit = U.pact_fwd_ref(x, gamma, nbits, to_bf16=to_bf16)
        val, codes, tunit = pact_fwd_torch(torch.from_numpy(x), float(gamma), nbits, to_bf16=to_bf16)
        assert np.float32(tunit.item()) == wunit and tunit.dtype == torch.float32
        assert np.array_equal(val.numpy(), want) and val.dtype == torch.float32
        assert np.array_equal(codes.numpy(), wcodes)
        assert codes.max().item() == 2 ** nbits - 1 and (val.numpy()[x < 0] < 0).any()
        rng = np.random.RandomState(7 + nbits)
        rd = U.bf16 if to_bf16 else (lambda v: v)
        dy = rd(rng.randn(n).astype(np.float32))
        add = rd(rng.randn(n).astype(np.float32)) if with_add else None
        wdx, wdg, wabs = U.pact_bwd_ref(x, dy, gamma, add, to_bf16=to_bf16)
        dx, dg, terms = pact_bwd_torch(torch.from_numpy(x), torch.from_numpy(dy), float(gamma),
                                       None if add is None else torch.from_numpy(add), to_bf16=to_bf16)
        assert np.array_equal(dx.numpy(), wdx) and wabs > 0
        assert abs(terms - wabs) <= 1e-12 * wabs and abs(dg - wdg) <= 1e-12 * wabs  # (fp64 sums, any order)
    for gamma in (0.0, -1.0):
        val, codes, tunit = pact_fwd_torch(torch.from_numpy(x), gamma, nbits, to_bf16=to_bf16)
        want, wcodes, wunit = U.pact_fwd_ref(x, gamma, nbits, to_bf16=to_bf16)
        assert not val.numpy().any() and not codes.numpy().any() and not want.any() and not wcodes.any()
        assert np.float32(tunit.item()) == wunit


# ----------------------------------------------------------------------------- 4. a step on mx.cpu()
@pytest.fixture(scope="module")
def unit_case():
    sym = U.pact_unit_net(abits=4, wbits=8, pact_init=2.0)
    params = U.init_net(sym, SHAPE, seed=0)
    data, label = U.batch(SHAPE, 8, seed=1)
    return sym, params, data, label


def test_cpu_context_step_against_fp64(unit_case):
    sym, params, data, label = unit_case
    res = U.module_step(sym, params, data, label, mx.cpu(), steps=1)
    assert type(res["mod"].executor).__name__ == "CPUExecutor"
    figs = U.check_step(res, sym, params, data, label)
    moved = [k for k, v in res["grads"][0].items() if k.endswith("_data_gamma") and v[0] != 0]
    assert len(moved) >= 4, res["grads"][0]  # (the thresholds clip: their gradients are not trivially zero)
    assert set(figs["codes"]) == {k for k in params if k.endswith("_data_gamma")}


def test_attached_graph_trains_and_checkpoints_on_cpu(tmp_path):
    """A config-style run: attach_quantize_node with PACT (Custom) / PACT_CXX (contrib) activations and
    Quantization_int8 weights on ResNet-20, first convolution skipped as the reference's configs skip it; bind, one
    step, checkpoint; the gammas are in the .params file under their argument names."""
    base = graphs.resnet20_cifar()
    shapes = shape_dict(base, (2, 3, 32, 32), (2,))
    for op_name in ("PACT", "PACT_CXX"):
        w, a = U.pact_settings(op_name, abits=4, init_value=3.0)
        sym = U.attach_quantize_node(base, shapes, w, a, skip_quantize_counts={"Convolution": 1})
        mod = mx.mod.Module(sym, context=mx.cpu())
        mod.bind([("data", (2, 3, 32, 32))], [("softmax_label", (2,))])
        mx.random.seed(3)
        mod.init_params(mx.init.Xavier(rnd_type="gaussian", factor_type="in", magnitude=2))
        mod.init_optimizer(optimizer="sgd", optimizer_params={"learning_rate": 0.1, "wd": 1e-4, "momentum": 0.9})
        data, label = U.batch((2, 3, 32, 32), 10, seed=5)
        mod.forward(mx.io.DataBatch(data=[mx.nd.array(data)], label=[mx.nd.array(label)]), is_train=True)
        mod.backward()
        mod.update()
        prefix = str(tmp_path / op_name)
        mod.save_checkpoint(prefix, 1)
        sym2, arg, aux = mx.model.load_checkpoint(prefix, 1)
        gam = [k for k in arg if k.endswith("_gamma") and sym.attr_dict()[k].get("__init__")]
        assert len(gam) == 19 and all(arg[k].shape == (1,) for k in gam)
        now = mod.get_params()[0]
        assert all(arg[k].asnumpy()[0] == now[k].asnumpy()[0] != 0 for k in gam)
        assert any(arg[k].asnumpy()[0] != np.float32(3.0) for k in gam)  # (trained, not just initialised)
        assert json.loads(sym2.tojson()) == json.loads(sym.tojson())
        m2 = mx.mod.Module(sym2, context=mx.cpu())
        m2.bind([("data", (2, 3, 32, 32))], [("softmax_label", (2,))], for_training=False)
        m2.init_params(arg_params=arg, aux_params=aux)
        b = mx.io.DataBatch(data=[mx.nd.array(data)], label=[mx.nd.array(label)])
        m2.forward(b, is_train=False)
        mod.forward(b, is_train=False)
        np.testing.assert_array_equal(m2.get_outputs()[0].asnumpy(), mod.get_outputs()[0].asnumpy())
        assert os.path.exists(prefix + "-0001.params")
