"""GDRQ (quantization with a mean-based clipping threshold and a symmetric signed code) without a GPU: the symbol
surface (mx.sym.contrib.GDRQ and mx.sym.Custom(op_type="GDRQ_PY")), the alphas' own initialisers on auxiliary
states, the plan's routing rule, the bind-time errors, a training step on mx.cpu() against the fp64 restatement, and
checkpoints."""
import json

import numpy as np
import pytest

import gdrq_util as U
import mxnet as mx
from graph_passes import _rebuild, shape_dict
from rn import graphs
from rn.executor import Plan, PlanError

SHAPE = (2, 3, 16, 16)


def _both_forms(**attrs):
    x = mx.sym.Activation(data=mx.sym.Variable("data"), act_type="relu", name="act")
    var = lambda: mx.sym.Variable("q_alpha", init=mx.init.Constant(1.0), dtype="float32")  # noqa: E731
    return [mx.sym.contrib.GDRQ(data=x, alpha=var(), name="q", **attrs),
            mx.sym.Custom(data=x, alpha=var(), op_type="GDRQ_PY", name="q", **attrs),
            mx.sym.contrib.GDRQ(data=x, name="q", **attrs),
            mx.sym.Custom(data=x, op_type="GDRQ_PY", name="q", **attrs)]


# ----------------------------------------------------------------------------- 1. symbol API
def test_symbol_lists_alpha_as_an_auxiliary_state():
    for s in _both_forms(nbits="4", fix_alpha="True"):
        assert s.list_arguments() == ["data"]
        assert s.list_auxiliary_states() == ["q_alpha"]
        args, outs, aux = s.infer_shape(data=(2, 8, 4, 4))
        assert args == [(2, 8, 4, 4)] and outs == [(2, 8, 4, 4)] and aux == [(1,)]


def test_json_round_trip_and_positional_rebuild():
    for s in _both_forms(nbits="4", is_weight="False", ktimes="3"):
        again = mx.sym.load_json(s.tojson())
        assert json.loads(again.tojson()) == json.loads(s.tojson())
        assert again.list_auxiliary_states() == ["q_alpha"] and again.list_arguments() == ["data"]
        # core/graph_optimize.py's reconstruction: positional children (data, then the aux state), string attrs
        rebuilt = _rebuild(s, lambda node, kids, attrs, op_of: None)
        assert json.loads(rebuilt.tojson())["nodes"] == json.loads(s.tojson())["nodes"]
        assert rebuilt.list_auxiliary_states() == ["q_alpha"]
        assert rebuilt.infer_shape(data=(2, 8, 4, 4))[2] == [(1,)]


def test_init_constants_arrive_in_aux_params():
    sym = U.gdrq_unit_net()
    mod = mx.mod.Module(sym, context=mx.cpu())
    mod.bind([("data", SHAPE)], [("softmax_label", (SHAPE[0],))])
    mod.init_params(mx.init.Xavier(rnd_type="gaussian", factor_type="in", magnitude=2))
    arg, aux = mod.get_params()
    assert not any(k.endswith("_alpha") for k in arg)
    wa = [k for k in aux if k.endswith("_weight_alpha")]
    da = [k for k in aux if k.endswith("_data_alpha")]
    assert len(wa) == 5 and len(da) == 5
    assert all(aux[k].shape == (1,) and aux[k].asnumpy()[0] == np.float32(0.5) for k in wa)
    assert all(aux[k].shape == (1,) and aux[k].asnumpy()[0] == np.float32(1.0) for k in da)
    assert all((v.asnumpy() == 1).all() for k, v in aux.items() if k.endswith("_moving_var"))


@pytest.mark.parametrize("op_name", ["GDRQ", "GDRQ_CXX"])
def test_attached_graph_trains_and_checkpoints_on_cpu(tmp_path, op_name):
    """A config-style run: attach_quantize_node with the config/quant_attrs.py GDRQ setting (every attribute a
    string) on ResNet-20, first convolution skipped as the reference's configs skip it; bind on mx.cpu(), two steps,
    checkpoint; every alpha is in the .params file as an auxiliary state, and a reload reproduces step 3's forward."""
    base = graphs.resnet20_cifar()
    shapes = shape_dict(base, (2, 3, 32, 32), (2,))
    w, a = U.gdrq_settings(op_name)
    sym = U.attach_quantize_node(base, shapes, w, a, skip_quantize_counts={"Convolution": 1})
    alphas = [n for n in sym.list_auxiliary_states() if n.endswith("_alpha")]
    assert len(alphas) == 19 + 21 and not any(n.endswith("_alpha") for n in sym.list_arguments())
    mod = mx.mod.Module(sym, context=mx.cpu())
    mod.bind([("data", (2, 3, 32, 32))], [("softmax_label", (2,))])
    mx.random.seed(3)
    mod.init_params(mx.init.Xavier(rnd_type="gaussian", factor_type="in", magnitude=2))
    mod.init_optimizer(optimizer="sgd", optimizer_params={"learning_rate": 0.1, "wd": 1e-4, "momentum": 0.9})
    data, label = U.batch((2, 3, 32, 32), 10, seed=5)
    b = mx.io.DataBatch(data=[mx.nd.array(data)], label=[mx.nd.array(label)])
    for _ in range(2):
        mod.forward(b, is_train=True)
        mod.backward()
        mod.update()
    prefix = str(tmp_path / op_name)
    mod.save_checkpoint(prefix, 2)
    saved = mx.nd.load(prefix + "-0002.params")
    assert all("aux:" + n in saved and saved["aux:" + n].shape == (1,) for n in alphas)
    assert not any(k.startswith("arg:") and k.endswith("_alpha") for k in saved)
    sym2, arg, aux = mx.model.load_checkpoint(prefix, 2)
    assert json.loads(sym2.tojson()) == json.loads(sym.tojson())
    # weights' thresholds follow 3 * mean|w|; the activations' stay at their initial 1.0
    assert all(aux[n].asnumpy()[0] == np.float32(1.0) for n in alphas if n.endswith("_data_alpha") or
               not n.endswith("_weight_alpha"))
    assert all(0 < aux[n].asnumpy()[0] != np.float32(0.5) for n in alphas if n.endswith("_weight_alpha"))
    m2 = mx.mod.Module(sym2, context=mx.cpu())
    m2.bind([("data", (2, 3, 32, 32))], [("softmax_label", (2,))])
    m2.init_params(arg_params=arg, aux_params=aux)
    m2.forward(b, is_train=True)
    mod.forward(b, is_train=True)
    assert np.isfinite(mod.get_outputs()[0].asnumpy()).all()
    np.testing.assert_array_equal(m2.get_outputs()[0].asnumpy(), mod.get_outputs()[0].asnumpy())


# ----------------------------------------------------------------------------- 2. routing, errors
def _plan(sym, monkeypatch=None, **env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return Plan(sym, [("data", SHAPE)], [("softmax_label", (SHAPE[0],))], dtype="float32")


def test_plan_routes_gdrq_convolutions_to_the_int8_forward(monkeypatch):
    monkeypatch.delenv("RN_INT8_MFMA", raising=False)
    p = _plan(U.gdrq_unit_net())
    assert p.summary()["gdrq"] == 5
    convs = [op for op in p.ops if op.kind == "conv"]
    acts = [op for op in p.ops if op.kind == "gdrq"]
    assert len(convs) == 4 and all(op.int8 and op.qsrc.kind == "gdrq" for op in convs)
    assert all(op.qweight["family"] == "gdrq" and op.qweight["nbits"] == 4 and not op.qweight["fix_alpha"] and
               op.qweight["ktimes"] == 3.0 for op in convs)
    # (the fc's GDRQ feeds no convolution: values only)
    assert [op.emit_codes for op in acts] == [op.name != "fc1_data" for op in acts]
    assert all(op.nbits == 4 and op.fix_alpha and not op.codes_wgrad for op in acts)
    # seven bits still fit a signed byte; eight do not, on either operand
    assert all(op.int8 for op in _plan(U.gdrq_unit_net(abits=7, wbits=7)).ops if op.kind == "conv")
    for q in (_plan(U.gdrq_unit_net(abits=8)), _plan(U.gdrq_unit_net(wbits=8)),
              _plan(U.gdrq_unit_net(), monkeypatch, RN_INT8_MFMA="0")):
        assert not any(op.int8 for op in q.ops if op.kind == "conv")
        assert not any(op.emit_codes for op in q.ops if op.kind == "gdrq")


def test_mixed_quantizer_pairs_lower(monkeypatch):
    monkeypatch.delenv("RN_INT8_MFMA", raising=False)
    # GDRQ activations with Quantization_int8 weights, PACT activations with GDRQ weights: int8 where both fit
    p = _plan(U.gdrq_unit_net(weight_op="Quantization_int8", wbits=8))
    assert all(op.int8 and op.qsrc.kind == "gdrq" and "family" not in op.qweight for op in p.ops if op.kind == "conv")
    p = _plan(U.gdrq_unit_net(act_op="PACT"))
    assert all(op.int8 and op.qsrc.kind == "pact" and op.qweight["family"] == "gdrq"
               for op in p.ops if op.kind == "conv")
    # an 8-bit GDRQ weight under a 4-bit PACT: the fake-quantized product
    p = _plan(U.gdrq_unit_net(act_op="PACT", wbits=8))
    assert not any(op.int8 for op in p.ops if op.kind == "conv")


def _one_quantizer(quant):
    x = mx.sym.Convolution(data=mx.sym.Variable("data"), num_filter=16, kernel=(3, 3), no_bias=True, name="c")
    x = quant(mx.sym.Activation(mx.sym.BatchNorm(x, name="b"), act_type="relu", name="r"))
    x = mx.sym.Pooling(data=x, global_pool=True, kernel=(1, 1), pool_type="avg")
    return mx.sym.SoftmaxOutput(mx.sym.FullyConnected(mx.sym.Flatten(x), num_hidden=4, name="fc"), name="softmax")


@pytest.mark.parametrize("form", ["contrib", "custom"])
def test_unsupported_attributes_fail_at_bind_by_name(form):
    make = mx.sym.contrib.GDRQ if form == "contrib" else \
        (lambda **kw: mx.sym.Custom(op_type="GDRQ_PY", **kw))
    for attr, value in (("group_size", "4"), ("delay_quant", "1")):
        s = _one_quantizer(lambda x: make(data=x, name="q", nbits="4", **{attr: value}))
        mod = mx.mod.Module(s, context=mx.cpu())
        with pytest.raises(PlanError, match="q: .*" + attr):
            mod.bind([("data", SHAPE)], [("softmax_label", (SHAPE[0],))])
    # the supported form of the same graph binds
    mod = mx.mod.Module(_one_quantizer(lambda x: make(data=x, name="q", nbits="4")), context=mx.cpu())
    mod.bind([("data", SHAPE)], [("softmax_label", (SHAPE[0],))])
    assert mod.executor.plan.summary()["gdrq"] == 1


def test_shared_alpha_is_refused():
    alpha = mx.sym.Variable("shared_alpha", init=mx.init.Constant(1.0))

    def two(x):
        a = mx.sym.contrib.GDRQ(data=x, alpha=alpha, name="qa", fix_alpha="True")
        b = mx.sym.contrib.GDRQ(data=x, alpha=alpha, name="qb", fix_alpha="True")
        return a + b
    mod = mx.mod.Module(_one_quantizer(two), context=mx.cpu())
    with pytest.raises(PlanError, match="shared_alpha is shared"):
        mod.bind([("data", SHAPE)], [("softmax_label", (SHAPE[0],))])


def test_made_up_custom_ops_stay_refused():
    s = _one_quantizer(lambda x: mx.sym.Custom(data=x, op_type="GDRQ_PY_V2", name="cu"))
    mod = mx.mod.Module(s, context=mx.cpu())
    with pytest.raises(PlanError, match="GDRQ_PY_V2"):
        mod.bind([("data", SHAPE)], [("softmax_label", (SHAPE[0],))])


# ----------------------------------------------------------------------------- 3. the restatements
def test_sum_chain_lengths():
    """The threshold bound's k, by hand (+ 3 for the count's conversion, the division and the product, + 1 for the
    second order): n = 16 fp32 is 4 chunks on 4 threads of one block: 4 serial adds + 6 + 2, one partial in one
    lane; n = 48051 bf16 is 24 blocks, 6006 chunks on 6144 threads (one round of 8) and a 3-element tail, 24
    partials in one lane; the capped grid: 2048 partials, 32 in each of 64 lanes. The weight pack: 64 x 256 threads,
    a 64 x 64 x 1 x 1 weight is 1024 chunks (one round of 4); a 3 x 3 64 -> 64 weight 9216 chunks."""
    assert U.gdrq_sum_chain(16, 4) == 4 + 6 + 2 + 1 + 1 + 3 + 1
    assert U.gdrq_sum_chain(1001 * 48 + 3, 2) == 8 + 1 + 6 + 2 + 24 + 1 + 3 + 1
    assert U.gdrq_sum_chain(2048 * 2048 * 8, 2) == 8 * 8 + 6 + 2 + 32 + 64 + 3 + 1
    assert U.wgdrq_sum_chain(64 * 64) == 4 + 6 + 2 + 64 + 3 + 1
    assert U.wgdrq_sum_chain(64 * 64 * 9) == 4 + 6 + 2 + 64 + 3 + 1
    assert U.wgdrq_sum_chain(64 * 256 * 4 * 2 + 3) == 2 * 4 + 1 + 6 + 2 + 64 + 3 + 1


def test_restatement_on_the_edge_inputs():
    """Two-sided clip, both boundaries, ties away from zero of both signs, the inclusive backward mask."""
    alpha, nbits = np.float32(7.5), 4  # unit = 0.5 exactly: every odd multiple of 0.25 is a representable tie
    x = U.edge_inputs(4160, False, alpha, np.float32(0.5), seed=1)
    v, q, unit = U.gdrq_fwd_ref(x, alpha, nbits)
    assert unit == np.float32(0.5) and q.min() == -15 and q.max() == 15
    assert (q[x >= alpha] == 15).all() and (q[x <= -alpha] == -15).all() and (x == alpha).any() and (x == -alpha).any()
    a = x[np.abs(x) < alpha] / unit
    ties = np.abs(a - np.trunc(a)) == 0.5
    assert (ties & (a > 0)).sum() >= 2 and (ties & (a < 0)).sum() >= 2
    assert np.array_equal(q[:8], [15, -15, 15, -15, 1, -1, 2, -3])  # (0.25 -> 1, -0.25 -> -1, 0.75 -> 2, -1.25 -> -3)
    dy = np.ones_like(x)
    dx = U.gdrq_bwd_ref(x, dy, alpha)
    assert (dx[np.abs(x) == alpha] == 1).all() and (dx[np.abs(x) > alpha] == 0).all()
    for bad in (0.0, -1.0):
        v, q, unit = U.gdrq_fwd_ref(x, bad, nbits)
        assert not v.any() and not q.any()
    assert U.gdrq_ema_ref(1.0, 0.25, 0.001) == np.float32(np.float32(1.0) + np.float32(np.float32(0.001) *
                                                                                     np.float32(0.75)))


# ----------------------------------------------------------------------------- 4. a step on mx.cpu()
# seeds and scales: init_net seed 0 (He-normal weights, scale 1), batch seed 1 (unit normal), activations' alpha 1.0
# -- checked on the CPU for both cases below: the fp32 torch step's codes differ from the free-running fp64 step's
# on at most 1 % of a node's elements and by one code (test_fp32_torch_step_meets_the_code_condition)
CASES = {"fixed": dict(act_fix_alpha=True), "moving": dict(act_fix_alpha=False, lamda=0.01)}


@pytest.fixture(scope="module", params=sorted(CASES))
def unit_case(request):
    sym = U.gdrq_unit_net(**CASES[request.param])
    params, aux = U.init_net(sym, SHAPE, seed=0)
    data, label = U.batch(SHAPE, 8, seed=1)
    return request.param, sym, params, aux, data, label


def test_fp32_torch_step_meets_the_code_condition(unit_case):
    import torch
    _, sym, params, aux, data, label = unit_case
    r32 = U.torch_step(sym, params, aux, data, label, torch.float32)
    free = U.torch_step(sym, params, aux, data, label, torch.float64)
    dec = {"gdrq": {k: {"codes": v["codes"].numpy()} for k, v in r32["decisions"]["gdrq"].items()}}
    mism = U.code_mismatch(dec, free)
    assert len(mism) == 10  # five weights, five activations
    print("worst code mismatch of the fp32 torch step", max(mism.values()))
    assert all(f <= 0.01 and d <= 1 for f, d in mism.values()), mism


def test_cpu_context_step_against_fp64(unit_case):
    case, sym, params, aux, data, label = unit_case
    res = U.module_step(sym, params, aux, data, label, mx.cpu(), steps=1)
    assert type(res["mod"].executor).__name__ == "CPUExecutor"
    figs = U.check_step(res, sym, params, aux, data, label)
    assert set(figs["codes"]) == set(aux) and len(aux) == 10
    dec = res["decisions"][0]["gdrq"]
    acts = [k for k in aux if k.endswith("_data_alpha")]
    # the thresholds clip (all but the fc's, whose pooled input stays below 1.0): the masks are not trivial
    clip = [k for k in aux if k != "fc1_data_alpha"]
    assert all(0 < dec[k]["mask"].mean() < 1 for k in acts if k in clip), {k: dec[k]["mask"].mean() for k in acts}
    assert all(np.abs(dec[k]["codes"]).max() == 15 for k in clip)
    assert all(dec[k]["codes"].min() == -15 for k in clip if k.endswith("_weight_alpha"))
    moved = [k for k in acts if res["aux"][0][k][0] != np.float32(1.0)]
    assert len(moved) == (0 if case == "fixed" else 5)
    assert all(res["aux"][0][k][0] != np.float32(0.5) for k in aux if k.endswith("_weight_alpha"))
