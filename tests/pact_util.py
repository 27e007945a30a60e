"""PACT test helpers: restatements of the two kernels, of a small PACT network in fp64, and the reference's
PACT graph surface driven through the `mxnet` shim's public API.

  pact_fwd_ref / pact_bwd_ref   numpy float32 restatements of rn_pact_fwd / rn_pact_bwd, bit for bit
                                (core/operator/PACT.py:102-144 with the arithmetic of include/rn.h)
  edge_inputs                   the kernels' edge inputs: negatives, values above and equal to gamma, exact ties
  pact_bwd_chain                the longest chain of fp32 additions of rn_pact_bwd's dgamma at a given n
  PactProp                      a CustomOpProp registered as "PACT_PY" (core/operator/PACT.py:146-166)
  create_quant_node / attach_quantize_node
                                core/graph_optimize.py:159-292 for quantize_op_name "PACT" (mx.sym.Custom),
                                "PACT_CXX" (mx.sym.contrib.PACT) and "Quantization_int8"
  pact_unit_net                 stem conv + one pre-activation bottleneck unit with a projection shortcut + head
  torch_step                    one training step of such a symbol in torch (fp64 or fp32), free-running or
                                replaying the discrete decisions a device made (ReLU masks, fake-quantized
                                weights, PACT codes and x < gamma masks)
  module_step / device_decisions  the same step through mx.mod.Module on mx.gpu() / mx.cpu(), with its decisions
"""
import ast
import json

import numpy as np
import torch
import torch.nn.functional as F

import mxnet as mx
from graph_passes import _rebuild
from rn import graphs


# ----------------------------------------------------------------------------- the kernels, restated
def bf16(a):
    """float32 array rounded to bf16 (nearest even) and widened again."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return t.to(torch.bfloat16).to(torch.float32).numpy()


def pact_fwd_ref(x, gamma, nbits, to_bf16=False):
    """(values, codes, unit) in numpy float32: unit = f32(g) / f32(L); a = c / unit; q = roundf(a) written as
    trunc(a) + sign(a) * (|a - trunc(a)| >= 0.5) -- the subtraction is exact, so there is no double rounding as in
    floor(|a| + 0.5) --; value = q * unit, rounded to bf16 where the storage is bf16. gamma <= 0: zeros."""
    x = np.asarray(x, dtype=np.float32)
    g = np.float32(gamma)
    unit = np.float32(g / np.float32(2 ** nbits - 1))
    if not unit > 0:
        return np.zeros_like(x), np.zeros_like(x), unit
    c = np.where(x < g, x, g).astype(np.float32)
    a = (c / unit).astype(np.float32)
    t = np.trunc(a)
    q = (t + np.sign(a) * (np.abs(a - t) >= np.float32(0.5))).astype(np.float32)
    v = (q * unit).astype(np.float32)
    return (bf16(v) if to_bf16 else v), q, unit


def pact_bwd_ref(x, dy, gamma, add=None, to_bf16=False):
    """(dx, dgamma in fp64, sum |dy * [x >= gamma]| in fp64): dx = dy * [x < gamma] (+ add, the add in fp32, then
    rounded to the storage type)."""
    x = np.asarray(x, dtype=np.float32)
    dy = np.asarray(dy, dtype=np.float32)
    keep = x < np.float32(gamma)
    dx = np.where(keep, dy, np.float32(0)).astype(np.float32)
    if add is not None:
        dx = (dx + np.asarray(add, dtype=np.float32)).astype(np.float32)
    clipped = np.where(keep, 0.0, dy.astype(np.float64))
    return (bf16(dx) if to_bf16 else dx), float(clipped.sum()), float(np.abs(clipped).sum())


def edge_inputs(n, to_bf16, gamma, unit, seed):
    """Negatives, values above gamma, elements equal to gamma, exact ties (odd multiples of unit / 2, both signs);
    rounded to the storage type first, so that the restatement sees what the device reads."""
    rng = np.random.RandomState(seed)
    x = (rng.randn(n) * 0.6 * gamma).astype(np.float32)
    x[rng.randint(0, n, size=max(n // 8, 2))] = gamma
    k = rng.randint(-7, 2 * 15, size=max(n // 4, 4))
    x[rng.randint(0, n, size=k.size)] = ((2 * k + 1) * (unit / 2)).astype(np.float32)
    x[:6] = [gamma, unit / 2, 2 * gamma, -gamma / 3, 3 * (unit / 2), -5 * (unit / 2)]  # (whatever the draw gave)
    return bf16(x) if to_bf16 else x


def pact_bwd_chain(n, itemsize):
    """The longest chain of fp32 additions on the way to rn_pact_bwd's dgamma[0], from its launch geometry
    (include/rn.h, csrc/rn_misc.hip pact_bwd_kernel): min(max(ceil(n / 2048), 1), 2048) blocks of 256 threads; a
    thread adds the 16 / itemsize elements of each of its 16-byte chunks one after the other, over
    ceil(chunks / threads) grid-stride rounds, plus at most one tail element; 6 butterfly stages across the 64
    lanes of a wave; 2 stages for the block's 4 waves; then the second launch: a lane adds 32 consecutive partials
    one after the other (fewer where there are fewer), and the ceil(blocks / 32) lane sums that are not zero are
    added one after the other (the zeros behind them add exactly)."""
    blocks = min(max(-(-n // 2048), 1), 2048)
    ce = 16 // itemsize
    rounds = -(-(n // ce) // (blocks * 256))
    per_thread = rounds * ce + (1 if n % ce else 0)
    return per_thread + 6 + 2 + min(blocks, 32) + -(-blocks // 32)


# ----------------------------------------------------------------------------- the reference's graph surface
@mx.operator.register("PACT_PY")
class PactProp(mx.operator.CustomOpProp):
    """core/operator/PACT.py:146-166; the shim reads list_arguments / infer_shape only (no Python op runs)."""

    def __init__(self, nbits="8"):
        self.nbits = int(nbits)
        super().__init__(True)

    def list_arguments(self):
        return ["data", "gamma"]

    def list_outputs(self):
        return ["output"]

    def infer_shape(self, in_shape):
        shape = in_shape[0]
        return [shape, [1]], [shape], []


def get_constant(value):
    """core/graph_optimize.py:32-34: the `__init__` attribute written by hand."""
    return '["constant", {"value": ' + str(value) + "}]"


def create_quant_node(var, setting):
    """core/graph_optimize.py:159-197 for the three supported quantize_op_name values."""
    name, attrs = setting["quantize_op_name"], setting.get("attrs", {})
    if name == "Quantization_int8":
        minmax = mx.sym.var(name=var.name + "_minmax", init=mx.init.Constant(setting.get("init_value") or 0))
        return mx.sym.contrib.Quantization_int8(name=var.name, data=var, minmax=minmax, **attrs)
    gamma = mx.sym.var(name=var.name + "_gamma", init=get_constant(setting.get("init_value") or 8.0))
    if name == "PACT":
        return mx.sym.Custom(name=var.name, data=var, gamma=gamma, **attrs, op_type="PACT_PY")
    assert name == "PACT_CXX", name
    return mx.sym.contrib.PACT(name=var.name, data=var, gamma=gamma, **attrs)


def attach_quantize_node(symbol, out_shape_dict, weight_setting, act_setting,
                         quantized_op=("Convolution", "FullyConnected", "Deconvolution"), skip_quantize_counts=None):
    """core/graph_optimize.py:199-292 (one quantizer per quantized tensor, whoever reads it)."""
    counts, made = {}, {}

    def quant(v, setting):
        if v.name not in made:
            made[v.name] = create_quant_node(v, setting)
        return made[v.name]

    def visit(node, kids, attrs, op_of):
        op = node["op"]
        if op not in quantized_op:
            return None
        counts[op] = counts.get(op, 0) + 1
        if skip_quantize_counts and counts[op] <= skip_quantize_counts.get(op, 0):
            new_kids = kids
        else:
            new_kids = [quant(kids[0], act_setting), quant(kids[1], weight_setting)] + kids[2:]
        return getattr(mx.sym, op)(*new_kids, name=node["name"], **attrs)

    graph = json.loads(symbol.tojson())
    for node in graph["nodes"]:
        if node["op"] == "null":
            a = node.setdefault("attrs", {})
            if "__shape__" not in a:
                a["__shape__"] = str(tuple(out_shape_dict[node["name"]]))
                a["__dtype__"] = "0"
    return _rebuild(mx.sym.load_json(json.dumps(graph)), visit)


def pact_settings(op_name, abits=4, wbits=8, init_value=None):
    """(weight_setting, act_setting) of a config-style run: Quantization_int8 weights, PACT activations."""
    w = {"quantize_op_name": "Quantization_int8", "init_value": 0,
         "attrs": {"nbits": str(wbits), "quant_mode": "minmax", "is_weight": "True", "is_weight_perchannel": "False",
                   "delay_quant": "0", "ema_decay": "0.99", "grad_mode": "ste"}}
    a = {"quantize_op_name": op_name, "init_value": init_value, "attrs": {"nbits": str(abits)}}
    return w, a


# ----------------------------------------------------------------------------- the small network
def pact_unit_net(num_classes=8, abits=4, wbits=8, pact_init=2.0, width=256):
    """Stem conv (3x3 / stride 2, unquantized) -> one pre-activation bottleneck unit width -> width/4 -> width/4 ->
    width with a projection shortcut (symbol/resnet_int8.py:12-66, every conv quantized: Quantization_int8 weights,
    PACT activations) -> BN + ReLU -> global average pool -> quantized fc -> softmax. conv1 is a 1x1 convolution
    from `width` to width / 4 channels and conv3 / the shortcut are 1x1 convolutions to `width`: the shapes at
    which the unquantized graph streams its data gradient / forward, and fuses BatchNorm work into them."""
    qkw = dict(act_op="PACT", abits=abits, wbits=wbits, pact_init=pact_init)
    data = mx.sym.Variable(name="data")
    body = mx.sym.Convolution(data=data, num_filter=width, kernel=(3, 3), stride=(2, 2), pad=(1, 1), no_bias=True,
                              name="conv0")
    body = graphs._int8_unit(body, width, width, (1, 1), False, "unit1", True, 0.9, qkw)
    body = graphs._relu(graphs._bn(body, "bn1"), "relu1")
    pool = mx.sym.Pooling(data=body, global_pool=True, kernel=(7, 7), pool_type="avg", name="pool1")
    fc = graphs.quant_fc("fc1", mx.sym.Flatten(data=pool), num_classes, width, **qkw)
    return mx.sym.SoftmaxOutput(data=fc, name="softmax")


def init_net(sym, data_shape, seed=0, weight_scale=1.0):
    """Deterministic fp32 parameters for every argument of `sym` but data / label: He-normal weights, BatchNorm
    gammas near 1 and betas near 0 (so that gradients are not degenerate), each PACT gamma from its own `__init__`
    attribute."""
    rng = np.random.RandomState(seed)
    arg_shapes, _, _ = sym.infer_shape(data=data_shape, softmax_label=(data_shape[0],))
    attrs = sym.attr_dict()
    params = {}
    for name, shp in zip(sym.list_arguments(), arg_shapes):
        if name in ("data", "softmax_label"):
            continue
        init = attrs.get(name, {}).get("__init__")
        if init:
            params[name] = np.full(shp, json.loads(init)[1]["value"], dtype=np.float32)
        elif name.endswith("_weight"):
            fan_in = int(np.prod(shp[1:]))
            params[name] = (rng.randn(*shp) * weight_scale * np.sqrt(2.0 / fan_in)).astype(np.float32)
        elif name.endswith("_gamma"):
            params[name] = (1.0 + 0.1 * rng.randn(*shp)).astype(np.float32)
        else:
            params[name] = (0.1 * rng.randn(*shp)).astype(np.float32)
    return params


def batch(data_shape, num_classes, seed=1, scale=1.0):
    rng = np.random.RandomState(seed)
    return (rng.randn(*data_shape) * scale).astype(np.float32), \
        rng.randint(0, num_classes, size=(data_shape[0],)).astype(np.float32)


# ----------------------------------------------------------------------------- the step in torch
def _lit(v, default=None):
    if v is None:
        return default
    try:
        return ast.literal_eval(v)
    except (ValueError, SyntaxError):
        return v


def _round_half_away(a):
    t = torch.trunc(a)
    return t + torch.sign(a) * ((a - t).abs() >= 0.5).to(a.dtype)


def torch_step(sym, params, data, label, dtype=torch.float64, replay=None, lr=0.1, wd=1e-4, momentum=0.9):
    """One forward / backward / SGD step of `sym` (read from its JSON) in torch at `dtype`, with MXNet's
    semantics: training-mode BatchNorm (biased variance), SoftmaxOutput's p - onehot gradient, Quantization_int8
    weights (t = max|w|, STE), PACT (c = where(x < gamma, x, gamma); out = round_half_away(c / unit) * unit with
    unit = gamma / L outside the recorded region), and the FIRST SGD step (the momentum buffer starts at zero, so
    `momentum` does not enter): w -= lr * (g / batch + wd * w), wd for *_weight / *_gamma and 0 otherwise.

    replay = {"relu": {Activation name: bool mask}, "wq": {quantizer name: values}, "pact": {gamma name:
    {"codes": .., "mask": ..}}} substitutes a device's discrete decisions; whatever is missing runs free. Returns
    prob, grads, args (after the update) and the decisions this run made itself."""
    replay = replay or {}
    tt = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)  # noqa: E731
    leaves = {k: tt(v).clone().requires_grad_(True) for k, v in params.items()}
    made = {"relu": {}, "wq": {}, "pact": {}}
    graph = json.loads(sym.tojson())
    vals = []
    logits = None
    for node in graph["nodes"]:
        op, name, a = node["op"], node["name"], node.get("attrs", {})
        ins = [vals[i] for i, _, *_ in node["inputs"]]
        if op == "null":
            out = tt(data) if name == "data" else tt(label) if name == "softmax_label" else leaves.get(name)
        elif op == "Convolution":
            assert _lit(a.get("no_bias"), False) and _lit(a.get("num_group"), 1) == 1
            out = F.conv2d(ins[0], ins[1], stride=_lit(a.get("stride"), (1, 1)), padding=_lit(a.get("pad"), (0, 0)))
        elif op == "BatchNorm":
            x, g, b = ins[0], ins[1], ins[2]
            if _lit(a.get("fix_gamma"), True):
                g = torch.ones_like(g)
            mean = x.mean(dim=(0, 2, 3), keepdim=True)
            var = ((x - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
            out = (x - mean) / torch.sqrt(var + float(_lit(a.get("eps"), 1e-3))) * g.view(1, -1, 1, 1) + \
                b.view(1, -1, 1, 1)
        elif op == "Activation":
            assert a["act_type"] == "relu"
            m = replay.get("relu", {}).get(name)
            m = (ins[0].detach() > 0) if m is None else \
                torch.as_tensor(np.asarray(m), dtype=torch.bool).reshape(ins[0].shape)
            made["relu"][name] = m
            out = ins[0] * m.to(dtype)
        elif op == "Pooling":
            assert _lit(a.get("global_pool"), False) and a.get("pool_type") == "avg"
            out = ins[0].mean(dim=(2, 3), keepdim=True)
        elif op == "Flatten":
            out = ins[0].reshape(ins[0].shape[0], -1)
        elif op == "FullyConnected":
            out = F.linear(ins[0], ins[1], ins[2] if len(ins) > 2 else None)
        elif op in ("_Plus", "elemwise_add"):
            out = ins[0] + ins[1]
        elif op == "_contrib_Quantization_int8":
            assert _lit(a.get("is_weight"), False), "only weight quantizers here"
            w = ins[0]
            v = replay.get("wq", {}).get(name)
            if v is None:
                unit = w.detach().abs().max() / float(2 ** (int(_lit(a.get("nbits"), 8)) - 1) - 1)
                v = _round_half_away(w.detach() / unit) * unit
            else:
                v = tt(v).reshape(w.shape)
            made["wq"][name] = v
            out = w + (v - w.detach())
        elif op == "_contrib_PACT" or (op == "Custom" and a.get("op_type") == "PACT_PY"):
            x, g = ins[0], ins[1]
            gname = graph["nodes"][node["inputs"][1][0]]["name"]
            levels = float(2 ** int(_lit(a.get("nbits"), 8)) - 1)
            unit = (g / levels).detach()
            r = replay.get("pact", {}).get(gname)
            if r is None:
                keep = x.detach() < g.detach()
                c = torch.where(keep, x, g.expand_as(x))
                q = _round_half_away(c.detach() / unit)
            else:
                keep = torch.as_tensor(np.asarray(r["mask"]), dtype=torch.bool).reshape(x.shape)
                c = torch.where(keep, x, g.expand_as(x))
                q = tt(r["codes"]).reshape(x.shape)
            made["pact"][gname] = {"codes": q, "mask": keep}
            out = c + (q * unit - c).detach()
        elif op == "SoftmaxOutput":
            logits = ins[0]
            out = torch.softmax(logits.detach(), dim=1)
        else:
            raise NotImplementedError(op)
        vals.append(out)
    prob = vals[graph["heads"][0][0]]
    onehot = F.one_hot(tt(label).long(), prob.shape[1]).to(dtype)
    logits.backward(prob - onehot)
    nb = prob.shape[0]
    grads, args = {}, {}
    for k, p in leaves.items():
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        grads[k] = g.numpy().copy()
        wdk = wd if (k.endswith("_weight") or k.endswith("_gamma")) else 0.0
        args[k] = (p.detach() - lr * (g / nb + wdk * p.detach())).numpy().copy()
    return {"prob": prob.numpy().copy(), "grads": grads, "args": args, "decisions": made}


# ----------------------------------------------------------------------------- the step through the Module
def _nchw(ex, t, buf):
    a = buf.float().cpu().numpy()
    if t.h == 1 and t.w == 1 and len(t.shape) == 2:
        return a.reshape(t.n, t.cp)[:, :t.c]
    return a.reshape(t.n, t.h, t.w, t.cp)[..., :t.c].transpose(0, 3, 1, 2)


def device_decisions(ex):
    """The discrete decisions of the executor's last forward, in torch_step's replay format. The GPU executor's are
    read back from its buffers: a PACT's codes from its int8 code buffer where it emits one, else from its values
    (code * unit, exact in fp32: the quotient rounds back to the integer); its mask from its stored input and the
    gamma the forward read."""
    if type(ex).__name__ == "CPUExecutor":
        d = ex.decisions
        return {"relu": {k: v.numpy() for k, v in d["relu"].items()},
                "wq": {k: v.numpy() for k, v in d["wq"].items()},
                "pact": {k: {"codes": v["codes"].numpy(), "mask": v["mask"].numpy(), "unit": v["unit"]}
                         for k, v in d["pact"].items()}}
    from step_util import gpu_quant_values, gpu_relu_masks
    out = {"relu": gpu_relu_masks(ex), "wq": {k: v for k, v in gpu_quant_values(ex).items()}, "pact": {}}
    for op in ex.plan.ops:
        if op.kind != "pact":
            continue
        gamma = np.float32(ex.get_param(op.gamma)[0])
        unit = float(op.unit.cpu().numpy()[0])
        x = _nchw(ex, op.x, ex.act(op.x)).astype(np.float32)
        if op.codes is not None:
            codes = _nchw(ex, op.x, op.codes).astype(np.float64)
        else:
            codes = np.rint(_nchw(ex, op.y, ex.act(op.y)).astype(np.float64) / unit)
        out["pact"][op.gamma] = {"codes": codes, "mask": x < gamma, "unit": unit, "gamma": float(gamma),
                                 "values": _nchw(ex, op.y, ex.act(op.y)).astype(np.float64)}
    return out


def module_step(sym, params, data, label, ctx, steps=1, lr=0.1, wd=1e-4, momentum=0.9, precision="float32"):
    """bind / init / forward / backward / update (core/solver.py:75-121); per step the probabilities, the decisions,
    the gradients and the parameters after the update."""
    kw = {} if ctx.device_type == "cpu" else {"precision": precision}
    mod = mx.mod.Module(sym, context=[ctx], **kw)
    mod.bind(data_shapes=[("data", data.shape)], label_shapes=[("softmax_label", label.shape)], for_training=True)
    mod.init_params(arg_params={k: v for k, v in params.items()}, aux_params=None, allow_missing=False)
    mod.init_optimizer(kvstore="local", optimizer="sgd",
                       optimizer_params={"learning_rate": lr, "wd": wd, "momentum": momentum})
    b = mx.io.DataBatch(data=[mx.nd.array(data)], label=[mx.nd.array(label)])
    ex = mod.executor
    out = {"prob": [], "decisions": [], "grads": [], "args": [], "mod": mod}
    for _ in range(steps):
        mod.forward(b, is_train=True)
        out["prob"].append(mod.get_outputs()[0].asnumpy().copy())
        out["decisions"].append(device_decisions(ex))
        mod.backward()
        out["grads"].append({n: ex.get_param(n, grad=True) for n in ex.plan.param_names})
        mod.update()
        out["args"].append({k: v.asnumpy() for k, v in mod.get_params()[0].items()})
    return out


def fro_rel(a, b):
    a = np.asarray(a, np.float64).ravel()
    b = np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-12))


def check_step(res, sym, params, data, label, step=0, base_tol=1e-4, factor=4.0, code_cap=0.01, **hyper):
    """The bar of step_util.replayed_parity for one Module step `res` (module_step): against the fp64 torch_step
    replaying the run's own decisions -- probabilities within base_tol of the largest one; every gradient and every
    updated parameter within max(base_tol, factor x the error the same replayed step makes in fp32), Frobenius-
    relative. And the condition under which that comparison means something: against the FREE-running fp64 step the
    run's PACT codes differ on at most `code_cap` of a node's elements and by at most one code. Returns the figures;
    raises AssertionError with the worst offenders."""
    dec = res["decisions"][step]
    ref = torch_step(sym, params, data, label, torch.float64, replay=dec, **hyper)
    r32 = torch_step(sym, params, data, label, torch.float32, replay=dec, **hyper)
    free = torch_step(sym, params, data, label, torch.float64, **hyper)
    figs = {"prob": float(np.abs(res["prob"][step] - ref["prob"]).max() / np.abs(ref["prob"]).max()), "codes": {},
            "grads": {}, "args": {}}
    for gname, d in dec["pact"].items():
        diff = np.abs(np.asarray(d["codes"], np.float64).ravel() -
                      free["decisions"]["pact"][gname]["codes"].numpy().ravel())
        figs["codes"][gname] = (float((diff != 0).mean()), float(diff.max()))
    for kind in ("grads", "args"):
        for n, v in ref[kind].items():
            e32 = fro_rel(r32[kind][n], v)
            figs[kind][n] = (fro_rel(res[kind][step][n], v), e32, max(base_tol, factor * e32))
    print("prob %.2e; worst code mismatch %s; worst grad %s; worst arg %s" % (
        figs["prob"], max(figs["codes"].values()), max(figs["grads"].items(), key=lambda kv: kv[1][0] / kv[1][2]),
        max(figs["args"].items(), key=lambda kv: kv[1][0] / kv[1][2])))
    bad_codes = {k: v for k, v in figs["codes"].items() if v[0] > code_cap or v[1] > 1}
    assert not bad_codes, bad_codes
    assert figs["prob"] < base_tol, figs["prob"]
    for kind in ("grads", "args"):
        bad = {k: v for k, v in figs[kind].items() if v[0] > v[2]}
        assert not bad, (kind, bad)
    return figs
