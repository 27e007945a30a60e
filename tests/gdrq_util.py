"""GDRQ test helpers: restatements of the kernels, of a small GDRQ network in fp64, and the reference's GDRQ graph
surface driven through the `mxnet` shim's public API.

  gdrq_fwd_ref / gdrq_bwd_ref   numpy float32 restatements of rn_gdrq_fwd's quantize pass / rn_gdrq_bwd, bit for bit
                                (core/operator/GDRQ.py:64-86,124-133 with the arithmetic of include/rn.h)
  gdrq_thr_ref / gdrq_ema_ref   the threshold ktimes * mean|x| in fp64, and the activation update applied to a given
                                threshold in float32, one rounding per operation
  edge_inputs                   two-sided edge inputs: values beyond +-alpha, equal to +-alpha, exact ties of both signs
  gdrq_sum_chain / wgdrq_sum_chain
                                the longest chain of fp32 roundings on the way to the threshold of rn_gdrq_fwd /
                                rn_weight_gdrq_pack at a given size
  wgdrq_pack_ref                the copies rn_weight_gdrq_pack writes, from a given alpha
  GdrqProp                      a CustomOpProp registered as "GDRQ_PY" (core/operator/GDRQ.py:154-190)
  create_quant_node / attach_quantize_node
                                core/graph_optimize.py:159-292 for quantize_op_name "GDRQ" (mx.sym.Custom) and
                                "GDRQ_CXX" (mx.sym.contrib.GDRQ)
  gdrq_unit_net                 stem conv + one pre-activation bottleneck unit with a projection shortcut + head
  torch_step                    one training step of such a symbol in torch (fp64 or fp32), free-running or
                                replaying the discrete decisions a device made (ReLU masks, GDRQ codes and
                                |x| <= alpha masks of activations, GDRQ codes of weights)
  module_step / device_decisions / check_step
                                the same step through mx.mod.Module on mx.gpu() / mx.cpu(), and its bar
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


def _roundf(a):
    """roundf (half away from zero) of a float32 array: a - trunc(a) is exact, so no double rounding."""
    t = np.trunc(a)
    return (t + np.sign(a) * (np.abs(a - t) >= np.float32(0.5))).astype(np.float32)


def gdrq_fwd_ref(x, alpha, nbits, to_bf16=False):
    """(values, codes, unit) in numpy float32: unit = f32(alpha) / f32(L), L = 2^nbits - 1; c = min(max(x, -alpha),
    alpha); q = roundf(c / unit); value = q * unit, rounded to bf16 where the storage is bf16. alpha <= 0: zeros."""
    x = np.asarray(x, dtype=np.float32)
    a = np.float32(alpha)
    unit = np.float32(a / np.float32(2 ** nbits - 1))
    if not unit > 0:
        return np.zeros_like(x), np.zeros_like(x), unit
    c = np.minimum(np.maximum(x, -a), a).astype(np.float32)
    q = _roundf((c / unit).astype(np.float32))
    v = (q * unit).astype(np.float32)
    return (bf16(v) if to_bf16 else v), q, unit


def gdrq_bwd_ref(x, dy, alpha, add=None, to_bf16=False):
    """dx = dy * [|x| <= alpha], the boundary included (+ add, the add in fp32, then rounded to the storage type)."""
    x = np.asarray(x, dtype=np.float32)
    dx = np.where(np.abs(x) <= np.float32(alpha), np.asarray(dy, dtype=np.float32), np.float32(0)).astype(np.float32)
    if add is not None:
        dx = (dx + np.asarray(add, dtype=np.float32)).astype(np.float32)
    return bf16(dx) if to_bf16 else dx


def gdrq_thr_ref(x, ktimes, count=None):
    """ktimes * sum|x| / count in fp64 (count: the real element count where x carries zero padding)."""
    x = np.asarray(x, dtype=np.float64)
    return float(ktimes) * float(np.abs(x).sum()) / float(x.size if count is None else count)


def gdrq_ema_ref(alpha0, thr, lamda):
    """The activation update of include/rn.h on a float32 threshold: alpha0 + lamda * (alpha0 - thr) -- the
    reference's sign --, the subtraction, the product and the sum each rounded to float32."""
    a0, t, lam = np.float32(alpha0), np.float32(thr), np.float32(lamda)
    return np.float32(a0 + np.float32(lam * np.float32(a0 - t)))


def edge_inputs(n, to_bf16, alpha, unit, seed, levels=15):
    """Values of both signs beyond +-alpha, elements equal to +alpha and to -alpha, exact ties (odd multiples of
    unit / 2, both signs); rounded to the storage type first, so that the restatement sees what the device reads."""
    rng = np.random.RandomState(seed)
    x = (rng.randn(n) * 0.8 * alpha).astype(np.float32)
    m = max(n // 8, 2)
    x[rng.randint(0, n, size=m)] = alpha
    x[rng.randint(0, n, size=m)] = -alpha
    k = rng.randint(-levels, levels, size=max(n // 4, 4))
    x[rng.randint(0, n, size=k.size)] = ((2 * k + 1) * (unit / 2)).astype(np.float32)
    head = [alpha, -alpha, 2 * alpha, -3 * alpha, unit / 2, -unit / 2, 3 * (unit / 2), -5 * (unit / 2)]
    x[:min(n, len(head))] = head[:n]  # (whatever the draw gave)
    return bf16(x) if to_bf16 else x


def gdrq_sum_chain(n, itemsize):
    """An upper bound k on the roundings between the exact ktimes * sum|x| / count and rn_gdrq_fwd's float32
    threshold, from its launch geometry (include/rn.h, csrc/rn_misc.hip gdrq_abssum_kernel / gdrq_alpha_kernel):
    min(max(ceil(n / 2048), 1), 2048) blocks of 256 threads; a thread adds the 16 / itemsize elements of each of its
    16-byte chunks one after the other, over ceil(chunks / threads) grid-stride rounds, plus at most one tail
    element; 6 butterfly stages across the 64 lanes of a wave; 2 stages for the block's 4 waves; then the second
    launch: a lane adds 32 consecutive partials one after the other (fewer where there are fewer), and the
    ceil(blocks / 32) lane sums that are not zero are added one after the other. Then the conversion of the count,
    the division and the product with ktimes: 3 more. Every term is non-negative, so the relative error is at most
    (1 + u)^k - 1 <= (k + 1) u for u = 2^-24 and k (k + 1) u <= 1: the + 1 is that second-order slack."""
    blocks = min(max(-(-n // 2048), 1), 2048)
    ce = 16 // itemsize
    rounds = -(-(n // ce) // (blocks * 256))
    per_thread = rounds * ce + (1 if n % ce else 0)
    return per_thread + 6 + 2 + min(blocks, 32) + -(-blocks // 32) + 3 + 1


def wgdrq_sum_chain(n):
    """The same bound for rn_weight_gdrq_pack on a 16-byte aligned master of n floats (wgdrq_abssum_kernel /
    wgdrq_state_kernel): 64 blocks of 256 threads per weight, a thread adds the 4 elements of each of its chunks
    over ceil(chunks / 16384) rounds plus at most one tail element; 6 + 2 stages; the 64 block partials added one
    after the other; the count's conversion, the division, the product; + 1 for the second order."""
    rounds = -(-(n // 4) // (64 * 256))
    return rounds * 4 + (1 if n % 4 else 0) + 6 + 2 + 64 + 3 + 1


def wgdrq_pack_ref(w, alpha, nbits, c, k_pad, to_bf16):
    """What rn_weight_gdrq_pack writes for the master w (K, RS, c_real), from a given alpha: qw (master layout), the
    int8 codes and the forward copy (K, RS, c; channels >= c_real left zero) and the data-gradient copy (c, RS,
    k_pad; columns >= K left zero), the copies rounded to bf16 where the call's dtype is bf16."""
    K, RS, cr = w.shape
    v, q, unit = gdrq_fwd_ref(w, alpha, nbits)
    vs = bf16(v) if to_bf16 else v
    codes = np.zeros((K, RS, c), dtype=np.int8)
    codes[..., :cr] = q.astype(np.int8)
    krsc = np.zeros((K, RS, c), dtype=np.float32)
    krsc[..., :cr] = vs
    crsk = np.zeros((c, RS, k_pad), dtype=np.float32)
    crsk[:cr, :, :K] = vs.transpose(2, 1, 0)
    return v, codes, krsc, crsk, unit


# ----------------------------------------------------------------------------- the reference's graph surface
def _flag(v):
    return v if isinstance(v, bool) else {"True": True, "False": False}[str(v)]


@mx.operator.register("GDRQ_PY")
class GdrqProp(mx.operator.CustomOpProp):
    """core/operator/GDRQ.py:154-190; the shim reads list_arguments / list_auxiliary_states / infer_shape only (no
    Python op runs)."""

    def __init__(self, nbits=4, group_size=-1, is_weight="False", lamda=0.001, delay_quant=0, fix_alpha="False",
                 ktimes=3):
        self.nbits, self.group_size, self.is_weight = int(nbits), int(group_size), _flag(is_weight)
        self.lamda, self.delay_quant = float(lamda), int(delay_quant)
        self.fix_alpha, self.ktimes = _flag(fix_alpha), float(ktimes)
        super().__init__(True)

    def list_arguments(self):
        return ["data"]

    def list_outputs(self):
        return ["output"]

    def list_auxiliary_states(self):
        return ["alpha"]

    def infer_shape(self, in_shape):
        shape = in_shape[0]
        if self.group_size == -1:
            return [shape], [shape], [[1]]
        return [shape], [shape], [[shape[0 if self.is_weight else 1] // self.group_size]]


def create_quant_node(var, setting):
    """core/graph_optimize.py:188-195: the alpha variable '<quantized tensor>_alpha' with its own initialiser."""
    name, attrs = setting["quantize_op_name"], setting.get("attrs", {})
    alpha = mx.sym.Variable(name=var.name + "_alpha", init=mx.init.Constant(setting.get("init_value") or 1.0),
                            dtype="float32")
    if name == "GDRQ":
        return mx.sym.Custom(name=var.name, data=var, alpha=alpha, **attrs, op_type="GDRQ_PY")
    assert name == "GDRQ_CXX", name
    return mx.sym.contrib.GDRQ(name=var.name, data=var, alpha=alpha, **attrs)


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


def gdrq_settings(op_name, wbits=4, abits=4, act_fix_alpha=True, **over):
    """(weight_setting, act_setting) as config/quant_attrs.py writes the GDRQ setting: every attribute a string."""
    def one(is_weight, nbits, fix_alpha, init):
        attrs = {"nbits": str(nbits), "fix_alpha": str(fix_alpha), "group_size": "-1", "is_weight": str(is_weight),
                 "lamda": "0.001", "delay_quant": "0", "ktimes": "3"}
        attrs.update({k: str(v) for k, v in over.items()})
        return {"quantize_op_name": op_name, "init_value": init, "attrs": attrs}
    return one(True, wbits, False, 0.5), one(False, abits, act_fix_alpha, 1.0)


# ----------------------------------------------------------------------------- the small network
def gdrq_unit_net(num_classes=8, abits=4, wbits=4, act_fix_alpha=True, act_init=1.0, lamda=0.001, width=256,
                  weight_op="GDRQ", act_op="GDRQ"):
    """Stem conv (3x3 / stride 2, unquantized) -> one pre-activation bottleneck unit width -> width/4 -> width/4 ->
    width with a projection shortcut (symbol/resnet_int8.py:12-66, every conv quantized) -> BN + ReLU -> global
    average pool -> quantized fc -> softmax, with the GDRQ setting of config/quant_attrs.py: weights follow
    3 * mean|w|, activations clip at `act_init` (fixed, or moving with `lamda` when act_fix_alpha is False)."""
    qkw = dict(act_op=act_op, weight_op=weight_op, abits=abits, wbits=wbits)
    if act_op == "GDRQ":
        qkw["gdrq_act"] = dict(fix_alpha=act_fix_alpha, init=act_init, lamda=lamda, ktimes=3)
    data = mx.sym.Variable(name="data")
    body = mx.sym.Convolution(data=data, num_filter=width, kernel=(3, 3), stride=(2, 2), pad=(1, 1), no_bias=True,
                              name="conv0")
    body = graphs._int8_unit(body, width, width, (1, 1), False, "unit1", True, 0.9, qkw)
    body = graphs._relu(graphs._bn(body, "bn1"), "relu1")
    pool = mx.sym.Pooling(data=body, global_pool=True, kernel=(7, 7), pool_type="avg", name="pool1")
    fc = graphs.quant_fc("fc1", mx.sym.Flatten(data=pool), num_classes, width, **qkw)
    return mx.sym.SoftmaxOutput(data=fc, name="softmax")


def init_net(sym, data_shape, seed=0, weight_scale=1.0):
    """Deterministic fp32 values for every argument of `sym` but data / label (He-normal weights, BatchNorm gammas
    near 1 and betas near 0, a variable with an `__init__` attribute from it) and for every auxiliary state that
    has an `__init__` attribute -- the alphas. Returns (params, aux)."""
    rng = np.random.RandomState(seed)
    arg_shapes, _, aux_shapes = sym.infer_shape(data=data_shape, softmax_label=(data_shape[0],))
    attrs = sym.attr_dict()
    params, aux = {}, {}
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
    for name, shp in zip(sym.list_auxiliary_states(), aux_shapes):
        init = attrs.get(name, {}).get("__init__")
        if init:
            aux[name] = np.full(shp, json.loads(init)[1]["value"], dtype=np.float32)
    return params, aux


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


def _is_gdrq(node):
    return node["op"] == "_contrib_GDRQ" or (node["op"] == "Custom" and node["attrs"].get("op_type") == "GDRQ_PY")


def torch_step(sym, params, aux, data, label, dtype=torch.float64, replay=None, lr=0.1, wd=1e-4, momentum=0.9):
    """One forward / backward / SGD step of `sym` (read from its JSON) in torch at `dtype`, with MXNet's semantics:
    training-mode BatchNorm (biased variance), SoftmaxOutput's p - onehot gradient, GDRQ (unless fix_alpha the
    threshold moves first: alpha = ktimes * mean|w| for a weight, alpha += lamda * (alpha - ktimes * mean|x|) for an
    activation; then out = round_half_away(clip(x, -alpha, alpha) / unit) * unit with unit = alpha / (2^nbits - 1);
    straight-through for weights, dy * [|x| <= alpha] for activations), and the FIRST SGD step (the momentum buffer
    starts at zero, so `momentum` does not enter): w -= lr * (g / batch + wd * w), wd for *_weight / *_gamma and 0
    otherwise. aux: the alphas before the step, by name.

    replay = {"relu": {Activation name: bool mask}, "gdrq": {alpha name: {"codes": .., "mask": ..}}} substitutes a
    device's discrete decisions -- the thresholds stay this run's own, they are continuous --; whatever is missing
    runs free. Returns prob, grads, args (after the update), alphas (after the forward) and the decisions this run
    made itself."""
    replay = replay or {}
    tt = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)  # noqa: E731
    leaves = {k: tt(v).clone().requires_grad_(True) for k, v in params.items()}
    alphas = {k: tt(v).reshape(()).clone() for k, v in aux.items()}
    made = {"relu": {}, "gdrq": {}}
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
        elif _is_gdrq(node):
            x = ins[0]
            aname = graph["nodes"][node["inputs"][1][0]]["name"]
            is_weight = bool(_lit(a.get("is_weight"), False))
            levels = float(2 ** int(_lit(a.get("nbits"), 4)) - 1)
            if not _lit(a.get("fix_alpha"), False):
                thr = float(_lit(a.get("ktimes"), 3)) * x.detach().abs().mean()
                al = alphas[aname]
                alphas[aname] = thr if is_weight else al + float(_lit(a.get("lamda"), 0.001)) * (al - thr)
            al = alphas[aname]
            unit = al / levels
            r = replay.get("gdrq", {}).get(aname)
            if r is None:
                keep = torch.ones_like(x, dtype=torch.bool) if is_weight else x.detach().abs() <= al
                q = _round_half_away(torch.minimum(torch.maximum(x.detach(), -al), al) / unit) if unit > 0 else \
                    torch.zeros_like(x.detach())
            else:
                keep = torch.as_tensor(np.asarray(r["mask"]), dtype=torch.bool).reshape(x.shape)
                q = tt(r["codes"]).reshape(x.shape)
            made["gdrq"][aname] = {"codes": q, "mask": keep}
            xm = x * keep.to(dtype)
            out = (q * unit).detach() + (xm - xm.detach())  # (exactly the value; the gradient is the mask's)
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
    return {"prob": prob.numpy().copy(), "grads": grads, "args": args,
            "alphas": {k: float(v) for k, v in alphas.items()}, "decisions": made}


# ----------------------------------------------------------------------------- the step through the Module
def _nchw(t, buf):
    a = buf.float().cpu().numpy()
    if t.h == 1 and t.w == 1 and len(t.shape) == 2:
        return a.reshape(t.n, t.cp)[:, :t.c]
    return a.reshape(t.n, t.h, t.w, t.cp)[..., :t.c].transpose(0, 3, 1, 2)


def device_decisions(ex):
    """The discrete decisions of the executor's last forward, in torch_step's replay format, with the alpha and the
    unit each GDRQ used. The GPU executor's are read back from its buffers: an activation's codes from its int8 code
    buffer where it emits one, else from its values (code * unit: the quotient rounds back to the integer), its
    mask from its stored input and the alpha the forward left; a weight's codes from its fake-quantized copy."""
    if type(ex).__name__ == "CPUExecutor":
        d = ex.decisions
        return {"relu": {k: v.numpy() for k, v in d["relu"].items()},
                "gdrq": {k: {"codes": v["codes"].numpy().astype(np.float64), "mask": v["mask"].numpy(),
                             "alpha": v["alpha"], "unit": v["unit"]} for k, v in d["gdrq"].items()}}
    from step_util import gpu_quant_values, gpu_relu_masks
    out = {"relu": gpu_relu_masks(ex), "gdrq": {}}
    qv = gpu_quant_values(ex)
    for op in ex.plan.ops:
        q = getattr(op, "qweight", None)
        if q is not None and q.get("family") == "gdrq":
            alpha = np.float32(ex.get_aux(q["alpha"])[0])
            unit = np.float32(alpha / np.float32(2 ** q["nbits"] - 1))
            v = qv[q["name"]].astype(np.float64)
            if len(ex.param_shape[op.weight]) == 2:
                v = v.reshape(ex.param_shape[op.weight])
            out["gdrq"][q["alpha"]] = {"codes": np.rint(v / float(unit)), "mask": np.ones(v.shape, dtype=bool),
                                       "alpha": float(alpha), "unit": float(unit), "values": v,
                                       "x": ex.get_param(op.weight)}
        if op.kind != "gdrq":
            continue
        alpha = np.float32(ex.get_aux(op.alpha)[0])
        unit = float(op.unit.cpu().numpy()[0])
        x = _nchw(op.x, ex.act(op.x)).astype(np.float32)
        vals = _nchw(op.y, ex.act(op.y)).astype(np.float64)
        codes = _nchw(op.x, op.codes).astype(np.float64) if op.codes is not None else np.rint(vals / unit)
        out["gdrq"][op.alpha] = {"codes": codes, "mask": np.abs(x) <= alpha, "alpha": float(alpha), "unit": unit,
                                 "values": vals, "x": x}
    return out


def module_step(sym, params, aux, data, label, ctx, steps=1, lr=0.1, wd=1e-4, momentum=0.9, precision="float32"):
    """bind / init / forward / backward / update (core/solver.py:75-121); per step the probabilities, the decisions,
    the gradients, the parameters after the update and every auxiliary state after the step. aux_params=None: the
    alphas come from their variables' own `__init__` (they must equal `aux`, which is asserted)."""
    kw = {} if ctx.device_type == "cpu" else {"precision": precision}
    mod = mx.mod.Module(sym, context=[ctx], **kw)
    mod.bind(data_shapes=[("data", data.shape)], label_shapes=[("softmax_label", label.shape)], for_training=True)
    mod.init_params(arg_params={k: v for k, v in params.items()}, aux_params=None, allow_missing=False)
    got = mod.get_params()[1]
    # (a weight's alpha is a function of the weight: the GPU executor's first repack has already recomputed it)
    assert all(np.array_equal(got[k].asnumpy(), v) for k, v in aux.items() if k.endswith("_data_alpha")), \
        "alphas do not start at their __init__"
    mod.init_optimizer(kvstore="local", optimizer="sgd",
                       optimizer_params={"learning_rate": lr, "wd": wd, "momentum": momentum})
    b = mx.io.DataBatch(data=[mx.nd.array(data)], label=[mx.nd.array(label)])
    ex = mod.executor
    out = {"prob": [], "decisions": [], "grads": [], "args": [], "aux": [], "mod": mod}
    for _ in range(steps):
        mod.forward(b, is_train=True)
        out["prob"].append(mod.get_outputs()[0].asnumpy().copy())
        out["decisions"].append(device_decisions(ex))
        mod.backward()
        out["grads"].append({n: ex.get_param(n, grad=True) for n in ex.plan.param_names})
        mod.update()
        arg, auxp = mod.get_params()
        out["args"].append({k: v.asnumpy() for k, v in arg.items()})
        out["aux"].append({k: v.asnumpy() for k, v in auxp.items()})
    return out


def fro_rel(a, b):
    a = np.asarray(a, np.float64).ravel()
    b = np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-12))


def code_mismatch(dec, free):
    """{alpha name: (fraction of elements whose code differs, largest difference)} of a run's GDRQ decisions
    against a free-running torch_step's."""
    out = {}
    for aname, d in dec["gdrq"].items():
        diff = np.abs(np.asarray(d["codes"], np.float64).ravel() -
                      free["decisions"]["gdrq"][aname]["codes"].numpy().ravel())
        out[aname] = (float((diff != 0).mean()), float(diff.max()))
    return out


def check_step(res, sym, params, aux, data, label, step=0, base_tol=1e-4, factor=4.0, code_cap=0.01, **hyper):
    """The bar of step_util.replayed_parity for the first Module step `res` (module_step): against the fp64
    torch_step replaying the run's own decisions -- probabilities within base_tol of the largest one; every
    gradient, every updated parameter and every alpha the forward used within max(base_tol, factor x the error the
    same replayed step makes in fp32), Frobenius-relative. And the condition under which that comparison means
    something: against the FREE-running fp64 step the run's GDRQ codes -- weights' included -- differ on at most
    `code_cap` of a node's elements and by at most one code. Returns the figures; raises AssertionError with the
    worst offenders."""
    assert step == 0, "torch_step is the first SGD step"
    dec = res["decisions"][step]
    ref = torch_step(sym, params, aux, data, label, torch.float64, replay=dec, **hyper)
    r32 = torch_step(sym, params, aux, data, label, torch.float32, replay=dec, **hyper)
    free = torch_step(sym, params, aux, data, label, torch.float64, **hyper)
    figs = {"prob": float(np.abs(res["prob"][step] - ref["prob"]).max() / np.abs(ref["prob"]).max()),
            "codes": code_mismatch(dec, free), "grads": {}, "args": {}, "alphas": {}}
    for kind in ("grads", "args"):
        for n, v in ref[kind].items():
            e32 = fro_rel(r32[kind][n], v)
            figs[kind][n] = (fro_rel(res[kind][step][n], v), e32, max(base_tol, factor * e32))
    for n, v in ref["alphas"].items():
        e32 = fro_rel(r32["alphas"][n], v)
        figs["alphas"][n] = (fro_rel(dec["gdrq"][n]["alpha"], v), e32, max(base_tol, factor * e32))
    print("prob %.2e; worst code mismatch %s; worst grad %s; worst arg %s; worst alpha %s" % (
        figs["prob"], max(figs["codes"].values()), max(figs["grads"].items(), key=lambda kv: kv[1][0] / kv[1][2]),
        max(figs["args"].items(), key=lambda kv: kv[1][0] / kv[1][2]),
        max(figs["alphas"].items(), key=lambda kv: kv[1][0] / kv[1][2])))
    bad_codes = {k: v for k, v in figs["codes"].items() if v[0] > code_cap or v[1] > 1}
    assert not bad_codes, bad_codes
    assert figs["prob"] < base_tol, figs["prob"]
    for kind in ("grads", "args", "alphas"):
        bad = {k: v for k, v in figs[kind].items() if v[0] > v[2]}
        assert not bad, (kind, bad)
    return figs
