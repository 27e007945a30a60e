"""QIL test helpers: restatements of the kernels, of a small QIL network in fp64, and the reference's QIL graph
surface driven through the `mxnet` shim's public API.

  qil_coef_ref / qil_fwd_ref / qil_bwd_ref   numpy float32 restatements of rn_qil_fwd / rn_qil_bwd in the kernels'
                                operation order (include/rn.h), bit for bit; the two sums in fp64
  qil_fp64                      core/operator/QIL.py:50-85,117-124 (the "ste" branch) restated in torch fp64: the
                                forward as written there, the backward by autograd
  edge_inputs                   the kernels' edge inputs: |x| == p, |x| == c, |x| > c (both signs), |x| < p, zeros,
                                +-0.5
  qil_bwd_chain                 the longest chain of fp32 additions on the way to dp[0] / dc[0] at a given n
  sgd_lrm_ref                   rn_sgd_mom_update*_lrm restated in float32
  create_quant_node / attach_quantize_node / qil_settings
                                core/graph_optimize.py:159-292 for quantize_op_name "QIL"
  qil_unit_net                  stem conv + one pre-activation bottleneck unit with a projection shortcut + head
  torch_step / module_step / device_decisions / check_step
                                one training step in torch (fp64 or fp32) replaying a device's discrete decisions
                                (ReLU masks, QIL codes and interval flags of weights and activations), and the same
                                step through mx.mod.Module
"""
import json

import numpy as np
import torch
import torch.nn.functional as F

import mxnet as mx
import pact_util as PU
from pact_util import _lit, _nchw, batch, bf16, fro_rel, get_constant, init_net  # noqa: F401  (re-exported)
from rn import graphs

f32 = np.float32


# ----------------------------------------------------------------------------- the kernels, restated
def qil_coef_ref(p, c):
    """(p, c, alpha, beta) after the clamp, every operation rounded to float32 on its own, in the order of
    include/rn.h: center = 0.5 (c + p); distance = 0.5 (c - p); alpha = 0.5 / distance;
    beta = (-0.5 center) / distance + 0.5."""
    p, c = f32(p), f32(c)
    p = f32(0) if p < 0 else p
    c = f32(1) if c > 1 else c
    center = f32(f32(0.5) * f32(c + p))
    distance = f32(f32(0.5) * f32(c - p))
    alpha = f32(f32(0.5) / distance)
    beta = f32(f32(f32(f32(-0.5) * center) / distance) + f32(0.5))
    return p, c, alpha, beta


def _sign(x):
    return (x > 0).astype(np.float32) - (x < 0).astype(np.float32)


def _roundf(r):
    """roundf on a float32 array: half away from zero, the sign of a zero kept. |r| - trunc(|r|) is exact."""
    a = np.abs(r)
    t = np.trunc(a)
    return np.copysign((t + (a - t >= f32(0.5))).astype(np.float32), r)


def qil_fwd_ref(x, p, c, nbits, to_bf16=False):
    """(values, codes, unit, p after the clamp, c after the clamp) in numpy float32: a = |x|, s = sign(x),
    t = s * (1 where a > c, alpha * a + beta where p <= a <= c, else 0), q = roundf(t * L), value = q / L."""
    x = np.asarray(x, dtype=np.float32)
    levels = f32(2 ** nbits - 1)
    p, c, alpha, beta = qil_coef_ref(p, c)
    a = np.abs(x)
    s = _sign(x)
    lin = ((alpha * a).astype(np.float32) + beta).astype(np.float32)
    flag = (a >= p) & (a <= c)
    m = np.where(a > c, f32(1), np.where(flag, lin, f32(0))).astype(np.float32)
    t = (s * m).astype(np.float32)
    q = _roundf((t * levels).astype(np.float32))
    v = (q / levels).astype(np.float32)
    return (bf16(v) if to_bf16 else v), q, f32(f32(1) / levels), p, c


def qil_bwd_ref(x, dy, p, c, add=None, to_bf16=False):
    """(dx, dp in fp64, dc in fp64, sum |dp terms| in fp64, sum |dc terms| in fp64). dx = dy * alpha where
    p <= |x| <= c and x != 0, else 0 (+ add, the add in fp32, then rounded to the storage type), alpha the float32
    coefficient; the sums exactly as QIL.py's autograd gives them, from the float32 inputs in fp64:
    dp = sum flag dy s (a - c) / (c - p)^2, dc = -sum flag dy s (a - p) / (c - p)^2."""
    x = np.asarray(x, dtype=np.float32)
    dy = np.asarray(dy, dtype=np.float32)
    p, c, alpha, _ = qil_coef_ref(p, c)
    a = np.abs(x)
    flag = (a >= p) & (a <= c)
    dx = np.where(flag & (x != 0), (dy * alpha).astype(np.float32), f32(0)).astype(np.float32)
    if add is not None:
        dx = (dx + np.asarray(add, dtype=np.float32)).astype(np.float32)
    d2 = (float(c) - float(p)) ** 2
    ds = dy.astype(np.float64) * _sign(x).astype(np.float64) * flag
    tp = ds * (a.astype(np.float64) - float(c)) / d2
    tc = -ds * (a.astype(np.float64) - float(p)) / d2
    return (bf16(dx) if to_bf16 else dx), float(tp.sum()), float(tc.sum()), float(np.abs(tp).sum()), \
        float(np.abs(tc).sum())


def qil_fp64(x, p, c, nbits, dy=None):
    """core/operator/QIL.py:50-85 in torch fp64, as written there (after the in-place clamp): the output, and with
    dy the autograd gradients (dx, dp, dc) of QIL.py:117-124 -- the rounding is outside the recorded region, so
    the gradient is the transform's."""
    dt = torch.float64
    xt = torch.as_tensor(np.asarray(x, dtype=np.float64), dtype=dt).clone().requires_grad_(True)
    pt = torch.tensor([min(max(float(p), 0.0), np.inf)], dtype=dt, requires_grad=True)
    ct = torch.tensor([min(float(c), 1.0)], dtype=dt, requires_grad=True)
    levels = float(2 ** nbits - 1)
    center = 0.5 * (ct + pt)
    distance = 0.5 * (ct - pt)
    alpha = 0.5 / distance
    beta = -0.5 * center / distance + 0.5
    a = xt.abs()
    s = torch.sign(xt)
    flag = ((a >= pt) * (a <= ct)).to(dt)
    out = s * (a > ct).to(dt) + s * (alpha * a + beta) * flag
    r = out.detach() * levels
    q = torch.trunc(r) + torch.sign(r) * ((r - torch.trunc(r)).abs() >= 0.5).to(dt)  # mx.nd.round: half away
    res = {"out": (q / levels).numpy(), "codes": q.numpy()}
    if dy is not None:
        out.backward(torch.as_tensor(np.asarray(dy, dtype=np.float64), dtype=dt))
        res.update(dx=xt.grad.numpy(), dp=float(pt.grad[0]), dc=float(ct.grad[0]))
    return res


def edge_inputs(n, to_bf16, p, c, seed):
    """|x| == p, |x| == c and |x| > c of both signs, |x| < p (where p > 0), zeros of both signs, +-0.5, and a
    spread over [-1.4, 1.4] around them; rounded to the storage type first (p, c and 0.5 must be representable in
    it), so that the restatement sees what the device reads. n >= 16."""
    rng = np.random.RandomState(seed)
    x = (rng.rand(n) * 2.8 - 1.4).astype(np.float32)
    for v in (p, c):
        i = rng.randint(0, n, size=max(n // 16, 2))
        x[i] = np.where(rng.rand(i.size) < 0.5, v, -v)
    x[rng.randint(0, n, size=max(n // 16, 1))] = 0.0
    x[:14] = [p, -p, c, -c, 1.25, -1.25, p / 2, -p / 2, 0.0, -0.0, 0.5, -0.5, (p + c) / 2, -(p + c) / 2]
    x = x.astype(np.float32)
    return bf16(x) if to_bf16 else x


def qil_bwd_chain(n, itemsize):
    """The longest chain of fp32 additions on the way to rn_qil_bwd's dp[0] / dc[0], from its launch geometry
    (include/rn.h, csrc/rn_misc.hip qil_bwd_kernel / qil_dpc_kernel) -- rn_pact_bwd's: min(max(ceil(n / 2048), 1),
    2048) blocks of 256 threads; a thread adds the 16 / itemsize elements of each of its 16-byte chunks one after
    the other, over ceil(chunks / threads) grid-stride rounds, plus at most one tail element; 6 butterfly stages
    across the 64 lanes of a wave; 2 stages for the block's 4 waves; then the second launch: a lane adds 32
    consecutive partials one after the other (fewer where there are fewer), and the ceil(blocks / 32) lane sums
    that are not zero are added one after the other."""
    return PU.pact_bwd_chain(n, itemsize)


# fp32 roundings of one term of dp / dc and of the scale, counted from qil_bwd_elem / qil_dpc_kernel: dy * s is
# exact; a - c (or a - p) 1; the product 1; d = c - p enters squared: 2; d * d 1; the division 1
QIL_TERM_ROUNDINGS = 6


def sgd_lrm_ref(w, g, mom, wds, lrms, lr, momentum, rescale, clip=-1.0):
    """rn_sgd_mom_update*_lrm on lists of float32 arrays, in float32 with the kernel's operations: lr_eff =
    lr * lr_mult (one product); gr = rescale * g (clipped); mom = momentum * mom - lr_eff * (gr + wd * w), contracted
    as the kernels' code has it: inner = fma(wd, w, gr), t = lr_eff * inner, mom = fma(momentum, mom, -t) -- the
    fused operations here in fp64 and rounded once (a float32 product is exact in fp64); w += mom. Returns (w, mom)
    lists."""
    ws, ms = [], []
    for wt, gt, mt, wd, lm in zip(w, g, mom, wds, lrms):
        lre = f32(f32(lr) * f32(lm)) if lm is not None else f32(lr)
        gr = (f32(rescale) * gt).astype(np.float32)
        if clip > 0:
            gr = np.clip(gr, f32(-clip), f32(clip))
        inner = (gr.astype(np.float64) + np.float64(f32(wd)) * wt.astype(np.float64)).astype(np.float32)  # fma
        t = (lre * inner).astype(np.float32)
        mv = (np.float64(f32(momentum)) * mt.astype(np.float64) - t.astype(np.float64)).astype(np.float32)  # fma
        ms.append(mv)
        ws.append((wt + mv).astype(np.float32))
    return ws, ms


# ----------------------------------------------------------------------------- the reference's graph surface
def create_quant_node(var, setting):
    """core/graph_optimize.py:159-175 for quantize_op_name "QIL" (and "Quantization_int8")."""
    name, attrs = setting["quantize_op_name"], setting.get("attrs", {})
    if name == "Quantization_int8":
        return PU.create_quant_node(var, setting)
    assert name == "QIL", name
    init_value = setting.get("init_value") or 1.0
    pruning_var = mx.sym.var(name=var.name + "_pruning_point", init=get_constant(0), lr_mult=0.01, wd_mult=0)
    clipping_var = mx.sym.var(name=var.name + "_clipping_point", init=get_constant(init_value), lr_mult=0.01,
                              wd_mult=0)
    gamma_var = mx.sym.var(name=var.name + "_gamma", init=mx.init.Constant(1.0))
    return mx.sym.Custom(name=var.name, data=var, pruning_point=pruning_var, clipping_point=clipping_var,
                         gamma=gamma_var, **attrs, op_type="QIL_PY")


def attach_quantize_node(symbol, out_shape_dict, weight_setting, act_setting,
                         quantized_op=("Convolution", "FullyConnected", "Deconvolution"), skip_quantize_counts=None):
    """core/graph_optimize.py:199-292 (one quantizer per quantized tensor, whoever reads it)."""
    from graph_passes import _rebuild
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


def qil_settings(wbits=4, abits=4, init_value=None):
    """(weight_setting, act_setting) of a config-style QIL run (config/quant_attrs.py's attribute strings)."""
    w = {"quantize_op_name": "QIL", "init_value": init_value,
         "attrs": {"is_weight": "True", "fix_gamma": "True", "nbits": str(wbits)}}
    a = {"quantize_op_name": "QIL", "init_value": init_value,
         "attrs": {"is_weight": "False", "fix_gamma": "True", "nbits": str(abits)}}
    return w, a


# ----------------------------------------------------------------------------- the small network
def qil_unit_net(num_classes=8, abits=4, wbits=4, qil_init=1.0, width=256):
    """pact_util.pact_unit_net with QIL quantizers on every weight and activation of the unit and the fc: stem conv
    (3x3 / stride 2, unquantized) -> one pre-activation bottleneck unit width -> width/4 -> width/4 -> width with a
    projection shortcut -> BN + ReLU -> global average pool -> quantized fc -> softmax."""
    qkw = dict(act_op="QIL", weight_op="QIL", abits=abits, wbits=wbits, qil_init=qil_init)
    data = mx.sym.Variable(name="data")
    body = mx.sym.Convolution(data=data, num_filter=width, kernel=(3, 3), stride=(2, 2), pad=(1, 1), no_bias=True,
                              name="conv0")
    body = graphs._int8_unit(body, width, width, (1, 1), False, "unit1", True, 0.9, qkw)
    body = graphs._relu(graphs._bn(body, "bn1"), "relu1")
    pool = mx.sym.Pooling(data=body, global_pool=True, kernel=(7, 7), pool_type="avg", name="pool1")
    fc = graphs.quant_fc("fc1", mx.sym.Flatten(data=pool), num_classes, width, **qkw)
    return mx.sym.SoftmaxOutput(data=fc, name="softmax")


def init_qil_net(sym, data_shape, seed=0, weight_scale=4.0, prune=0.05, clip=0.6):
    """pact_util.init_net, the He-normal weights scaled so that the quantized weights (|w| mapped onto [0, 1]
    between the points) spread over the codes, every pruning point at `prune` and clipping point at `clip`: both
    sums of every quantizer's backward then have terms, and elements fall below, inside and above the interval."""
    params = init_net(sym, data_shape, seed=seed, weight_scale=weight_scale)
    for k in params:
        if k.endswith("_pruning_point"):
            params[k][:] = prune
        elif k.endswith("_clipping_point"):
            params[k][:] = clip
    return params


# ----------------------------------------------------------------------------- the step in torch
def _round_half_away(a):
    t = torch.trunc(a)
    return t + torch.sign(a) * ((a - t).abs() >= 0.5).to(a.dtype)


def multipliers(sym, names):
    """MXNet's set_lr_mult / set_wd_mult, restated: {name: (lr_mult, wd_mult)}."""
    attrs = sym.attr_dict()
    out = {}
    for n in names:
        a = attrs.get(n, {})
        wm = 1.0 if (n.endswith("_weight") or n.endswith("_gamma")) else 0.0
        out[n] = (float(a.get("__lr_mult__", 1.0)), float(a.get("__wd_mult__", wm)))
    return out


def torch_step(sym, params, data, label, dtype=torch.float64, replay=None, lr=0.1, wd=1e-4, momentum=0.9):
    """pact_util.torch_step for graphs with QIL quantizers (weights and activations): one forward / backward / first
    SGD step of `sym` in torch at `dtype` with MXNet's semantics. A QIL node is core/operator/QIL.py:50-85 as written
    (after the clamp): t = s [a > c] + s (alpha a + beta) [p <= a <= c] under autograd, out = round(t L) / L outside
    it. The update honours the variables' lr_mult / wd_mult: w -= lr lr_mult (g / batch + wd wd_mult w).

    replay = {"relu": {name: mask}, "qil": {pruning-point name: {"codes", "flag", "above"}}} substitutes a device's
    discrete decisions; whatever is missing runs free. Returns prob, grads, args and the run's own decisions."""
    replay = replay or {}
    tt = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)  # noqa: E731
    start = {k: np.array(v, dtype=np.float64) for k, v in params.items()}
    for k in start:  # the forward's in-place clamp
        if k.endswith("_pruning_point"):
            start[k] = np.maximum(start[k], 0.0)
        elif k.endswith("_clipping_point"):
            start[k] = np.minimum(start[k], 1.0)
    leaves = {k: tt(v).clone().requires_grad_(True) for k, v in start.items()}
    made = {"relu": {}, "qil": {}}
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
        elif op == "Custom" and a.get("op_type") == "QIL_PY":
            x, p, c = ins[0], ins[1], ins[2]
            pname = graph["nodes"][node["inputs"][1][0]]["name"]
            levels = float(2 ** int(_lit(a.get("nbits"), 4)) - 1)
            center = 0.5 * (c + p)
            distance = 0.5 * (c - p)
            alpha = 0.5 / distance
            beta = -0.5 * center / distance + 0.5
            ax, s = x.abs(), torch.sign(x)
            r = replay.get("qil", {}).get(pname)
            if r is None:
                flag = (ax.detach() >= p.detach()) & (ax.detach() <= c.detach())
                above = ax.detach() > c.detach()
            else:
                flag = torch.as_tensor(np.asarray(r["flag"]), dtype=torch.bool).reshape(x.shape)
                above = torch.as_tensor(np.asarray(r["above"]), dtype=torch.bool).reshape(x.shape)
            t = s * above.to(dtype) + s * (alpha * ax + beta) * flag.to(dtype)
            q = _round_half_away(t.detach() * levels) if r is None else tt(r["codes"]).reshape(x.shape)
            made["qil"][pname] = {"codes": q, "flag": flag, "above": above}
            out = t + (q / levels - t).detach()
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
    mult = multipliers(sym, list(leaves))
    grads, args = {}, {}
    for k, p in leaves.items():
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        grads[k] = g.numpy().copy()
        lm, wm = mult[k]
        args[k] = (p.detach() - lr * lm * (g / nb + wd * wm * p.detach())).numpy().copy()
    return {"prob": prob.numpy().copy(), "grads": grads, "args": args, "decisions": made}


# ----------------------------------------------------------------------------- the step through the Module
def _wshape(ex, name, flat):
    """A master-layout (KRSC / plain) flat array of parameter `name` in MXNet's layout."""
    shp = ex.param_shape[name]
    if getattr(ex, "param_layout", {}).get(name) == "krsc":
        k, c, r, s = shp
        return flat.reshape(k, r, s, c).transpose(0, 3, 1, 2)
    return flat.reshape(shp)


def device_decisions(ex):
    """The discrete decisions of the executor's last forward, in torch_step's replay format. The GPU executor's are
    read back from its buffers: an activation QIL's codes from its int8 code buffer where it emits one, else from
    its values (value * L rounds back to the integer); a weight QIL's from its fake-quantized copy; the flags and
    |x| > c masks from the stored input and the points the forward left (clamped) in the master buffer."""
    if type(ex).__name__ == "CPUExecutor":
        d = ex.decisions
        return {"relu": {k: v.numpy() for k, v in d["relu"].items()},
                "qil": {k: {"codes": v["codes"].numpy(), "flag": v["flag"].numpy(), "above": v["above"].numpy()}
                        for k, v in d["qil"].items()}}
    from step_util import gpu_relu_masks
    out = {"relu": gpu_relu_masks(ex), "qil": {}}

    def entry(x, codes, pn, cn):
        p, c = f32(ex.get_param(pn)[0]), f32(ex.get_param(cn)[0])
        a = np.abs(x.astype(np.float32))
        return {"codes": codes, "flag": (a >= p) & (a <= c), "above": a > c, "p": float(p), "c": float(c)}
    for op in ex.plan.ops:
        q = op.qweight
        if q and q.get("family") == "qil":
            levels = float(2 ** q["nbits"] - 1)
            w = _wshape(ex, op.weight, ex.pview(op.weight).cpu().numpy())
            codes = np.rint(_wshape(ex, op.weight, op.qw.cpu().numpy()).astype(np.float64) * levels)
            out["qil"][q["prune"]] = entry(w, codes, q["prune"], q["clip"])
        if op.kind != "qil":
            continue
        levels = float(2 ** op.nbits - 1)
        x = _nchw(ex, op.x, ex.act(op.x)).astype(np.float32)
        if op.codes is not None:
            codes = _nchw(ex, op.x, op.codes).astype(np.float64)
        else:
            codes = np.rint(_nchw(ex, op.y, ex.act(op.y)).astype(np.float64) * levels)
        out["qil"][op.prune] = entry(x, codes, op.prune, op.clip)
        out["qil"][op.prune]["values"] = _nchw(ex, op.y, ex.act(op.y)).astype(np.float64)
    return out


def module_step(sym, params, data, label, ctx, steps=1, lr=0.1, wd=1e-4, momentum=0.9, precision="float32"):
    """pact_util.module_step with QIL's decisions."""
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


def check_step(res, sym, params, data, label, step=0, base_tol=1e-4, factor=4.0, code_cap=0.01, **hyper):
    """pact_util.check_step's bar, with its tolerances, for a QIL step: against the fp64 torch_step replaying the
    run's own decisions -- probabilities within base_tol of the largest one; every gradient and every updated
    parameter within max(base_tol, factor x the error the same replayed step makes in fp32), Frobenius-relative (a
    gradient that is zero in fp64 -- gamma's -- must be zero). And the condition under which that comparison means
    something: against the FREE-running fp64 step the run's QIL codes differ on at most `code_cap` of a node's
    elements and by at most one code. Returns the figures."""
    dec = res["decisions"][step]
    ref = torch_step(sym, params, data, label, torch.float64, replay=dec, **hyper)
    r32 = torch_step(sym, params, data, label, torch.float32, replay=dec, **hyper)
    free = torch_step(sym, params, data, label, torch.float64, **hyper)
    figs = {"prob": float(np.abs(res["prob"][step] - ref["prob"]).max() / np.abs(ref["prob"]).max()), "codes": {},
            "grads": {}, "args": {}}
    for pname, d in dec["qil"].items():
        diff = np.abs(np.asarray(d["codes"], np.float64).ravel() -
                      free["decisions"]["qil"][pname]["codes"].numpy().ravel())
        figs["codes"][pname] = (float((diff != 0).mean()), float(diff.max()))
    for kind in ("grads", "args"):
        for n, v in ref[kind].items():
            if not np.any(v):
                assert not np.any(res[kind][step][n]), (kind, n)
                continue
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
