"""Lower an mx.sym graph to a fused op list at fixed input shapes: the GPU-free half of the runtime.

`Plan` is pure Python and runs without a GPU (it is what the CPU tests check): shape inference, the fusions that
only the graph decides (residual adds into convolutions, BatchNorm+ReLU applied by its consumers, the int8 forward)
and one `PlanOp` per kernel-level operation. rn/executor.py binds the ops to device buffers and librn calls.
"""
import os

import numpy as np

from . import lib as L

F32, BF16 = L.RN_F32, L.RN_BF16


def _pad8(c):
    return (c + 7) // 8 * 8


def _parse(v, default=None):
    from mxnet.symbol import _parse as p  # the shim's attr parser
    return p(v) if v is not None else default


def _tup(v, n=2):
    from mxnet.symbol import _tup as t
    return t(v, n)


class PlanError(RuntimeError):
    pass


def multipliers(symbol, param_names):
    """(lr_mult, wd_mult) as MXNet's Optimizer.set_lr_mult / set_wd_mult fill them from a symbol ({parameter name:
    factor}; a name without an entry: 1): lr_mult from the variables' __lr_mult__; wd_mult 0 for every name that
    ends in neither _weight nor _gamma, then the variables' __wd_mult__ over that."""
    attrs = symbol.attr_dict()
    lr_mult, wd_mult = {}, {}
    for n in param_names:
        if not (n.endswith("_weight") or n.endswith("_gamma")):
            wd_mult[n] = 0.0
        a = attrs.get(n, {})
        if "__lr_mult__" in a:
            lr_mult[n] = float(a["__lr_mult__"])
        if "__wd_mult__" in a:
            wd_mult[n] = float(a["__wd_mult__"])
    return lr_mult, wd_mult


# ============================================================================= plan (CPU)
class TensorSpec:
    """An activation tensor: logical NCHW (or (N,F)) shape -> NHWC buffer with padded C."""

    def __init__(self, name, shape, dtype, needs_grad=True, kind="act"):
        self.name = name
        self.shape = tuple(shape)
        if len(shape) == 4:
            self.n, self.c, self.h, self.w = shape
        elif len(shape) == 2:
            self.n, self.c = shape
            self.h = self.w = 1
        else:
            raise PlanError("unsupported activation rank for %s: %s" % (name, shape))
        self.cp = _pad8(self.c)
        self.dtype = dtype
        self.needs_grad = needs_grad
        self.kind = kind  # act | logits | prob | data_nchw | label

    @property
    def rows(self):
        return self.n * self.h * self.w

    @property
    def numel(self):
        if self.kind in ("data_nchw", "prob", "label"):
            return int(np.prod(self.shape))
        return self.rows * self.cp


class PlanOp:
    """One kernel-level operation. Its attributes are the lowering's keyword arguments plus what later passes of the
    plan and the executor's binders stamp on it. The optional ones default here, so that readers use plain attribute
    access (class-level: they do not appear in vars(op))."""
    groups = 1           # Plan._lower_conv: the convolution's num_group
    qweight = None       # Plan._lower_conv / _lower_fc: the weight quantizer's record (Plan._weight_quant)
    xf = None            # Plan._fuse_bn_apply: the BatchNorm+ReLU this conv / pooling applies while loading
    apply_fused = False  # Plan._fuse_bn_apply / _fuse_bn_add: a BatchNorm applied by its consumers, y never written
    bn_a = None          # Plan._fuse_bn_add: the BatchNorm applied inside this add (bn_a_key: on which operand)
    bn_b = None          # Plan._fuse_bn_add: the second one, when both operands are BatchNorm outputs
    int8 = False         # Plan._mark_int8: the conv's forward runs on the int8 MFMAs
    qsrc = None          # Plan._mark_int8: the quantizer op whose codes an int8 conv reads
    value_users = None   # Plan._mark_int8: the ops that read a Quantization_int8 op's values
    desc = None          # Executor._describe_ops (bn) / the op's forward binder: its ctypes descriptor
    part_src = None      # Executor._mark_bn_stats: the conv / stem whose epilogue writes this BatchNorm's statistics
    part = None          # Executor._conv_fwd_call / _fwd_stem: the buffer of those statistics' block partials
    part_mm = None       # Executor._conv_fwd_call: per-block extremes of an int8 conv's output (want_mm)
    codes = None         # Executor._fwd_quant / _fwd_pact / _fwd_gdrq / _fwd_qil: the int8 codes a quantizer emits
    unit = None          # Executor._fwd_quant / _fwd_pact / _fwd_gdrq / _fwd_qil: the codes' unit (one fp32 value)
    pre_part = None      # Executor._bwd_add: a BatchNorm's backward reduction done by the add's ReLU backward

    def __init__(self, kind, name, **kw):
        self.kind = kind
        self.name = name
        self.__dict__.update(kw)

    def __repr__(self):
        return "<%s %s>" % (self.kind, self.name)


class Plan:
    """Fused op list for a symbol at fixed input shapes."""

    def __init__(self, symbol, data_shapes, label_shapes=(), dtype="bfloat16", for_training=True):
        self.symbol = symbol
        self.dtype = BF16 if dtype in ("bfloat16", "bf16", BF16) else F32
        self.for_training = for_training
        self.data_names = [n for n, _ in data_shapes]
        self.label_names = [n for n, _ in label_shapes]
        known = dict(list(data_shapes) + list(label_shapes))
        self.input_shapes = known
        self.topo = symbol._topo()
        self._infer(known)
        self.arg_names = symbol.list_arguments()
        self.aux_names = symbol.list_auxiliary_states()
        self.param_names = [n for n in self.arg_names if n not in known]
        self.tensors = {}
        self.alias = {}
        self.ops = []
        self.qweight = {}  # id(weight Quantization_int8 node) -> quant info
        self.qweight_gdrq = {}  # id(weight GDRQ node) -> quant info (family "gdrq")
        self._gdrq_alphas = {}  # alpha variable -> the GDRQ node that owns it
        self.qweight_qil = {}  # id(weight QIL node) -> quant info (family "qil")
        self._qil_vars = {}  # pruning / clipping / gamma variable -> the QIL node that owns it
        self._lower()

    # --- shapes of every node output
    def _infer(self, known):
        from mxnet.symbol import _infer_node, _parse as parse
        shapes = {}
        for n in self.topo:
            if n.op == "null":
                if n.name in known:
                    shapes[(id(n), 0)] = tuple(known[n.name])
                elif "__shape__" in n.attrs:
                    shapes[(id(n), 0)] = tuple(parse(n.attrs["__shape__"]))
        for n in self.topo:
            if n.op != "null":
                _infer_node(n, shapes, False)
        self.shapes = shapes

    def shape_of(self, node, idx=0):
        return self.shapes[(id(node), idx)]

    def param_shape(self, name):
        for n in self.topo:
            if n.op == "null" and n.name == name:
                return self.shapes[(id(n), 0)]
        raise KeyError(name)

    # --- helpers
    def _consumers(self):
        cons = {}
        for n in self.topo:
            for (i, _) in n.inputs:
                cons.setdefault(id(i), []).append(n)
        for n, _ in self.symbol._outputs:
            cons.setdefault(id(n), []).append(None)  # graph output
        return cons

    def tensor(self, node):
        key = id(node)
        while key in self.alias:
            key = self.alias[key]
        return self.tensors[key]

    def _new_tensor(self, node, shape, dtype=None, kind="act", needs_grad=True):
        t = TensorSpec(node.name, shape, self.dtype if dtype is None else dtype, needs_grad, kind)
        self.tensors[id(node)] = t
        return t

    def _var_input(self, node):
        """Follow identity/Cast/Flatten aliases back; return (node, is_variable)."""
        while node.op in ("identity", "Cast", "Flatten"):
            node = node.inputs[0][0]
        return node

    @staticmethod
    def _is_quant(node):
        return node is not None and node.op == "_contrib_Quantization_int8"

    def _quant_info(self, n):
        """Quantization_int8 attrs (int8_api.py:133-136; semantics clip_grad_quantization_int8.py)."""
        if _parse(n.attrs.get("quant_mode", "minmax")) != "minmax":
            raise PlanError("%s: quant_mode other than 'minmax' not supported" % n.name)
        if int(_parse(n.attrs.get("delay_quant", 0))):
            raise PlanError("%s: delay_quant > 0 not supported" % n.name)
        if _parse(n.attrs.get("is_weight_perchannel", False)):
            raise PlanError("%s: per-channel weight quantization not supported" % n.name)
        return dict(name=n.name, minmax=n.inputs[1][0].name, ema=float(_parse(n.attrs.get("ema_decay", 0.99))),
                    nbits=int(_parse(n.attrs.get("nbits", 8))),
                    is_weight=bool(_parse(n.attrs.get("is_weight", False))))

    def _stem_quant(self, node, cons):
        """A data Quantization_int8 whose only consumer is the stem conv (folded into its im2col)."""
        cl = cons.get(id(node), [])
        return self._is_quant(node) and len(cl) == 1 and cl[0] is not None and cl[0].op == "Convolution" and \
            self._is_stem(cl[0])

    # --- lowering
    _ADDS = ("_Plus", "elemwise_add", "ElementWiseSum")

    def _lower(self):
        """One _lower_* per operator over the topological order, then the fusions that read the whole op list."""
        cons = self._consumers()
        done = set()  # nodes lowered, or folded into the op of an earlier node
        self._lower_inputs()
        fused_add_into, fused_add_relu = self._find_fused_adds(cons)
        for n in self.topo:
            if n.op == "null" or id(n) in done:
                continue
            op = n.op
            if op in ("identity", "Flatten", "Cast"):
                self._lower_alias(n)
            elif op == "Convolution":
                self._lower_conv(n, fused_add_into.get(id(n)), done)
            elif op == "BatchNorm":
                self._lower_bn(n, cons, done)
            elif op == "_contrib_Quantization_int8":
                self._lower_quant(n, cons)
            elif self._is_gdrq(n):
                self._lower_gdrq(n)
            elif self._is_qil(n):
                self._lower_qil(n)
            elif op == "_contrib_PACT" or op == "Custom":
                self._lower_pact(n)
            elif op == "Activation":
                self._lower_relu(n)
            elif op in self._ADDS:
                self._lower_add(n, fused_add_relu.get(id(n)), done)
            elif op in ("_contrib_BroadcastScale", "broadcast_add"):
                self._lower_affine(n, cons, done)
            elif op == "Pooling":
                self._lower_pool(n)
            elif op == "FullyConnected":
                self._lower_fc(n)
            elif op == "SoftmaxOutput":
                self._lower_softmax(n)
            else:
                raise PlanError("operator %s (%s) is not supported by the MI355X runtime" % (op, n.name))
            done.add(id(n))
        self.outputs = [self.tensor(n) for n, _ in self.symbol._outputs]
        self._fuse_bn_apply()
        self._mark_int8()

    def _lower_inputs(self):
        """The data / label inputs' tensors."""
        for n in self.topo:
            if n.op == "null" and n.name in self.data_names:
                shp = self.shape_of(n)
                t = TensorSpec(n.name, shp, F32, needs_grad=False, kind="data_nchw")
                self.tensors[id(n)] = t
                self.data_tensor = t
            elif n.op == "null" and n.name in self.label_names:
                self.tensors[id(n)] = TensorSpec(n.name, (self.shape_of(n)[0], 1), F32, False, "label")

    @staticmethod
    def _only_relu(cons, n):
        """The ReLU Activation that is node n's only consumer, else None."""
        cl = cons.get(id(n), [])
        if len(cl) == 1 and cl[0] is not None and cl[0].op == "Activation" and \
                _parse(cl[0].attrs.get("act_type")) == "relu":
            return cl[0]
        return None

    def _find_fused_adds(self, cons):
        """Residual adds fused into a convolution (a conv output consumed only by the add), and the ReLUs fused
        into the other adds: ({id(conv node): (add node, other input node)}, {id(add node): relu node})."""
        order = {id(n): i for i, n in enumerate(self.topo)}
        fused_add_into, fused_add_relu = {}, {}
        for n in self.topo:
            if n.op in self._ADDS and len(n.inputs) == 2:
                a, b = n.inputs[0][0], n.inputs[1][0]
                cands = [x for x in (a, b) if x.op == "Convolution" and len(cons.get(id(x), [])) == 1
                         and id(x) not in fused_add_into and not self._is_stem(x)]
                if cands:
                    conv = max(cands, key=lambda x: order[id(x)])
                    other = b if conv is a else a
                    if order[id(other)] < order[id(conv)] or other.op == "null":
                        fused_add_into[id(conv)] = (n, other)
                        continue
                relu_node = self._only_relu(cons, n)
                if relu_node is not None:
                    fused_add_relu[id(n)] = relu_node
        return fused_add_into, fused_add_relu

    def _lower_alias(self, n):
        """identity / Flatten / Cast: another name for the input's tensor. Cast is a no-op under the runtime
        precision policy (bf16 / fp32 compute)."""
        src = n.inputs[0][0]
        if n.op == "Flatten":
            st = self.tensor(src)
            if st.kind == "act" and (st.h != 1 or st.w != 1):
                raise PlanError("Flatten of a spatial map (%s) is not supported" % n.name)
        self.alias[id(n)] = id(src) if id(src) not in self.alias else self.alias[id(src)]

    def _lower_quant(self, n, cons):
        """Quantization_int8: a weight quantizer becomes a record on its convolution (self.qweight), an
        activation quantizer a "quant" op; the stem's is folded into its im2col."""
        q = self._quant_info(n)
        src = n.inputs[0][0]
        if q["is_weight"]:
            if src.op != "null":
                raise PlanError("%s: weight quantization of a computed tensor" % n.name)
            q["param"] = src.name
            self.qweight[id(n)] = q
        elif not self._stem_quant(n, cons):
            x = self.tensor(src)
            if x.kind != "act":
                raise PlanError("%s: data quantization of a non-activation tensor" % n.name)
            y = self._new_tensor(n, x.shape)
            self.ops.append(PlanOp("quant", n.name, x=x, y=y, q=q))

    def _lower_relu(self, n):
        act = _parse(n.attrs.get("act_type"))
        if act != "relu":
            raise PlanError("Activation %s is not supported" % act)
        x = self.tensor(n.inputs[0][0])
        y = self._new_tensor(n, self.shape_of(n))
        self.ops.append(PlanOp("relu", n.name, x=x, y=y, relu_name=n.name))

    def _lower_add(self, n, relu_node, done):
        if len(n.inputs) != 2:
            raise PlanError("ElementWiseSum with %d inputs not supported" % len(n.inputs))
        a = self.tensor(n.inputs[0][0])
        b = self.tensor(n.inputs[1][0])
        y = self._new_tensor(n, self.shape_of(n))
        self.ops.append(PlanOp("add", n.name, a=a, b=b, y=y, relu=relu_node is not None,
                               relu_name=relu_node.name if relu_node is not None else None))
        if relu_node is not None:
            self.alias[id(relu_node)] = id(n)
            done.add(id(relu_node))

    def _lower_softmax(self, n):
        x = self.tensor(n.inputs[0][0])
        if x.kind != "logits":
            raise PlanError("SoftmaxOutput must follow FullyConnected")
        lab = self.tensors[id(n.inputs[1][0])]
        y = self._new_tensor(n, (x.n, x.c), F32, kind="prob", needs_grad=False)
        self.ops.append(PlanOp("softmax", n.name, x=x, label=lab, y=y,
                               grad_scale=float(_parse(n.attrs.get("grad_scale", 1.0)))))

    def _lower_pact(self, n):
        """PACT (core/graph_optimize.py:180-187): mx.sym.contrib.PACT or mx.sym.Custom(op_type="PACT_PY"), the
        activation quantizer with a learned clipping threshold -- out = round(min(x, gamma) / unit) * unit,
        unit = gamma / (2^nbits - 1) (core/operator/PACT.py:102-144). gamma is an ordinary trainable parameter of
        shape (1,): it joins the flat parameter / gradient / momentum buffers like a BatchNorm's. The Python
        forward / backward of the CustomOp are never run; any other Custom op_type has no kernel here."""
        if n.op == "Custom" and _parse(n.attrs.get("op_type")) != "PACT_PY":
            raise PlanError("operator Custom (%s, op_type=%s) is not supported by the MI355X runtime"
                            % (n.name, n.attrs.get("op_type")))
        if len(n.inputs) != 2:
            raise PlanError("%s: PACT takes data and gamma" % n.name)
        g = n.inputs[1][0]
        if g.op != "null" or g.name in self.input_shapes:
            raise PlanError("%s: PACT's gamma must be a parameter Variable" % n.name)
        if any(o.kind == "pact" and o.gamma == g.name for o in self.ops):
            raise PlanError("%s: gamma %s is shared with another PACT node (not supported)" % (n.name, g.name))
        nbits = int(_parse(n.attrs.get("nbits", 8)))
        if not 1 <= nbits <= 16:
            raise PlanError("%s: PACT nbits %d not supported" % (n.name, nbits))
        x = self.tensor(n.inputs[0][0])
        if x.kind != "act":
            raise PlanError("%s: PACT of a non-activation tensor" % n.name)
        y = self._new_tensor(n, x.shape)
        self.ops.append(PlanOp("pact", n.name, x=x, y=y, gamma=g.name, nbits=nbits))

    @staticmethod
    def _is_gdrq(node):
        return node is not None and (node.op == "_contrib_GDRQ" or
                                     (node.op == "Custom" and _parse(node.attrs.get("op_type")) == "GDRQ_PY"))

    def _lower_gdrq(self, n):
        """GDRQ (core/graph_optimize.py:188-195): mx.sym.contrib.GDRQ or mx.sym.Custom(op_type="GDRQ_PY"), per-tensor
        form -- out = round(clip(x, -alpha, alpha) / unit) * unit, unit = alpha / (2^nbits - 1), a symmetric signed
        code for weights and activations alike (core/operator/GDRQ.py:50-190; attribute defaults as GDRQ_PYProp).
        alpha is an auxiliary state of shape (1,), no parameter: with fix_alpha it keeps the value it was
        initialised or loaded with; otherwise thr = ktimes * mean|x| moves it before the clip -- a weight's alpha is
        set to thr, an activation's becomes alpha + lamda * (alpha - thr) in training forwards (the reference's sign).
        A weight quantizer becomes a record on its convolution (self.qweight_gdrq, straight-through backward); an
        activation quantizer a "gdrq" op. The Python forward / backward of the CustomOp are never run."""
        a = n.attrs
        if int(_parse(a.get("group_size", -1))) != -1:
            raise PlanError("%s: GDRQ group_size %s not supported (per-tensor thresholds only, group_size=-1)"
                            % (n.name, a.get("group_size")))
        if int(_parse(a.get("delay_quant", 0))):
            raise PlanError("%s: GDRQ delay_quant > 0 not supported" % n.name)
        if len(n.inputs) != 2:
            raise PlanError("%s: GDRQ takes data and the auxiliary state alpha" % n.name)
        av = n.inputs[1][0]
        if av.op != "null" or av.name in self.input_shapes:
            raise PlanError("%s: GDRQ's alpha must be an auxiliary state Variable" % n.name)
        if av.name in self._gdrq_alphas:
            raise PlanError("%s: alpha %s is shared with GDRQ node %s (not supported)"
                            % (n.name, av.name, self._gdrq_alphas[av.name]))
        self._gdrq_alphas[av.name] = n.name
        nbits = int(_parse(a.get("nbits", 4)))
        if not 1 <= nbits <= 16:
            raise PlanError("%s: GDRQ nbits %d not supported" % (n.name, nbits))
        q = dict(family="gdrq", name=n.name, alpha=av.name, nbits=nbits,
                 fix_alpha=bool(_parse(a.get("fix_alpha", False))), ktimes=float(_parse(a.get("ktimes", 3))),
                 lamda=float(_parse(a.get("lamda", 0.001))), is_weight=bool(_parse(a.get("is_weight", False))))
        src = n.inputs[0][0]
        if q["is_weight"]:
            if src.op != "null":
                raise PlanError("%s: weight quantization of a computed tensor" % n.name)
            q["param"] = src.name
            self.qweight_gdrq[id(n)] = q
            return
        x = self.tensor(src)
        if x.kind != "act":
            raise PlanError("%s: GDRQ of a non-activation tensor" % n.name)
        y = self._new_tensor(n, x.shape)
        self.ops.append(PlanOp("gdrq", n.name, x=x, y=y, alpha=av.name, nbits=nbits, fix_alpha=q["fix_alpha"],
                               ktimes=q["ktimes"], lamda=q["lamda"]))

    @staticmethod
    def _is_qil(node):
        return node is not None and node.op == "Custom" and _parse(node.attrs.get("op_type")) == "QIL_PY"

    def _lower_qil(self, n):
        """QIL (core/graph_optimize.py:169-175): mx.sym.Custom(op_type="QIL_PY"), quantization-interval learning
        (core/operator/QIL.py:34-176, the "ste" branch): |x| below the pruning point p goes to 0, above the clipping
        point c to +-1, the interval between them linearly onto [0, 1], then the grid of 2^nbits - 1 steps -- the
        output lives in [-1, 1], for weights and activations alike. p, c and gamma are ordinary trainable parameters
        of shape (1,) in the flat parameter / gradient / momentum buffers; every forward clamps p to >= 0 and c to
        <= 1 in place. gamma is never read (fix_gamma must be True) and its gradient is zero. A weight quantizer
        becomes a record on its convolution (self.qweight_qil; its backward scales the weight gradient and yields
        dp / dc: rn_weight_qil_bwd), an activation quantizer a "qil" op. The Python forward / backward of the
        CustomOp are never run."""
        a = n.attrs
        if not bool(_parse(a.get("fix_gamma", True))):
            raise PlanError("%s: QIL fix_gamma=False (a learned gamma) is not supported" % n.name)
        nbits = int(_parse(a.get("nbits", 4)))
        if not 1 <= nbits <= 16:
            raise PlanError("%s: QIL nbits %d not supported" % (n.name, nbits))
        if len(n.inputs) != 4:
            raise PlanError("%s: QIL takes data, pruning_point, clipping_point and gamma" % n.name)
        names = []
        for (v, _), what in zip(n.inputs[1:], ("pruning_point", "clipping_point", "gamma")):
            if v.op != "null" or v.name in self.input_shapes or v.name in self.aux_names:
                raise PlanError("%s: QIL's %s must be a parameter Variable" % (n.name, what))
            if v.name in self._qil_vars or v.name in names:
                raise PlanError("%s: %s %s is shared with QIL node %s (not supported)"
                                % (n.name, what, v.name, self._qil_vars.get(v.name, n.name)))
            names.append(v.name)
        for nm in names:
            self._qil_vars[nm] = n.name
        q = dict(family="qil", name=n.name, prune=names[0], clip=names[1], gamma=names[2], nbits=nbits,
                 is_weight=bool(_parse(a.get("is_weight", False))))
        src = n.inputs[0][0]
        if q["is_weight"]:
            if src.op != "null":
                raise PlanError("%s: weight quantization of a computed tensor" % n.name)
            q["param"] = src.name
            self.qweight_qil[id(n)] = q
            return
        x = self.tensor(src) if id(src) in self.tensors or id(src) in self.alias else None
        if x is None or x.kind != "act":
            raise PlanError("%s: QIL of a non-activation tensor" % n.name)
        y = self._new_tensor(n, x.shape)
        self.ops.append(PlanOp("qil", n.name, x=x, y=y, prune=names[0], clip=names[1], qgamma=names[2], nbits=nbits))

    def _nonneg(self, t):
        """Is activation tensor `t` known to be >= 0: written by a BatchNorm with fused ReLU, a relu op, an add
        with ReLU, or a pooling of one of those (PACT has no lower clip: only then are its codes 0 .. 2^nbits - 1)?"""
        for op in self.ops:
            if op.y is t:
                if op.kind in ("bn", "add"):
                    return bool(op.relu)
                return op.kind == "relu" or (op.kind == "pool" and self._nonneg(op.x))
        return False

    def _mark_int8(self):
        """Quantized convolutions (a Quantization_int8 on both the data and the weight: resnet_int8,
        attach_quantize_node) whose input quantizer can also emit int8 codes run their forward on the
        int8 MFMAs (rn_conv_fwd_i8): exact integer sums of the codes, scaled by the two units, instead
        of bf16 / fp32 products of the fake-quantized values. RN_INT8_MFMA=0: the fake-quant path.
        A PACT input quantizer qualifies with nbits <= 7 (its codes reach 2^nbits - 1) over a tensor known to be
        non-negative (_nonneg); otherwise its convolution multiplies the fake-quantized values. A GDRQ quantizer's
        codes are signed, -L .. L with L = 2^nbits - 1: it qualifies with nbits <= 7 on the data side whatever its
        input's sign, and on the weight side (Quantization_int8 weights: nbits <= 8); mixed pairs qualify side by
        side. A QIL quantizer's codes are signed too, -L .. L with unit 1 / L: the same rule on both sides."""
        producer = {id(op.y): op for op in self.ops if op.kind in ("quant", "pact", "gdrq", "qil")}
        on = os.environ.get("RN_INT8_MFMA", "1") != "0"
        for op in self.ops:
            if op.kind in ("quant", "pact", "gdrq", "qil"):
                op.emit_codes = False
            if op.kind in ("pact", "gdrq", "qil"):
                op.codes_wgrad = False  # (never for PACT / GDRQ / QIL: the values are always written)
        for op in self.ops:
            if op.kind != "conv":
                continue
            q = producer.get(id(op.x))
            if q is not None and q.kind == "pact":
                q_ok = q.nbits <= 7 and self._nonneg(q.x)
            elif q is not None and q.kind in ("gdrq", "qil"):
                q_ok = q.nbits <= 7  # (signed codes -L .. L, L = 2^nbits - 1 <= 127; the input's sign is free)
            else:
                q_ok = q is not None and q.q["nbits"] <= 8
            # (a GDRQ / QIL weight's codes reach 2^nbits - 1, a Quantization_int8 weight's 2^(nbits - 1) - 1)
            w_ok = op.qweight is not None and \
                op.qweight["nbits"] <= (7 if op.qweight.get("family") in ("gdrq", "qil") else 8)
            op.int8 = bool(on and w_ok and q_ok and op.groups == 1 and op.x.cp % 16 == 0 and
                           op.xf is None)
            op.qsrc = q if op.int8 else None
            if op.int8:
                q.emit_codes = True
        # (round 4's opt-in RN_QUANT_DEFER -- the values expanded from the codes on the weight-gradient stream
        # by rn_quant_int8_expand -- measured 4 % slower on C5 and was removed in round 5; the weight gradients
        # multiply the codes instead, codes_wgrad)
        users = {}
        for op in self.ops:
            for k in ("x", "a", "b", "res", "label"):
                t = getattr(op, k, None)
                if t is not None and hasattr(t, "numel"):
                    users.setdefault(id(t), []).append(op)
        for op in self.ops:
            if op.kind == "quant":
                op.value_users = users.get(id(op.y), [])
                op.codes_wgrad = False  # (the executor decides: _codes_wgrad)

    def _fuse_bn_apply(self):
        """BatchNorm+ReLU whose output feeds ONLY 1x1 convolutions (act1 -> conv1 / sc, act3 -> conv3
        of the pre-activation units, symbol/resnet.py:17-31) or poolings (relu0 -> pool0 of the stem and
        relu1 -> the global pool, symbol/resnet.py:94-97,111-113): the consumers stage max(x*sc+sh, 0)
        from the BN input while loading (rn_conv_fwd_x / rn_conv_bwd_filter_x / rn_pool_fwd_x) and the
        BN+ReLU output is never written or read back."""
        refs = {}
        for op in self.ops:
            for key in ("x", "res", "a", "b"):
                t = getattr(op, key, None)
                if isinstance(t, TensorSpec):
                    refs.setdefault(id(t), []).append((op, key))
        out_ids = {id(t) for t in self.outputs}
        self._fuse_bn_add(refs, out_ids)
        # default on since the LDS-DMA tiles apply it (igemm_big_kernel / wgrad_big_kernel XF): 22.82 ->
        # 22.17 ms per step on one box; RN_BN_APPLY_FUSION=0 writes act1 / act3
        if os.environ.get("RN_BN_APPLY_FUSION", "1") != "1":
            return
        # (the 3x3 stride-1 consumers too -- act2 -> conv2 of stage 1, RN_BN_APPLY_FUSION_3X3, rounds 4-5 -- measured
        # 0.6 % slower, then equal with the image-band forward: removed in round 6; the band kernels keep their
        # BN+ReLU-on-load forms, kernel-tested)
        def xf_ok(u):
            return u.groups == 1 and not u.qweight and tuple(u.kernel) == (1, 1)
        # (the poolings: rn_pool_fwd_x; round 6, RN_POOL_XF=0 for the A/B)
        pool_ok = os.environ.get("RN_POOL_XF", "1") == "1"
        for bn in self.ops:
            if bn.kind != "bn" or not bn.relu or id(bn.y) in out_ids:
                continue
            users = refs.get(id(bn.y), [])
            ok = users and all(key == "x" and ((u.kind == "conv" and xf_ok(u)) or (u.kind == "pool" and pool_ok))
                               for u, key in users)
            if not ok:
                continue
            bn.apply_fused = True
            bn.y.virtual = True
            for u, _ in users:
                u.xf = bn

    def _fuse_bn_add(self, refs, out_ids):
        """The post-activation unit tail (symbol/resnext.py:40-47, symbol/resnet.py:63-74: bn3 (+ the
        shortcut's BN) -> add -> relu): a BatchNorm without ReLU whose output only this add reads is
        applied inside the add (rn_bn_apply_add); its output is never written."""
        producer = {id(op.y): op for op in self.ops if op.kind == "bn"}
        for op in self.ops:
            if op.kind != "add" or op.a is op.b:
                continue
            fused = []
            for key in ("a", "b"):
                t = getattr(op, key)
                bn = producer.get(id(t))
                if bn is not None and not bn.relu and id(t) not in out_ids and len(refs.get(id(t), [])) == 1:
                    fused.append((key, bn))
            if not fused:
                continue
            op.bn_a_key, op.bn_a = fused[0]
            op.bn_b = fused[1][1] if len(fused) == 2 else None
            for _, bn in fused:
                bn.apply_fused = True
                bn.y.virtual = True

    def _is_stem(self, conv_node):
        src = conv_node.inputs[0][0]
        shp = self.shape_of(src)
        return len(shp) == 4 and shp[1] % 8 != 0

    def _param_node(self, node, idx):
        p = node.inputs[idx][0]
        if self._is_quant(p) and id(p) in self.qweight:
            return self.qweight[id(p)]["param"]
        if id(p) in self.qweight_gdrq:
            return self.qweight_gdrq[id(p)]["param"]
        if id(p) in self.qweight_qil:
            return self.qweight_qil[id(p)]["param"]
        if p.op != "null":
            raise PlanError("%s: computed weights are not supported" % node.name)
        return p.name

    def _weight_quant(self, node, idx=1):
        p = node.inputs[idx][0]
        if self._is_quant(p):
            return self.qweight.get(id(p))
        return self.qweight_gdrq.get(id(p)) or self.qweight_qil.get(id(p))

    def _conv_attrs(self, n):
        k = _tup(n.attrs["kernel"])
        st = _tup(n.attrs.get("stride", (1, 1))) or (1, 1)
        pd = _tup(n.attrs.get("pad", (0, 0))) or (0, 0)
        dl = _tup(n.attrs.get("dilate", (1, 1))) or (1, 1)
        g = int(_parse(n.attrs.get("num_group", 1)))
        if dl != (1, 1):
            raise PlanError("%s: dilation not supported" % n.name)
        return k, st, pd, g

    def _lower_conv(self, n, fused, done):
        """`fused`: (add node, other input node) of the residual add this convolution's epilogue performs."""
        k, st, pd, g = self._conv_attrs(n)
        xshape = self.shape_of(n.inputs[0][0])
        yshape = self.shape_of(n)
        wname = self._param_node(n, 1)
        if not _parse(n.attrs.get("no_bias", False)):
            raise PlanError("%s: convolution bias not supported" % n.name)
        y = self._new_tensor(n, yshape)
        if self._is_stem(n):
            if g != 1:
                raise PlanError("%s: grouped stem convolution not supported" % n.name)
            src = self._var_input(n.inputs[0][0])
            squant = None
            if self._is_quant(src):
                squant = self._quant_info(src)
                src = self._var_input(src.inputs[0][0])
            bn = None
            if src.op == "BatchNorm":
                bn = src
                src = self._var_input(bn.inputs[0][0])
                if not _parse(bn.attrs.get("fix_gamma", True)):
                    raise PlanError("stem BatchNorm must have fix_gamma=True")
            if not (src.op == "null" and src.name in self.data_names):
                raise PlanError("%s: a conv over %d channels must read the data input" % (n.name, xshape[1]))
            kc = _pad8(k[0] * k[1] * xshape[1])
            kc = (kc + 31) // 32 * 32
            op = PlanOp("stem", n.name, x=self.tensors[id(src)], y=y, weight=wname, kernel=k, stride=st, pad=pd,
                        kc=kc, bn=None, quant=squant, qweight=self._weight_quant(n))
            if bn is not None:
                op.bn = dict(name=bn.name, gamma=self._param_node(bn, 1), beta=self._param_node(bn, 2),
                             mean=bn.inputs[3][0].name, var=bn.inputs[4][0].name,
                             eps=float(_parse(bn.attrs.get("eps", 1e-3))),
                             momentum=float(_parse(bn.attrs.get("momentum", 0.9))),
                             use_global_stats=bool(_parse(bn.attrs.get("use_global_stats", False))))
            self.ops.append(op)
            return
        x = self.tensor(n.inputs[0][0])
        if x.kind != "act":
            raise PlanError("%s: convolution over the raw data input needs C %% 8 != 0 (stem) here" % n.name)
        res = None
        if fused is not None:
            res = self.tensor(fused[1])
        if g != 1 and (xshape[1] % 8 or yshape[1] % 8):
            raise PlanError("%s: grouped convolution needs channel counts that are multiples of 8" % n.name)
        self.ops.append(PlanOp("conv", n.name, x=x, y=y, weight=wname, kernel=k, stride=st, pad=pd, res=res,
                               groups=g, qweight=self._weight_quant(n)))
        if fused is not None:
            self.alias[id(fused[0])] = id(n)
            done.add(id(fused[0]))

    def _lower_bn(self, n, cons, done):
        cl = cons.get(id(n), [])
        relu_node = self._only_relu(cons, n)
        src = self._var_input(n.inputs[0][0])
        stem_consumers = [c for c in cl if c is not None and
                          ((c.op == "Convolution" and self._is_stem(c)) or self._stem_quant(c, cons))]
        if src.op == "null" and src.name in self.data_names and stem_consumers and len(cl) == 1:
            return  # folded into the stem conv (bn_data)
        x = self.tensor(n.inputs[0][0])
        shape = self.shape_of(n)
        y = self._new_tensor(n, shape)
        self.ops.append(PlanOp("bn", n.name, x=x, y=y, relu=relu_node is not None,
                               gamma=self._param_node(n, 1), beta=self._param_node(n, 2),
                               mean=n.inputs[3][0].name, var=n.inputs[4][0].name,
                               eps=float(_parse(n.attrs.get("eps", 1e-3))),
                               momentum=float(_parse(n.attrs.get("momentum", 0.9))),
                               fix_gamma=bool(_parse(n.attrs.get("fix_gamma", True))),
                               use_global_stats=bool(_parse(n.attrs.get("use_global_stats", False))),
                               relu_name=relu_node.name if relu_node is not None else None))
        if relu_node is not None:
            self.alias[id(relu_node)] = id(n)
            done.add(id(relu_node))

    def _chan_param(self, node_idx, c):
        """Name of a per-channel parameter Variable ((C,) or (1,C,1,1)), else None."""
        v = node_idx[0]
        shp = self.shapes.get((id(v), node_idx[1]))
        if v.op != "null" or v.name in self.data_names or shp is None:
            return None
        if int(np.prod(shp)) != c or (len(shp) == 4 and shp[1] != c):
            return None
        return v.name

    def _lower_affine(self, n, cons, done):
        """Per-channel affine y = [relu](x * scale + bias): the BroadcastScale -> broadcast_add pair that
        merge_bn folds an inference BatchNorm into (core/graph_optimize.py:90-93), a standalone
        broadcast_add of a per-channel parameter, or (two same-shape tensors) a plain add."""
        x = self.tensor(n.inputs[0][0])
        c = x.c
        scale = bias = None
        last = n
        if n.op == "_contrib_BroadcastScale":
            scale = self._chan_param(n.inputs[1], c)
            if scale is None:
                raise PlanError("%s: BroadcastScale needs a per-channel (1,C,1,1) scaler Variable" % n.name)
            cl = cons.get(id(n), [])
            if len(cl) == 1 and cl[0] is not None and cl[0].op == "broadcast_add" and cl[0].inputs[0][0] is n:
                bias = self._chan_param(cl[0].inputs[1], c)
                if bias is not None:
                    last = cl[0]
        else:
            bias = self._chan_param(n.inputs[1], c)
            if bias is None:
                other = self.tensor(n.inputs[1][0])
                if other.shape != x.shape:
                    raise PlanError("%s: broadcast_add of %s and %s not supported" % (n.name, x.shape, other.shape))
                y = self._new_tensor(n, self.shape_of(n))
                self.ops.append(PlanOp("add", n.name, a=x, b=other, y=y, relu=False, relu_name=None))
                return
        if x.kind != "act":
            raise PlanError("%s: per-channel affine over a non-activation tensor" % n.name)
        relu_node = self._only_relu(cons, last)
        y = self._new_tensor(n, self.shape_of(n))
        self.ops.append(PlanOp("affine", n.name, x=x, y=y, gamma=scale, beta=bias, relu=relu_node is not None,
                               relu_name=relu_node.name if relu_node is not None else None))
        for extra in (last, relu_node):
            if extra is not None and extra is not n:
                self.alias[id(extra)] = id(n)
                done.add(id(extra))

    def _lower_pool(self, n):
        x = self.tensor(n.inputs[0][0])
        y = self._new_tensor(n, self.shape_of(n))
        ptype = _parse(n.attrs.get("pool_type", "max"))
        if ptype not in ("max", "avg"):
            raise PlanError("pool_type %s not supported" % ptype)
        glob = bool(_parse(n.attrs.get("global_pool", False)))
        if _parse(n.attrs.get("pooling_convention", "valid")) != "valid" and not glob:
            raise PlanError("pooling_convention other than 'valid' not supported")
        k = _tup(n.attrs.get("kernel", (1, 1))) or (1, 1)
        st = _tup(n.attrs.get("stride", (1, 1))) or (1, 1)
        pd = _tup(n.attrs.get("pad", (0, 0))) or (0, 0)
        self.ops.append(PlanOp("pool", n.name, x=x, y=y, type=ptype, global_pool=glob, kernel=k, stride=st, pad=pd))

    def _lower_fc(self, n):
        x = self.tensor(n.inputs[0][0])
        if x.h != 1 or x.w != 1:
            raise PlanError("%s: FullyConnected over a spatial map is not supported" % n.name)
        nh = int(_parse(n.attrs["num_hidden"]))
        no_bias = bool(_parse(n.attrs.get("no_bias", False)))
        y = self._new_tensor(n, (x.n, nh), F32, kind="logits")
        self.ops.append(PlanOp("fc", n.name, x=x, y=y, weight=self._param_node(n, 1),
                               bias=None if no_bias else self._param_node(n, 2), nh=nh,
                               qweight=self._weight_quant(n)))

    def summary(self):
        kinds = {}
        for op in self.ops:
            kinds[op.kind] = kinds.get(op.kind, 0) + 1
        return kinds

    def train_flops(self):
        """Algorithmic FLOP per step (2 FLOP/MAC): fwd + dgrad (except the stem) + wgrad."""
        total = 0
        for op in self.ops:
            if op.kind in ("conv", "stem"):
                y = op.y
                cin = op.x.shape[1] // op.groups
                macs = y.n * y.h * y.w * y.c * cin * op.kernel[0] * op.kernel[1]
                total += 2 * macs * (2 if op.kind == "stem" else 3)
            elif op.kind == "fc":
                total += 2 * op.x.n * op.x.c * op.nh * 3
        return total
