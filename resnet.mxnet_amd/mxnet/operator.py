"""mx.operator: CustomOp registration surface.

The reference registers Python CustomOps at import time (symbol/clip_grad_quantization_int8.py:70,
symbol/quant_ops.py:44, core/operator/*.py), so the classes must exist for `from symbol import *`
to succeed. Executing a Python CustomOp inside the MI355X plan is not supported: this module stays a
registration surface. mx.sym.Custom asks the prop registered under its op_type for list_arguments(),
list_auxiliary_states() and infer_shape() only (symbol.py), so that Custom(data=, gamma=, nbits="4",
op_type="PACT_PY") gets its gamma input and Custom(data=, alpha=, op_type="GDRQ_PY") its auxiliary alpha;
a PACT_PY / GDRQ_PY / QIL_PY node lowers to the runtime's own PACT / GDRQ / QIL kernels (rn/executor.py), and a
graph with any other Custom op_type fails at bind with an error that names it. forward / backward of a CustomOp are
never called. "QIL_PY" has no contrib twin, so its input list is registered here (QilProp, below): rn.graphs and a
saved symbol's JSON build QIL nodes without the reference's core/operator/QIL.py; importing that file registers its
own prop over this one, with the same lists.
"""

_REGISTRY = {}


class CustomOp:
    def __init__(self):
        pass

    def forward(self, is_train, req, in_data, out_data, aux):
        raise NotImplementedError

    def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
        raise NotImplementedError

    def assign(self, dst, req, src):
        if req == "null":
            return
        if req in ("write", "inplace"):
            dst[:] = src
        elif req == "add":
            dst[:] = dst.asnumpy() + (src.asnumpy() if hasattr(src, "asnumpy") else src)


class CustomOpProp:
    def __init__(self, need_top_grad=True):
        self.need_top_grad_ = need_top_grad

    def list_arguments(self):
        return ["data"]

    def list_outputs(self):
        return ["output"]

    def list_auxiliary_states(self):
        return []

    def infer_shape(self, in_shape):
        return in_shape, (in_shape[0],) * len(self.list_outputs()), ()

    def declare_backward_dependency(self, out_grad, in_data, out_data):
        return out_grad + in_data + out_data


def register(reg_name):
    def do_register(prop_cls):
        _REGISTRY[reg_name] = prop_cls
        return prop_cls

    return do_register


def get_registry():
    return dict(_REGISTRY)


@register("QIL_PY")
class QilProp(CustomOpProp):
    """core/operator/QIL.py:154-176: data and three trainable (1,) inputs -- the pruning point, the clipping point
    and gamma (fix_gamma: never read)."""

    def __init__(self, is_weight="False", fix_gamma="True", nbits="4"):
        self.is_weight = str(is_weight) == "True"
        self.fix_gamma = str(fix_gamma) == "True"
        self.nbits = int(nbits)
        super().__init__(True)

    def list_arguments(self):
        return ["data", "pruning_point", "clipping_point", "gamma"]

    def infer_shape(self, in_shape):
        shape = in_shape[0]
        return [shape, [1], [1], [1]], [shape], []
