"""Print the executor's bound call plan for a graph, built without a GPU (Executor(plan, "cpu")), as text that
does not depend on addresses: two trees bind the same plan exactly when their dumps are byte-identical. CPU-only.
usage: python tools/plan_dump.py GRAPH [--shape N,C,H,W] [--dtype bfloat16|float32]
GRAPH: a builder in rn.graphs (resnet50, resnext50_32x4d, resnet50_int8, resnet50_qil, ...; default shape 2,3,64,64) or one of the
16-class graphs of tests/test_stream_hazards_cpu.py (small_resnet20, small_resnet50, small_resnext50,
small_resnet_int8; their shapes there).

One line per bound call: list name, index, "side" for a side-stream call, entry point, arguments. A device pointer
-- a call argument, a field of a ctypes structure or array, a word of a device table -- inside a tensor that the
executor or one of its plan's ops holds prints as A<k>+<offset>/<allocation bytes>, k the allocation's rank by first
appearance here; the two stream arguments as S0 / S1; structures field by field in their state after the whole build
(the backward edits descriptors that forward calls hold by reference). Any other pointer prints as RAW:<hex>."""
import argparse
import bisect
import ctypes as C
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "resnet.mxnet_amd")]
from rn import graphs  # noqa: E402
from rn.executor import Executor, Plan  # noqa: E402

_STAGES = ([3, 4, 6, 3], 4, [64, 256, 512, 1024, 2048], 16)
SMALL = {
    "small_resnet20": (lambda: graphs.resnet20_cifar(), (8, 3, 32, 32)),
    "small_resnet50": (lambda: graphs.resnet(*_STAGES), (2, 3, 64, 64)),
    "small_resnext50": (lambda: graphs.resnext(*_STAGES, "float32", 32), (2, 3, 64, 64)),
    "small_resnet_int8": (lambda: graphs.resnet_int8([1, 1, 1, 1], *_STAGES[1:]), (2, 3, 64, 64)),
}


def live_spans(ex):
    """[(start, end)] of every torch allocation the executor or its plan's ops keep alive (the walk of
    tests/test_symbol_plan.py::_live_tensors), by storage, so that a view names its allocation."""
    import torch
    seen, spans = set(), set()

    def walk(o, depth=0):
        if depth > 4 or id(o) in seen:
            return
        seen.add(id(o))
        if isinstance(o, torch.Tensor):
            s = o.untyped_storage()
            spans.add((s.data_ptr(), s.data_ptr() + max(s.nbytes(), 1)))
        elif isinstance(o, dict):
            for v in o.values():
                walk(v, depth + 1)
        elif isinstance(o, (list, tuple)):
            for v in o:
                walk(v, depth + 1)
    for holder in [ex] + list(ex.plan.ops):
        for v in vars(holder).values():
            walk(v)
    return sorted(spans)


class Dump:
    def __init__(self, ex):
        self.ex = ex
        self.spans = live_spans(ex)
        self.starts = [s for s, _ in self.spans]
        self.rank = {}

    def addr(self, v, pointer=False):
        i = bisect.bisect_right(self.starts, v) - 1
        if i >= 0 and v < self.spans[i][1]:
            k = self.rank.setdefault(i, len(self.rank))
            return "A%d+%d/%d" % (k, v - self.spans[i][0], self.spans[i][1] - self.spans[i][0])
        return "RAW:%#x" % v if pointer else str(v)

    def fmt(self, a):
        if a is self.ex._spv or a is self.ex._spv2:
            return "S0" if a is self.ex._spv else "S1"
        if a is None or isinstance(a, (float, str, bytes)):
            return repr(a)
        if isinstance(a, int):
            return self.addr(int(a))
        if isinstance(a, C.c_void_p):
            return "NULL" if not a.value else self.addr(a.value, pointer=True)
        if isinstance(a, C.Structure):
            return "%s{%s}" % (type(a).__name__, ", ".join(
                "%s=%s" % (f[0], self.fmt(getattr(a, f[0]))) for f in a._fields_))
        if isinstance(a, C.Array):
            return "[%s]" % ", ".join(self.fmt(v) for v in a)
        if hasattr(a, "_obj"):  # ctypes.byref(...)
            return "&" + self.fmt(a._obj)
        if hasattr(a, "value"):  # c_int32, ...
            return "%s(%s)" % (type(a).__name__, self.fmt(a.value))
        raise TypeError("plan_dump: argument of type %s" % type(a).__name__)

    def lines(self):
        ex = self.ex
        for lname in ("_fwd_train", "_fwd_infer", "_bwd", "wpack_calls", "unfused_packs"):
            for i, (name, _, args) in enumerate(getattr(ex, lname)):
                side = " side" if lname == "_bwd" and i in ex._side_idx else ""
                yield "%s %d%s %s(%s)" % (lname, i, side, name, ", ".join(self.fmt(a) for a in args))
        for tname in ("_wq_items", "_wg_items", "_wl_items", "opt_packs", "opt_work"):
            t = getattr(ex, tname, None)
            if t is not None:
                words = t.contiguous().view(-1).view(ex.torch.uint8).numpy().view("<u8")
                yield "%s %s" % (tname, " ".join(self.addr(int(w)) for w in words))
        for k in sorted(ex.fused_packs):
            yield "fused_packs %s %s" % (k, " ".join(self.fmt(v) for v in ex.fused_packs[k]))
        for k in sorted(ex.param_done_at):
            yield "param_done_at %s %d" % (k, ex.param_done_at[k])
        yield "buckets %s" % (ex.buckets(),)
        # the update's multiplier tables as Module.init_optimizer sets them; printed only where the symbol moves
        # one (a graph without __lr_mult__ / __wd_mult__ attributes dumps as it always did)
        from rn.plan import multipliers
        lr_mult, wd_mult = multipliers(ex.plan.symbol, ex.plan.param_names)
        name_rule = {n: 0.0 for n in ex.plan.param_names if not (n.endswith("_weight") or n.endswith("_gamma"))}
        if lr_mult or wd_mult != name_rule:
            ex.set_multipliers(lr_mult, wd_mult)
            yield "update %s" % ("rn_sgd_mom_update_pack_lrm" if ex.opt_packs is not None else "rn_sgd_mom_update_lrm")
            for n, lm, wm in zip(ex.param_order, ex.lr_mult, ex.wd_mult):
                if lm != 1.0 or wm != (0.0 if n in name_rule else 1.0):
                    yield "multipliers %s lr %r wd %r" % (n, float(lm), float(wm))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("graph")
    ap.add_argument("--shape", default=None)
    ap.add_argument("--dtype", default="bfloat16", choices=("bfloat16", "float32"))
    a = ap.parse_args()
    symf, shp = SMALL[a.graph] if a.graph in SMALL else (getattr(graphs, a.graph), (2, 3, 64, 64))
    if a.shape:
        shp = tuple(int(v) for v in a.shape.split(","))
    ex = Executor(Plan(symf(), [("data", shp)], [("softmax_label", (shp[0],))], dtype=a.dtype), "cpu")
    sys.stdout.write("\n".join(Dump(ex).lines()) + "\n")


if __name__ == "__main__":
    main()
