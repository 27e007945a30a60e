"""Bind a lowered mx.sym graph (rn/plan.py) to librn calls and run training steps on one MI355X.

This replaces what MXNet's Module/executor did under core/solver.py (bind :75,
forward :115, backward :116, update :121): shape inference, buffer allocation, op dispatch,
gradient fan-in accumulation (req='add') and the optimizer step -- all as a static plan of
C-ABI calls on one HIP stream.

Planning (`Plan`, rn/plan.py) is pure Python and runs without a GPU (it is what the CPU tests check).
`Executor` allocates device memory through PyTorch (plumbing only) and turns the plan into
lists of bound C calls: named pre-passes, then one `_fwd_<kind>` / `_bwd_<kind>` method per op kind, looked up
by name. Every compute op is a librn kernel; there is no fallback path (a kind without a binder is an error).

Layout: activations NHWC, channel stride padded to a multiple of 8, dtype bf16 (default) or
fp32 (`dtype='float32'`, exact-fp32 MFMA path used for parity). Parameters live in ONE flat
fp32 master buffer (conv / FC weights in KRSC), ordered in reverse forward order so that
gradient buckets complete front-to-back during backward (RCCL bucketing, rn/dist.py).
"""
import os

import numpy as np

from . import lib as L
from .plan import Plan, PlanError, PlanOp, TensorSpec, _pad8  # noqa: F401  (re-exported: tests, tools, the shim)

F32, BF16 = L.RN_F32, L.RN_BF16


# ============================================================================= executor (GPU)
class _GradState:
    """Gradient routing during backward-plan construction (req write/add, lazy fan-in)."""

    def __init__(self, ex):
        self.ex = ex
        self.has_value = set()
        self.pending = {}

    def read(self, t):
        key = id(t)
        pend = self.pending.pop(key, [])
        if key not in self.has_value:
            if not pend:
                return None
            if len(pend) == 1:
                return pend[0]
            buf = self.ex.grad_buf(t)
            self.ex._emit_bwd(("add", t.numel, pend[0], pend[1], buf))
            self.ex._gw[key] = ("other",)
            pend = pend[2:]
            self.has_value.add(key)
        else:
            buf = self.ex.grad_buf(t)
        for p in pend:
            self.ex._emit_bwd(("add", t.numel, buf, p, buf))
            self.ex._gw[key] = ("other",)
        return buf

    def contribute(self, t):
        """(out_buffer, add_src) for a kernel with an add_src operand."""
        key = id(t)
        buf = self.ex.grad_buf(t)
        if key in self.has_value:
            # another contribution lands in a buffer that already holds one: the previous writer's fused
            # BN reduction (self.ex._gw, pool / dgrad) saw a partial gradient. A fusing writer re-registers
            # itself after its call (its output then includes this add operand); any other writer leaves
            # the entry "other", so the BN backward runs its own reduction
            self.ex._gw[key] = ("other",)
            return buf, buf
        self.has_value.add(key)
        pend = self.pending.get(key)
        if pend:
            return buf, pend.pop(0)
        return buf, None

    def alias(self, t, buf):
        self.pending.setdefault(id(t), []).append(buf)


class Executor:
    """Device buffers + bound C calls for one Plan on one GPU."""

    def __init__(self, plan, device, bucket_bytes=None):
        if bucket_bytes is None:  # RCCL all-reduce bucket size (RN_BUCKET_MB, default 25 MB)
            bucket_bytes = int(float(os.environ.get("RN_BUCKET_MB", "25")) * (1 << 20))
        import torch
        self.torch = torch
        self.plan = plan
        self.device = torch.device(device)
        self.dtype = plan.dtype
        self.tdtype = torch.bfloat16 if self.dtype == BF16 else torch.float32
        self.lib = L.load()
        # device='cpu' builds the full call plan without launching anything (CPU dry-run tests)
        self.dry_run = self.device.type == "cpu"
        # every bound call shares ONE c_void_p stream argument, re-pointed at torch's current stream
        # whenever a call list runs: the plan then follows the caller's stream -- torch ops, RCCL
        # ordering and HIP-graph capture (torch.cuda.graph) all see the same stream
        self._spv = L.C.c_void_p(0)
        # weight gradients run on a second stream (RN_WGRAD_STREAM=0: all on one): each forks from
        # the compute stream right before it (its dy is final there, its x was final since the
        # forward) and the backward joins it at the end, so a layer's wgrad overlaps the next
        # layers' dgrad / BatchNorm kernels and fills the CUs their last rounds leave idle
        self._spv2 = L.C.c_void_p(0)
        self._side_stream = None
        if not self.dry_run and os.environ.get("RN_WGRAD_STREAM", "1") == "1":
            self._side_stream = torch.cuda.Stream(device=self.device)
        # the weight gradients' split-M grids: part of the chip when they overlap the data-gradient chain,
        # all of it when they run serialised (before the plan sizes its workspace from the same key)
        # (50 % for every graph; round 6, one box, timed steps without event packets: C2 18.82 / 18.83 vs
        # 19.08 / 19.03 ms at 45 %, 55 % 18.95 / 18.98, 60 % 18.97, 70 % 19.00; C4 26.79 vs 27.01, C5 21.23 vs 21.32)
        self.wgrad_split_pct = L.WGRAD_SPLIT_OVERLAPPED
        L.set_wgrad_split(os.environ.get("RN_WGRAD_STREAM", "1") == "1", self.wgrad_split_pct)
        self._side_idx = set()
        self._side_pre = set()  # (of _side_idx) SIDE_PRE_CALLS
        self._events = {}
        self._side_enabled = True  # False: the side-stream calls run on the compute stream (serialised timing)
        self._sync_stream()
        self._acts = {}
        self._grads = {}
        self._fwd_train, self._fwd_infer, self._bwd = [], [], []
        # Quantization_int8: activation EMA states initialise from the first training batch
        self._qfirst = L.C.c_int32(1)
        self._build_params()
        self._alloc_acts()
        self._build_forward()
        self._build_backward()
        self._route_wgrads()
        self._build_update()
        self.bucket_bytes = bucket_bytes
        # the trailing bucket (RN_TAIL_BUCKET_MB, default 5 MB): the parameters at the flat buffer's end --
        # the stem's and the first stage's, whose gradients the backward completes last -- get a bucket of
        # their own, so that only this small one is exposed after the backward's last kernel
        self.tail_bucket_bytes = int(float(os.environ.get("RN_TAIL_BUCKET_MB", "5")) * (1 << 20))
        self.num_update = 0

    @property
    def side_enabled(self):
        return self._side_enabled

    @side_enabled.setter
    def side_enabled(self, on):
        """False: the weight gradients run on the compute stream, serialised (bench.py's calibration step),
        with the whole chip's split-M grids -- as RN_WGRAD_STREAM=0 runs them (lib.set_wgrad_split; the
        workspace is sized for both)."""
        on = bool(on)
        if on != self._side_enabled and self._side_stream is not None:
            L.set_wgrad_split(on, self.wgrad_split_pct)
        self._side_enabled = on

    # ------------------------------------------------------------------ buffers
    def _zeros(self, numel, dtype):
        return self.torch.zeros(int(max(numel, 1)), dtype=dtype, device=self.device)

    def _tdt(self, d):
        return self.torch.bfloat16 if d == BF16 else self.torch.float32

    def act(self, t):
        b = self._acts.get(id(t))
        if b is None:
            b = self._zeros(t.numel, self._tdt(t.dtype))
            self._acts[id(t)] = b
        return b

    def grad_buf(self, t):
        b = self._grads.get(id(t))
        if b is None:
            b = self._zeros(t.numel, self.tdtype)
            self._grads[id(t)] = b
        return b

    def _build_params(self):
        torch = self.torch
        plan = self.plan
        # reverse forward order: grads of late layers complete first during backward
        order = []
        seen = set()
        for op in plan.ops:
            for key in ("weight", "bias"):
                nm = getattr(op, key, None)
                if nm and nm not in seen:
                    order.append(nm)
                    seen.add(nm)
            for key in ("gamma", "beta"):
                nm = getattr(op, key, None)
                if nm and nm not in seen:
                    order.append(nm)
                    seen.add(nm)
            if op.kind == "stem" and op.bn:
                for key in ("gamma", "beta"):
                    nm = op.bn[key]
                    if nm not in seen:
                        order.append(nm)
                        seen.add(nm)
            # a QIL quantizer's pruning point, clipping point and (never read) gamma: the op's own, or its weight's
            qil = op.qweight if (op.qweight or {}).get("family") == "qil" else None
            for nm in ([qil["prune"], qil["clip"], qil["gamma"]] if qil else []) + \
                    ([op.prune, op.clip, op.qgamma] if op.kind == "qil" else []):
                if nm not in seen:
                    order.append(nm)
                    seen.add(nm)
        missing = [n for n in plan.param_names if n not in seen]
        if missing:
            raise PlanError("parameters not consumed by any lowered op: %s" % missing[:5])
        order = list(reversed(order))
        self.param_order = order
        self.param_off = {}
        self.param_shape = {}
        self.param_layout = {}
        off = 0
        conv_w = {op.weight for op in plan.ops if op.kind in ("conv", "stem")}
        for nm in order:
            shp = tuple(plan.param_shape(nm))
            self.param_shape[nm] = shp
            self.param_layout[nm] = "krsc" if (nm in conv_w and len(shp) == 4) else "plain"
            self.param_off[nm] = off
            off += int(np.prod(shp))
            off = (off + 3) // 4 * 4  # 16-byte aligned tensors
        self.nparam = off
        self.master = self._zeros(off, torch.float32)
        self.grad = self._zeros(off, torch.float32)
        self.mom = self._zeros(off, torch.float32)
        # aux (moving stats)
        self.aux_off = {}
        aoff = 0
        for nm in plan.aux_names:
            shp = tuple(plan.param_shape(nm))
            self.aux_off[nm] = (aoff, shp)
            aoff += int(np.prod(shp))
        self.aux = self._zeros(aoff, torch.float32)
        # device optimizer tables
        offs = [self.param_off[n] for n in order]
        nums = [int(np.prod(self.param_shape[n])) for n in order]
        self.opt_offsets = torch.tensor(offs, dtype=torch.int64, device=self.device)
        self.opt_numels = torch.tensor(nums, dtype=torch.int64, device=self.device)
        self.wd_mult = np.array([1.0 if (n.endswith("_weight") or n.endswith("_gamma")) else 0.0 for n in order],
                                dtype=np.float32)
        self.opt_wds = torch.zeros(len(order), dtype=torch.float32, device=self.device)
        self._wd_value = None
        self.lr_mult = np.ones(len(order), dtype=np.float32)
        self.opt_lrms = None  # the device table of rn_sgd_mom_update*_lrm: only where a multiplier is not 1

    def set_multipliers(self, lr_mult, wd_mult):
        """MXNet's Optimizer.lr_mult / wd_mult ({parameter name: factor}; a name without an entry: 1). The
        learning-rate table reaches the update (rn_sgd_mom_update*_lrm) only where some factor differs from 1: every
        other graph keeps today's calls."""
        self.wd_mult = np.array([wd_mult.get(n, 1.0) for n in self.param_order], dtype=np.float32)
        self._wd_value = None
        self.lr_mult = np.array([lr_mult.get(n, 1.0) for n in self.param_order], dtype=np.float32)
        self.opt_lrms = None
        if (self.lr_mult != 1.0).any():
            self.opt_lrms = self.torch.from_numpy(self.lr_mult.copy()).to(self.device)

    def pview(self, name):
        o = self.param_off[name]
        return self.master[o:o + int(np.prod(self.param_shape[name]))]

    def gview(self, name):
        o = self.param_off[name]
        return self.grad[o:o + int(np.prod(self.param_shape[name]))]

    def aview(self, name):
        o, shp = self.aux_off[name]
        return self.aux[o:o + int(np.prod(shp))]

    def _alloc_acts(self):
        for t in self.plan.tensors.values():
            if not getattr(t, "virtual", False):  # a fused BN+ReLU output is never materialised
                self.act(t)
        # input pipeline (data/imagenet.py SyntheticDataIter hands pinned host batches): two device
        # buffers; the stem reads whichever _in_ptr points at
        t = self.plan.data_tensor
        self._in_bufs = [self.act(t), None]
        self._in_free = [None, None]
        self._in_idx = 0
        self._in_ptr = L.C.c_void_p(self._in_bufs[0].data_ptr())
        self._copy_stream = None
        self.stats = self._zeros(4, self.torch.float32)

    # ------------------------------------------------------------------ helpers
    def _p(self, t):
        return None if t is None else L.ptr(t)

    def _pp(self, name):
        return L.C.c_void_p(self.master.data_ptr() + 4 * self.param_off[name])

    def _gp(self, name):
        return L.C.c_void_p(self.grad.data_ptr() + 4 * self.param_off[name])

    def _ap(self, name):
        return L.C.c_void_p(self.aux.data_ptr() + 4 * self.aux_off[name][0])

    def _call(self, fname, *args):
        fn = getattr(self.lib, fname)
        return (fname, fn, args)

    def _emit_bwd(self, item):
        if item[0] == "add":
            _, n, a, b, dst = item
            self._bwd.append(self._call("rn_eltwise_add", n, self.dtype, self._p(a), self._p(b), self._p(dst), 0,
                                        self._sp()))
        else:
            self._bwd.append(item)

    def _sp(self):
        return self._spv

    @property
    def stream(self):
        return None if self.dry_run else self.torch.cuda.current_stream(self.device)

    def _sync_stream(self):
        if not self.dry_run:
            self._spv.value = self.torch.cuda.current_stream(self.device).cuda_stream
            if self._side_stream is not None:
                self._spv2.value = self._side_stream.cuda_stream if self.side_enabled else self._spv.value

    # (rn_weight_qil_bwd: it rewrites the weight gradient its weight-gradient call just left, on the same stream)
    WGRAD_CALLS = ("rn_conv_bwd_filter", "rn_conv_bwd_filter_ws", "rn_conv_bwd_filter_x", "rn_conv_bwd_filter_i8",
                   "rn_stem_conv_wgrad_p4", "rn_stem_clip_wgrad", "rn_stem_clip_wgrad_chunk", "rn_stem_clip_dbeta",
                   "rn_weight_qil_bwd")
    # side-stream calls that depend on the forward only, not on the backward so far: no fork of their own
    # (they run while the side stream waits for the next dy), except the first of a step
    SIDE_PRE_CALLS = ("rn_stem_clip_mask",)

    def _stem_clip_mask(self, op):
        """Does the int8 stem's input-quantizer clip gradient ride in its weight gradient (bf16 NHWC-8
        image, rn_stem_clip_*; RN_STEM_CLIP_MASK=0: the gather kernel rn_stem_quant_clip_grad)?"""
        return bool(op.kind == "stem" and op.quant and op.bn and self.dtype == BF16 and not op.p4 and
                    self.lib is not None and os.environ.get("RN_STEM_CLIP_MASK", "1") == "1" and
                    self.lib.rn_stem_clip_supported(L.C.byref(op.dfull)))

    def _route_wgrads(self):
        """Bind the weight-gradient calls of the backward plan to the side stream.

        Invariant: the shared split-M slab workspace (self.wgrad_ws) is used by these calls only, so
        with the side stream on it is touched by that one stream, in plan order."""
        if self._side_stream is None:
            return
        ws = self.wgrad_ws.data_ptr() if self.wgrad_ws is not None else None
        for i, (name, fn, args) in enumerate(self._bwd):
            if name in self.WGRAD_CALLS + self.SIDE_PRE_CALLS and args and args[-1] is self._spv:
                self._bwd[i] = (name, fn, args[:-1] + (self._spv2,))
                self._side_idx.add(i)
                if name in self.SIDE_PRE_CALLS:
                    self._side_pre.add(i)
            elif ws is not None and any(isinstance(a, L.C.c_void_p) and a.value == ws for a in args):
                raise PlanError("%s uses the weight-gradient slab workspace but is not routed to the side "
                                "stream" % name)

    def _event(self, key):
        """One persistent HIP event per fork / join point of the backward plan (re-recorded every
        step): no event is created or destroyed while a stream may still wait on it."""
        ev = self._events.get(key)
        if ev is None:
            ev = self._events[key] = self.torch.cuda.Event()
        return ev

    def _fork(self, key):
        """The side stream continues after everything enqueued on the compute stream so far."""
        ev = self._event(("fork", key))
        ev.record(self.torch.cuda.current_stream(self.device))
        self._side_stream.wait_event(ev)

    def _join(self):
        ev = self._event(("join",))
        ev.record(self._side_stream)
        self.torch.cuda.current_stream(self.device).wait_event(ev)

    def _conv_desc(self, n, h, w, c, c_real, k, kernel, stride, pad, groups=1):
        d = L.ConvDesc(dtype=self.dtype, n=n, h=h, w=w, c=c, c_real=c_real, k=k, k_pad=_pad8(k), r=kernel[0],
                       s=kernel[1], stride_h=stride[0], stride_w=stride[1], pad_h=pad[0], pad_w=pad[1],
                       groups=groups)
        L.check(self.lib.rn_conv_desc_init(L.C.byref(d)), "rn_conv_desc_init")
        return d

    def _codes_wgrad(self, plan):
        """Quantizers whose fake-quantized values only int8 convolutions read, each of whose weight
        gradients takes the int8 codes instead (rn_conv_bwd_filter_i8: dW = unit * sum dy * code, the
        streaming and 128 / 256-column kernels, every ResNet-50 layer but stage 1's 3x3): the forward
        writes the codes only,
        and the bf16 values -- 2 of the pass's 5 bytes per element -- are never written or read
        (RN_QUANT_CODES_WGRAD=0: values + bf16 weight gradients)."""
        on = os.environ.get("RN_QUANT_CODES_WGRAD", "1") == "1" and self.dtype == L.RN_BF16
        for op in plan.ops:
            if op.kind != "quant":
                continue
            us = op.value_users
            ok = on and op.emit_codes and bool(us) and \
                all(u.kind == "conv" and u.int8 and u.qsrc is op for u in us)
            if ok:
                for u in us:
                    x, y = u.x, u.y
                    d = self._conv_desc(x.n, x.h, x.w, x.cp, x.c, y.c, u.kernel, u.stride, u.pad, u.groups)
                    ok = ok and int(self.lib.rn_conv_wgrad_i8_supported(L.C.byref(d))) == 1
            op.codes_wgrad = bool(ok)

    # ------------------------------------------------------------------ forward
    def _build_forward(self):
        """The pre-passes that stamp the ops, then one _fwd_<kind>(op, F, I) per op appending its calls to the
        train-mode (F) and infer-mode (I) lists, then the batched weight packs."""
        plan = self.plan
        self._descs = []  # keep ctypes structs alive
        self._codes_wgrad(plan)
        self.packs = []   # weight pack calls (bind time / set_params)
        # every weight quantizer in one rn_weight_quant_pack (RN_WQUANT_BATCH=0: three calls per weight)
        self._wq_batch = os.environ.get("RN_WQUANT_BATCH", "1") == "1"
        self._wq_ops = []
        self._wg_ops = []  # the ops with a GDRQ weight: one rn_weight_gdrq_pack for all of them
        self._gdrq_ws = None  # rn_gdrq_fwd's block partials: one buffer for every updating GDRQ (compute stream)
        self._wl_ops = []  # the ops with a QIL weight: one rn_weight_qil_pack for all of them
        self.fused_packs = {}  # param -> rn_wpack fields: copies rewritten by the SGD kernel itself
        self.unfused_packs = []  # packs that still run after every update (grouped, fake-quantized)
        # the grouped layers' repacks in one rn_conv_weight_pack_multi (RN_GPACK_BATCH=0: one call each)
        self._gpack_batch = os.environ.get("RN_GPACK_BATCH", "1") == "1"
        self._gpacks = []
        self._stem_ws_numel = 64  # (grown by _fwd_stem)
        # in this order: _mark_quant_bn reads the part_src that _mark_bn_stats sets; the binders below read the
        # descriptors, the workspaces and all of these marks
        self._mark_bn_stats()
        self._describe_ops()
        self._mark_quant_bn()
        for op in plan.ops:
            F, I = [], []
            # (_weight_source may append the bind-time quantizer calls of the unbatched path to self.packs: before
            # the op's own pack)
            op.wsrc = self._weight_source(op) if op.qweight else \
                (self._pp(op.weight) if getattr(op, "weight", None) else None)
            getattr(self, "_fwd_" + op.kind)(op, F, I)
            self._fwd_train.extend(F)
            self._fwd_infer.extend(I)
        self.stem_ws = self._zeros(self._stem_ws_numel, self.torch.float32)
        self._bind_weight_packs()

    def _mark_bn_stats(self):
        """BatchNorm statistics straight from the producing conv's epilogue (no separate stats pass): sets
        conv.bnstats and bn.part_src. The stem's is provisional: _fwd_stem, bound before the BatchNorm that reads
        part_src, clears both where the stem does not run the band kernel with whole bands per workgroup."""
        plan = self.plan
        producer = {}
        for op in plan.ops:  # (a plan bound again starts clean)
            op.bnstats = False
            op.part_src = None
            if op.kind in ("conv", "stem"):
                producer[id(op.y)] = op
        # default on since the 256-row conv tiles (measured -0.6 % step time with the bwd fusion)
        # fused only where the producer runs the 256-row tile: the 128-row kernel's epilogue costs
        # more than the statistics pass it saves (RN_BN_EPILOGUE_STATS=2: every conv producer)
        stats_mode = os.environ.get("RN_BN_EPILOGUE_STATS", "1")
        if stats_mode not in ("1", "2"):
            return
        for op in plan.ops:
            if op.kind == "bn" and not op.use_global_stats:
                src = producer.get(id(op.x))
                if src is not None and src.kind == "conv" and src.y.c % 8 == 0 and src.y.cp == op.x.cp and \
                        (stats_mode == "2" or self._big_tile(src, 0) or self._grouped_fuse(src, 0)) and \
                        not self._depthwise(src):
                    src.bnstats = True
                    op.part_src = src
                elif src is not None and src.kind == "stem" and src.y.cp == op.x.cp:
                    # (bn0's statistics from the stem band kernel: kept only where the stem runs it with
                    # whole bands per workgroup, rn_stem_bnstats_blocks; decided when the stem is built)
                    src.bnstats = True
                    op.part_src = src

    def _describe_ops(self):
        """The BatchNorm descriptors (held by reference by every call bound from here on: the backward writes
        clip / clip2 / dy2 and _fwd_bn xmm into them afterwards, and the calls see it) and the two workspaces sized
        over all ops."""
        ws_bytes = 64
        for op in self.plan.ops:
            if op.kind == "bn":
                d = L.BNDesc(dtype=self.dtype, m=op.x.rows, c=op.x.cp, c_real=op.x.c, eps=op.eps,
                             momentum=op.momentum, fix_gamma=int(op.fix_gamma), relu=int(op.relu))
                ws_bytes = max(ws_bytes, self.lib.rn_bn_workspace_bytes(L.C.byref(d)))
                op.desc = d
            elif op.kind == "affine":
                d = L.BNDesc(dtype=self.dtype, m=op.x.rows, c=op.x.cp, c_real=op.x.c, eps=0.0, momentum=0.0,
                             fix_gamma=0, relu=int(op.relu))
                ws_bytes = max(ws_bytes, self.lib.rn_bn_workspace_bytes(L.C.byref(d)))
            elif op.kind == "stem":
                x = op.x
                b = op.bn or {}
                op.bn_desc = L.BNDesc(dtype=self.dtype, m=x.n * x.h * x.w, c=8, c_real=x.c, eps=b.get("eps", 1e-5),
                                      momentum=b.get("momentum", 0.9), fix_gamma=1, relu=0)
                ws_bytes = max(ws_bytes, 2 * 8 * 256 * 4 + 64)
        self.ws = self._zeros(ws_bytes // 4 + 16, self.torch.float32)
        self._wsp = self._p(self.ws)
        self.qws = self._zeros(4096, self.torch.float32)
        self._qwsp = self._p(self.qws)

    def _mark_quant_bn(self):
        """Activation quantizers whose BatchNorm(+ReLU) input nothing else reads (the int8 graph): the
        quantizer applies the BN on load (rn_quant_int8_fwd_codes_bn, bit-identical) and the BN's
        output is never written -- with the folded straight-through backward nothing reads it. Where
        cp % 16 != 0 or a quantizer emits no codes: rn_bn_apply + rn_quant_int8_fwd_codes. Reads bn.part_src
        (_mark_bn_stats) and op.int8."""
        for op in self.plan.ops:  # (a plan bound again starts clean)
            op.bn_src = None
            op.bn_peer = None  # the second quantizer of the same BN output (written by this op's call)
            op.bn_lead = None  # (the quantizer whose call writes this one)
            op.want_mm = False
            op.mm_src = None
            if op.kind == "bn":
                op.apply_in_quant = False
        for bn, qs in self._quant_groups().values():
            if all(q.emit_codes for q in qs) and bn.x.cp % 16 == 0:
                bn.apply_in_quant = True
                qs[0].bn_src = bn
                if len(qs) == 2:
                    qs[0].bn_peer, qs[1].bn_lead = qs[1], qs[0]
                # the quantizers' max from the producing int8 conv's per-block extremes of the BN input
                # (rn_conv_fwd_i8_mm -> rn_bn_desc.xmm) instead of a pass over it
                src = bn.part_src
                if src is not None and src.int8 and bn.relu and self.dtype == BF16:
                    src.want_mm = True
                    src.mm_gamma = None if bn.fix_gamma else bn.gamma  # (its sign is the BN scale's)
                    bn.mm_src = src

    def _fwd_stem(self, op, F, I):
        """conv0 over the 3-channel input: bn_data statistics straight from the NCHW batch, one
        pass writing the normalised NHWC-8 copy, then the implicit GEMM in its small-C mode
        (k = tap*8 + c flattened; symbol/resnet.py:90-93)."""
        sp, wsp = self._spv, self._wsp
        x, y = op.x, op.y
        dfull = self._conv_desc(x.n, x.h, x.w, 8, x.c, y.c, op.kernel, op.stride, op.pad)
        assert (dfull.p, dfull.q) == (y.h, y.w), (op.name, dfull.p, dfull.q, y.h, y.w)
        op.dfull = op.desc = dfull
        # bf16 (not int8-quantized): the zero-bordered NHWC4 image instead of NHWC-8 (the
        # reduction runs over 8x8 taps x 4 channels = 256 instead of 7x7 x 8 = 392, and no
        # in-image tests); its border is zeroed here once, the prepare pass writes the inside
        hp = max(x.h + 2 * op.pad[0], (dfull.p - 1) * op.stride[0] + 8)
        wp = max(x.w + 2 * op.pad[1], (dfull.q - 1) * op.stride[1] + 8)
        op.p4 = None
        # (the NHWC4 stem's weight gradient adds with atomics: not in the deterministic mode)
        if self.dtype == BF16 and not op.quant and os.environ.get("RN_DETERMINISTIC", "0") != "1" and \
                self.lib.rn_stem_p4_supported(L.C.byref(dfull), hp, wp):
            op.p4 = (hp, wp)
            op.x8 = self._zeros(x.n * hp * wp * 4, self.tdtype)
            op.wk = self._zeros(y.c * 256, self.tdtype)
            c_ = self._call("rn_stem_weight_pack_p4", L.C.byref(dfull), op.wsrc, self._p(op.wk), sp)
            self.packs.append(c_)
            self.unfused_packs.append(c_)
        else:
            op.x8 = self._zeros(x.n * x.h * x.w * 8, self.tdtype)
            op.wk = self._zeros(y.c * op.kernel[0] * op.kernel[1] * 8, self.tdtype)
            self._add_pack(op, dfull, op.wk, None)
        self._stem_ws_numel = max(self._stem_ws_numel, y.h * y.w * y.cp + y.h * op.kernel[1] * y.c +
                                  y.c * op.kernel[0] * op.kernel[1] + 64)
        xnchw = self._in_ptr  # the current input buffer (double-buffered H2D pipeline)
        op.bnbuf = self._zeros(4 * 8, self.torch.float32)
        sm, si, sc, sh = [L.C.c_void_p(op.bnbuf.data_ptr() + 32 * i) for i in range(4)]
        op.bn_ptrs = (sm, si, sc, sh)
        b = op.bn
        if b:
            bnargs = (self._pp(b["gamma"]), self._pp(b["beta"]), self._ap(b["mean"]), self._ap(b["var"]))
            mode_f = 1 if b["use_global_stats"] else 0
            mode_i = 1
        else:
            bnargs = (None, None, None, None)
            mode_f = mode_i = 2
        for lst, mode in ((F, mode_f), (I, mode_i)):
            if op.p4:
                lst.append(self._call("rn_stem_prepare_p4", L.C.byref(op.bn_desc), xnchw, x.n, x.c, x.h, x.w,
                                      self._p(op.x8), op.p4[0], op.p4[1], op.pad[0], op.pad[1], mode,
                                      *bnargs, sm, si, sc, sh, wsp, sp))
            else:
                lst.append(self._call("rn_stem_prepare", L.C.byref(op.bn_desc), xnchw, x.n, x.c, x.h, x.w,
                                      self._p(op.x8), mode, *bnargs, sm, si, sc, sh, wsp, sp))
        if op.quant:
            q = op.quant
            for lst, tr in ((F, 1), (I, 0)):
                lst.append(self._call("rn_quant_int8_fwd", self.dtype, x.n * x.h * x.w * 8, self._p(op.x8),
                                      self._p(op.x8), self._ap(q["minmax"]), 0, tr, q["ema"], self._qfirst,
                                      q["nbits"], self._qwsp, sp))
        nblk = int(self.lib.rn_stem_bnstats_blocks(L.C.byref(dfull), *op.p4)) if (op.p4 and op.bnstats) else 0
        if op.bnstats and nblk <= 0:  # the BatchNorm runs its own statistics pass
            op.bnstats = False
            for o in self.plan.ops:  # (bn0 is bound after this op: its binder sees part_src cleared)
                if o.part_src is op:
                    o.part_src = None
        if op.p4:
            c_ = self._call("rn_stem_conv_fwd_p4", L.C.byref(dfull), self._p(op.x8), self._p(op.wk),
                            self._p(self.act(y)), op.p4[0], op.p4[1], sp)
            I.append(c_)
            if op.bnstats:  # + bn0's statistics of the stored output, one block per band workgroup
                op.part_blocks, op.part_rows = nblk, y.rows // nblk
                op.part = self._zeros(nblk * 3 * y.cp, self.torch.float32)
                F.append(self._call("rn_stem_conv_fwd_p4_bnstats", L.C.byref(dfull), self._p(op.x8), self._p(op.wk),
                                    self._p(self.act(y)), op.p4[0], op.p4[1], self._p(op.part), sp))
            else:
                F.append(c_)
        else:
            I.append(self._call("rn_conv_fwd", L.C.byref(dfull), self._p(op.x8), self._p(op.wk),
                                self._p(self.act(y)), self.dtype, None, None, sp))
            F.append(self._conv_fwd_call(op, dfull, self._p(op.x8), None))

    def _fwd_conv(self, op, F, I):
        x, y = op.x, op.y
        d = self._conv_desc(x.n, x.h, x.w, x.cp, x.c, y.c, op.kernel, op.stride, op.pad, op.groups)
        assert (d.p, d.q) == (y.h, y.w), (op.name, d.p, d.q, y.h, y.w)
        op.desc = d
        op.wc = self._zeros(self.lib.rn_conv_pack_numel(L.C.byref(d), 1), self.tdtype)
        wgdrq = op in self._wg_ops or op in self._wl_ops
        if wgdrq and op.groups == 1 and not op.int8:
            # (both compute copies written by rn_weight_gdrq_pack / rn_weight_qil_pack; their padding stays zero)
            op.wk = self._zeros(self.lib.rn_conv_pack_numel(L.C.byref(d), 0), self.tdtype)
        elif op.int8:
            # forward copy: the int8 codes (KRSC); the data-gradient copy stays the
            # fake-quantized values in the compute dtype (STE backward)
            op.wk = None
            op.wk8 = self.torch.zeros(int(self.lib.rn_conv_pack_numel(L.C.byref(d), 0)),
                                      dtype=self.torch.int8, device=self.device)
            if not self._wq_batch and not wgdrq:  # (batched: written by rn_weight_quant_pack)
                self._add_pack(op, d, None, op.wc)
                c_ = self._call("rn_conv_weight_pack_i8", L.C.byref(d), self._pp(op.weight),
                                self._p(op.wunit), self._p(op.wk8), self._spv)
                self.packs.append(c_)
                self.unfused_packs.append(c_)
        else:
            op.wk = self._zeros(self.lib.rn_conv_pack_numel(L.C.byref(d), 0), self.tdtype)
            self._add_pack(op, d, op.wk, op.wc)
        res = self._p(self.act(op.res)) if op.res is not None else None
        xin = self._p(self.act(op.xf.x)) if op.xf is not None else self._p(self.act(x))
        I.append(self._conv_fwd_call(op, d, xin, res, stats=False))
        # (allocates op.part / op.part_mm, which the BatchNorm bound after this conv reads)
        F.append(self._conv_fwd_call(op, d, xin, res))

    def _fwd_bn(self, op, F, I):
        sp, wsp = self._spv, self._wsp
        x, y = op.x, op.y
        c = x.cp
        op.buf = self._zeros(4 * c, self.torch.float32)
        op.sm, op.si, op.sc, op.sh = [L.C.c_void_p(op.buf.data_ptr() + 4 * c * i) for i in range(4)]
        gamma = self._pp(op.gamma)
        # fused into the 1x1 consumers' loads or the quantizer's: coefficients only
        yptr = None if op.apply_fused or op.apply_in_quant else self._p(self.act(y))
        # (part_mm: allocated by _conv_fwd_call when the producing int8 conv, earlier in the plan, was bound)
        if op.mm_src is not None and op.mm_src.part_mm is not None:
            op.desc.xmm = op.mm_src.part_mm.data_ptr()
            op.desc.xmm_blocks = op.mm_src.part_blocks
        infer = self._call("rn_bn_fwd_infer", L.C.byref(op.desc), self._p(self.act(x)), yptr,
                           gamma, self._pp(op.beta), self._ap(op.mean), self._ap(op.var), op.sc, op.sh, sp)
        if op.use_global_stats:
            F.append(infer)
        elif op.part_src is not None:
            s_ = op.part_src
            F.append(self._call("rn_bn_fwd_train_part", L.C.byref(op.desc), self._p(s_.part), s_.part_blocks,
                                s_.part_rows, s_.y.cp, self._p(self.act(x)), yptr, gamma, self._pp(op.beta),
                                self._ap(op.mean), self._ap(op.var), op.sm, op.si, op.sc, op.sh, wsp, sp))
        else:
            F.append(self._call("rn_bn_fwd_train", L.C.byref(op.desc), self._p(self.act(x)), yptr, gamma,
                                self._pp(op.beta), self._ap(op.mean),
                                self._ap(op.var), op.sm, op.si, op.sc, op.sh, wsp, sp))
        I.append(infer)

    def _fwd_affine(self, op, F, I):
        """y = [relu](x*scale + bias) with per-channel parameters copied into channel-padded
        coefficient vectors each forward (set_params / SGD may change them)."""
        sp = self._spv
        x, y = op.x, op.y
        c = x.cp
        op.buf = self._zeros(4 * c, self.torch.float32)
        if op.gamma is None:
            op.buf[:x.c] = 1.0
        op.sc, op.sh, op.zero, op.one = [L.C.c_void_p(op.buf.data_ptr() + 4 * c * i) for i in range(4)]
        op.buf[3 * c:3 * c + x.c] = 1.0
        op.desc = L.BNDesc(dtype=self.dtype, m=x.rows, c=c, c_real=x.c, eps=0.0, momentum=0.0,
                           fix_gamma=int(op.gamma is None), relu=int(op.relu))
        calls = [self._call("rn_cast", x.c, self._pp(nm), F32, dst, F32, sp)
                 for nm, dst in ((op.gamma, op.sc), (op.beta, op.sh)) if nm is not None]
        calls.append(self._call("rn_bn_apply", L.C.byref(op.desc), self._p(self.act(x)), self._p(self.act(y)),
                                op.sc, op.sh, sp))
        F.extend(calls)
        I.extend(calls)

    def _fwd_relu(self, op, F, I):
        c = self._call("rn_eltwise_add", op.x.numel, self.dtype, self._p(self.act(op.x)), None,
                       self._p(self.act(op.y)), 1, self._spv)
        F.append(c)
        I.append(c)

    def _fwd_quant(self, op, F, I):
        sp, qwsp = self._spv, self._qwsp
        q = op.q
        for o in (op, op.bn_peer):
            if o is not None and o.emit_codes and o.codes is None:
                # + the int8 codes and unit the consumers' int8 forward reads
                o.codes = self.torch.zeros(o.x.numel, dtype=self.torch.int8, device=self.device)
                o.unit = self._zeros(1, self.torch.float32)
        # (codes_wgrad: codes only, the weight gradients multiply them)
        vout = lambda o: None if o.codes_wgrad else self._p(self.act(o.y))  # noqa: E731
        for lst, tr in ((F, 1), (I, 0)):
            if op.bn_lead is not None:
                pass  # written by its peer's call
            elif op.bn_peer is not None:
                bn, o2 = op.bn_src, op.bn_peer
                lst.append(self._call("rn_quant_int8_fwd_codes_bn2", L.C.byref(bn.desc), self._p(self.act(bn.x)), bn.sc,
                                      bn.sh, vout(op), self._p(op.codes), self._p(op.unit), self._ap(q["minmax"]),
                                      q["ema"], q["nbits"], vout(o2), self._p(o2.codes), self._p(o2.unit),
                                      self._ap(o2.q["minmax"]), o2.q["ema"], o2.q["nbits"], tr, self._qfirst, qwsp, sp))
            elif op.bn_src is not None:
                bn = op.bn_src
                lst.append(self._call("rn_quant_int8_fwd_codes_bn", L.C.byref(bn.desc), self._p(self.act(bn.x)), bn.sc,
                                      bn.sh, vout(op), self._p(op.codes), self._p(op.unit), self._ap(q["minmax"]), tr,
                                      q["ema"], self._qfirst, q["nbits"], qwsp, sp))
            elif op.emit_codes:
                lst.append(self._call("rn_quant_int8_fwd_codes", self.dtype, op.x.numel, self._p(self.act(op.x)),
                                      vout(op), self._p(op.codes), self._p(op.unit), self._ap(q["minmax"]), 0, tr,
                                      q["ema"], self._qfirst, q["nbits"], qwsp, sp))
            else:
                lst.append(self._call("rn_quant_int8_fwd", self.dtype, op.x.numel, self._p(self.act(op.x)),
                                      self._p(self.act(op.y)), self._ap(q["minmax"]), 0, tr, q["ema"],
                                      self._qfirst, q["nbits"], qwsp, sp))

    def _fwd_pact(self, op, F, I):
        """The same in training and inference; gamma is read on the device from the flat master buffer, so
        every step (and a replayed graph) sees the value the last update left. The values are always
        written; with emit_codes also the int8 codes and the unit the consumers' int8 forward reads."""
        op.unit = self._zeros(1, self.torch.float32)
        op.codes = self.torch.zeros(op.x.numel, dtype=self.torch.int8, device=self.device) \
            if op.emit_codes else None
        c = self._call("rn_pact_fwd", self.dtype, op.x.numel, self._p(self.act(op.x)), self._pp(op.gamma),
                       op.nbits, self._p(self.act(op.y)), self._p(op.codes), self._p(op.unit), self._spv)
        F.append(c)
        I.append(c)

    def _fwd_gdrq(self, op, F, I):
        """alpha is read (and, in training without fix_alpha, first updated) on the device in the aux buffer:
        no host synchronisation, a replayed graph sees the current value. Inference never writes it. The
        values are always written; with emit_codes also the signed int8 codes and the unit."""
        x = op.x
        op.unit = self._zeros(1, self.torch.float32)
        op.codes = self.torch.zeros(x.numel, dtype=self.torch.int8, device=self.device) \
            if op.emit_codes else None
        if not op.fix_alpha and self._gdrq_ws is None:  # (one buffer, made by the first op that needs it)
            nmax = max(o.x.numel for o in self.plan.ops if o.kind == "gdrq" and not o.fix_alpha)
            self._gdrq_ws = self._zeros(int(self.lib.rn_gdrq_ws_bytes(nmax)) // 4, self.torch.float32)
        for lst, upd in ((F, int(not op.fix_alpha)), (I, 0)):
            lst.append(self._call("rn_gdrq_fwd", self.dtype, x.numel, x.rows * x.c, self._p(self.act(x)),
                                  self._ap(op.alpha), op.nbits, upd, op.ktimes, op.lamda, self._p(self.act(op.y)),
                                  self._p(op.codes), self._p(op.unit),
                                  self._p(self._gdrq_ws) if upd else None, self._spv))

    def _fwd_qil(self, op, F, I):
        """The same in training and inference; the pruning and clipping points are read, clamped and written back on
        the device in the flat master buffer. The values are always written; with emit_codes also the signed int8
        codes and the unit 1 / L the consumers' int8 forward reads."""
        op.unit = self._zeros(1, self.torch.float32)
        op.codes = self.torch.zeros(op.x.numel, dtype=self.torch.int8, device=self.device) \
            if op.emit_codes else None
        c = self._call("rn_qil_fwd", self.dtype, op.x.numel, self._p(self.act(op.x)), self._pp(op.prune),
                       self._pp(op.clip), op.nbits, self._p(self.act(op.y)), self._p(op.codes), self._p(op.unit),
                       self._spv)
        F.append(c)
        I.append(c)

    def _fwd_add(self, op, F, I):
        if op.bn_a is not None:  # the BatchNorms of the post-activation unit tail applied inside the add
            bna, bnb = op.bn_a, op.bn_b
            other = op.b if op.bn_a_key == "a" else op.a
            c = self._call("rn_bn_apply_add", L.C.byref(bna.desc), self._p(self.act(bna.x)), bna.sc, bna.sh,
                           self._p(self.act(bnb.x if bnb is not None else other)), bnb.sc if bnb is not None else None,
                           bnb.sh if bnb is not None else None, self._p(self.act(op.y)), int(op.relu), self._spv)
        else:
            c = self._call("rn_eltwise_add", op.y.numel, self.dtype, self._p(self.act(op.a)),
                           self._p(self.act(op.b)), self._p(self.act(op.y)), int(op.relu), self._spv)
        F.append(c)
        I.append(c)

    def _fwd_pool(self, op, F, I):
        x, y = op.x, op.y
        d = L.PoolDesc(dtype=self.dtype, n=x.n, h=x.h, w=x.w, c=x.cp, r=op.kernel[0], s=op.kernel[1],
                       stride_h=op.stride[0], stride_w=op.stride[1], pad_h=op.pad[0], pad_w=op.pad[1],
                       type=L.RN_POOL_MAX if op.type == "max" else L.RN_POOL_AVG, global_pool=int(op.global_pool))
        L.check(self.lib.rn_pool_desc_init(L.C.byref(d)), "rn_pool_desc_init")
        assert (d.p, d.q) == (y.h, y.w), (op.name, d.p, d.q, y.h, y.w)
        op.desc = d
        op.argmax = self.torch.zeros(max(y.rows * y.cp, 1), dtype=self.torch.uint8, device=self.device) \
            if op.type == "max" else None
        if op.xf is not None:  # the producing BatchNorm+ReLU applied while loading
            c = self._call("rn_pool_fwd_x", L.C.byref(d), self._p(self.act(op.xf.x)), self._p(self.act(y)),
                           self._p(op.argmax), op.xf.sc, op.xf.sh, self._spv)
        else:
            c = self._call("rn_pool_fwd", L.C.byref(d), self._p(self.act(x)), self._p(self.act(y)),
                           self._p(op.argmax), self._spv)
        F.append(c)
        I.append(c)

    def _fwd_fc(self, op, F, I):
        x, y = op.x, op.y
        d = self._conv_desc(x.n, 1, 1, x.cp, x.c, op.nh, (1, 1), (1, 1), (0, 0))
        op.desc = d
        op.wk = self._zeros(op.nh * x.cp, self.tdtype)
        op.wc = self._zeros(x.cp * _pad8(op.nh), self.tdtype)
        if op not in self._wg_ops and op not in self._wl_ops:  # (a GDRQ / QIL weight: copies written by its pack)
            self._add_pack(op, d, op.wk, op.wc)
        bias = self._pp(op.bias) if op.bias else None
        c = self._call("rn_conv_fwd", L.C.byref(d), self._p(self.act(x)), self._p(op.wk),
                       self._p(self.act(y)), F32, None, bias, self._spv)
        F.append(c)
        I.append(c)

    def _fwd_softmax(self, op, F, I):
        x = op.x
        # gradient of the logits is produced here (SoftmaxOutput's backward needs no head grad)
        dl = self.grad_buf(x)
        F.append(self._call("rn_softmax_output", self.dtype, x.n, x.c, x.cp, self._p(self.act(x)),
                            self._p(self.act(op.label)), self._p(self.act(op.y)), self._p(dl),
                            op.grad_scale, self._p(self.stats), self._spv))
        I.append(self._call("rn_softmax_output", self.dtype, x.n, x.c, x.cp, self._p(self.act(x)),
                            self._p(self.act(op.label)), self._p(self.act(op.y)), None, op.grad_scale, None, self._spv))

    def _wquant_shape(self, op):
        """(k, c_real, r*s) of a quantized weight."""
        shape = self.plan.param_shape(op.weight)
        return shape[0], shape[1], int(np.prod(shape[2:])) if len(shape) > 2 else 1

    def _bind_weight_packs(self):
        """The three batched tails, bound after the forward walk has met every weight: rn_weight_quant_pack and
        rn_weight_gdrq_pack go to the front of the pack lists (the stem's and the grouped layers' packs read their
        fake-quantized copies), rn_conv_weight_pack_multi to the end."""
        sp = self._spv
        if self._wq_ops:
            items = []
            for op in self._wq_ops:
                k, creal, rs = self._wquant_shape(op)
                i8 = op.int8
                d = op.desc if i8 else None
                assert not i8 or (d.groups <= 1 and d.k == k and d.c_real == creal and d.r * d.s == rs)
                items.append(L.WQuantItem(
                    master=self._pp(op.weight).value, qw=op.qw.data_ptr(),
                    unit=op.wunit.data_ptr() if i8 else None, minmax=self._ap(op.qweight["minmax"]).value,
                    w_codes=op.wk8.data_ptr() if i8 else None, w_crsk=op.wc.data_ptr() if i8 else None, k=k, rs=rs,
                    c_real=creal, c=d.c if i8 else creal, k_pad=d.k_pad if i8 else k, nbits=int(op.qweight["nbits"])))
            arr = (L.WQuantItem * len(items))(*items)
            self._wq_items = self.torch.frombuffer(bytearray(arr), dtype=self.torch.uint8).to(self.device)
            c_ = self._call("rn_weight_quant_pack", self._p(self._wq_items), len(items), self.dtype, self._qwsp, sp)
            self.packs.insert(0, c_)
            self.unfused_packs.insert(0, c_)
        if self._wg_ops:
            # every GDRQ weight in one rn_weight_gdrq_pack, ahead of the packs that read its fake-quantized copies
            # (the stem's and the grouped layers'): thresholds, units, the copies of the dense layers
            items = []
            for op in self._wg_ops:
                k, creal, rs = self._wquant_shape(op)
                i8 = op.int8
                dense = op.kind == "fc" or (op.kind == "conv" and op.groups == 1)
                d = op.desc if dense else None
                assert not dense or (d.k == k and d.c_real == creal and d.r * d.s == rs), op.name
                q = op.qweight
                items.append(L.WGdrqItem(
                    master=self._pp(op.weight).value, qw=op.qw.data_ptr(),
                    unit=op.wunit.data_ptr() if i8 else None, alpha=self._ap(q["alpha"]).value,
                    w_codes=op.wk8.data_ptr() if i8 else None, w_krsc=op.wk.data_ptr() if dense and not i8 else None,
                    w_crsk=op.wc.data_ptr() if dense else None, k=k, rs=rs, c_real=creal, c=d.c if dense else creal,
                    k_pad=d.k_pad if dense else k, nbits=int(q["nbits"]), fix_alpha=int(q["fix_alpha"]),
                    ktimes=float(q["ktimes"])))
            arr = (L.WGdrqItem * len(items))(*items)
            self._wg_items = self.torch.frombuffer(bytearray(arr), dtype=self.torch.uint8).to(self.device)
            self._wg_ws = self._zeros(int(self.lib.rn_weight_gdrq_ws_bytes(len(items))) // 4, self.torch.float32)
            c_ = self._call("rn_weight_gdrq_pack", self._p(self._wg_items), len(items), self.dtype,
                            self._p(self._wg_ws), sp)
            self.packs.insert(0, c_)
            self.unfused_packs.insert(0, c_)
        if self._wl_ops:
            # every QIL weight in one rn_weight_qil_pack, ahead of the packs that read its fake-quantized copies
            items = []
            for op in self._wl_ops:
                k, creal, rs = self._wquant_shape(op)
                i8 = op.int8
                dense = op.kind == "fc" or (op.kind == "conv" and op.groups == 1)
                d = op.desc if dense else None
                assert not dense or (d.k == k and d.c_real == creal and d.r * d.s == rs), op.name
                q = op.qweight
                items.append(L.WQilItem(
                    master=self._pp(op.weight).value, qw=op.qw.data_ptr(),
                    unit=op.wunit.data_ptr() if i8 else None, p=self._pp(q["prune"]).value,
                    c=self._pp(q["clip"]).value, w_codes=op.wk8.data_ptr() if i8 else None,
                    w_krsc=op.wk.data_ptr() if dense and not i8 else None, w_crsk=op.wc.data_ptr() if dense else None,
                    k=k, rs=rs, c_real=creal, c_stride=d.c if dense else creal, k_pad=d.k_pad if dense else k,
                    nbits=int(q["nbits"])))
            arr = (L.WQilItem * len(items))(*items)
            self._wl_items = self.torch.frombuffer(bytearray(arr), dtype=self.torch.uint8).to(self.device)
            self._wl_ws = self._zeros(int(self.lib.rn_weight_qil_ws_bytes(len(items))) // 4, self.torch.float32)
            c_ = self._call("rn_weight_qil_pack", self._p(self._wl_items), len(items), self.dtype,
                            self._p(self._wl_ws), sp)
            self.packs.insert(0, c_)
            self.unfused_packs.insert(0, c_)
        if self._gpacks:
            n = len(self._gpacks)
            vp = lambda v: v.value if isinstance(v, L.C.c_void_p) else v  # noqa: E731
            self._gp_arrays = ((type(self._gpacks[0][0]) * n)(*[g[0] for g in self._gpacks]),
                               (L.C.c_void_p * n)(*[vp(g[1]) for g in self._gpacks]),
                               (L.C.c_void_p * n)(*[g[2].data_ptr() if g[2] is not None else None
                                                    for g in self._gpacks]),
                               (L.C.c_void_p * n)(*[g[3].data_ptr() if g[3] is not None else None
                                                    for g in self._gpacks]))
            self.unfused_packs.append(self._call("rn_conv_weight_pack_multi", *self._gp_arrays, n, sp))

    def _big_tile(self, op, mode, min_cols=None):
        """Does conv `op` run its forward (mode 0) / data gradient (mode 1) on a 256/224-row LDS-DMA
        tile of at least min_cols columns (the BN epilogue fusions run there; the fp64-accumulated
        variant on the 128/256-column tiles only)?"""
        if op.kind != "conv" or self.lib is None:
            return False
        if op.int8 and mode == 0:  # the int8 forward's tile (its dgrad is the bf16 one)
            x, y = op.x, op.y
            d = self._conv_desc(x.n, x.h, x.w, x.cp, x.c, y.c, op.kernel, op.stride, op.pad, op.groups)
            mc = min_cols if min_cols is not None else 128
            return int(self.lib.rn_conv_tile(L.C.byref(d), 2)) >= mc
        if min_cols is None:  # (64, the 64-column tile too -- RN_BN_FUSION_MIN_COLS -- measured 0.6 % slower per step)
            min_cols = 128
        x, y = op.x, op.y
        d = self._conv_desc(x.n, x.h, x.w, x.cp, x.c, y.c, op.kernel, op.stride, op.pad, op.groups)
        return int(self.lib.rn_conv_tile(L.C.byref(d), mode)) >= min_cols

    def _grouped_fuse(self, op, mode):
        """Does grouped conv `op` carry the BN fusion in its forward (mode 0: the statistics epilogue of
        the block-diagonal 256x64 tile) / data gradient (mode 1: the BN-backward reduction of that tile
        or of the direct kernel, rn_conv_bwd_data_bnred)?"""
        if op.kind != "conv" or op.groups <= 1 or self.lib is None or self.dtype != L.RN_BF16:
            return False
        x, y = op.x, op.y
        d = self._conv_desc(x.n, x.h, x.w, x.cp, x.c, y.c, op.kernel, op.stride, op.pad, op.groups)
        if mode == 1 and d.grouped_direct == 1:
            return True
        return int(self.lib.rn_conv_tile(L.C.byref(d), mode)) == 64

    def _depthwise(self, op):
        """Does conv `op` run the depthwise kernels (grouped_direct = 2)? They carry no BatchNorm fusion: the
        BatchNorm after a depthwise conv runs its own statistics pass and rn_bn_bwd, whatever the fusion
        switches say."""
        if op.kind != "conv" or op.groups <= 1 or self.lib is None:
            return False
        x, y = op.x, op.y
        d = self._conv_desc(x.n, x.h, x.w, x.cp, x.c, y.c, op.kernel, op.stride, op.pad, op.groups)
        return d.grouped_direct == 2

    def _conv_fwd_call(self, op, d, xptr, res, stats=True):
        """Conv forward; emits the next BatchNorm's statistics when one consumes y (training), and
        applies the producing BatchNorm+ReLU on load when that BN is fused (op.xf)."""
        sp = self._spv
        y = self._p(self.act(op.y))
        if op.int8:
            part = None
            if stats and op.bnstats:
                if op.part is None:
                    op.part_rows = int(self.lib.rn_conv_bn_part_rows(L.C.byref(d), 2))
                    op.part_blocks = -(-op.y.rows // op.part_rows)
                    op.part = self._zeros(op.part_blocks * 3 * op.y.cp, self.torch.float32)
                part = self._p(op.part)
                if op.want_mm:  # + per-block max / min of y for the quantizers that read bn(y)
                    if op.part_mm is None:
                        op.part_mm = self._zeros(op.part_blocks * op.y.cp, self.torch.float32)
                    sign = self._pp(op.mm_gamma) if op.mm_gamma else None
                    return self._call("rn_conv_fwd_i8_mm", L.C.byref(d), self._p(op.qsrc.codes), self._p(op.wk8),
                                      y, self.dtype, res, self._p(op.qsrc.unit), self._p(op.wunit), part,
                                      self._p(op.part_mm), sign, sp)
            return self._call("rn_conv_fwd_i8", L.C.byref(d), self._p(op.qsrc.codes), self._p(op.wk8), y,
                              self.dtype, res, self._p(op.qsrc.unit), self._p(op.wunit), part, sp)
        sc, sh = (op.xf.sc, op.xf.sh) if op.xf is not None else (None, None)
        part = None
        if stats and op.bnstats:
            if op.part is None:
                op.part_blocks = int(self.lib.rn_conv_bnstats_blocks(L.C.byref(d)))
                op.part_rows = int(self.lib.rn_conv_bn_part_rows(L.C.byref(d), 0))
                op.part = self._zeros(op.part_blocks * 3 * op.y.cp, self.torch.float32)
            part = self._p(op.part)
        if sc is None and part is None:
            return self._call("rn_conv_fwd", L.C.byref(d), xptr, self._p(op.wk), y, self.dtype, res, None, sp)
        return self._call("rn_conv_fwd_x", L.C.byref(d), xptr, self._p(op.wk), y, self.dtype, res, None, sc, sh,
                          part, sp)

    def _stem_chunks(self, op, dy):
        """Image chunks of the stem's BN-backward apply + weight gradient (RN_STEM_CHUNKS, default 4;
        1 = one rn_bn_bwd and one wgrad): the NHWC4 stem, or the int8 stem's NHWC-8 image with the clip
        masks (rn_stem_clip_wgrad_chunk), with a side stream, whose output gradient is the dx of the
        rn_bn_bwd call just emitted (no add operand, no paired gradient)."""
        nch = int(os.environ.get("RN_STEM_CHUNKS", "4"))
        side = self._side_stream is not None or (self.dry_run and os.environ.get("RN_WGRAD_STREAM", "1") == "1")
        if nch <= 1 or not (op.p4 or self._stem_clip_mask(op)) or not side or dy is None or op.dfull.n % nch or \
                not self._bwd:
            return 1
        name, _, args = self._bwd[-1]
        # (rn_bn_bwd_part: the pool backward reduced the BN, rn_pool_bwd_bnred)
        dx, add = (args[3], args[4]) if name == "rn_bn_bwd" else (args[5], args[6]) if name == "rn_bn_bwd_part" \
            else (None, None)
        if dx is None or add is not None:
            return 1
        bn = args[0]._obj
        if bn.dy2 or bn.c != op.dfull.k_pad or bn.m != op.dfull.n * op.dfull.p * op.dfull.q or \
                dx.value != self._p(dy).value:
            return 1
        return nch

    def _weight_source(self, op):
        """Quantization_int8 on a weight (int8_api.py:131-132): the compute copies are packed from a
        fake-quantized fp32 copy of the master, refreshed with every repack; the STE passes the
        gradient to the master unchanged."""
        q = op.qweight
        n = int(np.prod(self.plan.param_shape(op.weight)))
        op.qw = self._zeros(n, self.torch.float32)
        if op.int8:  # also keeps the unit for the int8 codes of the forward copy
            op.wunit = self._zeros(1, self.torch.float32)
        if q.get("family") == "gdrq":
            # a GDRQ weight (core/operator/GDRQ.py: alpha = ktimes * mean|w| unless fix_alpha, clip, round; plain
            # STE): always through the batched rn_weight_gdrq_pack, built after the forward
            self._wg_ops.append(op)
            return self._p(op.qw)
        if q.get("family") == "qil":
            # a QIL weight (core/operator/QIL.py): always through the batched rn_weight_qil_pack, built after the
            # forward; its backward rewrites the weight gradient (_wqil_bwd)
            self._wl_ops.append(op)
            return self._p(op.qw)
        if self._wq_batch:
            # one batched rn_weight_quant_pack for every weight quantizer (built after the forward):
            # the fake-quantized copy, and for the int8 convs their codes and data-gradient copy too
            self._wq_ops.append(op)
            return self._p(op.qw)
        if op.int8:
            c = self._call("rn_quant_int8_fwd_codes", F32, n, self._pp(op.weight), self._p(op.qw), None,
                           self._p(op.wunit), self._ap(q["minmax"]), 1, 1, q["ema"], 0, q["nbits"], self._qwsp,
                           self._spv)
        else:
            c = self._call("rn_quant_int8_fwd", F32, n, self._pp(op.weight), self._p(op.qw),
                           self._ap(q["minmax"]), 1, 1, q["ema"], 0, q["nbits"], self._qwsp, self._spv)
        self.packs.append(c)
        self.unfused_packs.append(c)
        return self._p(op.qw)

    def _add_pack(self, op, d, wk, wc):
        """Compute copies of op's weight. Dense weights packed straight from the master are
        rewritten by the fused SGD kernel (rn_sgd_mom_update_pack); the bind-time pack below also
        writes their zero padding, which that kernel never touches."""
        c = self._call("rn_conv_weight_pack", L.C.byref(d), op.wsrc, self._p(wk), self._p(wc), self._spv)
        self.packs.append(c)
        if d.groups == 1 and not op.qweight:
            self.fused_packs[op.weight] = (wk.data_ptr() if wk is not None else 0,
                                           wc.data_ptr() if wc is not None else 0,
                                           d.k, d.r * d.s, d.c_real, d.c, d.k_pad)
        elif d.groups > 1 and self._gpack_batch:
            self._gpacks.append((d, op.wsrc, wk, wc))  # -> one rn_conv_weight_pack_multi
        else:
            self.unfused_packs.append(c)

    # ------------------------------------------------------------------ backward
    def _wgrad_call(self, d, x, dy, dw):
        """rn_conv_bwd_filter, through the split-M slab workspace where the kernel uses one."""
        if self.wgrad_ws is not None and int(self.lib.rn_conv_wgrad_ws_bytes(L.C.byref(d))) > 0:
            return self._call("rn_conv_bwd_filter_ws", L.C.byref(d), x, dy, dw, self._p(self.wgrad_ws),
                              self.wgrad_ws_bytes, self._spv)
        return self._call("rn_conv_bwd_filter", L.C.byref(d), x, dy, dw, self._spv)

    # the recomputed BN backward's size gate: measured cold per layer, the recomputed chain wins from
    # 98 MiB up on both layer classes (stage 1's from 25 MiB) and loses or ties below (stage 2's class at 49 MiB: 2 %
    # slower; both at 12 MiB and less)
    RECOMPUTE_MIN_BYTES = 64 << 20

    def _bn_recompute_ok(self, op, cop, cadd, min_bytes):
        """May the BatchNorm `op`, whose output gradient the data gradient of conv `cop` completes, take its
        backward from a recomputed dgrad (rn_conv_bwd_data_bnapply)? Where that dgrad is the streaming kernel
        (rn_conv_dgrad_streamed: the pre-activation units' conv1 of stages 1 and 2, symbol/resnet.py:17-20, a 1x1
        reduction over 64 or 128 channels into 4x as many) and the only writer of the gradient (no fan-in add: the
        reduction-only pass takes none). On the 224-row tiles (stages 3 and 4) the stored path is faster. Only
        where the gradient that is then never stored has at least `min_bytes` (None: never): a small one comes back
        from the caches and the stored path measured as fast or faster."""
        d = cop.desc
        return (min_bytes is not None and op.y.numel * 2 >= min_bytes
                and self.dtype == L.RN_BF16 and cadd is None and not op.desc.clip and op.y.c == d.c and cop.x is op.y
                and int(self.lib.rn_conv_dgrad_streamed(L.C.byref(d))) == 1
                and int(self.lib.rn_conv_tile(L.C.byref(d), 1)) >= 128)

    def _quant_groups(self):
        """{id(bn): (bn, [quant ops])} for the BatchNorm+ReLU outputs that only activation quantizers
        (Quantization_int8 of data, the int8 graph) read -- one, or two (symbol/resnet_int8.py: a stage's
        first unit quantizes act1 for conv1 and for the shortcut conv). Their straight-through backwards
        (zero where the input is >= the moving threshold, clip_grad_quantization_int8.py) fold into that
        BN's backward (rn_bn_desc.clip, and clip2 / dy2 for the second), so the quantizers cost no
        backward pass, and their forwards apply the BN on load (rn_quant_int8_fwd_codes_bn[2]): the BN
        output is never written. RN_QUANT_BWD_FOLD=0: separate rn_quant_int8_bwd passes."""
        if os.environ.get("RN_QUANT_BWD_FOLD", "1") != "1":
            return {}
        ops = self.plan.ops
        readers, qreaders = {}, {}
        for o in ops:
            for k in ("x", "a", "b", "res", "label"):
                t = getattr(o, k, None)
                if isinstance(t, TensorSpec):
                    readers[id(t)] = readers.get(id(t), 0) + 1
                    if o.kind == "quant" and k == "x" and not o.q.get("is_weight"):
                        qreaders.setdefault(id(t), []).append(o)
        outs = {id(t) for t in self.plan.outputs}
        groups = {}
        for bn in ops:
            if bn.kind != "bn" or not bn.relu or id(bn.y) in outs or bn.apply_fused:
                continue
            qs = qreaders.get(id(bn.y), [])
            if qs and len(qs) == readers.get(id(bn.y)) and len(qs) <= 2:
                groups[id(bn)] = (bn, qs)
        return groups

    def _build_backward(self):
        """The setup passes, then one _bwd_<kind>(op, dy, gs) per op in reverse plan order, dy the op's output
        gradient and gs the gradient routing."""
        gs = _GradState(self)
        self.param_done_at = {}  # param -> index in self._bwd after which its grad is final
        self._gw = {}  # id(tensor) -> last writer of its gradient buffer: ("dgrad", call index, conv op)
        self._pact_ws = None  # rn_pact_bwd's block partials: one buffer for every PACT (compute stream, plan order)
        self._qil_ws = None  # rn_qil_bwd's, likewise
        self._wqil_ws = None  # rn_weight_qil_bwd's: the weight gradients' stream, plan order
        self._bind_quant_folds()
        self._read_bn_bwd_modes()
        self._size_wgrad_ws()  # (before every binder: they pass the slab, or test for it)
        self._bwd_stem_clip_masks()  # (first in self._bwd: depends on the forward only, SIDE_PRE_CALLS)
        for op in reversed(self.plan.ops):
            if op.kind == "softmax":
                gs.has_value.add(id(op.x))  # dlogits written by the forward softmax call
                continue
            dy = self._qpair_dy(op, gs) if op.kind == "bn" and op.qpair else gs.read(op.y)
            if dy is not None:
                getattr(self, "_bwd_" + op.kind)(op, dy, gs)
            dy = None  # (a recomputed BatchNorm releases its output gradient's buffer: no name here keeps it)
        self._gw = {}  # (the writer records hold gradient tensors and serve only while the plan is bound)

    def _bind_quant_folds(self):
        """The quantizers whose backward folds into a BatchNorm's (_quant_groups): self._folds {id(quant op): bn},
        and a single quantizer's threshold into its BN's descriptor -- which the forward calls already hold by
        reference."""
        groups = self._quant_groups()
        self._folds = {id(q): bn for bn, qs in groups.values() for q in qs}
        for op in self.plan.ops:
            if op.kind == "bn":
                op.qpair = False
                op.qorder = []  # the folded quantizers in backward order (their gradients' pending order)
                op.pre_part = None  # set by the residual add's fused ReLU backward (this build)
                op.recomputed = False  # its backward applied by a recomputed dgrad (rn_conv_bwd_data_bnapply)
        for bn, qs in groups.values():
            if len(qs) == 1:
                bn.desc.clip = self._ap(qs[0].q["minmax"]).value  # (the threshold the forward just updated)
            else:
                bn.qpair = True  # clip / clip2 / dy2 set where its backward is bound (_qpair_dy)

    def _read_bn_bwd_modes(self):
        # default on where the dgrad runs the 256-row tile (see RN_BN_EPILOGUE_STATS; =2: every dgrad)
        self._bwd_fusion = os.environ.get("RN_BN_BWD_FUSION", "1") in ("1", "2")
        self._bwd_all = os.environ.get("RN_BN_BWD_FUSION", "1") == "2"
        # the BN backward applied by a recomputed streamed dgrad (rn_conv_bwd_data_bnapply, _bn_recompute_ok):
        # RN_BN_BWD_RECOMPUTE=0 keeps the stored gradient everywhere, 1 recomputes every such layer whatever its
        # size, unset those of at least RECOMPUTE_MIN_BYTES (DESIGN.md has the measurements)
        rmode = os.environ.get("RN_BN_BWD_RECOMPUTE", "")
        if rmode not in ("", "0", "1"):
            raise L.RNError("RN_BN_BWD_RECOMPUTE=%r: 0, 1 or unset" % rmode)
        self._recompute_min_bytes = {"": self.RECOMPUTE_MIN_BYTES, "0": None, "1": 0}[rmode]
        # (removed in round 6, measured neutral, its kernel kept and kernel-tested by tests/test_kernels_gpu.py::
        # test_dgrad_quant_pair_clip_fold: a quantizer pair's clips folded into the later data gradient,
        # RN_QUANT_PAIR_FUSION -- rn_conv_bwd_data_bnred_clip2; C5 22.68 / 22.69 vs 22.69 / 22.68 ms)

    def _wgrad_ws_need(self):
        """Bytes of split-M slab workspace the largest weight gradient needs under the current grid split."""
        ops = self.plan.ops
        need = [int(self.lib.rn_conv_wgrad_ws_bytes(L.C.byref(op.desc))) for op in ops
                if op.kind in ("conv", "fc") and op.desc is not None]
        # (the stem's weight gradient; it needs a slab only in the deterministic mode)
        need += [int(self.lib.rn_conv_wgrad_ws_bytes(L.C.byref(op.dfull))) for op in ops
                 if op.kind == "stem" and not op.p4]
        need += [int(self.lib.rn_stem_clip_wgrad_ws_bytes(L.C.byref(op.dfull))) for op in ops
                 if op.kind == "stem" and self._stem_clip_mask(op)]
        need += [int(self.lib.rn_conv_wgrad_i8_ws_bytes(L.C.byref(op.desc))) for op in ops
                 if op.kind == "conv" and op.qsrc is not None and op.qsrc.codes_wgrad]
        return max(need + [0])

    def _size_wgrad_ws(self):
        """One workspace for the weight gradients' split-M partial tiles (rn_conv_bwd_filter_ws),
        sized for the largest layer. Shared safely because every call using it is a weight-gradient
        call, and those all run in plan order on ONE stream (the side stream when it is on:
        _route_wgrads enforces this). None where no layer needs a slab."""
        self.wgrad_ws = None
        # sized for both weight-gradient grids: the overlapped one (part of the chip) and the whole
        # chip, which a serialised step (side_enabled False: bench.py's calibration) runs with
        self.wgrad_ws_bytes = self._wgrad_ws_need()
        if os.environ.get("RN_WGRAD_STREAM", "1") == "1":
            L.set_wgrad_split(False)
            self.wgrad_ws_bytes = max(self.wgrad_ws_bytes, self._wgrad_ws_need())
            L.set_wgrad_split(True, self.wgrad_split_pct)
        if self.wgrad_ws_bytes > 0:
            self.wgrad_ws = self._zeros(self.wgrad_ws_bytes // 4, self.torch.float32)

    def _wgrad_ws_args(self, use=True):
        """(workspace pointer, bytes) operands of the weight gradients that take the slab as an option."""
        return (self._p(self.wgrad_ws), self.wgrad_ws_bytes) if use and self.wgrad_ws is not None else (None, 0)

    def _bwd_stem_clip_masks(self):
        for op in self.plan.ops:
            if op.kind == "stem" and self._stem_clip_mask(op):
                # the int8 stem's clip masks into the NHWC-8 image's free channels (rn_stem_clip_mask),
                # first on the weight-gradient stream: its clip gradient then rides in the stem's weight
                # gradient (rn_stem_clip_wgrad / rn_stem_clip_dbeta) instead of a gather at the step's end
                _, _, sc, sh = op.bn_ptrs
                op.clip_ext = self._zeros(op.dfull.k * op.dfull.r * op.dfull.s * 2 * op.dfull.c_real,
                                          self.torch.float32)
                self._bwd.append(self._call("rn_stem_clip_mask", L.C.byref(op.dfull), self._in_ptr, sc, sh,
                                            self._ap(op.quant["minmax"]), self._p(op.x8), self._spv))

    def _qpair_dy(self, op, gs):
        """The output gradient of a BatchNorm with two folded quantizers: their gradients stay separate (dy,
        rn_bn_desc.dy2), the thresholds go into the descriptor the forward calls hold by reference."""
        assert id(op.y) not in gs.has_value
        pend = gs.pending.pop(id(op.y), [])
        if not pend:
            return None
        op.desc.clip = self._ap(op.qorder[0].q["minmax"]).value
        if len(pend) == 2:
            op.desc.clip2 = self._ap(op.qorder[1].q["minmax"]).value
            op.desc.dy2 = self._p(pend[1]).value
        return pend[0]

    def _wqil_bwd(self, op):
        """The backward of a QIL weight quantizer, right after the weight gradient of op (KRSC, as the master) and on
        its stream: dw *= alpha * [p <= |w| <= c] * [w != 0] in place, and the gradients of its pruning and clipping
        points; gamma's stays the zero the backward starts from. Before the gradient's bucket is final."""
        q = op.qweight
        if not q or q.get("family") != "qil":
            return
        if self._wqil_ws is None:  # (one buffer, made by the first weight that needs it)
            nmax = max(int(np.prod(self.plan.param_shape(o.weight))) for o in self._wl_ops)
            self._wqil_ws = self._zeros(int(self.lib.rn_qil_bwd_ws_bytes(nmax)) // 4, self.torch.float32)
        n = int(np.prod(self.plan.param_shape(op.weight)))
        self._bwd.append(self._call("rn_weight_qil_bwd", n, self._pp(op.weight), self._gp(op.weight),
                                    self._pp(q["prune"]), self._pp(q["clip"]), self._gp(q["prune"]),
                                    self._gp(q["clip"]), self._p(self._wqil_ws), self._spv))
        for nm in (q["prune"], q["clip"], q["gamma"]):
            self.param_done_at[nm] = len(self._bwd)

    def _bwd_fc(self, op, dy, gs):
        x = op.x
        self._bwd.append(self._wgrad_call(op.desc, self._p(self.act(x)), self._p(dy), self._gp(op.weight)))
        self._wqil_bwd(op)
        if op.bias:
            self._bwd.append(self._call("rn_col_sum", self.dtype, x.n, op.nh, _pad8(op.nh), self._p(dy),
                                        self._gp(op.bias), 0, self._spv))
            self.param_done_at[op.bias] = len(self._bwd)
        self.param_done_at[op.weight] = len(self._bwd)
        if x.needs_grad:
            out, add = gs.contribute(x)
            self._bwd.append(self._call("rn_conv_bwd_data", L.C.byref(op.desc), self._p(dy), self._p(op.wc),
                                        self._p(out), self._p(add), self._spv))

    def _bwd_conv(self, op, dy, gs):
        x, sp = op.x, self._spv
        if op.xf is not None:  # input = BN+ReLU(bn input), applied on load
            ws = int(self.lib.rn_conv_wgrad_ws_bytes(L.C.byref(op.desc))) > 0
            self._bwd.append(self._call("rn_conv_bwd_filter_x", L.C.byref(op.desc), self._p(self.act(op.xf.x)),
                                        self._p(dy), self._gp(op.weight), op.xf.sc, op.xf.sh,
                                        *self._wgrad_ws_args(ws), sp))
        elif op.qsrc is not None and op.qsrc.codes_wgrad:  # the input's codes, x its unit
            q = op.qsrc
            self._bwd.append(self._call("rn_conv_bwd_filter_i8", L.C.byref(op.desc), self._p(q.codes), self._p(q.unit),
                                        self._p(dy), self._gp(op.weight), *self._wgrad_ws_args(), sp))
        else:
            self._bwd.append(self._wgrad_call(op.desc, self._p(self.act(x)), self._p(dy), self._gp(op.weight)))
        self._wqil_bwd(op)
        self.param_done_at[op.weight] = len(self._bwd)
        if x.needs_grad:
            out, add = gs.contribute(x)
            self._bwd.append(self._call("rn_conv_bwd_data", L.C.byref(op.desc), self._p(dy), self._p(op.wc),
                                        self._p(out), self._p(add), sp))
            self._gw[id(x)] = ("dgrad", len(self._bwd) - 1, op, dy, out, add)
        if op.res is not None and op.res.needs_grad:
            gs.alias(op.res, dy)

    def _bwd_stem_chunked(self, op, dy, nch):
        """The stem BN's dx (= dy here) per image chunk, each chunk's weight gradient (side
        stream) starting as soon as its rows are applied: only the last chunk's wgrad
        stays on the step's critical path (rn_bn_bwd then reduces + finalizes only)."""
        sp = self._spv
        bname, bfn, bargs = self._bwd[-1]
        if bname == "rn_bn_bwd":
            self._bwd[-1] = (bname, bfn, bargs[:3] + (None,) + bargs[4:])
        else:  # rn_bn_bwd_part: finalize only, its coefficients where rn_bn_bwd_apply_rows reads
            # them (after the reduction partials of rn_bn_bwd's own layout in the workspace)
            bd, part, nrb, xp_, dyp_, dxp_, _, gp_, smp, sip, scp, shp, dgp, dbp, wsp_, _ = bargs
            coef = wsp_.value + 4 * 2 * int(self.lib.rn_bn_reduce_blocks(bd)) * bd._obj.c
            self._bwd[-1] = self._call("rn_bn_bwd_finalize", bd, part, nrb, gp_, smp, sip, dgp, dbp,
                                       L.C.c_void_p((coef + 15) // 16 * 16), sp)
            bargs = (bd, xp_, dyp_, dxp_, None, gp_, smp, sip, scp, shp, dgp, dbp, wsp_, sp)
        d = op.dfull
        nc = d.n // nch
        rows = nc * d.p * d.q
        for i in range(nch):
            dc = self._conv_desc(nc, d.h, d.w, d.c, d.c_real, d.k, (d.r, d.s), (d.stride_h, d.stride_w),
                                 (d.pad_h, d.pad_w))
            self._descs.append(dc)
            self._bwd.append(self._call("rn_bn_bwd_apply_rows", bargs[0], bargs[1], bargs[2], bargs[3],
                                        None, bargs[8], bargs[9], bargs[12], i * rows, rows, sp))
            dyc = L.C.c_void_p(self._p(dy).value + i * rows * d.k_pad * 2)
            if op.p4:
                hp, wp = op.p4
                self._bwd.append(self._call("rn_stem_conv_wgrad_p4", L.C.byref(dc),
                    L.C.c_void_p(op.x8.data_ptr() + i * nc * hp * wp * 4 * 2), dyc, self._gp(op.weight), hp, wp, sp))
            else:  # the int8 stem: NHWC-8 chunks, clip masks in channels c_real..
                self._bwd.append(self._call("rn_stem_clip_wgrad_chunk", L.C.byref(dc),
                    L.C.c_void_p(op.x8.data_ptr() + i * nc * d.h * d.w * 8 * 2), dyc, self._gp(op.weight),
                    self._p(op.clip_ext), *self._wgrad_ws_args(), int(i == 0), int(i == nch - 1), sp))

    def _bwd_stem(self, op, dy, gs):
        sp = self._spv
        nch = self._stem_chunks(op, dy)
        if nch > 1:
            self._bwd_stem_chunked(op, dy, nch)
        elif op.p4:
            self._bwd.append(self._call("rn_stem_conv_wgrad_p4", L.C.byref(op.dfull), self._p(op.x8),
                                        self._p(dy), self._gp(op.weight), op.p4[0], op.p4[1], sp))
        elif self._stem_clip_mask(op):
            self._bwd.append(self._call("rn_stem_clip_wgrad", L.C.byref(op.dfull), self._p(op.x8), self._p(dy),
                                        self._gp(op.weight), self._p(op.clip_ext), *self._wgrad_ws_args(), sp))
        else:
            self._bwd.append(self._wgrad_call(op.dfull, self._p(op.x8), self._p(dy), self._gp(op.weight)))
        self._wqil_bwd(op)
        self.param_done_at[op.weight] = len(self._bwd)
        if op.bn:
            self._bwd.append(self._call("rn_stem_shift_grad", L.C.byref(op.dfull), self._p(dy),
                                        op.wsrc, self._gp(op.bn["beta"]), self._p(self.stem_ws), sp))
            if op.quant and self._stem_clip_mask(op):
                self._bwd.append(self._call("rn_stem_clip_dbeta", L.C.byref(op.dfull), self._p(op.clip_ext),
                                            op.wsrc, self._gp(op.bn["beta"]), sp))
            elif op.quant:
                _, _, sc, sh = op.bn_ptrs
                self._bwd.append(self._call("rn_stem_quant_clip_grad", L.C.byref(op.dfull), self._in_ptr, sc, sh,
                                            self._ap(op.quant["minmax"]),
                                            self._p(dy), op.wsrc, self._gp(op.bn["beta"]), sp))
            self.param_done_at[op.bn["beta"]] = len(self._bwd)
            self.param_done_at[op.bn["gamma"]] = len(self._bwd)

    def _bn_bwd_part_call(self, op, part, nblocks, dy, out, add):
        """rn_bn_bwd_part: finalize + apply over a reduction another kernel left in `part`."""
        return self._call("rn_bn_bwd_part", L.C.byref(op.desc), self._p(part), nblocks, self._p(self.act(op.x)),
                          self._p(dy), self._p(out), self._p(add), self._pp(op.gamma), op.sm, op.si, op.sc, op.sh,
                          self._gp(op.gamma), self._gp(op.beta), self._wsp, self._spv)

    def _bwd_bn(self, op, dy, gs):
        x, sp = op.x, self._spv
        out, add = (gs.contribute(x) if x.needs_grad else (None, None))
        w = self._gw.get(id(op.y))
        # (may the kernel that completed dy, a conv dgrad or a pooling backward, carry this BN's reduction?)
        fusable = bool(self._bwd_fusion and not op.desc.dy2 and w and w[0] in ("dgrad", "pool") and dy is w[4])
        if op.use_global_stats:
            # moving statistics are constants of the graph (fix_bn): dx = gamma*invstd*dz
            self._bwd.append(self._call("rn_bn_bwd_global", L.C.byref(op.desc), self._p(self.act(x)), self._p(dy),
                                        self._p(out), self._p(add), self._pp(op.gamma), self._ap(op.mean),
                                        self._ap(op.var), op.sc, op.sh,
                                        self._gp(op.gamma), self._gp(op.beta), self._wsp, sp))
        elif fusable and w[0] == "dgrad" and \
                op.y.c % 8 == 0 and op.y.c == op.y.cp and \
                (self._bwd_all or self._big_tile(w[2], 1) or self._grouped_fuse(w[2], 1)) and \
                not self._depthwise(w[2]) and \
                (not op.desc.clip or self._big_tile(w[2], 1)):  # (the clip: bf16 LDS-DMA tiles)
            self._bwd_bn_from_dgrad(op, dy, out, add, w)
        elif fusable and not op.desc.clip and w[0] == "pool" and \
                op.y.c == op.y.cp and self.dtype == BF16 and \
                int(self.lib.rn_pool_bwd_bnred_blocks(L.C.byref(w[2].desc))) > 0:
            # the max-pool backward that completes this BN's output gradient (the stem's bn0 ->
            # relu0 -> pool0) also reduces its backward; the BN then needs only finalize + apply
            _, pi, pop, pdy, pout, padd = w
            op.bnred_blocks = int(self.lib.rn_pool_bwd_bnred_blocks(L.C.byref(pop.desc)))
            op.bnred = self._zeros(op.bnred_blocks * op.y.cp * 2, self.torch.float32)
            self._bwd[pi] = self._call("rn_pool_bwd_bnred", L.C.byref(pop.desc), self._p(pdy), self._p(pop.argmax),
                                       self._p(pout), self._p(padd), self._p(self.act(x)), op.sm, op.sc, op.sh,
                                       int(op.relu), self._p(op.bnred), sp)
            self._bwd.append(self._bn_bwd_part_call(op, op.bnred, op.bnred_blocks, dy, out, add))
        elif op.pre_part is not None and not op.desc.dy2:
            # the reduction was done by the residual add's ReLU backward (rn_relu_bwd_bnred)
            self._bwd.append(self._bn_bwd_part_call(op, op.pre_part, op.pre_nrb, dy, out, add))
        else:
            self._bwd.append(self._call("rn_bn_bwd", L.C.byref(op.desc), self._p(self.act(x)), self._p(dy),
                                        self._p(out), self._p(add), self._pp(op.gamma), op.sm, op.si, op.sc,
                                        op.sh, self._gp(op.gamma), self._gp(op.beta), self._wsp, sp))
        self.param_done_at[op.gamma] = len(self._bwd)
        self.param_done_at[op.beta] = len(self._bwd)

    def _bwd_bn_from_dgrad(self, op, dy, out, add, w):
        """The conv dgrad that completes this BN's output gradient also reduces its backward
        (sum dz, sum dz*(x - mean)); the BN then needs only finalize + apply. `w`: that dgrad's writer record."""
        x, sp = op.x, self._spv
        _, ci, cop, cdy, cout, cadd = w
        op.bnred_blocks = int(self.lib.rn_conv_bnred_blocks(L.C.byref(cop.desc)))
        op.bnred = self._zeros(op.bnred_blocks * op.y.cp * 2, self.torch.float32)
        if self._bn_recompute_ok(op, cop, cadd, self._recompute_min_bytes):
            # pass 1 only reduces (the BN-width gradient is never written), finalize, then the same
            # dgrad recomputed with the BN backward applied in its epilogue (bit-identical)
            op.coef = self._zeros(4 * op.y.cp, self.torch.float32)
            self._bwd[ci] = self._call("rn_conv_bwd_data_bnred", L.C.byref(cop.desc), self._p(cdy), self._p(cop.wc),
                                       None, None, self._p(self.act(x)), op.sm, op.sc,
                                       op.sh, int(op.relu), self._p(op.bnred), sp)
            self._bwd.append(self._call("rn_bn_bwd_finalize", L.C.byref(op.desc), self._p(op.bnred), op.bnred_blocks,
                                        self._pp(op.gamma), op.sm, op.si,
                                        self._gp(op.gamma), self._gp(op.beta), self._p(op.coef), sp))
            self._bwd.append(self._call("rn_conv_bwd_data_bnapply", L.C.byref(cop.desc), self._p(cdy), self._p(cop.wc),
                                        self._p(out), self._p(add), self._p(self.act(x)),
                                        self._p(op.coef), op.sc, op.sh, int(op.relu), sp))
            # the gradient of the BN's output is never stored: the buffer bound for it when conv1's data
            # gradient was planned is released here (this dgrad was its only writer, the BN its only
            # reader; no bound call holds its pointer any more) -- every reference: the buffer table and
            # the writer record here, the binders' own names as they return (nothing is allocated in between)
            assert self._grads.get(id(cop.x)) is cout
            del self._grads[id(cop.x)]
            self._gw[id(op.y)] = ("other",)
            op.recomputed = True
            return
        if op.desc.clip:  # (a folded quantizer straight-through clip)
            self._bwd[ci] = self._call("rn_conv_bwd_data_bnred_clip", L.C.byref(cop.desc), self._p(cdy),
                                       self._p(cop.wc), self._p(cout), self._p(cadd), self._p(self.act(x)), op.sm,
                                       op.sc, op.sh, int(op.relu), L.C.c_void_p(op.desc.clip), self._p(op.bnred), sp)
        else:
            self._bwd[ci] = self._call("rn_conv_bwd_data_bnred", L.C.byref(cop.desc), self._p(cdy), self._p(cop.wc),
                                       self._p(cout), self._p(cadd), self._p(self.act(x)), op.sm, op.sc, op.sh,
                                       int(op.relu), self._p(op.bnred), sp)
        self._bwd.append(self._bn_bwd_part_call(op, op.bnred, op.bnred_blocks, dy, out, add))

    def _bwd_affine(self, op, dy, gs):
        """The global-statistics BN backward with mean 0, variance 1, eps 0: dz = dy*[y > 0],
        dscale = sum(dz*x), dbias = sum(dz), dx = scale*dz."""
        x = op.x
        out, add = (gs.contribute(x) if x.needs_grad else (None, None))
        if op.gamma is None or op.beta is None:
            op.gscratch = self._zeros(x.cp, self.torch.float32)
        dg = self._gp(op.gamma) if op.gamma is not None else self._p(op.gscratch)
        db = self._gp(op.beta) if op.beta is not None else self._p(op.gscratch)
        self._bwd.append(self._call("rn_bn_bwd_global", L.C.byref(op.desc), self._p(self.act(x)), self._p(dy),
                                    self._p(out), self._p(add), op.sc, op.zero, op.one,
                                    op.sc, op.sh, dg, db, self._wsp, self._spv))
        for nm in (op.gamma, op.beta):
            if nm is not None:
                self.param_done_at[nm] = len(self._bwd)

    def _bwd_quant(self, op, dy, gs):
        if op.x.needs_grad and id(op) in self._folds:
            # straight-through: the gradient passes unchanged to the BN output, whose backward
            # applies the clip; the conv that wrote dy stays its last writer (BN reduction fusion)
            gs.alias(op.x, dy)
            bn = self._folds[id(op)]
            bn.qorder.append(op)
            if bn.qpair:
                self._gw[id(op.x)] = ("other",)
            elif id(op.y) in self._gw:
                self._gw[id(op.x)] = self._gw[id(op.y)]
        elif op.x.needs_grad:
            out, add = gs.contribute(op.x)
            self._bwd.append(self._call("rn_quant_int8_bwd", self.dtype, op.x.numel, self._p(self.act(op.x)),
                                        self._p(dy), self._p(out), self._ap(op.q["minmax"]), 0, self._p(add),
                                        self._spv))

    def _bwd_pact(self, op, dy, gs):
        """dx = dy * [x < gamma] and dgamma = sum dy * [x >= gamma] in one pass (+ the ordered sum of its
        block partials, which writes the gradient). This call is the last writer of x's gradient and
        fuses no BatchNorm reduction: the BatchNorm that produced x runs its own rn_bn_bwd."""
        if self._pact_ws is None:  # (one buffer, made by the first op that needs it)
            nmax = max(o.x.numel for o in self.plan.ops if o.kind == "pact")
            self._pact_ws = self._zeros(int(self.lib.rn_pact_bwd_ws_bytes(nmax)) // 4, self.torch.float32)
        if op.x.needs_grad:
            out, add = gs.contribute(op.x)
            self._gw[id(op.x)] = ("other",)
        else:  # (no consumer of dx: a scratch buffer takes it)
            out, add = self._zeros(op.x.numel, self.tdtype), None
            self._grads[("pact_dx", id(op))] = out
        self._bwd.append(self._call("rn_pact_bwd", self.dtype, op.x.numel, self._p(self.act(op.x)), self._p(dy),
                                    self._pp(op.gamma), self._p(out), self._p(add),
                                    self._gp(op.gamma), self._p(self._pact_ws), self._spv))
        self.param_done_at[op.gamma] = len(self._bwd)

    def _bwd_gdrq(self, op, dy, gs):
        """dx = dy * [|x| <= alpha], the boundary included (rn_gdrq_bwd; the BatchNorm-folded clip and
        rn_quant_int8_bwd exclude it), with the alpha the forward left. alpha has no gradient. As for
        PACT this call is the last writer of x's gradient and fuses no BatchNorm reduction."""
        if op.x.needs_grad:
            out, add = gs.contribute(op.x)
            self._gw[id(op.x)] = ("other",)
            self._bwd.append(self._call("rn_gdrq_bwd", self.dtype, op.x.numel, self._p(self.act(op.x)),
                                        self._p(dy), self._ap(op.alpha), self._p(out), self._p(add), self._spv))

    def _bwd_qil(self, op, dy, gs):
        """dx = dy * alpha over p <= |x| <= c, x != 0, and the gradients of the pruning and clipping points in one
        pass (+ the ordered sums of its block partials, which write them); gamma's stays zero. As for PACT this
        call is the last writer of x's gradient and fuses no BatchNorm reduction."""
        if self._qil_ws is None:  # (one buffer, made by the first op that needs it)
            nmax = max(o.x.numel for o in self.plan.ops if o.kind == "qil")
            self._qil_ws = self._zeros(int(self.lib.rn_qil_bwd_ws_bytes(nmax)) // 4, self.torch.float32)
        if op.x.needs_grad:
            out, add = gs.contribute(op.x)
            self._gw[id(op.x)] = ("other",)
        else:  # (no consumer of dx: a scratch buffer takes it)
            out, add = self._zeros(op.x.numel, self.tdtype), None
            self._grads[("qil_dx", id(op))] = out
        self._bwd.append(self._call("rn_qil_bwd", self.dtype, op.x.numel, self._p(self.act(op.x)), self._p(dy),
                                    self._pp(op.prune), self._pp(op.clip), self._p(out), self._p(add),
                                    self._gp(op.prune), self._gp(op.clip), self._p(self._qil_ws), self._spv))
        for nm in (op.prune, op.clip, op.qgamma):
            self.param_done_at[nm] = len(self._bwd)

    def _bwd_relu(self, op, dy, gs):
        if op.x.needs_grad:
            out, add = gs.contribute(op.x)
            self._bwd.append(self._call("rn_relu_bwd", op.y.numel, self.dtype, self._p(self.act(op.y)),
                                        self._p(dy), self._p(out), self._p(add), self._spv))

    def _bwd_add(self, op, dy, gs):
        g = dy
        if op.relu:
            # held by the executor: the bound call keeps only the raw pointer (a dropped
            # tensor would be recycled by the caching allocator while the plan writes it)
            gbuf = self._zeros(op.y.numel, self.tdtype)
            self._grads[("relu_add", id(op))] = gbuf
            # the BatchNorms applied inside this add (rn_bn_apply_add) get their backward
            # reductions from the same pass (rn_relu_bwd_bnred)
            inside = [b for b in (op.bn_a, op.bn_b) if b is not None]
            bns = [b for b in inside if not b.use_global_stats]
            # (round 4's opt-in RN_RELU_BNRED_DGRAD -- this pass in the next unit's conv1 data-gradient
            # epilogue -- measured 3 % slower on C4 and was removed in round 5: the epilogue streamed
            # its extra tensors at ~3.5 TB/s, this pass runs at ~5.5)
            if bns and len(bns) == len(inside):
                for b in bns:
                    b.pre_nrb = int(self.lib.rn_bn_reduce_blocks(L.C.byref(b.desc)))
                    b.pre_part = self._zeros(b.pre_nrb * b.x.cp * 2, self.torch.float32)
                b2 = bns[1] if len(bns) == 2 else None
                self._bwd.append(self._call("rn_relu_bwd_bnred", L.C.byref(bns[0].desc), self._p(self.act(op.y)),
                    self._p(dy), self._p(gbuf), self._p(self.act(bns[0].x)), bns[0].sm, self._p(bns[0].pre_part),
                    self._p(self.act(b2.x)) if b2 else None, b2.sm if b2 else None,
                    self._p(b2.pre_part) if b2 else None, self._spv))
            else:
                self._bwd.append(self._call("rn_relu_bwd", op.y.numel, self.dtype, self._p(self.act(op.y)),
                                            self._p(dy), self._p(gbuf), None, self._spv))
            g = gbuf
        for t in (op.a, op.b):
            if t.needs_grad:
                gs.alias(t, g)

    def _bwd_pool(self, op, dy, gs):
        x = op.x
        if x.needs_grad:
            out, add = gs.contribute(x)
            self._bwd.append(self._call("rn_pool_bwd", L.C.byref(op.desc), self._p(dy), self._p(op.argmax),
                                        self._p(out), self._p(add), self._spv))
            self._gw[id(x)] = ("pool", len(self._bwd) - 1, op, dy, out, add)

    # ------------------------------------------------------------------ update
    def _build_update(self):
        self.wpack_calls = list(self.packs)
        self.opt_packs = None
        if self.fused_packs:
            dt = np.dtype([("krsc", "<u8"), ("crsk", "<u8"), ("k", "<i4"), ("rs", "<i4"), ("creal", "<i4"),
                           ("c", "<i4"), ("kpad", "<i4"), ("pad", "<i4")])
            tab = np.zeros(len(self.param_order), dtype=dt)
            for i, nm in enumerate(self.param_order):
                e = self.fused_packs.get(nm)
                if e is not None:
                    tab[i] = e + (0,)
            nums = np.array([int(np.prod(self.param_shape[n])) for n in self.param_order], dtype=np.int64)
            cap = int(sum((n + 4095) // 4096 for n in nums) + sum(
                ((e[2] + 63) // 64) * e[3] * ((e[4] + 63) // 64) for e in self.fused_packs.values()))
            work = np.zeros((cap, 4), dtype=np.int32)
            nwork = self.lib.rn_sgd_pack_work(len(nums), nums.ctypes.data_as(L.C.c_void_p),
                                              tab.ctypes.data_as(L.C.c_void_p), work.ctypes.data_as(L.C.c_void_p),
                                              cap)
            if nwork < 0:
                raise L.RNError("rn_sgd_pack_work: %s" % self.lib.rn_last_error().decode())
            self.opt_packs = self.torch.from_numpy(tab.view(np.uint8).copy()).to(self.device)
            self.opt_work = self.torch.from_numpy(work[:nwork].copy()).to(self.device)
            self.opt_nwork = int(nwork)

    # ------------------------------------------------------------------ running
    def _run(self, calls):
        if self.dry_run:  # the plan only (CPU tests): nothing is launched
            return
        for name, fn, args in calls:
            r = fn(*args)
            if r != 0:
                raise L.RNError("%s: %s" % (name, self.lib.rn_last_error().decode()))

    def set_input(self, data_np, label_np=None):
        """H2D copy of one batch (host numpy / torch) into the data/label buffers.

        A pinned host batch (mx.nd.array(..., ctx=cpu_pinned), data/imagenet.py:17-18) is copied
        asynchronously on a separate copy stream into the buffer the previous step is NOT using;
        the compute stream waits only for that copy. Because the host enqueues a whole step ahead of
        the GPU, step t+1's PCIe transfer overlaps step t's backward."""
        torch = self.torch
        t = self.plan.data_tensor
        src = torch.as_tensor(np.ascontiguousarray(data_np, dtype=np.float32)) if isinstance(data_np, np.ndarray) \
            else data_np
        src = src.reshape(-1)
        if src.dtype != torch.float32:
            src = src.to(torch.float32)
        if not self.dry_run and src.device.type == "cpu" and src.is_pinned():
            i = self._in_idx ^ 1
            if self._in_bufs[i] is None:
                self._in_bufs[i] = self._zeros(t.numel, torch.float32)
                self._copy_stream = torch.cuda.Stream(self.device)
            cs = self._copy_stream
            if self._in_free[i] is not None:
                cs.wait_event(self._in_free[i])  # the step that last read this buffer has finished
            with torch.cuda.stream(cs):
                self._in_bufs[i].copy_(src, non_blocking=True)
                done = torch.cuda.Event()
                done.record(cs)
            torch.cuda.current_stream(self.device).wait_event(done)
            self._in_idx = i
            self._in_ptr.value = self._in_bufs[i].data_ptr()
        else:
            self._in_bufs[self._in_idx].copy_(src, non_blocking=True)
        if label_np is not None:
            for tt in self.plan.tensors.values():
                if tt.kind == "label":
                    lsrc = torch.as_tensor(np.ascontiguousarray(label_np, dtype=np.float32)) \
                        if isinstance(label_np, np.ndarray) else label_np
                    self.act(tt).copy_(lsrc.reshape(-1).to(torch.float32), non_blocking=True)

    def _mark_input_read(self):
        if not self.dry_run and self._in_bufs[1] is not None:
            ev = self.torch.cuda.Event()
            ev.record(self.torch.cuda.current_stream(self.device))
            self._in_free[self._in_idx] = ev

    def forward(self, is_train=True):
        self._sync_stream()
        self._run(self._fwd_train if is_train else self._fwd_infer)
        if is_train:
            self._qfirst.value = 0
        self._mark_input_read()

    def backward(self, hooks=None):
        self._sync_stream()
        self.grad.zero_()
        side = self._side_stream if (self._side_idx and self.side_enabled) else None
        if not hooks and side is None:
            self._run(self._bwd)
            self._mark_input_read()
            return
        # hooks: {bwd index -> callable}, e.g. RCCL bucket all-reduce launches; with the wgrad side
        # stream a hook runs on it after a fork, so its collective follows both streams' writes
        hooks = hooks or {}
        forked = False
        for i, (name, fn, args) in enumerate(self._bwd):
            if side is not None and i in self._side_idx and (not forked or i not in self._side_pre):
                self._fork(i)  # (the first side call of the step waits for the forward too)
                forked = True
            r = 0 if self.dry_run else fn(*args)
            if r != 0:
                raise L.RNError("%s: %s" % (name, self.lib.rn_last_error().decode()))
            h = hooks.get(i + 1)
            if h is not None:
                if side is not None:
                    self._fork(("hook", i))
                    with self.torch.cuda.stream(side):
                        h()
                else:
                    h()
        if side is not None:
            self._join()
        self._mark_input_read()

    def repack_weights(self):
        self._sync_stream()
        self._run(self.wpack_calls)

    def sgd_update(self, lr, wd, momentum, rescale_grad, clip=-1.0):
        self._sync_stream()
        if self.dry_run:
            return
        if self._wd_value != wd:
            self.opt_wds.copy_(self.torch.from_numpy(self.wd_mult * np.float32(wd)))
            self._wd_value = wd
        if self.opt_lrms is not None:  # (some lr_mult differs from 1: the entry points with the multiplier table)
            self._sgd_update_lrm(lr, momentum, rescale_grad, clip)
            return
        if self.opt_packs is not None:
            L.check(self.lib.rn_sgd_mom_update_pack(len(self.param_order), self._p(self.opt_offsets),
                                                    self._p(self.opt_numels), self._p(self.opt_wds),
                                                    self._p(self.master), self._p(self.grad), self._p(self.mom),
                                                    self._p(self.opt_packs), self._p(self.opt_work),
                                                    self.opt_nwork, self.dtype, float(lr), None,
                                                    float(momentum), float(rescale_grad), float(clip), self._sp()),
                    "rn_sgd_mom_update_pack")
            self._run(self.unfused_packs)
            return
        L.check(self.lib.rn_sgd_mom_update(len(self.param_order), self._p(self.opt_offsets),
                                           self._p(self.opt_numels), self._p(self.opt_wds), self._p(self.master),
                                           self._p(self.grad), self._p(self.mom), None, F32, float(lr), None,
                                           float(momentum), float(rescale_grad), float(clip), self._sp()),
                "rn_sgd_mom_update")
        self.repack_weights()

    def _sgd_update_lrm(self, lr, momentum, rescale_grad, clip):
        n, lrm = len(self.param_order), self._p(self.opt_lrms)
        if self.opt_packs is not None:
            L.check(self.lib.rn_sgd_mom_update_pack_lrm(n, self._p(self.opt_offsets), self._p(self.opt_numels),
                                                        self._p(self.opt_wds), lrm, self._p(self.master),
                                                        self._p(self.grad), self._p(self.mom), self._p(self.opt_packs),
                                                        self._p(self.opt_work), self.opt_nwork, self.dtype, float(lr),
                                                        None, float(momentum), float(rescale_grad), float(clip),
                                                        self._sp()), "rn_sgd_mom_update_pack_lrm")
            self._run(self.unfused_packs)
            return
        L.check(self.lib.rn_sgd_mom_update_lrm(n, self._p(self.opt_offsets), self._p(self.opt_numels),
                                               self._p(self.opt_wds), lrm, self._p(self.master), self._p(self.grad),
                                               self._p(self.mom), None, F32, float(lr), None, float(momentum),
                                               float(rescale_grad), float(clip), self._sp()), "rn_sgd_mom_update_lrm")
        self.repack_weights()

    # ------------------------------------------------------------------ param I/O (MXNet layouts)
    def set_param(self, name, value):
        v = np.asarray(value, dtype=np.float32)
        if tuple(v.shape) != self.param_shape[name]:
            raise ValueError("shape mismatch for %s: %s vs %s" % (name, v.shape, self.param_shape[name]))
        if self.param_layout[name] == "krsc":
            v = v.transpose(0, 2, 3, 1)
        self.pview(name).copy_(self.torch.from_numpy(np.ascontiguousarray(v).reshape(-1)))

    def get_param(self, name, grad=False):
        src = self.gview(name) if grad else self.pview(name)
        shp = self.param_shape[name]
        v = src.detach().cpu().numpy()
        if self.param_layout[name] == "krsc":
            k, c, r, s = shp
            return v.reshape(k, r, s, c).transpose(0, 3, 1, 2).copy()
        return v.reshape(shp).copy()

    def set_aux(self, name, value):
        v = np.asarray(value, dtype=np.float32).reshape(-1)
        self.aview(name).copy_(self.torch.from_numpy(v))

    def get_aux(self, name):
        o, shp = self.aux_off[name]
        return self.aview(name).detach().cpu().numpy().reshape(shp).copy()

    def output(self, i=0):
        t = self.plan.outputs[i]
        a = self.act(t)
        if t.kind == "prob":
            return a.view(t.n, t.c)
        return a

    # ------------------------------------------------------------------ gradient buckets
    def buckets(self):
        """[(start, end, last_bwd_index)] over the flat grad buffer: ~bucket_bytes each, except the trailing
        bucket -- the longest suffix of the parameter order (the earliest layers, whose gradients are final
        last) within tail_bucket_bytes -- which stands alone so that little is left to sum once the backward
        has ended (core/solver.py:116-121: the kvstore push of the last gradients)."""
        out = []
        order = list(self.param_order)
        sizes = [int(np.prod(self.param_shape[nm])) for nm in order]
        tail_at = len(order)
        tb = getattr(self, "tail_bucket_bytes", 0)
        acc = 0
        while tail_at > 0 and (acc + sizes[tail_at - 1]) * 4 <= tb:
            tail_at -= 1
            acc += sizes[tail_at]
        if tail_at == 0 or acc == 0:
            tail_at = len(order)  # (everything within the tail size, or nothing fits: the plain plan)
        cur_start, cur_end, cur_last = None, None, 0
        for k, nm in enumerate(order):
            o = self.param_off[nm]
            n = sizes[k]
            last = self.param_done_at.get(nm, len(self._bwd))
            if k == tail_at and cur_start is not None:  # close the head before the trailing bucket
                out.append((cur_start, o, cur_last))
                cur_start = None
            if cur_start is None:
                cur_start, cur_end, cur_last = o, o + n, last
            else:
                cur_end, cur_last = o + n, max(cur_last, last)
            if k < tail_at and (cur_end - cur_start) * 4 >= self.bucket_bytes:
                out.append((cur_start, cur_end, cur_last))
                cur_start = None
        if cur_start is not None:
            out.append((cur_start, self.nparam, max(cur_last, 0)))
        # a bucket may only launch after every earlier bucket's params are final too
        fixed, run = [], 0
        for s, e, last in out:
            run = max(run, last)
            fixed.append((s, e, run))
        return fixed
