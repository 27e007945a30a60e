"""tests/layerwise.py's Checker with the QIL calls: every rn_qil_fwd and every weight of rn_weight_qil_pack bit for
bit from the device's own inputs and the points in the flat master buffer (qil_util.qil_fwd_ref), every rn_qil_bwd
and rn_weight_qil_bwd: dx / the in-place dw bit for bit, dp / dc within the kernels' summation bound, in their own
slots of the flat gradient buffer."""
import numpy as np
import torch

import qil_util as U
from layerwise import Checker


def _np(t):
    return t.detach().float().cpu().numpy()


class QilChecker(Checker):
    def __init__(self, ex, **kw):
        super().__init__(ex, **kw)
        self.qil_stats = {}  # {QIL name: p, c, fractions below / inside / above the interval, highest |code|}
        self.qil_bwd = []    # per rn_qil_bwd / rn_weight_qil_bwd call: name, add operand, aliasing, dp, dc
        self.qil_by_p = {ex._pp(o.prune).value: ("act", o) for o in ex.plan.ops if o.kind == "qil"}
        for o in ex.plan.ops:
            q = o.qweight
            if q and q.get("family") == "qil":
                self.qil_by_p[ex._pp(q["prune"]).value] = ("weight", o)

    def _points(self, pn, cn):
        return np.float32(self.ex.pview(pn)[0].item()), np.float32(self.ex.pview(cn)[0].item())

    def _stats(self, name, x, q, p, c, levels):
        a = np.abs(x)
        self.qil_stats[name] = {"p": float(p), "c": float(c), "below": float((a < p).mean()),
                                "inside": float(((a >= p) & (a <= c)).mean()), "above": float((a > c).mean()),
                                "max_code": int(np.abs(q).max()), "levels": int(levels)}

    # ------------------------------------------------------------------ forward
    def check_forward(self):
        super().check_forward()
        for op in self.ex.plan.ops:
            if op.kind == "qil":
                self.check_qil(op)
                self.fwd_skipped["qil"] -= 1
        if self.fwd_skipped.get("qil") == 0:
            del self.fwd_skipped["qil"]

    def check_qil(self, op):
        """An activation QIL (rn_qil_fwd) over the whole buffer, padded channels included: the unit, the values, and
        where it emits them the int8 codes; the points the forward left are inside [0, 1]."""
        ex = self.ex
        bf = ex.dtype == 0
        x = _np(ex.act(op.x))
        p, c = self._points(op.prune, op.clip)
        val, q, unit, p1, c1 = U.qil_fwd_ref(x, p, c, op.nbits, to_bf16=bf)
        m = {"clamped": 0.0 if (p1, c1) == (p, c) else 1.0,
             "unit": 0.0 if np.float32(op.unit[0].item()) == unit else 1.0,
             "values": float((_np(ex.act(op.y)) != val).mean())}
        if op.codes is not None:
            m["codes"] = float((op.codes.cpu().numpy() != q.astype(np.int8)).mean())
        self._stats(op.name, _np(self.act_nchw(op.x)), q, p, c, 2 ** op.nbits - 1)
        self.add_metric("qil", op.name, m, {k: 0.0 for k in m})

    def check_weight_quant(self, op):
        q = op.qweight
        if q.get("family") != "qil":
            return super().check_weight_quant(op)
        ex = self.ex
        bf = ex.dtype == 0
        p, c = self._points(q["prune"], q["clip"])
        shp = ex.param_shape[op.weight]
        k, cr = shp[0], shp[1]
        r_, s_ = (shp[2], shp[3]) if len(shp) == 4 else (1, 1)
        wm = _np(self.param(op.weight))  # KRSC, as the pack reads it
        val, code, unit, p1, c1 = U.qil_fwd_ref(wm, p, c, q["nbits"])
        oihw = lambda a: torch.from_numpy(a.reshape(k, r_, s_, cr).transpose(0, 3, 1, 2).copy())  # noqa: E731
        low = oihw(U.bf16(val) if bf else val)
        m = {"clamped": 0.0 if (p1, c1) == (p, c) else 1.0, "values": float((_np(op.qw) != val).mean())}
        d = op.desc
        if op.int8:
            m["unit"] = 0.0 if np.float32(op.wunit[0].item()) == unit else 1.0
            m["codes"] = self.mismatch(self.w_from_krsc(op.wk8, d).cpu(), oihw(code))["mismatch"]
        elif op.kind == "fc":
            m["krsc"] = self.mismatch(op.wk.view(d.k, d.c)[:, :d.c_real].float().cpu(), low.view(k, cr))["mismatch"]
        else:
            m["krsc"] = self.mismatch(self.w_from_krsc(op.wk, d).cpu(), low)["mismatch"]
        if op.kind == "fc":
            m["crsk"] = self.mismatch(op.wc.view(d.c, d.k_pad)[:d.c_real, :d.k].t().float().cpu(),
                                      low.view(k, cr))["mismatch"]
        else:
            m["crsk"] = self.mismatch(self.w_from_crsk(op.wc, d).cpu(), low)["mismatch"]
        self._stats(q["name"], wm, code, p, c, 2 ** q["nbits"] - 1)
        self.add_metric("weight_qil", q["name"], m, {kk: 0.0 for kk in m})

    # ------------------------------------------------------------------ backward (hooks)
    def _qil_bwd_post(self, kind, name, pn, cn, n, x, dy, add, dx_dev, dpp, dcp, itemsize, call):
        ex = self.ex
        p, c = self._points(pn, cn)
        bf = ex.dtype == 0 and kind == "act"
        dx, wp, wc, ap, ac = U.qil_bwd_ref(_np(x), _np(dy), p, c, None if add is None else _np(add), to_bf16=bf)
        k = U.qil_bwd_chain(n, itemsize) + U.QIL_TERM_ROUNDINGS
        m = {"dx": float((_np(dx_dev) != dx).mean())}
        for key, nm, ptr, want, asum in (("dp", pn, dpp, wp, ap), ("dc", cn, dcp, wc, ac)):
            dev = float(ex.gview(nm)[0])
            call[key] = dev
            m[key] = abs(dev - want) / (k * 2.0 ** -24 * asum) if asum > 0 else (0.0 if dev == 0.0 else float("inf"))
            try:
                slot = self.grad_name(ptr)
            except KeyError:
                slot = None
            m[key + "_slot"] = 0.0 if slot == nm else 1.0
        self.add_metric("qil_bwd" if kind == "act" else "weight_qil_bwd", name, m,
                        {"dx": 0.0, "dp": 1.0, "dc": 1.0, "dp_slot": 0.0, "dc_slot": 0.0})

    def _h_rn_qil_bwd(self, args, state):
        """An activation QIL's backward: dy and add taken before the call (either may be the buffer dx overwrites)."""
        n, xp, dyp, pp, cp, dxp, addp, dpp, dcp = args[1:10]
        _, op = self.qil_by_p[pp.value]
        call = {"name": op.name, "add": addp is not None, "aliased": addp is not None and addp.value == dxp.value}
        self.qil_bwd.append(call)
        sd, sa = self._snap(dyp, state, "dy"), self._snap(addp, state, "add")

        def pre():
            sd()
            sa()

        def post():
            x = self.t(xp)[:n]
            add = state["add"][:n] if state["add"] is not None else None
            self._qil_bwd_post("act", op.name, op.prune, op.clip, n, x, state["dy"][:n], add, self.t(dxp)[:n], dpp, dcp,
                               x.element_size(), call)
        return pre, post

    def _h_rn_weight_qil_bwd(self, args, state):
        """A QIL weight's backward: the weight gradient as its weight-gradient call left it, taken before the call
        that rewrites it in place."""
        n, wp, dwp, pp, cp, dpp, dcp = args[0:7]
        _, op = self.qil_by_p[pp.value]
        q = op.qweight
        call = {"name": q["name"], "add": False, "aliased": False}
        self.qil_bwd.append(call)

        def pre():
            state["dw"] = self.ex.gview(op.weight).clone()

        def post():
            assert dwp.value == self.ex._gp(op.weight).value and wp.value == self.ex._pp(op.weight).value
            self._qil_bwd_post("weight", q["name"], q["prune"], q["clip"], n, self.param(op.weight), state["dw"], None,
                               self.ex.gview(op.weight), dpp, dcp, 4, call)
        return pre, post
