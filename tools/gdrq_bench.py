"""Time of the GDRQ kernels against the kernels with the same traffic, paired:

  rn_gdrq_fwd, update = 0 (values + int8 codes)  vs  rn_pact_fwd (the same three tensors)
  rn_gdrq_fwd, update = 1                        vs  rn_gdrq_fwd, update = 0: the sum|x| pass + the small launch
  rn_gdrq_bwd                                    vs  rn_quant_int8_bwd (the same three tensors, the other mask)
  rn_weight_gdrq_pack                            vs  rn_weight_quant_pack on ResNet-50's weight set (qw, the int8
                                                     codes and the data-gradient copy of every dense convolution)

at 256 x 56 x 56 x 64, bf16. Each call is timed on its own between two events after the caches were evicted (--cold,
the default: in a training step these tensors do not come from the caches), the two kernels of a pair alternating;
a repeat is the median over --iters such calls, and the spread is the range of that median over --repeats repeats of
the same command in one process.

python tools/gdrq_bench.py [--iters 20] [--repeats 3] [--warm] [--nbits 4]
Prints one JSON line per kernel and one per pair.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "resnet.mxnet_amd")]


def _weight_items(torch, L, dev):
    """Both packs' item arrays over the dense convolution weights of ResNet-50 (batch-independent), sharing every
    buffer: the master, qw, unit, the state, the int8 codes and the data-gradient copy."""
    from rn import graphs
    from rn.plan import Plan, _pad8
    plan = Plan(graphs.resnet50_gdrq(), [("data", (2, 3, 224, 224))], [("softmax_label", (2,))])
    keep, qi, gi = [], [], []
    for op in plan.ops:
        if op.kind != "conv" or op.groups != 1:
            continue
        k, cr, r, s = plan.param_shape(op.weight)
        rs, c, kp = r * s, _pad8(cr), _pad8(k)
        t = [torch.randn(k * rs * cr, device=dev) * 0.05, torch.zeros(k * rs * cr, device=dev),
             torch.zeros(1, device=dev), torch.full((1,), 0.5, device=dev),
             torch.zeros(k * rs * c, dtype=torch.int8, device=dev),
             torch.zeros(c * rs * kp, dtype=torch.bfloat16, device=dev)]
        keep.append(t)
        m, qw, unit, state, codes, crsk = [v.data_ptr() for v in t]
        qi.append(L.WQuantItem(master=m, qw=qw, unit=unit, minmax=state, w_codes=codes, w_crsk=crsk, k=k, rs=rs,
                               c_real=cr, c=c, k_pad=kp, nbits=8))
        gi.append(L.WGdrqItem(master=m, qw=qw, unit=unit, alpha=state, w_codes=codes, w_krsc=None, w_crsk=crsk, k=k,
                              rs=rs, c_real=cr, c=c, k_pad=kp, nbits=4, fix_alpha=0, ktimes=3.0))
    up = lambda items, cls: torch.frombuffer(bytearray((cls * len(items))(*items)), dtype=torch.uint8).to(dev)  # noqa
    return keep, up(qi, L.WQuantItem), up(gi, L.WGdrqItem), len(qi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--nbits", type=int, default=4)
    ap.add_argument("--warm", action="store_true", help="do not evict the caches before each timed call")
    ap.add_argument("--size", default="256x56x56x64")
    a = ap.parse_args()
    import torch
    from rn import lib as L
    lib = L.load()
    dev = torch.device("cuda:0")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    flush = None if a.warm else torch.empty(128 << 20, dtype=torch.float32, device=dev)
    n = 1
    for d in a.size.split("x"):
        n *= int(d)
    x = (torch.randn(n, device=dev).abs() * 1.5).to(torch.bfloat16)
    dy = torch.randn(n, device=dev).to(torch.bfloat16)
    out, dx = torch.empty_like(x), torch.empty_like(x)
    codes = torch.empty(n, dtype=torch.int8, device=dev)
    unit = torch.zeros(1, device=dev)
    thr = torch.full((1,), 3.0, device=dev)
    ws = torch.zeros(int(lib.rn_gdrq_ws_bytes(n)) // 4, device=dev)
    keep, qitems, gitems, count = _weight_items(torch, L, dev)
    qws = torch.zeros(max(4096, 2 * count), device=dev)
    gws = torch.zeros(int(lib.rn_weight_gdrq_ws_bytes(count)) // 4, device=dev)

    def gfwd(update):  # (lamda = 0: the updating form leaves alpha where it is)
        return lambda: lib.rn_gdrq_fwd(L.RN_BF16, n, n, P(x), P(thr), a.nbits, update, 3.0, 0.0, P(out), P(codes),
                                       P(unit), P(ws), st)
    pairs = {
        "fwd": (("rn_gdrq_fwd", gfwd(0)),
                ("rn_pact_fwd", lambda: lib.rn_pact_fwd(L.RN_BF16, n, P(x), P(thr), a.nbits, P(out), P(codes), P(unit),
                                                        st))),
        "fwd_update": (("rn_gdrq_fwd_update", gfwd(1)), ("rn_gdrq_fwd", gfwd(0))),
        "bwd": (("rn_gdrq_bwd", lambda: lib.rn_gdrq_bwd(L.RN_BF16, n, P(x), P(dy), P(thr), P(dx), None, st)),
                ("rn_quant_int8_bwd", lambda: lib.rn_quant_int8_bwd(L.RN_BF16, n, P(x), P(dy), P(dx), P(thr), 0, None,
                                                                    st))),
        "wpack": (("rn_weight_gdrq_pack", lambda: lib.rn_weight_gdrq_pack(P(gitems), count, L.RN_BF16, P(gws), st)),
                  ("rn_weight_quant_pack", lambda: lib.rn_weight_quant_pack(P(qitems), count, L.RN_BF16, P(qws), st))),
    }
    for pair, pair_calls in pairs.items():
        for _, fn in pair_calls:
            for _ in range(3):
                L.check(fn(), pair)
        torch.cuda.synchronize()
        med = {name: [] for name, _ in pair_calls}
        for _ in range(a.repeats):
            evs = {name: [] for name, _ in pair_calls}
            for _ in range(a.iters):
                for name, fn in pair_calls:  # alternating
                    if flush is not None:
                        flush.fill_(1.0)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    evs[name].append((e0, e1))
            torch.cuda.synchronize()
            for name in evs:
                med[name].append(statistics.median(e0.elapsed_time(e1) for e0, e1 in evs[name]))
        rows = {}
        for name, _ in pair_calls:
            ms = statistics.median(med[name])
            rows[name] = {"pair": pair, "kernel": name, "cold": flush is not None, "ms": round(ms, 4),
                          "repeat_ms": [round(v, 4) for v in med[name]],
                          "spread_ms": round(max(med[name]) - min(med[name]), 4)}
            print(json.dumps(rows[name]), flush=True)
        (pn, _), (yn, _) = pair_calls
        spread = max(rows[pn]["spread_ms"], rows[yn]["spread_ms"])
        diff = rows[pn]["ms"] - rows[yn]["ms"]
        print(json.dumps({"pair": pair, "size": a.size if pair != "wpack" else "%d weights" % count,
                          "first_minus_second_ms": round(diff, 4), "spread_ms": spread,
                          "within_spread": bool(abs(diff) <= spread)}), flush=True)


if __name__ == "__main__":
    main()
