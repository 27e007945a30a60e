"""Bandwidth of the two PACT kernels against the Quantization_int8 kernels with the same traffic, paired:

  rn_pact_fwd (values + int8 codes)  vs  rn_quant_int8_fwd_codes (training: the same apply pass + a max pass)
  rn_pact_bwd (dx + the dgamma sum)  vs  rn_quant_int8_bwd       (the same three tensors, no reduction)

at the two largest ResNet-50 activation sizes of batch 256 (256 x 56 x 56 x 64 and x 256), bf16. Each call is timed
on its own between two events after the caches were evicted (--cold, the default: in a training step these tensors do
not come from the caches), the two kernels of a pair alternating; a repeat is the median over --iters such calls, and
the spread is the range of that median over --repeats repeats of the same command in one process.

python tools/pact_bench.py [--iters 20] [--repeats 3] [--warm] [--nbits 4]
Prints one JSON line per (size, kernel) and a verdict per pair: not slower = within three spreads of the yardstick.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "resnet.mxnet_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--nbits", type=int, default=4)
    ap.add_argument("--warm", action="store_true", help="do not evict the caches before each timed call")
    ap.add_argument("--sizes", default="256x56x56x64,256x56x56x256")
    a = ap.parse_args()
    import torch
    from rn import lib as L
    lib = L.load()
    dev = torch.device("cuda:0")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    flush = None if a.warm else torch.empty(128 << 20, dtype=torch.float32, device=dev)
    for size in a.sizes.split(","):
        n = 1
        for d in size.split("x"):
            n *= int(d)
        x = (torch.randn(n, device=dev).abs() * 1.5).to(torch.bfloat16)
        dy = torch.randn(n, device=dev).to(torch.bfloat16)
        out = torch.empty_like(x)
        dx = torch.empty_like(x)
        codes = torch.empty(n, dtype=torch.int8, device=dev)
        unit = torch.zeros(1, device=dev)
        gamma = torch.full((1,), 3.0, device=dev)
        minmax = torch.full((1,), 3.0, device=dev)
        dgamma = torch.zeros(1, device=dev)
        ws = torch.zeros(int(lib.rn_pact_bwd_ws_bytes(n)) // 4, device=dev)
        qws = torch.zeros(4096, device=dev)
        calls = {
            "fwd": (("rn_pact_fwd", 5, lambda: lib.rn_pact_fwd(L.RN_BF16, n, P(x), P(gamma), a.nbits, P(out), P(codes),
                                                               P(unit), st)),
                    ("rn_quant_int8_fwd_codes", 7, lambda: lib.rn_quant_int8_fwd_codes(
                        L.RN_BF16, n, P(x), P(out), P(codes), P(unit), P(minmax), 0, 1, 0.99, 0, 8, P(qws), st))),
            "bwd": (("rn_pact_bwd", 6, lambda: lib.rn_pact_bwd(L.RN_BF16, n, P(x), P(dy), P(gamma), P(dx), None,
                                                               P(dgamma), P(ws), st)),
                    ("rn_quant_int8_bwd", 6, lambda: lib.rn_quant_int8_bwd(L.RN_BF16, n, P(x), P(dy), P(dx), P(minmax),
                                                                           0, None, st))),
        }
        for pair, pair_calls in calls.items():
            for _, _, fn in pair_calls:
                for _ in range(3):
                    L.check(fn(), pair)
            torch.cuda.synchronize()
            med = {name: [] for name, _, _ in pair_calls}
            for _ in range(a.repeats):
                evs = {name: [] for name, _, _ in pair_calls}
                for _ in range(a.iters):
                    for name, _, fn in pair_calls:  # alternating
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
            for name, bpe, _ in pair_calls:
                ms = statistics.median(med[name])
                rows[name] = {"size": size, "n": n, "kernel": name, "cold": flush is not None, "ms": round(ms, 4),
                              "repeat_ms": [round(v, 4) for v in med[name]],
                              "spread_ms": round(max(med[name]) - min(med[name]), 4), "bytes_per_element": bpe,
                              "GBps": round(bpe * n / ms / 1e6, 1)}
                print(json.dumps(rows[name]), flush=True)
            (pn, _, _), (yn, _, _) = pair_calls
            spread = max(rows[pn]["spread_ms"], rows[yn]["spread_ms"])
            diff = rows[pn]["ms"] - rows[yn]["ms"]
            print(json.dumps({"size": size, "pair": pair, "pact_minus_yardstick_ms": round(diff, 4),
                              "spread_ms": spread, "not_slower": bool(diff <= 3 * spread)}), flush=True)


if __name__ == "__main__":
    main()
