"""Training-step time of any rn.graphs builder: forward + backward + SGD update through the drop-in's
Module, timed the way bench.py times its loop (inputs resident on the device, warm-up steps, then N eager
steps between two events and one synchronise). Prints one JSON line.

python tools/step_time.py --graph mobilenet [--batch 256] [--image 224] [--precision bfloat16]
                          [--steps 20] [--warmup 5] [--classes 1000]
--graph: mobilenet (= mobilenet_1_0), or the name of any zero-argument-callable builder in rn/graphs.py
(resnet50, resnext50_32x4d, resnet50_int8, resnet20_cifar, ...). Builders that take a resolution
(mobilenet) get --image.
"""
import argparse
import inspect
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "resnet.mxnet_amd")]


def build_symbol(name, classes, image):
    from rn import graphs
    fn = getattr(graphs, name, None)
    if fn is None or not callable(fn) or name.startswith("_"):
        raise SystemExit("unknown graph %r (a builder in rn/graphs.py)" % name)
    params = inspect.signature(fn).parameters
    kw = {}
    if "num_classes" in params:
        kw["num_classes"] = classes
    if "resolution" in params:
        kw["resolution"] = image
    return fn(**kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", required=True)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--image", type=int, default=224)
    ap.add_argument("--precision", default="bfloat16")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--classes", type=int, default=1000)
    a = ap.parse_args()
    import numpy as np
    import torch
    import mxnet as mx
    from rn import lib as L
    sym = build_symbol(a.graph, a.classes, a.image)
    shp = (a.batch, 3, a.image, a.image)
    mod = mx.mod.Module(sym, context=[mx.gpu(0)], precision=a.precision)
    mod.bind(data_shapes=[("data", shp)], label_shapes=[("softmax_label", (a.batch,))], for_training=True)
    mx.random.seed(2)
    mod.init_params(mx.init.Xavier(rnd_type="gaussian", factor_type="in", magnitude=2))
    mod.init_optimizer(kvstore="device", optimizer="sgd",
                       optimizer_params={"learning_rate": 0.1, "wd": 1e-4, "momentum": 0.9, "multi_precision": True})
    data = np.random.default_rng(0).uniform(-1, 1, shp).astype(np.float32)
    label = np.random.default_rng(1).integers(0, a.classes, (a.batch,)).astype(np.float32)
    batch = mx.io.DataBatch(data=[mx.nd.array(data)], label=[mx.nd.array(label)])
    mod.forward(batch, is_train=True)  # H2D once: the inputs stay resident
    torch.cuda.synchronize()

    def step():
        mod.forward(None, is_train=True)
        mod.backward()
        mod.update()

    for _ in range(max(a.warmup, 1)):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.steps
    prob = mod.get_outputs()[0].asnumpy()
    flops = mod.executor.plan.train_flops()
    print(json.dumps({"graph": a.graph, "batch": a.batch, "image": a.image, "precision": a.precision,
                      "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(ms, 4),
                      "images_per_sec": round(a.batch / ms * 1e3, 2),
                      "train_tflops_per_sec": round(flops / ms / 1e9, 2), "finite": bool(np.isfinite(prob).all()),
                      "library": os.path.relpath(L.LIB_PATH, REPO), "build_id": L.load().rn_build_id().decode()}),
          flush=True)


if __name__ == "__main__":
    main()
