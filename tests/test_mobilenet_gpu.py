"""MobileNet-v1 (symbol/mobilenet.py) through the drop-in on the GPU.

fp32: one whole step against the fp64 oracle with the device's ReLU decisions replayed, bars of
tests/test_step_gpu.py. bf16: every kernel of a step against its fp32 recompute from the device's own inputs
(tests/layerwise.py, its BF16_BAR / WGRAD_BAR) with all 13 depthwise layers' forward, data gradient and weight
gradient on record; the whole step's distance to fp64 bounded by the bf16-storage emulation's own (ReLU
decisions replayed, as tests/test_step_bf16_gpu.py does for ResNet-50); the loss falling over 3 SGD steps."""
import numpy as np
import pytest
import torch

from mobilenet_util import DW_NAMES, oracle_mobilenet
from oracle import net as onet, ops
from rn import graphs
from step_util import ce_loss, fro_rel, grad_summary, max_rel, module_step, oracle_state, oracle_step, replayed_parity

pytestmark = pytest.mark.gpu


def _small():
    g = oracle_mobilenet(8, 0.25)
    args, aux = oracle_state(g)
    data, label = onet.synthetic_batch(4, (3, 64, 64), 8)
    return g, args, aux, data, label


def test_mobilenet_fp32_small(gpu):
    g, args, aux, data, label = _small()
    res = module_step(graphs.mobilenet(8, alpha=0.25, resolution=64), args, aux, data, label, "float32")
    assert len(res["relu_masks"][0]) == 27
    errs, ref = replayed_parity(res, g, args, aux, data, label)
    worst = max(errs.items(), key=lambda kv: kv[1][0] / kv[1][2])
    print("fp32 step: prob %.2e, worst gradient %s %.2e (numpy fp32 %.2e, tol %.2e)"
          % (max_rel(res["prob"][0], ref["prob"][0]), worst[0], *worst[1]))
    assert max_rel(res["prob"][0], ref["prob"][0]) < 1e-4
    bad = {n: v for n, v in errs.items() if v[0] > v[2]}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1][0])[:5]
    worst = max((fro_rel(res["args"][n], ref["args"][n]), n) for n in ref["args"])
    assert worst[0] < 1e-4, worst


def test_mobilenet_bf16_layerwise(gpu):
    """alpha 0.5 (16 .. 512 depthwise channels), 8 images of 96x96, after one full step (the depthwise compute
    copies are then the ones rn_conv_weight_pack_multi rewrote)."""
    from layerwise import BF16_BAR, WGRAD_BAR  # noqa: F401  (the bars ck.failures() applies)
    from test_step_bf16_gpu import _layerwise
    ck = _layerwise(graphs.mobilenet(1000, alpha=0.5, resolution=96), 8, 96, "bfloat16", warm=1)
    dws = [op for op in ck.ex.plan.ops if op.kind == "conv" and op.groups > 1]
    assert [op.name for op in dws] == DW_NAMES and all(op.desc.grouped_direct == 2 for op in dws)
    by_kind = {}
    for r in ck.rec:
        by_kind.setdefault(r[0], set()).add(r[1])
    assert by_kind.get("conv_fwd_grouped") == set(DW_NAMES), by_kind.get("conv_fwd_grouped")
    assert by_kind.get("dgrad_grouped") == set(DW_NAMES), by_kind.get("dgrad_grouped")
    assert by_kind.get("wgrad_grouped") == {n + "_weight" for n in DW_NAMES}, by_kind.get("wgrad_grouped")
    # the calls that run them were hooked, not passed over
    assert not {"rn_conv_bwd_data", "rn_conv_bwd_filter_ws", "rn_conv_bwd_filter"} & set(ck.skipped), ck.skipped
    assert ck.covered.get("rn_conv_bwd_filter_ws", 0) >= 13
    # every forward op was checked, conv_1 (a stem without bn_data) included: the checker re-lays the image
    # itself for it; test_mobilenet_bf16_stem below holds it to the oracle at two widths besides
    assert not ck.fwd_skipped, ck.fwd_skipped
    assert len(by_kind.get("stem_conv_fwd", ())) == 1, by_kind.get("stem_conv_fwd")
    assert len(by_kind.get("conv_fwd", ())) == 13  # the pointwise layers
    bad = ck.failures()
    assert not bad, bad[:10]


def test_mobilenet_bf16_stem(gpu):
    """conv_1: 3x3 / stride 2 over the 3 input channels with no BatchNorm before it, a stem shape of its own
    (the layerwise checker re-computes it from the device's own re-laid image at one width). Against the oracle's
    convolution of the bf16-rounded input and weights, the kernels' bar (1.5e-2 of max |ref|)."""
    import mxnet as mx
    from gpu_util import bf16_round
    rng = np.random.default_rng(3)
    data = rng.uniform(-1, 1, (4, 3, 64, 64)).astype(np.float32)
    for alpha in (0.25, 1):
        mod = mx.mod.Module(graphs.mobilenet(8, alpha=alpha, resolution=64), context=[mx.gpu(0)], precision="bfloat16")
        mod.bind(data_shapes=[("data", data.shape)], label_shapes=[("softmax_label", (4,))])
        mx.random.seed(2)
        mod.init_params(mx.init.Xavier(rnd_type="gaussian", factor_type="in", magnitude=2))
        mod.forward(mx.io.DataBatch(data=[mx.nd.array(data)], label=[mx.nd.array(np.zeros(4, np.float32))]),
                    is_train=True)
        torch.cuda.synchronize()
        ex = mod.executor
        stem = [op for op in ex.plan.ops if op.kind == "stem"][0]
        t = stem.y
        y = ex.act(t).float().cpu().numpy().reshape(t.n, t.h, t.w, t.cp)[..., :t.c].transpose(0, 3, 1, 2)
        w = ex.get_param("conv_1_conv2d_weight")
        ref = ops.conv2d_fwd(bf16_round(data), bf16_round(w), (2, 2), (1, 1))
        err = float(np.abs(y - ref).max() / np.abs(ref).max())
        print("conv_1 alpha", alpha, "p4" if stem.p4 else "nhwc8", "err %.2e" % err)
        assert err < 1.5e-2, (alpha, err)


def test_mobilenet_bf16_step_and_loss(gpu):
    """Default knobs. Step 1's gradients against fp64 with the device's ReLU decisions replayed: no further
    than a small multiple of the bf16-storage emulation's own distance (the factors and floors of
    test_resnet50_bf16_step_gradients); then the loss over 3 SGD steps on the fixed batch falls."""
    g, args, aux, data, label = _small()
    res = module_step(graphs.mobilenet(8, alpha=0.25, resolution=64), args, aux, data, label, "bfloat16", lr=0.05,
                      steps=3)
    torch.cuda.synchronize()
    masks = res["relu_masks"][0]
    ref = oracle_step(g, args, aux, data, label)
    emu = oracle_step(g, args, aux, data, label, storage="bf16")
    raw_dev = grad_summary(res["grads"][0], ref["grads"][0])
    raw_emu = grad_summary(emu["grads"][0], ref["grads"][0])
    ref_m = oracle_step(g, args, aux, data, label, relu_masks=masks)
    emu_m = oracle_step(g, args, aux, data, label, storage="bf16", relu_masks=masks)
    s_dev = grad_summary(res["grads"][0], ref_m["grads"][0])
    s_emu = grad_summary(emu_m["grads"][0], ref_m["grads"][0])
    p_dev = max_rel(res["prob"][0], ref_m["prob"][0])
    p_emu = max_rel(emu_m["prob"][0], ref_m["prob"][0])
    print("unreplayed  device vs fp64:", raw_dev, " bf16 emulation vs fp64:", raw_emu)
    print("replayed    device vs fp64:", s_dev, "prob", p_dev, " bf16 emulation vs fp64:", s_emu, "prob", p_emu)
    assert raw_dev["median"] < 1.5 * raw_emu["median"] + 0.1, (raw_dev, raw_emu)
    assert 1 - s_dev["cos"] < 1.5 * (1 - s_emu["cos"]) + 0.01, (s_dev, s_emu)
    for k in ("fro", "median", "p95"):
        assert s_dev[k] < 1.5 * s_emu[k] + 0.02, (k, s_dev, s_emu)
    assert p_dev < 2 * p_emu + 0.02, (p_dev, p_emu)
    losses = [ce_loss(p, label) for p in res["prob"]]
    print("losses", losses)
    assert all(np.isfinite(p).all() for p in res["prob"])
    assert losses[2] < losses[0], losses
