"""The BatchNorm backward applied by the recomputed streamed conv1 data gradient (dgrad1x1_stream_kernel's apply
form at 64 channels per wave, its per-channel constants in LDS; rn_conv_dgrad_streamed; the executor's
RN_BN_BWD_RECOMPUTE route).

* per kernel: reduction-only rn_conv_bwd_data_bnred + rn_bn_bwd_finalize + rn_conv_bwd_data_bnapply against the
  stored path (rn_conv_bwd_data_bnred + rn_bn_bwd_part) bit for bit, and against the fp64 oracle;
* the apply call repeated: bit for bit (what found round 6's missing MFMA wait states);
* one step of a two-unit bottleneck net with RN_BN_BWD_RECOMPUTE unset, 1 (the route at any size) and 0 (off), each
  in a fresh process: bit-identical;
* rn_conv_dgrad_streamed's shape rule and the default's size gate, on the host.
"""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ops
from rn import lib as L
from gpu_util import BF16, bf16_round, conv_desc, from_nhwc, p, rel_err, stream, to_nhwc

TESTS = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(TESTS)

# (n, C, h, w, K): the BN has C channels, the 1x1 convolution reduces over K
SHAPES = [
    (3, 256, 14, 14, 64),    # one column group, 64 channels per wave; last block of 140 rows = 8 steps + 12 rows
    (2, 512, 9, 11, 128),    # two column groups, KS = 4; one short block
    (1, 256, 15, 15, 64),    # 225 rows: a second block of one row
    (5, 128, 7, 9, 64),      # C % 256 != 0: 32 channels per wave
]


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    n, c, h, w, k = shape
    rng = np.random.default_rng(21)
    xb = bf16_round(rng.standard_normal((n, c, h, w)) * 1.5 + 0.3)  # BN input
    gamma, beta = rng.uniform(0.5, 1.5, c), rng.standard_normal(c) * 0.2
    wt = bf16_round(rng.standard_normal((k, c, 1, 1)) / np.sqrt(c))
    dy = bf16_round(rng.standard_normal((n, k, h, w)))
    res = bf16_round(rng.standard_normal((n, c, h, w)) * 0.5)  # the gradient fan-in (add_src of the apply)
    return xb, gamma, beta, wt, dy, res


@functools.lru_cache(maxsize=None)
def _oracle(shape, relu):
    """fp64: the conv data gradient, stored as bf16, through the BN(+ReLU) backward (without the fan-in)."""
    xb, gamma, beta, wt, dy, _ = _inputs(shape)
    a_ref, cache = ops.bn_train_fwd(xb, gamma, beta, 1e-5, False)
    act = ops.relu_fwd(a_ref) if relu else a_ref
    dact, _ = ops.conv2d_bwd(act, wt, dy, (1, 1), (0, 0))
    dz = ops.relu_bwd(bf16_round(dact), act) if relu else bf16_round(dact)
    return ops.bn_train_bwd(dz, cache, False)


class _Dev:
    """The device side of one shape: the BN forward's saved statistics and the packed weight."""

    def __init__(self, shape, gpu):
        n, c, h, w, k = shape
        xb, gamma, beta, wt, dy, res = _inputs(shape)
        self.lib = L.load()
        self.d = d = conv_desc(BF16, n, c, h, w, k, 1, 1, 1, 0)
        assert self.lib.rn_conv_dgrad_streamed(C.byref(d)) == 1 and self.lib.rn_conv_tile(C.byref(d), 1) >= 128
        self.wc = torch.zeros(d.c * d.k_pad, dtype=torch.bfloat16, device=gpu)
        master = torch.from_numpy(np.ascontiguousarray(wt.transpose(0, 2, 3, 1), dtype=np.float32)).reshape(-1).to(gpu)
        L.call("rn_conv_weight_pack", C.byref(d), p(master), None, p(self.wc), stream())
        self.bd = bd = L.BNDesc(dtype=BF16, m=n * h * w, c=d.c, c_real=c, eps=1e-5, momentum=0.9, fix_gamma=0, relu=1)
        f = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float32, device=gpu)
        self.zf = lambda: torch.zeros(d.c, dtype=torch.float32, device=gpu)
        self.g_d, b_d, mm, mv = f(gamma), f(beta), f(np.zeros(c)), f(np.ones(c))
        self.sm, self.si, self.sc, self.sh = self.zf(), self.zf(), self.zf(), self.zf()
        self.ws = torch.zeros(self.lib.rn_bn_workspace_bytes(C.byref(bd)) // 4 + 16, dtype=torch.float32, device=gpu)
        self.xbd, self.dyd, self.resd = to_nhwc(xb, BF16, gpu), to_nhwc(dy, BF16, gpu), to_nhwc(res, BF16, gpu)
        L.call("rn_bn_fwd_train", C.byref(bd), p(self.xbd), None, p(self.g_d), p(b_d), p(mm), p(mv), p(self.sm),
               p(self.si), p(self.sc), p(self.sh), p(self.ws), stream())
        self.nrb = self.lib.rn_conv_bnred_blocks(C.byref(d))
        self.gpu = gpu

    def bn_desc(self, relu):
        self.bd.relu = relu
        return C.byref(self.bd)

    def parts(self):
        return torch.full((self.nrb * self.d.c * 2,), float("nan"), dtype=torch.float32, device=self.gpu)

    def stored(self, relu, add):
        d, part, dact = C.byref(self.d), self.parts(), torch.zeros_like(self.xbd)
        L.call("rn_conv_bwd_data_bnred", d, p(self.dyd), p(self.wc), p(dact), None, p(self.xbd), p(self.sm), p(self.sc),
               p(self.sh), relu, p(part), stream())
        dx, dg, db = torch.full_like(self.xbd, float("nan")), self.zf(), self.zf()
        L.call("rn_bn_bwd_part", self.bn_desc(relu), p(part), self.nrb, p(self.xbd), p(dact), p(dx), p(add),
               p(self.g_d), p(self.sm), p(self.si), p(self.sc), p(self.sh), p(dg), p(db), p(self.ws), stream())
        return dx, dg, db, part

    def reduce_finalize(self, relu):
        d, part = C.byref(self.d), self.parts()
        L.call("rn_conv_bwd_data_bnred", d, p(self.dyd), p(self.wc), None, None, p(self.xbd), p(self.sm), p(self.sc),
               p(self.sh), relu, p(part), stream())
        coef, dg, db = torch.zeros(4 * self.d.c, dtype=torch.float32, device=self.gpu), self.zf(), self.zf()
        L.call("rn_bn_bwd_finalize", self.bn_desc(relu), p(part), self.nrb, p(self.g_d), p(self.sm), p(self.si), p(dg),
               p(db), p(coef), stream())
        return coef, dg, db, part

    def apply(self, coef, relu, add):
        dx = torch.full_like(self.xbd, float("nan"))
        L.call("rn_conv_bwd_data_bnapply", C.byref(self.d), p(self.dyd), p(self.wc), p(dx), p(add), p(self.xbd),
               p(coef), p(self.sc), p(self.sh), relu, stream())
        return dx


@pytest.fixture
def deterministic():
    L.call("rn_set_tuning", 17, 1)
    yield
    L.call("rn_set_tuning", 17, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("with_add", [0, 1], ids=["noadd", "add"])
@pytest.mark.parametrize("relu", [1, 0], ids=["relu", "norelu"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stream_recompute_chain(gpu, deterministic, shape, relu, with_add):
    """Recomputed chain == stored chain bit for bit (dx, dgamma, dbeta, the partials), and dx within the bf16 bar
    of test_dgrad_bn_backward_recompute (3e-2 of the largest reference value) of the fp64 oracle."""
    n, c, h, w, k = shape
    dev = _Dev(shape, gpu)
    add = dev.resd if with_add else None
    dx0, dg0, db0, part0 = dev.stored(relu, add)
    coef, dg1, db1, part1 = dev.reduce_finalize(relu)
    dx1 = dev.apply(coef, relu, add)
    torch.cuda.synchronize()
    assert not torch.isnan(dx1).any()
    assert torch.equal(part0, part1)
    assert torch.equal(dg0.view(torch.int32), dg1.view(torch.int32))
    assert torch.equal(db0.view(torch.int32), db1.view(torch.int32))
    assert torch.equal(dx0.view(torch.int16), dx1.view(torch.int16))
    dx_ref, dg_ref, db_ref = _oracle(shape, relu)
    if with_add:
        dx_ref = dx_ref + _inputs(shape)[5]
    err = rel_err(from_nhwc(dx1, c), dx_ref)
    print("dx vs fp64 oracle: %.3e (bar 3e-2)" % err)
    assert err < 3e-2
    assert rel_err(db1.cpu().numpy()[:c], db_ref) < 2e-2 and rel_err(dg1.cpu().numpy()[:c], dg_ref) < 2e-2


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_stream_apply_repeat(gpu, shape):
    """The apply call twice on the same inputs: the same bits."""
    dev = _Dev(shape, gpu)
    coef = dev.reduce_finalize(1)[0]
    outs = [dev.apply(coef, 1, dev.resd) for _ in range(2)]
    torch.cuda.synchronize()
    assert not torch.isnan(outs[0]).any()
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))


# ---------------------------------------------------------------------------------------------- executor
def _two_unit_net():
    from rn import graphs
    # the ImageNet stem (16 x 16 -> 4 x 4) -> two pre-activation bottleneck units 64 -> 256 -> bn1 / pool / fc
    return graphs.resnet([2], 1, [64, 256], 16)


GRAD_BYTES = 4 * 4 * 4 * 256 * 2  # the two-unit net's gradient of unit 2's bn1 output at batch 4, 16 x 16 (bf16)


def _child(out_path, gate=None):
    """One bf16 step of the two-unit net (batch 4, 16 x 16); everything it computed into out_path (.npz). gate:
    the default's size gate (Executor.RECOMPUTE_MIN_BYTES) for this process, so that the unset default recomputes
    at this small size as it does at ResNet-50's."""
    import mxnet as mx
    if gate is not None:
        from rn.executor import Executor
        Executor.RECOMPUTE_MIN_BYTES = int(gate)
    rng = np.random.default_rng(5)
    data = rng.standard_normal((4, 3, 16, 16)).astype(np.float32)
    label = rng.integers(0, 16, 4).astype(np.float32)
    mod = mx.mod.Module(_two_unit_net(), context=[mx.gpu(0)], precision="bfloat16")
    mod.bind(data_shapes=[("data", data.shape)], label_shapes=[("softmax_label", label.shape)], for_training=True)
    ex = mod.executor
    args, aux = {}, {}
    for name in ex.plan.param_names:
        shp = ex.param_shape[name]
        if name.endswith("_gamma"):
            v = rng.uniform(0.5, 1.5, shp)
        elif name.endswith(("_beta", "_bias")):
            v = rng.standard_normal(shp) * 0.2
        else:
            v = rng.standard_normal(shp) / np.sqrt(np.prod(shp[1:]))
        args[name] = v.astype(np.float32)
    for name in ex.plan.aux_names:
        shp = ex.aux_off[name][1]
        aux[name] = (np.ones(shp) if name.endswith("_var") else np.zeros(shp)).astype(np.float32)
    mod.init_params(arg_params=args, aux_params=aux)
    mod.init_optimizer(kvstore="device", optimizer="sgd",
                       optimizer_params={"learning_rate": 0.1, "wd": 1e-4, "momentum": 0.9})
    mod.forward(mx.io.DataBatch(data=[mx.nd.array(data)], label=[mx.nd.array(label)]), is_train=True)
    out = {"prob": mod.get_outputs()[0].asnumpy()}
    mod.backward()
    for n in ex.plan.param_names:
        out["grad:" + n] = ex.get_param(n, grad=True)
    mod.update()
    arg_o, aux_o = mod.get_params()
    out.update({"arg:" + k: v.asnumpy() for k, v in arg_o.items()})
    out.update({"aux:" + k: v.asnumpy() for k, v in aux_o.items()})
    plan = {"bwd": [c[0] for c in ex._bwd],
            "recomputed": [op.name for op in ex.plan.ops if op.kind == "bn" and op.recomputed]}
    np.savez(out_path, plan=np.array(json.dumps(plan)), **out)


def _run_child(tmp_path, tag, recompute_env, gate=None):
    env = {k: v for k, v in os.environ.items() if k != "RN_BN_BWD_RECOMPUTE"}
    if recompute_env is not None:
        env["RN_BN_BWD_RECOMPUTE"] = recompute_env
    env["RN_DETERMINISTIC"] = "1"
    env["PYTHONPATH"] = os.pathsep.join([REPO, os.path.join(REPO, "resnet.mxnet_amd"), TESTS])
    path = str(tmp_path / (tag + ".npz"))
    cmd = [sys.executable, "-s", os.path.abspath(__file__), path] + ([str(gate)] if gate is not None else [])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    z = np.load(path)
    return {k: z[k] for k in z.files if k != "plan"}, json.loads(str(z["plan"]))


@pytest.mark.gpu
def test_executor_recompute_route(gpu, tmp_path):
    """RN_BN_BWD_RECOMPUTE unset against 0 (the stored path), deterministic mode, a fresh process each: updated
    parameters, gradients, BN statistics and probabilities bit for bit. The unset default recomputes from its size
    gate up; the child that stands for it here has the gate at this net's 32 KB gradient (ResNet-50's are above
    the shipped 64 MiB): unit 2's bn1 -- whose output gradient the streamed conv1 data gradient alone writes -- is
    recomputed, unit 1's (64 channels, two readers) is not. Unset with the shipped gate keeps the stored plan at
    this size (test_recompute_size_gate has the gate's edges and RN_BN_BWD_RECOMPUTE=1)."""
    new, plan_new = _run_child(tmp_path, "unset_gate", None, gate=GRAD_BYTES)
    dflt, plan_dflt = _run_child(tmp_path, "unset", None)
    old, plan_old = _run_child(tmp_path, "zero", "0")
    assert plan_new["recomputed"] == ["stage1_unit2_bn1"], plan_new["recomputed"]
    assert plan_new["bwd"].count("rn_conv_bwd_data_bnapply") == 1
    assert plan_new["bwd"].count("rn_bn_bwd_part") == plan_old["bwd"].count("rn_bn_bwd_part") - 1
    assert plan_old["recomputed"] == [] and "rn_conv_bwd_data_bnapply" not in plan_old["bwd"]
    assert plan_dflt["bwd"] == plan_old["bwd"]
    assert set(new) == set(old) == set(dflt)
    assert any(k.startswith("aux:") for k in new) and any(k.startswith("grad:") for k in new)
    for k in sorted(new):
        for a in (new[k], dflt[k]):
            b = old[k]
            assert a.dtype == b.dtype and a.shape == b.shape and np.isfinite(a).all(), k
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), k


# ---------------------------------------------------------------------------------------------- host
def _desc(n, c, h, w, k, stride=1):
    return conv_desc(BF16, n, c, h, w, k, 1, 1, stride, 0)


def test_dgrad_streamed_query():
    """rn_conv_dgrad_streamed: 1 for the conv1 data gradients of ResNet-50's stage-1 units 2-3 and stage-2 units
    2-4 at batch 256; 0 for K = 256, for stride 2, and once n h w c 2 bytes reach 2^31 (the kernel's buffer
    descriptors count bytes in 32-bit ints)."""
    from rn import graphs
    from rn.executor import Plan
    lib = L.load()
    q = lambda d: int(lib.rn_conv_dgrad_streamed(C.byref(d)))
    plan = Plan(graphs.resnet50(), [("data", (256, 3, 224, 224))], [("softmax_label", (256,))])
    names = ["stage1_unit2_conv1", "stage1_unit3_conv1", "stage2_unit2_conv1", "stage2_unit3_conv1",
             "stage2_unit4_conv1"]
    convs = {op.name: op for op in plan.ops if op.kind == "conv"}
    for nm in names:
        op = convs[nm]
        assert tuple(op.kernel) == (1, 1) and tuple(op.stride) == (1, 1)
        assert q(_desc(op.x.n, op.x.c, op.x.h, op.x.w, op.y.c)) == 1, nm
    assert q(_desc(256, 1024, 14, 14, 256)) == 0       # K = 256 (stage 3: the tiles)
    assert q(_desc(256, 512, 28, 28, 128, stride=2)) == 0
    assert q(_desc(255, 1024, 64, 64, 128)) == 1       # 2^31 - 2^23 bytes
    assert q(_desc(256, 1024, 64, 64, 128)) == 0       # 2^31 bytes
    assert q(_desc(512, 1024, 64, 64, 128)) == 0       # 2^32: past an int's wrap-around


def _live_bf16(numel):
    """Live bf16 tensors of `numel` elements anywhere in the process (whatever holds them)."""
    import gc
    import warnings
    gc.collect()
    with warnings.catch_warnings():  # (isinstance on torch's deprecated module attributes warns)
        warnings.simplefilter("ignore")
        return sum(1 for o in gc.get_objects()
                   if isinstance(o, torch.Tensor) and o.dtype == torch.bfloat16 and o.numel() == numel)


def test_recompute_size_gate(monkeypatch):
    """The default plan (RN_BN_BWD_RECOMPUTE unset) recomputes a streamed layer's BN only where the gradient it
    then never stores has at least Executor.RECOMPUTE_MIN_BYTES (64 MiB: ResNet-50 at batch 256 has 392 and 196 MiB
    there); 1 recomputes at any size, 0 never; any other value is refused. Dry run of the two-unit net (the
    gradient: 4 * 4 * 4 rows of 256 bf16 channels). A recomputed BN's output-gradient buffer is released: the bound
    executor keeps exactly one bf16 tensor of that size fewer alive than the stored plan's, and no writer records."""
    from rn.executor import Executor, Plan
    assert Executor.RECOMPUTE_MIN_BYTES == 64 << 20 <= 256 * 28 * 28 * 512 * 2

    def bind():
        p = Plan(_two_unit_net(), [("data", (4, 3, 16, 16))], [("softmax_label", (4,))], dtype="bfloat16")
        ex = Executor(p, "cpu")
        names = [c[0] for c in ex._bwd]
        got = [op.name for op in p.ops if op.kind == "bn" and op.recomputed]
        assert names.count("rn_conv_bwd_data_bnapply") == len(got) and ex._gw == {}
        for op in p.ops:
            if op.kind == "bn" and op.recomputed:
                assert op.y.numel * 2 == GRAD_BYTES and id(op.y) not in ex._grads
        return got, _live_bf16(GRAD_BYTES // 2), ex
    monkeypatch.delenv("RN_BN_BWD_RECOMPUTE", raising=False)
    got, live_stored, ex = bind()
    assert got == []
    del ex
    monkeypatch.setattr(Executor, "RECOMPUTE_MIN_BYTES", GRAD_BYTES)
    got, live_recomputed, ex = bind()
    assert got == ["stage1_unit2_bn1"]
    assert live_recomputed == live_stored - 1, (live_stored, live_recomputed)
    del ex
    monkeypatch.setattr(Executor, "RECOMPUTE_MIN_BYTES", GRAD_BYTES + 1)
    assert bind()[0] == []
    monkeypatch.setenv("RN_BN_BWD_RECOMPUTE", "1")
    got, live_forced, ex = bind()
    assert got == ["stage1_unit2_bn1"] and live_forced == live_stored - 1
    del ex
    monkeypatch.setenv("RN_BN_BWD_RECOMPUTE", "0")
    monkeypatch.setattr(Executor, "RECOMPUTE_MIN_BYTES", 0)
    assert bind()[0] == []
    monkeypatch.setenv("RN_BN_BWD_RECOMPUTE", "yes")
    with pytest.raises(L.RNError):
        bind()


if __name__ == "__main__":
    _child(*sys.argv[1:3])
