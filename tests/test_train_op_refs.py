"""The float64 references of tests/train_op_refs.py (what tests/test_gpu_train_ops.py holds the training kernels to) against
independent formulations -- torch.nn.functional and the oracle's own layer functions, which goldens pin to the reference project --
to 1e-10 in float64; and the proof that the GPU test's bound bites: deliberate mutants of a reference, on the GPU test's own inputs,
each miss it by at least 10 x.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

from oracle import nets
from tests import train_op_refs as T
from tests.helpers import rel_rms

EXACT = 1e-10


def nchw(x):
    return x.permute(0, 3, 1, 2)


def nhwc(x):
    return x.permute(0, 2, 3, 1)


def r64(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def close(a, b, what=""):
    err = rel_rms(a.detach(), b.detach())
    assert err <= EXACT, (what, err)


def grads_close(ya, yb, leaves, what):
    d = r64(*ya.shape, seed=99)
    for ga, gb in zip(torch.autograd.grad(ya, leaves, d), torch.autograd.grad(yb, leaves, d)):
        close(ga, gb, what + " gradient")


@pytest.mark.parametrize("C,groups,film,p", [(8, 8, 0, 0.0), (24, 8, 1, 0.2), (64, 8, 1, 0.0), (512, 8, 0, 0.2)])
def test_gn_act_is_group_norm_film_silu(C, groups, film, p):
    z, gamma, beta = r64(3, 5, 7, C, seed=1, scale=1.5).requires_grad_(), r64(C, seed=2).requires_grad_(), r64(C, seed=3).requires_grad_()
    ss = r64(3, 2 * C, seed=4, scale=0.5).requires_grad_() if film else None
    keep = (torch.rand(3, 5, 7, C, generator=torch.Generator().manual_seed(5)) >= p).double() if p else None
    want = F.group_norm(nchw(z), groups, gamma, beta, eps=1e-5)
    if film:
        want = want * (ss[:, :C, None, None] + 1) + ss[:, C:, None, None]
    want = nhwc(F.silu(want))
    if p:
        want = want * keep / (1 - p)
    got = T.gn_act(z, gamma, beta, groups, ss, keep, p)
    close(got, want, "gn_act")
    grads_close(got, want, [z, gamma, beta] + ([ss] if film else []), "gn_act")


@pytest.mark.parametrize("k,s,pd,ci,co,ws", [(L[0], L[1], L[2], L[3], L[4], L[5]) for L in T.CONV_LAYERS] + [(4, 2, 1, 64, 64, 0)])
@pytest.mark.parametrize("h,w", [(11, 13), (12, 16)])
def test_conv_is_conv2d_on_the_standardised_weight(k, s, pd, ci, co, ws, h, w):
    x, wt, b = r64(2, h, w, ci, seed=1).requires_grad_(), r64(co, ci, k, k, seed=2).requires_grad_(), r64(co, seed=3).requires_grad_()
    wh = wt
    if ws:
        wh = (wt - wt.mean((1, 2, 3), keepdim=True)) * (wt.var((1, 2, 3), unbiased=False, keepdim=True) + 1e-5).rsqrt()
    want = nhwc(F.conv2d(nchw(x), wh, b, stride=s, padding=pd))
    got = T.conv(x, wt, b, s, pd, bool(ws))
    close(got, want, "conv")
    grads_close(got, want, [x, wt, b], "conv")


@pytest.mark.parametrize("n", [1, 63, 65])
def test_attention_is_scaled_dot_product_attention(n):
    qkv = r64(2, 1, n, 384, seed=n, scale=1.5).requires_grad_()
    q, k, v = (qkv[..., i * 128:(i + 1) * 128].reshape(2, n, 4, 32).transpose(1, 2) for i in range(3))
    want = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(2, 1, n, 128)
    got = T.attention(qkv)
    close(got, want, "attention")
    grads_close(got, want, [qkv], "attention")


def attn_params(C, seed, linear):
    qk = "m.fn.fn.to_qkv.1.weight" if linear else "m.fn.fn.to_qkv.weight"
    return {"m.fn.norm.g": 1 + r64(1, C, 1, 1, seed=seed, scale=0.3), qk: r64(384, C, 1, 1, seed=seed + 1, scale=C ** -0.5),
            "m.fn.fn.to_out.weight": r64(C, 128, 1, 1, seed=seed + 2, scale=0.1), "m.fn.fn.to_out.bias": r64(C, seed=seed + 3)}, qk


@pytest.mark.parametrize("C,h,w,p", [(24, 3, 11, 0.0), (64, 15, 15, 0.1)])
def test_linear_attention_block_is_the_oracles(C, h, w, p):
    """LayerNorm -> Dropout -> to_qkv -> core -> to_out -> + x, from the op references, against oracle.nets._linear_attention."""
    P, qk = attn_params(C, 10, True)
    x = r64(2, h, w, C, seed=20, scale=1.5)
    keep = (torch.rand(2, h, w, C, generator=torch.Generator().manual_seed(6)) >= p).double()
    want = nhwc(nets._linear_attention(P, "m", nchw(x), 4, 32, p, nets.DropoutFromList([nchw(keep)])))
    ln = T.layernorm(x, P["m.fn.norm.g"], keep if p else None, p)
    close(T.layernorm(x, P["m.fn.norm.g"]), nhwc(nets._channel_layernorm(nchw(x), P["m.fn.norm.g"])), "layernorm")
    got = T.conv(T.linattn(T.conv(ln, P[qk])), P["m.fn.fn.to_out.weight"], P["m.fn.fn.to_out.bias"]) + x
    close(got, want, "linear attention block")


@pytest.mark.parametrize("C,h,w,p", [(24, 3, 11, 0.0), (64, 5, 13, 0.15)])
def test_attention_block_is_the_oracles(C, h, w, p):
    P, qk = attn_params(C, 30, False)
    x = r64(2, h, w, C, seed=40, scale=1.5)
    n = h * w
    keep = (torch.rand(2, 4, n, n, generator=torch.Generator().manual_seed(7)) >= p).double()
    want = nhwc(nets._full_attention(P, "m", nchw(x), 4, 32, p, nets.DropoutFromList([keep])))
    core = T.attention(T.conv(T.layernorm(x, P["m.fn.norm.g"]), P[qk]), keep if p else None, p)
    close(T.conv(core, P["m.fn.fn.to_out.weight"], P["m.fn.fn.to_out.bias"]) + x, want, "attention block")


@pytest.mark.parametrize("cin,cout,film", [(8, 8, 1), (24, 40, 1), (40, 24, 0)])
def test_resnet_block_is_the_oracles(cin, cout, film):
    """ws-conv -> GroupNorm + FiLM (SiLU -> Linear) + SiLU + Dropout, twice, + residual 1x1 conv, against oracle.nets._resnet_block."""
    P = {}
    for i, (a, b) in enumerate(((cin, cout), (cout, cout))):
        P[f"b.block{i + 1}.proj.weight"], P[f"b.block{i + 1}.proj.bias"] = r64(b, a, 3, 3, seed=50 + i, scale=0.2), r64(b, seed=52 + i)
        P[f"b.block{i + 1}.norm.weight"], P[f"b.block{i + 1}.norm.bias"] = 1 + r64(b, seed=54 + i, scale=0.3), r64(b, seed=56 + i)
    if film:
        P["b.mlp.1.weight"], P["b.mlp.1.bias"] = r64(2 * cout, 16, seed=58, scale=0.2), r64(2 * cout, seed=59, scale=0.2)
    if cin != cout:
        P["b.residual_conv.weight"], P["b.residual_conv.bias"] = r64(cout, cin, 1, 1, seed=60, scale=0.3), r64(cout, seed=61)
    x, temb = r64(2, 7, 9, cin, seed=62, scale=1.5), r64(2, 16, seed=63)
    keeps = [(torch.rand(2, 7, 9, cout, generator=torch.Generator().manual_seed(70 + i)) >= 0.2).double() for i in range(2)]
    want = nhwc(nets._resnet_block(P, "b", nchw(x), temb if film else None, 8, 0.2, 0.2, nets.DropoutFromList([nchw(k) for k in keeps])))
    close(T.conv(x, P["b.block1.proj.weight"], P["b.block1.proj.bias"], 1, 1, True),
          nhwc(nets._ws_conv3x3(P, "b.block1.proj", nchw(x))), "ws conv")
    ss = T.linear(temb, P["b.mlp.1.weight"], P["b.mlp.1.bias"], True) if film else None
    h1 = T.gn_act(T.conv(x, P["b.block1.proj.weight"], P["b.block1.proj.bias"], 1, 1, True), P["b.block1.norm.weight"], P["b.block1.norm.bias"], 8, ss,
                  keeps[0], 0.2)
    h2 = T.gn_act(T.conv(h1, P["b.block2.proj.weight"], P["b.block2.proj.bias"], 1, 1, True), P["b.block2.norm.weight"], P["b.block2.norm.bias"], 8, None,
                  keeps[1], 0.2)
    res = T.conv(x, P["b.residual_conv.weight"], P["b.residual_conv.bias"]) if cin != cout else x
    close(h2 + res, want, "resnet block")


def test_small_ops_are_torchs():
    x = r64(3, 3, 5, 8, seed=80, scale=1.5)
    close(T.gelu(x), F.gelu(x), "gelu")
    close(T.up2_nearest(x), nhwc(F.interpolate(nchw(x), scale_factor=2, mode="nearest")), "up2_nearest")
    w, b = r64(6, 8, seed=81), r64(6, seed=82)
    close(T.linear(x[0, 0], w, b, True), F.linear(F.silu(x[0, 0]), w, b), "linear")
    t, fw = torch.rand(3, dtype=torch.float64), r64(5, seed=83)
    # the oracle's time embedding with an identity first Linear and the GELU undone is its feature vector (t.float() is exact here)
    t = t.float().double()
    P = {"e.0.weights": fw, "e.1.weight": torch.eye(11, dtype=torch.float64), "e.1.bias": torch.zeros(11, dtype=torch.float64),
         "e.3.weight": torch.eye(11, dtype=torch.float64), "e.3.bias": torch.zeros(11, dtype=torch.float64)}
    close(F.gelu(T.learned_sinu(t, fw)), nets.time_embedding(P, "e", t, 0), "learned_sinu")


# ---- unet_simple's ops
@pytest.mark.parametrize("kind", T.US_KINDS)
@pytest.mark.parametrize("C,act,film,p", [(8, "leaky", 0, 0.0), (24, "relu", 1, 0.1), (64, "leaky", 1, 0.0)])
def test_norm_act_is_the_oracles_block_tail(kind, C, act, film, p):
    """BatchNorm2d / GroupNorm(8) -> FiLM -> (Leaky)ReLU -> Dropout against torch.nn.functional and the oracle's unet_simple layer
    functions (nets._norm, nets.film); the running statistics against torch.nn.BatchNorm2d(momentum=0.1)."""
    z, gamma, beta = r64(3, 5, 7, C, seed=1, scale=1.5).requires_grad_(), (1 + r64(C, seed=2, scale=0.3)).requires_grad_(), r64(C, seed=3).requires_grad_()
    rmean, rvar = r64(C, seed=4, scale=0.5), 0.5 + torch.rand(C, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    temb = r64(3, 16, seed=6)
    P = {"n.weight": gamma, "n.bias": beta, "n.running_mean": rmean, "n.running_var": rvar,
         "t.1.weight": r64(2 * C, 16, seed=7, scale=0.2).requires_grad_(), "t.1.bias": r64(2 * C, seed=8, scale=0.2).requires_grad_()}
    keep = (torch.rand(3, 5, 7, C, generator=torch.Generator().manual_seed(9)) >= p).double() if p else None
    want = nets._norm(P, "n", nchw(z), "gn" if kind == "gn8" else "bn", kind == "bn_batch")
    if film:
        scale, shift = nets.film(P, "t", temb)
        want = want * (scale + 1) + shift
    want = nhwc(F.leaky_relu(want, nets.LEAKY_SLOPE) if act == "leaky" else F.relu(want))
    if p:
        want = want * keep / (1 - p)
    ss = T.linear(temb, P["t.1.weight"], P["t.1.bias"], True) if film else None
    got = T.norm_act(z, gamma, beta, rmean, rvar, 8 if kind == "gn8" else 0, kind == "bn_running", act, ss, keep, p)
    close(got, want, "norm_act")
    grads_close(got, want, [z, gamma, beta] + ([P["t.1.weight"], P["t.1.bias"]] if film else []), "norm_act")
    if kind == "bn_batch":
        bn = torch.nn.BatchNorm2d(C, momentum=0.1).double().train()
        with torch.no_grad():
            bn.running_mean.copy_(rmean)
            bn.running_var.copy_(rvar)
            bn(nchw(z))
        m, v = T.bn_running_update(z.detach(), rmean, rvar)
        close(m, bn.running_mean, "running_mean")
        close(v, bn.running_var, "running_var")


@pytest.mark.parametrize("h,w,oh,ow", [(11, 13, 16, 16), (16, 16, 11, 13), (5, 4, 10, 8), (1, 1, 2, 2), (7, 9, 7, 9)])
def test_resize_and_up2_are_interpolate(h, w, oh, ow):
    x = r64(2, h, w, 8, seed=h * w, scale=1.5).requires_grad_()
    for nearest in (False, True):
        want = nhwc(F.interpolate(nchw(x), size=(oh, ow), mode="nearest" if nearest else "bilinear"))
        got = T.resize(x, oh, ow, nearest)
        close(got, want, "resize")
        grads_close(got, want, [x], "resize")
    if (oh, ow) == (2 * h, 2 * w):
        a, b = x[..., :3], x[..., 3:]
        want = nhwc(F.interpolate(torch.cat([nchw(a), nchw(b)], 1), scale_factor=2, mode="bilinear"))
        close(T.up2_bilinear(a, b), want, "up2_bilinear of two sources")
        close(T.up2_bilinear(x), want, "up2_bilinear")
        grads_close(T.up2_bilinear(a, b), want, [x], "up2_bilinear")


def test_resize_is_the_oracles_explicit_formula():
    """nets.bilinear_resize_explicit is written in float32 (its weights are float32 numbers): on float64 data it is held to float32's eps."""
    x = r64(2, 11, 13, 5, seed=3)
    err = rel_rms(T.resize(x, 16, 16), nhwc(nets.bilinear_resize_explicit(nchw(x), 16, 16)).double())
    assert err <= 1e-6, err


@pytest.mark.parametrize("d,C,h,w", [(8, 1, 4, 4), (8, 3, 11, 13), (64, 3, 5, 7)])
def test_conv_transpose4s2_is_conv_transpose2d(d, C, h, w):
    x, wt, b = r64(2, h, w, d, seed=1).requires_grad_(), r64(d, C, 4, 4, seed=2, scale=0.2).requires_grad_(), r64(C, seed=3).requires_grad_()
    want = nhwc(F.conv_transpose2d(nchw(x), wt, b, stride=2, padding=1))
    got = T.conv_transpose4s2(x, wt, b)
    close(got, want, "conv_transpose4s2")
    grads_close(got, want, [x, wt, b], "conv_transpose4s2")


# ---- the bound bites: each mutant, on the inputs of the GPU cases it can show at, misses TOL by at least 10 x in some compared tensor
def _where(op, pred):
    return [pytest.param(op, args, id=f"{op}-{cid}") for cid, args in T.specs(op) if pred(args)]


MUTANTS = {
    # the last pixel of the last 32-pixel chunk left out of the k-softmax statistics
    "kstat_last_pixel": _where("linattn", lambda a: a[0] > 1),
    "v_not_over_hw": _where("linattn", lambda a: a[0] > 1),
    "second_split": _where("linattn", lambda a: a[0] > 256),
    "dv_without_keep": _where("attention", lambda a: a[2] > 0),
    # n / (n - 1) moves rstd by 1 / (2 (n - 1)): shown where a statistic has n <= 1000 elements (>= 5e-4), which every LayerNorm and
    # weight-standardised case has and the GroupNorm cases of few pixels or few channels per group have; a group of ONE element (C = 8
    # at hw = 1) has no unbiased variance
    "unbiased": _where("layernorm", lambda a: True) + _where("gn_act", lambda a: 1 < a[1] * (a[0] // 8) <= 1000) + _where("conv", lambda a: a[5]),
    "quad_group": _where("gn_act", lambda a: a[0] == 24),
    # unet_simple's ops.  Per-sample statistics differ from the batch's wherever there is more than one sample and more than one pixel
    "per_sample_count": _where("norm_act", lambda a: a[0] == "bn_batch" and a[4] > 1 and a[2] * a[3] > 1),
    # cnt / (cnt - 1) moves the statistic's variance term by 1 / (cnt - 1): shown at every batch-statistics case of more than one value
    "biased_running_var": _where("norm_act", lambda a: a[0] == "bn_batch" and 1 < a[4] * a[2] * a[3] <= 2000),
    "skip_half_dropped": _where("up2_bilinear", lambda a: a[3] > 0),
    "no_half_pixel": _where("resize", lambda a: (a[0], a[1]) != (a[2], a[3]) and not a[4]),
    "taps_transposed": _where("convt", lambda a: True),
}


@pytest.mark.parametrize("mutant,op,args", [pytest.param(m, *p.values, id=f"{m}-{p.id}") for m, ps in MUTANTS.items() for p in ps])
def test_the_bound_tells_a_mutant_from_the_reference(mutant, op, args):
    case = T.build(op, args)
    keep = T.engine_keep(case)
    ref, mut = case.run(keep=keep), case.run(keep=keep, mutant=mutant)
    worst = max(rel_rms(mut[k], ref[k]) for k in ref if float(ref[k].abs().max()) > 0)
    assert worst >= 10 * T.TOL, f"{mutant} moves the worst tensor by {worst:.3e} only"
