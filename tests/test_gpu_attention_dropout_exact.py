"""-m gpu: the exact form of the 16-bit Attention probability dropout (dyf_set_attention_dropout(DYF_ATTN_DROPOUT_EXACT)).

In exact mode a 16-bit engine draws nn.Dropout(p)'s keep bits from the stream of the fp32 / training path: the row's site key, element
(h * N + i) * N + j of the row's (4, N, N) probabilities, 16-bit slice of its pair word against floor((1 - p) * 65536), survivors scaled
by 1 / (1 - p) -- tests/rng_host.py row_mask_nhwc((4, N, N), ...) on the host.  Checked here

  1. bit for bit, mask by mask, on each of the three Attention kernels (the form is forced and read back from the form log);
  2. against the fp32 core on the engine's own generator (same masks, 16-bit rounding apart);
  3. on whole unet.Unet forwards and rollouts against the oracle on host-rebuilt masks and against an fp32 engine;
  4. in its plumbing: row offsets, graph replay, switching the mode of a live engine, the C ABI's refusals, injected masks.

Tolerances are the ones the 16-bit paths are already held to: the dropout-free core's 2e-3 (fp16) / 1e-2 (bf16) of
tests/test_gpu_fp16.py, per forward 2.5e-3 (fp16, tests/test_gpu_fp16.py) / 2e-2 (bf16, tests/test_gpu_unet_resnet.py), rollouts 1e-2 / 2.5e-2."""
import numpy as np
import pytest
import torch

import dyffusion_amd as D
from dyffusion_amd import _lib as L
from oracle import nets, sampler
from tests.gpu_common import DEV, cached
from tests.helpers import rel_rms
from tests.rng_host import ResnetEngineDropout, row_mask_nhwc
from tests.test_gpu_unet_resnet import engine_masks, mirror, seeded_unet

pytestmark = pytest.mark.gpu
DTYPES = ["fp16", "bf16"]
TOL_CORE = {"fp16": 2e-3, "bf16": 1e-2}
TOL_FORWARD = {"fp16": 2.5e-3, "bf16": 2e-2}
TOL_ROLLOUT = {"fp16": 1e-2, "bf16": 2.5e-2}
HALF_ULP = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8}  # relative rounding of the output type (round to nearest)


@pytest.fixture(scope="module")
def engines():
    cfg = D.resnet_net_config(in_channels=2, cond_channels=0, out_channels=1, dim=64, dim_mults=(1, 2))
    made = {}

    def get(dtype):
        if dtype not in made:
            made[dtype] = D.HipEngine(cfg, cfg, 16, 16, max_batch=2, use_graph=False, dtype=dtype, attention_dropout="exact")
        return made[dtype]

    yield get
    for e in made.values():
        e.close()


# ------------------------------------------------------------------------------------------------ 1. masks, bit for bit
KERNEL_CASES = [("attention_kernel<exact>", 0, n) for n in (1, 33, 65)] + \
               [("flash_attention2_kernel<QB=1,exact>", 2, n) for n in (2, 31, 33, 130, 225)] + \
               [("flash_attention4_kernel<NW=4,exact>", 4, n) for n in (128, 384)] + \
               [("flash_attention4_kernel<NW=8,exact>", 4, n) for n in (512, 768)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form,flash,N", KERNEL_CASES, ids=[f"{f.split('<')[0]}-{f.split('<')[1][:-1]}-N{n}" for f, _, n in KERNEL_CASES])
def test_exact_masks_equal_the_host_restatement_bit_for_bit(engines, form_switch, dtype, form, flash, N):
    """q = k = 0 makes every probability 1 / N; V one-hot over a block of 32 keys makes out[i, h * 32 + c] = keep(i, j0 + c) * scale / N:
    one launch per key block (the generator re-seeded before each, so every launch draws forward 0) recovers the engine's whole keep
    tensor (nb, 4, N, N).  nb = 3 rows at row offset 5."""
    eng = engines(dtype)
    assert eng.attention_dropout == "exact"
    form_switch.setenv("DYF_FLASH_ATTN", str(flash))
    nb, grow, seed = 3, 5, 20261019 + N
    eng.set_row_offset(grow)
    try:
        for p in (0.1, 0.7):
            keep = torch.zeros(nb, 4, N, N, dtype=torch.bool)
            vals = []
            eng.form_log(True)
            for j0 in range(0, N, 32):
                w = min(32, N - j0)
                qkv = torch.zeros(nb, N, 384, dtype=eng.torch_dtype)
                for h in range(4):
                    qkv[:, torch.arange(j0, j0 + w), 256 + h * 32 + torch.arange(w)] = 1.0
                eng.seed(seed)
                out = eng.op_attention(qkv.to(DEV), p_drop=p).float().cpu().reshape(nb, N, 4, 32)[..., :w]  # (nb, i, h, c)
                keep[:, :, :, j0:j0 + w] = (out != 0).permute(0, 2, 1, 3)
                vals.append(out[out != 0])
            log = eng.form_log_read()
            eng.form_log(False)
            assert list(log) == [form] and log[form] == {nb: (N + 31) // 32}, log
            want = torch.from_numpy(np.stack([row_mask_nhwc((4, N, N), p, seed, 0, 0, grow + r) for r in range(nb)]))
            wrong = int((keep != want).sum())
            print(f"{form} {dtype} N={N} p={p}: kept {float(keep.float().mean()):.4f}, bits differing from the host restatement: {wrong}")
            assert wrong == 0
            vals = torch.cat(vals).double()
            expect = (1.0 / N) / (1.0 - p)
            worst = float(((vals - expect).abs() / expect).max()) if vals.numel() else 0.0
            print(f"    survivors: worst relative distance from (1/N) / (1 - p) = {worst:.3e} (half ulp {HALF_ULP[dtype]:.3e})")
            assert worst <= HALF_ULP[dtype] + 1e-6  # (1e-6: the fp32 arithmetic before the output is rounded)
    finally:
        eng.form_log(False)
        eng.set_row_offset(0)


# ------------------------------------------------------------------------------------------------ 2. same masks as fp32
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [33, 128, 225, 512])
def test_exact_mode_matches_the_fp32_core_on_the_engines_generator(engines, dtype, N):
    eng = engines(dtype)
    nb, p, seed = 2, 0.3, 77 + N
    qkv = (torch.randn(nb, N, 384, generator=torch.Generator().manual_seed(N)) * 1.5).to(eng.torch_dtype).to(DEV)

    def arm():
        eng.seed(seed)
        eng.set_row_offset(3)

    try:
        arm()
        want = eng.op_attention_f32(qkv.float().contiguous(), p_drop=p).cpu()
        arm()
        got = eng.op_attention(qkv, p_drop=p).float().cpu()
        eng.set_attention_dropout("fast")
        arm()
        fast = eng.op_attention(qkv, p_drop=p).float().cpu()
    finally:
        eng.set_attention_dropout("exact")
        eng.set_row_offset(0)
    err, err_fast = rel_rms(got, want), rel_rms(fast, want)
    print(f"N={N} {dtype}: 16-bit core vs fp32 core on the engine's generator, rel-rms exact {err:.3e} (fast mode, other masks: {err_fast:.3e})")
    assert err <= TOL_CORE[dtype]


# ------------------------------------------------------------------------------------------------ 3. network level
MCFG_I = dict(dim=64, dim_mults=[1, 2], with_time_emb=True, block_dropout=0.3, block_dropout1=0.0, attn_dropout=0.6,
              resnet_block_groups=8, input_dropout=0.0, upsample_dims=None)
MCFG_F = dict(MCFG_I, block_dropout=0.0, attn_dropout=0.0)
HP = dict(timesteps=4, forward_conditioning="none", interpolate_before_t1=True, schedule="before_t1_only", sampling_type="cold",
          refine_intermediate_predictions=False, enable_interpolator_dropout=True)
GRIDS = [((30, 30), 225, "flash_attention2_kernel<QB=1,exact>"), ((32, 16), 128, "flash_attention4_kernel<NW=4,exact>"),
         ((64, 32), 512, "flash_attention4_kernel<NW=8,exact>")]
NB, SEED, GROW = 2, 4242, 3


def _weights():
    return seeded_unet(64, (1, 2), 2, 2, seed=71), seeded_unet(64, (1, 2), 4, 2, seed=72)


def _inputs(hw):
    g = torch.Generator().manual_seed(hw[0] * 100 + hw[1])
    return torch.randn(NB, 2, *hw, generator=g), torch.randn(NB, 4, *hw, generator=g), torch.tensor([1.0, 2.5])


def _oracle_forward(hw, tokens):
    def run():
        _, PI = _weights()
        _, xi, t = _inputs(hw)
        drop = ResnetEngineDropout(SEED, tokens, row_offset=GROW)
        drop.begin_forward()
        with torch.no_grad():
            return nets.resnet_unet_forward(PI, MCFG_I, xi, t, None, dropout=drop)
    return cached(f"attn_exact_forward_{hw[0]}x{hw[1]}", run)


def _oracle_rollout(hw, tokens):
    def run():
        PF, PI = _weights()
        x0, _, _ = _inputs(hw)
        drop = ResnetEngineDropout(SEED, tokens, row_offset=GROW)

        def i_fn(x, t, cond):
            drop.begin_forward()
            return nets.resnet_unet_forward(PI, MCFG_I, x, t, cond, dropout=drop)

        with torch.no_grad():
            return sampler.sample_loop(lambda x, t, cond: nets.resnet_unet_forward(PF, MCFG_F, x, t, cond), i_fn, x0, None, HP)
    return cached(f"attn_exact_rollout_{hw[0]}x{hw[1]}", run)


def _model(dtype, mode="exact", **kw):
    PF, PI = _weights()
    opts = dict(max_batch=NB, dtype=dtype, attention_dropout=mode)
    opts.update(kw)
    return D.DYffusion(mirror(PF, MCFG_F, 2, 0, 2), D.InterpolatorHandle(mirror(PI, MCFG_I, 4, 0, 2), 4), **opts, **HP)


def _rollout(m, x0, seed=SEED, offset=GROW):
    m.seed(seed)
    m.set_row_offset(offset)
    return {k: v.clone() for k, v in m.sample(x0).items()}


def _engine_rollout(dtype, hw):
    """one rollout per (dtype, grid) for the tests of this module that compare it with something"""
    def run():
        m = _model(dtype)
        m._ensure_engine(hw, NB).form_log(True)
        got = {k: v.cpu() for k, v in _rollout(m, _inputs(hw)[0].to(DEV)).items()}
        got["__forms__"] = sorted(m._engine.form_log_read())
        m._engine.form_log(False)
        m._engine.close()
        return got
    return cached(f"attn_exact_engine_rollout_{dtype}_{hw[0]}x{hw[1]}", run)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw,tokens,form", GRIDS, ids=["30x30-225tok", "32x16-128tok", "64x32-512tok"])
def test_rng_mode_forward_equals_the_oracle_on_host_rebuilt_masks(hw, tokens, form, dtype):
    _, PI = _weights()
    _, xi, t = _inputs(hw)
    net = mirror(PI, MCFG_I, 4, 0, 2, dtype)
    net.engine_attention_dropout = "exact"
    eng = net._own_engine(NB, hw)
    assert eng.attention_dropout == "exact" and eng.dtype == dtype
    eng.seed(SEED)
    eng.set_row_offset(GROW)
    eng.form_log(True)
    with net.inference_dropout_scope(True):
        got = net(xi.to(DEV), time=t.to(DEV)).cpu()
    forms = eng.form_log_read()
    eng.form_log(False)
    assert form in forms and not any(k.startswith(("flash_attention", "attention_kernel")) and "exact" not in k for k in forms), sorted(forms)
    err = rel_rms(got, _oracle_forward(hw, tokens))
    print(f"{hw} {dtype}: rng-mode forward, exact attention dropout, vs oracle on host-rebuilt masks: rel-rms {err:.3e}")
    eng.close()
    assert err <= TOL_FORWARD[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw,tokens,form", GRIDS, ids=["30x30-225tok", "32x16-128tok", "64x32-512tok"])
def test_rng_mode_rollout_equals_the_oracle_on_host_rebuilt_masks(hw, tokens, form, dtype):
    got = _engine_rollout(dtype, hw)
    want = _oracle_rollout(hw, tokens)
    assert form in got["__forms__"], got["__forms__"]
    assert sorted(k for k in got if k != "__forms__") == sorted(want)
    worst = max(rel_rms(got[k], want[k]) for k in want)
    print(f"{hw} {dtype}: T = 4 rollout, exact attention dropout, vs oracle on host-rebuilt masks: worst rel-rms {worst:.3e}")
    assert worst <= TOL_ROLLOUT[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw,tokens,form", GRIDS, ids=["30x30-225tok", "32x16-128tok", "64x32-512tok"])
def test_exact_rollout_matches_the_fp32_engine_on_the_same_seed(hw, tokens, form, dtype):
    def run32():
        m = _model("fp32", mode="fast")  # (the fp32 path does not depend on the mode)
        out = {k: v.cpu() for k, v in _rollout(m, _inputs(hw)[0].to(DEV)).items()}
        m._engine.close()
        return out
    want = cached(f"attn_exact_fp32_rollout_{hw[0]}x{hw[1]}", run32)
    got = _engine_rollout(dtype, hw)
    worst = max(rel_rms(got[k], want[k]) for k in want)
    print(f"{hw} {dtype}: T = 4 rollout, exact attention dropout, vs an fp32 engine on the same seed: worst rel-rms {worst:.3e}")
    assert worst <= TOL_ROLLOUT[dtype]


# ------------------------------------------------------------------------------------------------ 4. invariance and plumbing
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_do_not_depend_on_batching_and_graph_replay_equals_eager(dtype):
    hw = (30, 30)
    g = torch.Generator().manual_seed(8)
    x0 = torch.randn(4, 2, *hw, generator=g).to(DEV)

    def run(rows, offset, use_graph):
        m = _model(dtype, max_batch=4, batch_invariant=True, use_graph=use_graph)
        out = _rollout(m, x0[rows], offset=offset)
        assert m._engine.attention_dropout == "exact"
        m._engine.close()
        return out

    full, eager = run(slice(0, 4), 0, True), run(slice(0, 4), 0, False)
    lo, hi = run(slice(0, 2), 0, True), run(slice(2, 4), 2, True)
    for k in full:
        assert torch.equal(full[k], eager[k]), k
        assert torch.equal(full[k][:2], lo[k]) and torch.equal(full[k][2:], hi[k]), k
    assert not torch.equal(full["t4_preds"][0], full["t4_preds"][1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_switching_the_mode_of_a_live_engine(dtype):
    hw = (32, 16)
    x0 = _inputs(hw)[0].to(DEV)
    m = _model(dtype, mode="fast", use_graph=True)
    fast1 = _rollout(m, x0)
    eng = m._engine
    assert eng.attention_dropout == "fast"
    m.set_attention_dropout("exact")
    assert eng.attention_dropout == "exact" and m._engine is eng
    exact1 = _rollout(m, x0)
    fresh = _model(dtype, mode="exact", use_graph=True)
    exact2 = _rollout(fresh, x0)
    m.set_attention_dropout("fast")
    fast2 = _rollout(m, x0)
    for k in fast1:
        assert torch.equal(exact1[k], exact2[k]), k   # the graph captured in fast mode was not replayed
        assert torch.equal(fast1[k], fast2[k]), k     # ... and the fast one came back
        assert not torch.equal(fast1[k], exact1[k]), k
    fresh._engine.close()
    eng.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_c_abi_defaults_and_refusals(dtype, form_switch):
    cfg = D.resnet_net_config(in_channels=2, cond_channels=0, out_channels=1, dim=64, dim_mults=(1, 2))
    eng = D.HipEngine(cfg, cfg, 16, 16, max_batch=1, use_graph=False, dtype=dtype)
    lib = eng._lib
    assert lib.dyf_attention_dropout(eng._h) == L.ATTN_DROPOUT_FAST and eng.attention_dropout == "fast"
    for bad in (-1, 2, 7):
        assert lib.dyf_set_attention_dropout(eng._h, bad) == L.DYF_ERR_INVALID_ARGUMENT
        assert lib.dyf_attention_dropout(eng._h) == L.ATTN_DROPOUT_FAST
    with pytest.raises(ValueError):
        eng.set_attention_dropout("EXACT")
    assert lib.dyf_set_attention_dropout(eng._h, L.ATTN_DROPOUT_EXACT) == L.DYF_OK
    assert lib.dyf_attention_dropout(eng._h) == L.ATTN_DROPOUT_EXACT
    # 32 768 tokens: one past the 32-bit element index of the exact form -- refused before anything is launched (the output pointer is
    # the input's: nothing is written, and the 25 MB input stays the only allocation)
    qkv = torch.zeros(1, 32768, 384, dtype=eng.torch_dtype, device=DEV)
    eng.form_log(True)
    st = lib.dyf_op_attention_dropout(eng._h, qkv.data_ptr(), 1, 32768, 0.1, qkv.data_ptr(), None)
    assert st == L.DYF_ERR_UNSUPPORTED and eng.form_log_read() == {}
    assert "32767" in lib.dyf_last_error(eng._h).decode()
    eng.form_log(False)
    del qkv
    # engines without a unet.Unet accept the call
    scfg = D.net_config(in_channels=3, cond_channels=0, out_channels=3, dim=64, upsample_dims=[64, 64])
    se = D.HipEngine(scfg, scfg, 16, 16, max_batch=1, use_graph=False, dtype=dtype, attention_dropout="exact")
    assert se.attention_dropout == "exact"
    se.close()
    eng.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_injected_masks_do_not_depend_on_the_mode(dtype):
    hw = (32, 16)
    _, PI = _weights()
    _, xi, t = _inputs(hw)
    src = nets.DropoutSeeded(11, record=True)
    with torch.no_grad():
        nets.resnet_unet_forward(PI, MCFG_I, xi, t, None, dropout=src)
    net = mirror(PI, MCFG_I, 4, 0, 2, dtype)
    eng = net._own_engine(NB, hw)
    outs = {}
    for mode in ("fast", "exact"):
        eng.set_attention_dropout(mode)
        outs[mode] = eng.net_forward(0, xi.to(DEV), t.to(DEV), None, dropout_mode=2, masks=engine_masks(src.masks, 2)).clone()
    assert torch.equal(outs["fast"], outs["exact"])
    eng.close()
