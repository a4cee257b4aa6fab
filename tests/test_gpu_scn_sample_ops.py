"""-m gpu: the SimpleConvNet sampling path (csrc/simple_conv_net.hip) against float64 at its edge shapes -- H != W, kernels larger than the
grid, a first block with a residual, no time embedding, no condition, 1 and 6 blocks, dim % 8 != 0, per-row times, nb < max_batch --
in both builds (bf16, fp16) and at the three sampling precisions, with dropout off, injected masks and the engine generator's masks
rebuilt on the host; one block at a time through the conv seam (op_conv2d_ex, path 0); and a non-square generator-dropout rollout of a
SimpleConvNet pair against the oracle sampler.

References, cases and bounds: tests/scn_sample_refs.py (checked on the CPU by tests/test_scn_sample_refs.py).  No bound comes from the
code under test: 16 bit: rel_rms(engine, M64) <= floor = rel_rms(M64, E64); fp32 / bf16x3: rel_rms(engine, E64) <= 1e-5; a block:
excess <= floor.  Every test prints its worst value, the floor and the fp32-arithmetic baseline."""
import pytest
import torch

import dyffusion_amd as D
from oracle import init as oinit
from oracle import nets, sampler
from tests import scn_sample_refs as R
from tests import scn_train_refs as S
from tests.gpu_common import DEV
from tests.helpers import rel_rms
from tests.test_gpu_fp32_sampling import TOL32

pytestmark = pytest.mark.gpu
BUILDS = ("bf16", "fp16")
IDS = [c["id"] for c in R.CASES]
CASE_MODES = [(c["id"], mode) for c in R.CASES for mode in R.modes_of(c)]  # a case without dropout sites runs with dropout off only
DIRECT = "conv_direct_kernel"


def _net(dim, ks, p, n_in, n_cond, n_out, time_emb=True):
    return D.SimpleConvNet(dim=dim, with_time_emb=time_emb, kernel_sizes=ks, dropout=p, num_input_channels=n_in, num_output_channels=n_out,
                           num_conditional_channels=n_cond)


@pytest.fixture(scope="module")
def engines():
    """One engine per (case, build) for the whole module: the precision is switched on it."""
    made = {}

    def get(cid, build):
        if (cid, build) not in made:
            c = R.CASE[cid]
            cfg = _net(c["dim"], c["ks"], c["p"], c["n_in"], c["n_cond"], c["n_out"], c["time_emb"]).engine_net_config()
            eng = D.HipEngine(cfg, cfg, c["h"], c["w"], max_batch=c["max_batch"], use_graph=False, dtype=build)
            eng.load_weights(0, R.build(cid)["P"])
            made[(cid, build)] = eng
        return made[(cid, build)]
    yield get
    for eng in made.values():
        eng.close()


def _forward(eng, cid, mode):
    """-> {reference mode: output}: one forward, or for "gen" the first and the second forward after seed() at row offset ROW_OFFSET."""
    b = R.build(cid)
    dev = lambda v: None if v is None else v.to(DEV)
    x, t, c = dev(b["x"]), dev(b["t"]), dev(b["c"])
    if mode == "off":
        return {"off": eng.net_forward(0, x, t, c).cpu()}
    if mode == "mask":
        return {"mask": eng.net_forward(0, x, t, c, dropout_mode=2, masks=[k.to(DEV) for k in b["keeps"]]).cpu()}
    eng.seed(R.SEED)
    eng.set_row_offset(R.ROW_OFFSET)
    try:
        return {"gen": eng.net_forward(0, x, t, c, dropout_mode=1).cpu(), "gen1": eng.net_forward(0, x, t, c, dropout_mode=1).cpu()}
    finally:
        eng.set_row_offset(0)


# ------------------------------------------------------------------------------------------------ the whole forward, 16 bit
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("cid,mode", CASE_MODES, ids=lambda v: v)
def test_forward_16bit_sits_within_the_storage_floor_of_the_rounding_model(engines, cid, mode, build):
    case = R.CASE[cid]
    eng = engines(cid, build)
    eng.set_sample_precision(16)
    if mode == "off":  # every block is one launch of the direct kernel
        eng.form_log(True)
        try:
            outs = _forward(eng, cid, mode)
            forms = eng.form_log_read()
        finally:
            eng.form_log(False)
        assert {k: v for k, v in forms.items() if k.startswith("conv_")} == {DIRECT: {case["nb"]: len(case["ks"])}}, forms
    else:
        outs = _forward(eng, cid, mode)
    for ref_mode, got in outs.items():
        e64, m64, floor = R.refs(cid, build, ref_mode)
        m32 = rel_rms(R.rounded(cid, build, ref_mode, torch.float32), m64)
        err = rel_rms(got, m64)
        print(f"[scn16] {cid} {build} {ref_mode}: engine vs M64 {err:.3e} = {err / floor:.3f} floors (floor {floor:.3e}; M32 {m32 / floor:.3f} floors; "
              f"engine vs E64 {rel_rms(got, e64):.3e})")
        assert torch.isfinite(got).all()
        assert err <= floor, (cid, build, ref_mode, err, floor)
    if mode == "gen":
        assert not torch.equal(outs["gen"], outs["gen1"])


# ------------------------------------------------------------------------------------------------ the whole forward, fp32 and bf16x3
@pytest.mark.parametrize("cid,mode", [cm for cm in CASE_MODES if cm[1] != "mask"], ids=lambda v: v)
def test_forward_fp32_and_bf16x3_meet_the_fp32_bound(engines, cid, mode):
    """dyf_set_sample_precision(32) and (48) on the bf16 build's engine.  bf16x3 keeps fp32 conv operands for this backbone
    (tests/test_gpu_bf16x3_sampling.py, section G): the two outputs are equal bit for bit."""
    eng = engines(cid, "bf16")
    outs = {}
    try:
        for bits in (32, 48):
            eng.set_sample_precision(bits)
            assert eng.sample_precision == bits
            outs[bits] = _forward(eng, cid, mode)
    finally:
        eng.set_sample_precision(16)
    for ref_mode in outs[32]:
        e64 = R.refs(cid, None, ref_mode)
        torch32 = rel_rms(R.exact(cid, ref_mode, torch.float32), e64)
        for bits in (32, 48):
            err = rel_rms(outs[bits][ref_mode], e64)
            print(f"[scn32] {cid} precision {bits} {ref_mode}: engine vs E64 {err:.3e} (bound {R.TOL:.0e}; fp32 torch {torch32:.3e})")
            assert err <= R.TOL, (cid, bits, ref_mode, err)
        assert torch.equal(outs[32][ref_mode], outs[48][ref_mode]), (cid, ref_mode)


def test_the_stem_channel_limit_stays_with_the_backbones_that_have_a_stem():
    """res0-64 enters block 0 with 64 channels; a U-Net with 33 channels in front of its stem is still refused when its engine is made."""
    cfg = D.UNet(dim=8, with_time_emb=True, upsample_dims=[64, 64], num_input_channels=32, num_output_channels=1,
                 num_conditional_channels=1).engine_net_config()
    with pytest.raises(NotImplementedError, match="channel counts"):
        D.HipEngine(cfg, cfg, 8, 8, max_batch=1, use_graph=False)
    c = R.CASE["res0-64"]
    assert c["n_in"] + c["n_cond"] == c["dim"] == 64


# ------------------------------------------------------------------------------------------------ one block through the conv seam
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("bc", R.BLOCK_CASES, ids=R.block_id)
def test_block_through_the_conv_seam(engines, bc, build):
    """op_conv2d_ex(path=0, act=4 = erf GELU) with per-row coefficient rows, the residual where cin == cout, an injected mask on the
    marked cases; conv_direct_kernel, by the form log."""
    eng = engines("golden-shape", build)
    b = R.block_build(bc, build)
    dev = lambda v: None if v is None else v.to(DEV).contiguous()
    eng.form_log(True)
    try:
        got = eng.op_conv2d_ex(dev(b["x"]), b["w"], 1, b["pad"], dev(b["A"]), dev(b["C"]), act=4, path=0, residual=dev(b["res"]),
                               mask=dev(b["keep"]), p=R.BLOCK_P if b["keep"] is not None else 0.0).cpu()
        forms = eng.form_log_read()
    finally:
        eng.form_log(False)
    assert {k for k in forms if k.startswith("conv_")} == {DIRECT}, forms
    ref = b["ref"]()
    excess, floor = R.excess_floor(got, ref, b["dt"])
    base, _ = R.excess_floor(R.round16(b["ref"](torch.float32), b["dt"]), ref, b["dt"])
    print(f"[scnblk] {R.block_id(bc)} {build}: excess {excess:.3e} = {excess / floor:.3f} floors (floor {floor:.3e}; fp32 torch rounded once "
          f"{base / floor:.3f} floors)")
    assert got.dtype == b["dt"] and excess <= floor, (R.block_id(bc), build, excess, floor)


# ------------------------------------------------------------------------------------------------ a non-square generator-dropout rollout
def test_fp32_nonsquare_rollout_with_generator_dropout_equals_oracle_on_host_rebuilt_masks():
    """A SimpleConvNet pair on 6 x 10, dim 8, k = 5, 3, h = 3, cold sampling + refine, forward_conditioning 'data', nb = 3, fp32 engine with
    the interpolator's dropout drawn by the engine generator; two consecutive sample() calls with the graph on.  The oracle sampler runs
    on the host-rebuilt masks of forward counters [0, n_i) and [n_i, 2 n_i), the un-paired forward order (the pattern of
    tests/test_gpu_fp32_sampling.py::test_fp32_rng_mode_rollout_equals_oracle_with_host_reproduced_masks)."""
    C, Cs, h, nb, H, W, dim, ks, p = 2, 1, 3, 3, 6, 10, 8, [5, 3], 0.1
    cfg = dict(dim=dim, kernel_sizes=ks, with_time_emb=True, dropout=p, residual=True)
    hp = dict(timesteps=h, forward_conditioning="data", interpolate_before_t1=True, schedule="before_t1_only", sampling_type="cold",
              refine_intermediate_predictions=True, enable_interpolator_dropout=True, num_input_channels=C)
    PF = oinit.seeded_state(oinit.simple_conv_net_param_shapes(dim, C + C + Cs, C, ks), seed=71, gain=R.GAIN)
    PI = oinit.seeded_state(oinit.simple_conv_net_param_shapes(dim, 2 * C + Cs, C, ks), seed=72, gain=R.GAIN)
    Fn, In = _net(dim, ks, p, C, C + Cs, C), _net(dim, ks, p, 2 * C, Cs, C)
    Fn.load_state_dict(PF, strict=True)
    In.load_state_dict(PI, strict=True)
    m = D.DYffusion(Fn, D.InterpolatorHandle(In, h), timesteps=h, forward_conditioning="data", interpolate_before_t1=True,
                    refine_intermediate_predictions=True, enable_interpolator_dropout=True, max_batch=nb, dtype="fp32", use_graph=True)
    g = torch.Generator().manual_seed(73)
    x0, c = torch.randn(nb, C, H, W, generator=g), torch.rand(nb, Cs, H, W, generator=g)
    seed = 20261021
    m.seed(seed)
    got1 = {k: v.cpu() for k, v in m.sample(x0.to(DEV), static_condition=c.to(DEV)).items()}
    got2 = {k: v.cpu() for k, v in m.sample(x0.to(DEV), static_condition=c.to(DEV)).items()}  # graph replay
    assert m._engine.dtype == "fp32" and m._engine.sample_precision == 32

    def oracle(first_forward):
        drop = S.EngineMasks(seed, first_forward=first_forward)

        def i_fn(x, t, cond):
            drop.begin_forward()
            return nets.simple_conv_net_forward(PI, cfg, x, t, cond, dropout=drop)

        with torch.no_grad():
            out = sampler.sample_loop(lambda x, t, cond: nets.simple_conv_net_forward(PF, cfg, x, t, cond), i_fn, x0, c, hp)
        return out, drop.fwd + 1

    want1, nfwd = oracle(0)
    want2, nfwd2 = oracle(nfwd)
    n_f, n_i = m._engine.forward_counts()
    assert nfwd == n_i and nfwd2 == 2 * n_i
    for tag, got, want in (("first call", got1, want1), ("graph replay", got2, want2)):
        assert sorted(got) == sorted(want)
        worst = max(rel_rms(got[k], want[k]) for k in want)
        print(f"[scnroll] fp32 6x10 generator-dropout rollout ({tag}): worst rel-rms vs the oracle on host-rebuilt masks {worst:.3e} (bound {TOL32:.0e})")
        assert worst <= TOL32
    apart = min(rel_rms(got1[k], got2[k]) for k in got1)
    print(f"[scnroll] the two calls are {apart:.3e} apart")
    assert apart > 1e-2
