"""-m gpu: the sampling mode `dtype="bf16x3"` (dyf_set_sample_precision(48)): the fp32 sampling forward with (hi, lo) bf16 operands --
a_lo b_hi + a_hi b_lo + a_hi b_hi on the bf16 matrix cores -- in the convs the 16-bit training dispatch takes.

Bounds, both the project's own: one conv against float64 rel-RMS <= 1e-5 per tensor (tests/train_op_refs.TOL, the fp32-kernel bound; the
three-term arithmetic sits at 4.5e-6, a dropped term at 1.6e-3), a rollout <= 1e-4 per field against the fp32 oracle (TOL32 of
tests/test_gpu_fp32_sampling.py; tests/test_bf16x3_sampling_host.py shows the three-term model 6x inside and a dropped term 40x outside).
Every test prints its worst value.

The 3 x 3 halo layers of a sampling forward take the fused one-launch form `t_halo3x3_16x3f:forward` (csrc/train_halo16.hip);
DYF_SAMPLE_HALO_FUSED=0 sends them to the two-launch PASS form of the training step, the second implementation these tests hold it against.
"""
import gc
import json

import pytest
import torch

import dyffusion_amd as D
from oracle import nets
from tests import bf16x3_sampling_refs as B
from tests import train_op_refs as T
from tests.gpu_common import DEV, build_dyffusion, nhwc_masks, oracle_rollout
from tests.helpers import load_npz, rel_rms, split_state
from tests.test_gpu_fp32_sampling import RESNET_GOLDENS
from tests.test_gpu_sampler import NAMES

pytestmark = pytest.mark.gpu
TOL32 = B.TOL32
FUSED, PASS = "t_halo3x3_16x3f:forward", "t_halo3x3_16x3:forward"

# ------------------------------------------------------------------------------------------------ A. one conv through the op seam
# (k, stride, pad, cin, cout, ws, bias, h, w, nb, var0)
HALO = [
    ("3x3-64to64-64x96-nb4", (3, 1, 1, 64, 64, 0, 1, 64, 96, 4, 0)),     # 192 tiles: the smallest plane the halo launcher takes
    ("3x3-64to64-61x93-nb4", (3, 1, 1, 64, 64, 0, 1, 61, 93, 4, 0)),     # the same tile count, ragged edges on both axes
    ("3x3-64to128-64x48-nb4", (3, 1, 1, 64, 128, 0, 1, 64, 48, 4, 0)),   # two column blocks
    ("3x3-128to64-64x96-nb4", (3, 1, 1, 128, 64, 0, 1, 64, 96, 4, 0)),   # two channel chunks: the halo hand-over between chunks
    # 1 152 tiles x 1 column block / 512 workgroups: a workgroup walks two tiles (thalo_conv3x3: per = tiles * nblocks / 512)
    ("3x3-64to64-128x192-nb6", (3, 1, 1, 64, 64, 0, 1, 128, 192, 6, 0)),
]
BELOW = [
    ("3x3-64to64-32x32-nb4", (3, 1, 1, 64, 64, 0, 1, 32, 32, 4, 0)),     # split-K t_gemm_mfma16x3<forward>
    ("1x1-128to64-11x13-nb3", (1, 1, 0, 128, 64, 0, 1, 11, 13, 3, 0)),
    ("4x4s2-64to64-12x16-nb4", (4, 2, 1, 64, 64, 0, 1, 12, 16, 4, 0)),
]
OUTSIDE = ("3x3-24to40-ws-11x13-nb3", (3, 1, 1, 24, 40, 1, 1, 11, 13, 3, 0))


@pytest.fixture(scope="module")
def eng():
    cfg = D.net_config(in_channels=3, cond_channels=0, out_channels=3, dim=64, upsample_dims=[64, 64])
    e = D.HipEngine(cfg, cfg, 16, 16, max_batch=4, use_graph=False)
    e.set_sample_precision(48)
    assert e.sample_precision == 48
    yield e
    e.form_log(False)
    e.close()


_REFS = {}


def reference(args):
    """(case, float64 output) of a conv case: computed once, shared, never modified."""
    if args not in _REFS:
        case = T.build("conv", args)
        with torch.no_grad():
            y = case.fn([t.double() for t in case.ins], [t.double() for t in case.params])
        _REFS[args] = (case, y)
    return _REFS[args]


def run(eng, args, sample=True):
    """One op_train call of the case -> (y on the CPU, form log of the call)."""
    case, _ = reference(args)
    eng.form_log(True)  # clears
    r = eng.op_train(case.op, [t.to(DEV) for t in case.ins], case.params, case.dout.to(DEV), None, sample=sample, **case.kw)
    forms = sorted(eng.form_log_read())
    if sample:
        assert r["dinputs"] is None and r["dparams"] is None
    return r["y"].cpu(), forms


def held(eng, args, cid, **kw):
    y, forms = run(eng, args, **kw)
    _, want = reference(args)
    assert bool(torch.isfinite(y).all()), cid
    err = rel_rms(y.reshape(want.shape), want)
    print(f"bf16x3 sampling conv {cid}: rel-RMS {err:.3e} vs float64; forms {forms}")
    assert err <= T.TOL, (cid, err)
    assert not any(k.startswith("t_gemm_mfma<") for k in forms), forms
    return y, forms


@pytest.mark.parametrize("args", [pytest.param(a, id=cid) for cid, a in HALO])
def test_a_halo_convs_take_the_fused_form_and_hold_the_fp32_bound(eng, args, request, form_switch):
    cid = request.node.callspec.id
    y, forms = held(eng, args, cid)
    assert FUSED in forms and PASS not in forms, forms
    # again right after NaN-filled tensors of the output's size were freed: torch.empty hands those blocks to the next y
    junk = [torch.full(y.shape, float("nan"), device=DEV) for _ in range(2)]
    torch.cuda.synchronize()
    del junk
    again, _ = held(eng, args, cid + " (dirty buffers)")
    assert torch.equal(y, again)
    # the PASS form: the same bound, and the two implementations agree
    form_switch.setenv("DYF_SAMPLE_HALO_FUSED", "0")
    y_pass, forms = held(eng, args, cid + " (DYF_SAMPLE_HALO_FUSED=0)")
    assert PASS in forms and FUSED not in forms, forms
    junk = [torch.full(y.shape, float("nan"), device=DEV) for _ in range(2)]
    torch.cuda.synchronize()
    del junk
    again, _ = held(eng, args, cid + " (DYF_SAMPLE_HALO_FUSED=0, dirty buffers)")
    assert torch.equal(y_pass, again)
    diff = rel_rms(y, y_pass)
    print(f"bf16x3 sampling conv {cid}: fused vs PASS rel-RMS {diff:.3e}")
    assert diff <= 1e-5


@pytest.mark.parametrize("args", [pytest.param(a, id=cid) for cid, a in BELOW])
def test_a_forms_below_the_halo_threshold(eng, args, request):
    _, forms = held(eng, args, request.node.callspec.id)
    assert "t_gemm_mfma16x3<forward>" in forms and FUSED not in forms and PASS not in forms, forms


def test_a_conv_outside_the_channel_rules_is_the_op_under_32_bit_for_bit(eng):
    cid, args = OUTSIDE
    y48, forms = held(eng, args, cid)
    assert not any("16x3" in k for k in forms), forms
    eng.set_sample_precision(32)
    try:
        y32, _ = run(eng, args)
    finally:
        eng.set_sample_precision(48)
    assert torch.equal(y48, y32)


def test_a_training_keeps_the_pass_form_and_sample_reads_the_sampling_precision(eng):
    cid, args = HALO[0]
    eng.train_set_precision("bf16x3")
    try:
        _, forms = run(eng, args, sample=False)  # the recorded op and its adjoint under train_precision="bf16x3"
        assert PASS in forms and "t_halo3x3_16x3:dgrad" in forms and FUSED not in forms, forms
        eng.set_sample_precision(32)  # sample=True reads dyf_sample_precision, not the training setting
        _, forms = run(eng, args)
        assert not any("16x3" in k for k in forms), forms  # (the fp32 matrix-core forward notes no form of its own)
    finally:
        eng.set_sample_precision(48)
        eng.train_set_precision(None)  # not set, as the fixture left it
    # only the conv honours the flag: every other op refuses it
    import ctypes as C
    from dyffusion_amd import _lib as L
    x = torch.zeros(1, 4, 4, 8, device=DEV)
    y = torch.empty_like(x)
    desc = L.TrainOp(L.TRAIN_OPS["gelu"], 1, 4, 4, 8, 0, 0, 0, 0, 0, L.TOP_SAMPLE, 0.0)
    ins, none = (C.c_void_p * 1)(x.data_ptr()), (C.c_void_p * 1)(None)
    st = eng._lib.dyf_op_train_f32(eng._h, C.byref(desc), ins, none, x.data_ptr(), y.data_ptr(), none, none, eng._stream())
    assert st == L.DYF_ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError):
        eng.op_train("gelu", [x], (), x, sample=True)


# ------------------------------------------------------------------------------------------------ B. rollout, unet_simple
def _inputs():
    PF, PI, x0, c = B.simple_inputs()
    return PF, PI, x0.to(DEV), c.to(DEV)


def _clone(d):
    return {k: v.clone() for k, v in d.items()}


def test_b_rollout_on_a_128_grid_meets_the_fp32_line_graph_equals_eager():
    PF, PI, x0, c = _inputs()
    a = build_dyffusion(PF, PI, B.MK128, 3, 2, B.HP4, max_batch=3, use_graph=True, dtype="bf16x3")
    b = build_dyffusion(PF, PI, B.MK128, 3, 2, B.HP4, max_batch=3, use_graph=False, dtype="48")
    ya1, ya2 = _clone(a.sample(x0, static_condition=c)), _clone(a.sample(x0, static_condition=c))
    yb = _clone(b.sample(x0, static_condition=c))
    assert a._engine.dtype == "bf16x3" and a._engine.sample_precision == 48 and a._engine.forward_counts() == (4, 8)
    for k in yb:
        assert torch.equal(ya1[k], yb[k]) and torch.equal(ya2[k], yb[k]), k
    b._engine.form_log(True)
    b.sample(x0, static_condition=c)
    forms = sorted(b._engine.form_log_read())
    b._engine.form_log(False)
    assert FUSED in forms and "t_gemm_mfma16x3<forward>" in forms, forms
    want = B.simple_rollout(B.MK128)
    worst = B.worst({k: v.cpu() for k, v in ya1.items()}, want)
    f = build_dyffusion(PF, PI, B.MK128, 3, 2, B.HP4, max_batch=3, use_graph=False, dtype="fp32")
    y32 = f.sample(x0, static_condition=c)
    vs32 = max(rel_rms(ya1[k].cpu(), y32[k].cpu()) for k in y32)
    print(f"bf16x3 dim64 128x128 h=4 rollout: worst rel-RMS {worst:.3e} vs the fp32 oracle, {vs32:.3e} vs the fp32 engine")
    assert worst <= TOL32 and vs32 <= TOL32
    assert not any(torch.equal(ya1[k], y32[k]) for k in y32)


# ------------------------------------------------------------------------------------------------ C. the reference's goldens
@pytest.mark.parametrize("name", NAMES)
def test_c_rollout_matches_reference_golden(name):
    """tests/test_gpu_fp32_sampling.py::test_fp32_rollout_matches_reference_golden through a bf16x3 engine."""
    z = load_npz(name + ".npz")
    hp = json.loads(str(z["hp"]))
    PF, PI = split_state(z, "F"), split_state(z, "I")
    N, Bn = hp["num_predictions"], hp["B"]
    x0 = torch.from_numpy(z["x0"]).repeat(N, 1, 1, 1)
    c = torch.from_numpy(z["c"]).repeat(N, 1, 1, 1)
    m = build_dyffusion(PF, PI, hp["model"], 4, 1, hp, max_batch=N * Bn, dtype="bf16x3")
    masks = noise = None
    if hp.get("enable_interpolator_dropout"):
        src = nets.DropoutSeeded(hp["dropout_seed"], record=True)
        oracle_rollout(PF, PI, hp["model"], hp, x0, c, drop=src)
        masks = nhwc_masks(src.masks)
    if hp["forward_conditioning"] == "data+noise":
        gen = torch.Generator().manual_seed(hp["noise_seed"])
        draws = []

        def nf(t):
            draws.append(torch.randn(t.shape, generator=gen))
            return draws[-1]

        oracle_rollout(PF, PI, hp["model"], hp, x0, c, noise_fn=nf)
        noise = torch.stack(draws, 0).to(DEV)
    _, got, _ = m.sample_loop(x0.to(DEV), static_condition=c.to(DEV), _masks=masks, _noise=noise)
    assert m._engine.dtype == "bf16x3" and m._engine.sample_precision == 48
    want = {k[len("out::"):]: v for k, v in z.items() if k.startswith("out::")}
    assert sorted(got) == sorted(want)
    worst = max(rel_rms(got[k].cpu().reshape(w.shape), w) for k, w in want.items())
    print(name, "bf16x3 worst rel-rms", worst)
    assert worst <= TOL32


@pytest.mark.parametrize("name", RESNET_GOLDENS)
def test_c_small_resnet_unets_match_reference_goldens(name):
    from tests.test_gpu_unet_resnet import engine_masks, mirror
    z = load_npz(name + ".npz")
    P, cfg = split_state(z, "P"), json.loads(str(z["cfg"]))
    x, t = torch.from_numpy(z["x"]), torch.from_numpy(z["t"])
    c = torch.from_numpy(z["c"]) if "c" in z else None
    net = mirror(P, cfg, x.shape[1], 0 if c is None else c.shape[1], z["y_eval"].shape[1], "bf16x3")
    y = net(x.to(DEV), time=t.to(DEV), condition=None if c is None else c.to(DEV)).cpu()
    assert net._engine.dtype == "bf16x3" and net._engine.sample_precision == 48
    e_eval = rel_rms(y, z["y_eval"])
    src = nets.DropoutSeeded(int(z["dropout_seed"]), record=True)
    with torch.no_grad():
        nets.resnet_unet_forward(P, cfg, x, t, c, dropout=src)
    y = net._engine.net_forward(0, x.to(DEV), t.to(DEV), None if c is None else c.to(DEV), dropout_mode=2,
                                masks=engine_masks(src.masks, len(cfg["dim_mults"]))).cpu()
    e_drop = rel_rms(y, z["y_drop"])
    print(name, f"bf16x3 eval rel-rms {e_eval:.3e}, injected-mask dropout rel-rms {e_drop:.3e}")
    assert max(e_eval, e_drop) <= TOL32


# ------------------------------------------------------------------------------------------------ D. unet.Unet
def test_d_resnet_unet_forward_on_the_split_forms():
    from tests.test_gpu_unet_resnet import mirror
    P, x, t = B.resnet_inputs()
    net = mirror(P, B.RESNET_CFG, 2, 0, 1, "bf16x3")
    net(x.to(DEV), time=t.to(DEV))  # creates the engine
    net._engine.form_log(True)
    y = net(x.to(DEV), time=t.to(DEV)).cpu()
    forms = sorted(net._engine.form_log_read())
    net._engine.form_log(False)
    err = rel_rms(y, B.resnet_forward())
    print(f"bf16x3 unet.Unet dim 64 (1, 2), 4 x 64 x 96: rel-RMS {err:.3e} vs the fp32 oracle; forms {[k for k in forms if '16x3' in k]}")
    assert net._engine.sample_precision == 48 and err <= TOL32
    assert any("16x3" in k for k in forms), forms


# ------------------------------------------------------------------------------------------------ E. switching
def test_e_switching_the_precision_of_one_engine():
    """16 -> 48 -> 32 -> 48 -> 16 on one engine with graphs: no graph of another precision is ever replayed."""
    PF, PI, x0, c = _inputs()

    def used():
        free, total = torch.cuda.mem_get_info()
        return (total - free) / 2 ** 20

    def fresh(dtype):
        m = build_dyffusion(PF, PI, B.MK64, 3, 2, B.HP4, max_batch=3, use_graph=True, dtype=dtype)
        y = _clone(m.sample(x0, static_condition=c))
        m._engine.close()
        return y

    want48, want32 = fresh("bf16x3"), fresh("fp32")
    marks = []
    for _ in range(3):
        m = build_dyffusion(PF, PI, B.MK64, 3, 2, B.HP4, max_batch=3, use_graph=True)
        y16 = _clone(m.sample(x0, static_condition=c))
        eng = m._engine
        assert eng.sample_precision == 16 and eng.dtype == "bf16"
        got = {}
        for bits in (48, 32, 48):
            eng.set_sample_precision(bits)
            assert eng.sample_precision == bits
            got.setdefault(bits, []).append(_clone(m.sample(x0, static_condition=c)))
        with pytest.raises(ValueError):
            eng.set_sample_precision(24)
        assert eng.sample_precision == 48
        eng.set_sample_precision(16)
        y16b = m.sample(x0, static_condition=c)
        for k in y16:
            assert torch.equal(y16[k], y16b[k]), k
            assert torch.equal(got[48][0][k], want48[k]) and torch.equal(got[48][1][k], want48[k]), k
            assert torch.equal(got[32][0][k], want32[k]), k
            assert not torch.equal(want48[k], want32[k]) and not torch.equal(y16[k], want48[k]), k
        eng.close()
        del m, eng, y16b, got
        gc.collect()
        torch.cuda.synchronize()
        marks.append(used())
    print("MiB in use after each close:", [round(v) for v in marks])
    assert marks[-1] - marks[1] <= 32.0


# ------------------------------------------------------------------------------------------------ F. streams
def test_f_same_seed_draws_the_same_masks_as_fp32_and_row_groups_do_not_split(form_switch):
    """Interpolator dropout from the engine generator: a wrong keep bit anywhere moves a field by > 5e-2.  With row groups configured
    (two groups of two rows here) a 48 engine runs the call as ONE group, like a 32 engine: a split call would run the groups' 16-bit
    forwards, 1e-2 away."""
    hp = dict(B.HP4, enable_interpolator_dropout=True)
    PF, PI = B.simple_inputs()[:2]
    g = torch.Generator().manual_seed(22)
    nb = 4
    x0, c = torch.randn(nb, 3, 23, 11, generator=g).to(DEV), torch.rand(nb, 2, 23, 11, generator=g).to(DEV)

    def run_(dtype, **kw):
        m = build_dyffusion(PF, PI, B.MK64, 3, 2, hp, max_batch=nb, dtype=dtype, **kw)
        m.seed(42)
        m.set_row_offset(3)
        y = _clone(m.sample(x0, static_condition=c))
        return y, m._engine

    y32, _ = run_("fp32")
    y48, _ = run_("bf16x3")
    worst = max(rel_rms(y48[k].cpu(), y32[k].cpu()) for k in y32)
    print(f"bf16x3 vs fp32, same seed and row offset, engine-generator dropout: worst rel-RMS {worst:.3e}")
    assert worst <= TOL32
    y48g, eng = run_("bf16x3", row_groups=3)
    assert eng.row_groups == 1 and all(torch.equal(y48g[k], y48[k]) for k in y48)  # 4 rows: below the 16 rows a group needs
    form_switch.setenv("DYF_GROUP_MIN_ROWS", "2")  # read when an engine is created: 4 rows are enough for two groups
    y48g, eng = run_("bf16x3", row_groups=3)
    assert eng.row_groups == 2  # configured (dyf_set_row_groups clamps to max_batch / min rows) ...
    for k in y48:               # ... and not used: the ungrouped call, bit for bit
        assert torch.equal(y48g[k], y48[k]), k


# ------------------------------------------------------------------------------------------------ G. SimpleConvNet
def test_g_simple_conv_net_keeps_fp32_conv_operands():
    z = load_npz("net_simple_conv.npz")
    P, cfg = split_state(z, "P"), json.loads(str(z["cfg"]))
    x, t = torch.from_numpy(z["x"]), torch.from_numpy(z["t"])
    c = torch.from_numpy(z["c"]) if "c" in z else None
    ys = {}
    for dtype in ("bf16x3", "fp32"):
        net = D.SimpleConvNet(dim=cfg["dim"], with_time_emb=cfg.get("with_time_emb", True), kernel_sizes=cfg["kernel_sizes"],
                              dropout=cfg.get("dropout", 0.0), num_input_channels=x.shape[1], num_output_channels=z["y_eval"].shape[1],
                              num_conditional_channels=0 if c is None else c.shape[1])
        net.engine_dtype = dtype
        net.load_state_dict(P, strict=True)
        ys[dtype] = net(x.to(DEV), time=t.to(DEV), condition=None if c is None else c.to(DEV)).cpu()
        assert net._engine.dtype == dtype and net._engine.sample_precision == (48 if dtype == "bf16x3" else 32)
    err = rel_rms(ys["bf16x3"], z["y_eval"])
    print(f"bf16x3 simple_conv eval rel-rms {err:.3e}")
    assert torch.equal(ys["bf16x3"], ys["fp32"]) and err <= TOL32
