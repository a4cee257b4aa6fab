"""tests/scn_sample_refs.py -- the references, the rounding model and the bounds of the SimpleConvNet sampling tests -- checked on the CPU:
the exact reference is the oracle's network, the rounding model without rounding is the exact reference, fp32 arithmetic sits inside
half of every bound, every mutant of the model misses the bound it is aimed at by a factor of two or more, and the host-rebuilt
generator masks keep at the configured rate.  Every test prints what it measured (the figures in the docstring of scn_sample_refs)."""
import json
import math

import pytest
import torch

from oracle import nets
from tests import scn_sample_refs as R
from tests import scn_train_refs as S
from tests.helpers import load_npz, max_abs, rel_rms, split_state

IDS = [c["id"] for c in R.CASES]


def _modes(case):
    return R.modes_of(case) + (("gen1",) if case["p"] > 0 else ())


def test_exact_reference_is_the_oracle_network_on_the_golden(monkeypatch):
    """The oracle takes its sinusoidal time features in fp32 whatever it is handed; for the float64 comparison they are taken in
    float64 from the same formula (the unchanged fp32 oracle is compared too, at fp32 accuracy, and with the reference's golden)."""
    z = load_npz("net_simple_conv.npz")
    P, cfg = split_state(z, "P"), json.loads(str(z["cfg"]))
    x, t = torch.from_numpy(z["x"]), torch.from_numpy(z["t"])
    c = torch.from_numpy(z["c"]) if "c" in z else None
    P64 = S.to_dtype(P, torch.float64)
    with torch.no_grad():
        want32 = nets.simple_conv_net_forward(P, cfg, x, t, c)
        got32 = S.forward(P, cfg, x, t, c)
    e32 = rel_rms(got32, want32), rel_rms(want32, z["y_eval"])
    print("fp32: restatement vs oracle %.2e, oracle vs the reference's golden %.2e" % e32)
    assert max(e32) <= 5e-6

    def features64(tt, dim):
        half = dim // 2
        freqs = torch.exp(torch.arange(half, dtype=torch.float64) * (-math.log(10000.0) / (half - 1)))
        ang = tt.double()[:, None] * freqs[None, :]
        return torch.cat([ang.sin(), ang.cos()], dim=-1)
    monkeypatch.setattr(nets, "sinusoidal_features", features64)
    src = nets.DropoutSeeded(4242, record=True)
    d = lambda v: None if v is None else v.double()
    with torch.no_grad():
        want = nets.simple_conv_net_forward(P64, cfg, d(x), d(t), d(c))
        want_d = nets.simple_conv_net_forward(P64, cfg, d(x), d(t), d(c), dropout=src)
        got = S.forward(P64, cfg, x, t, c)
        got_d = S.forward(P64, cfg, x, t, c, dropout=S.MaskList(src.masks))
        model = R.model(P, cfg, x, t, c)
        model_d = R.model(P, cfg, x, t, c, keeps=[m.permute(0, 2, 3, 1).contiguous() for m in src.masks])
    errs = rel_rms(got, want), rel_rms(got_d, want_d), rel_rms(model, want), rel_rms(model_d, want_d)
    print("float64: E64 vs oracle eval %.2e, seeded dropout %.2e; M without rounding %.2e, %.2e" % errs)
    assert max(errs) <= 1e-12 and rel_rms(want_d, want) > 0.05


@pytest.mark.parametrize("cid", IDS)
def test_model_without_rounding_is_the_exact_reference(cid):
    """M with its rounding points off (the 16-bit ones and the fp32 storage of the coefficient tables) is E64, on every case and mode."""
    for mode in _modes(R.CASE[cid]):
        err = rel_rms(R.rounded(cid, None, mode), R.refs(cid, None, mode))
        print(f"{cid} {mode}: M without rounding vs E64 rel-RMS {err:.2e}")
        assert err <= 1e-12


@pytest.mark.parametrize("cid", IDS)
def test_fp32_arithmetic_sits_inside_half_of_every_bound(cid):
    case = R.CASE[cid]
    for mode in _modes(case):
        e = R.refs(cid, None, mode)
        f32 = rel_rms(R.exact(cid, mode, torch.float32), e)
        line = f"{cid} {mode}: fp32 torch vs E64 {f32:.2e} (bound {R.TOL:.0e})"
        assert f32 <= R.TOL / 2
        for dtname in R.DTYPES:
            _, m, floor = R.refs(cid, dtname, mode)
            m32 = rel_rms(R.rounded(cid, dtname, mode, torch.float32), m)
            line += f" | {dtname} floor {floor:.2e} M32/floor {m32 / floor:.3f}"
            assert m32 <= floor / 2, (cid, mode, dtname, m32, floor)
        print(line)


@pytest.mark.parametrize("name", list(R.MUTANTS))
def test_every_mutant_misses_the_bound_it_is_aimed_at(name):
    assert R.MUTANTS[name]
    for cid, mode, kind in R.MUTANTS[name]:
        ratio = R.mutant_ratio(name, cid, mode, kind)
        print(f"{name} on {cid} ({mode}, {kind}): {ratio:.1f} bounds")
        assert ratio >= 2.0, (name, cid, mode, kind, ratio)


def test_the_mutants_cover_every_case_and_every_edge_the_cases_are_there_for():
    aimed = {cid for pairs in R.MUTANTS.values() for cid, _, _ in pairs}
    assert set(IDS) <= aimed, sorted(set(IDS) - aimed)
    # the edges only some cases have: a mutant that cannot show elsewhere really is invisible there
    for name, cid, mode in (("hw_swapped", "golden-shape", "off"), ("no_res0", "golden-shape", "off"), ("coef_row0", "one-row-batch", "off"),
                            ("cat_order", "tiny-k15", "off"), ("film_swapped", "no-time", "off"), ("drop_scale", "tall", "mask")):
        assert R.mutant_ratio(name, cid, mode, "f32") <= 1e-3, (name, cid)  # (in units of the fp32 bound: float64 summation order at most)
    worst = max(R.mutant_ratio("residual_after_rounding", cid, "off", k) for cid in IDS for k in R.DTYPES)
    print(f"residual_after_rounding through the whole forward: at most {worst:.2f} floors -- the cancelling block case is what holds it")


@pytest.mark.parametrize("dtname", list(R.DTYPES))
@pytest.mark.parametrize("bc", R.BLOCK_CASES, ids=R.block_id)
def test_block_cases_fp32_rounded_once_sits_inside_half_the_floor(bc, dtname):
    b = R.block_build(bc, dtname)
    ref = b["ref"]()
    excess, floor = R.excess_floor(R.round16(b["ref"](torch.float32), b["dt"]), ref, b["dt"])
    print(f"block {R.block_id(bc)} {dtname}: floor {floor:.2e}, fp32 torch rounded once: excess / floor {excess / floor:.3f}")
    assert excess <= floor / 2
    assert b["A"].shape == (bc[5], bc[2]) and not torch.equal(b["A"][0], b["A"][-1])  # coefficient rows that differ per batch row
    assert (b["res"] is not None) == (bc[1] == bc[2])


@pytest.mark.parametrize("cid", [c["id"] for c in R.CASES if c["p"] > 0])
def test_host_rebuilt_generator_masks_keep_at_the_configured_rate(cid):
    case = R.CASE[cid]
    for fwd in (0, 1):
        keeps = R.gen_keeps(case, fwd)
        assert len(keeps) == len(case["ks"]) and all(k.shape == (case["nb"], case["h"], case["w"], case["dim"]) for k in keeps)
        n = sum(k.numel() for k in keeps)
        rate = sum(int(k.sum()) for k in keeps) / n
        sigma = math.sqrt(case["p"] * (1 - case["p"]) / n)
        print(f"{cid} forward {fwd}: keep rate {rate:.4f} over {n} elements, {abs(rate - (1 - case['p'])) / sigma:.2f} sigma from {1 - case['p']}")
        assert abs(rate - (1 - case["p"])) <= 4 * sigma
    a, b = R.gen_keeps(case, 0), R.gen_keeps(case, 1)
    assert all(not torch.equal(x, y) for x, y in zip(a, b))
    assert max_abs(R.refs(cid, None, "gen"), R.refs(cid, None, "gen1")) > 0
