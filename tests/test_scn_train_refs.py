"""tests/scn_train_refs.py -- the float64 restatement of the SimpleConvNet training step the GPU tests differentiate -- against the
imported reference's own step (tests/golden/scn_*.npz: losses, gradients and running statistics of p_losses / get_loss + backward
with every nn.Dropout drawing from DropoutSeeded(seed)), under the end-to-end tolerance of the GPU tests: losses 1e-4 relative,
every parameter's gradient within 1e-3 of the global gradient norm, running statistics rtol 1e-4 / atol 1e-6.  The second test shows
that this tolerance notices what a wrong kernel would do: one dropped conv tap, a missing residual, tanh-GELU for erf-GELU."""
import json

import pytest
import torch

from oracle.nets import DropoutSeeded
from tests import scn_train_refs as S
from tests.helpers import load_npz, split_state

FIXTURES = ["scn_plosses_train_a", "scn_plosses_train_b", "scn_interp_train_a", "scn_get_loss_a"]
LOSS_RTOL, GRAD_TOL = 1e-4, 1e-3


def _compare(name, **variant):
    z = load_npz(name + ".npz")
    hp = json.loads(str(z["hp"]))
    got, grads, stats = S.fixture_step(name, z, DropoutSeeded(hp["dropout_seed"]), **variant)
    want = json.loads(str(z["losses"]))
    loss_err = max(abs(got[k] - want[k]) / abs(want[k]) for k in want if k in got)
    worst, which, gn = S.grad_errors(grads, split_state(z, "G"))
    return z, loss_err, worst, which, gn, stats


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_matches_the_reference_step(name):
    z, loss_err, worst, which, gn, stats = _compare(name)
    print(f"{name}: loss error {loss_err:.2e}, grad norm {gn:.4f}, worst gradient error / grad norm {worst:.2e} ({which})")
    assert loss_err <= LOSS_RTOL
    assert worst <= GRAD_TOL
    B = split_state(z, "B")
    checked = 0
    for k, v in B.items():
        if k.endswith("num_batches_tracked"):
            continue
        assert torch.allclose(stats[k].float(), v, rtol=1e-4, atol=1e-6), k
        checked += 1
    assert checked == 2 * len(json.loads(str(z["hp"]))["model"]["kernel_sizes"])
    passes = 2 if name.startswith("scn_plosses") else 1
    assert all(int(v) == passes for k, v in B.items() if k.endswith("num_batches_tracked"))


@pytest.mark.parametrize("variant", [dict(drop_tap=(1, 0, 1)), dict(residual=False)], ids=["dropped-tap", "no-residual"])
def test_the_tolerance_notices_a_wrong_network(variant):
    """Measured on the four fixtures: a dropped tap of block 1 moves the worst gradient by 6e-2 .. 2.3e-1 of the gradient norm, a
    missing residual by 3.2e-1 .. 5.9e-1 (the restatement itself: 2e-7 .. 8e-7)."""
    for name in FIXTURES:
        _, loss_err, worst, which, _, _ = _compare(name, **variant)
        print(f"{name} {variant}: loss error {loss_err:.2e}, worst gradient error / grad norm {worst:.2e} ({which})")
        assert loss_err > LOSS_RTOL and worst > GRAD_TOL


def test_tanh_gelu_is_caught_by_the_single_op_bound_not_by_the_end_to_end_one():
    """tanh-GELU differs from erf-GELU by at most 4.7e-4 absolute.  Through a whole step that is 2.2e-4 .. 3.0e-4 of the gradient norm
    and 1.3e-5 .. 5.5e-5 of the loss on the four fixtures (printed): INSIDE the end-to-end tolerance, which therefore does not tell
    the two apart.  The single-op tolerance of tests/test_gpu_train_ops_scn.py (rel-RMS <= 1e-5 against float64) does: on one block,
    output moves by 1.1e-4 and its input gradient by 3.1e-4 rel-RMS.  That is the check a kernel with the wrong GELU fails."""
    from tests.helpers import rel_rms
    for name in FIXTURES:
        _, loss_err, worst, which, _, _ = _compare(name, gelu=S.gelu_tanh)
        print(f"{name} tanh-GELU end to end: loss error {loss_err:.2e}, worst gradient error / grad norm {worst:.2e} ({which})")
        assert worst > 1e-5  # visible, though inside the end-to-end tolerance
    z = load_npz("scn_plosses_train_a.npz")
    P = S.to_dtype(split_state(z, "F"), torch.float64)
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(4, 8, 10, 10, generator=g, dtype=torch.float64)
    temb = torch.randn(4, 16, generator=g, dtype=torch.float64)
    dy = torch.randn(4, 8, 10, 10, generator=g, dtype=torch.float64)
    res = {}
    for tag, fn in (("erf", S.gelu_erf), ("tanh", S.gelu_tanh)):
        x = x0.clone().requires_grad_(True)
        y = S.block(P, 1, x, temb, 7, 0.0, None, True, gelu=fn)
        (y * dy).sum().backward()
        res[tag] = (y.detach(), x.grad)
    e_y, e_dx = rel_rms(res["tanh"][0], res["erf"][0]), rel_rms(res["tanh"][1], res["erf"][1])
    print(f"one block, tanh- vs erf-GELU: output rel-RMS {e_y:.2e}, input gradient rel-RMS {e_dx:.2e}")
    assert e_y > 1e-5 and e_dx > 1e-5
