"""tests/golden/scn_*.npz ARE what the imported reference's SimpleConvNet training step produces today: where the reference checkout
is present (the build container; never the GPU box) regenerate them with tests/golden/make_scn_train_golden.py into a scratch
directory and compare every array with the committed file, bit for bit (in the manner of tests/test_optim_golden_regen.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FILES = ("scn_plosses_train_a.npz", "scn_plosses_train_b.npz", "scn_interp_train_a.npz", "scn_get_loss_a.npz")

needs_reference = pytest.mark.skipif(not os.path.isdir("/root/reference/src"),
                                     reason="the reference checkout is only present in the build container")


@needs_reference
def test_scn_training_fixtures_regenerate_bit_identically(tmp_path):
    env = dict(os.environ, DYF_GOLDEN_OUT=str(tmp_path), PYTHONHASHSEED="4242")
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_scn_train_golden.py")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert sorted(os.listdir(tmp_path)) == sorted(FILES)
    for name in FILES:
        with np.load(os.path.join(tmp_path, name), allow_pickle=False) as x, np.load(os.path.join(GOLDEN, name), allow_pickle=False) as y:
            assert sorted(x.files) == sorted(y.files), name
            for k in x.files:
                assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape, (name, k)
                if x[k].dtype.kind in "US":
                    assert json.loads(str(x[k])) == json.loads(str(y[k])), (name, k)
                else:
                    assert np.array_equal(x[k], y[k], equal_nan=True), (name, k)


def test_scn_training_fixtures_hold_what_the_tests_need():
    """Data only, far below the size limit of a committed file; weights, gradients of every parameter, running statistics, losses, seed."""
    for name in FILES:
        assert os.path.getsize(os.path.join(GOLDEN, name)) < 300_000, name
        with np.load(os.path.join(GOLDEN, name), allow_pickle=False) as z:
            hp, losses = json.loads(str(z["hp"])), json.loads(str(z["losses"]))
            assert "dropout_seed" in hp and "loss" in losses
            F = {k[3:] for k in z.files if k.startswith("F::")}
            G = {k[3:] for k in z.files if k.startswith("G::")}
            B = {k[3:] for k in z.files if k.startswith("B::")}
            params = {k for k in F if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
            assert G == params and B == F - params
            assert name.startswith("scn_plosses") == any(k.startswith("I::") for k in z.files)
            assert all(np.abs(z["G::" + k]).max() > 0 for k in params if not k.endswith("conv.bias"))
    with np.load(os.path.join(GOLDEN, "scn_get_loss_a.npz"), allow_pickle=False) as z:  # the residual is live in block 0
        w = z["F::convs.0.conv.weight"]
        assert w.shape[0] == w.shape[1]
