"""tests/golden/optim_adamw_ema.npz and optim_adamw_ema_moments.npz ARE what torch.optim.AdamW + clip_grad_norm_ + the reference's
LitEma produce today: where the reference checkout is present (the build container; never the GPU box) regenerate both with
tests/golden/make_optim_golden.py into a scratch directory and compare every array with the committed file, bit for bit (in the
manner of tests/test_golden_regen.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FILES = ("optim_adamw_ema.npz", "optim_adamw_ema_moments.npz")

needs_reference = pytest.mark.skipif(not os.path.isdir("/root/reference/src"),
                                     reason="the reference checkout is only present in the build container")


@needs_reference
def test_optimizer_fixtures_regenerate_bit_identically(tmp_path):
    env = dict(os.environ, DYF_GOLDEN_OUT=str(tmp_path), PYTHONHASHSEED="4242")
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_optim_golden.py")], env=env, capture_output=True, text=True, timeout=600)
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


def test_optimizer_fixtures_hold_what_the_gpu_tests_need():
    """Data only, both below the size limit of a committed file; both clip branches occur; every tensor has a deviation to compare with."""
    for name in FILES:
        assert os.path.getsize(os.path.join(GOLDEN, name)) < 1_000_000, name
    with np.load(os.path.join(GOLDEN, FILES[0]), allow_pickle=False) as z, np.load(os.path.join(GOLDEN, FILES[1]), allow_pickle=False) as mo:
        hp = json.loads(str(z["hp"]))
        assert len(hp["seeds"]) == len(hp["lrs"]) == 5 and hp["lrs"][1] != hp["lrs"][2]
        for tag in ("simple", "resnet"):
            names = json.loads(str(z[f"{tag}::names"]))
            norms = z[f"{tag}::norms"]
            assert all(n > hp["max_norm"] for n in norms[:3]) and all(n < hp["max_norm"] for n in norms[3:])
            for fam in ("w", "exp_avg", "exp_avg_sq", "ema"):
                dev = z[f"{tag}::dev_{fam}"]
                assert dev.shape == (len(names),) and np.all(dev > 0)
            for k in names:
                shape = z[f"{tag}::w::{k}"].shape
                assert z[f"{tag}::ema::{k.replace('.', '')}"].shape == shape
                assert mo[f"{tag}::exp_avg::{k}"].shape == shape and mo[f"{tag}::exp_avg_sq::{k}"].shape == shape
