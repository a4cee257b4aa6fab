"""CPU: the opt-in exact form of the 16-bit Attention probability dropout (dyf_set_attention_dropout) in the two builds of the
library, in the binding and in the Python options -- and the keep rate of the stream it draws, on the host restatement.

No GPU is needed: the libraries are only loaded and their symbols resolved, engines are stubbed."""
import math

import numpy as np
import pytest

import dyffusion_amd as D
from dyffusion_amd import _lib as L
from dyffusion_amd import dyffusion as dyffusion_module
from tests.rng_host import row_mask_nhwc


@pytest.mark.parametrize("build", ["bf16", "fp16"])
def test_both_builds_export_the_two_entry_points_without_an_abi_bump(build):
    lib = L.lib(build)
    assert lib.dyf_abi_version() == 9 and L.DYF_ABI_VERSION == 9
    for name in ("dyf_set_attention_dropout", "dyf_attention_dropout"):
        assert name in [s[0] for s in L.SYMBOLS]
        assert getattr(lib, name) is not None
    assert (L.ATTN_DROPOUT_FAST, L.ATTN_DROPOUT_EXACT) == (0, 1)
    # a null engine: the setter refuses, the getter reports -1 -- nothing touches a GPU
    assert lib.dyf_set_attention_dropout(None, 1) == L.DYF_ERR_INVALID_ARGUMENT
    assert lib.dyf_attention_dropout(None) == -1


def _pair(**kw):
    F = D.Unet(dim=8, dim_mults=(1, 2), with_time_emb=True, num_input_channels=2, num_output_channels=2)
    I = D.Unet(dim=8, dim_mults=(1, 2), with_time_emb=True, num_input_channels=4, num_output_channels=2, attn_dropout=0.1)
    return D.DYffusion(F, D.InterpolatorHandle(I, 4), timesteps=4, forward_conditioning="none", interpolate_before_t1=True, **kw)


def test_the_option_validates_its_values():
    assert L.attention_dropout_mode("fast") == 0 and L.attention_dropout_mode("exact") == 1
    for bad in ("Exact", "quad", "", None, 1, True):
        with pytest.raises(ValueError):
            L.attention_dropout_mode(bad)
    assert _pair()._engine_opts["attention_dropout"] == "fast"
    assert _pair(attention_dropout="exact")._engine_opts["attention_dropout"] == "exact"
    with pytest.raises(ValueError):
        _pair(attention_dropout="precise")
    m = _pair()
    with pytest.raises(ValueError):
        m.set_attention_dropout("slow")
    assert m._engine_opts["attention_dropout"] == "fast"  # a refused value changes nothing
    with pytest.raises(ValueError):  # before an engine (or a GPU) is asked for
        D.HipEngine(None, None, 8, 8, max_batch=1, attention_dropout="bogus")
    assert D.Unet.engine_attention_dropout == "fast"


class _StubEngine:
    created = []

    def __init__(self, fcfg, icfg, height, width, **opts):
        self.height, self.width, self.max_batch, self.opts = height, width, opts["max_batch"], dict(opts)
        self.mode = opts["attention_dropout"]
        self.closed = False
        _StubEngine.created.append(self)

    def set_attention_dropout(self, mode):
        self.mode = mode

    def seed(self, seed):
        pass

    def set_row_offset(self, row):
        pass

    def close(self):
        self.closed = True


def test_the_mode_survives_engine_re_creation(monkeypatch):
    _StubEngine.created = []
    monkeypatch.setattr(dyffusion_module, "HipEngine", _StubEngine)
    monkeypatch.setattr(D.Unet, "attach_engine", lambda self, engine, slot: None)
    m = _pair(attention_dropout="exact", max_batch=2)
    e1 = m._ensure_engine((16, 16), 2, sync=False)
    assert e1.opts["attention_dropout"] == "exact"
    e2 = m._ensure_engine((16, 16), 5, sync=False)  # batch growth
    assert e2 is not e1 and e1.closed and e2.opts["attention_dropout"] == "exact" and e2.max_batch == 5
    m.set_attention_dropout("fast")  # the live engine follows, and so does the next one
    assert e2.mode == "fast"
    e3 = m._ensure_engine((32, 16), 5, sync=False)  # new grid
    assert e3 is not e2 and e3.opts["attention_dropout"] == "fast"
    m.set_attention_dropout("exact")
    assert e3.mode == "exact" and m._ensure_engine((32, 32), 1, sync=False).opts["attention_dropout"] == "exact"
    assert len(_StubEngine.created) == 4


@pytest.mark.parametrize("p", [0.1, 0.6])
def test_the_exact_stream_keeps_at_nn_dropouts_rate(p):
    """Host restatement of the stream the exact form draws (tests/rng_host.py row_mask_nhwc on the (4, N, N) probabilities of OISST's
    225-token bottleneck, 8 rows): the kept fraction lies within four binomial standard errors of floor((1 - p) * 65536) / 65536.  At
    p = 0.1 that resolution (se = 2.4e-4) tells 1 - p = 0.9000 from the quad form's 230 / 256 = 0.8984."""
    rows, shape = 8, (4, 225, 225)
    n = rows * 4 * 225 * 225
    kept = sum(int(row_mask_nhwc(shape, p, 20261019, 0, 0, grow).sum()) for grow in range(rows))
    rate = math.floor(float(np.float32(np.float32(1.0) - np.float32(p)) * np.float32(65536.0))) / 65536.0
    se = math.sqrt(rate * (1.0 - rate) / n)
    frac = kept / n
    print(f"p={p}: kept {frac:.6f}, threshold rate {rate:.6f}, se {se:.2e}, deviation {abs(frac - rate) / se:.2f} se")
    assert abs(frac - rate) <= 4.0 * se
    if p == 0.1:  # the quad form's rate is not inside that band: the test can tell the two forms apart
        assert abs(230.0 / 256.0 - rate) > 4.0 * se
