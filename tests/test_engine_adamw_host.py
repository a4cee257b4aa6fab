"""EngineAdamW without a GPU: engines are built lazily, so constructing the optimizer, validating its arguments and moving state in
torch.optim.AdamW's format need none."""
import pytest
import torch

import dyffusion_amd as D
from dyffusion_amd.optim import ema_decay_at


def _net():
    return D.UNet(dim=4, with_time_emb=True, num_input_channels=4, num_output_channels=4, num_conditional_channels=1, upsample_dims=[16, 16])


def _pair():
    F = _net()
    I = D.UNet(dim=4, with_time_emb=True, num_input_channels=8, num_output_channels=4, num_conditional_channels=1, upsample_dims=[16, 16])
    return D.DYffusion(F, D.InterpolatorHandle(I, 4), timesteps=4, interpolate_before_t1=True, schedule="before_t1_only")


@pytest.mark.parametrize("kw,err", [
    (dict(betas=(1.0, 0.999)), ValueError), (dict(betas=(0.9, -0.1)), ValueError), (dict(betas=(0.9,)), ValueError),
    (dict(lr=-1e-3), ValueError), (dict(eps=-1.0), ValueError), (dict(weight_decay=-0.1), ValueError),
    (dict(ema_decay=1.5), ValueError), (dict(ema_decay=-0.01), ValueError)])
def test_constructor_rejects_bad_hyper_parameters(kw, err):
    net = _net()
    with pytest.raises(err):
        D.EngineAdamW(net, **kw)
    assert "_engine_optim" not in net.__dict__  # a refused construction attaches nothing
    D.EngineAdamW(net, lr=1e-3)


def test_constructor_rejects_owners_it_cannot_train():
    sc = D.SimpleConvNet(dim=8, num_input_channels=4, num_output_channels=4, spatial_shape=(8, 8))
    with pytest.raises(NotImplementedError):
        D.EngineAdamW(sc)
    with pytest.raises(TypeError):
        D.EngineAdamW(torch.nn.Linear(2, 2))
    m = _pair()
    opt = D.EngineAdamW(m, lr=1e-3, ema_decay=0.999)
    assert opt._net is m.model  # the forecaster is trained, the interpolator stays frozen
    with pytest.raises(RuntimeError):
        D.EngineAdamW(m.model)  # one resident optimizer per network
    opt.detach()
    D.EngineAdamW(m.model)


def test_state_dict_layout_is_torch_adamw_s():
    net = _net()
    opt = D.EngineAdamW(net, lr=2e-3, betas=(0.8, 0.95), eps=1e-7, weight_decay=1e-4, max_grad_norm=1.0, ema_decay=0.9999)
    ref = torch.optim.AdamW(net.parameters(), lr=2e-3, betas=(0.8, 0.95), eps=1e-7, weight_decay=1e-4)
    a, b = opt.state_dict(), ref.state_dict()
    assert set(a) == set(b) == {"state", "param_groups"}
    assert a["state"] == {} and b["state"] == {}  # nothing before the first step, as torch
    assert len(a["param_groups"]) == 1 and set(a["param_groups"][0]) == set(b["param_groups"][0])
    assert a["param_groups"][0]["params"] == b["param_groups"][0]["params"] == list(range(len(list(net.parameters()))))
    for k in ("lr", "betas", "eps", "weight_decay", "amsgrad"):
        assert a["param_groups"][0][k] == b["param_groups"][0][k], k
    # after a step torch has per-parameter state: it loads into EngineAdamW (held on the host until an engine exists) and comes back alike
    g = torch.Generator().manual_seed(3)
    for p in net.parameters():
        p.grad = torch.randn(p.shape, generator=g)
    ref.step()
    ref.step()
    b = ref.state_dict()
    opt.load_state_dict(b)
    a = opt.state_dict()
    assert sorted(a["state"]) == sorted(b["state"])
    for i in b["state"]:
        assert set(a["state"][i]) == set(b["state"][i]) == {"step", "exp_avg", "exp_avg_sq"}
        assert float(a["state"][i]["step"]) == float(b["state"][i]["step"]) == 2.0
        assert torch.equal(a["state"][i]["exp_avg"], b["state"][i]["exp_avg"]) and torch.equal(a["state"][i]["exp_avg_sq"], b["state"][i]["exp_avg_sq"])
    assert opt.step_count == 2
    # and the other way round
    fresh = torch.optim.AdamW(net.parameters(), lr=1.0)
    fresh.load_state_dict(a)
    assert fresh.param_groups[0]["lr"] == 2e-3 and all(float(s["step"]) == 2.0 for s in fresh.state.values())
    with pytest.raises(ValueError):
        opt.load_state_dict({"state": {}, "param_groups": [dict(b["param_groups"][0], params=[0, 1])]})


def test_schedulers_and_ema_names():
    net = _net()
    opt = D.EngineAdamW(net, lr=1e-3, ema_decay=0.9999)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda i: 0.5)
    assert opt.param_groups[0]["lr"] == 5e-4 and sched.get_last_lr() == [5e-4]
    ema = opt.ema_state_dict()
    names = [k for k, _ in net.named_parameters()]
    assert set(ema) == {k.replace(".", "") for k in names} | {"decay", "num_updates"}
    assert ema["decay"].dtype == torch.float32 and int(ema["num_updates"]) == 0
    assert torch.equal(ema[names[0].replace(".", "")], dict(net.named_parameters())[names[0]])  # the shadow starts as the weights
    with pytest.raises(RuntimeError):
        D.EngineAdamW(_net()).ema_state_dict()
    # the warm-up: min(decay, (1 + n) / (10 + n)) in fp32
    assert ema_decay_at(0.9999, 1) == float(torch.tensor(2.0) / torch.tensor(11.0))
    assert ema_decay_at(0.5, 1000) == 0.5 and ema_decay_at(0.9999, 10 ** 6) == float(torch.tensor(0.9999))


def test_step_without_an_engine_says_what_is_missing():
    opt = D.EngineAdamW(_net())
    with pytest.raises(RuntimeError, match="training forward"):
        opt.step()


def test_step_refuses_a_communicator_of_more_than_one_rank_and_more_parameter_groups():
    class StubEngine:  # what step() looks at before it launches anything
        comm_world, device, _before_close = 2, 0, []

        def optim_create(self, *a, **k):
            pass

    net = _net()
    opt = D.EngineAdamW(net, lr=1e-3)
    opt._stale = True  # (nothing to sync: the stub holds no weights)
    opt._bind(StubEngine(), 0)
    with pytest.raises(NotImplementedError, match="2 ranks"):
        opt.step()
    with pytest.raises(NotImplementedError, match="one parameter group"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(2))]})
