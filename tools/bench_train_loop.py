"""Time whole training-loop iterations (p_losses incl. the weight refresh, backward incl. the gradient export, AdamW) at BASELINE
configs[1] shapes.
usage: python tools/bench_train_loop.py [B] [cuda] [--optimizer {torch,torch-clip,engine}]
       python tools/bench_train_loop.py --config spring-mesh [B] [--trace]
  --config spring-mesh    the spring-mesh experiments instead (model/cnn_simple.yaml: SimpleConvNet dim 64, kernel_sizes [9, 7, 5, 3], 10 x 10
                          grid, B = 64 by default; experiment/spring_mesh.yaml: AdamW lr 4e-4, weight_decay 1e-4, gradient_clip_val 1.0: the
                          engine-resident optimizer for the forecaster, torch.optim.AdamW + clip_grad_norm_ on the module's
                          parameters for stage 1): whole iterations of the forecaster objective (lambda2 = 0.5) and of
                          interpolator stage 1, each in the default and in the deterministic mode, and next to each the same step in torch
                          eager on the same GPU (tests/scn_train_refs.py in fp32 on the device + torch.optim.AdamW + clip_grad_norm_): a
                          point of comparison, not a bar.  --trace: 12 iterations of the forecaster objective in the default mode and
                          nothing else (the run to put under rocprofv3 --kernel-trace --stats)
  cuda                    forecaster parameters resident on the GPU
  --optimizer torch       (default) torch.optim.AdamW(lr=1e-4) on the module, nothing else: the loop this tool has always timed, so its
                          figures compare like for like with earlier commits
  --optimizer torch-clip  the reference's recipe on the module: AdamW(weight_decay=1e-4) + clip_grad_norm_(1.0) (a host sync); no EMA
  --optimizer engine      dyffusion_amd.EngineAdamW with the same recipe plus the weight EMA: gradients, state and weights stay in the
                          engine (csrc/train_optim.hip).  Also prints the latency of a step by itself: 20 back-to-back steps between two
                          events, EACH of which includes the sum-of-squares launch, the status copy and the host's wait for the previous
                          step's outcome -- a latency, not the update kernel's bandwidth (that is read from a kernel trace: the
                          algorithmic bytes of opt_adamw_step, printed here, over its traced duration)"""
import os, statistics, sys, time, torch
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from tools._forms import forward_env_forms  # noqa: E402

forward_env_forms()  # DYF_* switches of this run -> dyf_debug_set_form
import bench
import dyffusion_amd as D
argv = sys.argv[1:]


def spring_mesh(B, trace=False):
    from oracle import init as oinit, losses
    from tests import scn_train_refs as S
    mk = dict(dim=64, kernel_sizes=[9, 7, 5, 3], with_time_emb=True, dropout=0.05)
    hp = dict(timesteps=4, schedule="before_t1_only", additional_interpolation_steps=0, additional_interpolation_steps_factor=0,
              interpolate_before_t1=True, time_encoding="dynamics", forward_conditioning="data", lambda_reconstruction=1.0,
              lambda_reconstruction2=0.5, loss_function="l1", enable_interpolator_dropout=True)
    C, Cs, h = 4, 1, hp["timesteps"]
    iters, keep = 40, 25
    PF = oinit.seeded_state(oinit.simple_conv_net_param_shapes(64, C + C + Cs, C, mk["kernel_sizes"]), seed=7, gain=0.8)
    PI = oinit.seeded_state(oinit.simple_conv_net_param_shapes(64, 2 * C + Cs, C, mk["kernel_sizes"]), seed=8, gain=0.8)
    g = torch.Generator().manual_seed(0)
    xt, cond = torch.randn(B, C, 10, 10, generator=g).cuda(), torch.randn(B, C, 10, 10, generator=g).cuda()
    sc, t = torch.rand(B, Cs, 10, 10, generator=g).cuda(), torch.randint(0, h, (B,), generator=g)
    dyn = torch.randn(B, 1 + h, C, 10, 10, generator=g).cuda()
    ti = torch.randint(1, h, (B,), generator=g)
    recipe = dict(lr=4e-4, weight_decay=1e-4)

    def mirror(P, n_in, n_cond):
        net = D.SimpleConvNet(dim=64, with_time_emb=True, kernel_sizes=mk["kernel_sizes"], dropout=mk["dropout"], num_input_channels=n_in,
                              num_output_channels=C, num_conditional_channels=n_cond, loss_function="l1")
        net.load_state_dict(P, strict=True)
        return net

    def sync():
        torch.cuda.synchronize()
        return time.perf_counter()

    def timed(step):
        nonlocal iters, keep
        ms = []
        for _ in range(iters):
            t0 = sync()
            step()
            ms.append(1e3 * (sync() - t0))
        return statistics.median(ms[-keep:]), min(ms[-keep:])

    def engine_loop(objective, det):
        if objective == "forecaster":
            m = D.DYffusion(mirror(PF, C, C + Cs), D.InterpolatorHandle(mirror(PI, 2 * C, Cs), h, 1), max_batch=B, train_deterministic=det,
                            **{k: v for k, v in hp.items()})
            m.train()
            m._ensure_engine((10, 10), B, sync=False)
            opt = D.EngineAdamW(m, max_grad_norm=1.0, **recipe)
            tg = t.cuda()
            loss = lambda: m.p_losses(xt, cond, tg, static_condition=sc)["loss"]
        else:
            net = mirror(PI, 2 * C, Cs).cuda()  # parameters on the GPU: gradients and weights move device to device
            net.train_deterministic = det
            net.train()
            net._own_engine(B, (10, 10))
            opt = torch.optim.AdamW(net.parameters(), **recipe)  # (the resident optimizer serves a DYffusion's forecaster)
            inputs, tgt, tg = torch.cat([dyn[:, 0], dyn[:, -1]], 1), dyn[torch.arange(B), ti].contiguous(), ti.float().cuda()
            loss = lambda: net.get_loss(inputs, tgt, condition=sc, time=tg)

        def step():
            opt.zero_grad()
            loss().backward()
            if objective != "forecaster":
                torch.nn.utils.clip_grad_norm_(net.parameters(), 1.0)
            opt.step()
        return timed(step)

    def eager_loop(objective):
        Pg = S.to_dtype(PF if objective == "forecaster" else PI, torch.float32, True, device="cuda")
        Pi = S.to_dtype(PI, torch.float32, device="cuda")
        ps = [v for v in Pg.values() if torch.is_tensor(v) and v.requires_grad]
        opt = torch.optim.AdamW(ps, **recipe)

        class Drop:
            def apply(self, x, p):
                return torch.nn.functional.dropout(x, p, training=True)
        drop, cfg = Drop(), dict(hp, model=mk)

        def step():
            opt.zero_grad()
            stats = {}
            f_fn = lambda x, tt, c: S.forward(Pg, mk, x, tt, c, dropout=drop, bn_training=True, new_stats=stats)
            if objective == "forecaster":
                out = losses.p_losses(f_fn, lambda x, tt, c: S.forward(Pi, mk, x, tt, c, dropout=drop), xt, cond, t, sc, cfg)["loss"]
            else:
                out = losses.interpolation_loss(f_fn, dyn, ti, sc, 1, "l1")
            out.backward()
            torch.nn.utils.clip_grad_norm_(ps, 1.0)
            opt.step()
            with torch.no_grad():
                for k, v in stats.items():
                    Pg[k].copy_(v)
        return timed(step)

    if trace:  # under rocprofv3 --kernel-trace --stats: a few iterations of the forecaster objective in the default mode, nothing else
        iters, keep = 12, 6
        med, lo = engine_loop("forecaster", False)
        print(f"spring-mesh forecaster objective, B = {B}, {iters} iterations under the tracer: {med:.2f} ms ({lo:.2f})")
        return
    print(f"spring-mesh training loop, SimpleConvNet dim 64 {mk['kernel_sizes']}, 10 x 10, B = {B}, dropout {mk['dropout']}: whole iterations "
          f"(zero_grad, loss, backward, AdamW + clip), median (min) of the last {keep} of {iters}")
    for objective in ("forecaster", "interpolator"):
        for det in (False, True):
            med, lo = engine_loop(objective, det)
            print(f"  engine  {objective:12s} {'deterministic' if det else 'default':13s}: {med:.2f} ms ({lo:.2f})")
        med, lo = eager_loop(objective)
        print(f"  eager   {objective:12s} torch fp32 on the device : {med:.2f} ms ({lo:.2f})")


if "--config" in argv:
    i = argv.index("--config")
    config = argv[i + 1]
    del argv[i:i + 2]
    if config != "spring-mesh":
        sys.exit(f"--config {config}: expected spring-mesh")
    trace = "--trace" in argv
    argv = [a for a in argv if a != "--trace"]
    spring_mesh(int(argv[0]) if argv else 64, trace)
    sys.exit(0)
which = "torch"
if "--optimizer" in argv:
    i = argv.index("--optimizer")
    which = argv[i + 1]
    del argv[i:i + 2]
if which not in ("torch", "torch-clip", "engine"):
    sys.exit(f"--optimizer {which}: expected torch, torch-clip or engine")
kw = dict(bench.DIFFUSION_KW, lambda_reconstruction=1.0, lambda_reconstruction2=0.5, loss_function="l1")
bench.DIFFUSION_KW.clear(); bench.DIFFUSION_KW.update(kw)
B = int(argv[0]) if len(argv) > 0 else 8
model, F, I = bench.build_model(B, use_graph=False)
if len(argv) > 1 and argv[1] == "cuda":
    F.cuda()
g = torch.Generator().manual_seed(0)
xt = torch.randn(B, 3, 221, 42, generator=g).cuda(); cond = torch.randn(B, 3, 221, 42, generator=g).cuda()
st = torch.rand(B, 2, 221, 42, generator=g).cuda(); t = torch.randint(0, 16, (B,), generator=g).cuda()
model.train()
if which == "engine":
    opt = D.EngineAdamW(model, lr=1e-4, weight_decay=1e-4, max_grad_norm=1.0, ema_decay=0.9999)
elif which == "torch-clip":
    opt = torch.optim.AdamW(model.model.parameters(), lr=1e-4, weight_decay=1e-4)
else:
    opt = torch.optim.AdamW(model.model.parameters(), lr=1e-4)
def sync(): torch.cuda.synchronize(); return time.perf_counter()
whole = []
for it in range(12):
    t0 = sync()
    opt.zero_grad()
    out = model.p_losses(xt, cond, t, static_condition=st)
    t1 = sync()
    out["loss"].backward()
    t2 = sync()
    if which == "torch-clip":
        torch.nn.utils.clip_grad_norm_(model.model.parameters(), 1.0)
    opt.step()
    t3 = sync()
    whole.append(1e3 * (t3 - t0))
    print(f"it {it}: p_losses (incl. weight re-upload) {1e3*(t1-t0):.0f} ms, backward (incl. gradient export) {1e3*(t2-t1):.0f} ms, optimizer {1e3*(t3-t2):.1f} ms")
print(f"optimizer={which} B={B}: whole iteration median of the last 8 = {statistics.median(whole[-8:]):.1f} ms (min {min(whole[-8:]):.1f})")
if which == "engine":
    params = dict(model.model.named_parameters())
    n = sum(p.numel() for p in params.values())
    n_conv = sum(p.numel() for k, p in params.items() if p.dim() == 4 and not k.endswith(".norm.g"))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        opt.step()
    reps = 20
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        opt.step()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    by = 36.0 * n + 4.0 * n_conv
    print(f"optimizer step by itself ({n} parameters, {n_conv} with a second layout): {1e3*ms:.1f} us per step (two launches, the status copy "
          f"and the wait for the previous step); algorithmic bytes of opt_adamw_step: {by/1e6:.2f} MB (36 B per parameter + 4 B per second-layout element)")
