"""Time whole training-loop iterations (p_losses incl. the weight refresh, backward incl. the gradient export, AdamW) at BASELINE
configs[1] shapes.
usage: python tools/bench_train_loop.py [B] [cuda] [--optimizer {torch,torch-clip,engine}]
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
