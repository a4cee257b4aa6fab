"""Time the flash-attention core (dyf_op_attention: 4 heads x 32 dims) at the bottleneck of BASELINE configs[4]: 16 384 tokens
(128 x 128), NB rows, without and with dropout on the probabilities.  usage: python tools/bench_attention.py [NB] [tokens] [p]
--fp32: the fp32 core of fp32 sampling instead (dyf_op_attention_f32), no dropout: form 0 (keeps its probabilities, <= 4096 tokens)
against form 1 (streaming, matrix cores), interleaved in one process; medians of the per-call times (form 0's call also allocates
its scratch probabilities: the seam's hipMalloc sits between the two events).
usage: python tools/bench_attention.py --fp32 [NB] [tokens]
--fp32-train: the recorded fp32 Attention of the training step, forward + backward through the one-op seam (dyf_op_train_f32):
"attention" (keeps its probabilities: t_at_fwd + t_at_bwd_row / _col) against "attention_stream" (t_at_stream_fwd keeping the softmax statistics +
t_at_stream_bwd_dq / _dkv), interleaved in one process, medians, at N = 1024 and 4096 for NB = 1 and 4, and "attention_stream" alone at
N = 16 384, NB = 1; and the device memory the engine holds after one call of each form (hipMemGetInfo around a fresh engine: its caching
pool's high-water mark).  These are SEAM WALL TIMES: they include the seam's allocations, copies and synchronisation, so they compare the
two forms with each other and nothing else.
usage: python tools/bench_attention.py --fp32-train
--exact-dropout: the 16-bit core WITH dropout on the probabilities in the engine's two attention-dropout modes (HipEngine.set_attention_dropout):
"fast" (the quad form, default) against "exact" (nn.Dropout's rate on the fp32 path's keep bits), interleaved in one process, medians of
the per-call times (the seam synchronises: one call = one launch); the kernel each mode ran is read from the form log.
usage: python tools/bench_attention.py --exact-dropout [--fp16] [NB] [tokens] [p]"""
import os
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from tools._forms import forward_env_forms  # noqa: E402

forward_env_forms()  # DYF_* switches of this run -> dyf_debug_set_form
import dyffusion_amd as D  # noqa: E402
from dyffusion_amd.engine import net_config  # noqa: E402

fp32 = "--fp32" in sys.argv
fp32_train = "--fp32-train" in sys.argv
exact_dropout = "--exact-dropout" in sys.argv
dtype16 = "fp16" if "--fp16" in sys.argv else "bf16"  # --fp16: the fp16 build of the library (16-bit cores only)
sys.argv = [a for a in sys.argv if a not in ("--fp32", "--fp32-train", "--exact-dropout", "--fp16")]
nb = int(sys.argv[1]) if len(sys.argv) > 1 else 4
n = int(sys.argv[2]) if len(sys.argv) > 2 else 16384
cfg = net_config(in_channels=3, cond_channels=2, out_channels=3, dim=64, with_time_emb=True, upsample_dims=(64, 64), dropout=0.0)
p = float(sys.argv[3]) if len(sys.argv) > 3 else 0.1
if fp32_train:
    import statistics
    import time

    def used_mib():
        free, total = torch.cuda.mem_get_info()
        return (total - free) / 2 ** 20

    def engine(rows):
        e = D.HipEngine(cfg, cfg, 23, 11, max_batch=rows, use_graph=False)
        e.train_set_precision(32)
        return e

    print("seam wall times (allocation, copies and synchronisation of the op seam included): comparable between the two forms only")
    for tokens, rows in ((1024, 1), (1024, 4), (4096, 1), (4096, 4), (16384, 1)):
        ops = ["attention_stream"] if tokens > 4096 else ["attention", "attention_stream"]
        gq = torch.Generator().manual_seed(tokens + rows)
        q = (torch.randn(rows, 1, tokens, 384, generator=gq) * 1.5).cuda()
        dy = torch.randn(rows, 1, tokens, 128, generator=gq).cuda()
        mem = {}
        for op in ops:  # a fresh engine per form: what its pool holds after one call
            torch.cuda.synchronize()
            base = used_mib()
            e = engine(rows)
            at_rest = used_mib()
            e.op_train(op, [q], [], dy)
            mem[op] = (used_mib() - at_rest, at_rest - base)
            e.close()
        e = engine(rows)
        for op in ops * 2:
            e.op_train(op, [q], [], dy)
        times = {op: [] for op in ops}
        for _ in range(3 if tokens > 4096 else 7):
            for op in ops:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e.op_train(op, [q], [], dy)
                torch.cuda.synchronize()
                times[op].append((time.perf_counter() - t0) * 1e3)
        e.close()
        for op in ops:
            print(f"fp32 training {op:16s} NB={rows}, {tokens:5d} tokens: forward + backward median {statistics.median(times[op]):9.3f} ms "
                  f"(min {min(times[op]):.3f}, max {max(times[op]):.3f}); engine pool after one call {mem[op][0]:8.1f} MiB")
    sys.exit(0)
eng = D.HipEngine(cfg, cfg, 23, 11, max_batch=max(1, nb), use_graph=False, dtype=dtype16)
g = torch.Generator().manual_seed(0)
qkv = torch.randn(nb, n, 384, generator=g).to(eng.torch_dtype).cuda()
fl = nb * 4 * 2 * 2 * n * n * 32
if fp32:
    import statistics

    q32 = torch.randn(nb, n, 384, generator=g).cuda()
    forms = [1] if n > 4096 else [0, 1]
    for f in forms * 3:  # warm-up: clocks up, both kernels loaded
        y = eng.op_attention_f32(q32, form=f)
    times = {f: [] for f in forms}
    for _ in range(5 if n > 4096 else 15):  # interleaved: both forms see the same clocks (the seam synchronises: one call = one launch)
        for f in forms:
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            y = eng.op_attention_f32(q32, form=f)
            ev1.record()
            torch.cuda.synchronize()
            times[f].append(ev0.elapsed_time(ev1))
    for f in forms:
        ms = statistics.median(times[f])
        print(f"fp32 attention core form {f} ({'streaming' if f else 'keeps P'}) NB={nb}, {n} tokens: median {ms:.3f} ms (min {min(times[f]):.3f}, "
              f"max {max(times[f]):.3f}), {fl / ms / 1e9:.1f} TFLOP/s = {fl / ms / 1e9 / 157:.3f} of the 157 TF fp32 matrix peak")
    sys.exit(0)
if exact_dropout:
    import statistics

    modes = ["fast", "exact"]
    kernel = {}
    for mode in modes * 5:  # warm-up: clocks up, both kernels loaded
        eng.set_attention_dropout(mode)
        eng.form_log(True)
        y = eng.op_attention(qkv, p)
        kernel[mode] = ", ".join(sorted(eng.form_log_read()))
    eng.form_log(False)
    times = {mode: [] for mode in modes}
    for _ in range(15 if n > 4096 else 50):  # interleaved: both modes see the same clocks
        for mode in modes:
            eng.set_attention_dropout(mode)
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            y = eng.op_attention(qkv, p)
            ev1.record()
            torch.cuda.synchronize()
            times[mode].append(ev0.elapsed_time(ev1))
    med = {mode: statistics.median(times[mode]) for mode in modes}
    for mode in modes:
        print(f"attention core NB={nb}, {n} tokens, dropout p={p}, {eng.dtype}, {mode:5s} ({kernel[mode]}): median {med[mode] * 1e3:.1f} us "
              f"(min {min(times[mode]) * 1e3:.1f}, max {max(times[mode]) * 1e3:.1f}), {fl / med[mode] / 1e9:.1f} TFLOP/s")
    print(f"exact / fast = {med['exact'] / med['fast']:.3f}")
    sys.exit(0)
for pd in (0.0, p):
    for _ in range(10):  # the device idles in a low-power state: ten launches before the timed ones (measured: one warm-up launch
        y = eng.op_attention(qkv, pd)  # and ten timed ones read 0.84 ms where the steady state is 0.76 ms)
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 50
    ev0.record()
    for _ in range(reps):
        y = eng.op_attention(qkv, pd)
    ev1.record()
    torch.cuda.synchronize()
    ms = ev0.elapsed_time(ev1) / reps
    print(f"attention core NB={nb}, {n} tokens, 4 heads x 32, dropout p={pd}: {ms:.3f} ms, {fl / ms / 1e9:.1f} TFLOP/s = "
          f"{fl / ms / 1e9 / 2500:.3f} of the dense MFMA peak, finite={bool(torch.isfinite(y.float()).all())}")
