"""AdamW kernel alone on the model's 1.246 G parameters (bf16 p / g / m / v: 17.4 GB per call).  python tools/adamw_bench.py
--sr: the nearest-rounding kernel and the stochastic-rounding one (ssi_adamw_step_sr) timed alternately in one process, medians of
--rounds rounds of --calls calls each; --json FILE also writes the result there."""
import argparse, json, os, statistics, sys, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'speech-integration_amd'))
from ssi import ops
ap = argparse.ArgumentParser()
ap.add_argument('--sr', action='store_true')
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--calls', type=int, default=10)
ap.add_argument('--n', type=int, default=1_246_058_496)
ap.add_argument('--json', default=None)
args = ap.parse_args()
n = args.n
p, g, m, v = [(torch.randn(n, device='cuda') * 0.01).to(torch.bfloat16) for _ in range(4)]
v.abs_()
hyper = dict(lr=1e-5, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, step=3, grad_scale_dev=None, zero_grad=False)
kernels = {'nearest': lambda: ops.adamw_step(p, g, m, v, **hyper)}
if args.sr:
    kernels['stochastic'] = lambda: ops.adamw_step(p, g, m, v, **hyper, sr_seed=42_831, elem_offset=0)
for fn in kernels.values():
    for _ in range(3): fn()
times = {k: [] for k in kernels}
for _ in range(args.rounds if args.sr else 1):
    for k, fn in kernels.items():
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(args.calls): fn()
        e.record(); torch.cuda.synchronize()
        times[k].append(s.elapsed_time(e) / args.calls)
out = {'elements': n, 'bytes_per_call': 7 * 2 * n, 'rounds': len(times['nearest']), 'calls_per_round': args.calls}
for k, t in times.items():
    ms = statistics.median(t)
    out[k] = {'median_ms': round(ms, 4), 'min_ms': round(min(t), 4), 'max_ms': round(max(t), 4), 'TB_per_s': round(7 * 2 * n / ms / 1e9, 3)}
    print(f"AdamW {k:10s} {n / 1e9:.3f} G elements: {ms:.3f} ms (min {min(t):.3f} max {max(t):.3f})  {7 * 2 * n / ms / 1e9:.2f} TB/s", flush=True)
if args.sr:
    out['stochastic_over_nearest'] = round(out['stochastic']['median_ms'] / out['nearest']['median_ms'], 4)
    print(f"stochastic / nearest: {out['stochastic_over_nearest']:.4f}", flush=True)
if args.json:
    with open(args.json, 'w') as f:
        json.dump(out, f, indent=1)
