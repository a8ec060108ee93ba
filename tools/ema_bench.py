"""What the parameter average costs (``ema_decay``, ssi_ema_update), on the synthetic headline geometry (Llama-3.2-1B + 5000 DSUs, bf16).
python tools/ema_bench.py [--part kernel|trainer|all] [--json FILE]

kernel   on the model's flat buffers (1.246 G bf16 elements): the plain AdamW step and the step followed by ``ssi_ema_update`` on the same
         stream, timed alternately in one process, --rounds rounds of --calls calls each; median, min and max of each, the difference, and
         beside it what the traffic predicts: the new pass moves 10 bytes per element (2 read, 4 + 4 read / written) where AdamW moves 14,
         so at AdamW's rate it costs 10 / 14 of that pass.
trainer  step time through ``Trainer.train()`` with ``ema_decay=0.9999`` against null, same build, --steps steps after --warmup; with AdamW
         under the backward the average rides on the same side stream, and what the step grows by against the kernel's own time says how much
         of the pass hides there."""
import argparse, json, os, shutil, statistics, sys, tempfile
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'speech-integration_amd')
sys.path.insert(0, PKG)
from ssi import ops
from ssi.config import compose
from ssi.train_utils import resolve_n_dsus
from ssi.trainer import Trainer

ap = argparse.ArgumentParser()
ap.add_argument('--part', default='all', choices=['kernel', 'trainer', 'all'])
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--calls', type=int, default=10)
ap.add_argument('--steps', type=int, default=12)
ap.add_argument('--warmup', type=int, default=4)
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--seq', type=int, default=2048)
ap.add_argument('--json', default=None)
args = ap.parse_args()


def trainer(ema_decay, steps):
    tmp = tempfile.mkdtemp(prefix='ssi_ema_')
    cfg = compose(os.path.join(PKG, 'conf'), 'sft', [
        'data=sft/mls-hubert_large_ll60k-layer_22', 'dtype=bf16', f'max_steps={steps}', 'gradient_accumulation_steps=1',
        f'tokenizer.max_seq_len={args.seq}', f'data.train.dataset.n_samples={steps * args.batch}', 'data.dev.dataset.n_samples=8',
        f'data.train.dataloader.batch_size={args.batch}', 'eval_steps=1000000000', 'save_steps=1000000000', f'output_dir={tmp}',
        f'checkpointer.output_dir={tmp}/ckpt', f'checkpointer.checkpoint_dir={tmp}/none', 'checkpointer.allow_random_init=true', 'speech.n_dsus=5000'])
    cfg.ema_decay = ema_decay
    resolve_n_dsus(cfg)
    t = Trainer(cfg)
    t.setup()
    return t, tmp


out = {}
if args.part in ('kernel', 'all'):
    t, tmp = trainer(0.9999, 1)
    m, opt = t.model, t.optimizer
    p, g, mo, v, ema = m._flat, m._flat_grad, opt._exp_avg, opt._exp_avg_sq, opt._ema
    total = p.numel()
    g.copy_((torch.randn(1 << 20, device='cuda') * 0.01).to(g.dtype).repeat(total // (1 << 20) + 1)[:total])
    mo.copy_(g); v.copy_(g).abs_()
    hyper = dict(lr=1e-5, weight_decay=0.01, beta1=0.9, beta2=0.999, eps=1e-8, step=3, grad_scale_dev=None, zero_grad=False)

    def plain():
        ops.adamw_step(p, g, mo, v, **hyper)

    def with_average():
        ops.adamw_step(p, g, mo, v, **hyper)
        ops.ema_update(ema, p, decay=0.9999)

    def average_alone():
        ops.ema_update(ema, p, decay=0.9999)

    forms = {'adamw': plain, 'adamw_then_ema': with_average, 'ema_alone': average_alone}
    for fn in forms.values():
        for _ in range(3): fn()
    times = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k, fn in forms.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(args.calls): fn()
            e.record(); torch.cuda.synchronize()
            times[k].append(s.elapsed_time(e) / args.calls)
    bytes_per_el = {'adamw': 14, 'adamw_then_ema': 24, 'ema_alone': 10}
    res = {'elements': total, 'rounds': args.rounds, 'calls_per_round': args.calls}
    for k, ts in times.items():
        ms = statistics.median(ts)
        res[k] = {'median_ms': round(ms, 4), 'min_ms': round(min(ts), 4), 'max_ms': round(max(ts), 4), 'GB_moved': round(bytes_per_el[k] * total / 1e9, 2),
                  'TB_per_s': round(bytes_per_el[k] * total / ms / 1e9, 3)}
        print(f"{k:16s} {ms:.4f} ms (min {min(ts):.4f} max {max(ts):.4f}) {res[k]['TB_per_s']:.2f} TB/s", flush=True)
    on_top = res['adamw_then_ema']['median_ms'] - res['adamw']['median_ms']
    expected = res['adamw']['median_ms'] * 10 / 14
    res['ema_on_top_ms'] = round(on_top, 4)
    res['expected_from_traffic_ms'] = round(expected, 4)
    res['on_top_over_expected'] = round(on_top / expected, 3)
    res['adamw_spread_ms'] = round(res['adamw']['max_ms'] - res['adamw']['min_ms'], 4)
    print(f"the average adds {on_top:.4f} ms to the AdamW pass; 10 / 14 of that pass would be {expected:.4f} ms ({on_top / expected:.2f} x)", flush=True)
    out['kernel'] = res
    t.cleanup(); del t, m, opt, p, g, mo, v, ema
    torch.cuda.empty_cache(); shutil.rmtree(tmp, ignore_errors=True)

if args.part in ('trainer', 'all'):
    res = {}
    steps = args.warmup + args.steps
    for name, decay in (('null', None), ('ema_0.9999', 0.9999)):
        t, tmp = trainer(decay, steps)
        t.train()
        torch.cuda.synchronize()
        dur = [r['duration_step'] for r in t.wandb_logger.records[args.warmup:]]
        assert len(dur) == args.steps
        res[name] = {'median_ms_per_step': round(1e3 * statistics.median(dur), 2), 'min_ms': round(1e3 * min(dur), 2), 'max_ms': round(1e3 * max(dur), 2),
                     'ms_of_each_step': [round(1e3 * d, 2) for d in dur], 'last_loss': t.wandb_logger.records[-1]['loss'],
                     'peak_memory_GB': round(torch.cuda.max_memory_allocated() / 1e9, 2)}
        print(f"trainer {name:10s} {res[name]['median_ms_per_step']:.2f} ms per step (min {res[name]['min_ms']:.2f} max {res[name]['max_ms']:.2f}), "
              f"peak {res[name]['peak_memory_GB']:.2f} GB", flush=True)
        t.cleanup(); del t
        torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats(); shutil.rmtree(tmp, ignore_errors=True)
    res['ema_minus_null_ms'] = round(res['ema_0.9999']['median_ms_per_step'] - res['null']['median_ms_per_step'], 2)
    res['null_spread_ms'] = round(res['null']['max_ms'] - res['null']['min_ms'], 2)
    res['same_loss'] = res['null']['last_loss'] == res['ema_0.9999']['last_loss']
    res['geometry'] = f'Llama-3.2-1B + 5000 DSUs, bf16, batch {args.batch} x seq {args.seq}, gradient_accumulation_steps 1, {args.steps} steps after {args.warmup}'
    print(f"ema_decay=0.9999 minus null: {res['ema_minus_null_ms']:+.2f} ms per step (null's own spread {res['null_spread_ms']:.2f} ms)", flush=True)
    out['trainer'] = res

if args.json:
    with open(args.json, 'w') as f:
        json.dump(out, f, indent=1)
