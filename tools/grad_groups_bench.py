"""What gradient groups cost (``grad_groups``, ssi/grad_groups.py), on the synthetic headline geometry (Llama-3.2-1B + 5000 DSUs, bf16).
python tools/grad_groups_bench.py [--part kernel|trainer|all] [--json profiles/grad_groups.json]

kernel   on the model's flat buffers (1.246 G bf16 elements), forms timed alternately in one process, --rounds rounds of --calls calls each:
         ``ssi_sumsq`` against ``ssi_sumsq_groups`` with 1 group in 1 segment and with the five-group example on the real layout; and
         ``ssi_adamw_step_seg`` against ``ssi_adamw_step_seg_gscale`` with all-one scales on the same refined table.  Each new form is set
         against the existing kernel of the same run; the margin is that kernel's own min-to-max spread over the rounds.
trainer  step time through ``Trainer.train()`` at log_interval 1, same build, --steps steps after --warmup: no key against ``clip: null``;
         ``clip_grad_norm: 1.0`` against a per-group clip with ``max_norm: 1.0``."""
import argparse, json, os, shutil, statistics, sys, tempfile
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'speech-integration_amd')
sys.path.insert(0, PKG)
from ssi import ops
from ssi.config import compose
from ssi.grad_groups import GradGroups
from ssi.param_groups import model_layout
from ssi.train_utils import resolve_n_dsus
from ssi.trainer import Trainer

GROUPS = [{'name': 'new_rows', 'params': ['tok_embeddings.weight'], 'token_types': ['dsu', 'modality']},
          {'name': 'embedding', 'params': ['tok_embeddings.weight']}, {'name': 'norms', 'params': ['*.scale']}, {'name': 'attn', 'params': ['*.attn.*']}]
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


def trainer(steps, grad_groups=None, extra=()):
    tmp = tempfile.mkdtemp(prefix='ssi_grad_groups_')
    cfg = compose(os.path.join(PKG, 'conf'), 'sft', [
        'data=sft/mls-hubert_large_ll60k-layer_22', 'dtype=bf16', f'max_steps={steps}', 'gradient_accumulation_steps=1', 'log_interval=1',
        f'tokenizer.max_seq_len={args.seq}', f'data.train.dataset.n_samples={steps * args.batch}', 'data.dev.dataset.n_samples=8',
        f'data.train.dataloader.batch_size={args.batch}', 'eval_steps=1000000000', 'save_steps=1000000000', f'output_dir={tmp}',
        f'checkpointer.output_dir={tmp}/ckpt', f'checkpointer.checkpoint_dir={tmp}/none', 'checkpointer.allow_random_init=true', 'speech.n_dsus=5000',
        *extra])
    if grad_groups is not None:
        cfg.grad_groups = grad_groups
    resolve_n_dsus(cfg)
    t = Trainer(cfg)
    t.setup()
    return t, tmp


def stats(ts):
    return {'median_ms': round(statistics.median(ts), 4), 'min_ms': round(min(ts), 4), 'max_ms': round(max(ts), 4)}


def against(res, new, old):
    """``new`` set against ``old`` of the same run: the ratio of the medians, and whether the difference lies inside ``old``'s own spread."""
    spread = res[old]['max_ms'] - res[old]['min_ms']
    d = res[new]['median_ms'] - res[old]['median_ms']
    res[new].update(against=old, ratio=round(res[new]['median_ms'] / res[old]['median_ms'], 4), minus_ms=round(d, 4),
                    yardstick_spread_ms=round(spread, 4), within_spread=bool(d <= spread))
    print(f"{new}: {res[new]['ratio']:.4f} x {old} ({d:+.4f} ms; {old}'s spread is {spread:.4f} ms)", flush=True)


out = {}
if args.part in ('kernel', 'all'):
    t, tmp = trainer(1)
    m, opt = t.model, t.optimizer
    layout, total = model_layout(m)
    p, g, mo, v = m._flat, m._flat_grad, opt._exp_avg, opt._exp_avg_sq
    g.copy_((torch.randn(1 << 20, device='cuda') * 0.01).to(g.dtype).repeat(total // (1 << 20) + 1)[:total])
    mo.copy_(g); v.copy_(g).abs_()
    gg = GradGroups.from_config({'groups': GROUPS, 'clip': {'max_norm': 1.0}}, layout, total, t.token_type_ranges, None, device='cuda')
    one, many = torch.zeros(1, device='cuda'), torch.zeros(gg.n_groups, device='cuda')
    ws = torch.empty(1 << 20, dtype=torch.uint8, device='cuda')
    hyper = dict(beta1=0.9, beta2=0.999, eps=1e-8, step=3, grad_scale_dev=None, zero_grad=False)
    lr, wd = 1e-5, 0.01
    segs = [s for s, _ in gg.refined]
    kw = dict(seg_end=[s.end for s in segs], seg_lr=[lr] * len(segs), seg_frozen=[False] * len(segs), seg_weight_decay=[wd] * len(segs))
    ones = torch.ones(len(segs), device='cuda')
    forms = {'sumsq': lambda: ops.sumsq(g, one, workspace=ws),
             'sumsq_groups_1_group': lambda: ops.sumsq_groups(g, [total], [0], 1, one, workspace=ws),
             'sumsq_groups_example': lambda: ops.sumsq_groups(g, gg.seg_end, gg.seg_group, gg.n_groups, many, workspace=ws),
             'adamw_seg': lambda: ops.adamw_step_seg(p, g, mo, v, **kw, **hyper),
             'adamw_seg_gscale_ones': lambda: ops.adamw_step_seg(p, g, mo, v, seg_scale_dev=ones, **kw, **hyper)}
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
    res = {'elements': total, 'rounds': args.rounds, 'calls_per_round': args.calls, 'groups': gg.names, 'segments_of_the_example': len(gg.seg_end)}
    for k, ts in times.items():
        res[k] = stats(ts)
        res[k]['TB_per_s'] = round((2 if k.startswith('sumsq') else 14) * total / res[k]['median_ms'] / 1e9, 3)
        print(f"{k:24s} {res[k]['median_ms']:.4f} ms (min {res[k]['min_ms']:.4f} max {res[k]['max_ms']:.4f}) {res[k]['TB_per_s']:.2f} TB/s", flush=True)
    against(res, 'sumsq_groups_1_group', 'sumsq')
    against(res, 'sumsq_groups_example', 'sumsq')
    against(res, 'adamw_seg_gscale_ones', 'adamw_seg')
    out['kernel'] = res
    t.cleanup(); del t, m, opt, p, g, mo, v
    torch.cuda.empty_cache(); shutil.rmtree(tmp, ignore_errors=True)

if args.part in ('trainer', 'all'):
    res = {}
    steps = args.warmup + args.steps
    runs = (('no_key', None, ()), ('clip_null', {'groups': GROUPS, 'clip': None}, ()), ('clip_grad_norm_1', None, ('clip_grad_norm=1.0',)),
            ('group_clip_max_norm_1', {'groups': GROUPS, 'clip': {'max_norm': 1.0}}, ()))
    for name, node, extra in runs:
        t, tmp = trainer(steps, node, extra)
        t.train()
        torch.cuda.synchronize()
        dur = [1e3 * r['duration_step'] for r in t.wandb_logger.records[args.warmup:]]
        assert len(dur) == args.steps
        res[name] = stats(dur)
        res[name].update(ms_of_each_step=[round(d, 2) for d in dur], last_loss=t.wandb_logger.records[-1]['loss'])
        print(f"trainer {name:22s} {res[name]['median_ms']:.2f} ms per step (min {res[name]['min_ms']:.2f} max {res[name]['max_ms']:.2f})", flush=True)
        t.cleanup(); del t
        torch.cuda.empty_cache(); shutil.rmtree(tmp, ignore_errors=True)
    against(res, 'clip_null', 'no_key')
    against(res, 'group_clip_max_norm_1', 'clip_grad_norm_1')
    res['geometry'] = f'Llama-3.2-1B + 5000 DSUs, bf16, batch {args.batch} x seq {args.seq}, gradient_accumulation_steps 1, log_interval 1, {args.steps} steps after {args.warmup}'
    out['trainer'] = res

if args.json:
    with open(args.json, 'w') as f:
        json.dump(out, f, indent=1)
