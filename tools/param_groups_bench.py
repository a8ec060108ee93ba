"""What parameter groups cost and save (``param_groups``, ssi/param_groups.py), on the synthetic headline geometry (Llama-3.2-1B + 5000 DSUs,
bf16).  python tools/param_groups_bench.py [--part kernel|trainer|all] [--json FILE]

kernel   AdamW alone on the model's flat buffers (1.246 G bf16 elements), four forms timed alternately in one process, --rounds rounds of
         --calls calls each: ``ssi_adamw_step``; ``ssi_adamw_step_seg`` with one segment; with the stage-1 table (only the new vocabulary rows
         train); with the no-decay-on-norm-scales table.  Each segmented form is set against the plain kernel of the same run; the margin is the
         plain kernel's own min-to-max spread over the rounds.
trainer  step time through ``Trainer.train()`` with the stage-1 rules against no rules, same build, --steps steps after --warmup."""
import argparse, json, os, shutil, statistics, sys, tempfile, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'speech-integration_amd')
sys.path.insert(0, PKG)
from ssi import ops
from ssi.config import compose
from ssi.param_groups import model_layout, resolve
from ssi.train_utils import resolve_n_dsus
from ssi.trainer import Trainer

STAGE1 = [{'params': ['tok_embeddings.weight'], 'token_types': ['dsu', 'modality']}, {'params': ['*'], 'frozen': True}]
NO_DECAY = [{'params': ['*.scale'], 'weight_decay': 0.0}]
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


def trainer(rules, steps):
    tmp = tempfile.mkdtemp(prefix='ssi_param_groups_')
    cfg = compose(os.path.join(PKG, 'conf'), 'sft', [
        'data=sft/mls-hubert_large_ll60k-layer_22', 'dtype=bf16', f'max_steps={steps}', 'gradient_accumulation_steps=1',
        f'tokenizer.max_seq_len={args.seq}', f'data.train.dataset.n_samples={steps * args.batch}', 'data.dev.dataset.n_samples=8',
        f'data.train.dataloader.batch_size={args.batch}', 'eval_steps=1000000000', 'save_steps=1000000000', f'output_dir={tmp}',
        f'checkpointer.output_dir={tmp}/ckpt', f'checkpointer.checkpoint_dir={tmp}/none', 'checkpointer.allow_random_init=true', 'speech.n_dsus=5000'])
    if rules is not None:
        cfg.param_groups = rules
    resolve_n_dsus(cfg)
    t = Trainer(cfg)
    t.setup()
    return t, tmp


out = {}
if args.part in ('kernel', 'all'):
    t, tmp = trainer(None, 1)
    m, opt = t.model, t.optimizer
    layout, total = model_layout(m)
    p, g, mo, v = m._flat, m._flat_grad, opt._exp_avg, opt._exp_avg_sq
    g.copy_((torch.randn(1 << 20, device='cuda') * 0.01).to(g.dtype).repeat(total // (1 << 20) + 1)[:total])
    mo.copy_(g); v.copy_(g).abs_()
    hyper = dict(beta1=0.9, beta2=0.999, eps=1e-8, step=3, grad_scale_dev=None, zero_grad=False)
    lr, wd = 1e-5, 0.01

    def seg_form(segs):
        kw = dict(seg_end=[s.end for s in segs], seg_lr=[lr * s.lr_scale for s in segs], seg_frozen=[s.frozen for s in segs],
                  seg_weight_decay=[wd if s.weight_decay is None else s.weight_decay for s in segs])
        return lambda: ops.adamw_step_seg(p, g, mo, v, **kw, **hyper)

    tables = {'stage1': resolve(STAGE1, layout, total, t.token_type_ranges), 'no_decay_on_norms': resolve(NO_DECAY, layout, total, t.token_type_ranges)}
    forms = {'plain': lambda: ops.adamw_step(p, g, mo, v, lr=lr, weight_decay=wd, **hyper),
             'seg_one_segment': seg_form(resolve([{'params': ['*']}], layout, total, None)),
             'seg_stage1': seg_form(tables['stage1']), 'seg_no_decay_on_norms': seg_form(tables['no_decay_on_norms'])}
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
    trainable = {k: sum(s.end - s.start for s in segs if not s.frozen) for k, segs in tables.items()}
    res = {'elements': total, 'rounds': args.rounds, 'calls_per_round': args.calls,
           'segments': {k: len(segs) for k, segs in tables.items()}, 'trainable_elements': trainable}
    for k, ts in times.items():
        ms = statistics.median(ts)
        n_el = trainable['stage1'] if k == 'seg_stage1' else total
        res[k] = {'median_ms': round(ms, 4), 'min_ms': round(min(ts), 4), 'max_ms': round(max(ts), 4), 'TB_per_s': round(7 * 2 * n_el / ms / 1e9, 3)}
        print(f"AdamW {k:24s} {ms:.4f} ms (min {min(ts):.4f} max {max(ts):.4f})", flush=True)
    spread = res['plain']['max_ms'] - res['plain']['min_ms']
    res['plain_spread_ms'] = round(spread, 4)
    for k in ('seg_one_segment', 'seg_no_decay_on_norms'):
        d = res[k]['median_ms'] - res['plain']['median_ms']
        res[k]['minus_plain_ms'] = round(d, 4)
        res[k]['within_plain_spread'] = bool(d <= spread)
        print(f"{k}: {d:+.4f} ms against the plain kernel, whose spread is {spread:.4f} ms", flush=True)
    out['kernel'] = res
    t.cleanup(); del t, m, opt, p, g, mo, v
    torch.cuda.empty_cache(); shutil.rmtree(tmp, ignore_errors=True)

if args.part in ('trainer', 'all'):
    res = {}
    steps = args.warmup + args.steps
    for name, rules in (('no_rules', None), ('stage1', STAGE1)):
        t, tmp = trainer(rules, steps)
        t.train()
        torch.cuda.synchronize()
        dur = [r['duration_step'] for r in t.wandb_logger.records[args.warmup:]]
        assert len(dur) == args.steps
        res[name] = {'median_ms_per_step': round(1e3 * statistics.median(dur), 2), 'min_ms': round(1e3 * min(dur), 2), 'max_ms': round(1e3 * max(dur), 2),
                     'ms_of_each_step': [round(1e3 * d, 2) for d in dur], 'last_loss': t.wandb_logger.records[-1]['loss']}
        print(f"trainer {name:9s} {res[name]['median_ms_per_step']:.2f} ms per step (min {res[name]['min_ms']:.2f} max {res[name]['max_ms']:.2f})", flush=True)
        t.cleanup(); del t
        torch.cuda.empty_cache(); shutil.rmtree(tmp, ignore_errors=True)
    res['stage1_over_no_rules'] = round(res['stage1']['median_ms_per_step'] / res['no_rules']['median_ms_per_step'], 4)
    res['geometry'] = f'Llama-3.2-1B + 5000 DSUs, bf16, batch {args.batch} x seq {args.seq}, gradient_accumulation_steps 1, {args.steps} steps after {args.warmup}'
    print(f"stage 1 / no rules: {res['stage1_over_no_rules']:.4f}", flush=True)
    out['trainer'] = res

if args.json:
    with open(args.json, 'w') as f:
        json.dump(out, f, indent=1)
