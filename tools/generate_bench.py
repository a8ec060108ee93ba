"""What greedy generation costs at the 1B shape (Llama-3.2-1B + 5000 DSUs, bf16, random weights): 256 prompts of about 1000 tokens, 256 new
tokens each.  python tools/generate_bench.py [--part all|run|steps|recompute|constrained|beam|sample|penalty|small_batch|split_kv|kv_fp8|weight_fp8|continuous] [--json profiles/generate.json]

run        prefill time, milliseconds per decode step (event time over all steps, host gaps included), generated tokens per second, and a
           self-check: the first generated token of every prompt against the argmax of a plain full forward of that prompt alone (with
           random weights the logits are nearly flat, so a token that differs must at least be a near-tie within the two runs' own difference).
steps      decode steps only, on a cache filled with random numbers at the same lengths: the part that runs under
           ``rocprofv3 --kernel-trace --stats`` in a run of its own, so that a step's kernel time splits into attention (kv_decode_kernel),
           the cache write (kv_store_kernel) and the rest.  Kernels launched fewer times than there are steps are set-up, not step.
recompute  for context, the only thing the code could do before: re-running the full forward for every new token (8 prompts, 4 tokens).
constrained  (not part of ``all``; python tools/generate_bench.py --part constrained --json profiles/generate_constrained.json) what constrained
           decoding costs, ONE process alternating the forms over ``--rounds`` rounds, median and min..max of the rounds: ``ssi_decode_select``
           alone on [prompts, vocab_pad] bf16 logits against a torch restatement (masked_fill + argmax + log_softmax gather), on one buffer (what
           the caches hold) and rotating over buffers larger than the caches together; and a decode step whose token comes from the kernel
           (``--allowed-types``, ``--min-new-tokens``) against the unconstrained step (argmax + the forward-only cross-entropy for the
           log-probability) and the step without log-probabilities, on a cache filled with random numbers at the same lengths.
beam       (not part of ``all``; python tools/generate_bench.py --part beam --json profiles/generate_beam.json) what beam search costs, ONE process
           alternating the forms over ``--rounds`` rounds, median and min..max: ``ssi_topk_logprob`` alone (k = ``--beam-width``, the stop tokens
           masked) against ``ssi_decode_select`` and a torch restatement; ``ssi_attn_decode_beam`` alone (``--prompts / --beam-width`` prompts x
           ``--beam-width`` beams, a random ancestry, rotating over the layers' caches) against ``ssi_attn_decode`` on the materialised cache,
           with their outputs compared bit for bit; a beam decode step (``decode_step_beam`` + ``ssi_topk_logprob``) against the greedy step
           (``decode_step`` + argmax) at the same rows and key counts; and one ``beam_search`` call end to end.
penalty    (not part of ``all``; python tools/generate_bench.py --part penalty --json profiles/generate_penalty.json) what the repetition, frequency
           and presence penalties cost inside the two selection kernels, ONE process: every penalised kernel against its plain kernel on the
           same logits, the plain sampler on fp32 logits beside it, a torch restatement, and a penalised decode step against the plain one.
sample     (not part of ``all``; python tools/generate_bench.py --part sample --json profiles/generate_sample.json) what sampling costs, ONE process
           alternating the forms over ``--rounds`` rounds, median and min..max: ``ssi_decode_sample`` alone on [prompts, vocab_pad] bf16 logits in
           three settings (temperature only; top_k = 50; top_p = 0.9) against ``ssi_decode_select`` and a torch restatement (sort, cumsum, a
           Gumbel argmax), with the walks of the row each setting makes and what reading the row once costs; a sampled decode step
           (``decode_step`` + ``ssi_decode_sample`` at top_k 50, top_p 0.9) against the greedy step with log-probabilities; and one ``sample``
           call with ``n = 4``.
small_batch (not part of ``all``; python tools/generate_bench.py --part small_batch --json profiles/generate_small_batch.json) what a decode step of
           1, 8, 16, 32 and 64 rows costs, ONE process alternating the forms over ``--rounds`` rounds, median and min..max: each of the five GEMMs
           of the 1B model (QKV + RoPE, output + residual, gate/up + SwiGLU, down + residual — walking the 16 layers' weights in turn — and the
           tied head) on the skinny kernel and on the 256-tile kernel with the rows padded to 256, with the skinny kernel's weight bytes per
           second; a whole ``decode_step`` on prompts of about ``--prompt-len`` tokens with ``small_batch`` on and off; and one
           ``ssi.prompting.probe`` call of one prompt end to end.  ``--part small_batch_steps``: a few small-batch steps and nothing else, to be
           run under a kernel trace.
all        the three as child processes, each under its own ``timeout``, chained with ``&&``; then the results and the floor from traffic
           alone (weights read once per step, the cache read once per step) are merged into --json.
split_kv   (not part of ``all``; python tools/generate_bench.py --part split_kv --json profiles/generate_split_kv.json) what splitting the keys of a
           decode attention over workgroups buys at few rows, ONE process, the forms alternating: per launch ``ssi_attn_decode`` against walk + merge
           at spans of 64 to 512 keys (rows 1 to 256, 256 / 1000 / 4000 keys, every layer's caches in turn; the beam pair at 8 rows), whole
           ``decode_step``s with and without ``split_kv``, ``generate`` and ``sample`` end to end — and the two choices the numbers make by rule: the
           default span and ``split_max_rows``.
kv_fp8     (not part of ``all``; python tools/generate_bench.py --part kv_fp8 --json profiles/generate_kv_fp8.json) what the FP8 K/V cache buys and
           costs, ONE process, the forms alternating: per launch ``ssi_attn_decode_fp8`` against ``ssi_attn_decode`` (1 / 8 / 64 / 256 rows x 1000 and
           4000 keys, every layer's caches in turn), the two stores at 256 rows, the beam pair at 64 x 4; whole ``decode_step``s at 256 rows and the
           small-batch step at 1 and 8 rows; ``generate`` end to end; and, recorded and not asserted, the share of greedy tokens equal between the two
           caches and the largest teacher-forced logit difference (random weights: nothing about a trained checkpoint).
continuous (not part of ``all``; python tools/generate_bench.py --part continuous --prompts 1024 --rounds 3 --json profiles/generate_continuous.json) what
           refilling finished rows buys end to end, ONE process: ``sample(n=1, temperature=1.0)`` with ``--new`` new tokens at the most and every
           100th id a stop token (on the near-flat distribution of random weights the lengths come out roughly geometric with mean about 100; the
           histogram that came out is recorded), static groups against ``continuous=True`` at every ``--admit-mins`` value, the forms alternating
           over ``--rounds`` rounds, median and min..max of the call's wall time (host clock around a call that ends in a synchronise), decode
           steps, the live share of the row-steps, admissions and prompts per admission; then the same without a stop set, where both schedules
           take the same steps and the difference is the pool's bookkeeping.  The static run of the same build is the baseline.
weight_fp8 (not part of ``all``; python tools/generate_bench.py --part weight_fp8 --json profiles/generate_weight_fp8.json) what FP8 weights buy and
           cost on the small-batch path, ONE process, the forms alternating: each of the five GEMMs at 1, 16 and 64 rows, ``_w8`` entry against plain
           skinny entry, with the weight bytes per second of both; the quantiser over the whole model; the small-batch ``decode_step`` at 1, 8, 16,
           32 and 64 rows with and without ``weight_quant``; ``generate`` of 1 and 8 prompts end to end (the object built inside the call, and
           prebuilt); the added bytes; and, recorded and not asserted, the teacher-forced logit difference with and without the quantised head and
           the share of equal greedy tokens (random weights: nothing about a trained checkpoint).
"""
import argparse, csv, glob, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'speech-integration_amd')
sys.path.insert(0, PKG)

ap = argparse.ArgumentParser()
ap.add_argument('--part', default='all', choices=['all', 'run', 'steps', 'recompute', 'constrained', 'beam', 'sample', 'penalty', 'small_batch', 'small_batch_steps', 'split_kv', 'kv_fp8', 'weight_fp8', 'continuous'])
ap.add_argument('--rows', type=int, default=1, help='small_batch_steps: rows of the traced steps')
ap.add_argument('--prompts', type=int, default=256)
ap.add_argument('--penalty-generated', type=int, default=128, help='penalty: generated tokens in every row\'s history')
ap.add_argument('--prompt-len', type=int, default=1000)
ap.add_argument('--new', type=int, default=256)
ap.add_argument('--trace-steps', type=int, default=32)
ap.add_argument('--json', default=None)
ap.add_argument('--allowed-types', default='text,special_text', help='constrained: kinds of get_token_type_ranges, comma-separated')
ap.add_argument('--min-new-tokens', type=int, default=0, help='constrained: rows below it take the mask without the stop tokens')
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--beam-width', type=int, default=4)
ap.add_argument('--admit-mins', default='1,8,16,32,64', help='continuous: the admit_min values to run')
ap.add_argument('--workload', default='both', choices=['both', 'stops', 'full'], help='continuous: the workload with the stop set, the one without, or both')
ap.add_argument('--workdir', default=os.path.join(ROOT, 'prof_out', 'generate_bench'))
args = ap.parse_args()
HBM_TB_S = (5.4, 6.4)   # what the README records for the AdamW and EMA passes


def build_model():
    import copy
    import torch
    from ssi.llama_configs import configllama3_2_1b
    from ssi.model import HipLlamaDecoder
    c = copy.deepcopy(configllama3_2_1b)
    c.n_dsus = 5000
    torch.manual_seed(0)
    m = HipLlamaDecoder(**c.parameters, dtype=torch.bfloat16, device='cuda', rope_cache_len=4096)
    with torch.no_grad():
        flat = m._flat.float().normal_(0.0, 0.02).to(torch.bfloat16)
        m._flat.copy_(flat)
        del flat
        m._view('emb')[m.vocab_size:].zero_()            # the pad rows of the table stay zero
        for p, name, _ in m._param_src:
            if name.endswith('norm'):
                p.fill_(1.0)
    m.eval()
    return m


def make_prompts(vocab):
    import torch
    g = torch.Generator().manual_seed(1)
    lens = torch.randint(args.prompt_len - 100, args.prompt_len + 101, (args.prompts,), generator=g).tolist()
    return [torch.randint(0, vocab, (n,), generator=g) for n in lens]


def traffic(model, lengths, steps):
    """Bytes a decode step has to read: every weight once, and the cached K and V of every live sequence (mean over the steps)."""
    per_token = 2 * model.num_layers * model.num_kv_heads * model.head_dim * 2
    cached = sum(lengths) + len(lengths) * (steps - 1) / 2
    return {'weights_GB': round(model._flat_numel * 2 / 1e9, 3), 'cache_bytes_per_token': per_token, 'cache_GB_mean_step': round(per_token * cached / 1e9, 3)}


def part_run():
    import torch
    from ssi.generate import generate
    model = build_model()
    prompts = make_prompts(model.vocab_size)
    lens = [p.numel() for p in prompts]
    V, n = model.vocab_size, len(prompts)
    with torch.inference_mode():
        generate(model, [p[:64] for p in prompts[:8]], max_new_tokens=4, stop_token_ids=[], pad_id=0)     # warm-up: library, arena
        cache = model.new_kv_cache(n, max(lens) + args.new)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        own = torch.arange(n, dtype=torch.int32, device='cuda')
        torch.cuda.synchronize()
        ev[0].record()
        logits = model.prefill(cache, prompts, max_new_tokens=args.new)
        first = logits[:, :V].argmax(-1)
        ev[1].record()
        tok = first
        for _ in range(args.new - 1):
            tok = model.decode_step(cache, tok, own)[:, :V].argmax(-1)
        ev[2].record()
        torch.cuda.synchronize()
        prefill_ms, decode_ms = ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])
        assert int(cache.errors) == 0
        del cache
        torch.cuda.empty_cache()
        t0 = time.perf_counter()
        gens = generate(model, prompts, max_new_tokens=args.new, stop_token_ids=[], pad_id=0)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        assert [g.token_ids[0] for g in gens] == first.tolist()
        # self-check against the plain full forward, one prompt at a time.  The two runs sum in another order (a prompt packed among others
        # against a row of its own), so their bf16 logits differ a little everywhere: `noise` is the largest such difference, and a first
        # token that differs is a near-tie if the full forward's lead of its own choice over the generated one is within twice that
        same, gap, noise = 0, 0.0, 0.0
        for i, p in enumerate(prompts):
            row = model(tokens=p[None].cuda())[0, -1]
            scale = float(row.abs().max())
            noise = max(noise, float((logits[i, :V].float() - row).abs().max()) / scale)
            best = int(row.argmax())
            if best == int(first[i]):
                same += 1
            else:
                gap = max(gap, float(row[best] - row[int(first[i])]) / scale)
    steps = args.new - 1
    tr = traffic(model, lens, steps)
    step_ms = decode_ms / steps
    floor = [(tr['weights_GB'] + tr['cache_GB_mean_step']) / bw for bw in HBM_TB_S]      # GB / (TB/s) = ms
    out = {'geometry': f'Llama-3.2-1B + 5000 DSUs, bf16, random weights; {n} prompts of {min(lens)}..{max(lens)} tokens (mean {sum(lens) / n:.0f}), {args.new} new tokens each',
           'prefill_ms': round(prefill_ms, 1), 'prefill_tokens_per_s': round(sum(lens) / prefill_ms * 1e3), 'decode_steps': steps,
           'decode_ms_per_step_event': round(step_ms, 3), 'generated_tokens_per_s_decode_only': round(n * steps / decode_ms * 1e3),
           'generated_tokens_per_s_with_prefill': round(n * args.new / (prefill_ms + decode_ms) * 1e3),
           'generate_call_wall_s': round(wall, 2), 'generate_call_tokens_per_s': round(n * args.new / wall),
           'sum_prompt_tokens': sum(lens), 'traffic_per_step': tr, 'floor_ms_per_step_at_5.4_and_6.4_TB_s': [round(f, 3) for f in floor],
           'step_over_floor': [round(step_ms / f, 2) for f in floor],
           'self_check': {'prompts': n, 'first_token_equals_full_forward_argmax': same, 'differs': n - same,
                          'largest_lead_lost_over_absmax': round(gap, 5), 'largest_logit_difference_between_the_two_runs_over_absmax': round(noise, 5),
                          'every_difference_is_a_near_tie': gap <= 2 * noise}}
    print(json.dumps(out, indent=1), flush=True)
    return out


def part_steps():
    import torch
    model = build_model()
    lens = [p.numel() for p in make_prompts(model.vocab_size)]
    n, V = len(lens), model.vocab_size
    with torch.inference_mode():
        cache = model.new_kv_cache(n, max(lens) + args.new)
        cache.k.normal_()
        cache.v.normal_()
        cache.lengths.copy_(torch.tensor(lens, dtype=torch.int32))
        own = torch.arange(n, dtype=torch.int32, device='cuda')
        tok = torch.zeros(n, dtype=torch.int64, device='cuda')
        for _ in range(args.trace_steps):
            tok = model.decode_step(cache, tok, own)[:, :V].argmax(-1)
        torch.cuda.synchronize()
        assert int(cache.errors) == 0
    print(f'{args.trace_steps} decode steps done', flush=True)


def part_recompute():
    import torch
    model = build_model()
    g = torch.Generator().manual_seed(2)
    B, S, new = 8, args.prompt_len, 4
    toks = torch.randint(0, model.vocab_size, (B, S), generator=g).cuda()
    with torch.inference_mode():
        model(tokens=toks[:, :64])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(new):
            nxt = model(tokens=toks)[:, -1].argmax(-1)
            toks = torch.cat([toks, nxt[:, None]], dim=1)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    out = {'what': f'full forward of all {B} x ~{S} tokens for every new token (no cache): what the code before this change could do',
           'ms_per_new_token_of_a_batch_of_8': round(dt / new * 1e3, 1), 'generated_tokens_per_s': round(B * new / dt, 1)}
    print(json.dumps(out, indent=1), flush=True)
    return out


def spread(xs, digits=2):
    return {'median': round(statistics.median(xs), digits), 'min': round(min(xs), digits), 'max': round(max(xs), digits)}


def part_constrained():
    import copy
    import torch
    from ssi import ops
    from ssi.constants import CROSS_ENTROPY_IGNORE_IDX as IGNORE
    from ssi.generate import _mask_words, allowed_mask
    from ssi.llama_configs import configllama3_2_1b
    from ssi.train_utils import get_token_type_ranges
    c = copy.deepcopy(configllama3_2_1b)
    c.n_dsus = 5000
    ranges = get_token_type_ranges(c)
    kinds = [k for k in args.allowed_types.split(',') if k]
    model = build_model()
    n, V, ld = args.prompts, model.vocab_size, model.vocab_pad
    allow = allowed_mask(V, ranges=[ranges[k] for k in kinds])
    first_special = ranges['special_text'][0]
    stops = allowed_mask(V, ids=[first_special + k for k in (1, 8, 9)])      # end_of_text, eom, eot: the tokenizer's default stop tokens
    allow, early = allow | stops, allow & ~stops
    allow_dev, allow_w, early_w = allow.cuda(), _mask_words(allow).cuda(), _mask_words(early).cuda()
    min_new = args.min_new_tokens
    n_gen = torch.zeros(n, dtype=torch.int32, device='cuda')
    tok = torch.empty(n, dtype=torch.int64, device='cuda')
    lp, nll, loss = (torch.empty(n, dtype=torch.float32, device='cuda') for _ in range(3))
    rk = torch.empty(n, dtype=torch.int32, device='cuda')

    def kernel(x):
        ops.decode_select(x, V, tok, lp, rk, allow=allow_w, allow_early=early_w if min_new else None, n_generated=n_gen if min_new else None,
                          min_new=min_new)
        return tok

    def restated(x):
        masked = x[:, :V].masked_fill(~allow_dev, float('-inf'))
        t = masked.argmax(-1)
        return t, torch.log_softmax(x[:, :V].float(), -1).gather(1, t[:, None])[:, 0]

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3        # us per call

    res = {'geometry': f'[{n}, {ld}] bf16 logits, vocab {V}; allowed {kinds} + 3 stop tokens = {int(allow.sum())} ids; min_new_tokens {min_new}; '
                       f'{args.rounds} rounds alternating the forms in one process'}
    with torch.inference_mode():
        g = torch.Generator(device='cuda').manual_seed(3)
        bufs = [torch.randn(n, ld, generator=g, device='cuda').mul_(3).to(torch.bfloat16) for _ in range(8)]      # 8 x 68 MB: beyond L2 + MALL
        t_k, l_k = kernel(bufs[0]).clone(), lp.clone()
        t_r, l_r = restated(bufs[0])
        res['self_check'] = {'tokens_equal_the_restatement': bool(torch.equal(t_k, t_r)),
                             'largest_logprob_difference': float((l_k - l_r).abs().max())}
        forms = {'decode_select_one_buffer_us': lambda i: kernel(bufs[0]), 'torch_restatement_one_buffer_us': lambda i: restated(bufs[0]),
                 'decode_select_rotating_buffers_us': lambda i: kernel(bufs[i % 8]), 'torch_restatement_rotating_buffers_us': lambda i: restated(bufs[i % 8])}
        for fn in forms.values():
            timed(fn, 8)
        got = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, fn in forms.items():
                got[k].append(timed(fn, 40))
        res['kernel_alone'] = {k: spread(v) for k, v in got.items()}
        res['kernel_alone']['row_bytes_read_once_MB'] = round(n * V * 2 / 1e6, 1)
        res['kernel_alone']['decode_select_TB_per_s_counting_one_read'] = {k: round(n * V * 2 / 1e6 / res['kernel_alone'][k]['median'], 2)
                                                                           for k in ('decode_select_one_buffer_us', 'decode_select_rotating_buffers_us')}
        del bufs
        torch.cuda.empty_cache()

        # a decode step, on a cache of random numbers at the prompts' lengths (every block of steps starts from the same lengths)
        lens = torch.tensor([p.numel() for p in make_prompts(V)], dtype=torch.int32)
        steps = args.trace_steps
        cache = model.new_kv_cache(n, int(lens.max()) + steps + 1)
        cache.k.normal_()
        cache.v.normal_()
        own = torch.arange(n, dtype=torch.int32, device='cuda')
        alive = torch.ones(n, dtype=torch.bool, device='cuda')

        def step_plain(t):
            return model.decode_step(cache, t, own)[:, :V].argmax(-1)

        def step_logprob(t):
            x = model.decode_step(cache, t, own)
            t = x[:, :V].argmax(-1)
            ops.ce_fwd_metrics(x, torch.where(alive, t, torch.full_like(t, IGNORE)), V, IGNORE, loss, None, nll, rk)
            return t

        def step_constrained(t):
            return kernel(model.decode_step(cache, t, own)).clone()

        def block(step):
            cache.lengths.copy_(lens)
            t = torch.zeros(n, dtype=torch.int64, device='cuda')
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(steps):
                t = step(t)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / steps

        sforms = {'unconstrained_argmax_only_ms': step_plain, 'unconstrained_with_logprob_ms': step_logprob, 'constrained_ms': step_constrained}
        for fn in sforms.values():
            block(fn)
        got = {k: [] for k in sforms}
        for _ in range(args.rounds):
            for k, fn in sforms.items():
                got[k].append(block(fn))
        assert int(cache.errors) == 0
        st = {k: spread(v, 4) for k, v in got.items()}
        st['steps_per_block'] = steps
        st['constrained_minus_unconstrained_with_logprob_ms'] = round(st['constrained_ms']['median'] - st['unconstrained_with_logprob_ms']['median'], 4)
        st['unconstrained_with_logprob_spread_ms'] = round(st['unconstrained_with_logprob_ms']['max'] - st['unconstrained_with_logprob_ms']['min'], 4)
        res['decode_step'] = st
    print(json.dumps(res, indent=1), flush=True)
    return res


def part_beam():
    import torch
    from ssi import ops
    from ssi.generate import _mask_words, allowed_mask, beam_search
    model = build_model()
    W, n, V, ld, L = args.beam_width, args.prompts, model.vocab_size, model.vocab_pad, model.num_layers
    H, KV, hd = model.num_heads, model.num_kv_heads, model.head_dim
    n_seq = n // W
    R = n_seq * W
    prompts = make_prompts(V)[:n_seq]
    lens = torch.tensor([p.numel() for p in prompts], dtype=torch.int32)
    stops = [V - 3, V - 2, V - 1]
    cont_w = _mask_words(~allowed_mask(V, ids=stops)).cuda()
    dev = dict(device='cuda')

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3        # us per call

    def rounds_of(forms, reps):
        for fn in forms.values():
            timed(fn, 4)
        got = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, fn in forms.items():
                got[k].append(timed(fn, reps))
        return {k: spread(v) for k, v in got.items()}

    res = {'geometry': f'Llama-3.2-1B + 5000 DSUs, bf16, random weights; {n_seq} prompts of {int(lens.min())}..{int(lens.max())} tokens x beam_width {W} = {R} rows; '
                       f'[{R}, {ld}] logits, vocab {V}; {args.rounds} rounds alternating the forms in one process'}
    with torch.inference_mode():
        # ---- top-k alone -------------------------------------------------------------------------------------------------------------
        g = torch.Generator(device='cuda').manual_seed(3)
        bufs = [torch.randn(R, ld, generator=g, **dev).mul_(3).to(torch.bfloat16) for _ in range(8)]      # 8 x 68 MB: beyond L2 + MALL
        idx, lp, lse = torch.empty((R, W), dtype=torch.int32, **dev), torch.empty((R, W), **dev), torch.empty(R, **dev)
        tok, slp, rk = torch.empty(R, dtype=torch.int64, **dev), torch.empty(R, **dev), torch.empty(R, dtype=torch.int32, **dev)
        allow_dev = ~allowed_mask(V, ids=stops).cuda()

        def restated(x):
            masked = x[:, :V].float().masked_fill(~allow_dev, float('-inf'))
            top = masked.topk(W, dim=-1)
            return top.indices, top.values - torch.logsumexp(x[:, :V].float(), -1, keepdim=True)

        ops.topk_logprob(bufs[0], V, W, idx, lp, lse, mask=cont_w)
        r_idx, r_lp = restated(bufs[0])
        same = idx.long() == r_idx                      # (torch.topk does not promise the lower column among equal bf16 values)
        res['topk_self_check'] = {'idx_equal_torch_topk': int(same.sum()), 'of': int(same.numel()),
                                  'values_equal_where_idx_differs': bool(torch.equal(bufs[0].gather(1, idx.long())[~same], bufs[0].gather(1, r_idx)[~same])),
                                  'largest_logprob_difference': float((lp - r_lp).abs().max())}
        forms = {'topk_logprob_one_buffer_us': lambda i: ops.topk_logprob(bufs[0], V, W, idx, lp, lse, mask=cont_w),
                 'decode_select_one_buffer_us': lambda i: ops.decode_select(bufs[0], V, tok, slp, rk, allow=cont_w),
                 'torch_restatement_one_buffer_us': lambda i: restated(bufs[0]),
                 'topk_logprob_rotating_buffers_us': lambda i: ops.topk_logprob(bufs[i % 8], V, W, idx, lp, lse, mask=cont_w),
                 'decode_select_rotating_buffers_us': lambda i: ops.decode_select(bufs[i % 8], V, tok, slp, rk, allow=cont_w),
                 'torch_restatement_rotating_buffers_us': lambda i: restated(bufs[i % 8])}
        res['topk_alone'] = rounds_of(forms, 40)
        res['topk_alone']['k'] = W
        res['topk_alone']['row_bytes_read_once_MB'] = round(R * V * 2 / 1e6, 1)
        del bufs
        torch.cuda.empty_cache()

        # ---- attention alone: every layer's caches in turn, generated position t = half of --new --------------------------------------
        t_mid = args.new // 2
        pcache, bcache = model.new_kv_cache(n_seq, int(lens.max())), model.new_kv_cache(R, t_mid + args.trace_steps + 1)
        for c in (pcache, bcache):
            c.k.normal_()
            c.v.normal_()
        own = torch.arange(R, dtype=torch.int32, **dev)
        seq_of = own // W
        plen = lens.cuda().repeat_interleave(W)
        width = t_mid + args.trace_steps + 1
        anc = (seq_of[:, None] * W + torch.randint(0, W, (R, width), generator=g, **dev)).to(torch.int32).contiguous()
        gen_len = torch.full((R,), t_mid, dtype=torch.int32, **dev)
        kv_len = (plen + gen_len).contiguous()
        cap = int(kv_len.max())
        mk = torch.zeros((L, R, cap, KV * hd), dtype=torch.bfloat16, **dev)
        mv = torch.zeros_like(mk)
        for r in range(R):                              # the materialised cache: the row's prompt keys, then its ancestry's
            s, a, b = int(seq_of[r]), int(plen[r]), int(plen[r]) + t_mid
            mk[:, r, :a], mv[:, r, :a] = pcache.k[:, s, :a], pcache.v[:, s, :a]
            pos = torch.arange(t_mid, **dev)
            mk[:, r, a:b], mv[:, r, a:b] = bcache.k[:, anc[r, :t_mid].long(), pos], bcache.v[:, anc[r, :t_mid].long(), pos]
        qkv = torch.randn(R, (H + 2 * KV) * hd, generator=g, **dev).to(torch.bfloat16)
        o_b, o_c = torch.empty((R, H * hd), dtype=torch.bfloat16, **dev), torch.empty((R, H * hd), dtype=torch.bfloat16, **dev)
        l_b, l_c = torch.empty((R, H), **dev), torch.empty((R, H), **dev)
        bad = torch.zeros(1, dtype=torch.int32, **dev)

        def beam_attn(i, lse_out=None):
            l = i % L
            ops.attn_decode_beam(qkv, pcache.k[l], pcache.v[l], bcache.k[l], bcache.v[l], seq_of, plen, gen_len, anc, o_b, lse_out, H, KV, hd, n_bad=bad)

        def cont_attn(i, lse_out=None):
            l = i % L
            ops.attn_decode(qkv, mk[l], mv[l], own, kv_len, o_c, lse_out, H, KV, hd, n_bad=bad)

        beam_attn(3, l_b)
        cont_attn(3, l_c)
        res['attention_self_check'] = {'out_bit_equal': bool(torch.equal(o_b, o_c)), 'lse_bit_equal': bool(torch.equal(l_b, l_c)), 'n_bad': int(bad)}
        res['attention_alone'] = rounds_of({'attn_decode_beam_us': beam_attn, 'attn_decode_materialised_us': cont_attn}, 2 * L)
        keys = int(kv_len.sum())
        per_key = 2 * KV * hd * 2
        res['attention_alone'].update({'layers_rotated': L, 'keys_walked_per_launch': keys, 'GB_walked_per_launch': round(keys * per_key / 1e9, 3),
                                       'GB_distinct_per_launch_beam': round((int(lens.sum()) + R * t_mid) * per_key / 1e9, 3)})
        for k in ('attn_decode_beam_us', 'attn_decode_materialised_us'):
            res['attention_alone'][k.replace('_us', '_TB_per_s_walked')] = round(keys * per_key / 1e6 / res['attention_alone'][k]['median'], 2)
        del mk, mv
        torch.cuda.empty_cache()

        # ---- a decode step: the same rows and key counts in both forms -------------------------------------------------------------------
        steps = args.trace_steps
        gcache = model.new_kv_cache(R, int(lens.max()) + t_mid + steps + 1)
        gcache.k.normal_()
        gcache.v.normal_()
        start = (plen + t_mid).contiguous()

        def greedy_block():
            gcache.lengths.copy_(start)
            t = torch.zeros(R, dtype=torch.int64, **dev)
            for _ in range(steps):
                t = model.decode_step(gcache, t, own)[:, :V].argmax(-1)

        def beam_block():
            t = torch.zeros(R, dtype=torch.int64, **dev)
            for j in range(steps):
                x = model.decode_step_beam(pcache, bcache, t, seq_of, plen, anc, t_mid + j)
                ops.topk_logprob(x, V, W, idx, lp, lse, mask=cont_w)
                t = idx[:, 0].long()

        def block_ms(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / steps

        sforms = {'greedy_step_ms': greedy_block, 'beam_step_ms': beam_block}
        for fn in sforms.values():
            block_ms(fn)
        got = {k: [] for k in sforms}
        for _ in range(args.rounds):
            for k, fn in sforms.items():
                got[k].append(block_ms(fn))
        assert int(gcache.errors) == 0 and int(bcache.errors) == 0 and int(pcache.errors) == 0
        st = {k: spread(v, 4) for k, v in got.items()}
        st.update({'steps_per_block': steps, 'generated_position_at_block_start': t_mid,
                   'beam_minus_greedy_ms': round(st['beam_step_ms']['median'] - st['greedy_step_ms']['median'], 4),
                   'greedy_spread_ms': round(st['greedy_step_ms']['max'] - st['greedy_step_ms']['min'], 4)})
        res['decode_step'] = st
        del gcache, pcache, bcache
        torch.cuda.empty_cache()

    # ---- one call, end to end (its own bookkeeping and read-backs included) ---------------------------------------------------------------
    beam_search(model, [p[:64] for p in prompts[:4]], beam_width=W, max_new_tokens=4, stop_token_ids=stops, pad_id=0)      # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    found = beam_search(model, prompts, beam_width=W, max_new_tokens=args.new, stop_token_ids=stops, pad_id=0, n_best=W, batch_size=n)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    n_tok = sum(len(h.token_ids) for hs in found for h in hs)
    res['beam_search_call'] = {'prompts': n_seq, 'beam_width': W, 'max_new_tokens': args.new, 'wall_s': round(wall, 2),
                               'hypotheses': sum(len(hs) for hs in found), 'tokens_in_hypotheses': n_tok,
                               'ended_by_length': sum(h.finish_reason == 'length' for hs in found for h in hs),
                               'ms_per_step_with_prefill_and_bookkeeping': round(wall / args.new * 1e3, 3)}
    print(json.dumps(res, indent=1), flush=True)
    return res


def part_sample():
    import torch
    from ssi import ops
    from ssi.constants import CROSS_ENTROPY_IGNORE_IDX as IGNORE
    from ssi.generate import sample
    model = build_model()
    n, V, ld = args.prompts, model.vocab_size, model.vocab_pad
    dev = dict(device='cuda')
    T = 0.8
    settings = {'temperature_only': dict(top_k=-1, top_p=1.0), 'top_k_50': dict(top_k=50, top_p=1.0), 'top_p_0.9': dict(top_k=-1, top_p=0.9),
                'top_k_50_top_p_0.9': dict(top_k=50, top_p=0.9)}
    walks = {'temperature_only': 2, 'top_k_50': 4, 'top_p_0.9': 4, 'top_k_50_top_p_0.9': 6}       # bf16: 2 radix passes per threshold

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3        # us per call

    res = {'geometry': f'[{n}, {ld}] bf16 logits (3 randn), vocab {V}, temperature {T}; {args.rounds} rounds alternating the forms in one process'}
    with torch.inference_mode():
        g = torch.Generator(device='cuda').manual_seed(3)
        x = torch.randn(n, ld, generator=g, **dev).mul_(3).to(torch.bfloat16)
        tok, lp, kept = torch.empty(n, dtype=torch.int64, **dev), torch.empty(n, **dev), torch.empty(n, dtype=torch.int32, **dev)
        rk = torch.empty(n, dtype=torch.int32, **dev)
        seqs = torch.arange(n, dtype=torch.int32, **dev)

        def kernel(s, step=0, logits=None):
            ops.decode_sample(x if logits is None else logits, V, tok, lp, kept, temperature=T, seed=1, step=step, sequence=seqs, **settings[s])
            return tok

        def restated(s):
            """torch: sort, the top-k cut, cumsum for the top-p cut, a Gumbel argmax over what is left (torch's own random bits)."""
            k, p = settings[s]['top_k'], settings[s]['top_p']
            v, idx = torch.sort(x[:, :V].float() / T, dim=-1, descending=True)
            if k > 0:
                v = v.masked_fill(v < v[:, k - 1:k], float('-inf'))
            if p < 1.0:
                pr = torch.softmax(v, -1)
                v = v.masked_fill((pr.cumsum(-1) - pr) >= p, float('-inf'))
            gum = -torch.log(-torch.log(torch.rand_like(v).clamp_(1e-7, 1 - 1e-7)))
            t = idx.gather(1, (v + gum).argmax(-1, keepdim=True))[:, 0]
            return t, torch.log_softmax(x[:, :V].float(), -1).gather(1, t[:, None])[:, 0]

        check = {}
        for s in settings:
            kernel(s)
            k, p = settings[s]['top_k'], settings[s]['top_p']
            v = torch.sort(x[:, :V].float(), dim=-1, descending=True).values
            want = torch.full((n,), V, dtype=torch.int64, **dev) if k <= 0 else (v >= v[:, k - 1:k]).sum(-1)
            check[s] = {'n_kept_mean': round(float(kept.float().mean()), 1), 'n_kept_equals_torch_count_without_top_p': bool(torch.equal(kept.long(), want)) if p >= 1.0 else None,
                        'tokens_in_range': bool(((tok >= 0) & (tok < V)).all())}
        res['self_check'] = check
        forms = {f'decode_sample_{s}_us': (lambda i, s=s: kernel(s, i)) for s in settings}
        forms['decode_select_us'] = lambda i: ops.decode_select(x, V, tok, lp, rk)
        forms.update({f'torch_restatement_{s}_us': (lambda i, s=s: restated(s)) for s in ('temperature_only', 'top_k_50', 'top_p_0.9')})
        for fn in forms.values():
            timed(fn, 4)
        got = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, fn in forms.items():
                got[k].append(timed(fn, 20))
        ka = {k: spread(v) for k, v in got.items()}
        per_walk = ka['decode_select_us']['median'] / 2
        ka['row_bytes_read_once_MB'] = round(n * V * 2 / 1e6, 1)
        ka['reading_the_rows_once_us_at_5.4_and_6.4_TB_s'] = [round(n * V * 2 / 1e6 / bw, 1) for bw in HBM_TB_S]
        ka['decode_select_per_walk_us'] = round(per_walk, 2)
        ka['walks'] = walks
        ka['over_walks_times_select_per_walk'] = {s: round(ka[f'decode_sample_{s}_us']['median'] / (walks[s] * per_walk), 2) for s in settings}
        res['kernel_alone'] = ka

        # a decode step, on a cache of random numbers at the prompts' lengths (every block of steps starts from the same lengths)
        lens = torch.tensor([p.numel() for p in make_prompts(V)], dtype=torch.int32)
        steps = args.trace_steps
        cache = model.new_kv_cache(n, int(lens.max()) + steps + 1)
        cache.k.normal_()
        cache.v.normal_()
        own = torch.arange(n, dtype=torch.int32, **dev)
        loss, nll = torch.empty(n, **dev), torch.empty(n, **dev)

        def step_greedy(t, j):
            xx = model.decode_step(cache, t, own)
            t = xx[:, :V].argmax(-1)
            ops.ce_fwd_metrics(xx, t, V, IGNORE, loss, None, nll, rk)
            return t

        def step_sampled(t, j):
            return kernel('top_k_50_top_p_0.9', j, model.decode_step(cache, t, own)).clone()

        def block(step):
            cache.lengths.copy_(lens)
            t = torch.zeros(n, dtype=torch.int64, **dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for j in range(steps):
                t = step(t, j)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / steps

        sforms = {'greedy_with_logprob_ms': step_greedy, 'sampled_top_k_50_top_p_0.9_ms': step_sampled}
        for fn in sforms.values():
            block(fn)
        got = {k: [] for k in sforms}
        for _ in range(args.rounds):
            for k, fn in sforms.items():
                got[k].append(block(fn))
        assert int(cache.errors) == 0
        st = {k: spread(v, 4) for k, v in got.items()}
        st.update({'steps_per_block': steps, 'sampled_minus_greedy_ms': round(st['sampled_top_k_50_top_p_0.9_ms']['median'] - st['greedy_with_logprob_ms']['median'], 4),
                   'greedy_spread_ms': round(st['greedy_with_logprob_ms']['max'] - st['greedy_with_logprob_ms']['min'], 4)})
        res['decode_step'] = st
        del cache
        torch.cuda.empty_cache()

    # ---- one call with n = 4, end to end ---------------------------------------------------------------------------------------------------
    prompts = make_prompts(V)[:n // 4]
    kw = dict(n=4, temperature=T, top_k=50, top_p=0.9, seed=1, stop_token_ids=[], pad_id=0)
    sample(model, [p[:64] for p in prompts[:4]], max_new_tokens=4, **kw)      # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    found = sample(model, prompts, max_new_tokens=args.new, batch_size=n, **kw)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    n_tok = sum(len(h.token_ids) for hs in found for h in hs)
    res['sample_call'] = {'prompts': len(prompts), 'n': 4, 'max_new_tokens': args.new, 'wall_s': round(wall, 2), 'generated_tokens': n_tok,
                          'generated_tokens_per_s': round(n_tok / wall), 'ms_per_step_with_prefill_and_bookkeeping': round(wall / args.new * 1e3, 3),
                          'distinct_samples_per_prompt_mean': round(sum(len({tuple(h.token_ids) for h in hs}) for hs in found) / len(found), 2),
                          'kept_tokens_mean': round(sum(h.n_kept_mean * len(h.token_ids) for hs in found for h in hs) / max(n_tok, 1), 2)}
    print(json.dumps(res, indent=1), flush=True)
    return res


def part_penalty():
    """What the repetition, frequency and presence penalties cost inside the two selection kernels, ONE process: each penalised kernel against
    its plain kernel on the same logits (greedy; temperature only; top-k 50; top-p 0.9; both), the plain sampler on fp32 logits for the
    settings whose bf16 radix passes double under penalties, a torch restatement (count scatter, the three passes over a copy, then the
    selection), and a penalised greedy decode step of the model against the plain one."""
    import torch
    from ssi import ops
    from ssi.constants import CROSS_ENTROPY_IGNORE_IDX as IGNORE
    model = build_model()
    n, V, ld = args.prompts, model.vocab_size, model.vocab_pad
    dev = dict(device='cuda')
    T, pen = 0.8, dict(repetition_penalty=1.3, frequency_penalty=0.5, presence_penalty=0.5)
    n_hist, ld_gen = args.penalty_generated, 256
    settings = {'temperature_only': dict(top_k=-1, top_p=1.0), 'top_k_50': dict(top_k=50, top_p=1.0), 'top_p_0.9': dict(top_k=-1, top_p=0.9),
                'top_k_50_top_p_0.9': dict(top_k=50, top_p=0.9)}
    thresholds = {'temperature_only': 0, 'top_k_50': 1, 'top_p_0.9': 1, 'top_k_50_top_p_0.9': 2}
    walks_plain = {s: 2 + 2 * t for s, t in thresholds.items()}           # bf16 keys: 2 radix passes per threshold
    walks_pen = {s: 2 + 4 * t for s, t in thresholds.items()}             # the penalised value is fp32: 4 passes per threshold

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3        # us per call

    res = {'geometry': f'[{n}, {ld}] bf16 logits (3 randn), vocab {V}; per row a prompt of {args.prompt_len} ids and {n_hist} generated ids (ld_gen {ld_gen}); '
                       f'penalties {pen}; temperature {T}; {args.rounds} rounds alternating the forms in one process',
           'dynamic_lds_bytes': ops.decode_penalty_lds_bytes(V, ld_gen)}
    with torch.inference_mode():
        g = torch.Generator(device='cuda').manual_seed(3)
        x = torch.randn(n, ld, generator=g, **dev).mul_(3).to(torch.bfloat16)
        x32 = x.float()
        tok, lp, kept = torch.empty(n, dtype=torch.int64, **dev), torch.empty(n, **dev), torch.empty(n, dtype=torch.int32, **dev)
        rk = torch.empty(n, dtype=torch.int32, **dev)
        seqs = torch.arange(n, dtype=torch.int32, **dev)
        pid = torch.randint(0, V, (n, args.prompt_len), generator=g, **dev).to(torch.int32)
        plen = torch.full((n,), args.prompt_len, dtype=torch.int32, **dev)
        gid = torch.randint(0, V, (n, ld_gen), generator=g, **dev)
        gid[:, 1:n_hist:4] = gid[:, 0:1]                                  # a loop: every fourth generated token is the row's first
        top = x[:, :V].float().topk(8, dim=-1).indices
        gid[:, 2:18:2] = top                                              # and the row's largest columns are in the history, so the choice moves
        n_gen = torch.full((n,), n_hist, dtype=torch.int32, **dev)
        n_bad = torch.zeros(1, dtype=torch.int32, **dev)
        hist = dict(prompt_ids=pid, prompt_len=plen, gen_ids=gid, n_generated=n_gen, n_bad=n_bad, **pen)

        def torch_penalised():
            """vLLM's apply_penalties in torch: the count scatter, the seen mask, and three passes over a copy of the logits."""
            cnt = torch.zeros(n, V, dtype=torch.int32, **dev).scatter_add_(1, gid[:, :n_hist], torch.ones(n, n_hist, dtype=torch.int32, **dev))
            seen = (cnt > 0).scatter_(1, pid.long(), True)
            y = x[:, :V].float()
            y = torch.where(seen, torch.where(y > 0, y / pen['repetition_penalty'], y * pen['repetition_penalty']), y)
            y = y - pen['frequency_penalty'] * cnt
            return y - pen['presence_penalty'] * (cnt > 0)

        def torch_greedy(i):
            t = torch_penalised().argmax(-1)
            return t, torch.log_softmax(x[:, :V].float(), -1).gather(1, t[:, None])[:, 0]

        def torch_sampled(i, s='top_k_50'):
            k = settings[s]['top_k']
            v, idx = torch.sort(torch_penalised() / T, dim=-1, descending=True)
            v = v.masked_fill(v < v[:, k - 1:k], float('-inf'))
            gum = -torch.log(-torch.log(torch.rand_like(v).clamp_(1e-7, 1 - 1e-7)))
            return idx.gather(1, (v + gum).argmax(-1, keepdim=True))[:, 0]

        ops.decode_select_pen(x, V, tok, lp, rk, **hist)
        want = torch_greedy(0)[0]
        res['self_check'] = {'greedy_tokens_equal_torch_restatement': round(float((tok == want).float().mean()), 4),
                             'rows_whose_choice_the_penalties_changed': int((rk != 0).sum()), 'n_bad': int(n_bad)}
        forms = {'decode_select_us': lambda i: ops.decode_select(x, V, tok, lp, rk),
                 'decode_select_pen_us': lambda i: ops.decode_select_pen(x, V, tok, lp, rk, **hist),
                 'decode_select_fp32_logits_us': lambda i: ops.decode_select(x32, V, tok, lp, rk)}
        for s, kw in settings.items():
            forms[f'decode_sample_{s}_us'] = lambda i, kw=kw: ops.decode_sample(x, V, tok, lp, kept, temperature=T, seed=1, step=i, sequence=seqs, **kw)
            forms[f'decode_sample_pen_{s}_us'] = lambda i, kw=kw: ops.decode_sample_pen(x, V, tok, lp, kept, temperature=T, seed=1, step=i,
                                                                                         sequence=seqs, **kw, **hist)
            if thresholds[s]:
                forms[f'decode_sample_fp32_logits_{s}_us'] = lambda i, kw=kw: ops.decode_sample(x32, V, tok, lp, kept, temperature=T, seed=1, step=i,
                                                                                                sequence=seqs, **kw)
        forms['torch_restatement_greedy_us'] = torch_greedy
        forms['torch_restatement_top_k_50_us'] = torch_sampled
        for fn in forms.values():
            timed(fn, 3)
        got = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, fn in forms.items():
                got[k].append(timed(fn, 4 if k.startswith('torch') else 20))
        ka = {k: spread(v) for k, v in got.items()}
        per_walk = ka['decode_select_us']['median'] / 2
        ka['decode_select_per_walk_us'] = round(per_walk, 2)
        ka['decode_select_fp32_logits_per_walk_us'] = round(ka['decode_select_fp32_logits_us']['median'] / 2, 2)
        ka['walks_plain'], ka['walks_penalised'] = walks_plain, walks_pen
        ka['select_pen_minus_select_us'] = round(ka['decode_select_pen_us']['median'] - ka['decode_select_us']['median'], 2)
        ka['penalised_over_walks_times_plain_per_walk'] = dict(
            {'greedy': round(ka['decode_select_pen_us']['median'] / (2 * per_walk), 2)},
            **{s: round(ka[f'decode_sample_pen_{s}_us']['median'] / (walks_pen[s] * per_walk), 2) for s in settings})
        ka['penalised_over_plain'] = dict({'greedy': round(ka['decode_select_pen_us']['median'] / ka['decode_select_us']['median'], 2)},
                                          **{s: round(ka[f'decode_sample_pen_{s}_us']['median'] / ka[f'decode_sample_{s}_us']['median'], 2) for s in settings})
        ka['penalised_bf16_over_plain_fp32_logits'] = {s: round(ka[f'decode_sample_pen_{s}_us']['median'] / ka[f'decode_sample_fp32_logits_{s}_us']['median'], 2)
                                                       for s in settings if thresholds[s]}
        res['kernel_alone'] = ka

        lens = torch.tensor([p.numel() for p in make_prompts(V)], dtype=torch.int32)
        steps = args.trace_steps
        cache = model.new_kv_cache(n, int(lens.max()) + steps + 1)
        cache.k.normal_()
        cache.v.normal_()
        own = torch.arange(n, dtype=torch.int32, **dev)
        loss, nll = torch.empty(n, **dev), torch.empty(n, **dev)

        def step_greedy(t, j):
            xx = model.decode_step(cache, t, own)
            t = xx[:, :V].argmax(-1)
            ops.ce_fwd_metrics(xx, t, V, IGNORE, loss, None, nll, rk)
            return t

        def step_penalised(t, j):
            ops.decode_select_pen(model.decode_step(cache, t, own), V, tok, lp, rk, **hist)
            return tok.clone()

        def block(step):
            cache.lengths.copy_(lens)
            t = torch.zeros(n, dtype=torch.int64, **dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for j in range(steps):
                t = step(t, j)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / steps

        sforms = {'greedy_with_logprob_ms': step_greedy, 'penalised_greedy_with_logprob_ms': step_penalised}
        for fn in sforms.values():
            block(fn)
        got = {k: [] for k in sforms}
        for _ in range(args.rounds):
            for k, fn in sforms.items():
                got[k].append(block(fn))
        assert int(cache.errors) == 0 and int(n_bad) == 0
        st = {k: spread(v, 4) for k, v in got.items()}
        st.update({'steps_per_block': steps, 'penalised_minus_greedy_ms': round(st['penalised_greedy_with_logprob_ms']['median'] - st['greedy_with_logprob_ms']['median'], 4),
                   'greedy_spread_ms': round(st['greedy_with_logprob_ms']['max'] - st['greedy_with_logprob_ms']['min'], 4)})
        res['decode_step'] = st
    print(json.dumps(res, indent=1), flush=True)
    return res


SMALL_ROWS = (1, 8, 16, 32, 64)


def _small_cache(model, rows, room=4096, dtype=None):
    """A cache of ``rows`` prompts of about --prompt-len tokens, prefilled, with ``room`` positions for the measured steps."""
    import torch
    g = torch.Generator().manual_seed(1)
    lens = torch.randint(args.prompt_len - 100, args.prompt_len + 101, (rows,), generator=g).tolist()
    prompts = [torch.randint(0, model.vocab_size, (n,), generator=g) for n in lens]
    cache = model.new_kv_cache(rows, max(lens) + room, dtype)
    model.prefill(cache, prompts)
    return cache, lens


def part_small_batch():
    import torch
    from ssi import ops
    from ssi.ops import GEMM_NT
    from ssi.prompting import probe
    model = build_model()
    D, I, L, dev = model.embed_dim, model.intermediate_dim, model.num_layers, dict(device='cuda')
    bf = torch.bfloat16

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3        # us per call

    res = {'geometry': f'1B shape, bf16; rows {list(SMALL_ROWS)}; {args.rounds} rounds alternating the forms in one process; the layer GEMMs walk the '
                       f'{L} layers\' weights in turn (call i reads layer i % {L}), the head reads the one table',
           'hbm_TB_per_s_of_the_adamw_and_ema_passes': list(HBM_TB_S)}
    with torch.inference_mode():
        g = torch.Generator(device='cuda').manual_seed(5)
        x256 = {k: torch.randn(256, k, generator=g, **dev).mul_(0.5).to(bf) for k in (D, I)}
        pos256 = torch.randint(0, 1000, (256,), generator=g, **dev).to(torch.int32)
        W = lambda name: [model._view(f'L{l}.{name}') for l in range(L)]   # noqa: E731
        wqkv, wo, w13, w2, emb = W('wqkv'), W('wo'), W('w13'), W('w2'), model._view('emb')
        H = model.num_heads + model.num_kv_heads
        out = {n: torch.empty(256, n, **dev, dtype=bf) for n in (model.qkv_dim, D, 2 * I, I, model.vocab_pad)}
        res_in = torch.randn(256, D, generator=g, **dev).to(bf)
        shapes = {
            'qkv_rope_3072x2048': (model.qkv_dim * D * 2,
                                   lambda m: (lambda i: ops.gemm_skinny_rope(x256[D][:m], wqkv[i % L], out[model.qkv_dim][:m], H, 64, model._rope, pos256[:m])),
                                   lambda i: ops.gemm_rope(x256[D], wqkv[i % L], out[model.qkv_dim], 256, H, 64, model._rope, positions=pos256)),
            'wo_residual_2048x2048': (D * D * 2,
                                      lambda m: (lambda i: ops.gemm_skinny(x256[D][:m], wo[i % L], out[D][:m], residual=res_in[:m])),
                                      lambda i: model._gemm(GEMM_NT, x256[D], wo[i % L], out[D], residual=res_in)),
            'w13_swiglu_16384x2048': (2 * I * D * 2,
                                      lambda m: (lambda i: ops.gemm_skinny_swiglu(x256[D][:m], w13[i % L], None, out[I][:m])),
                                      lambda i: ops.gemm_swiglu_fwd(x256[D], w13[i % L], out[2 * I], out[I])),
            'w2_residual_2048x8192': (D * I * 2,
                                      lambda m: (lambda i: ops.gemm_skinny(x256[I][:m], w2[i % L], out[D][:m], residual=res_in[:m])),
                                      lambda i: model._gemm(GEMM_NT, x256[I], w2[i % L], out[D], residual=res_in)),
            'head_133376x2048': (model.vocab_pad * D * 2,
                                 lambda m: (lambda i: ops.gemm_skinny(x256[D][:m], emb, out[model.vocab_pad][:m])),
                                 lambda i: ops.gemm(GEMM_NT, x256[D], emb, out[model.vocab_pad])),
        }
        gemms = {}
        for name, (wbytes, skinny_of, tiled) in shapes.items():
            reps = 8 if name.startswith('head') else 64
            forms = {f'skinny_M{m}_us': skinny_of(m) for m in SMALL_ROWS}
            forms['tile_256_rows_us'] = tiled
            for fn in forms.values():
                timed(fn, 4)
            rounds = {k: [] for k in forms}
            for _ in range(args.rounds):
                for k, fn in forms.items():
                    rounds[k].append(timed(fn, reps))
            entry = {k: spread(v) for k, v in rounds.items()}
            entry['weight_MB'] = round(wbytes / 1e6, 2)
            entry['skinny_weight_TB_per_s'] = {f'M{m}': round(wbytes / 1e6 / entry[f'skinny_M{m}_us']['median'], 2) for m in SMALL_ROWS}
            entry['tile_over_skinny'] = {f'M{m}': round(entry['tile_256_rows_us']['median'] / entry[f'skinny_M{m}_us']['median'], 2) for m in SMALL_ROWS}
            gemms[name] = entry
        res['gemms'] = gemms
        per_layer = lambda key: sum(gemms[n][key]['median'] for n in gemms if not n.startswith('head'))   # noqa: E731
        res['gemm_us_per_step_from_the_parts'] = dict(
            {f'skinny_M{m}': round(L * per_layer(f'skinny_M{m}_us') + gemms['head_133376x2048'][f'skinny_M{m}_us']['median'], 1) for m in SMALL_ROWS},
            tile_256_rows=round(L * per_layer('tile_256_rows_us') + gemms['head_133376x2048']['tile_256_rows_us']['median'], 1))
        del x256, out, res_in

        # whole steps: the same cache state for both forms of a row count (the lengths are put back before every block of steps)
        steps, st = 16, {}
        for m in SMALL_ROWS:
            cache, lens = _small_cache(model, m)
            start = cache.lengths.clone()
            tok = torch.randint(0, model.vocab_size, (m,), **dev)
            slot = torch.arange(m, dtype=torch.int32, **dev)

            def block(small):
                cache.lengths.copy_(start)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    model.decode_step(cache, tok, slot, small_batch=small)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / steps * 1e3      # ms per step, host clock: what a loop sees

            block(True), block(False)
            rounds = {'small_batch_ms': [], 'padded_ms': []}
            for _ in range(args.rounds):
                rounds['small_batch_ms'].append(block(True))
                rounds['padded_ms'].append(block(False))
            e = {k: spread(v, 3) for k, v in rounds.items()}
            e['prompt_tokens_mean'] = round(sum(lens) / m, 1)
            e['padded_minus_small_batch_ms'] = round(e['padded_ms']['median'] - e['small_batch_ms']['median'], 3)
            e['padded_spread_ms'] = round(e['padded_ms']['max'] - e['padded_ms']['min'], 3)
            e['small_batch_wins_by_more_than_the_padded_spread'] = bool(e['padded_minus_small_batch_ms'] > e['padded_spread_ms'])
            st[f'rows_{m}'] = e
            assert int(cache.errors) == 0
            del cache
        res['decode_step'] = dict(st, steps_per_block=steps, clock='host, synchronised around a block of steps')
        winners = [m for m in SMALL_ROWS if st[f'rows_{m}']['small_batch_wins_by_more_than_the_padded_spread']]
        res['skinny_max_rows'] = {'rule': 'the largest measured row count at which the small-batch step beats the padded step by more than the padded '
                                          'step\'s own min..max spread',
                                  'padded_step': 'measured on THIS build, not on the parent commit: an inference from the padded step\'s launches and kernels being the parent\'s '
                                                 '(kernel_lint --against the parent build, the recorded launch trace), not the parent\'s own measurement',
                                  'qualifying_rows': winners, 'chosen': max(winners) if winners else None, 'model_attribute': model.skinny_max_rows}
        # end to end: generate() of 8, 32 and 64 prompts, both ways.  With the flag a group also prefills prompt by prompt (one forward per
        # prompt instead of the packed rows), which is what a last group of many prompts pays for the cheaper steps.
        from ssi.generate import generate
        e2e = {}
        for n_p in (1, 8, 32, 64):
            gen = torch.Generator().manual_seed(7)
            lens = torch.randint(args.prompt_len - 100, args.prompt_len + 101, (n_p,), generator=gen).tolist()
            prompts = [torch.randint(0, model.vocab_size, (n,), generator=gen) for n in lens]

            def run(small, new):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                generate(model, prompts, max_new_tokens=new, stop_token_ids=[], pad_id=0, small_batch=small)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3

            run(True, 2), run(False, 2)
            rounds = {'small_batch_ms': [], 'padded_ms': [], 'small_batch_prefill_and_1_step_ms': [], 'padded_prefill_and_1_step_ms': []}
            for _ in range(3):
                rounds['small_batch_ms'].append(run(True, args.new))
                rounds['padded_ms'].append(run(False, args.new))
                rounds['small_batch_prefill_and_1_step_ms'].append(run(True, 2))
                rounds['padded_prefill_and_1_step_ms'].append(run(False, 2))
            e = {k: spread(v, 1) for k, v in rounds.items()}
            e['padded_over_small_batch'] = round(e['padded_ms']['median'] / e['small_batch_ms']['median'], 2)
            e['prefill_extra_ms_per_prompt'] = round((e['small_batch_prefill_and_1_step_ms']['median'] - e['padded_prefill_and_1_step_ms']['median']) / n_p, 2)
            e2e[f'prompts_{n_p}'] = e
        res['generate_end_to_end'] = dict(e2e, new_tokens=args.new, rounds=3,
                                          note='generate() of n prompts of about --prompt-len tokens, --new new tokens, host clock; with small_batch the group prefills prompt by prompt')
        res['weights_floor_ms_at_5.4_and_6.4_TB_s'] = [round(model._flat_numel * 2 / 1e9 / bw, 3) for bw in HBM_TB_S]

    class _Tok:                                                   # ids as text: the probe's host path without a tokenizer file
        eos_id, eom_id, eot_id, pad_id, special_tokens = 1, 2, 3, 0, {}

        def decode(self, ids, **kw):
            return ' '.join(map(str, ids))

    g = torch.Generator().manual_seed(2)
    prompt = torch.randint(4, model.vocab_size, (args.prompt_len,), generator=g).tolist()
    probe(model, _Tok(), [prompt], max_new_tokens=8, stop_token_ids=[])
    times = []
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        found = probe(model, _Tok(), [prompt], max_new_tokens=args.new, stop_token_ids=[])
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    n_new = len(found[0].generations[0].token_ids)
    res['probe_one_prompt'] = {'prompt_tokens': len(prompt), 'new_tokens': n_new, 'call_ms': spread(times, 1),
                               'ms_per_new_token_prefill_included': round(statistics.median(times) / n_new, 3)}
    print(json.dumps(res, indent=1))
    return res


SPLIT_ROWS, SPLIT_KEYS, SPLIT_SPANS = (1, 8, 16, 32, 64, 256), (256, 1000, 4000), (64, 128, 256, 512)


def part_split_kv():
    import torch
    from ssi import ops
    from ssi.generate import generate, sample
    model = build_model()
    L, H, KV, hd = model.num_layers, model.num_heads, model.num_kv_heads, model.head_dim
    dev, bf = dict(device='cuda'), torch.bfloat16

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3        # us per call

    def rounds_of(forms, reps):
        for fn in forms.values():
            timed(fn, 4)
        got = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, fn in forms.items():
                got[k].append(timed(fn, reps))
        return {k: spread(v) for k, v in got.items()}

    res = {'geometry': f'1B shape (32 / 8 / 64), bf16; {args.rounds} rounds alternating the forms in one process; per launch call i reads layer i % {L}\'s caches; '
                       f'the split forms are walk + merge, two launches, timed together',
           'hbm_TB_per_s_of_the_adamw_and_ema_passes': list(HBM_TB_S)}
    with torch.inference_mode():
        g = torch.Generator(device='cuda').manual_seed(11)
        R, cap = max(SPLIT_ROWS), max(SPLIT_KEYS)
        kc = torch.empty((L, R, cap, KV * hd), dtype=bf, **dev).normal_(generator=g)
        vc = torch.empty((L, R, cap, KV * hd), dtype=bf, **dev).normal_(generator=g)
        qkv = torch.randn(R, (H + 2 * KV) * hd, generator=g, **dev).to(bf)
        out = torch.empty((R, H * hd), dtype=bf, **dev)
        slot = torch.arange(R, dtype=torch.int32, **dev)
        ws = torch.empty(ops.attn_decode_split_workspace(R, H, hd, cap, min(SPLIT_SPANS)), **dev)
        per = {}
        for rows in SPLIT_ROWS:
            for keys in SPLIT_KEYS:
                kv_len = torch.full((rows,), keys, dtype=torch.int32, **dev)
                q, o, sl = qkv[:rows], out[:rows], slot[:rows]
                forms = {'plain_us': lambda i: ops.attn_decode(q, kc[i % L], vc[i % L], sl, kv_len, o, None, H, KV, hd)}
                for span in SPLIT_SPANS:
                    forms[f'split_span{span}_us'] = (lambda span: lambda i: ops.attn_decode_split(q, kc[i % L], vc[i % L], sl, kv_len, o, None, H, KV, hd,
                                                                                                   span=span, workspace=ws))(span)
                e = rounds_of(forms, 32)
                e['cache_MB_read'] = round(rows * keys * 2 * KV * hd * 2 / 1e6, 2)
                e['plain_over_split'] = {f'span{span}': round(e['plain_us']['median'] / e[f'split_span{span}_us']['median'], 2) for span in SPLIT_SPANS}
                e['best_split_TB_per_s'] = round(e['cache_MB_read'] / 1e6 / (min(e[f'split_span{span}_us']['median'] for span in SPLIT_SPANS) * 1e-6), 3)
                per[f'rows_{rows}_keys_{keys}'] = e
        res['per_launch'] = dict(per, note=f'the caches are [{R} slots, cap {cap}]: a launch of fewer rows and keys reads the first of them, so n_splits = ceil({cap} / span) '
                                           'in every launch and the workgroups beyond a row\'s keys return at once')
        # the default span: lowest median at 1 row and 1000 keys; of two spans inside each other's min..max spread, the larger
        at = per['rows_1_keys_1000']
        m = {span: at[f'split_span{span}_us'] for span in SPLIT_SPANS}
        best = min(SPLIT_SPANS, key=lambda sp: m[sp]['median'])
        inside = lambda a, b: m[b]['min'] <= m[a]['median'] <= m[b]['max'] and m[a]['min'] <= m[b]['median'] <= m[a]['max']   # noqa: E731
        chosen = max([best] + [sp for sp in SPLIT_SPANS if sp > best and inside(sp, best)])
        res['default_span'] = {'rule': 'the span with the lowest median at 1 row and 1000 keys; of two spans that lie inside each other\'s min..max spread the larger '
                                       '(fewer partials, a smaller workspace)',
                               'lowest_median': best, 'chosen': chosen, 'library_default': ops.attn_decode_split_span(hd, bf)}
        # the beam pair at 8 rows: one prompt of --prompt-len keys, 8 hypotheses, 128 generated positions read through a random ancestry
        W, t_mid = 8, 128
        pk, pv = kc[:, :1, :args.prompt_len].contiguous(), vc[:, :1, :args.prompt_len].contiguous()
        bk, bv = kc[:, :W, :t_mid + 1].contiguous(), vc[:, :W, :t_mid + 1].contiguous()
        anc = torch.randint(0, W, (W, t_mid + 1), generator=g, **dev).to(torch.int32).contiguous()
        pslot = torch.zeros(W, dtype=torch.int32, **dev)
        plen, glen = torch.full((W,), args.prompt_len, dtype=torch.int32, **dev), torch.full((W,), t_mid, dtype=torch.int32, **dev)
        forms = {'plain_us': lambda i: ops.attn_decode_beam(qkv[:W], pk[i % L], pv[i % L], bk[i % L], bv[i % L], pslot, plen, glen, anc, out[:W], None, H, KV, hd)}
        for span in SPLIT_SPANS:
            forms[f'split_span{span}_us'] = (lambda span: lambda i: ops.attn_decode_beam_split(qkv[:W], pk[i % L], pv[i % L], bk[i % L], bv[i % L], pslot, plen, glen,
                                                                                                anc, out[:W], None, H, KV, hd, span=span, workspace=ws))(span)
        e = rounds_of(forms, 32)
        e['plain_over_split'] = {f'span{span}': round(e['plain_us']['median'] / e[f'split_span{span}_us']['median'], 2) for span in SPLIT_SPANS}
        res['per_launch_beam_8_rows'] = dict(e, prompt_keys=args.prompt_len, generated_keys=t_mid)
        del kc, vc, pk, pv, bk, bv, ws
        torch.cuda.empty_cache()

        # whole steps: the same cache state for both forms of a row count (the lengths are put back before every block of steps)
        steps, st = 16, {}
        for m_rows, small in [(r, True) for r in (1, 8, 16, 32, 64)] + [(1, False), (8, False)]:
            cache, lens = _small_cache(model, m_rows, room=64)       # (a tight cap, as generate() opens it: n_splits follows the cap)
            start = cache.lengths.clone()
            tok = torch.randint(0, model.vocab_size, (m_rows,), **dev)
            sl = torch.arange(m_rows, dtype=torch.int32, **dev)
            model.split_max_rows = 256                       # the rule under measurement must not decide what is measured

            def block(split):
                cache.lengths.copy_(start)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    model.decode_step(cache, tok, sl, small_batch=small, split_kv=split)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / steps * 1e3      # ms per step, host clock: what a loop sees

            block(True), block(False)
            rounds = {'split_kv_ms': [], 'unsplit_ms': []}
            for _ in range(args.rounds):
                rounds['split_kv_ms'].append(block(True))
                rounds['unsplit_ms'].append(block(False))
            e = {k: spread(v, 3) for k, v in rounds.items()}
            e['prompt_tokens_mean'] = round(sum(lens) / m_rows, 1)
            e['unsplit_minus_split_kv_ms'] = round(e['unsplit_ms']['median'] - e['split_kv_ms']['median'], 3)
            e['unsplit_spread_ms'] = round(e['unsplit_ms']['max'] - e['unsplit_ms']['min'], 3)
            e['split_kv_wins_by_more_than_the_unsplit_spread'] = bool(e['unsplit_minus_split_kv_ms'] > e['unsplit_spread_ms'])
            st[f'rows_{m_rows}' + ('' if small else '_padded_to_256')] = e
            assert int(cache.errors) == 0
            del cache
        del model.split_max_rows
        res['decode_step'] = dict(st, steps_per_block=steps, span=int(model.split_span or ops.attn_decode_split_span(hd, bf)),
                                  clock='host, synchronised around a block of steps',
                                  note='rows_N: small_batch steps of N unpadded rows; rows_N_padded_to_256: the tile path with N live rows')
        winners = [r for r in (1, 8, 16, 32, 64) if st[f'rows_{r}']['split_kv_wins_by_more_than_the_unsplit_spread']]
        res['split_max_rows'] = {'rule': 'the largest measured row count at which the split-KV step beats the unsplit step by more than the unsplit step\'s own '
                                         'min..max spread; none: 0',
                                 'unsplit_step': 'measured on THIS build, not on the parent commit: an inference from kernel_lint --against the parent build, '
                                                 'which shows the plain decode kernels within a few instructions of the parent\'s, not the parent\'s own measurement',
                                 'qualifying_rows': winners, 'chosen': max(winners) if winners else 0, 'model_attribute': model.split_max_rows}

        # end to end (the model's own split_max_rows decides): generate() of 1 and 8 prompts of about --prompt-len tokens and of one long prompt, sample(n=8)
        e2e = {}
        long_len = model._rope.shape[0] - args.new - 40          # "about 4000": what the RoPE table of this model (4096) leaves room for
        for name, n_p, plen_ in (('prompts_1', 1, args.prompt_len), ('prompts_8', 8, args.prompt_len), (f'prompts_1_of_{long_len}_tokens', 1, long_len)):
            gen = torch.Generator().manual_seed(7)
            prompts = [torch.randint(0, model.vocab_size, (plen_ - 50 + 10 * i,), generator=gen) for i in range(n_p)]
            for small in (True, False):
                def run(split, new=args.new):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    generate(model, prompts, max_new_tokens=new, stop_token_ids=[], pad_id=0, small_batch=small, split_kv=split)
                    torch.cuda.synchronize()
                    return (time.perf_counter() - t0) * 1e3
                run(True, 2), run(False, 2)
                rounds = {'split_kv_ms': [], 'unsplit_ms': []}
                for _ in range(3):
                    rounds['split_kv_ms'].append(run(True))
                    rounds['unsplit_ms'].append(run(False))
                e = {k: spread(v, 1) for k, v in rounds.items()}
                e['unsplit_over_split_kv'] = round(e['unsplit_ms']['median'] / e['split_kv_ms']['median'], 3)
                e2e[name + ('_small_batch' if small else '_padded')] = e
        gen = torch.Generator().manual_seed(8)
        prompt = [torch.randint(0, model.vocab_size, (args.prompt_len,), generator=gen)]

        def run_sample(split, new=args.new):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sample(model, prompt, n=8, temperature=0.8, seed=1, max_new_tokens=new, stop_token_ids=[], pad_id=0, small_batch=True, split_kv=split)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        run_sample(True, 2), run_sample(False, 2)
        rounds = {'split_kv_ms': [], 'unsplit_ms': []}
        for _ in range(3):
            rounds['split_kv_ms'].append(run_sample(True))
            rounds['unsplit_ms'].append(run_sample(False))
        e = {k: spread(v, 1) for k, v in rounds.items()}
        e['unsplit_over_split_kv'] = round(e['unsplit_ms']['median'] / e['split_kv_ms']['median'], 3)
        e2e['sample_n8_one_prompt_small_batch'] = e
        res['end_to_end'] = dict(e2e, new_tokens=args.new, rounds=3, split_max_rows=model.split_max_rows,
                                 note='host clock around the whole call, prefill included; with split_kv (as with small_batch) a group that takes the path prefills prompt by prompt')
    print(json.dumps(res, indent=1))
    return res


def part_kv_fp8():
    """FP8 K/V cache against the cache in the model's dtype: per launch, per step, end to end, and what it does to the values."""
    import torch
    from ssi import ops
    from ssi.generate import generate
    model = build_model()
    L, H, KV, hd = model.num_layers, model.num_heads, model.num_kv_heads, model.head_dim
    dev, bf, u8 = dict(device='cuda'), torch.bfloat16, torch.uint8

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3        # us per call

    def rounds_of(forms, reps):
        for fn in forms.values():
            timed(fn, 4)
        got = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, fn in forms.items():
                got[k].append(timed(fn, reps))
        return {k: spread(v) for k, v in got.items()}

    def verdict(e, plain, fp8):
        """fp8 is faster than the plain form by more than the plain form's own min..max spread?"""
        e['plain_over_fp8'] = round(e[plain]['median'] / e[fp8]['median'], 3)
        e['plain_spread'] = round(e[plain]['max'] - e[plain]['min'], 3)
        e['fp8_wins_by_more_than_the_plain_spread'] = bool(e[plain]['median'] - e[fp8]['median'] > e['plain_spread'])
        return e

    res = {'geometry': f'1B shape (32 / 8 / 64), bf16; {args.rounds} rounds alternating the forms in one process, median (min - max); per launch call i reads '
                       f'layer i % {L}\'s caches',
           'hbm_TB_per_s_of_the_adamw_and_ema_passes': list(HBM_TB_S),
           'plain_form': 'measured on THIS build; that it stands for the parent\'s is an inference from tools/kernel_lint.py --against the parent build '
                         '(same registers or fewer, instruction counts within 2.5 %, mostly fewer), not a measurement of the parent'}
    with torch.inference_mode():
        g = torch.Generator(device='cuda').manual_seed(11)
        R, cap = 256, 4000
        kc = torch.empty((L, R, cap, KV * hd), dtype=bf, **dev).normal_(generator=g)
        vc = torch.empty((L, R, cap, KV * hd), dtype=bf, **dev).normal_(generator=g)
        qc, qe = torch.empty((2, L, R, cap, KV * hd), dtype=u8, **dev), torch.empty((2, L, R, cap, KV), dtype=u8, **dev)
        for w in range(2):
            for l in range(L):
                qc[w, l].random_(0, 0x7e, generator=g)                                                # any finite code
                qe[w, l].random_(118, 128, generator=g)
        qkv = torch.randn(R, (H + 2 * KV) * hd, generator=g, **dev).to(bf)
        out = torch.empty((R, H * hd), dtype=bf, **dev)
        slot = torch.arange(R, dtype=torch.int32, **dev)
        per = {}
        for rows in (1, 8, 64, 256):
            for keys in (1000, 4000):
                kv_len = torch.full((rows,), keys, dtype=torch.int32, **dev)
                q, o, sl = qkv[:rows], out[:rows], slot[:rows]
                forms = {'plain_us': lambda i: ops.attn_decode(q, kc[i % L], vc[i % L], sl, kv_len, o, None, H, KV, hd),
                         'fp8_us': lambda i: ops.attn_decode_fp8(q, qc[0, i % L], qc[1, i % L], qe[0, i % L], qe[1, i % L], sl, kv_len, o, None, H, KV, hd)}
                e = verdict(rounds_of(forms, 32), 'plain_us', 'fp8_us')
                e['cache_MB_read'] = {'plain': round(rows * keys * 2 * KV * hd * 2 / 1e6, 2), 'fp8': round(rows * keys * 2 * KV * (hd + 1) / 1e6, 2)}
                e['TB_per_s'] = {k: round(e['cache_MB_read'][k] / 1e6 / (e[k + '_us']['median'] * 1e-6), 3) for k in ('plain', 'fp8')}
                per[f'rows_{rows}_keys_{keys}'] = e
        res['per_launch_attention'] = per
        # the store at 256 rows: one position of every slot
        dest = (torch.arange(R, dtype=torch.int64, **dev) * cap + 17).contiguous()
        forms = {'plain_us': lambda i: ops.kv_store(qkv, dest, kc[i % L], vc[i % L], H, KV, hd),
                 'fp8_us': lambda i: ops.kv_store_fp8(qkv, dest, qc[0, i % L], qc[1, i % L], qe[0, i % L], qe[1, i % L], H, KV, hd)}
        res['per_launch_store_256_rows'] = verdict(rounds_of(forms, 32), 'plain_us', 'fp8_us')
        # the beam pair at 64 prompts x 4 beams: --prompt-len prompt keys, 128 generated positions read through a random ancestry
        P, W, t_mid = 64, 4, 128
        anc = torch.randint(0, P * W, (P * W, t_mid + 1), generator=g, **dev).to(torch.int32).contiguous()
        pslot = (torch.arange(P * W, dtype=torch.int32, **dev) // W).contiguous()
        plen, glen = torch.full((P * W,), args.prompt_len, dtype=torch.int32, **dev), torch.full((P * W,), t_mid, dtype=torch.int32, **dev)
        bk, bv = kc[:, :, :t_mid + 1].contiguous(), vc[:, :, :t_mid + 1].contiguous()
        bqc, bqe = qc[:, :, :, :t_mid + 1].contiguous(), qe[:, :, :, :t_mid + 1].contiguous()
        forms = {'plain_us': lambda i: ops.attn_decode_beam(qkv, kc[i % L, :P], vc[i % L, :P], bk[i % L], bv[i % L], pslot, plen, glen, anc, out, None, H, KV, hd),
                 'fp8_us': lambda i: ops.attn_decode_beam_fp8(qkv, (qc[0, i % L, :P], qc[1, i % L, :P], qe[0, i % L, :P], qe[1, i % L, :P]),
                                                               (bqc[0, i % L], bqc[1, i % L], bqe[0, i % L], bqe[1, i % L]), pslot, plen, glen, anc, out,
                                                               None, H, KV, hd)}
        res['per_launch_beam_64x4'] = dict(verdict(rounds_of(forms, 32), 'plain_us', 'fp8_us'), prompt_keys=args.prompt_len, generated_keys=t_mid)
        del kc, vc, qc, qe, bk, bv, bqc, bqe
        torch.cuda.empty_cache()

        # whole steps: the same prompts in a plain and an fp8 cache (the lengths are put back before every block of steps)
        steps, st, fidelity = 16, {}, {}
        for m_rows, small in ((256, False), (1, True), (8, True)):
            caches = {'plain_ms': _small_cache(model, m_rows, room=64)[0], 'fp8_ms': _small_cache(model, m_rows, room=64, dtype='fp8')[0]}
            start = caches['plain_ms'].lengths.clone()
            tok = torch.randint(0, model.vocab_size, (m_rows,), **dev)
            sl = torch.arange(m_rows, dtype=torch.int32, **dev)

            def block(which, keep=None):
                cache = caches[which]
                cache.lengths.copy_(start)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    logits = model.decode_step(cache, tok, sl, small_batch=small)
                    if keep is not None:
                        keep.append(logits[:, :model.vocab_size].float())
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / steps * 1e3      # ms per step, host clock: what a loop sees

            kept = {k: [] for k in caches}
            for k in caches:
                block(k, kept[k])
            if m_rows == 256:       # teacher-forced: both caches took the same prompts and the same tokens
                absmax = max(float(x.abs().max()) for x in kept['plain_ms'])
                worst = max(float((a - b).abs().max()) for a, b in zip(kept['plain_ms'], kept['fp8_ms']))
                fidelity['teacher_forced'] = {'steps': steps, 'rows': m_rows, 'max_abs_dlogit': round(worst, 4), 'logits_absmax': round(absmax, 4),
                                              'max_abs_dlogit_over_logits_absmax': round(worst / absmax, 5)}
            del kept
            rounds = {k: [] for k in caches}
            for _ in range(args.rounds):
                for k in caches:
                    rounds[k].append(block(k))
            e = verdict({k: spread(v, 3) for k, v in rounds.items()}, 'plain_ms', 'fp8_ms')
            e['cache_bytes'] = {k: sum(t.numel() * t.element_size() for t in (c.k, c.v, c.k_exp, c.v_exp) if t is not None) for k, c in caches.items()}
            st[f'rows_{m_rows}' + ('_small_batch' if small else '')] = e
            del caches
            torch.cuda.empty_cache()
        res['per_step'] = dict(st, note=f'{steps} decode steps a block on prompts of about {args.prompt_len} tokens, host clock')

    # end to end: generate of --prompts prompts with --new new tokens; the caches are opened (and their bytes allocated) inside the call
    prompts = make_prompts(model.vocab_size)
    found = {}

    def run(dtype):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        found[dtype] = generate(model, prompts, max_new_tokens=args.new, stop_token_ids=[], pad_id=0, kv_cache_dtype=dtype)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    run('auto'), run('fp8')
    rounds = {'plain_ms': [], 'fp8_ms': []}
    for _ in range(args.rounds):
        rounds['plain_ms'].append(run('auto'))
        rounds['fp8_ms'].append(run('fp8'))
    e = verdict({k: spread(v, 1) for k, v in rounds.items()}, 'plain_ms', 'fp8_ms')
    cap = max(p.numel() for p in prompts) + args.new
    e['cache_GB'] = {'plain': round(2 * L * args.prompts * cap * KV * hd * 2 / 1e9, 2), 'fp8': round(2 * L * args.prompts * cap * KV * (hd + 1) / 1e9, 2)}
    res['end_to_end_generate'] = dict(e, prompts=args.prompts, new_tokens=args.new, note='host clock around the whole call, prefill and cache allocation included')
    same = [sum(a == b for a, b in zip(x.token_ids, y.token_ids)) for x, y in zip(found['auto'], found['fp8'])]
    prefix = [next((i for i, (a, b) in enumerate(zip(x.token_ids, y.token_ids)) if a != b), len(x.token_ids)) for x, y in zip(found['auto'], found['fp8'])]
    fidelity['greedy'] = {'new_tokens': args.new, 'share_of_tokens_equal_position_by_position': round(sum(same) / (len(same) * args.new), 4),
                          'mean_tokens_before_the_first_difference': round(sum(prefix) / len(prefix), 1),
                          'prompts_equal_throughout': sum(p == args.new for p in prefix)}
    res['fidelity'] = dict(fidelity, note='recorded, not asserted.  The weights are random (normal, 0.02): next-token distributions are nearly flat, so a '
                                          'greedy path flips on small changes.  Nothing here says anything about WER on a trained checkpoint.')
    print(json.dumps(res, indent=1))
    return res


def part_weight_fp8():
    """FP8 weights against the bf16 weights on the small-batch path: per GEMM, the quantiser, per step, end to end, memory, fidelity."""
    import torch
    from ssi import ops
    from ssi.generate import generate
    model = build_model()
    D, I, L, dev, bf = model.embed_dim, model.intermediate_dim, model.num_layers, dict(device='cuda'), torch.bfloat16
    ROWS = (1, 16, 64)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3        # us per call

    def verdict(e, plain, fp8):
        """fp8 is faster than the plain form by more than the plain form's own min..max spread?"""
        e['plain_over_fp8'] = round(e[plain]['median'] / e[fp8]['median'], 3)
        e['plain_spread'] = round(e[plain]['max'] - e[plain]['min'], 3)
        e['fp8_wins_by_more_than_the_plain_spread'] = bool(e[plain]['median'] - e[fp8]['median'] > e['plain_spread'])
        return e

    res = {'geometry': f'1B shape, bf16; {args.rounds} rounds alternating the forms in one process, median (min - max); the layer GEMMs walk the {L} '
                       f'layers\' weights in turn (call i reads layer i % {L}), the head reads the one table',
           'hbm_TB_per_s_of_the_adamw_and_ema_passes': list(HBM_TB_S),
           'plain_form': 'the plain small-batch form measured on THIS build; it stands for the parent commit by tools/kernel_lint.py --against the parent '
                         'build (every kernel this part launches without fp8 is instruction-identical), not by a measurement of the parent'}
    with torch.inference_mode():
        # the quantiser over the whole model (the object the rest of the part reads)
        qw = model.quantize_weights()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            again = model.quantize_weights()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
            del again
        wbytes = sum(model._view(n).numel() * 2 for n in qw.mats)
        res['quantiser_whole_model'] = {'call_ms': spread(times, 2), 'matrices': len(qw.mats), 'bf16_GB_read_twice': round(wbytes / 1e9, 3),
                                        'note': 'host clock around quantize_weights(): the allocations and one launch per matrix included'}
        res['memory'] = {'added_bytes': qw.nbytes(), 'added_GB': round(qw.nbytes() / 1e9, 3), 'bf16_weights_GB': round(model._flat_numel * 2 / 1e9, 3),
                         'note': 'the bf16 weights stay (the embedding gather, prefill and every larger step read them): nothing is saved, a byte per weight is added'}

        g = torch.Generator(device='cuda').manual_seed(5)
        x = {k: torch.randn(64, k, generator=g, **dev).mul_(0.5).to(bf) for k in (D, I)}
        pos = torch.randint(0, 1000, (64,), generator=g, **dev).to(torch.int32)
        W = lambda name: [model._view(f'L{l}.{name}') for l in range(L)]   # noqa: E731
        Q = lambda name: [qw.mats[f'L{l}.{name}'] for l in range(L)]       # noqa: E731
        wqkv, wo, w13, w2, emb = W('wqkv'), W('wo'), W('w13'), W('w2'), model._view('emb')
        qqkv, qo, q13, q2, qemb = Q('wqkv'), Q('wo'), Q('w13'), Q('w2'), qw.mats['emb']
        H = model.num_heads + model.num_kv_heads
        out = {n: torch.empty(64, n, **dev, dtype=bf) for n in (model.qkv_dim, D, I, model.vocab_pad)}
        res_in = torch.randn(64, D, generator=g, **dev).to(bf)
        shapes = {
            'qkv_rope_3072x2048': (model.qkv_dim * D,
                                   lambda m: (lambda i: ops.gemm_skinny_rope(x[D][:m], wqkv[i % L], out[model.qkv_dim][:m], H, 64, model._rope, pos[:m])),
                                   lambda m: (lambda i: ops.gemm_skinny_rope_w8(x[D][:m], *qqkv[i % L], out[model.qkv_dim][:m], H, 64, model._rope, pos[:m]))),
            'wo_residual_2048x2048': (D * D,
                                      lambda m: (lambda i: ops.gemm_skinny(x[D][:m], wo[i % L], out[D][:m], residual=res_in[:m])),
                                      lambda m: (lambda i: ops.gemm_skinny_w8(x[D][:m], *qo[i % L], out[D][:m], residual=res_in[:m]))),
            'w13_swiglu_16384x2048': (2 * I * D,
                                      lambda m: (lambda i: ops.gemm_skinny_swiglu(x[D][:m], w13[i % L], None, out[I][:m])),
                                      lambda m: (lambda i: ops.gemm_skinny_swiglu_w8(x[D][:m], *q13[i % L], None, out[I][:m]))),
            'w2_residual_2048x8192': (D * I,
                                      lambda m: (lambda i: ops.gemm_skinny(x[I][:m], w2[i % L], out[D][:m], residual=res_in[:m])),
                                      lambda m: (lambda i: ops.gemm_skinny_w8(x[I][:m], *q2[i % L], out[D][:m], residual=res_in[:m]))),
            'head_133376x2048': (model.vocab_pad * D,
                                 lambda m: (lambda i: ops.gemm_skinny(x[D][:m], emb, out[model.vocab_pad][:m])),
                                 lambda m: (lambda i: ops.gemm_skinny_w8(x[D][:m], *qemb, out[model.vocab_pad][:m]))),
        }
        gemms = {}
        for name, (welems, plain_of, fp8_of) in shapes.items():
            reps = 8 if name.startswith('head') else 64
            entry = {'weight_MB': {'plain': round(welems * 2 / 1e6, 2), 'fp8': round((welems + welems // (D if 'x2048' in name else I)) / 1e6, 2)}}
            for m in ROWS:
                forms = {'plain_us': plain_of(m), 'fp8_us': fp8_of(m)}
                for fn in forms.values():
                    timed(fn, 4)
                got = {k: [] for k in forms}
                for _ in range(args.rounds):
                    for k, fn in forms.items():
                        got[k].append(timed(fn, reps))
                e = verdict({k: spread(v) for k, v in got.items()}, 'plain_us', 'fp8_us')
                e['weight_TB_per_s'] = {k: round(entry['weight_MB'][k] / e[k + '_us']['median'], 2) for k in ('plain', 'fp8')}
                entry[f'M{m}'] = e
            gemms[name] = entry
        res['gemms'] = gemms
        per_step = lambda k, m: L * sum(gemms[n][f'M{m}'][k]['median'] for n in gemms if not n.startswith('head')) + gemms['head_133376x2048'][f'M{m}'][k]['median']  # noqa: E731
        res['gemm_us_per_step_from_the_parts'] = {f'M{m}': {'plain': round(per_step('plain_us', m), 1), 'fp8': round(per_step('fp8_us', m), 1)} for m in ROWS}
        del x, out, res_in

        # whole small-batch steps on the same cache state (the lengths are put back before every block of steps)
        steps, st, fidelity = 16, {}, {}
        qn = model.quantize_weights(head=False)
        for m in SMALL_ROWS:
            cache, lens = _small_cache(model, m)
            start = cache.lengths.clone()
            tok = torch.randint(0, model.vocab_size, (m,), **dev)
            slot = torch.arange(m, dtype=torch.int32, **dev)

            def block(weights, keep=None):
                cache.lengths.copy_(start)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    logits = model.decode_step(cache, tok, slot, small_batch=True, weight_quant=weights)
                    if keep is not None:
                        keep.append(logits[:, :model.vocab_size].float())
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / steps * 1e3      # ms per step, host clock: what a loop sees

            kept = {'plain': [], 'fp8': [], 'fp8_bf16_head': []}
            block(None, kept['plain']), block(qw, kept['fp8'])
            if m == 8:      # teacher-forced: the same cache, the same tokens
                block(qn, kept['fp8_bf16_head'])
                absmax = max(float(t.abs().max()) for t in kept['plain'])
                for k in ('fp8', 'fp8_bf16_head'):
                    worst = max(float((a - b).abs().max()) for a, b in zip(kept['plain'], kept[k]))
                    same = sum(int((a.argmax(-1) == b.argmax(-1)).sum()) for a, b in zip(kept['plain'], kept[k]))
                    fidelity['teacher_forced_' + k] = {'steps': steps, 'rows': m, 'max_abs_dlogit': round(worst, 4), 'logits_absmax': round(absmax, 4),
                                                       'max_abs_dlogit_over_logits_absmax': round(worst / absmax, 5),
                                                       'share_of_equal_greedy_tokens': round(same / (steps * m), 4)}
            del kept
            rounds = {'plain_ms': [], 'fp8_ms': []}
            for _ in range(args.rounds):
                rounds['plain_ms'].append(block(None))
                rounds['fp8_ms'].append(block(qw))
            e = verdict({k: spread(v, 3) for k, v in rounds.items()}, 'plain_ms', 'fp8_ms')
            e['prompt_tokens_mean'] = round(sum(lens) / m, 1)
            st[f'rows_{m}'] = e
            assert int(cache.errors) == 0
            del cache
        del qn
        res['decode_step'] = dict(st, steps_per_block=steps, clock='host, synchronised around a block of steps')

    # end to end: generate() of 1 and 8 prompts, small_batch both ways; the object built inside the call, and prebuilt
    e2e, found = {}, {}
    for n_p in (1, 8):
        gen = torch.Generator().manual_seed(7)
        lens = torch.randint(args.prompt_len - 100, args.prompt_len + 101, (n_p,), generator=gen).tolist()
        prompts = [torch.randint(0, model.vocab_size, (n,), generator=gen) for n in lens]

        def run(key, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            found[key] = generate(model, prompts, max_new_tokens=args.new, stop_token_ids=[], pad_id=0, small_batch=True, **kw)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        forms = {'plain_ms': dict(), 'fp8_built_in_the_call_ms': dict(weight_dtype='fp8'), 'fp8_prebuilt_ms': dict(weight_dtype='fp8', weight_quant=qw)}
        for k, kw in forms.items():
            run(k, **kw)
        rounds = {k: [] for k in forms}
        for _ in range(3):
            for k, kw in forms.items():
                rounds[k].append(run(k, **kw))
        e = verdict({k: spread(v, 1) for k, v in rounds.items()}, 'plain_ms', 'fp8_prebuilt_ms')
        same = [sum(a == b for a, b in zip(x.token_ids, y.token_ids)) for x, y in zip(found['plain_ms'], found['fp8_prebuilt_ms'])]
        e['share_of_greedy_tokens_equal_position_by_position'] = round(sum(same) / (len(same) * args.new), 4)
        e2e[f'prompts_{n_p}'] = e
    res['generate_end_to_end'] = dict(e2e, new_tokens=args.new, rounds=3,
                                      note='generate(small_batch=True) of n prompts of about --prompt-len tokens, --new new tokens, host clock, prefill included')
    res['fidelity'] = dict(fidelity, note='recorded, not asserted.  The weights are random (normal, 0.02): next-token distributions are nearly flat, so a '
                                          'greedy path flips on small changes.  Nothing here says anything about WER on a trained checkpoint.')
    print(json.dumps(res, indent=1))
    return res


def part_continuous():
    import torch
    from ssi.generate import ADMIT_MIN_DEFAULT, READBACK_EVERY, plan_groups, sample, static_steps
    model = build_model()
    prompts = make_prompts(model.vocab_size)
    lens = [p.numel() for p in prompts]
    n, pool = len(prompts), 256
    admit_mins = [int(v) for v in args.admit_mins.split(',')]
    kw = dict(temperature=1.0, seed=11, max_new_tokens=args.new, pad_id=0, batch_size=pool)

    def run(stops, admit_min):
        """One call: (wall seconds, the schedule's numbers, the generated lengths)."""
        stats = {}
        mode = {} if admit_min is None else dict(continuous=True, admit_min=admit_min, continuous_report=stats)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gens = sample(model, prompts, stop_token_ids=stops, **mode, **kw)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        got = [len(gs[0].token_ids) for gs in gens]
        if admit_min is None:
            steps = static_steps(got, plan_groups(lens, pool), args.new, READBACK_EVERY)
            stats = {'decode_steps': steps, 'row_steps_live': sum(got), 'row_steps_total': steps * pool, 'admissions': -(-n // pool)}
        return wall, stats, got

    def workload(stops, forms):
        walls, last = {f: [] for f in forms}, {}
        for r in range(args.rounds):
            for f in forms:                               # the forms alternate within a round
                wall, stats, got = run(stops, forms[f])
                walls[f].append(wall)
                last[f] = (stats, got)
                print(f'round {r} {f}: {wall:.2f} s, {stats["decode_steps"]} steps', flush=True)
        out = {}
        for f in forms:
            stats, got = last[f]
            out[f] = {'wall_s': spread(walls[f]), 'decode_steps': stats['decode_steps'], 'admissions': stats['admissions'],
                      'prompts_per_admission': round(n / max(stats['admissions'], 1), 1),
                      'live_share_of_row_steps': round(stats['row_steps_live'] / max(stats['row_steps_total'], 1), 3),
                      'generated_tokens': sum(got), 'generated_tokens_per_s': round(sum(got) / statistics.median(walls[f]))}
        hist = [0] * (args.new // 32 + 1)
        for g in last['static'][1]:
            hist[g // 32] += 1
        out['generated_lengths_static'] = {'mean': round(sum(last['static'][1]) / n, 1), 'ended_by_length': sum(g == args.new for g in last['static'][1]),
                                           'histogram_by_32': hist}
        return out

    with torch.inference_mode():
        warm = dict(kw, max_new_tokens=24)                # warm-up: library, arena, the packed prefill of a group and of an admission
        sample(model, prompts[:pool + 40], stop_token_ids=list(range(0, model.vocab_size, 10)), **warm)
        sample(model, prompts[:pool + 40], stop_token_ids=list(range(0, model.vocab_size, 10)), continuous=True, admit_min=8, **warm)
        res = {'geometry': f'Llama-3.2-1B + 5000 DSUs, bf16, random weights; {n} prompts of {min(lens)}..{max(lens)} tokens (mean {sum(lens) / n:.0f}); '
                           f'sample(n=1, temperature=1.0), at most {args.new} new tokens, batch_size (static group / pool) {pool}; {args.rounds} rounds, '
                           f'the forms alternating in one process; wall_s: median [min, max] of the call',
               'admit_min_default': ADMIT_MIN_DEFAULT, 'sum_prompt_tokens': sum(lens)}
        forms = {'static': None, **{f'continuous_admit_min_{a}': a for a in admit_mins}}
        if args.workload in ('both', 'stops'):
            res['every_100th_id_stops'] = workload(list(range(0, model.vocab_size, 100)), forms)
        if args.workload in ('both', 'full'):
            res['no_stop_set'] = workload([], {'static': None, f'continuous_admit_min_{ADMIT_MIN_DEFAULT}': ADMIT_MIN_DEFAULT})
    print(json.dumps(res, indent=1), flush=True)
    return res


def part_small_batch_steps():
    """--trace-steps small-batch decode steps of --rows rows, for a kernel trace in a run of its own."""
    import torch
    model = build_model()
    with torch.inference_mode():
        cache, _ = _small_cache(model, args.rows)
        tok = torch.randint(0, model.vocab_size, (args.rows,), device='cuda')
        slot = torch.arange(args.rows, dtype=torch.int32, device='cuda')
        for _ in range(args.trace_steps):
            model.decode_step(cache, tok, slot, small_batch=True)
        torch.cuda.synchronize()


def split_trace(stats_csv, steps):
    rows = [r for r in csv.DictReader(open(stats_csv)) if int(r['Calls']) >= steps]
    ms = lambda sel: sum(float(r['TotalDurationNs']) for r in rows if sel(r['Name'])) / 1e6 / steps  # noqa: E731
    att, store = ms(lambda n: 'kv_decode_kernel' in n), ms(lambda n: 'kv_store_kernel' in n)
    total = ms(lambda n: True)
    top = sorted(rows, key=lambda r: -float(r['TotalDurationNs']))[:8]
    return {'steps_traced': steps, 'kernel_ms_per_step': round(total, 3), 'attention_ms_per_step': round(att, 3), 'kv_store_ms_per_step': round(store, 4),
            'rest_ms_per_step': round(total - att - store, 3),
            'largest_kernels': [{'name': r['Name'][:90], 'calls': int(r['Calls']), 'ms_per_step': round(float(r['TotalDurationNs']) / 1e6 / steps, 3)} for r in top]}


if args.part == 'run':
    res = part_run()
elif args.part == 'steps':
    part_steps()
    res = None
elif args.part == 'recompute':
    res = part_recompute()
elif args.part == 'constrained':
    res = part_constrained()
elif args.part == 'beam':
    res = part_beam()
elif args.part == 'sample':
    res = part_sample()
elif args.part == 'penalty':
    res = part_penalty()
elif args.part == 'small_batch':
    res = part_small_batch()
elif args.part == 'split_kv':
    res = part_split_kv()
elif args.part == 'kv_fp8':
    res = part_kv_fp8()
elif args.part == 'weight_fp8':
    res = part_weight_fp8()
elif args.part == 'continuous':
    res = part_continuous()
elif args.part == 'small_batch_steps':
    part_small_batch_steps()
    res = None
else:
    wd = args.workdir
    os.makedirs(wd, exist_ok=True)
    me = os.path.abspath(__file__)
    common = f'--prompts {args.prompts} --prompt-len {args.prompt_len} --new {args.new} --trace-steps {args.trace_steps}'
    cmd = (f'set -o pipefail; timeout -k 10 540 python {me} --part run {common} --json {wd}/run.json > {wd}/run.log 2>&1'
           f' && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d {wd}/trace -- python {me} --part steps {common} > {wd}/trace.log 2>&1'
           f' && timeout -k 10 300 python {me} --part recompute {common} --json {wd}/recompute.json > {wd}/recompute.log 2>&1')
    rc = subprocess.run(['bash', '-c', cmd]).returncode
    if rc != 0:
        sys.exit(f'a step failed (exit status {rc}); see the logs under {wd}')
    res = json.load(open(f'{wd}/run.json'))
    stats = sorted(glob.glob(f'{wd}/trace/**/*kernel_stats.csv', recursive=True))
    res['kernel_trace'] = split_trace(stats[-1], args.trace_steps)
    tr, kt = res['traffic_per_step'], res['kernel_trace']
    # the traced steps start at the prompts' lengths; the event time above is the mean over all steps, whose cache is a little longer
    traced_GB = tr['cache_bytes_per_token'] * (res['sum_prompt_tokens'] + args.prompts * (args.trace_steps - 1) / 2) / 1e9
    kt['cache_GB_per_traced_step'] = round(traced_GB, 3)
    kt['attention_TB_per_s'] = round(traced_GB / kt['attention_ms_per_step'], 2)
    kt['kernel_floor_ms_at_5.4_and_6.4_TB_s'] = [round((tr['weights_GB'] + traced_GB) / bw, 3) for bw in HBM_TB_S]
    kt['kernel_ms_over_floor'] = [round(kt['kernel_ms_per_step'] / f, 2) for f in kt['kernel_floor_ms_at_5.4_and_6.4_TB_s']]
    res['recompute_for_context'] = json.load(open(f'{wd}/recompute.json'))
    print(json.dumps(res, indent=1))

if args.json and res is not None:
    with open(args.json, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
