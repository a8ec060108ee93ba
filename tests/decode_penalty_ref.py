"""Parity of ``ssi_decode_select_pen`` and ``ssi_decode_sample_pen`` (csrc/decode_penalty.h): the penalised row ``y`` of include/ssi_hip.h
restated EXACTLY in numpy fp32, the float64 selector and sampler of tests/decode_select_ref.py and tests/decode_sample_ref.py run on ``y``
for the choice and on the stored ``x`` for ``logprob`` and ``rank``, an fp32 restatement with its mutants for the checker's CPU self-test,
and the histories and cases that tests/test_decode_penalty_ref.py (CPU) and tests/test_decode_penalty_gpu.py (GPU) share.

The definition, per row: H = the ids of the row's prompt and of its generated tokens, n_c = the occurrences of c among the generated ones,
    a_c = 1 (c outside H) | fl(1 / r) (c in H, x_c > 0) | fl(r) (c in H otherwise)
    t_c = fma(f, (float)n_c, n_c > 0 ? p : 0)
    y_c = fma(x_c, a_c, -t_c)                        (x_c itself for c outside H)
An id outside [0, vocab) is skipped and its row counted once in n_bad.

Why the bounds carry over.  y is formed by two fmas from fp32 inputs, and this file forms it with the same two roundings (the product of two
fp32 numbers is exact in float64, so one float64 addition and one rounding to fp32 is the fma), so the kernel's y and the reference's y are
the same fp32 numbers: nothing is bounded there.  The greedy token is a first maximum over exact numbers: exact.  The sampler's score bound
delta and mass bound eps (tests/decode_sample_ref.py) are stated for "an fp32 value x_c" and hold with y_c in its place, since nothing in
their derivation uses that x was STORED.  ``logprob`` and ``rank`` are functions of the stored row alone: ``decode_select_ref.Base``'s."""
import functools

import numpy as np
import torch

import decode_sample_ref as S
import decode_select_ref as D
from ce_parity import BF16, F32, VEC

PENALTIES = ((1.3, 0.0, 0.0), (0.8, 0.0, 0.0), (1.0, 0.7, 0.0), (1.0, -0.5, 0.0), (1.0, 0.0, 0.7), (1.0, 0.0, -0.5), (1.3, 0.7, -0.5),
             (0.8, -0.5, 0.7), (1.3, 0.7, 0.7))
DRAWS = (dict(T=1.0, top_k=-1, top_p=1.0), dict(T=0.7, top_k=50, top_p=1.0), dict(T=1.3, top_k=-1, top_p=0.9), dict(T=0.7, top_k=50, top_p=0.9))
LD_GENS = (1, 2, 255, 256, 257)
MUTANTS = ("prompt_ignored", "prompt_counted", "presence_without_count", "multiply_positive", "after_temperature", "penalty_in_logprob",
           "count_saturates", "collision_lost")
SAMPLE_ONLY = ("after_temperature",)
HISTORIES = ("empty", "one", "edges", "repeat300", "congruent", "full", "shared") + tuple(f"ld{n}" for n in LD_GENS)
MAX_ATTEMPTS = 12
GARBAGE = -3                                            # what lies beyond a row's n_generated and beyond a prompt's length: never read


def table_slots(ld_gen):
    hs = 64
    while hs < 2 * ld_gen:
        hs *= 2
    return hs


def lds_bytes(vocab, ld_gen):
    return 4 * ((vocab + 31) // 32) + 8 * table_slots(ld_gen)


class History:
    """``prompts``: the id lists of the prompt lines; ``prompt_row``: the line of every row (None: line r); ``gens``: the generated ids of every
    row (``n_generated`` is their number); ``ld_gen`` / ``ld_prompt``: the widths of the tensors."""

    def __init__(self, prompts, gens, ld_gen, prompt_row=None, ld_prompt=None):
        self.prompts, self.gens, self.prompt_row = [list(p) for p in prompts], [list(g) for g in gens], prompt_row
        self.ld_gen = int(ld_gen)
        self.ld_prompt = max([len(p) for p in self.prompts] + [0]) + 2 if ld_prompt is None else int(ld_prompt)
        self.rows = len(self.gens)
        assert all(len(g) <= self.ld_gen for g in self.gens)

    def line(self, r):
        return r if self.prompt_row is None else int(self.prompt_row[r])

    def tensors(self):
        """What the wrappers take: prompt_ids, prompt_len, prompt_row, gen_ids, n_generated."""
        pid = torch.full((len(self.prompts), self.ld_prompt), GARBAGE, dtype=torch.int32)
        for i, p in enumerate(self.prompts):
            pid[i, :len(p)] = torch.tensor(p, dtype=torch.int32)
        gid = torch.full((self.rows, self.ld_gen), GARBAGE, dtype=torch.int64)
        for i, g in enumerate(self.gens):
            gid[i, :len(g)] = torch.tensor(g, dtype=torch.int64)
        return dict(prompt_ids=pid, prompt_len=torch.tensor([len(p) for p in self.prompts], dtype=torch.int32),
                    prompt_row=None if self.prompt_row is None else torch.tensor(self.prompt_row, dtype=torch.int32), gen_ids=gid,
                    n_generated=torch.tensor([len(g) for g in self.gens], dtype=torch.int32))

    def counts(self, vocab, mutant=None):
        """(seen bool [rows, vocab], n int64 [rows, vocab], the number of rows that held an id out of range)."""
        seen, cnt, n_bad = np.zeros((self.rows, vocab), bool), np.zeros((self.rows, vocab), np.int64), 0
        hs = table_slots(self.ld_gen)
        for r in range(self.rows):
            p, g = self.prompts[self.line(r)], self.gens[r]
            n_bad += any(not 0 <= t < vocab for t in p + g)
            p, g = [t for t in p if 0 <= t < vocab], [t for t in g if 0 <= t < vocab]
            if mutant != "prompt_ignored":
                seen[r, p] = True
            seen[r, g] = True
            slots = {}
            for t in g + (p if mutant == "prompt_counted" else []):
                if mutant == "collision_lost" and slots.setdefault(t % hs, t) != t:
                    continue                            # the defect: a key whose home slot is taken is dropped
                cnt[r, t] += 1
            if mutant == "count_saturates":
                cnt[r] = np.minimum(cnt[r], 255)
        return seen, cnt, n_bad


def _fma32(a, b, c):
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
                + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


def penalised(x, vocab, hist, r, f, p, mutant=None):
    """fp32 ``y`` [rows, vocab] of the stored ``x`` [rows, ld], the kernel's two roundings."""
    xf = x[:, :vocab].float().numpy()
    seen, cnt, _ = hist.counts(vocab, mutant)
    inv_r, rr, ff, pp = np.float32(1.0 / r), np.float32(r), np.float32(f), np.float32(p)
    a = np.where(xf > 0, rr if mutant == "multiply_positive" else inv_r, rr)
    t = _fma32(ff, cnt.astype(np.float32), pp if mutant == "presence_without_count" else np.where(cnt > 0, pp, np.float32(0)))
    return np.where(seen, _fma32(xf, a, -t), xf)


# ---- the float64 references: the choice on y, the reports on x ---------------------------------------------------------------------------
def expect_select(base, y, M):
    """(token, logprob float64, its bound, rank) of ``ssi_decode_select_pen``: ``base`` is ``D.Base`` of the stored row."""
    tok = D._first_max(torch.from_numpy(y).double(), torch.as_tensor(M))
    live = tok >= 0
    lp = base.X.gather(1, tok.clamp(min=0)[:, None])[:, 0] - base.lse
    zero = torch.zeros_like(lp)
    return tok, torch.where(live, lp, zero), torch.where(live, base.dlse + D.U32 * lp.abs(), zero), D._rank(base.X, tok)


class Drawn:
    """The float64 sampler on y: ``S.Case`` of the penalised row (its keys, masses, scores and bounds are then those of y)."""

    def __init__(self, base, y, seqs, seed, step):
        self.base, self.case = base, S.Case(torch.from_numpy(y), y.shape[1], seqs, seed, step, vec=False)

    def expected(self, M, T, top_k, top_p):
        return self.case.expected(M, T, top_k, top_p)

    def judge(self, got, exp):
        """(token mismatches, n_kept mismatches, worst logprob err / bound, logprob misses): tokens and sets EXACT (the cases are committed
        clear of every boundary), the log-probability that of the RAW row within ``ssi_decode_select``'s bound."""
        tok, lp, kept = (t.detach().cpu() for t in got)
        bad_tok = int((tok != torch.from_numpy(exp.token)).sum())
        bad_kept = int((kept.long() != torch.from_numpy(exp.n_kept)).sum())
        ok = (tok >= 0) & (tok < self.case.vocab)
        elp = self.base.X.gather(1, tok.clamp(min=0)[:, None])[:, 0] - self.base.lse
        bound = self.base.dlse + D.U32 * elp.abs()
        elp, bound = torch.where(ok, elp, torch.zeros_like(elp)), torch.where(ok, bound, torch.zeros_like(bound))
        err = (lp.double() - elp).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
        return bad_tok, bad_kept, float(ratio.max()), int((~(err <= bound)).sum())


def clear(exp):
    """The committed-seed conditions on y: every draw more than 2 delta clear, every top-p boundary more than eps clear."""
    return bool(exp.margin_ok.all()) and not bool(exp.ambiguous.any())


# ---- the kernels in fp32, and their mutants --------------------------------------------------------------------------------------------
def _raw_logprob(x, vocab, tok, y=None):
    xf = x[:, :vocab].float() if y is None else torch.from_numpy(y)
    lp = xf.gather(1, tok.clamp(min=0)[:, None])[:, 0] - torch.logsumexp(xf, 1)
    return torch.where(tok >= 0, lp, torch.zeros_like(lp))


def restate_select(x, vocab, M, hist, r, f, p, mutant=None):
    """select_pen_kernel in fp32: (token, logprob fp32, rank)."""
    y = penalised(x, vocab, hist, r, f, p, mutant)
    tok = D._first_max(torch.from_numpy(y), torch.as_tensor(M))
    return tok, _raw_logprob(x, vocab, tok, y if mutant == "penalty_in_logprob" else None), D._rank(x[:, :vocab].float(), tok)


def restate_sample(x, vocab, M, hist, r, f, p, *, T, top_k, top_p, seed, step, seqs, mutant=None):
    """sample_pen_kernel in fp32: ``S.restate`` (the plain kernel) on the penalised row, the log-probability on the stored one."""
    if mutant == "after_temperature":                   # the defect: x / T is penalised, and drawn at temperature 1
        scaled = (x[:, :vocab].float().numpy() * np.float32(1.0 / T)).astype(np.float32)
        y, T = penalised(torch.from_numpy(scaled), vocab, hist, r, f, p), 1.0
    else:
        y = penalised(x, vocab, hist, r, f, p, mutant)
    tok, _, kept = S.restate(torch.from_numpy(y), vocab, M, T=T, top_k=top_k, top_p=top_p, seed=seed, step=step, seqs=seqs)
    return tok, _raw_logprob(x, vocab, tok, y if mutant == "penalty_in_logprob" else None), kept


def judge_select(got, exp):
    return D.judge(got, exp)


# ---- histories ---------------------------------------------------------------------------------------------------------------------------
def make_history(kind, x, vocab, allow, seed):
    """A history of every row of ``x`` built around the columns that matter — the row's largest values, so that a penalty moves the choice
    — with what the kind plants: column 0, column vocab - 1 (the scalar tail when vocab is no multiple of the vector), a disallowed column,
    ids in the prompt only / the output only / both, and per row a different mix."""
    rows = x.shape[0]
    g = np.random.default_rng(seed)
    order = np.argsort(-np.nan_to_num(x[:, :vocab].float().numpy(), nan=-np.inf), axis=1, kind="stable")
    top = lambda r, j: int(order[r, min(j, vocab - 1)])
    rnd = lambda n: [int(t) for t in g.integers(0, vocab, size=n)]
    off = [int(c) for c in np.flatnonzero(~allow.numpy())[:1]] if allow is not None else []
    if kind == "empty":
        return History([[] for _ in range(rows)], [[] for _ in range(rows)], ld_gen=4, ld_prompt=0)
    if kind == "one":
        return History([[] for _ in range(rows)], [[top(r, 0)] for r in range(rows)], ld_gen=1, ld_prompt=3)
    if kind == "edges":
        prompts = [[0, vocab - 1, top(r, 2), top(r, 1)] + off + rnd(5) for r in range(rows)]                 # top 2: the prompt only
        gens = [[top(r, 0), vocab - 1, top(r, 0), top(r, 3), top(r, 1)] + off + rnd(r % 4) for r in range(rows)]   # top 3: the output only
        return History(prompts, gens, ld_gen=12)
    if kind == "repeat300":
        # (the runner-up 300 times against the first 256 times: a count that stopped at 255 would order the two differently under f != 0)
        return History([rnd(3) for _ in range(rows)], [[top(r, 0)] * 256 + [top(r, 1)] * 300 + rnd(r % 3) for r in range(rows)], ld_gen=560)
    if kind == "congruent":                             # ld_gen 32 -> 64 slots: one home slot per row, so a full probe chain is walked
        gens = []
        for r in range(rows):                           # even rows: home 63, the chain wraps to 0, 1, ...; odd rows: the home of the row's
            home = 63 if r % 2 == 0 else top(r, 0) % 64  # first column, which arrives LAST, behind every id it collides with
            ids = [c for c in range(home, vocab, 64) if r % 2 == 0 or c != top(r, 0)][:31] or [vocab - 1]
            gens.append(ids + ([ids[0]] if r % 2 == 0 else [top(r, 0)]))
        return History([[top(r, 0), top(r, 1)] for r in range(rows)], gens, ld_gen=32)
    if kind == "full":                                  # the table at its fullest: ld_gen distinct ids (as many as the vocabulary has)
        n = min(256, vocab)
        gens = [[int(t) for t in np.concatenate([order[r, :n // 2], g.permutation(order[r, n // 2:])[:n - n // 2]])] for r in range(rows)]
        return History([rnd(4) for _ in range(rows)], gens, ld_gen=n)
    if kind == "shared":                                # two prompt lines for all rows: the n samples of a prompt
        prompts = [[top(0, 0), top(0, 1), 0] + rnd(6), [top(rows - 1, 0), vocab - 1] + rnd(2)]
        row = [0 if r < (rows + 1) // 2 else 1 for r in range(rows)]
        return History(prompts, [[top(r, 0)] * (r % 3) + rnd(r % 5) for r in range(rows)], ld_gen=8, prompt_row=row)
    if kind.startswith("ld"):                           # n_generated at 0, 1 and ld_gen in turn
        n = int(kind[2:])
        lens = [(0, 1, n)[r % 3] for r in range(rows)]
        gens = [([top(r, 0), top(r, 0), top(r, 1)] + [int(order[r, j % vocab]) for j in range(n)])[:k] for r, k in enumerate(lens)]
        return History([[top(r, 1)] + rnd(3) for r in range(rows)], gens, ld_gen=n)
    raise ValueError(kind)


def with_bad_ids(hist, vocab, rows_bad):
    """``hist`` with ids -1 and ``vocab`` planted into the prompt (even rows of ``rows_bad``) or the output (odd ones) of the given rows."""
    prompts, gens = [list(p) for p in hist.prompts], [list(g) for g in hist.gens]
    assert hist.prompt_row is None
    for r in rows_bad:
        if r % 2 == 0 or len(gens[r]) + 2 > hist.ld_gen:
            prompts[r] = [vocab] + prompts[r] + [-1]
        else:
            gens[r] = [-1] + gens[r] + [vocab]
    return History(prompts, gens, hist.ld_gen, ld_prompt=hist.ld_prompt + 2)


# ---- the committed cases -------------------------------------------------------------------------------------------------------------------
class Case:
    """One [rows, ld] input with the histories, masks and settings judged on it."""

    def __init__(self, x, vocab, seqs, seed, step, items):
        self.x, self.vocab, self.seqs, self.seed, self.step, self.items = x, vocab, seqs, seed, step, items
        self.base = D.Base(x, vocab)


def _items(x, vocab, rows, attempt):
    """[(history kind, History, allow, mask [rows, vocab], (r, f, p), draw setting)]: every history with the penalties, the draws and
    three mask kinds in turn."""
    kinds = [k for k in ("null", "complement", "alternating") if D.mask_exists(k, vocab) and (k == "null" or vocab > 1)]
    out = []
    for i, kind in enumerate(HISTORIES):
        allow, M = S.masks_of(kinds[i % len(kinds)], vocab, rows)
        hist = make_history(kind, x, vocab, allow, seed=100 * attempt + i)
        if lds_bytes(vocab, hist.ld_gen) > 57344:
            continue
        d = DRAWS[i % len(DRAWS)]
        if vocab > 2049 and d["top_p"] < 1.0 and d["top_k"] <= 0:
            # Top-p over the whole flagship vocabulary cannot be committed clear of eps: eps holds |K| 2^-39 = 2.4e-7 for the truncated
            # fixed-point terms, and around M / Z = 0.9 the fp32 value classes of a spread-out row lie about that far apart.  Under a top-k
            # of 1000 eps is a hundred times smaller and the top-p pass still runs over the 32-bit keys.
            d = dict(d, top_k=1000)
        out.append((kind, hist, allow, M, PENALTIES[i % len(PENALTIES)], d))
    return out


@functools.lru_cache(maxsize=None)
def case(vocab, rows, dtype):
    """The first attempt (logits seed ``1000 a + vocab + rows``, Philox seed ``2^34 + a``) at which every item's draw is clear of its
    boundaries on y: (Case, [Drawn per item], [Expected per item])."""
    ld = D.ld_of(vocab)
    for a in range(MAX_ATTEMPTS):
        x = D.make_logits(rows, vocab, ld, dtype, seed=1000 * a + vocab + rows)
        seqs = (torch.arange(rows, dtype=torch.int64) * 0x9E3779B1 + 5) & 0xffffffff
        c = Case(x, vocab, seqs, seed=(1 << 34) + a, step=7, items=_items(x, vocab, rows, a))
        drawn, exps = [], []
        for kind, hist, allow, M, (r, f, p), d in c.items:
            dr = Drawn(c.base, penalised(x, vocab, hist, r, f, p), seqs, c.seed, c.step)
            e = dr.expected(M, d["T"], d["top_k"], d["top_p"])
            if not clear(e):
                break
            drawn.append(dr)
            exps.append(e)
        else:
            return c, drawn, exps
    raise AssertionError(f"no seed in {MAX_ATTEMPTS} attempts is clear of every boundary at {vocab} x {rows} {dtype}")


SHAPES = S.SHAPES
CPU_SHAPES = [(v, 3) for v in (1, 7, 8, 9, 255, 257, 2049)]
