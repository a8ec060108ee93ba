"""The rules of ``ssi.generate.beam_search`` said again in plain Python, for one prompt at a time (tests/test_beam_search_host.py on hand-made
log-probability tables, tests/test_beam_search_gpu.py on ``OracleLlama`` by full recompute).  Nothing here calls the library.

``step_logprobs(tokens)`` gives the log-probabilities (a sequence of ``vocab`` floats, natural log, over ALL columns) of the token that
follows ``tokens`` (prompt + what the hypothesis has generated).  With ``W = beam_width``:

1. at step ``t`` the prompt has live beams ``b = 0..`` with scores ``s_b``; one beam with score 0 at ``t = 0``;
2. continuations: the ``W`` best ``(s_b + lp, b, token)`` over the live beams' allowed non-stop tokens — score descending, then beam
   ascending, then token ascending;
3. finishers: ``s_b + lp[stop]`` for every live beam and stop token; none while ``t < min_new``;
4. both merged in the same order; every finisher among the first ``W`` entries joins the pool with the final score
   ``score / (t + 1) ** length_penalty``, reason "stop", the stop token included;
5. the ``W`` continuations are the next beams;
6. done when the pool holds at least ``W``; after ``max_new`` steps the live beams join with "length" and ``s / max_new ** length_penalty``;
7. the result is the pool by final score descending (stable), cut to ``n_best``.

``trace`` (a dict, optional) collects what the margin condition of the GPU test looks at: ``"cont_gaps"`` and ``"merged_gaps"`` (the adjacent
score gaps among the first ``W + 1`` continuations / merged entries of every step), ``"final_gaps"`` (between adjacent final scores of the
whole pool), ``"done_at"`` (the step after which the pool was full, or None)."""
import math
from typing import NamedTuple, Optional


class Hyp(NamedTuple):
    token_ids: list
    finish_reason: str
    stop_reason: Optional[int]
    cumulative_logprob: float
    score: float


def _order(e):
    return (-e[0], e[1], e[2])


def _gaps(entries, n):
    s = [e[0] for e in entries[:n]]
    return [a - b for a, b in zip(s, s[1:])]


def beam_search_ref(step_logprobs, prompt, *, beam_width, max_new_tokens, stop_token_ids, length_penalty=1.0, n_best=1, allowed=None,
                    min_new_tokens=0, trace=None):
    W, stops = beam_width, sorted({int(t) for t in stop_token_ids})
    stopset = set(stops)
    beams, pool = [(0.0, [])], []
    tr = trace if trace is not None else {}
    tr.update(cont_gaps=[], merged_gaps=[], final_gaps=[], done_at=None)
    for t in range(max_new_tokens):
        conts, fins = [], []
        for b, (s, toks) in enumerate(beams):
            lp = step_logprobs(list(prompt) + toks)
            for tok in range(len(lp)):
                if tok not in stopset and (allowed is None or tok in allowed) and lp[tok] > -math.inf:
                    conts.append((s + float(lp[tok]), b, tok))
            if t >= min_new_tokens:
                fins += [(s + float(lp[tok]), b, tok) for tok in stops if lp[tok] > -math.inf]
        conts.sort(key=_order)
        tr["cont_gaps"] += _gaps(conts, W + 1)
        merged = sorted([(c, False) for c in conts[:W + 1]] + [(f, True) for f in fins], key=lambda e: _order(e[0]))
        tr["merged_gaps"] += _gaps([e for e, _ in merged], W + 1)
        for (sc, b, tok), is_fin in merged[:W]:
            if is_fin:
                pool.append(Hyp(beams[b][1] + [tok], "stop", tok, sc, sc / float((t + 1) ** length_penalty)))
        beams = [(sc, beams[b][1] + [tok]) for sc, b, tok in conts[:W]]
        if len(pool) >= W:
            beams, tr["done_at"] = [], t
            break
    pool += [Hyp(toks, "length", None, s, s / float(max_new_tokens ** length_penalty)) for s, toks in beams]
    pool.sort(key=lambda h: -h.score)                     # (stable: ties stay in the order of joining)
    tr["final_gaps"] = [a.score - b.score for a, b in zip(pool, pool[1:])]
    return pool[:n_best]
